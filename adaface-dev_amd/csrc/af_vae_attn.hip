// af_vae_attn.hip -- fused single-head attention for the VAE's one attention layer (mid.attn_1: head dim = C = 512 at SD-1.5 width, 128 at
// the reduced test width):  O = softmax(Q K^T) V  with online softmax, no [N, N] matrix in memory, any N % 8 == 0.
//
// af_attention keeps a wave's 32 queries x d outputs AND its Q fragments in registers, which stops at d = 160.  At d = 512 one 32-query block
// of O alone is 256 fp32 registers per lane, so here the work of a 64-query block is split ACROSS the four waves of a workgroup instead:
//   * S^T = K Q^T (v_mfma_f32_32x32x16_f16, the query on the MFMA lane as in af_attn.hip) for a stage of 32 keys is two 32 x 32 tiles, one per
//     32-query group qg.  Wave w = (qg, kh) forms the tile of group qg over HALF of the channels (kh) with its Q fragments resident in registers
//     (C / 32 half8 per lane), the two partners exchange their fp32 partial tiles through LDS and both hold the full tile after one add (a + b ==
//     b + a: bit-identical in both, so is everything they derive from it);
//   * the online-softmax state (reference m, sum l: one scalar per lane) is kept by both partners; P^T = exp2(S^T log2(e) - m) is rounded to
//     fp16 in the B-operand layout of the next product and written to LDS (each partner writes one 16-key half), with the group's rescale factor;
//   * O^T = V^T P^T: every wave owns C / 4 output channels for ALL 64 queries (C / 128 x 2 accumulator tiles = 128 registers at C = 512), reads
//     both groups' P^T fragments and its own V^T rows.  Per 64-query x 32-key stage a wave reads 16 KB of K, 8 KB of V^T and 8 KB of S / P from
//     LDS against 32 MFMAs; a wave that kept whole queries to itself would read all 64 KB of the K and V^T tile for 16 or 32 queries.
//   * m is a LAZY reference as in af_attn.hip: it moves only when a new score exceeds it by more than 2^8, so the O rescale (128 multiplies
//     per lane) is rare; p <= 2^8 is exact enough in fp16 and the sums are fp32.  The result is shift invariant.
//   * K [32 keys][C] and V^T [C][32 keys] stages are double-buffered through registers (global loads of stage t + 1 before the MFMAs of stage t,
//     LDS stores after them); three barriers per stage (partial S, P, buffer swap).
//   * V arrives TRANSPOSED ([B, C, ldv], key index contiguous, af_transpose_tokens) as for af_attention.  Keys >= N are never read: their K rows
//     and V^T chunks are zero-filled in registers and their scores are -inf; queries >= N of the last block are computed on zeros and not stored.
#include <math.h>

#include "af_common.h"

namespace {

struct VaeAttnArgs {
  const half_t* q;
  const half_t* k;
  const half_t* vt;
  half_t* o;
  int B, N;
  int ldq, ldk, ldv, ldo;
};

constexpr int VA_QB = 64;       // queries per workgroup
constexpr int VA_KB = 32;       // keys per stage
constexpr int VA_VST = 36;      // V^T LDS row stride in halves (72 B: conflict-free ds_read_b64 over 32 rows)
constexpr float VA_LAZY = 8.0f;
constexpr float VA_LOG2E = 1.4426950408889634f;

template <int C>
constexpr size_t va_lds_bytes() {
  return (size_t)2 * (VA_KB * (C + 8) + C * VA_VST) * sizeof(half_t)   // K + V^T stages, double-buffered
         + 4 * 16 * 64 * sizeof(float)                                 // partial S tiles
         + 2 * 2 * 64 * 8 * sizeof(half_t)                             // P^T fragments
         + 2 * 32 * sizeof(float) + 4 * sizeof(int);                   // rescale factors (then 1 / l), rescale flags
}

template <int C>
__global__ __launch_bounds__(256) void af_vae_attn_kernel(VaeAttnArgs a) {
  constexpr int NT = C / 128;             // 32-channel O^T tiles per wave
  constexpr int KS = C / 32;              // k-steps of 16 over this wave's half of the channels
  constexpr int KST = C + 8;              // K LDS row stride (halves)
  constexpr int KBUF = VA_KB * KST, VBUF = C * VA_VST, STAGE = KBUF + VBUF;
  constexpr int NKC = VA_KB * (C / 8) / 256;   // 16-byte chunks of a K stage per thread
  constexpr int NVC = C * 4 / 256;             // 16-byte chunks of a V^T stage per thread
  extern __shared__ __attribute__((aligned(16))) char af_smem[];
  half_t* lds = reinterpret_cast<half_t*>(af_smem);
  floatx4* Sx = reinterpret_cast<floatx4*>(lds + 2 * STAGE);
  half8_t* Ps = reinterpret_cast<half8_t*>(Sx + 4 * 4 * 64);
  float* Al = reinterpret_cast<float*>(Ps + 2 * 2 * 64);
  int* Fl = reinterpret_cast<int*>(Al + 2 * 32);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int qg = wave >> 1, kh = wave & 1;
  const int qblocks = (a.N + VA_QB - 1) / VA_QB;
  const int b = blockIdx.x / qblocks;
  const int q0 = (blockIdx.x - b * qblocks) * VA_QB;
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // ---- Q fragments of this wave's S tile: lane (r, hh) holds Q[q0 + 32 qg + r][kh C/2 + 16 s + 8 hh .. +7]
  half8_t qf[KS];
  {
    const int query = q0 + 32 * qg + r;
    const half_t* qp = a.q + ((size_t)b * a.N + (query < a.N ? query : 0)) * a.ldq + kh * (C / 2) + 8 * hh;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = query < a.N ? *reinterpret_cast<const half8_t*>(qp + 16 * s) : zero8;
  }

  half8_t rk[NKC], rv[NVC];
  // per-thread staging sources: one 32-bit element offset each (the entry point bounds every operand below 2^31 elements); the chunks j of a
  // thread differ by whole rows, i.e. by a wave-uniform step that folds into the scalar base
  constexpr int KROWS = 256 / (C / 8);                               // K rows between a thread's consecutive chunks
  const int krow = tid / (C / 8), vrow = tid >> 2, vkk = (tid & 3) * 8;
  const unsigned koff = (unsigned)krow * (unsigned)a.ldk + (unsigned)(tid - krow * (C / 8)) * 8u;
  const unsigned voff = (unsigned)vrow * (unsigned)a.ldv + (unsigned)vkk;
  const half_t* kbase = a.k + (size_t)b * a.N * a.ldk;
  const half_t* vbase = a.vt + (size_t)b * C * a.ldv;
  auto load_stage = [&](int key0) {
#pragma unroll
    for (int j = 0; j < NKC; ++j) {
      const half_t* src = kbase + (size_t)(key0 + j * KROWS) * a.ldk;
      rk[j] = key0 + j * KROWS + krow < a.N ? *reinterpret_cast<const half8_t*>(src + koff) : zero8;
    }
    const bool vok = key0 + vkk < a.N;                               // N % 8 == 0: a chunk of 8 keys is valid as a whole or not at all
#pragma unroll
    for (int j = 0; j < NVC; ++j) {
      const half_t* src = vbase + (size_t)(64 * j) * a.ldv + key0;
      rv[j] = vok ? *reinterpret_cast<const half8_t*>(src + voff) : zero8;
    }
  };
  auto store_stage = [&](int buf) {
    half_t* Ks = lds + buf * STAGE;
    half_t* Vs = Ks + KBUF;
#pragma unroll
    for (int j = 0; j < NKC; ++j) {
      const int i = tid + 256 * j;
      const int row = i / (C / 8), ch = i - row * (C / 8);
      *reinterpret_cast<half8_t*>(Ks + row * KST + ch * 8) = rk[j];
    }
#pragma unroll
    for (int j = 0; j < NVC; ++j) {
      const int i = tid + 256 * j;
      half_t* dst = Vs + (i >> 2) * VA_VST + (i & 3) * 8;
      const half4_t lo = {rv[j][0], rv[j][1], rv[j][2], rv[j][3]};
      const half4_t hi = {rv[j][4], rv[j][5], rv[j][6], rv[j][7]};
      *reinterpret_cast<half4_t*>(dst) = lo;
      *reinterpret_cast<half4_t*>(dst + 4) = hi;
    }
  };

  floatx16 o[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[t][g][i] = 0.f;
  float m = 0.f, l = 0.f;

  const int nstage = (a.N + VA_KB - 1) / VA_KB;
  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int st = 0; st < nstage; ++st) {
    const int key0 = st * VA_KB;
    const bool more = st + 1 < nstage;
    if (more) load_stage(key0 + VA_KB);
    const half_t* Ks = lds + (st & 1) * STAGE;
    const half_t* Vs = Ks + KBUF;

    // ---- partial S^T[key, query] of group qg over channel half kh
    floatx16 sT;
#pragma unroll
    for (int i = 0; i < 16; ++i) sT[i] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + r * KST + kh * (C / 2) + 16 * s + 8 * hh);
      sT = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sT, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const floatx4 v = {sT[4 * g], sT[4 * g + 1], sT[4 * g + 2], sT[4 * g + 3]};
      Sx[(wave * 4 + g) * 64 + lane] = v;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const floatx4 v = Sx[((wave ^ 1) * 4 + g) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) sT[4 * g + e] = (sT[4 * g + e] + v[e]) * VA_LOG2E;      // base-2 softmax domain
    }
    if (key0 + VA_KB > a.N) {                                                              // key tail: register 4g + e is key 8g + 4hh + e
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (key0 + 8 * (i >> 2) + 4 * hh + (i & 3) >= a.N) sT[i] = -INFINITY;
    }
    float mx = sT[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, sT[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // ---- lazy softmax reference (stage 0 always holds valid keys in both half-waves' maximum: N >= 8)
    float alpha = 1.f;
    int moved = 0;
    if (st == 0) {
      m = mx;
    } else if (__builtin_amdgcn_ballot_w64(mx - m > VA_LAZY) != 0) {
      const float delta = fmaxf(mx - m, 0.f);
      alpha = __builtin_amdgcn_exp2f(-delta);
      m += delta;
      l *= alpha;
      moved = 1;
    }
    half8_t pf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(sT[8 * s2 + j] - m);
        l += p;
        pf[s2][j] = (half_t)p;
      }
    Ps[(qg * 2 + kh) * 64 + lane] = kh ? pf[1] : pf[0];
    if (kh == 0) {
      if (hh == 0) Al[qg * 32 + r] = alpha;
      if (lane == 0) Fl[qg] = moved;
    }
    __syncthreads();

    // ---- O^T[channels of this wave, all 64 queries] += V^T P^T
    half8_t pb[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (__builtin_amdgcn_readfirstlane(Fl[g]) != 0) {
        const float al = Al[g * 32 + r];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[t][g][i] *= al;
      }
      pb[g][0] = Ps[(g * 2 + 0) * 64 + lane];
      pb[g][1] = Ps[(g * 2 + 1) * 64 + lane];
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const half_t* vp = Vs + (wave * (32 * NT) + 32 * t + r) * VA_VST + 16 * s2 + 4 * hh;
        const half4_t lo = *reinterpret_cast<const half4_t*>(vp);
        const half4_t hi = *reinterpret_cast<const half4_t*>(vp + 8);
        const half8_t vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pb[0][s2], o[t][0], 0, 0, 0);
        o[t][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pb[1][s2], o[t][1], 0, 0, 0);
      }
    }

    if (more) store_stage((st + 1) & 1);
    __syncthreads();
  }

  // ---- normalise and store: lane holds channels {32 t + 8 g + 4 hh + e} of this wave's slice for query r of each group
  l += __shfl_xor(l, 32, 64);
  if (kh == 0 && hh == 0) Al[qg * 32 + r] = 1.0f / l;
  __syncthreads();
#pragma unroll
  for (int g2 = 0; g2 < 2; ++g2) {
    const int query = q0 + 32 * g2 + r;
    if (query >= a.N) continue;
    const float inv = Al[g2 * 32 + r];
    half_t* op = a.o + ((size_t)b * a.N + query) * a.ldo + wave * (32 * NT) + 4 * hh;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const half4_t v = {(half_t)(o[t][g2][4 * g + 0] * inv), (half_t)(o[t][g2][4 * g + 1] * inv), (half_t)(o[t][g2][4 * g + 2] * inv),
                           (half_t)(o[t][g2][4 * g + 3] * inv)};
        *reinterpret_cast<half4_t*>(op + 32 * t + 8 * g) = v;
      }
  }
}

template <int C>
int launch_vae_attn(const VaeAttnArgs& a, hipStream_t stream) {
  constexpr size_t lds = va_lds_bytes<C>();
  static_assert(lds <= 160 * 1024, "af_vae_attention: LDS budget");
  static bool attr_set = false;  // benign race: idempotent attribute
  if (!af_allow_dyn_lds(reinterpret_cast<const void*>(&af_vae_attn_kernel<C>), lds, attr_set, "af_vae_attention")) return af_check_launch("af_vae_attention");
  const int qblocks = (a.N + VA_QB - 1) / VA_QB;
  hipLaunchKernelGGL((af_vae_attn_kernel<C>), dim3((unsigned)(a.B * qblocks)), dim3(256), lds, stream, a);
  return af_check_launch("af_vae_attention");
}

}  // namespace

extern "C" int af_vae_attention(const void* q, const void* k, const void* vt, void* o, int B, int N, int C, int ldq, int ldk, int ldv, int ldo,
                                void* stream) {
  AF_REQUIRE(q && k && vt && o, "af_vae_attention: null pointer");
  AF_REQUIRE(B > 0 && N > 0 && C > 0, "af_vae_attention: bad sizes");
  AF_REQUIRE(N % 8 == 0, "af_vae_attention: the token count must be a multiple of 8");
  AF_SUPPORTED(C == 128 || C == 512, "af_vae_attention: head dim must be 128 or 512");
  AF_REQUIRE(ldq >= C && ldk >= C && ldo >= C && ldq % 8 == 0 && ldk % 8 == 0 && ldo % 8 == 0,
             "af_vae_attention: q / k / o row strides must be >= C and multiples of 8");
  AF_REQUIRE(ldv >= N && ldv % 8 == 0, "af_vae_attention: ldv must be >= N and a multiple of 8");
  AF_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)o) % 16 == 0, "af_vae_attention: operands must be 16-byte aligned");
  // element offsets and the grid are formed in 32 bits on the host side of the launch: refuse what does not fit rather than wrap
  const int64_t lim = (int64_t)1 << 31;
  const int64_t ldmax = ldq > ldk ? (ldq > ldo ? ldq : ldo) : (ldk > ldo ? ldk : ldo);
  AF_SUPPORTED((int64_t)B * N * ldmax < lim && (int64_t)B * C * ldv < lim, "af_vae_attention: an operand of 2^31 elements or more");
  AF_SUPPORTED((int64_t)B * ((N + VA_QB - 1) / VA_QB) < lim, "af_vae_attention: too many query blocks");
  VaeAttnArgs a;
  a.q = (const half_t*)q;
  a.k = (const half_t*)k;
  a.vt = (const half_t*)vt;
  a.o = (half_t*)o;
  a.B = B;
  a.N = N;
  a.ldq = ldq;
  a.ldk = ldk;
  a.ldv = ldv;
  a.ldo = ldo;
  AfLaunchScope scope(AF_FAM_ATTN, stream);
  return C == 512 ? launch_vae_attn<512>(a, (hipStream_t)stream) : launch_vae_attn<128>(a, (hipStream_t)stream);
}
