// af_region_attn.hip -- regional prompts: a cross-attention core over R context sets per batch item, blended per query under the region weights,
//     o[b N + i, h d + j] = fp16( sum_r w[b, r, i] * sum_t softmax_t(scale <q[b, i, h, :], k[b, r, t, h, :]>) v[b, r, t, h, j] ),  t over L <= 80 keys,
// and af_region_weights, which turns the uint8 region masks into the four U-Net levels' normalised weights.
// Context set (b, r) is batch item b R + r of k ([L][ldk] token rows) and vt (V transposed, [heads d][ldv], element stride vt_batch_stride between
// items), addressed as af_attention_strided addresses its batch items, so a layer reads its slice of ONE stacked projection of all layers in place.
// The frame is af_attention's short-key kernel (af_xattn_kernel): the query on the MFMA lane from the first product to the store.
//   * a workgroup = 4 waves = 128 consecutive queries of one (batch item, head), 32 per wave; q fragments stay in registers over all regions;
//   * per region r: K_r [96][d] and V_r^T [3][32 DT][32 keys] of the head are staged in LDS (keys >= L zero), S^T = K Q^T for all keys
//     (v_mfma_f32_32x32x16_f16, <= 3 sub-tiles of 32 keys, two rolled passes: maximum, then exp2 and O_r^T = V^T P^T), one plain softmax;
//     the scale is applied to the fp32 scores (q is not rescaled in fp16), P^T <= 1 is rounded to fp16 ONCE as the MFMA operand, the row sum l is
//     the fp32 sum of the unrounded p;
//   * acc += (w / l) O_r in fp32 under a SELECT on w != 0 per query (lane): a query whose weight is exactly 0 keeps its accumulator whatever
//     O_r holds (NaN, Inf), so a region's K / V never reach a query outside it; o = fp16(acc) once;
//   * the SKIP: before the region loop EVERY wave reads the weights of all 128 queries of the tile (two per lane) and of its own 32, and forms
//     two R-bit masks with wave-wide ballots: `wg_mask` (some query of the tile has w != 0) is computed by every wave from the same read-only
//     words, so it is uniform over the workgroup; `wv_mask` is this wave's.  The two barriers of a region's iteration sit under wg_mask only
//     (workgroup-uniform control flow, decided before any barrier); a region the tile does not touch is neither staged nor read.  Under
//     wv_mask a wave skips its MFMAs only -- no barrier is inside that branch.
// Tails: query rows >= N are computed on zeros with weight 0 and never stored; channels >= d are zero in q and K and never stored.
#include <float.h>
#include <math.h>

#include "af_common.h"

namespace {

struct RegionAttnArgs {
  const half_t* q;
  const half_t* k;
  const half_t* vt;
  const float* w;
  half_t* o;
  int ldq, ldk, ldv, ldw, ldo;
  long vbs;            // elements between consecutive batch items of vt
  int R, N, L, heads, d;
  float c;             // scale * log2(e)
};

constexpr int RG_VST = 36;    // V^T LDS row stride in halves (72 B), as af_attention
constexpr int RG_LP = 96;     // keys staged (zero beyond L <= 80)
constexpr int RG_TILE = 128;  // queries per workgroup

// DS: 16-channel steps of the first product, ceil(d / 16) rounded up to an instantiated value
template <int DS>
__global__ __launch_bounds__(256) void af_region_attn_kernel(RegionAttnArgs a) {
  constexpr int DP = 16 * DS, DT = (DS + 1) / 2, DV = 32 * DT;
  constexpr int KST = DP + 8;
  constexpr int KCH = RG_LP * (DP / 8);         // 16-byte chunks of K
  constexpr int VCH = DV * (RG_LP / 8);         // 16-byte chunks of V^T
  constexpr int NKC = (KCH + 255) / 256, NVC = (VCH + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char af_smem[];
  half_t* Ks = reinterpret_cast<half_t*>(af_smem);     // [RG_LP][KST]
  half_t* Vs = Ks + RG_LP * KST;                       // [3 sub][DV][RG_VST]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tile0 = blockIdx.x * RG_TILE;
  const int query = tile0 + wave * 32 + r32;
  const bool qok = query < a.N;
  const int nsub = (a.L + 31) >> 5;
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // ---- q fragments: lane (r32, hh) holds channels 16 s2 + 8 hh .. + 7 of its query; rows >= N and channels >= d are zero
  half8_t qf[DS];
  {
    const half_t* qp = a.q + ((size_t)b * a.N + (qok ? query : 0)) * a.ldq + h * a.d;
#pragma unroll
    for (int s2 = 0; s2 < DS; ++s2) {
      const int dc = 16 * s2 + 8 * hh;
      qf[s2] = (qok && dc < a.d) ? *reinterpret_cast<const half8_t*>(qp + dc) : zero8;
    }
  }

  // ---- which regions reach this tile (uniform over the workgroup: every wave reduces the same 128 words) and this wave's 32 queries
  unsigned wg_mask = 0, wv_mask = 0;
  for (int r = 0; r < a.R; ++r) {
    const float* wr = a.w + ((size_t)b * a.R + r) * a.ldw;
    const int q1 = tile0 + lane, q2 = tile0 + 64 + lane;
    const float f1 = q1 < a.N ? wr[q1] : 0.f, f2 = q2 < a.N ? wr[q2] : 0.f;
    const float own = qok ? wr[query] : 0.f;
    if (__ballot(f1 != 0.f || f2 != 0.f) != 0) wg_mask |= 1u << r;
    if (__ballot(own != 0.f) != 0) wv_mask |= 1u << r;
  }

  floatx16 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

#pragma unroll 1
  for (int r = 0; r < a.R; ++r) {
    if (!((wg_mask >> r) & 1u)) continue;        // workgroup-uniform: all four waves take the same branch, the barriers below are not divergent
    const size_t item = (size_t)b * a.R + r;
    __syncthreads();                             // every wave has finished reading the previous region's tiles
    {
      // all global loads are issued before the first LDS store (af_xattn_kernel's two-phase staging)
      half8_t rk[NKC], rv[NVC];
#pragma unroll
      for (int j = 0; j < NKC; ++j) {
        const int i = tid + 256 * j;
        const int row = i / (DP / 8), ch = i - row * (DP / 8);
        rk[j] = (i < KCH && row < a.L && ch * 8 < a.d)
                    ? *reinterpret_cast<const half8_t*>(a.k + (item * a.L + row) * a.ldk + h * a.d + ch * 8) : zero8;
      }
#pragma unroll
      for (int j = 0; j < NVC; ++j) {
        const int i = tid + 256 * j;
        const int row = i / (RG_LP / 8), kk = (i - row * (RG_LP / 8)) * 8;
        rv[j] = (i < VCH && row < a.d && kk < a.L)
                    ? *reinterpret_cast<const half8_t*>(a.vt + item * a.vbs + (size_t)(h * a.d + row) * a.ldv + kk) : zero8;
      }
#pragma unroll
      for (int j = 0; j < NKC; ++j) {
        const int i = tid + 256 * j;
        const int row = i / (DP / 8), ch = i - row * (DP / 8);
        if (i < KCH) *reinterpret_cast<half8_t*>(Ks + row * KST + ch * 8) = rk[j];
      }
#pragma unroll
      for (int j = 0; j < NVC; ++j) {
        const int i = tid + 256 * j;
        if (i < VCH) {
          const int row = i / (RG_LP / 8), ch = i - row * (RG_LP / 8), kk = ch * 8;
          half8_t v = rv[j];
          if (kk < a.L && kk + 8 > a.L) {        // the padding of V^T rows beyond L holds anything: zero it
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (kk + e >= a.L) v[e] = (half_t)0;
          }
          half_t* dst = Vs + ((ch >> 2) * DV + row) * RG_VST + (ch & 3) * 8;
          const half4_t lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
          *reinterpret_cast<half4_t*>(dst) = lo;
          *reinterpret_cast<half4_t*>(dst + 4) = hi;
        }
      }
    }
    __syncthreads();                             // K_r and V_r^T are in LDS
    if (!((wv_mask >> r) & 1u)) continue;        // this wave's queries take nothing from the region: no MFMA (and no barrier in here)
    const float wq = qok ? a.w[item * a.ldw + query] : 0.f;

    auto score_tile = [&](int sub) {
      floatx16 sc;
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[i] = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < DS; ++s2) {
        const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + (sub * 32 + r32) * KST + 16 * s2 + 8 * hh);
        sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s2], sc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = sub * 32 + 8 * (i >> 2) + 4 * hh + (i & 3);
        sc[i] = key < a.L ? sc[i] * a.c : -INFINITY;     // keys >= L (zero rows of the staged tile) are excluded
      }
      return sc;
    };
    float mx = -FLT_MAX;
#pragma unroll 1
    for (int sub = 0; sub < nsub; ++sub) {
      const floatx16 sc = score_tile(sub);
#pragma unroll
      for (int i = 0; i < 16; i += 2) mx = fmaxf(fmaxf(mx, sc[i]), sc[i + 1]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    floatx16 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[t][i] = 0.f;
    float l = 0.f;
#pragma unroll 1
    for (int sub = 0; sub < nsub; ++sub) {
      const floatx16 sc = score_tile(sub);
      half8_t pf[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float pv = __builtin_amdgcn_exp2f(sc[8 * s2 + j] - mx);
          l += pv;
          pf[s2][j] = (half_t)pv;
        }
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const half_t* vp = Vs + (sub * DV + 32 * t + r32) * RG_VST + 16 * s2 + 4 * hh;
          const half4_t lo = *reinterpret_cast<const half4_t*>(vp);
          const half4_t hi = *reinterpret_cast<const half4_t*>(vp + 8);
          const half8_t vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[s2], o[t], 0, 0, 0);
        }
    }
    l += __shfl_xor(l, 32, 64);
    const float coef = wq / l;
    const bool take = wq != 0.f;                 // a select, not a multiply: 0 * NaN must not reach the accumulator
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = take ? fmaf(o[t][i], coef, acc[t][i]) : acc[t][i];
  }

  if (qok) {
    half_t* op = a.o + ((size_t)b * a.N + query) * a.ldo + h * a.d;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = 32 * t + 8 * g + 4 * hh;
        if (dd < a.d) {
          const half4_t v = {(half_t)acc[t][4 * g + 0], (half_t)acc[t][4 * g + 1], (half_t)acc[t][4 * g + 2], (half_t)acc[t][4 * g + 3]};
          *reinterpret_cast<half4_t*>(op + dd) = v;
        }
      }
  }
}

template <int DS>
int launch_region_attn(const RegionAttnArgs& a, int B, hipStream_t stream) {
  constexpr int DP = 16 * DS, DT = (DS + 1) / 2, DV = 32 * DT;
  constexpr size_t lds = (size_t)(RG_LP * (DP + 8) + 3 * DV * RG_VST) * sizeof(half_t);      // at most 96 * 168 * 2 + 3 * 160 * 72 = 66816 bytes
  static bool attr_set = false;  // benign race: idempotent attribute
  if (!af_allow_dyn_lds(reinterpret_cast<const void*>(&af_region_attn_kernel<DS>), lds, attr_set, "af_region_attention")) return af_check_launch("af_region_attention");
  const unsigned blocks = (unsigned)((a.N + RG_TILE - 1) / RG_TILE);
  hipLaunchKernelGGL((af_region_attn_kernel<DS>), dim3(blocks, a.heads, B), dim3(256), lds, stream, a);
  return af_check_launch("af_region_attention");
}

// ---- region masks -> weights.  One workgroup (one wave) per 64 x 64-pixel block = one cell of the coarsest level; lane = one 8 x 8-pixel cell of
// level 0.  The 8-bit sums are integers (exact); the mean of a cell is sum / (255 area) and the rule is applied to the means of each level.
struct RegionWeightArgs {
  const unsigned char* masks;   // [R - 1][H][W]
  float* w;                     // [R][ldw], level l at columns off_l .. off_l + N_l
  int R, H, W, ldw;
  float beta;
};

__device__ inline void region_rule(const RegionWeightArgs& a, const int* sums, int area, int col) {
  // m_r = sum_r / (255 area); s = sum_r m_r; w_r = (1 - beta) m_r / max(1, s); w_0 = beta + (1 - beta) (1 - min(1, s))
  const float den = 255.f * (float)area;
  float s = 0.f;
  for (int r = 0; r + 1 < a.R; ++r) s += (float)sums[r] / den;
  const float nb = 1.f - a.beta, dn = fmaxf(1.f, s);
  for (int r = 0; r + 1 < a.R; ++r) a.w[(size_t)(r + 1) * a.ldw + col] = nb * ((float)sums[r] / den) / dn;
  a.w[col] = a.beta + nb * (1.f - fminf(1.f, s));
}

__global__ __launch_bounds__(64) void af_region_weights_kernel(RegionWeightArgs a) {
  __shared__ int s0[7][64];
  const int lane = threadIdx.x, cx = lane & 7, cy = lane >> 3;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int w0 = a.W >> 3, h0 = a.H >> 3;          // level-0 grid
  int own[7];
  for (int r = 0; r + 1 < a.R; ++r) {
    const unsigned char* mp = a.masks + ((size_t)r * a.H + (by * 64 + cy * 8)) * a.W + bx * 64 + cx * 8;   // W % 64 == 0: 8-byte aligned
    int sum = 0;
    for (int y = 0; y < 8; ++y) {
      const uint2 v = *reinterpret_cast<const uint2*>(mp + (size_t)y * a.W);
      sum += (v.x & 255) + ((v.x >> 8) & 255) + ((v.x >> 16) & 255) + (v.x >> 24) + (v.y & 255) + ((v.y >> 8) & 255) + ((v.y >> 16) & 255) + (v.y >> 24);
    }
    own[r] = sum;
    s0[r][lane] = sum;
  }
  __syncthreads();
  const int n0 = h0 * w0, n1 = n0 >> 2, n2 = n0 >> 4;
  region_rule(a, own, 64, (by * 8 + cy) * w0 + bx * 8 + cx);
  int sums[7];
  if (lane < 16) {                                  // level 1: 4 x 4 cells of 16 x 16 pixels
    const int x = lane & 3, y = lane >> 2;
    for (int r = 0; r + 1 < a.R; ++r) {
      int t = 0;
      for (int j = 0; j < 4; ++j) t += s0[r][(2 * y + (j >> 1)) * 8 + 2 * x + (j & 1)];
      sums[r] = t;
    }
    region_rule(a, sums, 256, n0 + (by * 4 + y) * (w0 >> 1) + bx * 4 + x);
  }
  if (lane < 4) {                                   // level 2: 2 x 2 cells of 32 x 32 pixels
    const int x = lane & 1, y = lane >> 1;
    for (int r = 0; r + 1 < a.R; ++r) {
      int t = 0;
      for (int j = 0; j < 16; ++j) t += s0[r][(4 * y + (j >> 2)) * 8 + 4 * x + (j & 3)];
      sums[r] = t;
    }
    region_rule(a, sums, 1024, n0 + n1 + (by * 2 + y) * (w0 >> 2) + bx * 2 + x);
  }
  if (lane == 0) {                                  // level 3: the block
    for (int r = 0; r + 1 < a.R; ++r) {
      int t = 0;
      for (int j = 0; j < 64; ++j) t += s0[r][j];
      sums[r] = t;
    }
    region_rule(a, sums, 4096, n0 + n1 + n2 + by * (w0 >> 3) + bx);
  }
}

}  // namespace

extern "C" int af_region_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldv, int64_t vt_batch_stride, const void* w,
                                   int ldw, void* o, int ldo, int B, int R, int N, int L, int heads, int d, float scale, void* stream) {
  AF_REQUIRE(q && k && vt && w && o, "af_region_attention: null pointer");
  AF_REQUIRE(B > 0 && B <= 65535 && N > 0 && heads > 0 && heads <= 65535, "af_region_attention: bad sizes");
  AF_REQUIRE(R >= 1 && R <= 8, "af_region_attention: 1 <= R <= 8 context sets");
  AF_REQUIRE(L >= 1 && L <= 80, "af_region_attention: 1 <= L <= 80 context tokens");
  AF_REQUIRE(d >= 8 && d <= 160 && d % 8 == 0, "af_region_attention: head dim must be a multiple of 8 in 8 .. 160");
  const int64_t C = (int64_t)heads * d;
  AF_REQUIRE(ldq % 8 == 0 && ldo % 8 == 0 && ldk % 8 == 0 && ldq >= C && ldo >= C && ldk >= C,
             "af_region_attention: row strides must be multiples of 8 and >= heads * d");
  AF_REQUIRE(ldv % 8 == 0 && ldv >= L, "af_region_attention: ldv must be a multiple of 8 and >= L");
  AF_REQUIRE(ldw >= N, "af_region_attention: ldw < N");
  AF_REQUIRE(vt_batch_stride % 8 == 0 && vt_batch_stride >= C * ldv, "af_region_attention: vt_batch_stride must be a multiple of 8 and cover heads * d rows of ldv");
  AF_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)w | (uintptr_t)o) % 16 == 0, "af_region_attention: operands must be 16-byte aligned");
  const int64_t lim = (int64_t)1 << 31, rows = (int64_t)B * N, items = (int64_t)B * R;
  AF_REQUIRE(rows < lim && rows * ldq < lim && rows * ldo < lim && items * L * ldk < lim && items * ldw < lim,
             "af_region_attention: an operand of 2^31 elements or more");
  AF_REQUIRE(vt_batch_stride < lim && (items - 1) * vt_batch_stride + C * ldv < lim, "af_region_attention: an operand of 2^31 elements or more");
  RegionAttnArgs a;
  a.q = (const half_t*)q;
  a.k = (const half_t*)k;
  a.vt = (const half_t*)vt;
  a.w = (const float*)w;
  a.o = (half_t*)o;
  a.ldq = ldq;
  a.ldk = ldk;
  a.ldv = ldv;
  a.ldw = ldw;
  a.ldo = ldo;
  a.vbs = (long)vt_batch_stride;
  a.R = R;
  a.N = N;
  a.L = L;
  a.heads = heads;
  a.d = d;
  a.c = scale * 1.4426950408889634f;
  AfLaunchScope scope(AF_FAM_XATTN, stream);
  hipStream_t s = (hipStream_t)stream;
  const int ds = (d + 15) / 16;
  if (ds <= 1) return launch_region_attn<1>(a, B, s);
  if (ds <= 2) return launch_region_attn<2>(a, B, s);
  if (ds <= 3) return launch_region_attn<3>(a, B, s);
  if (ds <= 4) return launch_region_attn<4>(a, B, s);
  if (ds <= 5) return launch_region_attn<5>(a, B, s);
  if (ds <= 6) return launch_region_attn<6>(a, B, s);
  if (ds <= 8) return launch_region_attn<8>(a, B, s);
  return launch_region_attn<10>(a, B, s);
}

extern "C" int af_region_weights(const void* masks, int R, int H, int W, float beta, void* w, int ldw, void* stream) {
  AF_REQUIRE(w && (masks || R == 1), "af_region_weights: null pointer");
  AF_REQUIRE(R >= 1 && R <= 8, "af_region_weights: 1 <= R <= 8 context sets (R - 1 masks)");
  AF_REQUIRE(H >= 64 && W >= 64 && H % 64 == 0 && W % 64 == 0 && H <= 16384 && W <= 16384, "af_region_weights: H and W must be multiples of 64 in 64 .. 16384");
  AF_REQUIRE(beta >= 0.f && beta <= 1.f, "af_region_weights: beta outside [0, 1]");
  const int64_t n0 = (int64_t)(H / 8) * (W / 8), total = n0 + n0 / 4 + n0 / 16 + n0 / 64;
  AF_REQUIRE(ldw >= total && (int64_t)R * ldw < ((int64_t)1 << 31), "af_region_weights: ldw must cover the four levels (85 H W / 4096 columns)");
  AF_REQUIRE(((uintptr_t)masks % 8 == 0) && ((uintptr_t)w % 4 == 0), "af_region_weights: masks must be 8-byte aligned");
  RegionWeightArgs a;
  a.masks = (const unsigned char*)masks;
  a.w = (float*)w;
  a.R = R;
  a.H = H;
  a.W = W;
  a.ldw = ldw;
  a.beta = beta;
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(af_region_weights_kernel, dim3(W / 64, H / 64), dim3(64), 0, (hipStream_t)stream, a);
  return af_check_launch("af_region_weights");
}
