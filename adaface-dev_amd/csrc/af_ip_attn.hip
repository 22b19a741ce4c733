// af_ip_attn.hip -- the image-prompt half of IP-Adapter's decoupled cross-attention, added IN PLACE to the text attention's output:
//     o[b N + i, h d + j] = fp16( float(o[..]) + ip_scale * sum_t softmax_t(scale <q[b, i, h, :], k[b, t, h, :]>) v[b, t, h, j] ),  t over T <= 64 image tokens.
// k and v are ROW-MAJOR token rows ([T][>= heads d] per batch item, the layout the stacked to_k_ip | to_v_ip projection GEMM writes), each with its
// own row stride and its own element stride between batch items, so a layer reads its column slice of the one stacked projection in place.
// One workgroup (4 waves) owns one (batch item, head) and 64 consecutive query rows, 16 per wave.  (Walking 2 or 4 such tiles per wave to spread
// the K / V loads over more rows was measured and never faster: at N = 1024 it halves the workgroups and costs 16 -> 24 us, profiles/ip_adapter.txt.)
//   * K of the (b, h) sits in MFMA operand registers, V in one LDS tile shared by the four waves (keys >= T zero);
//   * every q and o element is touched once with 16-byte accesses: q goes straight into operand registers (lane = (query, 8-channel chunk)),
//     the o tile goes through a wave-private LDS tile [query][channel] in which it is updated and from which it leaves;
//   * S^T = K Q^T (v_mfma_f32_16x16x32_f16, channels zero-padded to a multiple of 32), the query on the MFMA lane, so the softmax is register
//     maxima / sums plus two cross-lane steps; P^T = exp2(S^T scale log2(e) - m) <= 1 is rounded to fp16 ONCE and is the B operand of
//     O^T = V^T P^T (v_mfma_f32_16x16x16_f16); scores, reference, sum and accumulation are fp32;
//   * the text result and the image result are summed in fp32 and rounded once: o_new = fp16(float(o_old) + (ip_scale / l) acc);
//   * tails: keys >= T are zero in registers / LDS and their scores are -inf; query rows >= N are computed on zeros and never stored; channels
//     >= d of the last 32-channel step are computed on the LDS row pad and never stored.
// Traffic: 2 * 3 * B N C bytes (q read, o read and written) plus the K / V tiles per workgroup from L2; the MFMAs (4 T d FLOP per query and head,
// T padded to 16) are far below the memory time -- the 16 x 16 MFMA form was chosen over VALU dot products because at T = 64, d = 160 the VALU
// form (2 T d FMA per query and head) would cost about three times the memory time, and the layout is the one af_temporal_attention runs on.
#include <math.h>

#include "af_common.h"

namespace {

struct IpAttnArgs {
  const half_t* q;
  const half_t* k;
  const half_t* v;
  half_t* o;
  int ldq, ldo, ldk, ldv;
  int kbs, vbs;        // element stride between batch items of k / v
  int N, T, heads, d;
  float scale2;        // scale * log2(e)
  float ip_scale;
};

constexpr int IP_WAVES = 4;

// NT: 16-key tiles (1, 2 or 4); KS: 32-channel steps of the first product, ceil(d / 32)
template <int NT, int KS>
__global__ __launch_bounds__(IP_WAVES * 64) void af_ip_attn_kernel(IpAttnArgs a) {
  constexpr int JT = 2 * KS;                      // 16-channel tiles of the second product
  constexpr int VST = 32 * KS + 8;                // LDS row stride in halves (rows stay 16-byte aligned)
  extern __shared__ __attribute__((aligned(16))) char af_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, hg = lane >> 4;
  const int d = a.d, T = a.T, N = a.N, D8 = d >> 3;
  const int h = blockIdx.y, b = blockIdx.z;
  half_t* Vs = reinterpret_cast<half_t*>(af_smem);                      // [16 NT keys][VST]
  half_t* Os = Vs + (16 * NT) * VST + (size_t)wave * 16 * VST;          // this wave's [16 queries][VST]
  const half_t* kb = a.k + (size_t)b * a.kbs + h * d;
  const half_t* vb = a.v + (size_t)b * a.vbs + h * d;
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // ---- K operand fragments: lane (lr, hg) holds channels 8 (4 s + hg) .. + 7 of key 16 gt + lr
  half8_t kf[NT][KS];
#pragma unroll
  for (int gt = 0; gt < NT; ++gt) {
    const int key = 16 * gt + lr;
    const half_t* rp = kb + (size_t)(key < T ? key : 0) * a.ldk;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c8 = 4 * s + hg;
      kf[gt][s] = (key < T && c8 < D8) ? *reinterpret_cast<const half8_t*>(rp + 8 * c8) : zero8;
    }
  }
  // ---- V tile -> LDS [16 NT keys][d], keys >= T zero
#pragma nounroll
  for (int i = threadIdx.x; i < 16 * NT * D8; i += IP_WAVES * 64) {
    const int key = i / D8, c8 = i - key * D8;
    const half8_t v = key < T ? *reinterpret_cast<const half8_t*>(vb + (size_t)key * a.ldv + 8 * c8) : zero8;
    *reinterpret_cast<half8_t*>(Vs + key * VST + 8 * c8) = v;
  }

  const int r0 = (blockIdx.x * IP_WAVES + wave) * 16;          // every wave of the workgroup runs the whole body (a dead one on zeros): the barriers are uniform
  // ---- q operand fragments: lane (lr, hg) holds channels 8 (4 s + hg) .. + 7 of query r0 + lr; rows >= N are zero
  half8_t qf[KS];
  {
    const int row = r0 + lr;
    const bool rok = row < N;
    const half_t* rp = a.q + ((size_t)b * N + (rok ? row : 0)) * a.ldq + h * d;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c8 = 4 * s + hg;
      qf[s] = (rok && c8 < D8) ? *reinterpret_cast<const half8_t*>(rp + 8 * c8) : zero8;
    }
  }
  // ---- the o tile -> this wave's LDS tile; rows >= N stay whatever they were and are never stored
#pragma nounroll
  for (int i = lane; i < 16 * D8; i += 64) {
    const int rr = i / D8, c8 = i - rr * D8;
    if (r0 + rr < N)
      *reinterpret_cast<half8_t*>(Os + rr * VST + 8 * c8) = *reinterpret_cast<const half8_t*>(a.o + ((size_t)b * N + r0 + rr) * a.ldo + h * d + 8 * c8);
  }

  // ---- S^T[key 16 gt + 4 hg + reg][query lr]
  floatx4 st[NT];
#pragma unroll
  for (int gt = 0; gt < NT; ++gt) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[gt][s], qf[s], acc, 0, 0, 0);
    st[gt] = acc;
  }
  // ---- softmax over the keys of each query (base 2); key 0 is always valid, so the reference is finite
  half4_t pf[NT];
  float m = -INFINITY;
#pragma unroll
  for (int gt = 0; gt < NT; ++gt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = 16 * gt + 4 * hg + e < T ? st[gt][e] * a.scale2 : -INFINITY;
      st[gt][e] = s;
      m = fmaxf(m, s);
    }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l = 0.f;
#pragma unroll
  for (int gt = 0; gt < NT; ++gt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pe = __builtin_amdgcn_exp2f(st[gt][e] - m);
      l += pe;
      pf[gt][e] = (half_t)pe;
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float w = a.ip_scale / l;

  __syncthreads();   // the V tile and this wave's o tile are in LDS

  // ---- O^T[channel 16 jt + 4 hg + reg][query lr] = sum over keys V[key][channel] P^T[key][query], then o += w O^T in fp32, rounded once
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int gt = 0; gt < NT; ++gt) {
      const half_t* vp = Vs + (16 * gt + 4 * hg) * VST + 16 * jt + lr;         // lane: channel 16 jt + lr, keys 16 gt + 4 hg + e
      const half4_t vf = {vp[0], vp[VST], vp[2 * VST], vp[3 * VST]};
      acc = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[gt], acc, 0, 0, 0);
    }
    half4_t* op = reinterpret_cast<half4_t*>(Os + lr * VST + 16 * jt + 4 * hg);   // channels < 16 JT < VST: inside the row
    const half4_t old = *op;
    const half4_t r = {(half_t)fmaf(acc[0], w, (float)old[0]), (half_t)fmaf(acc[1], w, (float)old[1]), (half_t)fmaf(acc[2], w, (float)old[2]),
                       (half_t)fmaf(acc[3], w, (float)old[3])};
    *op = r;
  }

  __syncthreads();   // the tile holds the updated rows
#pragma nounroll
  for (int i = lane; i < 16 * D8; i += 64) {
    const int rr = i / D8, c8 = i - rr * D8;
    if (r0 + rr < N)
      *reinterpret_cast<half8_t*>(a.o + ((size_t)b * N + r0 + rr) * a.ldo + h * d + 8 * c8) = *reinterpret_cast<const half8_t*>(Os + rr * VST + 8 * c8);
  }
}

template <int NT, int KS>
int launch_ip_attn(const IpAttnArgs& a, int B, hipStream_t stream) {
  constexpr size_t lds = (size_t)(16 * NT + IP_WAVES * 16) * (32 * KS + 8) * sizeof(half_t);   // at most 128 * 168 * 2 = 43008 bytes
  constexpr int rows_per_wg = IP_WAVES * 16;
  const unsigned blocks = (unsigned)((a.N + rows_per_wg - 1) / rows_per_wg);
  hipLaunchKernelGGL((af_ip_attn_kernel<NT, KS>), dim3(blocks, a.heads, B), dim3(IP_WAVES * 64), lds, stream, a);
  return af_check_launch("af_ip_attention_add");
}

template <int NT>
int dispatch_ip_attn(const IpAttnArgs& a, int B, hipStream_t stream) {
  switch ((a.d + 31) / 32) {
    case 1: return launch_ip_attn<NT, 1>(a, B, stream);
    case 2: return launch_ip_attn<NT, 2>(a, B, stream);
    case 3: return launch_ip_attn<NT, 3>(a, B, stream);
    case 4: return launch_ip_attn<NT, 4>(a, B, stream);
    default: return launch_ip_attn<NT, 5>(a, B, stream);
  }
}

}  // namespace

extern "C" int af_ip_attention_add(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, int64_t k_bstride, const void* v, int ldv,
                                   int64_t v_bstride, int B, int N, int T, int heads, int d, float scale, float ip_scale, void* stream) {
  AF_REQUIRE(o && q && k && v, "af_ip_attention_add: null pointer");
  AF_REQUIRE(B > 0 && B <= 65535 && N > 0 && heads > 0 && heads <= 65535, "af_ip_attention_add: bad sizes");
  AF_REQUIRE(T >= 1 && T <= 64, "af_ip_attention_add: 1 <= T <= 64 image tokens");
  AF_REQUIRE(d >= 8 && d <= 160 && d % 8 == 0, "af_ip_attention_add: head dim must be a multiple of 8 in 8 .. 160");
  const int64_t C = (int64_t)heads * d;
  AF_REQUIRE(ldq % 8 == 0 && ldo % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldq >= C && ldo >= C && ldk >= C && ldv >= C,
             "af_ip_attention_add: row strides must be multiples of 8 and >= heads * d");
  AF_REQUIRE(k_bstride >= 0 && v_bstride >= 0 && k_bstride % 8 == 0 && v_bstride % 8 == 0, "af_ip_attention_add: batch strides must be multiples of 8 and >= 0");
  AF_REQUIRE(((uintptr_t)o | (uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0, "af_ip_attention_add: operands must be 16-byte aligned");
  const int64_t lim = (int64_t)1 << 31, rows = (int64_t)B * N;
  AF_REQUIRE(rows < lim && rows * ldq < lim && rows * ldo < lim, "af_ip_attention_add: an operand of 2^31 elements or more");
  AF_REQUIRE(k_bstride < lim && v_bstride < lim && (B - 1) * k_bstride + (int64_t)(T - 1) * ldk + C < lim && (B - 1) * v_bstride + (int64_t)(T - 1) * ldv + C < lim,
             "af_ip_attention_add: an operand of 2^31 elements or more");
  if (ip_scale == 0.f) return AF_OK;
  IpAttnArgs a;
  a.q = (const half_t*)q;
  a.k = (const half_t*)k;
  a.v = (const half_t*)v;
  a.o = (half_t*)o;
  a.ldq = ldq;
  a.ldo = ldo;
  a.ldk = ldk;
  a.ldv = ldv;
  a.kbs = (int)k_bstride;
  a.vbs = (int)v_bstride;
  a.N = N;
  a.T = T;
  a.heads = heads;
  a.d = d;
  a.scale2 = scale * 1.4426950408889634f;
  a.ip_scale = ip_scale;
  AfLaunchScope scope(AF_FAM_ATTN, stream);
  if (T <= 16) return dispatch_ip_attn<1>(a, B, (hipStream_t)stream);
  if (T <= 32) return dispatch_ip_attn<2>(a, B, (hipStream_t)stream);
  return dispatch_ip_attn<4>(a, B, (hipStream_t)stream);
}
