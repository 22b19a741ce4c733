// af_temporal_attn.hip -- self-attention along the FRAME axis (AnimateDiff motion modules): a sequence is the F <= 32 frames of one pixel of one
// head, its tokens lie HW rows apart in the token-major activation.  One wave owns one (batch item, pixel, head) unit, the four waves of a
// workgroup take four consecutive heads (or the first heads of the next pixel), so a workgroup consumes contiguous spans of the F rows it touches.
//   * every q / k / v element is read from memory once, with 16-byte loads: q and k go straight into MFMA operand registers (lane = (frame,
//     8-channel chunk)), v goes through a wave-private LDS tile because the second product needs it with the frame index in the registers;
//   * S^T = K Q^T (v_mfma_f32_16x16x32_f16, channels zero-padded to a multiple of 32): the query sits on the MFMA lane, a lane's registers and
//     its three partner lane groups hold the keys, so the softmax is register maxima / sums plus two cross-lane steps;
//   * scores, reference, sum and the P V accumulation are fp32; P^T = exp2(S^T scale log2(e) - m) <= 1 is rounded to fp16 and IS the B operand
//     of O^T = V^T P^T (v_mfma_f32_16x16x16_f16: its k layout is the C/D row layout of the first product), 1 / l is applied in fp32;
//   * tails: frames >= F are zero-filled in registers / LDS and their scores are -inf, never read; a wave whose unit lies past the last one
//     computes on zeros and stores nothing; channel chunks >= d / 8 of the last 32-channel step are zero;
//   * the result goes back through the same LDS tile so that it leaves in 16-byte stores.
// Traffic: 2 (3 C + C) bytes per token row of a dense qkv; FLOPs (4 F d per token and head) are far below the memory time.
#include <math.h>

#include "af_common.h"

namespace {

struct TemporalAttnArgs {
  const half_t* qkv;
  half_t* out;
  int ld, B, F, HW, heads, d;
  int units;      // B * HW * heads
  float scale2;   // scale * log2(e)
};

constexpr int TA_WAVES = 4;

// NF: 16-frame tiles (1 or 2); KS: 32-channel steps of the first product, ceil(d / 32)
template <int NF, int KS>
__global__ __launch_bounds__(TA_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void af_temporal_attn_kernel(TemporalAttnArgs a) {
  constexpr int JT = 2 * KS;                      // 16-channel tiles of the second product; channels >= d are computed on the row pad and never stored
  constexpr int VST = 32 * KS + 8;                // LDS row stride in halves (rows stay 16-byte aligned); a constant keeps the addressing in immediates
  extern __shared__ __attribute__((aligned(16))) char af_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, hg = lane >> 4;
  const int d = a.d, F = a.F, D8 = d >> 3;
  half_t* Vs = reinterpret_cast<half_t*>(af_smem) + (size_t)wave * (16 * NF) * VST;

  const int unit = blockIdx.x * TA_WAVES + wave;
  const bool live = unit < a.units;
  const int u = live ? unit : 0;
  const int h = u % a.heads;
  const int bp = u / a.heads;
  const int p = bp % a.HW, b = bp / a.HW;
  const half_t* base = a.qkv + ((size_t)b * F * a.HW + p) * a.ld + h * d;      // q of frame 0; k at + C, v at + 2 C; frame step HW * ld
  const size_t fstep = (size_t)a.HW * a.ld;
  const int C = a.heads * d;
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // ---- q / k operand fragments: lane (lr, hg) holds channels 8 (4 s + hg) .. + 7 of frame 16 t + lr
  half8_t qf[NF][KS], kf[NF][KS];
#pragma unroll
  for (int t = 0; t < NF; ++t) {
    const int fr = 16 * t + lr;
    const half_t* rp = base + (size_t)(fr < F ? fr : 0) * fstep;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c8 = 4 * s + hg;
      const bool ok = live && fr < F && c8 < D8;
      qf[t][s] = ok ? *reinterpret_cast<const half8_t*>(rp + 8 * c8) : zero8;
      kf[t][s] = ok ? *reinterpret_cast<const half8_t*>(rp + C + 8 * c8) : zero8;
    }
  }
  // ---- v tile -> LDS [16 NF frames][d], frames >= F zero
#pragma nounroll
  for (int i = lane; i < 16 * NF * D8; i += 64) {
    const int fr = i / D8, c8 = i - fr * D8;
    const bool ok = live && fr < F;
    const half8_t v = ok ? *reinterpret_cast<const half8_t*>(base + (size_t)fr * fstep + 2 * C + 8 * c8) : zero8;
    *reinterpret_cast<half8_t*>(Vs + fr * VST + 8 * c8) = v;
  }

  // ---- S^T[key 16 gt + 4 hg + reg][query 16 ft + lr]
  floatx4 st[NF][NF];
#pragma unroll
  for (int gt = 0; gt < NF; ++gt)
#pragma unroll
    for (int ft = 0; ft < NF; ++ft) {
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[gt][s], qf[ft][s], acc, 0, 0, 0);
      st[gt][ft] = acc;
    }

  // ---- softmax over the keys of each query (base 2); key 0 is always valid, so the reference is finite
  half4_t pf[NF][NF];
  float inv[NF];
#pragma unroll
  for (int ft = 0; ft < NF; ++ft) {
    float m = -INFINITY;
#pragma unroll
    for (int gt = 0; gt < NF; ++gt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = 16 * gt + 4 * hg + e < F ? st[gt][ft][e] * a.scale2 : -INFINITY;
        st[gt][ft][e] = s;
        m = fmaxf(m, s);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int gt = 0; gt < NF; ++gt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = __builtin_amdgcn_exp2f(st[gt][ft][e] - m);
        l += pe;
        pf[gt][ft][e] = (half_t)pe;
      }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    inv[ft] = 1.0f / l;
  }

  __syncthreads();   // the v tile is in LDS

  // ---- O^T[channel 16 jt + 4 hg + reg][query 16 ft + lr] = sum over keys V[key][channel] P^T[key][query]
  floatx4 o[JT][NF];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
    for (int ft = 0; ft < NF; ++ft) o[jt][ft] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int gt = 0; gt < NF; ++gt) {
      const half_t* vp = Vs + (16 * gt + 4 * hg) * VST + 16 * jt + lr;         // lane: channel 16 jt + lr, keys 16 gt + 4 hg + e
      const half4_t vf = {vp[0], vp[VST], vp[2 * VST], vp[3 * VST]};
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) o[jt][ft] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[gt][ft], o[jt][ft], 0, 0, 0);
    }
  }

  __syncthreads();   // every v read is done: the tile now takes the result, [frame][channel]
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
    for (int ft = 0; ft < NF; ++ft) {
      const half4_t r = {(half_t)(o[jt][ft][0] * inv[ft]), (half_t)(o[jt][ft][1] * inv[ft]), (half_t)(o[jt][ft][2] * inv[ft]),
                         (half_t)(o[jt][ft][3] * inv[ft])};
      *reinterpret_cast<half4_t*>(Vs + (16 * ft + lr) * VST + 16 * jt + 4 * hg) = r;     // channels < 16 JT < VST: inside the row
    }
  }
  __syncthreads();
  if (live) {
    half_t* ob = a.out + ((size_t)b * F * a.HW + p) * C + h * d;
    const size_t ostep = (size_t)a.HW * C;
#pragma nounroll
    for (int i = lane; i < F * D8; i += 64) {
      const int fr = i / D8, c8 = i - fr * D8;
      *reinterpret_cast<half8_t*>(ob + (size_t)fr * ostep + 8 * c8) = *reinterpret_cast<const half8_t*>(Vs + fr * VST + 8 * c8);
    }
  }
}

template <int NF, int KS>
int launch_temporal_attn(const TemporalAttnArgs& a, hipStream_t stream) {
  constexpr size_t lds = (size_t)TA_WAVES * (16 * NF) * (32 * KS + 8) * sizeof(half_t);   // at most 4 * 32 * 168 * 2 = 43008 bytes
  const unsigned blocks = (unsigned)((a.units + TA_WAVES - 1) / TA_WAVES);
  hipLaunchKernelGGL((af_temporal_attn_kernel<NF, KS>), dim3(blocks), dim3(TA_WAVES * 64), lds, stream, a);
  return af_check_launch("af_temporal_attention");
}

template <int NF>
int dispatch_temporal_attn(const TemporalAttnArgs& a, hipStream_t stream) {
  switch ((a.d + 31) / 32) {
    case 1: return launch_temporal_attn<NF, 1>(a, stream);
    case 2: return launch_temporal_attn<NF, 2>(a, stream);
    case 3: return launch_temporal_attn<NF, 3>(a, stream);
    case 4: return launch_temporal_attn<NF, 4>(a, stream);
    default: return launch_temporal_attn<NF, 5>(a, stream);
  }
}

}  // namespace

extern "C" int af_temporal_attention(const void* qkv, int ld, void* out, int B, int F, int HW, int heads, int d, float scale, void* stream) {
  AF_REQUIRE(qkv && out, "af_temporal_attention: null pointer");
  AF_REQUIRE(B > 0 && HW > 0 && heads > 0, "af_temporal_attention: bad sizes");
  AF_REQUIRE(F >= 1 && F <= 32, "af_temporal_attention: 1 <= F <= 32 frames");
  AF_REQUIRE(d >= 8 && d <= 160 && d % 8 == 0, "af_temporal_attention: head dim must be a multiple of 8 in 8 .. 160");
  const int64_t C = (int64_t)heads * d;
  AF_REQUIRE(ld % 8 == 0 && (int64_t)ld >= 3 * C, "af_temporal_attention: ld must be a multiple of 8 and >= 3 * heads * d");
  AF_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0, "af_temporal_attention: operands must be 16-byte aligned");
  const int64_t lim = (int64_t)1 << 31, rows = (int64_t)B * F * HW;
  AF_REQUIRE(rows < lim && rows * ld < lim && rows * C < lim, "af_temporal_attention: an operand of 2^31 elements or more");
  TemporalAttnArgs a;
  a.qkv = (const half_t*)qkv;
  a.out = (half_t*)out;
  a.ld = ld;
  a.B = B;
  a.F = F;
  a.HW = HW;
  a.heads = heads;
  a.d = d;
  a.units = (int)((int64_t)B * HW * heads);
  a.scale2 = scale * 1.4426950408889634f;
  AfLaunchScope scope(AF_FAM_ATTN, stream);
  return F <= 16 ? dispatch_temporal_attn<1>(a, (hipStream_t)stream) : dispatch_temporal_attn<2>(a, (hipStream_t)stream);
}
