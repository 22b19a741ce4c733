// af_gfpgan.hip -- the kernels of the GFPGAN face restorer (adaface/gfpgan.py, GFPGANv1Clean) around the tuned convolutions of af_gemm.
//   af_modulate_weights      StyleGAN2's modulated convolution as a plain convolution on PER-SAMPLE weights: gain * d[b,o] * W[o,t,i] * s[b,i] into
//                            af_gemm's packed fp16 layout.  The activations stay unscaled and every weight row has unit norm (times gain), which is
//                            what fp16 wants; scaling the activations by the styles instead would leave fp16's range.
//   af_style_epilogue        + noise + bias, LeakyReLU 0.2, the SFT of the upper half of the channels, saturating fp16 conversion: one pass.
//   af_bilinear_up2          x2 bilinear (align_corners=False) with an optional addend (the RGB skip path).
//   af_face_paste_affine_u8  restored crops back into the uint8 photo under the faces' similarities, with a soft border.
// All four are memory-bound element-wise kernels: 16-byte accesses, 8 halves per lane (the paste works on bytes of one pixel per lane).
// Every product and sum is rounded on its own, as the header's formulas are written (no fused contraction).
#include "af_common.h"

#pragma clang fp contract(off)

namespace {

constexpr long LIM = 1L << 31;

inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One workgroup per (output channel o, sample b).  Pass 1: the demodulation sum over cin (lane-strided, wave-64 shuffle reduction, four partials
// through LDS).  Pass 2: the K = taps * cin row in 8-element pieces, one 16-byte store each; cin % 8 == 0 keeps a piece inside one tap.
__global__ __launch_bounds__(256) void modulate_weights_kernel(const float* __restrict__ w, const float* __restrict__ wsq,
                                                               const float* __restrict__ styles, half_t* __restrict__ out, int cout, int cin,
                                                               int taps, int npad, int kpad, int demod, float gain) {
  __shared__ float part[4];
  const int o = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* s = styles + (long)b * cin;
  float d = 1.f;
  if (demod) {
    const float* q = wsq + (long)o * cin;
    float acc = 0.f;
    for (int i = tid; i < cin; i += 256) acc += s[i] * s[i] * q[i];
    acc = af_wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    d = 1.0f / sqrtf(part[0] + part[1] + part[2] + part[3] + 1e-8f);
  }
  const float gd = gain * d;
  const int K = taps * cin;
  const float* wr = w + (long)o * K;
  half_t* dst = out + ((long)b * npad + o) * kpad;
  for (int k0 = tid * 8; k0 < K; k0 += 256 * 8) {
    const int i0 = k0 % cin;
    const floatx4 w0 = *reinterpret_cast<const floatx4*>(wr + k0), w1 = *reinterpret_cast<const floatx4*>(wr + k0 + 4);
    const floatx4 s0 = *reinterpret_cast<const floatx4*>(s + i0), s1 = *reinterpret_cast<const floatx4*>(s + i0 + 4);
    half8_t h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      h[e] = (half_t)(gd * w0[e] * s0[e]);
      h[4 + e] = (half_t)(gd * w1[e] * s1[e]);
    }
    *reinterpret_cast<half8_t*>(dst + k0) = h;
  }
}

__global__ __launch_bounds__(256) void style_epilogue_kernel(const half_t* __restrict__ y, const float* __restrict__ noise,
                                                             const float* __restrict__ bias, const half_t* __restrict__ scale,
                                                             const half_t* __restrict__ shift, half_t* __restrict__ out, int HW, int C8, float nw,
                                                             long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c0 = (int)(i % C8) * 8;
  const long row = i / C8;                                     // b * HW + p
  const int p = (int)(row % HW);
  const int C = C8 * 8, Ch = C >> 1;
  const half8_t v = *reinterpret_cast<const half8_t*>(y + i * 8);
  const float nz = noise ? nw * noise[p] : 0.f;
  const bool sft = scale != nullptr && c0 >= Ch;               // Ch % 8 == 0 (checked by the caller): a piece lies on one side
  half8_t sc = {0, 0, 0, 0, 0, 0, 0, 0}, sh = {0, 0, 0, 0, 0, 0, 0, 0};
  if (sft) {
    sc = *reinterpret_cast<const half8_t*>(scale + row * Ch + (c0 - Ch));
    sh = *reinterpret_cast<const half8_t*>(shift + row * Ch + (c0 - Ch));
  }
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float f = (float)v[e] + nz;
    if (bias) f += bias[c0 + e];
    f = f >= 0.f ? f : 0.2f * f;
    if (sft) f = f * (float)sc[e] + (float)sh[e];
    o[e] = (half_t)fminf(fmaxf(f, -65504.f), 65504.f);
  }
  *reinterpret_cast<half8_t*>(out + i * 8) = o;
}

__global__ __launch_bounds__(256) void bilinear_up2_kernel(const half_t* __restrict__ x, const half_t* __restrict__ addend,
                                                           half_t* __restrict__ out, int H, int W, int C8, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c = (int)(i % C8);
  long r = i / C8;
  const int ox = (int)(r % (2 * W));
  r /= 2 * W;
  const int oy = (int)(r % (2 * H));
  const long b = r / (2 * H);
  const int ky = oy >> 1, kx = ox >> 1;
  const bool oddy = oy & 1, oddx = ox & 1;
  const int y0 = max(oddy ? ky : ky - 1, 0), y1 = min(oddy ? ky + 1 : ky, H - 1);
  const int x0 = max(oddx ? kx : kx - 1, 0), x1 = min(oddx ? kx + 1 : kx, W - 1);
  const float wy0 = oddy ? 0.75f : 0.25f, wy1 = 1.f - wy0, wx0 = oddx ? 0.75f : 0.25f, wx1 = 1.f - wx0;
  const long C = 8L * C8;
  const half_t* base = x + b * H * W * C + c * 8;
  const half8_t a = *reinterpret_cast<const half8_t*>(base + ((long)y0 * W + x0) * C);
  const half8_t bq = *reinterpret_cast<const half8_t*>(base + ((long)y0 * W + x1) * C);
  const half8_t cq = *reinterpret_cast<const half8_t*>(base + ((long)y1 * W + x0) * C);
  const half8_t dq = *reinterpret_cast<const half8_t*>(base + ((long)y1 * W + x1) * C);
  half8_t ad = {0, 0, 0, 0, 0, 0, 0, 0};
  if (addend) ad = *reinterpret_cast<const half8_t*>(addend + i * 8);
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float top = wx0 * (float)a[e] + wx1 * (float)bq[e], bot = wx0 * (float)cq[e] + wx1 * (float)dq[e];
    float f = wy0 * top + wy1 * bot;
    if (addend) f += (float)ad[e];
    o[e] = (half_t)f;
  }
  *reinterpret_cast<half8_t*>(out + i * 8) = o;
}

// One lane per photo pixel.  A face is sampled only where m > erode >= 0, i.e. strictly inside the crop: x0 = floor(u) lies in [0, S - 2] (clamped all
// the same), so no tap leaves the crop and no address is formed for a skipped face (NaN coordinates fail the comparison).
__global__ __launch_bounds__(256) void face_paste_affine_u8_kernel(const unsigned char* __restrict__ photo, const half_t* __restrict__ crops,
                                                                   const float* __restrict__ mats, unsigned char* __restrict__ out, int W, int F,
                                                                   int S, int ld, float erode, float feather, int npix) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const int x = i % W, y = i / W;
  const unsigned char* src = photo + i * 3;
  const unsigned char p0 = src[0], p1 = src[1], p2 = src[2];
  float cur[3] = {(float)p0, (float)p1, (float)p2};
  bool touched = false;
  const float top = (float)(S - 1);
  for (int f = 0; f < F; ++f) {
    const float* m = mats + f * 6;
    const float u = m[0] * (float)x + m[1] * (float)y + m[2], v = m[3] * (float)x + m[4] * (float)y + m[5];
    const float md = fminf(fminf(u, v), fminf(top - u, top - v));
    if (!(md > erode) || !(u == u) || !(v == v)) continue;
    const float t = feather > 0.f ? fminf((md - erode) / feather, 1.f) : 1.f;
    const float alpha = t * t * (3.f - 2.f * t);
    const int x0 = min(max((int)floorf(u), 0), S - 2), y0 = min(max((int)floorf(v), 0), S - 2);
    const float ax = u - (float)x0, ay = v - (float)y0;
    const half_t* c00 = crops + (((long)f * S + y0) * S + x0) * ld;
    const half_t* c10 = c00 + (long)S * ld;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t0 = (1.f - ax) * (float)c00[c] + ax * (float)c00[ld + c];
      const float t1 = (1.f - ax) * (float)c10[c] + ax * (float)c10[ld + c];
      const float bil = (1.f - ay) * t0 + ay * t1;
      const float g = 255.f * fminf(fmaxf(bil / 2.f + 0.5f, 0.f), 1.f);
      const float ag = alpha * g, keep = (1.f - alpha) * cur[c];
      cur[c] = ag + keep;
    }
    touched = true;
  }
  unsigned char* dst = out + i * 3;
  dst[0] = touched ? (unsigned char)rintf(fminf(fmaxf(cur[0], 0.f), 255.f)) : p0;
  dst[1] = touched ? (unsigned char)rintf(fminf(fmaxf(cur[1], 0.f), 255.f)) : p1;
  dst[2] = touched ? (unsigned char)rintf(fminf(fmaxf(cur[2], 0.f), 255.f)) : p2;
}

}  // namespace

extern "C" int af_modulate_weights(const void* w, const void* wsq, const void* styles, void* out, int B, int cout, int cin, int taps, int npad,
                                   int kpad, int demod, float gain, void* stream) {
  AF_REQUIRE(w && styles && out, "af_modulate_weights: w, styles and out must not be NULL");
  AF_REQUIRE(demod == 0 || demod == 1, "af_modulate_weights: demod must be 0 or 1");
  AF_REQUIRE(wsq || !demod, "af_modulate_weights: demodulation needs wsq");
  AF_REQUIRE(B > 0 && cout > 0 && cin > 0 && cin % 8 == 0, "af_modulate_weights: B and cout must be positive, cin a positive multiple of 8");
  AF_REQUIRE(taps == 1 || taps == 9, "af_modulate_weights: taps must be 1 or 9");
  const long K = (long)taps * cin;
  AF_REQUIRE(kpad > 0 && kpad % 64 == 0 && kpad >= K, "af_modulate_weights: kpad must be a multiple of 64 and at least taps * cin");
  AF_REQUIRE(npad > 0 && npad % 128 == 0 && npad >= cout, "af_modulate_weights: npad must be a multiple of 128 and at least cout");
  AF_REQUIRE((long)B * npad * kpad < LIM && (long)cout * K < LIM && (long)B * cin < LIM,
             "af_modulate_weights: B * npad * kpad and cout * taps * cin must be below 2^31");
  AF_REQUIRE(B <= 65535, "af_modulate_weights: at most 65535 samples");
  AF_REQUIRE(aligned16(w) && aligned16(wsq) && aligned16(styles) && aligned16(out), "af_modulate_weights: pointers must be 16-byte aligned");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(modulate_weights_kernel, dim3((unsigned)cout, (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const float*)w,
                     (const float*)wsq, (const float*)styles, (half_t*)out, cout, cin, taps, npad, kpad, demod, gain);
  return af_check_launch("af_modulate_weights");
}

extern "C" int af_style_epilogue(const void* y, const void* noise, const void* bias, const void* scale, const void* shift, void* out, int B,
                                 int HW, int C, float nw, void* stream) {
  AF_REQUIRE(y && out, "af_style_epilogue: y and out must not be NULL");
  AF_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 8 == 0, "af_style_epilogue: B and HW must be positive, C a positive multiple of 8");
  AF_REQUIRE(noise || nw == 0.f, "af_style_epilogue: a noise weight needs the noise map");
  AF_REQUIRE((scale == nullptr) == (shift == nullptr), "af_style_epilogue: scale and shift go together");
  AF_REQUIRE(!scale || C % 16 == 0, "af_style_epilogue: the SFT half needs C to be a multiple of 16");
  AF_REQUIRE((long)B * HW * C < LIM, "af_style_epilogue: B * HW * C must be below 2^31");
  AF_REQUIRE(aligned16(y) && aligned16(out) && aligned16(scale) && aligned16(shift) && (reinterpret_cast<uintptr_t>(noise) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(bias) & 3) == 0,
             "af_style_epilogue: y, out, scale and shift must be 16-byte aligned (noise and bias 4-byte)");
  const long n8 = (long)B * HW * (C / 8);
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(style_epilogue_kernel, g1(n8), dim3(256), 0, (hipStream_t)stream, (const half_t*)y, (const float*)noise, (const float*)bias,
                     (const half_t*)scale, (const half_t*)shift, (half_t*)out, HW, C / 8, nw, n8);
  return af_check_launch("af_style_epilogue");
}

extern "C" int af_bilinear_up2(const void* x, const void* addend, void* out, int B, int H, int W, int C, void* stream) {
  AF_REQUIRE(x && out, "af_bilinear_up2: x and out must not be NULL");
  AF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "af_bilinear_up2: B, H and W must be positive, C a positive multiple of 8");
  const long n = 4L * B * H * W * C;
  AF_REQUIRE(n < LIM, "af_bilinear_up2: B * 2H * 2W * C must be below 2^31");
  AF_REQUIRE(aligned16(x) && aligned16(addend) && aligned16(out), "af_bilinear_up2: pointers must be 16-byte aligned");
  {
    const char* xb = (const char*)x;
    const char* ob = (const char*)out;
    AF_REQUIRE(xb + n / 2 <= ob || ob + 2 * n <= xb, "af_bilinear_up2: out overlaps x");
  }
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(bilinear_up2_kernel, g1(n / 8), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (const half_t*)addend, (half_t*)out, H, W,
                     C / 8, n / 8);
  return af_check_launch("af_bilinear_up2");
}

extern "C" int af_face_paste_affine_u8(const void* photo_u8, const void* crops, const void* mats, void* out_u8, int H, int W, int F, int S, int ld,
                                       float erode, float feather, void* stream) {
  AF_REQUIRE(photo_u8 && out_u8, "af_face_paste_affine_u8: photo and out must not be NULL");
  AF_REQUIRE(H > 0 && W > 0 && (long)H * W * 3 < LIM, "af_face_paste_affine_u8: H and W must be positive and H * W * 3 below 2^31");
  AF_REQUIRE(F >= 0 && F <= 16, "af_face_paste_affine_u8: F must be from 0 to 16");
  AF_REQUIRE(F == 0 || (crops && mats), "af_face_paste_affine_u8: crops and mats must not be NULL when F > 0");
  AF_REQUIRE(F == 0 || (S >= 2 && ld >= 3), "af_face_paste_affine_u8: S must be at least 2 and ld at least 3");
  AF_REQUIRE(F == 0 || (long)F * S * S * ld < LIM, "af_face_paste_affine_u8: F * S * S * ld must be below 2^31");
  AF_REQUIRE(erode >= 0.f && feather >= 0.f, "af_face_paste_affine_u8: erode and feather must be non-negative (and not NaN)");
  AF_REQUIRE((reinterpret_cast<uintptr_t>(crops) & 1) == 0 && (reinterpret_cast<uintptr_t>(mats) & 3) == 0,
             "af_face_paste_affine_u8: crops must be 2-byte and mats 4-byte aligned");
  {
    const char* pb = (const char*)photo_u8;
    const char* ob = (const char*)out_u8;
    const long n = (long)H * W * 3;
    AF_REQUIRE(pb == ob || pb + n <= ob || ob + n <= pb, "af_face_paste_affine_u8: out overlaps the photo without being it");
  }
  const int npix = H * W;
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(face_paste_affine_u8_kernel, g1(npix), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)photo_u8,
                     (const half_t*)crops, (const float*)mats, (unsigned char*)out_u8, W, F, S, ld, erode, feather, npix);
  return af_check_launch("af_face_paste_affine_u8");
}
