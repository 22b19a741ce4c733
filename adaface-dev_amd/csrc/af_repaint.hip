// af_repaint.hip -- the pixel-space ends of "repaint the faces of a photo" (adaface/face_repaint.py, AdaFaceWrapper's inpaint pipeline with
// mask_image="face" / crop_padding): everything between the photo and the VAE that is not the VAE.
//   af_face_alpha_mask   ellipses fp32 [F, 4] -> soft mask alpha fp32 [H, W] (smoothstep feather, max over the faces)
//   af_crop_resize_u8    photo uint8 [H, W, 3] + alpha, rectangle -> image uint8 [1, Hs, Ws, 3] (antialiased bilinear) and the latent mask
//                        fp32 [1, 1, Hs/8, Ws/8] (8 x 8 block maximum of the resampled alpha >= thr), one launch
//   af_paste_back_u8     decoded fp32 [B, 3, Hs, Ws] resampled to the rectangle, blended into the photo under alpha, uint8 [B, H, W, 3], one launch
// All three are bandwidth-bound: plain vector loads and stores, four pixels of one row per lane.  An RGB row is 3 W bytes, so a group of four
// pixels is 12 bytes at a 4-byte aligned offset exactly when W % 4 == 0 (and the base is aligned): then it moves as three dwords next to one
// 16-byte access of alpha (the "wide" form); any other width runs the same code with byte and dword accesses (the "scalar" form).
//
// The resampling rule (torch's F.interpolate(mode="bilinear", antialias=True, align_corners=False), separable, n_in -> n_out per axis):
//   s = n_in / n_out, sup = max(s, 1), c = s (i + 0.5), taps k in [max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))),
//   weight max(0, 1 - |(k - c + 0.5) / sup|) normalised by its sum over the taps.
// With D = 2 max(n_in, n_out) every quantity is an integer over 2 n_out: (k - c + 0.5) / sup = (2 n_out k + n_out - n_in (2 i + 1)) / D, so the tap
// range comes from integer divisions, the un-normalised weight is m_k / D with the INTEGER m_k = max(0, D - |2 n_out k + n_out - n_in (2 i + 1)|),
// and the normalised weight is m_k / sum(m): one correctly rounded fp32 division of two exact integers (below 2^24).  At s = 1 the taps are
// (i, weight 1) and (i + 1, weight 0 exactly), so the resample is the identity bit for bit.  The tap count is a run-time quantity.
// Sums run along x first, then y, as torch's two passes do; no fused contraction (the blend's alpha = 0 / alpha = 1 cases are exact as written).
#include "af_common.h"

#pragma clang fp contract(off)

namespace {

struct Axis {
  int lo, hi;          // taps [lo, hi)
  long num, step, D;   // m_k = max(0, D - |num + step (k - lo)|)
  float M;             // sum of m_k (exact while below 2^24)
};

__device__ __forceinline__ Axis make_axis(int n_in, int n_out, int i) {
  Axis a;
  a.step = 2L * n_out;
  a.D = 2L * max(n_in, n_out);
  const long cnum = (long)n_in * (2 * i + 1);                 // c = cnum / step
  const long lo_num = cnum - a.D + n_out;                     // (c - sup + 0.5) step
  a.lo = lo_num > 0 ? (int)(lo_num / a.step) : 0;
  a.hi = min((long)n_in, (cnum + a.D + n_out) / a.step);
  a.num = a.step * a.lo + n_out - cnum;                       // (lo - c + 0.5) step
  long M = 0, num = a.num;
  for (int k = a.lo; k < a.hi; ++k, num += a.step) M += max(0L, a.D - labs(num));
  a.M = (float)M;                                             // > 0: the tap nearest c - 0.5 is inside and has |.| <= step / 2 < D
  return a;
}
__device__ __forceinline__ float axis_weight(const Axis& a, long num) { return (float)max(0L, a.D - labs(num)) / a.M; }

struct __attribute__((packed, aligned(4))) Px4 {
  unsigned int w[3];
};

// four pixels (12 bytes) of an RGB row: three dwords in the wide form, n * 3 single bytes otherwise
template <bool WIDE>
__device__ __forceinline__ void load_px4(const unsigned char* p, int n, unsigned char (&v)[12]) {
  if (WIDE) {
    const Px4 q = *reinterpret_cast<const Px4*>(p);
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = (unsigned char)(q.w[e >> 2] >> (8 * (e & 3)));
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = e < 3 * n ? p[e] : (unsigned char)0;
  }
}
template <bool WIDE>
__device__ __forceinline__ void store_px4(unsigned char* p, int n, const unsigned char (&v)[12]) {
  if (WIDE) {
    Px4 q;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      q.w[d] = (unsigned)v[4 * d] | ((unsigned)v[4 * d + 1] << 8) | ((unsigned)v[4 * d + 2] << 16) | ((unsigned)v[4 * d + 3] << 24);
    *reinterpret_cast<Px4*>(p) = q;
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e)
      if (e < 3 * n) p[e] = v[e];
  }
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }   // NaN -> lo

// ---- af_face_alpha_mask: one lane per four pixels of a row --------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void face_alpha_mask_kernel(const float* __restrict__ ell, float* __restrict__ alpha, int F, int H, int W,
                                                              int gw, int ngroups, float feather) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;
  const int y = g / gw, x = (g - y * gw) * 4;
  const int n = min(4, W - x);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  const float py = (float)y + 0.5f;
  for (int f = 0; f < F; ++f) {
    const float cx = ell[4 * f], cy = ell[4 * f + 1], rx = ell[4 * f + 2], ry = ell[4 * f + 3];
    const float v = (py - cy) / ry, v2 = v * v;
    // |v| > 1 gives r >= |v| > 1 in fp32 too (rounding is monotonic), hence a_f = 0 exactly; u grows with x when rx > 0, so the same holds for
    // a group wholly to one side of the ellipse.  Most rows of a large photo skip every face here.
    if (fabsf(v) > 1.f) continue;
    if (rx > 0.f && (((float)x + 0.5f - cx) / rx > 1.f || ((float)(x + 3) + 0.5f - cx) / rx < -1.f)) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float u = ((float)(x + j) + 0.5f - cx) / rx;
      const float r = sqrtf(u * u + v2);
      float af;
      if (feather > 0.f) {
        const float t = clampf((1.f - r) / feather, 0.f, 1.f);
        af = t * t * (3.f - 2.f * t);
      } else {
        af = r <= 1.f ? 1.f : 0.f;
      }
      a[j] = fmaxf(a[j], af);
    }
  }
  float* o = alpha + y * W + x;                    // H * W < 2^31 / 3 (checked by the caller)
  if (WIDE) {
    *reinterpret_cast<floatx4*>(o) = floatx4{a[0], a[1], a[2], a[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) o[j] = a[j];
  }
}

// ---- af_crop_resize_u8: one wave per 8 rows x 32 columns of the output (four latent cells), one lane per four pixels of a row --------------
// lane = row * 8 + group; the cell of a lane is group >> 1, so a cell's 64 pixels sit in the 16 lanes that differ in lane bits 0, 3, 4, 5.
__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const unsigned char* __restrict__ photo, const float* __restrict__ alpha,
                                                             unsigned char* __restrict__ image, float* __restrict__ mask_lat, int W, int x0,
                                                             int y0, int cw, int ch, int Hs, int Ws, float thr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int oy = (blockIdx.y * 4 + wave) * 8 + (lane >> 3);
  const int ox = blockIdx.x * 32 + (lane & 7) * 4;
  const bool live = oy < Hs && ox < Ws;           // Ws % 8 == 0: a group of four is inside or outside as a whole
  float amax = -3.4028235e38f;
  if (live) {
    const Axis ay = make_axis(ch, Hs, oy);
    unsigned char o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const Axis ax = make_axis(cw, Ws, ox + j);
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      long ny = ay.num;
      for (int ky = ay.lo; ky < ay.hi; ++ky, ny += ay.step) {
        const float wy = axis_weight(ay, ny);
        const int row = (y0 + ky) * W + x0;        // taps stay inside the rectangle, the rectangle inside the photo
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        long nx = ax.num;
        for (int kx = ax.lo; kx < ax.hi; ++kx, nx += ax.step) {
          const float wx = axis_weight(ax, nx);
          const unsigned char* p = photo + (row + kx) * 3;
          r[0] += wx * (float)p[0];
          r[1] += wx * (float)p[1];
          r[2] += wx * (float)p[2];
          r[3] += wx * alpha[row + kx];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += wy * r[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * j + c] = (unsigned char)rintf(clampf(acc[c], 0.f, 255.f));
      amax = fmaxf(amax, acc[3]);
    }
    store_px4<true>(image + (oy * Ws + ox) * 3, 4, o);
  }
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 8, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
  if (live && (lane & 0x39) == 0) mask_lat[(oy >> 3) * (Ws >> 3) + (ox >> 3)] = amax >= thr ? 1.f : 0.f;
}

// ---- af_paste_back_u8: one lane per four pixels of a photo row, all B outputs ----------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void paste_back_u8_kernel(const float* __restrict__ dec, const unsigned char* __restrict__ photo,
                                                            const float* __restrict__ alpha, unsigned char* __restrict__ out, int B, int Hs,
                                                            int Ws, int H, int W, int x0, int y0, int cw, int ch, int gw, int ngroups) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;
  const int y = g / gw, x = (g - y * gw) * 4;
  const int n = min(4, W - x);
  const int pix = y * W + x;
  unsigned char p[12];
  load_px4<WIDE>(photo + pix * 3, n, p);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  bool any = false;
  if (y >= y0 && y < y0 + ch && x + 4 > x0 && x < x0 + cw) {
    if (WIDE) {
      const floatx4 q = *reinterpret_cast<const floatx4*>(alpha + pix);
      a[0] = q[0], a[1] = q[1], a[2] = q[2], a[3] = q[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) a[j] = alpha[pix + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= n || x + j < x0 || x + j >= x0 + cw) a[j] = 0.f;       // outside the rectangle: the photo
      any = any || a[j] != 0.f;
    }
  }
  const int img = H * W * 3, plane = Hs * Ws;      // B * H * W * 3 and B * 3 * Hs * Ws < 2^31 (checked by the caller)
  if (!any) {
    for (int b = 0; b < B; ++b) store_px4<WIDE>(out + b * img + pix * 3, n, p);
    return;
  }
  const Axis ay = make_axis(Hs, ch, y - y0);
  for (int b = 0; b < B; ++b) {
    unsigned char o[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) o[e] = p[e];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (a[j] == 0.f) continue;
      const Axis ax = make_axis(Ws, cw, x + j - x0);
      float acc[3] = {0.f, 0.f, 0.f};
      long ny = ay.num;
      for (int ky = ay.lo; ky < ay.hi; ++ky, ny += ay.step) {
        const float wy = axis_weight(ay, ny);
        const float* d = dec + b * 3 * plane + ky * Ws;
        float r[3] = {0.f, 0.f, 0.f};
        long nx = ax.num;
        for (int kx = ax.lo; kx < ax.hi; ++kx, nx += ax.step) {
          const float wx = axis_weight(ax, nx);
          r[0] += wx * d[kx];
          r[1] += wx * d[plane + kx];
          r[2] += wx * d[2 * plane + kx];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wy * r[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float gv = 255.f * clampf(acc[c] / 2.f + 0.5f, 0.f, 1.f);
        const float v = a[j] * gv + (1.f - a[j]) * (float)p[3 * j + c];
        o[3 * j + c] = (unsigned char)rintf(clampf(v, 0.f, 255.f));
      }
    }
    store_px4<WIDE>(out + b * img + pix * 3, n, o);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool rect_inside(int x0, int y0, int cw, int ch, int H, int W) {
  return x0 >= 0 && y0 >= 0 && cw >= 1 && ch >= 1 && (long)x0 + cw <= W && (long)y0 + ch <= H;
}
constexpr long LIM = 1L << 31;

}  // namespace

extern "C" int af_face_alpha_mask(const void* ellipses, void* alpha, int F, int H, int W, float feather, void* stream) {
  AF_REQUIRE(alpha && H > 0 && W > 0 && F >= 0 && (ellipses || F == 0), "af_face_alpha_mask: bad argument");
  AF_REQUIRE(feather >= 0.f && feather <= 3.0e38f, "af_face_alpha_mask: feather must be finite and >= 0");
  AF_REQUIRE((long)H * W * 3 < LIM, "af_face_alpha_mask: the photo needs fewer than 2^31 bytes (H * W * 3)");
  AF_REQUIRE(aligned(alpha, 4) && aligned(ellipses, 4), "af_face_alpha_mask: fp32 tensors must be 4-byte aligned");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const int gw = (W + 3) / 4, ng = H * gw;
  const dim3 grid((unsigned)((ng + 255) / 256));
  if (W % 4 == 0 && aligned(alpha, 16))
    hipLaunchKernelGGL(face_alpha_mask_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)ellipses, (float*)alpha, F, H, W,
                       gw, ng, feather);
  else
    hipLaunchKernelGGL(face_alpha_mask_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)ellipses, (float*)alpha, F, H, W,
                       gw, ng, feather);
  return af_check_launch("af_face_alpha_mask");
}

extern "C" int af_crop_resize_u8(const void* photo_u8, const void* alpha, void* image_u8, void* mask_lat, int H, int W, int x0, int y0, int cw,
                                 int ch, int Hs, int Ws, float thr, void* stream) {
  AF_REQUIRE(photo_u8 && alpha && image_u8 && mask_lat && H > 0 && W > 0, "af_crop_resize_u8: bad argument");
  AF_REQUIRE((long)H * W * 3 < LIM, "af_crop_resize_u8: the photo needs fewer than 2^31 bytes (H * W * 3)");
  AF_REQUIRE(rect_inside(x0, y0, cw, ch, H, W), "af_crop_resize_u8: the rectangle must be non-empty and inside the photo");
  AF_REQUIRE(Hs > 0 && Ws > 0 && Hs % 8 == 0 && Ws % 8 == 0, "af_crop_resize_u8: the working size must be positive multiples of 8");
  AF_REQUIRE((long)Hs * Ws * 3 < LIM, "af_crop_resize_u8: the working image needs fewer than 2^31 bytes (Hs * Ws * 3)");
  AF_REQUIRE(aligned(image_u8, 4) && aligned(alpha, 4) && aligned(mask_lat, 4), "af_crop_resize_u8: image, alpha and mask_lat must be 4-byte aligned");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)((Ws + 31) / 32), (unsigned)((Hs / 8 + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)photo_u8, (const float*)alpha, (unsigned char*)image_u8, (float*)mask_lat, W, x0, y0, cw, ch, Hs, Ws,
                     thr);
  return af_check_launch("af_crop_resize_u8");
}

extern "C" int af_paste_back_u8(const void* decoded, const void* photo_u8, const void* alpha, void* out_u8, int B, int Hs, int Ws, int H, int W,
                                int x0, int y0, int cw, int ch, void* stream) {
  AF_REQUIRE(decoded && photo_u8 && alpha && out_u8 && B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "af_paste_back_u8: bad argument");
  AF_REQUIRE((long)H * W * 3 < LIM && (long)B * H * W * 3 < LIM, "af_paste_back_u8: the output needs fewer than 2^31 bytes (B * H * W * 3)");
  AF_REQUIRE((long)B * 3 * Hs * Ws < LIM, "af_paste_back_u8: decoded needs fewer than 2^31 elements (B * 3 * Hs * Ws)");
  AF_REQUIRE(rect_inside(x0, y0, cw, ch, H, W), "af_paste_back_u8: the rectangle must be non-empty and inside the photo");
  AF_REQUIRE(aligned(decoded, 4) && aligned(alpha, 4), "af_paste_back_u8: fp32 tensors must be 4-byte aligned");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const int gw = (W + 3) / 4, ng = H * gw;
  const dim3 grid((unsigned)((ng + 255) / 256));
  if (W % 4 == 0 && aligned(photo_u8, 4) && aligned(out_u8, 4) && aligned(alpha, 16))
    hipLaunchKernelGGL(paste_back_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)decoded,
                       (const unsigned char*)photo_u8, (const float*)alpha, (unsigned char*)out_u8, B, Hs, Ws, H, W, x0, y0, cw, ch, gw, ng);
  else
    hipLaunchKernelGGL(paste_back_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)decoded,
                       (const unsigned char*)photo_u8, (const float*)alpha, (unsigned char*)out_u8, B, Hs, Ws, H, W, x0, y0, cw, ch, gw, ng);
  return af_check_launch("af_paste_back_u8");
}
