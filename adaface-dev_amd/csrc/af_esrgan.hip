// af_esrgan.hip -- the two kernels of the Real-ESRGAN upscaler (adaface/esrgan.py, RRDBNet).
//   af_dense_conv3x3     3x3 convolution (pad 1) of the first `cin` channels of a strided NHWC buffer into a narrow channel slice of the same or
//                        another buffer: bias, LeakyReLU and two scaled residuals in the epilogue, optional nearest-x2 upsample of the input
//                        (never materialised), optional uint8 output.  A dense block's concatenation is then a buffer layout, not a copy.
//   af_u8_unshuffle_f16  uint8 RGB image -> fp16 NHWC in [0, 1], pixel-unshuffled by r in {1, 2, 4}, channels zero-padded to cpad.
//
// af_dense_conv3x3 runs on the patch frame of af_conv3x3_patch.h at stride 1: a workgroup owns a 16 x 16 patch of output pixels of one image
// and all cout channels.  This file has what is the dense kernel's own.  Its source of halo pixels is a strided NHWC buffer with bounds on the
// OUTPUT grid: under `upsample` the halo is filled at output resolution from source pixel (y >> 1, x >> 1) and the compute loop is the same.
// Its weights are [npad][9 cin] halves (at most 64 x 1728).  Its epilogue takes the last fragment partly filled and writes fp16 or uint8.
#include "af_conv3x3_patch.h"

namespace {

struct DenseArgs {
  const half_t* x;
  const half_t* wt;
  const float* bias;
  void* out;
  const half_t* r1;
  const half_t* r2;
  int ldx, cin, ldo, cout, ldr1, ldr2;
  float alpha, beta, slope;
  int upsample, out_mode, H, W, Ho, Wo;

  // the frame's Src: element offset of the piece in x
  __device__ int locate(int b, int y, int x_, int q) const {
    const bool in = y >= 0 && y < Ho && x_ >= 0 && x_ < Wo;
    const int sy = upsample ? y >> 1 : y, sx = upsample ? x_ >> 1 : x_;
    return in ? ((b * H + sy) * W + sx) * ldx + q * 8 : -1;
  }
  __device__ uintx4_t fetch(int h, int c0, int) const { return *reinterpret_cast<const uintx4_t*>(x + h + c0); }
};

template <int NT>
__global__ __launch_bounds__(256) void dense_conv3x3_kernel(const DenseArgs a) {
  const int b = blockIdx.z;
  conv3x3_patch<1, NT>(a, b, a.wt, 9 * a.cin, a.cin, a.cin, a.Ho, a.Wo, [=](const floatx4& acc, int y, int x, int nt, int c4) {
    const int m = (b * a.Ho + y) * a.Wo + x;
    const int n0 = nt * 16 + c4;
    if (n0 >= a.cout) return;
    const bool full = n0 + 4 <= a.cout;
    const float slope = a.slope > 0.f ? a.slope : 1.f;   // no activation = slope 1: y * 1 is y, and the test stays out of the lanes' selects
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float y32 = acc[r];
      if (a.bias && n0 + r < a.cout) y32 += a.bias[n0 + r];
      v[r] = y32 >= 0.f ? y32 : slope * y32;
    }
    if (a.r1) {
      const half_t* p = a.r1 + m * a.ldr1 + n0;
      if (full) {
        const half4_t h = *reinterpret_cast<const half4_t*>(p);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = a.alpha * v[r] + (float)h[r];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < a.cout) v[r] = a.alpha * v[r] + (float)p[r];
      }
    }
    if (a.r2) {
      const half_t* p = a.r2 + m * a.ldr2 + n0;
      if (full) {
        const half4_t h = *reinterpret_cast<const half4_t*>(p);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = a.beta * v[r] + (float)h[r];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < a.cout) v[r] = a.beta * v[r] + (float)p[r];
      }
    }
    if (a.out_mode == 0) {
      half_t* o = (half_t*)a.out + m * a.ldo + n0;
      if (full) {
        *reinterpret_cast<half4_t*>(o) = half4_t{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < a.cout) o[r] = (half_t)v[r];
      }
    } else {
      unsigned char* o = (unsigned char*)a.out + m * a.cout + n0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < a.cout) o[r] = (unsigned char)rintf(255.f * fminf(fmaxf(v[r], 0.f), 1.f));
    }
  });
}

// one lane per 8 output channels (16 bytes) of one output pixel
__global__ __launch_bounds__(256) void u8_unshuffle_f16_kernel(const unsigned char* __restrict__ img, half_t* __restrict__ out, int H, int W, int r,
                                                              int cpad, int total) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int per = cpad >> 3;
  const int pix = g / per, c8 = (g - pix * per) * 8;
  const int Wr = W / r, Hr = H / r;
  const int j = pix % Wr, t = pix / Wr, i = t % Hr, b = t / Hr;
  const int rr = r * r;
  half8_t v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ch = c8 + e;
    float f = 0.f;
    if (ch < 3 * rr) {
      const int c = ch / rr, rem = ch - c * rr, dy = rem / r, dx = rem - dy * r;
      f = (float)img[((b * H + i * r + dy) * W + j * r + dx) * 3 + c] / 255.f;
    }
    v[e] = (half_t)f;
  }
  *reinterpret_cast<half8_t*>(out + pix * cpad + c8) = v;
}

// A residual against out: byte ranges apart, or exactly the out elements, or other channels of the same rows (same row stride).  Anything else
// would have one workgroup read what another writes.
inline bool residual_ok(const void* r, int ldr, const void* out, int ldo, int cout, long Mo, int out_mode) {
  if (!r) return true;
  const char* rb = (const char*)r;
  const char* re = rb + 2 * (Mo - 1) * ldr + 2 * (long)cout;
  const char* ob = (const char*)out;
  const char* oe = ob + (out_mode == 0 ? 2 * (Mo - 1) * ldo + 2 * (long)cout : Mo * cout);
  if (re <= ob || oe <= rb) return true;
  if (out_mode != 0 || ldr != ldo || (rb - ob) % 2 != 0) return false;
  const long d = (rb - ob) / 2;
  if (d == 0) return true;
  const long c = ((d % ldo) + ldo) % ldo;
  return c >= cout && c + cout <= ldo;
}

}  // namespace

extern "C" int af_dense_conv3x3(const void* x, int ldx, int cin, const void* wt, const void* bias, void* out, int ldo, int cout, const void* r1,
                                int ldr1, float alpha, const void* r2, int ldr2, float beta, float slope, int upsample, int out_mode, int B, int H,
                                int W, void* stream) {
  AF_REQUIRE(x && wt && out, "af_dense_conv3x3: x, wt and out must not be NULL");
  AF_REQUIRE(B > 0 && H > 0 && W > 0, "af_dense_conv3x3: B, H and W must be positive");
  AF_REQUIRE(cin % 32 == 0 && cin >= 32 && cin <= 192, "af_dense_conv3x3: cin must be a multiple of 32 from 32 to 192");
  AF_REQUIRE(cout >= 1 && cout <= 64, "af_dense_conv3x3: cout must be from 1 to 64");
  AF_REQUIRE(ldx >= cin && ldx % 8 == 0, "af_dense_conv3x3: ldx must be a multiple of 8 and at least cin");
  AF_REQUIRE((upsample == 0 || upsample == 1) && (out_mode == 0 || out_mode == 1), "af_dense_conv3x3: upsample and out_mode must be 0 or 1");
  AF_REQUIRE(out_mode == 1 || (ldo >= cout && ldo % 8 == 0), "af_dense_conv3x3: ldo must be a multiple of 8 and at least cout");
  AF_REQUIRE(r1 || !r2, "af_dense_conv3x3: r2 needs r1");
  AF_REQUIRE(!r1 || (ldr1 >= cout && ldr1 % 8 == 0), "af_dense_conv3x3: ldr1 must be a multiple of 8 and at least cout");
  AF_REQUIRE(!r2 || (ldr2 >= cout && ldr2 % 8 == 0), "af_dense_conv3x3: ldr2 must be a multiple of 8 and at least cout");
  AF_REQUIRE(aligned(x, 16) && aligned(wt, 16) && aligned(r1, 16) && aligned(r2, 16) && aligned(bias, 4) && (out_mode == 1 || aligned(out, 16)),
             "af_dense_conv3x3: x, wt, out, r1 and r2 must be 16-byte aligned (bias 4-byte)");
  const long up = upsample ? 2 : 1;
  const long Ho = up * H, Wo = up * W, Mo = (long)B * Ho * Wo;
  long ldmax = cout;
  if (out_mode == 0 && ldo > ldmax) ldmax = ldo;
  if (r1 && ldr1 > ldmax) ldmax = ldr1;
  if (r2 && ldr2 > ldmax) ldmax = ldr2;
  AF_REQUIRE((long)B * H * W * ldx < LIM && Mo * ldmax < LIM,
             "af_dense_conv3x3: B*H*W*ldx and B*Ho*Wo*max(ldo, ldr1, ldr2, cout) must be below 2^31 (32-bit offsets): split the batch");
  {
    // out against the channels [0, cin) the call reads.  Disjoint byte ranges are fine; otherwise out must sit in x's own rows (same stride, same
    // grid) on channels [c0, c0 + cout) with c0 >= cin.
    const char* xb = (const char*)x;
    const char* xe = xb + 2 * ((long)B * H * W - 1) * ldx + 2 * (long)cin;
    const char* ob = (const char*)out;
    const char* oe = ob + (out_mode == 0 ? 2 * (Mo - 1) * ldo + 2 * (long)cout : Mo * cout);
    if (ob < xe && xb < oe) {
      bool ok = out_mode == 0 && upsample == 0 && ldo == ldx && (ob - xb) % 2 == 0;
      if (ok) {
        const long d = (ob - xb) / 2;
        const long c0 = ((d % ldx) + ldx) % ldx;
        ok = c0 >= cin && c0 + cout <= ldx;
      }
      AF_REQUIRE(ok, "af_dense_conv3x3: out overlaps the input channels [0, cin) of x");
    }
  }
  AF_REQUIRE(residual_ok(r1, ldr1, out, ldo, cout, Mo, out_mode), "af_dense_conv3x3: r1 overlaps out without being exactly its elements");
  AF_REQUIRE(residual_ok(r2, ldr2, out, ldo, cout, Mo, out_mode), "af_dense_conv3x3: r2 overlaps out without being exactly its elements");
  DenseArgs a;
  a.x = (const half_t*)x, a.wt = (const half_t*)wt, a.bias = (const float*)bias, a.out = out;
  a.r1 = (const half_t*)r1, a.r2 = (const half_t*)r2;
  a.ldx = ldx, a.cin = cin, a.ldo = ldo, a.cout = cout, a.ldr1 = ldr1, a.ldr2 = ldr2;
  a.alpha = alpha, a.beta = beta, a.slope = slope;
  a.upsample = upsample, a.out_mode = out_mode, a.H = H, a.W = W, a.Ho = (int)Ho, a.Wo = (int)Wo;
  const dim3 grid((unsigned)((Wo + 15) / 16), (unsigned)((Ho + 15) / 16), (unsigned)B);
  AF_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "af_dense_conv3x3: more than 65535 patch rows or images");
  AfLaunchScope scope(AF_FAM_GEMM, stream);
  switch ((cout + 15) / 16) {
    case 1: hipLaunchKernelGGL(dense_conv3x3_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(dense_conv3x3_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(dense_conv3x3_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(dense_conv3x3_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
  }
  return af_check_launch("af_dense_conv3x3");
}

extern "C" int af_u8_unshuffle_f16(const void* img_u8, void* out, int B, int H, int W, int r, int cpad, void* stream) {
  AF_REQUIRE(img_u8 && out && B > 0 && H > 0 && W > 0, "af_u8_unshuffle_f16: bad argument");
  AF_REQUIRE(r == 1 || r == 2 || r == 4, "af_u8_unshuffle_f16: r must be 1, 2 or 4");
  AF_REQUIRE(H % r == 0 && W % r == 0, "af_u8_unshuffle_f16: H and W must be multiples of r");
  AF_REQUIRE((cpad == 32 || cpad == 64) && cpad >= 3 * r * r, "af_u8_unshuffle_f16: cpad must be 32 or 64 and at least 3 r^2");
  AF_REQUIRE(aligned(out, 16), "af_u8_unshuffle_f16: out must be 16-byte aligned");
  AF_REQUIRE((long)B * H * W * 3 < LIM && (long)B * (H / r) * (W / r) * cpad < LIM,
             "af_u8_unshuffle_f16: the image and the output need fewer than 2^31 elements: split the batch");
  const int total = B * (H / r) * (W / r) * (cpad / 8);
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(u8_unshuffle_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)img_u8, (half_t*)out, H, W, r, cpad, total);
  return af_check_launch("af_u8_unshuffle_f16");
}
