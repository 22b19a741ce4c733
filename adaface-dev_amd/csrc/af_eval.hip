// af_eval.hip -- the kernels of the image-scoring encoders (evaluation/vit.py: CLIP ViT-B/32, ViT-L/14 and DINO ViT-S/16):
//   af_vit_patch_rows   uint8 images [B, H, W, 3] -> the fp16 rows [B (C/p)^2][kpad] the patch-embedding GEMM reads: antialiased resize
//                       (triangle or cubic), centre crop, per-channel affine, unfold and zero padding in one launch
//   af_gelu_f16         y = x * 0.5 * (1 + erf(x / sqrt 2)), fp16 (DINO's MLP)
// af_vit_patch_rows is the only part of an evaluator that touches every input pixel.  One workgroup (256 lanes) per patch.  The source footprint
// of a patch is walked in chunks of rows, so its size in LDS does not depend on the resize ratio:
//   stage    the chunk's rows, only the columns the patch reads, as raw bytes into LDS with aligned dword loads (each input byte is loaded once
//            per patch instead of once per tap; skipped when the image base is not 4-byte aligned or one footprint row does not fit: then the
//            next pass reads global memory directly)
//   x pass   one lane per (source row, output column): the weighted sum over the column taps of the three channels -> fp32 in LDS
//   y pass   one lane per (output row, output column), up to four of them: the partial sums over the chunk's rows stay in registers
// Tap ranges and the first tap's offset are formed in fp64, the filter in fp32; each pass divides by the sum of its weights at the end.  The
// un-normalised weights of the patch's p columns and p rows are evaluated once into LDS when such a table fits (4 KB per axis) and where they are
// used otherwise, so nothing whose size depends on the ratio has to fit.  The finished row is assembled in LDS and leaves as 16-byte stores, pad
// columns included.  Measured and what bounds it: profiles/eval_encoders.txt, DESIGN.md 4.22.
#include "af_common.h"

namespace {

constexpr int VP_RAW_BYTES = 16384;    // LDS for the staged source bytes of one chunk (reused for the finished fp16 row: 3 * 32 * 32 + 8 halves)
constexpr int VP_H_FLOATS = 4096;      // LDS for the x pass' output of one chunk: rows * p * 3 floats (at least 42 rows at p = 32)
constexpr int VP_W_FLOATS = 1024;      // LDS per axis for the patch's filter weights: p * (taps per output index)
constexpr int VP_MAX_P = 32;
constexpr int VP_PAIRS = VP_MAX_P * VP_MAX_P / 256;

template <int FILTER>
__device__ __forceinline__ float vp_filter(float x) {
  x = fabsf(x);
  if (FILTER == 0) return fmaxf(0.f, 1.f - x);
  const float a = -0.5f;
  if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
  if (x < 2.f) return a * (((x - 5.f) * x + 8.f) * x - 4.f);
  return 0.f;
}

struct VpAxis {
  double s, sup;       // n_in / n_out, filter width * max(s, 1)
  float inv_sc;        // 1 / max(s, 1)
  int n_in;
};
__device__ __forceinline__ VpAxis vp_axis(int n_in, int n_out, double width) {
  VpAxis a;
  a.s = (double)n_in / (double)n_out;
  const double sc = a.s > 1.0 ? a.s : 1.0;
  a.sup = width * sc;
  a.inv_sc = (float)(1.0 / sc);
  a.n_in = n_in;
  return a;
}
// taps [k0, k1) of output index i and cm = centre - 0.5: the filter argument of tap k is (k - cm) * inv_sc
__device__ __forceinline__ void vp_taps(const VpAxis& a, int i, int& k0, int& k1, double& cm) {
  const double c = a.s * ((double)i + 0.5);
  k0 = max(0, (int)(c - a.sup + 0.5));
  k1 = min(a.n_in, (int)(c + a.sup + 0.5));
  cm = c - 0.5;
}

// the x pass for one (source row, output column): sp = the first tap's pixel (LDS or global)
template <int FILTER, typename Ptr>
__device__ __forceinline__ void vp_row_sum(Ptr sp, int k0, int k1, double cm, float inv_sc, float* __restrict__ out3) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, ws = 0.f;
  const float x0 = (float)((double)k0 - cm);       // |x0| <= sup + 1: adding the tap count in fp32 moves the filter argument by 2^-23 of the width
  const int n = k1 - k0;
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const float w = vp_filter<FILTER>((x0 + (float)j) * inv_sc);
    ws += w;
    a0 += w * (float)sp[3 * j];
    a1 += w * (float)sp[3 * j + 1];
    a2 += w * (float)sp[3 * j + 2];
  }
  out3[0] = a0 / ws;
  out3[1] = a1 / ws;
  out3[2] = a2 / ws;
}
// the same with the n un-normalised weights read from the patch's table
template <typename Ptr>
__device__ __forceinline__ void vp_row_sum_tab(Ptr sp, int n, const float* __restrict__ wrow, float* __restrict__ out3) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, ws = 0.f;
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const float w = wrow[j];
    ws += w;
    a0 += w * (float)sp[3 * j];
    a1 += w * (float)sp[3 * j + 1];
    a2 += w * (float)sp[3 * j + 2];
  }
  out3[0] = a0 / ws;
  out3[1] = a1 / ws;
  out3[2] = a2 / ws;
}
// un-normalised weights of the p output indices i0 .. of one axis: tab[i * nt + j] = f of tap k0(i) + j, 0 behind the last tap
template <int FILTER>
__device__ __forceinline__ void vp_fill_table(const VpAxis& a, int i0, int p, int nt, float* __restrict__ tab, int t) {
  for (int idx = t; idx < p * nt; idx += 256) {
    const int i = idx / nt, j = idx - i * nt;
    int k0, k1;
    double cm;
    vp_taps(a, i0 + i, k0, k1, cm);
    tab[idx] = j < k1 - k0 ? vp_filter<FILTER>(((float)((double)k0 - cm) + (float)j) * a.inv_sc) : 0.f;
  }
}

struct VpArgs {
  int H, W, Hr, Wr, top, left, G, p, kpad, aligned4;
  long total_bytes;
  float scale[3], shift[3];
};

template <int FILTER>
__global__ __launch_bounds__(256) void vit_patch_rows_kernel(const unsigned char* __restrict__ img, half_t* __restrict__ rows, const VpArgs A) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[VP_RAW_BYTES];
  __shared__ __attribute__((aligned(16))) float hbuf[VP_H_FLOATS];
  const int t = threadIdx.x, p = A.p, H = A.H, W = A.W;
  const long patch = blockIdx.x;                       // b * G * G + py * G + px
  const int PP = A.G * A.G;
  const int b = (int)(patch / PP), rem = (int)(patch - (long)b * PP);
  const int py = rem / A.G, px = rem - py * A.G;
  const double width = FILTER ? 2.0 : 1.0;
  const VpAxis ax = vp_axis(W, A.Wr, width), ay = vp_axis(H, A.Hr, width);
  const int X0 = A.left + px * p, Y0 = A.top + py * p;     // the patch in the resized image
  int kx0, kx1, ry0, ry1, tmp;
  double cm;
  vp_taps(ax, X0, kx0, tmp, cm);
  vp_taps(ax, X0 + p - 1, tmp, kx1, cm);
  vp_taps(ay, Y0, ry0, tmp, cm);
  vp_taps(ay, Y0 + p - 1, tmp, ry1, cm);
  const int fwb = (kx1 - kx0) * 3;                         // bytes of one footprint row
  const int rs = (fwb + 3 + 3) / 4 * 4;                    // its LDS stride: up to 3 bytes in front of it in its first aligned dword
  const bool staged = A.aligned4 && rs <= VP_RAW_BYTES;
  int rc_max = VP_H_FLOATS / (3 * p);
  if (staged) rc_max = min(rc_max, VP_RAW_BYTES / rs);
  const long img0 = (long)b * H * W * 3;

  // this lane's outputs: pixels q = t + 256 i of the patch, three channels each
  float acc[VP_PAIRS][3], wsy[VP_PAIRS];
  int qk0[VP_PAIRS], qk1[VP_PAIRS];
  double qcm[VP_PAIRS];
#pragma unroll
  for (int i = 0; i < VP_PAIRS; ++i) {
    acc[i][0] = acc[i][1] = acc[i][2] = wsy[i] = 0.f;
    const int q = t + 256 * i;
    qk0[i] = qk1[i] = 0;
    qcm[i] = 0.0;
    if (q < p * p) vp_taps(ay, Y0 + q / p, qk0[i], qk1[i], qcm[i]);
  }

  // The weight of (output index, tap) does not depend on the other axis: evaluated once per patch into LDS when the table fits (cubic up to a
  // ratio of 7.5 at p = 32), where they are used otherwise.  No output index has more than floor(2 sup) + 2 taps.
  __shared__ float wx[VP_W_FLOATS], wy[VP_W_FLOATS];
  const int ntx = (int)(2.0 * ax.sup) + 2, nty = (int)(2.0 * ay.sup) + 2;
  const bool tabx = ax.sup < 1.0e6 && p * ntx <= VP_W_FLOATS, taby = ay.sup < 1.0e6 && p * nty <= VP_W_FLOATS;
  if (tabx) vp_fill_table<FILTER>(ax, X0, p, ntx, wx, t);
  if (taby) vp_fill_table<FILTER>(ay, Y0, p, nty, wy, t);
  __syncthreads();

  for (int r0 = ry0; r0 < ry1; r0 += rc_max) {
    const int rc = min(rc_max, ry1 - r0);
    if (staged) {
      const int ndw = rs / 4;
      for (int idx = t; idx < rc * ndw; idx += 256) {
        const int rr = idx / ndw, j = idx - rr * ndw;
        const long g0 = img0 + ((long)(r0 + rr) * W + kx0) * 3;          // first byte of this row's footprint
        const long ga = (g0 & ~3L) + 4L * j;
        if (ga < g0 + fwb) {
          unsigned v = 0;
          if (ga + 4 <= A.total_bytes) {
            v = *reinterpret_cast<const unsigned*>(img + ga);
          } else {                                                       // the tensor's last, partial dword
            for (int e = 0; e < 4; ++e)
              if (ga + e < A.total_bytes) v |= (unsigned)img[ga + e] << (8 * e);
          }
          reinterpret_cast<unsigned*>(raw)[rr * ndw + j] = v;
        }
      }
      __syncthreads();
    }
    for (int idx = t; idx < rc * p; idx += 256) {
      const int rr = idx / p, x = idx - rr * p;
      int k0, k1;
      vp_taps(ax, X0 + x, k0, k1, cm);
      const long g0 = img0 + ((long)(r0 + rr) * W + kx0) * 3;
      if (staged && tabx)
        vp_row_sum_tab(raw + rr * rs + (int)(g0 & 3L) + (k0 - kx0) * 3, k1 - k0, wx + x * ntx, hbuf + idx * 3);
      else if (staged)
        vp_row_sum<FILTER>(raw + rr * rs + (int)(g0 & 3L) + (k0 - kx0) * 3, k0, k1, cm, ax.inv_sc, hbuf + idx * 3);
      else if (tabx)
        vp_row_sum_tab(img + g0 + (long)(k0 - kx0) * 3, k1 - k0, wx + x * ntx, hbuf + idx * 3);
      else
        vp_row_sum<FILTER>(img + g0 + (long)(k0 - kx0) * 3, k0, k1, cm, ax.inv_sc, hbuf + idx * 3);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VP_PAIRS; ++i) {
      const int q = t + 256 * i;
      const int x = q % p;
      const int lo = max(qk0[i], r0), hi = min(qk1[i], r0 + rc);       // empty for q >= p * p
      const float y0 = (float)((double)qk0[i] - qcm[i]);
      const float* wrow = wy + (q < p * p ? q / p : 0) * nty - qk0[i];
#pragma unroll 4
      for (int r = lo; r < hi; ++r) {
        const float w = taby ? wrow[r] : vp_filter<FILTER>((y0 + (float)(r - qk0[i])) * ay.inv_sc);
        const float* hp = hbuf + ((r - r0) * p + x) * 3;
        wsy[i] += w;
        acc[i][0] += w * hp[0];
        acc[i][1] += w * hp[1];
        acc[i][2] += w * hp[2];
      }
    }
    __syncthreads();
  }

  // the finished row: column c p^2 + dy p + dx, zeros behind 3 p^2
  half_t* orow = reinterpret_cast<half_t*>(raw);
  const int k3 = 3 * p * p, k8 = (k3 + 7) / 8 * 8;
#pragma unroll
  for (int i = 0; i < VP_PAIRS; ++i) {
    const int q = t + 256 * i;
    if (q < p * p) {
#pragma unroll
      for (int c = 0; c < 3; ++c)      // one multiply, one add, unfused: at ratio 1 the result is fp16(v * scale + shift) bit for bit
        orow[c * p * p + q] = (half_t)__fadd_rn(__fmul_rn(acc[i][c] / wsy[i], A.scale[c]), A.shift[c]);
    }
  }
  if (t < k8 - k3) orow[k3 + t] = (half_t)0.f;
  __syncthreads();
  half_t* dst = rows + patch * A.kpad;
  const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = t; j < A.kpad / 8; j += 256)
    *reinterpret_cast<half8_t*>(dst + j * 8) = j < k8 / 8 ? *reinterpret_cast<const half8_t*>(orow + j * 8) : zero;
}

// eight elements per lane: one 16-byte access when both pointers are aligned and the eight are inside, element by element otherwise
__device__ __forceinline__ float gelu_erf_exact(float x) {
  // x Phi(x) through erfc: 1 + erf(y) would cancel for x < 0, where the result is still well inside fp16's range (x = -4: -1.3e-4)
  return 0.5f * x * erfcf(-x * 0.70710678118654752f);
}
__global__ __launch_bounds__(256) void gelu_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long n, int vec) {
  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  if (vec && i0 + 8 <= n) {
    const half8_t v = *reinterpret_cast<const half8_t*>(x + i0);
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)gelu_erf_exact((float)v[e]);
    *reinterpret_cast<half8_t*>(y + i0) = o;
  } else {
    for (long i = i0; i < n && i < i0 + 8; ++i) y[i] = (half_t)gelu_erf_exact((float)x[i]);
  }
}

inline long rne_half(long n) {         // n / 2 rounded half to even, n >= 0 (Python's round)
  const long k = n / 2;
  return (n & 1) ? k + (k & 1) : k;
}

}  // namespace

extern "C" int af_vit_patch_rows(const void* img_u8, void* rows, int B, int H, int W, int keep_aspect, int S, int C, int p, int filter,
                                 const float* scale3, const float* shift3, int kpad, void* stream) {
  AF_REQUIRE(img_u8 && rows && scale3 && shift3, "af_vit_patch_rows: NULL pointer");
  AF_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && p >= 1, "af_vit_patch_rows: B, H, W, C and p must be positive");
  AF_REQUIRE(C % p == 0, "af_vit_patch_rows: C must be a multiple of p");
  AF_REQUIRE(!keep_aspect || (S >= 1 && C <= S), "af_vit_patch_rows: with keep_aspect the crop C must not exceed the shorter side S");
  AF_REQUIRE(filter == 0 || filter == 1, "af_vit_patch_rows: filter must be 0 (triangle) or 1 (cubic)");
  AF_REQUIRE((long)kpad >= 3L * p * p && kpad % 8 == 0, "af_vit_patch_rows: kpad must be a multiple of 8 and at least 3 p^2");
  const long LIM = 1L << 31, G = C / p;
  AF_REQUIRE((long)B * H * W * 3 < LIM, "af_vit_patch_rows: the images need fewer than 2^31 bytes (B * H * W * 3)");
  AF_REQUIRE((long)B * G * G < LIM && (long)B * G * G * kpad < LIM, "af_vit_patch_rows: the rows need fewer than 2^31 elements (B * (C/p)^2 * kpad)");
  AF_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "af_vit_patch_rows: rows must be 16-byte aligned");
  AF_SUPPORTED(p <= VP_MAX_P, "af_vit_patch_rows: patch sizes above 32 are not built");
  long Hr = C, Wr = C;
  if (keep_aspect) {
    if (H <= W) Hr = S, Wr = (long)S * W / H;
    else Wr = S, Hr = (long)S * H / W;
  }
  AF_REQUIRE(Hr < LIM && Wr < LIM, "af_vit_patch_rows: the resized image has a side of 2^31 or more");
  VpArgs a;
  a.H = H, a.W = W, a.Hr = (int)Hr, a.Wr = (int)Wr;
  a.top = (int)rne_half(Hr - C), a.left = (int)rne_half(Wr - C);
  a.G = (int)G, a.p = p, a.kpad = kpad;
  a.aligned4 = (reinterpret_cast<uintptr_t>(img_u8) & 3) == 0;
  a.total_bytes = (long)B * H * W * 3;
  for (int c = 0; c < 3; ++c) a.scale[c] = scale3[c], a.shift[c] = shift3[c];
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const dim3 grid((unsigned)(B * G * G));
  if (filter == 0)
    hipLaunchKernelGGL(vit_patch_rows_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)img_u8, (half_t*)rows, a);
  else
    hipLaunchKernelGGL(vit_patch_rows_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)img_u8, (half_t*)rows, a);
  return af_check_launch("af_vit_patch_rows");
}

extern "C" int af_gelu_f16(const void* x, void* y, int64_t n, void* stream) {
  AF_REQUIRE(x && y && n > 0, "af_gelu_f16: bad argument");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const long lanes = ((long)n + 7) / 8;
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, (long)n, vec);
  return af_check_launch("af_gelu_f16");
}
