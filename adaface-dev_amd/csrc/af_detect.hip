// af_detect.hip -- what the RetinaFace-R50 face detector (adaface/retinaface.py; biubug6 Pytorch_Retinaface, cfg_re50) needs around af_gemm.
// The network's FLOPs are GEMMs (1x1 convolutions, the im2col'd stem) and the implicit-GEMM 3x3 kernel; these are the layers between them
// and the post-processing that the reference leaves to the host:
//   af_stem_im2col7x7     uint8 photo -> normalised fp16 rows of the 7x7 / stride 2 / pad 3 window (the stem's A operand, K = 147 padded to 160)
//   af_relu_maxpool3x3s2  3x3 / stride 2 / pad 1 max + ReLU, NHWC fp16
//   af_subsample2x        the even pixels of an NHWC tensor (the A operand of a stride-2 1x1 shortcut)
//   af_upsample2x_add     y = a + nearest2x(b) (FPN top-down path)
//   af_retina_decode      three head tensors -> per-image candidate rows (box, score, landmarks, anchor) of the anchors that pass the threshold
//   af_retina_nms         sort + greedy IoU suppression of one image's candidates in LDS -> a fixed-size detection table
// The element-wise kernels move 8 channels (16 B) per lane like af_face.hip and are HBM / launch bound.  The decode reads 32 B and writes at
// most 64 B per anchor: launch bound at every image size the detector takes.  The NMS is latency bound: one workgroup per image, one barrier
// per candidate that is visited (at most C = 1024 rounds of a broadcast LDS read, one IoU and one flag write per lane).
#include "af_common.h"

namespace {

constexpr int STEM_K = 147;          // 7 * 7 * 3, column order (ky, kx, c)
constexpr int STEM_KPAD = 160;
constexpr int NMS_CAP = 1024;        // candidates per image = threads of the NMS workgroup
constexpr int ROW = 16;              // floats per candidate / detection row: x1 y1 x2 y2 score, 10 landmark coordinates, anchor index

struct StemNorm {
  float scale[3], shift[3];
};

// one lane per (output pixel, 8-column chunk): 20 chunks per row.  A tap outside the H x W image (the 3-pixel halo and the bottom / right
// padding up to the multiple of 32) is 0 in normalised space, so the normalisation cannot live in the weights.
__global__ __launch_bounds__(256) void stem_im2col7x7_kernel(const unsigned char* __restrict__ img, half_t* __restrict__ out, StemNorm nm,
                                                             int H, int W, int Ho, int Wo, int bgr, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int chunk = (int)(i % (STEM_KPAD / 8));
  long p = i / (STEM_KPAD / 8);
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const long b = p / Ho;
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = chunk * 8 + e;
    float v = 0.f;
    if (k < STEM_K) {
      const int ky = k / 21, kx = (k % 21) / 3, c = k % 3;
      const int y = 2 * oy - 3 + ky, x = 2 * ox - 3 + kx;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const long off = ((b * H + y) * W + x) * 3 + (bgr ? 2 - c : c);          // < 2^31 (checked by the caller)
        v = (float)img[off] * nm.scale[c] + nm.shift[c];
      }
    }
    o[e] = (half_t)v;
  }
  *reinterpret_cast<half8_t*>(out + i * 8) = o;
}

// max over the taps inside the image, then ReLU; the maximum starts at 0, which is what ReLU makes of any smaller value, so padding never wins
__global__ __launch_bounds__(256) void relu_maxpool3x3s2_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, int H, int W, int Ho,
                                                                int Wo, int C8, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c = (int)(i % C8);
  long p = i / C8;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const long b = p / Ho;
  float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = 2 * oy - 1 + ky;
    if (yy < 0 || yy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = 2 * ox - 1 + kx;
      if (xx < 0 || xx >= W) continue;
      const half8_t v = *reinterpret_cast<const half8_t*>(x + (((b * H + yy) * W + xx) * C8 + c) * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
    }
  }
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)m[e];
  *reinterpret_cast<half8_t*>(y + i * 8) = o;
}

__global__ __launch_bounds__(256) void subsample2x_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, int H, int W, int Ho, int Wo,
                                                          int C8, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c = (int)(i % C8);
  long p = i / C8;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const long b = p / Ho;
  *reinterpret_cast<half8_t*>(y + i * 8) = *reinterpret_cast<const half8_t*>(x + (((b * H + 2 * oy) * W + 2 * ox) * C8 + c) * 8);
}

// a [B, 2h, 2w, C], b [B, h, w, C]; fp32 sum rounded once
__global__ __launch_bounds__(256) void upsample2x_add_kernel(const half_t* __restrict__ a, const half_t* __restrict__ bs,
                                                             half_t* __restrict__ y, int h, int w, int C8, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c = (int)(i % C8);
  long p = i / C8;
  const int x = (int)(p % (2 * w));
  p /= 2 * w;
  const int yy = (int)(p % (2 * h));
  const long b = p / (2 * h);
  const half8_t va = *reinterpret_cast<const half8_t*>(a + i * 8);
  const half8_t vb = *reinterpret_cast<const half8_t*>(bs + (((b * h + (yy >> 1)) * w + (x >> 1)) * C8 + c) * 8);
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)va[e] + (float)vb[e]);
  *reinterpret_cast<half8_t*>(y + i * 8) = o;
}

struct RetinaLevels {
  const half_t* head[3];       // fp16 [B, Hk * Wk, 32]: per anchor a, 16 columns [box 4 | cls 2 | ldm 10]
  int H[3], W[3];
  int first[3];                // anchor index of the level's first anchor
  float step[3];
  float min_size[3][2];
  int anchors;                 // per image
};

// one lane per (image, anchor); biubug6's PriorBox order: level, row, column, min-size.  Everything in pixels of the padded image.
__global__ __launch_bounds__(256) void retina_decode_kernel(RetinaLevels L, float conf_thr, float* __restrict__ cand, int* __restrict__ count,
                                                           int cap, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = (int)(i / L.anchors), idx = (int)(i % L.anchors);
  const int lv = idx >= L.first[2] ? 2 : (idx >= L.first[1] ? 1 : 0);
  const int local = idx - L.first[lv];
  const int a = local & 1, cell = local >> 1;
  const int cy_i = cell / L.W[lv], cx_i = cell % L.W[lv];
  const half_t* row = L.head[lv] + ((long)b * L.H[lv] * L.W[lv] + cell) * 32 + a * 16;
  const half8_t r0 = *reinterpret_cast<const half8_t*>(row), r1 = *reinterpret_cast<const half8_t*>(row + 8);
  const float score = 1.0f / (1.0f + __expf((float)r0[4] - (float)r0[5]));
  if (!(score >= conf_thr)) return;                                        // NaN never passes
  const int slot = atomicAdd(count + b, 1);                                // counts every passing anchor, also beyond the capacity
  if (slot >= cap) return;
  const float s = L.min_size[lv][a], st = L.step[lv];
  const float ax = ((float)cx_i + 0.5f) * st, ay = ((float)cy_i + 0.5f) * st;
  const float vs = 0.1f * s;
  const float cx = ax + vs * (float)r0[0], cy = ay + vs * (float)r0[1];
  const float w = s * __expf(0.2f * (float)r0[2]), h = s * __expf(0.2f * (float)r0[3]);
  const float x1 = cx - 0.5f * w, y1 = cy - 0.5f * h;
  float o[ROW];
  o[0] = x1, o[1] = y1, o[2] = x1 + w, o[3] = y1 + h, o[4] = score;
  o[5] = ax + vs * (float)r0[6], o[6] = ay + vs * (float)r0[7];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[7 + 2 * k] = ax + vs * (float)r1[2 * k], o[8 + 2 * k] = ay + vs * (float)r1[2 * k + 1];
  o[15] = (float)idx;                                                      // exact: anchors < 2^24 (checked by the caller)
  floatx4* dst = reinterpret_cast<floatx4*>(cand + ((long)b * cap + slot) * ROW);
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[k] = floatx4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
}

// One workgroup of 1024 lanes per image, lane t <-> candidate t.
//  1. rank by counting: lane t walks all n (score, anchor) pairs (every lane reads the same LDS address: a broadcast) and counts those that
//     precede its own in the order (score descending, anchor ascending).  Anchors are distinct, so the ranks are a permutation and the
//     result does not depend on the order the decode appended in.
//  2. scatter box and source slot to the rank.
//  3. greedy suppression, one barrier round per visited candidate: if candidate i is alive, lane i copies its row to the output and every
//     later lane marks itself suppressed when IoU > thr; the round's barrier publishes the marks before i + 1 is looked at.
__global__ __launch_bounds__(NMS_CAP) void retina_nms_kernel(const float* __restrict__ cand, const int* __restrict__ count,
                                                             float* __restrict__ out, int* __restrict__ out_counts, int cap, int max_det,
                                                             float nms_thr) {
  __shared__ float key_score[NMS_CAP];
  __shared__ int key_anchor[NMS_CAP];
  __shared__ floatx4 box[NMS_CAP];
  __shared__ int src[NMS_CAP];
  __shared__ int dead[NMS_CAP];
  const int b = blockIdx.x, t = threadIdx.x;
  const int passing = count[b];
  const int n = min(passing, cap);
  const float* mine = cand + ((long)b * cap + t) * ROW;
  floatx4 bx = {0.f, 0.f, 0.f, 0.f};
  float sc = 0.f;
  int an = 0;
  if (t < n) {
    bx = *reinterpret_cast<const floatx4*>(mine);
    sc = mine[4];
    an = (int)mine[15];
    key_score[t] = sc;
    key_anchor[t] = an;
  }
  dead[t] = 0;
  __syncthreads();
  if (t < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = key_score[j];
      rank += (sj > sc || (sj == sc && key_anchor[j] < an)) ? 1 : 0;
    }
    box[rank] = bx;
    src[rank] = t;
  }
  __syncthreads();
  if (t < n) bx = box[t];
  const float area = (bx[2] - bx[0]) * (bx[3] - bx[1]);
  int kept = 0;
  for (int i = 0; i < n && kept < max_det; ++i) {
    if (!dead[i]) {                                                        // uniform: every lane reads the same flag
      if (t == i) {
        const floatx4* s = reinterpret_cast<const floatx4*>(cand + ((long)b * cap + src[i]) * ROW);
        floatx4* d = reinterpret_cast<floatx4*>(out + ((long)b * max_det + kept) * ROW);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = s[k];
      } else if (t > i && t < n) {
        const floatx4 o = box[i];
        const float iw = fmaxf(fminf(bx[2], o[2]) - fmaxf(bx[0], o[0]), 0.f), ih = fmaxf(fminf(bx[3], o[3]) - fmaxf(bx[1], o[1]), 0.f);
        const float inter = iw * ih;
        const float iou = inter / (area + (o[2] - o[0]) * (o[3] - o[1]) - inter);
        if (iou > nms_thr) dead[t] = 1;
      }
      ++kept;
    }
    __syncthreads();
  }
  for (int r = kept * ROW + t; r < max_det * ROW; r += NMS_CAP) out[(long)b * max_det * ROW + r] = 0.f;
  if (t == 0) {
    out_counts[2 * b] = kept;
    out_counts[2 * b + 1] = passing;
  }
}

inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr long LIM = 1L << 31;

}  // namespace

extern "C" int af_stem_im2col7x7(const void* image_u8, const float* scale, const float* shift, void* out, int B, int H, int W, int bgr,
                                 void* stream) {
  AF_REQUIRE(image_u8 && scale && shift && out && B > 0 && H > 0 && W > 0, "af_stem_im2col7x7: bad argument");
  AF_REQUIRE(al16(out), "af_stem_im2col7x7: out must be 16-byte aligned");
  AF_REQUIRE((long)B * H * W * 3 < LIM, "af_stem_im2col7x7: the images need fewer than 2^31 bytes (B * H * W * 3)");
  const int Ho = (H + 31) / 32 * 16, Wo = (W + 31) / 32 * 16;
  const long rows = (long)B * Ho * Wo;
  AF_REQUIRE(rows * STEM_KPAD * 2 < LIM, "af_stem_im2col7x7: the output needs fewer than 2^31 bytes (B * Ho * Wo * 160 * 2)");
  StemNorm nm;
  for (int c = 0; c < 3; ++c) nm.scale[c] = scale[c], nm.shift[c] = shift[c];
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const long n8 = rows * (STEM_KPAD / 8);
  hipLaunchKernelGGL(stem_im2col7x7_kernel, g1(n8), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)image_u8, (half_t*)out, nm, H, W,
                     Ho, Wo, bgr ? 1 : 0, n8);
  return af_check_launch("af_stem_im2col7x7");
}

extern "C" int af_relu_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, void* stream) {
  AF_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "af_relu_maxpool3x3s2: bad argument (C must be a positive multiple of 8)");
  AF_REQUIRE(al16(x) && al16(y), "af_relu_maxpool3x3s2: x and y must be 16-byte aligned");
  AF_REQUIRE((long)B * H * W * C * 2 < LIM, "af_relu_maxpool3x3s2: the input needs fewer than 2^31 bytes");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const long n8 = (long)B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(relu_maxpool3x3s2_kernel, g1(n8), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, H, W, Ho, Wo, C / 8, n8);
  return af_check_launch("af_relu_maxpool3x3s2");
}

extern "C" int af_subsample2x(const void* x, void* y, int B, int H, int W, int C, void* stream) {
  AF_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "af_subsample2x: bad argument (C must be a positive multiple of 8)");
  AF_REQUIRE(al16(x) && al16(y), "af_subsample2x: x and y must be 16-byte aligned");
  AF_REQUIRE((long)B * H * W * C * 2 < LIM, "af_subsample2x: the input needs fewer than 2^31 bytes");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const long n8 = (long)B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(subsample2x_kernel, g1(n8), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, H, W, Ho, Wo, C / 8, n8);
  return af_check_launch("af_subsample2x");
}

extern "C" int af_upsample2x_add(const void* a, const void* b, void* y, int B, int h, int w, int C, void* stream) {
  AF_REQUIRE(a && b && y && B > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0, "af_upsample2x_add: bad argument (C must be a positive multiple of 8)");
  AF_REQUIRE(al16(a) && al16(b) && al16(y), "af_upsample2x_add: a, b and y must be 16-byte aligned");
  AF_REQUIRE((long)B * h * w * 4 * C * 2 < LIM, "af_upsample2x_add: the output needs fewer than 2^31 bytes");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  const long n8 = (long)B * h * w * 4 * (C / 8);
  hipLaunchKernelGGL(upsample2x_add_kernel, g1(n8), dim3(256), 0, (hipStream_t)stream, (const half_t*)a, (const half_t*)b, (half_t*)y, h, w,
                     C / 8, n8);
  return af_check_launch("af_upsample2x_add");
}

extern "C" int af_retina_decode(const void* head0, const void* head1, const void* head2, const int* level_hw, const int* steps,
                                const float* min_sizes, int B, float conf_thr, void* cand, void* count, int C, void* stream) {
  AF_REQUIRE(head0 && head1 && head2 && level_hw && steps && min_sizes && cand && count && B > 0, "af_retina_decode: bad argument");
  AF_REQUIRE(C >= 1 && C <= NMS_CAP, "af_retina_decode: the capacity C must be in [1, 1024]");
  AF_REQUIRE(al16(head0) && al16(head1) && al16(head2) && al16(cand), "af_retina_decode: the head tensors and cand must be 16-byte aligned");
  RetinaLevels L;
  const void* heads[3] = {head0, head1, head2};
  long anchors = 0;
  for (int k = 0; k < 3; ++k) {
    AF_REQUIRE(level_hw[2 * k] > 0 && level_hw[2 * k + 1] > 0 && steps[k] > 0 && min_sizes[2 * k] > 0.f && min_sizes[2 * k + 1] > 0.f,
               "af_retina_decode: level sizes, steps and min-sizes must be positive");
    L.head[k] = (const half_t*)heads[k];
    L.H[k] = level_hw[2 * k], L.W[k] = level_hw[2 * k + 1];
    L.first[k] = (int)anchors;
    L.step[k] = (float)steps[k];
    L.min_size[k][0] = min_sizes[2 * k], L.min_size[k][1] = min_sizes[2 * k + 1];
    AF_REQUIRE((long)B * L.H[k] * L.W[k] * 64 < LIM, "af_retina_decode: a head tensor needs fewer than 2^31 bytes (B * Hk * Wk * 32 * 2)");
    anchors += 2L * L.H[k] * L.W[k];
    AF_REQUIRE(anchors < (1L << 24), "af_retina_decode: needs fewer than 2^24 anchors per image (the index is kept in an fp32)");
  }
  L.anchors = (int)anchors;
  const long n = anchors * B;
  AF_REQUIRE(n < LIM, "af_retina_decode: needs fewer than 2^31 anchors in the batch");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  if (hipMemsetAsync(count, 0, sizeof(int) * (size_t)B, (hipStream_t)stream) != hipSuccess) return af_check_launch("af_retina_decode");
  hipLaunchKernelGGL(retina_decode_kernel, g1(n), dim3(256), 0, (hipStream_t)stream, L, conf_thr, (float*)cand, (int*)count, C, n);
  return af_check_launch("af_retina_decode");
}

extern "C" int af_retina_nms(const void* cand, const void* count, void* out, void* out_counts, int B, int C, int max_det, float nms_thr,
                             void* stream) {
  AF_REQUIRE(cand && count && out && out_counts && B > 0, "af_retina_nms: bad argument");
  AF_REQUIRE(C >= 1 && C <= NMS_CAP, "af_retina_nms: the capacity C must be in [1, 1024]");
  AF_REQUIRE(max_det >= 1 && max_det <= C, "af_retina_nms: max_det must be in [1, C]");
  AF_REQUIRE(al16(cand) && al16(out), "af_retina_nms: cand and out must be 16-byte aligned");
  AF_REQUIRE((long)B * C * ROW * 4 < LIM, "af_retina_nms: the candidate lists need fewer than 2^31 bytes (B * C * 64)");
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(retina_nms_kernel, dim3(B), dim3(NMS_CAP), 0, (hipStream_t)stream, (const float*)cand, (const int*)count, (float*)out,
                     (int*)out_counts, C, max_det, nms_thr);
  return af_check_launch("af_retina_nms");
}
