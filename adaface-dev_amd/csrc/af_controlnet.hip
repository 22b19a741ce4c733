// af_controlnet.hip -- the kernel of ControlNet's hint encoder (ldm/modules/diffusionmodules/controlnet.py, input_hint_block).
//   af_hint_conv3x3      3x3 convolution (pad 1, stride 1 or 2) for narrow channel counts (16 .. 256 in, 16 .. 256 out, or a uint8 RGB image in):
//                        bias and SiLU in the epilogue, fp16 NHWC out.
//
// It runs on the patch frame of af_conv3x3_patch.h at both strides: a workgroup owns a patch of output pixels of one image and a slab of
// NT <= 4 fragments (16 NT channels) of cout; blockIdx.z runs over images x slabs.  This file has what is the hint kernel's own.  Its source of
// halo pixels is a cin-dense NHWC tensor with bounds on the INPUT grid, whose channels behind cin in the last chunk are zeros by predication and
// never read from memory; or, at in_mode 1, a uint8 RGB image: the three bytes of a pixel are put into the halo as the exact fp16 integers
// 0 .. 255 (channels 3 .. 31 zero) and the 1 / 255 is applied to the fp32 accumulator, so the image is neither copied to fp16 in memory nor
// rounded.  Its weights are [cout][9 cpad] halves (at most 1.2 MB).  Its epilogue writes whole fragments (cout % 16 == 0).
#include "af_conv3x3_patch.h"

namespace {

struct HintArgs {
  const void* x;
  const half_t* wt;
  const float* bias;
  half_t* out;
  int in_mode, cin, cpad, cout, act, nslab, H, W, Ho, Wo;
  float scale;

  // the frame's Src: index of the input pixel
  __device__ int locate(int b, int y, int x_, int) const { return y >= 0 && y < H && x_ >= 0 && x_ < W ? (b * H + y) * W + x_ : -1; }
  __device__ uintx4_t fetch(int h, int c0, int q) const {
    uintx4_t v = {0u, 0u, 0u, 0u};
    if (in_mode == 0) {
      if (c0 + q * 8 < cin) v = *reinterpret_cast<const uintx4_t*>((const half_t*)x + h * cin + c0 + q * 8);
    } else if (q == 0) {
      const unsigned char* p = (const unsigned char*)x + h * 3;
      const half8_t px = {(half_t)(float)p[0], (half_t)(float)p[1], (half_t)(float)p[2], (half_t)0.f,
                          (half_t)0.f,         (half_t)0.f,         (half_t)0.f,         (half_t)0.f};
      v = __builtin_bit_cast(uintx4_t, px);
    }
    return v;
  }
};

template <int S, int NT>
__global__ __launch_bounds__(256) void hint_conv3x3_kernel(const HintArgs a) {
  const int b = blockIdx.z / a.nslab, slab = blockIdx.z - b * a.nslab;
  const int kw = 9 * a.cpad;
  conv3x3_patch<S, NT>(a, b, a.wt + slab * NT * 16 * kw, kw, a.cpad, a.cpad, a.Ho, a.Wo, [=](const floatx4& acc, int y, int x, int nt, int c4) {
    const int m = (b * a.Ho + y) * a.Wo + x;
    const int n0 = (slab * NT + nt) * 16 + c4;
    half4_t h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float y32 = acc[r] * a.scale;
      if (a.bias) y32 += a.bias[n0 + r];
      h[r] = (half_t)(a.act ? y32 / (1.f + __expf(-y32)) : y32);
    }
    *reinterpret_cast<half4_t*>(a.out + m * a.cout + n0) = h;
  });
}

template <int S>
void launch(const HintArgs& a, int nt, dim3 grid, hipStream_t stream) {
  switch (nt) {
    case 1: hipLaunchKernelGGL((hint_conv3x3_kernel<S, 1>), grid, dim3(256), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((hint_conv3x3_kernel<S, 2>), grid, dim3(256), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((hint_conv3x3_kernel<S, 3>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((hint_conv3x3_kernel<S, 4>), grid, dim3(256), 0, stream, a); break;
  }
}

}  // namespace

extern "C" int af_hint_conv3x3(const void* x, int in_mode, int cin, const void* wt, const void* bias, void* out, int cout, int stride, int act,
                               int B, int H, int W, void* stream) {
  AF_REQUIRE(x && wt && out, "af_hint_conv3x3: x, wt and out must not be NULL");
  AF_REQUIRE(B > 0 && H > 0 && W > 0, "af_hint_conv3x3: B, H and W must be positive");
  AF_REQUIRE(in_mode == 0 || in_mode == 1, "af_hint_conv3x3: in_mode must be 0 (fp16 NHWC) or 1 (uint8 RGB)");
  AF_REQUIRE(in_mode == 1 || (cin % 16 == 0 && cin >= 16 && cin <= 256), "af_hint_conv3x3: cin must be a multiple of 16 from 16 to 256");
  AF_REQUIRE(in_mode == 0 || cin == 3, "af_hint_conv3x3: a uint8 image has cin = 3");
  AF_REQUIRE(cout % 16 == 0 && cout >= 16 && cout <= 256, "af_hint_conv3x3: cout must be a multiple of 16 from 16 to 256");
  AF_REQUIRE(stride == 1 || stride == 2, "af_hint_conv3x3: stride must be 1 or 2");
  AF_REQUIRE(act == 0 || act == 1, "af_hint_conv3x3: act must be 0 or 1 (SiLU)");
  AF_REQUIRE((in_mode == 1 || aligned(x, 16)) && aligned(wt, 16) && aligned(out, 8) && aligned(bias, 4),
             "af_hint_conv3x3: x (fp16) and wt must be 16-byte aligned, out 8-byte, bias 4-byte");
  const long Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  AF_REQUIRE((long)B * H * W * cin < LIM && (long)B * Ho * Wo * cout < LIM,
             "af_hint_conv3x3: B*H*W*cin and B*Ho*Wo*cout must be below 2^31 (32-bit offsets): split the batch");
  const int nf = cout / 16;
  const int nt = nf % 4 == 0 ? 4 : (nf % 3 == 0 ? 3 : (nf % 2 == 0 ? 2 : 1));   // fragments per slab: every slab whole
  HintArgs a;
  a.x = x, a.wt = (const half_t*)wt, a.bias = (const float*)bias, a.out = (half_t*)out;
  a.in_mode = in_mode, a.cin = cin, a.cpad = (cin + 31) / 32 * 32, a.cout = cout, a.act = act, a.nslab = nf / nt;
  a.H = H, a.W = W, a.Ho = (int)Ho, a.Wo = (int)Wo;
  a.scale = in_mode == 1 ? 1.f / 255.f : 1.f;
  const long ty = stride == 1 ? 16 : 8;
  const dim3 grid((unsigned)((Wo + 15) / 16), (unsigned)((Ho + ty - 1) / ty), (unsigned)(B * a.nslab));
  AF_REQUIRE(grid.y <= 65535u && (long)B * a.nslab <= 65535, "af_hint_conv3x3: more than 65535 patch rows or images x channel slabs");
  AfLaunchScope scope(AF_FAM_GEMM, stream);
  if (stride == 1)
    launch<1>(a, nt, grid, (hipStream_t)stream);
  else
    launch<2>(a, nt, grid, (hipStream_t)stream);
  return af_check_launch("af_hint_conv3x3");
}
