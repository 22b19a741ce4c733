// af_controlnet.hip -- the kernel of ControlNet's hint encoder (ldm/modules/diffusionmodules/controlnet.py, input_hint_block).
//   af_hint_conv3x3      3x3 convolution (pad 1, stride 1 or 2) for narrow channel counts (16 .. 256 in, 16 .. 256 out, or a uint8 RGB image in):
//                        bias and SiLU in the epilogue, fp16 NHWC out.
//
// The tuned implicit-GEMM tiles are 128 columns wide and idle on N = 16 / 32 / 96; af_dense_conv3x3 (af_esrgan.hip) has the right shape of tile
// but neither stride 2 nor these channel ranges.  This kernel keeps its frame: an implicit GEMM on v_mfma_f32_16x16x32_f16 whose A operand is
// the WEIGHTS (row = output channel) and whose B operand the PIXELS (column = the 16 pixels of one output row of the patch), so a lane ends up
// with four consecutive channels of one pixel: 8-byte stores.  A workgroup of four waves owns a patch of output pixels of one image -- 16 x 16
// at stride 1 (wave w: rows 4 w .. 4 w + 3), 8 x 16 at stride 2 (wave w: rows 2 w, 2 w + 1) -- and a slab of NT <= 4 fragments (16 NT channels)
// of cout; blockIdx.z runs over images x slabs.  Per 32-channel chunk of the input the patch's halo (18 x 18 input pixels at stride 1, 17 x 33
// at stride 2) goes into LDS once and the nine taps read it at shifted addresses.  Halo pixels outside the image, and channels behind cin in
// the last chunk, are written as zeros by predication and never read from memory.
// LDS image: four planes, one per 16-byte (8-channel) piece of the chunk, each [halo pixels][16 bytes], plane stride a multiple of the 256-byte
// bank row.  At stride 2 a halo row is stored de-interleaved (even columns 0 .. 16, then odd columns 17 .. 32), so the sixteen pixels 2 j + kx
// of a B fragment sit in sixteen consecutive 16-byte slots exactly as at stride 1: conflict-free ds_read_b128 at both strides.
// in_mode 1 (uint8 RGB image): the three bytes of a pixel are put into the halo as the exact fp16 integers 0 .. 255 (channels 3 .. 31 zero) and
// the 1 / 255 is applied to the fp32 accumulator, so the image is neither copied to fp16 in memory nor rounded.
// Weights ([cout][9 cpad] halves, at most 1.2 MB, L2-resident) come straight from global memory as K-contiguous 16-byte fragments, one tap ahead
// of the MFMAs that use them (a whole chunk ahead where NT <= 2 leaves the registers for it).
#include "af_common.h"

namespace {

constexpr long LIM = 1L << 31;

struct HintArgs {
  const void* x;
  const half_t* wt;
  const float* bias;
  half_t* out;
  int in_mode, cin, cpad, cout, act, nslab, H, W, Ho, Wo;
  float scale;
};

template <int S, int NT>
__global__ __launch_bounds__(256) void hint_conv3x3_kernel(const HintArgs a) {
  constexpr int PR = S == 1 ? 4 : 2;                     // output rows per wave
  constexpr int TY = 4 * PR;                             // output rows per workgroup
  constexpr int HH = S * (TY - 1) + 3, HW = S * 15 + 3;  // halo: 18 x 18 | 17 x 33 input pixels
  constexpr int HPIX = HH * HW;
  constexpr int PLANE = (HPIX * 16 + 255) / 256 * 256;   // 5376 | 9216 bytes
  constexpr int PIECES = HPIX * 4;
  constexpr int ITERS = (PIECES + 255) / 256;            // 6 | 9
  __shared__ __attribute__((aligned(16))) char lds[4 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox0 = blockIdx.x * 16, oy0 = blockIdx.y * TY;
  const int b = blockIdx.z / a.nslab, slab = blockIdx.z - b * a.nslab;
  const int fr = lane & 15, fq = lane >> 4;
  const int q = tid & 3;                                 // this thread's 8-channel piece of every halo pixel it stages (256 % 4 == 0)

  // halo pieces of this thread: input pixel index or -1 outside the image; LDS byte address or -1 behind the halo
  int pix[ITERS], dst[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int hp = (it * 256 + tid) >> 2;
    const int hy = hp / HW, hx = hp - hy * HW;
    const int y = S * oy0 - 1 + hy, x = S * ox0 - 1 + hx;
    const bool in = hp < HPIX && y >= 0 && y < a.H && x >= 0 && x < a.W;
    pix[it] = in ? (b * a.H + y) * a.W + x : -1;
    const int slot = hy * HW + (S == 2 ? (hx & 1) * 17 + (hx >> 1) : hx);
    dst[it] = hp < HPIX ? q * PLANE + slot * 16 : -1;
  }
  uintx4_t stage[ITERS];
  auto load_halo = [&](int c0) {
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      stage[it] = uintx4_t{0u, 0u, 0u, 0u};
      if (pix[it] < 0) continue;
      if (a.in_mode == 0) {
        if (c0 + q * 8 < a.cin) stage[it] = *reinterpret_cast<const uintx4_t*>((const half_t*)a.x + pix[it] * a.cin + c0 + q * 8);
      } else if (q == 0) {
        const unsigned char* p = (const unsigned char*)a.x + pix[it] * 3;
        const half8_t v = {(half_t)(float)p[0], (half_t)(float)p[1], (half_t)(float)p[2], (half_t)0.f,
                           (half_t)0.f,         (half_t)0.f,         (half_t)0.f,         (half_t)0.f};
        stage[it] = __builtin_bit_cast(uintx4_t, v);
      }
    }
  };

  floatx4 acc[PR][NT];
#pragma unroll
  for (int mt = 0; mt < PR; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int kw = 9 * a.cpad;
  const half_t* wl = a.wt + (slab * NT * 16 + fr) * kw + fq * 8;   // this lane's weight row (of the slab's fragment 0) and K piece
  const int pix0 = fq * PLANE + (wave * PR * S * HW + fr) * 16;

  constexpr bool WCHUNK = NT <= 2;
  constexpr int WT = WCHUNK ? 9 : 2;
  half8_t w[WT][NT];
  auto load_w = [&](int slot, int tap, int c0) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) w[slot][nt] = *reinterpret_cast<const half8_t*>(wl + nt * 16 * kw + tap * a.cpad + c0);
  };

  load_halo(0);
  for (int c0 = 0; c0 < a.cpad; c0 += 32) {
    if (WCHUNK) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) load_w(tap, tap, c0);
    } else {
      load_w(0, 0, c0);
    }
    __syncthreads();                                    // the previous chunk's fragment reads are done
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
      if (dst[it] >= 0) *reinterpret_cast<uintx4_t*>(lds + dst[it]) = stage[it];
    __syncthreads();
    if (c0 + 32 < a.cpad) load_halo(c0 + 32);

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int cur = WCHUNK ? tap : tap & 1;
      if (!WCHUNK && tap < 8) load_w(cur ^ 1, tap + 1, c0);
      const int ky = tap / 3, kx = tap - ky * 3;
      const int col = S == 2 ? (kx & 1) * 17 + (kx >> 1) : kx;
#pragma unroll
      for (int mt = 0; mt < PR; ++mt) {
        const half8_t px = *reinterpret_cast<const half8_t*>(lds + pix0 + ((mt * S + ky) * HW + col) * 16);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[cur][nt], px, acc[mt][nt], 0, 0, 0);
      }
    }
  }

  // epilogue: lane = pixel (oy0 + PR wave + mt, ox0 + fr), channels (slab NT + nt) * 16 + fq * 4 + 0..3 (cout % 16 == 0: always whole)
  const int x = ox0 + fr;
  if (x >= a.Wo) return;
#pragma unroll
  for (int mt = 0; mt < PR; ++mt) {
    const int y = oy0 + wave * PR + mt;
    if (y >= a.Ho) continue;
    const int m = (b * a.Ho + y) * a.Wo + x;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n0 = (slab * NT + nt) * 16 + fq * 4;
      half4_t h;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float y32 = acc[mt][nt][r] * a.scale;
        if (a.bias) y32 += a.bias[n0 + r];
        h[r] = (half_t)(a.act ? y32 / (1.f + __expf(-y32)) : y32);
      }
      *reinterpret_cast<half4_t*>(a.out + m * a.cout + n0) = h;
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

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
