// af_conv3x3_patch.h -- the frame of the two 3x3 convolutions (pad 1) for narrow channel counts: af_dense_conv3x3 (af_esrgan.hip) and
// af_hint_conv3x3 (af_controlnet.hip).  Each of them brings a source of halo pixels and an epilogue; everything between is here, once.
//
// The frame is an implicit GEMM on v_mfma_f32_16x16x32_f16.  The MFMA's A operand is the WEIGHTS (row = output channel) and its B operand the
// PIXELS (column = the 16 pixels of one output row of the patch), so a lane ends up with four consecutive channels of one pixel: 8-byte stores.
// A workgroup of four waves owns a patch of output pixels of one image -- 16 x 16 at stride 1 (wave w: rows 4 w .. 4 w + 3), 8 x 16 at stride 2
// (wave w: rows 2 w, 2 w + 1) -- and NT <= 4 fragments (16 NT channels) of the output.  Per 32-channel chunk of the input the patch's halo
// (18 x 18 input pixels at stride 1, 17 x 33 at stride 2) goes into LDS once and the nine taps read it at shifted addresses.  Halo pixels the
// source does not locate (outside the image) are written as zeros by predication and never read from memory, so nothing leaks from the
// neighbouring image of a batch.  The next chunk's halo is loaded into registers ahead of the MFMAs of the current one.
// LDS image: four planes, one per 16-byte (8-channel) piece of the chunk, each [halo pixels][16 bytes], plane stride a multiple of the 256-byte
// bank row.  A B fragment is lane l -> plane l >> 4, pixel base + (l & 15): every 16-lane group of a ds_read_b128 covers sixteen consecutive
// 16-byte slots whatever the base, which is conflict-free.  At stride 2 a halo row is stored de-interleaved (even columns 0 .. 16, then odd
// columns 17 .. 32), so the sixteen pixels 2 j + kx of a B fragment sit in sixteen consecutive slots exactly as at stride 1.
// Weights (rows of kw halves, L2-resident) come straight from global memory as K-contiguous 16-byte fragments: all nine taps of a chunk at once
// at NT <= 2, one tap ahead above that (WCHUNK below).  Every accumulator is summed chunk-major, taps 0 .. 8 inside a chunk.
#pragma once
#include "af_common.h"

namespace {

constexpr long LIM = 1L << 31;

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int S>
struct PatchGeom {
  static constexpr int PR = S == 1 ? 4 : 2;                     // output rows per wave
  static constexpr int TY = 4 * PR;                             // output rows per workgroup
  static constexpr int HH = S * (TY - 1) + 3, HW = S * 15 + 3;  // halo: 18 x 18 | 17 x 33 input pixels
  static constexpr int HPIX = HH * HW;
  static constexpr int PLANE = (HPIX * 16 + 255) / 256 * 256;   // 5376 | 9216 bytes
  static constexpr int ITERS = (HPIX * 4 + 255) / 256;          // 6 | 9 pieces of 16 bytes per thread and chunk
  static constexpr int col(int x) { return S == 2 ? (x & 1) * 17 + (x >> 1) : x; }   // slot of halo column x in its row
};

// One workgroup's patch (blockIdx.x, blockIdx.y) of image b.
//   Src: int locate(b, y, x, q)   handle of INPUT pixel (y, x) of image b, or -1 for a pixel to take as zeros; called once per halo pixel
//        uintx4_t fetch(h, c0, q) channels c0 + 8 q .. c0 + 8 q + 7 of the pixel with handle h, as 16 bytes; called per chunk
//        (q, the thread's piece, goes to both, so that a source can fold the piece's offset into its handle once)
//        Src and Epi come by value: through a reference their fields would be memory to the optimiser until the frame is inlined into the
//        kernel, and the epilogue's address arithmetic would be redone for every fragment.
//   wt:  the weight row of fragment 0, channel 0 of tap 0; kw halves to the next row, ktap to the next tap, kext (a multiple of 32) channels
//   Epi: epi(acc, y, x, nt, c4)   acc = channels 16 nt + c4 + 0 .. 3 of output pixel (y, x), y < Ho and x < Wo
template <int S, int NT, class Src, class Epi>
__device__ __forceinline__ void conv3x3_patch(const Src src, int b, const half_t* wt, int kw, int ktap, int kext, int Ho, int Wo, const Epi epi) {
  using G = PatchGeom<S>;
  __shared__ __attribute__((aligned(16))) char lds[4 * G::PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox0 = blockIdx.x * 16, oy0 = blockIdx.y * G::TY;
  const int fr = lane & 15, fq = lane >> 4;
  const int q = tid & 3;                                 // this thread's 8-channel piece of every halo pixel it stages (256 % 4 == 0)

  // halo pieces of this thread: the source's handle or -1 outside the image; LDS byte address or -1 behind the halo
  int pix[G::ITERS], dst[G::ITERS];
#pragma unroll
  for (int it = 0; it < G::ITERS; ++it) {
    const int hp = (it * 256 + tid) >> 2;
    const int hy = hp / G::HW, hx = hp - hy * G::HW;
    const int h = src.locate(b, S * oy0 - 1 + hy, S * ox0 - 1 + hx, q);
    pix[it] = hp < G::HPIX ? h : -1;
    dst[it] = hp < G::HPIX ? q * G::PLANE + (hy * G::HW + G::col(hx)) * 16 : -1;
  }
  uintx4_t stage[G::ITERS];
  auto load_halo = [&](int c0) {
#pragma unroll
    for (int it = 0; it < G::ITERS; ++it) {
      stage[it] = uintx4_t{0u, 0u, 0u, 0u};
      if (pix[it] >= 0) stage[it] = src.fetch(pix[it], c0, q);
    }
  };

  floatx4 acc[G::PR][NT];
#pragma unroll
  for (int mt = 0; mt < G::PR; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const half_t* wl = wt + fr * kw + fq * 8;             // this lane's weight row (of fragment 0) and K piece
  const int pix0 = fq * G::PLANE + (wave * G::PR * S * G::HW + fr) * 16;

  // weight fragments: a whole chunk (nine taps) at once where the registers allow it (NT <= 2: 36 / 72 VGPRs), issued ahead of the halo's LDS
  // write and its barriers so that their L2 latency is not paid tap by tap; one tap ahead otherwise.  Against one tap ahead everywhere, the dense
  // kernel at NT = 2 and 512 x 512: 51 -> 41 us at cin 64, 76 -> 59 us at cin 160, at 184 instead of 132 VGPRs (2 waves per SIMD instead of 3);
  // profiles/esrgan.txt.
  constexpr bool WCHUNK = NT <= 2;
  constexpr int WT = WCHUNK ? 9 : 2;
  half8_t w[WT][NT];
  auto load_w = [&](int slot, int tap, int c0) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) w[slot][nt] = *reinterpret_cast<const half8_t*>(wl + nt * 16 * kw + tap * ktap + c0);
  };

  load_halo(0);
  for (int c0 = 0; c0 < kext; c0 += 32) {
    if (WCHUNK) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) load_w(tap, tap, c0);
    } else {
      load_w(0, 0, c0);
    }
    __syncthreads();                                    // the previous chunk's fragment reads are done
#pragma unroll
    for (int it = 0; it < G::ITERS; ++it)
      if (dst[it] >= 0) *reinterpret_cast<uintx4_t*>(lds + dst[it]) = stage[it];
    __syncthreads();
    if (c0 + 32 < kext) load_halo(c0 + 32);

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int cur = WCHUNK ? tap : tap & 1;
      if (!WCHUNK && tap < 8) load_w(cur ^ 1, tap + 1, c0);
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int mt = 0; mt < G::PR; ++mt) {
        const half8_t px = *reinterpret_cast<const half8_t*>(lds + pix0 + ((mt * S + ky) * G::HW + G::col(kx)) * 16);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[cur][nt], px, acc[mt][nt], 0, 0, 0);
      }
    }
  }

  // lane = output pixel (oy0 + PR wave + mt, ox0 + fr), channels 16 nt + 4 fq + 0 .. 3
  const int x = ox0 + fr;
  if (x >= Wo) return;
#pragma unroll
  for (int mt = 0; mt < G::PR; ++mt) {
    const int y = oy0 + wave * G::PR + mt;
    if (y >= Ho) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) epi(acc[mt][nt], y, x, nt, fq * 4);
  }
}

}  // namespace
