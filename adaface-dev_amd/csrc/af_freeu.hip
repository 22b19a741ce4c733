// af_freeu.hip -- FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") on the two inputs of a decoder skip concatenation, NHWC fp16, gfx950.
//
//   h    [B, H, W, C ]  backbone: the first C/2 channels are multiplied per pixel by  f = (b - 1) * mhat + 1  (version 2;  f = b  for version 1),
//                       mhat = (m - lo) / (hi - lo), m = the pixel's mean over all C channels, lo / hi = min / max of m over the sample (hi == lo: 0)
//   skip [B, H, W, Cs]  every (sample, channel) plane gets the DFT bins {0, -1} x {0, -1} scaled by s -- in closed form
//                          y = x + (s - 1) / (HW) * sum_bins (A cos phi + B sin phi),   A = sum x cos phi, B = sum x sin phi
//
// Two launches, no atomics, no hand-off between workgroups inside a launch:
//   af_freeu_stats  one pass over h and skip: the pixel means and per-wave (lo, hi) partials; per (sample, skip channel) the seven sums
//                   S0 = sum d, Ph / Qh = sum d cos / sin(2 pi h / H), Pw / Qw the same along W, Pd / Qd = sum d cos / sin(2 pi (h / H + w / W)), as
//                   one partial per slice of the pixels, where d = x - pivot and the pivot is the plane's first pixel: the cosines and sines sum
//                   to zero over a plane, so the harmonic sums do not change, and a plane that is a large offset plus a small variation is summed
//                   at the size of the variation (the offset itself comes back in S0: sum x = HW pivot + S0)
//   af_freeu_apply  combines the partials in slice order (fixed, so two runs agree bit for bit) and does the two element-wise passes.
// A workgroup is either an "h" or a "skip" workgroup by its index (uniform over the workgroup): the only barriers sit in the skip role's
// straight-line code and in the apply kernel's h role ahead of its loop, all under workgroup-uniform conditions; the pixel-mean reduction is wave
// shuffles only.
//
// skip role decomposition (both kernels): a thread owns 8 consecutive channels (one 16-byte load per pixel) and one run of up to 8 pixels of one
// image row; per pixel it forms d, d cos(w), d sin(w) (3 FMAs per value), the row's cos / sin are applied once per run, and the diagonal bin comes from
// the angle addition formulas:  cos(a + b) = cos a cos b - sin a sin b.  cos / sin of the <= 128 row and column angles are a 2 KB LDS table
// (sincospif: exact at the quarter turns, so H or W of 2 and 4 give exact 0 / +-1).
#include <float.h>
#include <math.h>

#include "af_common.h"

namespace {

constexpr int FU_SEG = 8;          // pixels of one row per thread of the skip role
constexpr int FU_MAX_SIDE = 128;   // H, W <= 128: the LDS table
constexpr int FU_THREADS = 256;
constexpr int FU_RS = 36;          // floats per thread in the statistics kernel's reduction buffer: 4 sums x 8 channels + 4 of padding (16-byte rows)

struct FreeuGeom {
  int ng, lp, pb, nhb, nmm;                         // h role of stats: channel groups, lanes per pixel, pixels per workgroup, workgroups and (lo, hi) partials per sample
  int ngs, segs, units, np, cg, nchunks, nslices;   // skip role: channel groups, runs per row, runs per sample, runs and channel groups per workgroup
  int nv, ppa, nha;                                 // h role of apply: 16-byte vectors per pixel (first C/2 channels), pixels per workgroup, workgroups per sample
  int64_t off_mm, off_piv, off_sum, total;          // workspace (floats): mean [B][HW] at 0, (lo, hi) [B][nmm][2], pivot [B][Cs], sums [B][nslices][7][Cs]
};

inline int64_t r4(int64_t x) { return (x + 3) / 4 * 4; }

FreeuGeom freeu_geom(int B, int H, int W, int C, int Cs) {
  FreeuGeom g;
  const int HW = H * W;
  g.ng = C / 8;
  g.lp = 1;
  while (g.lp < g.ng && g.lp < 64) g.lp <<= 1;
  g.pb = FU_THREADS / g.lp;
  g.nhb = (HW + g.pb - 1) / g.pb;
  g.nmm = g.nhb * (FU_THREADS / 64);
  g.ngs = Cs / 8;
  g.segs = (W + FU_SEG - 1) / FU_SEG;
  g.units = H * g.segs;
  g.np = 1;
  while (g.np < g.units && g.np < 32) g.np <<= 1;
  g.cg = FU_THREADS / g.np;
  g.nchunks = (g.ngs + g.cg - 1) / g.cg;
  g.nslices = (g.units + g.np - 1) / g.np;
  g.nv = C / 16;
  g.ppa = 2048 / g.nv > 1 ? 2048 / g.nv : 1;
  g.nha = (HW + g.ppa - 1) / g.ppa;
  g.off_mm = r4((int64_t)B * HW);
  g.off_piv = g.off_mm + r4((int64_t)B * g.nmm * 2);
  g.off_sum = g.off_piv + r4((int64_t)B * Cs);
  g.total = g.off_sum + (int64_t)B * g.nslices * 7 * Cs;
  return g;
}

struct FreeuArgs {
  const half_t* h;
  const half_t* skip;
  half_t* h_out;
  half_t* skip_out;
  float* ws;
  FreeuGeom g;
  int H, W, C, Cs;
  int nh;             // workgroups of the h role per sample in THIS launch (0: the role is off)
  int version;
  float inv_c;        // 1 / C
  float bm1, b;       // b - 1, b
  float sm1, coef;    // s - 1, (s - 1) / (H W)
};

// cos / sin of 2 pi i / H (rows 0, 1) and 2 pi i / W (rows 2, 3)
__device__ __forceinline__ void fu_fill_table(float (*tab)[FU_MAX_SIDE], int H, int W, int t) {
  for (int i = t; i < H; i += FU_THREADS) {
    float s, c;
    sincospif(2.f * (float)i / (float)H, &s, &c);
    tab[0][i] = c;
    tab[1][i] = s;
  }
  for (int i = t; i < W; i += FU_THREADS) {
    float s, c;
    sincospif(2.f * (float)i / (float)W, &s, &c);
    tab[2][i] = c;
    tab[3][i] = s;
  }
}

// finite values saturate at the fp16 maximum; NaN and Inf pass (comparisons, not fmin / fmax, which would drop a NaN)
__device__ __forceinline__ float fu_sat(float v) {
  v = (v > 65504.f && v < INFINITY) ? 65504.f : v;
  v = (v < -65504.f && v > -INFINITY) ? -65504.f : v;
  return v;
}

// sum k of one run from its three row sums: S0, Ph, Qh, Pw, Qw, Pd, Qd (the diagonal bin by the angle addition formulas)
__device__ __forceinline__ float fu_run_sum(int k, float r0, float rc, float rs, float ch, float sh) {
  switch (k) {
    case 0: return r0;
    case 1: return r0 * ch;
    case 2: return r0 * sh;
    case 3: return rc;
    case 4: return rs;
    case 5: return rc * ch - rs * sh;
    default: return rc * sh + rs * ch;
  }
}

__global__ __launch_bounds__(FU_THREADS) void af_freeu_stats_kernel(FreeuArgs a) {
  __shared__ float tab[4][FU_MAX_SIDE];
  __shared__ __attribute__((aligned(16))) float red[FU_THREADS * FU_RS];
  const int t = threadIdx.x, b = blockIdx.y;
  const int HW = a.H * a.W;
  const FreeuGeom& g = a.g;
  if ((int)blockIdx.x < a.nh) {
    // ---- h role: lp lanes per pixel, 64 / lp pixels per wave; shuffles only
    const int wave = t >> 6, lane = t & 63;
    const int sub = lane & (g.lp - 1), pw = lane / g.lp;
    const int p = blockIdx.x * g.pb + wave * (64 / g.lp) + pw;
    const bool live = p < HW;
    float acc = 0.f;
    if (live) {
      const half_t* row = a.h + ((size_t)b * HW + p) * a.C;
      for (int i = sub; i < g.ng; i += g.lp) {
        const half8_t v = *reinterpret_cast<const half8_t*>(row + i * 8);
        acc += (((float)v[0] + (float)v[1]) + ((float)v[2] + (float)v[3])) + (((float)v[4] + (float)v[5]) + ((float)v[6] + (float)v[7]));
      }
    }
    for (int off = g.lp >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    const float m = acc * a.inv_c;
    if (live && sub == 0) a.ws[(size_t)b * HW + p] = m;
    float lo = live ? m : INFINITY, hi = live ? m : -INFINITY;
    const bool bad = __any(live && m != m);       // a NaN mean makes the sample's lo and hi NaN, as torch's min / max do
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, off, 64));
      hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if (lane == 0) {
      float* mm = a.ws + g.off_mm + ((size_t)b * g.nmm + blockIdx.x * (FU_THREADS / 64) + wave) * 2;
      mm[0] = bad ? NAN : lo;
      mm[1] = bad ? NAN : hi;
    }
    return;
  }
  // ---- skip role
  fu_fill_table(tab, a.H, a.W, t);
  __syncthreads();
  const int sidx = blockIdx.x - a.nh;
  const int chunk = sidx % g.nchunks, slice = sidx / g.nchunks;
  const int gl = t & (g.cg - 1), pl = t / g.cg;
  const int gi = chunk * g.cg + gl, unit = slice * g.np + pl;
  const bool col = gi < g.ngs, live = col && unit < g.units;
  const int row = live ? unit / g.segs : 0, w0 = live ? (unit % g.segs) * FU_SEG : 0;
  const int nw = live ? min(FU_SEG, a.W - w0) : 0;
  float r0[8], rc[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r0[j] = rc[j] = rs[j] = 0.f;
  if (live) {
    const half_t* plane = a.skip + (size_t)b * HW * a.Cs + gi * 8;
    const half8_t pv = *reinterpret_cast<const half8_t*>(plane);
    const half_t* base = plane + ((size_t)row * a.W + w0) * a.Cs;
    half8_t x[FU_SEG];
#pragma unroll
    for (int i = 0; i < FU_SEG; ++i)
      if (i < nw) x[i] = *reinterpret_cast<const half8_t*>(base + (size_t)i * a.Cs);
#pragma unroll
    for (int i = 0; i < FU_SEG; ++i)
      if (i < nw) {
        const float cw = tab[2][w0 + i], sw = tab[3][w0 + i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = (float)x[i][j] - (float)pv[j];
          r0[j] += d;
          rc[j] = fmaf(d, cw, rc[j]);
          rs[j] = fmaf(d, sw, rs[j]);
        }
      }
    if (slice == 0 && pl == 0) {
      float* piv = a.ws + g.off_piv + (size_t)b * a.Cs + gi * 8;
      *reinterpret_cast<float4*>(piv) = make_float4((float)pv[0], (float)pv[1], (float)pv[2], (float)pv[3]);
      *reinterpret_cast<float4*>(piv + 4) = make_float4((float)pv[4], (float)pv[5], (float)pv[6], (float)pv[7]);
    }
  }
  const float ch = tab[0][row], sh = tab[1][row];
  // the seven sums of this run, reduced over the workgroup's np runs in run order through LDS in two rounds (sums 0 .. 3, then 4 .. 6): every
  // thread stores its values, then thread o adds ONE (channel group, sum, channel) over the runs -- consecutive threads read consecutive words
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int k0 = half * 4, nk = half ? 3 : 4;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      if (kk < nk) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fu_run_sum(k0 + kk, r0[j], rc[j], rs[j], ch, sh);
        *reinterpret_cast<float4*>(&red[t * FU_RS + kk * 8]) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(&red[t * FU_RS + kk * 8 + 4]) = make_float4(v[4], v[5], v[6], v[7]);
      }
    __syncthreads();
    const int per = nk * 8, nout = g.cg * per;
    for (int o = t; o < nout; o += FU_THREADS) {
      const int glo = o / per, kj = o - glo * per;
      const int gio = chunk * g.cg + glo;
      if (gio < g.ngs) {
        float acc = red[glo * FU_RS + kj];
        for (int q = 1; q < g.np; ++q) acc += red[(q * g.cg + glo) * FU_RS + kj];
        a.ws[g.off_sum + (((size_t)b * g.nslices + slice) * 7 + k0 + (kj >> 3)) * a.Cs + gio * 8 + (kj & 7)] = acc;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(FU_THREADS) void af_freeu_apply_kernel(FreeuArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, b = blockIdx.y;
  const int HW = a.H * a.W;
  const FreeuGeom& g = a.g;
  if ((int)blockIdx.x < a.nh) {
    // ---- h role: h_out[:, :C/2] = sat(h * f)
    float lo = 0.f, hi = 0.f;
    if (a.version == 2) {
      float* wred = reinterpret_cast<float*>(smem);      // [4 waves][lo, hi, bad]
      const float* mm = a.ws + g.off_mm + (size_t)b * g.nmm * 2;
      lo = INFINITY, hi = -INFINITY;
      bool bad = false;
      for (int i = t; i < g.nmm; i += FU_THREADS) {
        const float x = mm[2 * i], y = mm[2 * i + 1];
        bad |= x != x || y != y;
        lo = fminf(lo, x);
        hi = fmaxf(hi, y);
      }
      bad = __any(bad);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
      }
      if ((t & 63) == 0) {
        wred[(t >> 6) * 3] = lo;
        wred[(t >> 6) * 3 + 1] = hi;
        wred[(t >> 6) * 3 + 2] = bad ? 1.f : 0.f;
      }
      __syncthreads();
      lo = fminf(fminf(wred[0], wred[3]), fminf(wred[6], wred[9]));
      hi = fmaxf(fmaxf(wred[1], wred[4]), fmaxf(wred[7], wred[10]));
      if (wred[2] + wred[5] + wred[8] + wred[11] != 0.f) lo = hi = NAN;
    }
    const float rng = hi - lo;
    const int p0 = blockIdx.x * g.ppa;
    const int items = min(g.ppa, HW - p0) * g.nv;
    const float* mean = a.ws + (size_t)b * HW;
#pragma unroll 4
    for (int i = t; i < items; i += FU_THREADS) {
      const int p = p0 + i / g.nv, v = i % g.nv;
      float f = a.b;
      if (a.version == 2) {
        const float mh = hi == lo ? 0.f : (mean[p] - lo) / rng;     // NaN lo / hi compare unequal: the factor is NaN
        f = fmaf(a.bm1, mh, 1.f);
      }
      const size_t off = ((size_t)b * HW + p) * a.C + v * 8;
      const half8_t x = *reinterpret_cast<const half8_t*>(a.h + off);
      half8_t y;
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = (half_t)fu_sat((float)x[j] * f);
      *reinterpret_cast<half8_t*>(a.h_out + off) = y;
    }
    return;
  }
  // ---- skip role: skip_out = sat(skip + (s - 1) / (HW) * low)
  float(*tab)[FU_MAX_SIDE] = reinterpret_cast<float(*)[FU_MAX_SIDE]>(smem);
  float4* comb = reinterpret_cast<float4*>(smem + 4 * FU_MAX_SIDE * sizeof(float));      // [cg][7 sums][2]
  fu_fill_table(tab, a.H, a.W, t);
  const int sidx = blockIdx.x - a.nh;
  const int chunk = sidx % g.nchunks, slice = sidx / g.nchunks;
  const int gl = t & (g.cg - 1), pl = t / g.cg;
  const int gi = chunk * g.cg + gl, unit = slice * g.np + pl;
  const bool col = gi < g.ngs, live = col && unit < g.units;
  // the slices' partial sums, added in slice order; the workgroup's np run lanes share the 14 float4 of a channel group
  if (col) {
    const float* src = a.ws + g.off_sum + (size_t)b * g.nslices * 7 * a.Cs + gi * 8;
    for (int q = pl; q < 14; q += g.np) {
      const float* s = src + (size_t)(q >> 1) * a.Cs + (q & 1) * 4;
      float4 acc = *reinterpret_cast<const float4*>(s);
      for (int sl = 1; sl < g.nslices; ++sl) {
        const float4 u = *reinterpret_cast<const float4*>(s + (size_t)sl * 7 * a.Cs);
        acc.x += u.x, acc.y += u.y, acc.z += u.z, acc.w += u.w;
      }
      comb[gl * 14 + q] = acc;
    }
  }
  __syncthreads();
  if (!live) return;
  const int row = unit / g.segs, w0 = (unit % g.segs) * FU_SEG;
  const int nw = min(FU_SEG, a.W - w0);
  const float eh = a.H > 1 ? 1.f : 0.f, ew = a.W > 1 ? 1.f : 0.f;     // a side of 1 has the one bin 0
  const float ch = tab[0][row] * eh, sh = tab[1][row] * eh;
  float S[7][8];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const float4 u0 = comb[gl * 14 + 2 * k], u1 = comb[gl * 14 + 2 * k + 1];
    S[k][0] = u0.x, S[k][1] = u0.y, S[k][2] = u0.z, S[k][3] = u0.w;
    S[k][4] = u1.x, S[k][5] = u1.y, S[k][6] = u1.z, S[k][7] = u1.w;
  }
  const float* piv = a.ws + g.off_piv + (size_t)b * a.Cs + gi * 8;
  const float4 p0 = *reinterpret_cast<const float4*>(piv), p1 = *reinterpret_cast<const float4*>(piv + 4);
  const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
  float T0[8], T1[8], T2[8];
  const float cw_scale = a.coef * ew;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // low = [S0 + Ph ch + Qh sh] + cos(w) [Pw + Pd ch + Qd sh] + sin(w) [Qw + Qd ch - Pd sh];  sum x = HW pivot + S0
    T0[j] = fmaf(a.sm1, pv[j], a.coef * (S[0][j] + (S[1][j] * ch + S[2][j] * sh)));
    T1[j] = cw_scale * (S[3][j] + (S[5][j] * ch + S[6][j] * sh));
    T2[j] = cw_scale * (S[4][j] + (S[6][j] * ch - S[5][j] * sh));
    if (!(fabsf(S[0][j]) <= FLT_MAX)) T0[j] = NAN;      // a plane that holds a NaN or an Inf is NaN everywhere, as its DFT is
  }
  const size_t base = ((size_t)b * HW + (size_t)row * a.W + w0) * a.Cs + gi * 8;
  half8_t x[FU_SEG];
#pragma unroll
  for (int i = 0; i < FU_SEG; ++i)
    if (i < nw) x[i] = *reinterpret_cast<const half8_t*>(a.skip + base + (size_t)i * a.Cs);
#pragma unroll
  for (int i = 0; i < FU_SEG; ++i)
    if (i < nw) {
      const float cw = tab[2][w0 + i], sw = tab[3][w0 + i];
      half8_t y;
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = (half_t)fu_sat((float)x[i][j] + fmaf(cw, T1[j], fmaf(sw, T2[j], T0[j])));
      *reinterpret_cast<half8_t*>(a.skip_out + base + (size_t)i * a.Cs) = y;
    }
}

// Everything both entry points refuse; fills the launch arguments.
int freeu_check(const char* fn, const void* h, const void* skip, const void* ws, int64_t ws_floats, int B, int H, int W, int C, int Cs, float b, float s,
                int version, FreeuArgs& a) {
  const std::string f(fn);
  AF_REQUIRE(h && skip && ws, f + ": null pointer");
  AF_REQUIRE(B >= 1 && B <= 65535, f + ": 1 <= B <= 65535");
  AF_REQUIRE(H >= 1 && H <= FU_MAX_SIDE && W >= 1 && W <= FU_MAX_SIDE, f + ": 1 <= H, W <= 128");
  AF_REQUIRE(C >= 16 && C % 16 == 0 && C <= 16384, f + ": C must be a multiple of 16 in 16 .. 16384");
  AF_REQUIRE(Cs >= 8 && Cs % 8 == 0 && Cs <= 16384, f + ": Cs must be a multiple of 8 in 8 .. 16384");
  AF_REQUIRE(version == 1 || version == 2, f + ": version must be 1 or 2");
  AF_REQUIRE(b >= 0.f && b <= FLT_MAX && s >= 0.f && s <= FLT_MAX, f + ": b and s must be finite and >= 0");
  const int64_t lim = (int64_t)1 << 31, px = (int64_t)B * H * W;
  AF_REQUIRE(px * C < lim && px * Cs < lim, f + ": a tensor of 2^31 elements or more");
  AF_REQUIRE(((uintptr_t)h | (uintptr_t)skip | (uintptr_t)ws) % 16 == 0, f + ": operands must be 16-byte aligned");
  a.g = freeu_geom(B, H, W, C, Cs);
  AF_REQUIRE(ws_floats >= a.g.total, f + ": the workspace is smaller than af_freeu_ws_floats");
  a.h = (const half_t*)h;
  a.skip = (const half_t*)skip;
  a.h_out = nullptr;
  a.skip_out = nullptr;
  a.ws = (float*)ws;
  a.H = H;
  a.W = W;
  a.C = C;
  a.Cs = Cs;
  a.nh = 0;
  a.version = version;
  a.inv_c = 1.f / (float)C;
  a.b = b;
  a.bm1 = b - 1.f;
  a.sm1 = s - 1.f;
  a.coef = (s - 1.f) / (float)(H * W);
  return AF_OK;
}

}  // namespace

extern "C" int64_t af_freeu_ws_floats(int B, int H, int W, int C, int Cs) {
  if (B < 1 || B > 65535 || H < 1 || H > FU_MAX_SIDE || W < 1 || W > FU_MAX_SIDE || C < 16 || C % 16 || C > 16384 || Cs < 8 || Cs % 8 || Cs > 16384)
    return af_fail(AF_E_BADARG, "af_freeu_ws_floats: a size outside what af_freeu_stats takes");
  return freeu_geom(B, H, W, C, Cs).total;
}

extern "C" int af_freeu_stats(const void* h, const void* skip, void* ws, int64_t ws_floats, int B, int H, int W, int C, int Cs, float b, float s,
                              int version, void* stream) {
  FreeuArgs a;
  const int rc = freeu_check("af_freeu_stats", h, skip, ws, ws_floats, B, H, W, C, Cs, b, s, version, a);
  if (rc != AF_OK) return rc;
  const bool do_h = version == 2 && b != 1.f, do_s = s != 1.f;
  if (!do_h && !do_s) return AF_OK;
  a.nh = do_h ? a.g.nhb : 0;
  const int ns = do_s ? a.g.nchunks * a.g.nslices : 0;
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(af_freeu_stats_kernel, dim3(a.nh + ns, B), dim3(FU_THREADS), 0, (hipStream_t)stream, a);
  return af_check_launch("af_freeu_stats");
}

extern "C" int af_freeu_apply(const void* h, const void* skip, const void* ws, int64_t ws_floats, void* h_out, void* skip_out, int B, int H, int W,
                              int C, int Cs, float b, float s, int version, void* stream) {
  FreeuArgs a;
  const int rc = freeu_check("af_freeu_apply", h, skip, ws, ws_floats, B, H, W, C, Cs, b, s, version, a);
  if (rc != AF_OK) return rc;
  AF_REQUIRE(h_out && skip_out, "af_freeu_apply: null pointer");
  AF_REQUIRE(((uintptr_t)h_out | (uintptr_t)skip_out) % 16 == 0, "af_freeu_apply: operands must be 16-byte aligned");
  a.h_out = (half_t*)h_out;
  a.skip_out = (half_t*)skip_out;
  const bool do_h = b != 1.f, do_s = s != 1.f;
  if (!do_h && !do_s) return AF_OK;
  a.nh = do_h ? a.g.nha : 0;
  const int ns = do_s ? a.g.nchunks * a.g.nslices : 0;
  const size_t lds = 4 * FU_MAX_SIDE * sizeof(float) + (size_t)a.g.cg * 14 * sizeof(float4);      // <= 59392 bytes (cg = 256 at 1 x 1)
  AfLaunchScope scope(AF_FAM_ELEM, stream);
  hipLaunchKernelGGL(af_freeu_apply_kernel, dim3(a.nh + ns, B), dim3(FU_THREADS), lds, (hipStream_t)stream, a);
  return af_check_launch("af_freeu_apply");
}
