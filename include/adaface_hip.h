/*
 * adaface_hip.h -- C ABI of libadaface_hip.so: the MI355X (gfx950) kernels of AdaFace's
 * denoising hot path (SD-1.5 U-Net epsilon-prediction).
 *
 * The reference (askerlee/AdaFace-dev) has no FFI layer: its seams are Python call
 * signatures that bottom out in torch ops.  Each entry point below names the reference
 * call site(s) (file:line relative to the reference tree) whose arithmetic it replaces;
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch); the library
 *     allocates nothing and keeps no global mutable state (re-entrant: forward thread and
 *     autograd thread may call concurrently);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     no call synchronises, so every call is hipGraph-capturable;
 *   - activations are fp16 ("h"), NHWC / token-major [rows, channels]; accumulation,
 *     statistics and softmax are fp32;
 *   - return value: 0 = ok, <0 = AF_E_* ; af_last_error() gives the message (thread-local).
 */
#ifndef ADAFACE_HIP_H
#define ADAFACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AF_OK 0
#define AF_E_BADARG (-1)      /* null pointer, negative size, misaligned dimension   */
#define AF_E_UNSUPPORTED (-2) /* shape outside what the kernels are built for        */
#define AF_E_HIP (-3)         /* launch failed; message holds hipGetErrorString      */

const char* af_last_error(void);
int af_version(void);
/* number of HIP devices visible, or AF_E_HIP (used by smoke tests; does not create a context) */
int af_device_count(void);

/* ---- profiling hook (bench.py roofline leg): when enabled, every launch of the kernel
 * family `family` is bracketed by hipEvents on its own stream; af_prof_read synchronises
 * those events and returns the launch count and summed milliseconds since the last reset. */
#define AF_FAM_GEMM 0   /* conv3x3 implicit-GEMM + linear/conv1x1 (one kernel template) */
#define AF_FAM_ATTN 1
#define AF_FAM_GNORM 2
#define AF_FAM_LNORM 3
#define AF_FAM_ELEM 4
#define AF_FAM_XATTN 5  /* af_attention launches with fewer keys than queries: the U-Net's cross-attention cores */
#define AF_FAM_COUNT 6
int af_prof_enable(int on);
int af_prof_reset(void);
int af_prof_read(int family, int* launches, double* total_ms);

/* ---- GEMM / implicit-GEMM convolution -------------------------------------------------
 * out[M,N] = epilogue( sum_k A[m,k] * Wt[n,k] )          (Wt is [Npad, Kpad], K contiguous)
 * Replaces: nn.Conv2d 3x3 / 1x1 (ldm/modules/diffusionmodules/util.py:214-224, called at
 * openaimodel.py:202-242,108,152,523,689; attention.py:269,280) and nn.Linear
 * (attention.py:34,54,156-162; openaimodel.py:511-515,221).
 *
 * A operand (activations, fp16):
 *   taps == 1 : plain rows.  k <  k1 reads a1[m*lda1 + k], k >= k1 reads a2[m*lda2 + (k-k1)]
 *               (a2 may be NULL when k1 == K): fuses torch.cat([h, skip], 1) (openaimodel.py:918).
 *   taps == 9 : 3x3, pad 1, implicit im2col over an NHWC image [B, H, W, c1 (+c2)]:
 *               k = tap*(c1+c2) + c ; stride 1|2 (Downsample, openaimodel.py:150-161);
 *               upsample=1 reads the nearest-x2 upsampled image without materialising it
 *               (Upsample, openaimodel.py:117-119); upsample=2 reads the ZERO-INSERTED x2 image of size
 *               Ho x Wo (data at even positions): with flipped/transposed weights this is the input
 *               gradient of the stride-2 convolution.  M = B*Ho*Wo.
 * Epilogue (fp32): + bias[n] ; + rowbias[(m / rows_per_batch)*ld_rowbias + n] (ResBlock time
 *   embedding add, openaimodel.py:265-274) ; act ; + residual[m*N + n] ; -> fp16.
 *   act: AF_ACT_NONE | AF_ACT_SILU | AF_ACT_GEGLU (Wt rows interleaved [16 x | 16 gate],
 *   out has N/2 columns: a * gelu_erf(g), attention.py:36-38).
 *   out_mode AF_OUT_SPLIT_T: columns n >= split_col are written TRANSPOSED to out2
 *   ([B, N - split_col, ld_out2] with token index contiguous): V^T for the attention kernel.
 *   out_mode AF_OUT_F32: out is fp32 [M][ld_out] -- the accumulator is stored without the fp16 cast (weight gradients: sums over
 *   thousands of tokens overflow fp16 long before they lose precision).  Standard epilogue only, N % 4 == 0, no splitk_fused.
 *   With split-K the reduce pass writes fp32; unsplit, tiles 1 / 2 do (tiles 3 .. 10 fall back to tile 1).
 */
#define AF_ACT_NONE 0
#define AF_ACT_SILU 1
#define AF_ACT_GEGLU 2
#define AF_ACT_QUICKGELU 3 /* x * sigmoid(1.702 x): CLIP text MLP (transformers QuickGELUActivation) */
#define AF_OUT_NORMAL 0
#define AF_OUT_SPLIT_T 1
#define AF_OUT_F32 2

typedef struct af_gemm_desc {
  const void* a1;       /* fp16 */
  const void* a2;       /* fp16 or NULL */
  const void* wt;       /* fp16 [Npad][Kpad], Npad % 128 == 0, Kpad % 64 == 0, zero padded */
  const void* bias;     /* fp32 [N] or NULL */
  const void* rowbias;  /* fp16 [B][ld_rowbias] or NULL */
  const void* residual; /* fp16 [M][N] or NULL */
  void* out;            /* fp16 [M][ld_out] (fp32 with AF_OUT_F32) */
  void* out2;           /* fp16, AF_OUT_SPLIT_T only */
  int32_t M, N, K;      /* logical sizes (K = taps*(c1+c2) for taps == 9) */
  int32_t kpad;         /* row stride of wt in elements */
  int32_t taps;         /* 1 or 9 */
  int32_t c1, c2;       /* channels of a1 / a2 (taps==1: k1 = c1, k2 = c2) */
  int32_t lda1, lda2;   /* taps==1 row strides in elements */
  int32_t B, H, W;      /* taps==9 input image (before upsample) */
  int32_t Ho, Wo;       /* taps==9 output image */
  int32_t stride;       /* 1 | 2 */
  int32_t upsample;     /* 0 | 1 (nearest x2) | 2 (zero-insert x2) | 3 (nearest x2 in PHASE form: the four output parities (py, px) as four 2x2
                           convolutions of the low-res image.  wt = the phase pack [4 N][kpad], rows phase-major (phase = 2 py + px), K = 4 c1 in
                           (a, b, cin) order, weight (a, b) of a phase = the sum of the 3x3 weights whose taps read low-res offset
                           (py - 1 + a, px - 1 + b); bias stays [N]; H, W = the low-res image, Ho = 2 H, Wo = 2 W, M = B Ho Wo, taps = 9.
                           Runs on tile 14 inside af_gemm_halo_variant's scope (answer 4) only; AF_E_UNSUPPORTED anywhere else) */
  int32_t rows_per_batch;
  int32_t ld_rowbias;
  int32_t act;
  int32_t out_mode;
  int32_t ld_out;       /* elements; 0 -> N (or N/2 for GEGLU) */
  int32_t split_col;    /* AF_OUT_SPLIT_T */
  int32_t ld_out2;      /* AF_OUT_SPLIT_T: tokens per batch item rounded up to 8 */
  int32_t tile;         /* 0 = auto (1 or 2), 1 = 128x128, 2 = 64x64 (register-staged), 3 = 128x128 and 4 = 128x320 LDS-DMA
                           pipelined ring (standard epilogue, channel counts % 32 == 0, no upsample, tile 4: N % 320
                           == 0; otherwise falls back to 1) */
                        /* 5 = 256x256 and 6 = 256x320 ring tiles (8 waves as 4 x 2): plain or GEGLU 1x1 GEMMs only, N % 256 / N % 320 == 0,
                           no split-K */
                        /* 7 .. 10 = whole-line kernel (64-wide K stages, LDS-DMA pieces of 8 rows x one 128-byte line, two slots; channel
                           counts and K padding multiples of 64): 7 = 128x320 (GEGLU 128x256, transposed-V split), 8 = 128x128 (4 waves; also GEGLU,
                           transposed-V split), 9 / 10 = GEGLU 256x320 / 256x256; tiles 7 and 8 also take upsample = 1 (nearest x2).  Anything outside a tile's scope falls back to tile 1 */
                        /* 11 = whole-line kernel, 128x160 tile of four waves (N % 160 == 0; standard epilogue, taps 1 / 9, nearest x2): 74 KB of
                           LDS, so TWO workgroups share a CU and one's epilogue / barrier waits run under the other's MFMAs: the faster
                           form when the 128x320 grid has under ~1.5 workgroups per CU (batch 1 - 4 passes, the 32x32 level) */
                        /* 12 / 13 = the 128x128 / 128x160 whole-line tiles with a FOUR-slot ring: three K stages in flight ahead of the MFMAs
                           instead of one (128 / 147 KB of LDS, one workgroup per CU): for grids of at most ~one workgroup per CU, where
                           nothing else covers a stage's L2 / HBM latency (the 16x16 level: weights read once, 160 tiles) */
                        /* 14 = halo-resident 3x3 kernel: 256 output pixels (whole image rows) x 160 channels per workgroup; per 64 input
                           channels the rows' (R+2) x (W+2) halo is loaded into LDS once and the nine taps read it at shifted addresses
                           (stride 1, pad 1, c1 % 64 == 0, c2 % 64 == 0 -- one or two channel-concatenated sources --, no K tail, N % 160 == 0,
                           Wo in {8, 16, 32, 64}, a tile = 256 / Wo whole rows of one image or whole images (the 8 x 8 level), upsample 0 / 1; split-K over 64-channel chunks of c1 + c2).  Main loop: ping-pong between the two
                           waves of a SIMD (one group issues a stage's 40 MFMAs while the other reads its fragments and issues its LDS-DMA
                           pieces; 160 KB of LDS).  Round 6: every per-stage address (fragment reads per tap, LDS-DMA pieces) is a register or a scalar +
                           immediate computed outside the loop, out-of-image halo lanes are EXEC-masked instead of reading a zero page (~10 instead of
                           ~80 vector instructions per 40-MFMA stage).  Also round 6, for the VAE's channel counts and image sizes (model.py:136-175, 536-567): where N is
                           a 128-multiple but no 160-multiple the tile is 256 x 128 (no K tail), and on images wider than 64 pixels (Wo % 16 == 0, Ho % 16 == 0; never
                           split) a tile is a 16 x 16-pixel PATCH of one image (18 x 18 halo) instead of whole rows.  af_gemm_halo_variant tells which form a
                           descriptor gets.  Outside that scope it falls back to tile 1 */
                        /* 19 = tile 14 with its round-5 main loop (addresses recomputed per stage): the A/B arm; bit-identical results */
                        /* 15 = whole-line kernel, 256 x 128 tile of eight waves (4 x 2; N % 128 == 0; standard epilogue, taps 1 / 9, nearest x2): 85 instead of
                           64 FLOP per operand byte for narrow outputs over many rows (the VAE decoder's 128- / 256-channel convolutions at 256^2 / 512^2) */
                        /* 16 / 17 = whole-line kernel, 64 x 128 / 128 x 64 tile of four waves (1 x 4 / 2 x 2; N % 128 / 64 == 0; standard and transposed-V-split epilogues, folded
                           LayerNorm, taps 1 / 9, no nearest x2, no K tail): 25 KB stages, so THREE workgroups share a CU -- a short-K GEMM's K step is a
                           memory round trip, and what hides it is the other workgroups' MFMAs, not a deeper ring */
                        /* 18 = SMALL plain GEMMs with their MFMA fragments straight from global memory (both operands are K-contiguous: a fragment is one 16-byte
                           load per lane), 32 x 64 outputs per workgroup, no LDS, no barrier, several K steps of fragments in flight, never split: the training
                           legs' GEMMs of a few hundred rows, which on tile 2 are chains of K / 64 dependent stages (+ a split-K reduce launch).  taps 1, one
                           source, standard epilogue, fp16 or fp32 output, K % 8 == 0, 16-byte aligned rows; outside that scope it falls back to tile 2 */
  int32_t splits;       /* split-K factor (<=1: none).  >1 needs the standard epilogue and a workspace:
                           each split writes an fp32 partial [M][N], a second launch reduces + applies the epilogue */
  void* workspace;      /* fp32, >= splits*M*N*4 bytes when splits > 1 */
  int64_t workspace_bytes;
  const void* zeros;    /* >= 16 bytes of zeros, 16-byte aligned: source of halo / out-of-range lanes (tile 3) */
  int32_t tap_shift;    /* 3x3 only: 0 = padding 1 on every side; 1 = taps shifted by +1 pixel, i.e. padding (0, 1, 0, 1) as the VAE
                           encoder's Downsample pads before its stride-2 conv (ldm/modules/diffusionmodules/model.py:73-77) */
  int32_t splitk_fused; /* split-K only: 1 = reduce inside the GEMM launch (tiles 3 .. 10, at most AF_SPLITK_MAX_TILES output tiles; otherwise the
                           two-launch form is used).  The LAST AF_SPLITK_COUNTER_BYTES of the workspace are then per-tile arrival counters:
                           the caller zeroes them once when it allocates the workspace, every launch leaves them zero.  The partial slabs
                           must fit in the first workspace_bytes - AF_SPLITK_COUNTER_BYTES bytes.  Results are bit-identical to the
                           two-launch form (slices are summed in slice order by the last-arriving workgroup of each tile) */
  const void* ln_colsum; /* fp32 [Npad] or NULL.  Non-NULL = LayerNorm folded into this GEMM (BasicTransformerBlock.norm1/2/3 in front of
                           attn1 q|k|v, attn2.to_q and the GEGLU projection, attention.py:242-252): a1 holds the UN-normalised rows, wt holds
                           fp16(gamma * W), bias holds b + W beta, ln_colsum[n] = sum_k wt[n][k] (of the fp16 values), and the epilogue
                           computes rstd_m * (acc - mean_m * ln_colsum[n]) + bias[n] with the row statistics (mean, biased variance over the
                           K = c1 columns, eps = ln_eps) accumulated from the A fragments inside the main loop.  Whole-line tiles (7 .. 13)
                           only, taps == 1, c2 == 0, no split-K; anything else is AF_E_UNSUPPORTED */
  float ln_eps;
  /* K-concatenated 1x1 tail of a 3x3 convolution (taps == 9 only; all NULL / 0 otherwise): behind the nine tap blocks K continues with c3 (+ c4)
   * PLAIN columns read from a3 [M][lda3] (| a4 [M][lda4]) at the OUTPUT pixel's row, K = 9 (c1 + c2) + c3 + c4 -- out = conv3x3(a1 | a2) + conv1x1(a3 | a4)
   * in one launch: the ResBlock's out_layers convolution and its channel-changing skip_connection (openaimodel.py:256-276; wt = [3x3 weights in
   * (ky, kx, cin) order | 1x1 weights], bias = the two biases added up).  stride 1, no upsample, no tap_shift, c3 / c4 multiples of 64, whole-line
   * tiles 7 .. 13 only (AF_E_UNSUPPORTED otherwise: the caller keeps the two-launch form for such shapes). */
  const void* a3;
  const void* a4;
  int32_t c3, c4, lda3, lda4;
  /* GroupNorm statistics of the OUTPUT from the producing GEMM's epilogue (all 0 / NULL otherwise): gn_partials != NULL makes the launch also write,
   * per (batch item b, 128-row tile blk of that item, group g of gn_cpg output channels), the partial (sum, M2) of the fp16 values it stores -- M2 = the sum of
   * squares about THAT BLOCK'S OWN MEAN; the consumer merges blocks pairwise (M2_a + M2_b + (mean_b - mean_a)^2 n_a n_b / (n_a + n_b)), so no
   * E[x^2] - mean^2 difference is ever formed and groups with |mean| >> sigma keep their variance (torch's fp32 group_norm, util.py:195-212, is the
   * reference) -- as fp32 [B][128][32][2]: exactly the partial workspace of af_groupnorm, so af_groupnorm_apply can normalise the tensor without a
   * statistics pass of its own (GroupNorm32 behind a convolution: openaimodel.py:202-233, 256-276; attention.py:283-291).  Needs the standard
   * epilogue on a whole-line tile whose width is a multiple of gn_cpg (tile 7: 128 x 320, tile 11 / 13: 128 x 160), gn_cpg even, N % gn_cpg == 0,
   * N / gn_cpg <= 32, rows_per_batch % 128 == 0 (or M % 128 == 0 when rows_per_batch is 0), rows_per_batch / 128 <= 128, fp16 output, no split-K;
   * anything else is AF_E_UNSUPPORTED (callers check af_gemm_gn_stats_ok first). */
  void* gn_partials;
  int32_t gn_cpg;
} af_gemm_desc;
#define AF_SPLITK_MAX_TILES 4096
#define AF_SPLITK_COUNTER_BYTES (AF_SPLITK_MAX_TILES * 4)

int af_gemm(const af_gemm_desc* d, void* stream);

/* ---- fused feed-forward of a transformer block at C = 320 ------------------------------------------------
 * Replaces, in ONE launch, BasicTransformerBlock's  x + ff(norm3(x))  (attention.py:31-58 FeedForward / GEGLU, :242-252) at the
 * 64 x 64 level of SD-1.5:  out = residual + b2 + W2 (v * gelu_erf(g)),  [v | g] = W1 LN(x) + b1, without the [M, inner]
 * intermediate ever leaving the compute unit.  x / residual / out: fp16 [M, C] (C = 320); w1: fp16 packed GEGLU-interleaved
 * [2 * inner][kpad1] with the LayerNorm's gamma folded in, b1 fp32 [2 * inner] (interleaved, + W1 beta), ln_colsum fp32 [2 * inner]
 * column sums of the packed rows (NULL: no LayerNorm in front); w2: fp16 packed [>= C rows][kpad2], b2 fp32 [C] (may be NULL);
 * zeros as af_gemm_desc.zeros.  AF_E_UNSUPPORTED for any other C.                                                              */
int af_ff_fused(const void* x, const void* w1, const void* b1, const void* ln_colsum, float ln_eps, int kpad1, const void* w2, const void* b2,
                int kpad2, const void* residual, void* out, int M, int C, int inner, const void* zeros, void* stream);
/* The same feed-forward with the SpatialTransformer's proj_out + residual behind it (round 6; attention.py:287-304: x = proj_out(blocks(...)) + x_in), one launch:
 *     x3  = residual + b2 + W2 (v * gelu_erf(g))        (af_ff_fused's result: here it never leaves the compute unit)
 *     out = x_in + bp + Wp x3
 * wp: fp16 packed [>= C rows][kpad_p], bp fp32 [C] (may be NULL), x_in fp16 [M, C].  gn_partials (may be NULL): the GroupNorm partial statistics of `out` as
 * af_gemm_desc.gn_partials leaves them, [M / rows_per_batch][128][32][2] floats, groups of gn_cpg channels, rows_per_batch a multiple of 128 (at most 128 blocks).
 * C = 320 only (AF_E_UNSUPPORTED otherwise); out / residual / x_in / b2 / bp 16-byte aligned. */
int af_ff_chain(const void* x, const void* w1, const void* b1, const void* ln_colsum, float ln_eps, int kpad1, const void* w2, const void* b2, int kpad2,
                const void* residual, const void* wp, const void* bp, int kpad_p, const void* x_in, void* out, void* gn_partials, int gn_cpg,
                int rows_per_batch, int M, int C, int inner, const void* zeros, void* stream);

/* Whole cross-attention block of a transformer layer at C = 320, 8 heads (the 64 x 64 level of SD-1.5) in ONE launch (replaces
 * attention.py:168-222 + the norm2 of :242-252): out = residual + bo + Wo . concat_h(softmax(q_h K_h^T scale) V_h), q = LN(x) Wq^T.
 * wq / bq / ln_colsum: the q projection packed with the LayerNorm folded in (as af_gemm_desc.ln_colsum takes it; ln_colsum NULL = x is
 * used as it is, bq NULL = no shift).  k [B * L][ldk] and vt [B][C][ldv] (batch stride vt_batch_stride; the row pad, keys L .. ldv-1, may hold ANYTHING: masked keys contribute nothing) are this
 * layer's slices of the context projection (head h at columns / rows 40 h ..).  N (tokens per image) % 128 == 0, L <= 80.
 * Round 6: C = 640 (8 heads of 80, the 32 x 32 level; N % 64 == 0) is taken too -- 64-token workgroups that stream both 640 x 640 weights; measured slower than
 * three launches there, so the module keeps it behind AF_FUSE_XATTN640.  Any other C: AF_E_UNSUPPORTED. */
int af_xattn_fused(const void* x, const void* wq, const void* bq, const void* ln_colsum, float ln_eps, int kpad_q, const void* k, int ldk,
                   const void* vt, int64_t vt_batch_stride, int ldv, const void* wo, const void* bo, int kpad_o, const void* residual,
                   void* out, int B, int N, int L, int C, int heads, float scale, const void* zeros, void* stream);

/* The same block with the SELF-attention's output projection chained in front (round 6; attention.py:242-252: x = attn1(norm1(x)) + x; x = attn2(norm2(x),
 * context) + x): x1 = ao W1^T + b1 + x0 is formed by the launch itself -- ao [B * N][C] the self-attention core's output, w1 / b1 attn1.to_out packed as for
 * af_gemm, x0 the transformer block's input -- written to the caller's scratch x1 [B * N][C] (a buffer of its own) and used as the cross-attention's
 * input AND residual; out = x1 + bo + Wo . attention(LN(x1) Wq^T, K, V).  One `[B * N, 320] x [320, 320]` launch and three passes over that tensor
 * less per transformer block.  The other arguments as af_xattn_fused. */
int af_xattn_chain(const void* ao, const void* w1, const void* b1, int kpad_1, const void* x0, void* x1, const void* wq, const void* bq,
                   const void* ln_colsum, float ln_eps, int kpad_q, const void* k, int ldk, const void* vt, int64_t vt_batch_stride, int ldv,
                   const void* wo, const void* bo, int kpad_o, void* out, int B, int N, int L, int C, int heads, float scale, const void* zeros,
                   void* stream);

/* PADDED LEADING DIMENSIONS -- the contract for every entry point that takes an ld larger than the logical extent (k / q rows wider than heads*d,
 * vt rows of ldv >= L keys, keybias rows of ldb >= L, out2 rows of ld_out2 >= rows_per_batch): a consumer NEVER lets bytes outside the logical
 * extent reach a result -- they may be uninitialised memory (NaN, Inf) -- and a producer that owns a padded output row (af_gemm's AF_OUT_SPLIT_T
 * out2, af_transpose_tokens) writes zeros into the pad.  Packed weights (wt) are different: the caller zero-pads them to [npad][kpad] when packing,
 * and the kernels rely on that.  tests/conftest.py runs every GPU test with NaN-filled torch.empty buffers to hold this.                        */

/* GroupNorm(32) of a single-source tensor whose partial statistics already exist (af_gemm_desc.gn_partials) + the 1x1 convolution behind it at C = 320
 * in ONE launch: out [B*HW][320] = GroupNorm(x) W^T + bias -- the SpatialTransformer's proj_in(norm(x)) (attention.py:283-291); the normalised
 * tensor never exists in memory.  partials fp32 [B][128][32][2], nblk = HW / 128 valid blocks per batch item; w packed as for af_gemm
 * ([>= 320][kpad]).  HW % 128 == 0.  AF_E_UNSUPPORTED for any other C / group count. */
int af_gn_proj_fused(const void* x, const void* partials, int nblk, const void* gamma, const void* beta, float eps, const void* w, const void* bias,
                     int kpad, void* out, int B, int HW, int C, int groups, const void* zeros, void* stream);

/* ---- GroupNorm(32) [+ SiLU], NHWC -----------------------------------------------------
 * Replaces GroupNorm32 + nn.SiLU (util.py:195-212; openaimodel.py:202-233,686-690; eps 1e-5)
 * and Normalize (attention.py:70-71; eps 1e-6).  x = concat(x1[.., c1], x2[.., c2]) along
 * channels (x2 may be NULL).  Two launches: partial sums -> normalise.
 * workspace: fp32, at least af_groupnorm_ws_floats(B) floats.  x1 / x2 / y / gamma / beta must
 * be 16-byte aligned (vector accesses); AF_E_BADARG otherwise.                              */
int af_groupnorm_ws_floats(int B);
/* GroupNorm(32) [+ SiLU] of a single-source tensor whose partial statistics already exist (af_gemm_desc.gn_partials of the launch that produced x):
 * partials fp32 [B][128][32][2] with nblk valid blocks per batch item; one launch (the normalising pass of af_groupnorm).  stats (optional) as
 * af_groupnorm_stats. */
int af_groupnorm_apply(const void* x, int C, const void* gamma, const void* beta, void* y, void* stats, int B, int HW, int groups, float eps,
                       int silu, const void* partials, int nblk, void* stream);
/* 1 when af_gemm with this (tile, splits) takes gn_partials for an output of N channels in groups of cpg and rows_per_batch rows per batch item */
int af_gemm_gn_stats_ok(int tile, int splits, int taps, int act, int out_mode, int N, int cpg, int rows_per_batch);
/* Which form of the halo-resident 3x3 kernel (tile 14) this descriptor would run: 0 = outside its scope (af_gemm falls back to a tap-by-tap tile),
 * 1 = 256 x 160 tiles on whole image rows, 2 = 256 x 128 tiles on whole image rows, 3 = 256 x 128 tiles on 16 x 16-pixel patches, 4 = the phase form
 * of the nearest-x2 convolution (upsample = 3: one source, c1 % 64 == 0, N % 160 == 0, W in {16, 32}, H W % 256 == 0, no split-K, no rowbias /
 * residual / gn_partials -- whether those three are set is read, nothing behind them).  This is the
 * predicate af_gemm itself launches on, and the only statement of that scope: callers ask it instead of repeating it.  Reads the shape and mode fields
 * only (taps, c1 .. c4, lda3, lda4, N, M, kpad, B, H, W, Ho, Wo, stride, upsample, tap_shift, act, out_mode, splits, and whether ln_colsum is set), no
 * operand pointer, so a host-side descriptor without operands gets the answer of the real launch; no launch. */
int af_gemm_halo_variant(const af_gemm_desc* d);
int af_groupnorm(const void* x1, const void* x2, int c1, int c2, const void* gamma, const void* beta,
                 void* y, int B, int HW, int groups, float eps, int silu, void* workspace, void* stream);

/* ---- LayerNorm over the last dim (nn.LayerNorm, attention.py:232-234; eps 1e-5) ------- */
/* same, and also writes stats fp32 [B, groups, 2] = (mean, rstd) for af_groupnorm_bwd */
int af_groupnorm_stats(const void* x1, const void* x2, int c1, int c2, const void* gamma, const void* beta,
                       void* y, void* stats, int B, int HW, int groups, float eps, int silu, void* workspace,
                       void* stream);

int af_layernorm(const void* x, const void* gamma, const void* beta, void* y, int rows, int C, float eps,
                 void* stream);

/* ---- fused attention core: softmax(q k^T * scale + keybias) v --------------------------
 * Replaces attention.py:180-204 (CrossAttention.forward between the projections) and the
 * explicit SDPA of adaface/diffusers_attn_lora_capture.py:79-139 without materialising
 * the [b*h, N, L] score tensor.
 *   q  [B, Nq, ldq]   k [B, L, ldk]   o [B, Nq, ldo]   (row strides in elements, >= heads*d:
 *   q and k may be column slices of one fused projection output)
 *   vt [B, heads*d, ldv] (V transposed, key index contiguous, ldv % 8 == 0)
 *   keybias: fp32 [B, ldb] added to every score row (0 = keep, -FLT_MAX = masked key as
 *   masked_fill_(~mask, -finfo.max) attention.py:188-194); NULL = none.  Keys >= L are
 *   always excluded.  d % 8 == 0, d <= 160.                                                */
int af_attention(const void* q, const void* k, const void* vt, void* o, const void* keybias, int B, int Nq,
                 int L, int heads, int d, int ldq, int ldk, int ldo, int ldv, int ldb, float scale, void* stream);
/* same, and also writes lse2 fp32 [B, heads, Nq] = log2(sum_j exp(score_ij)) (base-2 log-sum-exp of the
 * scaled+biased scores), which af_attention_bwd consumes. */
int af_attention_lse(const void* q, const void* k, const void* vt, void* o, void* lse2, int ld_lse, const void* keybias,
                     int B, int Nq, int L, int heads, int d, int ldq, int ldk, int ldo, int ldv, int ldb, float scale,
                     void* stream);

/* general form: causal_m > 0 adds CLIP's causal mask with `causal_m` keys per token (key j visible to query i
 * iff j / causal_m <= i): adaface/arc2face_models.py:145-231 (CLIPAttentionMKV, K/V widened x m). */
int af_attention_ex(const void* q, const void* k, const void* vt, void* o, void* lse2, int ld_lse, const void* keybias,
                    int causal_m, int B, int Nq, int L, int heads, int d, int ldq, int ldk, int ldo, int ldv, int ldb,
                    float scale, void* stream);
/* same with an explicit element stride between the batch items of vt (>= heads*d*ldv): lets vt be a row slice of a larger
 * [B, sum_C, ldv] tensor -- the U-Net computes the K / V^T projections of ALL its cross-attention layers in one GEMM */
int af_attention_strided(const void* q, const void* k, const void* vt, void* o, void* lse2, int ld_lse, const void* keybias, int causal_m,
                         int B, int Nq, int L, int heads, int d, int ldq, int ldk, int ldo, int ldv, int ldb, int64_t vt_batch_stride,
                         float scale, void* stream);

/* ---- attention backward (flash-style, recomputes P from q, k and lse2) -------------------
 * Input gradients of af_attention for dO = `dout`: dq [B,Nq,lddq], dk [B,L,lddk], dv [B,L,lddv].
 * q/k/v/o/dout are ROW-major token tensors (v is NOT transposed here) with row strides ld*;
 * lse2 fp32 [B, heads, ld_lse] from af_attention_lse, ld_lse >= roundup(Nq, 32), % 4 == 0.
 * scratch: >= af_attention_bwd_scratch_bytes(...) bytes (Q^T, K^T, dO^T copies and delta).
 * Reference: autograd of attention.py:180-204 (the reference stores the full score tensor).   */
int64_t af_attention_bwd_scratch_bytes(int B, int Nq, int L, int heads, int d);
int af_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const void* lse2,
                     int ld_lse, const void* keybias, int causal_m, void* dq, void* dk, void* dv, void* scratch,
                     int64_t scratch_bytes, int B, int Nq, int L, int heads, int d, int ldq, int ldk, int ldv,
                     int ldo, int lddo, int lddq, int lddk, int lddv, int ldb, float scale, void* stream);

/* explicit score / probability capture for one cross-attention layer (attention.py:207-220):
 * score[b,h,i,j] = q.k*scale, prob = softmax_j(score); fp32 outputs [B,heads,Nq,L].         */
int af_attention_scores(const void* q, const void* k, void* score, void* prob, int B, int Nq, int L, int heads,
                        int d, float scale, void* stream);

/* ---- explicit cross-attention of the capture / score-rewrite path (adaface/diffusers_attn_lora_capture.py:79-139, 309-315) ----
 * The captured cross-attention layers (22-24) materialise their scores so that they can be rewritten between the product and the
 * softmax (SC/MC mixing, subject-token normalisation) and captured WITH gradients.  q [B*Nq, ldq], k / v [B*L, ldk / ldv] fp16
 * row-major (head h = columns h*d ..), score / prob / dscore fp32 [B, heads, Nq, L] contiguous, L <= 128, d % 8 == 0.
 *   af_xattn_scores          score = scale * q k^T
 *   af_xattn_softmax_pv      prob = softmax_L(score);  o[B*Nq, ldo] = prob v                        (fp16)
 *   af_xattn_softmax_pv_bwd  dscore = prob * (dP - sum_L prob dP),  dP = dout v^T (+ dprob_ext, the gradient arriving on a captured prob; may be NULL)
 *   af_xattn_rowmix          out[B*Nq, ldout] = alpha * w x      (w fp32 [B,heads,Nq,L], x fp16 [B*L, ldx]):   dq = scale * dscore k
 *   af_xattn_colmix          out[B*L, ldout]  = alpha * w^T x    (x fp16 [B*Nq, ldx]):   dv = prob^T dout,  dk = scale * dscore^T q;
 *                            per (batch item, head) a GEMM over the queries on v_mfma_f32_16x16x4_f32 (f32 in / f32 accumulate: w is not rounded);
 *                            deterministic two-pass reduction over 16 query chunks through a caller-owned fp32 workspace          */
#define AF_XATTN_COLMIX_CHUNKS 16
int af_xattn_scores(const void* q, int ldq, const void* k, int ldk, void* score, int B, int Nq, int L, int heads, int d, float scale, void* stream);
int af_xattn_softmax_pv(const void* score, const void* v, int ldv, void* prob, void* o, int ldo, int B, int Nq, int L, int heads, int d, void* stream);
int af_xattn_softmax_pv_bwd(const void* prob, const void* v, int ldv, const void* dout, int lddo, const void* dprob_ext, void* dscore, int B, int Nq,
                            int L, int heads, int d, void* stream);
int af_xattn_rowmix(const void* w, const void* x, int ldx, void* out, int ldout, float alpha, int B, int Nq, int L, int heads, int d, void* stream);
int64_t af_xattn_colmix_ws_bytes(int B, int L, int heads, int d);
int af_xattn_colmix(const void* w, const void* x, int ldx, void* out, int ldout, float alpha, void* workspace, int64_t workspace_bytes, int B, int Nq,
                    int L, int heads, int d, void* stream);

/* ---- small element-wise kernels --------------------------------------------------------
 * timestep embedding [cos | sin] (util.py:154-174) -> fp16 [B, dim]                        */
int af_timestep_embedding(const void* timesteps_i64, void* out, int B, int dim, float max_period, void* stream);
/* NCHW fp32 -> NHWC fp16 with channel padding to cpad (zeros) and back (NHWC fp16 -> NCHW fp32) */
int af_nchw_f32_to_nhwc_f16(const void* x, void* y, int B, int C, int HW, int cpad, void* stream);
int af_nhwc_f16_to_nchw_f32(const void* x, void* y, int B, int C, int HW, int cstride, void* stream);
/* classifier-free guidance + DDIM update (ldm/models/diffusion/ddim.py:253-255, 279-301, sigma = 0):
 * eps = e_u + g (e_c - e_u); pred_x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t);
 * x_prev = sqrt(a_prev) pred_x0 + sqrt(1-a_prev) eps.   eps2 = [e_c ; e_u] fp32 [2n];
 * e_u == NULL (n_uncond = 0) means no guidance.  x, x_prev, pred_x0: fp32 [n].              */
int af_cfg_ddim_step(const void* eps2, const void* x, void* x_prev, void* pred_x0, int64_t n, int has_uncond,
                     float guidance, float a_t, float a_prev, void* stream);
/* classifier-free guidance + one DPM-Solver++ step (2S, midpoint; INTEGRATION.md "DPM-Solver++ scheduler") in data-prediction form:
 * e = e_u + g (e_c - e_u) (e = e_c when has_uncond == 0); x0 = (x - sigma_s e) / alpha_s;
 * x0_out = x0; x_out = c_base x_base + c0 x0 + c1 x0_prev, all fp32 [n].  eps2 = [e_c ; e_u] fp32 [2n] (or [n]).
 * x0_prev is not read when c1 == 0 and may then be NULL.  alpha_s in (0, 1], sigma_s in [0, 1), coefficients finite.        */
int af_cfg_dpmpp_step(const void* eps2, const void* x, const void* x_base, const void* x0_prev, void* x_out, void* x0_out, int64_t n,
                      int has_uncond, float guidance, float alpha_s, float sigma_s, float c_base, float c0, float c1, void* stream);
/* classifier-free guidance + one LCM step (multistep consistency sampling; INTEGRATION.md "LCM-LoRA"):
 * e = e_u + g (e_c - e_u) (e = e_c when has_uncond == 0); x0 = (x - sqrt_1ma e) / sqrt_a; denoised = c_out x0 + c_skip x;
 * x_next = sqrt_a_next denoised + sqrt_1ma_next noise, all fp32 [n].  eps2 = [e_c ; e_u] fp32 [2n] (or [n]).
 * noise == NULL is the last step: x_next = denoised, noise is not read.  sqrt_a (and, with noise, sqrt_a_next) in (0, 1],
 * sqrt_1ma (sqrt_1ma_next) in [0, 1), coefficients finite.                                                                  */
int af_cfg_lcm_step(const void* eps2, const void* x, const void* noise, void* x_next, void* denoised, int64_t n, int has_uncond,
                    float guidance, float sqrt_a, float sqrt_1ma, float c_out, float c_skip, float sqrt_a_next, float sqrt_1ma_next,
                    void* stream);
/* inpainting (INTEGRATION.md "Inpainting"): the three steps above with the mask blend as their tail, one launch each.  x_prev / x_out /
 * x_next become m ? x_new : known per element of output b, channel c, pixel p, where x_new is what the plain step writes,
 * m = mask[b % B_mask][p] (fp32 [B_mask,1,hw], binary: nonzero keeps x_new), z = z[b % B_img][c][p] (fp32 [B_img,4,hw]) and
 * known = fma(sb_next, noise[b][c][p], sa_next z) (noise fp32 [n / (4 hw), 4, hw]), or known = z when noise is NULL (the last
 * step; noise is not read).  pred_x0 / x0_out / denoised are not blended.  n % (4 hw) == 0, n < 2^31; 16-byte accesses when
 * hw % 4 == 0 and every pointer is aligned.  The LCM step's own re-noising draw stays `noise`; the blend's is `blend_noise`.  */
int af_cfg_ddim_inpaint_step(const void* eps2, const void* x, void* x_prev, void* pred_x0, int64_t n, int has_uncond, float guidance,
                             float a_t, float a_prev, const void* z, const void* noise, const void* mask, int B_img, int B_mask,
                             int64_t hw, float sa_next, float sb_next, void* stream);
int af_cfg_dpmpp_inpaint_step(const void* eps2, const void* x, const void* x_base, const void* x0_prev, void* x_out, void* x0_out,
                              int64_t n, int has_uncond, float guidance, float alpha_s, float sigma_s, float c_base, float c0, float c1,
                              const void* z, const void* noise, const void* mask, int B_img, int B_mask, int64_t hw, float sa_next,
                              float sb_next, void* stream);
int af_cfg_lcm_inpaint_step(const void* eps2, const void* x, const void* noise, void* x_next, void* denoised, int64_t n, int has_uncond,
                            float guidance, float sqrt_a, float sqrt_1ma, float c_out, float c_skip, float sqrt_a_next,
                            float sqrt_1ma_next, const void* z, const void* blend_noise, const void* mask, int B_img, int B_mask,
                            int64_t hw, float sa_next, float sb_next, void* stream);
/* q_sample (ldm/models/diffusion/ddpm.py:395-398): x_t = sa[b] x0 + sb[b] noise, fp32, per-sample scalars */
int af_q_sample(const void* x0, const void* noise, const void* sa, const void* sb, void* xt, int B, int64_t per,
                void* stream);
/* img2img input (diffusers' image preprocessing): img uint8 [B,H,W,3] (RGB, as PIL hands it over) -> out fp16 [B,H,W,8], the VAE
 * encoder's conv_in layout: channels 0-2 = (v / 255) * 2 - 1 computed in fp32 and rounded once, channels 3-7 written as 0.
 * out 16-byte aligned; any H, W.                                                                                             */
int af_image_u8_to_nhwc_f16(const void* img, void* out, int B, int H, int W, void* stream);
/* img2img latents from the encoder's conv_out output, one launch: h fp16 NHWC [B_img,hh,ww,8] (16-byte aligned);
 * moments = qw h + qb (quant_conv: qw fp32 [8 out][8 in] row-major, qb fp32 [8]); mean = moments[0:4],
 * logvar = clamp(moments[4:8], -30, 20); z = scale (mean + exp(0.5 logvar) n_post), n_post fp32 NCHW [B_img,4,hh,ww];
 * x_t = sa z + sb n_fwd, n_fwd / x_t fp32 NCHW [B_out,4,hh,ww]; output j reads image j % B_img.  B_out % B_img == 0.        */
int af_vae_latents_q_sample(const void* h, const void* qw, const void* qb, const void* n_post, const void* n_fwd, float scale, float sa,
                            float sb, void* x_t, int B_img, int B_out, int hh, int ww, void* stream);
/* the same, also writing the image latents z fp32 NCHW [B_img,4,hh,ww] (inpainting blends with them).  z must not be NULL.     */
int af_vae_latents_z_q_sample(const void* h, const void* qw, const void* qb, const void* n_post, const void* n_fwd, float scale,
                              float sa, float sb, void* x_t, void* z, int B_img, int B_out, int hh, int ww, void* stream);
/* high-resolution text2img, between the two passes, one launch:
 * out[p, Y, X] = fma(sb, noise[p, Y, X], sa * R(x)[p, Y, X]) over P = B*C planes; x fp32 [P, h, w], out / noise fp32 [P, H, W];
 * R = torch's F.interpolate(align_corners=False, antialias=False): mode 0 bilinear, 1 bicubic (A = -0.75);
 * noise == NULL: out = R(x) exactly (sa, sb ignored).  No workspace. */
int af_latent_resize_q_sample(const void* x, const void* noise, void* out, int P, int h, int w, int H, int W, int mode,
                              float sa, float sb, void* stream);

/* y = x * sigmoid(x), fp16 (nn.SiLU on the time embedding, openaimodel.py:219-220) */
int af_silu_f16(const void* x, void* y, int64_t n, void* stream);

/* ---- backward-pass kernels (activation gradients only: U-Net base weights are frozen, ddpm.py:4131) ----
 * GroupNorm(+SiLU) input gradient; x = concat(x1, x2) as in the forward, stats from af_groupnorm_stats,
 * dy/add [B,HW,c1+c2] (add optional, summed into dx), dx written to dx1 [B,HW,c1] / dx2 [B,HW,c2].      */
int af_groupnorm_bwd(const void* x1, const void* x2, int c1, int c2, const void* gamma, const void* beta,
                     const void* stats, const void* dy, const void* add, void* dx1, void* dx2, int B, int HW,
                     int groups, int silu, void* workspace, void* stream);
/* LayerNorm parameter gradients (the trainable LayerNorms of the CLIP encoders, subj_basis_generator.py:841-853): dgamma[c] =
 * sum_r dy[r,c] * (x[r,c] - mean_r) * rstd_r, dbeta[c] = sum_r dy[r,c]; x, dy fp16 [rows, C], outputs fp32 [C]; row_stats: caller-owned
 * fp32 scratch [rows][2] (mean, rstd: written by the first of the two launches); rows <= 2048, C <= 1536 */
int af_layernorm_param_grads(const void* x, const void* dy, void* dgamma, void* dbeta, void* row_stats, int rows, int C, float eps,
                             void* stream);
/* LayerNorm input gradient (+ optional `add`) */
int af_layernorm_bwd(const void* x, const void* gamma, const void* dy, const void* add, void* dx, int rows, int C,
                     float eps, void* stream);
/* un-fused GEGLU on the interleaved pre-activation hp [M, 2*inner] (training keeps hp): forward and input gradient */
int af_geglu_fwd(const void* hp, void* out, int64_t M, int inner, void* stream);
int af_geglu_bwd(const void* hp, const void* dout, void* dhp, int64_t M, int inner, void* stream);
/* adjoint of nearest-x2 upsampling: y [B,H,W,C] = 2x2 block sums of x [B,2H,2W,C] */
int af_sumpool2x2(const void* x, void* y, int B, int H, int W, int C, void* stream);
int af_add_f16(const void* a, const void* b, void* out, int64_t n, void* stream);
/* out = a + alpha * b: the decoder's skip-connection gradients joining the encoder's, scaled by res_hidden_states_gradscale
 * (adaface/diffusers_attn_lora_capture.py:23-42 ScaleGrad, :382-396) */
int af_axpy_f16(const void* a, const void* b, float alpha, void* out, int64_t n, void* stream);
/* x [B,N,ldx] (C columns) -> y [B,C,ldy] with the token index contiguous (zero padded to ldy) */
int af_transpose_tokens(const void* x, void* y, int B, int N, int C, int ldx, int ldy, void* stream);
/* two such transposes of the same [B, N] token grid in one launch (a weight gradient's operands dy^T and x^T): x1 [B*N, ldx1] -> y1 [B, C1, ldy],
 * x2 [B*N, ldx2] -> y2 [B, C2, ldy] */
int af_transpose_tokens_pair(const void* x1, void* y1, int C1, int ldx1, const void* x2, void* y2, int C2, int ldx2, int B, int N, int ldy,
                             void* stream);
/* cautious AdamW (ldm/c_adamw.py:65-123) over a flat fp32 buffer; seg_offsets int64 [nseg+1] delimit the
 * parameter tensors (the caution mask is renormalised per tensor); counts: uint32 [nseg] scratch.          */
int af_cadamw_step(void* p, const void* g, void* m, void* v, const void* seg_offsets, int nseg, void* counts, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, int correct_bias, void* stream);

/* ---- parameter-gradient helpers of the (trainable) CLIP text encoder -------------------------------
 * out fp32 [C] (+)= sum_rows a[r,c] * (b ? b[r,c] : 1): bias gradients (b = NULL) and LayerNorm gamma gradients
 * (a = dy, b = x_hat).  accumulate != 0 adds to `out`.                                                      */
int af_colsum(const void* a, const void* b, void* out, int rows, int C, int accumulate, void* stream);
/* same for tall inputs (rows >> C): `chunks` row ranges are folded by separate workgroups into partial (fp32 [chunks, C],
 * caller-owned) and then reduced in a fixed order -- deterministic, no atomics */
int af_colsum_tall(const void* a, const void* b, void* partial, void* out, int rows, int C, int chunks, int accumulate, void* stream);
/* quick-GELU x*sigmoid(1.702x) (CLIP MLP) and its input gradient, fp16 element-wise */
int af_quickgelu_fwd(const void* x, void* y, int64_t n, void* stream);
int af_quickgelu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
/* y = a * s (fp32), used to unscale the loss-scaled gradient arena before the optimizer step */
int af_scale_f32(void* a, float s, int64_t n, void* stream);
/* a = clamp(a, lo, hi): gradient clipping by VALUE over the flat gradient arena (Lightning `gradient_clip_algorithm: 'value'`,
 * `gradient_clip_val: 0.01` in configs/stable-diffusion/v1-distill-arc2face-ada.yaml:150-152; ddpm.py:496-497) */
int af_clamp_f32(void* a, float lo, float hi, int64_t n, void* stream);

/* ---- VAE decoder (ldm/modules/diffusionmodules/model.py:151-243 AttnBlock): row softmax of an explicit fp16 score matrix
 * [rows, L], L % 8 == 0, L <= 4096 (single-head 512-dim attention runs as af_gemm -> af_softmax_rows -> af_gemm) */
int af_softmax_rows(const void* x, void* y, int64_t rows, int L, void* stream);
/* The same layer fused, at any size: o = softmax(q k^T) v for ONE head of dim C in {128, 512} with online softmax -- no [N, N] matrix and no
 * workspace, memory is O(N C).  q, k [B*N, ldq / ldk] fp16 token rows (the C^-0.5 scale already folded into q), vt [B, C, ldv] the values
 * TRANSPOSED with the key index contiguous (af_transpose_tokens; ldv >= N), o [B*N, ldo].  N % 8 == 0, any N >= 8 (query and key tails are
 * handled; keys >= N and the ldv pad are never read as data); strides multiples of 8, operands 16-byte aligned.  fp32 scores, fp32 running
 * reference / sum and fp32 accumulation; P is rounded to fp16 as the MFMA operand.  AF_E_UNSUPPORTED for another C and for an operand of 2^31
 * elements or more (offsets are not wrapped).                                                                                             */
int af_vae_attention(const void* q, const void* k, const void* vt, void* o, int B, int N, int C, int ldq, int ldk, int ldv, int ldo, void* stream);
/* Self-attention along the frame axis (AnimateDiff motion modules).  qkv fp16, row r = (b*F + f)*HW + p (batch item b, frame f, pixel p)
 * holds q | k | v of that token at columns [0,C) | [C,2C) | [2C,3C), C = heads*d, row stride ld elements.
 * out fp16 [B*F*HW][C]:  out[(b*F+f)*HW+p, h*d+j] = sum_g softmax_g(scale * <q_f, k_g>) * v_g[j], g over the F frames of the same (b, p, h).
 * 1 <= F <= 32, d % 8 == 0, 8 <= d <= 160, ld % 8 == 0, ld >= 3C, 16-byte aligned pointers, any HW >= 1.  No workspace, one launch.
 * fp32 scores, softmax and accumulation; P is rounded to fp16 as the MFMA operand.  Every qkv element is read once (16-byte loads), so a dense
 * qkv costs 2 (3C + C) bytes per row.
 * AF_E_BADARG (before any launch): NULL pointer, a size outside the above, B*F*HW*ld or B*F*HW*C >= 2^31. */
int af_temporal_attention(const void* qkv, int ld, void* out, int B, int F, int HW, int heads, int d, float scale, void* stream);
/* The image-prompt half of IP-Adapter's decoupled cross-attention, added in place to the text attention's output o:
 *   o[b*N+i, h*d+j] = fp16( float(o[b*N+i, h*d+j]) + ip_scale * sum_t softmax_t(scale * <q[b,i,h,:], k[b,t,h,:]>) * v[b,t,h,j] ),  t over T tokens.
 * q fp16 [B*N, ldq] (read only), o fp16 [B*N, ldo] (updated in place).  k and v are ROW-MAJOR fp16 token rows: token t of batch item b starts
 * at k + b*k_bstride + t*ldk (v likewise) and holds its heads*d channels contiguously, so a layer reads its column slice of one stacked
 * [to_k_ip | to_v_ip] projection of all layers in place.  1 <= T <= 64, d % 8 == 0, 8 <= d <= 160, any N >= 1; row strides are multiples
 * of 8 and >= heads*d, batch strides multiples of 8 (0 shares one token set), pointers 16-byte aligned, B and heads <= 65535.
 * One launch, no workspace; every q and o element is touched once with 16-byte accesses, K and V of a (b, h) stay in registers / LDS.
 * fp32 scores, softmax and accumulation; P is rounded to fp16 once as the MFMA operand; the text and image results are summed in fp32 and
 * rounded once.  ip_scale == 0 returns AF_OK without a launch.
 * AF_E_BADARG (before any launch): NULL pointer, a size or stride outside the above, an operand of 2^31 elements or more. */
int af_ip_attention_add(void* o, int ldo, const void* q, int ldq, const void* k, int ldk, int64_t k_bstride, const void* v, int ldv,
                        int64_t v_bstride, int B, int N, int T, int heads, int d, float scale, float ip_scale, void* stream);
/* Regional prompts: the cross-attention core over R context sets per batch item, blended per query under the region weights w:
 *   o[b*N+i, h*d+j] = fp16( sum_r w[b*R+r, i] * sum_t softmax_t(scale * <q[b,i,h,:], k[b,r,t,h,:]>) * v[b,r,t,h,j] ),  t over L tokens, r over R sets.
 * q fp16 [B*N, ldq], o fp16 [B*N, ldo], w fp32 [B*R, ldw] (ldw >= N).  Context set (b, r) is batch item b*R+r of k and vt, addressed exactly as
 * af_attention_strided addresses its batch items: k rows (b*R+r)*L + t with row stride ldk, vt the values TRANSPOSED ([heads*d, ldv] per item,
 * key index contiguous, ldv >= L) at element stride vt_batch_stride (>= heads*d*ldv), so a layer reads its slice of ONE stacked projection of
 * all layers in place.  1 <= R <= 8, 1 <= L <= 80, d % 8 == 0, 8 <= d <= 160, any N >= 1; ldq / ldo / ldk / ldv and vt_batch_stride are multiples
 * of 8, ldq / ldo / ldk >= heads*d, pointers 16-byte aligned, B and heads <= 65535.
 * One launch, no workspace.  fp32 scores (the scale is applied to them, q is not rescaled in fp16), softmax, normalisation by the fp32 row sum and
 * weighted sum over the sets; P is rounded to fp16 once as the MFMA operand, o once.
 * The zero weight is a SELECT, not a multiply: a query with w[b*R+r, i] == 0 receives nothing from set (b, r) whatever its K / V hold (Inf and
 * NaN included); a 128-query tile whose weights for r are all 0 does not read K_r / V_r (so those need not even be written); a query whose
 * weights are all 0 gets zeros.  The skip is decided per workgroup before any barrier of the set's iteration (every wave reduces the tile's
 * weights itself), so no barrier sits in divergent control flow.
 * AF_E_BADARG (before any launch): NULL pointer, a size or stride outside the above, an operand of 2^31 elements or more. */
int af_region_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldv, int64_t vt_batch_stride,
                        const void* w, int ldw, void* o, int ldo, int B, int R, int N, int L, int heads, int d, float scale, void* stream);
/* The region weights of all four U-Net levels from R-1 uint8 masks [R-1, H, W] (0 .. 255, 255 = the region) in ONE launch: the masks are
 * area-averaged onto each level's token grid (cells of 8, 16, 32, 64 pixels: m_r = sum / (255 * area), the integer sum exact) and, with
 * s = sum_{r>=1} m_r:  w_r = (1 - beta) * m_r / max(1, s) for r >= 1,  w_0 = beta + (1 - beta) * (1 - min(1, s)).
 * w fp32 [R, ldw]: level l (0 .. 3, N_l = (H/8 >> l) * (W/8 >> l) tokens, row-major) at columns [off_l, off_l + N_l), off_0 = 0,
 * off_l = off_{l-1} + N_{l-1}; ldw >= 85 * H * W / 4096.  A cell no pixel of mask r touches holds exactly 0.0 in row r.
 * H and W multiples of 64 in 64 .. 16384, 1 <= R <= 8 (masks may be NULL at R == 1), 0 <= beta <= 1, masks 8-byte aligned.
 * AF_E_BADARG (before any launch) otherwise. */
int af_region_weights(const void* masks, int R, int H, int W, float beta, void* w, int ldw, void* stream);
/* FreeU (Si et al.) on the two inputs of a decoder skip concatenation, h [B, H, W, C] and skip [B, H, W, Cs], contiguous NHWC fp16, per sample:
 *   h[p, :C/2] *= f[p];   version 2: f = (b - 1) * mhat + 1, mhat = (m - lo) / (hi - lo), m[p] = fp32 mean of h[p, :] over all C channels, lo / hi
 *                         its min / max over the sample's pixels, mhat = 0 where hi == lo (the authors' code gives NaN there);   version 1: f = b
 *   skip plane (sample, channel) x -> y[h, w] = x[h, w] + (s - 1) / (H W) * sum_{u in Uh, v in Uw} (A_uv cos phi + B_uv sin phi),
 *                         phi = 2 pi (u h / H + v w / W), A_uv = sum x cos phi, B_uv = sum x sin phi, Uh = {0, -1 mod H}, Uw = {0, -1 mod W}
 * (the authors' Fourier_filter(skip, threshold = 1, scale = s) in closed form: four bins, two when a side is 1, one at 1 x 1).
 * af_freeu_stats makes one pass over h and skip and leaves in ws (fp32, af_freeu_ws_floats(B, H, W, C, Cs) floats, 16-byte aligned) the pixel
 * means with per-wave (lo, hi) partials (version 2 and b != 1 only) and, when s != 1, per (sample, skip channel) the plane's first pixel (the pivot
 * the sums are shifted by) and the seven sums as one partial per slice of the pixels; af_freeu_apply adds the partials in slice order and writes
 *   h_out[:, :C/2] = sat(h * f)   (channels C/2 .. C of h_out are NOT written: in place, h_out == h, is the intended form)   and
 *   skip_out = sat(skip + (s - 1) / (H W) * low)   (skip_out == skip is allowed).
 * No atomics and no hand-off between workgroups inside a launch: two runs are bit-identical.  fp32 throughout, each output rounded to fp16 once;
 * finite values saturate at +-65504, NaN and Inf stay.  A NaN pixel mean makes lo and hi, and with them that sample's h_out[:, :C/2], NaN; a skip
 * plane that holds a NaN or an Inf is NaN everywhere (as its DFT is); nothing crosses from one sample to another or from one plane to another.
 * s == 1: skip is not read and skip_out not written (no NaN from 0 * Inf); b == 1: h is not read and h_out not written; both 1: no launch.
 * 1 <= B <= 65535; 1 <= H, W <= 128; C % 16 == 0 in 16 .. 16384; Cs % 8 == 0 in 8 .. 16384; B*H*W*C and B*H*W*Cs below 2^31 (the kernels index
 * with 64 bits; the limit is the library's common one); b and s finite and >= 0; version 1 or 2; all pointers 16-byte aligned.
 * AF_E_BADARG before any launch, outputs and workspace untouched: anything else, a NULL pointer, ws_floats below af_freeu_ws_floats.
 * Both calls of a pair take the same sizes, b, s and version.  No allocation, no host synchronisation: the pair can be captured. */
int64_t af_freeu_ws_floats(int B, int H, int W, int C, int Cs);
int af_freeu_stats(const void* h, const void* skip, void* ws, int64_t ws_floats, int B, int H, int W, int C, int Cs, float b, float s, int version,
                   void* stream);
int af_freeu_apply(const void* h, const void* skip, const void* ws, int64_t ws_floats, void* h_out, void* skip_out, int B, int H, int W, int C,
                   int Cs, float b, float s, int version, void* stream);
/* its backward, ds = p * (dp - rowsum(p * dp)), for the decode-with-grad path of the ArcFace alignment loss (ddpm.py:2511-2535
 * differentiates through decode_first_stage_with_grad, ddpm.py:899-908) */
int af_softmax_rows_bwd(const void* p, const void* dp, void* ds, int64_t rows, int L, void* stream);
/* masked VAE-encoder attention (model.py:191-209): p fp16 [N, N] (post-softmax) *= ((cls[i] & cls[j]) != 0); cls uint8 [N]: bit 0 fg*aug != 0, bit 1 (1-fg)*aug != 0 */
int af_mask_pairs(void* p, const void* cls, int N, void* stream);
/* read every 128-byte line of [ptr, ptr + bytes) once (no writes): cache warm-up of packed weights ahead of the GEMM that streams them,
   meant for a side stream */
int af_prefetch(const void* ptr, int64_t bytes, void* stream);
/* the same with the grid capped at max_workgroups (256 threads each, striding over the lines): a prefetcher that runs BESIDE the GEMMs of a
   step on a second stream must not take the chip from them (ops.WeightPrefetcher) */
int af_prefetch_ex(const void* ptr, int64_t bytes, int max_workgroups, void* stream);

/* ---- ArcFace ResNetFace-18 IR-SE face encoder (reference evaluation/arcface_resnet.py:62-97, 139-154, 157-217) ----
 * NHWC fp16 activations, C % 8 == 0.  Convolutions / FCs are af_gemm calls with eval-mode BatchNorm folded on the host.
 * y = prelu(x * scale[c] + shift[c]); scale/shift fp32 [C] or both NULL; slope fp32 [1] device pointer or NULL (no PReLU) */
int af_affine_prelu(const void* x, const void* scale, const void* shift, const void* slope, void* y, int64_t rows, int C, void* stream);
/* the same with one slope per channel: slope fp32 [C] or NULL (IResNet, insightface's recogniser: nn.PReLU(planes)) */
int af_affine_prelu_ch(const void* x, const void* scale, const void* shift, const void* slope, void* y, int64_t rows, int C, void* stream);
/* 5-point face alignment into the recogniser's crop, one launch per image: image_u8 uint8 RGB [H, W, 3] contiguous, inv_mats fp32
 * [F, 2, 3] (crop -> image), out fp16 [F, size, size, 8] (16-byte aligned).  Output pixel (x, y) of face f samples the image at
 * (sx, sy) = inv_mats[f] . (x, y, 1): integer pixel coordinates without a half-pixel shift (cv2.warpAffine's convention), bilinear over the
 * four neighbours, a tap outside the image counts as 0 (BORDER_CONSTANT 0).  Channels 0-2 = (v - 127.5) / 127.5 in RGB order, fp32
 * arithmetic rounded once; channels 3-7 are written as 0.  size in {112, 128}, F >= 1, H * W * 3 < 2^31, F * size^2 < 2^31.          */
int af_face_align_crop(const void* image_u8, const void* inv_mats, void* out, int H, int W, int F, int size, void* stream);
/* x [B, 2Ho, 2Wo, C] -> y [B, Ho, Wo, C] (nn.MaxPool2d(2, 2), arcface_resnet.py:165) */
int af_maxpool2x2(const void* x, void* y, int B, int Ho, int Wo, int C, void* stream);
/* x [B, HW, C] -> out fp16 [B, C] (AdaptiveAvgPool2d(1), arcface_resnet.py:142) */
int af_global_avgpool(const void* x, void* out, int B, int HW, int C, void* stream);
/* y = prelu(x * sigmoid(se_logits[b, c]) + residual); se_logits fp16 [B, C] or NULL (use_se = False) (arcface_resnet.py:88-95,153) */
int af_se_residual_prelu(const void* x, const void* se_logits, const void* residual, const void* slope, void* y, int B, int HW, int C,
                         void* stream);
/* Input-gradient kernels of the same layers.  The encoder is frozen (arcface_wrapper.py:65-76) but calc_arcface_align_loss
 * (arcface_wrapper.py:89-166) back-propagates through it into the decoded image, so d/dx is needed and parameter gradients are not.
 * dx = dy * prelu'(x * scale + shift) * scale; x may be NULL when slope is NULL (pure affine) */
int af_affine_prelu_bwd(const void* x, const void* scale, const void* shift, const void* slope, const void* dy, void* dx, int64_t rows,
                        int C, void* stream);
/* x [B, 2Ho, 2Wo, C] (the forward input), dy [B, Ho, Wo, C] -> dx [B, 2Ho, 2Wo, C]: dy to the first maximum of each window */
int af_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int B, int Ho, int Wo, int C, void* stream);
/* dgl fp16 [B, C] = sigmoid'(se_logits) * mean_hw(dpre * x), dpre = dy * prelu'(x * sigmoid(se_logits) + residual): the gradient of
 * the SE logits ALREADY divided by HW (the squeeze's 1/HW, applied early so the fp16 value stays in range; the chain between is linear) */
int af_se_gate_grad(const void* x, const void* se_logits, const void* residual, const void* slope, const void* dy, void* dgl, int B, int HW,
                    int C, void* stream);
/* dx = dpre * sigmoid(se_logits) + dpool[b, c];  dres = dpre.  dpool fp16 [B, C] (the squeeze-branch gradient, 1/HW included) or NULL */
int af_se_residual_prelu_bwd(const void* x, const void* se_logits, const void* residual, const void* slope, const void* dy,
                             const void* dpool, void* dx, void* dres, int B, int HW, int C, void* stream);

/* ---- RetinaFace-R50 face detector (adaface/retinaface.py; biubug6 Pytorch_Retinaface cfg_re50): the layers between its GEMMs and the
 * post-processing.  NHWC fp16 activations, C % 8 == 0, tensors 16-byte aligned.  Every argument check precedes any launch (AF_E_BADARG, the
 * function named in af_last_error()); an operand whose byte offsets would reach 2^31 is refused.
 *
 * The stem's A operand: image_u8 uint8 RGB [B, H, W, 3] -> out fp16 [B * Ho * Wo, 160], the rows of the 7x7 / stride 2 / pad 3 convolution
 * over the image padded at the bottom and right to (Hp, Wp) = (H, W) rounded up to multiples of 32 (so every FPN level is exactly twice the
 * next): Ho = Hp / 2, Wo = Wp / 2.  Column (ky * 7 + kx) * 3 + c holds v * scale[c] + shift[c] of pixel (2 oy - 3 + ky, 2 ox - 3 + kx); a tap
 * outside the H x W image (halo and padding alike) is 0 in NORMALISED space, which is why the normalisation cannot be folded into the
 * weights.  Columns 147..159 are written as 0.  bgr != 0: output channel c reads image channel 2 - c.  scale, shift: HOST fp32 [3].        */
int af_stem_im2col7x7(const void* image_u8, const float* scale, const float* shift, void* out, int B, int H, int W, int bgr, void* stream);
/* y = relu(maxpool 3x3 / stride 2 / pad 1 (x)) (the two commute): x [B, H, W, C] -> y [B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C].  Padding
 * never wins the maximum. */
int af_relu_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, void* stream);
/* the even pixels: x [B, H, W, C] -> y [B, (H + 1) / 2, (W + 1) / 2, C], y[b, i, j] = x[b, 2i, 2j] (the A operand of a stride-2 1x1 convolution) */
int af_subsample2x(const void* x, void* y, int B, int H, int W, int C, void* stream);
/* y = a + nearest2x(b): a, y [B, 2h, 2w, C], b [B, h, w, C]; fp32 sum, rounded once (the FPN's top-down path) */
int af_upsample2x_add(const void* a, const void* b, void* y, int B, int h, int w, int C, void* stream);
/* Anchor decode + score filter.  head0..2: fp16 [B, Hk * Wk, 32], per anchor a in {0, 1} the 16 columns a * 16 + [box 4 | cls 2 | ldm 10].
 * HOST arrays: level_hw int [6] = (H0, W0, H1, W1, H2, W2), steps int [3], min_sizes fp32 [6] = two per level.  One lane per anchor, anchor
 * index = level offset + (i * Wk + j) * 2 + a (biubug6's PriorBox order).  In pixels, fp32, s = min_sizes[k][a]:
 *   cx = (j + 0.5) step + 0.1 box0 s, cy = (i + 0.5) step + 0.1 box1 s, w = s exp(0.2 box2), h = s exp(0.2 box3),
 *   x1 = cx - w / 2, y1 = cy - h / 2, x2 = x1 + w, y2 = y1 + h; landmark n = ((j + 0.5) step + 0.1 ldm[2n] s, (i + 0.5) step + 0.1 ldm[2n+1] s);
 *   score = 1 / (1 + exp(cls0 - cls1)).
 * An anchor with score >= conf_thr (NaN never passes) takes the next row of its image's list cand fp32 [B, C, 16] = x1, y1, x2, y2, score,
 * 10 landmark coordinates, anchor index, through a (vector) atomic counter; count int32 [B] is zeroed by this call and ends as the number of
 * PASSING anchors, also beyond the capacity C (1 <= C <= 1024; rows beyond it are dropped, which ones depends on scheduling).           */
int af_retina_decode(const void* head0, const void* head1, const void* head2, const int* level_hw, const int* steps, const float* min_sizes,
                     int B, float conf_thr, void* cand, void* count, int C, void* stream);
/* Non-maximum suppression of af_retina_decode's lists, one workgroup per image, candidates in LDS: sorted by (score descending, anchor index
 * ascending) -- a total order, so the result does not depend on the append order -- then greedily: a kept candidate suppresses every later
 * one with IoU > nms_thr, IoU = inter / (area_a + area_b - inter) with plain widths (torchvision's rule, not biubug6's "+ 1").  out fp32
 * [B, max_det, 16]: the first max_det kept rows in order, rows beyond `kept` zero; out_counts int32 [B, 2] = (kept, passing).
 * 1 <= max_det <= C <= 1024.                                                                                                            */
int af_retina_nms(const void* cand, const void* count, void* out, void* out_counts, int B, int C, int max_det, float nms_thr, void* stream);

/* ---- repainting faces in a photo (adaface/face_repaint.py; AdaFaceWrapper's inpaint pipeline with mask_image="face" / crop_padding): the
 * pixel-space steps around the VAE.  photo: uint8 RGB [H, W, 3]; alpha: fp32 [H, W]; rectangle (x0, y0, cw, ch) non-empty and inside the
 * photo.  32-bit offsets: H * W * 3 >= 2^31 (and B * H * W * 3 >= 2^31) is refused.  Every argument check precedes any launch (AF_E_BADARG,
 * the function named in af_last_error()).  Four pixels of a row per lane: 12-byte / 16-byte accesses when W % 4 == 0 and the bases are
 * aligned, byte / dword accesses otherwise.
 *
 * The resampling rule R(n_in -> n_out), separable, is torch's F.interpolate(mode="bilinear", antialias=True, align_corners=False):
 *   s = n_in / n_out, sup = max(s, 1), c = s (i + 0.5); taps k in [max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5)));
 *   weight max(0, 1 - |(k - c + 0.5) / sup|) / (its sum over the taps).  Tap ranges and un-normalised weights are exact integers over
 *   2 max(n_in, n_out); each normalised weight is one fp32 division; sums run along x, then y, in fp32.  At s = 1 it is the identity.
 *
 * Soft face mask.  ellipses fp32 [F, 4] rows (cx, cy, rx, ry) in photo pixels (device memory; NULL allowed when F = 0):
 *   r = sqrt(((x + 0.5 - cx) / rx)^2 + ((y + 0.5 - cy) / ry)^2), t = clamp((1 - r) / feather, 0, 1), a_f = t^2 (3 - 2 t)
 *   (feather = 0: a_f = (r <= 1)); alpha[y, x] = max_f a_f, 0 for F = 0.                                                                  */
int af_face_alpha_mask(const void* ellipses, void* alpha, int F, int H, int W, float feather, void* stream);
/* One launch: image uint8 [1, Hs, Ws, 3] = rint(clamp(R(photo[y0:y0+ch, x0:x0+cw]), 0, 255)) (ties to even; taps never leave the rectangle)
 * and mask_lat fp32 [1, 1, Hs/8, Ws/8] = (max over the 8 x 8 block of R(alpha[y0:y0+ch, x0:x0+cw]) >= thr).  Hs, Ws: positive multiples of 8. */
int af_crop_resize_u8(const void* photo_u8, const void* alpha, void* image_u8, void* mask_lat, int H, int W, int x0, int y0, int cw, int ch,
                      int Hs, int Ws, float thr, void* stream);
/* One launch: out uint8 [B, H, W, 3].  Outside the rectangle (and wherever alpha == 0) out = photo.  Inside, with d = R(decoded[b, c]) from
 * (Hs, Ws) to (ch, cw), decoded fp32 [B, 3, Hs, Ws] in [-1, 1] nominally: g = 255 clamp(d / 2 + 0.5, 0, 1),
 * out = rint(alpha g + (1 - alpha) p), ties to even, in this order and unfused: alpha = 0 gives p and alpha = 1 gives rint(g) bit for bit. */
int af_paste_back_u8(const void* decoded, const void* photo_u8, const void* alpha, void* out_u8, int B, int Hs, int Ws, int H, int W, int x0,
                     int y0, int cw, int ch, void* stream);

/* ---- Real-ESRGAN upscaler (adaface/esrgan.py, RRDBNet): a 3x3 convolution (pad 1) that reads the first cin channels of a strided NHWC buffer
 * and writes a narrow channel slice of the same or another buffer, so that a dense block's concatenation is a buffer layout and never a copy.
 * y[b,i,j,n] = bias[n] + sum_{ky,kx,c<cin} wt[n][(ky*3+kx)*cin + c] * X[b, i+ky-1, j+kx-1, c]      (zero outside the image)
 *   X[b,i,j,c] = x[((b*H + i)*W + j)*ldx + c]                        upsample == 0, output Ho x Wo = H x W
 *   X[b,i,j,c] = x[((b*H + (i>>1))*W + (j>>1))*ldx + c], 0 <= i < 2H  upsample == 1 (nearest x2, not materialised), output 2H x 2W
 * v = slope > 0 ? (y >= 0 ? y : slope*y) : y ;  if r1: v = alpha*v + r1[m*ldr1 + n] ;  if r2: v = beta*v + r2[m*ldr2 + n]   (all fp32)
 * out_mode 0: out fp16, out[m*ldo + n] = fp16(v) for n < cout.  Channels >= cout of the row and any bytes between rows are NOT written.
 * out_mode 1: out uint8 [M][cout] tight (ldo ignored), out = rint(255 * min(max(v, 0), 1)), round-half-even.
 * x fp16, cin % 32 == 0, 32 <= cin <= 192, ldx >= cin.  wt fp16 [npad][9*cin], npad = cout rounded up to 16, zero rows behind cout.
 * 1 <= cout <= 64.  bias fp32 [cout] or NULL.  ldx, ldo, ldr1, ldr2 % 8 == 0, 16-byte aligned pointers.
 * out may lie in x's buffer on channels disjoint from [0, cin) (the dense-block write: same row stride, same grid).  r1 / r2 may be exactly
 * the out elements, or other channels of out's rows (same row stride); any other overlap of their byte range with out's is refused.  That
 * out does not overlap wt or bias is the caller's duty (not checked).
 * AF_E_BADARG before any launch: NULL x / wt / out, a size outside the above, an out range that overlaps channels [0, cin) of x,
 * r1 / r2 overlapping out otherwise than stated, r2 without r1, B*H*W*ldx or B*Ho*Wo*max(ldo, ldr1, ldr2, cout) at or above 2^31.  No workspace, one launch. */
int af_dense_conv3x3(const void* x, int ldx, int cin, const void* wt, const void* bias, void* out, int ldo, int cout,
                     const void* r1, int ldr1, float alpha, const void* r2, int ldr2, float beta, float slope,
                     int upsample, int out_mode, int B, int H, int W, void* stream);
/* img uint8 [B, H, W, 3] -> out fp16 [B, H/r, W/r, cpad]: channel c*r*r + dy*r + dx = img[b, i*r+dy, j*r+dx, c] / 255 (torch's pixel_unshuffle
 * order), channels 3 r^2 .. cpad zero.  r in {1, 2, 4}, H % r == W % r == 0, cpad in {32, 64} and >= 3 r^2; fewer than 2^31 elements each side. */
int af_u8_unshuffle_f16(const void* img_u8, void* out, int B, int H, int W, int r, int cpad, void* stream);

/* ---- GFPGAN face restoration (adaface/gfpgan.py, GFPGANv1Clean): the kernels around the tuned convolutions.  Every argument check precedes any
 * launch (AF_E_BADARG, the function named in af_last_error()); a tensor of 2^31 elements or more is refused (32-bit offsets).
 *
 * Per-sample weights of a StyleGAN2 modulated convolution, in af_gemm's packed layout.  w fp32 [cout][taps][cin] (taps 1 or 9, K = taps * cin in
 * (ky, kx, c) order), wsq fp32 [cout][cin] = sum over the taps of w^2 (NULL allowed when demod == 0), styles fp32 [B][cin]:
 *   d[b,o] = demod ? 1 / sqrt(sum_i styles[b,i]^2 * wsq[o,i] + 1e-8) : 1
 *   out[(b * npad + o) * kpad + t * cin + i] = fp16(gain * d[b,o] * w[o,t,i] * styles[b,i])       for o < cout
 * all in fp32 (the sum over i in any order), rounded to fp16 once.  Only the cout x K block of each slice is written: rows cout .. npad and
 * columns K .. kpad are the caller's zeros, written once when the buffer is allocated.  cin % 8 == 0, kpad % 64 == 0, kpad >= K,
 * npad % 128 == 0, npad >= cout, B * npad * kpad < 2^31, 16-byte aligned pointers. */
int af_modulate_weights(const void* w, const void* wsq, const void* styles, void* out, int B, int cout, int cin, int taps, int npad, int kpad,
                        int demod, float gain, void* stream);
/* StyleConv's tail and the SFT of the next layer in one pass.  y, out fp16 [B, HW, C] (out may be y), noise fp32 [HW] (NULL allowed when
 * nw == 0), bias fp32 [C] or NULL, scale / shift fp16 [B, HW, C / 2], both or neither:
 *   v = y + nw * noise[p] + bias[c];  v = v >= 0 ? v : 0.2 * v;  if scale and c >= C / 2: v = v * scale[b,p,c - C/2] + shift[b,p,c - C/2]
 *   out = fp16(min(max(v, -65504), 65504))
 * in fp32 in this order, unfused.  The clamp makes an fp16 overflow saturate at +-65504 instead of becoming inf.  C % 8 == 0 (C % 16 == 0 with
 * scale / shift), B * HW * C < 2^31, 16-byte aligned pointers. */
int af_style_epilogue(const void* y, const void* noise, const void* bias, const void* scale, const void* shift, void* out, int B, int HW, int C,
                      float nw, void* stream);
/* x fp16 [B, H, W, C] -> out fp16 [B, 2H, 2W, C] = F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) (+ addend
 * [B, 2H, 2W, C] or NULL).  Output row 2k reads rows (k - 1, k) with weights (0.25, 0.75), row 2k + 1 rows (k, k + 1) with (0.75, 0.25),
 * indices clamped to [0, H - 1]; the same along x:
 *   out = fp16(wy0 * (wx0 * x[y0,x0] + wx1 * x[y0,x1]) + wy1 * (wx0 * x[y1,x0] + wx1 * x[y1,x1]) + addend)     fp32, unfused.
 * C % 8 == 0, B * 2H * 2W * C < 2^31, 16-byte aligned pointers, out must not overlap x. */
int af_bilinear_up2(const void* x, const void* addend, void* out, int B, int H, int W, int C, void* stream);
/* Restored face crops back into the photo, one launch.  photo, out uint8 [H, W, 3] (out may be photo), crops fp16 [F, S, S, ld] with RGB in
 * channels 0-2 (nominally in [-1, 1]), mats fp32 [F, 2, 3] (image -> crop, integer pixel coordinates as in af_face_align_crop), erode >= 0 and
 * feather >= 0 in crop pixels.  Per pixel (x, y), cur = photo[y, x] as fp32, then for f = 0 .. F - 1 in order:
 *   (u, v) = mats[f] . (x, y, 1);  m = min(u, v, S - 1 - u, S - 1 - v);  skipped unless m > erode (alpha = 0)
 *   t = feather > 0 ? min((m - erode) / feather, 1) : 1;  alpha = t * t * (3 - 2 t)
 *   g = 255 * min(max(bilinear(crops[f], u, v) / 2 + 0.5, 0), 1);  cur = alpha * g + (1 - alpha) * cur        (fp32, unfused)
 * out = rint(cur), ties to even, once at the end; a pixel no face reaches with m > erode is the photo's byte, bit for bit.  Since alpha -> 0
 * towards the crop border, the border is never a discontinuity.  0 <= F <= 16 (F = 0: a copy; crops and mats may then be NULL), S >= 2,
 * ld >= 3, H * W * 3 < 2^31, F * S * S * ld < 2^31. */
int af_face_paste_affine_u8(const void* photo_u8, const void* crops, const void* mats, void* out_u8, int H, int W, int F, int S, int ld,
                            float erode, float feather, void* stream);
/* af_face_align_crop for the restorer's crop sizes: the same kernel and formula, size any multiple of 8 from 8 to 1024 (the recogniser's entry
 * above keeps refusing everything but 112 and 128). */
int af_face_align_crop_any(const void* image_u8, const void* inv_mats, void* out, int H, int W, int F, int size, void* stream);

/* ---- ControlNet (ldm/modules/diffusionmodules/controlnet.py): the hint encoder's convolution.  A 3x3 convolution, pad 1, stride s in {1, 2},
 * for the narrow channel counts the tuned 128-column tiles idle on, with bias and SiLU in the epilogue:
 *   y[b,i,j,n] = bias[n] + sum_{ky,kx,c<cin} w[n][ky][kx][c] * X[b, s*i+ky-1, s*j+kx-1, c]        (zero outside the image, fp32 accumulation)
 *   out[b,i,j,n] = fp16(act ? y * sigmoid(y) : y)      Ho = (H-1)/s + 1, Wo = (W-1)/s + 1, out fp16 NHWC [B,Ho,Wo,cout] tight
 * in_mode 0: x fp16 NHWC [B,H,W,cin] tight, cin % 16 == 0, 16 <= cin <= 256, X = x.
 * in_mode 1: x uint8 [B,H,W,3], cin = 3, X = x / 255: the bytes enter the products as the exact integers 0 .. 255 and the 1 / 255 multiplies
 *            the fp32 sum (no fp16 copy of the image exists, in memory or in rounding).
 * cout % 16 == 0, 16 <= cout <= 256.  bias fp32 [cout] or NULL (no bias).  act in {0, 1}.
 * Device weight layout: wt fp16 [cout][9 * cpad], cpad = cin rounded up to a multiple of 32 (3 -> 32, 16 -> 32, 96 -> 96, 256 -> 256),
 *   wt[n * 9 * cpad + (ky * 3 + kx) * cpad + c] = fp16(w[n][ky][kx][c]) for c < cin and ZERO for cin <= c < cpad.
 *   The zero rows are part of the contract: the kernel multiplies them with the zeros it supplies for the missing channels.
 * x (in_mode 0) and wt 16-byte aligned, out 8-byte, bias 4-byte.  out must not overlap x, wt or bias (the caller's duty, not checked).
 * One launch, no workspace, on `stream`.  Exactly B*Ho*Wo*cout elements of out are written; nothing outside x's B*H*W*cin elements, wt's
 * cout*9*cpad and bias's cout is read: the zero border comes from predication, not from a padded copy.
 * AF_E_BADARG before any launch (af_last_error() names the function): NULL x / wt / out, B, H or W below 1, in_mode outside {0, 1}, cin or cout
 * outside the above, a stride other than 1 or 2, act outside {0, 1}, a misaligned pointer, B*H*W*cin or B*Ho*Wo*cout at or above 2^31
 * (32-bit offsets), more than 65535 patch rows (Ho / 16 at stride 1, Ho / 8 at stride 2) or B times the number of channel slabs (at most cout / 16) above 65535. */
int af_hint_conv3x3(const void* x, int in_mode, int cin, const void* wt, const void* bias, void* out, int cout, int stride, int act, int B,
                    int H, int W, void* stream);

/* ---- scoring images (evaluation/vit.py, evaluation/eval_utils.py: the CLIP and DINO vision towers): the front of a ViT, one launch.
 * img_u8 uint8 [B, H, W, 3] (RGB) -> rows fp16 [B * P][kpad], P = (C / p)^2: what torchvision's Resize / CenterCrop / Normalize (or the HF ViT
 * feature extractor's square resize) followed by the unfold of a stride-p convolution produce, as the A operand of the patch-embedding GEMM.
 *   Resize target (Hr, Wr): keep_aspect = 1 is Resize(S): the shorter side becomes S, the longer (S * long) / short in integer division;
 *     keep_aspect = 0: Hr = Wr = C, S is ignored.
 *   Resampling, separable, torch's F.interpolate(antialias=True, align_corners=False) -- the family of the rule R stated above
 *     af_face_alpha_mask -- with a filter f of width w: filter = 0 the triangle max(0, 1 - |x|), w = 1; filter = 1 the cubic with a = -0.5,
 *     ((a + 2) x - (a + 3)) x^2 + 1 for |x| < 1, a (((x - 5) x + 8) x - 4) for 1 <= |x| < 2, 0 beyond, w = 2.  Per axis, n_in -> n_out:
 *     s = n_in / n_out, sc = max(s, 1), sup = w sc, c = s (i + 0.5); taps k in [max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5)));
 *     weight f((k - c + 0.5) / sc) / (its sum over the taps).  Tap ranges and the first tap's argument are formed in fp64, f and the sums
 *     in fp32 over the values 0 .. 255 (the division by the sum of the weights last), along x, then y; no rounding and no clamp in between: cubic overshoot below 0 and above 255 is kept, as torchvision keeps it on
 *     float tensors.  At s = 1 both filters are the identity.
 *   Centre crop C x C of the resized image: top = rne((Hr - C) / 2), left = rne((Wr - C) / 2), half to even (torchvision's int(round(.)) is
 *     Python's round).  Only pixels inside the crop are computed.
 *   Value: v * scale3[c] + shift3[c], one fp32 multiply and one fp32 add, rounded to fp16 once.  scale3 / shift3: HOST arrays of three floats
 *     (the caller passes 1 / (255 std) and -mean / std); they are read before the call returns.
 *   Layout: row b P + py (C / p) + px; column c p^2 + dy p + dx -- the flatten order of the convolution weight [E, 3, p, p], so
 *     weight.reshape(E, 3 p^2) is the GEMM's weight as it stands; columns 3 p^2 .. kpad - 1 are written as zeros (p = 14: 588 -> 640; a
 *     GEMM whose K runs to kpad reads them).
 * Any H, W >= 1, up-sizing and any ratio: the source footprint of a patch is walked in chunks, nothing is assumed to fit on chip.
 * AF_E_BADARG before any launch (af_last_error() names the function): a NULL pointer; B, H, W, C or p below 1; C % p != 0; keep_aspect with
 * C > S; kpad < 3 p^2 or kpad % 8 != 0; filter outside {0, 1}; B * H * W * 3 or B * P * kpad at or above 2^31; rows not 16-byte aligned.
 * AF_E_UNSUPPORTED: p > 32.  No workspace. */
int af_vit_patch_rows(const void* img_u8, void* rows, int B, int H, int W, int keep_aspect, int S, int C, int p, int filter,
                      const float* scale3, const float* shift3, int kpad, void* stream);
/* y = x * 0.5 * (1 + erf(x / sqrt(2))), fp16 in and out, fp32 inside (nn.GELU, the MLP of DINO's ViT): relative error below one fp16
 * rounding over the whole range, the negative tail included (formed as x * erfc(-x / sqrt 2) / 2, which does not cancel) */
int af_gelu_f16(const void* x, void* y, int64_t n, void* stream);

/* ---- trainable DoRA adapters on the U-Net's up_blocks.3 convolutions (adaface/diffusers_attn_lora_capture.py:541-591; peft
 * DoraConv2dLayer.forward: y = base(x) + (s - 1) * conv(xd, W) + s * scaling * B(A(xd)), xd = dropout(x)) ---------------------
 * out = y0 + u[c] * c2 + v[c] * lb   (fp16 [rows, C]; u = s - 1, v = s * scaling, fp32 [C]) */
int af_dora_combine(const void* y0, const void* c2, const void* lb, const void* u, const void* v, void* out, int64_t rows, int C,
                    void* stream);
/* out = a * b, fp16 (dropout: b holds 0 or 1 / (1 - p)) */
int af_mul_f16(const void* a, const void* b, void* out, int64_t n, void* stream);
/* x [B,H,W,C] fp16 -> out [B*Ho*Wo, 9*C] with column order (ky, kx, c), zero halo, pad 1: the explicit operand of a 3x3 conv's
 * weight gradient (a GEMM over pixels) */
int af_im2col3x3(const void* x, void* out, int B, int H, int W, int C, int stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADAFACE_HIP_H */
