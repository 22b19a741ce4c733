"""Tensor-level wrappers over the C ABI (include/adaface_hip.h).

torch is plumbing here: it owns device memory and the current HIP stream; every function
below hands raw device pointers to ``libadaface_hip.so`` and raises ``RuntimeError`` on any
failure.  There is no eager / CPU fallback.

Activation convention: fp16, channels-last.  A feature map is a contiguous tensor
``[B, H, W, C]`` (equivalently tokens ``[B, H*W, C]``).

Concurrency: launches go to ``torch.cuda.current_stream()``.  The caller-owned scratch the C ABI asks for (GroupNorm partials,
split-K slabs, attention-backward copies, the zero page) is cached here PER DEVICE, not per stream: the hot path is
single-stream by design (one process per GPU, one HIP stream, the hipGraph replays on it), so two streams of one process must
not run these wrappers concurrently.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import AF_ACT_GEGLU, AF_ACT_NONE, AF_ACT_QUICKGELU, AF_ACT_SILU, AF_OUT_F32, AF_OUT_NORMAL, AF_OUT_SPLIT_T, GemmDesc

F16 = torch.float16
NEG_MAX = -torch.finfo(torch.float32).max



def param_key(p):
    """Identity + modification state of a parameter, the key of every derived-weight cache (fp16 packs, merged adapters).
    `_version` only sees autograd-visible in-place writes; parameters that live in a flat optimizer arena
    (ldm.c_adamw.FlatArena) are rewritten by a raw HIP kernel / an in-place collective, so the arena hands each of them its
    generation counter (`p._af_gen`, a shared one-element list) and bumps it on every such write."""
    if p is None:
        return None
    gen = p.__dict__.get("_af_gen")          # (a failed getattr on a tensor costs as much as the rest of this function: ~14,000 calls per Stage-2 micro-batch)
    return (p.data_ptr(), p._version, p.device, gen[0] if gen is not None else -1)


def _stream() -> int:
    # the raw handle of torch's current stream on the current device: two C calls (~0.3 us) instead of the ~3 us of
    # torch.cuda.current_stream().cuda_stream -- this runs once per launch, ~11,000 times in a Stage-2 micro-batch
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _checked(name: str, *args) -> int:
    """Call the library's entry point ``name`` with ``args`` as they stand; RuntimeError (naming it) if it fails."""
    rc = getattr(_lib.lib(), name)(*args)
    _lib.check(rc, name)
    return rc


def _launch(name: str, *args, what: Optional[str] = None) -> int:
    """The same for a launch: ``args`` are the entry point's arguments up to its last one, the stream, which is the current one."""
    rc = getattr(_lib.lib(), name)(*args, _stream())
    _lib.check(rc, what or name)
    return rc


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk_f16(t: torch.Tensor, name: str):
    if t.dtype != F16 or not t.is_cuda or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous fp16 device tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- weights
@dataclass
class PackedWeight:
    """fp16 [Npad, Kpad] K-contiguous weight (+ fp32 bias) laid out for af_gemm."""
    wt: torch.Tensor
    bias: Optional[torch.Tensor]
    N: int
    K: int
    kpad: int
    taps: int = 1
    cin: int = 0  # channels per tap as seen by the kernel (after any channel padding)
    ln_cs: Optional[torch.Tensor] = None   # folded LayerNorm (pack_matrix_ln): fp32 [Npad] column sums of the fp16 rows
    ln_eps: float = 0.0
    k_tail: int = 0   # pack_conv3x3_skip: plain K columns behind the nine tap blocks (the ResBlock's 1x1 shortcut inside its second convolution)
    aliased: bool = False   # wt IS the caller's tensor (pack_matrix fast path): read-only -- in-place refresh paths must replace, never copy_ into it
    up2: bool = False       # pack_conv3x3_up2: rows [4 N] phase-major, K = 4 cin (conv3x3_up2 only)


def pack_matrix(w2d: torch.Tensor, bias: Optional[torch.Tensor], device, taps: int = 1, cin: int = 0) -> PackedWeight:
    """w2d: [N, K] (any float dtype, any device) -> zero-padded fp16 [roundup(N,128), roundup(K,64)]."""
    N, K = w2d.shape
    npad, kpad = round_up(N, 128), round_up(K, 64)
    if ((npad, kpad) == (N, K) and w2d.dtype == F16 and w2d.is_contiguous() and w2d.device == torch.device(device) and not w2d.requires_grad
            and not isinstance(w2d, torch.nn.Parameter)):
        # already in the packed layout (an fp16 activation used as the B operand of a product: the feature-matching losses' 4096-row matrices):
        # no zero-fill, no copy.  The pack ALIASES the caller's tensor and is marked so (read-only: refresh-in-place code checks `aliased`);
        # parameters never take this path, frozen fp16 ones included
        b = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        return PackedWeight(w2d, b, N, K, kpad, taps, cin if cin else K, aliased=True)
    wt = torch.zeros((npad, kpad), dtype=F16, device=device)
    wt[:N, :K] = w2d.detach().to(device=device, dtype=F16)
    b = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
    return PackedWeight(wt, b, N, K, kpad, taps, cin if cin else K)


def pack_matrix_ln(w2d: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float, device) -> PackedWeight:
    """Weight of a Linear that consumes LayerNorm(x) (BasicTransformerBlock.norm1/2/3 -> attn1 q|k|v, attn2.to_q, ff GEGLU projection;
    reference attention.py:242-252), packed so that af_gemm can take the UN-normalised rows:
        LN(x) W^T + b = rstd * (x (gamma * W)^T - mean * colsum(gamma * W)) + (b + W beta).
    The kernel accumulates mean / rstd of each row from the A fragments of its own main loop (af_gemm_desc.ln_colsum).  Column sums are
    taken over the fp16-rounded packed rows, so the rank-one correction cancels the mean term exactly as the MFMAs saw it."""
    w = w2d.detach().to(device=device, dtype=torch.float32)
    g, bt = gamma.detach().to(device=device, dtype=torch.float32), beta.detach().to(device=device, dtype=torch.float32)
    b = (w * bt[None, :]).sum(dim=1)                       # W beta (element-wise: no vendor gemv for a one-off pack)
    if bias is not None:
        b = b + bias.detach().to(device=device, dtype=torch.float32)
    pw = pack_matrix(w * g[None, :], b, device)
    pw.ln_cs = pw.wt.float().sum(dim=1).contiguous()
    pw.ln_eps = float(eps)
    return pw


def pack_conv3x3(w: torch.Tensor, bias: Optional[torch.Tensor], device, cin_pad: int = 0) -> PackedWeight:
    """[Cout, Cin, 3, 3] -> [Cout, 9*Cin'] with K order (ky, kx, cin); Cin' = max(Cin, cin_pad)."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    w = w.detach().permute(0, 2, 3, 1)  # [Cout, 3, 3, Cin]
    cinp = max(cin, cin_pad)
    if cinp != cin:
        w = torch.nn.functional.pad(w, (0, cinp - cin))
    return pack_matrix(w.reshape(cout, 9 * cinp), bias, device, taps=9, cin=cinp)


def pack_conv3x3_skip(w3: torch.Tensor, b3: Optional[torch.Tensor], w1: torch.Tensor, b1: Optional[torch.Tensor], device) -> PackedWeight:
    """out = conv3x3(h; w3, b3) + conv1x1(x; w1, b1) as ONE K-concatenated implicit GEMM (af_gemm_desc.a3 / a4): [Cout, 9 Cin | Cs] with the 3x3
    block in (ky, kx, cin) order and the 1x1 weights behind it; the biases add up.  The ResBlock's out_layers convolution + skip_connection
    (openaimodel.py:256-276).  Cin and Cs must be multiples of 64 (every SD-1.5 block is)."""
    cout, cin, kh, kw = w3.shape
    assert kh == 3 and kw == 3 and w1.shape[0] == cout and w1.shape[2:] == (1, 1)
    cs = w1.shape[1]
    assert cin % 64 == 0 and cs % 64 == 0, "pack_conv3x3_skip: channel counts must be multiples of 64"
    w = torch.cat([w3.detach().permute(0, 2, 3, 1).reshape(cout, 9 * cin).float(), w1.detach().reshape(cout, cs).float().to(w3.device)], dim=1)
    b = None
    if b3 is not None or b1 is not None:
        b = torch.zeros(cout, dtype=torch.float32, device=w3.device)
        if b3 is not None:
            b = b + b3.detach().float()
        if b1 is not None:
            b = b + b1.detach().float().to(b.device)
    pw = pack_matrix(w, b, device, taps=9, cin=cin)
    pw.k_tail = cs
    return pw


def up2_phase_weights(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [4, Cout, 2, 2, Cin] in w's dtype: nearest x2 followed by the 3x3 convolution is, for the output pixels of parity (py, px),
    a 2x2 convolution of the LOW-res image over the offsets {py - 1, py} x {px - 1, px} (tap i of output row 2y + py reads source row
    y + floor((py + i - 1) / 2)).  Its weights are the sums of the 3x3 weights that fold onto one source pixel:
        py = 0: a = 0 <- w0,       a = 1 <- w1 + w2          py = 1: a = 0 <- w0 + w1,  a = 1 <- w2          (the same in x)
    phase = 2 py + px.  Pass fp32 (or fp64) weights: the sums are meant to be rounded to fp16 ONCE, afterwards."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    fold = w.new_zeros((2, 2, 3))                                 # fold[parity, a, tap] = 1 where the tap lands on offset a
    fold[0, 0, 0] = fold[0, 1, 1] = fold[0, 1, 2] = 1
    fold[1, 0, 0] = fold[1, 0, 1] = fold[1, 1, 2] = 1
    return torch.einsum("pai,qbj,ocij->pqoabc", fold, fold, w).reshape(4, cout, 2, 2, cin)


def pack_conv3x3_up2(w: torch.Tensor, bias: Optional[torch.Tensor], device) -> PackedWeight:
    """The phase pack of a 3x3 convolution that runs behind a nearest-x2 upsample (af_gemm_desc.upsample = 3): [4 Cout, 4 Cin], rows phase-major,
    K order (a, b, cin); the sums formed in fp32 from the parameter and rounded to fp16 once (summing the rounded fp16 weights is 1.4x further
    from fp64).  The bias stays the original [Cout]."""
    cout, cin = w.shape[:2]
    wp = up2_phase_weights(w.detach().to(device=device, dtype=torch.float32)).reshape(4 * cout, 4 * cin)
    pw = pack_matrix(wp, bias, device, taps=9, cin=cin)
    pw.N, pw.up2 = cout, True
    return pw


def pack_ff_proj_out(w2: torch.Tensor, b2: Optional[torch.Tensor], wp: torch.Tensor, bp: Optional[torch.Tensor], device) -> PackedWeight:
    """The feed-forward's second projection with the SpatialTransformer's proj_out folded behind it, as ONE K-concatenated GEMM over [g ; x2]:
        x_in + b_p + W_p (x2 + b2 + W2 g) = x_in + (W_p b2 + b_p) + [W_p W2 | W_p] [g ; x2]
    -> [C, 4C + C] (w2 [C, 4C], wp [C, C] or [C, C, 1, 1]).  The product and the bias are formed in fp32 from the parameters and rounded to fp16 once,
    as pack_conv3x3_up2 forms its sums.  A pure function of its four tensors."""
    w2f = w2.detach().to(device=device, dtype=torch.float32)
    wpf = wp.detach().to(device=device, dtype=torch.float32).reshape(wp.shape[0], -1)
    assert wpf.shape[1] == w2f.shape[0], f"pack_ff_proj_out: proj_out takes {wpf.shape[1]} channels, the feed-forward gives {w2f.shape[0]}"
    b = None
    if b2 is not None:
        b = (wpf * b2.detach().to(device=device, dtype=torch.float32)[None, :]).sum(dim=1)
    if bp is not None:
        bpf = bp.detach().to(device=device, dtype=torch.float32)
        b = bpf if b is None else b + bpf
    # W_p W2 element-wise, a few output rows at a time (at most 2^26 products in flight): no vendor GEMM for a one-off pack, as pack_matrix_ln
    rows = max(1, (1 << 26) // (wpf.shape[1] * w2f.shape[1]))
    prod = torch.cat([(wpf[i:i + rows, :, None] * w2f[None, :, :]).sum(dim=1) for i in range(0, wpf.shape[0], rows)], dim=0)
    return pack_matrix(torch.cat([prod, wpf], dim=1), b, device)


def interleave_geglu(w: torch.Tensor, b: torch.Tensor):
    """GEGLU projection [2*inner, C]: rows [value | gate] -> 16-row groups [16 value, 16 gate, ...]
    so value and gate of a channel land in the same lane / register of adjacent MFMA tiles."""
    inner = w.shape[0] // 2
    assert inner % 16 == 0
    wv, wg = w[:inner].reshape(inner // 16, 16, -1), w[inner:].reshape(inner // 16, 16, -1)
    wi = torch.stack([wv, wg], dim=1).reshape(2 * inner, -1)
    bv, bg = b[:inner].reshape(inner // 16, 16), b[inner:].reshape(inner // 16, 16)
    bi = torch.stack([bv, bg], dim=1).reshape(2 * inner)
    return wi, bi


# ----------------------------------------------------------------------------- launch tuning
# (tile, splits) per GEMM shape, measured on an MI355X by tools/autotune_gemm.py and committed as
# tuning/gfx950_gemm.json; shapes not in the table use the library's heuristic (tile 0, no split).
import json as _json
import os as _os

_TUNE_PATH = _os.environ.get("AF_TUNE_TABLE") or _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "tuning", "gfx950_gemm.json")
_tune_table = None
def conv_halo_eligible(d) -> bool:
    """Whether af_gemm runs descriptor ``d`` on the halo-resident 3x3 kernel when asked for tile 14 / 19 -- the library's own launch predicate
    (af_gemm_halo_variant, csrc/af_gemm3.hip::conv3h_variant; no launch, operand pointers are not read).  The table's key carries no image
    geometry, so a tabled or default tile 14 can meet a latent outside that scope (W not 8 / 16 / 32 / 64, ragged rows, ...); the library then
    falls back to the register-staged kernel, which writes no GroupNorm statistics and has no K tail.  Every caller that depends on the kernel
    really running asks here: _launch_gemm (VAE_HALO_DEFAULT, producer statistics), conv3x3 (K tail), tools/autotune_gemm.py, the tuned-shape tests."""
    return _lib.lib().af_gemm_halo_variant(C.byref(d)) != 0


_tune_recorder = None      # set by tools/autotune_gemm.py: callable(key, desc, device) -> (tile, splits)
_splitk_ws = {}
SPLITK_WS_BYTES = 192 << 20


def tune_table():
    global _tune_table
    if _tune_table is None:
        try:
            with open(_TUNE_PATH) as f:
                _tune_table = {k: tuple(v) for k, v in _json.load(f).items()}
        except FileNotFoundError:
            _tune_table = {}
    return _tune_table


_zero_pages = {}


def _zero_page(device) -> torch.Tensor:
    z = _zero_pages.get(device)
    if z is None:
        z = torch.zeros(64, dtype=F16, device=device)
        _zero_pages[device] = z
    return z


def _splitk_workspace(device) -> torch.Tensor:
    """fp32 partial slabs + (last AF_SPLITK_COUNTER_BYTES) the per-tile arrival counters of the in-kernel reduction, which must be
    zero between launches: zeroed here once, every launch restores them."""
    key = device if _ws_lane == 0 else (device, _ws_lane)
    ws = _splitk_ws.get(key)
    if ws is None:
        ws = torch.empty((SPLITK_WS_BYTES // 4,), dtype=torch.float32, device=device)
        ws[-(_lib.AF_SPLITK_COUNTER_BYTES // 4):].zero_()
        _splitk_ws[key] = ws
    return ws


_ws_lane = 0


def set_workspace_lane(lane: int) -> int:
    """Launches issued from now on use split-K workspace number ``lane`` (0 = the default one).  The slab workspace is the one piece of scratch every
    launch of a device shares; a caller that runs two independent passes CONCURRENTLY on two streams (tools/probes/r06w_two_streams.py) gives each stream
    its own lane while it issues that stream's launches.  Returns the previous lane."""
    global _ws_lane
    prev, _ws_lane = _ws_lane, int(lane)
    return prev


# split-K with at most this many slices is reduced inside the GEMM launch by the last-arriving workgroup of each tile (one launch
# instead of two: af_gemm_desc.splitk_fused).  MEASURED SLOWER than the chip-wide reduce pass on every shape of this path but two
# tiny ones (profiles/r02e_splitk_fused.txt: e.g. M2048 N1280 K1280 x2: 29.1 vs 24.5 us, conv 8x16x16 1280->1280 x4: 89.3 vs
# 78.3 us -- the one reducer workgroup per tile reads its slabs at a dependent-latency rate while the separate pass spreads them
# over all CUs and the launch boundary costs only ~1.5 us under graph replay), so the default is 0 = never; the path stays
# available (bit-identical results, tests/test_hip_kernels.py) for callers whose launch boundaries are expensive.
VAE_HALO_DEFAULT = _os.environ.get("AF_VAE_HALO_DEFAULT", "1") != "0"     # untabled VAE-kind 3x3 shapes go to the halo-resident kernel (see _launch_gemm)
SPLITK_FUSED_MAX = int(_os.environ.get("AF_SPLITK_FUSED_MAX", "0"))


# Round 5: the same in-kernel reduction chosen by SIZE for the register-staged tiles (1 / 2): when all slabs of a launch together are at most this
# many bytes (the training legs' batch-1 passes: M 64 ... 1024 rows, a few output tiles, 2 - 16 slices) the reduce pass is a ~5 us launch that moves
# a few hundred KB, and the last-arriving workgroup of a tile reads its slabs in about a microsecond.  0 = off.
SPLITK_FUSED_BYTES = int(_os.environ.get("AF_SPLITK_FUSED_BYTES", "0"))


# Round 5: tile 18 (fragments straight from global memory, no LDS / barrier / split-K) for the SMALL plain GEMMs the table or the heuristic would
# give to the register-staged 64 x 64 tile (tile 2, often with split-K): at most this many rows, K <= SMALL_GEMM_MAX_K.  0 rows = off.
SMALL_GEMM_MAX_M = int(_os.environ.get("AF_SMALL_GEMM_MAX_M", "0"))
SMALL_GEMM_MAX_K = int(_os.environ.get("AF_SMALL_GEMM_MAX_K", "3072"))


GN_FROM_PRODUCER = _os.environ.get("AF_GN_FROM_PRODUCER", "1") != "0"   # GroupNorm statistics from the producing GEMM's epilogue (0: always a statistics pass)


class GnPartials:
    """Partial GroupNorm statistics of a tensor, written by the GEMM launch that produced it (af_gemm_desc.gn_partials).  They describe the
    bytes that launch stored: `attach` records the tensor's storage address and autograd version, and `partials_of` hands them out only
    while both still match -- an in-place write between the producer and the GroupNorm (`y.add_(1)`, `copy_`) bumps the version, the
    statistics are dropped and the consumer runs its own statistics pass."""
    __slots__ = ("ws", "nblk", "cpg", "B", "hw", "C", "ptr", "version")

    def __init__(self, ws, nblk, cpg, B, hw, C):
        self.ws, self.nblk, self.cpg, self.B, self.hw, self.C = ws, nblk, cpg, B, hw, C
        self.ptr, self.version = 0, -1

    @classmethod
    def alloc(cls, device, B: int, hw: int, C: int, cpg: int) -> "GnPartials":
        """The workspace a producing launch fills for B images of hw rows (128-row blocks) x C channels in groups of cpg: [B][128 blocks][32 groups][sum, sumsq]."""
        return cls(torch.empty((B, 128, 32, 2), dtype=torch.float32, device=device), hw // 128, cpg, B, hw, C)

    def attach(self, t: torch.Tensor) -> torch.Tensor:
        self.ptr, self.version = t.data_ptr(), t._version
        t._gn_partials = self
        return t


def partials_of(x: torch.Tensor) -> Optional["GnPartials"]:
    """The statistics x's producer left, or None when there are none or x has been written since (views share the version counter)."""
    gn = getattr(x, "_gn_partials", None)
    if gn is None or gn.ptr != x.data_ptr() or gn.version != x._version:
        return None
    return gn


class WeightPrefetcher:
    """Weight prefetch on a SECOND stream inside a captured step (round 5 experiment; bench.py --prefetch-stream).

    Inside a denoise step every GEMM meets its weights cold in HBM (1.72 GB stream through once per U-Net pass; the GEMM family takes 7.0 ms
    on warm operands and 8.6 ms in the step, profiles/r04v_*).  The in-kernel prologue touch (af_common.h) only covers the first K stages.
    This object replays the step's own launch order: `record()` + one eager pass notes (weight pointer, bytes) of every weight-consuming
    launch; during the capture, in front of launch i the side stream waits for the main stream's position (so it runs beside launch i) and
    reads the weights of launch i + depth (af_prefetch_ex: one dword per 128-byte line, a capped grid), which brings them into the
    Infinity Cache (and 1/8 of them into the consumer XCD's L2).  The main stream never waits for the side stream except once at the end
    of the capture (`join`): the prefetch is a hint, results are bit-identical with and without it."""

    def __init__(self, depth: int = 2, max_workgroups: int = 64, min_bytes: int = 1 << 18):
        self.depth, self.max_wg, self.min_bytes = depth, max_workgroups, min_bytes
        self.plan, self.mode, self.i, self.side, self.issued = [], None, 0, None, 0

    def record(self):
        self.plan, self.mode = [], "record"
        return self

    def play(self, side_stream):
        self.mode, self.i, self.side, self.issued = "play", 0, side_stream, 0
        return self

    def stop(self):
        self.mode = None

    def note(self, ptr: int, nbytes: int):
        if self.mode == "record":
            self.plan.append((ptr, nbytes))
        elif self.mode == "play":
            i = self.i
            self.i = i + 1
            j = i + self.depth
            if i < len(self.plan) and self.plan[i][0] != ptr:
                raise RuntimeError("WeightPrefetcher: the captured pass does not follow the recorded launch order")
            if j < len(self.plan) and self.plan[j][1] >= self.min_bytes and torch.cuda.is_current_stream_capturing():
                ev = torch.cuda.Event()
                ev.record()                                  # the main stream's position: everything before launch i
                self.side.wait_event(ev)
                _checked("af_prefetch_ex", self.plan[j][0], self.plan[j][1], self.max_wg, self.side.cuda_stream)
                self.issued += 1

    def join(self):
        """End of the capture: the forked stream must rejoin the capturing one."""
        if self.mode == "play" and self.side is not None and self.issued:
            torch.cuda.current_stream().wait_stream(self.side)
        self.mode = None


_weight_prefetcher: Optional[WeightPrefetcher] = None


def set_weight_prefetcher(p: Optional[WeightPrefetcher]):
    global _weight_prefetcher
    _weight_prefetcher = p


def _pf_note(*weights):
    if _weight_prefetcher is not None and _weight_prefetcher.mode is not None:
        for w in weights:
            _weight_prefetcher.note(w.data_ptr(), w.numel() * w.element_size())


def _launch_gemm(d: "GemmDesc", device, what: str, tile: int = 0, splits: int = 0, gn_cpg: int = 0):
    """Pick (tile, splits) -- explicit args > recorder (autotune) > table > heuristic -- and launch.  gn_cpg > 0: the caller's output feeds a
    GroupNorm with groups of gn_cpg channels; when the chosen launch can (af_gemm_gn_stats_ok) it also writes the partial statistics and a
    GnPartials is returned (None otherwise)."""
    if tile == 0 and splits == 0:
        key = f"{d.taps},{d.M},{d.N},{d.K},{d.act},{d.out_mode},{d.stride},{d.upsample}"
        if d.ln_colsum:
            key += ",ln"
        if _tune_recorder is not None:
            tile, splits = _tune_recorder(key, d, device)
        else:
            tile, splits = tune_table().get(key, (0, 1))
            if d.ln_colsum and tile == 0:
                tile, splits = tune_table().get(key[:-3], (0, 1))
            if VAE_HALO_DEFAULT and tile == 0 and d.taps == 9 and d.N % 160 != 0 and d.M >= 16384 and conv_halo_eligible(d):
                # a 3x3 convolution of the VAE's kind (128-multiples of channels over many pixels) at a batch size the table has not met: the halo-resident
                # kernel's 256 x 128 forms win every such shape the table holds by 20 - 40 % (profiles/r06t_try14.log)
                tile, splits = 14, 1
    if (SMALL_GEMM_MAX_M and tile in (0, 2) and d.taps == 1 and d.M <= SMALL_GEMM_MAX_M and d.K <= SMALL_GEMM_MAX_K and not d.a2 and not d.ln_colsum
            and d.act != AF_ACT_GEGLU and d.out_mode != AF_OUT_SPLIT_T and d.K % 8 == 0 and _tune_recorder is None
            and (tile == 2 or (d.M * d.N <= (1 << 21)))):
        tile, splits = 18, 1                                  # the library falls back to tile 2 if a stride / alignment rule is not met
    if d.ln_colsum:
        # the folded LayerNorm lives in the whole-line kernel only (tiles 7 .. 13, 16, 17), unsplit
        splits = 1
        if tile < 7 or tile in (14, 15) or tile > 17 or (tile in (9, 10) and d.act != AF_ACT_GEGLU) or (tile in (16, 17) and d.act == AF_ACT_GEGLU):
            if d.act == AF_ACT_GEGLU:
                tile = 7 if d.N % 256 == 0 else 8
            else:
                tile = 7 if (d.N % 320 == 0 and d.M >= 8192) else 8
    d.tile = tile
    d.zeros = _zero_page(device).data_ptr()
    f32 = d.out_mode == AF_OUT_F32
    d.splits = max(1, splits)
    if d.splits > 1:
        if d.act == AF_ACT_GEGLU or d.out_mode == AF_OUT_SPLIT_T:
            d.splits = 1
        else:
            ws = _splitk_workspace(device)
            d.splits = max(1, min(d.splits, (ws.numel() * 4 - _lib.AF_SPLITK_COUNTER_BYTES) // (d.M * d.N * 4)))
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
            small = d.tile in (0, 1, 2) and d.splits <= 16 and d.splits * d.M * d.N * 4 <= SPLITK_FUSED_BYTES
            d.splitk_fused = int((d.splits <= SPLITK_FUSED_MAX or small) and not f32)
    gn = None
    if gn_cpg and GN_FROM_PRODUCER and _tune_recorder is None:
        rpb = d.rows_per_batch if d.rows_per_batch > 0 else d.M
        if (d.tile not in (14, 19) or conv_halo_eligible(d)) and d.M % rpb == 0 and d.ld_out in (0, d.N) \
                and _lib.lib().af_gemm_gn_stats_ok(d.tile, d.splits, d.taps, d.act, d.out_mode, d.N, gn_cpg, rpb) == 1:
            gn = GnPartials.alloc(device, d.M // rpb, rpb, d.N, gn_cpg)
            d.gn_partials, d.gn_cpg = gn.ws.data_ptr(), gn_cpg
    if _weight_prefetcher is not None and _weight_prefetcher.mode is not None:
        _weight_prefetcher.note(int(d.wt), int(d.kpad) * round_up(int(d.N) * (4 if d.upsample == 3 else 1), 128) * 2)
    _launch("af_gemm", C.byref(d), what=what)
    return gn


# ----------------------------------------------------------------------------- gemm / conv
def gemm(a1: torch.Tensor, pw: PackedWeight, *, a2: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
         rows_per_batch: int = 0, residual: Optional[torch.Tensor] = None, act: int = AF_ACT_NONE,
         split_col: int = 0, ld_out2: int = 0, tile: int = 0, splits: int = 0, out_f32: bool = False, gn_cpg: int = 0,
         out: Optional[torch.Tensor] = None):
    """Plain-rows GEMM: a1 [M, K1] (+ a2 [M, K2], concatenated along K) x pw.  Returns out
    ([M, N], or [M, N/2] for GEGLU), or (out [M, split_col], out2 [B, N-split_col, ld_out2]).  out_f32: the fp32 accumulator is
    returned (AF_OUT_F32; weight gradients).  out: a contiguous fp16 [M, N] tensor to write instead of a fresh one (standard epilogue only)
    -- a slice of a batch's output when the weights differ per sample (adaface/gfpgan.py)."""
    _chk_f16(a1, "gemm.a1")
    M, k1 = a1.shape
    k2 = 0
    if a2 is not None:
        _chk_f16(a2, "gemm.a2")
        k2 = a2.shape[1]
        assert a2.shape[0] == M
    assert k1 + k2 == pw.K, f"gemm: K mismatch {k1}+{k2} vs {pw.K}"
    assert out is None or not (split_col or out_f32), "gemm: out= goes with the standard fp16 epilogue only"
    d = GemmDesc()
    d.a1, d.a2, d.wt, d.bias = _p(a1), _p(a2), _p(pw.wt), _p(pw.bias)
    d.rowbias, d.residual = _p(rowbias), _p(residual)
    d.M, d.N, d.K, d.kpad, d.taps = M, pw.N, pw.K, pw.kpad, 1
    d.c1, d.c2, d.lda1, d.lda2 = k1, k2, k1, k2
    d.rows_per_batch = rows_per_batch
    d.ld_rowbias = 0 if rowbias is None else rowbias.stride(0)
    d.act = act
    if pw.ln_cs is not None:
        assert a2 is None and not out_f32, "gemm: a folded LayerNorm takes one source and the fp16 epilogues"
        d.ln_colsum, d.ln_eps = _p(pw.ln_cs), pw.ln_eps
    out2 = None
    if split_col:
        assert rows_per_batch > 0 and M % rows_per_batch == 0
        nb = M // rows_per_batch
        ld_out2 = ld_out2 or round_up(rows_per_batch, 8)
        out = torch.empty((M, split_col), dtype=F16, device=a1.device)
        out2 = torch.empty((nb, pw.N - split_col, ld_out2), dtype=F16, device=a1.device)
        d.out_mode, d.split_col, d.ld_out2, d.out2 = AF_OUT_SPLIT_T, split_col, ld_out2, _p(out2)
    elif out_f32:
        assert act == AF_ACT_NONE and pw.N % 4 == 0
        out = torch.empty((M, pw.N), dtype=torch.float32, device=a1.device)
        d.out_mode = AF_OUT_F32
    elif out is not None:
        _chk_f16(out, "gemm.out")
        assert act != AF_ACT_GEGLU and tuple(out.shape) == (M, pw.N), f"gemm: out must be [{M}, {pw.N}], got {tuple(out.shape)}"
    else:
        n_out = pw.N // 2 if act == AF_ACT_GEGLU else pw.N
        out = torch.empty((M, n_out), dtype=F16, device=a1.device)
    if residual is not None:
        _chk_f16(residual, "gemm.residual")
        assert residual.shape == out.shape
    d.out = _p(out)
    gn = _launch_gemm(d, a1.device, "af_gemm", tile, splits, gn_cpg=0 if (split_col or out_f32) else gn_cpg)
    if gn is not None:
        gn.attach(out)                   # rides on the tensor object: GroupNorm32.hip picks it up (ops.groupnorm)
    return (out, out2) if split_col else out


def conv3x3_skip_tile(M: int, N: int, cin: int, ktail: int):
    """(tile, splits) for a 3x3 convolution with a K-concatenated 1x1 tail: its own tuned entry when the table has one on a whole-line tile,
    else what the table says for the plain convolution of the same shape (the tail only lengthens K), else a whole-line default."""
    for K in (9 * cin + ktail, 9 * cin):
        t = tune_table().get(f"9,{M},{N},{K},0,0,1,0")
        if t is not None and 7 <= t[0] <= 14:          # (14: the halo-resident kernel takes the tail since round 6; outside its scope conv3x3 takes _whole_line_tile)
            return t
    return _whole_line_tile(M, N), 1


def _whole_line_tile(M: int, N: int) -> int:
    """The whole-line tap-by-tap tile for a 3x3 convolution the table has no (usable) entry for: 128 x 320, 128 x 160 or 128 x 128."""
    return 7 if (N % 320 == 0 and M >= 8192) else (11 if N % 160 == 0 else 8)


def conv3x3(x: torch.Tensor, pw: PackedWeight, *, x2: Optional[torch.Tensor] = None, stride: int = 1, upsample: bool = False,
            rowbias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, tile: int = 0,
            splits: int = 0, out_hw=None, tap_shift: int = 0, skip=None, gn_cpg: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / pad 1 convolution as implicit GEMM (tap_shift=1: padding (0, 1, 0, 1) instead, the VAE encoder's Downsample).  x [B,H,W,C1] (+ x2 [B,H,W,C2] channel-concat)
    -> [B,Ho,Wo,Cout].  rowbias [B, >=Cout] is added per batch item (time-embedding), residual
    [B,Ho,Wo,Cout] after it.  out: a contiguous fp16 [B,Ho,Wo,Cout] tensor to write instead of a fresh one."""
    _chk_f16(x, "conv3x3.x")
    B, H, W, c1 = x.shape
    c2 = 0
    if x2 is not None:
        _chk_f16(x2, "conv3x3.x2")
        assert x2.shape[:3] == x.shape[:3]
        c2 = x2.shape[3]
    assert pw.taps == 9 and pw.cin == c1 + c2, f"conv3x3: channel mismatch {c1}+{c2} vs {pw.cin}"
    assert (pw.k_tail > 0) == (skip is not None), "conv3x3: a weight packed with a 1x1 tail (pack_conv3x3_skip) needs skip=(s1, s2 | None), and vice versa"
    he, we = (2 * H, 2 * W) if upsample else (H, W)
    ho, wo = (he + 2 - 3) // stride + 1, (we + 2 - 3) // stride + 1
    if int(upsample) == 2:      # zero-inserted image (stride-2 dgrad): output size = forward input size
        ho, wo = out_hw if out_hw is not None else (2 * H, 2 * W)
        assert ho in (2 * H, 2 * H - 1) and wo in (2 * W, 2 * W - 1)
    if out is None:
        out = torch.empty((B, ho, wo, pw.N), dtype=F16, device=x.device)
    else:
        _chk_f16(out, "conv3x3.out")
        assert tuple(out.shape) == (B, ho, wo, pw.N), f"conv3x3: out must be {(B, ho, wo, pw.N)}, got {tuple(out.shape)}"
    d = GemmDesc()
    d.a1, d.a2, d.wt, d.bias = _p(x), _p(x2), _p(pw.wt), _p(pw.bias)
    d.rowbias, d.residual, d.out = _p(rowbias), _p(residual), _p(out)
    d.M, d.N, d.K, d.kpad, d.taps = B * ho * wo, pw.N, pw.K, pw.kpad, 9
    d.c1, d.c2 = c1, c2
    d.B, d.H, d.W, d.Ho, d.Wo = B, H, W, ho, wo
    d.stride, d.upsample, d.tap_shift = stride, int(upsample), int(tap_shift)
    d.rows_per_batch = ho * wo
    d.ld_rowbias = 0 if rowbias is None else rowbias.stride(0)
    if residual is not None:
        _chk_f16(residual, "conv3x3.residual")
        assert residual.shape == out.shape
    if skip is not None:
        # the 1x1 tail reads s1 (| s2) at the output pixel: same grid as the output, stride 1
        s1, s2 = skip
        assert stride == 1 and not upsample and not tap_shift and (ho, wo) == (H, W)
        _chk_f16(s1, "conv3x3.skip")
        assert s1.shape[:3] == out.shape[:3]
        c3, c4 = s1.shape[3], 0
        if s2 is not None:
            _chk_f16(s2, "conv3x3.skip2")
            assert s2.shape[:3] == out.shape[:3]
            c4 = s2.shape[3]
        assert c3 + c4 == pw.k_tail, f"conv3x3: skip channels {c3}+{c4} vs the packed tail {pw.k_tail}"
        d.a3, d.a4, d.c3, d.c4, d.lda3, d.lda4 = _p(s1), _p(s2), c3, c4, c3, c4
        if tile == 0 and splits == 0 and _tune_recorder is None:
            tile, splits = conv3x3_skip_tile(d.M, d.N, c1 + c2, pw.k_tail)
            if tile == 14 and not conv_halo_eligible(d):
                tile, splits = _whole_line_tile(d.M, d.N), 1          # (the kernel tile 14 falls back to has no K tail)
    gn = _launch_gemm(d, x.device, "af_gemm(conv3x3)", tile, splits, gn_cpg=gn_cpg)
    if gn is not None:
        gn.attach(out)
    return out


# The phase form at the 8 x 8 level runs on a whole-line tile under split-K, and which tile and how many slices pay is a per-shape measurement:
# (output rows, Cout, 4 Cin) -> (tile, splits), the fastest of an isolated sweep (profiles/r08_fold_proj_out_up2_8x8.txt).  Kept apart from
# tuning/gfx950_gemm.json, whose keys describe launches the tuned-shape sweep can rebuild from the key alone.
UP2_SPLITK_SHAPES = {(2048, 1280, 5120): (7, 4)}


def conv_up2_config(B: int, H: int, W: int, c1: int, cout: int):
    """(tile, splits) Conv2d.hip asks the phase form of nearest x2 + 3x3 for at this shape: the halo-resident kernel (tile 14, unsplit) -- the 16 x 16
    and 32 x 32 levels -- or, for the 8 x 8 shapes of UP2_SPLITK_SHAPES, their measured whole-line tile and split count.  An 8 x 8 shape that has not
    been measured keeps the nine-tap launch (tile 14 is outside the form's scope there: conv_up2_eligible says no)."""
    return UP2_SPLITK_SHAPES.get((B * 4 * H * W, cout, 4 * c1), (14, 1)) if (H, W) == (8, 8) else (14, 1)


def conv_up2_desc(B: int, H: int, W: int, c1: int, cout: int, *, c2: int = 0, rowbias=None, residual=None, tile: int = 14, splits: int = 1) -> "GemmDesc":
    """The descriptor of nearest x2 + 3x3 in its phase form (upsample = 3; K = 4 c1 on the pack_conv3x3_up2 weights), shape and mode fields, the launch
    configuration and the epilogue operands only -- what conv_up2_eligible reads."""
    d = GemmDesc()
    d.tile = tile
    d.rowbias, d.residual = _p(rowbias), _p(residual)
    d.M, d.N, d.K, d.kpad, d.taps = B * 4 * H * W, cout, 4 * c1, round_up(4 * c1, 64), 9
    d.c1, d.c2 = c1, c2
    d.B, d.H, d.W, d.Ho, d.Wo = B, H, W, 2 * H, 2 * W
    d.stride, d.upsample = 1, 3
    d.rows_per_batch = 4 * H * W
    d.ld_rowbias = 0 if rowbias is None else rowbias.stride(0)
    d.splits = splits
    return d


def conv_up2_eligible(d) -> bool:
    """Whether af_gemm runs the phase-form descriptor ``d`` (conv_up2_desc) -- the library's own launch predicate, as conv_halo_eligible: 4 = the
    halo-resident kernel's phase form (tile 14, unsplit), 5 = the whole-line tile d.tile under split-K with the phase-mapped reduce (the 8 x 8 level)."""
    return _lib.lib().af_gemm_halo_variant(C.byref(d)) in (4, 5)


def conv3x3_up2(x: torch.Tensor, pw: PackedWeight, *, tile: int = 14, splits: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Nearest x2 + 3x3 / pad 1 as four 2x2 phase convolutions of x [B,H,W,Cin] -> [B,2H,2W,Cout] (pw from pack_conv3x3_up2).  Runs inside
    conv_up2_eligible only (tile, splits: conv_up2_config): outside it the library refuses (callers ask first and keep conv3x3(upsample=True)).
    out: a contiguous fp16 [B,2H,2W,Cout] tensor to write instead of a fresh one."""
    _chk_f16(x, "conv3x3_up2.x")
    B, H, W, c1 = x.shape
    assert pw.up2 and pw.cin == c1, f"conv3x3_up2: needs a pack_conv3x3_up2 weight of {c1} input channels"
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, pw.N), dtype=F16, device=x.device)
    else:
        _chk_f16(out, "conv3x3_up2.out")
        assert tuple(out.shape) == (B, 2 * H, 2 * W, pw.N), f"conv3x3_up2: out must be {(B, 2 * H, 2 * W, pw.N)}, got {tuple(out.shape)}"
    d = conv_up2_desc(B, H, W, c1, pw.N, tile=tile, splits=splits)
    assert d.K == pw.K and d.kpad == pw.kpad
    d.a1, d.wt, d.bias, d.out = _p(x), _p(pw.wt), _p(pw.bias), _p(out)
    _launch_gemm(d, x.device, "af_gemm(conv3x3_up2)", tile, splits)
    return out


def ff_fused(x2d: torch.Tensor, pw1: PackedWeight, pw2: PackedWeight, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = residual + b2 + W2 (v * gelu(g)), [v | g] = W1 LN(x) + b1 in one launch (af_ff_fused; C = 320 only).  pw1: the GEGLU-
    interleaved first projection, normally with the LayerNorm folded in (GEGLU.packed_ln); pw2: the second projection."""
    _chk_f16(x2d, "ff_fused.x")
    M, Cn = x2d.shape
    assert pw1.K == Cn and pw2.N == Cn and pw2.K * 2 == pw1.N and pw1.bias is not None
    out = torch.empty((M, Cn), dtype=F16, device=x2d.device)
    if residual is not None:
        _chk_f16(residual, "ff_fused.residual")
        assert residual.shape == out.shape
    _pf_note(pw1.wt, pw2.wt)
    _launch("af_ff_fused", _p(x2d), _p(pw1.wt), _p(pw1.bias), _p(pw1.ln_cs), float(pw1.ln_eps), pw1.kpad, _p(pw2.wt), _p(pw2.bias), pw2.kpad,
            _p(residual), _p(out), M, Cn, pw2.K, _p(_zero_page(x2d.device)))
    return out


def ff_chain(x2d: torch.Tensor, pw1: PackedWeight, pw2: PackedWeight, residual: torch.Tensor, pw_p: PackedWeight, x_in: torch.Tensor, *, rows_per_batch: int,
             gn_cpg: int = 0) -> torch.Tensor:
    """af_ff_chain: `ff_fused` with the SpatialTransformer's proj_out + residual behind it, one launch -- out = x_in + b_p + W_p (residual + b2 + W2 (v * gelu(g))).
    gn_cpg > 0: `out` feeds a GroupNorm with groups of gn_cpg channels; where the shape allows, the launch leaves the partial statistics with it (GnPartials)."""
    _chk_f16(x2d, "ff_chain.x")
    _chk_f16(residual, "ff_chain.residual")
    _chk_f16(x_in, "ff_chain.x_in")
    M, Cn = x2d.shape
    assert pw1.K == Cn and pw2.N == Cn and pw2.K * 2 == pw1.N and pw1.bias is not None and pw_p.N == Cn and pw_p.K == Cn and pw_p.ln_cs is None
    assert residual.shape == x2d.shape and x_in.shape == x2d.shape and M % rows_per_batch == 0
    out = torch.empty((M, Cn), dtype=F16, device=x2d.device)
    gn, gnp = None, None
    if gn_cpg and GN_FROM_PRODUCER and gn_cpg % 2 == 0 and Cn % gn_cpg == 0 and Cn // gn_cpg <= 32 and rows_per_batch % 128 == 0 and rows_per_batch // 128 <= 128:
        gn = GnPartials.alloc(x2d.device, M // rows_per_batch, rows_per_batch, Cn, gn_cpg)
        gnp = gn.ws.data_ptr()
    _pf_note(pw1.wt, pw2.wt, pw_p.wt)
    _launch("af_ff_chain", _p(x2d), _p(pw1.wt), _p(pw1.bias), _p(pw1.ln_cs), float(pw1.ln_eps), pw1.kpad, _p(pw2.wt), _p(pw2.bias), pw2.kpad, _p(residual),
            _p(pw_p.wt), _p(pw_p.bias), pw_p.kpad, _p(x_in), _p(out), gnp, int(gn_cpg if gn is not None else 0), int(rows_per_batch), M, Cn, pw2.K,
            _p(_zero_page(x2d.device)))
    if gn is not None:
        gn.attach(out)
    return out


# ----------------------------------------------------------------------------- norms
_gn_ws = {}


def xattn_fused(x2d: torch.Tensor, pw_q: PackedWeight, k: torch.Tensor, vt: torch.Tensor, pw_o: PackedWeight, *, B: int, N: int, L: int, heads: int,
                scale: float, ldk: int, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The whole cross-attention block of a C = 320 transformer layer in one launch (af_xattn_fused): q projection (pw_q: normally with
    the LayerNorm folded in, ops.pack_matrix_ln), 77-key attention over k [B*L, >= C] (row stride ldk) / vt [B, C, ld], output projection
    pw_o with its bias, residual."""
    _chk_f16(x2d, "xattn_fused.x")
    M, Cn = x2d.shape
    assert M == B * N and pw_q.N == Cn and pw_o.N == Cn and pw_o.K == Cn and vt.stride(2) == 1 and k.stride(1) == 1
    out = torch.empty_like(x2d)
    if residual is not None:
        _chk_f16(residual, "xattn_fused.residual")
        assert residual.shape == x2d.shape
    _pf_note(pw_q.wt, pw_o.wt)
    _launch("af_xattn_fused", _p(x2d), _p(pw_q.wt), _p(pw_q.bias), _p(pw_q.ln_cs), float(pw_q.ln_eps), pw_q.kpad, _p(k), int(ldk), _p(vt), int(vt.stride(0)),
            int(vt.stride(1)), _p(pw_o.wt), _p(pw_o.bias), pw_o.kpad, _p(residual), _p(out), B, N, L, Cn, heads, float(scale),
            _zero_page(x2d.device).data_ptr())
    return out


def xattn_chain(ao: torch.Tensor, pw_o1: PackedWeight, x0: torch.Tensor, pw_q: PackedWeight, k: torch.Tensor, vt: torch.Tensor, pw_o: PackedWeight, *,
                B: int, N: int, L: int, heads: int, scale: float, ldk: int) -> torch.Tensor:
    """af_xattn_chain: the self-attention's output projection + residual (ao, pw_o1, x0) in front of the C = 320 cross-attention block, one launch.
    Returns the block's output; the intermediate x1 = ao W1^T + b1 + x0 lives in a scratch tensor of this call."""
    _chk_f16(ao, "xattn_chain.ao")
    _chk_f16(x0, "xattn_chain.x0")
    M, Cn = ao.shape
    assert M == B * N and x0.shape == ao.shape and pw_o1.N == Cn and pw_o1.K == Cn and pw_q.N == Cn and pw_o.N == Cn and pw_o.K == Cn
    assert vt.stride(2) == 1 and k.stride(1) == 1 and pw_o1.ln_cs is None
    x1 = torch.empty_like(ao)
    out = torch.empty_like(ao)
    _pf_note(pw_o1.wt, pw_q.wt, pw_o.wt)
    _launch("af_xattn_chain", _p(ao), _p(pw_o1.wt), _p(pw_o1.bias), pw_o1.kpad, _p(x0), _p(x1), _p(pw_q.wt), _p(pw_q.bias), _p(pw_q.ln_cs), float(pw_q.ln_eps),
            pw_q.kpad, _p(k), int(ldk), _p(vt), int(vt.stride(0)), int(vt.stride(1)), _p(pw_o.wt), _p(pw_o.bias), pw_o.kpad, _p(out), B, N, L, Cn,
            heads, float(scale), _zero_page(ao.device).data_ptr())
    return out


def _grow_scratch(cache: dict, device, need: int, dtype, floor: int = 0) -> torch.Tensor:
    """Per-device scratch that grows on demand.  A hipGraph bakes in the address of whatever buffer a captured launch was given, and
    growing the cached buffer frees the old one -- so while the current stream is CAPTURING the scratch comes from the capturing graph's
    own pool instead (it lives exactly as long as that graph), and the growable buffer only ever serves eager launches."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((need,), dtype=dtype, device=device)
    sc = cache.get(device)
    if sc is None or sc.numel() < need:
        sc = torch.empty((max(need, floor),), dtype=dtype, device=device)
        cache[device] = sc
    return sc


def _gn_workspace(device, B: int) -> torch.Tensor:
    return _grow_scratch(_gn_ws, device, _lib.lib().af_groupnorm_ws_floats(max(B, 16)), torch.float32)


def _groupnorm(x, gamma, beta, eps, silu, x2, groups, want_stats: bool):
    """groupnorm / groupnorm_train: one launch, chosen by what x's producer left -- its partial statistics (GnPartials), or nothing (a statistics
    pass).  Returns (y, stats); stats is None unless want_stats."""
    _chk_f16(x, "groupnorm.x")
    B, c1 = x.shape[0], x.shape[-1]
    hw = x.numel() // (B * c1)
    c2 = 0
    if x2 is not None:
        _chk_f16(x2, "groupnorm.x2")
        c2 = x2.shape[-1]
    y = torch.empty(tuple(x.shape[:-1]) + (c1 + c2,), dtype=F16, device=x.device)
    stats = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device) if want_stats else None
    gn = partials_of(x) if x2 is None else None
    if gn is not None and gn.B == B and gn.hw == hw and gn.C == c1 and gn.cpg * groups == c1 and x.is_contiguous():
        # the launch that produced x left its partial statistics: normalise in one pass, no statistics pass (af_groupnorm_apply)
        _launch("af_groupnorm_apply", _p(x), c1, _p(gamma), _p(beta), _p(y), _p(stats), B, hw, groups, float(eps), int(silu), _p(gn.ws), gn.nblk)
        return y, stats
    ws = _gn_workspace(x.device, B)
    if stats is None:
        _launch("af_groupnorm", _p(x), _p(x2), c1, c2, _p(gamma), _p(beta), _p(y), B, hw, groups, float(eps), int(silu), _p(ws))
    else:
        _launch("af_groupnorm_stats", _p(x), _p(x2), c1, c2, _p(gamma), _p(beta), _p(y), _p(stats), B, hw, groups, float(eps), int(silu), _p(ws))
    return y, stats


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, silu: bool, *,
              x2: Optional[torch.Tensor] = None, groups: int = 32) -> torch.Tensor:
    """x [B, ..., C1] (+ x2 [B, ..., C2]) -> [B, ..., C1+C2] fp16; gamma/beta fp32 [C1+C2]."""
    return _groupnorm(x, gamma, beta, eps, silu, x2, groups, False)[0]


def groupnorm_train(x, gamma, beta, eps, silu, *, x2=None, groups=32):
    """groupnorm() that also returns the (mean, rstd) statistics fp32 [B, groups, 2] for the backward."""
    return _groupnorm(x, gamma, beta, eps, silu, x2, groups, True)


def gn_proj_fused(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, pw: PackedWeight, groups: int = 32) -> Optional[torch.Tensor]:
    """GroupNorm(x) followed by a 1x1 convolution / Linear at C = 320 in ONE launch (af_gn_proj_fused): x [B, ..., 320] carrying the partial
    statistics its producer left (x._gn_partials) -> [B * HW, N = 320] token-major.  Returns None when x does not qualify (no partials, another
    width, ragged image size): the caller then runs the two launches."""
    gn = partials_of(x)
    B, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (B * c)
    if (gn is None or c != 320 or groups != 32 or pw.N != 320 or pw.K != 320 or pw.ln_cs is not None or hw % 128 != 0 or gn.B != B or gn.hw != hw or gn.C != c
            or gn.cpg * groups != c or not x.is_contiguous()):
        return None
    _chk_f16(x, "gn_proj_fused.x")
    out = torch.empty((B * hw, pw.N), dtype=F16, device=x.device)
    _pf_note(pw.wt)
    _launch("af_gn_proj_fused", _p(x), _p(gn.ws), gn.nblk, _p(gamma), _p(beta), float(eps), _p(pw.wt), _p(pw.bias), pw.kpad, _p(out), B, hw, c, groups,
            _zero_page(x.device).data_ptr())
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    _chk_f16(x, "layernorm.x")
    Cn = x.shape[-1]
    y = torch.empty_like(x)
    _launch("af_layernorm", _p(x), _p(gamma), _p(beta), _p(y), x.numel() // Cn, Cn, float(eps))
    return y


# ----------------------------------------------------------------------------- attention
def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, *, B: int, Nq: int, L: int, heads: int, d: int,
              ldq: int, ldk: int, keybias: Optional[torch.Tensor] = None, scale: Optional[float] = None,
              want_lse: bool = False, causal_m: int = 0):
    """q [B*Nq, ldq-wide rows], k [B*L, ldk-wide rows], vt [B, heads*d, ldv] -> o [B*Nq, heads*d]
    (and, with want_lse, the base-2 log-sum-exp fp32 [B, heads, roundup(Nq,32)] for the backward)."""
    Cn = heads * d
    o = torch.empty((B * Nq, Cn), dtype=F16, device=q.device)
    scale = d ** -0.5 if scale is None else scale
    ldb = 0 if keybias is None else keybias.stride(0)
    lse = torch.empty((B, heads, round_up(Nq, 32)), dtype=torch.float32, device=q.device) if want_lse else None
    _launch("af_attention_strided", _p(q), _p(k), _p(vt), _p(o), _p(lse), 0 if lse is None else lse.stride(1), _p(keybias),
            int(causal_m), B, Nq, L, heads, d, ldq, ldk, Cn, vt.stride(1), ldb, vt.stride(0), float(scale))
    return (o, lse) if want_lse else o


_attn_scratch = {}


def attention_bwd(q, k, v, o, dout, lse, *, B: int, Nq: int, L: int, heads: int, d: int, ldq: int, ldk: int, ldv: int,
                  dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor, lddq: int, lddk: int, lddv: int,
                  keybias: Optional[torch.Tensor] = None, scale: Optional[float] = None, causal_m: int = 0):
    """Input gradients of `attention`.  q/k/v: row-major token tensors (views allowed: row strides ldq/ldk/ldv);
    o, dout [B*Nq, heads*d] contiguous; dq/dk/dv are written in place with row strides lddq/lddk/lddv."""
    Cn = heads * d
    scale = d ** -0.5 if scale is None else scale
    need = _lib.lib().af_attention_bwd_scratch_bytes(B, Nq, L, heads, d)
    sc = _grow_scratch(_attn_scratch, q.device, need, torch.uint8, floor=64 << 20)
    ldb = 0 if keybias is None else keybias.stride(0)
    _launch("af_attention_bwd", _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), lse.stride(1), _p(keybias), int(causal_m), _p(dq), _p(dk),
            _p(dv), _p(sc), sc.numel(), B, Nq, L, heads, d, ldq, ldk, ldv, Cn, Cn, lddq, lddk, lddv, ldb, float(scale))


def attention_scores(q: torch.Tensor, k: torch.Tensor, *, B: int, Nq: int, L: int, heads: int, d: int,
                     scale: Optional[float] = None):
    """Explicit (score, prob) fp32 [B, heads, Nq, L] for the capture path; q [B*Nq, C], k [B*L, C] contiguous."""
    _chk_f16(q, "attention_scores.q")
    _chk_f16(k, "attention_scores.k")
    score = torch.empty((B, heads, Nq, L), dtype=torch.float32, device=q.device)
    prob = torch.empty_like(score)
    scale = d ** -0.5 if scale is None else scale
    _launch("af_attention_scores", _p(q), _p(k), _p(score), _p(prob), B, Nq, L, heads, d, float(scale))
    return score, prob


# ---- explicit cross-attention (capture / score-rewrite path; csrc/af_xattn_explicit.hip) -- q [B*Nq, >=C], k / v [B*L, >=C] fp16 rows
def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D operand expected"
    return t.stride(0)


def _chk_f16_rows(t: torch.Tensor, name: str):
    """fp16 device matrix whose rows are contiguous (a column slice of a wider buffer is fine: the kernels take leading dimensions)."""
    if t.dtype != F16 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 != 0 or t.data_ptr() % 16 != 0:
        raise RuntimeError(f"{name}: expected an fp16 device matrix with contiguous, 16-byte aligned rows, got {t.dtype} {t.device} strides {t.stride()}")


def xattn_scores(q, k, *, B, Nq, L, heads, d, scale):
    """score fp32 [B, heads, Nq, L] = scale * q k^T."""
    _chk_f16_rows(q, "xattn_scores.q")
    _chk_f16_rows(k, "xattn_scores.k")
    score = torch.empty((B, heads, Nq, L), dtype=torch.float32, device=q.device)
    _launch("af_xattn_scores", _p(q), _ld(q), _p(k), _ld(k), _p(score), B, Nq, L, heads, d, float(scale))
    return score


def xattn_softmax_pv(score, v, *, B, Nq, L, heads, d):
    """(prob fp32 [B, heads, Nq, L], o fp16 [B*Nq, heads*d]) from (rewritten) scores."""
    _chk_f16_rows(v, "xattn_softmax_pv.v")
    assert score.dtype == torch.float32 and score.is_contiguous() and tuple(score.shape) == (B, heads, Nq, L)
    prob = torch.empty_like(score)
    o = torch.empty((B * Nq, heads * d), dtype=F16, device=v.device)
    _launch("af_xattn_softmax_pv", _p(score), _p(v), _ld(v), _p(prob), _p(o), heads * d, B, Nq, L, heads, d)
    return prob, o


def xattn_softmax_pv_bwd(prob, v, dout, dprob_ext, *, B, Nq, L, heads, d):
    """dscore fp32 [B, heads, Nq, L]; dprob_ext: gradient arriving on the captured probabilities (fp32, same shape) or None."""
    _chk_f16_rows(dout, "xattn_softmax_pv_bwd.dout")
    dscore = torch.empty_like(prob)
    if dprob_ext is not None:
        dprob_ext = dprob_ext.to(torch.float32).contiguous()
    _launch("af_xattn_softmax_pv_bwd", _p(prob), _p(v), _ld(v), _p(dout), _ld(dout), _p(dprob_ext), _p(dscore), B, Nq, L, heads, d)
    return dscore


def xattn_rowmix(w, x, alpha, *, B, Nq, L, heads, d):
    """out fp16 [B*Nq, heads*d] = alpha * w x  (w fp32 [B, heads, Nq, L], x fp16 [B*L, >=C])."""
    out = torch.empty((B * Nq, heads * d), dtype=F16, device=x.device)
    _launch("af_xattn_rowmix", _p(w), _p(x), _ld(x), _p(out), heads * d, float(alpha), B, Nq, L, heads, d)
    return out


def xattn_colmix(w, x, alpha, *, B, Nq, L, heads, d):
    """out fp16 [B*L, heads*d] = alpha * w^T x  (x fp16 [B*Nq, >=C]): the reductions over the queries (dk, dv)."""
    out = torch.empty((B * L, heads * d), dtype=F16, device=x.device)
    nb = int(_lib.lib().af_xattn_colmix_ws_bytes(B, L, heads, d))
    ws = torch.empty((nb // 4,), dtype=torch.float32, device=x.device)
    _launch("af_xattn_colmix", _p(w), _p(x), _ld(x), _p(out), heads * d, float(alpha), _p(ws), nb, B, Nq, L, heads, d)
    return out


def make_keybias(mask: torch.Tensor, L: int) -> torch.Tensor:
    """mask [B, L] (nonzero = keep) -> fp32 [B, roundup(L, 64)] additive bias: 0 / -FLT_MAX
    (== masked_fill_(~mask, -finfo.max), attention.py:188-194)."""
    B = mask.shape[0]
    kb = torch.zeros((B, round_up(L, 64)), dtype=torch.float32, device=mask.device)
    kb[:, :L] = torch.where(mask.bool(), 0.0, NEG_MAX)
    return kb


# ----------------------------------------------------------------------------- element-wise
def timestep_embedding(timesteps: torch.Tensor, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    t = timesteps.to(dtype=torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), dtype=F16, device=t.device)
    _launch("af_timestep_embedding", _p(t), _p(out), t.shape[0], dim, float(max_period))
    return out


def nchw_f32_to_nhwc_f16(x: torch.Tensor, cpad: int = 0) -> torch.Tensor:
    x = x.to(torch.float32).contiguous()
    B, Cn, H, W = x.shape
    cpad = max(cpad, Cn)
    y = torch.empty((B, H, W, cpad), dtype=F16, device=x.device)
    _launch("af_nchw_f32_to_nhwc_f16", _p(x), _p(y), B, Cn, H * W, cpad)
    return y


def nhwc_f16_to_nchw_f32(x: torch.Tensor, Cn: Optional[int] = None) -> torch.Tensor:
    _chk_f16(x, "nhwc_f16_to_nchw_f32.x")
    B, H, W, cs = x.shape
    Cn = Cn or cs
    y = torch.empty((B, Cn, H, W), dtype=torch.float32, device=x.device)
    _launch("af_nhwc_f16_to_nchw_f32", _p(x), _p(y), B, Cn, H * W, cs)
    return y


def silu(x: torch.Tensor) -> torch.Tensor:
    _chk_f16(x, "silu.x")
    y = torch.empty_like(x)
    _launch("af_silu_f16", _p(x), _p(y), x.numel())
    return y


def gelu(x: torch.Tensor) -> torch.Tensor:
    """erf-GELU, fp16 (af_gelu_f16): the MLP activation of DINO's ViT."""
    _chk_f16(x, "gelu.x")
    y = torch.empty_like(x)
    _launch("af_gelu_f16", _p(x), _p(y), x.numel())
    return y


VIT_FILTERS = {"bilinear": 0, "bicubic": 1}


def vit_resize_geometry(H: int, W: int, keep_aspect: bool, S: int, C: int):
    """(Hr, Wr, top, left) of af_vit_patch_rows (the rule is in include/adaface_hip.h): torchvision's Resize(S) + CenterCrop(C), or the square
    resize to C x C.  Python's round is half to even, as the library's."""
    if not keep_aspect:
        return C, C, 0, 0
    Hr, Wr = (S, S * W // H) if H <= W else (S * H // W, S)
    return Hr, Wr, int(round((Hr - C) / 2.0)), int(round((Wr - C) / 2.0))


_vit_affine_cache = {}


def _vit_affine(mean, std):
    """The host arrays af_vit_patch_rows takes: 1 / (255 std), -mean / std (built once per normalisation)."""
    key = (mean, std)
    if key not in _vit_affine_cache:
        f3 = _lib.C.c_float * 3
        _vit_affine_cache[key] = (f3(*[1.0 / (255.0 * float(s)) for s in std]), f3(*[-float(m) / float(s) for m, s in zip(mean, std)]))
    return _vit_affine_cache[key]


def vit_patch_rows(images_u8: torch.Tensor, *, keep_aspect: bool, S: int, C: int, p: int, filter: str, mean, std, kpad: int = 0) -> torch.Tensor:
    """uint8 [B, H, W, 3] device images -> fp16 [B * (C / p)^2, kpad] rows of the patch-embedding GEMM: antialiased resize, centre crop,
    (v / 255 - mean) / std and the unfold in one launch (af_vit_patch_rows).  kpad defaults to 3 p^2 rounded up to 64."""
    if images_u8.dtype != torch.uint8 or not images_u8.is_cuda or images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_contiguous():
        raise RuntimeError(f"vit_patch_rows: expected contiguous uint8 device images [B, H, W, 3], got {images_u8.dtype} {tuple(images_u8.shape)} {images_u8.device}")
    if filter not in VIT_FILTERS:
        raise ValueError(f"vit_patch_rows: filter must be one of {sorted(VIT_FILTERS)}, got {filter!r}")
    B, H, W, _ = images_u8.shape
    kpad = kpad or round_up(3 * p * p, 64)
    rows = torch.empty((B * (C // max(p, 1)) ** 2, kpad), dtype=F16, device=images_u8.device)
    scale, shift = _vit_affine(tuple(mean), tuple(std))
    _launch("af_vit_patch_rows", _p(images_u8), _p(rows), B, H, W, int(bool(keep_aspect)), int(S), int(C), int(p), VIT_FILTERS[filter], scale, shift, kpad)
    return rows


@dataclass
class InpaintBlend:
    """The mask blend an inpaint step applies to its new latent x_new [B, 4, h, w] (INTEGRATION.md "Inpainting" rule 4):
    x_next = mask ? x_new : known, known = fma(sb, noise, sa z), or z itself when noise is None (the last step).  z fp32
    [B_img, 4, h, w] and mask fp32 {0, 1} [B_mask, 1, h, w] broadcast by b % B_img / b % B_mask; noise fp32 [B, 4, h, w]."""
    z: torch.Tensor
    noise: Optional[torch.Tensor]
    mask: torch.Tensor
    sa: float = 0.0
    sb: float = 0.0

    def args(self, x: torch.Tensor):
        """The blend's C-ABI arguments for a step on x [B, 4, h, w], after checking shapes, dtypes and devices."""
        if x.dim() != 4 or x.shape[1] != 4:
            raise RuntimeError(f"inpaint step: x must be [B, 4, h, w], got {tuple(x.shape)}")
        B, _, h, w = x.shape
        want = [("z", self.z, 4, None), ("mask", self.mask, 1, None)]
        if self.noise is not None:
            want.append(("noise", self.noise, 4, B))
        for name, t, c, b in want:
            if t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.dim() != 4 or \
                    tuple(t.shape[1:]) != (c, h, w) or (b is not None and t.shape[0] != b) or t.shape[0] < 1:
                raise RuntimeError(f"inpaint blend.{name}: expected contiguous fp32 [{b or 'N'}, {c}, {h}, {w}] on {x.device}, got "
                                   f"{t.dtype} {tuple(t.shape)} on {t.device}")
        return [_p(self.z), None if self.noise is None else _p(self.noise), _p(self.mask), self.z.shape[0], self.mask.shape[0],
                h * w, float(self.sa), float(self.sb)]


def _cfg_step(kind: str, eps2: torch.Tensor, x: torch.Tensor, inputs, scalars, has_uncond: bool, blend: Optional[InpaintBlend]):
    """The body of the three fused sampler steps: af_cfg_<kind>_step, or af_cfg_<kind>_inpaint_step with ``blend``, on eps2 fp32
    [2n or n] and x fp32 [n].  ``inputs`` are the step's extra fp32 [n] streams in C-ABI order (None: passed as NULL),
    ``scalars`` its coefficients after has_uncond.  Returns (new latent, x0-like output)."""
    assert eps2.dtype == torch.float32 and x.dtype == torch.float32 and eps2.is_contiguous() and x.is_contiguous()
    n = x.numel()
    assert eps2.numel() == (2 * n if has_uncond else n)
    for t in inputs:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
    out, aux = torch.empty_like(x), torch.empty_like(x)
    name = f"af_cfg_{kind}_step" if blend is None else f"af_cfg_{kind}_inpaint_step"
    args = [_p(eps2), _p(x), *(None if t is None else _p(t) for t in inputs), _p(out), _p(aux), n, int(has_uncond),
            *(float(v) for v in scalars), *(() if blend is None else blend.args(x))]
    _launch(name, *args)
    return out, aux


def cfg_ddim_step(eps2: torch.Tensor, x: torch.Tensor, guidance: float, a_t: float, a_prev: float, has_uncond: bool = True,
                  blend: Optional[InpaintBlend] = None):
    """eps2 fp32 [2n or n] = [e_cond ; e_uncond], x fp32 [n] -> (x_prev, pred_x0), ddim.py:253-302 (sigma = 0).  With ``blend``
    (x [B, 4, h, w]), x_prev is blended (af_cfg_ddim_inpaint_step); pred_x0 is not."""
    return _cfg_step("ddim", eps2, x, [], [guidance, a_t, a_prev], has_uncond, blend)


def cfg_dpmpp_step(eps2: torch.Tensor, x: torch.Tensor, x_base: torch.Tensor, x0_prev: Optional[torch.Tensor], guidance: float,
                   alpha_s: float, sigma_s: float, c_base: float, c0: float, c1: float, has_uncond: bool = True,
                   blend: Optional[InpaintBlend] = None):
    """eps2 fp32 [2n or n] = [e_cond ; e_uncond], x / x_base / x0_prev fp32 [n] -> (x_out, x0_out): one DPM-Solver++ step,
    x0 = (x - sigma_s e) / alpha_s, x_out = c_base x_base + c0 x0 + c1 x0_prev (x0_prev unused, may be None, when c1 == 0).
    With ``blend`` (x [B, 4, h, w]), x_out is blended (af_cfg_dpmpp_inpaint_step); x0_out is not."""
    assert x_base is not None and (c1 == 0.0 or x0_prev is not None)
    return _cfg_step("dpmpp", eps2, x, [x_base, x0_prev if c1 != 0.0 else None], [guidance, alpha_s, sigma_s, c_base, c0, c1],
                     has_uncond, blend)


def cfg_lcm_step(eps2: torch.Tensor, x: torch.Tensor, noise: Optional[torch.Tensor], guidance: float, sqrt_a: float, sqrt_1ma: float,
                 c_out: float, c_skip: float, sqrt_a_next: float = 0.0, sqrt_1ma_next: float = 0.0, has_uncond: bool = True,
                 blend: Optional[InpaintBlend] = None):
    """eps2 fp32 [2n or n] = [e_cond ; e_uncond], x / noise fp32 [n] -> (x_next, denoised): one LCM step,
    x0 = (x - sqrt_1ma e) / sqrt_a, denoised = c_out x0 + c_skip x, x_next = sqrt_a_next denoised + sqrt_1ma_next noise
    (noise None: the last step, x_next = denoised).  With ``blend`` (x [B, 4, h, w]), x_next is blended
    (af_cfg_lcm_inpaint_step); denoised is not."""
    return _cfg_step("lcm", eps2, x, [noise], [guidance, sqrt_a, sqrt_1ma, c_out, c_skip, sqrt_a_next, sqrt_1ma_next], has_uncond,
                     blend)


def q_sample(x0: torch.Tensor, noise: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """x_t = sa[b] x0 + sb[b] noise (ddpm.py:395-398); fp32."""
    x0, noise = x0.to(torch.float32).contiguous(), noise.to(torch.float32).contiguous()
    sa, sb = sa.to(torch.float32).contiguous(), sb.to(torch.float32).contiguous()
    B = x0.shape[0]
    xt = torch.empty_like(x0)
    _launch("af_q_sample", _p(x0), _p(noise), _p(sa), _p(sb), _p(xt), B, x0.numel() // B)
    return xt


def image_u8_to_nhwc_f16(img_u8: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [B, H, W, 3] -> fp16 [B, H, W, 8] = (v / 255) * 2 - 1 in channels 0-2, zeros in 3-7 (the VAE encoder's input)."""
    if img_u8.dtype != torch.uint8 or not img_u8.is_cuda or not img_u8.is_contiguous():
        raise RuntimeError(f"image_u8_to_nhwc_f16: expected a contiguous uint8 device tensor, got {img_u8.dtype} {img_u8.device}")
    if img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise RuntimeError(f"image_u8_to_nhwc_f16: expected [B, H, W, 3], got {tuple(img_u8.shape)}")
    B, H, W, _ = img_u8.shape
    out = torch.empty((B, H, W, 8), dtype=F16, device=img_u8.device)
    _launch("af_image_u8_to_nhwc_f16", _p(img_u8), _p(out), B, H, W)
    return out


def vae_latents_q_sample(h: torch.Tensor, qw: torch.Tensor, qb: torch.Tensor, n_post: torch.Tensor, n_fwd: torch.Tensor, scale: float,
                         sa: float, sb: float, out_count: int, with_z: bool = False):
    """Encoder output h fp16 [B_img, hh, ww, 8] -> x_t fp32 [out_count, 4, hh, ww]: quant_conv (qw fp32 [8, 8] out x in, qb fp32 [8]),
    posterior sample z = scale (mean + exp(0.5 clamp(logvar, -30, 20)) n_post), then sa z + sb n_fwd.  Output j uses image
    j % B_img; n_post fp32 [B_img, 4, hh, ww], n_fwd fp32 [out_count, 4, hh, ww].  ``with_z`` returns (x_t, z), z fp32
    [B_img, 4, hh, ww] (af_vae_latents_z_q_sample, the same launch)."""
    _chk_f16(h, "vae_latents_q_sample.h")
    if h.dim() != 4 or h.shape[3] != 8:
        raise RuntimeError(f"vae_latents_q_sample: h must be [B, hh, ww, 8], got {tuple(h.shape)}")
    B_img, hh, ww, _ = h.shape
    want = {"qw": (qw, (8, 8)), "qb": (qb, (8,)), "n_post": (n_post, (B_img, 4, hh, ww)), "n_fwd": (n_fwd, (out_count, 4, hh, ww))}
    for name, (t, shape) in want.items():
        if t.dtype != torch.float32 or t.device != h.device or not t.is_contiguous() or tuple(t.shape) != shape:
            raise RuntimeError(f"vae_latents_q_sample.{name}: expected contiguous fp32 {shape} on {h.device}, got {t.dtype} "
                               f"{tuple(t.shape)} on {t.device}")
    if out_count <= 0 or out_count % B_img != 0:
        raise RuntimeError(f"vae_latents_q_sample: out_count {out_count} is not a positive multiple of the image count {B_img}")
    x_t = torch.empty((out_count, 4, hh, ww), dtype=torch.float32, device=h.device)
    args = [_p(h), _p(qw), _p(qb), _p(n_post), _p(n_fwd), float(scale), float(sa), float(sb), _p(x_t)]
    if not with_z:
        _launch("af_vae_latents_q_sample", *args, B_img, out_count, hh, ww)
        return x_t
    z = torch.empty((B_img, 4, hh, ww), dtype=torch.float32, device=h.device)
    _launch("af_vae_latents_z_q_sample", *args, _p(z), B_img, out_count, hh, ww)
    return x_t, z


RESIZE_MODES = {"bilinear": 0, "bicubic": 1}


def latent_resize_q_sample(x: torch.Tensor, size_hw, mode: str = "bilinear", noise: Optional[torch.Tensor] = None, sa: float = 1.0,
                           sb: float = 0.0) -> torch.Tensor:
    """x fp32 [B, C, h, w] -> fp32 [B, C, H, W], size_hw = (H, W): F.interpolate(x, size_hw, mode, align_corners=False) in fp32
    ("bilinear" or "bicubic", not antialiased), then sa r + sb noise with ``noise`` fp32 [B, C, H, W]; the resampled tensor itself
    when ``noise`` is None (sa, sb unused).  One launch (af_latent_resize_q_sample)."""
    if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.dim() != 4:
        raise RuntimeError(f"latent_resize_q_sample.x: expected a contiguous fp32 device tensor [B, C, h, w], got {x.dtype} "
                           f"{tuple(x.shape)} on {x.device}")
    if mode not in RESIZE_MODES:
        raise RuntimeError(f"latent_resize_q_sample: mode must be one of {sorted(RESIZE_MODES)}, got {mode!r}")
    B, Cn, h, w = x.shape
    H, W = (int(s) for s in size_hw)
    if H < 1 or W < 1:
        raise RuntimeError(f"latent_resize_q_sample: size_hw must be positive, got {(H, W)}")
    if noise is not None and (noise.dtype != torch.float32 or noise.device != x.device or not noise.is_contiguous()
                              or tuple(noise.shape) != (B, Cn, H, W)):
        raise RuntimeError(f"latent_resize_q_sample.noise: expected contiguous fp32 {(B, Cn, H, W)} on {x.device}, got {noise.dtype} "
                           f"{tuple(noise.shape)} on {noise.device}")
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=x.device)
    _launch("af_latent_resize_q_sample", _p(x), _p(noise), _p(out), B * Cn, h, w, H, W, RESIZE_MODES[mode], float(sa), float(sb))
    return out


# ----------------------------------------------------------------------------- backward ops
def groupnorm_bwd(x, gamma, beta, stats, dy, silu, *, x2=None, add=None, groups=32):
    """Input gradient of groupnorm(+SiLU): returns dx (or (dx1, dx2) when x2 is given)."""
    B, c1 = x.shape[0], x.shape[-1]
    hw = x.numel() // (B * c1)
    c2 = 0 if x2 is None else x2.shape[-1]
    _chk_f16(dy, "groupnorm_bwd.dy")
    dx1 = torch.empty_like(x)
    dx2 = None if x2 is None else torch.empty_like(x2)
    _launch("af_groupnorm_bwd", _p(x), _p(x2), c1, c2, _p(gamma), _p(beta), _p(stats), _p(dy), _p(add), _p(dx1), _p(dx2), B,
            hw, groups, int(silu), _p(_gn_workspace(x.device, B)))
    return dx1 if x2 is None else (dx1, dx2)


def layernorm_bwd(x, gamma, dy, eps=1e-5, add=None):
    dx = torch.empty_like(x)
    Cn = x.shape[-1]
    _launch("af_layernorm_bwd", _p(x), _p(gamma), _p(dy), _p(add), _p(dx), x.numel() // Cn, Cn, float(eps))
    return dx


def layernorm_param_grads(x, dy, eps=1e-5):
    """(dgamma, dbeta) fp32 [C] of a LayerNorm over the last dim from its input and output gradient (rows <= 2048, C <= 1536)."""
    Cn = x.shape[-1]
    rows = x.numel() // Cn
    out = torch.empty((2 * Cn + 2 * rows,), dtype=torch.float32, device=x.device)        # dgamma | dbeta | row statistics scratch
    dg, db, st = out[:Cn], out[Cn:2 * Cn], out[2 * Cn:]
    _launch("af_layernorm_param_grads", _p(x), _p(dy), _p(dg), _p(db), _p(st), rows, Cn, float(eps))
    return dg, db


def geglu_fwd(hp):
    M, two_i = hp.shape
    out = torch.empty((M, two_i // 2), dtype=F16, device=hp.device)
    _launch("af_geglu_fwd", _p(hp), _p(out), M, two_i // 2)
    return out


def geglu_bwd(hp, dout):
    dhp = torch.empty_like(hp)
    _launch("af_geglu_bwd", _p(hp), _p(dout), _p(dhp), hp.shape[0], hp.shape[1] // 2)
    return dhp


def sumpool2x2(x):
    B, H2, W2, Cn = x.shape
    y = torch.empty((B, H2 // 2, W2 // 2, Cn), dtype=F16, device=x.device)
    _launch("af_sumpool2x2", _p(x), _p(y), B, H2 // 2, W2 // 2, Cn)
    return y


def add(a, b):
    _chk_f16(a, "add.a")
    _chk_f16(b, "add.b")
    assert a.shape == b.shape
    out = torch.empty_like(a)
    _launch("af_add_f16", _p(a), _p(b), _p(out), a.numel())
    return out


def axpy(a, b, alpha):
    """a + alpha * b (fp16)."""
    _chk_f16(a, "axpy.a")
    _chk_f16(b, "axpy.b")
    assert a.shape == b.shape
    out = torch.empty_like(a)
    _launch("af_axpy_f16", _p(a), _p(b), float(alpha), _p(out), a.numel())
    return out


def transpose_tokens(x, B, N, Cn, ldx):
    """x: rows of a [B*N, ldx] token tensor (Cn columns from x's first column) -> [B, Cn, roundup(N, 8)]."""
    ldy = round_up(N, 8)
    y = torch.empty((B, Cn, ldy), dtype=F16, device=x.device)
    _launch("af_transpose_tokens", _p(x), _p(y), B, N, Cn, ldx, ldy)
    return y


def cadamw_step(p, g, m, v, seg_offsets, counts, *, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, step=1, correct_bias=True):
    """Fused cautious-AdamW step (c_adamw.py:65-123) on flat fp32 buffers; seg_offsets int64 [nseg+1] on the device."""
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous()
    _launch("af_cadamw_step", _p(p), _p(g), _p(m), _p(v), _p(seg_offsets), seg_offsets.numel() - 1, _p(counts), float(lr),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), int(correct_bias))


def colsum(a, b=None, out=None, accumulate=False):
    """fp32 [C] = sum over rows of a (* b): bias / LayerNorm-gamma gradients."""
    rows, Cn = a.shape
    if out is None:
        out = torch.empty((Cn,), dtype=torch.float32, device=a.device)
    if rows >= 2048:                                           # tall: spread the rows over workgroups (two deterministic passes)
        chunks = min(256, (rows + 255) // 256)
        partial = torch.empty((chunks, Cn), dtype=torch.float32, device=a.device)
        _launch("af_colsum_tall", _p(a), _p(b), _p(partial), _p(out), rows, Cn, chunks, int(accumulate))
        return out
    _launch("af_colsum", _p(a), _p(b), _p(out), rows, Cn, int(accumulate))
    return out


def quickgelu_fwd(x):
    y = torch.empty_like(x)
    _launch("af_quickgelu_fwd", _p(x), _p(y), x.numel())
    return y


def quickgelu_bwd(x, dy):
    dx = torch.empty_like(x)
    _launch("af_quickgelu_bwd", _p(x), _p(dy), _p(dx), x.numel())
    return dx


def clamp_f32_(a, lo, hi):
    _launch("af_clamp_f32", _p(a), float(lo), float(hi), a.numel())
    return a


def scale_f32_(a, s):
    _launch("af_scale_f32", _p(a), float(s), a.numel())
    return a


def softmax_rows(x):
    """Row softmax of an fp16 [rows, L] score matrix (fp32 inside)."""
    _chk_f16(x, "softmax_rows.x")
    rows, L = x.shape
    y = torch.empty_like(x)
    _launch("af_softmax_rows", _p(x), _p(y), rows, L)
    return y


VAE_ATTN_DIMS = (128, 512)          # head dims af_vae_attention is built for: the mid width of the reduced test VAE and of SD-1.5's
VAE_ATTN_MAX_TOKENS = 16384         # a 128 x 128 latent (1024 x 1024 image): the range the kernel is tested over


def vae_attention(q, k, v, *, B: int, N: int, C: int):
    """Fused single-head attention of the VAE's attention layer: q, k, v [B*N, C] fp16 token rows (column slices of wider buffers are fine), the
    C^-0.5 scale already in q -> softmax(q k^T) v [B*N, C].  Online softmax in one launch, no [N, N] matrix; any N % 8 == 0.  The kernel reads
    the values key-contiguous, so v is transposed first ([B, C, N], 2 N C bytes: noise beside the 4 N^2 C FLOP)."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _chk_f16_rows(t, f"vae_attention.{name}")
        if t.shape[0] != B * N or t.shape[1] != C:
            raise RuntimeError(f"vae_attention.{name}: expected [{B * N}, {C}], got {tuple(t.shape)}")
    vt = transpose_tokens(v, B, N, C, _ld(v))
    o = torch.empty((B * N, C), dtype=F16, device=q.device)
    _launch("af_vae_attention", _p(q), _p(k), _p(vt), _p(o), B, N, C, _ld(q), _ld(k), vt.stride(1), C)
    return o


TEMPORAL_ATTN_MAX_FRAMES = 32      # af_temporal_attention: 1 <= F <= 32, head dim % 8 == 0 in 8 .. 160


def temporal_attention(qkv, *, B: int, F: int, HW: int, heads: int, d: int, scale=None):
    """Self-attention along the frame axis (motion modules): qkv [B*F*HW, >= 3*heads*d] fp16 token rows, row (b*F + f)*HW + p holding
    q | k | v of frame f of pixel p -> [B*F*HW, heads*d], softmax over the F frames of each (b, p, head).  One launch, no workspace, no transpose."""
    _chk_f16_rows(qkv, "temporal_attention.qkv")
    Cn = heads * d
    if qkv.shape[0] != B * F * HW or qkv.shape[1] < 3 * Cn:
        raise RuntimeError(f"temporal_attention.qkv: expected [{B * F * HW}, >= {3 * Cn}], got {tuple(qkv.shape)}")
    o = torch.empty((B * F * HW, Cn), dtype=F16, device=qkv.device)
    _launch("af_temporal_attention", _p(qkv), _ld(qkv), _p(o), B, F, HW, heads, d, float(d ** -0.5 if scale is None else scale))
    return o


IP_ATTN_MAX_TOKENS = 64           # af_ip_attention_add: 1 <= T <= 64 image tokens, head dim % 8 == 0 in 8 .. 160


def ip_attention_add(o, q, k, v, *, B: int, N: int, heads: int, d: int, ip_scale: float, scale=None):
    """IP-Adapter's decoupled cross-attention, in place: o [B*N, >= heads*d] += ip_scale * softmax(scale q k^T) v over the T image tokens of
    each batch item, summed with o in fp32 and rounded once.  q [B*N, >= heads*d] token rows; k, v [B, T, heads*d] fp16 views with contiguous
    channels (any row / batch stride that is a multiple of 8: a column slice of a stacked projection, or ``expand``-ed shared tokens).
    One launch, no workspace.  Returns o."""
    _chk_f16_rows(o, "ip_attention_add.o")
    _chk_f16_rows(q, "ip_attention_add.q")
    Cn = heads * d
    for t, name in ((o, "o"), (q, "q")):
        if t.shape[0] != B * N or t.shape[1] < Cn:
            raise RuntimeError(f"ip_attention_add.{name}: expected [{B * N}, >= {Cn}], got {tuple(t.shape)}")
    for t, name in ((k, "k"), (v, "v")):
        if t.dtype != F16 or not t.is_cuda or t.dim() != 3 or t.stride(2) != 1 or t.shape[0] != B or t.shape[2] != Cn or t.shape[1] != k.shape[1]:
            raise RuntimeError(f"ip_attention_add.{name}: expected an fp16 device view [{B}, T, {Cn}] with contiguous channels, got {t.dtype} {t.device} "
                               f"{tuple(t.shape)} strides {t.stride()}")
    _launch("af_ip_attention_add", _p(o), _ld(o), _p(q), _ld(q), _p(k), k.stride(1), k.stride(0), _p(v), v.stride(1), v.stride(0),
            B, N, k.shape[1], heads, d, float(d ** -0.5 if scale is None else scale), float(ip_scale))
    return o


REGION_MAX = 8                    # af_region_attention: 1 <= R <= 8 context sets per batch item (the base prompt + up to 7 regions)
REGION_MAX_TOKENS = 80            # ... of 1 <= L <= 80 context tokens each


def region_attention(q, k, vt, w, *, B: int, R: int, N: int, L: int, heads: int, d: int, ldk: int, scale=None, out=None):
    """Regional prompts: o [B*N, heads*d] = sum_r w[b*R+r, i] * softmax(scale q k_r^T) v_r over the R context sets of each batch item, blended in
    fp32 and rounded once (af_region_attention, one launch, no workspace).  q [B*N, >= heads*d] token rows; context set (b, r) is batch item
    b*R+r of k (rows (b*R+r)*L + t, row stride ``ldk``) and vt ([B*R, heads*d, >= L], V transposed; a row slice of a taller tensor keeps its
    strides) -- the operands of ``attention`` with the sets as batch items, so a layer reads its slice of one stacked projection in place.  w fp32 [B*R, >= N] with contiguous rows.  A weight that is exactly 0 is a select: that query
    takes nothing from the set (NaN included), and a 128-query tile with no nonzero weight for a set does not read it.  ``out``: write there
    ([B*N, >= heads*d] rows) instead of a new tensor.  Returns o."""
    _chk_f16_rows(q, "region_attention.q")
    Cn = heads * d
    if out is None:
        out = torch.empty((B * N, Cn), dtype=F16, device=q.device)
    _chk_f16_rows(out, "region_attention.out")
    for t, name in ((q, "q"), (out, "out")):
        if t.shape[0] != B * N or t.shape[1] < Cn:
            raise RuntimeError(f"region_attention.{name}: expected [{B * N}, >= {Cn}], got {tuple(t.shape)}")
    for t, name in ((k, "k"), (vt, "vt")):
        if t.dtype != F16 or not t.is_cuda or t.stride(-1) != 1:
            raise RuntimeError(f"region_attention.{name}: expected an fp16 device tensor with a contiguous last dim, got {t.dtype} {t.device} strides {t.stride()}")
    if w.dtype != torch.float32 or not w.is_cuda or w.dim() != 2 or w.stride(1) != 1 or w.shape[0] != B * R or w.shape[1] < N:
        raise RuntimeError(f"region_attention.w: expected an fp32 device matrix [{B * R}, >= {N}] with contiguous rows, got {w.dtype} {w.device} "
                           f"{tuple(w.shape)} strides {w.stride()}")
    if vt.dim() != 3 or vt.shape[0] != B * R or vt.shape[1] != Cn:
        raise RuntimeError(f"region_attention.vt: expected [{B * R}, {Cn}, ldv], got {tuple(vt.shape)}")
    _launch("af_region_attention", _p(q), _ld(q), _p(k), int(ldk), _p(vt), vt.stride(1), vt.stride(0), _p(w), w.stride(0), _p(out), _ld(out),
            B, R, N, L, heads, d, float(d ** -0.5 if scale is None else scale))
    return out


def region_level_sizes(H: int, W: int):
    """Tokens of the four U-Net levels of an H x W-pixel image (latent side = pixels / 8, then / 1, 2, 4, 8)."""
    n0 = (H // 8) * (W // 8)
    return [n0, n0 // 4, n0 // 16, n0 // 64]


def region_weights(masks, beta: float, H: Optional[int] = None, W: Optional[int] = None, device=None):
    """The region weights of all four U-Net levels in one launch (af_region_weights).  masks uint8 [R-1, H, W] on the device (0 .. 255, 255 = the
    region; None with H, W and device for no region: R = 1) -> (w fp32 [R, sum N_l], [views [R, N_l] of its column ranges, l = 0 .. 3]).
    Each mask is area-averaged onto the level's token grid, then w_r = (1 - beta) m_r / max(1, s), w_0 = beta + (1 - beta)(1 - min(1, s)),
    s = sum_r m_r.  H and W are multiples of 64."""
    if masks is not None:
        if masks.dtype != torch.uint8 or not masks.is_cuda or masks.dim() != 3 or not masks.is_contiguous():
            raise RuntimeError(f"region_weights.masks: expected a contiguous uint8 device tensor [R-1, H, W], got {masks.dtype} {masks.device} {tuple(masks.shape)}")
        H, W, device = masks.shape[1], masks.shape[2], masks.device
    R = 1 if masks is None else masks.shape[0] + 1
    sizes = region_level_sizes(H, W)
    w = torch.empty((R, sum(sizes)), dtype=torch.float32, device=device)
    _launch("af_region_weights", _p(masks), R, H, W, float(beta), _p(w), w.stride(0))
    levels, off = [], 0
    for n in sizes:
        levels.append(w[:, off:off + n])
        off += n
    return w, levels


_freeu_ws = {}


def _chk_freeu(h, skip, b, s, version):
    _chk_f16(h, "freeu.h")
    _chk_f16(skip, "freeu.skip")
    if h.dim() != 4 or skip.dim() != 4 or h.shape[:3] != skip.shape[:3] or h.device != skip.device:
        raise RuntimeError(f"freeu: h and skip must be [B, H, W, C] and [B, H, W, Cs] on one device, got {tuple(h.shape)} and {tuple(skip.shape)}")
    return (h.shape[0], h.shape[1], h.shape[2], h.shape[3], skip.shape[3], float(b), float(s), int(version))


def freeu_workspace_size(B: int, H: int, W: int, C: int, Cs: int) -> int:
    """fp32 elements of the workspace af_freeu_stats / af_freeu_apply share at these sizes (the library's own count)."""
    return _checked("af_freeu_ws_floats", B, H, W, C, Cs)


def freeu_stats(h, skip, b: float, s: float, version: int = 2, ws=None):
    """The statistics pass of FreeU (af_freeu_stats, one launch; none when b == s == 1): the pixel means of h with their (lo, hi) partials and the
    seven shifted sums of every skip plane, into ``ws`` (fp32, >= freeu_workspace_size; default: the per-device scratch).  Returns ws."""
    args = _chk_freeu(h, skip, b, s, version)
    if ws is None:
        ws = _grow_scratch(_freeu_ws, h.device, freeu_workspace_size(*args[:5]), torch.float32)
    elif ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous():
        raise RuntimeError(f"freeu_stats.ws: expected a contiguous fp32 device tensor, got {ws.dtype} {ws.device}")
    _launch("af_freeu_stats", _p(h), _p(skip), _p(ws), ws.numel(), *args)
    return ws


def freeu(h, skip, b: float, s: float, version: int = 2, out_h=None, out_skip=None):
    """FreeU on the inputs of a skip concatenation, h [B, H, W, C] and skip [B, H, W, Cs] (contiguous NHWC fp16) -> (h', skip'): the first C/2
    channels of h times (b - 1) * mhat + 1 (version 2; b for version 1), every skip plane with its lowest spatial frequencies scaled by s
    (include/adaface_hip.h).  Two launches, af_freeu_stats and af_freeu_apply; b == 1 or s == 1 leaves that tensor alone (it is returned as it
    is, or copied when another ``out_*`` is given), and b == s == 1 launches nothing.  ``out_h`` / ``out_skip``: write there; the input itself
    (in place) is allowed and, for h, spares the copy of the untouched upper half of the channels.  Statistics a producer attached to a tensor
    written in place are dropped (the write bypasses torch's version counter)."""
    args = _chk_freeu(h, skip, b, s, version)
    b, s = args[5], args[6]
    for o, x, name in ((out_h, h, "out_h"), (out_skip, skip, "out_skip")):
        if o is not None and o is not x:
            _chk_f16(o, f"freeu.{name}")
            if o.shape != x.shape or o.device != x.device:
                raise RuntimeError(f"freeu.{name}: expected {tuple(x.shape)} on {x.device}, got {tuple(o.shape)} on {o.device}")
    do_h, do_s = b != 1.0, s != 1.0
    if do_h or do_s:
        ws = freeu_stats(h, skip, b, s, version)          # refuses bad b / s / version / sizes before anything is written
    oh = h if not do_h and out_h is None else (torch.empty_like(h) if out_h is None else out_h)
    os_ = skip if not do_s and out_skip is None else (torch.empty_like(skip) if out_skip is None else out_skip)
    Cn = h.shape[3]
    if oh is not h:
        if do_h:
            oh[..., Cn // 2:] = h[..., Cn // 2:]           # the kernel writes the first half only
        else:
            oh.copy_(h)
    if os_ is not skip and not do_s:
        os_.copy_(skip)
    if do_h or do_s:
        _launch("af_freeu_apply", _p(h), _p(skip), _p(ws), ws.numel(), _p(oh), _p(os_), *args)
        for o, x, did in ((oh, h, do_h), (os_, skip, do_s)):
            if did and o is x and getattr(o, "_gn_partials", None) is not None:
                o._gn_partials = None
    return oh, os_


def softmax_rows_bwd(p, dp):
    """ds = p * (dp - rowsum(p * dp)) for fp16 [rows, L] probabilities and their gradient."""
    _chk_f16(p, "softmax_rows_bwd.p")
    _chk_f16(dp, "softmax_rows_bwd.dp")
    assert p.shape == dp.shape
    ds = torch.empty_like(p)
    _launch("af_softmax_rows_bwd", _p(p), _p(dp), _p(ds), p.shape[0], p.shape[1])
    return ds


def mask_pairs_(p, cls):
    """In place: p [N, N] fp16 *= ((cls[i] & cls[j]) != 0); cls uint8 [N] (bit 0 foreground, bit 1 background)."""
    assert p.shape[0] == p.shape[1] == cls.numel() and cls.dtype == torch.uint8
    _launch("af_mask_pairs", _p(p), _p(cls), p.shape[0])
    return p


# ----------------------------------------------------------------------------- trainable DoRA adapters
def dora_combine(y0, c2, lb, u, v):
    """y0 + u[c] * c2 + v[c] * lb over the last (channel) axis; u, v fp32 [C]."""
    Cn = y0.shape[-1]
    out = torch.empty_like(y0)
    _launch("af_dora_combine", _p(y0), _p(c2), _p(lb), _p(u), _p(v), _p(out), y0.numel() // Cn, Cn)
    return out


def mul(a, b):
    _chk_f16(a, "mul.a")
    _chk_f16(b, "mul.b")
    assert a.shape == b.shape
    out = torch.empty_like(a)
    _launch("af_mul_f16", _p(a), _p(b), _p(out), a.numel())
    return out


def im2col3x3(x, stride=1):
    """x [B,H,W,C] fp16 -> [B*Ho*Wo, 9*C], column order (ky, kx, c)."""
    B, H, W, Cn = x.shape
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    out = torch.empty((B * Ho * Wo, 9 * Cn), dtype=F16, device=x.device)
    _launch("af_im2col3x3", _p(x), _p(out), B, H, W, Cn, stride)
    return out


# ----------------------------------------------------------------------------- ArcFace ResNetFace encoder
def _chk_face_params(op, device, Cn, scale=None, shift=None, slope=None):
    """scale / shift: contiguous fp32 [C] on the tensors' device, both or neither; slope: one fp32 value there (nn.PReLU())."""
    if (scale is None) != (shift is None):
        raise RuntimeError(f"{op}.{'shift' if shift is None else 'scale'}: scale and shift go together")
    for name, t, shape in (("scale", scale, (Cn,)), ("shift", shift, (Cn,)), ("slope", slope, (1,))):
        if t is not None and (t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or tuple(t.shape) != shape):
            raise RuntimeError(f"{op}.{name}: expected contiguous fp32 {shape} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _chk_f16_like(t, ref, shape, name):
    """t: a contiguous fp16 tensor of ``shape`` on ``ref``'s device."""
    _chk_f16(t, name)
    if tuple(t.shape) != tuple(shape) or t.device != ref.device:
        raise RuntimeError(f"{name}: expected {tuple(shape)} on {ref.device}, got {tuple(t.shape)} on {t.device}")


def _chk_even_nhwc(x, name):
    _chk_nhwc(x, name)
    if x.shape[1] % 2 or x.shape[2] % 2:
        raise RuntimeError(f"{name}: the 2x2 / stride 2 pool needs an even height and width, got {tuple(x.shape)}")


def affine_prelu(x, scale=None, shift=None, slope=None):
    """y = prelu(x * scale[c] + shift[c]) over the last (channel) axis; any of the two stages may be absent."""
    _chk_f16(x, "affine_prelu.x")
    Cn = x.shape[-1]
    _chk_face_params("affine_prelu", x.device, Cn, scale, shift, slope)
    y = torch.empty_like(x)
    _launch("af_affine_prelu", _p(x), _p(scale), _p(shift), _p(slope), _p(y), x.numel() // Cn, Cn)
    return y


def affine_prelu_ch(x, scale=None, shift=None, slope=None):
    """``affine_prelu`` with one PReLU slope per channel (slope fp32 [C], nn.PReLU(C)): IResNet's activations."""
    _chk_f16(x, "affine_prelu_ch.x")
    Cn = x.shape[-1]
    for name, t in (("scale", scale), ("shift", shift), ("slope", slope)):
        if t is not None and (t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or tuple(t.shape) != (Cn,)):
            raise RuntimeError(f"affine_prelu_ch.{name}: expected contiguous fp32 ({Cn},) on {x.device}, got {t.dtype} {tuple(t.shape)} "
                               f"on {t.device}")
    y = torch.empty_like(x)
    _launch("af_affine_prelu_ch", _p(x), _p(scale), _p(shift), _p(slope), _p(y), x.numel() // Cn, Cn)
    return y


def face_align_crop(image_u8, inv_mats, size=112):
    """uint8 RGB photo [H, W, 3] + inverse similarity matrices fp32 [F, 2, 3] (crop -> image) -> the recogniser's input, fp16
    [F, size, size, 8]: bilinear, cv2.warpAffine's pixel convention, outside the image = 0, (v - 127.5) / 127.5 in channels 0-2, zeros in
    3-7.  One launch per image (af_face_align_crop)."""
    if image_u8.dtype != torch.uint8 or not image_u8.is_cuda or not image_u8.is_contiguous():
        raise RuntimeError(f"face_align_crop: expected a contiguous uint8 device tensor, got {image_u8.dtype} {image_u8.device} "
                           f"contiguous={image_u8.is_contiguous()}")
    if image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise RuntimeError(f"face_align_crop: expected [H, W, 3], got {tuple(image_u8.shape)}")
    if (inv_mats.dtype != torch.float32 or inv_mats.device != image_u8.device or not inv_mats.is_contiguous() or inv_mats.dim() != 3
            or tuple(inv_mats.shape[1:]) != (2, 3)):
        raise RuntimeError(f"face_align_crop.inv_mats: expected contiguous fp32 [F, 2, 3] on {image_u8.device}, got {inv_mats.dtype} "
                           f"{tuple(inv_mats.shape)} on {inv_mats.device}")
    H, W, _ = image_u8.shape
    nf, size = inv_mats.shape[0], int(size)
    if size not in (112, 128):                       # (before the allocation: the C ABI refuses it too)
        raise RuntimeError(f"face_align_crop: size must be 112 or 128, got {size}")
    out = torch.empty((nf, size, size, 8), dtype=F16, device=image_u8.device)
    _launch("af_face_align_crop", _p(image_u8), _p(inv_mats), _p(out), H, W, nf, size)
    return out


def face_align_crop_any(image_u8, inv_mats, size):
    """``face_align_crop`` at the face restorer's crop sizes (af_face_align_crop_any): any multiple of 8 from 8 to 1024."""
    if image_u8.dtype != torch.uint8 or not image_u8.is_cuda or not image_u8.is_contiguous() or image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise RuntimeError(f"face_align_crop_any: expected a contiguous uint8 device tensor [H, W, 3], got {image_u8.dtype} {tuple(image_u8.shape)} "
                           f"on {image_u8.device}")
    if (inv_mats.dtype != torch.float32 or inv_mats.device != image_u8.device or not inv_mats.is_contiguous() or inv_mats.dim() != 3
            or tuple(inv_mats.shape[1:]) != (2, 3) or inv_mats.shape[0] < 1):
        raise RuntimeError(f"face_align_crop_any.inv_mats: expected contiguous fp32 [F >= 1, 2, 3] on {image_u8.device}, got {inv_mats.dtype} "
                           f"{tuple(inv_mats.shape)} on {inv_mats.device}")
    H, W, _ = image_u8.shape
    nf, size = inv_mats.shape[0], int(size)
    if size < 8 or size > 1024 or size % 8:
        raise RuntimeError(f"face_align_crop_any: size must be a multiple of 8 from 8 to 1024, got {size}")
    out = torch.empty((nf, size, size, 8), dtype=F16, device=image_u8.device)
    _launch("af_face_align_crop_any", _p(image_u8), _p(inv_mats), _p(out), H, W, nf, size)
    return out


# ----------------------------------------------------------------------------- GFPGAN face restorer (af_gfpgan.hip)
def _chk_f32(t, shape, name, device):
    if t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected contiguous fp32 {tuple(shape)} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def modulate_weights(w, wsq, styles, out, gain=1.0):
    """Per-sample weights of a modulated convolution (af_modulate_weights): w fp32 [cout, taps, cin], wsq fp32 [cout, cin] or None (no
    demodulation), styles fp32 [B, cin] -> out fp16 [B, npad, kpad] (the caller's buffer, zeroed once: only the cout x taps * cin block of every
    slice is written), out[b, o, t * cin + i] = gain * d[b, o] * w[o, t, i] * styles[b, i]."""
    cout, taps, cin = w.shape
    B = styles.shape[0]
    _chk_f32(w, (cout, taps, cin), "modulate_weights.w", out.device)
    _chk_f32(styles, (B, cin), "modulate_weights.styles", out.device)
    if wsq is not None:
        _chk_f32(wsq, (cout, cin), "modulate_weights.wsq", out.device)
    _chk_f16(out, "modulate_weights.out")
    if out.dim() != 3 or out.shape[0] != B:
        raise RuntimeError(f"modulate_weights.out: expected [{B}, npad, kpad], got {tuple(out.shape)}")
    _launch("af_modulate_weights", _p(w), _p(wsq), _p(styles), _p(out), B, cout, cin, taps, out.shape[1], out.shape[2], int(wsq is not None), float(gain))
    return out


def style_epilogue(y, noise=None, bias=None, scale=None, shift=None, nw=0.0, out=None):
    """lrelu(y + nw * noise[p] + bias[c], 0.2), then v * scale + shift on the upper half of the channels, saturating at +-65504
    (af_style_epilogue).  y fp16 [B, H, W, C] (or [B, HW, C]); noise fp32 with H * W elements; bias fp32 [C]; scale / shift fp16 [B, H, W, C / 2].
    out=y works in place."""
    _chk_f16(y, "style_epilogue.y")
    B, Cn = y.shape[0], y.shape[-1]
    hw = y.numel() // (B * Cn)
    dev = y.device
    if noise is not None:
        _chk_f32(noise, noise.shape, "style_epilogue.noise", dev)
        if noise.numel() != hw:
            raise RuntimeError(f"style_epilogue.noise: expected {hw} elements, got {tuple(noise.shape)}")
    if bias is not None:
        _chk_f32(bias, (Cn,), "style_epilogue.bias", dev)
    if (scale is None) != (shift is None):
        raise RuntimeError("style_epilogue: scale and shift go together")
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _chk_f16(t, "style_epilogue." + name)
            if t.numel() != B * hw * (Cn // 2) or t.shape[-1] != Cn // 2 or Cn % 16:
                raise RuntimeError(f"style_epilogue.{name}: expected [B, HW, C / 2] for y {tuple(y.shape)}, got {tuple(t.shape)}")
    if out is None:
        out = torch.empty_like(y)
    else:
        _chk_f16(out, "style_epilogue.out")
        assert out.shape == y.shape
    _launch("af_style_epilogue", _p(y), _p(noise), _p(bias), _p(scale), _p(shift), _p(out), B, hw, Cn, float(nw))
    return out


def bilinear_up2(x, addend=None):
    """fp16 [B, H, W, C] -> [B, 2H, 2W, C], torch's bilinear x2 with align_corners=False (+ addend) (af_bilinear_up2)."""
    _chk_nhwc(x, "bilinear_up2.x")
    B, H, W, Cn = x.shape
    out = torch.empty((B, 2 * H, 2 * W, Cn), dtype=F16, device=x.device)
    if addend is not None:
        _chk_f16(addend, "bilinear_up2.addend")
        if addend.shape != out.shape:
            raise RuntimeError(f"bilinear_up2.addend: expected {tuple(out.shape)}, got {tuple(addend.shape)}")
    _launch("af_bilinear_up2", _p(x), _p(addend), _p(out), B, H, W, Cn)
    return out


def face_paste_affine_u8(photo_u8, crops, mats, erode, feather):
    """Restored crops back into the photo (af_face_paste_affine_u8): photo uint8 [H, W, 3], crops fp16 [F, S, S, ld] or None, mats fp32
    [F, 2, 3] (image -> crop) or None, erode / feather in crop pixels -> uint8 [H, W, 3]."""
    _chk_photo(photo_u8, "face_paste_affine_u8.photo")
    H, W, _ = photo_u8.shape
    nf = 0 if crops is None else crops.shape[0]
    out = torch.empty_like(photo_u8)
    S = ld = 0
    if nf:
        _chk_f16(crops, "face_paste_affine_u8.crops")
        if crops.dim() != 4 or crops.shape[1] != crops.shape[2] or crops.device != photo_u8.device:
            raise RuntimeError(f"face_paste_affine_u8.crops: expected [F, S, S, ld] on {photo_u8.device}, got {tuple(crops.shape)} on {crops.device}")
        _chk_f32(mats, (nf, 2, 3), "face_paste_affine_u8.mats", photo_u8.device)
        S, ld = crops.shape[1], crops.shape[3]
    _launch("af_face_paste_affine_u8", _p(photo_u8), _p(crops) if nf else None, _p(mats) if nf else None, _p(out), H, W, nf, S, ld,
            float(erode), float(feather))
    return out


# ----------------------------------------------------------------------------- RetinaFace detector (af_detect.hip)
RETINA_CAPACITY = 1024              # candidates per image af_retina_nms holds in LDS
RETINA_STEPS = (8, 16, 32)
RETINA_MIN_SIZES = ((16.0, 32.0), (64.0, 128.0), (256.0, 512.0))
STEM_COLS = 160                     # 7 * 7 * 3 = 147 columns of the stem's im2col rows, zero-padded to a multiple of 8


def _chk_nhwc(t, name):
    _chk_f16(t, name)
    if t.dim() != 4 or t.shape[3] % 8 or t.numel() == 0:
        raise RuntimeError(f"{name}: expected a non-empty NHWC tensor with C % 8 == 0, got {tuple(t.shape)}")


def stem_im2col7x7(images_u8, scale, shift, bgr=False):
    """uint8 RGB photos [B, H, W, 3] -> (fp16 rows [B * Ho * Wo, 160] of the 7x7 / stride 2 / pad 3 stem over the image padded to multiples
    of 32, (Ho, Wo)); columns (ky, kx, c) = v * scale[c] + shift[c], a tap outside the image 0, columns 147-159 zero (af_stem_im2col7x7).
    scale, shift: three floats each."""
    if images_u8.dtype != torch.uint8 or not images_u8.is_cuda or not images_u8.is_contiguous():
        raise RuntimeError(f"stem_im2col7x7: expected a contiguous uint8 device tensor, got {images_u8.dtype} {images_u8.device} "
                           f"contiguous={images_u8.is_contiguous()}")
    if images_u8.dim() != 4 or images_u8.shape[3] != 3 or images_u8.numel() == 0:
        raise RuntimeError(f"stem_im2col7x7: expected [B, H, W, 3], got {tuple(images_u8.shape)}")
    scale, shift = [float(v) for v in scale], [float(v) for v in shift]
    if len(scale) != 3 or len(shift) != 3:
        raise RuntimeError("stem_im2col7x7: scale and shift take three values each")
    B, H, W, _ = images_u8.shape
    Ho, Wo = round_up(H, 32) // 2, round_up(W, 32) // 2
    if B * H * W * 3 >= 1 << 31 or B * Ho * Wo * STEM_COLS * 2 >= 1 << 31:           # (before the allocation: the C ABI refuses it too)
        raise RuntimeError(f"stem_im2col7x7: {tuple(images_u8.shape)} needs 2^31 bytes or more in one operand; split the batch")
    out = torch.empty((B * Ho * Wo, STEM_COLS), dtype=F16, device=images_u8.device)
    f3 = C.c_float * 3
    _launch("af_stem_im2col7x7", _p(images_u8), f3(*scale), f3(*shift), _p(out), B, H, W, int(bool(bgr)))
    return out, (Ho, Wo)


def relu_maxpool3x3s2(x):
    """relu(max_pool2d(x, 3, 2, 1)) on NHWC fp16."""
    _chk_nhwc(x, "relu_maxpool3x3s2.x")
    B, H, W, Cn = x.shape
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cn), dtype=F16, device=x.device)
    _launch("af_relu_maxpool3x3s2", _p(x), _p(y), B, H, W, Cn)
    return y


def subsample2x(x):
    """x[:, ::2, ::2, :] as a contiguous NHWC tensor: what a stride-2 1x1 convolution reads."""
    _chk_nhwc(x, "subsample2x.x")
    B, H, W, Cn = x.shape
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, Cn), dtype=F16, device=x.device)
    _launch("af_subsample2x", _p(x), _p(y), B, H, W, Cn)
    return y


def upsample2x_add(a, b):
    """a [B, 2h, 2w, C] + nearest2x(b [B, h, w, C])."""
    _chk_nhwc(a, "upsample2x_add.a")
    _chk_nhwc(b, "upsample2x_add.b")
    B, h, w, Cn = b.shape
    if tuple(a.shape) != (B, 2 * h, 2 * w, Cn) or a.device != b.device:
        raise RuntimeError(f"upsample2x_add: a must be [B, 2h, 2w, C] for b {tuple(b.shape)} on {b.device}, got {tuple(a.shape)} on {a.device}")
    y = torch.empty_like(a)
    _launch("af_upsample2x_add", _p(a), _p(b), _p(y), B, h, w, Cn)
    return y


def retina_decode(heads, level_hw, conf_thr, capacity=RETINA_CAPACITY, steps=RETINA_STEPS, min_sizes=RETINA_MIN_SIZES):
    """Three head tensors fp16 [B, Hk * Wk, 32] (per anchor 16 columns [box 4 | cls 2 | ldm 10]) -> (cand fp32 [B, capacity, 16], count
    int32 [B]): the rows x1, y1, x2, y2, score, 10 landmark coordinates, anchor index of the anchors with score >= conf_thr, in pixels, in
    no particular order (af_retina_decode; the rules are in include/adaface_hip.h).  count is the number that passed, also beyond capacity."""
    if len(heads) != 3 or len(level_hw) != 3:
        raise RuntimeError("retina_decode: three levels")
    B = heads[0].shape[0]
    for k, (hd, (hk, wk)) in enumerate(zip(heads, level_hw)):
        _chk_f16(hd, f"retina_decode.heads[{k}]")
        if tuple(hd.shape) != (B, hk * wk, 32) or hd.device != heads[0].device or hd.numel() == 0:
            raise RuntimeError(f"retina_decode.heads[{k}]: expected [{B}, {hk * wk}, 32] on {heads[0].device}, got {tuple(hd.shape)} on {hd.device}")
    capacity = int(capacity)
    if not 1 <= capacity <= RETINA_CAPACITY:
        raise RuntimeError(f"retina_decode: capacity must be in [1, {RETINA_CAPACITY}], got {capacity}")
    cand = torch.empty((B, capacity, 16), dtype=torch.float32, device=heads[0].device)
    count = torch.empty((B,), dtype=torch.int32, device=heads[0].device)
    hw = (C.c_int * 6)(*[int(v) for pair in level_hw for v in pair])
    st = (C.c_int * 3)(*[int(v) for v in steps])
    ms = (C.c_float * 6)(*[float(v) for pair in min_sizes for v in pair])
    _launch("af_retina_decode", _p(heads[0]), _p(heads[1]), _p(heads[2]), hw, st, ms, B, float(conf_thr), _p(cand), _p(count), capacity)
    return cand, count


def retina_nms(cand, count, nms_thr, max_det=64):
    """Sort + greedy suppression of ``retina_decode``'s lists (af_retina_nms) and ONE device-to-host copy -> (table fp32 [B, max_det, 16] in
    kept order, rows beyond ``kept`` zero; counts int32 [B, 2] = (kept, passing)), host tensors.  More passing anchors than the capacity:
    RuntimeError (which of them made the list depends on scheduling, so it is never returned)."""
    if cand.dtype != torch.float32 or not cand.is_cuda or not cand.is_contiguous() or cand.dim() != 3 or cand.shape[2] != 16:
        raise RuntimeError(f"retina_nms.cand: expected contiguous fp32 [B, C, 16] on the device, got {cand.dtype} {tuple(cand.shape)} on {cand.device}")
    B, cap, _ = cand.shape
    if count.dtype != torch.int32 or count.device != cand.device or not count.is_contiguous() or tuple(count.shape) != (B,):
        raise RuntimeError(f"retina_nms.count: expected contiguous int32 [{B}] on {cand.device}, got {count.dtype} {tuple(count.shape)} on {count.device}")
    max_det = int(max_det)
    if not 1 <= cap <= RETINA_CAPACITY or not 1 <= max_det <= cap:
        raise RuntimeError(f"retina_nms: needs 1 <= max_det <= capacity <= {RETINA_CAPACITY}, got max_det {max_det}, capacity {cap}")
    buf = torch.empty((B * max_det * 16 + B * 2,), dtype=torch.float32, device=cand.device)          # table | counts: one copy out
    table, counts = buf[:B * max_det * 16], buf[B * max_det * 16:]
    _launch("af_retina_nms", _p(cand), _p(count), _p(table), _p(counts), B, cap, max_det, float(nms_thr))
    host = buf.cpu()
    table, counts = host[:B * max_det * 16].reshape(B, max_det, 16), host[B * max_det * 16:].view(torch.int32).reshape(B, 2)
    if int(counts[:, 1].max()) > cap:
        raise RuntimeError(f"retina_nms: {int(counts[:, 1].max())} anchors passed the confidence threshold in one image, more than the "
                           f"{cap} the detector keeps; raise the confidence threshold")
    return table, counts


def maxpool2x2(x):
    """2x2 / stride 2 max over NHWC fp16; the height and width must be even (the kernel rebuilds the source row stride from the output width)."""
    _chk_even_nhwc(x, "maxpool2x2.x")
    B, H2, W2, Cn = x.shape
    y = torch.empty((B, H2 // 2, W2 // 2, Cn), dtype=F16, device=x.device)
    _launch("af_maxpool2x2", _p(x), _p(y), B, H2 // 2, W2 // 2, Cn)
    return y


def global_avgpool(x):
    _chk_f16(x, "global_avgpool.x")
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError(f"global_avgpool.x: expected a non-empty NHWC tensor, got {tuple(x.shape)}")
    B, H, W, Cn = x.shape
    out = torch.empty((B, Cn), dtype=F16, device=x.device)
    _launch("af_global_avgpool", _p(x), _p(out), B, H * W, Cn)
    return out


def se_residual_prelu(x, se_logits, residual, slope):
    _chk_nhwc(x, "se_residual_prelu.x")
    B, H, W, Cn = x.shape
    _chk_f16_like(residual, x, x.shape, "se_residual_prelu.residual")
    if se_logits is not None:
        _chk_f16_like(se_logits, x, (B, Cn), "se_residual_prelu.se_logits")
    if slope is None:
        raise RuntimeError("se_residual_prelu.slope: the block's PReLU slope is required")
    _chk_face_params("se_residual_prelu", x.device, Cn, slope=slope)
    y = torch.empty_like(x)
    _launch("af_se_residual_prelu", _p(x), _p(se_logits), _p(residual), _p(slope), _p(y), B, H * W, Cn)
    return y


def affine_prelu_bwd(dy, x=None, scale=None, shift=None, slope=None):
    """Input gradient of ``affine_prelu``; x (the forward input) is only read when there is a PReLU."""
    _chk_f16(dy, "affine_prelu_bwd.dy")
    Cn = dy.shape[-1]
    if x is not None:
        _chk_f16_like(x, dy, dy.shape, "affine_prelu_bwd.x")
    elif slope is not None:
        raise RuntimeError("affine_prelu_bwd.x: the PReLU gradient needs the forward input x")
    _chk_face_params("affine_prelu_bwd", dy.device, Cn, scale, shift, slope)
    dx = torch.empty_like(dy)
    _launch("af_affine_prelu_bwd", _p(x), _p(scale), _p(shift), _p(slope), _p(dy), _p(dx), dy.numel() // Cn, Cn)
    return dx


def maxpool2x2_bwd(x, dy):
    """dy routed to the first maximum of each 2x2 window of x (torch's rule); every element of dx is written."""
    _chk_even_nhwc(x, "maxpool2x2_bwd.x")
    B, H2, W2, Cn = x.shape
    _chk_f16_like(dy, x, (B, H2 // 2, W2 // 2, Cn), "maxpool2x2_bwd.dy")
    dx = torch.empty_like(x)
    _launch("af_maxpool2x2_bwd", _p(x), _p(dy), _p(dx), B, H2 // 2, W2 // 2, Cn)
    return dx


def _chk_se_operands(op, x, se_logits, residual, slope, dy):
    _chk_f16(x, f"{op}.x")
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError(f"{op}.x: expected a non-empty NHWC tensor, got {tuple(x.shape)}")
    _chk_f16_like(residual, x, x.shape, f"{op}.residual")
    _chk_f16_like(dy, x, x.shape, f"{op}.dy")
    if se_logits is not None:
        _chk_f16_like(se_logits, x, (x.shape[0], x.shape[3]), f"{op}.se_logits")
    if slope is None:
        raise RuntimeError(f"{op}.slope: the block's PReLU slope is required")
    _chk_face_params(op, x.device, x.shape[3], slope=slope)


def se_gate_grad(x, se_logits, residual, slope, dy):
    """-> fp16 [B, C]: gradient of the SE logits divided by H*W (see include/adaface_hip.h)."""
    if se_logits is None:
        raise RuntimeError("se_gate_grad.se_logits: the gate logits are required")
    _chk_se_operands("se_gate_grad", x, se_logits, residual, slope, dy)
    B, H, W, Cn = x.shape
    dgl = torch.empty((B, Cn), dtype=F16, device=x.device)
    _launch("af_se_gate_grad", _p(x), _p(se_logits), _p(residual), _p(slope), _p(dy), _p(dgl), B, H * W, Cn)
    return dgl


def se_residual_prelu_bwd(x, se_logits, residual, slope, dy, dpool=None):
    """-> (dx, dresidual) of ``se_residual_prelu``; dpool [B, C] is the squeeze branch's gradient (1/HW included)."""
    _chk_se_operands("se_residual_prelu_bwd", x, se_logits, residual, slope, dy)
    B, H, W, Cn = x.shape
    if dpool is not None:
        _chk_f16_like(dpool, x, (B, Cn), "se_residual_prelu_bwd.dpool")
    dx, dres = torch.empty_like(x), torch.empty_like(x)
    _launch("af_se_residual_prelu_bwd", _p(x), _p(se_logits), _p(residual), _p(slope), _p(dy), _p(dpool), _p(dx), _p(dres), B, H * W, Cn)
    return dx, dres


# ----------------------------------------------------------------------------- repainting faces in a photo (af_repaint.hip)
def _chk_photo(photo_u8, name):
    if photo_u8.dtype != torch.uint8 or not photo_u8.is_cuda or not photo_u8.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous uint8 device tensor, got {photo_u8.dtype} {photo_u8.device} "
                           f"contiguous={photo_u8.is_contiguous()}")
    if photo_u8.dim() != 3 or photo_u8.shape[2] != 3 or photo_u8.numel() == 0:
        raise RuntimeError(f"{name}: expected a non-empty [H, W, 3], got {tuple(photo_u8.shape)}")
    if photo_u8.numel() >= 1 << 31:                          # (before any allocation: the C ABI refuses it too)
        raise RuntimeError(f"{name}: {tuple(photo_u8.shape)} needs 2^31 bytes or more")


def _chk_alpha(alpha, photo_u8, name):
    H, W, _ = photo_u8.shape
    if (alpha.dtype != torch.float32 or alpha.device != photo_u8.device or not alpha.is_contiguous() or tuple(alpha.shape) != (H, W)):
        raise RuntimeError(f"{name}: expected contiguous fp32 [{H}, {W}] on {photo_u8.device}, got {alpha.dtype} {tuple(alpha.shape)} on "
                           f"{alpha.device}")


def _chk_rect(rect, H, W, name):
    x0, y0, cw, ch = (int(v) for v in rect)
    if x0 < 0 or y0 < 0 or cw < 1 or ch < 1 or x0 + cw > W or y0 + ch > H:
        raise RuntimeError(f"{name}: the rectangle (x0, y0, cw, ch) = {(x0, y0, cw, ch)} must be non-empty and inside the {W} x {H} photo")
    return x0, y0, cw, ch


def face_alpha_mask(ellipses, photo_hw, feather):
    """Ellipses fp32 [F, 4] rows (cx, cy, rx, ry) in photo pixels (F may be 0) -> the soft face mask alpha fp32 [H, W] on the ellipses'
    device: smoothstep of (1 - r) / feather per face, maximum over the faces (af_face_alpha_mask; the rule is in include/adaface_hip.h)."""
    if (ellipses.dtype != torch.float32 or not ellipses.is_cuda or not ellipses.is_contiguous() or ellipses.dim() != 2
            or ellipses.shape[1] != 4):
        raise RuntimeError(f"face_alpha_mask.ellipses: expected contiguous fp32 [F, 4] on the device, got {ellipses.dtype} "
                           f"{tuple(ellipses.shape)} on {ellipses.device}")
    H, W = (int(v) for v in photo_hw)
    feather = float(feather)
    if H < 1 or W < 1 or H * W * 3 >= 1 << 31:               # (before the allocation: the C ABI refuses it too)
        raise RuntimeError(f"face_alpha_mask: the photo must be non-empty and need fewer than 2^31 bytes, got {W} x {H}")
    if not 0 <= feather < float("inf"):
        raise RuntimeError(f"face_alpha_mask: feather must be finite and >= 0, got {feather}")
    alpha = torch.empty((H, W), dtype=torch.float32, device=ellipses.device)
    nf = ellipses.shape[0]
    _launch("af_face_alpha_mask", _p(ellipses) if nf else None, _p(alpha), nf, H, W, feather)
    return alpha


def crop_resize_u8(photo_u8, alpha, rect, work_hw, thr=1.0 / 255.0):
    """photo uint8 [H, W, 3] and alpha fp32 [H, W], rect = (x0, y0, cw, ch), work_hw = (Hs, Ws) multiples of 8 -> (image uint8
    [1, Hs, Ws, 3], mask_lat fp32 {0, 1} [1, 1, Hs/8, Ws/8]): the rectangle resampled by torch's antialiased bilinear rule and rounded to
    even, and the latent cells whose 8 x 8 block of the resampled alpha reaches thr.  One launch (af_crop_resize_u8)."""
    _chk_photo(photo_u8, "crop_resize_u8.photo")
    _chk_alpha(alpha, photo_u8, "crop_resize_u8.alpha")
    H, W, _ = photo_u8.shape
    x0, y0, cw, ch = _chk_rect(rect, H, W, "crop_resize_u8")
    Hs, Ws = (int(v) for v in work_hw)
    if Hs < 8 or Ws < 8 or Hs % 8 or Ws % 8 or Hs * Ws * 3 >= 1 << 31:
        raise RuntimeError(f"crop_resize_u8: the working size must be positive multiples of 8 below 2^31 bytes, got {Ws} x {Hs}")
    image = torch.empty((1, Hs, Ws, 3), dtype=torch.uint8, device=photo_u8.device)
    mask_lat = torch.empty((1, 1, Hs // 8, Ws // 8), dtype=torch.float32, device=photo_u8.device)
    _launch("af_crop_resize_u8", _p(photo_u8), _p(alpha), _p(image), _p(mask_lat), H, W, x0, y0, cw, ch, Hs, Ws, float(thr))
    return image, mask_lat


def paste_back_u8(decoded, photo_u8, alpha, rect):
    """decoded fp32 [B, 3, Hs, Ws] (what the VAE decodes, nominally in [-1, 1]) resampled to the rectangle, mapped to [0, 255], blended into
    the photo under alpha and rounded to even -> uint8 [B, H, W, 3]; outside the rectangle and wherever alpha == 0 the photo's own bytes.
    One launch (af_paste_back_u8)."""
    _chk_photo(photo_u8, "paste_back_u8.photo")
    _chk_alpha(alpha, photo_u8, "paste_back_u8.alpha")
    if (decoded.dtype != torch.float32 or decoded.device != photo_u8.device or not decoded.is_contiguous() or decoded.dim() != 4
            or decoded.shape[1] != 3 or decoded.numel() == 0):
        raise RuntimeError(f"paste_back_u8.decoded: expected non-empty contiguous fp32 [B, 3, Hs, Ws] on {photo_u8.device}, got {decoded.dtype} "
                           f"{tuple(decoded.shape)} on {decoded.device}")
    H, W, _ = photo_u8.shape
    x0, y0, cw, ch = _chk_rect(rect, H, W, "paste_back_u8")
    B, _, Hs, Ws = decoded.shape
    if B * H * W * 3 >= 1 << 31 or decoded.numel() >= 1 << 31:
        raise RuntimeError(f"paste_back_u8: {B} photos of {W} x {H} (or decoded {tuple(decoded.shape)}) need 2^31 bytes / elements or more; "
                           "split the batch")
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=photo_u8.device)
    _launch("af_paste_back_u8", _p(decoded), _p(photo_u8), _p(alpha), _p(out), B, Hs, Ws, H, W, x0, y0, cw, ch)
    return out


# ----------------------------------------------------------------------------- Real-ESRGAN (adaface/esrgan.py)
def _chk_nhwc_buf(t, name):
    if t.dtype != F16 or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 or t.numel() == 0:
        raise RuntimeError(f"{name}: expected a non-empty contiguous fp16 device tensor [B, H, W, ld], got {t.dtype} {tuple(t.shape)} on {t.device}")


def _slice_ptr(t, ch, cout, grid, name):
    """Address of channel ``ch`` of the NHWC buffer ``t`` (whose [B, H, W] must be ``grid``) and its row stride."""
    _chk_nhwc_buf(t, name)
    if tuple(t.shape[:3]) != tuple(grid) or ch < 0 or ch % 8 or ch + cout > t.shape[3]:
        raise RuntimeError(f"{name}: channels [{ch}, {ch + cout}) of {tuple(t.shape)} do not fit the output grid {tuple(grid)} (the offset "
                           "must be a multiple of 8)")
    return t.data_ptr() + 2 * ch, t.shape[3]


def dense_conv3x3_weight(weight: torch.Tensor, cin_pad: Optional[int] = None) -> torch.Tensor:
    """A torch conv weight [cout, cin, 3, 3] -> af_dense_conv3x3's fp16 [npad][9 * cin_pad] (K order (ky, kx, c)), npad = cout rounded up to
    16, input channels zero-padded to ``cin_pad`` (default: cin rounded up to 32)."""
    cout, cin = weight.shape[:2]
    cp = cin_pad if cin_pad is not None else (cin + 31) // 32 * 32
    w = torch.zeros(((cout + 15) // 16 * 16, 3, 3, cp), dtype=F16, device=weight.device)
    w[:cout, :, :, :cin] = weight.permute(0, 2, 3, 1).to(F16)
    return w.reshape(w.shape[0], 9 * cp).contiguous()


def dense_conv3x3(x, cin, wt, bias, out, out_ch, cout, r1=None, r1_ch=0, alpha=1.0, r2=None, r2_ch=0, beta=1.0, slope=0.0, upsample=False):
    """One af_dense_conv3x3 launch: the 3x3 convolution (pad 1) of channels [0, cin) of the NHWC buffer ``x`` [B, H, W, ldx] (nearest-x2
    upsampled first under ``upsample``, never materialised) written to channels [out_ch, out_ch + cout) of ``out`` [B, Ho, Wo, ldo], which
    may be ``x`` itself on channels behind cin.  v = lrelu(conv + bias, slope); with r1: v = alpha v + r1[..., r1_ch:]; with r2 too:
    v = beta v + r2[..., r2_ch:].  Nothing else of ``out`` is written.  ``wt`` as dense_conv3x3_weight makes it, ``bias`` fp32 [cout] or None."""
    _chk_nhwc_buf(x, "dense_conv3x3.x")
    B, H, W, ldx = x.shape
    grid = (B, 2 * H, 2 * W) if upsample else (B, H, W)
    po, ldo = _slice_ptr(out, out_ch, cout, grid, "dense_conv3x3.out")
    p1, ld1 = _slice_ptr(r1, r1_ch, cout, grid, "dense_conv3x3.r1") if r1 is not None else (None, 0)
    p2, ld2 = _slice_ptr(r2, r2_ch, cout, grid, "dense_conv3x3.r2") if r2 is not None else (None, 0)
    _launch("af_dense_conv3x3", _p(x), ldx, cin, _p(wt), _p(bias), po, ldo, cout, p1, ld1, alpha, p2, ld2, beta, slope, int(upsample), 0, B, H, W)
    return out


def dense_conv3x3_u8(x, cin, wt, bias, cout, slope=0.0, upsample=False):
    """As dense_conv3x3 with the uint8 epilogue: a new tight uint8 [B, Ho, Wo, cout] = rint(255 clamp(v, 0, 1)), ties to even."""
    _chk_nhwc_buf(x, "dense_conv3x3_u8.x")
    B, H, W, ldx = x.shape
    s = 2 if upsample else 1
    out = torch.empty((B, s * H, s * W, cout), dtype=torch.uint8, device=x.device)
    _launch("af_dense_conv3x3", _p(x), ldx, cin, _p(wt), _p(bias), _p(out), 0, cout, None, 0, 1.0, None, 0, 1.0, slope, int(upsample), 1, B, H, W)
    return out


def u8_unshuffle_f16(img_u8: torch.Tensor, r: int, cpad: int) -> torch.Tensor:
    """uint8 RGB [B, H, W, 3] -> fp16 [B, H / r, W / r, cpad]: pixel_unshuffle(img / 255, r) in torch's channel order, zeros behind 3 r^2."""
    if img_u8.dtype != torch.uint8 or not img_u8.is_cuda or not img_u8.is_contiguous() or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise RuntimeError(f"u8_unshuffle_f16: expected a contiguous uint8 device tensor [B, H, W, 3], got {img_u8.dtype} "
                           f"{tuple(img_u8.shape)} on {img_u8.device}")
    B, H, W, _ = img_u8.shape
    out = torch.empty((B, H // max(r, 1), W // max(r, 1), cpad), dtype=F16, device=img_u8.device)
    _launch("af_u8_unshuffle_f16", _p(img_u8), _p(out), B, H, W, r, cpad)
    return out


# ----------------------------------------------------------------------------- ControlNet (ldm/modules/diffusionmodules/controlnet.py)
def pack_hint_conv3x3(weight: torch.Tensor) -> torch.Tensor:
    """A torch conv weight [cout, cin, 3, 3] -> af_hint_conv3x3's fp16 [cout][9 * cpad] (K order (ky, kx, c)), input channels zero-padded to
    cpad = cin rounded up to a multiple of 32 (include/adaface_hip.h)."""
    cout, cin = weight.shape[:2]
    cp = (cin + 31) // 32 * 32
    w = torch.zeros((cout, 3, 3, cp), dtype=F16, device=weight.device)
    w[:, :, :, :cin] = weight.detach().permute(0, 2, 3, 1).to(F16)
    return w.reshape(cout, 9 * cp).contiguous()


def hint_conv3x3(x: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor], *, stride: int = 1, act: bool = True) -> torch.Tensor:
    """One af_hint_conv3x3 launch: 3x3 / pad 1 / stride 1 | 2 convolution of x -- fp16 NHWC [B, H, W, cin], or a uint8 RGB image [B, H, W, 3]
    read as x / 255 -- with ``wt`` as pack_hint_conv3x3 makes it and ``bias`` fp32 [cout] or None -> fp16 [B, Ho, Wo, cout], SiLU under ``act``."""
    if x.dtype not in (F16, torch.uint8) or not x.is_cuda or not x.is_contiguous() or x.dim() != 4 or x.numel() == 0:
        raise RuntimeError(f"hint_conv3x3: expected a non-empty contiguous fp16 or uint8 device tensor [B, H, W, C], got {x.dtype} "
                           f"{tuple(x.shape)} on {x.device}")
    B, H, W, cin = x.shape
    mode = int(x.dtype == torch.uint8)
    cp = (cin + 31) // 32 * 32
    if wt.dtype != F16 or not wt.is_cuda or not wt.is_contiguous() or wt.dim() != 2 or wt.shape[1] != 9 * cp:
        raise RuntimeError(f"hint_conv3x3: wt must be a contiguous fp16 device tensor [cout, {9 * cp}] (pack_hint_conv3x3), got {wt.dtype} "
                           f"{tuple(wt.shape)} on {wt.device}")
    cout = wt.shape[0]
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_cuda or not bias.is_contiguous() or tuple(bias.shape) != (cout,)):
        raise RuntimeError(f"hint_conv3x3: bias must be a contiguous fp32 device tensor [{cout}], got {bias.dtype} {tuple(bias.shape)}")
    s = int(stride)
    out = torch.empty((B, (H - 1) // max(s, 1) + 1, (W - 1) // max(s, 1) + 1, cout), dtype=F16, device=x.device)
    _launch("af_hint_conv3x3", _p(x), mode, cin, _p(wt), _p(bias), _p(out), cout, s, int(bool(act)), B, H, W)
    return out


# ----------------------------------------------------------------------------- profiling hook
def prof_enable(on: bool):
    _checked("af_prof_enable", int(on))


def prof_reset():
    _checked("af_prof_reset")


def prof_read(family: int):
    n, ms = C.c_int(0), C.c_double(0.0)
    _checked("af_prof_read", family, C.byref(n), C.byref(ms))
    return n.value, ms.value
