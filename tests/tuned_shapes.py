"""Operand geometry for every key of the tuned tile table (adaface-dev_amd/tuning/gfx950_gemm.json), shared by the GPU sweep
(test_hip_tuned_shapes.py) and its host-only coverage check (test_tuned_shapes_host.py).

A key is `taps,M,N,K,act,out_mode,stride,upsample[,ln]` (ops._launch_gemm).  It carries no image geometry, no split of K between two
sources and no K tail, so the sweep rebuilds them here:
  * taps 9, K % 9 == 0: a plain 3x3 convolution with cin = K / 9;
  * taps 9, K % 9 != 0: a ResBlock's second convolution with its 1x1 shortcut concatenated along K: cin = N, ktail = K - 9 N (a positive multiple
    of 64; the shortcut widths the project uses are never multiples of 9, so the two kinds cannot be confused);
  * geometry (a) is a square image at a project level (U-Net latent 64 / 32 / 16 / 8, VAE 512 ... 64, face 112 ... 7) with B = M / (Ho Wo);
    geometry (b), where the same M allows one, is a non-square image that the halo-resident kernel (tile 14) does not take.
"""
import os
import zlib
from dataclasses import dataclass
from typing import List, Optional

UNET_LEVELS = (64, 32, 16, 8)
VAE_LEVELS = (512, 256, 128, 64)
FACE_LEVELS = (112, 56, 28, 14, 7)
SKIP_CONCAT = {960: 640, 1280: 640, 1920: 1280, 2560: 1280}      # U-Net decoder inputs [h | skip]: cin -> width of the first source
SELF_ATTN_TOKENS = (4096, 1024, 256, 64)                          # q | k | v projections (out_mode 1, split_col = 2C)
CROSS_ATTN_TOKENS = (77, 97, 20)                                  # k | v projections of the context (K = 768)
ROWBIAS_TOKENS = (4096, 1024, 256, 64, 77, 97)

# ops / _lib constants, repeated so that this module imports without the package (the host test checks they agree)
AF_ACT_NONE, AF_ACT_SILU, AF_ACT_GEGLU, AF_ACT_QUICKGELU = 0, 1, 2, 3
AF_OUT_NORMAL, AF_OUT_SPLIT_T, AF_OUT_F32 = 0, 1, 2

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adaface-dev_amd", "tuning", "gfx950_gemm.json")


@dataclass(frozen=True)
class Key:
    taps: int
    M: int
    N: int
    K: int
    act: int
    out_mode: int
    stride: int
    upsample: int
    ln: bool


@dataclass(frozen=True)
class ConvGeo:
    B: int
    H: int
    W: int
    Ho: int
    Wo: int
    cin: int
    ktail: int
    stride: int
    upsample: int
    tap_shift: int = 0
    c2: int = 0            # second source (x2=) or, with a K tail, second skip source: its channel count
    label: str = "a"


def parse_key(key: str) -> Key:
    f = key.split(",")
    if len(f) not in (8, 9) or (len(f) == 9 and f[8] != "ln"):
        raise ValueError(f"tuned key {key!r}: expected taps,M,N,K,act,out_mode,stride,upsample[,ln]")
    taps, M, N, K, act, out_mode, stride, upsample = (int(v) for v in f[:8])
    k = Key(taps, M, N, K, act, out_mode, stride, upsample, len(f) == 9)
    if taps not in (1, 9) or min(M, N, K) <= 0 or act not in (0, 1, 2, 3) or out_mode not in (0, 1, 2):
        raise ValueError(f"tuned key {key!r}: unknown form")
    if taps == 9 and (act != 0 or out_mode != 0 or k.ln or stride not in (1, 2) or upsample not in (0, 1, 2) or (upsample and stride != 1)):
        raise ValueError(f"tuned key {key!r}: a 3x3 form the sweep cannot build")
    return k


def conv_channels(k: Key):
    """(cin, ktail) of a 3x3 key."""
    if k.K % 9 == 0:
        return k.K // 9, 0
    ktail = k.K - 9 * k.N
    if ktail <= 0 or ktail % 64 != 0 or k.N % 64 != 0 or k.stride != 1 or k.upsample:
        raise ValueError(f"3x3 key with K = {k.K}: neither 9 * cin nor 9 * N + a 64-multiple shortcut (N = {k.N})")
    return k.N, ktail


def _in_hw(k: Key, Ho: int, Wo: int):
    """Input size of an output grid Ho x Wo, or None when no input gives it."""
    if k.upsample:
        return (Ho // 2, Wo // 2) if Ho % 2 == 0 and Wo % 2 == 0 else None
    if k.stride == 2:
        return 2 * Ho, 2 * Wo
    return Ho, Wo


def _levels(k: Key, cin: int):
    unet = k.N % 160 == 0 or cin % 160 == 0 or k.N == 4 or cin == 8
    return (UNET_LEVELS + VAE_LEVELS + FACE_LEVELS) if unet else (VAE_LEVELS + UNET_LEVELS + FACE_LEVELS)


def halo_scope_desc(k: Key, g: ConvGeo):
    """A host-side descriptor of the launch, for ops.conv_halo_eligible (the scope of tile 14)."""
    from adaface_dev_amd._lib import GemmDesc
    d = GemmDesc()
    d.taps, d.M, d.N, d.K, d.kpad = 9, g.B * g.Ho * g.Wo, k.N, k.K, (k.K + 63) // 64 * 64
    d.c1, d.c2 = (g.cin - g.c2, g.c2) if not g.ktail else (g.cin, 0)
    if g.ktail:
        d.c3, d.c4 = g.ktail - g.c2, g.c2
        d.lda3, d.lda4 = d.c3, d.c4
    d.B, d.H, d.W, d.Ho, d.Wo = g.B, g.H, g.W, g.Ho, g.Wo
    d.stride, d.upsample, d.tap_shift = g.stride, g.upsample, g.tap_shift
    d.act, d.out_mode, d.splits = k.act, k.out_mode, 1
    return d


def conv_geometries(k: Key) -> List[ConvGeo]:
    """Geometry (a) (+ (b) where one exists, + the stride-2 tap_shift form, + a two-source split where cin / the shortcut is a U-Net concat)."""
    from adaface_dev_amd import ops
    cin, ktail = conv_channels(k)
    geos = []
    for L in _levels(k, cin):
        hw = _in_hw(k, L, L)
        if hw is not None and k.M % (L * L) == 0:
            geos.append(ConvGeo(k.M // (L * L), hw[0], hw[1], L, L, cin, ktail, k.stride, k.upsample, label=f"a:{k.M // (L * L)}x{L}x{L}"))
            break
    if not geos:
        raise ValueError(f"3x3 key M = {k.M}: no square image at a project level")
    a = geos[0]
    for Wo in (48, 24, 40, 12, 20, 6, 128, 4, 2):
        found = None
        for Ho in (k.M // Wo, 4, 6, 12, 2, 3):
            if Ho <= 0 or k.M % (Ho * Wo) != 0 or (Ho, Wo) == (a.Ho, a.Wo):
                continue
            hw = _in_hw(k, Ho, Wo)
            if hw is None:
                continue
            g = ConvGeo(k.M // (Ho * Wo), hw[0], hw[1], Ho, Wo, cin, ktail, k.stride, k.upsample, label=f"b:{k.M // (Ho * Wo)}x{Ho}x{Wo}")
            if not ops.conv_halo_eligible(halo_scope_desc(k, g)):
                found = g
                break
        if found is not None:
            geos.append(found)
            break
    if k.stride == 2:
        geos.append(ConvGeo(a.B, a.H, a.W, a.Ho, a.Wo, cin, ktail, 2, 0, tap_shift=1, label=a.label + ":tap_shift"))
    if ktail and ktail in SKIP_CONCAT:
        geos.append(ConvGeo(a.B, a.H, a.W, a.Ho, a.Wo, cin, ktail, 1, 0, c2=ktail - SKIP_CONCAT[ktail], label=a.label + ":skip2"))
    elif not ktail and cin in SKIP_CONCAT:
        geos.append(ConvGeo(a.B, a.H, a.W, a.Ho, a.Wo, cin, 0, k.stride, k.upsample, c2=cin - SKIP_CONCAT[cin], label=a.label + ":x2"))
    return geos


def split_tokens(k: Key):
    """(rows_per_batch, split_col) of a split-transposed (out_mode 1) key: a context k | v projection (K = 768) or a q | k | v projection."""
    if k.K == 768:
        cands, split = CROSS_ATTN_TOKENS, k.N // 2
    else:
        if k.N % 3:
            raise ValueError(f"split-transposed key N = {k.N}: not q | k | v")
        cands, split = SELF_ATTN_TOKENS, 2 * k.N // 3
    for t in cands:
        if k.M % t == 0:
            if split % 16:
                break
            return t, split
    raise ValueError(f"split-transposed key M = {k.M}, N = {k.N}: no production token count divides M")


def gemm_two_source_split(k: Key) -> Optional[int]:
    """K1 of a two-source (a2=) run where K splits into two 64-multiples (never with the folded LayerNorm: it takes one source)."""
    if k.ln or k.K % 64 or k.K < 128:
        return None
    return (k.K // 2) // 64 * 64


def with_extras(key: str) -> bool:
    """Bias + residual (+ row bias) on every other key, chosen by a hash of the key (stable across runs and hosts)."""
    return zlib.crc32(key.encode()) % 2 == 1


def validate(key: str):
    """Everything the sweep builds for one key; raises ValueError when the key has a form it cannot build."""
    k = parse_key(key)
    if k.taps == 9:
        return k, conv_geometries(k)
    if k.act == AF_ACT_GEGLU and (k.N % 32 or k.out_mode != AF_OUT_NORMAL):
        raise ValueError(f"GEGLU key {key!r}: N must be a multiple of 32 and the output plain")
    if k.out_mode == AF_OUT_F32 and (k.act != AF_ACT_NONE or k.ln or k.N % 4):
        raise ValueError(f"fp32-output key {key!r}: no activation / LayerNorm, N % 4 == 0")
    if k.out_mode == AF_OUT_SPLIT_T:
        split_tokens(k)
    return k, []
