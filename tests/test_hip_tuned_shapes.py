"""Every shape of the tuned tile table, dispatched as production dispatches it, against a plain fp32 CPU reference; and the 32-bit address
limits of the LDS-DMA kernels (2^24 pixels, 2^32 bytes) crossed on purpose.  `pytest -m gpu`.

The kernel tests (test_hip_kernels.py) pin each tile at hand-picked shapes with the tile forced.  Production reaches the kernels through
ops._launch_gemm: table lookup, split-K workspace clamp, the library's own fallbacks for geometries outside a tile's scope (the table's key
carries no image geometry).  Here every key runs with tile = 0, splits = 0 on operands rebuilt from the key (tests/tuned_shapes.py), at the
project geometry that produced it and at one the halo-resident kernel does not take.

Reference: sampled output rows with all their columns -- every row of the first and last 256, the first and last row of every 128-row
block (at most 4096 rows; a seeded subset of blocks beyond that), 512 seeded random rows -- computed on the CPU in fp32 from the same
fp16 operands (3x3 patches are gathered on the device by plain indexing, a copy, and reassembled on the host: a multi-GB input is never
copied whole).  Each sampled row and the whole sample must be within the bound of the per-form kernel test: TOL = 2e-3 for fp16 outputs
(one fp16 rounding, folded LayerNorm included), 1e-5 against an fp64 reference for fp32 outputs.  The whole output must be finite: the
suite's poison fixture fills every torch.empty with NaN, so an unwritten tile shows up.
"""
import json
import os
import random
import zlib

import pytest
import torch
import torch.nn.functional as F

import tuned_shapes as TS

pytestmark = pytest.mark.gpu

TOL = 2e-3                # fp16 outputs (test_hip_kernels.TOL; test_gemm_folded_layernorm* use the same)
TOL_F32 = 1e-5            # fp32 outputs vs fp64 (test_gemm_fp32_output_and_wgrad_past_the_fp16_range)
GN_MAX_ELEMS = 64 << 20   # GroupNorm-from-the-producer check up to ~64 M output elements

with open(TS.TABLE) as _f:
    KEYS = list(json.load(_f))

_RAN = set()              # keys whose test body ran to its checks (pass or fail): compared with the table by the last test
_WORST = {}               # (form, tile) -> worst per-row rel-L2, printed by the last test


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(shape, dev, seed, scale=1.0):
    """fp16 N(0, scale^2) generated on the device (multi-GB operands never cross the bus)."""
    x = torch.randn(shape, generator=_gen(dev, seed), device=dev, dtype=torch.float16)
    return x.mul_(scale) if scale != 1.0 else x


def _cpu_randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16)


def sample_rows(M: int, seed: int) -> torch.Tensor:
    rows = set(range(min(256, M))) | set(range(max(0, M - 256), M))
    nblk = (M + 127) // 128
    rnd = random.Random(seed)
    blocks = range(nblk) if 2 * nblk <= 4096 else rnd.sample(range(nblk), 2048)
    for b in blocks:
        rows.add(b * 128)
        rows.add(min(M, b * 128 + 128) - 1)
    rows.update(rnd.sample(range(M), min(512, M)))
    return torch.tensor(sorted(rows), dtype=torch.long)


def check_rows(got: torch.Tensor, ref: torch.Tensor, tol: float, what: str, form: str, tile=None):
    """got / ref: [R, N] (CPU).  Each row's rel-L2 and the whole sample's within tol."""
    got, ref = got.double(), ref.double()
    err = (got - ref).norm(dim=1)
    den = ref.norm(dim=1).clamp_min(1e-30)
    per_row = err / den
    worst = float(per_row.max())
    whole = float(err.norm() / ref.norm().clamp_min(1e-30))
    k = (form, tile)
    _WORST[k] = max(_WORST.get(k, 0.0), worst)
    i = int(per_row.argmax())
    assert worst < tol, f"{what}: worst sampled row (#{i} of the sample) rel-L2 {worst:.3e} >= {tol:g}"
    assert whole < tol, f"{what}: sample rel-L2 {whole:.3e} >= {tol:g}"


def _route(key):
    from adaface_dev_amd import ops
    return ops.tune_table().get(key, (0, 1))


# ----------------------------------------------------------------------------------------------------------------------------- 1x1 GEMMs
def _act_ref(h, act):
    if act == TS.AF_ACT_SILU:
        return F.silu(h)
    if act == TS.AF_ACT_QUICKGELU:
        return h * torch.sigmoid(1.702 * h)
    if act == TS.AF_ACT_GEGLU:
        x, g = h.chunk(2, dim=-1)
        return x * F.gelu(g)
    return h


def _run_gemm_key(dev, key, k, k1):
    """One launch of the key's GEMM through the production dispatch (+ its check).  k1: K of the first source of a two-source run."""
    from adaface_dev_amd import ops
    seed = 1000 + zlib.crc32(key.encode()) % 100000
    M, N, K = k.M, k.N, k.K
    extras = TS.with_extras(key)
    f32 = k.out_mode == TS.AF_OUT_F32
    if k.ln:       # rows whose mean is far from zero (3 sigma) with an outlier channel: the residual stream a LayerNorm sees
        a = _randn((M, K), dev, seed, 2.0).add_(3.0)
        a[:, 5] *= 8.0
        gam = torch.randn(K, generator=torch.Generator().manual_seed(3)) * 0.2 + 1
        bet = torch.randn(K, generator=torch.Generator().manual_seed(4)) * 0.2
    else:
        a = _randn((M, K), dev, seed, 0.5 if f32 else 1.0)
    w = _cpu_randn((N, K), seed + 1, K ** -0.5)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)) * 0.3
    if k.act == TS.AF_ACT_GEGLU:
        wi, bi = ops.interleave_geglu(w.float(), bias)
        wpk, bpk = wi, bi
    else:
        wpk, bpk = w, bias
    use_bias = extras or k.act == TS.AF_ACT_GEGLU or k.ln
    if k.ln:
        pw = ops.pack_matrix_ln(wpk, bpk if use_bias else None, gam, bet, 1e-5, dev)
    else:
        pw = ops.pack_matrix(wpk, bpk if use_bias else None, dev)
    rows = sample_rows(M, seed)
    kw = {}
    rpb, rowbias, residual = 0, None, None
    n_out = N // 2 if k.act == TS.AF_ACT_GEGLU else N
    if k.out_mode == TS.AF_OUT_SPLIT_T:
        rpb, split = TS.split_tokens(k)
        kw.update(rows_per_batch=rpb, split_col=split)
    elif extras and k.act != TS.AF_ACT_GEGLU and not f32:
        residual = _randn((M, n_out), dev, seed + 3)
        kw["residual"] = residual
    if extras and k.act != TS.AF_ACT_GEGLU and not f32:
        if not rpb:
            rpb = next((t for t in TS.ROWBIAS_TOKENS if M % t == 0 and M > t), 0)
        if rpb:
            rowbias = _randn((M // rpb, N), dev, seed + 4, 0.5)
            kw.update(rowbias=rowbias, rows_per_batch=rpb)
    if k1 is None:
        out = ops.gemm(a, pw, act=k.act, out_f32=f32, **kw)
    else:
        a1, a2 = a[:, :k1].contiguous(), a[:, k1:].contiguous()
        out = ops.gemm(a1, pw, a2=a2, act=k.act, out_f32=f32, **kw)
        del a1, a2
    out2 = None
    if k.out_mode == TS.AF_OUT_SPLIT_T:
        out, out2 = out
    tag = f"{key} {'a2 K1=' + str(k1) if k1 else 'one source'} extras={extras}"
    assert torch.isfinite(out).all(), f"{tag}: non-finite output (an unwritten tile?)"
    if out2 is not None:
        assert torch.isfinite(out2).all(), f"{tag}: non-finite V^T output"
    # reference on the sampled rows
    ar = a[rows.to(dev)].cpu()
    dt = torch.float64 if f32 else torch.float32
    x = ar.to(dt)
    if k.ln:
        x = F.layer_norm(x, (K,), gam.to(dt), bet.to(dt), 1e-5)
    h = x @ w.to(dt).t()
    if use_bias:
        h = h + bias.to(dt)
    if rowbias is not None:
        h = h + rowbias.cpu().to(dt)[rows // rpb]
    h = _act_ref(h, k.act)
    if residual is not None:
        h = h + residual[rows.to(dev)].cpu().to(dt)
    form = f"1x1 act{k.act} out{k.out_mode}{' ln' if k.ln else ''}"
    tile = _route(key)[0]
    if out2 is None:
        check_rows(out[rows.to(dev)].cpu(), h, TOL_F32 if f32 else TOL, tag, form, tile)
    else:
        split = kw["split_col"]
        check_rows(out[rows.to(dev)].cpu(), h[:, :split], TOL, tag + " [q | k columns]", form, tile)
        vt = out2.permute(0, 2, 1)[(rows // rpb).to(dev), (rows % rpb).to(dev)]         # V^T [batch, channel, token] back to token rows
        check_rows(vt.cpu(), h[:, split:], TOL, tag + " [V^T columns]", form, tile)
        ld2 = out2.shape[2]
        if ld2 > rpb:
            assert (out2[:, :, rpb:] == 0).all(), f"{tag}: the row pad of V^T must be zero"


# ----------------------------------------------------------------------------------------------------------------------------- 3x3 convs
def gather_patches(xs, g: TS.ConvGeo, rows: torch.Tensor, dev) -> torch.Tensor:
    """[R, 9 * cin] fp32 CPU: the nine input pixels of each sampled output pixel (tap order (ky, kx), channels of all sources), zero
    outside the image.  The device only indexes (a copy); the masking happens on the host."""
    m = rows.to(dev)
    HoWo = g.Ho * g.Wo
    b, r = m // HoWo, m % HoWo
    oy, ox = (r // g.Wo)[:, None, None], (r % g.Wo)[:, None, None]
    ky = torch.arange(3, device=dev).view(1, 3, 1)
    kx = torch.arange(3, device=dev).view(1, 1, 3)
    if g.upsample == 1:                            # nearest x2: taps walk the 2H x 2W grid
        uy, ux = oy + ky - 1, ox + kx - 1
        valid = (uy >= 0) & (uy < 2 * g.H) & (ux >= 0) & (ux < 2 * g.W)
        iy, ix = uy.clamp(min=0) // 2, ux.clamp(min=0) // 2
    elif g.upsample == 2:                          # zero-inserted image of Ho x Wo: only even positions hold pixels
        uy, ux = oy + ky - 1, ox + kx - 1
        valid = (uy >= 0) & (uy < g.Ho) & (ux >= 0) & (ux < g.Wo) & (uy % 2 == 0) & (ux % 2 == 0)
        iy, ix = uy.clamp(min=0) // 2, ux.clamp(min=0) // 2
    elif g.tap_shift:                              # padding (0, 1, 0, 1)
        iy, ix = oy * g.stride + ky, ox * g.stride + kx
        valid = (iy < g.H) & (ix < g.W)
    else:
        iy, ix = oy * g.stride + ky - 1, ox * g.stride + kx - 1
        valid = (iy >= 0) & (iy < g.H) & (ix >= 0) & (ix < g.W)
    iy, ix = iy.clamp(0, g.H - 1), ix.clamp(0, g.W - 1)
    pix = ((b[:, None, None] * g.H + iy) * g.W + ix).reshape(-1)
    parts = [x.view(-1, x.shape[-1])[pix].cpu().float().view(len(rows), 9, x.shape[-1]) for x in xs]
    p = torch.cat(parts, dim=2) if len(parts) > 1 else parts[0]
    p = p * valid.reshape(len(rows), 9, 1).cpu().float()
    return p.reshape(len(rows), -1)


def _conv_expected_tile(k: TS.Key, key: str, g: TS.ConvGeo):
    """(tile, splits) conv3x3 will hand to the library at this geometry (tile 0 = its heuristic)."""
    from adaface_dev_amd import ops
    d = TS.halo_scope_desc(k, g)
    if g.ktail:
        tile, splits = ops.conv3x3_skip_tile(k.M, k.N, g.cin, g.ktail)
        if tile == 14 and not ops.conv_halo_eligible(d):
            tile, splits = (7 if (k.N % 320 == 0 and k.M >= 8192) else (11 if k.N % 160 == 0 else 8)), 1
        return tile, splits, d
    tile, splits = _route(key)
    return tile, splits, d


def _run_conv_key(dev, key, k, g: TS.ConvGeo, gn: bool):
    from adaface_dev_amd import _lib, ops
    seed = 2000 + zlib.crc32((key + g.label).encode()) % 100000
    extras = TS.with_extras(key)
    N, cin, ktail = k.N, g.cin, g.ktail
    c1 = cin - g.c2 if not ktail else cin
    w = _cpu_randn((N, k.K), seed + 1, k.K ** -0.5)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)) * 0.3
    w3 = w[:, :9 * cin].reshape(N, 3, 3, cin).permute(0, 3, 1, 2)
    if ktail:
        pw = ops.pack_conv3x3_skip(w3, bias if extras else None, w[:, 9 * cin:].reshape(N, ktail, 1, 1), None, dev)
    else:
        pw = ops.pack_conv3x3(w3, bias if extras else None, dev)
    xs = [_randn((g.B, g.H, g.W, c1), dev, seed + 3)]
    if g.c2 and not ktail:
        xs.append(_randn((g.B, g.H, g.W, g.c2), dev, seed + 4))
    skips = []
    if ktail:
        s1 = ktail - g.c2
        skips = [_randn((g.B, g.Ho, g.Wo, s1), dev, seed + 5)]
        if g.c2:
            skips.append(_randn((g.B, g.Ho, g.Wo, g.c2), dev, seed + 6))
    rowbias = _randn((g.B, N), dev, seed + 7, 0.5) if extras else None
    residual = _randn((g.B, g.Ho, g.Wo, N), dev, seed + 8) if extras else None
    kw = dict(x2=xs[1] if len(xs) > 1 else None, stride=g.stride, upsample=g.upsample, tap_shift=g.tap_shift, rowbias=rowbias, residual=residual)
    if g.upsample == 2:
        kw["upsample"], kw["out_hw"] = 2, (g.Ho, g.Wo)
    if ktail:
        kw["skip"] = (skips[0], skips[1] if len(skips) > 1 else None)
    out = ops.conv3x3(xs[0], pw, **kw)
    tag = f"{key} geometry {g.label} (B={g.B} {g.H}x{g.W} -> {g.Ho}x{g.Wo}, c1={c1} c2={g.c2}{' ktail=' + str(ktail) if ktail else ''}) extras={extras}"
    assert out.shape == (g.B, g.Ho, g.Wo, N)
    assert torch.isfinite(out).all(), f"{tag}: non-finite output (an unwritten tile?)"
    rows = sample_rows(k.M, seed)
    p = gather_patches(xs, g, rows, dev)
    if ktail:
        m = rows.to(dev)
        p = torch.cat([p] + [s.view(-1, s.shape[-1])[m].cpu().float() for s in skips], dim=1)
    ref = p @ w.float().t()
    if extras:
        ref = ref + bias + rowbias.cpu().float()[rows // (g.Ho * g.Wo)] + residual.view(-1, N)[rows.to(dev)].cpu().float()
    tile, splits, d = _conv_expected_tile(k, key, g)
    form = f"3x3 s{g.stride} up{g.upsample}{' tail' if ktail else ''}{' halo' if tile == 14 and ops.conv_halo_eligible(d) else ''}"
    check_rows(out.view(-1, N)[rows.to(dev)].cpu(), ref, TOL, tag, form, tile)
    if not gn:
        return
    # GroupNorm statistics from the producing launch, as the ResBlocks ask for them
    cpg = N // 32
    y = ops.conv3x3(xs[0], pw, gn_cpg=cpg, **kw)
    assert torch.isfinite(y).all(), f"{tag} gn_cpg={cpg}: non-finite output"
    check_rows(y.view(-1, N)[rows.to(dev)].cpu(), ref, TOL, tag + f" gn_cpg={cpg}", form + " gn", tile)
    want_stats = (tile not in (14, 19) or ops.conv_halo_eligible(d)) and _lib.lib().af_gemm_gn_stats_ok(tile, splits, 9, k.act, k.out_mode, N, cpg, g.Ho * g.Wo) == 1
    assert (ops.partials_of(y) is not None) == want_stats, f"{tag}: producer statistics {'missing' if want_stats else 'unexpected'}"
    gam = (torch.randn(N, generator=torch.Generator().manual_seed(seed + 9)) * 0.3 + 1).to(dev)
    bet = (torch.randn(N, generator=torch.Generator().manual_seed(seed + 10)) * 0.3).to(dev)
    for silu in (False, True):
        yn = ops.groupnorm(y, gam, bet, 1e-5, silu)
        refn = F.group_norm(y.float().permute(0, 3, 1, 2), 32, gam, bet, 1e-5)
        refn = F.silu(refn) if silu else refn
        num = (yn.float().permute(0, 3, 1, 2) - refn).double().norm()
        e = float(num / refn.double().norm())
        assert e < TOL, f"{tag}: GroupNorm(silu={silu}) of the producer's output rel-L2 {e:.3e}"


def _gn_eligible(k: TS.Key, key: str, g: TS.ConvGeo) -> bool:
    from adaface_dev_amd import _lib
    tile, splits, _ = _conv_expected_tile(k, key, g)
    return (k.N % 32 == 0 and k.M * k.N <= GN_MAX_ELEMS and g.Ho * g.Wo % 128 == 0
            and _lib.lib().af_gemm_gn_stats_ok(tile, splits, 9, k.act, k.out_mode, k.N, k.N // 32, g.Ho * g.Wo) == 1)


# ----------------------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("key", KEYS)
def test_tuned_shape(dev, key):
    """One table key: all its runs through ops.gemm / ops.conv3x3 with tile = 0, splits = 0."""
    k, geos = TS.validate(key)           # a key the builders cannot parse fails here
    _RAN.add(key)
    if k.taps == 1:
        _run_gemm_key(dev, key, k, None)
        k1 = TS.gemm_two_source_split(k)
        if k1 is not None:
            _run_gemm_key(dev, key, k, k1)
    else:
        for i, g in enumerate(geos):
            _run_conv_key(dev, key, k, g, gn=(i == 0 and _gn_eligible(k, key, g)))


# ----------------------------------------------------------------------------------------------------------------------------- untabled shapes
# both sides of each heuristic boundary of ops._launch_gemm / ops.conv3x3_skip_tile; (name, key fields, geometry)
UNTABLED_CONVS = [
    # VAE_HALO_DEFAULT: M >= 16384 and N % 160 != 0 and tile-14 geometry -> tile 14, else the library's heuristic
    ("vae_halo_M16384", 1, 16384, 128, 128, 0, 1, 256, 64),
    ("vae_halo_M16128", 1, 16128, 128, 128, 0, 1, 252, 64),
    ("vae_halo_N256", 1, 16384, 256, 128, 0, 1, 128, 128),
    ("vae_halo_N320", 1, 16384, 320, 128, 0, 1, 128, 128),
    ("vae_halo_ragged_Ho8_Wo128", 16, 16384, 128, 128, 0, 1, 8, 128),
    ("vae_halo_patches_Wo96", 2, 18432, 128, 256, 0, 1, 96, 96),
    # K tail on shapes the table does not name: the whole-line default; and a tabled tile-14 key at a geometry tile 14 does not take
    ("tail_untabled_24x40", 2, 1920, 320, 320, 640, 1, 24, 40),
    ("tail_tile14_key_Wo128", 1, 16384, 320, 320, 640, 1, 128, 128),
    ("tail_tile14_key_Wo48", 2, 1536, 1280, 1280, 2560, 1, 16, 48),
]


@pytest.mark.parametrize("name,B,M,N,cin,ktail,stride,Ho,Wo", UNTABLED_CONVS, ids=[c[0] for c in UNTABLED_CONVS])
def test_untabled_conv_routing(dev, name, B, M, N, cin, ktail, stride, Ho, Wo):
    from adaface_dev_amd import ops
    assert B * Ho * Wo == M
    K = 9 * cin + ktail
    key = f"9,{M},{N},{K},0,0,{stride},0"
    k = TS.parse_key(key)
    if name.startswith("tail_tile14"):
        assert ops.conv3x3_skip_tile(M, N, cin, ktail)[0] == 14, f"{key}: expected a tabled tile-14 entry"
    else:
        assert key not in ops.tune_table(), f"{key} is in the table: pick another untabled shape"
    g = TS.ConvGeo(B, Ho, Wo, Ho, Wo, cin, ktail, stride, 0, label=name)
    if name == "vae_halo_M16384":
        assert ops.conv_halo_eligible(TS.halo_scope_desc(k, g))
    _run_conv_key(dev, key, k, g, gn=False)


UNTABLED_GEMMS = [
    # folded LayerNorm on an untabled shape: tile 7 (N % 320 == 0, M >= 8192) / tile 8; GEGLU: tile 7 (N % 256 == 0) / tile 8
    ("ln_tile7", "1,8320,320,320,0,0,0,0,ln"),
    ("ln_tile8", "1,8064,320,320,0,0,0,0,ln"),
    ("ln_geglu_tile7", "1,520,2560,320,2,0,0,0,ln"),
    ("ln_geglu_tile8", "1,520,640,320,2,0,0,0,ln"),
    ("ln_plain_entry_tile2", "1,1024,640,320,0,0,0,0,ln"),        # the plain key's entry (tile 2) is outside the folded form's scope
]


@pytest.mark.parametrize("name,key", UNTABLED_GEMMS, ids=[c[0] for c in UNTABLED_GEMMS])
def test_untabled_gemm_routing(dev, name, key):
    from adaface_dev_amd import ops
    assert key not in ops.tune_table(), f"{key} is in the table: pick another untabled shape"
    plain = ops.tune_table().get(key[:-3])
    assert (plain is not None and plain[0] < 7) if name == "ln_plain_entry_tile2" else plain is None
    _run_gemm_key(dev, key, TS.parse_key(key), None)


# ----------------------------------------------------------------------------------------------------------------------------- address-width edges
def _need(dev, nbytes):
    free = torch.cuda.mem_get_info(dev)[0]
    if free < nbytes:
        pytest.skip(f"needs {nbytes / 2**30:.1f} GiB free device memory, {free / 2**30:.1f} GiB free")


def _conv_tiles(pw_desc):
    """Every tile af_gemm takes this descriptor on (tools/autotune_gemm.py::candidate_ok, splits 1)."""
    import tools.autotune_gemm as AT
    from adaface_dev_amd import _lib, ops
    return [t for t in range(1, 18) if AT.candidate_ok(pw_desc, t, 1, _lib, ops)]


def _edge_rows(M, limits, seed):
    rows = set(sample_rows(M, seed).tolist())
    for lim in limits:
        rows.update(range(max(0, lim - 384), min(M, lim + 384)))
    return torch.tensor(sorted(rows), dtype=torch.long)


def _conv_edge(dev, g: TS.ConvGeo, N, limit_rows, seed):
    from adaface_dev_amd import ops
    k = TS.Key(9, g.B * g.Ho * g.Wo, N, 9 * g.cin + g.ktail, 0, 0, g.stride, 0, False)
    w = _cpu_randn((N, k.K), seed + 1, k.K ** -0.5)
    w3 = w[:, :9 * g.cin].reshape(N, 3, 3, g.cin).permute(0, 3, 1, 2)
    pw = ops.pack_conv3x3_skip(w3, None, w[:, 9 * g.cin:].reshape(N, g.ktail, 1, 1), None, dev) if g.ktail else ops.pack_conv3x3(w3, None, dev)
    x = _randn((g.B, g.H, g.W, g.cin), dev, seed + 3)
    s = _randn((g.B, g.Ho, g.Wo, g.ktail), dev, seed + 5) if g.ktail else None
    rows = _edge_rows(k.M, limit_rows, seed)
    p = gather_patches([x], g, rows, dev)
    if g.ktail:
        p = torch.cat([p, s.view(-1, g.ktail)[rows.to(dev)].cpu().float()], dim=1)
    ref = p @ w.float().t()
    del p
    tiles = [0] + _conv_tiles(TS.halo_scope_desc(k, g))
    for tile in tiles:
        out = ops.conv3x3(x, pw, stride=g.stride, skip=(s, None) if g.ktail else None, tile=tile, splits=1 if tile else 0)
        what = f"3x3 B={g.B} {g.H}x{g.W} -> {g.Ho}x{g.Wo} {g.cin}{'+' + str(g.ktail) if g.ktail else ''} -> {N} stride {g.stride}, tile {tile or 'default'}"
        assert torch.isfinite(out).all(), f"{what}: non-finite output"
        for lim in limit_rows:                    # both sides of the limit on their own (a wrap past it must not hide in the rest of the sample)
            side = (rows >= lim - 384) & (rows < lim + 384)
            sel = rows[side]
            check_rows(out.view(-1, N)[sel.to(dev)].cpu(), ref[side], TOL, what + f" rows {lim - 384} .. {lim + 383}", "edge 3x3", tile)
        check_rows(out.view(-1, N)[rows.to(dev)].cpu(), ref, TOL, what, "edge 3x3", tile)
        del out
    return tiles


def test_conv3x3_input_above_4GiB_vae_512_level(dev):
    """A 3x3 convolution of the VAE's 512-level kind (256 -> 128 channels) at batch 33: a 4.4 GB input.  The untabled shape's default
    (VAE_HALO_DEFAULT) and every forced tile must leave the 32-bit-offset kernels for one with 64-bit addressing; rows whose input pixels lie
    on both sides of byte 2^32 are checked."""
    g = TS.ConvGeo(33, 512, 512, 512, 512, 256, 0, 1, 0)
    _need(dev, (2 * 33 * 512 * 512 * (256 + 128) + (4 << 30)))
    px = (1 << 32) // (256 * 2)                   # first input pixel at or past byte 2^32
    _conv_edge(dev, g, 128, [px], seed=71)


def test_conv3x3_stride2_input_above_4GiB_output_below(dev):
    """Stride 2 over the same 4.4 GB input: M * cin * 2 (what the whole-line kernel's guard sizes) stays below 2^32, so the whole-line tiles
    take it and rely on their 64-bit per-pixel pointers for the 3x3 taps.  Output rows of images 31 and 32 read input pixels on both sides
    of byte 2^32."""
    g = TS.ConvGeo(33, 512, 512, 256, 256, 256, 0, 2, 0)
    _need(dev, (2 * 33 * 512 * 512 * 256 + 2 * 33 * 256 * 256 * 128 + (4 << 30)))
    assert 33 * 512 * 512 * 256 * 2 >= 1 << 32 and 33 * 256 * 256 * 256 * 2 < 1 << 32
    _conv_edge(dev, g, 128, [32 * 256 * 256], seed=72)


def test_conv3x3_k_tail_past_2_24_pixels(dev):
    """The halo-resident kernel's K-tail form multiplies pixel indices with __umul24.  64 -> 160 channels with a 64-channel shortcut on
    4112 images of 64 x 64 (B*H*W just above 2^24): the default dispatch and every tile that takes the descriptor, rows on both sides of
    pixel 2^24.  conv3h_variant / ops.conv_halo_eligible keep the tail form below 2^24 pixels."""
    from adaface_dev_amd import ops
    g = TS.ConvGeo(4112, 64, 64, 64, 64, 64, 64, 1, 0)
    _need(dev, 4112 * 4096 * (64 + 64 + 2 * 160) * 2 + (4 << 30))
    k = TS.Key(9, 4112 * 4096, 160, 640, 0, 0, 1, 0, False)
    _conv_edge(dev, g, 160, [1 << 24], seed=73)
    assert not ops.conv_halo_eligible(TS.halo_scope_desc(k, g))


def test_gemm_weight_above_4GiB(dev):
    """A packed weight (B operand) of 4.3 GB: M = 256, N = 65536 + 256, K = 32768.  Columns n >= 65536 start at byte n * kpad * 2 >= 2^32:
    the default dispatch and every tile that takes the descriptor, columns on both sides of the limit."""
    import tools.autotune_gemm as AT
    from adaface_dev_amd import _lib, ops
    M, N, K = 256, 65536 + 256, 32768
    _need(dev, N * K * 2 + (6 << 30))
    w = _randn((N, K), dev, 81)
    pw = ops.pack_matrix(w, None, dev)           # already in the packed layout: aliased, no 4.3 GB copy
    assert pw.aliased
    a = _randn((M, K), dev, 82, K ** -0.5)
    cols = sorted(set(range(0, 256)) | set(range(65536 - 256, N)) | set(random.Random(83).sample(range(N), 512)))
    cols_t = torch.tensor(cols, dtype=torch.long)
    ref = a.cpu().float() @ w[cols_t.to(dev)].cpu().float().t()
    d = _lib.GemmDesc()
    d.taps, d.M, d.N, d.K, d.kpad, d.c1, d.act, d.out_mode = 1, M, N, K, pw.kpad, K, 0, 0
    tiles = [0] + [t for t in range(1, 18) if AT.candidate_ok(d, t, 1, _lib, ops)]
    hi = cols_t >= 65536
    for tile in tiles:
        out = ops.gemm(a, pw, tile=tile, splits=1 if tile else 0)
        what = f"gemm M={M} N={N} K={K}, tile {tile or 'default'}"
        assert torch.isfinite(out).all(), f"{what}: non-finite output"
        got = out[:, cols_t.to(dev)].cpu()
        check_rows(got[:, ~hi].t(), ref[:, ~hi].t(), TOL, what + " columns < 65536 (per column)", "edge gemm", tile)
        check_rows(got[:, hi].t(), ref[:, hi].t(), TOL, what + " columns >= 65536 (per column)", "edge gemm", tile)
        check_rows(got, ref, TOL, what, "edge gemm", tile)
        del out


# ----------------------------------------------------------------------------------------------------------------------------- coverage
def test_every_table_key_ran(dev):
    """No silent skips: every key of the table ran through test_tuned_shape in this session."""
    from adaface_dev_amd import ops
    table = set(ops.tune_table())
    assert set(KEYS) == table
    missing = table - _RAN
    print(f"\ntuned shapes: {len(_RAN)} of {len(table)} keys ran; worst per-row rel-L2 per (form, tile):")
    for (form, tile), e in sorted(_WORST.items(), key=lambda kv: (kv[0][0], -1 if kv[0][1] is None else kv[0][1])):
        print(f"  {form:28s} tile {tile}: {e:.2e}")
    if os.environ.get("AF_TUNED_SHAPES_REPORT"):
        with open(os.environ["AF_TUNED_SHAPES_REPORT"], "w") as f:
            json.dump({"keys_ran": len(_RAN), "keys": len(table), "worst_row_rel_l2": {f"{fm} | tile {t}": e for (fm, t), e in sorted(_WORST.items(), key=str)}}, f, indent=1)
    assert not missing, f"{len(missing)} table keys did not run, e.g. {sorted(missing)[:5]}"
