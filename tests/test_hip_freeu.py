"""af_freeu_stats / af_freeu_apply on a real MI355X (`pytest -m gpu`), through ``ops.freeu`` and the C ABI, against the fp64 restatement of
tests/freeu_util.py.

The bound.  Every output must satisfy  |got - ref64| <= 2^-11 |ref64| + E32:  2^-11 |ref| is the one rounding to fp16 (all values here are
normal fp16 numbers) and E32 bounds what the fp32 path adds, with u = 2^-24.  b and s reach the kernels as fp32, so the reference is computed
with the fp32-rounded b and s.

* skip.  The kernels sum d = x - p0 (p0: the plane's first pixel; exact or rounded once, covered below) against cos / sin tables.  Let
  D = sum_pixels |x - p0| per plane.  A table value is sincospif's (<= 2 ulp of a number <= 1) or, for the diagonal bin, two products and a
  difference of such values: absolute error <= 2^-19.  Each of the seven sums is a sum of HW products in some order (rows first, then a tree):
  |error| <= ((HW + 8) u + 2^-19) D =: es D  (any-order summation (HW - 1) u sum|terms|, <= 8 further roundings per term for d, the products and
  the per-run fold, and the table error times sum |d|).  low = S0 + sum of six (sum x table value) products, |S_k| <= D: the second use of the
  tables adds 6 x 2^-19 D and the <= 16 operations on partial results of size <= 7 D add 128 u D.  So
      E_low = D (7 es + 6 x 2^-19 + 128 u),
  and  y = x + (s - 1) p0 + ((s - 1) / HW) low  in five more operations on numbers of size <= M = |x| + |s - 1| (|p0| + 7 D / HW):
      E32_skip = |s - 1| / HW * E_low + 8 u M.
* h, version 2.  m[p] is an fp32 sum of C values in some order, times 1 / C:  |dm| <= (C + 1) u mean_c |h[p, c]| =: em[p], Em = max_p em[p].
  With R = hi - lo (fp64):  mhat = (m - lo) / R has |d mhat| <= (2 Em + 2 mhat Em) / R (1 + o(Em / R)) + 3 u <= 4.04 Em / R + 4 u  once
  Em / R < 1e-3, which the test asserts of its data (the outlier pixel's mean is 20 away).  A sample whose pixel means are all equal in fp64
  must give hi == lo on the device too: its values are multiples of 2^-5 in [32, 64), so every fp32 sum of up to 2048 of them is exact in
  any order (22 bits), and d mhat = 0.  Then  h' = h ((b - 1) mhat + 1):
      E32_h = |h| (|b - 1| d mhat + 4 u max(1, b));      version 1:  E32_h = 4 u b |h|.
The same test shows on the CPU that the bound can fail: the restatement with the diagonal bin (-1, -1) replaced by (-1, +1), and the
restatement with one bin dropped, both miss it by more than 10 x on this data.  The diagonal swap is asserted where it is a different bin:
H >= 3 and W >= 3 (at a side of 1 there is no diagonal bin, at a side of 2 the bins -1 and +1 coincide).

Measured on an MI355X (profiles/freeu.txt): worst |got - ref64| / bound 0.978 over the eight cases (the fp16 rounding term: the fp64 reference
rounded to fp16 sits at the same 0.978 there); the wrong restatements miss the bound by 198 x to 29561 x."""
import functools

import numpy as np
import pytest
import torch

from freeu_util import freeu_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

#        H   W   C     Cs    B  b    s    version
CASES = [(1, 1, 1280, 1280, 2, 1.5, 0.9, 2),        # one bin, hi == lo
         (2, 1, 256, 256, 2, 1.6, 0.2, 2),          # two bins, Nyquist == -1
         (3, 5, 128, 64, 2, 1.2, 0.9, 1),           # odd, non-square, version 1
         (8, 8, 1280, 1280, 2, 1.5, 0.9, 2),
         (16, 24, 640, 320, 2, 1.6, 0.2, 2),        # C != Cs, a partial run of pixels is absent but two slices are present
         (5, 3, 16, 24, 2, 1.3, 2.5, 2),            # channel tails: 3 groups of 8 channels, runs of 3 pixels
         (8, 8, 1280, 1280, 2, 1.4, 0.0, 1),
         (64, 64, 640, 320, 1, 1.6, 0.2, 2)]        # 8 slices of the skip, 16 workgroups of pixel means per sample: the partials are combined
IDS = [f"{c[0]}x{c[1]}-C{c[2]}-Cs{c[3]}-B{c[4]}-b{c[5]}-s{c[6]}-v{c[7]}" for c in CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def f32(v):
    return float(np.float32(v))


def make_inputs(H, W, C, Cs, B, seed):
    """h and skip, fp16 NHWC: a large offset plus a small variation (mean 40, sigma 1, clipped to [33, 63] so that all values share the fp16
    exponent of 32 .. 64); sample 0 of h has one outlier pixel (all channels + 20: its mean sets hi); sample 1 of h has a pixel-constant channel
    mean (every pixel a permutation of one vector); every sample of skip has one outlier pixel (+ 3000 in all channels) and random planes."""
    g = np.random.default_rng(seed)
    h = np.clip(40.0 + g.standard_normal((B, H, W, C)), 33.0, 63.0)
    if H * W > 1:
        h[0, H // 3, W // 2, :] = np.clip(h[0, H // 3, W // 2, :] + 20.0, 33.0, 63.0)
    if B > 1:
        v = h[1, 0, 0, :].astype(np.float16).astype(np.float64)
        for p in range(H * W):
            h[1, p // W, p % W, :] = g.permutation(v)
    skip = np.clip(40.0 + g.standard_normal((B, H, W, Cs)), 33.0, 63.0)
    if H * W > 1:
        for b in range(B):
            skip[b, (H // 2 + b) % H, W // 3, :] += 3000.0
    return torch.from_numpy(h.astype(np.float16)), torch.from_numpy(skip.astype(np.float16))


def bounds(h16, skip16, b, s, version):
    """(E32_h, E32_skip) per element, as derived in the module docstring, each times (1 + 2^-11) for the rounding of the error itself."""
    h = h16.numpy().astype(np.float64)
    x = skip16.numpy().astype(np.float64)
    B, H, W, C = h.shape
    HW = H * W
    if version == 1:
        eh = 4 * U * b * np.abs(h)
    else:
        m = h.mean(axis=3, keepdims=True)
        em = (C + 1) * U * np.abs(h).mean(axis=3, keepdims=True)
        Em = em.max(axis=(1, 2), keepdims=True)
        R = m.max(axis=(1, 2), keepdims=True) - m.min(axis=(1, 2), keepdims=True)
        exact = bool(np.all(h * 32 == np.round(h * 32)) and h.min() >= 32 and h.max() < 64 and C <= 2048)
        assert np.all((R > 0) | exact), "a constant-mean sample whose fp32 sums are not exact"
        assert np.all((R == 0) | (Em < 1e-3 * np.where(R == 0, 1.0, R))), "ill-conditioned data: the spread of the pixel means is within their error"
        dmh = np.where(R == 0, 0.0, 4.04 * Em / np.where(R == 0, 1.0, R) + 4 * U)
        eh = np.abs(h) * (abs(b - 1) * dmh + 4 * U * max(1.0, b))
    p0 = x[:, :1, :1, :]
    D = np.abs(x - p0).sum(axis=(1, 2), keepdims=True)
    es = (HW + 8) * U + 2.0 ** -19
    e_low = D * (7 * es + 6 * 2.0 ** -19 + 128 * U)
    M = np.abs(x) + abs(s - 1) * (np.abs(p0) + 7 * D / HW)
    ek = abs(s - 1) / HW * e_low + 8 * U * M
    k = 1 + 2.0 ** -11
    return eh * k, ek * k


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs, the fp64 reference and the bounds of CASES[i], computed once and shared (never written to)."""
    H, W, C, Cs, B, b, s, version = CASES[i]
    b, s = f32(b), f32(s)
    h16, skip16 = make_inputs(H, W, C, Cs, B, 1000 + i)
    rh, rk = freeu_ref(h16, skip16, b, s, version)
    eh, ek = bounds(h16, skip16, b, s, version)
    return dict(h=h16, skip=skip16, b=b, s=s, version=version, ref_h=rh, ref_skip=rk, tol_h=2.0 ** -11 * np.abs(rh) + eh, tol_skip=2.0 ** -11 * np.abs(rk) + ek)


def run(dev, h16, skip16, b, s, version, **kw):
    from adaface_dev_amd import ops
    oh, ok = ops.freeu(h16.to(dev), skip16.to(dev), b, s, version, **kw)
    torch.cuda.synchronize()
    return oh.cpu(), ok.cpu()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_freeu_within_the_fp32_bound_of_fp64(dev, i):
    c = case(i)
    H, W, C = CASES[i][:3]
    # the bound can fail: two wrong restatements miss it by more than 10 x (CPU only)
    wrong = {}
    if H >= 3 and W >= 3:
        wrong["diagonal bin (-1, +1)"] = freeu_ref(c["h"], c["skip"], c["b"], c["s"], c["version"], diag_v=+1)[1]
    drop = (-1, 0) if H > 1 else ((0, -1) if W > 1 else (0, 0))
    wrong[f"bin {drop} dropped"] = freeu_ref(c["h"], c["skip"], c["b"], c["s"], c["version"], drop=drop)[1]
    for name, bad in wrong.items():
        r = float((np.abs(bad - c["ref_skip"]) / c["tol_skip"]).max())
        print(f"freeu {IDS[i]}: {name}: worst |wrong - ref| / bound = {r:.1f}")
        assert r >= 10, (name, r)
    oh, ok = run(dev, c["h"], c["skip"], c["b"], c["s"], c["version"])
    rh = float((np.abs(oh.numpy().astype(np.float64) - c["ref_h"]) / c["tol_h"]).max())
    rk = float((np.abs(ok.numpy().astype(np.float64) - c["ref_skip"]) / c["tol_skip"]).max())
    print(f"freeu {IDS[i]}: worst |got - ref64| / bound: h {rh:.3f}, skip {rk:.3f}")
    assert torch.equal(oh[..., C // 2:], c["h"][..., C // 2:])                    # the upper half of h is untouched
    assert rh <= 1 and rk <= 1, (rh, rk)
    # the outputs differ from the inputs by far more than the bound: the test sees the effect
    assert float((np.abs(c["ref_skip"] - c["skip"].numpy()) / c["tol_skip"]).max()) > 10
    if H * W > 1:                                                               # (at 1 x 1 the pixel mean is constant: h stays)
        assert float((np.abs(c["ref_h"] - c["h"].numpy()) / c["tol_h"]).max()) > 10


@pytest.mark.parametrize("i", [3, 5, 7], ids=[IDS[3], IDS[5], IDS[7]])
def test_deterministic_and_in_place_equals_out_of_place(dev, i):
    c = case(i)
    a = run(dev, c["h"], c["skip"], c["b"], c["s"], c["version"])
    b = run(dev, c["h"], c["skip"], c["b"], c["s"], c["version"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    from adaface_dev_amd import ops
    hd, kd = c["h"].to(dev), c["skip"].to(dev)
    for t in (hd, kd):                                                             # statistics a producer might have left: stale after the rewrite,
        ops.GnPartials(None, 1, 1, 1, 1, 1).attach(t)                              # which torch's version counter does not see
        assert ops.partials_of(t) is not None
    oh, ok = ops.freeu(hd, kd, c["b"], c["s"], c["version"], out_h=hd, out_skip=kd)
    torch.cuda.synchronize()
    assert oh is hd and ok is kd
    assert torch.equal(hd.cpu(), a[0]) and torch.equal(kd.cpu(), a[1])
    assert ops.partials_of(hd) is None and ops.partials_of(kd) is None           # the consuming GroupNorm computes its own statistics


def test_saturation(dev):
    """h near 60000 with b = 1.5 gives exactly 65504, not inf: version 1 everywhere, version 2 at the pixel whose mean is the sample's maximum."""
    h = torch.full((1, 1, 2, 16), 60000.0, dtype=torch.float16)
    h[0, 0, 1, :] = 100.0
    skip = torch.ones((1, 1, 2, 8), dtype=torch.float16)
    for version in (1, 2):
        oh, _ = run(dev, h, skip, 1.5, 1.0, version)
        assert torch.all(oh[0, 0, 0, :8] == 65504.0) and torch.all(oh[0, 0, 0, 8:] == 60000.0)
        assert torch.all(oh[0, 0, 1, :8] == (150.0 if version == 1 else 100.0))
    # -60000 saturates at -65504; the skip saturates too: a constant plane of 60000 with s = 2 doubles its mean
    oh, ok = run(dev, -h, torch.full((1, 1, 2, 8), 60000.0, dtype=torch.float16), 1.5, 2.0, 1)
    assert torch.all(oh[0, 0, 0, :8] == -65504.0) and torch.all(ok == 65504.0)


def test_nan_stays_in_its_sample_and_plane(dev):
    c = case(4)
    clean_h, clean_k = run(dev, c["h"], c["skip"], c["b"], c["s"], c["version"])
    C = c["h"].shape[3]
    h = c["h"].clone()
    h[0, 3, 5, 7] = float("nan")
    oh, ok = run(dev, h, c["skip"], c["b"], c["s"], c["version"])
    assert torch.equal(oh[1], clean_h[1]) and torch.equal(ok, clean_k)            # sample 1 and the skip: bit-identical
    assert bool(torch.isnan(oh[0, ..., :C // 2]).all())                          # a NaN pixel mean makes lo / hi NaN: the sample's boosted half is NaN
    skip = c["skip"].clone()
    skip[0, 2, 3, 9] = float("nan")
    oh, ok = run(dev, c["h"], skip, c["b"], c["s"], c["version"])
    assert torch.equal(ok[1], clean_k[1]) and torch.equal(oh, clean_h)
    assert bool(torch.isnan(ok[0, :, :, 9]).all())                               # the plane is NaN everywhere, as its DFT is
    others = [j for j in range(skip.shape[3]) if j != 9]
    assert torch.equal(ok[0][..., others], clean_k[0][..., others])              # the other planes of sample 0: bit-identical


def test_identity(dev, monkeypatch):
    from adaface_dev_amd import ops
    c = case(2)
    hd, kd = c["h"].to(dev), c["skip"].to(dev)
    kd[0, 1, 1, 3] = float("inf")
    # s == 1: the skip is handed back as it is, inf and all, and h is boosted as without the inf
    oh, ok = ops.freeu(hd, kd, 1.5, 1.0, 2)
    torch.cuda.synchronize()
    assert ok is kd and oh is not hd
    ref_h, _ = run(dev, c["h"], c["skip"], 1.5, 1.0, 2)
    assert torch.equal(oh.cpu(), ref_h) and not torch.equal(oh, hd)
    out_k = torch.zeros_like(kd)
    ops.freeu(hd, kd, 1.5, 1.0, 2, out_skip=out_k)
    torch.cuda.synchronize()
    assert torch.equal(out_k.view(torch.int16), kd.view(torch.int16))
    # b == 1: h is handed back as it is
    k2 = c["skip"].to(dev)
    oh, ok = ops.freeu(hd, k2, 1.0, 0.5, 2)
    torch.cuda.synchronize()
    assert oh is hd and ok is not k2 and torch.equal(k2.cpu(), c["skip"]) and not torch.equal(ok.cpu(), c["skip"])
    # b == s == 1: no launch at all, the inputs are returned
    def no_launch(*a, **k):
        raise AssertionError("a launch with b == s == 1")
    monkeypatch.setattr(ops, "_launch", no_launch)
    oh, ok = ops.freeu(hd, kd, 1.0, 1.0, 2)
    assert oh is hd and ok is kd


def test_capture_replay_equals_eager(dev):
    """The pair captured in one graph on one stream, replayed on changed inputs, equals the eager result bit for bit (no host synchronisation,
    the workspace from the graph's pool)."""
    from adaface_dev_amd import ops
    c0, c1 = case(3), case(6)                                   # the same shape, different data
    hd, kd = c0["h"].to(dev), c0["skip"].to(dev)
    ops.freeu(hd, kd, c0["b"], c0["s"], 2)                      # warm-up: code objects, the eager scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        oh, ok = ops.freeu(hd, kd, c0["b"], c0["s"], 2)
    hd.copy_(c1["h"].to(dev))
    kd.copy_(c1["skip"].to(dev))
    g.replay()
    torch.cuda.synchronize()
    eh, ek = run(dev, c1["h"], c1["skip"], c0["b"], c0["s"], 2)
    assert torch.equal(oh.cpu(), eh) and torch.equal(ok.cpu(), ek)
    del g


def test_refusals_leave_outputs_and_workspace_untouched(dev):
    from adaface_dev_amd import _lib, ops
    L = _lib.lib()
    B, H, W, C, Cs = 2, 4, 4, 32, 16
    h = torch.full((B, H, W, C), 3.0, dtype=torch.float16, device=dev)
    skip = torch.full((B, H, W, Cs), 5.0, dtype=torch.float16, device=dev)
    n = ops.freeu_workspace_size(B, H, W, C, Cs)
    ws = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    oh, ok = torch.full_like(h, 9.0), torch.full_like(skip, 11.0)
    good = dict(h=h.data_ptr(), skip=skip.data_ptr(), ws=ws.data_ptr(), ws_floats=n, h_out=oh.data_ptr(), skip_out=ok.data_ptr(), B=B, H=H, W=W, C=C, Cs=Cs,
                b=1.5, s=0.5, version=2)
    bad = [dict(h=None), dict(skip=None), dict(ws=None), dict(h_out=None), dict(skip_out=None), dict(ws_floats=n - 1), dict(ws_floats=0),
           dict(B=0), dict(B=65536), dict(H=0), dict(H=129), dict(W=0), dict(W=129), dict(C=24), dict(C=8), dict(C=0), dict(C=16400), dict(Cs=12),
           dict(Cs=0), dict(Cs=16392), dict(b=-0.5), dict(b=float("nan")), dict(b=float("inf")), dict(s=-1.0), dict(s=float("nan")),
           dict(s=float("inf")), dict(version=0), dict(version=3), dict(h=h.data_ptr() + 2), dict(B=65535, H=128, W=128, C=16384, Cs=16384)]
    for change in bad:
        a = dict(good, **change)
        if "h_out" not in change and "skip_out" not in change:
            rc = L.af_freeu_stats(a["h"], a["skip"], a["ws"], a["ws_floats"], a["B"], a["H"], a["W"], a["C"], a["Cs"], a["b"], a["s"], a["version"], None)
            assert rc == _lib.AF_E_BADARG, ("stats", change, rc)
        rc = L.af_freeu_apply(a["h"], a["skip"], a["ws"], a["ws_floats"], a["h_out"], a["skip_out"], a["B"], a["H"], a["W"], a["C"], a["Cs"], a["b"],
                              a["s"], a["version"], None)
        assert rc == _lib.AF_E_BADARG, ("apply", change, rc)
        assert L.af_last_error().decode().startswith("af_freeu_")
    assert L.af_freeu_ws_floats(B, H, W, 24, Cs) == _lib.AF_E_BADARG
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()) and bool((oh == 9.0).all()) and bool((ok == 11.0).all()) and bool((h == 3.0).all()) and bool((skip == 5.0).all())
    # b == s == 1 through the C ABI: accepted, nothing launched, nothing written
    assert L.af_freeu_stats(good["h"], good["skip"], good["ws"], n, B, H, W, C, Cs, 1.0, 1.0, 2, None) == 0
    assert L.af_freeu_apply(good["h"], good["skip"], good["ws"], n, good["h_out"], good["skip_out"], B, H, W, C, Cs, 1.0, 1.0, 2, None) == 0
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()) and bool((oh == 9.0).all()) and bool((ok == 11.0).all())
    # ops refuses what the library refuses, before anything is written
    for kw in (dict(b=-1.0), dict(s=float("nan")), dict(version=3)):
        a = dict(dict(b=1.5, s=0.5, version=2), **kw)
        with pytest.raises(RuntimeError, match="af_freeu_stats"):
            ops.freeu(h, skip, a["b"], a["s"], a["version"], out_h=oh, out_skip=ok)
    torch.cuda.synchronize()
    assert bool((oh == 9.0).all()) and bool((ok == 11.0).all())
