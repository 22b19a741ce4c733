"""The trainable path's autograd nodes on a real MI355X, node by node, against fp64 on the CPU.  `pytest -m gpu`.

Every reference is plain torch in fp64 on the CPU on the numbers the device sees: activations are fp16 tensors, parameters fp32
masters holding fp16-representable values (so the weight pack's rounding is not part of the error).  A backward is isolated from its
forward's output rounding by a LINEAR loss `(y.float() * G).sum()` with G fp16-representable: the incoming gradient is exactly G.
Where the backward depends on a saved forward output (the softmax probabilities of the explicit attention) the reference is autograd
of the fp64 restatement.  Every compared tensor is checked twice: rel-L2 and max|got - ref| / max|ref| (a wrong tail row does not show
in the rel-L2 of a large tensor).

DERIVED bounds
  F16_L2 = 6e-4, F16_MAX = 2^-10    a result that is ONE fp16 rounding of an fp32 value: per element at most 2^-11 |value|, so the
                                    rel-L2 is at most 4.9e-4 and the largest error at most 2^-11 max|ref|; the rest is room for the fp32
                                    evaluation underneath.
  f32_bound(K, extra)               an fp32 result differs from fp64 by its accumulation: (sqrt(K) + extra) 2^-24 with K the reduction
                                    length and `extra` the fp32 roundings of ONE term's own evaluation (stated at each use).  The same
                                    number bounds both figures.
MEASURED bounds (worst value over the cases of the test on MI355X, times two, rounded up to one digit; never looser than 5e-3 for a
result that has passed through an fp16 rounding of an intermediate, 1e-4 for a pure fp32 one).  The kernels are deterministic, the factor
covers other seeds.
  PROB_*     softmax probabilities (fp32 through __expf)                         test_explicit_attention_chain
  QUANT_*    matmul_nt gradients against the UNQUANTISED dC (the node rounds dC to fp16 once)   test_matmul_nt
  LAYER_*    one encoder layer, forward rounding compounds over nine fp16 tensors   test_encoder_layer
The measured worst values stand next to each bound below."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

F16_L2 = 6e-4
F16_MAX = 2.0 ** -10
F32_EPS = 2.0 ** -24
# measured on MI355X (worst over the cases) -> twice that, rounded up to one digit
PROB_L2, PROB_MAX = 7e-7, 2e-6          # 3.08e-7 at (1, 20, 1, 168, 33); 6.31e-7 at (1, 63, 1, 32, 101)
QUANT_L2, QUANT_MAX = 5e-4, 7e-4        # 2.11e-4 at (257, 320, 256) dBt x1e-12; 3.48e-4 at (30, 16, 12) dA x1e+12
LAYER_L2, LAYER_MAX = 3e-3, 3e-3        # 1.00e-3 d(q_proj.weight), m = 1; 1.10e-3 d(k_proj.weight), m = 1


def f32_bound(K, extra=1):
    return (math.sqrt(K) + extra) * F32_EPS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    """fp16 values (CPU) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16)


def cmp(tag, got, ref, l2_tol, max_tol, dtype=None):
    """Both figures of `got` (device or host tensor) against the fp64 `ref`; prints them, then asserts.  Returns (rel-L2, max / max)."""
    assert got is not None, (tag, "no tensor came back")
    if dtype is not None:
        assert got.dtype == dtype, (tag, got.dtype, dtype)
    g = got.detach().double().cpu()
    r = ref.detach().double()
    assert g.shape == r.shape, (tag, tuple(g.shape), tuple(r.shape))
    assert bool(torch.isfinite(g).all()), (tag, "not every element was written / finite")
    e2 = rel_l2(g.numpy(), r.numpy())
    em = float((g - r).abs().max() / r.abs().max().clamp_min(1e-300))
    print(f"ERR {tag}: rel-L2 {e2:.3e} (< {l2_tol:.1e})  max/max {em:.3e} (< {max_tol:.1e})")
    assert e2 < l2_tol and em < max_tol, (tag, e2, l2_tol, em, max_tol)
    return e2, em


@contextlib.contextmanager
def launches():
    """Names of the library launches made inside the block (a device path that quietly became torch makes none)."""
    from adaface_dev_amd import ops
    names, orig = [], ops._launch

    def spy(name, *a, **k):
        names.append(k.get("what") or name)
        return orig(name, *a, **k)

    ops._launch = spy
    try:
        yield names
    finally:
        ops._launch = orig


def master(t16, dev, grad=True):
    """An fp32 master parameter on the device holding the fp16-representable values of `t16`."""
    return torch.nn.Parameter(t16.float().to(dev), requires_grad=grad)


# ============================================================================================================ 1. LinearFn
LINEAR_CASES = [(77, 64, 192), (130, 72, 40), (1, 64, 64), (300, 768, 64)]
# requires_grad on (x, w, b, res)
LINEAR_MODES = {"all": (True, True, True, True), "w_only": (False, True, False, False), "x_res": (True, False, False, True)}


@functools.lru_cache(maxsize=None)
def linear_problem(M, K, N):
    """Operands and the fp64 results with a bias and a residual, shared by every variant of the case (dx, dW, db do not depend on
    whether a bias or a residual is present)."""
    x, w, b = rnd((M, K), 1), rnd((N, K), 2, K ** -0.5), rnd((N,), 3, 0.5)
    res, G = rnd((M, N), 4), rnd((M, N), 5)
    xd, wd, Gd = x.double(), w.double(), G.double()
    y0 = xd @ wd.t()
    return dict(x=x, w=w, b=b, res=res, G=G, y0=y0, dx=Gd @ wd, dw=Gd.t() @ xd, db=Gd.sum(0))


@pytest.mark.parametrize("M,K,N", LINEAR_CASES)
def test_linear_fn(dev, M, K, N):
    """autograd_ops.linear on diffusionmodules.util.Linear: y = x W^T (+ b) (+ res); dx = G W, dW = G^T x (fp32), db = column sums of G
    (fp32), d(res) = G bit for bit -- with / without bias, with / without residual, and with requires_grad on everything, on w alone, on
    x and res alone (a gradient that was not asked for is None; one that was asked for is there).  (130, 72, 40): M no 64-multiple and K
    no 128-multiple, both transposes of `wgrad` zero-fill their pads under the NaN-filled torch.empty of conftest.
    Bounds derived: y, dx one fp16 rounding; dW, db fp32 sums over the M tokens of exact products: f32_bound(M, 1) (the result's rounding).
    Worst on MI355X: y 2.25e-4 / 4.23e-4 (rel-L2 / max), dx 2.11e-4 / 3.63e-4 of 6e-4 / 9.8e-4; dW 6.4e-8 of 5.8e-7 at M = 77, max 2.1e-7 of
    1.1e-6 at M = 300; db 1.4e-8 / 3.8e-8 of 5.8e-7."""
    from adaface_dev_amd import autograd_ops as ag
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import Linear
    P = linear_problem(M, K, N)
    G16 = P["G"].to(dev)
    for has_bias in (True, False):
        for has_res in (True, False):
            for mode, (gx, gw, gb, gr) in LINEAR_MODES.items():
                tag = f"linear {M, K, N} bias={int(has_bias)} res={int(has_res)} {mode}"
                lin = Linear(K, N, bias=has_bias)
                lin.weight = master(P["w"], dev, gw)
                if has_bias:
                    lin.bias = master(P["b"], dev, gb)
                x = P["x"].to(dev).requires_grad_(gx)
                res = P["res"].to(dev).requires_grad_(gr) if has_res else None
                with launches() as names:
                    y = ag.linear(lin, x, residual=res)
                assert set(names) == {"af_gemm"}, (tag, names)
                y_ref = P["y0"] + (P["b"].double() if has_bias else 0) + (P["res"].double() if has_res else 0)
                cmp(f"{tag} y", y, y_ref, F16_L2, F16_MAX, torch.float16)
                raw = y.grad_fn.apply(G16)                         # what the node hands back, None included
                assert len(raw) == 5 and raw[4] is None, tag
                dx, dw, db, dres = raw[:4]
                if gx:
                    cmp(f"{tag} dx", dx, P["dx"], F16_L2, F16_MAX, torch.float16)
                else:
                    assert dx is None, tag
                if gw:
                    cmp(f"{tag} dW", dw, P["dw"], f32_bound(M), f32_bound(M), torch.float32)
                else:
                    assert dw is None, tag
                if gb and has_bias:
                    cmp(f"{tag} db", db, P["db"], f32_bound(M), f32_bound(M), torch.float32)
                else:
                    assert db is None, tag
                if gr and has_res:
                    assert dres is not None, (tag, "the residual gradient was dropped")
                    assert dres.dtype == torch.float16 and torch.equal(dres, G16), (tag, "d(res) is not G bit for bit")
                else:
                    assert dres is None, tag
                # the same through the engine: leaves receive what the node returned
                (y.float() * G16.float()).sum().backward()
                for name, leaf, want in (("x", x, dx), ("w", lin.weight, dw), ("b", lin.bias, db), ("res", res, dres)):
                    if leaf is None:
                        continue
                    if want is None:
                        assert leaf.grad is None, (tag, name)
                    else:
                        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, want), (tag, name)


# ========================================================================================================= 2. QKVLinearFn
QKV_SCALES = (1.0, 3.0, 0.2)              # the three column blocks of G: a mixed-up slice is off by a factor, not by noise


@functools.lru_cache(maxsize=None)
def qkv_problem(M, E):
    x = rnd((M, E), 11)
    ws = [rnd((E, E), 12 + i, E ** -0.5) for i in range(3)]
    bs = [rnd((E,), 15 + i, 0.5) for i in range(3)]
    G = torch.cat([rnd((M, E), 18 + i, s) for i, s in enumerate(QKV_SCALES)], 1)
    xd, Gd = x.double(), G.double()
    wcat = torch.cat([w.double() for w in ws], 0)
    y = xd @ wcat.t() + torch.cat([b.double() for b in bs])
    dws = [Gd[:, i * E:(i + 1) * E].t() @ xd for i in range(3)]
    dbs = [Gd[:, i * E:(i + 1) * E].sum(0) for i in range(3)]
    return dict(x=x, ws=ws, bs=bs, G=G, y=y, dx=Gd @ wcat, dws=dws, dbs=dbs)


def _mkv(E, heads, multiplier=1):
    from adaface_dev_amd.adaface.arc2face_models import CLIPAttentionMKV, clip_text_config
    return CLIPAttentionMKV(clip_text_config(hidden_size=E, num_attention_heads=heads, num_hidden_layers=1, intermediate_size=2 * E),
                            multiplier=multiplier)


@pytest.mark.parametrize("M,E", [(154, 80), (77, 64)])
def test_qkv_linear_fn(dev, M, E):
    """QKVLinearFn on the packs of a multiplier-1 CLIPAttentionMKV: qkv [M, 3E] = x [Wq; Wk; Wv]^T + [bq; bk; bv]; the incoming gradient
    has column blocks of scale 1 / 3 / 0.2, so each of the SIX parameter gradients is compared with its own fp64 value and a swapped
    slice is off by a factor 3 .. 15.  Second run: only wk and bv ask for a gradient.
    Bounds derived: qkv, dx one fp16 rounding; dW*, db* fp32 sums over M tokens: f32_bound(M, 1).
    Worst on MI355X: qkv 2.09e-4 / 3.67e-4, dx 2.12e-4 / 3.23e-4; the six parameter gradients 8.6e-8 / 2.1e-7 of 8.0e-7 (M = 154)."""
    from adaface_dev_amd import autograd_ops as ag
    P = qkv_problem(M, E)
    G16 = P["G"].to(dev)
    names6 = ("wq", "wk", "wv", "bq", "bk", "bv")
    for mode in ("all", "wk_bv"):
        want = {n: (mode == "all" or n in ("wk", "bv")) for n in names6}
        attn = _mkv(E, 2)
        for proj, w, b, nw, nb in zip((attn.q_proj, attn.k_proj, attn.v_proj), P["ws"], P["bs"], names6[:3], names6[3:]):
            proj.weight, proj.bias = master(w, dev, want[nw]), master(b, dev, want[nb])
        x = P["x"].to(dev).requires_grad_(mode == "all")
        tag = f"qkv {M, E} {mode}"
        with launches() as names:
            qkv = ag.QKVLinearFn.apply(x, *attn._qkv_params(), attn)
        assert set(names) == {"af_gemm"}, (tag, names)
        cmp(f"{tag} qkv", qkv, P["y"], F16_L2, F16_MAX, torch.float16)
        raw = qkv.grad_fn.apply(G16)
        assert len(raw) == 8 and raw[7] is None, tag
        if mode == "all":
            cmp(f"{tag} dx", raw[0], P["dx"], F16_L2, F16_MAX, torch.float16)
        else:
            assert raw[0] is None, tag
        got = dict(zip(names6, raw[1:7]))
        refs = dict(zip(names6, P["dws"] + P["dbs"]))
        for n in names6:
            if want[n]:
                cmp(f"{tag} d{n}", got[n], refs[n], f32_bound(M), f32_bound(M), torch.float32)
            else:
                assert got[n] is None, (tag, n)
        if mode == "all":
            for a, b in (("bq", "bk"), ("bq", "bv"), ("bk", "bv"), ("wq", "wk"), ("wq", "wv"), ("wk", "wv")):
                assert not torch.equal(got[a], got[b]), (tag, a, b, "two projections received the same gradient")
        (qkv.float() * G16.float()).sum().backward()
        for n, p in zip(names6, attn._qkv_params()):
            if want[n]:
                assert p.grad is not None and p.grad.dtype == p.dtype and torch.equal(p.grad, got[n]), (tag, n)
            else:
                assert p.grad is None, (tag, n)


# ========================================================================================================== 3. LayerNormFn
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_stream(C):
    """2049 rows of one generator stream at width C: the 2048-row problem is its first 2048 rows."""
    g = torch.Generator().manual_seed(100 + C)
    rows = 2049
    off = (2.0 + 2.0 * torch.rand((rows, 1), generator=g)) * (2.0 * (torch.rand((rows, 1), generator=g) > 0.5).float() - 1.0)
    x = torch.randn((rows, C), generator=g) + off                                            # row means 2 .. 4 sigma off zero, either sign
    dy = torch.randn((rows, C), generator=g)
    gamma = 1.0 + 0.2 * torch.randn((C,), generator=g)
    beta = 0.3 * torch.randn((C,), generator=g)
    return x.half(), dy.half(), gamma.half(), beta.half()


@functools.lru_cache(maxsize=None)
def ln_problem(rows, C):
    x, dy, gamma, beta = (t.clone() for t in ln_stream(C))
    x, dy = x[:rows].contiguous(), dy[:rows].contiguous()
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xd, (C,), gd, bd, LN_EPS)
    y.backward(dy.double())
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, y=y.detach(), dx=xd.grad, dg=gd.grad, db=bd.grad)


def ln_term_roundings(x):
    """fp32 roundings carried by ONE term dy * (x - mean) * rstd of dgamma, in units of 2^-24 of the term, worst case, from the data alone.
    A row's mean and variance are fp32 sums of C values of one sign (the mean is 2 .. 4 sigma off zero, squares are positive): a lane adds
    8 ceil(C / 512) values in sequence, six butterfly levels join the 64 lanes, so at most depth = 8 ceil(C / 512) + 6 roundings of a partial
    sum.  The mean's error reaches x_hat multiplied by |mean| / sigma, the variance's by 1/2; the subtraction, the reciprocal square root
    (1 ulp = 2 units) and the product add 4."""
    xd = x.double()
    C = xd.shape[1]
    depth = 8 * ((C + 511) // 512) + 6
    ratio = float((xd.mean(1).abs() / xd.std(1, unbiased=False).clamp_min(1e-6)).max())
    return (ratio + 0.5) * depth + 4


def _run_layernorm(dev, P, pdtype, tag, Pb=None):
    """Pb: the problem whose row count and data set the fp32 bounds (the 2049-row stream for both sides of the branch switch)."""
    Pb = P if Pb is None else Pb
    bound_rows = Pb["x"].shape[0]
    from adaface_dev_amd import autograd_ops as ag
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import LayerNorm
    C = P["x"].shape[1]
    ln = LayerNorm(C, eps=LN_EPS)
    ln.weight = torch.nn.Parameter(P["gamma"].to(device=dev, dtype=pdtype))
    ln.bias = torch.nn.Parameter(P["beta"].to(device=dev, dtype=pdtype))
    x = P["x"].to(dev).requires_grad_(True)
    with launches() as names:
        y = ag.layer_norm(ln, x)
        (y.float() * P["dy"].to(dev).float()).sum().backward()
    cmp(f"{tag} y", y, P["y"], F16_L2, F16_MAX, torch.float16)
    cmp(f"{tag} dx", x.grad, P["dx"], F16_L2, F16_MAX, torch.float16)
    if pdtype == torch.float32:
        tg, tb = (f32_bound(bound_rows, ln_term_roundings(Pb["x"])),) * 2, (f32_bound(bound_rows, 1),) * 2
    else:
        tg = tb = (F16_L2, F16_MAX)                               # fp16 parameters: the fp32 sums are rounded once to the parameter's dtype
    cmp(f"{tag} dgamma", ln.weight.grad, P["dg"], *tg, pdtype)
    cmp(f"{tag} dbeta", ln.bias.grad, P["db"], *tb, pdtype)
    return names


@pytest.mark.parametrize("rows,C", [(77, 768), (130, 1024), (5, 1536), (1, 8), (2048, 64), (2049, 64)])
def test_layer_norm_fn(dev, rows, C):
    """LayerNormFn against fp64 autograd of F.layer_norm: y, dx, dgamma, dbeta; row means offset by ~3 sigma, gamma 1 +- 0.2, beta != 0.
    C = 768 / 1024 are the CLIP towers' widths, 1536 the kernels' limit, (1, 8) the smallest problem; 2048 rows is the last size ONE call of the
    fused parameter-gradient kernel takes and 2049 the first that is split (2048 + 1 rows, fp32 sums added) -- the same generator stream, and
    BOTH are held to the bound of 2049 rows.  Until this test 2049 rows took a branch that rounded x_hat to fp16 before the column sum:
    dgamma rel-L2 2.70e-4, max 2.67e-4 against this bound of 8.0e-6 (2048 rows: 1.9e-7); LayerNormFn.backward now splits instead.  Parameter gradients come back in the parameter's dtype (fp32 masters here; fp16 parameters in test_layer_norm_fn_fp16_parameters).
    Bounds derived: y, dx one fp16 rounding; dgamma f32_bound(rows, ln_term_roundings), dbeta f32_bound(rows, 1) (see _run_layernorm).
    Worst on MI355X: y 2.25e-4 / 4.13e-4, dx 2.51e-4 / 3.35e-4; dgamma 1.9e-7 / 2.3e-7 of 6.8e-6 .. 8.0e-6 (2048 rows 1.90e-7, 2049 rows
    1.92e-7); dbeta 8.2e-8 / 1.2e-7 of 2.8e-6 (2049 rows)."""
    names = _run_layernorm(dev, ln_problem(rows, C), torch.float32, f"layernorm {rows, C}", ln_problem(2049, C) if rows >= 2048 else None)
    assert names.count("af_layernorm_param_grads") == (rows + 2047) // 2048, (names, "one fused parameter-gradient call per 2048 rows")


def test_layer_norm_fn_fp16_parameters(dev):
    """fp16 gamma / beta: the gradients come back as fp16 (one rounding of the fp32 sums)."""
    _run_layernorm(dev, ln_problem(77, 768), torch.float16, "layernorm fp16-params (77, 768)")


# ========================================================================================================== 4. QuickGeluFn
@pytest.mark.parametrize("n", [8, 100000])
def test_quick_gelu_fn(dev, n):
    """x * sigmoid(1.702 x) and its derivative at +-12 and +-60 (the sigmoid saturates both ways; exp(102) is past fp32's range) among
    values of a few units; one vector of eight, and 100 000 elements.  Everything finite.  Bounds derived: one fp16 rounding.
    Worst on MI355X: y 1.41e-4 / 3.2e-5, dx 2.00e-4 / 4.32e-4."""
    from adaface_dev_amd import autograd_ops as ag
    x = (torch.randn(n, generator=torch.Generator().manual_seed(7)) * 4).clamp(-12, 12)
    x[:8] = torch.tensor([-60.0, 60.0, -12.0, 12.0, 0.5, -0.5, 3.0, -3.0])
    x, G = x.half(), rnd((n,), 8)
    xr = x.double().requires_grad_(True)
    ref = xr * torch.sigmoid(1.702 * xr)
    ref.backward(G.double())
    xd = x.to(dev).requires_grad_(True)
    y = ag.QuickGeluFn.apply(xd)
    (y.float() * G.to(dev).float()).sum().backward()
    cmp(f"quickgelu {n} y", y, ref, F16_L2, F16_MAX, torch.float16)
    cmp(f"quickgelu {n} dx", xd.grad, xr.grad, F16_L2, F16_MAX, torch.float16)
    # the saturated ends, element by element: y(-60) = 0, y(60) = 60, dx(-60) = 0, dx(60) = G
    yh, gh = y.detach().cpu(), xd.grad.cpu()
    assert float(yh[0]) == 0.0 and float(yh[1]) == 60.0 and float(gh[0]) == 0.0 and float(gh[1]) == float(G[1])


# ===================================================================================== 5. MatmulNTFn / matmul_nt / low_rank_product
MATMUL_CASES = [(100, 64, 132), (64, 8, 4), (257, 320, 256), (30, 16, 12)]


def node_dc(G):
    """The dC MatmulNTFn.backward uses, restated: scaled by 2^floor(log2(256 / max|dC|)), rounded to fp16, unscaled (fp64 result)."""
    amax = G.abs().amax().float().clamp_min(1e-30)
    scale = torch.exp2(torch.floor(torch.log2(256.0 / amax)))
    return (G.float() * scale).to(torch.float16).double() / scale.double()


@pytest.mark.parametrize("M,K,N", MATMUL_CASES)
def test_matmul_nt(dev, M, K, N):
    """matmul_nt(a, bt) = a bt^T (fp32) and both gradients.  (100, 64, 132), (64, 8, 4) and (30, 16, 12) have N % 8 == 4: the forward takes
    them (N % 4 == 0) and the backward, whose A operand is dC [M, N], was refused by af_gemm (c1 % 8) until MatmulNTFn.backward padded dC to a
    multiple of 8 columns.  dC = standard normal times 1e-12, 1, 1e+12; all zero (exact zeros back, no NaN); one entry 1e6 times the rest.
    Derived: forward f32_bound(K, 1); gradients against fp64 on the dC THE NODE USES (node_dc: power-of-two scale, fp16, unscale):
    dA f32_bound(N, 1), dBt f32_bound(M, 1) -- the products of fp16 values are exact in fp32 and the scale is a power of two.
    Measured: gradients against the UNQUANTISED dC (one fp16 rounding of every dC entry, 2^-11 relative each): QUANT_L2 / QUANT_MAX; the
    outlier case's distance to the unquantised gradient is printed, not asserted (the small entries fall into fp16's subnormals by design).
    Worst on MI355X: c 3.5e-8 / 6.7e-8 of 2.3e-7 (K = 8); gradients on the node's dC 4.3e-8 / 7.4e-8 of 1.8e-7 (N = 4); against the unquantised
    dC 2.11e-4 / 3.48e-4 (-> QUANT_L2 5e-4, QUANT_MAX 7e-4); outlier: 6.4e-5 from the unquantised gradient at every shape."""
    from adaface_dev_amd import autograd_ops as ag
    a16, b16 = rnd((M, K), 21), rnd((N, K), 22)
    a, bt = a16.float().to(dev).requires_grad_(True), b16.float().to(dev).requires_grad_(True)
    ad, bd = a16.double(), b16.double()
    tag = f"matmul_nt {M, K, N}"
    with launches() as names:
        c = ag.matmul_nt(a, bt)
    assert "af_gemm" in names, (tag, "the device path was not taken", names)
    cmp(f"{tag} c", c, ad @ bd.t(), f32_bound(K), f32_bound(K), torch.float32)
    G0 = torch.randn((M, N), generator=torch.Generator().manual_seed(23))
    for mag in (1e-12, 1.0, 1e12):
        G = (G0 * mag).float()
        da, dbt = torch.autograd.grad(c, (a, bt), G.to(dev), retain_graph=True)
        Gq = node_dc(G)
        cmp(f"{tag} x{mag:g} dA (node's dC)", da, Gq @ bd, f32_bound(N), f32_bound(N), torch.float32)
        cmp(f"{tag} x{mag:g} dBt (node's dC)", dbt, Gq.t() @ ad, f32_bound(M), f32_bound(M), torch.float32)
        cmp(f"{tag} x{mag:g} dA QUANT", da, G.double() @ bd, QUANT_L2, QUANT_MAX)
        cmp(f"{tag} x{mag:g} dBt QUANT", dbt, G.double().t() @ ad, QUANT_L2, QUANT_MAX)
    da, dbt = torch.autograd.grad(c, (a, bt), torch.zeros((M, N), device=dev), retain_graph=True)
    assert da.dtype == torch.float32 and dbt.dtype == torch.float32
    assert bool((da == 0).all()) and bool((dbt == 0).all()), (tag, "an all-zero dC must give exact zeros")
    G = G0.clone().float()
    G[M // 2, N // 3] = 1e6
    da, dbt = torch.autograd.grad(c, (a, bt), G.to(dev), retain_graph=True)
    Gq = node_dc(G)
    cmp(f"{tag} outlier dA (node's dC)", da, Gq @ bd, f32_bound(N), f32_bound(N), torch.float32)
    cmp(f"{tag} outlier dBt (node's dC)", dbt, Gq.t() @ ad, f32_bound(M), f32_bound(M), torch.float32)
    print(f"INFO {tag} outlier, distance to the unquantised gradient: dA {rel_l2(da.double().cpu().numpy(), (G.double() @ bd).numpy()):.3e} "
          f"dBt {rel_l2(dbt.double().cpu().numpy(), (G.double().t() @ ad).numpy()):.3e}")
    # one gradient alone
    a2 = a16.float().to(dev).requires_grad_(True)
    c2 = ag.matmul_nt(a2, b16.float().to(dev))
    da2, = torch.autograd.grad(c2, (a2,), G0.to(dev))
    cmp(f"{tag} dA alone", da2, node_dc(G0) @ bd, f32_bound(N), f32_bound(N), torch.float32)


def test_low_rank_product(dev):
    """low_rank_product(b, a) = b a in fp32: (Cout, r, Cin) = (64, 8, 72) on the device kernel; r = 4 and Cin = 70 are outside the kernel's
    sizes (K % 8, N % 4) and must be plain torch, with no library launch.  Derived: f32_bound(r, 1).  Worst on MI355X: 4.7e-8 / 1.2e-7 of 2.3e-7."""
    from adaface_dev_amd import autograd_ops as ag
    for cout, r, cin, device_path in ((64, 8, 72, True), (64, 4, 72, False), (64, 8, 70, False)):
        b16, a16 = rnd((cout, r), 31), rnd((r, cin), 32)
        b, a = b16.float().to(dev), a16.float().to(dev)
        with launches() as names:
            out = ag.low_rank_product(b, a)
        tag = f"low_rank_product {cout, r, cin}"
        assert ("af_gemm" in names) == device_path and (device_path or names == []), (tag, names)
        assert tuple(out.shape) == (cout, cin) and not out.requires_grad
        cmp(tag, out, b16.double() @ a16.double(), f32_bound(r), f32_bound(r), torch.float32)
        if not device_path:
            assert torch.equal(out, b @ a), tag


# ================================================================================ 6. explicit attention as a chain of the two nodes
CHAIN_CASES = [(1, 5, 2, 8, 16), (1, 5, 2, 8, 17), (2, 65, 2, 24, 80), (2, 65, 2, 24, 81), (1, 63, 1, 32, 100), (1, 63, 1, 32, 101),
               (1, 17, 2, 48, 112), (1, 17, 2, 48, 113), (1, 1, 1, 56, 128), (1, 33, 1, 64, 33), (1, 33, 1, 88, 33), (1, 20, 1, 168, 33)]
PAD = 8          # q / k / v are columns PAD .. PAD + C of buffers 2 PAD wider than C (leading dimension > C, 16-byte aligned rows)


@functools.lru_cache(maxsize=None)
def chain_problem(B, N, heads, d, L, masked):
    """Operands, the fixed rewrite and loss weights, and the fp64 restatement with its autograd for the three loss variants
    ('both': Ws, Wp, Wo;  'no_p': Wp = 0;  'no_o': Wo = 0)."""
    C = heads * d
    g = torch.Generator().manual_seed(1000 * L + d)
    bufs = {n: rnd((B * rows, C + 2 * PAD), 40 + i) for i, (n, rows) in enumerate((("q", N), ("k", L), ("v", L)))}
    mult = 1.0 + 0.1 * torch.randn((B, heads, N, L), generator=g)
    bias = torch.zeros((1, 1, 1, L))
    if masked:
        bias[..., 1::3] = -math.inf                               # a fixed third of the keys, never all of them
    Ws, Wp = torch.randn((B, heads, N, L), generator=g), torch.randn((B, heads, N, L), generator=g)
    Wo = rnd((B * N, C), 43)
    scale = float(torch.tensor(d ** -0.5, dtype=torch.float32))   # the fp32 number the library receives
    q, k, v = (bufs[n][:, PAD:PAD + C].double().requires_grad_(True) for n in ("q", "k", "v"))
    split = lambda t, n: t.reshape(B, n, heads, d).permute(0, 2, 1, 3)
    score = scale * (split(q, N) @ split(k, L).transpose(-1, -2))
    prob = torch.softmax(score * mult.double() + bias.double(), dim=-1)
    o = (prob @ split(v, L)).permute(0, 2, 1, 3).reshape(B * N, C)
    terms = dict(s=(score * Ws.double()).sum(), p=(prob * Wp.double()).sum(), o=(o * Wo.double()).sum())
    grads = {}
    for variant, use in (("both", "spo"), ("no_p", "so"), ("no_o", "sp")):
        gs = torch.autograd.grad(sum(terms[t] for t in use), (q, k, v), retain_graph=True, allow_unused=True)
        grads[variant] = tuple(torch.zeros_like(t) if g is None else g for g, t in zip(gs, (q, k, v)))      # Wo = 0: dv is exactly zero
    return dict(bufs=bufs, mult=mult, bias=bias, Ws=Ws, Wp=Wp, Wo=Wo, scale=scale, score=score.detach(), prob=prob.detach(), o=o.detach(),
                grads=grads)


@pytest.mark.parametrize("B,N,heads,d,L", CHAIN_CASES)
def test_explicit_attention_chain(dev, B, N, heads, d, L):
    """_ScoresFn -> rewrite -> _SoftmaxPVFn differentiated as ONE chain against fp64 autograd: q, k, v are column slices of wider fp16
    leaves; the rewrite multiplies the scores by a fixed fp32 tensor near 1 and (second variant) adds -inf on a fixed third of the keys;
    loss = sum score Ws + sum prob Wp + sum o Wo, and again with Wp = 0 and with Wo = 0.  Every L and d sits on an edge of the launchers of
    af_xattn_explicit.hip (L: 16, 80, 100 / 112, 128;  d: 16 / 32 / 48 / 64 / 80 for the mix and column-mix kernels), N crosses the 16- and 64-query
    tiles and goes below one tile (N = 1, 5: most column-mix chunks and waves have no query), d = 168 runs the wave-per-row kernels.
    Derived: score f32_bound(d, 1) (the scale's product); o, dq, dk, dv one fp16 rounding of fp32 arithmetic on fp32 probabilities.
    Measured: prob 3.08e-7 / 6.31e-7 (-> PROB_L2 7e-7, PROB_MAX 2e-6).
    Worst on MI355X: score 2.1e-7 of 8.3e-7 (d = 168), max 1.7e-7 of 3.5e-7 (d = 24); o 2.24e-4 / 3.55e-4, dq 2.48e-4 / 4.71e-4, dk 2.26e-4 / 4.56e-4,
    dv 2.17e-4 / 4.51e-4 of 6e-4 / 9.8e-4."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.capture_graph import _ScoresFn, _SoftmaxPVFn
    C = heads * d
    for masked in (False, True):
        P = chain_problem(B, N, heads, d, L, masked)
        mult, bias = P["mult"].to(dev), P["bias"].to(dev)
        Ws, Wp, Wo = P["Ws"].to(dev), P["Wp"].to(dev), P["Wo"].to(dev).float()
        for variant in ("both", "no_p", "no_o"):
            tag = f"chain {B, N, heads, d, L} masked={int(masked)} {variant}"
            leaves = {n: P["bufs"][n].to(dev).requires_grad_(True) for n in ("q", "k", "v")}
            q, k, v = (leaves[n][:, PAD:PAD + C] for n in ("q", "k", "v"))
            score = _ScoresFn.apply(q, k, B, N, L, heads, d, P["scale"])
            prob, o = _SoftmaxPVFn.apply(score * mult + bias, v, B, N, L, heads, d)
            loss = (score * Ws).sum()
            if variant != "no_p":
                loss = loss + (prob * Wp).sum()
            if variant != "no_o":
                loss = loss + (o.float() * Wo).sum()
            loss.backward()
            if variant == "both":
                cmp(f"{tag} score", score, P["score"], f32_bound(d), f32_bound(d), torch.float32)
                cmp(f"{tag} prob PROB", prob, P["prob"], PROB_L2, PROB_MAX, torch.float32)
                cmp(f"{tag} o", o, P["o"], F16_L2, F16_MAX, torch.float16)
                if masked:
                    assert bool((prob[..., 1::3] == 0).all()), (tag, "a masked key has a probability")
            for n, ref in zip(("q", "k", "v"), P["grads"][variant]):
                gfull = leaves[n].grad
                assert gfull is not None and gfull.dtype == torch.float16, (tag, n)
                cmp(f"{tag} d{n}", gfull[:, PAD:PAD + C], ref, F16_L2, F16_MAX)
                assert bool((gfull[:, :PAD] == 0).all()) and bool((gfull[:, PAD + C:] == 0).all()), (tag, n, "gradient outside the slice")


# =============================================================================================== 7. one encoder layer end to end
LAYER = dict(E=80, heads=2, inter=160, B=2, T=9)


def _layer_params(m):
    """(name, shape, std) of every parameter of a CLIPEncoderLayer whose attention has multiplier m, in named_parameters order."""
    E, I = LAYER["E"], LAYER["inter"]
    return [("self_attn.k_proj.weight", (m * E, E), E ** -0.5), ("self_attn.k_proj.bias", (m * E,), 0.3),
            ("self_attn.v_proj.weight", (m * E, E), E ** -0.5), ("self_attn.v_proj.bias", (m * E,), 0.3),
            ("self_attn.q_proj.weight", (E, E), E ** -0.5), ("self_attn.q_proj.bias", (E,), 0.3),
            ("self_attn.out_proj.weight", (E, E), E ** -0.5), ("self_attn.out_proj.bias", (E,), 0.3),
            ("layer_norm1.weight", (E,), None), ("layer_norm1.bias", (E,), 0.3),
            ("mlp.fc1.weight", (I, E), E ** -0.5), ("mlp.fc1.bias", (I,), 0.3),
            ("mlp.fc2.weight", (E, I), I ** -0.5), ("mlp.fc2.bias", (E,), 0.3),
            ("layer_norm2.weight", (E,), None), ("layer_norm2.bias", (E,), 0.3)]


@functools.lru_cache(maxsize=None)
def layer_problem(m):
    """fp16-representable parameters, input and output gradient; the fp64 restatement of the layer (LayerNorm, q / k / v with m keys per token
    and the causal rule j // m <= i, out_proj + residual, LayerNorm, fc1, quick-GELU, fc2 + residual) and its autograd."""
    E, heads, B, T = LAYER["E"], LAYER["heads"], LAYER["B"], LAYER["T"]
    d = E // heads
    params = {}
    for i, (name, shape, std) in enumerate(_layer_params(m)):
        params[name] = (1.0 + 0.2 * rnd(shape, 60 + i).float()).half() if std is None else rnd(shape, 60 + i, std)
    h, G = rnd((B * T, E), 90), rnd((B * T, E), 91)
    p = {n: t.double().requires_grad_(True) for n, t in params.items()}
    hd = h.double().requires_grad_(True)
    lin = lambda x, n: x @ p[n + ".weight"].t() + p[n + ".bias"]
    x1 = F.layer_norm(hd, (E,), p["layer_norm1.weight"], p["layer_norm1.bias"], 1e-5)
    q = lin(x1, "self_attn.q_proj").reshape(B, T, heads, d).permute(0, 2, 1, 3)
    kp = lin(x1, "self_attn.k_proj")
    kp.retain_grad()
    k = kp.reshape(B, T * m, heads, d).permute(0, 2, 1, 3)
    v = lin(x1, "self_attn.v_proj").reshape(B, T * m, heads, d).permute(0, 2, 1, 3)
    s = d ** -0.5 * (q @ k.transpose(-1, -2))
    visible = torch.arange(T * m)[None, :] // m <= torch.arange(T)[:, None]
    s = s.masked_fill(~visible, -math.inf)
    o = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * T, E)
    h2 = lin(o, "self_attn.out_proj") + hd
    f = lin(F.layer_norm(h2, (E,), p["layer_norm2.weight"], p["layer_norm2.bias"], 1e-5), "mlp.fc1")
    out = lin(f * torch.sigmoid(1.702 * f), "mlp.fc2") + h2
    out.backward(G.double())
    # m = 1: a constant added to every key moves each score row by a constant, which the softmax does not see: d(k_proj.bias) = sum of the
    # rows of dk is ZERO analytically (1e-15 in fp64).  Its error is measured against what is being summed: the column sums of |dk|
    kb_scale = kp.grad.abs().sum(0) if m == 1 else None
    return dict(params=params, h=h, G=G, out=out.detach(), dh=hd.grad, grads={n: t.grad for n, t in p.items()}, kb_scale=kb_scale)


@pytest.mark.parametrize("m", [1, 2])
def test_encoder_layer(dev, m):
    """CLIPEncoderLayer.hip_autograd at hidden 80, 2 heads of 40, intermediate 160, B = 2, T = 9 against its fp64 restatement: the output, the
    input gradient and EVERY parameter gradient.  m = 1: QKVLinearFn + AttentionQKVFn; m = 2: the attention widened to two keys per token
    (three LinearFn + AttentionFn).  The only test here in which forward rounding compounds (nine fp16 tensors between input and output).
    Measured: LAYER_L2 / LAYER_MAX for every tensor (the parameter gradients are fp32 sums of fp16 activation gradients: they carry the
    fp16 chain's error, so they belong with the fp16 results).  Worst on MI355X: 1.00e-3 / 1.10e-3 (-> LAYER_L2 3e-3, LAYER_MAX 3e-3)."""
    from adaface_dev_amd.adaface.arc2face_models import CLIPAttentionMKV, CLIPEncoderLayer, clip_text_config
    P = layer_problem(m)
    cfg = clip_text_config(hidden_size=LAYER["E"], num_attention_heads=LAYER["heads"], num_hidden_layers=1, intermediate_size=LAYER["inter"])
    layer = CLIPEncoderLayer(cfg)
    if m != 1:
        layer.self_attn = CLIPAttentionMKV(cfg, multiplier=m)
    named = dict(layer.named_parameters())
    assert sorted(named) == sorted(P["params"]), "the restatement does not cover the layer's parameters"
    with torch.no_grad():
        for n, t in P["params"].items():
            assert tuple(named[n].shape) == tuple(t.shape), n
            named[n].copy_(t.float())
    layer = layer.to(dev)
    h = P["h"].to(dev).requires_grad_(True)
    with launches() as names:
        out = layer.hip_autograd(h, LAYER["B"], LAYER["T"])
        (out.float() * P["G"].to(dev).float()).sum().backward()
    assert "af_attention_bwd" in names and names.count("af_gemm") >= 8, names
    tag = f"layer m={m}"
    cmp(f"{tag} LAYER out", out, P["out"], LAYER_L2, LAYER_MAX, torch.float16)
    cmp(f"{tag} LAYER dh", h.grad, P["dh"], LAYER_L2, LAYER_MAX, torch.float16)
    for n, p in layer.named_parameters():
        if P["kb_scale"] is not None and n == "self_attn.k_proj.bias":
            # zero up to cancellation (layer_problem): the same two figures with sum_rows |dk| in place of the vanishing reference
            assert p.grad is not None and p.grad.dtype == torch.float32
            diff = p.grad.double().cpu() - P["grads"][n]
            e2, em = float(diff.norm() / P["kb_scale"].norm()), float(diff.abs().max() / P["kb_scale"].max())
            print(f"ERR {tag} LAYER d {n} (against sum |dk|): rel-L2 {e2:.3e} (< {LAYER_L2:.1e})  max/max {em:.3e} (< {LAYER_MAX:.1e})")
            assert e2 < LAYER_L2 and em < LAYER_MAX, (tag, n, e2, em)
            continue
        cmp(f"{tag} LAYER d {n}", p.grad, P["grads"][n], LAYER_L2, LAYER_MAX, torch.float32)
