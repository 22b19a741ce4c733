"""The ArcFace ResNetFace-18 IR-SE encoder's non-matmul kernels (csrc/af_face.hip), their ``ops`` wrappers and the ``hip_train`` / ``hip_bwd``
pairs of evaluation/arcface_resnet.py on a real MI355X (`pytest -m gpu`), each against an fp64 CPU reference computed from the same
fp16-rounded operands and fp32 parameters the device gets.  Nothing in a reference comes from the library.

Kernels (section 1).  Bound per ELEMENT of an fp16 output: ``2^-11 |ref|`` (``2^-25`` below fp16's normal range: half an ulp of the stored
value) ``+ 4 e32``, ``e32`` the largest error in that case of a plain fp32 torch CPU evaluation of the same formula (reductions summed
sequentially, the least accurate order) against fp64.  ``af_sigmoid`` is ``v_rcp_f32(1 + v_exp_f32(-x log2 e))``: both instructions are
accurate to 1 ulp ("AMD Instinct MI300 / CDNA3 Instruction Set Architecture", 2024, V_EXP_F32 / V_RCP_F32; HIP's ``__expf`` is
``native_exp``: one multiply by log2 e in front of V_EXP_F32), the multiply's rounding moves e = exp(-x) by |x| 2^-23 relative, so e is off
by (|x| + 1) 2^-23 relative and g = 1 / (1 + e) by g (1 - g) (|x| + 1) 2^-23 + 1.5 g 2^-23 (the add's and the reciprocal's rounding):
``_dsig``.  A PReLU decision may differ only where an affine or that sigmoid stands in front of it and the fp64 pre-activation lies within
their error of zero; such elements may match either branch and may be at most 1e-3 of a case (planted exact zeros are never excluded:
there the forward is 0 and every backward kernel gives ``slope * dy``, torch's rule).

Blocks (sections 3, 4).  ``_block_fwd`` / ``_block_bwd`` restate IRBlock + SEBlock in fp64 on the folded, fp16-rounded weights; every PReLU
takes its mask, the max-pool its argmax.  The device's input gradient is compared with the reference's vector-Jacobian product under the
DEVICE's decisions (recomputed on the host from the saved fp16 activations): with the masks fixed the block is linear in dy, so what is left
is fp16 rounding.  The bound is twice the error of the same restatement with every stored tensor rounded to 11 significant bits (fp16's
precision, no exponent limit: an underflow on the device is an error, not part of the bound), measured against the same reference."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F64 = torch.float64
TINY = 2.0 ** -14          # fp16's smallest normal number


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- helpers
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(k) for k in key))) % (2 ** 31))


def _h(shape, g, amp=1.0):
    """fp16 N(0, amp^2) values."""
    return (amp * torch.randn(tuple(shape), generator=g)).to(torch.float16)


def _dsig(s):
    """Bound on |af_sigmoid(s) - sigmoid(s)| (module docstring)."""
    g = torch.sigmoid(s)
    return (g * (1 - g) * (s.abs() + 1.0) + 1.5 * g) * 2.0 ** -23


def _call(name, *args):
    from adaface_dev_amd import _lib, ops
    rc = getattr(_lib.lib(), name)(*args, ops._stream())
    torch.cuda.synchronize()
    return rc


def _ok(name, *args):
    from adaface_dev_amd import _lib
    _lib.check(_call(name, *args), name)


def _out(dev, shape):
    return torch.full(tuple(shape), 777.0, dtype=torch.float16, device=dev)


def _assert_f16(what, got, ref, e32, extra=None, alt=None, amb=None):
    """got (fp16, host) against ref (fp64) element by element; ``alt`` / ``amb``: the other branch's value and where it is allowed."""
    got = got.cpu()
    assert got.dtype == torch.float16 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), what
    refh = ref.to(torch.float16)
    inf = torch.isinf(refh)                               # beyond 65504: inf on both sides, same sign
    assert bool((got[inf] == refh[inf]).all()), what
    bound = torch.where(ref.abs() < TINY, torch.full_like(ref, 2.0 ** -25), ref.abs() * 2.0 ** -11) + 4.0 * e32
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref).abs()
    n_amb = 0
    if amb is not None and bool(amb.any()):
        n_amb = int(amb.sum())
        abound = torch.where(alt.abs() < TINY, torch.full_like(alt, 2.0 ** -25), alt.abs() * 2.0 ** -11) + 4.0 * e32
        ok_alt = amb & ((got.double() - alt).abs() <= (abound if extra is None else abound + extra))
        err = torch.where(ok_alt, torch.zeros_like(err), err)
        assert n_amb <= 1e-3 * ref.numel(), (what, n_amb, ref.numel())
    bad = (err > bound) & ~inf
    worst = float((err / bound)[~inf].max()) if bool((~inf).any()) else 0.0
    print(f"{what}: worst err / bound {worst:.3f} (e32 {float(e32):.2e}, {n_amb} undecided of {ref.numel()})")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


def _prelu(f, sl):
    return f if sl is None else torch.where(f >= 0, f, f * sl)


def _prelu_grad(f, d, sl):
    return d if sl is None else torch.where(f > 0, d, d * sl)          # torch's rule: the slope at 0


# ----------------------------------------------------------------------------- 1. af_affine_prelu / _ch / _bwd
# (rows, C): n8 = rows * C / 8 = 1, 255, 256, 258 (257 is prime: 256 below, 258 above), a C / 8 that is no power of two in one workgroup and in four
AFFINE_SHAPES = [(1, 8), (255, 8), (32, 64), (43, 48), (7, 24), (5, 72), (101, 72)]
SLOPES = [0.25, 0.0, 1.0, -0.5, 1.5]


def _affine_case(rows, C, mode, slope, per_channel=False):
    g = _gen("affine", rows, C, mode, slope, per_channel)
    x = _h((rows, C), g)
    dy = _h((rows, C), g)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:max(2, flat.numel() // 16)]
    flat[idx[0::2]] = 0.0                                  # exact zeros of both signs at the decision
    flat[idx[1::2]] = -0.0
    scale = shift = sl = None
    if "a" in mode:
        scale = 1.0 + 0.2 * torch.randn(C, generator=g)
        shift = 0.3 * torch.randn(C, generator=g)
        shift[::3] = 0.0                                   # x = +-0 with zero shift: f = 0 exactly
    if "p" in mode:
        sl = torch.full((1,), slope) if not per_channel else slope + 0.25 * torch.randn(C, generator=g)
    return x, dy, scale, shift, sl


def _affine_refs(x, dy, scale, shift, sl):
    """fp64 forward / backward, the other branch, where it is allowed, e32 of both."""
    out = {}
    for dt in (F64, torch.float32):
        f = x.to(dt)
        d = dy.to(dt)
        if scale is not None:
            f = f * scale.to(dt) + shift.to(dt)
            d = d * scale.to(dt)
        s = None if sl is None else sl.to(dt)
        out[dt] = (f, _prelu(f, s), _prelu_grad(f, d, s), d)
    f, y, dx, d = out[F64]
    f32, y32, dx32, _ = out[torch.float32]
    ef = (f32.double() - f).abs().max()
    amb = alt_y = alt_dx = None
    if sl is not None and scale is not None:
        planted = (x == 0) & (shift == 0)[None, :]
        amb = (f.abs() <= 4 * ef) & ~planted
        alt_y = torch.where(f >= 0, f * sl.double(), f)
        alt_dx = torch.where(f > 0, d * sl.double(), d)
        y32, dx32 = torch.where(amb, y.float(), y32), torch.where(amb, dx.float(), dx32)      # (e32 is the arithmetic's error, not a decision's)
    return y, dx, (y32.double() - y).abs().max(), (dx32.double() - dx).abs().max(), amb, alt_y, alt_dx


@pytest.mark.parametrize("mode", ["ap", "p", "a"])
@pytest.mark.parametrize("rows,C", AFFINE_SHAPES)
def test_affine_prelu_kernels_vs_fp64(dev, rows, C, mode):
    """af_affine_prelu, af_affine_prelu_ch and af_affine_prelu_bwd in every operand combination: scale + shift and slope, slope only, scale + shift only."""
    for per_channel in (False, True):
        x, dy, scale, shift, sl = _affine_case(rows, C, mode, 0.25, per_channel)
        y_ref, dx_ref, ey, edx, amb, alt_y, alt_dx = _affine_refs(x, dy, scale, shift, sl)
        xd, dyd = x.to(dev), dy.to(dev)
        pd = [None if t is None else t.to(dev) for t in (scale, shift, sl)]
        ptr = [None if t is None else t.data_ptr() for t in pd]
        y = _out(dev, (rows, C))
        entry = "af_affine_prelu_ch" if per_channel else "af_affine_prelu"
        _ok(entry, xd.data_ptr(), *ptr, y.data_ptr(), rows, C)
        _assert_f16(f"{entry} {rows}x{C} {mode}", y, y_ref, ey, alt=alt_y, amb=amb)
        if not per_channel:
            dx = _out(dev, (rows, C))
            _ok("af_affine_prelu_bwd", xd.data_ptr() if sl is not None else None, *ptr, dyd.data_ptr(), dx.data_ptr(), rows, C)
            _assert_f16(f"af_affine_prelu_bwd {rows}x{C} {mode}", dx, dx_ref, edx, alt=alt_dx, amb=amb)
            if sl is None:                                 # x is not read without a PReLU: passing it changes nothing
                dx2 = _out(dev, (rows, C))
                _ok("af_affine_prelu_bwd", xd.data_ptr(), *ptr, dyd.data_ptr(), dx2.data_ptr(), rows, C)
                assert torch.equal(dx2, dx)


@pytest.mark.parametrize("slope", SLOPES)
def test_prelu_decisions_at_exact_zeros(dev, slope):
    """x = +-0 (no affine, and under an affine with zero shift) and x = 0, residual = 0: the forward is 0 and all three backward kernels give
    slope * dy.  Without an affine f = x exactly, so nothing is excluded; the slopes include 0, 1, a negative one and one above 1."""
    rows, C = 37, 24
    B, HW = 3, 35
    for mode in ("p", "ap"):
        x, dy, scale, shift, sl = _affine_case(rows, C, mode, slope)
        y_ref, dx_ref, ey, edx, amb, alt_y, alt_dx = _affine_refs(x, dy, scale, shift, sl)
        pd = [None if t is None else t.to(dev) for t in (scale, shift, sl)]
        ptr = [None if t is None else t.data_ptr() for t in pd]
        xd, dyd, y, dx = x.to(dev), dy.to(dev), _out(dev, (rows, C)), _out(dev, (rows, C))
        _ok("af_affine_prelu", xd.data_ptr(), *ptr, y.data_ptr(), rows, C)
        _ok("af_affine_prelu_bwd", xd.data_ptr(), *ptr, dyd.data_ptr(), dx.data_ptr(), rows, C)
        _assert_f16(f"af_affine_prelu slope {slope} {mode}", y, y_ref, ey, alt=alt_y, amb=amb)
        _assert_f16(f"af_affine_prelu_bwd slope {slope} {mode}", dx, dx_ref, edx, alt=alt_dx, amb=amb)
        zero = (x == 0) if scale is None else ((x == 0) & (shift == 0)[None, :])
        assert int(zero.sum()) >= 8
        assert bool((y.cpu()[zero] == 0).all())
        want = dy.double() * slope * (1.0 if scale is None else scale.double()[None, :])        # one fp16 rounding of two fp32 products
        assert bool(((dx.cpu()[zero].double() - want[zero]).abs() <= want[zero].abs() * (2.0 ** -11 + 2.0 ** -22) + 2.0 ** -25).all())
    case = _se_case(B, HW, C, slope, with_se=True)
    _check_se_kernels(dev, case, f"zeros slope {slope}", with_dpool=True)
    _check_gate_grad(dev, case, f"zeros slope {slope}")
    x, r, dy, se, sl, dpool = case
    zero = (x == 0) & (r == 0)
    assert int(zero.sum()) >= 8
    xd, rd, dyd, sed, sld = (t.to(dev) for t in (x, r, dy, se, sl))
    y, dx, dres = (_out(dev, x.shape) for _ in range(3))
    _ok("af_se_residual_prelu", xd.data_ptr(), sed.data_ptr(), rd.data_ptr(), sld.data_ptr(), y.data_ptr(), B, HW, C)
    _ok("af_se_residual_prelu_bwd", xd.data_ptr(), sed.data_ptr(), rd.data_ptr(), sld.data_ptr(), dyd.data_ptr(), None, dx.data_ptr(),
        dres.data_ptr(), B, HW, C)
    assert bool((y.cpu()[zero] == 0).all())
    want = (dy.double() * slope).to(torch.float16)                     # dresidual = slope * dy, one rounding
    assert torch.equal(dres.cpu()[zero], want[zero])


def test_affine_beyond_fp16_range_is_inf_on_both_sides(dev):
    """An affine result beyond 65504 is inf in the device output and in the fp64 reference rounded to fp16 (and -inf * slope keeps its sign)."""
    rows, C = 9, 24
    x, dy, scale, shift, sl = _affine_case(rows, C, "ap", 0.25)
    for i in range(rows):                                  # every |f| is 2e4 or more: some finite, some beyond the range, no decision near 0
        x[i, :] = (-1.0) ** i * (16000.0 + 6000.0 * i)
    x[8, :] = 65504.0
    scale[:] = scale.abs() + 1.2
    y_ref, _, ey, _, amb, alt_y, _ = _affine_refs(x, dy, scale, shift, sl)
    assert int(torch.isinf(y_ref.to(torch.float16)).sum()) >= 2 * C
    pd = [t.to(dev) for t in (scale, shift, sl)]
    xd, y = x.to(dev), _out(dev, (rows, C))
    _ok("af_affine_prelu", xd.data_ptr(), *[t.data_ptr() for t in pd], y.data_ptr(), rows, C)
    _assert_f16("af_affine_prelu overflow", y, y_ref, ey, alt=alt_y, amb=amb)


# ----------------------------------------------------------------------------- 1. SE excite + shortcut + PReLU, forward and backward
def _se_case(B, HW, C, slope, with_se, logits=None):
    g = _gen("se", B, HW, C, slope, with_se)
    x, r, dy = _h((B, HW, C), g), _h((B, HW, C), g), _h((B, HW, C), g)
    n = x.numel()
    idx = torch.randperm(n, generator=g)[:max(2, n // 16)]
    x.view(-1)[idx] = 0.0                                  # x = 0, residual = +-0: pre = 0 exactly
    r.view(-1)[idx[0::2]] = 0.0
    r.view(-1)[idx[1::2]] = -0.0
    se = None
    if with_se:
        se = _h((B, C), g, 1.5) if logits is None else logits
    dpool = _h((B, C), g, 0.1)
    return x, r, dy, se, torch.full((1,), slope), dpool


def _se_refs(x, r, dy, se, sl, dpool):
    """fp64 y, dx, dresidual, their e32, the sigmoid's room, the other branch and where it is allowed."""
    res = {}
    for dt in (F64, torch.float32):
        gt = torch.ones((x.shape[0], 1, x.shape[2]), dtype=dt) if se is None else torch.sigmoid(se.to(dt))[:, None, :]
        pre = x.to(dt) * gt + r.to(dt)
        res[dt] = (pre, gt)
    pre, gt = res[F64]
    pre32 = res[torch.float32][0]
    dg = torch.zeros_like(gt) if se is None else _dsig(se.double())[:, None, :]
    room = x.double().abs() * dg                            # what the fast sigmoid may move pre by
    planted = (x == 0) & (r == 0)
    amb = ((pre.abs() <= 4 * (pre32.double() - pre).abs().max() + room) & ~planted) if se is not None else torch.zeros_like(planted)
    slq, dyq = sl.double(), dy.double()
    dp = 0.0 if dpool is None else dpool.double()[:, None, :]
    d = torch.where(pre > 0, dyq, dyq * slq)
    d_alt = torch.where(pre > 0, dyq * slq, dyq)
    ref = dict(y=_prelu(pre, slq), dx=d * gt + dp, dres=d)
    alt = dict(y=torch.where(pre >= 0, pre * slq, pre), dx=d_alt * gt + dp, dres=d_alt)
    # fp32 evaluation with the fp64 decision (e32 is the arithmetic's error)
    gt32, sl32, dy32 = res[torch.float32][1], sl.float(), dy.float()
    d32 = torch.where(pre > 0, dy32, dy32 * sl32)
    f32 = dict(y=torch.where(pre >= 0, pre32, pre32 * sl32), dx=d32 * gt32 + (0.0 if dpool is None else dpool.float()[:, None, :]), dres=d32)
    e32 = {k: (f32[k].double() - ref[k]).abs().max() for k in ref}
    amp = max(1.0, abs(float(sl)))
    extra = dict(y=room * amp, dx=dyq.abs() * amp * dg, dres=torch.zeros_like(room))
    return ref, alt, amb, e32, extra, pre, gt


def _check_se_kernels(dev, case, what, with_dpool):
    x, r, dy, se, sl, dpool = case
    B, HW, C = x.shape
    dpool = dpool if with_dpool else None
    ref, alt, amb, e32, extra, _, _ = _se_refs(x, r, dy, se, sl, dpool)
    xd, rd, dyd, sld = x.to(dev), r.to(dev), dy.to(dev), sl.to(dev)
    sed = None if se is None else se.to(dev)
    dpd = None if dpool is None else dpool.to(dev)
    p = lambda t: None if t is None else t.data_ptr()
    y, dx, dres = (_out(dev, x.shape) for _ in range(3))
    _ok("af_se_residual_prelu", p(xd), p(sed), p(rd), p(sld), p(y), B, HW, C)
    _ok("af_se_residual_prelu_bwd", p(xd), p(sed), p(rd), p(sld), p(dyd), p(dpd), p(dx), p(dres), B, HW, C)
    for k, got in (("y", y), ("dx", dx), ("dres", dres)):
        _assert_f16(f"af_se_residual_prelu{'' if k == 'y' else '_bwd'}.{k} {what}", got, ref[k], e32[k], extra=extra[k], alt=alt[k], amb=amb)


# (B, HW, C): one thread; n8 = 255, 256, 258; a workgroup that straddles two batch items (105 chunks per item); the same in several workgroups
SE_SHAPES = [(1, 1, 8), (1, 255, 8), (2, 16, 64), (2, 43, 24), (3, 35, 24), (3, 35, 72)]


@pytest.mark.parametrize("with_se,with_dpool", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,HW,C", SE_SHAPES)
def test_se_residual_prelu_kernels_vs_fp64(dev, B, HW, C, with_se, with_dpool):
    """af_se_residual_prelu and af_se_residual_prelu_bwd with and without se_logits / dpool; every item's gate and dpool on its own pixels."""
    _check_se_kernels(dev, _se_case(B, HW, C, 0.25, with_se), f"{B}x{HW}x{C} se={with_se} dpool={with_dpool}", with_dpool)


# ----------------------------------------------------------------------------- 1. af_se_gate_grad
def _gate_grad_refs(x, r, dy, se, sl):
    """fp64 sigmoid' * mean_hw(dpre * x), e32 (fp32, summed sequentially), the room of the fast sigmoid and of undecided elements."""
    _, _, amb, _, _, pre, gt = _se_refs(x, r, dy, se, sl, None)
    HW = x.shape[1]
    slq = sl.double()
    term = torch.where(pre > 0, dy.double(), dy.double() * slq) * x.double()
    S = term.sum(dim=1)
    g = gt[:, 0, :]
    ref = S * g * (1 - g) / HW
    g32 = torch.sigmoid(se.float())
    t32 = torch.where(pre > 0, dy.float(), dy.float() * sl.float()) * x.float()
    f32 = t32.cumsum(dim=1)[:, -1, :] * g32 * (1 - g32) / HW
    e32 = (f32.double() - ref).abs().max()
    dsp = _dsig(se.double()) + 2.0 ** -23                    # |g (1 - g) - sigmoid'|: the gate's error plus the rounding of 1 - g
    extra = S.abs() / HW * dsp + ((1 - slq).abs() * (dy.double() * x.double()).abs() * amb).sum(dim=1) * g * (1 - g) / HW
    return ref, e32, extra, int(amb.sum())


def _check_gate_grad(dev, case, what):
    x, r, dy, se, sl, _ = case
    B, HW, C = x.shape
    ref, e32, extra, n_amb = _gate_grad_refs(x, r, dy, se, sl)
    assert n_amb <= 1e-3 * x.numel()
    t = [v.to(dev) for v in (x, se, r, sl, dy)]
    dgl = _out(dev, (B, C))
    _ok("af_se_gate_grad", *[v.data_ptr() for v in t], dgl.data_ptr(), B, HW, C)
    _assert_f16(f"af_se_gate_grad {what}", dgl, ref, e32, extra=extra)
    return dgl.cpu().double()


@pytest.mark.parametrize("HW", [1, 3, 4, 5, 4096])
def test_se_gate_grad_vs_fp64(dev, HW):
    """Fewer pixels than waves, as many, more, and the 64 x 64 level; channel counts of one partial slab, one whole slab and a slab and a tail
    (the kernel reads scalars, so C = 20 is legal)."""
    for C in (8, 20, 64, 72):
        _check_gate_grad(dev, _se_case(2, HW, C, 0.25, True), f"HW {HW} C {C}")


def test_gate_logit_extremes(dev):
    """Gate logits +-20 and +-65504: the gate is 0 or 1 to rounding, its gradient 0 or tiny, nothing is NaN."""
    B, HW, C = 3, 35, 24
    logits = torch.zeros((B, C))
    logits[:, 0::4], logits[:, 1::4], logits[:, 2::4], logits[:, 3::4] = 20.0, -20.0, 65504.0, -65504.0
    logits = logits.to(torch.float16)
    case = _se_case(B, HW, C, 0.25, True, logits=logits)
    _check_se_kernels(dev, case, "extreme logits", with_dpool=True)
    got = _check_gate_grad(dev, case, "extreme logits")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1e-5          # |S| / HW is a few units, sigmoid' and its error below 4e-7
    assert bool((got[:, 2::4] == 0).all()) and bool((got[:, 3::4] == 0).all())


# ----------------------------------------------------------------------------- 1. max-pool
def _pool_case(B, H, W, C):
    """Small integers (ties in every position of the window, all-negative windows) with planted +0 / -0 ties and +-65504."""
    g = _gen("pool", B, H, W, C)
    x = torch.randint(-3, 3, (B, H, W, C), generator=g).to(torch.float16)
    x[:, 0:2, 0:2, :] = -torch.rand((B, 2, 2, C), generator=g).to(torch.float16) - 1.0          # all negative, distinct
    x[:, 0:2, 2:4, :] = -2.0                                                                      # all negative, four-way tie
    x[:, 2:4, 0:2, :] = torch.tensor([0.0, -0.0, -0.0, 0.0]).to(torch.float16).reshape(1, 2, 2, 1)   # +0 first
    x[:, 2:4, 2:4, :] = torch.tensor([-0.0, 0.0, -1.0, 0.0]).to(torch.float16).reshape(1, 2, 2, 1)   # -0 first
    for k in range(4):                                                                            # the maximum in each position, +-65504 among them
        win = torch.full((2, 2), -65504.0)
        win[k // 2, k % 2] = 65504.0 if k % 2 else -3.0
        x[:, 4:6, 2 * k:2 * k + 2, k % C] = win.to(torch.float16)
    for a, b in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):                                  # two-way ties at every pair of positions
        win = torch.full((4,), -1.0)
        win[a] = win[b] = 2.5
        x[:, H - 2:H, 0:2, (a * 4 + b) % C] = win.reshape(2, 2).to(torch.float16)
    return x, _h((B, H // 2, W // 2, C), g)


@pytest.mark.parametrize("B,H,W,C", [(1, 6, 8, 8), (2, 6, 10, 24), (3, 8, 12, 72)])
def test_maxpool2x2_and_backward_bit_exact(dev, B, H, W, C):
    """Non-square sizes, one workgroup and several.  Forward equals F.max_pool2d; backward equals torch's routing (the first maximum of the
    window); every element of dx is written (dx starts as 777)."""
    x, dy = _pool_case(B, H, W, C)
    xr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 2, 2)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    xd, dyd = x.to(dev), dy.to(dev)
    y, dx = _out(dev, (B, H // 2, W // 2, C)), _out(dev, (B, H, W, C))
    _ok("af_maxpool2x2", xd.data_ptr(), y.data_ptr(), B, H // 2, W // 2, C)
    _ok("af_maxpool2x2_bwd", xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), B, H // 2, W // 2, C)
    assert torch.equal(y.cpu().float(), ref.detach().permute(0, 2, 3, 1))
    assert torch.equal(dx.cpu().float(), xr.grad.permute(0, 2, 3, 1))
    from adaface_dev_amd import ops
    assert torch.equal(ops.maxpool2x2(xd), y) and torch.equal(ops.maxpool2x2_bwd(xd, dyd), dx)


# ----------------------------------------------------------------------------- 1. global average pool
def _avgpool_check(dev, x, what, view=None):
    B, HW, C = x.shape
    ref = x.double().mean(dim=1)
    e32 = (x.float().cumsum(dim=1)[:, -1, :] / HW - ref).abs().max()
    xd = x.to(dev) if view is None else view
    out = _out(dev, (B, C))
    _ok("af_global_avgpool", xd.data_ptr(), out.data_ptr(), B, HW, C)
    _assert_f16(f"af_global_avgpool {what}", out, ref, e32)


@pytest.mark.parametrize("HW", [1, 127, 128, 129, 4096])
def test_global_avgpool_vs_fp64(dev, HW):
    """One pixel, one short of the 128 pixel slots, exactly one pass, a second pass, the 64 x 64 level; one partial 64-channel slab, exactly one, one
    and a partial one, two and a partial one.  A constant offset keeps the means away from 0, so the relative bound is a real one."""
    for C in (8, 64, 72, 136):
        x = (_h((2, HW, C), _gen("avg", HW, C)).float() + 0.5).to(torch.float16)
        _avgpool_check(dev, x, f"HW {HW} C {C}")


@pytest.mark.parametrize("HW", [1, 129])
def test_global_avgpool_scalar_form(dev, HW):
    """The scalar (vec == 0) form through the entry point: C = 20, and C = 72 at a base address that is not 16-byte aligned."""
    x = (_h((2, HW, 20), _gen("avg20", HW)).float() + 0.5).to(torch.float16)
    _avgpool_check(dev, x, f"HW {HW} C 20")
    x = (_h((2, HW, 72), _gen("avg72u", HW)).float() + 0.5).to(torch.float16)
    buf = torch.zeros(x.numel() + 8, dtype=torch.float16, device=dev)
    view = buf[4:4 + x.numel()]
    view.copy_(x.reshape(-1).to(dev))
    assert view.data_ptr() % 16 == 8
    _avgpool_check(dev, x, f"HW {HW} C 72 unaligned", view=view)


# ----------------------------------------------------------------------------- 1. refusals
_SIG = {
    "af_affine_prelu": ("x scale shift slope y rows C", "y"),
    "af_affine_prelu_ch": ("x scale shift slope y rows C", "y"),
    "af_maxpool2x2": ("x y B Ho Wo C", "y"),
    "af_global_avgpool": ("x y B HW C", "y"),
    "af_se_residual_prelu": ("x se res slope y B HW C", "y"),
    "af_affine_prelu_bwd": ("x scale shift slope dy dx rows C", "dx"),
    "af_maxpool2x2_bwd": ("x dy dx B Ho Wo C", "dx"),
    "af_se_gate_grad": ("x se res slope dy dgl B HW C", "dgl"),
    "af_se_residual_prelu_bwd": ("x se res slope dy dpool dx dres B HW C", "dx dres"),
}
_REFUSALS = [
    ("af_affine_prelu", dict(C=12)), ("af_affine_prelu", dict(C=0)), ("af_affine_prelu", dict(rows=0)), ("af_affine_prelu", dict(shift=None)),
    ("af_affine_prelu", dict(scale=None)), ("af_affine_prelu", dict(x=None)), ("af_affine_prelu", dict(y=None)),
    ("af_affine_prelu_ch", dict(C=12)), ("af_affine_prelu_ch", dict(rows=-1)), ("af_affine_prelu_ch", dict(shift=None)),
    ("af_affine_prelu_ch", dict(scale=None)), ("af_affine_prelu_ch", dict(x=None)), ("af_affine_prelu_ch", dict(y=None)),
    ("af_maxpool2x2", dict(C=12)), ("af_maxpool2x2", dict(B=0)), ("af_maxpool2x2", dict(Ho=0)), ("af_maxpool2x2", dict(Wo=-1)),
    ("af_maxpool2x2", dict(x=None)), ("af_maxpool2x2", dict(y=None)),
    ("af_global_avgpool", dict(HW=0)), ("af_global_avgpool", dict(B=0)), ("af_global_avgpool", dict(C=0)), ("af_global_avgpool", dict(x=None)),
    ("af_global_avgpool", dict(y=None)),
    ("af_se_residual_prelu", dict(C=12)), ("af_se_residual_prelu", dict(HW=0)), ("af_se_residual_prelu", dict(B=-2)),
    ("af_se_residual_prelu", dict(x=None)), ("af_se_residual_prelu", dict(res=None)), ("af_se_residual_prelu", dict(slope=None)),
    ("af_se_residual_prelu", dict(y=None)),
    ("af_affine_prelu_bwd", dict(C=12)), ("af_affine_prelu_bwd", dict(rows=0)), ("af_affine_prelu_bwd", dict(shift=None)),
    ("af_affine_prelu_bwd", dict(scale=None)), ("af_affine_prelu_bwd", dict(x=None)), ("af_affine_prelu_bwd", dict(dy=None)),
    ("af_affine_prelu_bwd", dict(dx=None)),
    ("af_maxpool2x2_bwd", dict(C=12)), ("af_maxpool2x2_bwd", dict(Ho=0)), ("af_maxpool2x2_bwd", dict(Wo=0)), ("af_maxpool2x2_bwd", dict(x=None)),
    ("af_maxpool2x2_bwd", dict(dy=None)), ("af_maxpool2x2_bwd", dict(dx=None)),
    ("af_se_gate_grad", dict(HW=0)), ("af_se_gate_grad", dict(C=0)), ("af_se_gate_grad", dict(B=0)), ("af_se_gate_grad", dict(x=None)),
    ("af_se_gate_grad", dict(se=None)), ("af_se_gate_grad", dict(res=None)), ("af_se_gate_grad", dict(slope=None)),
    ("af_se_gate_grad", dict(dy=None)), ("af_se_gate_grad", dict(dgl=None)),
    ("af_se_residual_prelu_bwd", dict(C=12)), ("af_se_residual_prelu_bwd", dict(B=0)), ("af_se_residual_prelu_bwd", dict(HW=-1)),
    ("af_se_residual_prelu_bwd", dict(x=None)), ("af_se_residual_prelu_bwd", dict(res=None)), ("af_se_residual_prelu_bwd", dict(slope=None)),
    ("af_se_residual_prelu_bwd", dict(dy=None)), ("af_se_residual_prelu_bwd", dict(dx=None)), ("af_se_residual_prelu_bwd", dict(dres=None)),
]


@pytest.mark.parametrize("entry,change", _REFUSALS, ids=[f"{e[3:]}-{k}={v}" for e, c in _REFUSALS for k, v in c.items()])
def test_face_kernel_refusals_leave_the_output_untouched(dev, entry, change):
    """C % 8 != 0 where the kernel needs 16-byte chunks, scale without shift (and the reverse), a PReLU gradient without x, a NULL operand, a
    non-positive size: AF_E_BADARG, and no output (pre-filled with 777) is written."""
    from adaface_dev_amd import _lib
    B, Ho, Wo, C = 2, 3, 4, 16
    big = lambda: torch.zeros((B, 2 * Ho, 2 * Wo, C), dtype=torch.float16, device=dev)
    t = dict(x=big(), se=torch.zeros((B, C), dtype=torch.float16, device=dev), res=big(), dy=big(), dpool=torch.zeros((B, C), dtype=torch.float16, device=dev),
             scale=torch.ones(C, device=dev), shift=torch.zeros(C, device=dev), slope=torch.full((C,), 0.25, device=dev))
    names, outs = _SIG[entry]
    outs = {n: _out(dev, (B, 2 * Ho, 2 * Wo, C)) for n in outs.split()}
    size = dict(rows=B * 4 * Ho * Wo, B=B, Ho=Ho, Wo=Wo, HW=4 * Ho * Wo, C=C)
    args = []
    for n in names.split():
        if n in change:
            args.append(change[n])
        elif n in size:
            args.append(size[n])
        else:
            args.append((outs[n] if n in outs else t[n]).data_ptr())
    rc = _call(entry, *args)
    assert rc == _lib.AF_E_BADARG
    for o in outs.values():
        assert bool((o == 777.0).all())


# ----------------------------------------------------------------------------- 2. the wrappers
def test_face_wrappers_refuse_bad_operands(dev):
    """Every tensor must be fp16, on the device and contiguous, every parameter contiguous fp32 of the right length there, the pooled sides even: a
    RuntimeError that names the operand.  The calls the network makes (a 2-D SE hidden row, nn.Parameter slopes) still pass."""
    from adaface_dev_amd import ops
    B, H, W, C = 2, 4, 6, 16
    x = torch.zeros((B, H, W, C), dtype=torch.float16, device=dev)
    se = torch.zeros((B, C), dtype=torch.float16, device=dev)
    dyp = torch.zeros((B, H // 2, W // 2, C), dtype=torch.float16, device=dev)
    sc, sh, sl = torch.ones(C, device=dev), torch.zeros(C, device=dev), nn.Parameter(torch.full((1,), 0.25, device=dev))
    strided = torch.zeros((B, H, W, 2 * C), dtype=torch.float16, device=dev)[..., :C]
    odd_h, odd_w = x[:, :3].contiguous(), x[:, :, :5].contiguous()
    bad_t = [("fp32", x.float()), ("strided", strided), ("host", x.cpu())]
    bad_p = lambda p: [p.detach().half(), p.detach().double(), p.detach().cpu(), p.detach()[:0].contiguous(), torch.cat([p.detach(), p.detach()])]
    calls = []                                             # (operand named in the message, callable)
    for _, b in bad_t:
        calls += [("affine_prelu.x", lambda b=b: ops.affine_prelu(b, sc, sh, sl)), ("maxpool2x2.x", lambda b=b: ops.maxpool2x2(b)),
                  ("global_avgpool.x", lambda b=b: ops.global_avgpool(b)),
                  ("se_residual_prelu.x", lambda b=b: ops.se_residual_prelu(b, se, x, sl)),
                  ("se_residual_prelu.residual", lambda b=b: ops.se_residual_prelu(x, se, b, sl)),
                  ("affine_prelu_bwd.dy", lambda b=b: ops.affine_prelu_bwd(b, x, sc, sh, sl)),
                  ("affine_prelu_bwd.x", lambda b=b: ops.affine_prelu_bwd(x, b, sc, sh, sl)),
                  ("maxpool2x2_bwd.x", lambda b=b: ops.maxpool2x2_bwd(b, dyp)),
                  ("se_gate_grad.x", lambda b=b: ops.se_gate_grad(b, se, x, sl, x)),
                  ("se_gate_grad.residual", lambda b=b: ops.se_gate_grad(x, se, b, sl, x)),
                  ("se_gate_grad.dy", lambda b=b: ops.se_gate_grad(x, se, x, sl, b)),
                  ("se_residual_prelu_bwd.x", lambda b=b: ops.se_residual_prelu_bwd(b, se, x, sl, x)),
                  ("se_residual_prelu_bwd.residual", lambda b=b: ops.se_residual_prelu_bwd(x, se, b, sl, x)),
                  ("se_residual_prelu_bwd.dy", lambda b=b: ops.se_residual_prelu_bwd(x, se, x, sl, b))]
    for b in (se.float(), se.cpu(), torch.zeros((B, 2 * C), dtype=torch.float16, device=dev)[:, :C], se[:1].contiguous()):
        calls += [("se_residual_prelu.se_logits", lambda b=b: ops.se_residual_prelu(x, b, x, sl)),
                  ("se_gate_grad.se_logits", lambda b=b: ops.se_gate_grad(x, b, x, sl, x)),
                  ("se_residual_prelu_bwd.se_logits", lambda b=b: ops.se_residual_prelu_bwd(x, b, x, sl, x)),
                  ("se_residual_prelu_bwd.dpool", lambda b=b: ops.se_residual_prelu_bwd(x, se, x, sl, x, b))]
    for b in (dyp.float(), dyp.cpu(), x):
        calls.append(("maxpool2x2_bwd.dy", lambda b=b: ops.maxpool2x2_bwd(x, b)))
    for b in bad_p(sc) + [torch.stack([sc, sc], dim=-1)[..., 0]]:
        calls += [("affine_prelu.scale", lambda b=b: ops.affine_prelu(x, b, sh, sl)), ("affine_prelu.shift", lambda b=b: ops.affine_prelu(x, sc, b, sl)),
                  ("affine_prelu_bwd.scale", lambda b=b: ops.affine_prelu_bwd(x, x, b, sh, sl)),
                  ("affine_prelu_bwd.shift", lambda b=b: ops.affine_prelu_bwd(x, x, sc, b, sl))]
    for b in bad_p(sl):
        calls += [("affine_prelu.slope", lambda b=b: ops.affine_prelu(x, sc, sh, b)), ("affine_prelu_bwd.slope", lambda b=b: ops.affine_prelu_bwd(x, x, sc, sh, b)),
                  ("se_residual_prelu.slope", lambda b=b: ops.se_residual_prelu(x, se, x, b)),
                  ("se_gate_grad.slope", lambda b=b: ops.se_gate_grad(x, se, x, b, x)),
                  ("se_residual_prelu_bwd.slope", lambda b=b: ops.se_residual_prelu_bwd(x, se, x, b, x))]
    calls += [("affine_prelu.shift", lambda: ops.affine_prelu(x, sc, None, sl)), ("affine_prelu.scale", lambda: ops.affine_prelu(x, None, sh, sl)),
              ("affine_prelu_bwd.shift", lambda: ops.affine_prelu_bwd(x, x, sc, None, sl)), ("affine_prelu_bwd.x", lambda: ops.affine_prelu_bwd(x, None, slope=sl)),
              ("se_residual_prelu.slope", lambda: ops.se_residual_prelu(x, se, x, None)), ("se_gate_grad.se_logits", lambda: ops.se_gate_grad(x, None, x, sl, x)),
              ("maxpool2x2.x", lambda: ops.maxpool2x2(odd_h)), ("maxpool2x2.x", lambda: ops.maxpool2x2(odd_w)),
              ("maxpool2x2_bwd.x", lambda: ops.maxpool2x2_bwd(odd_h, dyp[:, :1].contiguous())), ("maxpool2x2_bwd.x", lambda: ops.maxpool2x2_bwd(odd_w, dyp[:, :, :2].contiguous()))]
    for name, fn in calls:
        with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
            fn()
    # what the network calls
    row = torch.zeros((B, 8), dtype=torch.float16, device=dev)
    assert ops.affine_prelu(row, slope=sl).shape == row.shape and ops.affine_prelu_bwd(row, row, slope=sl).shape == row.shape
    assert ops.affine_prelu(x, sc, sh).shape == x.shape and ops.affine_prelu_bwd(x, None, sc, sh).shape == x.shape
    assert ops.maxpool2x2(x).shape == dyp.shape and ops.maxpool2x2_bwd(x, dyp).shape == x.shape and ops.global_avgpool(x).shape == se.shape
    assert ops.se_residual_prelu(x, se, x, sl).shape == x.shape and ops.se_residual_prelu(x, None, x, sl).shape == x.shape
    assert ops.se_gate_grad(x, se, x, sl, x).shape == se.shape
    assert ops.se_residual_prelu_bwd(x, se, x, sl, x, se)[0].shape == x.shape and ops.se_residual_prelu_bwd(x, None, x, sl, x)[1].shape == x.shape


# ----------------------------------------------------------------------------- 3. blocks against a decision-aligned fp64 reference
def _id(t):
    return t


def _r11(t):
    """Round to 11 significant bits (fp16's precision) without fp16's exponent limits."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


def _r16(t):
    return t.to(torch.float16).double()


def _bn_fold(sd, p, eps=1e-5):
    """eval-mode BatchNorm as y = x * s + t, in fp32 like the pack."""
    s = sd[p + "weight"].float() / torch.sqrt(sd[p + "running_var"].float() + eps)
    return s, sd[p + "bias"].float() - sd[p + "running_mean"].float() * s


def _conv_fold(sd, conv, bn):
    """The following BatchNorm folded into the filter in fp32, the filter rounded to fp16, the bias kept in fp32."""
    s, t = _bn_fold(sd, bn)
    return _r16(sd[conv + "weight"].float() * s[:, None, None, None]), t.double()


def _block_params(sd, p, stride, use_se):
    from types import SimpleNamespace
    s0, t0 = _bn_fold(sd, p + "bn0.")
    W = SimpleNamespace(stride=stride, se=use_se, s0=s0.double()[None, :, None, None], t0=t0.double()[None, :, None, None],
                        sl=sd[p + "prelu.weight"].double(), wd=None, bd=None)
    W.w1, W.b1 = _conv_fold(sd, p + "conv1.", p + "bn1.")
    W.w2, W.b2 = _conv_fold(sd, p + "conv2.", p + "bn2.")
    if p + "downsample.0.weight" in sd:
        W.wd, W.bd = _conv_fold(sd, p + "downsample.0.", p + "downsample.1.")
    if use_se:
        W.f0, W.fb0 = _r16(sd[p + "se.fc.0.weight"].float()), sd[p + "se.fc.0.bias"].double()
        W.f2, W.fb2 = _r16(sd[p + "se.fc.2.weight"].float()), sd[p + "se.fc.2.bias"].double()
        W.sl_se = sd[p + "se.fc.1.weight"].double()
    return W


def _se_fwd(W, c2, rnd=_id, ms=None):
    """SEBlock up to the gate logits: (hidden pre-activation s, logits)."""
    s = rnd(rnd(c2.mean(dim=(2, 3))) @ W.f0.t() + W.fb0)
    ms = (s > 0) if ms is None else ms
    return s, rnd(rnd(torch.where(ms, s, s * W.sl_se)) @ W.f2.t() + W.fb2)


def _se_bwd(W, ms, dgl, rnd=_id):
    """Gradient of the pooled input from the gradient of the logits."""
    t = rnd(dgl @ W.f2)
    return rnd(rnd(torch.where(ms, t, t * W.sl_se)) @ W.f0)


def _block_fwd(W, x, rnd=_id, masks=None):
    """IRBlock on NCHW fp64; rnd is applied wherever the HIP path stores fp16.  masks: the PReLU decisions (default: the evaluation's own)."""
    from types import SimpleNamespace
    A = SimpleNamespace(x=x, s=None, gates=None)
    A.c1 = rnd(F.conv2d(rnd(x * W.s0 + W.t0), W.w1, W.b1, 1, 1))
    m1 = (A.c1 > 0) if masks is None else masks.m1
    A.a1 = rnd(torch.where(m1, A.c1, A.c1 * W.sl))
    A.c2 = rnd(F.conv2d(A.a1, W.w2, W.b2, W.stride, 1))
    g = 1.0
    if W.se:
        A.s, A.gates = _se_fwd(W, A.c2, rnd, None if masks is None else masks.ms)
        g = torch.sigmoid(A.gates)[:, :, None, None]
    A.res = x if W.wd is None else rnd(F.conv2d(x, W.wd, W.bd, W.stride, 0))
    A.pre = A.c2 * g + A.res
    m2 = (A.pre > 0) if masks is None else masks.m2
    A.y = rnd(torch.where(m2, A.pre, A.pre * W.sl))
    return A


def _masks_of(W, A):
    """The PReLU decisions of the backward kernels, from stored activations (host arithmetic, fp64)."""
    from types import SimpleNamespace
    g = torch.sigmoid(A.gates)[:, :, None, None] if W.se else 1.0
    return SimpleNamespace(m1=A.c1 > 0, ms=(A.s > 0) if W.se else None, m2=(A.c2 * g + A.res) > 0)


def _block_bwd(W, A, M, dy, rnd=_id):
    """The vector-Jacobian product of ``_block_fwd`` at activations A under decisions M -> (dx, d(logits) / HW), in hip_bwd's order."""
    from torch.nn.grad import conv2d_input
    dpre = torch.where(M.m2, dy, dy * W.sl)
    dgl = None
    if W.se:
        g = torch.sigmoid(A.gates)
        dgl = rnd(g * (1 - g) * (dpre * A.c2).mean(dim=(2, 3)))
        dc2 = rnd(dpre * g[:, :, None, None] + _se_bwd(W, M.ms, dgl, rnd)[:, :, None, None])
    else:
        dc2 = rnd(dpre)
    dres = rnd(dpre)
    da = rnd(conv2d_input(A.c1.shape, W.w2, dc2, stride=W.stride, padding=1))
    dc1 = rnd(torch.where(M.m1, da, da * W.sl))
    dx = rnd(rnd(conv2d_input(A.x.shape, W.w1, dc1, stride=1, padding=1)) * W.s0)
    if W.wd is not None:
        dres = rnd(conv2d_input(A.x.shape, W.wd, dres, stride=W.stride, padding=0))
    return rnd(dx + dres), dgl


def _err(got, ref):
    d = got - ref
    return float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max())


def _within(what, got, ref, emu, report):
    """got against ref: rel-L2 and largest error at most twice those of the 11-bit-storage evaluation ``emu``."""
    (gr, gm), (er, em) = _err(got, ref), _err(emu, ref)
    print(f"{what}: rel-L2 {gr:.3e} max {gm:.3e}   11-bit storage on the CPU: {er:.3e} / {em:.3e}   bound {2 * er:.3e} / {2 * em:.3e}")
    report.append((what, gr, gm, er, em))
    return gr <= 2 * er and gm <= 2 * em


def _pair_check(what, W, x, dy, D, dx, dgl):
    """One block: D (activations), dx, dgl from the device against the fp64 reference, bounds from the 11-bit-storage evaluation."""
    R, E = _block_fwd(W, x), _block_fwd(W, x, _r11)
    report, ok = [], True
    for k in ("c1", "c2", "res", "y") + (("s", "gates") if W.se else ()):
        ok &= _within(f"{what} {k}", getattr(D, k), getattr(R, k), getattr(E, k), report)
    # decisions: the device's may differ from the reference's only inside the forward bound of the pre-activation
    MR, MD, ME = _masks_of(W, R), _masks_of(W, D), _masks_of(W, E)
    n_dis = n_all = 0
    for k, pre_r, pre_e in (("m1", R.c1, E.c1), ("m2", R.pre, E.pre)) + ((("ms", R.s, E.s),) if W.se else ()):
        dis = getattr(MR, k) != getattr(MD, k)
        n_dis, n_all = n_dis + int(dis.sum()), n_all + dis.numel()
        assert bool((pre_r[dis].abs() <= 2 * float((pre_e - pre_r).abs().max())).all()), (what, k)
    print(f"{what}: {n_dis} of {n_all} decisions differ from the reference's")
    assert n_dis <= 1e-3 * n_all, (what, n_dis, n_all)
    # backward: each evaluation against the reference's vector-Jacobian product under that evaluation's own decisions
    ref_d, ref_dgl_d = _block_bwd(W, R, MD, dy)
    ref_e, ref_dgl_e = _block_bwd(W, R, ME, dy)
    emu_dx, emu_dgl = _block_bwd(W, E, ME, dy, _r11)
    (gr, gm), (er, em) = _err(dx, ref_d), _err(emu_dx, ref_e)
    print(f"{what} dx: rel-L2 {gr:.3e} max {gm:.3e}   11-bit storage on the CPU: {er:.3e} / {em:.3e}   bound {2 * er:.3e} / {2 * em:.3e}")
    ok &= gr <= 2 * er and gm <= 2 * em
    if W.se:
        (gr, gm), (er, em) = _err(dgl, ref_dgl_d), _err(emu_dgl, ref_dgl_e)
        print(f"{what} dgl: rel-L2 {gr:.3e} max {gm:.3e}   11-bit storage on the CPU: {er:.3e} / {em:.3e}   bound {2 * er:.3e} / {2 * em:.3e}")
        ok &= gr <= 2 * er and gm <= 2 * em
    return ok


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=torch.float16)


def _nchw(t):
    return t.cpu().double().permute(0, 3, 1, 2)


def _device_block(dev, blk, P, Pb, W, x, dy):
    """hip_train / hip_bwd (and af_se_gate_grad on the same operands) -> host fp64 NCHW activations, dx, dgl."""
    from types import SimpleNamespace
    from adaface_dev_amd import ops
    y, (c1, c2, gates, res, s, _) = sv = blk.hip_train(_nhwc(x, dev), P)
    dyd = _nhwc(dy, dev)
    dgl = ops.se_gate_grad(c2, gates, res, blk.prelu.weight, dyd).cpu() if blk.use_se else None
    dx = blk.hip_bwd(sv[1], dyd, P, Pb)
    D = SimpleNamespace(x=x, c1=_nchw(c1), c2=_nchw(c2), res=_nchw(res), y=_nchw(y), s=None, gates=None)
    if blk.use_se:
        hid = W.f0.shape[0]
        assert bool((s[:, hid:] == 0).all())               # the zero-padded hidden units
        D.s, D.gates = s[:, :hid].cpu().double(), gates.cpu().double()
    return D, _nchw(dx), None if dgl is None else dgl.double()


def _make_block(dev, inplanes, planes, stride, use_se, seed):
    from adaface_dev_amd import rng
    from adaface_dev_amd.evaluation.arcface_resnet import IRBlock
    down = None
    if stride != 1 or inplanes != planes:
        down = nn.Sequential(nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(planes))
    blk = IRBlock(inplanes, planes, stride, down, use_se=use_se).eval()
    sd = rng.synth_face_state_dict(blk.state_dict(), seed=seed)
    blk.load_state_dict(sd)
    return blk.to(dev), _block_params(sd, "", stride, use_se)


BLOCK_CASES = {"64_16x16": (64, 64, 1, 16, 16), "64_15x17": (64, 64, 1, 15, 17), "64_to_128_stride2": (64, 128, 2, 16, 16)}


@pytest.mark.parametrize("use_se", [True, False])
@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_ir_block_pair_vs_decision_aligned_fp64(dev, name, use_se):
    """IRBlock.hip_train / hip_bwd with the real slopes: y, every saved activation and dx within twice the error of 11-bit storage (printed per
    tensor).  64 planes give the SE hidden width 4 zero-padded to 8, 128 planes a hidden width of 8; 15 x 17 leaves partial tiles.
    dx, rel-L2 / largest error, 11-bit storage on the CPU (the bound is twice that) | worst seen on the MI355X:
        64, 16 x 16        SE 2.65e-4 / 1.75e-3 | 2.64e-4 / 1.75e-3      no SE 3.10e-4 / 1.88e-3 | 3.11e-4 / 1.88e-3
        64, 15 x 17        SE 2.65e-4 / 1.51e-3 | 2.65e-4 / 1.51e-3      no SE 3.12e-4 / 2.46e-3 | 3.13e-4 / 2.46e-3
        64 -> 128, stride 2   SE 3.22e-4 / 2.08e-3 | 3.21e-4 / 2.08e-3      no SE 3.37e-4 / 1.89e-3 | 3.37e-4 / 1.89e-3
    y: at most 3.55e-4 / 2.5e-3 | 3.56e-4 / 2.5e-3; the SE logits 4.2e-4 | 4.1e-4.  3 to 7 of ~65,000 decisions differ from the reference's
    (1.1e-4 at most)."""
    inpl, planes, stride, H, Wd = BLOCK_CASES[name]
    blk, W = _make_block(dev, inpl, planes, stride, use_se, seed=61)
    g = _gen("block", name)
    x = _h((2, inpl, H, Wd), g).double()
    dy = _h((2, planes, (H - 1) // stride + 1, (Wd - 1) // stride + 1), g).double()
    # the restatement's own backward against autograd through its forward
    xr = x.clone().requires_grad_(True)
    R = _block_fwd(W, xr)
    (auto,) = torch.autograd.grad(R.y, xr, dy)
    R = _block_fwd(W, x)
    assert _err(_block_bwd(W, R, _masks_of(W, R), dy)[0], auto)[0] < 1e-12
    D, dx, dgl = _device_block(dev, blk, blk.pack(dev), blk.pack_bwd(dev), W, x, dy)
    assert _pair_check(f"IRBlock {name} se={use_se}", W, x, dy, D, dx, dgl)


@pytest.mark.parametrize("C", [64, 128])
def test_se_block_logits_pair_vs_fp64(dev, C):
    """SEBlock.logits / logits_bwd alone at the hidden widths 4 (zero-padded to 8) and 8.  Gradient of the pooled input, rel-L2 / largest
    error, 11-bit storage on the CPU | MI355X: C = 64 2.73e-4 / 3.68e-5 | the same; C = 128 3.53e-4 / 4.68e-5 | the same."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.evaluation.arcface_resnet import SEBlock
    se = SEBlock(C).eval()
    sd = rng.synth_face_state_dict(se.state_dict(), seed=62)
    se.load_state_dict(sd)
    se = se.to(dev)
    W = _block_params({**{"se." + k: v for k, v in sd.items()}, **_DUMMY_BLOCK(C)}, "", 1, True)
    g = _gen("seblock", C)
    x, dgl = _h((2, C, 5, 7), g).double(), _h((2, C), g, 0.05).double()
    keep = []
    gates = se.logits(_nhwc(x, dev), se.pack(dev), keep)
    dpool = se.logits_bwd(dgl.to(device=dev, dtype=torch.float16), keep[0], se.pack_bwd(dev))
    hid = W.f0.shape[0]
    assert bool((keep[0][:, hid:] == 0).all())
    s_d = keep[0][:, :hid].cpu().double()
    (s_r, gates_r), (s_e, gates_e) = _se_fwd(W, x), _se_fwd(W, x, _r11)
    report = []
    ok = _within(f"SEBlock {C} s", s_d, s_r, s_e, report) & _within(f"SEBlock {C} logits", gates.cpu().double(), gates_r, gates_e, report)
    dis = (s_d > 0) != (s_r > 0)
    assert bool((s_r[dis].abs() <= 2 * float((s_e - s_r).abs().max())).all())
    ok &= _within(f"SEBlock {C} dpool", dpool.cpu().double(), _se_bwd(W, s_d > 0, dgl), _se_bwd(W, s_d > 0, dgl, _r11), report)
    assert ok


def _DUMMY_BLOCK(C):
    """The entries of a block's state dict ``_block_params`` reads besides the SE ones (unused by the SE-only test)."""
    bn = lambda p: {p + "weight": torch.ones(C), p + "bias": torch.zeros(C), p + "running_mean": torch.zeros(C), p + "running_var": torch.ones(C)}
    return {**bn("bn0."), **bn("bn1."), **bn("bn2."), "conv1.weight": torch.zeros(C, C, 3, 3), "conv2.weight": torch.zeros(C, C, 3, 3),
            "prelu.weight": torch.full((1,), 0.25)}


# ----------------------------------------------------------------------------- 3. stem and head
def _stem_params(sd):
    from types import SimpleNamespace
    S = SimpleNamespace(sl=sd["prelu.weight"].double())
    S.w, S.b = _conv_fold(sd, "conv1.", "bn1.")
    return S


def _pool_idx(a1):
    """torch's argmax of every 2x2 window: the first maximum."""
    return F.max_pool2d(a1.detach(), 2, 2, return_indices=True)[1]


def _stem_fwd(S, x, rnd=_id, m=None, idx=None):
    """conv1 (+ bn1), PReLU, 2x2 max-pool; m / idx: the PReLU decisions and the pool's argmax (default: the evaluation's own)."""
    from types import SimpleNamespace
    A = SimpleNamespace(x=x)
    A.c1 = rnd(F.conv2d(x, S.w, S.b, 1, 1))
    A.a1 = rnd(torch.where((A.c1 > 0) if m is None else m, A.c1, A.c1 * S.sl))
    idx = _pool_idx(A.a1) if idx is None else idx
    A.h = A.a1.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    return A


def _stem_bwd(S, A, m, idx, dh, rnd=_id):
    from torch.nn.grad import conv2d_input
    da1 = torch.zeros_like(A.a1).flatten(2).scatter(2, idx.flatten(2), dh.flatten(2)).view(A.a1.shape)
    return rnd(conv2d_input(A.x.shape, S.w, rnd(torch.where(m, da1, da1 * S.sl)), stride=1, padding=1))


def _stem_check(what, S, x, dh, D, dx):
    R, E = _stem_fwd(S, x), _stem_fwd(S, x, _r11)
    report, ok = [], True
    for k in ("c1", "a1", "h"):
        ok &= _within(f"{what} {k}", getattr(D, k), getattr(R, k), getattr(E, k), report)
    dis = (R.c1 > 0) != (D.c1 > 0)
    assert bool((R.c1[dis].abs() <= 2 * float((E.c1 - R.c1).abs().max())).all()) and int(dis.sum()) <= 1e-3 * dis.numel()
    # the pool may pick another pixel only where the reference's two candidates lie within twice the forward bound of each other
    iR, iD, iE = _pool_idx(R.a1), _pool_idx(D.a1), _pool_idx(E.a1)
    flat = R.a1.flatten(2)
    gap = (flat.gather(2, iR.flatten(2)) - flat.gather(2, iD.flatten(2))).abs()
    print(f"{what}: {int(dis.sum())} of {dis.numel()} PReLU decisions and {int((iR != iD).sum())} of {iR.numel()} pool choices differ from the reference's")
    assert float(gap.max()) <= 4 * float((E.a1 - R.a1).abs().max())
    (gr, gm) = _err(dx, _stem_bwd(S, R, D.c1 > 0, iD, dh))
    (er, em) = _err(_stem_bwd(S, E, E.c1 > 0, iE, dh, _r11), _stem_bwd(S, R, E.c1 > 0, iE, dh))
    print(f"{what} dx: rel-L2 {gr:.3e} max {gm:.3e}   11-bit storage on the CPU: {er:.3e} / {em:.3e}   bound {2 * er:.3e} / {2 * em:.3e}")
    return ok and gr <= 2 * er and gm <= 2 * em


def _device_stem(dev, m, P, Pb, x, dh):
    from types import SimpleNamespace
    from adaface_dev_amd import ops
    c1 = ops.conv3x3(ops.nchw_f32_to_nhwc_f16(x.float().contiguous().to(dev), cpad=8), P["conv1"])
    a1 = ops.affine_prelu(c1, slope=m.prelu.weight)
    h = ops.maxpool2x2(a1)
    dc1 = ops.affine_prelu_bwd(ops.maxpool2x2_bwd(a1, _nhwc(dh, dev)), c1, slope=m.prelu.weight)
    dx = ops.nhwc_f16_to_nchw_f32(ops.conv3x3(dc1, Pb["conv1"]), 1)
    return SimpleNamespace(x=x, c1=_nchw(c1), a1=_nchw(a1), h=_nchw(h)), dx.cpu().double()


def _head_params(sd):
    """bn4 . flatten . fc5 . bn5 as one matrix on NHWC-ordered columns, folded in fp32 and rounded to fp16 like the pack."""
    s4, t4 = _bn_fold(sd, "bn4.")
    s5, t5 = _bn_fold(sd, "bn5.")
    w5 = sd["fc5.weight"].float().reshape(512, 512, 8, 8)
    b5 = sd["fc5.bias"].float() + (w5 * t4[None, :, None, None]).sum(dim=(1, 2, 3))
    w5 = (w5 * s4[None, :, None, None]).permute(0, 2, 3, 1).reshape(512, 8 * 8 * 512)
    return _r16(w5 * s5[:, None]), (b5 * s5 + t5).double()


def _head_fwd(Hd, h, rnd=_id):
    """h NCHW [B, 512, 8, 8] -> embeddings [B, 512]."""
    return rnd(h.permute(0, 2, 3, 1).reshape(h.shape[0], -1) @ Hd[0].t() + Hd[1])


def _head_bwd(Hd, dy, rnd=_id):
    return rnd(dy @ Hd[0]).reshape(dy.shape[0], 8, 8, 512).permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------- 4. the walk at the magnitudes it really has
def _loss(emb, target):
    return (1 - F.cosine_similarity(emb, target, dim=-1)).sum() + 1e-3 * (emb ** 2).mean()


def _walk_state():
    """resnet_face18(use_se=True) on [2, 1, 128, 128] once in fp64: every block's input, the gradient of the cosine + L2 loss at every block
    output, and the power of two FaceEncodeFn.backward scales the incoming gradient by."""
    from types import SimpleNamespace
    from adaface_dev_amd import rng
    from adaface_dev_amd.evaluation.arcface_resnet import resnet_face18
    m = resnet_face18(use_se=True).eval()
    sd = rng.synth_face_state_dict(m.state_dict(), seed=50)
    m.load_state_dict(sd)
    K = SimpleNamespace(m=m, sd=sd, x=_r16(rng.synth_input("face.gx", (2, 1, 128, 128), seed=58)),
                        target=F.normalize(rng.synth_input("face.gt", (2, 512), seed=58), dim=-1).double())
    K.S, K.Hd = _stem_params(sd), _head_params(sd)
    K.Ws = [_block_params(sd, f"layer{li}.{bi}.", 2 if (li > 1 and bi == 0) else 1, True) for li in range(1, 5) for bi in range(2)]
    with torch.enable_grad():
        xr = K.x.clone().requires_grad_(True)
        hs = [_stem_fwd(K.S, xr).h]
        for W in K.Ws:
            hs.append(_block_fwd(W, hs[-1]).y)
        emb = _head_fwd(K.Hd, hs[-1])
        for t in hs + [emb]:
            t.retain_grad()
        _loss(emb, K.target).backward()
    K.h, K.G, K.emb, K.dE, K.dx = [t.detach() for t in hs], [t.grad for t in hs], emb.detach(), emb.grad, xr.grad
    K.scale = float(torch.exp2(torch.floor(torch.log2(256.0 / K.dE.abs().amax()))))
    return K


@pytest.fixture(scope="module")
def walk():
    return _walk_state()


@pytest.fixture(scope="module")
def net(dev, walk):
    m = walk.m.to(dev)
    return m, m._prepared(), m._prepared_bwd()


def _low_share(t):
    """Share of an fp16 tensor's entries that are zero or subnormal."""
    return float((t.abs() < TINY).double().mean())


def test_stem_and_head_pairs_vs_fp64(dev, walk, net):
    """The stem (conv1 + bn1, PReLU, 2x2 max-pool) on a non-square image and the head (bn4 . flatten . fc5 . bn5 as one GEMM), forward and
    backward, with N(0, 1) gradients.  rel-L2 / largest error, 11-bit storage on the CPU | MI355X: stem dx 1.91e-4 / 3.89e-3 | the same (1
    of 10,240 pool choices differs); head y 2.07e-4 / 1.05e-3 | 2.07e-4 / 1.05e-3; head dh 2.07e-4 / 2.44e-4 | 2.08e-4 / 2.44e-4."""
    from adaface_dev_amd import ops
    m, P, Pb = net
    g = _gen("stem")
    x, dh = _h((2, 1, 16, 20), g).double(), _h((2, 64, 8, 10), g).double()
    D, dx = _device_stem(dev, m, P, Pb, x, dh)
    assert _stem_check("stem 16x20", walk.S, x, dh, D, dx)
    h, dy = _h((2, 512, 8, 8), g).double(), _h((2, 512), g).double()
    y = ops.gemm(_nhwc(h, dev).reshape(2, 8 * 8 * 512), P["fc5"])
    dhd = ops.gemm(dy.to(device=dev, dtype=torch.float16), Pb["fc5"]).reshape(2, 8, 8, 512)
    report = []
    ok = _within("head y", y.cpu().double(), _head_fwd(walk.Hd, h), _head_fwd(walk.Hd, h, _r11), report)
    ok &= _within("head dh", _nchw(dhd), _head_bwd(walk.Hd, dy), _head_bwd(walk.Hd, dy, _r11), report)
    assert ok


@pytest.mark.parametrize("i", range(8))
def test_walk_block_at_its_real_gradient(dev, walk, net, i):
    """Block i of resnet_face18(use_se=True) on the reference's own input (rounded to fp16) with the gradient the real walk hands it,
    half(s * G_i), s the power of two FaceEncodeFn.backward picks: dx against s * the decision-aligned fp64 gradient, bound as in section 3.
    Prints the share of the incoming gradient and of af_se_gate_grad's output that is zero or subnormal in fp16.
    Measured on the MI355X: s = 2^14, max |half(s G_i)| 23 to 30 at every block; zero or subnormal 0 to 3e-4 of half(s G_i) and 1 to 3
    ENTRIES of af_se_gate_grad's output per block (its largest entry 8.6e-3 at the 64 x 64 level to 0.54 at 8 x 8, fp16's smallest normal
    number is 6.1e-5): the fp16 dgl / HW does not underflow on a real walk, and no block misses the bound.
    dx, rel-L2 / largest error, 11-bit storage on the CPU | MI355X, blocks 0 to 7:
        2.60e-4 / 8.37e-3 | 2.60e-4 / 8.37e-3      2.60e-4 / 8.17e-3 | 2.60e-4 / 8.17e-3      3.18e-4 / 1.29e-2 | 3.18e-4 / 1.29e-2
        2.60e-4 / 7.91e-3 | 2.60e-4 / 7.91e-3      3.15e-4 / 1.40e-2 | 3.16e-4 / 1.40e-2      2.50e-4 / 7.99e-3 | 2.50e-4 / 8.82e-3
        3.18e-4 / 1.57e-2 | 3.17e-4 / 1.57e-2      2.53e-4 / 9.92e-3 | 2.53e-4 / 1.02e-2
    af_se_gate_grad's output: 3.8e-4 to 4.7e-4 rel-L2 on both sides.  4 to 63 decisions per block differ (6e-5 of them at most)."""
    m, P, Pb = net
    W, blk = walk.Ws[i], list(m.blocks())[i]
    x, dy = _r16(walk.h[i]), _r16(walk.scale * walk.G[i + 1])
    D, dx, dgl = _device_block(dev, blk, P["blocks"][i], Pb["blocks"][i], W, x, dy)
    print(f"walk block {i}: s = {walk.scale:g}, max |half(s G)| {float(dy.abs().max()):.3e}, zero or subnormal: {_low_share(dy):.4f} of half(s G), "
          f"{_low_share(dgl):.4f} of af_se_gate_grad's output (largest {float(dgl.abs().max()):.3e})")
    assert _pair_check(f"walk block {i}", W, x, dy, D, dx, dgl)


def test_walk_stem_at_its_real_gradient(dev, walk, net):
    """The stem on the network's input with half(s * G_0), the gradient at the max-pool's output (2e-4 of it zero or subnormal).  dx, rel-L2 /
    largest error: 11-bit storage on the CPU 2.12e-4 / 1.39e-2, the MI355X the same; 77 of 524,288 pool choices differ from the reference's, each
    between two candidates closer than the forward bound allows to tell apart."""
    m, P, Pb = net
    dh = _r16(walk.scale * walk.G[0])
    print(f"walk stem: zero or subnormal: {_low_share(dh):.4f} of half(s G)")
    D, dx = _device_stem(dev, m, P, Pb, walk.x, dh)
    assert _stem_check("walk stem", walk.S, walk.x, dh, D, dx)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_face_encode_fn_is_the_chained_blocks(dev, walk, net, dt):
    """FaceEncodeFn end to end: its input gradient is, bit for bit, the head, the eight hip_bwd and the stem chained on the scaled fp16 gradient and
    unscaled; an all-zero dy gives an all-zero finite gradient; a second backward raises."""
    from adaface_dev_amd import ops
    m, P, Pb = net
    target = walk.target.to(dev).float()
    xd = walk.x.to(dev).to(dt).requires_grad_(True)
    emb = m(xd)
    seen = []
    emb.register_hook(lambda gr: seen.append(gr.detach().clone()))
    _loss(emb.float(), target).backward()
    assert emb.dtype == dt and xd.grad.dtype == dt and len(seen) == 1
    y, (c1, a1, saved) = m.hip_train(xd.detach())
    assert torch.equal(y if dt == torch.float16 else y.to(dt), emb.detach())
    dy = seen[0]
    scale = torch.exp2(torch.floor(torch.log2(256.0 / dy.abs().amax().float())))
    assert dt == torch.float16 or float(scale) == walk.scale              # (an fp16 caller's dy is rounded before the scale is chosen)
    dh = ops.gemm((dy.float() * scale).to(torch.float16).contiguous(), Pb["fc5"]).reshape(2, 8, 8, 512)
    for blk, bp, bpb, sv in reversed(list(zip(m.blocks(), P["blocks"], Pb["blocks"], saved))):
        dh = blk.hip_bwd(sv, dh, bp, bpb)
    dc1 = ops.affine_prelu_bwd(ops.maxpool2x2_bwd(a1, dh), c1, slope=m.prelu.weight)
    want = (ops.nhwc_f16_to_nchw_f32(ops.conv3x3(dc1, Pb["conv1"]), 1) / scale).to(dt)
    assert torch.equal(xd.grad, want)
    assert float(xd.grad.float().abs().max()) > 0
    x2 = walk.x.to(dev).to(dt).requires_grad_(True)
    e2 = m(x2)
    e2.backward(torch.zeros_like(e2), retain_graph=True)
    assert bool(torch.isfinite(x2.grad).all()) and bool((x2.grad == 0).all())
    with pytest.raises(RuntimeError, match="second backward"):
        e2.backward(torch.ones_like(e2))
    assert all(p.grad is None for p in m.parameters())
