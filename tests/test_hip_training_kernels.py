"""Training-path kernels on a real MI355X, kernel by kernel.  `pytest -m gpu`.

A. The attention forward's log-sum-exp and `af_attention_bwd` in the call forms the trainers use -- operands that are column
   slices of ONE packed fp16 buffer, gradients written into column slices of ONE buffer, the causal predicate `j // m <= i`,
   key masks with an entirely masked first stage and with an entirely masked batch item -- against one fp64 autograd
   reference on the fp16-rounded operands.  Bounds: o rel-L2 < 3e-3 (one fp16 rounding of the output), dq / dk / dv each
   rel-L2 < 5e-3 (P and dz are rounded to fp16 before the second MFMA product: test_hip_backward_ops.py), lse max |error|
   < 2e-3 in base-2 units: the kernels that sum fp16-rounded P through the ones row carry at most 2^-11 relative error per
   term, log2(1 + 2^-11) = 7e-4, with the fp32 accumulation and the hardware exp2 / log2 on top (about 3x the derived term).
   Worst lse error measured on MI355X: 1.09e-3, general kernel, packed qkv causal (1, 40, 2, 8); the other cases of the general
   kernel 3.0e-4 .. 6.3e-4, short-key kernel 4.2e-4, two-chain kernel 3.5e-4.  The d = 8 figure is above the derived 7e-4 because
   the forward kernels also round q * scale * log2(e) to fp16 before the score product (up to 2^-11 of each |q_c k_c| term of a
   score); rows of a causal case that see one or two keys do not average that out.
B. The small element-wise / gather kernels of the training path that had no test of their own, against plain torch on the
   same inputs (bit-equal where the kernel does one rounding of an exactly representable fp32 expression)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 3e-3            # o: one fp16 rounding of the output
GRAD_TOL = 5e-3       # dq, dk, dv (docstring of test_hip_backward_ops.py)
LSE_TOL = 2e-3        # base-2 units, derived above
ELEM_TOL = 6e-4       # one fp16 rounding of an element-wise result (test_hip_capture_graph.py)
LN2 = math.log(2.0)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16)


# ----------------------------------------------------------------------------------------------------------- reference
def ref_attention(q, k, v, do, heads, keymask=None, causal_m=0):
    """fp64 autograd on the CPU.  q, do [B, Nq, C], k, v [B, L, C] (fp16-rounded values); keymask bool [B, L] (True = keep) or
    None; causal_m > 0: key j visible to query i iff j // causal_m <= i.  Returns o [B, Nq, C], the natural-log lse of the
    filled scores [B, heads, Nq] and dq, dk, dv for the output gradient `do`."""
    B, Nq, C = q.shape
    L, d = k.shape[1], C // heads
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    split = lambda t, n: t.reshape(B, n, heads, d).permute(0, 2, 1, 3)
    score = d ** -0.5 * (split(qd, Nq) @ split(kd, L).transpose(-1, -2))            # [B, heads, Nq, L]
    visible = torch.ones(B, Nq, L, dtype=torch.bool)
    if keymask is not None:
        visible &= keymask[:, None, :]
    if causal_m:
        visible &= (torch.arange(L)[None, :] // causal_m <= torch.arange(Nq)[:, None])[None]
    score = score.masked_fill(~visible[:, None], -torch.finfo(score.dtype).max)
    lse = torch.logsumexp(score, dim=-1)
    o = (torch.softmax(score, dim=-1) @ split(vd, L)).permute(0, 2, 1, 3).reshape(B, Nq, C)
    o.backward(do.double())
    return o.detach(), lse.detach(), qd.grad, kd.grad, vd.grad


def make_mask(kind, B, L):
    """None | 'half0': item 0 has its FIRST L/2 keys masked (the first 32-key stage -- at L = 96 also the forward's first 64-key
    stage half -- is entirely masked, a later one is not) | 'dead0': item 0 has EVERY key masked.  Other items: ~30 % masked."""
    if kind is None:
        return None
    mask = torch.rand(B, L, generator=torch.Generator().manual_seed(9)) > 0.3
    mask[0] = False
    if kind == "half0":
        mask[0, L // 2:] = True
    return mask


@functools.lru_cache(maxsize=None)
def problem(B, Nq, L, heads, d, mask_kind=None, causal_m=0):
    """Operands (fp16, CPU) and their fp64 reference, computed once per shape and shared by the tests that use it."""
    C = heads * d
    q, k, v, do = rnd((B, Nq, C), 1), rnd((B, L, C), 2), rnd((B, L, C), 3), rnd((B, Nq, C), 4)
    mask = make_mask(mask_kind, B, L)
    return (q, k, v, do, mask) + ref_attention(q, k, v, do, heads, mask, causal_m)


# ------------------------------------------------------------------------------------------------------------- runners
def run_packed_qkv(dev, q, k, v, do, mask, heads, causal_m, spare=0):
    """Self-attention on ONE packed [B*N, 3C (+ spare)] buffer, as CrossAttention.hip_train / hip_bwd and AttentionQKVFn call it:
    q | k | v are column blocks (row stride 3C + spare), dq | dk | dv the column blocks of one gradient buffer."""
    from adaface_dev_amd import ops
    B, N, C = q.shape
    d, ld = C // heads, 3 * C + spare
    qkv = torch.full((B * N, ld), NAN, dtype=torch.float16)          # spare columns hold NaN: reading them poisons the result
    qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C] = q.reshape(B * N, C), k.reshape(B * N, C), v.reshape(B * N, C)
    qkv = qkv.to(dev)
    kb = None if mask is None else ops.make_keybias(mask.to(dev), N)
    vt = ops.transpose_tokens(qkv[:, 2 * C:], B, N, C, ld)
    o, lse = ops.attention(qkv, qkv[:, C:], vt, B=B, Nq=N, L=N, heads=heads, d=d, ldq=ld, ldk=ld, keybias=kb, want_lse=True,
                           causal_m=causal_m)
    dqkv = torch.empty_like(qkv)                                      # NaN-poisoned by conftest: finite afterwards == written
    dqkv[:, 3 * C:] = 7.0
    ops.attention_bwd(qkv, qkv[:, C:], qkv[:, 2 * C:], o, do.reshape(B * N, C).to(dev), lse, B=B, Nq=N, L=N, heads=heads, d=d,
                      ldq=ld, ldk=ld, ldv=ld, dq=dqkv, dk=dqkv[:, C:], dv=dqkv[:, 2 * C:], lddq=ld, lddk=ld, lddv=ld, keybias=kb,
                      causal_m=causal_m)
    g = dqkv.cpu()
    assert torch.equal(g[:, 3 * C:], torch.full((B * N, spare), 7.0, dtype=torch.float16)), "spare gradient columns were written"
    return o.cpu(), lse.cpu(), g[:, :C], g[:, C:2 * C], g[:, 2 * C:3 * C]


def run_packed_kv(dev, q, k, v, do, heads, spare=0):
    """Cross-attention as CrossAttention.hip_train / hip_bwd call it: q [B*N, C]; k | v column blocks of one [B*L, 2C (+ spare)]
    buffer; dq its own tensor, dk | dv the column blocks of one [B*L, 2C (+ spare)] gradient buffer."""
    from adaface_dev_amd import ops
    B, N, C = q.shape
    L, d, ld = k.shape[1], C // heads, 2 * C + spare
    kv = torch.full((B * L, ld), NAN, dtype=torch.float16)
    kv[:, :C], kv[:, C:2 * C] = k.reshape(B * L, C), v.reshape(B * L, C)
    qd, kv = q.reshape(B * N, C).to(dev), kv.to(dev)
    vt = ops.transpose_tokens(kv[:, C:], B, L, C, ld)
    o, lse = ops.attention(qd, kv, vt, B=B, Nq=N, L=L, heads=heads, d=d, ldq=C, ldk=ld, want_lse=True)
    dq, dkv = torch.empty_like(qd), torch.empty_like(kv)
    dkv[:, 2 * C:] = 7.0
    ops.attention_bwd(qd, kv, kv[:, C:], o, do.reshape(B * N, C).to(dev), lse, B=B, Nq=N, L=L, heads=heads, d=d, ldq=C, ldk=ld,
                      ldv=ld, dq=dq, dk=dkv, dv=dkv[:, C:], lddq=C, lddk=ld, lddv=ld)
    g = dkv.cpu()
    assert torch.equal(g[:, 2 * C:], torch.full((B * L, spare), 7.0, dtype=torch.float16)), "spare gradient columns were written"
    return o.cpu(), lse.cpu(), dq.cpu(), g[:, :C], g[:, C:2 * C]


def run_multikey(dev, q, k, v, do, heads, m):
    """AttentionFn's form: q [B*T, E], k / v [B*T*m, E] contiguous (row stride E), L = T*m, causal_m = m."""
    from adaface_dev_amd import ops
    B, T, E = q.shape
    L, d = k.shape[1], E // heads
    qd, kd, vd = q.reshape(B * T, E).to(dev), k.reshape(B * L, E).to(dev), v.reshape(B * L, E).to(dev)
    vt = ops.transpose_tokens(vd, B, L, E, E)
    o, lse = ops.attention(qd, kd, vt, B=B, Nq=T, L=L, heads=heads, d=d, ldq=E, ldk=E, scale=d ** -0.5, want_lse=True, causal_m=m)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    ops.attention_bwd(qd, kd, vd, o, do.reshape(B * T, E).to(dev), lse, B=B, Nq=T, L=L, heads=heads, d=d, ldq=E, ldk=E, ldv=E,
                      dq=dq, dk=dk, dv=dv, lddq=E, lddk=E, lddv=E, scale=d ** -0.5, causal_m=m)
    return o.cpu(), lse.cpu(), dq.cpu(), dk.cpu(), dv.cpu()


def check(tag, got, ref, rows=None, lse_rows=None, kernel=None):
    """got = (o, lse2, dq, dk, dv) of the kernels (2-D token rows), ref = (o, lse, dq, dk, dv) of ref_attention; `rows` restricts
    the comparison to a list of batch items, `lse_rows` the lse comparison (a fully masked item has no meaningful lse)."""
    o, lse2, dq, dk, dv = got
    ro, rlse, rdq, rdk, rdv = ref
    B, Nq = ro.shape[0], ro.shape[1]
    rows = list(range(B)) if rows is None else rows
    lse_rows = rows if lse_rows is None else lse_rows
    errs = {}
    for name, g, r in (("o", o, ro), ("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        g = g.reshape(r.shape)
        assert bool(torch.isfinite(g).all()), (tag, name, "not every element was written / finite")
        errs[name] = rel_l2(g[rows].double().numpy(), r[rows].numpy())
    errs["lse"] = None
    if lse2 is not None and lse_rows:
        errs["lse"] = float((lse2[lse_rows, :, :Nq].double() - rlse[lse_rows] / LN2).abs().max())
    print(f"{tag}: o {errs['o']:.2e} dq {errs['dq']:.2e} dk {errs['dk']:.2e} dv {errs['dv']:.2e} "
          f"lse(base 2) {'-' if errs['lse'] is None else format(errs['lse'], '.2e')}" + (f" [{kernel} kernel]" if kernel else ""))
    assert errs["o"] < TOL, (tag, errs)
    for name in ("dq", "dk", "dv"):
        assert errs[name] < GRAD_TOL, (tag, name, errs)
    if errs["lse"] is not None:
        assert errs["lse"] < LSE_TOL, (tag, errs)
    return errs


# --------------------------------------------------------------------- A1. packed qkv, causal m = 1 (AttentionQKVFn's form)
QKV_CAUSAL = [(2, 77, 2, 64), (3, 22, 2, 64), (1, 40, 2, 8)]


@pytest.mark.parametrize("B,T,heads,d", QKV_CAUSAL)
def test_attention_packed_qkv_causal(dev, B, T, heads, d):
    """Row stride 3E, causal_m = 1 (the CLIP text transformer).  Forward: the general kernel (causal)."""
    q, k, v, do, _, *ref = problem(B, T, T, heads, d, None, 1)
    check(f"qkv-causal {B, T, heads, d}", run_packed_qkv(dev, q, k, v, do, None, heads, 1), ref, kernel="general")


@pytest.mark.parametrize("B,T,heads,d", QKV_CAUSAL)
def test_attention_qkv_autograd_node(dev, B, T, heads, d):
    """The same through AttentionQKVFn.apply + .backward: the node's own arguments (strides, causal_m = 1, transpose_tokens)."""
    from adaface_dev_amd.autograd_ops import AttentionQKVFn
    q, k, v, do, _, *ref = problem(B, T, T, heads, d, None, 1)
    E = heads * d
    qkv = torch.cat([q, k, v], -1).reshape(B * T, 3 * E).to(dev).requires_grad_(True)
    o = AttentionQKVFn.apply(qkv, B, T, heads, d ** -0.5, True)
    o.backward(do.reshape(B * T, E).to(dev))
    g = qkv.grad.cpu()
    check(f"AttentionQKVFn {B, T, heads, d}", (o.detach().cpu(), None, g[:, :E], g[:, E:2 * E], g[:, 2 * E:]), ref)


# ------------------------------------------------------------------------ A2. multi-key causal (AttentionFn's form)
# L = T*m; (2, 22, 4, ..): L = 88 and (1, 22, 3, ..): L = 66 leave the key count ragged over the 32-key (backward) and the 64-key (forward) stage
MULTIKEY = [(2, 77, 2, 2, 64), (2, 22, 4, 2, 64), (1, 22, 3, 1, 64)]


def multikey_problem(B, T, m, heads, d):
    """The m-aware reference; before any kernel runs, show that the case tells `j // m <= i` from `j <= i`."""
    q, k, v, do, _, *ref = problem(B, T, T * m, heads, d, None, m)
    o1, _, dq1, dk1, dv1 = problem(B, T, T * m, heads, d, None, 1)[5:]
    assert rel_l2(o1.numpy(), ref[0].numpy()) > 10 * TOL
    for a, b in ((dq1, ref[2]), (dk1, ref[3]), (dv1, ref[4])):
        assert rel_l2(a.numpy(), b.numpy()) > 10 * GRAD_TOL
    return q, k, v, do, ref


@pytest.mark.parametrize("B,T,m,heads,d", MULTIKEY)
def test_attention_multikey_causal(dev, B, T, m, heads, d):
    """q [B*T, E], k / v [B*T*m, E], causal_m = m (the Arc2Face text encoder's multi-key attention).  Forward: the general kernel."""
    q, k, v, do, ref = multikey_problem(B, T, m, heads, d)
    check(f"multikey-causal {B, T, m, heads, d}", run_multikey(dev, q, k, v, do, heads, m), ref, kernel="general")


@pytest.mark.parametrize("B,T,m,heads,d", MULTIKEY)
def test_attention_multikey_autograd_node(dev, B, T, m, heads, d):
    """The same through AttentionFn.apply + .backward: `m if causal else 0`, L = T*m, the strides."""
    from adaface_dev_amd.autograd_ops import AttentionFn
    q, k, v, do, ref = multikey_problem(B, T, m, heads, d)
    E, L = heads * d, T * m
    qd, kd, vd = (t.reshape(-1, E).to(dev).requires_grad_(True) for t in (q, k, v))
    o = AttentionFn.apply(qd, kd, vd, B, T, m, heads, d ** -0.5, True)
    o.backward(do.reshape(B * T, E).to(dev))
    check(f"AttentionFn {B, T, m, heads, d}", (o.detach().cpu(), None, qd.grad.cpu(), kd.grad.cpu(), vd.grad.cpu()), ref)


# ----------------------------------------------------------- A3. U-Net training self-attention: packed 3C, keybias, no causal
@pytest.mark.parametrize("B,N,heads,d", [(2, 96, 2, 40), (1, 72, 1, 160)])
def test_attention_packed_qkv_keybias(dev, B, N, heads, d):
    """Item 0 has its first N/2 keys masked (an entirely masked stage before a visible one), the other item ~30 % at random.
    Forward: the general kernel (keybias)."""
    q, k, v, do, mask, *ref = problem(B, N, N, heads, d, "half0", 0)
    check(f"qkv-keybias {B, N, heads, d}", run_packed_qkv(dev, q, k, v, do, mask, heads, 0), ref, kernel="general")


def test_attention_packed_qkv_two_chain_lse(dev):
    """Packed 3C, no mask, Nq = L = 512, d = 40: the forward's two-chain kernel writes the lse."""
    B, N, heads, d = 1, 512, 2, 40
    q, k, v, do, _, *ref = problem(B, N, N, heads, d, None, 0)
    check(f"qkv-plain {B, N, N, heads, d}", run_packed_qkv(dev, q, k, v, do, None, heads, 0), ref, kernel="two-chain")


# ------------------------------------------------------------------------------- A4. cross-attention: q at C, k | v at 2C
@pytest.mark.parametrize("B,N,L,heads,d", [(2, 100, 77, 2, 40), (1, 33, 20, 2, 80)])
def test_attention_cross_packed_kv(dev, B, N, L, heads, d):
    """Forward: the short-key kernel (no bias, not causal, L <= 128)."""
    q, k, v, do, _, *ref = problem(B, N, L, heads, d, None, 0)
    check(f"cross-kv {B, N, L, heads, d}", run_packed_kv(dev, q, k, v, do, heads), ref, kernel="short-key")


# ------------------------------------------------------------------------------------------ A5. a fully masked batch item
def test_attention_bwd_fully_masked_item(dev):
    """Every key of item 0 is masked: masked_fill(-finfo.max) semantics make its softmax uniform, so o = mean(v), dv = (1/L) sum_i dO_i
    and -- the fill cuts the score gradient -- dq = dk = 0 EXACTLY.  Item 1 (partly masked) is unaffected.
    Before the fix in af_attn_bwd.hip the backward recomputed p = exp2(t - lse) = exp2(-FLT_MAX + FLT_MAX) = 1 instead of 1/L for such
    rows; measured on MI355X for item 0: max|dq| = 45.0, max|dk| = 51.6, dv rel-L2 error 95.0 (dv = L times the reference).  With the
    fix: dq = dk = 0, dv error 3.6e-4."""
    B, N, heads, d = 2, 96, 2, 40
    q, k, v, do, mask, *ref = problem(B, N, N, heads, d, "dead0", 0)
    assert not bool(mask[0].any()) and bool(mask[1].any()) and not bool(mask[1].all())
    got = run_packed_qkv(dev, q, k, v, do, mask, heads, 0)
    o, dq, dk, dv = (t.reshape(B, N, -1) for t in (got[0], got[2], got[3], got[4]))
    for t in (o, dq, dk, dv):
        assert bool(torch.isfinite(t).all())
    mean_v = v[0].double().mean(0, keepdim=True).expand(N, -1)
    e_o = rel_l2(o[0].double().numpy(), mean_v.numpy())
    e_dv = rel_l2(dv[0].double().numpy(), ref[4][0].numpy())
    print(f"dead item: o vs mean(v) {e_o:.2e}  max|dq| {float(dq[0].abs().max()):.3e}  max|dk| {float(dk[0].abs().max()):.3e}  dv {e_dv:.3e}")
    assert float(ref[2][0].abs().max()) == 0 and float(ref[3][0].abs().max()) == 0          # the reference is exactly zero
    assert e_o < TOL
    assert float(dq[0].abs().max()) == 0 and float(dk[0].abs().max()) == 0
    assert e_dv < GRAD_TOL
    check("dead item's neighbour", got, ref, rows=[1], kernel="general")


# --------------------------------------------------------------------------------- A6. nothing outside the slices is written
def test_attention_bwd_writes_only_its_slices(dev):
    """Buffers 16 columns wider than needed (3E + 16, 2C + 16): the spare INPUT columns hold NaN (a read would poison a result), the
    spare GRADIENT columns a sentinel that must survive bit for bit (asserted in the runners); everything inside dq | dk | dv is finite."""
    B, T, heads, d = 2, 77, 2, 64
    q, k, v, do, _, *ref = problem(B, T, T, heads, d, None, 1)
    check(f"qkv-causal +16 {B, T, heads, d}", run_packed_qkv(dev, q, k, v, do, None, heads, 1, spare=16), ref, kernel="general")
    B, N, L, heads, d = 2, 100, 77, 2, 40
    q, k, v, do, _, *ref = problem(B, N, L, heads, d, None, 0)
    check(f"cross-kv +16 {B, N, L, heads, d}", run_packed_kv(dev, q, k, v, do, heads, spare=16), ref, kernel="short-key")


# =========================================================================================== B. small training-path kernels
def test_quickgelu_fwd_bwd(dev):
    """x * sigmoid(1.702 x) and its gradient, |x| up to 12 (both sigmoid tails); 5000 elements: the last workgroup is partial."""
    from adaface_dev_amd import ops
    n = 5000
    x = (torch.randn(n, generator=torch.Generator().manual_seed(1)) * 4).clamp(-12, 12)
    x[:8] = torch.tensor([-12.0, 12.0, -11.5, 11.5, 0.0, -0.0, 1e-3, -1e-3])
    x, dy = x.half(), rnd((n,), 2)
    xr = x.double().requires_grad_(True)
    ref = xr * torch.sigmoid(1.702 * xr)
    ref.backward(dy.double())
    y, dx = ops.quickgelu_fwd(x.to(dev)), ops.quickgelu_bwd(x.to(dev), dy.to(dev))
    e_y, e_dx = rel_l2(y.double().cpu().numpy(), ref.detach().numpy()), rel_l2(dx.double().cpu().numpy(), xr.grad.numpy())
    print(f"quickgelu: y {e_y:.2e} dx {e_dx:.2e}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert e_y < ELEM_TOL and e_dx < ELEM_TOL


def test_axpy_and_mul_bit_equal(dev):
    from adaface_dev_amd import ops
    a, b = rnd((37, 200), 1), rnd((37, 200), 2)                         # 7400 elements
    for alpha in (0.5, 0.3):                                            # the trainer's value and a non-dyadic one
        want = (a.float() + alpha * b.float()).half()
        assert torch.equal(ops.axpy(a.to(dev), b.to(dev), alpha).cpu(), want), alpha
    assert torch.equal(ops.mul(a.to(dev), b.to(dev)).cpu(), (a.float() * b.float()).half())


def _same_bits(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_scale_and_clamp_f32(dev, n):
    """In-place fp32 scale and clamp at sizes around the 256-thread workgroup, with +-inf; the clamp propagates NaN as torch.clamp does."""
    from adaface_dev_amd import ops
    a = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    special = torch.tensor([float("inf"), -float("inf"), 0.0, -0.0, 1.0, -1.0])
    a[:min(n, 6)] = special[:min(n, 6)]
    for s in (1.0 / 1024, 0.37):
        assert _same_bits(ops.scale_f32_(a.clone().to(dev), s).cpu(), a * s), (n, s)
    assert _same_bits(ops.clamp_f32_(a.clone().to(dev), -1.0, 1.0).cpu(), torch.clamp(a, -1.0, 1.0)), n
    a[n // 2] = NAN
    got = ops.clamp_f32_(a.clone().to(dev), -0.5, 2.0).cpu()
    assert bool(torch.isnan(got[n // 2])) and _same_bits(got, torch.clamp(a, -0.5, 2.0)), n


@pytest.mark.parametrize("B,H,W,C,stride", [(2, 5, 7, 8, 1), (1, 6, 9, 16, 2), (2, 7, 7, 24, 2)])
def test_im2col3x3(dev, B, H, W, C, stride):
    """Bit-equal to F.unfold of the zero-padded NCHW input with the columns re-ordered to (ky, kx, c)."""
    from adaface_dev_amd import ops
    x = rnd((B, H, W, C), 1)
    cols = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1, stride=stride)      # [B, C*9, P], rows ordered (c, ky, kx)
    P = cols.shape[-1]
    want = cols.reshape(B, C, 9, P).permute(0, 3, 2, 1).reshape(B * P, 9 * C).half()
    got = ops.im2col3x3(x.to(dev), stride).cpu()
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("shape", [(2, 3, 5, 24), (1, 1, 200, 64)])
def test_dora_combine(dev, shape):
    from adaface_dev_amd import ops
    C = shape[-1]
    y0, c2, lb = rnd(shape, 1), rnd(shape, 2), rnd(shape, 3)
    u = torch.randn(C, generator=torch.Generator().manual_seed(4)) * 0.3
    v = torch.randn(C, generator=torch.Generator().manual_seed(5)) * 0.5
    got = ops.dora_combine(y0.to(dev), c2.to(dev), lb.to(dev), u.to(dev), v.to(dev)).cpu()
    want = y0.double() + u.double() * c2.double() + v.double() * lb.double()
    err = rel_l2(got.double().numpy(), want.numpy())
    print(f"dora_combine {shape}: {err:.2e}")
    assert err < ELEM_TOL
