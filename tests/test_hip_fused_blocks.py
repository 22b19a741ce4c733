"""The one-launch transformer-block kernels of the 64 x 64 / 32 x 32 levels on a real MI355X against fp64 on the CPU, figure by figure and
cell by cell: af_xattn_fused (C = 320, C = 640), af_xattn_chain, af_gn_proj_fused (csrc/af_xattn_fused.hip), af_ff_fused, af_ff_chain
(csrc/af_gemm3.hip).  `pytest -m gpu`; the two host-only tests at the end carry no mark.  Conventions of tests/test_hip_autograd_nodes.py.
The modules only route to these kernels from 8192 tokens / 24576 rows, so every case calls the C entry point itself (ops._launch) on a
NaN-filled output buffer that is 128 rows longer than M.

REFERENCE (ref_*): plain torch in fp64 on the CPU on the numbers the device sees -- activations, K, V^T, residuals are fp16 tensors, weights
and biases hold fp16-representable values, gamma / beta are fp32; LayerNorm / GroupNorm in fp64, then the UN-folded weight, so the rounding
pack_matrix_ln makes of gamma * W is part of the error.
RESTATEMENT (re_*): the kernel's data flow on the CPU in fp32 with an fp16 rounding exactly where the kernel's comments say a value becomes
fp16 (the scaled q, the un-normalised P, O in the tile, the GEGLU product, x1 / x3 of the chains, the normalised tile of af_gn_proj_fused, the
output) and the one-pass q / C - mean^2 variance.  It takes nothing from the device; it anchors the bounds (test_restatement_stays_inside_half_
the_bound) and carries the planted defects (test_planted_defects_are_seen).

FIGURES (`figures`), each asserted: (a) rel-L2 and max|got - ref| / max|ref| of the whole tensor; (b) both per batch item; (c) where W_o is the
identity (out IS the attention output O) both per CELL of 16 tokens x one head, the cell's rms and largest error over the tensor's max|ref|;
(d) for an output that carries a residual, instead of (a) / (b): the largest (|got - ref| - 2^-11 |ref|) / max|branch_ref|, whole tensor and per
batch item, against the branch's max bound (branch_ref: the fp64 reference without the residual) -- the residual is 3 to 6 times the branch and
would divide the branch's error by as much in (a).

Paths reached
  test_xattn_fused      af_xattn320t_kernel<2> at (B, N) = (1, 128) one workgroup, (2, 128) a second image, (3, 256) a tile that is not the first of
                        its image; af_xattn640t_kernel<2> at (1, 64), (2, 64), (3, 128).  L = 1, 3, 4 (live_mask granules), 16, 17 (key tiles), 63, 64,
                        65, 77 (the 16-key tail on mfma_k16), 80.  Folded LayerNorm on / off, bias + residual on / off, K a column slice (ldk = C + 64) and
                        V^T a row slice of NaN-filled buffers with ldv = roundup(L, 8) and + 8, NaN behind key L - 1.  Inputs: flat; context row 0 x 5 and
                        row L - 1 x 5 (one key takes nearly all of the mass at its tokens; at L = 77 the spike sits in the mfma_k16 tail); all context rows
                        equal (uniform softmax); token rows with |mean| / sigma = 10 and 30.  (x 5, not x 8: with the 64-wide context of these cases an
                        8-fold key puts the RESTATEMENT at 1.1e-3 max / max, past half the ceiling -- the fp16 rounding of the scaled q times the key --
                        and a 6-fold one within 2 % of it.)
  test_xattn_identity   W_o = I, no bias, no residual, L = 77 and 17: figure (c) on O itself, all six input classes (the spike x 3: ID_SPIKE).
  test_xattn_chain      af_xattn320t_kernel<2, true>, the same shapes, L = 1, 37, 77, 80, a caller-owned x1; x1 one fp16 rounding; out under (d) on
                        the stored x1; bit equality with af_xattn_fused on the stored x1, x1 against af_gemm tile 7.
  test_ff_fused         af_ff320_kernel<false>, M = 1, 127, 128, 129, 300, inner 1280; LayerNorm and residual on / off; flat, row means of 10 and 30
                        sigma, gate pre-activations of +-12 on a tenth of the inner channels.
  test_ff_chain         af_ff320_kernel<true> at (1, 128), (2, 128), (3, 256) with gn_cpg = 10 and at M = 300 without partials; the partials it leaves
                        through af_groupnorm_apply against fp64 group_norm of the returned tensor, also with x_in at per-group means of 100 sigma and
                        with +-6e4 outliers.
  test_gn_proj_fused    af_gn_proj320_kernel at (1, 128), (2, 128), (3, 256), (1, 16384) (nblk = 128: eight trips of the fold loop per lane); partials
                        from an identity af_gemm tile 7; zero-mean, |mean| / sigma = 10 / 100 / 1000, opposite-signed +-6e4 outliers; and the two-launch
                        form (af_groupnorm_apply, af_gemm) under the same bounds.
Every launch is repeated once and must return the same bits; rows M .. M + 127 of the output buffer must still be NaN.

DERIVED bounds: F16_L2 / F16_MAX (test_hip_autograd_nodes.py) for x1 of the chain and for the GroupNorm from the partials af_ff_chain leaves.
MEASURED bounds (the rule of test_hip_module_grads.py: worst value on MI355X over the cases, times two, rounded up to one digit, never past
FWD_CEIL = 2e-3 in either figure), as (rel-L2, max) of the branch; the max bound is T of figure (d).  The anchor is on the reference side: the
restatement alone is within HALF of each bound of fp64 on every case (host test), so no bound can have been fitted to a wrong kernel, and on the
device every figure above 1e-4 must stay within TWICE the restatement's figure of the same case (`hold(..., re=)`; worst ratio measured: 1.55 at
C = 640, 2 x 64, L = 80, row means of 30 sigma -- the order of the one-pass sums; a fifth of an fp16 half-ulp and below, the ratio is noise).
The measured worst values stand beside each constant below."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_hip_autograd_nodes import F16_L2, F16_MAX, cmp, launches, rnd

gpu = pytest.mark.gpu
FWD_CEIL = 2e-3
HALF_ULP = 2.0 ** -11
# (rel-L2, max / max) of the branch; measured on MI355X (worst over the cases) -> twice that, rounded up to one digit, never past the ceiling
XA320 = (FWD_CEIL, FWD_CEIL)    # 5.27e-4 at 1x128 L=63 key0 ln=1; 8.04e-4 at identity 3x256 L=17 last [item 1]; (d) 6.45e-4 at 1x128 L=17 last ln=1 -- both at the ceiling
XA640 = (FWD_CEIL, FWD_CEIL)    # 5.13e-4 at 3x128 L=80 key0 ln=1 [item 1]; 8.22e-4 at 1x64 L=64 last ln=1; (d) 6.27e-4 at 3x128 L=65 key0 ln=1 [item 2] -- both at the ceiling
CH_T = FWD_CEIL                 # (d) 7.53e-4 at 1x128 L=37 last
FF = (9e-4, FWD_CEIL)           # 4.03e-4 at M=1 sat ln=1; 5.49e-4 at M=1 sat ln=0 (ceiling); (d) 3.37e-4 at M=129 mean30
FFC_T = 5e-4                    # (d) 2.22e-4 at 2x128 outliers [item 0]
GP = (6e-4, FWD_CEIL)           # 2.93e-4 at 1x16384 ratio1000; 5.53e-4 at 3x256 outliers [item 1] (ceiling)
RE_FACTOR, RE_FLOOR = 2.0, 1e-4  # a device figure against the restatement's figure of the same case

HEADS, CTX_DIM, LN_EPS, GN_EPS = 8, 64, 1e-5, 1e-6
LOG2E = 1.4426950408889634
PAD_ROWS = 128                                   # NaN rows behind M in every output buffer


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def frnd(shape, seed, scale=1.0):
    """fp32 holding fp16-representable values."""
    return rnd(shape, seed, scale).float()


def affine(C, seed):
    """gamma / beta of a norm, fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.2


def rows_with_mean(rows, C, ratio, seed):
    """Rows with |mean| / sigma = ratio, alternating in sign (test_gemm_folded_layernorm_rows_with_mean_above_their_spread)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, C), generator=g) + ratio * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]).half()


def fold_ln(w, bias, gamma, beta):
    """What ops.pack_matrix_ln hands the kernel, on the CPU: fp16(gamma * W), its fp32 row sums, bias + W beta."""
    w16 = (w * gamma[None, :]).half()
    b = (w * beta[None, :]).sum(dim=1)
    return w16, w16.float().sum(dim=1), b if bias is None else b + bias


def one_pass_stats(x, eps):
    """mean and rstd of the rows as the kernels take them: fp32 sums, q / C - mean^2."""
    C = x.shape[1]
    mean = x.sum(dim=1) / C
    var = ((x * x).sum(dim=1) / C - mean * mean).clamp_min(0.0)
    return mean[:, None], torch.rsqrt(var + eps)[:, None]


# ============================================================================================================ figures
def _pair(e, r, scale=None):
    if scale is None:
        return float(e.norm() / r.norm().clamp_min(1e-300)), float(e.abs().max() / r.abs().max().clamp_min(1e-300))
    return float(e.pow(2).mean().sqrt() / scale), float(e.abs().max() / scale)


def figures(got, ref, bounds, B=1, cell=0, branch=None):
    """{name: (figure, bound)} of `got` [M, C] against the fp64 `ref`: (a), (b), (c) with `cell` columns per head, or (d) when `branch` (the
    fp64 reference without the residual) is given.  bounds = (rel-L2, max)."""
    g, r = got.detach().double().cpu(), ref.double()
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    assert bool(torch.isfinite(g).all()), "not every element was written / finite"
    e = g - r
    M, C = r.shape
    out = {}
    if branch is not None:
        slack = (e.abs() - HALF_ULP * r.abs()).clamp_min(0.0)
        out["d"] = (float(slack.max() / branch.abs().max()), bounds[1])
        for b in range(B if B > 1 else 0):
            sl = slice(b * (M // B), (b + 1) * (M // B))
            out[f"d[{b}]"] = (float(slack[sl].max() / branch[sl].abs().max()), bounds[1])
        return out
    l2, mx = _pair(e, r)
    out["l2"], out["max"] = (l2, bounds[0]), (mx, bounds[1])
    for b in range(B if B > 1 else 0):
        sl = slice(b * (M // B), (b + 1) * (M // B))
        assert float(r[sl].abs().max()) > 0, "degenerate reference slab"
        l2, mx = _pair(e[sl], r[sl])
        out[f"l2[{b}]"], out[f"max[{b}]"] = (l2, bounds[0]), (mx, bounds[1])
    if cell:
        ec = e.reshape(M // 16, 16, C // cell, cell)
        rmax = r.abs().max()
        out["cell-l2"] = (float(ec.pow(2).mean(dim=(1, 3)).sqrt().max() / rmax), bounds[0])
        out["cell-max"] = (float(ec.abs().amax(dim=(1, 3)).max() / rmax), bounds[1])
    return out


WORST = {}


def hold(kernel, tag, got, ref, bounds, re=None, **kw):
    """Print the figures, record the worst per kernel, assert every one; re = the restatement's result for the same case: no figure above RE_FLOOR may be
    more than RE_FACTOR times the restatement's own."""
    f = figures(got, ref, bounds, **kw)
    print(f"ERR {kernel} {tag}: " + "  ".join(f"{k} {v:.3e}" for k, (v, _) in f.items()))
    for k, (v, _) in f.items():
        kind = "d" if k.startswith("d") else ("max" if "max" in k else "l2")
        if v > WORST.get((kernel, kind), (0.0, ""))[0]:
            WORST[(kernel, kind)] = (v, f"{tag} {k}")
    bad = {k: (v, b) for k, (v, b) in f.items() if not v < b}
    assert not bad, (kernel, tag, bad)
    if re is not None:
        fr = figures(re, ref, bounds, **kw)
        far = {k: (v, fr[k][0]) for k, (v, _) in f.items() if v > RE_FLOOR and v > RE_FACTOR * fr[k][0]}
        for k, (v, _) in f.items():
            if v > RE_FLOOR and v / fr[k][0] > WORST.get((kernel, "ratio"), (0.0, ""))[0]:
                WORST[(kernel, "ratio")] = (v / fr[k][0], f"{tag} {k}")
        assert not far, (kernel, tag, "more than twice the restatement's figure", far)


def report(kernel):
    for (kn, kind), (v, tag) in sorted(WORST.items()):
        if kn == kernel:
            print(f"WORST {kn} {kind}: {v:.3e} at {tag}")


def nan_out(dev, M, C):
    return torch.full((M + PAD_ROWS, C), float("nan"), dtype=torch.float16, device=dev)


def twice(tag, launch, M, C, dev):
    """Run `launch(out)` on two NaN-filled buffers: the same bits, nothing written behind row M.  -> out[:M]"""
    a, b = nan_out(dev, M, C), nan_out(dev, M, C)
    launch(a)
    launch(b)
    assert bool(torch.isnan(a[M:]).all()) and bool(torch.isnan(b[M:]).all()), (tag, "rows behind M were written")
    assert torch.equal(a[:M], b[:M]), (tag, "a second call gave other bits")
    return a[:M]


# ============================================================================================================ cross-attention
XA_SHAPES = {320: ((1, 128), (2, 128), (3, 256)), 640: ((1, 64), (2, 64), (3, 128))}
XA_L = (1, 3, 4, 16, 17, 63, 64, 65, 77, 80)
XA_CLASSES = ("flat", "key0", "last", "equal", "mean10", "mean30")
CHAIN_L = (1, 37, 77, 80)
# W_o = I shows O itself: without W_o's averaging over 320 channels the fp16 rounding of the scaled q, amplified by an 8-fold key, alone reaches 1.7e-3 max / max in
# the restatement (past half the ceiling); a 3-fold key still takes 0.97 .. 0.99 of the mass at its tokens and stays at 8.0e-4
ID_SPIKE = 3.0


@functools.lru_cache(maxsize=None)
def xa_weights(C, identity=False):
    wq = frnd((C, C), 101, C ** -0.5)
    wk, wv = frnd((C, CTX_DIM), 102, CTX_DIM ** -0.5), frnd((C, CTX_DIM), 103, CTX_DIM ** -0.5)
    wo = torch.eye(C) if identity else frnd((C, C), 104, C ** -0.5)
    bo = frnd((C,), 105, 0.5)
    gamma, beta = affine(C, 106)
    return dict(wq=wq, wk=wk, wv=wv, wo=wo, bo=bo, gamma=gamma, beta=beta, folded=fold_ln(wq, None, gamma, beta))


def xa_inputs(C, B, N, L, cls, spike=5.0):
    """x [B N, C], K [B, L, C], V [B, L, C] (fp16) of an input class."""
    W = xa_weights(C)
    seed = 1000 * L + 10 * B + XA_CLASSES.index(cls)
    x = rows_with_mean(B * N, C, float(cls[4:]), seed) if cls.startswith("mean") else rnd((B * N, C), seed)
    ctx = rnd((B, L, CTX_DIM), seed + 1).float()
    if cls == "key0":
        ctx[:, 0] *= spike
    elif cls == "last":
        ctx[:, L - 1] *= spike
    elif cls == "equal":
        ctx[:] = ctx[:, :1]
    return x, (ctx @ W["wk"].t()).half(), (ctx @ W["wv"].t()).half()


def xa_cases(C, B, N):
    """(L, class, ln, res_bias, ldv_extra): every L meets every class; the switches rotate with both indices, so every class meets both values of every
    switch and every shape all eight combinations (the row-mean classes are statements about the LayerNorm and always have it)."""
    for li, L in enumerate(XA_L):
        for ci, cls in enumerate(XA_CLASSES):
            ln = True if cls.startswith("mean") else (li + ci) % 2 == 0
            yield L, cls, ln, (li // 2 + ci) % 2 == 0, 8 * ((li + ci // 2 + li // 4) % 2)


def attn_core64(q, k, v, B, N, L, scale):
    """softmax(q k^T scale) v per image and head in fp64: q [B N, C], k / v [B, L, C] -> [B N, C]."""
    C = q.shape[1]
    d = C // HEADS
    qh = q.reshape(B, N, HEADS, d).permute(0, 2, 1, 3)
    kh = k.double().reshape(B, L, HEADS, d).permute(0, 2, 1, 3)
    vh = v.double().reshape(B, L, HEADS, d).permute(0, 2, 1, 3)
    o = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1) @ vh
    return o.permute(0, 2, 1, 3).reshape(B * N, C)


def ref_xattn(W, x, k, v, B, N, L, ln, with_bias):
    """The branch in fp64: to_out(attention(to_q(LN(x)), K, V)) (+ bias)."""
    C = x.shape[1]
    xd = x.double()
    if ln:
        xd = F.layer_norm(xd, (C,), W["gamma"].double(), W["beta"].double(), LN_EPS)
    o = attn_core64(xd @ W["wq"].double().t(), k, v, B, N, L, (C // HEADS) ** -0.5)
    out = o @ W["wo"].double().t()
    return out + W["bo"].double() if with_bias else out


def re_xattn(W, x, k, v, B, N, L, ln, with_bias, res=None, defect=None):
    """af_xattn320t_kernel / af_xattn640t_kernel restated: fp32, with fp16 roundings of the scaled q, the un-normalised P (the row sum is taken from the
    fp32 values), O in the tile and the output; one-pass LayerNorm statistics on the folded weight.
    defect: 'lastkey' (key L - 1 dropped for head 3 in the 16-token tile 5), 'tail64' (keys >= 64 dropped for head 3), 'lastrow' (the branch of the last
    row zero), 'image' (image 1 reads image 0's K / V^T)."""
    C = x.shape[1]
    d = C // HEADS
    xf = x.float()
    if ln:
        w16, cs, bq = W["folded"]
        mean, rstd = one_pass_stats(xf, LN_EPS)
        q = rstd * (xf @ w16.float().t() - mean * cs) + bq
    else:
        q = xf @ W["wq"].t()
    q = (q * torch.tensor(d ** -0.5 * LOG2E, dtype=torch.float32)).half().float()
    O = torch.zeros((B * N, C))
    for b in range(B):
        kb = 0 if (defect == "image" and b == 1) else b
        for h in range(HEADS):
            cols = slice(h * d, (h + 1) * d)
            s = q[b * N:(b + 1) * N, cols] @ k[kb][:, cols].float().t()
            live = torch.ones((N, L), dtype=torch.bool)
            if defect == "lastkey" and b == 0 and h == 3:
                live[80:96, L - 1] = False
            if defect == "tail64" and h == 3:
                live[:, 64:] = False
            s = s.masked_fill(~live, -3.0e38)
            p = torch.exp2(s - s.max(dim=1, keepdim=True).values)
            o = (p.half().float() @ v[kb][:, cols].float()) * (1.0 / p.sum(dim=1, keepdim=True))
            O[b * N:(b + 1) * N, cols] = o.half().float()
    out = O @ W["wo"].t()
    if with_bias:
        out = out + W["bo"]
    if defect == "lastrow":
        out[-1] = 0.0
    if res is not None:
        out = out + res.float()
    return out.half()


class XaPacks:
    """Device packs of xa_weights(C), built once per test."""

    def __init__(self, dev, C, identity=False):
        from adaface_dev_amd import ops
        W = xa_weights(C, identity)
        self.W, self.dev, self.C = W, dev, C
        self.q_ln = ops.pack_matrix_ln(W["wq"], None, W["gamma"], W["beta"], LN_EPS, dev)
        self.q = ops.pack_matrix(W["wq"], None, dev)
        self.o_b = ops.pack_matrix(W["wo"], W["bo"], dev)
        self.o = ops.pack_matrix(W["wo"], None, dev)

    def kv(self, k, v, L, ldv_extra):
        """K as a column slice of a NaN-filled [B L, C + 64] buffer, V^T as a row slice of a NaN-filled [B, C + 16, ldv] one, NaN behind key L - 1."""
        B, C = k.shape[0], self.C
        ldk, ldv = C + 64, (L + 7) // 8 * 8 + ldv_extra
        kbuf = torch.full((B * L, ldk), float("nan"), dtype=torch.float16)
        kbuf[:, 32:32 + C] = k.reshape(B * L, C)
        vbuf = torch.full((B, C + 16, ldv), float("nan"), dtype=torch.float16)
        vbuf[:, 8:8 + C, :L] = v.permute(0, 2, 1)
        return kbuf.to(self.dev)[:, 32:32 + C], ldk, vbuf.to(self.dev)[:, 8:8 + C, :]

    def launch(self, x, kd, ldk, vtd, B, N, L, ln, with_bias, res):
        """-> a function that launches af_xattn_fused into a given output buffer."""
        from adaface_dev_amd import ops
        pq, po = (self.q_ln if ln else self.q), (self.o_b if with_bias else self.o)
        assert vtd.stride(2) == 1 and kd.stride(1) == 1
        return lambda out: ops._launch(
            "af_xattn_fused", x.data_ptr(), pq.wt.data_ptr(), ops._p(pq.bias), ops._p(pq.ln_cs), float(pq.ln_eps), pq.kpad, kd.data_ptr(), ldk, vtd.data_ptr(),
            int(vtd.stride(0)), int(vtd.stride(1)), po.wt.data_ptr(), ops._p(po.bias), po.kpad, ops._p(res), out.data_ptr(), B, N, L, self.C, HEADS,
            float((self.C // HEADS) ** -0.5), ops._zero_page(self.dev).data_ptr())


@gpu
@pytest.mark.parametrize("C,B,N", [(C, B, N) for C in (320, 640) for B, N in XA_SHAPES[C]])
def test_xattn_fused(dev, C, B, N):
    """af_xattn_fused on the grid of the docstring: the branch under (a) / (b), the output with bias + residual under (d).
    Worst on MI355X: see XA320 / XA640."""
    packs, bounds, name = XaPacks(dev, C), (XA320 if C == 320 else XA640), f"xattn{C}"
    res = rnd((B * N, C), 7, 3.0)                                       # the residual stream: three times the branch and more
    res_d = res.to(dev)
    for L, cls, ln, rb, ldx in xa_cases(C, B, N):
        tag = f"{B}x{N} L={L} {cls} ln={int(ln)} res+bias={int(rb)} ldv+{ldx}"
        x, k, v = xa_inputs(C, B, N, L, cls)
        kd, ldk, vtd = packs.kv(k, v, L, ldx)
        xd = x.to(dev)
        out = twice(tag, packs.launch(xd, kd, ldk, vtd, B, N, L, ln, rb, res_d if rb else None), B * N, C, dev)
        branch = ref_xattn(packs.W, x, k, v, B, N, L, ln, rb)
        re = re_xattn(packs.W, x, k, v, B, N, L, ln, rb, res if rb else None)
        if rb:
            hold(name, tag, out, branch + res.double(), bounds, re, B=B, branch=branch)
        else:
            hold(name, tag, out, branch, bounds, re, B=B)
    report(name)


@gpu
@pytest.mark.parametrize("C,B,N", [(320, 3, 256), (640, 3, 128)])
def test_xattn_identity(dev, C, B, N):
    """W_o = the fp16 identity, no bias, no residual: `out` is the attention output O itself, every (16-token tile, head) cell under figure (c)."""
    packs, bounds, name = XaPacks(dev, C, identity=True), (XA320 if C == 320 else XA640), f"xattn{C}"
    for L in (77, 17):
        for i, cls in enumerate(XA_CLASSES):
            tag = f"identity {B}x{N} L={L} {cls}"
            x, k, v = xa_inputs(C, B, N, L, cls, ID_SPIKE)
            kd, ldk, vtd = packs.kv(k, v, L, 8 * (i % 2))
            out = twice(tag, packs.launch(x.to(dev), kd, ldk, vtd, B, N, L, True, False, None), B * N, C, dev)
            hold(name, tag, out, ref_xattn(packs.W, x, k, v, B, N, L, True, False), bounds, re_xattn(packs.W, x, k, v, B, N, L, True, False), B=B, cell=C // HEADS)
    report(name)


# ------------------------------------------------------------------------------------------------------------ af_xattn_chain
@functools.lru_cache(maxsize=None)
def chain_front(B, N):
    """ao, W_1, b_1, x0 in front of the block, and x1 = ao W_1^T + b_1 + x0 in fp64."""
    C = 320
    ao, x0 = rnd((B * N, C), 201), rnd((B * N, C), 202, 3.0)
    w1, b1 = frnd((C, C), 203, C ** -0.5), frnd((C,), 204, 0.5)
    return dict(ao=ao, x0=x0, w1=w1, b1=b1, x1=ao.double() @ w1.double().t() + b1.double() + x0.double())


def re_chain(W, P, k, v, B, N, L, defect=None):
    """af_xattn320t_kernel<2, true> restated: x1 rounds to fp16 once, is the block's input AND its residual.  defect 'x0': the un-added x0 as the final residual."""
    x1 = (P["ao"].float() @ P["w1"].t() + P["b1"] + P["x0"].float()).half()
    return x1, re_xattn(W, x1, k, v, B, N, L, True, True, res=P["x0"] if defect == "x0" else x1)


@gpu
@pytest.mark.parametrize("B,N", XA_SHAPES[320])
def test_xattn_chain(dev, B, N):
    """af_xattn_chain through the C entry point with a caller-owned x1.  x1 is one fp16 rounding of fp64; `out` is held under (d) on the x1 the launch
    stored (the number the rest of the kernel saw), the branch being everything except x1; bit for bit what af_xattn_fused gives on that x1."""
    from adaface_dev_amd import ops
    C, M = 320, B * N
    packs, P = XaPacks(dev, C), chain_front(B, N)
    W = packs.W
    p1 = ops.pack_matrix(P["w1"], P["b1"], dev)
    ao_d, x0_d = P["ao"].to(dev), P["x0"].to(dev)
    x1_g = ops.gemm(ao_d, p1, residual=x0_d, tile=7)
    for i, L in enumerate(CHAIN_L):
        for cls in ("flat", "key0", "last", "equal"):
            tag = f"chain {B}x{N} L={L} {cls}"
            _, k, v = xa_inputs(C, B, N, L, cls)
            kd, ldk, vtd = packs.kv(k, v, L, 8 * (i % 2))
            pq, po = packs.q_ln, packs.o_b
            x1s = [nan_out(dev, M, C), nan_out(dev, M, C)]

            def launch(out, x1s=x1s, n=[0]):
                x1 = x1s[n[0] % 2]
                n[0] += 1
                ops._launch("af_xattn_chain", ao_d.data_ptr(), p1.wt.data_ptr(), ops._p(p1.bias), p1.kpad, x0_d.data_ptr(), x1.data_ptr(), pq.wt.data_ptr(),
                            ops._p(pq.bias), ops._p(pq.ln_cs), float(pq.ln_eps), pq.kpad, kd.data_ptr(), ldk, vtd.data_ptr(), int(vtd.stride(0)),
                            int(vtd.stride(1)), po.wt.data_ptr(), ops._p(po.bias), po.kpad, out.data_ptr(), B, N, L, C, HEADS, float(40 ** -0.5),
                            ops._zero_page(dev).data_ptr())
            out = twice(tag, launch, M, C, dev)
            assert torch.equal(x1s[0][:M], x1s[1][:M]) and bool(torch.isnan(x1s[0][M:]).all()), (tag, "x1")
            x1 = x1s[0][:M].contiguous()
            cmp(f"{tag} x1", x1, P["x1"], F16_L2, F16_MAX, torch.float16)
            assert torch.equal(x1, x1_g) or float((x1.double() - x1_g.double()).norm() / x1_g.double().norm()) < 2e-4, (tag, "x1 against af_gemm")
            two = twice(tag + " two launches", packs.launch(x1, kd, ldk, vtd, B, N, L, True, True, x1), M, C, dev)
            assert torch.equal(out, two), (tag, "the chained launch and af_xattn_fused on its x1 differ")
            x1c = x1.cpu()
            branch = ref_xattn(W, x1c, k, v, B, N, L, True, True)
            hold("chain", tag, out, branch + x1c.double(), (CH_T, CH_T), B=B, branch=branch)
    report("chain")


# ============================================================================================================ feed-forward
FF_M = (1, 127, 128, 129, 300)
FF_CLASSES = ("flat", "mean10", "mean30", "sat")
FF_INNER = 1280


@functools.lru_cache(maxsize=None)
def ff_weights(sat=False):
    C = 320
    w1, b1 = frnd((2 * FF_INNER, C), 301, C ** -0.5), frnd((2 * FF_INNER,), 302, 0.1)
    if sat:                                                             # gate pre-activations of +-12 on a tenth of the inner channels
        b1 = b1.clone()
        b1[FF_INNER:FF_INNER + 128:2] = 12.0
        b1[FF_INNER + 1:FF_INNER + 128:2] = -12.0
    w2, b2 = frnd((C, FF_INNER), 303, FF_INNER ** -0.5), frnd((C,), 304, 0.5)
    wp, bp = frnd((C, C), 305, C ** -0.5), frnd((C,), 306, 0.5)
    gamma, beta = affine(C, 307)
    return dict(w1=w1, b1=b1, w2=w2, b2=b2, wp=wp, bp=bp, gamma=gamma, beta=beta, folded=fold_ln(w1, b1, gamma, beta))


def ff_x(M, cls):
    seed = 3000 + 10 * M + FF_CLASSES.index(cls)
    return rows_with_mean(M, 320, float(cls[4:]), seed) if cls.startswith("mean") else rnd((M, 320), seed)


def ref_ff(W, x, ln):
    """The branch in fp64: W2 (v * gelu(g)) + b2, [v | g] = W1 LN(x) + b1."""
    xd = x.double()
    if ln:
        xd = F.layer_norm(xd, (320,), W["gamma"].double(), W["beta"].double(), LN_EPS)
    hv, hg = (xd @ W["w1"].double().t() + W["b1"].double()).chunk(2, dim=-1)
    return (hv * F.gelu(hg)) @ W["w2"].double().t() + W["b2"].double()


def re_ff(W, x, ln, res=None, defect=None, tail=None):
    """af_ff320_kernel restated: fp32 with the GEGLU product (and x3 of the chain) rounded to fp16; one-pass LayerNorm statistics on the folded weight.
    tail = x_in: the proj_out tail of af_ff_chain.  defect: 'drop' (the 64-wide inner chunk 7 dropped), 'swap' (value and gate halves swapped in chunk 7)."""
    xf = x.float()
    if ln:
        w16, cs, b1 = W["folded"]
        mean, rstd = one_pass_stats(xf, LN_EPS)
        h = rstd * (xf @ w16.float().t() - mean * cs) + b1
    else:
        h = xf @ W["w1"].t() + W["b1"]
    hv, hg = (t.clone() for t in h.chunk(2, dim=-1))
    c7 = slice(7 * 64, 8 * 64)
    if defect == "swap":
        hv[:, c7], hg[:, c7] = hg[:, c7].clone(), hv[:, c7].clone()
    g = (hv * F.gelu(hg)).half().float()
    if defect == "drop":
        g[:, c7] = 0.0
    out = g @ W["w2"].t() + W["b2"]
    if res is not None:
        out = out + res.float()
    if tail is None:
        return out.half()
    return (out.half().float() @ W["wp"].t() + W["bp"] + tail.float()).half()


class FfPacks:
    def __init__(self, dev, sat=False):
        from adaface_dev_amd import ops
        W = ff_weights(sat)
        self.W, self.dev = W, dev
        wi, bi = ops.interleave_geglu(W["w1"], W["b1"])
        self.p1 = ops.pack_matrix(wi, bi, dev)
        wi, bi = ops.interleave_geglu(W["w1"] * W["gamma"][None, :], W["b1"] + (W["w1"] * W["beta"][None, :]).sum(dim=1))   # as GEGLU.packed_ln
        self.p1_ln = ops.pack_matrix(wi, bi, dev)
        self.p1_ln.ln_cs, self.p1_ln.ln_eps = self.p1_ln.wt.float().sum(dim=1).contiguous(), LN_EPS
        self.p2 = ops.pack_matrix(W["w2"], W["b2"], dev)
        self.pp = ops.pack_matrix(W["wp"], W["bp"], dev)


@gpu
@pytest.mark.parametrize("M", FF_M)
def test_ff_fused(dev, M):
    """af_ff_fused: ragged M around the 128-row tile, LayerNorm and residual on / off, the four input classes (the row-mean classes with the LayerNorm only:
    they are statements about its variance).  Worst on MI355X: see FF."""
    from adaface_dev_amd import ops
    packs = {False: FfPacks(dev), True: FfPacks(dev, sat=True)}
    res = rnd((M, 320), 8, 3.0)
    res_d = res.to(dev)
    for cls in FF_CLASSES:
        pk = packs[cls == "sat"]
        x = ff_x(M, cls)
        xd = x.to(dev)
        for ln in ((True,) if cls.startswith("mean") else (True, False)):
            branch = ref_ff(pk.W, x, ln)
            for with_res in (True, False):
                tag = f"M={M} {cls} ln={int(ln)} res={int(with_res)}"
                p1 = pk.p1_ln if ln else pk.p1

                def launch(out):
                    ops._launch("af_ff_fused", xd.data_ptr(), p1.wt.data_ptr(), ops._p(p1.bias), ops._p(p1.ln_cs), float(p1.ln_eps), p1.kpad, pk.p2.wt.data_ptr(),
                                ops._p(pk.p2.bias), pk.p2.kpad, ops._p(res_d if with_res else None), out.data_ptr(), M, 320, FF_INNER, ops._zero_page(dev).data_ptr())
                out = twice(tag, launch, M, 320, dev)
                if with_res:
                    hold("ff", tag, out, branch + res.double(), FF, re_ff(pk.W, x, ln, res), branch=branch)
                else:
                    hold("ff", tag, out, branch, FF, re_ff(pk.W, x, ln))
    report("ff")


# ------------------------------------------------------------------------------------------------------------ af_ff_chain
FFC_SHAPES = ((1, 128, 10), (2, 128, 10), (3, 256, 10), (1, 300, 0))     # (B, N, gn_cpg)
FFC_CLASSES = ("flat", "gmean100", "outliers")


def ffc_x_in(B, N, cls):
    """x_in of the SpatialTransformer: flat; per-group means of 100 sigma (alternating sign); a handful of +-6e4 values per third group (the constructions
    of the two hostile GroupNorm tests of test_hip_kernels.py).  The outliers stay 5e3 below the fp16 maximum: the sum with the branch stays inside fp16."""
    C, cpg = 320, 10
    g = torch.Generator().manual_seed(4000 + 10 * B + FFC_CLASSES.index(cls))
    x = torch.randn((B, N, C), generator=g)
    if cls == "gmean100":
        mean = (100.0 * (1 + 0.1 * torch.arange(32).float() / 32)).repeat_interleave(cpg)
        x = x + mean * torch.where(torch.arange(C) // cpg % 2 == 0, 1.0, -1.0)
    elif cls == "outliers":
        for b in range(B):
            for gi in range(0, 32, 3):
                ch0 = gi * cpg
                x[b, 0, ch0] = 6.0e4 if gi % 2 else -6.0e4
                x[b, N // 2, ch0 + 1] = -6.0e4 if gi % 2 else 6.0e4
                x[b, N - 1, ch0 + cpg - 1] = 6.0e4
    return x.half().reshape(B * N, C)


def ref_ffc(W, x, res):
    """The branch of af_ff_chain in fp64: everything except x_in."""
    return (ref_ff(W, x, True) + res.double()) @ W["wp"].double().t() + W["bp"].double()


@gpu
@pytest.mark.parametrize("B,N,cpg", FFC_SHAPES)
def test_ff_chain(dev, B, N, cpg):
    """af_ff_chain: out = x_in + b_p + W_p x3 under (d) (the branch: everything except x_in), and the GroupNorm partials its epilogue leaves: af_groupnorm_apply
    on them against fp64 group_norm of the RETURNED tensor is one fp16 rounding, also when x_in carries group means of 100 sigma or +-6e4 outliers."""
    from adaface_dev_amd import ops
    C, M = 320, B * N
    pk = FfPacks(dev)
    x, res = rnd((M, C), 11), rnd((M, C), 12, 3.0)
    xd, res_d = x.to(dev), res.to(dev)
    branch = ref_ffc(pk.W, x, res)
    gam, bet = affine(C, 13)
    for cls in FFC_CLASSES:
        tag = f"ffchain {B}x{N} cpg={cpg} {cls}"
        x_in = ffc_x_in(B, N, cls)
        x_in_d = x_in.to(dev)
        gns = [ops.GnPartials.alloc(dev, B, N, C, cpg) if cpg else None for _ in range(2)]
        p1 = pk.p1_ln

        def launch(out, n=[0]):
            gn = gns[n[0] % 2]
            n[0] += 1
            ops._launch("af_ff_chain", xd.data_ptr(), p1.wt.data_ptr(), ops._p(p1.bias), ops._p(p1.ln_cs), float(p1.ln_eps), p1.kpad, pk.p2.wt.data_ptr(),
                        ops._p(pk.p2.bias), pk.p2.kpad, res_d.data_ptr(), pk.pp.wt.data_ptr(), ops._p(pk.pp.bias), pk.pp.kpad, x_in_d.data_ptr(), out.data_ptr(),
                        None if gn is None else gn.ws.data_ptr(), cpg, N, M, C, FF_INNER, ops._zero_page(dev).data_ptr())
        out = twice(tag, launch, M, C, dev)
        hold("ffchain", tag, out, branch + x_in.double(), (FFC_T, FFC_T), re_ff(pk.W, x, True, res, tail=x_in), B=B, branch=branch)
        if cpg:
            assert torch.equal(gns[0].ws[:, :N // 128], gns[1].ws[:, :N // 128]), (tag, "the partials of a second call differ")
            y = out.contiguous().reshape(B, N, C)
            gns[0].attach(y)
            with launches() as names:
                yn = ops.groupnorm(y, gam.to(dev), bet.to(dev), 1e-5, False)
            assert names == ["af_groupnorm_apply"], (tag, names)
            ref = F.group_norm(y.double().cpu().permute(0, 2, 1), 32, gam.double(), bet.double(), 1e-5).permute(0, 2, 1)
            cmp(f"{tag} groupnorm from the partials", yn, ref, F16_L2, F16_MAX, torch.float16)
            for b in range(B):
                cmp(f"{tag} groupnorm from the partials [item {b}]", yn[b], ref[b], F16_L2, F16_MAX)
    report("ffchain")


# ============================================================================================================ af_gn_proj_fused
GP_SHAPES = ((1, 128), (2, 128), (3, 256), (1, 16384))
GP_CLASSES = ("zero-mean", "ratio10", "ratio100", "ratio1000", "outliers")


@functools.lru_cache(maxsize=None)
def gp_weights():
    C = 320
    gamma, beta = affine(C, 501)
    return dict(w=frnd((C, C), 502, C ** -0.5), b=frnd((C,), 503, 0.5), gamma=gamma, beta=beta)


def gp_x(B, HW, cls):
    """[B, HW, 320] fp16: zero-mean with a spread that differs per image (1, 1.5, 2: statistics of the wrong image are visible); group means of ratio x sigma;
    opposite-signed +-6e4 outliers (the constructions of the two hostile GroupNorm tests of test_hip_kernels.py)."""
    C, cpg = 320, 10
    g = torch.Generator().manual_seed(5000 + 10 * B + GP_CLASSES.index(cls))
    x = torch.randn((B, HW, C), generator=g)
    if cls == "zero-mean":
        x = x * (1 + 0.5 * torch.arange(B).float())[:, None, None]
    elif cls.startswith("ratio"):
        ratio = float(cls[5:])
        sigma = 0.25 if ratio >= 1000 else 1.0
        mean = (ratio * sigma * (1 + 0.1 * torch.arange(32).float() / 32)).repeat_interleave(cpg)
        x = x * sigma + mean * torch.where(torch.arange(C) // cpg % 2 == 0, 1.0, -1.0)
    else:
        for b in range(B):
            for gi in range(0, 32, 3):
                ch0 = gi * cpg
                x[b, 0, ch0] = 6.0e4 if gi % 2 else -6.0e4
                x[b, HW // 2, ch0 + 1] = -6.0e4 if gi % 2 else 6.0e4
                x[b, HW - 1, ch0 + cpg - 1] = 6.0e4
    return x.half()


def ref_gp(W, x):
    B, HW, C = x.shape
    xn = F.group_norm(x.double().permute(0, 2, 1), 32, W["gamma"].double(), W["beta"].double(), GN_EPS).permute(0, 2, 1).reshape(B * HW, C)
    return xn @ W["w"].double().t() + W["b"].double()


def re_gp(W, x, defect=None):
    """af_gn_proj320_kernel restated: mean and variance per (image, group) about the mean, rounded to fp32 (the kernel merges shifted (sum, M2) partials: there is no E[x^2] - mean^2 to restate),
    the normalised tile x * (rstd gamma) + (beta - mean rstd gamma) rounded to fp16, the projection in fp32.  defect 'stats': group 5 of image 1 normalised with
    image 0's statistics."""
    B, HW, C = x.shape
    xg = x.float().reshape(B, HW, 32, C // 32)
    mean = xg.double().mean(dim=(1, 3), keepdim=True)
    var = (xg.double() - mean).pow(2).mean(dim=(1, 3), keepdim=True).float()
    mean = mean.float()
    if defect == "stats":
        mean[1, :, 5], var[1, :, 5] = mean[0, :, 5].clone(), var[0, :, 5].clone()
    sc = torch.rsqrt(var + GN_EPS) * W["gamma"].reshape(1, 1, 32, -1)
    sh = W["beta"].reshape(1, 1, 32, -1) - mean * sc
    tile = (xg * sc + sh).half().float().reshape(B * HW, C)
    return (tile @ W["w"].t() + W["b"]).half()


@gpu
@pytest.mark.parametrize("B,HW", GP_SHAPES)
def test_gn_proj_fused(dev, B, HW):
    """af_gn_proj_fused on the partials an identity af_gemm (tile 7, gn_cpg = 10) leaves, and the two launches it replaces, both against fp64.
    Worst on MI355X: see GP."""
    from adaface_dev_amd import ops
    C, M = 320, B * HW
    W = gp_weights()
    pw, eye = ops.pack_matrix(W["w"], W["b"], dev), ops.pack_matrix(torch.eye(C), None, dev)
    gam, bet = W["gamma"].to(dev), W["beta"].to(dev)
    for cls in GP_CLASSES:
        tag = f"gnproj {B}x{HW} {cls}"
        x = gp_x(B, HW, cls)
        y = ops.gemm(x.reshape(M, C).to(dev), eye, rows_per_batch=HW, tile=7, gn_cpg=10)
        gn = ops.partials_of(y)
        assert gn is not None and gn.nblk == HW // 128, (tag, "the producer was expected to leave its statistics")
        assert torch.equal(y.cpu(), x.reshape(M, C)), (tag, "identity weights must reproduce the input")

        def launch(out):
            ops._launch("af_gn_proj_fused", y.data_ptr(), gn.ws.data_ptr(), gn.nblk, gam.data_ptr(), bet.data_ptr(), GN_EPS, pw.wt.data_ptr(), ops._p(pw.bias), pw.kpad,
                        out.data_ptr(), B, HW, C, 32, ops._zero_page(dev).data_ptr())
        out = twice(tag, launch, M, C, dev)
        ref, re = ref_gp(W, x), re_gp(W, x)
        hold("gnproj", tag, out, ref, GP, re, B=B)
        y3 = y.reshape(B, HW, C)
        y3._gn_partials = gn
        with launches() as names:
            two = ops.gemm(ops.groupnorm(y3, gam, bet, GN_EPS, False).reshape(M, C), pw, tile=7)
        assert names[0] == "af_groupnorm_apply", (tag, names)
        hold("gnproj", tag + " two launches", two, ref, GP, re, B=B)
    report("gnproj")


# ============================================================================================================ host-only
def _half(bounds):
    return bounds[0] / 2, bounds[1] / 2


def _inside(kernel, tag, got, ref, bounds, **kw):
    f = figures(got, ref, _half(bounds), **kw)
    for k, (v, _) in f.items():
        kind = "d" if k.startswith("d") else ("max" if "max" in k else "l2")
        if v > WORST.get((kernel, kind), (0.0, ""))[0]:
            WORST[(kernel, kind)] = (v, f"{tag} {k}")
    bad = {k: (v, b) for k, (v, b) in f.items() if not v < b}
    assert not bad, (kernel, tag, bad)


def test_restatement_stays_inside_half_the_bound():
    """The reference side of every bound: on every case of the device tests the CPU restatement of the kernel's data flow is within HALF of the bound of fp64
    in every figure -- the bounds leave the kernel's own fp16 roundings a factor of two and no more.  (The (1, 16384) case of af_gn_proj_fused on two classes.)"""
    for C in (320, 640):
        W, bounds = xa_weights(C), (XA320 if C == 320 else XA640)
        for B, N in XA_SHAPES[C]:
            res = rnd((B * N, C), 7, 3.0)
            for L, cls, ln, rb, _ in xa_cases(C, B, N):
                x, k, v = xa_inputs(C, B, N, L, cls)
                branch = ref_xattn(W, x, k, v, B, N, L, ln, rb)
                got = re_xattn(W, x, k, v, B, N, L, ln, rb, res if rb else None)
                tag = f"re xattn{C} {B}x{N} L={L} {cls} ln={int(ln)} res+bias={int(rb)}"
                if rb:
                    _inside(f"re-xattn{C}", tag, got, branch + res.double(), bounds, B=B, branch=branch)
                else:
                    _inside(f"re-xattn{C}", tag, got, branch, bounds, B=B)
        Wi, (B, N) = xa_weights(C, True), XA_SHAPES[C][2]
        for L in (77, 17):
            for cls in XA_CLASSES:
                x, k, v = xa_inputs(C, B, N, L, cls, ID_SPIKE)
                _inside(f"re-xattn{C}", f"re identity {C} L={L} {cls}", re_xattn(Wi, x, k, v, B, N, L, True, False), ref_xattn(Wi, x, k, v, B, N, L, True, False),
                        bounds, B=B, cell=C // HEADS)
    W = xa_weights(320)
    for B, N in XA_SHAPES[320]:
        P = chain_front(B, N)
        for L in CHAIN_L:
            for cls in ("flat", "key0", "last", "equal"):
                _, k, v = xa_inputs(320, B, N, L, cls)
                x1, out = re_chain(W, P, k, v, B, N, L)
                cmp(f"re chain {B}x{N} x1", x1, P["x1"], F16_L2, F16_MAX)
                branch = ref_xattn(W, x1, k, v, B, N, L, True, True)
                _inside("re-chain", f"re chain {B}x{N} L={L} {cls}", out, branch + x1.double(), (CH_T, CH_T), B=B, branch=branch)
    for M in FF_M:
        res = rnd((M, 320), 8, 3.0)
        for cls in FF_CLASSES:
            Wf, x = ff_weights(cls == "sat"), ff_x(M, cls)
            for ln in ((True,) if cls.startswith("mean") else (True, False)):
                branch = ref_ff(Wf, x, ln)
                _inside("re-ff", f"re ff M={M} {cls} ln={int(ln)}", re_ff(Wf, x, ln), branch, FF)
                _inside("re-ff", f"re ff M={M} {cls} ln={int(ln)} res", re_ff(Wf, x, ln, res), branch + res.double(), FF, branch=branch)
    Wf = ff_weights()
    for B, N, _ in FFC_SHAPES:
        x, res = rnd((B * N, 320), 11), rnd((B * N, 320), 12, 3.0)
        branch = ref_ffc(Wf, x, res)
        for cls in FFC_CLASSES:
            x_in = ffc_x_in(B, N, cls)
            _inside("re-ffchain", f"re ffchain {B}x{N} {cls}", re_ff(Wf, x, True, res, tail=x_in), branch + x_in.double(), (FFC_T, FFC_T), B=B, branch=branch)
    Wg = gp_weights()
    for B, HW in GP_SHAPES:
        for cls in (GP_CLASSES if HW < 16384 else ("zero-mean", "ratio1000")):
            x = gp_x(B, HW, cls)
            _inside("re-gnproj", f"re gnproj {B}x{HW} {cls}", re_gp(Wg, x), ref_gp(Wg, x), GP, B=B)
    for kernel in sorted({k for k, _ in WORST if k.startswith("re-")}):
        report(kernel)


def _seen(tag, got, ref, bounds, **kw):
    """A planted defect must push at least one figure to three times its bound."""
    f = figures(got, ref, bounds, **kw)
    worst = max(f.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"DEFECT {tag}: {worst[0]} {worst[1][0]:.3e} = {worst[1][0] / worst[1][1]:.1f} x its bound")
    assert worst[1][0] >= 3 * worst[1][1], (tag, f)


def test_planted_defects_are_seen():
    """Sensitivity: each defect, planted in the restatement (which is inside half the bound without it), pushes at least one figure past three times its bound --
    at the largest shapes of the device tests, where the whole-tensor rel-L2 of a residual-carrying output would let most of them through."""
    for C in (320, 640):
        bounds, (B, N), L = (XA320 if C == 320 else XA640), XA_SHAPES[C][2], 77
        Wi, W = xa_weights(C, True), xa_weights(C)
        res = rnd((B * N, C), 7, 3.0)
        for cls in ("flat", "last"):
            xi, ki, vi = xa_inputs(C, B, N, L, cls, ID_SPIKE)
            x, k, v = xa_inputs(C, B, N, L, cls)
            ref_i = ref_xattn(Wi, xi, ki, vi, B, N, L, True, False)
            for defect in ("lastkey", "tail64"):
                _seen(f"xattn{C} {cls} {defect} (W_o = I)", re_xattn(Wi, xi, ki, vi, B, N, L, True, False, defect=defect), ref_i, bounds, B=B, cell=C // HEADS)
            branch = ref_xattn(W, x, k, v, B, N, L, True, True)
            for defect in ("lastkey", "tail64", "lastrow", "image"):
                _seen(f"xattn{C} {cls} {defect} (residual)", re_xattn(W, x, k, v, B, N, L, True, True, res, defect=defect), branch + res.double(), bounds, B=B,
                      branch=branch)
    (B, N), W = XA_SHAPES[320][2], xa_weights(320)
    P = chain_front(B, N)
    _, k, v = xa_inputs(320, B, N, 77, "flat")
    x1, out = re_chain(W, P, k, v, B, N, 77, defect="x0")
    branch = ref_xattn(W, x1, k, v, B, N, 77, True, True)
    _seen("chain: x0 as the final residual", out, branch + x1.double(), (CH_T, CH_T), B=B, branch=branch)
    Wf, M = ff_weights(), 300
    x, res = ff_x(M, "flat"), rnd((M, 320), 8, 3.0)
    branch = ref_ff(Wf, x, True)
    for defect in ("drop", "swap"):
        _seen(f"ff {defect}", re_ff(Wf, x, True, res, defect=defect), branch + res.double(), FF, branch=branch)
    out = re_ff(Wf, x, True, res).float()
    out[-1] = res[-1].float()
    _seen("ff: the last row's branch zero", out.half(), branch + res.double(), FF, branch=branch)
    B, N = 3, 256
    x, res, x_in = rnd((B * N, 320), 11), rnd((B * N, 320), 12, 3.0), ffc_x_in(B, N, "flat")
    _seen("ffchain drop", re_ff(Wf, x, True, res, defect="drop", tail=x_in), ref_ffc(Wf, x, res) + x_in.double(), (FFC_T, FFC_T), B=B, branch=ref_ffc(Wf, x, res))
    Wg = gp_weights()
    for cls in ("zero-mean",):
        x = gp_x(3, 256, cls)
        _seen(f"gnproj {cls}: a group with the neighbouring image's statistics", re_gp(Wg, x, defect="stats"), ref_gp(Wg, x), GP, B=3)
