"""The SpatialTransformer's proj_out folded into the feed-forward's second projection (ops.pack_ff_proj_out, attention.FOLD_PROJ_OUT):
    x_in + b_p + W_p (x2 + b2 + W2 g) = x_in + (W_p b2 + b_p) + [W_p W2 | W_p] [g ; x2]
one K = 5 C GEMM where the feed-forward runs as two GEMMs (C = 640 / 1280).  The pack on the CPU against fp64; the block against the fp32
oracle, measured beside the two-launch form in the same test; the GroupNorm partials, the repack after an in-place weight change and the launch
count."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------- the pack, no GPU
def test_pack_is_the_fp64_product_rounded_once():
    """[W_p W2 | W_p] and W_p b2 + b_p against fp64: every weight within one fp16 ulp of the fp64 value (the fp32 product's own error is three
    orders below an fp16 ulp at K = C = 128), the bias to fp32 accuracy."""
    from adaface_dev_amd import ops
    C = 128
    g = torch.Generator().manual_seed(7)
    w2 = torch.randn((C, 4 * C), generator=g) * (4 * C) ** -0.5
    b2 = torch.randn(C, generator=g) * 0.05
    wp = torch.randn((C, C, 1, 1), generator=g) * C ** -0.5
    bp = torch.randn(C, generator=g) * 0.05
    pw = ops.pack_ff_proj_out(w2, b2, wp, bp, "cpu")
    assert (pw.N, pw.K, pw.kpad) == (C, 5 * C, 5 * C) and pw.wt.dtype == torch.float16 and pw.wt.shape == (C, 5 * C) and pw.ln_cs is None
    wp64 = wp.double().reshape(C, C)
    want = torch.cat([wp64 @ w2.double(), wp64], dim=1)
    ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) - 10), torch.tensor(2.0 ** -24, dtype=torch.float64))
    assert bool(((pw.wt.double() - want).abs() <= ulp).all())
    assert torch.equal(pw.wt[:, 4 * C:], wp.reshape(C, C).to(torch.float16))
    assert float((pw.bias.double() - (wp64 @ b2.double() + bp.double())).abs().max()) < 1e-6
    # a pure function of its four tensors
    again = ops.pack_ff_proj_out(w2, b2, wp, bp, "cpu")
    assert torch.equal(again.wt, pw.wt) and torch.equal(again.bias, pw.bias)


# ------------------------------------------------------------------------------- the block
CASES = [(640, 2, 32), (1280, 2, 16), (1280, 2, 8)]      # (C, B, H = W); 8 x 8: M = 128, the block's `small` LayerNorm path


@functools.lru_cache(maxsize=None)
def block(C):
    """The module with synthetic weights (proj_out drawn like every other tensor, not left at zero) and its fp32 state dict; built once per width."""
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.attention import SpatialTransformer
    st = SpatialTransformer(C, 8, C // 8, depth=1, context_dim=768)
    rng.load_synth_weights(st, seed=21)
    sd = {k: v.detach().clone() for k, v in st.state_dict().items()}
    assert float(sd["proj_out.weight"].abs().max()) > 0
    return st.to("cuda:0").eval(), sd


@functools.lru_cache(maxsize=None)
def case(C, B, H):
    """Inputs and the fp32 CPU oracle's output (never modified)."""
    from adaface_dev_amd import rng
    from oracle import unet_oracle as O
    _, sd = block(C)
    x = rng.synth_input(f"fold.x.{C}.{H}", (B, C, H, H), seed=21)
    ctx = rng.synth_input(f"fold.ctx.{C}.{H}", (B, 77, 768), seed=21)
    with torch.no_grad():
        ref = O.spatial_transformer(sd, "", x, ctx, None, 8)
    return x, ctx, ref.numpy()


def run(st, x, ctx, fold, monkeypatch, dev):
    """SpatialTransformer.hip with the switch set -> (NHWC fp16 output carrying whatever partials the launch left, GEMM-family launches)."""
    from adaface_dev_amd import _lib, ops
    from adaface_dev_amd.ldm.modules import attention
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import to_nhwc_f16
    monkeypatch.setattr(attention, "FOLD_PROJ_OUT", fold)
    xd, cd = to_nhwc_f16(x.to(dev)).contiguous(), ctx.to(dev).to(torch.float16).contiguous()
    with torch.no_grad():
        st.hip(xd, cd)                                        # packs are built here, outside the counted pass
        torch.cuda.synchronize()
        ops.prof_enable(True)
        ops.prof_reset()
        try:
            out = st.hip(xd, cd)
            torch.cuda.synchronize()
            n, _ = ops.prof_read(_lib.AF_FAM_GEMM)
        finally:
            ops.prof_enable(False)
    return out, n


def nchw(out):
    return out.float().cpu().permute(0, 3, 1, 2).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("C,B,H", CASES)
def test_folded_block_against_the_oracle_and_the_two_launch_form(dev, monkeypatch, C, B, H):
    """Measured tolerance: the two-launch form's error against the fp32 oracle is taken in this test; the folded form may be at most 1.5 x that
    far, and the two forms agree within the sum of their errors.  One GEMM-family launch fewer, exactly."""
    st, _ = block(C)
    x, ctx, ref = case(C, B, H)
    out0, n0 = run(st, x, ctx, False, monkeypatch, dev)
    out1, n1 = run(st, x, ctx, True, monkeypatch, dev)
    e0, e1 = rel_l2(nchw(out0), ref), rel_l2(nchw(out1), ref)
    e01 = rel_l2(nchw(out1), nchw(out0))
    print(f"fold proj_out C={C} B={B} {H}x{H}: rel_l2 vs fp32 oracle two-launch {e0:.3e}, folded {e1:.3e}; folded vs two-launch {e01:.3e}; "
          f"GEMM launches {n0} -> {n1}")
    assert np.isfinite(nchw(out1)).all()
    assert e0 < 1e-2                                          # (only that the yardstick form itself is sound: five times the block parity tests' bound)
    assert e1 <= 1.5 * e0
    assert e01 <= e0 + e1
    assert n1 == n0 - 1
    # the partials the next GroupNorm reads: the folded launch leaves them wherever the two-launch form did
    from adaface_dev_amd import ops
    g0, g1 = ops.partials_of(out0), ops.partials_of(out1)
    assert g0 is None or g1 is not None
    if g0 is not None:
        check_partials(g0, g1, out0)


def check_partials(g0, g1, out):
    """[B][blocks][32][sum, sumsq] of two launches that computed the same tensor to ~1e-3: the sums of squares agree to 1e-3 relative; a sum
    (which may cancel to nothing) to 1e-3 of its natural scale sqrt(n sumsq), n = 128 rows x cpg channels."""
    assert (g0.nblk, g0.cpg, g0.B, g0.hw, g0.C) == (g1.nblk, g1.cpg, g1.B, g1.hw, g1.C)
    a, b = g0.ws[:, :g0.nblk].double().cpu(), g1.ws[:, :g1.nblk].double().cpu()
    assert bool(((a[..., 1] - b[..., 1]).abs() <= 1e-3 * a[..., 1]).all())
    assert bool(((a[..., 0] - b[..., 0]).abs() <= 1e-3 * torch.sqrt(128.0 * g0.cpg * a[..., 1])).all())
    # ... and they describe the tensor: per image and group against the stored fp16 values
    Bn, C = g0.B, g0.C
    v = out.reshape(Bn, g0.hw, C // g0.cpg, g0.cpg).double().cpu()
    assert torch.allclose(a[..., 1].sum(1), (v * v).sum((1, 3)), rtol=2e-3)


@pytest.mark.gpu
def test_gn_partials_ride_on_the_folded_launch(dev):
    """The launch itself on a tile that writes GroupNorm partials (128 x 160, unsplit): two sources + residual + partials in one launch, against
    the two GEMMs on the same tile."""
    from adaface_dev_amd import ops
    C, M, rpb = 640, 2048, 1024
    g = torch.Generator().manual_seed(9)
    rnd = lambda shape, s=1.0: (torch.randn(shape, generator=g) * s)
    w2, b2, wp, bp = rnd((C, 4 * C), (4 * C) ** -0.5), rnd((C,), 0.05), rnd((C, C), C ** -0.5), rnd((C,), 0.05)
    gg, x2, x_in = (rnd((M, 4 * C)).to(torch.float16).to(dev), rnd((M, C)).to(torch.float16).to(dev), rnd((M, C)).to(torch.float16).to(dev))
    y = ops.gemm(gg, ops.pack_matrix(w2, b2, dev), residual=x2, tile=11, splits=1)
    out0 = ops.gemm(y, ops.pack_matrix(wp, bp, dev), residual=x_in, rows_per_batch=rpb, gn_cpg=C // 32, tile=11, splits=1)
    out1 = ops.gemm(gg, ops.pack_ff_proj_out(w2, b2, wp, bp, dev), a2=x2, residual=x_in, rows_per_batch=rpb, gn_cpg=C // 32, tile=11, splits=1)
    g0, g1 = ops.partials_of(out0), ops.partials_of(out1)
    assert g0 is not None and g1 is not None
    check_partials(g0, g1, out0)
    ref = (x_in.double().cpu() + bp.double() + (x2.double().cpu() + b2.double() + gg.double().cpu() @ w2.double().t()) @ wp.double().t()).numpy()
    e0, e1 = rel_l2(out0.double().cpu().numpy(), ref), rel_l2(out1.double().cpu().numpy(), ref)
    print(f"fold proj_out launch M={M} C={C}: rel_l2 vs fp64 two-launch {e0:.3e}, folded {e1:.3e}")
    assert e1 <= 1.5 * e0


@pytest.mark.gpu
def test_in_place_weight_change_repacks(dev, monkeypatch):
    """A merged LoRA writes ff.net[2].weight in place: the folded pack is keyed on the four parameters and follows."""
    C, B, H = 1280, 2, 8
    st, _ = block(C)
    x, ctx, _ = case(C, B, H)
    before, _ = run(st, x, ctx, True, monkeypatch, dev)
    lin = st.transformer_blocks[-1].ff.net[2]
    saved = lin.weight.detach().clone()
    try:
        with torch.no_grad():
            lin.weight.mul_(1.5)
        after, _ = run(st, x, ctx, True, monkeypatch, dev)
        two, _ = run(st, x, ctx, False, monkeypatch, dev)
        stale = rel_l2(nchw(before), nchw(two))               # where a pack that did not follow would leave the output
        assert stale > 1e-2                                   # the change is visible ...
        assert rel_l2(nchw(after), nchw(two)) < 0.1 * stale   # ... and the folded form went with the two-launch form, which reads the parameter's own pack
    finally:
        with torch.no_grad():
            lin.weight.copy_(saved)
