"""``af_temporal_attention`` on a real MI355X (`pytest -m gpu`): self-attention along the frame axis, called through the C entry point.

Reference: fp64 on the CPU from the same fp16-rounded inputs; nothing in it comes from the kernel.  Bound per case:
``2^-10 * max|v| + 4 * e32`` -- the first term is one fp16 rounding of P (relative 2^-11, |out| <= max|v|) plus one of the output, ``e32`` is
the largest error of a plain fp32 torch CPU evaluation against the fp64 reference (room for another summation order).

Shapes are the smallest at which the kernel takes another path: one 16-frame tile and two, a frame tail, a pixel count that leaves waves of
the last workgroup idle, head dims that fill 1, 2 and 5 channel steps (40 and 24 leave a partial step), padded rows, one token per frame."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (B, F, HW, heads, d, ld - 3C)
CASES = {
    "one_frame": (1, 1, 64, 2, 24, 0),
    "frame_tail_pixel_tail": (1, 7, 37, 2, 8, 0),
    "typical": (1, 16, 64, 8, 40, 0),
    "max_frames_max_dim_padded": (2, 32, 64, 8, 160, 8),
    "one_token_per_frame": (1, 24, 1, 3, 48, 0),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _inputs(name, amp=1.0):
    B, F, HW, heads, d, pad = CASES[name]
    C = heads * d
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    qkv = torch.randn((B * F * HW, 3 * C + pad), generator=g)
    qkv[:, :2 * C] *= amp
    return qkv.to(torch.float16)


def _reference(qkv, B, F, HW, heads, d, scale, dtype):
    """softmax over the frames of each (b, p, h) in ``dtype`` on the CPU -> [B*F*HW, C]."""
    C = heads * d
    x = qkv[:, :3 * C].to(dtype).reshape(B, F, HW, 3, heads, d)
    q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))          # [B, HW, heads, F, d]
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return (p @ v).permute(0, 3, 1, 2, 4).reshape(B * F * HW, C)


def _run(dev, qkv, B, F, HW, heads, d, scale):
    from adaface_dev_amd import _lib, ops
    x = qkv.to(dev)
    out = torch.full((B * F * HW, heads * d), 777.0, dtype=torch.float16, device=dev)
    rc = _lib.lib().af_temporal_attention(x.data_ptr(), x.stride(0), out.data_ptr(), B, F, HW, heads, d, float(scale), ops._stream())
    _lib.check(rc, "af_temporal_attention")
    torch.cuda.synchronize()
    return out.cpu()


def _check(dev, name, amp=1.0, scale=None):
    B, F, HW, heads, d, _ = CASES[name]
    qkv = _inputs(name, amp)
    scale = d ** -0.5 if scale is None else scale
    ref = _reference(qkv, B, F, HW, heads, d, scale, torch.float64)
    e32 = float((_reference(qkv, B, F, HW, heads, d, scale, torch.float32).double() - ref).abs().max())
    vmax = float(qkv[:, 2 * heads * d:3 * heads * d].abs().max())
    bound = 2.0 ** -10 * vmax + 4 * e32
    out = _run(dev, qkv, B, F, HW, heads, d, scale)
    assert bool(torch.isfinite(out).all())
    err = float((out.double() - ref).abs().max())
    print(f"af_temporal_attention {name}: max err {err:.3e}, bound {bound:.3e} (max|v| {vmax:.3f}, e32 {e32:.3e})")
    assert err <= bound
    return qkv, out, ref


@pytest.mark.parametrize("name", list(CASES))
def test_temporal_attention_vs_fp64(dev, name):
    qkv, out, _ = _check(dev, name)
    if name == "one_frame":            # softmax over one key is 1: the output is v, within one fp16 ulp
        C = CASES[name][3] * CASES[name][4]
        v = qkv[:, 2 * C:3 * C]
        ulp = torch.maximum(torch.nextafter(v.abs(), torch.full_like(v, 65504.0)).float() - v.abs().float(), torch.tensor(2.0 ** -24))
        assert bool(((out.float() - v.float()).abs() <= ulp).all())


@pytest.mark.parametrize("name", ["frame_tail_pixel_tail", "typical", "max_frames_max_dim_padded"])
def test_temporal_attention_large_scores(dev, name):
    """Scores scaled so that the largest reaches +-30: the exponentials span e^-60 .. 1, nothing overflows and the bound still holds."""
    B, F, HW, heads, d, _ = CASES[name]
    qkv = _inputs(name)
    C = heads * d
    x = qkv[:, :3 * C].double().reshape(B, F, HW, 3, heads, d)
    q, k = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(2))
    smax = float((q @ k.transpose(-1, -2)).abs().max())
    _check(dev, name, scale=30.0 / smax)


def test_temporal_attention_ops_wrapper_matches_entry_point(dev):
    from adaface_dev_amd import ops
    B, F, HW, heads, d, _ = CASES["typical"]
    qkv = _inputs("typical")
    want = _run(dev, qkv, B, F, HW, heads, d, d ** -0.5)
    got = ops.temporal_attention(qkv.to(dev), B=B, F=F, HW=HW, heads=heads, d=d)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("what", ["F0", "F33", "d12", "ld_small", "null_qkv", "null_out"])
def test_temporal_attention_refusals_leave_the_output_untouched(dev, what):
    from adaface_dev_amd import _lib, ops
    B, F, HW, heads, d = 1, 4, 8, 2, 16
    C = heads * d
    x = torch.zeros((B * 33 * HW, 3 * C), dtype=torch.float16, device=dev)
    out = torch.full((B * 33 * HW, C), 777.0, dtype=torch.float16, device=dev)
    xp, op, ld = x.data_ptr(), out.data_ptr(), 3 * C
    if what == "F0":
        F = 0
    elif what == "F33":
        F = 33
    elif what == "d12":
        d = 12
    elif what == "ld_small":
        ld = 3 * C - 8
    elif what == "null_qkv":
        xp = None
    else:
        op = None
    rc = _lib.lib().af_temporal_attention(xp, ld, op, B, F, HW, heads, d, ctypes.c_float(0.25), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.AF_E_BADARG
    assert bool((out == 777.0).all())
