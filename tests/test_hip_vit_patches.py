"""af_vit_patch_rows and af_gelu_f16 on a real MI355X (`pytest -m gpu`), through the C entry points (INTEGRATION.md "Scoring images").

af_vit_patch_rows.  The reference is tests/vit_restatement.py in fp64: F.interpolate(antialias=True) on the 0 .. 255 values, crop, affine,
unfold; nothing in it comes from the kernel.  Bound per case (fp16 output, the project's own for such kernels, test_hip_hint_conv.py):
2^-10 max|ref| + 4 e32 -- one fp16 rounding of the output (2^-11 relative) with room, and e32 = the largest error of the same reference
evaluated in fp32 on the CPU against fp64 (the kernel sums in fp32 too, in another order).  The output is a sentinel-filled tensor of the
exact size at the front of a larger allocation whose tail must keep the sentinel; pad columns must be exactly zero.

af_gelu_f16: fp64 reference, 2^-10 max(|ref|, 2^-14) per element: one fp16 rounding (2^-11 relative; 2^-25 absolute below the normal
range) with room."""
import ctypes
import math

import pytest
import torch

import vit_restatement as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7ABC          # an fp16 bit pattern (finite, 54144.0) no result takes
TAIL = 4096
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)

# (H, W), keep_aspect, S, C, p, kpad
CASES = {
    "odd_37x53": ((37, 53), 1, 16, 16, 8, 192),              # odd sizes, W % 4 != 0, ratio about 2.3
    "left6_96x130": ((96, 130), 1, 32, 32, 8, 192),          # half-to-even left = 6
    "left4_39x50": ((39, 50), 1, 32, 32, 8, 192),            # half-to-even left = 4
    "portrait_64x48": ((64, 48), 1, 32, 32, 16, 768),        # top = 5
    "upsize_20x28": ((20, 28), 1, 32, 32, 8, 192),           # taps clipped at the border, cubic overshoot
    "identity_32x32": ((32, 32), 1, 32, 32, 8, 192),
    "kpad640_300x70": ((300, 70), 1, 28, 28, 14, 640),       # 588 -> 640; ratio 2.5, a long tail cropped away
    "aniso_450x41": ((450, 41), 0, 0, 32, 8, 192),           # ratios of about 14 and 1.3 in one call
    "constant_1x1": ((1, 1), 0, 0, 16, 8, 192),
    # beyond the issue's table: the paths the kernel takes at other sizes
    "p32_chunks_200x180": ((200, 180), 1, 64, 64, 32, 3072),   # p = 32: four pixels per lane, 42-row chunks (two per patch)
    "wide_8x30000": ((8, 30000), 0, 0, 16, 8, 192),            # one footprint row does not fit the staging buffer: direct reads
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def make_images(H, W, seed):
    """B = 2 different images: seeded noise; the second also carries hard black / white blocks (what makes a cubic overshoot)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    if H >= 8 and W >= 8:
        img[1, : H // 2, : W // 2] = 0
        img[1, : H // 2, W // 2:] = 255
        img[1, H // 2:, : W // 2] = 255
    return img


def run(dev, img, keep, S, C, p, filt, kpad, scale3, shift3, img_offset=0):
    """One call into the front of a sentinel-filled allocation -> (rows [B P, kpad] fp16, tail) on the CPU.  img_offset: the image starts that
    many bytes into its allocation (a base that is not 4-byte aligned)."""
    from adaface_dev_amd import _lib
    L = _lib.lib()
    B, H, W, _ = img.shape
    n = B * (C // p) ** 2 * kpad
    buf = torch.empty(n + TAIL, dtype=torch.int16, device=dev).fill_(SENTINEL)
    holder = torch.zeros(img.numel() + 16, dtype=torch.uint8, device=dev)
    holder[img_offset:img_offset + img.numel()] = img.reshape(-1).to(dev)
    f3 = ctypes.c_float * 3
    rc = L.af_vit_patch_rows(holder.data_ptr() + img_offset, buf.data_ptr(), B, H, W, keep, S, C, p, filt, f3(*scale3), f3(*shift3), kpad, None)
    torch.cuda.synchronize()
    assert rc == 0, L.af_last_error()
    buf = buf.cpu()
    return buf[:n].view(torch.float16).reshape(-1, kpad), buf[n:]


def check(dev, name, filt, img_offset=0):
    (H, W), keep, S, C, p, kpad = CASES[name]
    img = make_images(H, W, seed=len(name) + 7 * filt)
    scale3, shift3 = R.scale_shift(CLIP_MEAN, CLIP_STD)
    got, tail = run(dev, img, keep, S, C, p, filt, kpad, scale3, shift3, img_offset)
    pix64, raw64 = R.preprocess_ref(img, keep, S, C, filt, scale3, shift3, torch.float64)
    pix32, _ = R.preprocess_ref(img, keep, S, C, filt, scale3, shift3, torch.float32)
    ref = R.rows_ref(pix64, p, kpad)
    e32 = float((pix32.double() - pix64).abs().max())
    bound = 2.0 ** -10 * float(ref.abs().max()) + 4 * e32
    err = float((got.double() - ref).abs().max())
    print(f"{name} filter {filt}: err {err:.3e} bound {bound:.3e} (max|ref| {float(ref.abs().max()):.3f}, e32 {e32:.2e})")
    assert got.shape == ref.shape
    assert bool((tail == SENTINEL).all()), "the kernel wrote behind its output"
    assert not bool((got.view(torch.int16) == SENTINEL).any()), "an output element was not written"
    assert bool((got[:, 3 * p * p:].view(torch.int16) == 0).all()), "pad columns must be exactly zero"
    assert torch.isfinite(got.float()).all()
    assert err <= bound, (name, filt, err, bound)
    return img, got, raw64


@pytest.mark.parametrize("filt", [0, 1], ids=["triangle", "cubic"])
@pytest.mark.parametrize("name", list(CASES))
def test_patch_rows(dev, name, filt):
    img, got, raw64 = check(dev, name, filt)
    (H, W), keep, S, C, p, kpad = CASES[name]
    if name == "upsize_20x28" and filt == 1:
        assert float(raw64.min()) < -1.0 and float(raw64.max()) > 256.0, "the case must hold cubic overshoot on both sides"
    if name == "identity_32x32":
        scale3, shift3 = R.scale_shift(CLIP_MEAN, CLIP_STD)
        v = img.permute(0, 3, 1, 2).float()
        want = (v * torch.tensor(scale3).view(1, 3, 1, 1) + torch.tensor(shift3).view(1, 3, 1, 1)).half()       # fp32 multiply, fp32 add, one rounding
        assert torch.equal(got[:, :3 * p * p], R.rows_ref(want, p, kpad)[:, :3 * p * p]), "at ratio 1 every value is fp16(v * scale + shift)"
    if name == "constant_1x1":
        for b in range(2):
            for c in range(3):
                assert len(torch.unique(got[b * 4:(b + 1) * 4, c * 64:(c + 1) * 64])) == 1


@pytest.mark.parametrize("filt", [0, 1], ids=["triangle", "cubic"])
def test_unaligned_image_base(dev, filt):
    """An image that starts one byte into its allocation cannot be staged with aligned dword loads: the direct-read path, same result."""
    check(dev, "odd_37x53", filt, img_offset=1)
    check(dev, "kpad640_300x70", filt, img_offset=3)


def test_half_to_even_crops_differ_from_half_up(dev):
    """The two crop cases really pin the rounding: the neighbouring offset gives another result."""
    for name, other in (("left6_96x130", 5), ("left4_39x50", 5)):
        (H, W), keep, S, C, p, kpad = CASES[name]
        img = make_images(H, W, seed=len(name))
        scale3, shift3 = R.scale_shift(CLIP_MEAN, CLIP_STD)
        got, _ = run(dev, img, keep, S, C, p, 0, kpad, scale3, shift3)
        Hr, Wr, top, left = R.resize_geometry(H, W, keep, S, C)
        raw = torch.nn.functional.interpolate(img.permute(0, 3, 1, 2).double(), size=(Hr, Wr), mode="bilinear", antialias=True)
        sc, sh = torch.tensor(scale3).double().view(1, 3, 1, 1), torch.tensor(shift3).double().view(1, 3, 1, 1)
        wrong = R.rows_ref(raw[:, :, top:top + C, other:other + C] * sc + sh, p, kpad)
        assert float((got.double() - wrong).abs().max()) > 0.1


def test_bad_arguments_leave_the_output_untouched(dev):
    from adaface_dev_amd import _lib
    L = _lib.lib()
    f3 = ctypes.c_float * 3
    sc, sh = f3(1, 1, 1), f3(0, 0, 0)
    img = make_images(37, 53, 1).to(dev)
    out = torch.empty(2 * 4 * 192 + TAIL, dtype=torch.int16, device=dev).fill_(SENTINEL)
    ok = dict(img=img.data_ptr(), rows=out.data_ptr(), B=2, H=37, W=53, keep=1, S=16, C=16, p=8, filt=1, sc=sc, sh=sh, kpad=192)
    bad = [dict(img=None), dict(rows=None), dict(sc=None), dict(sh=None), dict(C=12), dict(C=24, S=16), dict(kpad=184), dict(kpad=196), dict(filt=2),
           dict(B=2 ** 20, H=32, W=32), dict(kpad=2 ** 28)]
    for kw in bad:
        a = dict(ok, **kw)
        rc = L.af_vit_patch_rows(a["img"], a["rows"], a["B"], a["H"], a["W"], a["keep"], a["S"], a["C"], a["p"], a["filt"], a["sc"], a["sh"], a["kpad"], None)
        assert rc == _lib.AF_E_BADARG and b"af_vit_patch_rows" in L.af_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())


def test_ops_wrapper_matches_the_entry_point(dev):
    from adaface_dev_amd import ops
    (H, W), keep, S, C, p, kpad = CASES["kpad640_300x70"]
    img = make_images(H, W, seed=3)
    scale3, shift3 = R.scale_shift(CLIP_MEAN, CLIP_STD)
    got, _ = run(dev, img, keep, S, C, p, 1, kpad, scale3, shift3)
    rows = ops.vit_patch_rows(img.to(dev), keep_aspect=True, S=S, C=C, p=p, filter="bicubic", mean=CLIP_MEAN, std=CLIP_STD)
    torch.cuda.synchronize()
    assert rows.shape == (2 * 4, 640) and torch.equal(rows.cpu(), got)


# ---- af_gelu_f16 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 4099, 2 ** 16 + 3])
def test_gelu(dev, n):
    from adaface_dev_amd import _lib, ops
    special = torch.tensor([0.0, 65504.0, -65504.0, 1e-4, -1e-4, -0.0])
    x = torch.cat([special, torch.linspace(-6, 6, max(n, 7))])[:n] if n >= 7 else special[[3, 0, 1, 2, 4, 5][:n]]
    x = x.half()
    buf = torch.empty(n + TAIL, dtype=torch.int16, device=dev).fill_(SENTINEL)
    xd = x.to(dev)
    rc = _lib.lib().af_gelu_f16(xd.data_ptr(), buf.data_ptr(), n, None)
    torch.cuda.synchronize()
    assert rc == 0
    buf = buf.cpu()
    got, tail = buf[:n].view(torch.float16), buf[n:]
    xf = x.double()
    ref = xf * 0.5 * (1.0 + torch.erf(xf / math.sqrt(2.0)))
    bound = 2.0 ** -10 * torch.clamp(ref.abs(), min=2.0 ** -14)
    err = (got.double() - ref).abs()
    print(f"gelu n={n}: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((tail == SENTINEL).all()) and torch.isfinite(got.float()).all()
    assert bool((err <= bound).all()), (x[err > bound], got[err > bound], ref[err > bound])
    if n >= 8:
        assert torch.equal(ops.gelu(xd).cpu(), got)
        # an unaligned slice takes the element-wise path
        assert torch.equal(ops.gelu(xd[1:]).cpu(), got[1:])
        y1 = torch.empty(n + 1, dtype=torch.float16, device=dev)
        assert _lib.lib().af_gelu_f16(xd.data_ptr(), y1[1:].data_ptr(), n, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(y1[1:].cpu(), got)
