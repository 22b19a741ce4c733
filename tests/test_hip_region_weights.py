"""``af_region_weights`` on a real MI355X (`pytest -m gpu`): uint8 region masks -> the four U-Net levels' normalised fp32 weights in one launch.

Reference: the Python restatement below (``F.avg_pool2d`` of each mask onto the level's token grid, then the rule
``w_r = (1 - beta) m_r / max(1, s)``, ``w_0 = beta + (1 - beta)(1 - min(1, s))``, ``s = sum_r m_r``) in fp32 on the CPU.  The 8-bit sums of a
cell are integers below 2^24, so they (and their division by the power-of-two area) are exact in fp32 whatever the summation order; what is
left are the few fp32 operations of the rule, so agreement is asked to 2 ulp.  Rows sum to 1 within 1e-6, and a cell that no pixel of a mask
touches holds exactly 0.0 in that region's row (the attention kernel's skip relies on it)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H, W = 64, 128
BETAS = [0.0, 0.2, 1.0]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def restated_region_weights(masks_u8, beta):
    """masks uint8 [R-1, H, W] -> four fp32 [R, N_l] (level l: cells of 8 * 2^l pixels, row-major)."""
    out = []
    m255 = masks_u8.to(torch.float32)[None]                              # [1, R-1, H, W], integer-valued
    for lvl in range(4):
        cell = 8 << lvl
        m = (F.avg_pool2d(m255, cell) / 255.0)[0].reshape(masks_u8.shape[0], -1)      # [R-1, N_l]
        s = torch.zeros_like(m[0])
        for r in range(m.shape[0]):
            s = s + m[r]
        nb = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(beta, dtype=torch.float32)
        regions = nb * m / torch.clamp(s, min=1.0)
        base = torch.tensor(beta, dtype=torch.float32) + nb * (1.0 - torch.clamp(s, max=1.0))
        out.append(torch.cat([base[None], regions], 0))
    return out


@pytest.fixture(scope="module")
def masks():
    """Three overlapping masks on 64 x 128: a hard left part whose edge cuts 8-pixel cells, a soft (random grey) disc over the middle that
    overlaps it, and a band that overlaps both; the right 24 columns and the top 8 rows are touched by none."""
    g = torch.Generator().manual_seed(64128)
    m = torch.zeros((3, H, W), dtype=torch.uint8)
    m[0, 8:, :61] = 255
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disc = ((yy - 36) ** 2 + (xx - 60) ** 2) < 24 ** 2
    m[1][disc] = torch.randint(1, 256, (int(disc.sum()),), generator=g, dtype=torch.uint8)
    m[2, 40:56, 20:104] = 200
    return m


@pytest.mark.parametrize("beta", BETAS)
def test_region_weights_match_the_restatement(dev, masks, beta):
    from adaface_dev_amd import ops
    w, levels = ops.region_weights(masks.to(dev), beta)
    torch.cuda.synchronize()
    want = restated_region_weights(masks, beta)
    sizes = ops.region_level_sizes(H, W)
    assert sizes == [128, 32, 8, 2] and tuple(w.shape) == (4, 170)
    for lvl, (got, ref) in enumerate(zip(levels, want)):
        got = got.cpu()
        assert tuple(got.shape) == (4, sizes[lvl]) == tuple(ref.shape)
        ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -126)) * 2.0 ** -23
        worst = float(((got - ref).abs() / ulp).max())
        print(f"af_region_weights beta={beta} level {lvl}: worst difference {worst:.2f} ulp")
        assert worst <= 2.0
        assert float((got.double().sum(0) - 1.0).abs().max()) <= 1e-6
        # exact zeros outside each mask
        cell = 8 << lvl
        touched = F.max_pool2d(masks.to(torch.float32)[None], cell)[0].reshape(3, -1) > 0
        assert bool((got[1:][~touched] == 0.0).all())
        assert int((~touched).sum()) > 0 or lvl == 3
        if beta < 1.0:
            assert bool((got[1:][touched] > 0.0).all())


def test_region_weights_no_region_is_all_base(dev):
    from adaface_dev_amd import ops
    w, levels = ops.region_weights(None, 0.2, H=H, W=W, device=dev)
    torch.cuda.synchronize()
    assert tuple(w.shape) == (1, 170) and bool((w == 1.0).all())


@pytest.mark.parametrize("what", ["H_not_64", "W_small", "R9", "beta_neg", "beta_big", "ldw_small", "null_w", "null_masks"])
def test_region_weights_refusals_leave_w_untouched(dev, masks, what):
    import ctypes

    from adaface_dev_amd import _lib, ops
    md = masks.to(dev)
    w = torch.full((4, 170), 777.0, dtype=torch.float32, device=dev)
    a = dict(masks=md.data_ptr(), R=4, H=H, W=W, beta=0.2, w=w.data_ptr(), ldw=170)
    a.update({"H_not_64": dict(H=72), "W_small": dict(W=32), "R9": dict(R=9), "beta_neg": dict(beta=-0.1), "beta_big": dict(beta=1.5),
              "ldw_small": dict(ldw=169), "null_w": dict(w=None), "null_masks": dict(masks=None)}[what])
    rc = _lib.lib().af_region_weights(a["masks"], a["R"], a["H"], a["W"], ctypes.c_float(a["beta"]), a["w"], a["ldw"], ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.AF_E_BADARG
    assert bool((w == 777.0).all())
