"""FreeU on the CPU in fp64, for the tests: the authors' ``torch.fft`` composition, the closed form the kernels implement (with the two
wrong variants the GPU test uses to show that its bound can fail) and the whole rule on NHWC fp16 inputs.  No GPU, no kernels."""
import numpy as np
import torch

F16_MAX = 65504.0


def fourier_filter_fft(x, threshold, scale):
    """The authors' ``Fourier_filter`` (FreeU's patch of the ldm / diffusers U-Net), x [B, C, H, W] -> the same shape, in x's precision."""
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    B, C, H, W = x_freq.shape
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def bins(H, W, diag_v=-1, drop=None):
    """The scaled DFT bins {0, -1 mod H} x {0, -1 mod W} as (u, v) with u, v in {0, -1}: four, two when a side is 1, one at 1 x 1.
    ``diag_v=+1`` replaces the diagonal bin (-1, -1) by (-1, +1) and ``drop=(u, v)`` leaves one bin out: the two faults the GPU test's bound is
    shown to catch."""
    out = []
    for u in ([0, -1] if H > 1 else [0]):
        for v in ([0, -1] if W > 1 else [0]):
            if (u, v) == drop:
                continue
            out.append((u, diag_v) if (u, v) == (-1, -1) else (u, v))
    return out


def lowpass_closed(x, s, diag_v=-1, drop=None):
    """The closed form, x fp64 [B, H, W, C] (NHWC) -> y:
        y[h, w] = x[h, w] + (s - 1) / (H W) * sum_bins (A cos phi + B sin phi),  phi = 2 pi (u h / H + v w / W),  A = sum x cos phi,  B = sum x sin phi."""
    x = np.asarray(x, dtype=np.float64)
    _, H, W, _ = x.shape
    hh, ww = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    low = np.zeros_like(x)
    for u, v in bins(H, W, diag_v, drop):
        phi = 2.0 * np.pi * (u * hh / H + v * ww / W)
        c, sn = np.cos(phi), np.sin(phi)
        A = np.einsum("bhwc,hw->bc", x, c)
        Bq = np.einsum("bhwc,hw->bc", x, sn)
        low += A[:, None, None, :] * c[None, :, :, None] + Bq[:, None, None, :] * sn[None, :, :, None]
    return x + (s - 1.0) / (H * W) * low


def boost_factor(h, b, version):
    """The per-pixel factor of the backbone boost, h fp64 [B, H, W, C] -> [B, H, W, 1]: version 2: (b - 1) * mhat + 1 with mhat the channel mean
    scaled to [0, 1] per sample and 0 where the sample's mean is constant (hi == lo: the authors' code divides 0 by 0 there); version 1: b."""
    h = np.asarray(h, dtype=np.float64)
    if version == 1:
        return np.full(h.shape[:3] + (1,), float(b))
    m = h.mean(axis=3, keepdims=True)
    lo, hi = m.min(axis=(1, 2), keepdims=True), m.max(axis=(1, 2), keepdims=True)          # numpy's min / max hand a NaN on, as torch's do
    with np.errstate(invalid="ignore", divide="ignore"):
        mhat = np.where(hi == lo, 0.0, (m - lo) / (hi - lo))
    return (b - 1.0) * mhat + 1.0


def sat(x):
    """Finite values saturate at the fp16 maximum; NaN and Inf stay."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.clip(x, -F16_MAX, F16_MAX), x)


def freeu_ref(h16, skip16, b, s, version=2, diag_v=-1, drop=None):
    """FreeU restated in fp64 from the fp16 inputs (torch or numpy, NHWC) -> (h', skip') fp64, saturated but NOT rounded to fp16.
    b == 1 / s == 1 leave that tensor as it is.  A skip plane that holds a NaN or an Inf is NaN everywhere, as its DFT is."""
    h = np.asarray(h16.detach().cpu().numpy() if torch.is_tensor(h16) else h16, dtype=np.float64)
    k = np.asarray(skip16.detach().cpu().numpy() if torch.is_tensor(skip16) else skip16, dtype=np.float64)
    ho, ko = h.copy(), k.copy()
    if b != 1:
        C = h.shape[3]
        with np.errstate(invalid="ignore"):
            ho[..., :C // 2] = sat(h[..., :C // 2] * boost_factor(h, b, version))
    if s != 1:
        finite = np.isfinite(k).all(axis=(1, 2), keepdims=True)
        with np.errstate(invalid="ignore"):
            y = lowpass_closed(np.where(finite, k, 0.0), s, diag_v, drop)
        ko = sat(np.where(finite, y, np.nan))
    return ho, ko


def to_f16(x):
    """fp64 -> fp16 (round to nearest even) as a torch tensor."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(np.asarray(x, dtype=np.float64).astype(np.float16))
