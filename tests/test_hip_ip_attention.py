"""``af_ip_attention_add`` on a real MI355X (`pytest -m gpu`): IP-Adapter's image-token softmax added in place to the text attention's
output, called through the C entry point.

Reference: fp64 on the CPU from the same fp16 inputs (q, k, v and the incoming o); nothing in it comes from the kernel.  Bound per case:
``2^-10 * |s| * max|v| + 2^-11 * max|ref| + 4 * e32`` -- the first term is one fp16 rounding of P (relative 2^-11, sum_t p_t |v_t| <= max|v|)
plus slack of the same size, the second the single rounding of the output, ``e32`` the largest error of a plain fp32 torch CPU evaluation
against the fp64 reference (room for another summation order).  The kernel rounds nowhere else: o is widened to fp32 and summed there.

Shapes are the smallest at which the kernel takes another path: one key; a query tail inside the only 16-query tile with the smallest head
dim; the stock 4 tokens with a partial 32-channel step; 16 keys (one full key tile) read as column slices of a wider stacked tensor with a
batch stride; 64 keys (four key tiles) at the largest head dim with padded q / o rows; one query with an odd T.  Two cases were added for
edges of this tiling: ``two_key_tiles`` (17 <= T <= 32 runs a two-tile instantiation, and its N = 70 leaves three waves of the second
workgroup partly or wholly idle) and ``many_workgroups_query_tail`` (17 workgroups of 64 queries per head, the last with 6 live rows)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (B, N, T, heads, d, ldq - C, ldo - C, stacked k / v)
CASES = {
    "one_key": (1, 64, 1, 2, 24, 0, 0, False),
    "query_tail_smallest_d": (1, 37, 4, 2, 8, 0, 0, False),
    "stock": (1, 64, 4, 8, 40, 0, 0, False),
    "stacked_kv_batch_stride": (2, 128, 16, 8, 80, 0, 0, True),
    "max_T_max_d_padded": (2, 64, 64, 8, 160, 16, 8, False),
    "one_query_odd_T": (1, 1, 5, 3, 48, 0, 0, False),
    "two_key_tiles": (1, 70, 20, 2, 40, 0, 8, False),
    "many_workgroups_query_tail": (1, 1030, 4, 1, 16, 8, 0, True),
}
SENTINEL = 777.0
EXTRA_ROWS = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _inputs(name):
    """q [B*N, C + qpad], o [B*N + EXTRA_ROWS, C + opad] (pad columns and extra rows hold the sentinel), k / v [B, T, C] views (column slices of
    one wider [B, T + 2, 3 C + 8] tensor when stacked), all fp16 on the CPU."""
    B, N, T, heads, d, qpad, opad, stacked = CASES[name]
    C = heads * d
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    q = torch.randn((B * N, C + qpad), generator=g).to(torch.float16)
    o = torch.full((B * N + EXTRA_ROWS, C + opad), SENTINEL, dtype=torch.float16)
    o[:B * N, :C] = torch.randn((B * N, C), generator=g).to(torch.float16)
    if stacked:
        kv = torch.randn((B, T + 2, 3 * C + 8), generator=g).to(torch.float16)
        k, v = kv[:, :T, 8:8 + C], kv[:, :T, 8 + 2 * C:8 + 3 * C]
    else:
        k = torch.randn((B, T, C), generator=g).to(torch.float16)
        v = torch.randn((B, T, C), generator=g).to(torch.float16)
    return q, o, k, v


def _reference(q, o, k, v, B, N, heads, d, scale, ip_scale, dtype):
    """o + ip_scale * softmax(scale q k^T) v per (b, h) in ``dtype`` on the CPU -> [B*N, C]."""
    C, T = heads * d, k.shape[1]
    qh = q[:, :C].to(dtype).reshape(B, N, heads, d).permute(0, 2, 1, 3)
    kh = k.to(dtype).reshape(B, T, heads, d).permute(0, 2, 1, 3)
    vh = v.to(dtype).reshape(B, T, heads, d).permute(0, 2, 1, 3)
    p = torch.softmax((qh @ kh.transpose(-1, -2)) * scale, dim=-1)
    return o[:B * N, :C].to(dtype) + ip_scale * (p @ vh).permute(0, 2, 1, 3).reshape(B * N, C)


def _view_on(dev, t):
    """``t`` on the device with the strides and offset it has on the CPU (a slice stays a slice of its copied base)."""
    base = t if t._base is None else t._base
    return base.to(dev).as_strided(t.shape, t.stride(), t.storage_offset())


def _run(dev, q, o, k, v, B, N, heads, d, scale, ip_scale):
    """The entry point on device copies that keep the CPU tensors' strides -> the whole o buffer back on the CPU."""
    from adaface_dev_amd import _lib, ops
    qd, od = q.to(dev), o.to(dev)
    kd, vd = _view_on(dev, k), _view_on(dev, v)
    rc = _lib.lib().af_ip_attention_add(od.data_ptr(), od.stride(0), qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(1), kd.stride(0),
                                        vd.data_ptr(), vd.stride(1), vd.stride(0), B, N, k.shape[1], heads, d, float(scale), float(ip_scale),
                                        ops._stream())
    _lib.check(rc, "af_ip_attention_add")
    torch.cuda.synchronize()
    return od.cpu()


def _check(dev, name, ip_scale=1.0, q_amp=None):
    B, N, T, heads, d, _, _, _ = CASES[name]
    C = heads * d
    q, o, k, v = _inputs(name)
    scale = d ** -0.5
    if q_amp is not None:                      # amplify q so that the largest |score| is q_amp, then work from the fp16 q the kernel sees
        qh = q[:, :C].double().reshape(B, N, heads, d).permute(0, 2, 1, 3)
        kh = k.double().reshape(B, T, heads, d).permute(0, 2, 1, 3)
        smax = float(((qh @ kh.transpose(-1, -2)) * scale).abs().max())
        q = (q.float() * (q_amp / smax)).to(torch.float16)
        assert bool(torch.isfinite(q).all())
    ref = _reference(q, o, k, v, B, N, heads, d, scale, ip_scale, torch.float64)
    e32 = float((_reference(q, o, k, v, B, N, heads, d, scale, ip_scale, torch.float32).double() - ref).abs().max())
    vmax = float(v.abs().max())
    bound = 2.0 ** -10 * abs(ip_scale) * vmax + 2.0 ** -11 * float(ref.abs().max()) + 4 * e32
    out = _run(dev, q, o, k, v, B, N, heads, d, scale, ip_scale)
    got = out[:B * N, :C]
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - ref).abs().max())
    print(f"af_ip_attention_add {name} s={ip_scale} amp={q_amp}: max err {err:.3e}, bound {bound:.3e} (max|v| {vmax:.3f}, e32 {e32:.3e})")
    assert err <= bound
    # pad columns and the rows past B*N keep the sentinel
    assert bool((out[:, C:] == SENTINEL).all()) and bool((out[B * N:] == SENTINEL).all())
    return q, o, k, v, out


@pytest.mark.parametrize("name", list(CASES))
def test_ip_attention_add_vs_fp64(dev, name):
    q, o, k, v, out = _check(dev, name)
    if name == "one_key":              # softmax over one key is 1: the result is fp16(o + v)
        B, N, T, heads, d = CASES[name][:5]
        C = heads * d
        want = (o[:B * N, :C].float() + v.reshape(B, 1, C).float().expand(B, N, C).reshape(B * N, C)).to(torch.float16)
        assert torch.equal(out[:B * N, :C], want)


@pytest.mark.parametrize("name", ["stock", "max_T_max_d_padded"])
@pytest.mark.parametrize("ip_scale", [0.5, -1.25])
def test_ip_attention_add_scales(dev, name, ip_scale):
    _check(dev, name, ip_scale=ip_scale)


@pytest.mark.parametrize("name", ["query_tail_smallest_d", "stock", "stacked_kv_batch_stride", "max_T_max_d_padded", "two_key_tiles"])
def test_ip_attention_add_large_scores(dev, name):
    """q amplified so that the scores reach +-60: the exponentials span e^-120 .. 1, nothing overflows and the same bound holds."""
    _check(dev, name, q_amp=60.0)


def test_ip_attention_add_zero_scale_leaves_o_bit_identical(dev):
    B, N, T, heads, d = CASES["stock"][:5]
    q, o, k, v = _inputs("stock")
    out = _run(dev, q, o, k, v, B, N, heads, d, d ** -0.5, 0.0)
    assert torch.equal(out, o)


def test_ip_attention_add_ops_wrapper_matches_entry_point(dev):
    from adaface_dev_amd import ops
    name = "stacked_kv_batch_stride"
    B, N, T, heads, d = CASES[name][:5]
    q, o, k, v = _inputs(name)
    want = _run(dev, q, o, k, v, B, N, heads, d, d ** -0.5, 0.75)
    kd, vd = _view_on(dev, k), _view_on(dev, v)
    od = o.to(dev)
    got = ops.ip_attention_add(od[:B * N], q.to(dev), kd, vd, B=B, N=N, heads=heads, d=d, ip_scale=0.75)
    assert got.data_ptr() == od.data_ptr()
    assert torch.equal(od.cpu(), want)


BADARGS = ["T0", "T65", "d12", "d168", "N0", "ldq_small", "ldo_odd", "ldk_small", "vbs_odd", "null_o", "null_q", "null_k", "null_v",
           "misaligned_k", "q_2p31", "k_2p31"]


@pytest.mark.parametrize("what", BADARGS)
def test_ip_attention_add_refusals_leave_o_untouched(dev, what):
    from adaface_dev_amd import _lib, ops
    B, N, T, heads, d = 1, 8, 4, 2, 16
    C = heads * d
    q = torch.zeros((B * N, C), dtype=torch.float16, device=dev)
    k = torch.zeros((B, 65, C + 8), dtype=torch.float16, device=dev)
    v = torch.zeros((B, 65, C + 8), dtype=torch.float16, device=dev)
    o = torch.full((B * N, C), SENTINEL, dtype=torch.float16, device=dev)
    a = dict(o=o.data_ptr(), ldo=C, q=q.data_ptr(), ldq=C, k=k.data_ptr(), ldk=C + 8, kbs=65 * (C + 8), v=v.data_ptr(), ldv=C + 8, vbs=65 * (C + 8),
             B=B, N=N, T=T, heads=heads, d=d)
    a.update({"T0": dict(T=0), "T65": dict(T=65), "d12": dict(d=12), "d168": dict(d=168), "N0": dict(N=0), "ldq_small": dict(ldq=C - 8),
              "ldo_odd": dict(ldo=C + 4), "ldk_small": dict(ldk=C - 8), "vbs_odd": dict(vbs=65 * (C + 8) + 4), "null_o": dict(o=None),
              "null_q": dict(q=None), "null_k": dict(k=None), "null_v": dict(v=None), "misaligned_k": dict(k=k.data_ptr() + 8),
              "q_2p31": dict(B=2048, N=1 << 15, ldq=32), "k_2p31": dict(B=3, kbs=(1 << 30))}[what])
    rc = _lib.lib().af_ip_attention_add(a["o"], a["ldo"], a["q"], a["ldq"], a["k"], a["ldk"], a["kbs"], a["v"], a["ldv"], a["vbs"], a["B"], a["N"],
                                        a["T"], a["heads"], a["d"], ctypes.c_float(0.25), ctypes.c_float(1.0), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.AF_E_BADARG
    assert bool((o == SENTINEL).all())
