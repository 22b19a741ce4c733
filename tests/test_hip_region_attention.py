"""``af_region_attention`` on a real MI355X (`pytest -m gpu`): the cross-attention core over R context sets per batch item, blended per query
under the region weights, called through the C entry point.

Reference: fp64 on the CPU from the same fp16 operands and fp32 weights; a set whose weight for a query is exactly 0 is SKIPPED for that
query there too (the zero-weight contract is a select).  Nothing in it comes from the kernel.  Bound, per output element:

    |o - ref| <= 2^-11 |ref| + 2^-10 sum_r w_r sum_t p_t |v_t| + 1e-6

the first term is the one rounding of o, the second the fp16 rounding of P (relative 2^-11 per p_t against the normalised fp32 row sum) with
slack of the same size.  The worst ratio err / bound of each case is printed (``-s``) and recorded in profiles/region_attention.txt.

Shapes are the smallest at which each mechanism can break: d in {8, 40, 80, 160} (one k-step, a partial 32-channel tile, a whole number of
tiles, the largest), heads in {1, 2, 8}, N in {1, 7, 64, 72, 200} (one query, a tail inside the first wave, half a 128-query tile, a tail in
the third wave, two tiles with a tail), L in {1, 77, 80}, R in {1, 2, 3, 8}, B in {1, 3}, padded q / o rows, k as a column slice of a wider
row, vt as a row slice with a larger batch stride, ldw > N."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (B, R, N, L, heads, d, ldq - C, ldo - C, k / vt as slices of a stacked tensor, ldw - N, weight pattern)
CASES = {
    "soft_d40_two_tiles": (1, 2, 200, 77, 8, 40, 0, 0, False, 0, "soft"),
    "hard_d80_three_sets_padded": (3, 3, 200, 77, 2, 80, 16, 8, False, 0, "hard"),
    "soft_d160_L80_sliced_kv_ldw": (1, 2, 72, 80, 2, 160, 0, 0, True, 24, "soft"),
    "one_query_one_key_d8_eight_sets": (1, 8, 1, 1, 1, 8, 0, 0, False, 0, "soft"),
    "soft_d8_heads2": (1, 2, 64, 77, 2, 8, 8, 0, False, 0, "soft"),
    "hard_N7_eight_sets_B3": (3, 8, 7, 77, 1, 40, 0, 0, True, 1, "hard"),
    "nan_set_zero_over_whole_tiles": (3, 3, 200, 77, 2, 40, 0, 0, False, 0, "nan_tiles"),
    "nan_v_zero_for_part_of_a_tile": (1, 2, 64, 77, 2, 40, 0, 0, False, 0, "nan_partial"),
    "all_zero_rows": (1, 2, 72, 77, 1, 80, 0, 8, False, 0, "zero_rows"),
    "one_set_weight_one": (1, 1, 200, 77, 8, 40, 0, 0, False, 0, "ones"),
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
    """q [B*N, C + qpad], o [B*N + EXTRA_ROWS, C + opad] full of the sentinel, k [B*R*L, C] rows (a column slice of a [.., 2 C + 8] tensor when
    sliced), vt [B*R, C, ldv] (a row slice of a [B*R, 2 C + 8, ldv] tensor when sliced), w fp32 [B*R, N + wpad]; all on the CPU."""
    B, R, N, L, heads, d, qpad, opad, sliced, wpad, pattern = CASES[name]
    C = heads * d
    ldv = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    q = torch.randn((B * N, C + qpad), generator=g).to(torch.float16)
    o = torch.full((B * N + EXTRA_ROWS, C + opad), SENTINEL, dtype=torch.float16)
    if sliced:
        k = torch.randn((B * R * L, 2 * C + 8), generator=g).to(torch.float16)[:, 8:8 + C]
        vt = torch.randn((B * R, 2 * C + 8, ldv), generator=g).to(torch.float16)[:, C:2 * C, :]
    else:
        k = torch.randn((B * R * L, C), generator=g).to(torch.float16)
        vt = torch.randn((B * R, C, ldv), generator=g).to(torch.float16)
    w = torch.full((B * R, N + wpad), 0.5)                    # the pad holds a weight the kernel must never read as a query's
    wv = w[:, :N].reshape(B, R, N)
    if pattern == "soft":                                     # a random point of the simplex per query, no exact zero
        e = torch.rand((B, R, N), generator=g) + 0.05
        wv.copy_(e / e.sum(1, keepdim=True))
    elif pattern == "ones":
        wv.fill_(1.0)
    elif pattern in ("hard", "zero_rows"):                    # a partition into R runs whose boundaries fall inside a tile (and move with b)
        wv.zero_()
        for b in range(B):
            for i in range(N):
                wv[b, min(R - 1, (i * R + b) // N), i] = 1.0
        if pattern == "zero_rows":
            wv[:, :, 5:9] = 0.0
            wv[:, :, N - 1] = 0.0
    elif pattern == "nan_tiles":
        # per batch item: set 0 everywhere, a live set blended with it in the first 128-query tile only, a dead set (which of 1 / 2 alternates with b)
        wv.zero_()
        for b in range(B):
            live, dead = (1, 2) if b % 2 == 0 else (2, 1)
            e = torch.rand((N,), generator=g) * 0.8 + 0.1
            wv[b, 0] = e
            wv[b, live, :128] = 1.0 - e[:128]                 # the live set reaches the first tile only: the second tile skips it
            wv[b, 0, 128:] = 1.0
            item = b * R + dead                               # the dead set is 0 over every tile and its K / V are NaN
            k[item * L:(item + 1) * L] = float("nan")
            vt[item] = float("nan")
    elif pattern == "nan_partial":
        e = torch.rand((N,), generator=g) * 0.8 + 0.1
        wv[0, 0] = e
        wv[0, 1] = 1.0 - e
        wv[0, 0, 10:41] = 1.0                                 # queries 10 .. 40 (parts of the first two waves) take nothing from set 1 ...
        wv[0, 1, 10:41] = 0.0
        vt[1, 3, 5] = float("nan")                            # ... whose V holds NaN and Inf
        vt[1, C - 1, 0] = float("inf")
    return q, o, k, vt, w


def _reference(q, k, vt, w, B, R, N, L, heads, d, scale, dtype=torch.float64):
    """(ref [B*N, C], mag [B*N, C] = sum_r w_r sum_t p_t |v_t|) in ``dtype`` on the CPU; set r is skipped for the queries whose weight is 0."""
    C = heads * d
    qh = q[:, :C].to(dtype).reshape(B, N, heads, d).permute(0, 2, 1, 3)                          # [B, h, N, d]
    kh = k.to(dtype).reshape(B, R, L, heads, d).permute(0, 1, 3, 2, 4)                             # [B, R, h, L, d]
    vh = vt[:, :, :L].to(dtype).reshape(B, R, heads, d, L).permute(0, 1, 2, 4, 3)                  # [B, R, h, L, d]
    ref = torch.zeros((B, heads, N, d), dtype=dtype)
    mag = torch.zeros_like(ref)
    for r in range(R):
        wr = w[:, :N].reshape(B, R, N)[:, r].to(dtype)[:, None, :, None]                           # [B, 1, N, 1]
        p = torch.softmax((qh @ kh[:, r].transpose(-1, -2)) * scale, dim=-1)
        take = wr != 0
        ref = torch.where(take, ref + wr * (p @ vh[:, r]), ref)
        mag = torch.where(take, mag + wr.abs() * (p @ vh[:, r].abs()), mag)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, C)
    return back(ref), back(mag)


def _view_on(dev, t):
    """``t`` on the device with the strides and offset it has on the CPU (a slice stays a slice of its copied base)."""
    base = t if t._base is None else t._base
    return base.to(dev).as_strided(t.shape, t.stride(), t.storage_offset())


def _run(dev, q, o, k, vt, w, B, R, N, L, heads, d, scale):
    """The entry point on device copies that keep the CPU tensors' strides -> the whole o buffer back on the CPU."""
    from adaface_dev_amd import _lib, ops
    qd, od, wd = q.to(dev), o.to(dev), w.to(dev)
    kd, vd = _view_on(dev, k), _view_on(dev, vt)
    rc = _lib.lib().af_region_attention(qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(1), vd.stride(0),
                                        wd.data_ptr(), wd.stride(0), od.data_ptr(), od.stride(0), B, R, N, L, heads, d, ctypes.c_float(scale),
                                        ops._stream())
    _lib.check(rc, "af_region_attention")
    torch.cuda.synchronize()
    return od.cpu()


def _bound(ref, mag):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -10 * mag + 1e-6


def _check(dev, name):
    B, R, N, L, heads, d = CASES[name][:6]
    C = heads * d
    q, o, k, vt, w = _inputs(name)
    scale = d ** -0.5
    ref, mag = _reference(q, k, vt, w, B, R, N, L, heads, d, scale)
    out = _run(dev, q, o, k, vt, w, B, R, N, L, heads, d, scale)
    got = out[:B * N, :C].double()
    ok = torch.isfinite(ref)                       # (only "nan_v_zero_for_part_of_a_tile" has non-finite reference elements: see its test)
    bound = _bound(ref, mag)
    ratio = float(((got - ref).abs()[ok] / bound[ok]).max())
    print(f"af_region_attention {name}: worst err / bound {ratio:.3f} (max err {float((got - ref).abs()[ok].max()):.3e})")
    assert bool(torch.isfinite(got[ok]).all())
    assert ratio <= 1.0
    # pad columns and the rows past B*N keep the sentinel
    assert bool((out[:, C:] == SENTINEL).all()) and bool((out[B * N:] == SENTINEL).all())
    return q, k, vt, w, out, ref, mag


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("nan_") and n not in ("all_zero_rows", "one_set_weight_one")])
def test_region_attention_vs_fp64(dev, name):
    _check(dev, name)


def test_region_attention_skips_a_nan_set_that_is_zero_over_whole_tiles(dev):
    """Per batch item one set has weight 0 for every query and NaN in all of its K and V; another reaches the first 128-query tile only.
    The output is finite everywhere and within the bound of the reference, which skips the set too."""
    name = "nan_set_zero_over_whole_tiles"
    B, R, N, L, heads, d = CASES[name][:6]
    _, _, _, _, out, ref, _ = _check(dev, name)
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(out[:B * N, :heads * d]).all())


def test_region_attention_zero_weight_is_a_select_inside_a_tile(dev):
    """Set 1's V holds a NaN and an Inf; the queries whose weight for set 1 is exactly 0 are finite and within the bound, the others are
    non-finite exactly where the reference is."""
    name = "nan_v_zero_for_part_of_a_tile"
    B, R, N, L, heads, d = CASES[name][:6]
    C = heads * d
    _, _, _, w, out, ref, _ = _check(dev, name)              # _check compares every element whose reference is finite
    got = out[:B * N, :C]
    zero = w[1, :N] == 0
    assert int(zero.sum()) == 31
    assert bool(torch.isfinite(ref[zero]).all()) and bool(torch.isfinite(got[zero]).all())
    assert not bool(torch.isfinite(ref[~zero]).all())
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref))


def test_region_attention_all_zero_rows_are_exact_zeros(dev):
    name = "all_zero_rows"
    B, R, N, L, heads, d = CASES[name][:6]
    _, _, _, w, out, _, _ = _check(dev, name)
    dead = (w[:, :N].reshape(B, R, N) == 0).all(1).reshape(B * N)
    assert int(dead.sum()) == 5
    got = out[:B * N, :heads * d]
    assert bool((got[dead] == 0).all()) and not bool((got[~dead] == 0).all(1).any())


def test_region_attention_one_set_matches_ops_attention(dev):
    """R = 1 with w = 1 is the plain core: within the same bound of ``ops.attention`` on the same operands (which is itself only near the fp64
    reference: the two kernels round differently, so the bound is applied to their difference, around the reference's magnitudes)."""
    from adaface_dev_amd import ops
    name = "one_set_weight_one"
    B, R, N, L, heads, d = CASES[name][:6]
    C = heads * d
    q, k, vt, w, out, ref, mag = _check(dev, name)
    plain = ops.attention(q.to(dev), k.to(dev), vt.to(dev), B=B, Nq=N, L=L, heads=heads, d=d, ldq=q.shape[1], ldk=C).cpu().double()
    ratio = float(((out[:B * N, :C].double() - plain).abs() / _bound(ref, mag)).max())
    print(f"af_region_attention {name}: worst |region - ops.attention| / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_region_attention_ops_wrapper_matches_entry_point(dev):
    from adaface_dev_amd import ops
    name = "soft_d160_L80_sliced_kv_ldw"
    B, R, N, L, heads, d = CASES[name][:6]
    q, o, k, vt, w = _inputs(name)
    want = _run(dev, q, o, k, vt, w, B, R, N, L, heads, d, d ** -0.5)
    kd, vd = _view_on(dev, k), _view_on(dev, vt)
    got = ops.region_attention(q.to(dev), kd, vd, w.to(dev), B=B, R=R, N=N, L=L, heads=heads, d=d, ldk=kd.stride(0))
    assert got.shape == (B * N, heads * d)
    assert torch.equal(got.cpu(), want[:B * N, :heads * d])
    assert ops.REGION_MAX == 8


BADARGS = ["R0", "R9", "L0", "L81", "d12", "d4", "d168", "N0", "B0", "B65536", "heads65536", "ldq_small", "ldq_odd", "ldo_odd", "ldk_small", "ldv_small",
           "ldv_odd", "ldw_small", "vbs_odd", "vbs_small", "null_q", "null_k", "null_vt", "null_w", "null_o", "misaligned_k", "misaligned_o",
           "q_2p31", "k_2p31", "vt_2p31", "w_2p31"]


@pytest.mark.parametrize("what", BADARGS)
def test_region_attention_refusals_leave_o_untouched(dev, what):
    from adaface_dev_amd import _lib, ops
    B, R, N, L, heads, d = 1, 2, 8, 5, 2, 16
    C = heads * d
    q = torch.zeros((B * N, C), dtype=torch.float16, device=dev)
    k = torch.zeros((B * R * L, C + 8), dtype=torch.float16, device=dev)
    vt = torch.zeros((B * R, C, 8), dtype=torch.float16, device=dev)
    w = torch.ones((B * R, N), dtype=torch.float32, device=dev)
    o = torch.full((B * N, C), SENTINEL, dtype=torch.float16, device=dev)
    a = dict(q=q.data_ptr(), ldq=C, k=k.data_ptr(), ldk=C + 8, vt=vt.data_ptr(), ldv=8, vbs=C * 8, w=w.data_ptr(), ldw=N, o=o.data_ptr(), ldo=C,
             B=B, R=R, N=N, L=L, heads=heads, d=d)
    a.update({"R0": dict(R=0), "R9": dict(R=9), "L0": dict(L=0), "L81": dict(L=81, ldv=88, vbs=C * 88), "d12": dict(d=12), "d4": dict(d=4),
              "d168": dict(d=168, ldq=336, ldo=336, ldk=336, vbs=336 * 8), "N0": dict(N=0), "B0": dict(B=0), "B65536": dict(B=65536),
              "heads65536": dict(heads=65536, d=8, ldq=1 << 19, ldo=1 << 19, ldk=1 << 19, vbs=1 << 22), "ldq_small": dict(ldq=C - 8),
              "ldq_odd": dict(ldq=C + 4), "ldo_odd": dict(ldo=C + 4), "ldk_small": dict(ldk=C - 8), "ldv_small": dict(L=9), "ldv_odd": dict(ldv=12, vbs=C * 12),
              "ldw_small": dict(ldw=N - 1), "vbs_odd": dict(vbs=C * 8 + 4), "vbs_small": dict(vbs=C * 8 - 8), "null_q": dict(q=None),
              "null_k": dict(k=None), "null_vt": dict(vt=None), "null_w": dict(w=None), "null_o": dict(o=None),
              "misaligned_k": dict(k=k.data_ptr() + 8), "misaligned_o": dict(o=o.data_ptr() + 8),
              "q_2p31": dict(B=2048, N=1 << 15, ldq=32, ldw=1 << 15), "k_2p31": dict(B=32768, R=8, L=80, ldv=80, vbs=C * 80, ldk=1024),
              "vt_2p31": dict(B=3, vbs=1 << 30), "w_2p31": dict(B=65535, R=8, ldw=4104)}[what])
    rc = _lib.lib().af_region_attention(a["q"], a["ldq"], a["k"], a["ldk"], a["vt"], a["ldv"], a["vbs"], a["w"], a["ldw"], a["o"], a["ldo"], a["B"],
                                        a["R"], a["N"], a["L"], a["heads"], a["d"], ctypes.c_float(0.25), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.AF_E_BADARG
    assert bool((o == SENTINEL).all())
