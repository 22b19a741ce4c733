"""Host-only checks of the tuned-shape sweep (test_hip_tuned_shapes.py) and of the address-width guards of ops.conv_halo_eligible."""
import json

import pytest

import tuned_shapes as TS


def _table():
    with open(TS.TABLE) as f:
        return list(json.load(f))


def test_constants_match_the_library_binding():
    from adaface_dev_amd import _lib
    assert (TS.AF_ACT_NONE, TS.AF_ACT_SILU, TS.AF_ACT_GEGLU, TS.AF_ACT_QUICKGELU) == (_lib.AF_ACT_NONE, _lib.AF_ACT_SILU, _lib.AF_ACT_GEGLU, _lib.AF_ACT_QUICKGELU)
    assert (TS.AF_OUT_NORMAL, TS.AF_OUT_SPLIT_T, TS.AF_OUT_F32) == (_lib.AF_OUT_NORMAL, _lib.AF_OUT_SPLIT_T, _lib.AF_OUT_F32)


def test_every_table_key_has_a_geometry_the_sweep_builds():
    """A future table entry whose form the sweep cannot build fails here, before any GPU run."""
    from adaface_dev_amd import ops
    keys = _table()
    assert len(keys) == len(ops.tune_table()) > 0
    bad = []
    for key in keys:
        try:
            k, geos = TS.validate(key)
        except ValueError as e:
            bad.append(str(e))
            continue
        if k.taps == 1:
            continue
        assert geos and geos[0].label.startswith("a:"), key
        for g in geos:
            assert g.B >= 1 and g.B * g.Ho * g.Wo == k.M, (key, g)
            assert 9 * g.cin + g.ktail == k.K and g.ktail % 64 == 0, (key, g)
            assert (k.K % 9 == 0) == (g.ktail == 0), (key, g)
            if g.upsample:
                assert (g.Ho, g.Wo) == (2 * g.H, 2 * g.W), (key, g)
            else:
                assert (g.Ho, g.Wo) == ((g.H - 1) // g.stride + 1, (g.W - 1) // g.stride + 1), (key, g)
            if g.label.startswith("b:"):
                assert not ops.conv_halo_eligible(TS.halo_scope_desc(k, g)), (key, g)
        a = geos[0]
        assert a.Ho == a.Wo and (a.Ho in TS.UNET_LEVELS + TS.VAE_LEVELS + TS.FACE_LEVELS or a.H in TS.UNET_LEVELS + TS.VAE_LEVELS), (key, a)
    assert not bad, bad[:5]


def test_no_tabled_shape_reaches_the_address_width_guards():
    """The 2^24-pixel and 2^32-byte guards only take shapes far larger than any the table holds: at the geometry that produced each 3x3 key,
    none of them applies, so no tabled shape changes kernel, tile or split."""
    for key in _table():
        k, geos = TS.validate(key)
        npad, kpad = (k.N + 127) // 128 * 128, (k.K + 63) // 64 * 64
        assert npad * kpad * 2 < 1 << 32, key
        for g in geos:
            assert g.B * g.H * g.W * g.cin * 2 < 1 << 32 and k.M * max(g.ktail, 1) * 2 < 1 << 32, (key, g)
            if g.ktail:
                assert g.B * g.H * g.W < 1 << 24, (key, g)


@pytest.mark.parametrize("B,ok", [(4095, True), (4096, False), (4112, False)])
def test_halo_scope_keeps_the_k_tail_below_2_24_pixels(B, ok):
    """conv3h_variant multiplies the tail form's pixel indices with __umul24: ops.conv_halo_eligible must agree that it stops at 2^24 pixels."""
    from adaface_dev_amd import ops
    k = TS.Key(9, B * 4096, 160, 640, 0, 0, 1, 0, False)
    g = TS.ConvGeo(B, 64, 64, 64, 64, 64, 64, 1, 0)
    assert ops.conv_halo_eligible(TS.halo_scope_desc(k, g)) == ok
    plain = TS.ConvGeo(B, 64, 64, 64, 64, 64, 0, 1, 0)                # without the tail the 2^32-byte gather limit applies: 2^25 pixels at 64 channels
    assert ops.conv_halo_eligible(TS.halo_scope_desc(TS.Key(9, B * 4096, 160, 576, 0, 0, 1, 0, False), plain))


def test_halo_scope_stops_at_4GiB_operands():
    from adaface_dev_amd import ops
    vae16 = TS.ConvGeo(16, 512, 512, 512, 512, 256, 0, 1, 0)          # the VAE decoder's 512 level at batch 16: 2.1 GB input, in scope (patches)
    vae33 = TS.ConvGeo(33, 512, 512, 512, 512, 256, 0, 1, 0)          # batch 33: 4.4 GB input
    k16, k33 = TS.Key(9, 16 * 512 * 512, 128, 2304, 0, 0, 1, 0, False), TS.Key(9, 33 * 512 * 512, 128, 2304, 0, 0, 1, 0, False)
    assert ops.conv_halo_eligible(TS.halo_scope_desc(k16, vae16))
    assert not ops.conv_halo_eligible(TS.halo_scope_desc(k33, vae33))
    g = TS.ConvGeo(1, 16, 16, 16, 16, 2048, 0, 1, 0)
    small, huge = TS.Key(9, 256, 1280, 9 * 2048, 0, 0, 1, 0, False), TS.Key(9, 256, 128 * 1024, 9 * 2048, 0, 0, 1, 0, False)
    assert ops.conv_halo_eligible(TS.halo_scope_desc(small, g))
    assert not ops.conv_halo_eligible(TS.halo_scope_desc(huge, g))  # 131072 x 18432 fp16 weight: 4.8 GB
