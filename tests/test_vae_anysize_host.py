"""The VAE at any image size, CPU only: the ``af_vae_attention`` C ABI entry (declared, exported, listed; argument validation returns
AF_E_* before any launch), the attention layer's dispatch rule as a pure function, and the wrapper's size refusals before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT
from adaface_dev_amd import TINY_UNET_CONFIG, _lib
from adaface_dev_amd.adaface.adaface_wrapper import MAX_IMAGE_SIDE, AdaFaceWrapper
from adaface_dev_amd.adaface.arc2face_models import clip_text_config
from adaface_dev_amd.ldm.modules.diffusionmodules.model import vae_attention_path


def test_af_vae_attention_is_declared_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "adaface_hip.h")).read()
    assert re.search(r"\bint\s+af_vae_attention\s*\(", hdr)
    assert "af_vae_attention" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "af_vae_attention")


def _call(q=True, k=True, vt=True, o=True, B=1, N=64, C=512, ldq=None, ldk=None, ldv=None, ldo=None):
    """af_vae_attention on a host buffer: every case here must be refused before any launch, so nothing is ever dereferenced."""
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    ld = lambda v, d: d if v is None else v                                                  # noqa: E731
    return _lib.lib().af_vae_attention(p if q else None, p if k else None, p if vt else None, p if o else None, B, N, C,
                                       ld(ldq, C), ld(ldk, C), ld(ldv, N), ld(ldo, C), None)


def test_af_vae_attention_argument_validation_without_a_gpu():
    for which in ("q", "k", "vt", "o"):
        assert _call(**{which: False}) == _lib.AF_E_BADARG
    assert b"null pointer" in _lib.lib().af_last_error()
    assert _call(N=12) == _lib.AF_E_BADARG                       # N % 8 != 0
    assert _call(N=0) == _lib.AF_E_BADARG
    assert _call(C=256) == _lib.AF_E_UNSUPPORTED                 # C outside {128, 512}
    assert _call(C=160) == _lib.AF_E_UNSUPPORTED
    assert _call(ldq=504) == _lib.AF_E_BADARG                    # a row stride below C
    assert _call(ldk=516) == _lib.AF_E_BADARG                    # ... or not a multiple of 8
    assert _call(ldo=508) == _lib.AF_E_BADARG
    assert _call(ldv=56) == _lib.AF_E_BADARG                     # V^T rows shorter than N keys
    assert _call(ldv=68) == _lib.AF_E_BADARG
    assert _call(B=256, N=16384) == _lib.AF_E_UNSUPPORTED        # 2^31 elements: past the 32-bit guard, refused and not wrapped
    assert b"2^31" in _lib.lib().af_last_error()
    assert _call(B=2, N=16384, ldq=1 << 16) == _lib.AF_E_UNSUPPORTED
    assert _call(C=128, B=1, N=8, ldv=1 << 24) == _lib.AF_E_UNSUPPORTED


def test_dispatch_keeps_the_gemm_form_wherever_it_was_accepted():
    """The no-behaviour-change claim: with the switch off, every (N, C) the three-launch form accepts (tokens % 128 == 0 up to 4096,
    C % 128 == 0) stays "gemm", masked or not, forward-only or with a backward."""
    for C in (128, 256, 384, 512, 640):
        for N in range(128, 4096 + 1, 128):
            for masked in (False, True):
                for train in (False, True):
                    assert vae_attention_path(N, C, masked=masked, train=train, flash_env=False) == "gemm", (N, C, masked, train)
    # masked and decode-with-grad calls keep it under the switch too
    for N in (256, 4096):
        assert vae_attention_path(N, 512, masked=True, flash_env=True) == "gemm"
        assert vae_attention_path(N, 512, train=True, flash_env=True) == "gemm"


@pytest.mark.parametrize("N,C,masked,train,flash_env,want", [
    (4096, 512, False, False, True, "flash"),        # the A/B switch
    (256, 128, False, False, True, "flash"),
    (4096, 256, False, False, True, "gemm"),         # a C the kernel is not built for stays where it was
    (3136, 512, False, False, False, "flash"),       # 448 x 448: not a multiple of 128
    (6144, 512, False, False, False, "flash"),       # 768 x 512: beyond af_softmax_rows
    (16384, 512, False, False, False, "flash"),      # 1024 x 1024
    (8, 512, False, False, False, "flash"),
    (960, 128, False, False, False, "flash"),
    (200, 128, False, False, True, "flash"),
    (16392, 512, False, False, False, None),         # beyond the kernel's range
    (6144, 256, False, False, False, None),          # another C
    (3136, 512, True, False, False, None),           # the pair mask at a size the GEMM form refuses
    (6144, 512, False, True, False, None),           # a backward there
    (6144, 512, True, False, True, None),
    (100, 512, False, False, False, None),           # N % 8 != 0
    (4100, 512, False, False, True, None),
])
def test_dispatch_table(N, C, masked, train, flash_env, want):
    if want is None:
        with pytest.raises(NotImplementedError, match="af_vae_attention"):
            vae_attention_path(N, C, masked=masked, train=train, flash_env=flash_env)
    else:
        assert vae_attention_path(N, C, masked=masked, train=train, flash_env=flash_env) == want


def _wrapper(pipeline_name):
    from adaface_dev_amd.ldm.modules.diffusionmodules.model import AutoencoderKL
    cc = clip_text_config(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128)
    ae = AutoencoderKL(dict(ch=32, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=[], dropout=0.0, in_channels=3,
                            resolution=128, z_channels=4, double_z=True))
    return AdaFaceWrapper(pipeline_name=pipeline_name, clip_config=cc, unet_config=dict(TINY_UNET_CONFIG), vae=ae, device="cpu")


def _img(w, h):
    return Image.fromarray(np.zeros((h, w, 3), dtype=np.uint8))


def test_wrapper_refuses_sides_above_1024_before_any_gpu_work():
    """Everything lives on the CPU here: reaching a kernel would raise a RuntimeError, not the ValueError that names the limit."""
    assert MAX_IMAGE_SIDE == 1024
    pe = torch.zeros(1, 77, 64)
    w = _wrapper("img2img")
    with pytest.raises(ValueError, match="1024"):
        w(_img(1088, 512), None, prompt_embeds=(pe, pe), out_image_count=1)
    with pytest.raises(ValueError, match="1024"):
        w(_img(512, 1100), None, prompt_embeds=(pe, pe), out_image_count=1)           # prepared as 512 x 1088
    w = _wrapper("inpaint")
    with pytest.raises(ValueError, match="1024"):
        w(_img(1088, 64), None, prompt_embeds=(pe, pe), out_image_count=1, mask_image=Image.new("L", (1088, 64), 255))
    w = _wrapper("text2img")
    with pytest.raises(ValueError, match="128"):
        w(torch.zeros(2, 4, 136, 64), None, prompt_embeds=(pe, pe), out_image_count=2)
    with pytest.raises(ValueError, match="128"):
        w(torch.zeros(1, 4, 64, 136), None, prompt_embeds=(pe, pe), out_image_count=1)
