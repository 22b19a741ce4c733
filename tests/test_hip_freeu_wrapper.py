"""``AdaFaceWrapper.enable_freeu`` / ``disable_freeu`` on a real MI355X (`pytest -m gpu`): the reduced-width wrapper of tests/test_hip_clip.py, two
steps, text2img (latents) and inpaint (images)."""
import numpy as np
import pytest
import torch

from test_hip_img2img import _pil, _unet_cfg
from test_vae_oracle import VAE_SMALL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _wrapper(dev, pipeline):
    from adaface_dev_amd import rng
    from adaface_dev_amd.adaface.adaface_wrapper import AdaFaceWrapper
    from adaface_dev_amd.adaface.arc2face_models import clip_text_config
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cc = clip_text_config(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512)
    ld = LatentDiffusion(_unet_cfg())
    ae = None
    if pipeline == "inpaint":
        ae = ld.instantiate_first_stage(dict(VAE_SMALL, double_z=True))
        with torch.no_grad():
            for n, p in ae.named_parameters():
                p.copy_(rng.synth_tensor(n, p.shape, seed=92))
    w = AdaFaceWrapper(pipeline_name=pipeline, clip_config=cc, ldm=ld, vae=ae, device=dev, num_inference_steps=2)
    rng.load_synth_weights(w.ldm.model.diffusion_model, seed=63)
    return w.to(dev)


def _generate(w, dev, pipeline):
    from adaface_dev_amd import rng
    from PIL import Image
    pe = rng.synth_input("fu.pe", (1, 77, 128), seed=85).to(dev)
    ne = rng.synth_input("fu.ne", (1, 77, 128), seed=86).to(dev)
    if pipeline == "text2img":
        out = w(rng.synth_input("fu.noise", (2, 4, 16, 16), seed=60), None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2)
        torch.cuda.synchronize()
        return out.float().cpu().numpy()
    mask = np.zeros((128, 128), dtype=np.uint8)
    mask[:, :64] = 255
    out = w(_pil(128, 128, seed=4), None, prompt_embeds=(pe, ne), guidance_scale=4.0, out_image_count=2, ref_img_strength=1.0,
            generator=torch.Generator().manual_seed(7), mask_image=Image.fromarray(mask))
    return np.stack([np.asarray(im) for im in out])


@pytest.mark.parametrize("pipeline", ["text2img", "inpaint"])
def test_enable_disable_freeu(dev, pipeline):
    w = _wrapper(dev, pipeline)
    plain = _generate(w, dev, pipeline)
    assert np.array_equal(_generate(w, dev, pipeline), plain)
    w.enable_freeu()
    on = _generate(w, dev, pipeline)
    assert on.shape == plain.shape and np.isfinite(on.astype(np.float64)).all()
    changed = float(np.mean(on != plain))
    print(f"{pipeline}: enable_freeu() changes {100 * changed:.1f} % of the output values")
    assert changed > 0.5
    w.disable_freeu()
    assert np.array_equal(_generate(w, dev, pipeline), plain)
    w.enable_freeu(1, 1, 1, 1)
    assert np.array_equal(_generate(w, dev, pipeline), plain)
    w.disable_freeu()
