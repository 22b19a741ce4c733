"""The benchmarked denoise step on a real MI355X (`pytest -m gpu`): the SD-1.5-size U-Net at U-Net batch 8 (4 images, CFG cond + uncond),
built the way bench.py's denoise leg builds it, against the fp32 CPU oracle, and its captured-graph replay against eager launches.

At this shape the C = 320 level runs the one-launch kernels that the other network-level tests (batch 1 or reduced width) stay below:
af_xattn_chain (U-Net batch x tokens >= XATTN_FUSE_MIN_TOKENS) and af_ff_chain (>= 24576 rows).  The file pins
* the epsilon of all 8 samples and the guidance signal e_c - e_u of every image against the oracle, which launches ran, and a negative
  control showing that the guidance bound catches a small error in the chained cross-attention launch;
* hipGraph replay of the step (with and without the weight-prefetch stream) bitwise against eager calls on the same buffers;
* two short trajectories of DDIMSampler.p_sample_ddim (the bench's first 4 steps, the img2img tail) against the oracle per step, and the
  bench's eager step bitwise against p_sample_ddim.

The construction below restates bench.py's run_denoise: LatentDiffusion(SD15_UNET_CONFIG), synthetic weights drawn on the device (seed 0),
inputs bench.x / bench.ctx / bench.uctx at seed 42, the 50-step DDIM schedule at guidance 4.  The oracle takes the device model's weights.
"""
import time

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_hip_unet import NET_TOL

pytestmark = pytest.mark.gpu

B = 4                      # images; the U-Net batch is 2 * B
T_EPS = 501                # the DDIM timestep of the one-call check (index 25 of the 50-step schedule)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class _Bench:
    pass


@pytest.fixture(scope="module")
def bench(dev):
    """bench.py run_denoise's model, inputs and schedule, plus the oracle's copy of the weights."""
    from adaface_dev_amd import SD15_UNET_CONFIG, rng
    from adaface_dev_amd.ldm.models.diffusion.ddim import DDIMSampler
    from adaface_dev_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    with rng.skip_default_init():
        ldm = LatentDiffusion(SD15_UNET_CONFIG)
    ldm = ldm.to(dev).eval()
    unet = ldm.model.diffusion_model
    rng.load_synth_weights(unet, seed=0, on_device=True)
    unet.prepare()
    for p in unet.parameters():
        p.requires_grad_(False)
    b = _Bench()
    b.cfg, b.ldm, b.unet = SD15_UNET_CONFIG, ldm, unet
    b.x = rng.synth_input("bench.x", (B, 4, 64, 64), seed=42)
    b.c = rng.synth_input("bench.ctx", (B, 77, 768), seed=42)
    b.u = rng.synth_input("bench.uctx", (B, 77, 768), seed=42)
    b.sampler = DDIMSampler(ldm)
    b.sampler.make_schedule(50, verbose=False)
    b.ts_desc = b.sampler.ddim_timesteps[::-1].copy()
    b.scales = b.sampler.guide_scales(50, 4.0)
    b.sd = {k: v.detach().float().cpu() for k, v in unet.state_dict().items()}
    yield b
    del b.sd
    torch.cuda.synchronize()


def _oracle_pair(b, x1, t, j):
    """The oracle's [e_cond ; e_uncond] of image j at latent x1 [1, 4, 64, 64] (cpu fp32) and timestep t."""
    from oracle import unet_oracle as O
    with torch.no_grad():
        return O.unet_forward(b.sd, b.cfg, torch.cat([x1, x1]), torch.tensor([t, t]), torch.cat([b.c[j:j + 1], b.u[j:j + 1]]), {})


@pytest.fixture(scope="module")
def oracle_eps(bench):
    """The oracle on the bench's step input at T_EPS: [8, 4, 64, 64] in the U-Net's (cond, uncond) row order."""
    t0 = time.perf_counter()
    pairs = [_oracle_pair(bench, bench.x[j:j + 1], T_EPS, j) for j in range(B)]
    print(f"\noracle: {2 * B} sample-forwards in {time.perf_counter() - t0:.1f} s")
    return torch.cat([p[:1] for p in pairs] + [p[1:] for p in pairs])


def _step_inputs(b, dev, t):
    x_in = torch.cat([b.x, b.x]).to(dev)
    t_in = torch.full((2 * B,), t, dtype=torch.int64, device=dev)
    ctx2 = torch.cat([b.c, b.u]).to(torch.float16).to(dev).contiguous()
    return x_in, t_in, ctx2


def _eps_errors(e, ref):
    """-> (worst per-sample rel-L2 of epsilon, worst per-image rel-L2 of the guidance signal e_c - e_u)."""
    e, ref = e.double(), ref.double()
    per = [rel_l2(e[i].numpy(), ref[i].numpy()) for i in range(2 * B)]
    guid = [rel_l2((e[j] - e[B + j]).numpy(), (ref[j] - ref[B + j]).numpy()) for j in range(B)]
    return per, guid


# measured on MI355X: 5.30e-3 at most (test_bench_shape_eps_vs_oracle); 2.1x that, below 3 x NET_TOL
GUIDANCE_TOL = 1.1e-2


_ROUTED = ("xattn_chain", "xattn_fused", "ff_chain", "ff_fused", "gn_proj_fused")


def _count_routes(monkeypatch):
    """Wrap the one-launch entry points of ops with counters (gn_proj_fused counts the calls that launched, i.e. did not return None)."""
    from adaface_dev_amd import ops
    counts = dict.fromkeys(_ROUTED, 0)

    def wrap(name):
        fn = getattr(ops, name)

        def counted(*a, **k):
            out = fn(*a, **k)
            if out is not None:
                counts[name] += 1
            return out
        monkeypatch.setattr(ops, name, counted)

    for name in _ROUTED:
        wrap(name)
    return counts


def test_bench_shape_eps_vs_oracle(dev, bench, oracle_eps, monkeypatch):
    """One U-Net call on the bench's step input (U-Net batch 8, t = 501) against the oracle, sample by sample, and the guidance
    signal e_c - e_u of each image (CFG multiplies it by 4; the cross-attention layers carry it).  Measured on MI355X: epsilon
    rel-L2 1.51 - 1.64e-3 per sample (bound NET_TOL), e_c - e_u 4.32 - 5.30e-3 per image (bound GUIDANCE_TOL = 1.1e-2, 2.1x).

    Routing at this shape: the 5 SpatialTransformers of the 64 x 64 level run af_xattn_chain and af_ff_chain (5 each), no
    af_xattn_fused (C = 320 takes the chained form; C = 640 is off while AF_FUSE_XATTN640 is unset) and no af_ff_fused (the chained
    form replaces it).  The 5 SpatialTransformers there also take GroupNorm + proj_in as one launch (af_gn_proj_fused, fed by the
    statistics the ResBlock's convolution left).  At U-Net batch 1 none of these runs: a threshold that moves fails here."""
    from adaface_dev_amd.ldm.modules import attention as A
    assert not A.FUSE_XATTN640 and A.CHAIN_XATTN and A.CHAIN_PROJ_OUT and A.FUSE_FF and A.FUSE_XATTN
    counts = _count_routes(monkeypatch)
    x_in, t_in, ctx2 = _step_inputs(bench, dev, T_EPS)
    with torch.no_grad():
        eps = bench.unet(x_in, t_in, ctx2, extra_info=None).cpu()
    routed8 = dict(counts)
    for k in counts:
        counts[k] = 0
    with torch.no_grad():
        bench.unet(x_in[:1], t_in[:1], ctx2[:1], extra_info=None)
    torch.cuda.synchronize()
    routed1 = dict(counts)
    per, guid = _eps_errors(eps, oracle_eps)
    print(f"bench shape eps vs oracle, per sample: {' '.join(f'{v:.3e}' for v in per)}")
    print(f"bench shape e_c - e_u vs oracle, per image: {' '.join(f'{v:.3e}' for v in guid)}  (bound {GUIDANCE_TOL:.1e})")
    print(f"routing at U-Net batch 8: {routed8}; at U-Net batch 1: {routed1}")
    assert torch.isfinite(eps).all()
    assert max(per) < NET_TOL
    assert max(guid) < GUIDANCE_TOL
    assert routed8 == {"xattn_chain": 5, "xattn_fused": 0, "ff_chain": 5, "ff_fused": 0, "gn_proj_fused": 5}
    assert routed1 == dict.fromkeys(_ROUTED, 0)


# the smallest relative change of the chained cross-attention's softmax scale (of 1.0025, 1.005, 1.01, 1.02, 1.05) that the guidance
# check catches
NEG_CONTROL_SCALE = 1.01


def test_negative_control_guidance_bound_catches_a_scaled_xattn_chain(dev, bench, oracle_eps, monkeypatch):
    """af_xattn_chain with its softmax scale multiplied by NEG_CONTROL_SCALE (5 of the 16 cross-attention layers, the 64 x 64 level):
    the e_c - e_u check of test_bench_shape_eps_vs_oracle must fail.  Measured on MI355X: e_c - e_u 0.96 - 1.21e-2 per image (bound
    1.1e-2), while every sample's epsilon stays within NET_TOL (3.3e-3 at most): only the guidance signal sees the error.  A factor of
    1.005 gives 7.6e-3 (not caught), 1.02 gives 1.8 - 2.3e-2 (caught on every image)."""
    from adaface_dev_amd import ops
    orig = ops.xattn_chain
    calls = []

    def scaled(*a, scale, **k):
        calls.append(scale)
        return orig(*a, scale=scale * NEG_CONTROL_SCALE, **k)

    monkeypatch.setattr(ops, "xattn_chain", scaled)
    x_in, t_in, ctx2 = _step_inputs(bench, dev, T_EPS)
    with torch.no_grad():
        eps = bench.unet(x_in, t_in, ctx2, extra_info=None).cpu()
    per, guid = _eps_errors(eps, oracle_eps)
    print(f"negative control (xattn_chain scale x {NEG_CONTROL_SCALE}): eps per sample max {max(per):.3e}, "
          f"e_c - e_u per image {' '.join(f'{v:.3e}' for v in guid)}  (bound {GUIDANCE_TOL:.1e})")
    assert len(calls) == 5
    assert max(guid) >= GUIDANCE_TOL


# ---------------------------------------------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("prefetch", [0, 2], ids=["plain", "prefetch2"])
def test_graph_replay_is_bitwise_eager(dev, bench, prefetch):
    """bench.py's capture of `unet(x_in, t_in, ctx2)` (eager warm-up, a warm-up on a side stream, thread_local capture; with
    prefetch > 0 the ops.WeightPrefetcher recorded in the side-stream warm-up and played beside the capture) replayed on rewritten
    static buffers: three (x, t) sets, one of them with a new context written into ctx2, each bitwise equal to an eager call on the
    same buffers; then the bench's step loop (ops.cfg_ddim_step) for 3 steps, replay and eager bitwise equal in x and pred_x0 after
    every step.  Measured on MI355X: bitwise equal in both forms (the prefetch stream issues 156 prefetch launches for 184
    weight-consuming launches)."""
    from adaface_dev_amd import ops, rng
    unet, s = bench.unet, bench.sampler
    x_in = torch.empty((2 * B, 4, 64, 64), dtype=torch.float32, device=dev)
    t_in = torch.empty((2 * B,), dtype=torch.int64, device=dev)
    ctx_bench = torch.cat([bench.c, bench.u]).to(torch.float16).to(dev).contiguous()
    ctx2 = ctx_bench.clone()
    xd = bench.x.to(dev)

    def load(x, t):
        x_in[:B].copy_(x)
        x_in[B:].copy_(x)
        t_in.fill_(int(t))

    def unet_eps():
        return unet(x_in, t_in, ctx2, extra_info=None)

    g, pf, eps_g = torch.cuda.CUDAGraph(), None, None
    try:
        with torch.no_grad():
            load(xd, bench.ts_desc[0])
            unet_eps()                                    # eager warm-up
            torch.cuda.synchronize()
            side_warm = torch.cuda.Stream()
            side_warm.wait_stream(torch.cuda.current_stream())
            if prefetch:
                pf = ops.WeightPrefetcher(depth=prefetch)
                ops.set_weight_prefetcher(pf.record())
            with torch.cuda.stream(side_warm):
                unet_eps()
            torch.cuda.current_stream().wait_stream(side_warm)
            side = torch.cuda.Stream() if pf is not None else None
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    if pf is not None:
                        pf.play(side)
                    eps_g = unet_eps()
                    if pf is not None:
                        pf.join()
            finally:
                ops.set_weight_prefetcher(None)
            if pf is not None:
                print(f"prefetch stream: {pf.issued} prefetch launches for {len(pf.plan)} weight-consuming launches")
                assert pf.issued > 0

            ctx_new = torch.cat([rng.synth_input("bsh.ctx.alt", (B, 77, 768), seed=43), bench.u]).to(torch.float16).to(dev)
            cases = [(xd, 981, None),
                     (rng.synth_input("bsh.x.a", (B, 4, 64, 64), seed=43).to(dev), 501, ctx_new),
                     (rng.synth_input("bsh.x.b", (B, 4, 64, 64), seed=44).to(dev) * 0.3, 1, ctx_bench)]
            seen = []
            for x, t, ctx in cases:
                if ctx is not None:
                    ctx2.copy_(ctx)
                load(x, t)
                g.replay()
                r = eps_g.clone()
                e = unet_eps()
                assert torch.isfinite(r).all()
                assert torch.equal(r, e), f"t = {t}: replay vs eager rel-L2 {rel_l2(r.cpu().numpy(), e.cpu().numpy()):.3e}"
                seen.append(r)
            assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])

            xg, xe = xd.clone(), xd.clone()
            for i in range(3):
                index = 50 - i - 1
                a_t, a_prev = float(s.ddim_alphas[index]), float(s.ddim_alphas_prev[index])
                load(xg, bench.ts_desc[i])
                g.replay()
                xg, x0g = ops.cfg_ddim_step(eps_g, xg, bench.scales[i], a_t, a_prev, True)
                load(xe, bench.ts_desc[i])
                xe, x0e = ops.cfg_ddim_step(unet_eps(), xe, bench.scales[i], a_t, a_prev, True)
                assert torch.equal(xg, xe) and torch.equal(x0g, x0e), f"step {i} (t = {bench.ts_desc[i]})"
            torch.cuda.synchronize()
            print(f"graph replay ({'prefetch depth %d' % prefetch if prefetch else 'no prefetch'}): 3 input sets + 3 bench steps bitwise equal to eager")
    finally:
        del eps_g, g
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- trajectories
# 2x the worst per-step value measured on MI355X (docstring of test_trajectory_vs_oracle)
TRAJ_TOL = {"bench4": {"pred_x0": 5.6e-3, "update": 5.6e-3, "teacher_eps": 8.4e-3},
            "img2img_tail": {"pred_x0": 1.6e-3, "update": 8e-3, "teacher_eps": 8.2e-3}}


def _oracle_schedule():
    from oracle import diffusion_oracle as D
    tabs = D.register_schedule(D.make_beta_schedule_linear())
    ts = D.make_ddim_timesteps(50)
    _, a, ap = D.make_ddim_sampling_parameters(tabs["alphas_cumprod"], ts)
    return tabs, ts, a, ap


@pytest.mark.parametrize("segment", ["bench4", "img2img_tail"])
def test_trajectory_vs_oracle(dev, bench, segment):
    """DDIMSampler.p_sample_ddim on all 4 images (U-Net batch 8, guidance 4) against the oracle following one image with
    cfg_combine / ddim_update on the CPU.  bench4: the bench's first 4 steps from bench.x (t = 981, 961, 941, 921; image 0).
    img2img_tail: sample_img2img(50, strength 0.06) -- 3 steps, t = 41, 21, 1 -- from q_sample(x0, t = 41) (image 2).
    Per step: pred_x0, the accumulated update x_k - x_T, and the teacher-forced guided epsilon (the GPU run on the oracle's own
    x_k, which separates one step's error from the drift).  Worst step measured on MI355X (the bounds TRAJ_TOL are 2x):
        bench4        pred_x0 2.78e-3, x_k - x_T 2.79e-3, teacher-forced eps 4.19e-3 (all at t = 981, falling over the 4 steps)
        img2img_tail  pred_x0 7.6e-4,  x_k - x_T 3.99e-3, teacher-forced eps 4.09e-3
    The guided epsilon e_u + 4 (e_c - e_u) carries about 2.5x the error of one sample's epsilon; at t <= 41 x_k - x_T is a small step,
    so its relative error follows that of epsilon rather than that of pred_x0.
    bench4 also checks that the bench's eager step (static buffers, fp16 context, ops.cfg_ddim_step) is bitwise p_sample_ddim."""
    from adaface_dev_amd import ops, rng
    from oracle import diffusion_oracle as D
    ldm, s = bench.ldm, bench.sampler
    tabs, ts, a_o, ap_o = _oracle_schedule()
    assert np.array_equal(ts, s.ddim_timesteps)
    c = (bench.c.to(dev), [""] * B, {})
    u = (bench.u.to(dev), [""] * B, {})
    if segment == "bench4":
        j, steps = 0, [(i, 50 - i - 1, bench.scales[i]) for i in range(4)]
        x_T = bench.x.to(dev)
    else:
        j = 2
        n, t_first = s.img2img_steps(50, 0.06)
        assert (n, t_first) == (3, 41)
        steps = [(i, n - 1 - i, sc) for i, sc in enumerate(s.guide_scales(n, 4.0))]
        x0 = rng.synth_input("bsh.i2i.x0", (B, 4, 64, 64), seed=45)
        noise = rng.synth_input("bsh.i2i.noise", (B, 4, 64, 64), seed=45)
        tt = torch.full((B,), t_first, dtype=torch.int64)
        x_T = ldm.q_sample(x0.to(dev), tt.to(dev), noise.to(dev))
        assert rel_l2(x_T.cpu().numpy(), D.q_sample(tabs, x0, tt, noise).numpy()) < 1e-6

    # the GPU trajectory, through the product sampler
    gpu = []
    if segment == "bench4":
        x = x_T
        for i, index, sc in steps:
            t = torch.full((B,), int(s.ddim_timesteps[index]), dtype=torch.int64, device=dev)
            xn, x0n = s.p_sample_ddim(x, c, t, index=index, guidance_scale=sc, unconditional_conditioning=u)
            if i == 0:
                # the bench's eager step on the same inputs (bench.py run_denoise: static buffers, fp16 context, the fused step)
                x_in, t_in, ctx2 = _step_inputs(bench, dev, int(t[0]))
                with torch.no_grad():
                    eb = bench.unet(x_in, t_in, ctx2, extra_info=None)
                xb, x0b = ops.cfg_ddim_step(eb, x.contiguous(), sc, float(s.ddim_alphas[index]), float(s.ddim_alphas_prev[index]), True)
                assert torch.equal(xb, xn) and torch.equal(x0b, x0n)
            gpu.append((x, xn, x0n))
            x = xn
    else:
        orig = s.p_sample_ddim

        def recording(xk, *a, **k):
            out = orig(xk, *a, **k)
            gpu.append((xk, out[0], out[1]))
            return out

        s.p_sample_ddim = recording
        try:
            lat, _ = s.sample_img2img(50, 0.06, B, x_T, c, guidance_scale=4.0, unconditional_conditioning=u)
        finally:
            del s.p_sample_ddim
        assert len(gpu) == len(steps) and torch.equal(lat, gpu[-1][1])

    # the oracle follows image j; teacher forcing: the GPU on the oracle's x_k (image j's row replaced)
    t0 = time.perf_counter()
    xT_j = x_T[j:j + 1].cpu()
    xo = xT_j.clone()
    tol = TRAJ_TOL[segment]
    worst = dict.fromkeys(tol, 0.0)
    for (i, index, sc), (xk_g, xn_g, x0n_g) in zip(steps, gpu):
        t = int(ts[index])
        e2 = _oracle_pair(bench, xo, t, j)
        e_o = D.cfg_combine(e2[:1], e2[1:], sc)
        xn_o, x0n_o = D.ddim_update(xo, e_o, float(a_o[index]), float(ap_o[index]))

        x_tf = xk_g.clone()
        x_tf[j:j + 1] = xo.to(dev)
        tt = torch.full((2 * B,), t, dtype=torch.int64, device=dev)
        with torch.no_grad():
            e2_g = ldm.apply_model(torch.cat([x_tf, x_tf]), tt, (torch.cat([c[0], u[0]]), [""] * (2 * B), {})).cpu()
        e_tf = D.cfg_combine(e2_g[j:j + 1].double(), e2_g[B + j:B + j + 1].double(), sc)

        err = {"pred_x0": rel_l2(x0n_g[j:j + 1].cpu().numpy(), x0n_o.numpy()),
               "update": rel_l2((xn_g[j:j + 1].cpu() - xT_j).numpy(), (xn_o - xT_j).numpy()),
               "teacher_eps": rel_l2(e_tf.numpy(), e_o.numpy())}
        print(f"{segment} step {i} (t = {t}, image {j}): pred_x0 {err['pred_x0']:.3e}  x_k - x_T {err['update']:.3e}  "
              f"teacher-forced eps {err['teacher_eps']:.3e}")
        for k, v in err.items():
            worst[k] = max(worst[k], v)
        xo = xn_o
    print(f"{segment}: oracle {2 * len(steps)} sample-forwards in {time.perf_counter() - t0:.1f} s; worst {worst}")
    for k, v in worst.items():
        assert v < tol[k], (k, v)
