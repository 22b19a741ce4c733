#!/usr/bin/env python
"""Timings behind profiles/vae_anysize_attention.txt (MI355X): the VAE attention layer's two forms and the whole VAE at sizes the fused
kernel opens.  Medians of --reps runs after --warmup, with min / max; both arms of an A/B in one process, alternated.

    python tools/bench_vae_anysize.py kernels     # N = 4096 three launches vs af_vae_attention (events), af_vae_attention at 3136 / 6144 / 16384
    python tools/bench_vae_anysize.py vae         # decode 4 x 512^2 (switch off / on), decode 4 x 768x512, decode 1 x 1024^2, encode 1 x 768x512
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_vae_anysize.py trace    # per-kernel times of both forms at N = 4096
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

MFMA_ROOF = 2.5e15      # dense fp16 FLOP/s


def _qkv(N, C, dev):
    g = torch.Generator().manual_seed(N)
    mk = lambda s: (torch.randn((N, C), generator=g) * s).half().to(dev)              # noqa: E731
    return mk(C ** -0.5), mk(1.0), mk(1.0)


def _three_launches(ops, q, k, vt, N, C):
    p = ops.softmax_rows(ops.gemm(q, ops.PackedWeight(k, None, N, C, C, 1, C)))
    return ops.gemm(p, ops.PackedWeight(vt[0], None, C, N, N, 1, N))


def _time(fns, reps, warmup):
    """fns: {name: callable}; alternated rep by rep; returns {name: (median, min, max)} in ms."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in ts.items()}


def _show(name, r, extra=""):
    print(f"{name:58s} median {r[0]:9.3f} ms   min {r[1]:9.3f}   max {r[2]:9.3f}{extra}", flush=True)


def kernels(args, dev):
    from adaface_dev_amd import _lib, ops
    N, C = 4096, 512
    q, k, v = _qkv(N, C, dev)
    vt = ops.transpose_tokens(v, 1, N, C, C)
    o = torch.empty((N, C), dtype=torch.float16, device=dev)

    def fused_only():         # the kernel alone on a ready V^T, as the three launches below use a ready V^T
        _lib.check(_lib.lib().af_vae_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), 1, N, C, C, C, vt.stride(1), C,
                                               ops._stream()), "af_vae_attention")
    r = _time({"gemm": lambda: _three_launches(ops, q, k, vt, N, C), "flash": fused_only}, args.reps, args.warmup)
    _show("N=4096 C=512 q.k^T GEMM + af_softmax_rows + P.v GEMM", r["gemm"])
    _show("N=4096 C=512 af_vae_attention", r["flash"], f"   {4 * N * N * C / (r['flash'][0] * 1e-3) / MFMA_ROOF:6.1%} of the MFMA roof")
    for N in (3136, 6144, 16384):
        q, k, v = _qkv(N, C, dev)
        vt = ops.transpose_tokens(v, 1, N, C, C)
        o = torch.empty((N, C), dtype=torch.float16, device=dev)
        f = lambda: _lib.check(_lib.lib().af_vae_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), 1, N, C, C, C,   # noqa: E731
                                                           vt.stride(1), C, ops._stream()), "af_vae_attention")
        r = _time({"flash": f}, args.reps, args.warmup)["flash"]
        _show(f"N={N} C=512 af_vae_attention", r, f"   {4 * N * N * C / (r[0] * 1e-3) / MFMA_ROOF:6.1%} of the MFMA roof")


def trace(args, dev):
    from adaface_dev_amd import ops
    N, C = 4096, 512
    q, k, v = _qkv(N, C, dev)
    vt = ops.transpose_tokens(v, 1, N, C, C)
    for _ in range(args.warmup + args.reps):
        _three_launches(ops, q, k, vt, N, C)
        ops.vae_attention(q, k, v, B=1, N=N, C=C)
    torch.cuda.synchronize()


def vae(args, dev):
    from adaface_dev_amd import rng
    from adaface_dev_amd.ldm.modules.diffusionmodules.model import AutoencoderKL
    ae = AutoencoderKL()
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(rng.synth_tensor(n, p.shape, seed=90))
    ae = ae.to(dev).eval()

    def dec(z, flash):
        def f():
            if flash:
                os.environ["AF_VAE_FLASH"] = "1"
            else:
                os.environ.pop("AF_VAE_FLASH", None)
            with torch.no_grad():
                return ae.decode(z)
        return f
    z = rng.synth_input("vae.bench", (4, 4, 64, 64), seed=1).to(dev)
    r = _time({"off": dec(z, False), "on": dec(z, True)}, args.reps, args.warmup)
    _show("decode 4 x 512x512, AF_VAE_FLASH off (three launches)", r["off"])
    _show("decode 4 x 512x512, AF_VAE_FLASH=1 (af_vae_attention)", r["on"])
    os.environ.pop("AF_VAE_FLASH", None)
    for shape, what in (((4, 4, 96, 64), "decode 4 x 512x768 (96 x 64 latents)"), ((1, 4, 128, 128), "decode 1 x 1024x1024")):
        z = rng.synth_input("vae.bench", shape, seed=1).to(dev)
        r = _time({"d": dec(z, False)}, args.reps, args.warmup)["d"]
        assert bool(torch.isfinite(dec(z, False)()).all())
        _show(what, r)
    x = rng.synth_input("vae.bench.img", (1, 3, 768, 512), seed=2).to(dev)

    def enc():
        with torch.no_grad():
            return ae.encode(x)
    _show("encode 1 x 512x768", _time({"e": enc}, args.reps, args.warmup)["e"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "trace", "vae"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    {"kernels": kernels, "trace": trace, "vae": vae}[a.what](a, torch.device("cuda:0"))
