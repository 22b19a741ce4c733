"""The hand-written hip_train / hip_bwd / hip_dgrad pairs of the U-Net and VAE modules and the capture-graph nodes built on them, on a real
MI355X, pair by pair, against fp64 on the CPU.  `pytest -m gpu`.  Conventions of tests/test_hip_autograd_nodes.py (rnd, cmp, master, launches).

Every reference is plain torch.nn.functional in fp64 on the CPU, written out below (r_*), with torch autograd for the gradients, on the numbers
the device sees: activations and incoming gradients are fp16 tensors, parameters fp32 masters holding fp16-representable values (`fill`), the
zero_modules (proj_out, the ResBlock's second convolution) get non-zero weights, GroupNorm inputs a mean offset (`gn_input`).  The pair is called
directly (`y, saved = m.hip_train(...)`, `m.hip_bwd(saved, G)`); the capture-graph nodes through Node.apply and a linear loss.  Every compared
tensor is checked by rel-L2 and max|got - ref| / max|ref|, on the whole tensor AND on every batch item (`both`; a two-source gradient per source),
for shape, dtype and all-finite (cmp), and a second call must give the same bits (`twice`).  Which arm ran is asked of the project's own predicate
and, where a launch name tells it, of the launches() spy.

Arms reached
  test_conv_pairs            Conv2d.hip_train / hip_bwd / hip_dgrad: 3x3 stride 1; stride 2 at 16x16 and at 15x17 (forward 8x9, the 2H - 1 arm of
                             conv3x3(upsample=2)); 1x1; cin_pad 4 -> 8; the head's dgrad (4 output channels, gradient padded to 8)
  test_linear_dgrad          Linear.hip_dgrad with / without residual
  test_groupnorm_pair        GroupNorm32.hip_train / hip_bwd: SiLU on / off, eps 1e-5 / 1e-6, one / two sources, add on / off, C = 320, 192 + 128, 2560, 1280 + 1280
  test_layernorm_bwd         LayerNorm.hip / hip_bwd with / without add, C = 320 / 1280
  test_resblock_pair         identity shortcut; fused 1x1 shortcut (_skip_fusable) from a SkipCat; un-fusable 1x1 shortcut (own launch), also from a
                             SkipCat; identity on a SkipCat (torch.cat); each with a raw [B, emb] embedding and an EmbPack slice (row stride != Cout)
  test_resblock_dora_node    _ResBlockFn with DoRA adapters on conv1 / conv2 / conv_shortcut: dh, dskip and the nine adapter gradients
  test_updown_pairs          openaimodel.Downsample (16x16, 15x17) / Upsample (nine-tap gather at 8x8 -> 16x16; four-phase pack at 16x16 -> 32x32, C = 320, the
                             smallest shape conv_up2_eligible accepts at tile 14 -- at 8x8 the predicate refuses tile 14 for every width, so the phase
                             form is not reachable there without the AF_UP2_PHASE_8X8 switch) through TimestepEmbedSequential; a sequential whose
                             first layer took a SkipCat returns the pair
  test_self_attention_pair   CrossAttention self arm, d = 40 / 80 / 160, N = 64: no mask; key bias with item 0 partly and item 1 fully masked; residual
  test_self_attention_ln     the folded q | k | v pack (ln=) at N = 1024, C = 320
  test_cross_attention_pair  cross arm, L = 77 / 1 / 97, dctx None and accumulated into an incoming dctx
  test_feedforward_pair      FeedForward / GEGLU: folded LN (C = 320, 130 rows; C = 1280, 64 rows), un-folded (C = 96, 77 rows)
  test_transformer_block     BasicTransformerBlock both arms (ln_fold yes / no) at d = 40 / 80 / 160, with / without key bias
  test_spatial_transformer   SpatialTransformer C = 320 at 8x8 / 32x32, C = 1280 at 8x8: no mask, [B, 1, 2H, 2W] mask, live_mask_rule with an empty item
  test_st_nodes              _STPreFn (loss on x1 / qin / both), _STPostFn (d(x_in) == G bit for bit), _FrozenLinearFn
  test_head_and_layout_nodes _HeadFn (pad arm and 8-wide gradient), _NHWCToNCHW (channels < C), ScaleGrad / gen_gradient_scaler at 0 / 1 / 0.5
  test_trunk_node            _TrunkFn on the tiny U-Net (hip_train_trunk / hip_bwd_trunk, res_gradscale 0.5): G, G 2^-20, G 2^10; a skip gradient None;
                             x.requires_grad False
  test_unet_pair             UNetModel.hip_train / hip_bwd on the tiny U-Net
  test_vae_pairs             model.ResnetBlock identity / nin_shortcut, AttnBlock (N = 128, C = 128; N = 256, C = 512; mask refused), Upsample
  test_vae_decoder_pair      Decoder.hip_train / hip_bwd on a two-level decoder

DERIVED bounds (test_hip_autograd_nodes.py): F16_L2 / F16_MAX for a result that is ONE fp16 rounding of an fp32 value -- the leaf dgrads, the
LayerNorm and GroupNorm outputs and backward outputs, d(x_in).
MEASURED bounds (worst value over the cases of the test on MI355X, times two, rounded up to one digit; the kernels are deterministic, the factor
covers other seeds), for every pair whose backward reads fp16 intermediates saved by its forward.  CEILING: no forward may need more than 2e-3
(BLOCK_TOL of test_hip_unet.py), no gradient more than 5e-3 (the attention-backward bound of test_hip_backward_ops.py), in either figure.
The per-item and per-source figures use the same bounds; every reference slab is checked to be non-degenerate (`both`).
The measured worst values stand next to each constant below."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_hip_autograd_nodes import F16_L2, F16_MAX, cmp, launches, rnd

pytestmark = pytest.mark.gpu

FWD_CEIL, GRAD_CEIL = 2e-3, 5e-3
# (forward rel-L2, forward max, gradient rel-L2, gradient max); measured on MI355X (worst over the cases) -> twice that, rounded up to one digit
# and never past the ceiling: where twice the worst value would pass it (marked "ceiling") the bound IS the ceiling and the margin is what is left
RES = (8e-4, 2e-3, 9e-4, 2e-3)           # 3.89e-4 seq y [item 1]; 6.59e-4 unfused_cat emb=raw y [item 1]; 4.38e-4 seq dx_skip [item 1]; 7.46e-4 fused_320 emb=pack dx_skip [item 0]
DORA = (9e-4, 2e-3, 2e-3, 2e-3)          # 4.28e-4, 7.05e-4 y [item 1]; 9.03e-4, 8.95e-4 d conv1.lora_magnitude_vector
ATT = (9e-4, 2e-3, 2e-3, 2e-3)           # 4.01e-4, 5.01e-4 self ln out [item 0]; 6.60e-4 self ln d(LN(x)) [item 1]; 7.90e-4 cross d=40 L=77 dx [item 0]
FFN = (7e-4, 1e-3, 1e-3, 2e-3)           # 3.44e-4 C=96 out; 4.86e-4 C=320 out; 4.88e-4, 5.51e-4 C=320 d(LN(x))
BLK = (2e-3, FWD_CEIL, 2e-3, 3e-3)       # 5.09e-4 C=1280 2x64 x3 [item 0]; 1.03e-3 C=640 1x1024 x3 (ceiling); 8.56e-4 C=320 2x64 dctx [item 0]; 1.12e-3 C=320 2x64 masked dctx [item 1]
STR = (8e-4, 1e-3, 2e-3, 3e-3)           # 3.91e-4 C=320 8x8 mask out [item 0]; 4.99e-4 C=1280 8x8 mask out [item 0]; 9.51e-4 C=1280 8x8 dctx [item 0]; 1.09e-3 C=320 32x32 mask dctx
NODE = (1e-3, 2e-3, 2e-3, 2e-3)          # 4.56e-4, 7.42e-4 pre qin [item 1]; 5.48e-4 pre loss=qin dx [item 1]; 6.95e-4 pre loss=qin dx [item 0]
TRUNK = (FWD_CEIL, FWD_CEIL, 5e-3, GRAD_CEIL)     # 1.30e-3, 1.43e-3 h [item 1] (ceiling); 2.23e-3 dcontext (skip1 None) [item 1]; 2.69e-3 dcontext (skip1 None) (ceiling)
UNET = (FWD_CEIL, FWD_CEIL, GRAD_CEIL, GRAD_CEIL)  # 1.70e-3 eps [item 1]; 1.87e-3 eps [item 0]; 2.89e-3 dcontext [item 1]; 4.74e-3 dcontext -- all four at the ceiling
VAE = (FWD_CEIL, FWD_CEIL, 3e-3, 3e-3)   # 1.05e-3 decoder y [item 0]; 1.21e-3 decoder y (ceiling); 1.28e-3 decoder dz [item 0]; 1.49e-3 decoder dz


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adaface_dev_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ================================================================================================================= helpers
def fill(mod, seed):
    """Every parameter of `mod` := fp16-representable values in its fp32 master: matrices and kernels N(0, 1 / fan_in), norm gains 1 +- 0.2,
    biases N(0, 0.1^2) -- the zero_modules included.  -> {name: fp64 CPU copy}."""
    P = {}
    with torch.no_grad():
        for i, (n, p) in enumerate(mod.named_parameters()):
            s = 1000 * seed + i
            if p.dim() >= 2:
                t = rnd(tuple(p.shape), s, p[0].numel() ** -0.5)
            elif n.endswith("weight"):
                t = (1.0 + 0.2 * rnd(tuple(p.shape), s).float()).half()
            else:
                t = rnd(tuple(p.shape), s, 0.1)
            p.copy_(t.float())
            P[n] = t.double()
    return P


def sub(P, prefix):
    return {n[len(prefix):]: t for n, t in P.items() if n.startswith(prefix)}


def gn_input(shape, seed):
    """A GroupNorm input: scale 2, mean offset 0.5."""
    return (rnd(shape, seed, 2.0).float() + 0.5).half()


def flat(ts):
    out = []
    for t in ts if isinstance(ts, (tuple, list)) else (ts,):
        out += flat(t) if isinstance(t, (tuple, list)) else [t]
    return out


def twice(tag, fn):
    """fn() called twice: every tensor it returns must have the same bits both times.  -> the first result."""
    a, b = fn(), fn()
    fa, fb = [t for t in flat(a) if torch.is_tensor(t) or t is None], [t for t in flat(b) if torch.is_tensor(t) or t is None]
    assert len(fa) == len(fb), tag
    for i, (u, v) in enumerate(zip(fa, fb)):
        assert (u is None and v is None) or (u is not None and v is not None and torch.equal(u, v)), (tag, i, "the second call gave other bits")
    return a


def both(tag, got, ref, l2, mx, B=0, dtype=torch.float16):
    """cmp on the whole tensor and on each of its B batch items (batch-major leading dimension); no reference slab may be degenerate."""
    assert got is not None, (tag, "no tensor came back")
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    cmp(tag, got, ref, l2, mx, dtype)
    if B > 1:
        g, r = got.detach().reshape(B, -1), ref.detach().reshape(B, -1)
        assert slabs_ok(ref, B), (tag, "a reference slab is degenerate")
        for i in range(B):
            cmp(f"{tag} [item {i}]", g[i], r[i], l2, mx)


def slabs_ok(ref, B):
    r = ref.detach().reshape(B, -1).abs()
    return float(r.amax(1).min()) > 0.05 * float(r.max()) and float(r.pow(2).sum(1).min()) > 0.0025 * float(r.pow(2).sum(1).max())


def ref_grads(y, G, xs):
    """fp64 gradients of the linear loss sum(y G) w.r.t. xs."""
    return torch.autograd.grad((y * G.double()).sum(), xs, retain_graph=True, allow_unused=True)


def leaf(t16):
    return t16.double().requires_grad_(True)


# ------------------------------------------------------------------------------------------ fp64 restatements (NHWC / token-major)
def r_conv(x, w, b, stride=1):
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=stride, padding=w.shape[-1] // 2).permute(0, 2, 3, 1)


def r_up(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def r_gn(x, w, b, eps, silu, groups=32):
    y = F.group_norm(x.permute(0, 3, 1, 2), groups, w, b, eps).permute(0, 2, 3, 1)
    return F.silu(y) if silu else y


def r_ln(x, P, name):
    return F.layer_norm(x, (x.shape[-1],), P[name + ".weight"], P[name + ".bias"], 1e-5)


def r_res(x, e, P):
    """ResBlock on x [B, H, W, Cin] (a SkipCat: the concatenation) with e [B, Cout] = emb_layers(emb)."""
    h = r_conv(r_gn(x, P["in_layers.0.weight"], P["in_layers.0.bias"], 1e-5, True), P["in_layers.2.weight"], P["in_layers.2.bias"]) + e[:, None, None, :]
    h = r_conv(r_gn(h, P["out_layers.0.weight"], P["out_layers.0.bias"], 1e-5, True), P["out_layers.3.weight"], P["out_layers.3.bias"])
    return h + (r_conv(x, P["skip_connection.weight"], P["skip_connection.bias"]) if "skip_connection.weight" in P else x)


def r_emb(emb, P):
    return F.linear(F.silu(emb), P["emb_layers.1.weight"], P["emb_layers.1.bias"])


def r_attn(x, src, P, heads, keep=None):
    """CrossAttention on x [B, N, C] with keys / values from src [B, L, Cc]; keep [B, L] bool: masked_fill(~keep, -finfo.max)."""
    B, N, _ = x.shape
    q, k, v = x @ P["to_q.weight"].t(), src @ P["to_k.weight"].t(), src @ P["to_v.weight"].t()
    C = q.shape[-1]
    d = C // heads
    sp = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    s = (sp(q) @ sp(k).transpose(-1, -2)) * d ** -0.5
    if keep is not None:
        s = s.masked_fill(~keep[:, None, None, :], -torch.finfo(s.dtype).max)
    o = (torch.softmax(s, dim=-1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, N, C)
    return o @ P["to_out.0.weight"].t() + P["to_out.0.bias"]


def r_ff(x, P):
    a, gate = F.linear(x, P["net.0.proj.weight"], P["net.0.proj.bias"]).chunk(2, dim=-1)
    return F.linear(a * F.gelu(gate), P["net.2.weight"], P["net.2.bias"])


def r_block(x, ctx, P, heads, keep=None):
    x1 = r_attn(r_ln(x, P, "norm1"), r_ln(x, P, "norm1"), sub(P, "attn1."), heads, keep) + x
    x2 = r_attn(r_ln(x1, P, "norm2"), ctx, sub(P, "attn2."), heads) + x1
    return r_ff(r_ln(x2, P, "norm3"), sub(P, "ff.")) + x2


def r_keep(mask, H, W, live_rule=False):
    """[B, 1, h0, w0] mask -> [B, H W] bool at the layer's resolution (nearest), or None where the live rule drops it for the whole batch."""
    if mask is None:
        return None
    m2 = F.interpolate(mask.float(), size=(H, W), mode="nearest").reshape(mask.shape[0], H * W) != 0
    if live_rule and bool((m2.sum(1) == 0).any()):
        return None
    return m2


def r_st(x, ctx, P, heads, keep=None):
    B, H, W, C = x.shape
    y = r_conv(r_gn(x, P["norm.weight"], P["norm.bias"], 1e-6, False), P["proj_in.weight"], P["proj_in.bias"]).reshape(B, H * W, -1)
    y = r_block(y, ctx, sub(P, "transformer_blocks.0."), heads, keep)
    return r_conv(y.reshape(B, H, W, -1), P["proj_out.weight"], P["proj_out.bias"]) + x


# ============================================================================================================ 1. leaf pairs
CONV_CASES = {  # name: (cin, cout, kernel, stride, H, W, cin_pad)
    "3x3": (64, 128, 3, 1, 8, 8, 0), "3x3s2": (64, 64, 3, 2, 16, 16, 0), "3x3s2_odd": (64, 64, 3, 2, 15, 17, 0), "1x1": (64, 128, 1, 1, 8, 8, 0),
    "cin_pad": (4, 64, 3, 1, 8, 8, 8), "head": (64, 4, 3, 1, 8, 8, 0)}


@functools.lru_cache(maxsize=None)
def conv_problem(name):
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import Conv2d
    cin, cout, k, stride, H, W, cin_pad = CONV_CASES[name]
    conv = Conv2d(cin, cout, k, stride=stride, padding=k // 2)
    conv.cin_pad = cin_pad
    P = fill(conv, 11)
    x = rnd((2, H, W, cin), 12)
    xd = leaf(x)
    y = r_conv(xd, P["weight"], P["bias"], stride)
    G = rnd(tuple(y.shape), 13)
    return dict(conv=conv, x=x, G=G, y=y.detach(), dx=ref_grads(y, G, (xd,))[0])


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_pairs(dev, name):
    """Conv2d.hip_train / hip_bwd (= hip_dgrad with the saved input size) against F.conv2d and its autograd.  3x3s2_odd: the forward output is 8x9 and
    in_hw = (15, 17) is the 2H - 1 arm of conv3x3(upsample=2).  cin_pad: the input carries 4 zero channels, the gradient comes back 4 wide.  head: 4 output
    channels, the incoming gradient zero padded to 8 (what _HeadFn and UNetModel.hip_bwd hand it).
    Bounds derived: y, dx one fp16 rounding of an fp32 sum.  Worst on MI355X: 2.18e-4 (head y) / 3.83e-4 (3x3 dx) of 6e-4 / 9.8e-4."""
    cin, cout, k, stride, H, W, cin_pad = CONV_CASES[name]
    P = conv_problem(name)
    conv = P["conv"].to(dev)
    x = P["x"].to(dev)
    if cin_pad:
        x = F.pad(x, (0, cin_pad - cin))
    G = P["G"].to(dev)
    Gd = F.pad(G, (0, 8 - cout)) if cout % 8 else G

    def run():
        y, saved = conv.hip_train(x)
        return y, conv.hip_bwd(saved, Gd), conv.hip_dgrad(Gd, in_hw=(H, W))

    with launches() as names:
        y, dx, dx2 = twice(name, run)
    assert names and all(n.startswith("af_gemm") for n in names), names
    assert conv.hip_train(x)[1] == (H, W)
    assert torch.equal(dx, dx2), "hip_bwd and hip_dgrad(in_hw=) differ"
    both(f"conv {name} y", y, P["y"], F16_L2, F16_MAX, 2)
    both(f"conv {name} dx", dx, P["dx"], F16_L2, F16_MAX, 2)
    if name == "3x3s2_odd":
        assert tuple(y.shape) == (2, 8, 9, cout)


@pytest.mark.parametrize("with_res", [False, True])
def test_linear_dgrad(dev, with_res):
    """Linear.hip_dgrad: dx = G W (+ residual), one fp16 rounding of the fp32 sum (derived bound).  Worst on MI355X: 2.07e-4 / 3.68e-4."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import Linear
    M, K, N = 77, 320, 192
    lin = Linear(K, N)
    P = fill(lin, 21)
    G, res = rnd((M, N), 22), rnd((M, K), 23)
    ref = G.double() @ P["weight"] + (res.double() if with_res else 0)
    lin = lin.to(dev)
    with launches() as names:
        dx, = twice("linear", lambda: (lin.hip_dgrad(G.to(dev), residual=res.to(dev) if with_res else None),))
    assert set(names) == {"af_gemm"}, names
    both(f"linear dgrad res={int(with_res)}", dx, ref, F16_L2, F16_MAX)


GN_CASES = [(320, 0), (192, 128), (2560, 0), (1280, 1280)]


@functools.lru_cache(maxsize=None)
def gn_problem(c1, c2):
    C, B, H, W = c1 + c2, 2, 8, 8
    g = (1.0 + 0.2 * rnd((C,), 31).float()).half()
    b = rnd((C,), 32, 0.2)
    x1, x2 = gn_input((B, H, W, c1), 33), (gn_input((B, H, W, c2), 34) if c2 else None)
    G, add = rnd((B, H, W, C), 35), rnd((B, H, W, C), 36)
    out = {}
    for silu in (True, False):
        for eps in (1e-5, 1e-6):
            xs = [leaf(x1)] + ([leaf(x2)] if c2 else [])
            y = r_gn(torch.cat(xs, -1), g.double(), b.double(), eps, silu)
            out[(silu, eps)] = (y.detach(), ref_grads(y, G, xs))
    return dict(g=g, b=b, x1=x1, x2=x2, G=G, add=add, refs=out)


@pytest.mark.parametrize("c1,c2", GN_CASES)
def test_groupnorm_pair(dev, c1, c2):
    """GroupNorm32.hip_train / hip_bwd against F.group_norm (+ F.silu) and its autograd: SiLU on / off, eps 1e-5 / 1e-6, one source or two (the
    groups span the concatenation; 192 + 128: groups of 10 channels, one of them has channels of both sources; 1280 + 1280: the widest decoder input), with and without
    `add` (the reference adds it in fp64; with two sources `add` is as wide as both and each source takes its columns).
    Bounds derived: y and every dx one fp16 rounding of fp32 arithmetic.  Worst on MI355X: 2.15e-4 (192 + 128 dx1) / 4.58e-4 (192 + 128 y)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import GroupNorm32
    P = gn_problem(c1, c2)
    C = c1 + c2
    x1, x2 = P["x1"].to(dev), (P["x2"].to(dev) if c2 else None)
    G, add = P["G"].to(dev), P["add"].to(dev)
    for (silu, eps), (y_ref, dref) in P["refs"].items():
        gn = GroupNorm32(32, C, eps=eps)
        with torch.no_grad():
            gn.weight.copy_(P["g"].float())
            gn.bias.copy_(P["b"].float())
        gn = gn.to(dev)
        for with_add in (False, True):
            tag = f"groupnorm {c1}+{c2} silu={int(silu)} eps={eps:g} add={int(with_add)}"

            def run():
                y, st = gn.hip_train(x1, silu=silu, x2=x2)
                return y, gn.hip_bwd(x1, st, G, silu=silu, x2=x2, add=add if with_add else None)

            with launches() as names:
                y, dx = twice(tag, run)
            assert "af_groupnorm_bwd" in names, (tag, names)
            both(f"{tag} y", y, y_ref, F16_L2, F16_MAX, 2)
            got = (dx,) if x2 is None else dx
            assert len(got) == len(dref), tag
            off = 0
            for i, (gi, ri) in enumerate(zip(got, dref)):
                w = ri.shape[-1]
                ri = ri + (P["add"][..., off:off + w].double() if with_add else 0)
                both(f"{tag} dx{i + 1}", gi, ri, F16_L2, F16_MAX, 2)
                off += w


@pytest.mark.parametrize("C", [320, 1280])
def test_layernorm_bwd(dev, C):
    """LayerNorm.hip and hip_bwd (with / without add) against F.layer_norm and its autograd at 77 rows; row means offset.  Derived: one fp16 rounding.  Worst on MI355X: 2.08e-4 (C = 1280 dx) / 4.36e-4 (C = 320 dx)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import LayerNorm
    rows = 77
    ln = LayerNorm(C)
    P = fill(ln, 41)
    x, G, add = (rnd((rows, C), 42, 2.0).float() - 0.3).half(), rnd((rows, C), 43), rnd((rows, C), 44)
    xd = leaf(x)
    y_ref = F.layer_norm(xd, (C,), P["weight"], P["bias"], 1e-5)
    dref, = ref_grads(y_ref, G, (xd,))
    ln = ln.to(dev)
    for with_add in (False, True):
        with launches() as names:
            y, dx = twice("layernorm", lambda: (ln.hip(x.to(dev)), ln.hip_bwd(x.to(dev), G.to(dev), add=add.to(dev) if with_add else None)))
        assert "af_layernorm_bwd" in names, names
        both(f"layernorm {C} y", y, y_ref, F16_L2, F16_MAX)
        both(f"layernorm {C} add={int(with_add)} dx", dx, dref + (add.double() if with_add else 0), F16_L2, F16_MAX)


# ============================================================================================================== 2. ResBlock
RES_CASES = {  # name: (c1, c2, cout, H = W, fused shortcut)
    "identity": (320, 0, 320, 8, False), "fused_1280": (1280, 1280, 1280, 8, True), "fused_320": (640, 320, 320, 16, True),
    "unfused": (96, 0, 64, 8, False), "unfused_cat": (64, 32, 64, 8, False), "identity_cat": (32, 32, 64, 8, False)}
EMB, EMB_OFF, EMB_EXTRA = 128, 24, 64


@functools.lru_cache(maxsize=None)
def res_problem(name):
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import ResBlock
    c1, c2, cout, hw, _ = RES_CASES[name]
    B = 2
    rb = ResBlock(c1 + c2, EMB, 0.0, out_channels=cout)
    P = fill(rb, 51)
    x1, x2 = gn_input((B, hw, hw, c1), 52), (gn_input((B, hw, hw, c2), 53) if c2 else None)
    emb, all_out, G = rnd((B, EMB), 54), rnd((B, cout + EMB_EXTRA), 55, 0.5), rnd((B, hw, hw, cout), 56)
    refs = {}
    for kind in ("raw", "pack"):
        xs = [leaf(x1)] + ([leaf(x2)] if c2 else [])
        e = r_emb(emb.double(), P) if kind == "raw" else all_out[:, EMB_OFF:EMB_OFF + cout].double()
        y = r_res(torch.cat(xs, -1), e, P)
        refs[kind] = (y.detach(), ref_grads(y, G, xs))
    return dict(rb=rb, P=P, x1=x1, x2=x2, emb=emb, all_out=all_out, G=G, refs=refs)


@pytest.mark.parametrize("name", list(RES_CASES))
def test_resblock_pair(dev, name):
    """ResBlock.hip_train / hip_bwd against the fp64 restatement (GroupNorm + SiLU, 3x3, + emb, GroupNorm + SiLU, 3x3, + shortcut) at B = 2: y, then dx or
    (dx_h, dx_skip) each on its own.  The time embedding once as a raw [B, emb] tensor (SiLU + emb_layers on the device) and once as an EmbPack whose all_out is
    64 columns wider than this block's slice at offset 24 (row stride != Cout).  fused_*: the 1x1 shortcut runs inside the second convolution in the forward
    and as its own dgrad in the backward (_skip_fusable asserted); unfused*: its own launch both ways; identity_cat: torch.cat.
    Measured (RES): the backward reads the fp16 conv1 output and block inputs."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import EmbPack, SkipCat
    c1, c2, cout, hw, fused = RES_CASES[name]
    P = res_problem(name)
    rb = P["rb"].to(dev)
    x1, x2 = P["x1"].to(dev), (P["x2"].to(dev) if c2 else None)
    assert (not isinstance(rb.skip_connection, torch.nn.Identity) and rb._skip_fusable(x1, x2)) == fused
    G = P["G"].to(dev)
    xin = SkipCat((x1, x2)) if c2 else x1
    for kind in ("raw", "pack"):
        if kind == "raw":
            rb._emb_slice, emb = None, P["emb"].to(dev)
        else:
            rb._emb_slice, emb = (EMB_OFF, cout), EmbPack(None, P["all_out"].to(dev))
            assert emb.all_out.stride(0) != cout
        tag = f"RES {name} emb={kind}"

        def run():
            y, saved = rb.hip_train(xin, emb)
            return y, rb.hip_bwd(saved, G)

        with launches() as names:
            y, dx = twice(tag, run)
        assert names.count("af_groupnorm_bwd") == 4 and sum(n.startswith("af_gemm") for n in names) >= 8, (tag, names)
        y_ref, dref = P["refs"][kind]
        both(f"{tag} y", y, y_ref, RES[0], RES[1], 2)
        if c2:
            assert isinstance(dx, tuple) and len(dx) == 2, tag
            both(f"{tag} dx_h", dx[0], dref[0], RES[2], RES[3], 2)
            both(f"{tag} dx_skip", dx[1], dref[1], RES[2], RES[3], 2)
        else:
            both(f"{tag} dx", dx, dref[0], RES[2], RES[3], 2)


def r_dora_conv(x, W, b, A, Bm, m, scaling):
    """peft's DoRA convolution in branch form: base(x) + (s - 1) conv(x, W) + s scaling B(A(x)), s = m / ||W + scaling B A|| with the norm detached."""
    norm = (W + scaling * (Bm.flatten(1) @ A.flatten(1)).reshape(W.shape)).flatten(1).norm(dim=1).detach()
    s = m / norm
    xc = x.permute(0, 3, 1, 2)
    pad = W.shape[-1] // 2
    lora = F.conv2d(F.conv2d(xc, A, None, padding=pad), Bm)
    y = F.conv2d(xc, W, b, padding=pad) + (s - 1)[None, :, None, None] * F.conv2d(xc, W, None, padding=pad) + (s * scaling)[None, :, None, None] * lora
    return y.permute(0, 2, 3, 1)


DORA_KEYS = {"conv1": "in_layers.2", "conv2": "out_layers.3", "conv_shortcut": "skip_connection"}
DORA_RANK, DORA_ALPHA = 32, 16


@functools.lru_cache(maxsize=None)
def dora_problem():
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import ResBlock
    from adaface_dev_amd.ldm.modules.dora import DoRAConvAdapter
    c1, c2, cout, hw, B = 64, 32, 64, 8, 2
    rb = ResBlock(c1 + c2, EMB, 0.0, out_channels=cout)
    P = fill(rb, 61)
    ads, A = {}, {}
    for i, (key, lname) in enumerate(DORA_KEYS.items()):
        conv = dict(rb.named_modules())[lname]
        ad = DoRAConvAdapter(conv, rank=DORA_RANK, lora_alpha=DORA_ALPHA, lora_dropout=0.0)
        a, b = rnd(tuple(ad.lora_A.shape), 62 + i, 0.05), rnd(tuple(ad.lora_B.shape), 65 + i, 0.2)
        m = (ad.lora_magnitude_vector.detach() * (1.0 + 0.2 * rnd((cout,), 68 + i).float().abs())).half()
        with torch.no_grad():
            ad.lora_A.copy_(a.float()), ad.lora_B.copy_(b.float()), ad.lora_magnitude_vector.copy_(m.float())
        ads[key] = ad
        A[key] = dict(lora_A=leaf(a), lora_B=leaf(b), lora_magnitude_vector=leaf(m))
    x1, x2 = gn_input((B, hw, hw, c1), 71), gn_input((B, hw, hw, c2), 72)
    emb, G = rnd((B, EMB), 73), rnd((B, hw, hw, cout), 74)
    xs = [leaf(x1), leaf(x2)]
    x = torch.cat(xs, -1)
    sc = DORA_ALPHA / DORA_RANK
    dc = lambda key, t: r_dora_conv(t, P[DORA_KEYS[key] + ".weight"], P[DORA_KEYS[key] + ".bias"], A[key]["lora_A"], A[key]["lora_B"],
                                    A[key]["lora_magnitude_vector"], sc)
    h = dc("conv1", r_gn(x, P["in_layers.0.weight"], P["in_layers.0.bias"], 1e-5, True)) + r_emb(emb.double(), P)[:, None, None, :]
    y = dc("conv2", r_gn(h, P["out_layers.0.weight"], P["out_layers.0.bias"], 1e-5, True)) + dc("conv_shortcut", x)
    names = [(k, p) for k in sorted(A) for p in ("lora_A", "lora_B", "lora_magnitude_vector")]
    grads = ref_grads(y, G, xs + [A[k][p] for k, p in names])
    return dict(rb=rb, ads=ads, x1=x1, x2=x2, emb=emb, G=G, y=y.detach(), dx=grads[:2], names=names, dparams=grads[2:])


def test_resblock_dora_node(dev):
    """_ResBlockFn.apply on a 64 + 32 -> 64 ResBlock with trainable DoRA adapters (rank 32, dropout 0) on conv1, conv2 and conv_shortcut, against fp64 autograd
    of the branch form (r_dora_conv): y, dh, dskip and the nine adapter gradients (lora_A, lora_B, magnitude of each).  Measured (DORA)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.capture_graph import _ResBlockFn, resblock_lora_params
    P = dora_problem()
    rb = P["rb"].to(dev)
    rb._emb_slice = None
    lora = {k: ad.to(dev).train() for k, ad in P["ads"].items()}
    G = P["G"].to(dev)

    def run():
        for ad in lora.values():
            for p in ad.parameters():
                p.grad = None
        h, skip = P["x1"].to(dev).requires_grad_(True), P["x2"].to(dev).requires_grad_(True)
        with launches() as names:
            y = _ResBlockFn.apply(rb, h, skip, P["emb"].to(dev), lora, *resblock_lora_params(lora))
            (y.float() * G.float()).sum().backward()
        assert "af_groupnorm_bwd" in names and rb._lora is None
        return [y.detach(), h.grad, skip.grad] + [getattr(lora[k], p).grad.clone() for k, p in P["names"]]

    out = twice("dora", run)
    both("DORA y", out[0], P["y"], DORA[0], DORA[1], 2)
    both("DORA dh", out[1], P["dx"][0], DORA[2], DORA[3], 2)
    both("DORA dskip", out[2], P["dx"][1], DORA[2], DORA[3], 2)
    for (k, p), got, ref in zip(P["names"], out[3:], P["dparams"]):
        both(f"DORA d {k}.{p}", got, ref, DORA[2], DORA[3], dtype=torch.float32)


# ======================================================================================================== 3. Down / Upsample
@functools.lru_cache(maxsize=None)
def updown_problem(kind, C, H, W):
    from adaface_dev_amd.ldm.modules.diffusionmodules import model as vae
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import Downsample, Upsample
    m = {"down": lambda: Downsample(C, True, out_channels=C), "up": lambda: Upsample(C, True, out_channels=C), "vae_up": lambda: vae.Upsample(C, True)}[kind]()
    P = fill(m, 81)
    x = rnd((2, H, W, C), 82)
    xd = leaf(x)
    y = r_conv(xd, P["op.weight"], P["op.bias"], 2) if kind == "down" else r_conv(r_up(xd), P["conv.weight"], P["conv.bias"])
    G = rnd(tuple(y.shape), 83)
    return dict(m=m, P=P, x=x, G=G, y=y.detach(), dx=ref_grads(y, G, (xd,))[0])


@pytest.mark.parametrize("kind,C,H,W,phase", [("down", 64, 16, 16, None), ("down", 64, 15, 17, None), ("up", 64, 8, 8, False), ("up", 320, 16, 16, True)])
def test_updown_pairs(dev, kind, C, H, W, phase):
    """openaimodel.Downsample / Upsample as the only layer of a TimestepEmbedSequential: hip_train / hip_bwd against F.conv2d (stride 2; nearest x2 in front) and
    its autograd.  down 15x17: odd sizes both ways (forward 8x9).  up: the forward's form is asked of ops.conv_up2_config / conv_up2_eligible and seen in the
    launch name -- the nine-tap gather at 8x8, the four-phase pack at 16x16 with C = 320; the backward is the plain dgrad + 2x2 block sums either way.
    Bounds derived: y one fp16 rounding; dx (up) a sum of four fp16 dgrad values rounded again: per element at most 2^-11 (sum |v_i| + |sum v_i|), so twice the single-rounding bounds.
    Worst on MI355X: y 2.92e-4 (up 320) / 4.32e-4 (down 15x17); dx (up) 2.97e-4 / 5.55e-4 of 1.2e-3 / 2.0e-3."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import TimestepEmbedSequential
    P = updown_problem(kind, C, H, W)
    seq = TimestepEmbedSequential(P["m"]).to(dev)
    x, G = P["x"].to(dev), P["G"].to(dev)

    def run():
        y, saved = seq.hip_train(x, None)
        return y, seq.hip_bwd(saved, G)

    with launches() as names:
        y, (dx, dctx) = twice(kind, run)
    assert dctx is None
    if phase is not None:
        tile, splits = ops.conv_up2_config(2, H, W, C, C)
        assert (tile == 14 and ops.conv_up2_eligible(ops.conv_up2_desc(2, H, W, C, C, tile=tile, splits=splits))) == phase
        assert ("af_gemm(conv3x3_up2)" in names) == phase and "af_sumpool2x2" in names, names
    k = 1 if kind == "down" else 2
    both(f"{kind} {C} {H}x{W} y", y, P["y"], F16_L2, F16_MAX, 2)
    both(f"{kind} {C} {H}x{W} dx", dx, P["dx"], k * F16_L2, k * F16_MAX, 2)


def test_sequential_returns_the_pair_for_a_skipcat(dev):
    """TimestepEmbedSequential(ResBlock 64 + 32 -> 64, Upsample) on a SkipCat: hip_bwd returns ((dx_h, dx_skip), None), each against fp64.  Measured (RES)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import SkipCat, TimestepEmbedSequential
    R, U = res_problem("unfused_cat"), updown_problem("up", 64, 8, 8)
    seq = TimestepEmbedSequential(R["rb"], U["m"]).to(dev)
    R["rb"]._emb_slice = None
    xs = [leaf(R["x1"]), leaf(R["x2"])]
    y_ref = r_conv(r_up(r_res(torch.cat(xs, -1), r_emb(R["emb"].double(), R["P"]), R["P"])), U["P"]["conv.weight"], U["P"]["conv.bias"])
    G = rnd(tuple(y_ref.shape), 91)
    dref = ref_grads(y_ref, G, xs)

    def run():
        y, saved = seq.hip_train(SkipCat((R["x1"].to(dev), R["x2"].to(dev))), R["emb"].to(dev))
        return y, seq.hip_bwd(saved, G.to(dev))

    y, (dx, dctx) = twice("seq", run)
    assert dctx is None and isinstance(dx, tuple) and len(dx) == 2
    both("RES seq y", y, y_ref, RES[0], RES[1], 2)
    both("RES seq dx_h", dx[0], dref[0], RES[2], RES[3], 2)
    both("RES seq dx_skip", dx[1], dref[1], RES[2], RES[3], 2)


# ========================================================================================================== 4. CrossAttention
HEADS = 8
CTX_DIM = 768


def att_keep(B, N):
    """Item 0 keeps ~70 % of the keys, the last item none."""
    keep = torch.rand((B, N), generator=torch.Generator().manual_seed(101)) > 0.3
    keep[B - 1] = False
    return keep


@functools.lru_cache(maxsize=None)
def self_problem(d, masked):
    from adaface_dev_amd.ldm.modules.attention import CrossAttention
    B, N, C = 2, 64, HEADS * d
    m = CrossAttention(C, None, HEADS, d)
    P = fill(m, 102)
    x, res, G = rnd((B, N, C), 103), rnd((B, N, C), 104), rnd((B, N, C), 105)
    keep = att_keep(B, N) if masked else None
    xd = leaf(x)
    y = r_attn(xd, xd, P, HEADS, keep) + res.double()
    return dict(m=m, x=x, res=res, G=G, keep=keep, y=y.detach(), dx=ref_grads(y, G, (xd,))[0])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_self_attention_pair(dev, d, masked):
    """CrossAttention.hip_train / hip_bwd, self arm, 8 heads of d = 40 / 80 / 160 at B = 2, N = 64 with a residual: out and dx per item.  masked: a key bias with
    item 0 partly and item 1 FULLY masked -- the reference is masked_fill(~keep, -finfo.max), so item 1 attends uniformly and no gradient reaches its scores.
    Measured (ATT)."""
    from adaface_dev_amd import ops
    P = self_problem(d, masked)
    B, N, C = 2, 64, HEADS * d
    m = P["m"].to(dev)
    x, res, G = (P[k].to(dev).reshape(B * N, C) for k in ("x", "res", "G"))
    kb = ops.make_keybias(P["keep"].to(dev), N) if masked else None

    def run():
        y, saved = m.hip_train(x, B, N, None, kb, residual=res)
        return y, m.hip_bwd(saved, G)

    tag = f"ATT self d={d} masked={int(masked)}"
    with launches() as names:
        y, (dx, dctx) = twice(tag, run)
    assert "af_attention_bwd" in names and "af_attention_strided" in names and dctx is None, (tag, names)
    both(f"{tag} out", y, P["y"].reshape(B * N, C), ATT[0], ATT[1], B)
    both(f"{tag} dx", dx, P["dx"].reshape(B * N, C), ATT[2], ATT[3], B)


@functools.lru_cache(maxsize=None)
def self_ln_problem():
    from adaface_dev_amd.ldm.modules.attention import CrossAttention
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import LayerNorm
    B, N, d = 2, 1024, 40
    C = HEADS * d
    m, ln = CrossAttention(C, None, HEADS, d), LayerNorm(C)
    P, Pl = fill(m, 111), fill(ln, 112)
    x, G = (rnd((B, N, C), 113, 2.0).float() - 0.3).half(), rnd((B, N, C), 114)
    xn = F.layer_norm(x.double(), (C,), Pl["weight"], Pl["bias"], 1e-5).requires_grad_(True)
    y = r_attn(xn, xn, P, HEADS)
    return dict(m=m, ln=ln, x=x, G=G, y=y.detach(), dxn=ref_grads(y, G, (xn,))[0])


def test_self_attention_ln(dev):
    """The folded q | k | v pack: hip_train(x, ln=norm) takes the UN-normalised rows at B x N = 2 x 1024, C = 320 (attention.ln_fold asserted, no LayerNorm
    launch); the backward differentiates up to LN's output, and so does the reference (the gradient w.r.t. LN(x) computed in fp64).  Measured (ATT)."""
    from adaface_dev_amd.ldm.modules import attention
    P = self_ln_problem()
    B, N, C = 2, 1024, 320
    assert attention.ln_fold(C, B * N)
    m, ln = P["m"].to(dev), P["ln"].to(dev)
    x, G = P["x"].to(dev).reshape(B * N, C), P["G"].to(dev).reshape(B * N, C)

    def run():
        y, saved = m.hip_train(x, B, N, None, None, ln=ln)
        return y, m.hip_bwd(saved, G)

    with launches() as names:
        y, (dxn, _) = twice("self ln", run)
    assert "af_layernorm" not in names and "af_attention_bwd" in names, names
    both("ATT self ln out", y, P["y"].reshape(B * N, C), ATT[0], ATT[1], B)
    both("ATT self ln d(LN(x))", dxn, P["dxn"].reshape(B * N, C), ATT[2], ATT[3], B)


@functools.lru_cache(maxsize=None)
def cross_problem(d, L):
    from adaface_dev_amd.ldm.modules.attention import CrossAttention
    B, N, C = 2, 64, HEADS * d
    m = CrossAttention(C, CTX_DIM, HEADS, d)
    P = fill(m, 121)
    x, ctx, res, G, dctx_in = rnd((B, N, C), 122), rnd((B, L, CTX_DIM), 123), rnd((B, N, C), 124), rnd((B, N, C), 125), rnd((B, L, CTX_DIM), 126)
    xd, cd = leaf(x), leaf(ctx)
    y = r_attn(xd, cd, P, HEADS) + res.double()
    dx, dctx = ref_grads(y, G, (xd, cd))
    # L = 1: the softmax of one key is the constant 1, so d(score) and with it dx are EXACTLY zero.  The scale such a dx is measured against: the dx that
    # d(score) = dP = dO . v would carry (the device forms d(score) = P (dP - sum P dP), a difference of two roundings of dP)
    do = (G.double() @ P["to_out.0.weight"]).reshape(B, N, HEADS, d)
    kh, vh = ((ctx[:, :1].double() @ P[n].t()).reshape(B, 1, HEADS, d) for n in ("to_k.weight", "to_v.weight"))
    dx_unit = (((do * vh).sum(-1, keepdim=True) * kh * d ** -0.5).reshape(B, N, C) @ P["to_q.weight"]) if L == 1 else None
    return dict(m=m, x=x, ctx=ctx, res=res, G=G, dctx_in=dctx_in, y=y.detach(), dx=dx, dctx=dctx, dx_unit=dx_unit)


@pytest.mark.parametrize("L", [77, 1, 97])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_cross_attention_pair(dev, d, L):
    """CrossAttention.hip_train / hip_bwd, cross arm, context [2, L, 768] with L = 77 (the text encoder), 1 (a single key: the softmax is 1) and 97 (past one
    64-key block, no multiple of 8), with a residual.  Once with dctx = None, once with an incoming fp16 dctx that must come back as dctx + own (the reference
    adds in fp64).  out, dx, dctx per item.  Measured (ATT)."""
    P = cross_problem(d, L)
    B, N, C = 2, 64, HEADS * d
    m = P["m"].to(dev)
    x, res, G = (P[k].to(dev).reshape(B * N, C) for k in ("x", "res", "G"))
    ctx, dctx_in = P["ctx"].to(dev), P["dctx_in"].to(dev).reshape(B * L, CTX_DIM)
    for incoming in (False, True):
        def run():
            y, saved = m.hip_train(x, B, N, ctx, None, residual=res)
            return y, m.hip_bwd(saved, G, dctx_in if incoming else None)

        tag = f"ATT cross d={d} L={L} dctx_in={int(incoming)}"
        with launches() as names:
            y, (dx, dctx) = twice(tag, run)
        assert "af_attention_bwd" in names, (tag, names)
        both(f"{tag} out", y, P["y"].reshape(B * N, C), ATT[0], ATT[1], B)
        if L == 1:
            # the reference is exactly zero (cross_problem): |dx| against the dx of d(score) = dP.  Derived: dP - sum P dP is a difference of two values that
            # each carry the fp16 rounding of o / dO (2^-11), so at most 2^-10 of it is left: F16_MAX in both figures.  Worst on MI355X: 2.3e-7 / 2.8e-7
            assert float(P["dx"].abs().max()) < 1e-12 * float(P["dx_unit"].abs().max())
            assert dx.dtype == torch.float16 and tuple(dx.shape) == (B * N, C) and bool(torch.isfinite(dx).all())
            g, u = dx.double().cpu().reshape(B, -1), P["dx_unit"].reshape(B, -1)
            for i in range(B):
                e2, em = float(g[i].norm() / u[i].norm()), float(g[i].abs().max() / u[i].abs().max())
                print(f"ERR {tag} dx [item {i}] (against the dx of d(score) = dP): rel-L2 {e2:.3e} (< {F16_MAX:.1e})  max/max {em:.3e} (< {F16_MAX:.1e})")
                assert e2 < F16_MAX and em < F16_MAX, (tag, i, e2, em)
        else:
            both(f"{tag} dx", dx, P["dx"].reshape(B * N, C), ATT[2], ATT[3], B)
        ref = P["dctx"] + (P["dctx_in"].double() if incoming else 0)
        both(f"{tag} dctx", dctx, ref.reshape(B * L, CTX_DIM), ATT[2], ATT[3], B)


# ======================================================================================================= 5. FeedForward / GEGLU
FF_CASES = [(320, 130), (96, 77), (1280, 64)]


@functools.lru_cache(maxsize=None)
def ff_problem(C, rows):
    from adaface_dev_amd.ldm.modules.attention import FeedForward
    from adaface_dev_amd.ldm.modules.diffusionmodules.util import LayerNorm
    ff, ln = FeedForward(C, glu=True), LayerNorm(C)
    P, Pl = fill(ff, 131), fill(ln, 132)
    x, res, G = (rnd((rows, C), 133, 2.0).float() - 0.3).half(), rnd((rows, C), 134), rnd((rows, C), 135)
    xn = F.layer_norm(x.double(), (C,), Pl["weight"], Pl["bias"], 1e-5).requires_grad_(True)
    y = r_ff(xn, P) + res.double()
    return dict(ff=ff, ln=ln, x=x, res=res, G=G, xn=xn.detach(), y=y.detach(), dxn=ref_grads(y, G, (xn,))[0])


@pytest.mark.parametrize("C,rows", FF_CASES)
def test_feedforward_pair(dev, C, rows):
    """FeedForward.hip_train / hip_bwd (GEGLU.hip_train / hip_bwd inside) + residual against fp64: where attention.ln_fold(C) holds (C = 320 at 130 rows, C = 1280 at
    64 rows) the LayerNorm is folded into the GEGLU projection and the pair takes the un-normalised rows; at C = 96 it is not, and the pair takes the device
    LayerNorm's output (one more fp16 tensor).  The gradient is the one w.r.t. LN's output both ways.  Training never runs the one-launch af_ff_* forms.
    Measured (FFN)."""
    from adaface_dev_amd.ldm.modules import attention
    P = ff_problem(C, rows)
    folded = attention.ln_fold(C)
    assert folded == (C % 64 == 0)
    ff, ln = P["ff"].to(dev), P["ln"].to(dev)
    x, res, G = P["x"].to(dev), P["res"].to(dev), P["G"].to(dev)

    def run():
        y, hp = ff.hip_train(x if folded else ln.hip(x), residual=res, ln=ln if folded else None)
        return y, ff.hip_bwd(hp, G)

    tag = f"FFN C={C} rows={rows} folded={int(folded)}"
    with launches() as names:
        y, dxn = twice(tag, run)
    assert "af_geglu_fwd" in names and "af_geglu_bwd" in names and not any(n.startswith("af_ff_") for n in names), (tag, names)
    assert ("af_layernorm" in names) == (not folded), (tag, names)
    both(f"{tag} out", y, P["y"], FFN[0], FFN[1])
    both(f"{tag} d(LN(x))", dxn, P["dxn"], FFN[2], FFN[3])


# ================================================================================================== 6. BasicTransformerBlock
BLK_CASES = [(320, 1, 1024, False), (320, 2, 64, False), (640, 1, 1024, False), (1280, 2, 64, False), (320, 1, 1024, True), (320, 2, 64, True)]
CTX_L = 77


def blk_keep(B, N):
    """Every item keeps a part of the keys (item b masks another ~30 %)."""
    return torch.rand((B, N), generator=torch.Generator().manual_seed(141)) > 0.3


@functools.lru_cache(maxsize=None)
def blk_problem(C, B, N, masked):
    from adaface_dev_amd.ldm.modules.attention import BasicTransformerBlock
    blk = BasicTransformerBlock(C, HEADS, C // HEADS, context_dim=CTX_DIM)
    P = fill(blk, 142)
    x, ctx, G = rnd((B, N, C), 143), rnd((B, CTX_L, CTX_DIM), 144), rnd((B, N, C), 145)
    keep = blk_keep(B, N) if masked else None
    xd, cd = leaf(x), leaf(ctx)
    y = r_block(xd, cd, P, HEADS, keep)
    dx, dctx = ref_grads(y, G, (xd, cd))
    return dict(blk=blk, x=x, ctx=ctx, G=G, keep=keep, y=y.detach(), dx=dx, dctx=dctx)


@pytest.mark.parametrize("C,B,N,masked", BLK_CASES)
def test_transformer_block(dev, C, B, N, masked):
    """BasicTransformerBlock.hip_train / hip_bwd at the production head dims 40 / 80 / 160 with a 77 x 768 context: B x N = 1 x 1024 takes the arm with all three
    LayerNorms folded (no af_layernorm launch in the forward), 2 x 64 the arm with none folded (three) -- attention.ln_fold asserted; the two C = 320 cases again
    with a key bias on the self-attention.  x3, dx, dctx (per item at B = 2).  Measured (BLK)."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules import attention
    P = blk_problem(C, B, N, masked)
    folded = attention.ln_fold(C, B * N)
    assert folded == (B * N >= 1024)
    blk = P["blk"].to(dev)
    x, G, ctx = P["x"].to(dev).reshape(B * N, C), P["G"].to(dev).reshape(B * N, C), P["ctx"].to(dev)
    kb = ops.make_keybias(P["keep"].to(dev), N) if masked else None
    fwd_names = []

    def run():
        with launches() as nf:
            y, saved = blk.hip_train(x, B, N, ctx, kb)
        fwd_names[:] = nf
        return y, blk.hip_bwd(saved, G, None)

    tag = f"BLK C={C} {B}x{N} masked={int(masked)} folded={int(folded)}"
    with launches() as names:
        y, (dx, dctx) = twice(tag, run)
    assert fwd_names.count("af_layernorm") == (0 if folded else 3), (tag, fwd_names)
    assert names.count("af_layernorm_bwd") == 6 and names.count("af_attention_bwd") == 4 and "af_geglu_bwd" in names, (tag, names)
    both(f"{tag} x3", y, P["y"].reshape(B * N, C), BLK[0], BLK[1], B)
    both(f"{tag} dx", dx, P["dx"].reshape(B * N, C), BLK[2], BLK[3], B)
    both(f"{tag} dctx", dctx, P["dctx"].reshape(B * CTX_L, CTX_DIM), BLK[2], BLK[3], B)


# ===================================================================================================== 7. SpatialTransformer
ST_CASES = [(320, 8, "none"), (320, 8, "mask"), (320, 8, "live"), (320, 32, "none"), (320, 32, "mask"), (1280, 8, "none"), (1280, 8, "mask")]


def st_mask(B, hw, live):
    """[B, 1, 2 hw, 2 hw]: item 0 masks its upper third, item 1 a column band; live: item 1 is set at odd positions only, which the nearest resize (it reads
    the even ones) never meets -- its mask is empty at this resolution."""
    m = torch.ones((B, 1, 2 * hw, 2 * hw))
    m[0, :, :(2 * hw) // 3] = 0
    m[1, :, :, hw:hw + hw // 2] = 0
    if live:
        m[1] = 0
        m[1, :, 1::2, 1::2] = 1
    return m


@functools.lru_cache(maxsize=None)
def st_problem(C, hw, mode):
    from adaface_dev_amd.ldm.modules.attention import SpatialTransformer
    B = 2
    st = SpatialTransformer(C, HEADS, C // HEADS, context_dim=CTX_DIM)
    P = fill(st, 151)
    x, ctx, G = gn_input((B, hw, hw, C), 152), rnd((B, CTX_L, CTX_DIM), 153), rnd((B, hw, hw, C), 154)
    mask = None if mode == "none" else st_mask(B, hw, mode == "live")
    keep = r_keep(mask, hw, hw, live_rule=mode == "live")
    xd, cd = leaf(x), leaf(ctx)
    y = r_st(xd, cd, P, HEADS, keep)
    dx, dctx = ref_grads(y, G, (xd, cd))
    return dict(st=st, x=x, ctx=ctx, G=G, mask=mask, keep=keep, y=y.detach(), dx=dx, dctx=dctx)


@pytest.mark.parametrize("C,hw,mode", ST_CASES)
def test_spatial_transformer(dev, C, hw, mode):
    """SpatialTransformer.hip_train / hip_bwd at B = 2 (GroupNorm 1e-6, proj_in, the block, a NON-ZERO proj_out, + input): out, dx -- the full gradient, the
    residual path hip_bwd carries as add=dy included -- and dctx, per item.  mask: [B, 1, 2H, 2W], nearest-resized (r_keep restates it with F.interpolate);
    live: live_mask_rule = True and an item whose mask is empty at this resolution: the key bias is dropped for the whole batch, in the reference too (asserted:
    the reference runs unmasked).  32x32: 2 x 1024 rows, the folded arm.  Measured (STR)."""
    P = st_problem(C, hw, mode)
    B = 2
    st = P["st"].to(dev)
    st.live_mask_rule = mode == "live"
    assert (P["keep"] is None) == (mode != "mask")
    x, G, ctx = P["x"].to(dev), P["G"].to(dev), P["ctx"].to(dev)
    mask = None if P["mask"] is None else P["mask"].to(dev)

    def run():
        y, saved = st.hip_train(x, ctx, mask)
        return y, st.hip_bwd(saved, G, None)

    tag = f"STR C={C} {hw}x{hw} {mode}"
    with launches() as names:
        y, (dx, dctx) = twice(tag, run)
    assert "af_groupnorm_bwd" in names and names.count("af_attention_bwd") == 4, (tag, names)
    both(f"{tag} out", y, P["y"], STR[0], STR[1], B)
    both(f"{tag} dx", dx, P["dx"], STR[2], STR[3], B)
    both(f"{tag} dctx", dctx, P["dctx"].reshape(B * CTX_L, CTX_DIM), STR[2], STR[3], B)


# ===================================================================================================== 8. capture-graph nodes
@functools.lru_cache(maxsize=None)
def node_problem():
    """SpatialTransformer(320, 8, 40) at 8x8, B = 2, cut where capture_graph.py cuts it: (x1, qin) = pre(x); out = post(x2, x_in)."""
    from adaface_dev_amd.ldm.modules.attention import SpatialTransformer
    B, hw, C = 2, 8, 320
    st = SpatialTransformer(C, HEADS, C // HEADS, context_dim=CTX_DIM)
    P = fill(st, 161)
    Pb = sub(P, "transformer_blocks.0.")
    x, G1, Gq = gn_input((B, hw, hw, C), 162), rnd((B * hw * hw, C), 163), rnd((B * hw * hw, C), 164, 3.0)
    keep = att_keep(B, hw * hw)
    keep[B - 1] = torch.rand((hw * hw,), generator=torch.Generator().manual_seed(165)) > 0.5
    xd = leaf(x)
    y = r_conv(r_gn(xd, P["norm.weight"], P["norm.bias"], 1e-6, False), P["proj_in.weight"], P["proj_in.bias"]).reshape(B, hw * hw, C)
    n1 = r_ln(y, Pb, "norm1")
    x1 = (r_attn(n1, n1, sub(Pb, "attn1."), HEADS, keep) + y).reshape(B * hw * hw, C)
    qin = r_ln(x1, Pb, "norm2")
    pre = dict(x1=x1.detach(), qin=qin.detach(), d_x1=ref_grads(x1, G1, (xd,))[0], d_qin=ref_grads(qin, Gq, (xd,))[0])
    x2, x_in, G = rnd((B * hw * hw, C), 166), gn_input((B, hw, hw, C), 167), rnd((B, hw, hw, C), 168)
    x2d = leaf(x2)
    x3 = r_ff(r_ln(x2d, Pb, "norm3"), sub(Pb, "ff.")) + x2d
    out = r_conv(x3.reshape(B, hw, hw, C), P["proj_out.weight"], P["proj_out.bias"]) + x_in.double()
    post = dict(x2=x2, x_in=x_in, G=G, out=out.detach(), dx2=ref_grads(out, G, (x2d,))[0])
    lin = sub(Pb, "attn2.to_q.")
    xl, Gl = rnd((B * hw * hw, C), 169), rnd((B * hw * hw, C), 170)
    frozen = dict(x=xl, G=Gl, y=xl.double() @ lin["weight"].t(), dx=Gl.double() @ lin["weight"])
    return dict(st=st, x=x, G1=G1, Gq=Gq, keep=keep, pre=pre, post=post, frozen=frozen)


def test_st_nodes(dev):
    """_STPreFn (with a key bias): a gradient on x1 only (dqin is None: the norm2 backward is skipped), on qin only (dx1 is None: norm2's backward without add), on
    both (add = dx1) -- the node's backward called directly, since the engine materialises zeros for an output without a loss -- and both again through
    Node.apply and a linear loss (the same bits); qin's gradient is 3x larger so that neither term hides in the other.  _STPostFn: dx2, and d(x_in) == G bit for bit.  _FrozenLinearFn on
    attn2.to_q: y and dx (derived: one fp16 rounding), no gradient for the frozen weight (worst 2.10e-4 / 3.06e-4).  Measured (NODE)."""
    from adaface_dev_amd import ops
    from adaface_dev_amd.ldm.modules.diffusionmodules.capture_graph import _FrozenLinearFn, _STPostFn, _STPreFn
    P = node_problem()
    B, hw, C = 2, 8, 320
    st = P["st"].to(dev)
    kb = ops.make_keybias(P["keep"].to(dev), hw * hw)
    G1, Gq = P["G1"].to(dev), P["Gq"].to(dev)
    pre = P["pre"]
    for mode in ("x1", "qin", "both", "engine"):
        def run():
            x = P["x"].to(dev).requires_grad_(True)
            x1, qin = _STPreFn.apply(st, x, kb)
            if mode == "engine":                     # a linear loss on both outputs through the autograd engine
                ((x1.float() * G1.float()).sum() + (qin.float() * Gq.float()).sum()).backward()
                return x1.detach(), qin.detach(), x.grad
            # the node's backward called directly: the engine would hand it zeros, not None, for an output without a loss
            res = x1.grad_fn.apply(None if mode == "qin" else G1, None if mode == "x1" else Gq)
            assert len(res) == 3 and res[0] is None and res[2] is None
            return x1.detach(), qin.detach(), res[1]

        tag = f"NODE pre loss={mode}"
        with launches() as names:
            x1, qin, dx = twice(tag, run)
        assert names.count("af_layernorm_bwd") == 2 * (1 if mode == "x1" else 2) and "af_attention_bwd" in names and "af_groupnorm_bwd" in names, (tag, names)
        if mode == "engine":
            assert torch.equal(dx, dx_both), "the engine and the direct call differ"
            continue
        dx_both = dx
        both(f"{tag} x1", x1, pre["x1"], NODE[0], NODE[1], B)
        both(f"{tag} qin", qin, pre["qin"], NODE[0], NODE[1], B)
        ref = {"x1": pre["d_x1"], "qin": pre["d_qin"], "both": pre["d_x1"] + pre["d_qin"]}[mode]
        both(f"{tag} dx", dx, ref, NODE[2], NODE[3], B)
    assert slabs_ok(pre["d_x1"], B) and slabs_ok(pre["d_qin"], B)
    assert 0.2 < float(pre["d_x1"].norm() / pre["d_qin"].norm()) < 5, "one term of the 'both' gradient would hide in the other"

    post = P["post"]
    G = post["G"].to(dev)

    def run_post():
        x2, x_in = post["x2"].to(dev).requires_grad_(True), post["x_in"].to(dev).requires_grad_(True)
        out = _STPostFn.apply(st, x2, x_in)
        (out.float() * G.float()).sum().backward()
        return out.detach(), x2.grad, x_in.grad

    with launches() as names:
        out, dx2, dxin = twice("post", run_post)
    assert "af_geglu_bwd" in names and "af_layernorm_bwd" in names, names
    both("NODE post out", out, post["out"], NODE[0], NODE[1], B)
    both("NODE post dx2", dx2, post["dx2"], NODE[2], NODE[3], B)
    assert dxin.dtype == torch.float16 and torch.equal(dxin, G), "d(x_in) is not G bit for bit"

    fr = P["frozen"]
    lin = st.transformer_blocks[0].attn2.to_q
    lin.weight.requires_grad_(True)
    x = fr["x"].to(dev).requires_grad_(True)
    with launches() as names:
        y = _FrozenLinearFn.apply(x, lin)
        (y.float() * fr["G"].to(dev).float()).sum().backward()
    assert set(names) == {"af_gemm"} and lin.weight.grad is None, names
    both("frozen linear y", y, fr["y"], F16_L2, F16_MAX, B)
    both("frozen linear dx", x.grad, fr["dx"], F16_L2, F16_MAX, B)


def tiny_unet(seed):
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from test_hip_unet import GPU_TINY_CONFIG
    m = UNetModel(**GPU_TINY_CONFIG)
    return m, fill(m, seed)


@functools.lru_cache(maxsize=None)
def head_problem():
    B, hw = 2, 16
    unet, P = tiny_unet(171)
    h, G = gn_input((B, hw, hw, 64), 172), rnd((B, 4, hw, hw), 173)
    hd = leaf(h)
    eps = r_conv(r_gn(hd, P["out.0.weight"], P["out.0.bias"], 1e-5, True), P["out.2.weight"], P["out.2.bias"]).permute(0, 3, 1, 2)
    return dict(unet=unet, h=h, G=G, eps=eps.detach(), dh=ref_grads(eps, G, (hd,))[0])


def test_head_and_layout_nodes(dev):
    """_HeadFn on the tiny U-Net's head (GroupNorm + SiLU + 64 -> 4 convolution) through _NHWCToNCHW(fp32, 4): the 4-wide gradient takes the F.pad arm; the
    node's backward again with a gradient that is already 8 wide (zero padded): the same bits.  _NHWCToNCHW with channels < C: forward keeps the first
    channels, backward permutes back and gives the dropped channels exactly zero.  ScaleGrad / gen_gradient_scaler at 0 (detached), 1 (the identity, the same
    tensor) and 0.5 (exact halves).  Measured (NODE): dh reads the fp16 head input; eps derived (one fp16 rounding of GroupNorm + SiLU, then of the sum:
    twice the single-rounding bound; worst on MI355X 2.75e-4 / 3.83e-4)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.capture_graph import ScaleGrad, _HeadFn, _NHWCToNCHW, gen_gradient_scaler
    P = head_problem()
    B, hw = 2, 16
    unet = P["unet"].to(dev)
    G = P["G"].to(dev)

    def run():
        h = P["h"].to(dev).requires_grad_(True)
        e = _HeadFn.apply(unet, h)
        eps = _NHWCToNCHW.apply(e, torch.float32, 4)
        assert tuple(e.shape) == (B, hw, hw, 4) and eps.is_contiguous()
        (eps * G.float()).sum().backward()
        # the node's backward on an 8-wide gradient: no pad
        e2 = _HeadFn.apply(unet, h)
        g8 = F.pad(G.permute(0, 2, 3, 1), (0, 4)).contiguous()
        return eps.detach(), h.grad, e2.grad_fn.apply(g8)[1]

    with launches() as names:
        eps, dh, dh8 = twice("head", run)
    assert "af_groupnorm_bwd" in names, names
    both("NODE head eps", eps, P["eps"], 2 * F16_L2, 2 * F16_MAX, B, torch.float32)
    both("NODE head dh", dh, P["dh"], NODE[2], NODE[3], B)
    assert torch.equal(dh, dh8), "the padded and the 8-wide gradient give different bits"

    y16 = rnd((B, 5, 6, 16), 174)
    g = rnd((B, 12, 5, 6), 175)
    for dtype in (torch.float32, torch.float16):
        y = y16.to(dev).requires_grad_(True)
        out = _NHWCToNCHW.apply(y, dtype, 12)
        assert out.dtype == dtype and tuple(out.shape) == (B, 12, 5, 6) and torch.equal(out.cpu().double(), y16.permute(0, 3, 1, 2)[:, :12].double())
        (out.float() * g.to(dev).float()).sum().backward()
        assert y.grad.dtype == torch.float16 and torch.equal(y.grad[..., :12].cpu(), g.permute(0, 2, 3, 1)) and bool((y.grad[..., 12:] == 0).all())

    t16 = rnd((3, 40), 176)
    for alpha in (0, 1, 0.5):
        t = t16.to(dev).requires_grad_(True)
        out = gen_gradient_scaler(alpha)(t)
        assert torch.equal(out, t)
        if alpha == 0:
            assert not out.requires_grad
            continue
        assert (out is t) == (alpha == 1)
        (out.float() * t16.to(dev).float()).sum().backward()
        assert torch.equal(t.grad.cpu(), (t16.float() * alpha).half())
    t = t16.to(dev).requires_grad_(True)
    ScaleGrad.apply(t, 0.0).sum().backward()
    assert bool((t.grad == 0).all())


def r_timestep_embedding(t, dim, max_period=10000.0):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    args = t.double()[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def r_unet(unet, P, x, e_all, ctx, n_tail=0, gs=1.0, head=False):
    """The U-Net walk in fp64 on x [B, H, W, 4]: the module tree gives the ORDER of the layers and their integer hyper-parameters, every number comes from P.
    e_all [B, sum Cout]: the batched emb_layers output (slices as UNetModel._assign_emb_slices lays them out).  n_tail > 0: stop in front of the last n_tail decoder
    blocks -> (h, skips in pop order).  gs: the gradient scale of the skips consumed by output blocks >= num_res_blocks + 1."""
    from adaface_dev_amd.ldm.modules.attention import SpatialTransformer
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import Downsample, ResBlock, Upsample

    def run(seq, prefix, h):
        for j, layer in enumerate(seq):
            p = sub(P, f"{prefix}.{j}.")
            if isinstance(layer, ResBlock):
                off, w = layer._emb_slice
                h = r_res(h, e_all[:, off:off + w], p)
            elif isinstance(layer, SpatialTransformer):
                h = r_st(h, ctx, p, layer.transformer_blocks[0].attn1.heads)
            elif isinstance(layer, Downsample):
                h = r_conv(h, p["op.weight"], p["op.bias"], 2)
            elif isinstance(layer, Upsample):
                h = r_conv(r_up(h), p["conv.weight"], p["conv.bias"])
            else:
                h = r_conv(h, p["weight"], p["bias"])
        return h

    hs, h = [], x
    for i, seq in enumerate(unet.input_blocks):
        h = run(seq, f"input_blocks.{i}", h)
        hs.append(h)
    h = run(unet.middle_block, "middle_block", h)
    n_out = len(unet.output_blocks)
    for oi in range(n_out - n_tail):
        skip = hs.pop()
        if gs != 1.0 and oi >= unet.num_res_blocks + 1:
            skip = skip * gs + (skip * (1.0 - gs)).detach()
        h = run(unet.output_blocks[oi], f"output_blocks.{oi}", torch.cat([h, skip], -1))
    if n_tail:
        return h, [hs.pop() for _ in range(n_tail)]
    return r_conv(r_gn(h, P["out.0.weight"], P["out.0.bias"], 1e-5, True), P["out.2.weight"], P["out.2.bias"])


TRUNK_GS = 0.5


@functools.lru_cache(maxsize=None)
def trunk_problem():
    B, hw, L = 2, 16, 77
    unet, P = tiny_unet(181)
    x, ctx = rnd((B, 4, hw, hw), 182), rnd((B, L, 64), 183)
    e_all = rnd((B, unet._emb_total), 184, 0.5)
    xd, cd = leaf(x), leaf(ctx)
    h, skips = r_unet(unet, P, xd.permute(0, 2, 3, 1), e_all.double(), cd, n_tail=3, gs=TRUNK_GS)
    outs = [h] + skips
    Gs = [rnd(tuple(o.shape), 185 + i) for i, o in enumerate(outs)]
    terms = [(o * g.double()).sum() for o, g in zip(outs, Gs)]
    full = torch.autograd.grad(sum(terms), (xd, cd), retain_graph=True)
    no1 = torch.autograd.grad(terms[0] + terms[1] + terms[3], (xd, cd), retain_graph=True)
    return dict(unet=unet, x=x, ctx=ctx, e_all=e_all, outs=[o.detach() for o in outs], Gs=Gs, full=full, no1=no1)


def test_trunk_node(dev):
    """_TrunkFn (UNetModel.hip_train_trunk / hip_bwd_trunk) on the tiny U-Net at a 16x16 latent, B = 2, n_tail = 3, res_gradscale 0.5 (so that the scaled and
    the unscaled skips differ), against fp64 autograd of r_unet; the EmbPack holds given fp16 numbers.  h and the three skips, then the node's backward, called
    directly so that None and fp32 gradients reach it as given:
      * G of order 1, G 2^10 and G 2^-20.  The rescale is 2^floor(log2(256 / max|G|)): for G and G 2^10 the scaled fp16 gradients are the SAME numbers, so
        after unscaling the results are bit-equal by construction.  For G 2^-20 the scale is clamped at 2^24 and the walk runs on gradients HALF as large:
        every fp16 operation is the same up to that factor except where a value falls below 2^-14 (subnormal: one bit fewer) one binade sooner.  Measured on
        MI355X: no such value reaches a result -- the distance is 0, the three runs are bit-equal after unscaling, and that is what is asserted.
      * one skip's gradient None: the reference drops that term.
      * x.requires_grad False: dx is None and dcontext has the same bits.
    Measured (TRUNK)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules.capture_graph import _TrunkFn
    from adaface_dev_amd.ldm.modules.diffusionmodules.openaimodel import EmbPack
    P = trunk_problem()
    B = 2
    unet = P["unet"].to(dev)
    emb = EmbPack(None, P["e_all"].to(dev))
    Gs = [g.to(dev) for g in P["Gs"]]

    def run(mult=1.0, drop=None, need_dx=True):
        x = P["x"].float().to(dev).requires_grad_(need_dx)
        ctx = P["ctx"].float().to(dev).requires_grad_(True)
        outs = _TrunkFn.apply(unet, x, emb, ctx, None, 3, TRUNK_GS)
        gin = [None if i == drop else g.float() * mult for i, g in enumerate(Gs)]
        res = outs[0].grad_fn.apply(*gin)
        assert len(res) == 7 and all(res[i] is None for i in (0, 2, 4, 5, 6))
        return [o.detach() for o in outs], res[1], res[3]

    with launches() as names:
        outs, dx, dctx = twice("trunk", run)
    assert "af_attention_bwd" in names and "af_groupnorm_bwd" in names and "af_axpy_f16" in names and "af_add_f16" in names, names
    for i, (o, ref) in enumerate(zip(outs, P["outs"])):
        both(f"TRUNK {'h' if i == 0 else f'skip{i - 1}'}", o, ref, TRUNK[0], TRUNK[1], B)
    both("TRUNK dx", dx, P["full"][0], TRUNK[2], TRUNK[3], B, torch.float32)
    both("TRUNK dcontext", dctx, P["full"][1], TRUNK[2], TRUNK[3], B, torch.float32)
    _, dx_hi, dctx_hi = run(mult=2.0 ** 10)
    assert torch.equal(dx_hi, dx * 2.0 ** 10) and torch.equal(dctx_hi, dctx * 2.0 ** 10), "G and G 2^10 walk on the same fp16 numbers"
    _, dx_lo, dctx_lo = run(mult=2.0 ** -20)
    both("TRUNK dx (G 2^-20)", dx_lo * 2.0 ** 20, P["full"][0], TRUNK[2], TRUNK[3], B, torch.float32)
    both("TRUNK dcontext (G 2^-20)", dctx_lo * 2.0 ** 20, P["full"][1], TRUNK[2], TRUNK[3], B, torch.float32)
    assert torch.equal(dx_lo * 2.0 ** 20, dx) and torch.equal(dctx_lo * 2.0 ** 20, dctx), "G 2^-20 (scale clamped at 2^24) is not bit-equal to G after unscaling"
    _, dx_n, dctx_n = run(drop=2)
    both("TRUNK dx (skip1 None)", dx_n, P["no1"][0], TRUNK[2], TRUNK[3], B, torch.float32)
    both("TRUNK dcontext (skip1 None)", dctx_n, P["no1"][1], TRUNK[2], TRUNK[3], B, torch.float32)
    _, dx_0, dctx_0 = run(need_dx=False)
    assert dx_0 is None and torch.equal(dctx_0, dctx)


@functools.lru_cache(maxsize=None)
def unet_problem():
    B, hw, L = 2, 16, 77
    unet, P = tiny_unet(191)
    x, ctx, t = rnd((B, hw, hw, 4), 192), rnd((B, L, 64), 193), torch.tensor([17, 801])
    semb = F.silu(F.linear(F.silu(F.linear(r_timestep_embedding(t, 64), P["time_embed.0.weight"], P["time_embed.0.bias"])), P["time_embed.2.weight"],
                           P["time_embed.2.bias"]))
    e_all = torch.zeros((B, unet._emb_total), dtype=torch.float64)
    for n, rb in unet.named_modules():
        if hasattr(rb, "_emb_slice") and rb._emb_slice is not None:
            off, w = rb._emb_slice
            e_all[:, off:off + w] = F.linear(semb, P[n + ".emb_layers.1.weight"], P[n + ".emb_layers.1.bias"])
    xd, cd = leaf(x), leaf(ctx)
    eps = r_unet(unet, P, xd, e_all, cd)
    G = rnd(tuple(eps.shape), 194)
    dx, dctx = ref_grads(eps, G, (xd, cd))
    return dict(unet=unet, x=x, ctx=ctx, t=t, G=G, eps=eps.detach(), dx=dx, dctx=dctx)


def test_unet_pair(dev):
    """UNetModel.hip_train / hip_bwd on the tiny U-Net (16x16 latent, B = 2, timesteps 17 and 801) against r_unet with the time embedding restated in fp64: eps, dx
    (4 channels back from the 8-wide input) and dcontext, per item.  Measured (UNET): ~25 blocks of fp16 intermediates both ways, heads of 8 / 16 / 32 channels -- eps 1.70e-3 / 1.87e-3, dx 2.50e-3 / 2.71e-3, dcontext
    2.89e-3 / 4.74e-3 (the sum of 16 cross-attention layers' k | v gradients; its largest error sits on one entry): inside the ceilings, with no room for the factor two."""
    P = unet_problem()
    B = 2
    unet = P["unet"].to(dev)
    x, ctx, t = F.pad(P["x"], (0, 4)).to(dev), P["ctx"].to(dev), P["t"].to(dev)
    G8 = F.pad(P["G"], (0, 4)).to(dev)

    def run():
        eps, saved = unet.hip_train(x, t, ctx)
        return eps, unet.hip_bwd(saved, G8)

    with launches() as names:
        eps, (dx, dctx) = twice("unet", run)
    assert "af_attention_bwd" in names and "af_groupnorm_bwd" in names, names
    both("UNET eps", eps, P["eps"], UNET[0], UNET[1], B)
    both("UNET dx", dx, P["dx"], UNET[2], UNET[3], B)
    both("UNET dcontext", dctx, P["dctx"], UNET[2], UNET[3], B)


# ======================================================================================================= 9. VAE decoder pairs
def r_vae_res(x, P):
    h = r_conv(r_gn(x, P["norm1.weight"], P["norm1.bias"], 1e-6, True), P["conv1.weight"], P["conv1.bias"])
    h = r_conv(r_gn(h, P["norm2.weight"], P["norm2.bias"], 1e-6, True), P["conv2.weight"], P["conv2.bias"])
    return h + (r_conv(x, P["nin_shortcut.weight"], P["nin_shortcut.bias"]) if "nin_shortcut.weight" in P else x)


def r_vae_attn(x, P):
    B, H, W, C = x.shape
    hn = r_gn(x, P["norm.weight"], P["norm.bias"], 1e-6, False)
    q, k, v = (r_conv(hn, P[n + ".weight"], P[n + ".bias"]).reshape(B, H * W, C) for n in ("q", "k", "v"))
    o = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1) @ v
    return r_conv(o.reshape(B, H, W, C), P["proj_out.weight"], P["proj_out.bias"]) + x


VAE_CASES = {"res_identity": ("res", 128, 128, 16, 16), "res_nin": ("res", 256, 128, 16, 16), "attn_128": ("attn", 128, 128, 8, 16),
             "attn_512": ("attn", 512, 512, 16, 16), "upsample": ("up", 128, 128, 8, 8)}


@functools.lru_cache(maxsize=None)
def vae_problem(name):
    from adaface_dev_amd.ldm.modules.diffusionmodules import model as vae
    kind, cin, cout, H, W = VAE_CASES[name]
    if kind == "up":
        return updown_problem("vae_up", cin, H, W)
    m = vae.ResnetBlock(in_channels=cin, out_channels=cout, temb_channels=0) if kind == "res" else vae.AttnBlock(cin)
    P = fill(m, 201)
    x = gn_input((2, H, W, cin), 202)
    xd = leaf(x)
    y = r_vae_res(xd, P) if kind == "res" else r_vae_attn(xd, P)
    G = rnd(tuple(y.shape), 203)
    return dict(m=m, x=x, G=G, y=y.detach(), dx=ref_grads(y, G, (xd,))[0])


@pytest.mark.parametrize("name", list(VAE_CASES))
def test_vae_pairs(dev, name):
    """model.py's ResnetBlock (identity and nin_shortcut), AttnBlock -- at N = 8 x 16 = 128 tokens of 128 channels, the smallest the training form takes
    (vae_attention_path(train=True) == "gemm" asserted, af_softmax_rows_bwd seen), and at 256 tokens of 512 channels; hip_train refuses a mask -- and Upsample
    (nine-tap gather, dgrad + 2x2 sums), B = 2, against fp64.  Measured (VAE); Upsample derived as in test_updown_pairs (worst y 2.08e-4 / 4.08e-4, dx 2.98e-4 / 4.48e-4)."""
    from adaface_dev_amd.ldm.modules.diffusionmodules import model as vae
    kind, cin, cout, H, W = VAE_CASES[name]
    P = vae_problem(name)
    m = P["m"].to(dev)
    x, G = P["x"].to(dev), P["G"].to(dev)

    def run():
        y, saved = m.hip_train(x)
        return y, m.hip_bwd(saved, G)

    with launches() as names:
        y, dx = twice(name, run)
    if kind == "attn":
        assert vae.vae_attention_path(H * W, cin, train=True) == "gemm" and "af_softmax_rows_bwd" in names and "af_groupnorm_bwd" in names, names
        with pytest.raises(NotImplementedError):
            m.hip_train(x, mask={"fg_mask": torch.ones((2, 1, H, W), device=dev)})
    elif kind == "res":
        assert names.count("af_groupnorm_bwd") == 4, names
    else:
        assert "af_sumpool2x2" in names and "af_gemm(conv3x3_up2)" not in names, names
    b = (2 * F16_L2, 2 * F16_MAX) if kind == "up" else VAE[2:]
    both(f"VAE {name} y", y, P["y"], *((F16_L2, F16_MAX) if kind == "up" else VAE[:2]), 2)
    both(f"VAE {name} dx", dx, P["dx"], b[0], b[1], 2)


@functools.lru_cache(maxsize=None)
def decoder_problem():
    from adaface_dev_amd.ldm.modules.diffusionmodules import model as vae
    dec = vae.Decoder(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[], in_channels=3, resolution=32, z_channels=4)
    P = fill(dec, 211)
    z = rnd((2, 8, 16, 4), 212)
    zd = leaf(z)
    h = r_conv(zd, P["conv_in.weight"], P["conv_in.bias"])
    h = r_vae_res(h, sub(P, "mid.block_1."))
    h = r_vae_attn(h, sub(P, "mid.attn_1."))
    h = r_vae_res(h, sub(P, "mid.block_2."))
    for lvl in (1, 0):
        for i in range(2):
            h = r_vae_res(h, sub(P, f"up.{lvl}.block.{i}."))
        if lvl:
            h = r_conv(r_up(h), P["up.1.upsample.conv.weight"], P["up.1.upsample.conv.bias"])
    y = r_conv(r_gn(h, P["norm_out.weight"], P["norm_out.bias"], 1e-6, True), P["conv_out.weight"], P["conv_out.bias"])
    G = rnd(tuple(y.shape), 213)
    return dict(dec=dec, z=z, G=G, y=y.detach(), dz=ref_grads(y, G, (zd,))[0])


def test_vae_decoder_pair(dev):
    """Decoder.hip_train / hip_bwd on a two-level decoder (ch 64, ch_mult (1, 2), one ResnetBlock per level + 1, z [2, 8, 16, 4 -> 8]): conv_in, mid block
    (ResnetBlock, AttnBlock at 128 tokens, ResnetBlock), two levels with one Upsample, norm_out, conv_out (3 -> 8 padded channels, the pad exactly zero)
    against fp64.  Measured (VAE)."""
    P = decoder_problem()
    dec = P["dec"].to(dev)
    z, G8 = F.pad(P["z"], (0, 4)).to(dev), F.pad(P["G"], (0, 5)).to(dev)

    def run():
        y, saved = dec.hip_train(z)
        return y, dec.hip_bwd(saved, G8)

    with launches() as names:
        y, dz = twice("decoder", run)
    assert "af_softmax_rows_bwd" in names and "af_sumpool2x2" in names and "af_groupnorm_bwd" in names, names
    assert tuple(y.shape) == (2, 16, 32, 8) and tuple(dz.shape) == (2, 8, 16, 8)
    assert bool((y[..., 3:] == 0).all()) and bool((dz[..., 4:] == 0).all())
    both("VAE decoder y", y[..., :3], P["y"], VAE[0], VAE[1], 2)
    both("VAE decoder dz", dz[..., :4], P["dz"], VAE[2], VAE[3], 2)
