"""The routing of a transformer block (attention.block_plan and its parts xattn_route / ff_route / ln_fold), pinned on the CPU against a literal table.

Every expected value below was computed at the commit BEFORE the plan existed, from that commit's own predicates (CrossAttention.xattn_fusable,
FeedForward.ff_fusable, BasicTransformerBlock.post_done and the branch conditions of BasicTransformerBlock.hip / hip_train and of the motion module), on
the CPU; none comes from the functions under test.  A routing default or threshold that moves fails here in milliseconds; the launch counts of the full
U-Net stay pinned on the GPU in test_hip_bench_shape.py."""
import pytest

from adaface_dev_amd.ldm.modules import attention as A

# (switches set for the row, (C, B, N, L), attn1 captures, attn2 captures, a folded proj_out pack is on offer,
#  (LayerNorm kernels, xattn, ff with proj_out offered, ff without)); LayerNorm kernels: none, norm1 + norm2 (norm3 stays folded) or all three; L = 77
# context tokens, None = no context
BLOCK = [
    # default switches
    ({}, (320, 8, 4096, 77), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({}, (320, 6, 4096, 77), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({}, (320, 2, 4096, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({}, (320, 1, 4096, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 2, 4096, 81), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 2, 4032, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 256, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (640, 8, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 1, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 1, 512, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (1280, 8, 256, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (1280, 2, 256, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    # attn1 captures
    ({}, (320, 8, 4096, 77), True, False, True, ('none', 'fused', 'chain', 'fused')),
    ({}, (320, 6, 4096, 77), True, False, True, ('none', 'fused', 'chain', 'fused')),
    ({}, (320, 2, 4096, 77), True, False, True, ('none', 'fused', 'fold', 'split')),
    ({}, (320, 1, 4096, 77), True, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 2, 4096, 81), True, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 2, 4032, 77), True, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 256, 77), True, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (640, 8, 1024, 77), True, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 1, 1024, 77), True, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 1, 512, 77), True, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (1280, 8, 256, 77), True, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (1280, 8, 64, 77), True, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (1280, 2, 256, 77), True, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (96, 2, 1024, 77), True, False, True, ('all', 'split', 'split', 'split')),
    # attn2 captures
    ({}, (320, 8, 4096, 77), False, True, True, ('none', 'split', 'chain', 'fused')),
    ({}, (320, 6, 4096, 77), False, True, True, ('none', 'split', 'chain', 'fused')),
    ({}, (320, 2, 4096, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 4096, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 2, 4096, 81), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 2, 4032, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 256, 77), False, True, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (640, 8, 1024, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 1, 1024, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 1, 512, 77), False, True, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (1280, 8, 256, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (1280, 8, 64, 77), False, True, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (1280, 2, 256, 77), False, True, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (96, 2, 1024, 77), False, True, True, ('all', 'split', 'split', 'split')),
    # both capture
    ({}, (320, 8, 4096, 77), True, True, True, ('none', 'split', 'chain', 'fused')),
    ({}, (320, 2, 4096, 77), True, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (640, 8, 1024, 77), True, True, True, ('none', 'split', 'fold', 'split')),
    ({}, (1280, 8, 64, 77), True, True, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (96, 2, 1024, 77), True, True, True, ('all', 'split', 'split', 'split')),
    # one switch flipped at a time
    ({'FOLD_LAYERNORM': False}, (320, 8, 4096, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FOLD_LAYERNORM': False}, (320, 2, 4096, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FOLD_LAYERNORM': False}, (640, 8, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FOLD_LAYERNORM': False}, (1280, 8, 64, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FOLD_LAYERNORM': False}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FUSE_XATTN': False}, (320, 8, 4096, 77), False, False, True, ('none', 'split', 'chain', 'fused')),
    ({'FUSE_XATTN': False}, (320, 2, 4096, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({'FUSE_XATTN': False}, (640, 8, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({'FUSE_XATTN': False}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'FUSE_XATTN': False}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'CHAIN_XATTN': False}, (320, 8, 4096, 77), False, False, True, ('none', 'fused', 'chain', 'fused')),
    ({'CHAIN_XATTN': False}, (320, 2, 4096, 77), False, False, True, ('none', 'fused', 'fold', 'split')),
    ({'CHAIN_XATTN': False}, (640, 8, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({'CHAIN_XATTN': False}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'CHAIN_XATTN': False}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FUSE_FF': False}, (320, 8, 4096, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({'FUSE_FF': False}, (320, 2, 4096, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({'FUSE_FF': False}, (640, 8, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({'FUSE_FF': False}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'FUSE_FF': False}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'CHAIN_PROJ_OUT': False}, (320, 8, 4096, 77), False, False, True, ('none', 'chain', 'fused', 'fused')),
    ({'CHAIN_PROJ_OUT': False}, (320, 2, 4096, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({'CHAIN_PROJ_OUT': False}, (640, 8, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({'CHAIN_PROJ_OUT': False}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'CHAIN_PROJ_OUT': False}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FOLD_PROJ_OUT': False}, (320, 8, 4096, 77), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({'FOLD_PROJ_OUT': False}, (320, 2, 4096, 77), False, False, True, ('none', 'chain', 'split', 'split')),
    ({'FOLD_PROJ_OUT': False}, (640, 8, 1024, 77), False, False, True, ('none', 'split', 'split', 'split')),
    ({'FOLD_PROJ_OUT': False}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'split', 'split')),
    ({'FOLD_PROJ_OUT': False}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FUSE_XATTN640': True}, (320, 8, 4096, 77), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({'FUSE_XATTN640': True}, (320, 2, 4096, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({'FUSE_XATTN640': True}, (640, 8, 1024, 77), False, False, True, ('none', 'fused', 'fold', 'split')),
    ({'FUSE_XATTN640': True}, (1280, 8, 64, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'FUSE_XATTN640': True}, (96, 2, 1024, 77), False, False, True, ('all', 'split', 'split', 'split')),
    ({'FUSE_XATTN640': True}, (640, 1, 512, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    # the C = 640 one-launch arm under capture, and with its token threshold lowered below LN_FOLD_MIN_ROWS
    ({'FUSE_XATTN640': True}, (640, 8, 1024, 77), True, False, True, ('none', 'fused', 'fold', 'split')),
    ({'FUSE_XATTN640': True}, (640, 8, 1024, 77), False, True, True, ('none', 'split', 'fold', 'split')),
    ({'FUSE_XATTN640': True, 'XATTN640_FUSE_MIN_TOKENS': 64}, (640, 1, 512, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'FUSE_XATTN640': True, 'XATTN640_FUSE_MIN_TOKENS': 64}, (640, 1, 1024, 77), False, False, True, ('none', 'fused', 'fold', 'split')),
    ({'FUSE_XATTN640': True}, (640, 4, 1000, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    # no folded proj_out pack on offer
    ({}, (320, 8, 4096, 77), False, False, False, ('none', 'chain', 'chain', 'fused')),
    ({}, (320, 2, 4096, 77), False, False, False, ('none', 'chain', 'split', 'split')),
    ({}, (640, 8, 1024, 77), False, False, False, ('none', 'split', 'split', 'split')),
    ({}, (1280, 8, 64, 77), False, False, False, ('norm12', 'split', 'split', 'split')),
    ({}, (96, 2, 1024, 77), False, False, False, ('all', 'split', 'split', 'split')),
    # both sides of each threshold
    ({}, (640, 1, 1023, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (640, 1, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 1023, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({}, (320, 1, 1024, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 8191, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 63, 128, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 64, 128, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({}, (320, 1, 8192, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({}, (320, 1, 24575, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 1, 24576, 77), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({}, (320, 191, 128, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({}, (320, 192, 128, 77), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({}, (320, 2, 4096, 80), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({}, (320, 2, 4096, 81), False, False, True, ('none', 'split', 'fold', 'split')),
    ({}, (320, 8, 4096, 80), False, False, True, ('none', 'chain', 'chain', 'fused')),
    ({}, (320, 8, 4096, 81), False, False, True, ('none', 'split', 'chain', 'fused')),
    ({}, (320, 8, 4096, None), False, False, True, ('none', 'split', 'chain', 'fused')),
    ({}, (640, 8, 1024, None), False, False, True, ('none', 'split', 'fold', 'split')),
    # the token threshold moved
    ({'XATTN_FUSE_MIN_TOKENS': 8193}, (320, 2, 4096, 77), False, False, True, ('none', 'split', 'fold', 'split')),
    ({'XATTN_FUSE_MIN_TOKENS': 1024}, (320, 8, 128, 77), False, False, True, ('none', 'chain', 'fold', 'split')),
    ({'XATTN_FUSE_MIN_TOKENS': 256}, (320, 2, 128, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
    ({'XATTN_FUSE_MIN_TOKENS': 1024}, (320, 7, 128, 77), False, False, True, ('norm12', 'split', 'fold', 'split')),
]

# (switches, (C, B, N, L), LayerNorm folded into to_q, the layer captures, one launch, chainable)
XATTN_ALONE = [
    ({}, (320, 2, 4096, 77), True, False, True, True),
    ({}, (320, 2, 4096, 77), False, False, False, False),
    ({}, (320, 2, 4096, 77), True, True, False, False),
    ({}, (320, 1, 4096, 77), True, False, False, False),
    ({}, (320, 2, 4096, 81), True, False, False, False),
    ({}, (640, 8, 1024, 77), True, False, False, False),
    ({'FUSE_XATTN640': True}, (640, 8, 1024, 77), True, False, True, False),
    ({'FUSE_XATTN640': True}, (640, 8, 1000, 77), True, False, False, False),
    ({'FUSE_XATTN640': True, 'XATTN640_FUSE_MIN_TOKENS': 64}, (640, 2, 256, 77), True, False, True, False),
    ({'FUSE_XATTN640': True, 'XATTN640_FUSE_MIN_TOKENS': 64}, (640, 3, 64, 77), True, False, True, False),
    ({'FUSE_XATTN640': True, 'XATTN640_FUSE_MIN_TOKENS': 64}, (640, 1, 32, 77), True, False, False, False),
    ({'FUSE_XATTN': False}, (320, 2, 4096, 77), True, False, False, False),
    ({'XATTN_FUSE_MIN_TOKENS': 256}, (320, 2, 128, 77), True, False, True, True),
    ({}, (1280, 8, 256, 77), True, False, False, False),
]
# (switches, C, rows, LayerNorm folded in, one launch)
FF_ALONE = [
    ({}, 320, 24576, True, True),
    ({}, 320, 24575, True, False),
    ({}, 320, 24576, False, False),
    ({}, 640, 24576, True, False),
    ({'FUSE_FF': False}, 320, 24576, True, False),
]
# (FOLD_LAYERNORM, C, rows, folded into a q | k | v projection of that many rows, folded into the GEGLU projection)
LN_FOLD = [
    (True, 320, 1024, True, True),
    (True, 320, 1023, False, True),
    (True, 96, 2048, False, False),
    (True, 1280, 64, False, True),
    (True, 640, 4096, True, True),
    (False, 320, 1024, False, False),
    (False, 320, 1023, False, False),
    (False, 96, 2048, False, False),
    (False, 1280, 64, False, False),
    (False, 640, 4096, False, False),
]

LN_KERNELS = {"none": (False, False), "norm12": (True, False), "all": (True, True)}
SWITCH_DEFAULTS = dict(FOLD_LAYERNORM=True, FUSE_GN_PROJ=True, CHAIN_XATTN=True, XATTN_FUSE_MIN_TOKENS=8192, CHAIN_PROJ_OUT=True, FOLD_PROJ_OUT=True,
                       FUSE_XATTN640=False, XATTN640_FUSE_MIN_TOKENS=4096, FUSE_XATTN=True, FUSE_FF=True, FF_FUSE_MIN_ROWS=24576, LN_FOLD_MIN_ROWS=1024)


@pytest.fixture
def switches(monkeypatch):
    """Sets the module's switches to their defaults (whatever AF_* the environment holds), then a row's own on top."""
    def set_(row_switches):
        for k, v in {**SWITCH_DEFAULTS, **row_switches}.items():
            assert hasattr(A, k), k
            monkeypatch.setattr(A, k, v)
    return set_


def test_switch_defaults(monkeypatch):
    """With no AF_* variable set, the module's switches are the defaults the table was computed under."""
    import importlib.util
    import os
    for k in list(os.environ):
        if k.startswith("AF_"):
            monkeypatch.delenv(k)
    spec = importlib.util.find_spec(A.__name__)
    fresh = importlib.util.module_from_spec(spec)           # a second copy of the module: the imported one keeps its state
    spec.loader.exec_module(fresh)
    assert {k: getattr(fresh, k) for k in SWITCH_DEFAULTS} == SWITCH_DEFAULTS


def test_block_plan_table(switches):
    assert len(BLOCK) > 100
    for sw, (C, B, N, L), cap1, cap2, can_fold, (ln, xattn, ff_with, ff_without) in BLOCK:
        switches(sw)
        for want, ff in ((True, ff_with), (False, ff_without)):
            p = A.block_plan(C, B, N, L, 8, C, capture1=cap1, capture2=cap2, want_proj_out=want, can_fold_proj_out=can_fold)
            row = (sw, (C, B, N, L), cap1, cap2, can_fold, want)
            assert ((p.ln12, p.ln3), p.xattn, p.ff) == (LN_KERNELS[ln], xattn, ff), row
            # invariants
            assert p.proj_out == (p.ff in ("chain", "fold")) and (want or not p.proj_out), row
            assert p.xattn in ("chain", "fused", "split") and p.ff in ("chain", "fused", "fold", "split"), row
            if p.xattn == "chain":
                assert A.FOLD_LAYERNORM and not p.ln12 and not cap1 and not cap2 and C == 320, row
            if p.xattn != "split":
                assert not p.ln12 and not cap2 and L is not None, row
            if p.ff != "split":
                assert not p.ln3, row


def test_block_plan_other_heads(switches):
    """The one-launch cross-attention kernels are 8-head, inner_dim = C kernels."""
    switches({})
    assert A.block_plan(320, 8, 4096, 77, 8, 320).xattn == "chain"
    assert A.block_plan(320, 8, 4096, 77, 4, 320).xattn == "split"
    assert A.block_plan(320, 8, 4096, 77, 8, 512).xattn == "split"


def test_layers_alone(switches):
    """CrossAttention.hip / FeedForward.hip called on their own decide with the same functions: a key mask forces the three launches, an offered chain is
    taken at C = 320 only, and no proj_out is ever inside."""
    for sw, (C, B, N, L), folded, cap, fused, chainable in XATTN_ALONE:
        switches(sw)
        assert A.xattn_route(C, B, N, L, 8, C, folded, cap) == ("fused" if fused else "split"), (sw, C, B, N, L, folded, cap)
        assert A.xattn_route(C, B, N, L, 8, C, folded, cap, chain=True) == ("chain" if chainable else "fused" if fused else "split"), (sw, C, B, N, L)
        assert A.xattn_route(C, B, N, L, 8, C, folded, cap, masked=True, chain=True) == "split"
    for sw, C, M, folded, fused in FF_ALONE:
        switches(sw)
        assert A.ff_route(C, M, folded) == ("fused" if fused else "split"), (sw, C, M, folded)


def test_fold_rule_of_training_and_motion(switches):
    """The training pass and the temporal attention fold a LayerNorm from 1024 rows up only (all three norms or none); the feed-forward's at every size."""
    for fold, C, M, with_rows, without_rows in LN_FOLD:
        switches({"FOLD_LAYERNORM": fold})
        assert (A.ln_fold(C, M), A.ln_fold(C)) == (with_rows, without_rows), (fold, C, M)
