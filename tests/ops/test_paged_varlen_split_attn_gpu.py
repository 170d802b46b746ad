"""Split-KV ragged-batch paged attention (csrc/paged_varlen_split_attention.hip)
against the fp64 reference of the ragged kernel.  Pools and tables are those
of tests/ops/test_paged_attn_gpu.py: shuffled pages, K = +1e30 / V = -1e30 in
every slot past each sequence's last visible key.

Tolerance |out - ref| <= 2^-7*|ref| + 2^-7*max|v|, the project's
(tests/ops/test_decode_attn_gpu.py has the derivation).  It holds unchanged:
the partials are fp32 and unnormalised, so merging them (the four waves of a
short tile, then the splits) adds at most 4 + n_splits <= 12 fp32 roundings
to an fp32 accumulation over <= 320 terms and no bf16 rounding; P and the
output are rounded to bf16 exactly once, as in the unsplit kernel.
"""
import functools

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (paged_kernel_supported,
                                               paged_varlen_attention)
from tests.ops.test_paged_attn_gpu import (B, CAP, H, SHAPES, _build, _check,
                                           _layout, _slopes)
from tests.ops.test_paged_varlen_attn_gpu import _dev, _last, _q, _qkv, _ref

pytestmark = pytest.mark.gpu

# 3 does not divide the 5 key tiles, 5 gives one tile per split, 8 dead splits
SPLITS = (0, 1, 2, 3, 5, 8)
# (lens, starts, padding rows): decode rows at both ends of the cache and at
# the chunk edges; a decode row with a ragged piece; a piece whose first rows
# lie below a later split's start and whose last rows reach into it, with an
# empty sequence on either side; padding; a start outside the cache
CASES = [([1, 1], [0, CAP - 1], 0), ([1, 1], [63, 64], 0),
         ([1, 1], [128, 64], 0), ([1, 37], [300, 100], 0),
         ([70, 0], [60, 7], 0), ([0, 70], [7, 60], 0), ([1, 5], [200, 3], 7),
         ([5, 3], [CAP - 2, CAP + 1000], 0), ([5, 3], [CAP - 2, -3], 0),
         ([1, 3], [-(1 << 40), 1 << 40], 0)]


def _attn(*args, **kw):
    return get_extension(required=True).paged_varlen_split_attn(*args, **kw)


@functools.lru_cache(maxsize=None)
def _case(D, Hkv, PAGE, ci, kind):
    """Operands and fp64 reference of one case: built once, shared by every
    n_splits, never modified."""
    lens, starts, pad = CASES[ci]
    q_wide, k_log, v_log = _qkv(D, Hkv)
    args = (_q(q_wide, sum(lens) + pad),
            *_build(k_log, v_log, PAGE, _last(lens, starts)), _slopes(kind),
            D ** -0.5, *_dev(lens, starts))
    return args, _ref(*args), v_log.double().abs().max().item()


@pytest.mark.parametrize("n_splits", SPLITS)
@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_random_inputs(D, Hkv, PAGE, n_splits):
    for ci, (lens, starts, _) in enumerate(CASES):
        for kind in ("alibi", "zero"):
            args, ref, vmax = _case(D, Hkv, PAGE, ci, kind)
            out = _attn(*args, n_splits)
            assert out.dtype == torch.bfloat16 and out.is_contiguous()
            _check(out, ref, vmax, f"{kind} lens={lens} at {starts}")
            zero = (ref == 0).all(-1).all(-1)
            assert zero[sum(lens):].all() and (out[zero] == 0).all()
            if not 0 <= starts[1] < CAP:
                assert zero[lens[0]:].all(), "rows outside the cache"
            assert torch.equal(out, _attn(*args, n_splits)), "not deterministic"
            # the body that serves every tile from the shared staged tile
            _check(_attn(*args, n_splits, short_body=False), ref, vmax,
                   f"shared-tile body, {kind} lens={lens} at {starts}")


@pytest.mark.parametrize("n_splits", (0, 3))
@pytest.mark.parametrize("heads,Hkv", [(16, 2), (16, 1), (6, 2)])
def test_group_sizes(heads, Hkv, n_splits):
    """A decode row and a 19-token piece: G = 8 packs two tokens in wave 0's
    rows, G = 16 makes one token fill them exactly, G = 3 does not share a
    tile and runs one head per workgroup."""
    D, PAGE, lens, starts = 64, 16, [1, 19], [200, 50]
    q_wide, k_log, v_log = _qkv(D, Hkv, heads)
    args = (_q(q_wide, sum(lens)),
            *_build(k_log, v_log, PAGE, _last(lens, starts)),
            alibi_slopes(heads).to("cuda", torch.float32), D ** -0.5,
            *_dev(lens, starts))
    _check(_attn(*args, n_splits), _ref(*args),
           v_log.double().abs().max().item(), f"G={heads // Hkv}")


def test_poisoned_workspace():
    """The workspace is torch.empty: freed NaN blocks of exactly its tensors'
    sizes (and a larger one) are what the caching allocator hands back.  Dead
    splits and rows below a split's start leave their acc unwritten, and the
    combine must select them away, never weigh them with 0."""
    D, Hkv, PAGE, n_splits = 64, 2, 16, 8
    args, ref, vmax = _case(D, Hkv, PAGE, 3, "alibi")
    ext = get_extension(required=True)
    n_slot = ext.paged_varlen_split_plan(args[0].size(0), B, H, Hkv, CAP)[1]
    rows = n_slot * n_splits * Hkv * 64
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    poison = [nan(rows, D), nan(rows, 2), nan(rows, D), nan(rows, 2),
              nan(4 * rows, D)]
    torch.cuda.synchronize()
    del poison
    out = _attn(*args, n_splits)
    _check(out, ref, vmax, "poisoned workspace")


@pytest.mark.parametrize("n_splits", (0, 2))
@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_reads_everything_on_device(D, Hkv, PAGE, n_splits):
    """A captured call replays with the cu_q, start, table and pools that are
    in the tensors at replay time: sequence 0 goes from a decode row (a short
    tile) to a 9-row piece and its start across the first chunk edge, each
    sequence's second page moves."""
    lens1, starts1, lens2, starts2 = [1, 7], [60, 3], [9, 2], [62, 100]
    q_wide, k_log, v_log = _qkv(D, Hkv)
    q = _q(q_wide, 12)                  # the replay's last row is padding
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, _last(lens1, starts1))
    cu, st = _dev(lens1, starts1)
    args = (q, k_pool, v_pool, table, _slopes("alibi"), D ** -0.5, cu, st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _attn(*args, n_splits)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _attn(*args, n_splits)

    assign, spare, _ = _layout(PAGE)
    moved = assign.clone()
    moved[:, 1] = torch.tensor(spare[1:1 + B])
    k2, v2, table2 = _build(k_log, v_log, PAGE, _last(lens2, starts2),
                            assign=moved)
    cu2, st2 = _dev(lens2, starts2)
    cu.copy_(cu2), st.copy_(st2)                # all in place
    k_pool.copy_(k2), v_pool.copy_(v2), table.copy_(table2)
    eager = _attn(*args[:6], cu2, st2, n_splits)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    _check(out, _ref(*args), v_log.double().abs().max().item(), "replay")


def test_dispatch_and_host_checks(monkeypatch):
    args, ref, vmax = _case(64, 2, 16, 3, "alibi")
    ext = get_extension(required=True)
    calls = []
    for name in ("paged_varlen_attn", "paged_varlen_split_attn"):
        real = getattr(ext, name)
        monkeypatch.setattr(
            ext, name,
            lambda *a, _n=name, _f=real: calls.append(_n) or _f(*a))
    paged_varlen_attention(*args)
    paged_varlen_attention(*args, n_splits=None)
    assert calls == ["paged_varlen_attn"] * 2
    _check(paged_varlen_attention(*args, n_splits=0), ref, vmax, "dispatched")
    assert calls[2:] == ["paged_varlen_split_attn"]
    for bad in (-1, 65):
        with pytest.raises(RuntimeError, match="n_splits"):
            _attn(*args, bad)
        with pytest.raises(ValueError, match="n_splits"):
            paged_varlen_attention(*args, n_splits=bad)
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    assert not paged_kernel_supported(args[0][None], args[1])
    del calls[:]
    off = paged_varlen_attention(*args, n_splits=0)
    assert not calls, "PG_DECODE_ATTN=0 must not launch"
    assert torch.isfinite(off).all()
