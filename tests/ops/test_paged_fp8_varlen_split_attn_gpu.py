"""fp8 split-KV ragged-batch paged attention
(csrc/paged_fp8_varlen_split_attention.hip) against the fp64 varlen reference
on the same bytes and scales.

Cases and plans are those of the bf16 split test, inputs (with the per-row
power-of-two factors, so a scale read from the wrong row, head or tensor
fails) those of the fp8 varlen test, pools those of the fp8 decode test:
everything beyond the live rows is K byte 0x7E, V byte 0xFE and scale 1e30, so
a result within the bound shows that no byte and no scale past the last
visible key leaks, through any split.

Bound |out - ref| <= 2^-7*|ref| + 2^-7*vmax, vmax the largest dequantised live
|v|; no new number.  The fp8 derivation of
tests/ops/test_paged_fp8_prefill_attn_gpu.py holds for each partial: same CAP
= 320, fp8 -> bf16 exact, the K scale one fp32 multiply on the score, the V
scale applied to the fp32 weight BEFORE its single bf16 rounding into P, in
both bodies alike (the short body converts K in registers instead of through
LDS, which rounds nothing).  The split test's argument holds for the merges:
partials are fp32 and unnormalised, so the four waves of a short tile and the
splits add at most 4 + n_splits <= 12 fp32 roundings and no bf16 rounding; the
output is rounded to bf16 once.
"""
import functools

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_fp8_kernel_supported, paged_varlen_attention,
    paged_varlen_attention_reference)
from tests.ops.test_paged_attn_gpu import B, CAP, H, SHAPES, _check, _slopes
from tests.ops.test_paged_fp8_attn_gpu import _build, _vmax
from tests.ops.test_paged_fp8_varlen_attn_gpu import _inputs
from tests.ops.test_paged_varlen_attn_gpu import _dev, _last, _q
from tests.ops.test_paged_varlen_split_attn_gpu import CASES, SPLITS

pytestmark = pytest.mark.gpu


def _attn(*args, **kw):
    return get_extension(required=True).paged_varlen_split_attn_fp8(*args, **kw)


def _operands(D, Hkv, PAGE, lens, starts, pad, slopes, heads=H):
    """(args, fp64 reference, vmax) of one packed batch."""
    q_wide, k_log, v_log = _inputs(D, Hkv, heads)
    last = _last(lens, starts)
    kp, vp, ks, vs, table = _build(k_log, v_log, PAGE, last)
    args = (_q(q_wide, sum(lens) + pad), kp, vp, ks, vs, table, slopes,
            D ** -0.5, *_dev(lens, starts))
    return args, _ref(*args), _vmax(vp, vs, table, last)


def _ref(q, kp, vp, ks, vs, table, slopes, scale, cu, st):
    return paged_varlen_attention_reference(
        q.double(), kp, vp, table, slopes.double(), scale, cu, st, ks, vs)


@functools.lru_cache(maxsize=None)
def _case(D, Hkv, PAGE, ci, kind):
    """Built once, shared by every n_splits, never modified."""
    return _operands(D, Hkv, PAGE, *CASES[ci], _slopes(kind))


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
            _check(_attn(*args, n_splits, short_body=False), ref, vmax,
                   f"shared-tile body, {kind} lens={lens} at {starts}")


@pytest.mark.parametrize("n_splits", (0, 3))
@pytest.mark.parametrize("heads,Hkv", [(16, 2), (16, 1), (6, 2)])
def test_group_sizes(heads, Hkv, n_splits):
    """A decode row and a 19-token piece at G = 8, 16 and 3 (one head per
    workgroup), as in the bf16 split test."""
    args, ref, vmax = _operands(
        64, Hkv, 16, [1, 19], [200, 50], 0,
        alibi_slopes(heads).to("cuda", torch.float32), heads)
    _check(_attn(*args, n_splits), ref, vmax, f"G={heads // Hkv}")


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
    _check(_attn(*args, n_splits), ref, vmax, "poisoned workspace")


@pytest.mark.parametrize("n_splits", (0, 2))
@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture(D, Hkv, PAGE, n_splits):
    """A captured call replays with the cu_q, start, table, pools and scales
    that are in the tensors at replay time: sequence 0 goes from a decode row
    (a short tile) to a 9-row piece and its start across the first chunk
    edge, and every page moves to another pool slot."""
    lens2, starts2 = [9, 2], [62, 100]
    slopes = _slopes("alibi")
    args, _, _ = _operands(D, Hkv, PAGE, [1, 7], [60, 3], 4, slopes)
    new, _, vmax = _operands(D, Hkv, PAGE, lens2, starts2, 1, slopes)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _attn(*args, n_splits)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _attn(*args, n_splits)

    # pool slot i of the replay holds what slot perm[i] held in `new`
    perm = torch.randperm(new[1].size(0), device="cuda",
                          generator=torch.Generator("cuda").manual_seed(PAGE))
    for dst, src in zip(args[1:3], new[1:3]):           # all in place
        dst.view(torch.uint8).copy_(src.view(torch.uint8)[perm])
    for dst, src in zip(args[3:5], new[3:5]):
        dst.copy_(src[perm])
    args[5].copy_(torch.argsort(perm)[new[5].long()])
    args[8].copy_(new[8]), args[9].copy_(new[9])
    eager = _attn(*args, n_splits)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    _check(out, _ref(*args), vmax, "replay")


def test_dispatch(monkeypatch):
    args, ref, vmax = _case(64, 2, 16, 3, "alibi")
    q, kp, vp, ks, vs, table, slopes, scale, cu, st = args
    call = lambda **kw: paged_varlen_attention(
        q, kp, vp, table, slopes, scale, cu, st, ks, vs, **kw)
    ext = get_extension(required=True)
    direct = ext.paged_varlen_attn_fp8(*args)
    calls = []
    for name in ("paged_varlen_attn_fp8", "paged_varlen_split_attn_fp8"):
        real = getattr(ext, name)
        monkeypatch.setattr(
            ext, name,
            lambda *a, _n=name, _f=real: calls.append(_n) or _f(*a))
    assert paged_fp8_kernel_supported(q[None], kp)
    _check(call(n_splits=0), ref, vmax, "dispatched")
    assert calls == ["paged_varlen_split_attn_fp8"]
    assert torch.equal(call(n_splits=None), direct) \
        and torch.equal(call(), direct)
    assert calls[1:] == ["paged_varlen_attn_fp8"] * 2
    for bad in (-1, 65):
        with pytest.raises(RuntimeError, match="n_splits"):
            _attn(*args, bad)
        with pytest.raises(ValueError, match="n_splits"):
            call(n_splits=bad)
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    del calls[:]
    _check(call(n_splits=0), ref, vmax, "reference path")
    assert not calls, "PG_DECODE_ATTN=0 must not launch"
