"""Ragged-batch paged attention kernel (csrc/paged_varlen_attention.hip)
against the fp64 reference, which is the paged prefill reference applied per
sequence.  Pools and tables are those of tests/ops/test_paged_attn_gpu.py:
shuffled pages, K = +1e30 / V = -1e30 in every slot past each sequence's last
visible key.  Tolerance |out - ref| <= 2^-7*|ref| + 2^-7*max|v|: the
derivation of tests/ops/test_decode_attn_gpu.py covers this kernel unchanged
(the same bf16 P and output rounding, fp32 accumulation over <= 320 terms).
"""
import functools

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_kernel_supported, paged_varlen_attention,
    paged_varlen_attention_reference)
from tests.ops.test_paged_attn_gpu import (B, CAP, H, SHAPES, _build, _check,
                                           _layout, _slopes)

pytestmark = pytest.mark.gpu

T_MAX = 200
# (lens, starts, padding rows, strided q): single rows at both ends of the
# cache, an empty sequence on either side, one row more than a tile of gp = 4,
# 2 and 1, several ragged tiles, an end at capacity, padding, a strided q
CASES = [([1, 1], [0, CAP - 1], 0, False), ([0, 5], [7, 3], 0, False),
         ([5, 0], [3, 7], 0, False), ([16, 17], [0, 0], 0, False),
         ([32, 33], [0, 0], 0, False), ([64, 65], [0, 0], 0, False),
         ([130, 37], [17, 100], 0, False), ([70, 3], [CAP - 70, 200], 0, False),
         ([1, 100], [300, 0], 0, False), ([33, 20], [5, 60], 7, False),
         ([40, 9], [10, 250], 0, True)]
# rows past capacity, and a start wholly outside the cache on either side
CASES += [([5, 3], [CAP - 2, far], 0, False)
          for far in (CAP, CAP + 1000, -3, -(1 << 40), 1 << 40)]


def _attn(*args):
    return get_extension(required=True).paged_varlen_attn(*args)


@functools.lru_cache(maxsize=None)
def _qkv(D, Hkv, heads=H):
    """One set of random logical inputs per shape, shared, never modified; q
    is a view of a wider buffer for the strided case."""
    g = torch.Generator(device="cuda").manual_seed(5000 + D + 7 * Hkv + heads)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    return mk(T_MAX, heads, D + 8), mk(B, Hkv, CAP, D), mk(B, Hkv, CAP, D)


def _q(q_wide, T, strided=False):
    q = q_wide[:T, :, 8:]
    return q if strided else q.contiguous()


def _dev(lens, starts):
    """cu_q and start on the device."""
    return (torch.tensor([0, lens[0], sum(lens)], device="cuda",
                         dtype=torch.int32),
            torch.tensor(starts, device="cuda", dtype=torch.long))


def _last(lens, starts):
    """Last visible key per sequence (key 0 for an empty one)."""
    return [min(max(s + n - 1, 0), CAP - 1) for n, s in zip(lens, starts)]


def _ref(q, k_pool, v_pool, table, slopes, scale, cu, st):
    return paged_varlen_attention_reference(
        q.double(), k_pool.double(), v_pool.double(), table, slopes.double(),
        scale, cu, st)


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_random_inputs(D, Hkv, PAGE):
    q_wide, k_log, v_log = _qkv(D, Hkv)
    vmax = v_log.double().abs().max().item()
    for lens, starts, pad, strided in CASES:
        q = _q(q_wide, sum(lens) + pad, strided)
        assert q.is_contiguous() != strided
        pools = _build(k_log, v_log, PAGE, _last(lens, starts))
        for kind in ("alibi", "zero"):
            args = (q, *pools, _slopes(kind), D ** -0.5, *_dev(lens, starts))
            out = _attn(*args)
            assert out.dtype == torch.bfloat16 and out.is_contiguous()
            ref = _ref(*args)
            _check(out, ref, vmax, f"{kind} lens={lens} at {starts}")
            # padding and out-of-range rows: zero in the reference, and
            # EXACTLY zero from the kernel
            zero = (ref == 0).all(-1).all(-1)
            assert zero[sum(lens):].all() and (out[zero] == 0).all()
            if starts[1] >= CAP or starts[1] <= -3:
                assert zero[2:].all(), "rows outside the cache"
            assert torch.equal(out, _attn(*args)), "not deterministic"


@pytest.mark.parametrize("heads,Hkv", [(16, 2), (16, 1), (6, 2)])
def test_group_sizes(heads, Hkv):
    """G = 8 and 16 share a tile (a wave holds 2 tokens, 1 token); G = 3
    does not divide the tile and runs one head per workgroup."""
    D, PAGE, lens, starts = 64, 16, [19, 6], [50, 0]
    q_wide, k_log, v_log = _qkv(D, Hkv, heads)
    args = (_q(q_wide, sum(lens)),
            *_build(k_log, v_log, PAGE, _last(lens, starts)),
            alibi_slopes(heads).to("cuda", torch.float32), D ** -0.5,
            *_dev(lens, starts))
    _check(_attn(*args), _ref(*args), v_log.double().abs().max().item(),
           f"G={heads // Hkv}")


def _edge_cases(PAGE):
    """Two sequences of different lengths in one call; j* at a token boundary
    inside a GQA-packed tile, at the M-tile edges of gp = 4, 2 and 1 (tokens
    16, 32, 64), at key-tile and page edges and at both sequences' ends."""
    for lens, starts in (([65, 8], [0, 60]), ([PAGE + 2, 130], [PAGE - 1, 17])):
        last = _last(lens, starts)
        s0, s1 = starts
        for js in sorted({j for j in (0, s0, s0 + 1, s0 + 15, s0 + 16, s0 + 31,
                                      s0 + 32, 63, 64, 127, 128, PAGE - 1,
                                      PAGE, 2 * PAGE - 1, 2 * PAGE, s1,
                                      s1 + 1, s1 + 63, s1 + 64, *last)
                          if j <= max(last)}):
            yield lens, starts, last, js


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_causal_edge_at_token_tile_and_page_boundaries(D, Hkv, PAGE):
    """The construction of tests/ops/test_paged_prefill_attn_gpu.py: one
    query vector; K zero except row j*, aligned with it so strongly that a
    row which sees j* returns v[j*] and the row at j*-1 does not."""
    q_wide, _, v_log = _qkv(D, Hkv)
    G = H // Hkv
    scale = D ** -0.5
    gain = 30 + 0.25 * CAP
    vmax = v_log.double().abs().max().item()
    q_same = q_wide[:1, :, 8:].expand(T_MAX, H, D).contiguous()
    q0 = q_same[0, ::G].float()                                # [Hkv, D]
    krow = (gain * q0 / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    for lens, starts, last, js in _edge_cases(PAGE):
        k_log = torch.zeros_like(v_log)
        k_log[:, :, js] = krow
        pools = _build(k_log, v_log, PAGE, last)
        for kind in ("alibi", "zero"):
            what = f"{kind} lens={lens} starts={starts} j*={js}"
            args = (q_same[:sum(lens)], *pools, _slopes(kind), scale,
                    *_dev(lens, starts))
            ref = _ref(*args)
            _check(_attn(*args), ref, vmax, what)
            # on the reference alone: the construction does what it says
            for b, c0 in enumerate((0, lens[0])):
                if js > last[b]:
                    continue                    # sequence b never sees j*
                target = v_log[b, :, js].double()              # [Hkv, D]
                first = max(js - starts[b], 0)  # first row with p >= j*
                bound = 2.0 ** -7 * target.abs() + 2.0 ** -7 * vmax
                seen = ref[c0 + first:c0 + lens[b], ::G]       # [rows, Hkv, D]
                assert ((seen - target).abs() <= bound).all(), what
                if first > 0:
                    before = ref[c0 + first - 1, ::G]
                    assert ((before - target).abs() > 4 * bound).any(), what


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_reads_everything_on_device(D, Hkv, PAGE):
    """A captured call replays with the cu_q, start, table and pools that are
    in the tensors at replay time, at fixed T: the row split moves, a start
    crosses the first key-tile edge, each sequence's second page moves."""
    lens1, starts1, lens2, starts2 = [5, 7], [60, 3], [9, 2], [62, 100]
    q_wide, k_log, v_log = _qkv(D, Hkv)
    q = _q(q_wide, 12)                  # the replay's last row is padding
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, _last(lens1, starts1))
    cu, st = _dev(lens1, starts1)
    args = (q, k_pool, v_pool, table, _slopes("alibi"), D ** -0.5, cu, st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _attn(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _attn(*args)

    assign, spare, _ = _layout(PAGE)
    moved = assign.clone()
    moved[:, 1] = torch.tensor(spare[1:1 + B])
    k2, v2, table2 = _build(k_log, v_log, PAGE, _last(lens2, starts2),
                            assign=moved)
    assert (table2[:, 1] != table[:, 1]).all()
    cu2, st2 = _dev(lens2, starts2)
    cu.copy_(cu2), st.copy_(st2)                # all in place
    k_pool.copy_(k2), v_pool.copy_(v2), table.copy_(table2)
    eager = _attn(*args[:6], cu2, st2)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    _check(out, _ref(*args), v_log.double().abs().max().item(), "replay")


def test_host_checks():
    D, Hkv, PAGE = 64, 2, 16
    q_wide, k_log, v_log = _qkv(D, Hkv)
    q = _q(q_wide, 8)
    kp, vp, table = _build(k_log, v_log, PAGE, [9] * B)
    slopes = _slopes("alibi")
    cu, st = _dev([5, 3], [5, 2])
    good = dict(q=q, kp=kp, vp=vp, table=table, slopes=slopes, cu=cu, st=st)
    narrow = lambda t: t[..., :32].contiguous()
    for match, change in [
            ("bf16", dict(q=q.float())), ("bf16", dict(vp=vp.half())),
            ("GPU", dict(kp=kp.cpu())), ("GPU", dict(slopes=slopes.cpu())),
            ("page size", dict(kp=kp[:, :, :8], vp=vp[:, :, :8])),
            ("64 or 128", dict(q=narrow(q), kp=narrow(kp), vp=narrow(vp))),
            ("multiple of kv heads",
             dict(q=q[:, :3].contiguous(), slopes=slopes[:3].contiguous())),
            ("cu_q", dict(cu=cu.long())), ("cu_q", dict(cu=cu.cpu())),
            ("block_table must be", dict(cu=cu[:2].contiguous())),
            ("at most 1024 sequences",
             dict(cu=torch.zeros(1026, device="cuda", dtype=torch.int32)))]:
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match=match):
            _attn(a["q"], a["kp"], a["vp"], a["table"], a["slopes"], 0.125,
                  a["cu"], a["st"])


def test_opt_out_and_dispatch(monkeypatch):
    D, Hkv, PAGE, lens, starts = 64, 2, 16, [20, 7], [30, 0]
    q_wide, k_log, v_log = _qkv(D, Hkv)
    args = (_q(q_wide, sum(lens)),
            *_build(k_log, v_log, PAGE, _last(lens, starts)),
            _slopes("alibi"), D ** -0.5, *_dev(lens, starts))
    ext = get_extension(required=True)
    calls = []
    real = ext.paged_varlen_attn
    monkeypatch.setattr(ext, "paged_varlen_attn",
                        lambda *a: calls.append("varlen") or real(*a))
    on = paged_varlen_attention(*args)
    assert calls == ["varlen"]
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    assert not paged_kernel_supported(args[0][None], args[1])
    off = paged_varlen_attention(*args)
    assert calls == ["varlen"], "PG_DECODE_ATTN=0 must not launch"
    assert off.shape == on.shape and torch.isfinite(off).all()
    _check(on, _ref(*args), v_log.double().abs().max().item(), "dispatched")
