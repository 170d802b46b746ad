"""fp8 ragged-batch paged attention kernel
(csrc/paged_fp8_varlen_attention.hip) against the fp64 varlen reference on
the same bytes and scales.

Shapes, cases, layouts and the bound check are those of the bf16 varlen and
the fp8 tests (imported).  The fp8 ``_build`` poisons everything beyond the
live rows with K byte 0x7E, V byte 0xFE and scale 1e30: a result within the
bound shows that no byte AND no scale beyond the last visible key leaks.

Bound |out - ref| <= 2^-7*|ref| + 2^-7*vmax, vmax the largest dequantised live
|v|: the derivation of tests/ops/test_paged_fp8_prefill_attn_gpu.py carries
over unchanged (same CAP = 320, same conversions and roundings).

A scale read from the wrong row, head or tensor must fail: logical V row j of
kv head hk is multiplied by 2^((j + hk) % 3) and K row j by
2^((j + hk + 1) % 3) / 2 before quantising, as in that test.
"""
import functools

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_fp8_kernel_supported, paged_gather_dequant, paged_varlen_attention,
    paged_varlen_attention_reference)
from tests.ops.test_paged_attn_gpu import CAP, H, SHAPES, _check, _slopes
from tests.ops.test_paged_fp8_attn_gpu import _build, _vmax
from tests.ops.test_paged_varlen_attn_gpu import (CASES, T_MAX, _dev,
                                                  _edge_cases, _last, _q, _qkv)

pytestmark = pytest.mark.gpu


def _ext():
    return get_extension(required=True)


@functools.lru_cache(maxsize=None)
def _inputs(D, Hkv, heads=H):
    """The bf16 varlen test's q, k, v with the row factors of the module
    docstring (powers of two: exact in bf16).  Shared, never modified."""
    q_wide, k, v = _qkv(D, Hkv, heads)
    e = torch.arange(CAP, device="cuda")[None, :] \
        + torch.arange(Hkv, device="cuda")[:, None]            # [Hkv, CAP]
    fk = (2.0 ** ((e + 1) % 3) / 2)[None, :, :, None]
    fv = (2.0 ** (e % 3))[None, :, :, None]
    return q_wide, (k.float() * fk).bfloat16(), (v.float() * fv).bfloat16()


def _ref(q, cache, slopes, scale, cu, st):
    kp, vp, ks, vs, table = cache
    return paged_varlen_attention_reference(
        q.double(), kp, vp, table, slopes.double(), scale, cu, st, ks, vs)


def _run(q, cache, slopes, scale, cu, st):
    kp, vp, ks, vs, table = cache
    return _ext().paged_varlen_attn_fp8(q, kp, vp, ks, vs, table, slopes,
                                        scale, cu, st)


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_random_inputs(D, Hkv, PAGE):
    q_wide, k_log, v_log = _inputs(D, Hkv)
    for lens, starts, pad, strided in CASES:
        q, last = _q(q_wide, sum(lens) + pad, strided), _last(lens, starts)
        cache = _build(k_log, v_log, PAGE, last)
        vmax = _vmax(cache[1], cache[3], cache[4], last)
        for kind in ("alibi", "zero"):
            args = (q, cache, _slopes(kind), D ** -0.5, *_dev(lens, starts))
            out = _run(*args)
            assert out.dtype == torch.bfloat16 and out.is_contiguous()
            ref = _ref(*args)
            _check(out, ref, vmax, f"{kind} lens={lens} at {starts}")
            # padding and out-of-range rows: zero in the reference, and
            # EXACTLY zero from the kernel
            zero = (ref == 0).all(-1).all(-1)
            assert zero[sum(lens):].all() and (out[zero] == 0).all()
            if starts[1] >= CAP or starts[1] <= -3:
                assert zero[2:].all(), "rows outside the cache"
            assert torch.equal(out, _run(*args)), "not deterministic"


@pytest.mark.parametrize("heads,Hkv", [(16, 2), (16, 1), (6, 2)])
def test_group_sizes(heads, Hkv):
    """G = 8 and 16 share a tile, G = 3 runs one head per workgroup."""
    D, PAGE, lens, starts = 64, 16, [19, 6], [50, 0]
    q_wide, k_log, v_log = _inputs(D, Hkv, heads)
    last = _last(lens, starts)
    cache = _build(k_log, v_log, PAGE, last)
    args = (_q(q_wide, sum(lens)), cache,
            alibi_slopes(heads).to("cuda", torch.float32), D ** -0.5,
            *_dev(lens, starts))
    _check(_run(*args), _ref(*args),
           _vmax(cache[1], cache[3], cache[4], last), f"G={heads // Hkv}")


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_causal_edge_at_token_tile_and_page_boundaries(D, Hkv, PAGE):
    """The one-hot-K construction of the bf16 varlen test: all query rows are
    q0, K is zero (amax == 0: scale 0, bytes 0) except row j*, so a row that
    sees j* returns the dequantised v[j*] and the row at j*-1 does not."""
    q_wide, _, v_log = _inputs(D, Hkv)
    G, scale = H // Hkv, D ** -0.5
    q_same = q_wide[:1, :, 8:].expand(T_MAX, H, D).contiguous()
    q0 = q_same[0, ::G].float()                                # [Hkv, D]
    krow = ((30 + 0.25 * CAP) * q0
            / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    for lens, starts, last, js in _edge_cases(PAGE):
        k_log = torch.zeros_like(v_log)
        k_log[:, :, js] = krow
        cache = _build(k_log, v_log, PAGE, last)
        vmax = _vmax(cache[1], cache[3], cache[4], last)
        vg = paged_gather_dequant(cache[1], cache[3], cache[4], CAP,
                                  torch.float64)               # [B, Hkv, CAP, D]
        for kind in ("alibi", "zero"):
            what = f"{kind} lens={lens} starts={starts} j*={js}"
            args = (q_same[:sum(lens)], cache, _slopes(kind), scale,
                    *_dev(lens, starts))
            ref = _ref(*args)
            _check(_run(*args), ref, vmax, what)
            # on the reference alone: the construction does what it says
            for b, c0 in enumerate((0, lens[0])):
                if js > last[b]:
                    continue                    # sequence b never sees j*
                target = vg[b, :, js]                          # [Hkv, D]
                first = max(js - starts[b], 0)  # first row with p >= j*
                bound = 2.0 ** -7 * target.abs() + 2.0 ** -7 * vmax
                seen = ref[c0 + first:c0 + lens[b], ::G]       # [rows, Hkv, D]
                assert ((seen - target).abs() <= bound).all(), what
                if first > 0:
                    before = ref[c0 + first - 1, ::G]
                    assert ((before - target).abs() > 4 * bound).any(), what


def _tok(lens, starts, table, T):
    """The per-token view of the packed rows: position and table row of every
    token; padding rows sit at CAP, where the write drops them."""
    seq = [b for b, n in enumerate(lens) for _ in range(n)]
    pos = [s + i for n, s in zip(lens, starts) for i in range(n)]
    pad = T - len(seq)
    return (torch.tensor(pos + [CAP] * pad, device="cuda", dtype=torch.long),
            table[torch.tensor(seq + [0] * pad, device="cuda")].contiguous())


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_write_then_varlen(D, Hkv, PAGE):
    """One captured per-token write + varlen call replays with the cu_q, start
    and token positions that are in the tensors at replay time, at fixed T:
    the row split moves and sequence 0 crosses the first key-tile edge.  Bit
    for bit as the eager calls and within the fp64 bound."""
    ext = _ext()
    lens1, starts1, lens2, starts2, T = [5, 7], [60, 3], [9, 2], [62, 100], 12
    q_wide, k_log, v_log = _inputs(D, Hkv)
    q, slopes, scale = _q(q_wide, T), _slopes("alibi"), D ** -0.5
    last = _last(lens2, starts2)        # >= the first round's last rows
    cache = _build(k_log, v_log, PAGE, last)
    kp, vp, ks, vs, table = cache
    new = torch.randn(T, Hkv, 1, D, device="cuda").bfloat16()
    cu, st = _dev(lens1, starts1)
    tok_pos, tok_table = _tok(lens1, starts1, table, T)

    def step():
        ext.paged_kv_write_fp8(new, new, kp, vp, ks, vs, tok_table, tok_pos)
        return _run(q, cache, slopes, scale, cu, st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for dst, src in zip((cu, st, tok_pos, tok_table),
                        (*_dev(lens2, starts2),
                         *_tok(lens2, starts2, table, T))):
        dst.copy_(src)                  # all in place
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, step())
    assert (out[sum(lens2):] == 0).all()
    _check(out, _ref(q, cache, slopes, scale, cu, st),
           _vmax(vp, vs, table, last), "replay across key 64")


def test_dispatch_and_opt_out(monkeypatch):
    D, Hkv, PAGE, lens, starts = 64, 2, 16, [20, 7], [30, 0]
    q_wide, k_log, v_log = _inputs(D, Hkv)
    last = _last(lens, starts)
    cache = _build(k_log, v_log, PAGE, last)
    kp, vp, ks, vs, table = cache
    q, slopes, scale = _q(q_wide, sum(lens)), _slopes("alibi"), D ** -0.5
    cu, st = _dev(lens, starts)
    direct = _run(q, cache, slopes, scale, cu, st)

    ext, calls = _ext(), []
    real = ext.paged_varlen_attn_fp8
    monkeypatch.setattr(ext, "paged_varlen_attn_fp8",
                        lambda *a: calls.append(1) or real(*a))
    assert paged_fp8_kernel_supported(q[None], kp)
    on = paged_varlen_attention(q, kp, vp, table, slopes, scale, cu, st, ks,
                                vs)
    assert len(calls) == 1 and torch.equal(on, direct)
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    off = paged_varlen_attention(q, kp, vp, table, slopes, scale, cu, st, ks,
                                 vs)
    assert len(calls) == 1, "PG_DECODE_ATTN=0 must not launch"
    ref, vmax = _ref(q, cache, slopes, scale, cu, st), _vmax(vp, vs, table, last)
    _check(on, ref, vmax, "dispatched kernel")
    _check(off, ref, vmax, "reference path")
