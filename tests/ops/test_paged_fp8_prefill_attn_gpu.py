"""fp8 paged prefill attention kernel (csrc/paged_fp8_prefill_attention.hip)
against the fp64 paged reference on the same bytes and scales.

Shapes, cases, layouts and the bound check are those of the bf16 prefill and
the fp8 decode tests (imported).  The fp8 ``_build`` poisons everything beyond
the live rows with K byte 0x7E, V byte 0xFE and scale 1e30: a result within
the bound shows that no byte AND no scale beyond the last visible key leaks.

Bound |out - ref| <= 2^-7*|ref| + 2^-7*vmax, vmax the largest dequantised live
|v|: the derivation of tests/ops/test_paged_fp8_attn_gpu.py at CAP = 320 —
dequantisation to bf16 is exact, the scale multiplies are single fp32
roundings, and the bf16 rounding of weight * v_scale adds <= 2^-9 * max|v|
like the bf16 P of the twin.

Randn rows all have nearly the same amax, so a scale read from the wrong row,
head or tensor would pass: logical V row j of kv head hk is multiplied by
2^((j + hk) % 3) and K row j by 2^((j + hk + 1) % 3) / 2 before quantising.
"""
import functools

import pytest
import torch

from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_fp8_kernel_supported, paged_gather_dequant, paged_prefill_attention,
    paged_prefill_attention_reference)
from tests.ops.test_paged_attn_gpu import (B, CAP, H, SHAPES, _check,
                                           _pos_tensor, _slopes)
from tests.ops.test_paged_fp8_attn_gpu import _build, _vmax
from tests.ops.test_paged_prefill_attn_gpu import (_cases, _edge_cases, _last,
                                                   _qkv)

pytestmark = pytest.mark.gpu


def _ext():
    return get_extension(required=True)


@functools.lru_cache(maxsize=None)
def _inputs(D, Hkv):
    """The bf16 test's q, k, v with the row factors of the module docstring
    (powers of two: exact in bf16).  Shared, never modified."""
    q, k, v = _qkv(D, Hkv)
    e = torch.arange(CAP, device="cuda")[None, :] \
        + torch.arange(Hkv, device="cuda")[:, None]            # [Hkv, CAP]
    fk = (2.0 ** ((e + 1) % 3) / 2)[None, :, :, None]
    fv = (2.0 ** (e % 3))[None, :, :, None]
    return q, (k.float() * fk).bfloat16(), (v.float() * fv).bfloat16()


def _ref(q, cache, slopes, scale, start):
    kp, vp, ks, vs, table = cache
    return paged_prefill_attention_reference(
        q.double(), kp, vp, table, slopes.double(), scale, start, ks, vs)


def _run(q, cache, slopes, scale, start):
    kp, vp, ks, vs, table = cache
    return _ext().paged_prefill_attn_fp8(q, kp, vp, ks, vs, table, slopes,
                                         scale, start)


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_random_inputs(D, Hkv, PAGE):
    q_all, k_log, v_log = _inputs(D, Hkv)
    scale = D ** -0.5
    for start, Sq in _cases(PAGE):
        q, last = q_all[:, :, :Sq], _last(start, Sq)
        cache = _build(k_log, v_log, PAGE, last)
        st = _pos_tensor(start * B if len(start) == 1 else start)
        vmax = _vmax(cache[1], cache[3], cache[4], last)
        for kind in ("alibi", "zero"):
            slopes = _slopes(kind)
            out = _run(q, cache, slopes, scale, st)
            assert out.dtype == torch.bfloat16 and out.shape == q.shape
            assert out.transpose(1, 2).is_contiguous()
            _check(out, _ref(q, cache, slopes, scale, st), vmax,
                   f"{kind} start={start} Sq={Sq}")


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_causal_edge_at_tile_and_page_boundaries(D, Hkv, PAGE):
    """The one-hot-K construction of the bf16 test: all query rows are q0, K
    is zero (amax == 0: scale 0, bytes 0) except row j*, so a row that sees
    j* returns the dequantised v[j*] and the row before it does not."""
    q_all, _, v_log = _inputs(D, Hkv)
    G, scale = H // Hkv, D ** -0.5
    q0 = q_all[:, ::G, 0].float()                              # [B, Hkv, D]
    krow = ((30 + 0.25 * CAP) * q0
            / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    q_same = q_all[:, :, :1].expand(-1, -1, q_all.size(2), -1).contiguous()
    for start, Sq, js in _edge_cases(PAGE):
        q = q_same[:, :, :Sq]
        k_log = torch.zeros_like(v_log)
        k_log[:, :, js] = krow
        last = _last([start], Sq)
        cache = _build(k_log, v_log, PAGE, last)
        st = _pos_tensor([start])
        vmax = _vmax(cache[1], cache[3], cache[4], last)
        target = paged_gather_dequant(cache[1], cache[3], cache[4], CAP,
                                      torch.float64)[:, :, js]  # [B, Hkv, D]
        for kind in ("alibi", "zero"):
            slopes = _slopes(kind)
            what = f"{kind} start={start} Sq={Sq} j*={js}"
            ref = _ref(q, cache, slopes, scale, st)
            _check(_run(q, cache, slopes, scale, st), ref, vmax, what)
            # on the reference alone: the construction does what it says
            first = max(js - start, 0)          # first row with p_i >= j*
            bound = 2.0 ** -7 * target.abs() + 2.0 ** -7 * vmax
            seen = ref[:, ::G, first:]                   # [B, Hkv, rows, D]
            assert ((seen - target[:, :, None]).abs()
                    <= bound[:, :, None]).all(), what
            if first > 0:
                before = ref[:, ::G, first - 1]
                assert ((before - target).abs() > 4 * bound).any(), what


def test_rows_past_capacity_are_zero():
    D, Hkv, PAGE = 64, 2, 16
    q_all, k_log, v_log = _inputs(D, Hkv)
    Sq = 5
    q, slopes, scale = q_all[:, :, :Sq], _slopes("alibi"), D ** -0.5
    cache = _build(k_log, v_log, PAGE, [CAP - 1] * B)
    st = _pos_tensor([CAP - 2])
    out = _run(q, cache, slopes, scale, st)
    assert torch.isfinite(out).all() and (out[:, :, 2:] == 0).all()
    _check(out[:, :, :2], _ref(q, cache, slopes, scale, st)[:, :, :2],
           _vmax(cache[1], cache[3], cache[4], [CAP - 1] * B),
           "rows below capacity")
    # a start wholly outside the cache, either side: zeros, nothing read
    for far in (CAP, CAP + 1000, -Sq, -(1 << 40), 1 << 40):
        out = _run(q, cache, slopes, scale, _pos_tensor([far]))
        assert (out == 0).all(), far


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_write_then_prefill(D, Hkv, PAGE):
    """One captured write + prefill replays at the start in the tensor at
    replay time, across the first tile edge, bit for bit as the eager calls
    and within the fp64 bound."""
    ext = _ext()
    s1, s2, Sq = 40, 62, 5
    q_all, k_log, v_log = _inputs(D, Hkv)
    q, slopes, scale = q_all[:, :, :Sq], _slopes("alibi"), D ** -0.5
    last = _last([s2], Sq)
    cache = _build(k_log, v_log, PAGE, last)
    kp, vp, ks, vs, table = cache
    new = torch.randn(B, Hkv, Sq, D, device="cuda").bfloat16()
    st = _pos_tensor([s1])

    def step():
        ext.paged_kv_write_fp8(new, new, kp, vp, ks, vs, table, st)
        return _run(q, cache, slopes, scale, st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    st.fill_(s2)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, step())
    _check(out, _ref(q, cache, slopes, scale, st),
           _vmax(vp, vs, table, last), "replay at start 62")


def test_host_checks_and_dispatch(monkeypatch):
    D, Hkv, PAGE = 64, 2, 16
    q_all, k_log, v_log = _inputs(D, Hkv)
    start, Sq = [30], 20
    q, slopes, scale = q_all[:, :, :Sq], _slopes("alibi"), D ** -0.5
    cache = _build(k_log, v_log, PAGE, _last(start, Sq))
    kp, vp, ks, vs, table = cache
    st = _pos_tensor(start)
    call = lambda q=q, kp=kp, ks=ks, vs=vs, table=table: \
        _run(q, (kp, vp, ks, vs, table), slopes, scale, st)
    with pytest.raises(RuntimeError, match="k_pool must be float8_e4m3fn"):
        call(kp=kp.view(torch.uint8).bfloat16())
    with pytest.raises(RuntimeError, match="v_scale must be fp32"):
        call(vs=vs.double())
    with pytest.raises(RuntimeError, match="k_scale has sizes"):
        call(ks=ks[:, :, :8].contiguous())
    with pytest.raises(RuntimeError, match="int32 GPU tensor"):
        call(table=table.cpu())
    with pytest.raises(RuntimeError, match="Sq >= 1"):
        call(q=q[:, :, :0])

    ext, calls = _ext(), []
    real = ext.paged_prefill_attn_fp8
    monkeypatch.setattr(ext, "paged_prefill_attn_fp8",
                        lambda *a: calls.append(1) or real(*a))
    assert paged_fp8_kernel_supported(q, kp)
    on = paged_prefill_attention(q, kp, vp, table, slopes, scale, st, ks, vs)
    assert len(calls) == 1
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    off = paged_prefill_attention(q, kp, vp, table, slopes, scale, st, ks, vs)
    assert len(calls) == 1, "PG_DECODE_ATTN=0 must not launch"
    ref = _ref(q, cache, slopes, scale, st)
    vmax = _vmax(vp, vs, table, _last(start, Sq))
    _check(on, ref, vmax, "dispatched kernel")
    _check(off, ref, vmax, "reference path")
