"""Paged prefill attention kernel (csrc/paged_prefill_attention.hip) against
the fp64 paged reference.

Pools and tables are those of tests/ops/test_paged_attn_gpu.py (its
construction is reused): shuffled, interleaved, non-monotone pages; page 0,
every spare table entry and every slot past the last query position
``start + Sq - 1`` hold K = +1e30 / V = -1e30.  A finite result within the
bound shows that nothing beyond the last visible key leaks.

Tolerance |out - ref| <= 2^-7*|ref| + 2^-7*max|v|: the derivation of
tests/ops/test_decode_attn_gpu.py covers this kernel as it stands — bf16
output rounding <= 2^-9|out|, bf16 P adds <= 2^-9 max|v|, fp32 accumulation
over <= CAP = 320 terms, 4x margin.
"""
import functools

import pytest
import torch

from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_kernel_supported, paged_prefill_attention,
    paged_prefill_attention_reference)
from tests.ops.test_paged_attn_gpu import (B, CAP, H, SHAPES, _build, _check,
                                           _layout, _pos_tensor, _slopes)

pytestmark = pytest.mark.gpu

SQ_MAX = 130


def _ext():
    return get_extension(required=True)


def _cases(PAGE):
    """(start per row, Sq): one key, a ragged block, exactly one block, one
    row more, a chunk straddling the first tile edge, a block-aligned chunk,
    a chunk straddling a page edge, three query blocks with a ragged tail of
    2, a chunk that ends at capacity, the last slot, per-row starts."""
    return [([0], 1), ([0], 5), ([0], 64), ([0], 65), ([63], 2), ([64], 64),
            ([PAGE - 1], PAGE + 2), ([17], 130), ([CAP - 70], 70),
            ([CAP - 1], 1), ([100, 3], 37)]


@functools.lru_cache(maxsize=None)
def _qkv(D, Hkv):
    """One set of random logical inputs per shape, shared, never modified."""
    g = torch.Generator(device="cuda").manual_seed(4000 + D + 7 * Hkv)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    return mk(B, H, SQ_MAX, D), mk(B, Hkv, CAP, D), mk(B, Hkv, CAP, D)


def _last(start, Sq):
    """Last visible key per batch row."""
    return [min(s + Sq - 1, CAP - 1) for s in (start * B)[:B]]


def _ref(q, k_pool, v_pool, table, slopes, scale, start):
    return paged_prefill_attention_reference(
        q.double(), k_pool.double(), v_pool.double(), table, slopes.double(),
        scale, start)


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_random_inputs(D, Hkv, PAGE):
    ext = _ext()
    q_all, k_log, v_log = _qkv(D, Hkv)
    scale = D ** -0.5
    vmax = v_log.double().abs().max().item()
    for start, Sq in _cases(PAGE):
        q = q_all[:, :, :Sq]
        k_pool, v_pool, table = _build(k_log, v_log, PAGE, _last(start, Sq))
        st = _pos_tensor(start * B if len(start) == 1 else start)
        for kind in ("alibi", "zero"):
            slopes = _slopes(kind)
            out = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes,
                                         scale, st)
            assert out.dtype == torch.bfloat16 and out.shape == q.shape
            assert out.transpose(1, 2).is_contiguous()
            ref = _ref(q, k_pool, v_pool, table, slopes, scale, st)
            _check(out, ref, vmax, f"{kind} start={start} Sq={Sq}")


def _edge_cases(PAGE):
    for start, Sq in ((0, 65), (60, 8), (PAGE - 1, PAGE + 2), (17, 130)):
        last = start + Sq - 1
        for js in sorted({j for j in (0, start, start + 1, last, 63, 64, 127,
                                      128, PAGE - 1, PAGE, 2 * PAGE - 1,
                                      2 * PAGE) if j <= last}):
            yield start, Sq, js


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_causal_edge_at_tile_and_page_boundaries(D, Hkv, PAGE):
    """All query rows are one vector q0; K is zero except row j*, aligned
    with q0 so strongly that a row which sees j* returns v[j*].  The row at
    position j*-1 must NOT: an off-by-one at the causal edge, a tile or a
    page boundary moves it by far more than the bound, where among 300
    random keys it could hide."""
    ext = _ext()
    q_all, _, v_log = _qkv(D, Hkv)
    G = H // Hkv
    scale = D ** -0.5
    gain = 30 + 0.25 * CAP
    vmax = v_log.double().abs().max().item()
    q0 = q_all[:, ::G, 0].float()                              # [B, Hkv, D]
    krow = (gain * q0 / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    q_same = q_all[:, :, :1].expand(B, H, SQ_MAX, D).contiguous()
    for start, Sq, js in _edge_cases(PAGE):
        q = q_same[:, :, :Sq]
        k_log = torch.zeros_like(v_log)
        k_log[:, :, js] = krow
        k_pool, v_pool, table = _build(k_log, v_log, PAGE,
                                       _last([start], Sq))
        st = _pos_tensor([start])
        target = v_log[:, :, js].double()                      # [B, Hkv, D]
        for kind in ("alibi", "zero"):
            slopes = _slopes(kind)
            what = f"{kind} start={start} Sq={Sq} j*={js}"
            out = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes,
                                         scale, st)
            ref = _ref(q, k_pool, v_pool, table, slopes, scale, st)
            _check(out, ref, vmax, what)
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
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    q_all, k_log, v_log = _qkv(D, Hkv)
    start, Sq = CAP - 2, 5
    q = q_all[:, :, :Sq]
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, [CAP - 1] * B)
    st, slopes = _pos_tensor([start]), _slopes("alibi")
    out = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes,
                                 D ** -0.5, st)
    assert torch.isfinite(out).all()
    assert (out[:, :, 2:] == 0).all()
    ref = _ref(q, k_pool, v_pool, table, slopes, D ** -0.5, st)
    assert (ref[:, :, 2:] == 0).all()
    _check(out[:, :, :2], ref[:, :, :2], v_log.double().abs().max().item(),
           "rows below capacity")
    # a start wholly outside the cache, either side: zeros, nothing read
    for far in (CAP, CAP + 1000, -Sq, -(1 << 40), 1 << 40):
        out = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes,
                                     D ** -0.5, _pos_tensor([far]))
        assert (out == 0).all(), far


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 2, 16), (128, 1, 64)])
def test_single_row_agrees_with_decode(D, Hkv, PAGE):
    ext = _ext()
    q_all, k_log, v_log = _qkv(D, Hkv)
    q = q_all[:, :, :1]
    vmax = v_log.double().abs().max().item()
    for p in (0, PAGE - 1, PAGE, 64, 200, CAP - 1):
        k_pool, v_pool, table = _build(k_log, v_log, PAGE, [p] * B)
        st, slopes = _pos_tensor([p]), _slopes("alibi")
        ref = _ref(q, k_pool, v_pool, table, slopes, D ** -0.5, st)
        out = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes,
                                     D ** -0.5, st)
        dec = ext.paged_decode_attn(q, k_pool, v_pool, table, slopes,
                                    D ** -0.5, st, 0)
        _check(out, ref, vmax, f"prefill kernel, pos={p}")
        _check(dec, ref, vmax, f"decode kernel, pos={p}")


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 2, 16), (128, 1, 64)])
def test_deterministic(D, Hkv, PAGE):
    ext = _ext()
    q_all, k_log, v_log = _qkv(D, Hkv)
    start, Sq = [100, 3], 130
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, _last(start, Sq))
    args = (q_all, k_pool, v_pool, table, _slopes("alibi"), D ** -0.5,
            _pos_tensor(start))
    assert torch.equal(ext.paged_prefill_attn(*args),
                       ext.paged_prefill_attn(*args))


def test_table_row_slice_needs_no_copy():
    """block_table rows of a larger table (row stride != max_pages) and the
    matching start slice work as views."""
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    q_all, k_log, v_log = _qkv(D, Hkv)
    start, Sq = [200, 37], 40
    q = q_all[:, :, :Sq]
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, _last(start, Sq))
    big = torch.zeros(B + 2, table.size(1) + 3, dtype=torch.int32,
                      device="cuda")
    big[1:1 + B, :table.size(1)] = table
    big_start = torch.tensor([0, *start, 0], device="cuda")
    view, st = big[1:1 + B, :table.size(1)], big_start[1:1 + B]
    assert not view.is_contiguous()
    slopes = _slopes("alibi")
    a = ext.paged_prefill_attn(q, k_pool, v_pool, view, slopes, D ** -0.5, st)
    b = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes, D ** -0.5,
                               _pos_tensor(start))
    assert torch.equal(a, b)


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_reads_start_and_table_on_device(D, Hkv, PAGE):
    """A captured call replays at the start AND through the table that are
    in the tensors at replay time: the replay crosses the first tile edge,
    and each sequence's second page has moved to another pool page."""
    ext = _ext()
    s1, s2, Sq = 60, 70, 5
    q_all, k_log, v_log = _qkv(D, Hkv)
    q = q_all[:, :, :Sq]
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, _last([s1], Sq))
    scale, slopes = D ** -0.5, _slopes("alibi")
    st = _pos_tensor([s1])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes, scale, st)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes, scale,
                                     st)

    assign, spare, _ = _layout(PAGE)
    moved = assign.clone()
    moved[:, 1] = torch.tensor(spare[1:1 + B])
    k2, v2, table2 = _build(k_log, v_log, PAGE, _last([s2], Sq), assign=moved)
    assert (table2[:, 1] != table[:, 1]).all()
    st.fill_(s2)                     # all in place: the captured addresses
    k_pool.copy_(k2), v_pool.copy_(v2), table.copy_(table2)
    graph.replay()
    torch.cuda.synchronize()
    eager = ext.paged_prefill_attn(q, k_pool, v_pool, table, slopes, scale,
                                   _pos_tensor([s2]))
    assert torch.equal(out, eager)
    ref = _ref(q, k_pool, v_pool, table, slopes, scale, st)
    _check(out, ref, v_log.double().abs().max().item(), "replay at start 70")


def test_host_checks():
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    q_all, k_log, v_log = _qkv(D, Hkv)
    q = q_all[:, :, :5]
    kp, vp, table = _build(k_log, v_log, PAGE, [9] * B)
    slopes, scale, st = _slopes("alibi"), 0.125, _pos_tensor([5])
    call = ext.paged_prefill_attn
    with pytest.raises(RuntimeError, match="bf16"):
        call(q.float(), kp, vp, table, slopes, scale, st)
    with pytest.raises(RuntimeError, match="bf16"):
        call(q, kp, vp.half(), table, slopes, scale, st)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q, kp.cpu(), vp, table, slopes, scale, st)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q, kp, vp, table, slopes.cpu(), scale, st)
    with pytest.raises(RuntimeError, match="page size"):
        call(q, kp[:, :, :8], vp[:, :, :8], table, slopes, scale, st)
    with pytest.raises(RuntimeError, match="64 or 128"):
        call(q[..., :32].contiguous(), kp[..., :32].contiguous(),
             vp[..., :32].contiguous(), table, slopes, scale, st)
    q3 = torch.zeros(B, 3, 5, D, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of kv heads"):
        call(q3, kp, vp, table, slopes[:3].contiguous(), scale, st)
    with pytest.raises(RuntimeError, match="int32"):
        call(q, kp, vp, table.long(), slopes, scale, st)
    with pytest.raises(RuntimeError, match="int32"):
        call(q, kp, vp, table.cpu(), slopes, scale, st)
    with pytest.raises(RuntimeError, match="block_table must be"):
        call(q, kp, vp, table[:1], slopes, scale, st)
    with pytest.raises(RuntimeError, match="start"):
        call(q, kp, vp, table, slopes, scale, _pos_tensor([1, 2, 3]))
    with pytest.raises(RuntimeError, match="start"):
        call(q, kp, vp, table, slopes, scale, st.int())
    with pytest.raises(TypeError):
        call(q, kp, vp, table, slopes, scale, None)
    with pytest.raises(RuntimeError, match="sizes"):
        call(q, kp, vp[:, :1], table, slopes, scale, st)
    with pytest.raises(RuntimeError, match="Sq >= 1"):
        call(q[:, :, :0], kp, vp, table, slopes, scale, st)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(q.transpose(2, 3), kp, vp, table, slopes, scale, st)


def test_opt_out_and_dispatch(monkeypatch):
    D, Hkv, PAGE = 64, 2, 16
    q_all, k_log, v_log = _qkv(D, Hkv)
    start, Sq = [30], 20
    q = q_all[:, :, :Sq]
    kp, vp, table = _build(k_log, v_log, PAGE, _last(start, Sq))
    st, slopes = _pos_tensor(start), _slopes("alibi")
    assert paged_kernel_supported(q, kp)
    ext = _ext()
    calls = []
    real = ext.paged_prefill_attn
    monkeypatch.setattr(ext, "paged_prefill_attn",
                        lambda *a: calls.append("prefill") or real(*a))
    on = paged_prefill_attention(q, kp, vp, table, slopes, D ** -0.5, st)
    assert calls == ["prefill"]
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    assert not paged_kernel_supported(q, kp)
    off = paged_prefill_attention(q, kp, vp, table, slopes, D ** -0.5, st)
    assert calls == ["prefill"], "PG_DECODE_ATTN=0 must not launch"
    assert off.shape == on.shape and torch.isfinite(off).all()
    ref = _ref(q, kp, vp, table, slopes, D ** -0.5, st)
    _check(on, ref, v_log.double().abs().max().item(), "dispatched kernel")
    q_grad = q.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="inference-only"):
        paged_prefill_attention(q_grad, kp, vp, table, slopes, D ** -0.5, st)
