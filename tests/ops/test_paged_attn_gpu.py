"""Paged decode attention and cache-write kernels
(csrc/decode_attention.hip, PAGED instantiations) against the fp64 paged
reference and, bit for bit, against the contiguous kernel on the gathered
cache.

Pool layout of every case: more pages than needed; the two sequences' pages
are a shuffled, interleaved, non-monotone selection; every page outside a
live prefix (page 0 included), every table entry beyond the live page count
(it names a VALID poison page) and every slot > p of the last live page hold
K = +1e30 / V = -1e30.  A finite result within the bound shows that nothing
beyond p leaks, through the table or through the page.  All ids in every
table are in range: no test relies on the in-kernel clamp.

Tolerance |out - ref| <= 2^-7*|ref| + 2^-7*max|v|, the derivation of
tests/ops/test_decode_attn_gpu.py unchanged: capacity is that test's 320
rows, so fp32 accumulation still runs over <= 320 terms.
"""
import functools

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_decode_attention, paged_decode_attention_reference, paged_gather,
    paged_kernel_supported, paged_kv_write)

pytestmark = pytest.mark.gpu

B, H, CAP = 2, 4, 320
TILE = 64
SHAPES = [(D, Hkv, PAGE) for D in (64, 128) for Hkv in (4, 2, 1)
          for PAGE in (16, 64)]
SPLITS = (1, 4, 0)  # forced, forced, auto
POISON_K, POISON_V = 1e30, -1e30


def _ext():
    return get_extension(required=True)


def _chunk(n_splits, Hkv, D):
    """The plan rule of the kernel's file header on Skv = max_pages*PAGE."""
    if n_splits == 0:
        return _ext().decode_attn_plan(B, Hkv, CAP, D)[1]
    per_split = (CAP + n_splits - 1) // n_splits
    return (per_split + TILE - 1) // TILE * TILE


def _positions(c, PAGE):
    return sorted({min(max(p, 0), CAP - 1)
                   for p in (0, 1, PAGE - 1, PAGE, c - 1, c, c + 1, CAP - 1)})


def _cases(D, Hkv, PAGE):
    for n in SPLITS:
        c = _chunk(n, Hkv, D)
        for p in _positions(c, PAGE):
            yield n, c, [p] * B
        yield n, c, [min(c + 1, CAP - 1), 0]


def _slopes(kind):
    s = alibi_slopes(H) if kind == "alibi" else torch.zeros(H)
    return s.to("cuda", torch.float32)


@functools.lru_cache(maxsize=None)
def _qkv(D, Hkv):
    """One set of random logical inputs per shape, shared, never modified."""
    g = torch.Generator(device="cuda").manual_seed(2000 + D + 7 * Hkv)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    return mk(B, H, 1, D), mk(B, Hkv, CAP, D), mk(B, Hkv, CAP, D)


@functools.lru_cache(maxsize=None)
def _layout(PAGE):
    """(assign [B, max_pages], spare ids): pages 1.. of a pool of
    2*max_pages + 9 pages, shuffled and dealt alternately to the two
    sequences; the rest (and page 0) stay poison."""
    max_pages = CAP // PAGE
    n_pool = 2 * max_pages + 9
    g = torch.Generator().manual_seed(PAGE)
    perm = (torch.randperm(n_pool - 1, generator=g) + 1).tolist()
    assign = torch.tensor([perm[0:2 * max_pages:2], perm[1:2 * max_pages:2]])
    assert (assign[:, 1:] < assign[:, :-1]).any()          # non-monotone
    return assign, perm[2 * max_pages:], n_pool


def _pos_tensor(pos_rows):
    rows = pos_rows if len(set(pos_rows)) > 1 else pos_rows[:1]
    return torch.tensor(rows, device="cuda", dtype=torch.long)


def _build(k_log, v_log, PAGE, pos_rows, assign=None):
    """Pools and table holding the logical rows 0..p of every sequence, all
    the rest poison (module docstring)."""
    base, spare, n_pool = _layout(PAGE)
    assign = base if assign is None else assign
    Hkv, D = k_log.size(1), k_log.size(3)
    max_pages = CAP // PAGE
    p = torch.tensor(pos_rows)
    live = torch.arange(max_pages)[None, :] <= (p // PAGE)[:, None]
    table = torch.where(live, assign, torch.tensor(spare[0]))
    assert table.min() >= 0 and table.max() < n_pool       # ids in range
    pools = []
    for logical, poison in ((k_log, POISON_K), (v_log, POISON_V)):
        logical = logical.clone()
        for b, pb in enumerate(pos_rows):
            logical[b, :, pb + 1:] = poison
        pages = logical.view(B, Hkv, max_pages, PAGE, D).permute(0, 2, 1, 3, 4)
        pool = torch.full((n_pool, Hkv, PAGE, D), poison, device="cuda",
                          dtype=torch.bfloat16)
        pool[assign[live].cuda()] = pages[live.cuda()]
        pools.append(pool)
    return pools[0], pools[1], table.to("cuda", torch.int32)


def _check(out, ref, vmax, what):
    assert out.shape == ref.shape, what
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out.double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -7 * vmax
    worst = (err - bound).max().item()
    assert worst <= 0, (f"{what}: max err {err.max().item():.4g}, exceeds "
                        f"the bound by {worst:.4g}")


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_random_inputs(D, Hkv, PAGE):
    ext = _ext()
    q, k_log, v_log = _qkv(D, Hkv)
    scale = D ** -0.5
    vmax = v_log.double().abs().max().item()
    for n, c, rows in _cases(D, Hkv, PAGE):
        k_pool, v_pool, table = _build(k_log, v_log, PAGE, rows)
        pos = _pos_tensor(rows)
        kg = paged_gather(k_pool, table, CAP).contiguous()
        vg = paged_gather(v_pool, table, CAP).contiguous()
        for kind in ("alibi", "zero"):
            slopes = _slopes(kind)
            what = f"{kind} n_splits={n} chunk={c} pos={rows}"
            out = ext.paged_decode_attn(q, k_pool, v_pool, table, slopes,
                                        scale, pos, n)
            assert out.dtype == torch.bfloat16
            assert out.transpose(1, 2).is_contiguous()
            ref = paged_decode_attention_reference(
                q.double(), k_pool.double(), v_pool.double(), table,
                slopes.double(), scale, pos)
            _check(out, ref, vmax, what)
            # one online-softmax body, same operations in the same order
            flat = ext.decode_attn(q, kg, vg, slopes, scale, pos, n)
            assert torch.equal(out, flat), f"{what}: differs from decode_attn"


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_every_index_is_reachable(D, Hkv, PAGE):
    """K is zero except row j*, aligned with the group's first q head
    strongly enough that softmax puts all weight there: out == v[j*].  A
    page or split boundary that is dropped, counted twice or looked up in
    the wrong table entry shows here."""
    ext = _ext()
    q, _, v_log = _qkv(D, Hkv)
    G = H // Hkv
    scale = D ** -0.5
    gain = 30 + 0.25 * CAP
    vmax = v_log.double().abs().max().item()
    q0 = q[:, ::G, 0].float()                                  # [B, Hkv, D]
    krow = (gain * q0 / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    for n in SPLITS:
        c = _chunk(n, Hkv, D)
        for p in _positions(c, PAGE):
            for js in sorted({min(j, p)
                              for j in (0, p, PAGE - 1, PAGE, c - 1, c)}):
                k_log = torch.zeros_like(v_log)
                k_log[:, :, js] = krow
                k_pool, v_pool, table = _build(k_log, v_log, PAGE, [p] * B)
                for kind in ("alibi", "zero"):
                    out = ext.paged_decode_attn(
                        q, k_pool, v_pool, table, _slopes(kind), scale,
                        _pos_tensor([p] * B), n)
                    assert torch.isfinite(out).all()
                    _check(out[:, ::G, 0], v_log[:, :, js].double(), vmax,
                           f"{kind} n_splits={n} chunk={c} pos={p} j*={js}")


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 2, 16), (128, 1, 64)])
def test_deterministic(D, Hkv, PAGE):
    ext = _ext()
    q, k_log, v_log = _qkv(D, Hkv)
    rows = [CAP - 1, CAP // 2]
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, rows)
    pos = _pos_tensor(rows)
    for n in SPLITS:
        a = ext.paged_decode_attn(q, k_pool, v_pool, table, _slopes("alibi"),
                                  D ** -0.5, pos, n)
        b = ext.paged_decode_attn(q, k_pool, v_pool, table, _slopes("alibi"),
                                  D ** -0.5, pos, n)
        assert torch.equal(a, b)


def test_table_row_slice_needs_no_copy():
    """block_table rows of a larger table (row stride != max_pages) and the
    matching pos slice work as views."""
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    q, k_log, v_log = _qkv(D, Hkv)
    rows = [200, 37]
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, rows)
    big = torch.zeros(B + 2, table.size(1) + 3, dtype=torch.int32,
                      device="cuda")
    big[1:1 + B, :table.size(1)] = table
    big_pos = torch.tensor([0, *rows, 0], device="cuda")
    view, pos = big[1:1 + B, :table.size(1)], big_pos[1:1 + B]
    assert not view.is_contiguous()
    slopes = _slopes("alibi")
    a = ext.paged_decode_attn(q, k_pool, v_pool, view, slopes, D ** -0.5,
                              pos, 0)
    b = ext.paged_decode_attn(q, k_pool, v_pool, table, slopes, D ** -0.5,
                              _pos_tensor(rows), 0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_reads_pos_and_table_on_device(D, Hkv, PAGE):
    """A captured call replays at the position AND through the table that
    are in the tensors at replay time: the replay crosses a split boundary,
    and each sequence's second page has moved to another pool page."""
    ext = _ext()
    n = 4
    c = _chunk(n, Hkv, D)
    p1, p2 = c - 1, c + 1
    q, k_log, v_log = _qkv(D, Hkv)
    k_pool, v_pool, table = _build(k_log, v_log, PAGE, [p1] * B)
    scale, slopes = D ** -0.5, _slopes("alibi")
    pos = _pos_tensor([p1])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.paged_decode_attn(q, k_pool, v_pool, table, slopes, scale, pos, n)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext.paged_decode_attn(q, k_pool, v_pool, table, slopes, scale,
                                    pos, n)

    assign, spare, _ = _layout(PAGE)
    moved = assign.clone()
    moved[:, 1] = torch.tensor(spare[1:1 + B])
    k2, v2, table2 = _build(k_log, v_log, PAGE, [p2] * B, assign=moved)
    assert (table2[:, 1] != table[:, 1]).all()
    pos.fill_(p2)                    # all in place: the captured addresses
    k_pool.copy_(k2), v_pool.copy_(v2), table.copy_(table2)
    graph.replay()
    torch.cuda.synchronize()
    eager = ext.paged_decode_attn(q, k_pool, v_pool, table, slopes, scale,
                                  _pos_tensor([p2]), n)
    assert torch.equal(out, eager)
    ref = paged_decode_attention_reference(
        q.double(), k_pool.double(), v_pool.double(), table, slopes.double(),
        scale, pos)
    _check(out, ref, v_log.double().abs().max().item(), "replay at p2")


# ------------------------------------------------------------------ kv write

SENTINEL = 0x5A5B       # a bf16 bit pattern no randn value rounds to by luck


def _sentinel_pools(PAGE, Hkv, D):
    _, _, n_pool = _layout(PAGE)
    mk = lambda: torch.full((n_pool, Hkv, PAGE, D), SENTINEL, device="cuda",
                            dtype=torch.int16).view(torch.bfloat16)
    return mk(), mk()


def _full_table(PAGE):
    return _layout(PAGE)[0].to("cuda", torch.int32)


def _write_cases(PAGE):
    return [(1, [PAGE - 1]), (1, [PAGE]), (37, [0]), (37, [5]),
            (37, [5, PAGE]),
            (5, [CAP - 2])]      # the last three rows fall past capacity


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (64, 1, 64),
                                        (128, 2, 16), (128, 4, 64)])
def test_kv_write(D, Hkv, PAGE):
    ext = _ext()
    table = _full_table(PAGE)
    g = torch.Generator(device="cuda").manual_seed(3000 + D + Hkv + PAGE)
    for s_new, start in _write_cases(PAGE):
        k_pool, v_pool = _sentinel_pools(PAGE, Hkv, D)
        # transposed views of a wider buffer (strided in every dim but the
        # last), as the models hand in slices of a fused projection
        mk = lambda: torch.randn(
            B, s_new, Hkv, D + 8, device="cuda",
            generator=g).bfloat16()[..., 8:].transpose(1, 2)
        k_new, v_new = mk(), mk()
        assert not k_new.is_contiguous() and k_new.stride(3) == 1
        ext.paged_kv_write(k_new, v_new, k_pool, v_pool, table,
                           torch.tensor(start, device="cuda"))
        kg = paged_gather(k_pool, table, CAP)
        vg = paged_gather(v_pool, table, CAP)
        touched = torch.zeros(k_pool.size(0), PAGE, dtype=torch.bool)
        for b in range(B):
            lo = start[b % len(start)]
            kept = min(s_new, CAP - lo)         # rows past CAP are dropped
            assert kept == s_new or (s_new, lo) == (5, CAP - 2)
            assert torch.equal(kg[b, :, lo:lo + kept], k_new[b, :, :kept])
            assert torch.equal(vg[b, :, lo:lo + kept], v_new[b, :, :kept])
            for j in range(lo, lo + kept):
                touched[table[b, j // PAGE].item(), j % PAGE] = True
        # EVERY other pool element still holds the sentinel bits
        keep = ~touched.cuda()[:, None, :, None].expand_as(k_pool)
        what = f"S_new={s_new} start={start}"
        assert (k_pool.view(torch.int16)[keep] == SENTINEL).all(), what
        assert (v_pool.view(torch.int16)[keep] == SENTINEL).all(), what


def test_kv_write_graph_capture_reads_start_on_device():
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    table = _full_table(PAGE)
    k_pool, v_pool = _sentinel_pools(PAGE, Hkv, D)
    k_new = torch.randn(B, 1, Hkv, D, device="cuda").bfloat16().transpose(1, 2)
    v_new = torch.randn(B, 1, Hkv, D, device="cuda").bfloat16().transpose(1, 2)
    start = torch.tensor([3, PAGE - 1], device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.paged_kv_write(k_new, v_new, k_pool, v_pool, table, start)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ext.paged_kv_write(k_new, v_new, k_pool, v_pool, table, start)
    start.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    kg = paged_gather(k_pool, table, CAP)
    for b, lo in enumerate((3, PAGE - 1)):
        for j in (lo, lo + 1):                  # warm-up row, replayed row
            assert torch.equal(kg[b, :, j], k_new[b, :, 0])
    written = (k_pool.view(torch.int16) != SENTINEL).any(-1).any(1).sum()
    assert written.item() == 2 * B


# --------------------------------------------------------------- host checks

def test_host_checks_decode():
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    q, k_log, v_log = _qkv(D, Hkv)
    kp, vp, table = _build(k_log, v_log, PAGE, [5] * B)
    slopes, scale, pos = _slopes("alibi"), 0.125, _pos_tensor([5])
    call = ext.paged_decode_attn
    with pytest.raises(RuntimeError, match="bf16"):
        call(q.float(), kp, vp, table, slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="bf16"):
        call(q, kp, vp.half(), table, slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q, kp.cpu(), vp, table, slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q, kp, vp, table, slopes.cpu(), scale, pos, 0)
    with pytest.raises(RuntimeError, match="page size"):
        call(q, kp[:, :, :8], vp[:, :, :8], table, slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="64 or 128"):
        call(q[..., :32].contiguous(), kp[..., :32].contiguous(),
             vp[..., :32].contiguous(), table, slopes, scale, pos, 0)
    q3 = torch.zeros(B, 3, 1, D, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of kv heads"):
        call(q3, kp, vp, table, slopes[:3].contiguous(), scale, pos, 0)
    with pytest.raises(RuntimeError, match="int32"):
        call(q, kp, vp, table.long(), slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="int32"):
        call(q, kp, vp, table.cpu(), slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="block_table must be"):
        call(q, kp, vp, table[:1], slopes, scale, pos, 0)
    with pytest.raises(RuntimeError, match="pos"):
        call(q, kp, vp, table, slopes, scale, _pos_tensor([1, 2, 3]), 0)
    with pytest.raises(RuntimeError, match="pos"):
        call(q, kp, vp, table, slopes, scale, pos.int(), 0)
    with pytest.raises(TypeError):              # pos is required here
        call(q, kp, vp, table, slopes, scale, None, 0)
    with pytest.raises(RuntimeError, match="n_splits"):
        call(q, kp, vp, table, slopes, scale, pos, 65)
    with pytest.raises(RuntimeError, match="sizes"):
        call(q, kp, vp[:, :1], table, slopes, scale, pos, 0)


def test_host_checks_write():
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    table = _full_table(PAGE)
    kp, vp = _sentinel_pools(PAGE, Hkv, D)
    new = torch.zeros(B, Hkv, 3, D, device="cuda", dtype=torch.bfloat16)
    start = torch.tensor([4], device="cuda")
    call = ext.paged_kv_write
    with pytest.raises(RuntimeError, match="bf16"):
        call(new.float(), new, kp, vp, table, start)
    with pytest.raises(RuntimeError, match="bf16"):
        call(new, new, kp, vp.half(), table, start)
    with pytest.raises(RuntimeError, match="GPU"):
        call(new, new.cpu(), kp, vp, table, start)
    with pytest.raises(RuntimeError, match="page size"):
        call(new, new, kp[:, :, :8], vp[:, :, :8], table, start)
    with pytest.raises(RuntimeError, match="64 or 128"):
        call(new[..., :32].contiguous(), new[..., :32].contiguous(),
             kp[..., :32].contiguous(), vp[..., :32].contiguous(), table,
             start)
    with pytest.raises(RuntimeError, match="kv heads"):
        call(new[:, :1], new[:, :1], kp, vp, table, start)
    with pytest.raises(RuntimeError, match="int32"):
        call(new, new, kp, vp, table.long(), start)
    with pytest.raises(RuntimeError, match="start"):
        call(new, new, kp, vp, table, start.int())
    with pytest.raises(RuntimeError, match="start"):
        call(new, new, kp, vp, table, torch.zeros(3, dtype=torch.long,
                                                  device="cuda"))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(new.transpose(2, 3), new.transpose(2, 3), kp, vp, table, start)
    assert (kp.view(torch.int16) == SENTINEL).all()      # nothing launched


def test_opt_out_and_dispatch(monkeypatch):
    D, Hkv, PAGE = 64, 2, 16
    q, k_log, v_log = _qkv(D, Hkv)
    kp, vp, table = _build(k_log, v_log, PAGE, [40] * B)
    pos, slopes = _pos_tensor([40]), _slopes("alibi")
    assert paged_kernel_supported(q, kp)
    assert not paged_kernel_supported(q.float(), kp.float())
    ext = _ext()
    calls = []
    real_attn, real_write = ext.paged_decode_attn, ext.paged_kv_write
    monkeypatch.setattr(ext, "paged_decode_attn",
                        lambda *a: calls.append("attn") or real_attn(*a))
    monkeypatch.setattr(ext, "paged_kv_write",
                        lambda *a: calls.append("write") or real_write(*a))
    new = torch.randn(B, Hkv, 1, D, device="cuda").bfloat16()
    on = paged_decode_attention(q, kp, vp, table, slopes, D ** -0.5, pos)
    kp1, vp1 = kp.clone(), vp.clone()
    paged_kv_write(new, new, kp1, vp1, table, pos)
    assert calls == ["attn", "write"]
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    assert not paged_kernel_supported(q, kp)
    off = paged_decode_attention(q, kp, vp, table, slopes, D ** -0.5, pos)
    kp2, vp2 = kp.clone(), vp.clone()
    paged_kv_write(new, new, kp2, vp2, table, pos)
    assert calls == ["attn", "write"], "PG_DECODE_ATTN=0 must not launch"
    assert torch.equal(kp1, kp2) and torch.equal(vp1, vp2)
    assert off.shape == on.shape and torch.isfinite(off).all()
    ref = paged_decode_attention_reference(
        q.double(), kp.double(), vp.double(), table, slopes.double(),
        D ** -0.5, pos)
    _check(on, ref, v_log.double().abs().max().item(), "dispatched kernel")
