"""Paged KV cache on the CPU: the pure-torch definitions
(ops/paged_attention.py), the page allocator (models/kv_cache.py
PagedKVCache) and per-row rope positions.  No GPU, no extension."""
import pytest
import torch

from pipegoose_amd.models.kv_cache import PagedKVCache
from pipegoose_amd.ops.decode_attention import decode_attention_reference
from pipegoose_amd.ops.paged_attention import (
    paged_decode_attention, paged_decode_attention_reference, paged_gather,
    paged_kv_write, paged_kv_write_reference)
from pipegoose_amd.ops.rope import rope_at_position

B, H, HKV, D, PAGE, MAX_PAGES, N_PAGES = 2, 4, 2, 16, 16, 4, 12


def _table():
    """Two shuffled, interleaved, non-monotone page lists."""
    return torch.tensor([[7, 2, 9, 4], [3, 10, 1, 8]], dtype=torch.int32)


def _pools(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N_PAGES, HKV, PAGE, D, generator=g),
            torch.randn(N_PAGES, HKV, PAGE, D, generator=g))


def test_gather_follows_the_table():
    pool, _ = _pools(0)
    table = _table()
    rows = paged_gather(pool, table, 37)
    assert rows.shape == (B, HKV, 37, D)
    for b in range(B):
        for j in (0, 15, 16, 31, 32, 36):
            assert torch.equal(rows[b, :, j],
                               pool[table[b, j // PAGE], :, j % PAGE])


@pytest.mark.parametrize("s_new,start", [(1, [15]), (1, [16]), (37, [0]),
                                         (37, [5]), (37, [5, 16])])
def test_write_then_gather_round_trips(s_new, start):
    k_pool, v_pool = _pools(1)
    k0, v0 = k_pool.clone(), v_pool.clone()
    table = _table()
    g = torch.Generator().manual_seed(2)
    # transposed (strided) views, as the models hand them in
    k_new = torch.randn(B, s_new, HKV, D, generator=g).transpose(1, 2)
    v_new = torch.randn(B, s_new, HKV, D, generator=g).transpose(1, 2)
    st = torch.tensor(start)
    paged_kv_write_reference(k_new, v_new, k_pool, v_pool, table, st)
    kg = paged_gather(k_pool, table, MAX_PAGES * PAGE)
    vg = paged_gather(v_pool, table, MAX_PAGES * PAGE)
    touched = torch.zeros(N_PAGES, PAGE, dtype=torch.bool)
    for b in range(B):
        lo = start[b % len(start)]
        assert torch.equal(kg[b, :, lo:lo + s_new], k_new[b])
        assert torch.equal(vg[b, :, lo:lo + s_new], v_new[b])
        for j in range(lo, lo + s_new):
            touched[table[b, j // PAGE], j % PAGE] = True
    keep = ~touched[:, None, :, None].expand_as(k_pool)
    assert torch.equal(k_pool[keep], k0[keep])
    assert torch.equal(v_pool[keep], v0[keep])


def test_write_drops_rows_past_capacity():
    k_pool, v_pool = _pools(3)
    k0 = k_pool.clone()
    table = _table()
    cap = MAX_PAGES * PAGE
    k_new = torch.randn(B, HKV, 5, D)
    v_new = torch.randn(B, HKV, 5, D)
    paged_kv_write_reference(k_new, v_new, k_pool, v_pool, table,
                             torch.tensor([cap - 2]))
    kg = paged_gather(k_pool, table, cap)
    assert torch.equal(kg[:, :, cap - 2:], k_new[:, :, :2])
    changed = (k_pool != k0).any(-1).any(1)            # [n_pages, PAGE]
    assert changed.sum().item() == 2 * B               # nothing wrapped


def test_paged_reference_is_the_reference_on_the_gathered_cache():
    k_pool, v_pool = _pools(4)
    table = _table()
    q = torch.randn(B, H, 1, D)
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625])
    pos = torch.tensor([37, 3])
    cap = MAX_PAGES * PAGE
    want = decode_attention_reference(
        q, paged_gather(k_pool, table, cap), paged_gather(v_pool, table, cap),
        slopes, 0.25, pos)
    got = paged_decode_attention_reference(q, k_pool, v_pool, table, slopes,
                                           0.25, pos)
    assert torch.equal(got, want)
    # on the CPU the dispatching ops ARE the references
    assert torch.equal(
        paged_decode_attention(q, k_pool, v_pool, table, slopes, 0.25, pos),
        want)
    a, b = _pools(5), _pools(5)
    k_new, v_new = torch.randn(B, HKV, 3, D), torch.randn(B, HKV, 3, D)
    paged_kv_write(k_new, v_new, a[0], a[1], table, pos)
    paged_kv_write_reference(k_new, v_new, b[0], b[1], table, pos)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_inference_only_guard():
    k_pool, v_pool = _pools(6)
    table, pos = _table(), torch.tensor([3])
    q = torch.randn(B, H, 1, D, requires_grad=True)
    slopes = torch.zeros(H)
    with pytest.raises(RuntimeError, match="inference-only"):
        paged_decode_attention(q, k_pool, v_pool, table, slopes, 0.25, pos)
    k_new = torch.randn(B, HKV, 1, D, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        paged_kv_write(k_new, k_new, k_pool, v_pool, table, pos)
    with torch.no_grad():
        paged_decode_attention(q, k_pool, v_pool, table, slopes, 0.25, pos)
        paged_kv_write(k_new, k_new, k_pool, v_pool, table, pos)


def _cache(n_pages=6, max_seqs=3, max_len=64):
    return PagedKVCache(2, max_seqs, n_pages, 16, max_len, HKV, D,
                        torch.float32, "cpu")


def _check_ownership(cache):
    owned = [p for pages in cache.pages for p in pages]
    assert 0 not in owned and 0 not in cache._free     # the null page
    assert len(set(owned)) == len(owned)               # no double ownership
    assert sorted(owned + cache._free) == list(range(1, cache.n_pages))
    for slot, pages in enumerate(cache.pages):
        row = cache.block_table[slot].tolist()
        assert row[:len(pages)] == pages
        assert all(e == 0 for e in row[len(pages):])
        assert torch.equal(cache.block_table[slot].cpu(),
                           cache.table_host[slot])


def test_allocator():
    cache = _cache()
    assert cache.n_free_pages == 5 and cache.max_pages == 4
    assert not cache.block_table.any()
    cache.allocate(0, 17)                   # 2 pages
    cache.allocate(1, 16)                   # 1 page
    cache.allocate(0, 20)                   # already covered
    _check_ownership(cache)
    assert [len(p) for p in cache.pages] == [2, 1, 0]
    cache.allocate(1, 33)                   # grows by 2: the pool is empty
    _check_ownership(cache)
    assert cache.n_free_pages == 0
    before = cache.block_table.clone()
    with pytest.raises(RuntimeError, match="out of pages"):
        cache.allocate(2, 1)
    assert torch.equal(cache.block_table, before)      # nothing half-done
    _check_ownership(cache)
    with pytest.raises(RuntimeError, match="max_len"):
        cache.allocate(0, 65)
    cache.pos_t[0] = 9
    cache.free(0)
    assert cache.n_free_pages == 2 and cache.pos_t[0].item() == 0
    assert not cache.block_table[0].any()
    cache.allocate(2, 32)                   # the freed pages are reused
    _check_ownership(cache)
    for slot in (1, 2):
        cache.free(slot)
    assert cache.n_free_pages == 5
    _check_ownership(cache)


def test_rows_are_views():
    cache = _cache()
    rows = cache.rows(1, 3)
    assert len(rows) == 2 and rows[0].paged
    assert rows[1].k_pool is cache.k_pools[1]
    assert rows[0].block_table.data_ptr() == cache.block_table[1].data_ptr()
    assert rows[0].pos_t.data_ptr() == cache.pos_t[1:].data_ptr()
    cache.allocate(1, 16), cache.allocate(2, 16)
    rows.advance(3)
    assert cache.pos_t.tolist() == [0, 3, 3] and cache.filled == [0, 3, 3]
    with pytest.raises(AssertionError, match="empty"):
        rows[0].assert_empty()
    cache.rows(0, 1)[0].assert_empty()


def test_rope_at_per_row_positions():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 4, 1, 32, generator=g)
    pos = torch.tensor([0, 17, 300])
    got = rope_at_position(x, 10000.0, pos)
    for b in range(3):
        want = rope_at_position(x[b:b + 1], 10000.0, pos[b:b + 1])
        assert torch.equal(got[b:b + 1], want)
