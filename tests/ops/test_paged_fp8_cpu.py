"""fp8 paged cache on the CPU: the reference quantiser, the dispatch of the
ops to the references, and the cache bookkeeping.  Bounds as in
tests/ops/test_paged_fp8_attn_gpu.py."""
import pytest
import torch

from pipegoose_amd.models.kv_cache import PagedKVCache
from pipegoose_amd.ops.paged_attention import (
    paged_decode_attention, paged_decode_attention_reference,
    paged_gather_dequant, paged_kv_write, quantize_rows_fp8)

FP8 = torch.float8_e4m3fn


def test_reference_quantiser_meets_the_format_bounds():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(40, 64, generator=g).bfloat16()
    x[3] = 0
    x[4] = 1e-3
    x[4, 7] = 3e4
    q, sc = quantize_rows_fp8(x)
    assert q.dtype == FP8 and sc.dtype == torch.float32
    assert sc[3] == 0 and (q[3].float() == 0).all()
    want = x.double().abs().amax(-1) / 448
    assert ((sc.double() - want).abs() <= 2.0 ** -22 * want).all()
    y = q.double() * sc.double()[:, None]
    bound = torch.maximum(x.double().abs() * 2.0 ** -4,
                          sc.double()[:, None] * 2.0 ** -10)
    assert ((y - x.double()).abs() <= bound * (1 + 2.0 ** -10)).all()


def test_ops_with_scales_run_the_references_on_cpu():
    B, H, Hkv, D, PAGE, n_pages = 2, 4, 2, 64, 16, 7
    g = torch.Generator().manual_seed(12)
    k_pool = torch.zeros(n_pages, Hkv, PAGE, D, dtype=FP8)
    v_pool = torch.zeros_like(k_pool)
    k_scale, v_scale = torch.zeros(2, n_pages, Hkv, PAGE).unbind(0)
    table = torch.tensor([[5, 2, 0], [1, 6, 0]], dtype=torch.int32)
    k_new = torch.randn(B, Hkv, 20, D, generator=g).bfloat16()
    v_new = torch.randn(B, Hkv, 20, D, generator=g).bfloat16()
    paged_kv_write(k_new, v_new, k_pool, v_pool, table, torch.tensor([3]),
                   k_scale=k_scale, v_scale=v_scale)
    kg = paged_gather_dequant(k_pool, k_scale, table, 3 * PAGE, torch.float64)
    assert (kg[:, :, 3:23] - k_new.double()).abs().max() \
        <= k_new.double().abs().max() * 2.0 ** -3
    assert (kg[:, :, :3] == 0).all() and (kg[:, :, 23:] == 0).all()
    q = torch.randn(B, H, 1, D, generator=g).bfloat16()
    slopes, pos = torch.zeros(H), torch.tensor([22, 10])
    out = paged_decode_attention(q, k_pool, v_pool, table, slopes, 0.125, pos,
                                 k_scale=k_scale, v_scale=v_scale)
    assert out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    assert torch.equal(out, paged_decode_attention_reference(
        q, k_pool, v_pool, table, slopes, 0.125, pos, k_scale, v_scale))
    with pytest.raises(ValueError, match="go together"):
        paged_decode_attention(q, k_pool, v_pool, table, slopes, 0.125, pos,
                               k_scale=k_scale)


def test_cache_allocates_byte_pools_and_shares_scales_with_pages():
    cache = PagedKVCache(2, 2, 9, 16, 64, 2, 64, torch.bfloat16, "cpu",
                         kv_dtype=FP8)
    assert cache.k_pools[0].dtype == FP8 and cache.v_pools[1].dtype == FP8
    assert cache.k_pools[0].element_size() == 1
    for sc in cache.k_scales + cache.v_scales:
        assert sc.shape == (9, 2, 16) and sc.dtype == torch.float32
        assert not sc.any()
    cache.allocate(0, 40)
    rows = cache.rows(0, 1)
    assert rows[1].k_scale is cache.k_scales[1]
    k = torch.randn(1, 2, 40, 64).bfloat16()
    paged_kv_write(k, k, rows[0].k_pool, rows[0].v_pool, rows[0].block_table,
                   rows[0].pos_t, k_scale=rows[0].k_scale,
                   v_scale=rows[0].v_scale)
    rows.advance(40)
    assert cache.fork(0, 1, 40) == 32
    cache.allocate(1, 48)
    table = cache.block_table
    assert torch.equal(table[1, :2], table[0, :2]) and table[1, 2] != table[0, 2]
    a, b = (paged_gather_dequant(cache.k_pools[0], cache.k_scales[0],
                                 table[s:s + 1], 32, torch.float32)
            for s in (0, 1))
    assert torch.equal(a, b) and a.abs().max() > 0
    bf16 = PagedKVCache(1, 1, 3, 16, 32, 2, 64, torch.bfloat16, "cpu")
    assert bf16.k_scales == [None] and bf16.rows(0, 1)[0].k_scale is None


def test_unsupported_kv_dtype_raises():
    with pytest.raises(ValueError, match="kv_dtype"):
        PagedKVCache(1, 1, 3, 16, 32, 2, 64, torch.bfloat16, "cpu",
                     kv_dtype=torch.float16)
