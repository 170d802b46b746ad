"""Paged prefill attention on the CPU: the pure-torch definition
(ops/paged_attention.py) against a dense fp64 computation written out here,
out-of-range rows, multi-row ``rope_at_position``, and the reference-only
assertions of the GPU edge test.  No GPU, no extension."""
import math

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops.paged_attention import (
    paged_gather, paged_prefill_attention,
    paged_prefill_attention_reference)
from pipegoose_amd.ops.rope import _rope_ref, rope_at_position

B, H, HKV, D, PAGE, MAX_PAGES, N_PAGES = 2, 4, 2, 16, 16, 4, 12
CAP = MAX_PAGES * PAGE


def _table():
    """Two shuffled, interleaved, non-monotone page lists."""
    return torch.tensor([[7, 2, 9, 4], [3, 10, 1, 8]], dtype=torch.int32)


def _pools(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N_PAGES, HKV, PAGE, D, generator=g).double(),
            torch.randn(N_PAGES, HKV, PAGE, D, generator=g).double())


def _dense(q, k_pool, v_pool, table, slopes, scale, start):
    """Row by row, key by key, in fp64: no gather helper, no masking trick."""
    Sq = q.size(2)
    G = H // HKV
    out = torch.zeros(B, H, Sq, D, dtype=torch.float64)
    for b in range(B):
        for i in range(Sq):
            p = start[b % len(start)] + i
            if not 0 <= p < CAP:
                continue
            for h in range(H):
                keys = [k_pool[table[b, j // PAGE], h // G, j % PAGE]
                        for j in range(p + 1)]
                vals = [v_pool[table[b, j // PAGE], h // G, j % PAGE]
                        for j in range(p + 1)]
                s = torch.stack([
                    scale * (q[b, h, i] @ key) + slopes[h] * (j - p)
                    for j, key in enumerate(keys)])
                w = torch.exp(s - s.max())
                out[b, h, i] = (w / w.sum()) @ torch.stack(vals)
    return out


@pytest.mark.parametrize("start,Sq", [([0], 1), ([0], 5), ([15], 3),
                                      ([16], 16), ([7], 40), ([30, 3], 20),
                                      ([CAP - 1], 1)])
@pytest.mark.parametrize("kind", ["alibi", "zero"])
def test_reference_against_dense_fp64(start, Sq, kind):
    k_pool, v_pool = _pools(10)
    table = _table()
    g = torch.Generator().manual_seed(11 + Sq)
    q = torch.randn(B, H, Sq, D, generator=g).double()
    slopes = (alibi_slopes(H) if kind == "alibi" else torch.zeros(H)).double()
    scale = D ** -0.5
    want = _dense(q, k_pool, v_pool, table, slopes, scale, start)
    got = paged_prefill_attention_reference(q, k_pool, v_pool, table, slopes,
                                            scale, torch.tensor(start))
    assert got.shape == (B, H, Sq, D) and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12
    # on the CPU the dispatching op IS the reference
    assert torch.equal(
        paged_prefill_attention(q, k_pool, v_pool, table, slopes, scale,
                                torch.tensor(start)), got)


def test_rows_outside_the_cache_are_zero_and_slots_beyond_do_not_leak():
    k_pool, v_pool = _pools(12)
    table = _table()
    q = torch.randn(B, H, 5, D).double()
    slopes = alibi_slopes(H).double()
    start = [CAP - 2]
    want = _dense(q, k_pool, v_pool, table, slopes, 0.25, start)
    got = paged_prefill_attention_reference(q, k_pool, v_pool, table, slopes,
                                            0.25, torch.tensor(start))
    assert torch.isfinite(got).all()
    assert (got[:, :, 2:] == 0).all()
    assert (got - want).abs().max().item() <= 1e-12
    for far in ([CAP], [-5], [-(1 << 40)], [1 << 40]):
        out = paged_prefill_attention_reference(
            q, k_pool, v_pool, table, slopes, 0.25, torch.tensor(far))
        assert (out == 0).all(), far
    # slots past the last query position may hold anything, NaN included
    start, Sq = [3, 20], 4
    for b, s in enumerate(start):
        for j in range(s + Sq, CAP):
            k_pool[table[b, j // PAGE], :, j % PAGE] = float("nan")
            v_pool[table[b, j // PAGE], :, j % PAGE] = float("nan")
    got = paged_prefill_attention_reference(
        q[:, :, :Sq], k_pool, v_pool, table, slopes, 0.25,
        torch.tensor(start))
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_at_position_rotates_row_i_at_pos_plus_i(dtype):
    x = torch.randn(B, H, 7, D).to(dtype)
    for pos in ([5], [0], [37, 3]):
        got = rope_at_position(x, 10000.0, torch.tensor(pos))
        assert got.shape == x.shape and got.dtype == dtype
        for b in range(B):
            p = pos[b % len(pos)]
            assert torch.equal(got[b:b + 1], _rope_ref(x[b:b + 1], 10000.0, p))
    # one row stays the decode step it was
    one = rope_at_position(x[:, :, :1], 10000.0, torch.tensor([37, 3]))
    for b, p in enumerate((37, 3)):
        assert torch.equal(one[b:b + 1],
                           _rope_ref(x[b:b + 1, :, :1], 10000.0, p))


@pytest.mark.parametrize("Dh,Hkv,page", [(64, 4, 16), (128, 1, 64)])
def test_edge_construction_separates_the_causal_edge(Dh, Hkv, page):
    """The reference-only assertions of the GPU edge test, at its shapes
    (B=2, H=4, CAP=320, bf16-rounded inputs): with K zero except row j*,
    aligned with the one query vector at gain 30 + 0.25*CAP, every row at
    p >= j* returns v[j*] within the GPU bound, and the row at j*-1 misses it
    by more than 4x the bound in some element."""
    cap, n_q = 320, 130
    G = H // Hkv
    scale = Dh ** -0.5
    gain = 30 + 0.25 * cap
    g = torch.Generator().manual_seed(13 + Dh)
    q_all = torch.randn(B, H, 1, Dh, generator=g).bfloat16()
    v_log = torch.randn(B, Hkv, cap, Dh, generator=g).bfloat16()
    vmax = v_log.double().abs().max().item()
    q0 = q_all[:, ::G, 0].float()
    krow = (gain * q0 / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    # identity layout: page i of sequence b is pool page 1 + b*max_pages + i
    max_pages = cap // page
    table = (1 + torch.arange(B * max_pages, dtype=torch.int32)
             ).view(B, max_pages)

    def pool_of(logical):
        pool = torch.zeros(1 + B * max_pages, Hkv, page, Dh,
                           dtype=torch.float64)
        pool[1:] = logical.double().view(B, Hkv, max_pages, page, Dh) \
            .permute(0, 2, 1, 3, 4).reshape(B * max_pages, Hkv, page, Dh)
        return pool

    v_pool = pool_of(v_log)
    assert torch.equal(paged_gather(v_pool, table, cap), v_log.double())
    for start, Sq in ((0, 65), (60, 8), (page - 1, page + 2), (17, n_q)):
        last = start + Sq - 1
        q = q_all.double().expand(B, H, Sq, Dh)
        for js in sorted({j for j in (0, start, start + 1, last, 63, 64, 127,
                                      128, page - 1, page, 2 * page - 1,
                                      2 * page) if j <= last}):
            k_log = torch.zeros_like(v_log)
            k_log[:, :, js] = krow
            target = v_log[:, :, js].double()
            bound = 2.0 ** -7 * target.abs() + 2.0 ** -7 * vmax
            for slopes in (alibi_slopes(H).double(),
                           torch.zeros(H, dtype=torch.float64)):
                ref = paged_prefill_attention_reference(
                    q, pool_of(k_log), v_pool, table, slopes, scale,
                    torch.tensor([start]))
                first = max(js - start, 0)
                seen = ref[:, ::G, first:]
                assert ((seen - target[:, :, None]).abs()
                        <= bound[:, :, None]).all(), (start, Sq, js)
                if first > 0:
                    before = ref[:, ::G, first - 1]
                    assert ((before - target).abs() > 4 * bound).any(), \
                        (start, Sq, js)
    assert math.exp(-30) * cap < 2.0 ** -7      # why the gain is enough
