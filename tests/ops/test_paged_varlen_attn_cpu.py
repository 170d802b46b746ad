"""Ragged-batch paged attention on the CPU: the packed definition
(ops/paged_attention.py) against the paged prefill reference run once per
sequence, in fp64, on the pools and tables of
tests/ops/test_paged_prefill_attn_cpu.py.  No GPU, no extension."""
import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops.paged_attention import (
    paged_prefill_attention_reference, paged_varlen_attention,
    paged_varlen_attention_reference)
from tests.ops.test_paged_prefill_attn_cpu import CAP, D, H, _pools, _table


@pytest.mark.parametrize("lens,starts,pad", [
    ([1, 1], [0, CAP - 1], 0), ([0, 5], [7, 3], 0), ([5, 0], [3, 7], 2),
    ([17, 40], [16, 7], 0), ([20, 3], [30, CAP - 2], 3)])
@pytest.mark.parametrize("kind", ["alibi", "zero"])
def test_reference_is_the_prefill_reference_per_sequence(lens, starts, pad,
                                                         kind):
    k_pool, v_pool = _pools(20)
    table = _table()
    T = sum(lens) + pad
    q = torch.randn(T, H, D, generator=torch.Generator().manual_seed(T)
                    ).double()
    slopes = (alibi_slopes(H) if kind == "alibi" else torch.zeros(H)).double()
    cu = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32)
    st = torch.tensor(starts)
    got = paged_varlen_attention_reference(q, k_pool, v_pool, table, slopes,
                                           0.25, cu, st)
    assert got.shape == (T, H, D) and got.dtype == torch.float64
    assert (got[sum(lens):] == 0).all()
    for b in range(2):
        rows = slice(int(cu[b]), int(cu[b + 1]))
        if not lens[b]:
            continue
        qb = q[rows].transpose(0, 1)[None]                    # [1, H, len, D]
        want = paged_prefill_attention_reference(
            qb, k_pool, v_pool, table[b:b + 1], slopes, 0.25, st[b:b + 1])
        assert (got[rows].transpose(0, 1) - want[0]).abs().max() <= 1e-12
    # on the CPU the dispatching op IS the reference
    assert torch.equal(paged_varlen_attention(q, k_pool, v_pool, table,
                                              slopes, 0.25, cu, st), got)
