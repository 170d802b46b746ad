"""sample_logits on the CPU (the torch path, fp32 logits) against the fp64
reference of tests/ops/_sample_refs.py: exact tokens at interval midpoints,
u = 0 and u = nextafter(1, 0)."""
import pytest
import torch

from pipegoose_amd.ops.sampling import sample_logits

from tests.ops._sample_refs import CASES, exact_cases

CPU_CASES = [name for name in CASES if name != "V250880"]


@pytest.mark.parametrize("name", CPU_CASES)
def test_inverse_cdf_exact(name):
    row, heads, T, k, p = CASES[name]
    u, want = exact_cases(row, heads, T, k, p)
    logits = row.float().expand(u.numel(), -1)
    assert torch.equal(sample_logits(logits, u, T, k, p), want)


def test_greedy_lowest_index_of_tied_maximum_and_mixed_batch():
    row, heads, *_ = CASES["tie_at_top_p"]      # the maximum is alone
    tied = row.float().clone()
    tied[[5, 300, 4000]] = 11.0
    logits = torch.stack([tied, row.float(), tied])
    u = torch.tensor([0.9, 0.4, 0.4])
    T = torch.tensor([0.0, 1.0, 1.0])
    out = sample_logits(logits, u, T, 2, 1.0)
    assert out[0] == 5
    for r in range(3):
        alone = sample_logits(logits[r:r + 1], u[r:r + 1], T[r:r + 1], 2, 1.0)
        assert out[r] == alone[0]
