"""The HIP sampler (csrc/sampling.hip) against the fp64 reference of
tests/ops/_sample_refs.py.  Tokens are compared exactly: the cases keep every
decision MARGIN away from a rounding (exact_cases)."""
import pytest
import torch

from pipegoose_amd.ops.sampling import sample_logits

from tests.ops._sample_refs import CASES, exact_cases

pytestmark = pytest.mark.gpu

PARAMS = [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.9), (1.3, 50, 0.8),
          (0.0, 0, 1.0)]


@pytest.mark.parametrize("name", list(CASES))
def test_inverse_cdf_exact(name):
    row, heads, T, k, p = CASES[name]
    u, want = exact_cases(row, heads, T, k, p)
    logits = row.cuda().expand(u.numel(), -1).contiguous()
    out = sample_logits(logits, u.cuda(), T, k, p, splits=3)
    assert torch.equal(out.cpu(), want)


def _mixed_batch():
    """Five rows of V = 4104, one per PARAMS entry (the last greedy, with a
    tied maximum), and a random u."""
    row = CASES["V4104"][0]
    logits = torch.stack([row.roll(r) for r in range(len(PARAMS))])
    logits[-1, [5, 300, 4000]] = 11.0
    g = torch.Generator().manual_seed(1)
    u = torch.rand(len(PARAMS), generator=g)
    T, k, p = (torch.tensor(x) for x in zip(*PARAMS))
    return logits.cuda(), u.cuda(), T.cuda(), k.int().cuda(), p.cuda()


def test_per_row_parameters_and_greedy_rows_equal_rows_alone():
    logits, u, T, k, p = _mixed_batch()
    out = sample_logits(logits, u, T, k, p)
    assert out[-1] == 5         # greedy: the lowest index of the tied maximum
    for r in range(len(PARAMS)):
        s = slice(r, r + 1)
        alone = sample_logits(logits[s], u[s], T[s], k[s], p[s])
        assert out[r] == alone[0], r


def test_split_invariance_and_determinism():
    logits, u, T, k, p = _mixed_batch()
    big = CASES["V250880"][0].cuda().expand(len(PARAMS), -1).contiguous()
    for z in (logits, big):
        first = sample_logits(z, u, T, k, p, splits=1)
        for splits in (1, 3, 0):
            assert torch.equal(sample_logits(z, u, T, k, p, splits=splits),
                               first), splits


def test_graph_replays_equal_eager():
    logits, u, T, k, p = _mixed_batch()
    z, v = logits.clone(), u.clone()
    sample_logits(z, v, T, k, p)                # warm the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sample_logits(z, v, T, k, p)
    for shift in (1, 2, 3):                     # several replays, new inputs
        z.copy_(logits.roll(shift, dims=1))
        v.copy_((u + 0.3 * shift) % 1.0)
        graph.replay()
        assert torch.equal(out, sample_logits(z.clone(), v.clone(), T, k, p))
