"""grouped_linear's eager path (CPU, fp32) against a per-expert F.linear
loop, and the Experts layer under PG_MOE_GROUPED=2 against the loop path."""
import os

import pytest
import torch
import torch.nn.functional as TF
from torch import nn

from pipegoose_amd.nn.expert_parallel.experts import Experts
from pipegoose_amd.ops.grouped_gemm import grouped_linear, supported
from pipegoose_amd.testing.utils import init_parallel_context, spawn

COUNTS = [0, 3, 0, 5, 1]
K, N = 12, 20


def _offsets(counts):
    return torch.tensor([0] + list(torch.tensor(counts).cumsum(0)),
                        dtype=torch.int32)


def _params(E, bias, seed):
    torch.manual_seed(seed)
    ws = [torch.randn(N, K, requires_grad=True) for _ in range(E)]
    bs = [torch.randn(N, requires_grad=True) for _ in range(E)] if bias \
        else None
    return ws, bs


@pytest.mark.parametrize("bias", [False, True])
def test_fallback_matches_per_expert_loop(bias):
    E, T = len(COUNTS), sum(COUNTS)
    ws, bs = _params(E, bias, 3)
    ws2, bs2 = _params(E, bias, 3)
    torch.manual_seed(4)
    x = torch.randn(T, K, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    g = torch.randn(T, N)

    assert not supported(x, ws)
    y = grouped_linear(x, _offsets(COUNTS), ws, bs)

    outs, start = [], 0
    for e, c in enumerate(COUNTS):
        outs.append(TF.linear(x2[start:start + c], ws2[e],
                              bs2[e] if bias else None))
        start += c
    ref = torch.cat(outs)

    assert y.shape == (T, N)
    assert torch.allclose(y, ref, atol=1e-5), (y - ref).abs().max()
    y.backward(g)
    ref.backward(g)
    assert torch.allclose(x.grad, x2.grad, atol=1e-5)
    for e in range(E):
        assert ws[e].grad is not None
        assert torch.allclose(ws[e].grad, ws2[e].grad, atol=1e-5)
        if bias:
            assert bs[e].grad is not None
            assert torch.allclose(bs[e].grad, bs2[e].grad, atol=1e-5)
        if COUNTS[e] == 0:  # empty experts: all-zero grads, never None
            assert torch.count_nonzero(ws[e].grad) == 0
            if bias:
                assert torch.count_nonzero(bs[e].grad) == 0


def test_fallback_rejects_wrong_arity():
    ws, bs = _params(3, True, 0)
    x = torch.randn(4, K)
    with pytest.raises(ValueError):
        grouped_linear(x, _offsets([1, 3]), ws, bs)
    with pytest.raises(ValueError):
        grouped_linear(x, _offsets([1, 2, 1]), ws, bs[:2])


H, NUM_EXPERTS = 16, 4


def _mlp():
    return nn.Sequential(nn.Linear(H, 4 * H), nn.GELU(), nn.Linear(4 * H, H))


def _run_hip_impl_parity(rank, world_size, port):
    """PG_MOE_GROUPED=2 routes the top-2 weighted mask path through
    grouped_linear; outputs/grads must match the per-expert loop."""
    os.environ["PG_MOE_GROUPED"] = "2"
    try:
        ctx = init_parallel_context(rank, world_size, port)
        torch.manual_seed(8)
        grouped = Experts(NUM_EXPERTS, _mlp(), enable_tensor_parallel=False,
                          parallel_context=ctx)
        torch.manual_seed(8)
        loop = Experts(NUM_EXPERTS, _mlp(), enable_tensor_parallel=False,
                       parallel_context=ctx)
        loop._grouped = None  # force the per-expert loop
        assert grouped._grouped is not None
        calls = []
        import pipegoose_amd.ops.grouped_gemm as gg
        real = gg.grouped_linear

        def spy(*a, **kw):
            calls.append(1)
            return real(*a, **kw)
        gg.grouped_linear = spy
        try:
            n_tok = 24
            x1 = torch.randn(2, n_tok // 2, H, requires_grad=True)
            x2 = x1.detach().clone().requires_grad_(True)
            route = torch.stack([torch.randperm(NUM_EXPERTS)[:2]
                                 for _ in range(n_tok)])
            weight = torch.zeros(n_tok, NUM_EXPERTS)
            weight.scatter_(1, route, torch.rand(n_tok, 2) + 0.1)
            o1 = grouped(x1, route, weight)
            o2 = loop(x2, route, weight)
        finally:
            gg.grouped_linear = real
        assert len(calls) == 2, "impl='hip' must go through grouped_linear"
        assert torch.allclose(o1, o2, atol=1e-5), (o1 - o2).abs().max()
        g = torch.randn_like(o1)
        o1.backward(g)
        o2.backward(g)
        assert torch.allclose(x1.grad, x2.grad, atol=1e-5)
        for p1, p2 in zip(grouped.parameters(), loop.parameters()):
            assert p1.grad is not None
            if p2.grad is None:
                continue
            assert torch.allclose(p1.grad, p2.grad, atol=1e-5)
        ctx.destroy()
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)


def test_experts_hip_impl_matches_loop():
    spawn(_run_hip_impl_parity, world_size=1)
