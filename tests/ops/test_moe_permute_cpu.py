"""ops/moe_permute.py on the CPU: the torch reference route plan against a
brute-force Python loop, permute/combine autograd against a dense one-hot
formulation (gradcheck, fp64), and the Experts layer under PG_MOE_GROUPED=3
falling back to exactly what PG_MOE_GROUPED=2 computes."""
import os

import pytest
import torch
from torch import nn

from pipegoose_amd.nn.expert_parallel.experts import Experts
from pipegoose_amd.ops.moe_permute import (RoutePlan, combine, permute,
                                           route_plan, route_plan_reference,
                                           supported)
from pipegoose_amd.testing.utils import init_parallel_context, spawn


def _brute_plan(order, weight, e0, E):
    N, k = order.shape
    S = N * k
    buckets = [[] for _ in range(E)]
    for s in range(S):
        t, eid = s // k, int(order.reshape(-1)[s])
        if not (e0 <= eid < e0 + E):
            continue
        if weight is not None:
            if not (0 <= eid < weight.size(1)):
                continue
            if not float(weight[t, eid]) > 0:      # NaN: not kept
                continue
        buckets[eid - e0].append(s)
    rows = [s for b in buckets for s in b]
    offsets = [0]
    for b in buckets:
        offsets.append(offsets[-1] + len(b))
    slot_of_row = rows + [-1] * (S - len(rows))
    row_of_slot = [-1] * S
    for r, s in enumerate(rows):
        row_of_slot[s] = r
    return offsets, row_of_slot, slot_of_row


def _routes(name, N, k, E_tot, gen):
    """(order [N,k] int64, weight [N,E_tot] fp32 or None, e0, E)."""
    order = torch.stack([torch.randperm(E_tot, generator=gen)[:k]
                         for _ in range(N)] or
                        [torch.zeros(k, dtype=torch.int64)])[:N]
    weight = torch.zeros(N, E_tot)
    if N:
        weight.scatter_(1, order, torch.rand(N, k, generator=gen) + 0.1)
    e0, E = 0, E_tot
    if name == "one_expert":
        order = torch.full((N, k), E_tot - 1, dtype=torch.int64)
        weight = torch.ones(N, E_tot)
    elif name == "empty_experts":
        order = order % 2 * (E_tot - 1)            # only experts 0 and last
        weight = torch.ones(N, E_tot)
    elif name == "zeroed":
        drop = torch.rand(N, E_tot, generator=gen) < 0.3
        weight = torch.where(drop, torch.zeros(()), weight)
    elif name == "all_dropped":
        weight = torch.zeros(N, E_tot)
    elif name == "offset":
        e0, E = 2, max(E_tot - 4, 1)               # ids outside on both sides
    elif name == "no_weight":
        weight = None
    elif name == "bad_ids_nan":
        order = order.clone()
        order.reshape(-1)[0::5] = E_tot + 3
        order.reshape(-1)[1::7] = -2
        if N:
            weight[N // 2, order[N // 2, 0].clamp(0, E_tot - 1)] = float("nan")
    return order, weight, e0, E


PATTERNS = ["random", "one_expert", "empty_experts", "zeroed", "all_dropped",
            "offset", "no_weight", "bad_ids_nan"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N,k,E_tot", [(0, 2, 8), (1, 1, 8), (37, 1, 8),
                                       (37, 2, 8), (29, 3, 8)])
def test_reference_plan_matches_brute_force(pattern, N, k, E_tot):
    gen = torch.Generator().manual_seed(N * 31 + k)
    order, weight, e0, E = _routes(pattern, N, k, E_tot, gen)
    off, ros, sor = route_plan_reference(order, weight, e0, E)
    b_off, b_ros, b_sor = _brute_plan(order, weight, e0, E)
    assert off.dtype == ros.dtype == sor.dtype == torch.int32
    assert off.tolist() == b_off
    assert ros.tolist() == b_ros
    assert sor.tolist() == b_sor
    # the properties themselves, not only agreement with the loop
    S, M = N * k, off[-1].item()
    assert sor[M:].eq(-1).all() and sor[:M].ge(0).all()
    for r in range(M):
        assert ros[sor[r]].item() == r             # inverse maps
    assert ros.ge(0).sum().item() == M
    ids = order.reshape(-1)
    for e in range(E):
        seg = sor[off[e]:off[e + 1]]
        assert (ids[seg.long()] == e0 + e).all()   # right expert
        assert (seg[1:] > seg[:-1]).all()          # stable: slots ascend
    plan = route_plan(order, weight, e0, E)        # CPU -> the reference
    assert isinstance(plan, RoutePlan) and (plan.num_tokens, plan.k) == (N, k)
    assert torch.equal(plan.offsets, off)
    assert torch.equal(plan.row_of_slot, ros)
    assert torch.equal(plan.slot_of_row, sor)


def test_supported_is_false_off_device():
    assert not supported(torch.zeros(4, 8, dtype=torch.bfloat16), 8)
    assert not supported(torch.zeros(4, 8), 8)


def _dense(plan, S, N):
    """One-hot P [S,N] with xs = P @ x, and Q [N,S] with row t picking the
    rows of token t's kept slots (out = (Q * gate-per-row) @ ys)."""
    k = plan.k
    P = torch.zeros(S, N, dtype=torch.float64)
    slot_at = torch.zeros(S, S, dtype=torch.float64)   # [row, slot]
    for r, s in enumerate(plan.slot_of_row.tolist()):
        if s >= 0:
            P[r, s // k] = 1
            slot_at[r, s] = 1
    return P, slot_at


@pytest.mark.parametrize("k,pattern", [(1, "zeroed"), (2, "zeroed"),
                                       (3, "offset")])
def test_autograd_matches_dense_one_hot(k, pattern):
    N, H, E_tot = 7, 4, 8
    gen = torch.Generator().manual_seed(5 + k)
    order, weight, e0, E = _routes(pattern, N, k, E_tot, gen)
    plan = route_plan(order, weight, e0, E)
    S = N * k
    assert 0 < plan.offsets[-1].item() < S         # live and dead rows
    P, slot_at = _dense(plan, S, N)
    x = torch.randn(N, H, dtype=torch.float64, generator=gen,
                    requires_grad=True)
    ys = torch.randn(S, H, dtype=torch.float64, generator=gen,
                     requires_grad=True)
    gates = torch.rand(S, dtype=torch.float64, generator=gen) + 0.5
    gates.requires_grad_(True)

    assert torch.equal(permute(x, plan), P @ x)

    def dense_combine(ys_, g_):
        per_row = slot_at @ g_ if g_ is not None else slot_at.sum(1)
        return P.t() @ (per_row.unsqueeze(-1) * ys_)
    assert torch.allclose(combine(ys, gates, plan), dense_combine(ys, gates),
                          atol=1e-12)
    assert torch.allclose(combine(ys, None, plan), dense_combine(ys, None),
                          atol=1e-12)

    assert torch.autograd.gradcheck(lambda a: permute(a, plan), (x,))
    assert torch.autograd.gradcheck(lambda a, g: combine(a, g, plan),
                                    (ys, gates))
    assert torch.autograd.gradcheck(lambda a: combine(a, None, plan), (ys,))
    # analytic grads equal the dense formulation's, dropped gates get 0
    gout = torch.randn(N, H, dtype=torch.float64, generator=gen)
    g1 = torch.autograd.grad(combine(ys, gates, plan), (ys, gates), gout)
    g2 = torch.autograd.grad(dense_combine(ys, gates), (ys, gates), gout)
    for a, b in zip(g1, g2):
        assert torch.allclose(a, b, atol=1e-12)
    assert g1[1][plan.row_of_slot < 0].eq(0).all()
    assert g1[0][plan.offsets[-1].item():].eq(0).all()   # dead rows: zeros


H, NUM_EXPERTS = 16, 4


def _mlp():
    return nn.Sequential(nn.Linear(H, 4 * H), nn.GELU(), nn.Linear(4 * H, H))


def _run_mode3_is_mode2_on_cpu(rank, world_size, port):
    ctx = init_parallel_context(rank, world_size, port)
    try:
        torch.manual_seed(8)
        mod = Experts(NUM_EXPERTS, _mlp(), enable_tensor_parallel=False,
                      parallel_context=ctx)
        assert mod._grouped is not None
        n_tok = 24
        x = torch.randn(2, n_tok // 2, H)
        g = torch.randn(2, n_tok // 2, H)
        for topk in (1, 2):
            route = torch.stack([torch.randperm(NUM_EXPERTS)[:topk]
                                 for _ in range(n_tok)])
            weight = torch.zeros(n_tok, NUM_EXPERTS)
            weight.scatter_(1, route, torch.rand(n_tok, topk) + 0.1)
            res = {}
            for mode in ("2", "3"):
                os.environ["PG_MOE_GROUPED"] = mode
                xi = x.clone().requires_grad_(True)
                wi = weight.clone().requires_grad_(True)
                mod.zero_grad(set_to_none=True)
                out = mod(xi, route, wi)
                out.backward(g)
                res[mode] = [out.detach(), xi.grad, wi.grad] + \
                    [p.grad.clone() for p in mod.parameters()]
            for a, b in zip(res["2"], res["3"]):
                assert torch.equal(a, b)
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)
        ctx.destroy()


def test_experts_mode3_equals_mode2_on_cpu():
    spawn(_run_mode3_is_mode2_on_cpu, world_size=1)
