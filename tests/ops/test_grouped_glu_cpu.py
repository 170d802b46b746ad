"""Gated (SwiGLU) expert bank without a GPU: grouped_glu's eager path
against a per-expert autograd loop, the bank matcher, the Experts layer
under PG_MOE_GROUPED=2/3 against the default loop (mask dispatch, and
all-to-all over two gloo ranks), and ExpertParallel wrapping the llama and
bloom models."""
import os

import pytest
import torch
import torch.nn.functional as TF
from torch import nn

from pipegoose_amd.nn.expert_parallel import GatedExpertMLP
from pipegoose_amd.nn.expert_parallel.experts import Experts
from pipegoose_amd.nn.expert_parallel.grouped import (grouped_glu_mlp_forward,
                                                      match_grouped_glu)
from pipegoose_amd.ops.grouped_gemm import grouped_glu, supported_glu
from pipegoose_amd.testing.utils import init_parallel_context, spawn

COUNTS = (0, 3, 5, 0, 1)
K, I = 12, 20


def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return torch.tensor(off, dtype=torch.int32)


def _weights(E, seed):
    torch.manual_seed(seed)
    return ([torch.randn(I, K, requires_grad=True) for _ in range(E)],
            [torch.randn(I, K, requires_grad=True) for _ in range(E)])


@pytest.mark.parametrize("fused", [True, False])
def test_eager_path_matches_per_expert_loop(fused):
    E, T = len(COUNTS), sum(COUNTS)
    wg, wu = _weights(E, 3)
    wg2, wu2 = _weights(E, 3)
    torch.manual_seed(4)
    x = torch.randn(T, K, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    dh = torch.randn(T, I)

    assert not supported_glu(x, wg, wu)
    h = grouped_glu(x, _offsets(COUNTS), wg, wu, fused=fused)

    outs, s = [], 0
    for e, c in enumerate(COUNTS):
        xe = x2[s:s + c]
        outs.append(TF.silu(xe @ wg2[e].t()) * (xe @ wu2[e].t()))
        s += c
    ref = torch.cat(outs)

    assert h.shape == (T, I)
    assert torch.allclose(h, ref, atol=1e-5), (h - ref).abs().max()
    h.backward(dh)
    ref.backward(dh)
    assert torch.allclose(x.grad, x2.grad, atol=1e-5)
    for e, c in enumerate(COUNTS):
        for w, w2 in ((wg[e], wg2[e]), (wu[e], wu2[e])):
            assert w.grad is not None
            if c == 0:  # empty experts: all-zero grads, never None
                assert torch.count_nonzero(w.grad) == 0
            else:
                assert torch.allclose(w.grad, w2.grad, atol=1e-5)


def test_rejects_wrong_arity():
    wg, wu = _weights(3, 0)
    x = torch.randn(4, K)
    with pytest.raises(ValueError):
        grouped_glu(x, _offsets([1, 3]), wg, wu)
    with pytest.raises(ValueError):
        grouped_glu(x, _offsets([1, 2, 1]), wg, wu[:2])


def test_gated_expert_mlp_is_the_llama_formula():
    torch.manual_seed(1)
    m = GatedExpertMLP(8, 24)
    assert [n for n, _ in m.named_parameters()] == [
        "gate_proj.weight", "up_proj.weight", "down_proj.weight"]
    assert m.down_proj.weight.shape == (8, 24)
    assert GatedExpertMLP(8, 24, out=16).down_proj.weight.shape == (16, 24)
    x = torch.randn(5, 8)
    ref = TF.linear(TF.silu(TF.linear(x, m.gate_proj.weight))
                    * TF.linear(x, m.up_proj.weight), m.down_proj.weight)
    assert torch.allclose(m(x), ref, atol=1e-6)


def test_match_grouped_glu():
    bank = nn.ModuleList(GatedExpertMLP(8, 24) for _ in range(3))
    wg, wu, wd = match_grouped_glu(bank)
    for e, m in enumerate(bank):
        assert wg[e] is m.gate_proj.weight
        assert wu[e] is m.up_proj.weight
        assert wd[e] is m.down_proj.weight

    mixed = nn.ModuleList([GatedExpertMLP(8, 24), GatedExpertMLP(8, 32)])
    assert match_grouped_glu(mixed) is None
    mixed_out = nn.ModuleList([GatedExpertMLP(8, 24),
                               GatedExpertMLP(8, 24, out=16)])
    assert match_grouped_glu(mixed_out) is None

    biased = nn.ModuleList(GatedExpertMLP(8, 24) for _ in range(2))
    biased[1].up_proj = nn.Linear(8, 24, bias=True)
    assert match_grouped_glu(biased) is None

    plain = nn.ModuleList(
        nn.Sequential(nn.Linear(8, 24), nn.SiLU(), nn.Linear(24, 8))
        for _ in range(2))
    assert match_grouped_glu(plain) is None
    assert match_grouped_glu(nn.ModuleList()) is None


H, INTER, NUM_EXPERTS = 16, 40, 4


def _run_layer_parity(rank, world_size, port, mode, topk, zeroed):
    """A GatedExpertMLP bank under PG_MOE_GROUPED=2/3 goes through
    grouped_glu_mlp_forward and equals the default per-expert loop."""
    ctx = init_parallel_context(rank, world_size, port)
    torch.manual_seed(8)
    grouped = Experts(NUM_EXPERTS, GatedExpertMLP(H, INTER),
                      enable_tensor_parallel=False, parallel_context=ctx)
    torch.manual_seed(8)
    loop = Experts(NUM_EXPERTS, GatedExpertMLP(H, INTER),
                   enable_tensor_parallel=False, parallel_context=ctx)
    assert grouped._grouped is None and grouped._grouped_glu is not None
    # the bmm bank has no gated form: modes 0 and 1 keep the loop
    assert not grouped._bank_modes("0") and not grouped._bank_modes("1")
    assert grouped._bank_modes("2") and grouped._bank_modes("3")

    import pipegoose_amd.nn.expert_parallel.grouped as grp
    calls, real = [], grp.grouped_glu_mlp_forward

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    n_tok = 24
    torch.manual_seed(9 + topk)
    x1 = torch.randn(2, n_tok // 2, H, requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    route = torch.stack([torch.randperm(NUM_EXPERTS)[:topk]
                         for _ in range(n_tok)])
    kept = torch.rand(n_tok, topk) + 0.1
    if zeroed:  # capacity drops
        kept = kept * (torch.rand(n_tok, topk) >= 0.25)
    weight = torch.zeros(n_tok, NUM_EXPERTS).scatter_(1, route, kept)
    w1 = weight.clone().requires_grad_(True)
    w2 = weight.clone().requires_grad_(True)

    grp.grouped_glu_mlp_forward = spy
    os.environ["PG_MOE_GROUPED"] = mode
    try:
        o1 = grouped(x1, route, w1)
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)
        grp.grouped_glu_mlp_forward = real
    o2 = loop(x2, route, w2)
    assert len(calls) == 1, "the gated bank must run as one grouped call"
    assert torch.allclose(o1, o2, atol=1e-5), (o1 - o2).abs().max()
    g = torch.randn_like(o1)
    o1.backward(g)
    o2.backward(g)
    assert torch.allclose(x1.grad, x2.grad, atol=1e-5)
    assert torch.allclose(w1.grad, w2.grad, atol=1e-5)
    for p1, p2 in zip(grouped.parameters(), loop.parameters()):
        assert p1.grad is not None and p2.grad is not None
        assert torch.allclose(p1.grad, p2.grad, atol=1e-5)

    # under the default mode the same module runs the loop
    calls.clear()
    grp.grouped_glu_mlp_forward = spy
    try:
        o3 = grouped(x1.detach(), route, weight)
    finally:
        grp.grouped_glu_mlp_forward = real
    assert not calls and torch.allclose(o3, o2, atol=1e-5)
    ctx.destroy()


@pytest.mark.parametrize("zeroed", [False, True])
@pytest.mark.parametrize("topk", [1, 2])
@pytest.mark.parametrize("mode", ["2", "3"])
def test_gated_experts_grouped_modes_match_loop(mode, topk, zeroed):
    spawn(_run_layer_parity, world_size=1, mode=mode, topk=topk,
          zeroed=zeroed)


def _run_llama_moe_step(rank, world_size, port):
    from pipegoose_amd.models.llama import LlamaForCausalLM, llama_tiny
    from pipegoose_amd.nn import ExpertParallel
    from pipegoose_amd.nn.expert_parallel import (ExpertLoss,
                                                  SwitchNoisePolicy,
                                                  Top2Router)
    from pipegoose_amd.nn.expert_parallel.layers import ExpertLayer

    ctx = init_parallel_context(rank, world_size, port)
    cfg = llama_tiny()
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg, ctx)
    model = ExpertParallel(
        model, NUM_EXPERTS,
        expert=GatedExpertMLP(cfg.hidden_size, cfg.intermediate_size),
        router=Top2Router(SwitchNoisePolicy(), NUM_EXPERTS, cfg.hidden_size),
        parallel_context=ctx).parallelize()
    layers = [m for m in model.modules() if isinstance(m, ExpertLayer)]
    assert len(layers) == cfg.n_layer == 2
    assert all(isinstance(b.mlp, ExpertLayer) for b in model.model.layers)
    assert all(m._experts._grouped_glu is not None for m in layers)

    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    ids = torch.randint(0, cfg.vocab_size, (2, 16))
    os.environ["PG_MOE_GROUPED"] = "2"
    try:
        loss = ExpertLoss(lambda: model(ids, labels=ids))()
        loss.backward()
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)
    assert torch.isfinite(loss)
    for m in layers:
        for name, p in m._experts.named_parameters():
            assert p.grad is not None, name
    before = layers[0].experts[0].gate_proj.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, layers[0].experts[0].gate_proj.weight)
    ctx.destroy()


def test_expert_parallel_wraps_llama_and_trains_a_step():
    spawn(_run_llama_moe_step, world_size=1)


def _run_bloom_still_wraps(rank, world_size, port):
    from pipegoose_amd.models.bloom import BloomForCausalLM, bloom_tiny
    from pipegoose_amd.nn import ExpertParallel
    from pipegoose_amd.nn.expert_parallel import (SwitchNoisePolicy,
                                                  Top1Router)
    from pipegoose_amd.nn.expert_parallel.layers import ExpertLayer

    ctx = init_parallel_context(rank, world_size, port)
    cfg = bloom_tiny()
    model = ExpertParallel(
        BloomForCausalLM(cfg, ctx), NUM_EXPERTS,
        router=Top1Router(SwitchNoisePolicy(), NUM_EXPERTS, cfg.hidden_size),
        parallel_context=ctx).parallelize()
    n = sum(isinstance(m, ExpertLayer) for m in model.modules())
    assert n == cfg.n_layer
    ctx.destroy()


def test_expert_parallel_still_wraps_bloom():
    spawn(_run_bloom_still_wraps, world_size=1)


def test_grouped_glu_mlp_forward_composes_the_two_ops():
    E = len(COUNTS)
    wg, wu = _weights(E, 5)
    wd = [torch.randn(K, I) for _ in range(E)]
    x = torch.randn(sum(COUNTS), K)
    off = _offsets(COUNTS)
    out = grouped_glu_mlp_forward(x, off, wg, wu, wd)
    s = 0
    for e, c in enumerate(COUNTS):
        xe = x[s:s + c]
        ref = (TF.silu(xe @ wg[e].t()) * (xe @ wu[e].t())) @ wd[e].t()
        assert torch.allclose(out[s:s + c], ref, atol=1e-4)
        s += c


def _run_alltoall_gated(rank, world_size, port):
    """The use_hip branch of the all-to-all dispatch (gloo, 2 ranks): a
    gated bank under PG_MOE_GROUPED=2 equals the same module's loop."""
    import pipegoose_amd.nn.expert_parallel.grouped as grp
    ctx = init_parallel_context(rank, world_size, port,
                                tensor_parallel_size=2)
    torch.manual_seed(2)  # same seed every rank -> identical experts
    experts = Experts(NUM_EXPERTS, GatedExpertMLP(H, INTER),
                      enable_tensor_parallel=True, parallel_context=ctx,
                      dispatch="alltoall")
    assert experts.num_local_experts == 2
    assert experts._grouped_glu is not None
    torch.manual_seed(3)
    x = torch.randn(2, 8, H)
    route = torch.stack([torch.randperm(NUM_EXPERTS)[:2] for _ in range(16)])
    weight = torch.zeros(16, NUM_EXPERTS).scatter_(
        1, route, torch.rand(16, 2) + 0.1)
    g = torch.randn(2, 8, H)

    calls, real = [], grp.grouped_glu_mlp_forward

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    res = {}
    for mode in ("2", None):
        xi = x.clone().requires_grad_(True)
        experts.zero_grad()
        grp.grouped_glu_mlp_forward = spy
        if mode is not None:
            os.environ["PG_MOE_GROUPED"] = mode
        try:
            out = experts(xi, route, weight)
            out.backward(g)
        finally:
            os.environ.pop("PG_MOE_GROUPED", None)
            grp.grouped_glu_mlp_forward = real
        res[mode] = [out.detach(), xi.grad] + [
            p.grad.clone() for p in experts.parameters()]
    assert len(calls) == 1, "only PG_MOE_GROUPED=2 takes the bank call"
    for a, b in zip(res["2"], res[None]):
        assert torch.allclose(a, b, atol=1e-5), (a - b).abs().max()
    ctx.destroy()


def test_alltoall_gated_bank_matches_loop_tp2():
    spawn(_run_alltoall_gated, world_size=2)
