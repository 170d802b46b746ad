"""Gated (SwiGLU) expert bank on the GPU (csrc/grouped_gemm.hip):
grouped_glu_fwd bitwise against the two plain grouped forwards and the
silu_mul kernel, grouped_glu_dgrad against an fp32 oracle, the autograd op
fused vs composed, dead rows past offsets[E], and the Experts layer and a
tiny llama under PG_MOE_GROUPED=3."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 128), (192, 384)]          # (K, I)
COUNT_SETS = [(0, 1, 127, 128, 129, 0, 300, 37), (5,), (0, 0, 200, 0),
              (3,) * 64]                  # the last fills both pointer tables
CASES = [(k, i, c) for (k, i) in SHAPES for c in COUNT_SETS]


def _ext():
    from pipegoose_amd.ops import get_extension
    return get_extension(required=True)


def _uniform_nonzero(shape, gen):
    """bf16 uniform in [-1, 1] with no zeros, so a leak from a neighbouring
    segment (or an unmasked tail row) always shows."""
    t = torch.rand(shape, generator=gen, device="cuda") * 2 - 1
    t = torch.where(t.abs() < 1e-2, torch.full_like(t, 0.5), t)
    return t.to(torch.bfloat16)


def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return torch.tensor(off, dtype=torch.int32, device="cuda")


def _silu32(g):
    return g / (1 + torch.exp(-g))


@functools.lru_cache(maxsize=None)
def _case(K, I, counts):
    """Inputs, the plain-kernel references and the fp32 oracles for one
    (K, I, counts); built once, shared by every test of that case and never
    modified."""
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(2000 + K + I + len(counts))
    E, T = len(counts), sum(counts)
    x = _uniform_nonzero((T, K), gen)
    dg = _uniform_nonzero((T, I), gen)
    du = _uniform_nonzero((T, I), gen)
    dh = _uniform_nonzero((T, I), gen)
    wg = [_uniform_nonzero((I, K), gen) for _ in range(E)]
    wu = [_uniform_nonzero((I, K), gen) for _ in range(E)]
    off = _offsets(counts)
    g = ext.grouped_gemm_fwd(x, wg, off, None)
    u = ext.grouped_gemm_fwd(x, wu, off, None)
    h = ext.silu_mul_fwd(g, u)
    h32 = _silu32(g.float()) * u.float()       # from the ROUNDED g, u
    dx32 = torch.empty(T, K, device="cuda")
    s = 0
    for e, c in enumerate(counts):
        dx32[s:s + c] = dg[s:s + c].float() @ wg[e].float() \
            + du[s:s + c].float() @ wu[e].float()
        s += c
    return dict(x=x, dg=dg, du=du, dh=dh, wg=wg, wu=wu, off=off, g=g, u=u,
                h=h, h32=h32, dx32=dx32, counts=counts)


def _check(got, ref, what):
    err = (got.float() - ref).abs().max().item() if ref.numel() else 0.0
    scale = max(1.0, ref.abs().max().item() if ref.numel() else 0.0)
    print(f"{what}: max|err|={err:.4g} bound={0.02 * scale:.4g}")
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    assert err < 0.02 * scale, f"{what}: {err} vs {0.02 * scale}"
    return err


@pytest.mark.parametrize("K,I,counts", CASES)
def test_fwd_is_bitwise_the_plain_kernels(K, I, counts):
    """g and u are accumulated by the MFMA sequence of the plain forward
    (only their column placement in the block differs) and h applies
    silu_mul's formula to the rounded g, u: all three are bitwise."""
    c, ext = _case(K, I, counts), _ext()
    h, g, u = ext.grouped_glu_fwd(c["x"], c["wg"], c["wu"], c["off"], True)
    assert h.dtype == g.dtype == u.dtype == torch.bfloat16
    assert h.shape == g.shape == u.shape == (sum(counts), I)
    assert torch.equal(g, c["g"])
    assert torch.equal(u, c["u"])
    assert torch.equal(h, c["h"])
    _check(h, c["h32"], "h vs fp32 silu*mul of the rounded g, u")
    h2, g2, u2 = ext.grouped_glu_fwd(c["x"], c["wg"], c["wu"], c["off"],
                                     False)
    assert torch.equal(h2, h)
    assert g2.numel() == 0 and u2.numel() == 0


@pytest.mark.parametrize("K,I,counts", CASES)
def test_dgrad(K, I, counts):
    c, ext = _case(K, I, counts), _ext()
    dx = ext.grouped_glu_dgrad(c["dg"], c["du"], c["wg"], c["wu"], c["off"])
    assert dx.dtype == torch.bfloat16
    err = _check(dx, c["dx32"], "fused dgrad")
    composed = ext.grouped_gemm_dgrad(c["dg"], c["wg"], c["off"]) \
        + ext.grouped_gemm_dgrad(c["du"], c["wu"], c["off"])
    err_c = _check(composed, c["dx32"], "composed dgrad")
    print(f"dgrad max|err|: fused {err:.4g} composed {err_c:.4g}")


def _run_op(c, fused):
    from pipegoose_amd.ops.grouped_gemm import grouped_glu, supported_glu
    x = c["x"].clone().requires_grad_(True)
    wg = [w.clone().requires_grad_(True) for w in c["wg"]]
    wu = [w.clone().requires_grad_(True) for w in c["wu"]]
    assert supported_glu(x, wg, wu)
    h = grouped_glu(x, c["off"], wg, wu, fused=fused)
    h.backward(c["dh"])
    return [h.detach(), x.grad] + [w.grad for w in wg + wu]


@functools.lru_cache(maxsize=None)
def _op_oracle(K, I, counts):
    """fp32 autograd of silu(x Wg^T) * (x Wu^T) per segment."""
    c = _case(K, I, counts)
    x = c["x"].float().requires_grad_(True)
    wg = [w.float().requires_grad_(True) for w in c["wg"]]
    wu = [w.float().requires_grad_(True) for w in c["wu"]]
    outs, s = [], 0
    for e, n in enumerate(counts):
        xe = x[s:s + n]
        outs.append(_silu32(xe @ wg[e].t()) * (xe @ wu[e].t()))
        s += n
    torch.cat(outs).backward(c["dh"].float())
    return x.grad, [w.grad for w in wg], [w.grad for w in wu]


@pytest.mark.parametrize("K,I,counts", CASES)
def test_autograd_fused_vs_composed(K, I, counts):
    c, E = _case(K, I, counts), len(counts)
    fused = _run_op(c, (True, True))
    composed = _run_op(c, False)
    assert torch.equal(fused[0], c["h"]) and torch.equal(composed[0], c["h"])
    # same wgrad kernel on the same dg, du, x
    for a, b in zip(fused[2:], composed[2:]):
        assert torch.equal(a, b)
    dx32, dwg32, dwu32 = _op_oracle(K, I, counts)
    _check(fused[1], dx32, "x.grad fused")
    _check(composed[1], dx32, "x.grad composed")
    for e in range(E):
        _check(fused[2 + e], dwg32[e], f"dWg[{e}]")
        _check(fused[2 + E + e], dwu32[e], f"dWu[{e}]")
        if counts[e] == 0:  # empty experts: exact zeros
            assert torch.count_nonzero(fused[2 + e]) == 0
            assert torch.count_nonzero(fused[2 + E + e]) == 0
    # the default and the mixed selections are the same numbers forward
    for sel in (None, True, (True, False), (False, True)):
        got = _run_op(c, sel)
        assert torch.equal(got[0], c["h"])
        _check(got[1], dx32, f"x.grad fused={sel}")
        for a, b in zip(got[2:], fused[2:]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("K,I,counts", CASES)
def test_bitwise_repeatable(K, I, counts):
    c, ext = _case(K, I, counts), _ext()
    runs = []
    for _ in range(2):
        h, g, u = ext.grouped_glu_fwd(c["x"], c["wg"], c["wu"], c["off"],
                                      True)
        dx = ext.grouped_glu_dgrad(c["dg"], c["du"], c["wg"], c["wu"],
                                   c["off"])
        runs.append([h, g, u, dx] + _run_op(c, True))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fused", [True, False])
def test_zero_rows(fused):
    from pipegoose_amd.ops.grouped_gemm import grouped_glu
    ext, E, K, I = _ext(), 3, 64, 128
    gen = torch.Generator(device="cuda").manual_seed(5)
    wg = [_uniform_nonzero((I, K), gen) for _ in range(E)]
    wu = [_uniform_nonzero((I, K), gen) for _ in range(E)]
    off = _offsets((0, 0, 0))
    x = torch.empty(0, K, device="cuda", dtype=torch.bfloat16)
    d = torch.empty(0, I, device="cuda", dtype=torch.bfloat16)
    h, g, u = ext.grouped_glu_fwd(x, wg, wu, off, True)
    assert h.shape == g.shape == u.shape == (0, I)
    assert ext.grouped_glu_dgrad(d, d, wg, wu, off).shape == (0, K)

    params = [w.clone().requires_grad_(True) for w in wg + wu]
    xr = x.clone().requires_grad_(True)
    h = grouped_glu(xr, off, params[:E], params[E:], fused=fused)
    assert h.shape == (0, I)
    h.sum().backward()
    assert xr.grad.shape == (0, K)
    for p in params:
        assert p.grad is not None and torch.count_nonzero(p.grad) == 0


@pytest.mark.parametrize("K,I,E", [(96, 128, 4), (64, 192, 4), (64, 128, 65)])
def test_unsupported_shapes_take_the_eager_path(K, I, E):
    from pipegoose_amd.ops.grouped_gemm import grouped_glu, supported_glu
    gen = torch.Generator(device="cuda").manual_seed(7)
    counts = tuple(3 + (e % 4) for e in range(E))
    T = sum(counts)
    x = _uniform_nonzero((T, K), gen).requires_grad_(True)
    wg = [_uniform_nonzero((I, K), gen).requires_grad_(True)
          for _ in range(E)]
    wu = [_uniform_nonzero((I, K), gen).requires_grad_(True)
          for _ in range(E)]
    assert not supported_glu(x, wg, wu)
    h = grouped_glu(x, _offsets(counts), wg, wu)
    dh = _uniform_nonzero((T, I), gen)
    h.backward(dh)
    s = 0
    for e, c in enumerate(counts):
        xe = x[s:s + c].detach().float().requires_grad_(True)
        wge = wg[e].detach().float().requires_grad_(True)
        wue = wu[e].detach().float().requires_grad_(True)
        ref = _silu32(xe @ wge.t()) * (xe @ wue.t())
        ref.backward(dh[s:s + c].float())
        _check(h[s:s + c], ref.detach(), f"h[{e}]")
        _check(x.grad[s:s + c], xe.grad, f"dx[{e}]")
        _check(wg[e].grad, wge.grad, f"dWg[{e}]")
        _check(wu[e].grad, wue.grad, f"dWu[{e}]")
        s += c


def test_rows_past_offsets_end_are_dead():
    """T = S rows, offsets[E] = M < S, NaN in the rows >= M of X, dg, du:
    live rows of g, u, h, dX and all of dWg, dWu are bitwise those of the
    M-row call."""
    ext = _ext()
    K, I = 192, 384
    c = _case(K, I, COUNT_SETS[0])
    E, M, dead = len(c["counts"]), sum(c["counts"]), 150
    off = c["off"]

    def padded(t):
        nan = torch.full((dead, t.size(1)), float("nan"), device="cuda",
                         dtype=t.dtype)
        return torch.cat([t, nan])

    xs, dgs, dus = padded(c["x"]), padded(c["dg"]), padded(c["du"])
    h, g, u = ext.grouped_glu_fwd(xs, c["wg"], c["wu"], off, True)
    assert h.shape == (M + dead, I)
    assert torch.equal(g[:M], c["g"]) and torch.equal(u[:M], c["u"])
    assert torch.equal(h[:M], c["h"])
    h2, _, _ = ext.grouped_glu_fwd(xs, c["wg"], c["wu"], off, False)
    assert torch.equal(h2[:M], c["h"])
    dx = ext.grouped_glu_dgrad(c["dg"], c["du"], c["wg"], c["wu"], off)
    dx_s = ext.grouped_glu_dgrad(dgs, dus, c["wg"], c["wu"], off)
    assert dx_s.shape == (M + dead, K) and torch.equal(dx_s[:M], dx)
    for d, ds in ((c["dg"], dgs), (c["du"], dus)):
        dw, _ = ext.grouped_gemm_wgrad(d, c["x"], off, E, False)
        dw_s, _ = ext.grouped_gemm_wgrad(ds, xs, off, E, False)
        assert torch.equal(dw_s, dw)
        assert torch.isfinite(dw_s.float()).all()

    # the autograd op on the padded buffer, on either route: dead rows of
    # dh are NaN too
    from pipegoose_amd.ops.grouped_gemm import grouped_glu
    for fused in (True, False):
        ref = _run_op(c, fused)
        x = xs.clone().requires_grad_(True)
        wg = [w.clone().requires_grad_(True) for w in c["wg"]]
        wu = [w.clone().requires_grad_(True) for w in c["wu"]]
        out = grouped_glu(x, off, wg, wu, fused=fused)
        out.backward(padded(c["dh"]))
        assert torch.equal(out[:M], ref[0])
        assert torch.equal(x.grad[:M], ref[1])
        for w, r in zip(wg + wu, ref[2:]):
            assert torch.equal(w.grad, r)


# ------------------------------------------------------------------ layer
def _dist_env():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29895")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")


def _layer_inputs(E, T, H, topk, zeroed):
    x = torch.randn(2, T // 2, H, device="cuda", dtype=torch.bfloat16)
    route = torch.stack([torch.randperm(E, device="cuda")[:topk]
                         for _ in range(T)])
    kept = torch.rand(T, topk, device="cuda") + 0.1
    if zeroed:  # ~25 % of the kept weights zeroed (capacity drops)
        kept = kept * (torch.rand(T, topk, device="cuda") >= 0.25)
    weight = torch.zeros(T, E, device="cuda")
    weight.scatter_(1, route, kept)
    g = torch.randn(2, T // 2, H, device="cuda", dtype=torch.bfloat16)
    return x, route, weight, g


def _run_layer(mod, mode, dtype, x, route, weight, g):
    xi = x.detach().to(dtype).clone().requires_grad_(True)
    wi = weight.detach().to(dtype).clone().requires_grad_(True)
    if mode is None:
        os.environ.pop("PG_MOE_GROUPED", None)
    else:
        os.environ["PG_MOE_GROUPED"] = mode
    try:
        out = mod(xi, route, wi)
        out.backward(g.to(dtype))
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)
    res = {"out": out.detach(), "x.grad": xi.grad, "weight.grad": wi.grad}
    for name, p in mod.named_parameters():
        assert p.grad is not None, name
        res[name] = p.grad
    return res


class _Spy:
    """Records the names of the extension entry points that are fetched."""

    def __init__(self, ext, calls):
        self._ext, self._calls = ext, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._ext, name)


def _spy_extension(monkeypatch, calls, fused=True):
    """Record the extension calls of the grouped and permute ops, with the
    gated bank's fused kernels switched on or off for both passes."""
    import pipegoose_amd.ops.grouped_gemm as gg
    import pipegoose_amd.ops.moe_permute as mp
    spy = _Spy(_ext(), calls)
    monkeypatch.setattr(gg, "FUSED_FWD_DEFAULT", fused)
    monkeypatch.setattr(gg, "FUSED_DGRAD_DEFAULT", fused)
    monkeypatch.setattr(gg, "get_extension", lambda required=False: spy)
    monkeypatch.setattr(mp, "get_extension", lambda required=False: spy)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("zeroed", [False, True])
@pytest.mark.parametrize("topk", [1, 2])
def test_gated_experts_layer_fused_vs_loop(topk, zeroed, fused, monkeypatch):
    """A GatedExpertMLP bank under PG_MOE_GROUPED=3 may be at most 2x as
    far from the fp32-parameter oracle as the default bf16 loop (out,
    x.grad, the grad reaching `weight`, every parameter grad), with the
    fused GLU kernels and with the composed route."""
    _dist_env()
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.nn.expert_parallel import GatedExpertMLP
    from pipegoose_amd.nn.expert_parallel.experts import Experts

    ctx = ParallelContext.from_torch()
    try:
        torch.manual_seed(29 + topk + 2 * zeroed)
        H, I, E, T = 128, 512, 8, 600
        bank = Experts(E, GatedExpertMLP(H, I), enable_tensor_parallel=False,
                       parallel_context=ctx).to("cuda", torch.bfloat16)
        # the ParallelContext holds process groups: share it, don't copy
        loop = copy.deepcopy(bank, {id(ctx): ctx})
        oracle = copy.deepcopy(bank, {id(ctx): ctx}).float()
        x, route, weight, g = _layer_inputs(E, T, H, topk, zeroed)
        assert bank._grouped_glu is not None
        assert bank._fused_applies(x.reshape(-1, H),
                                   weight.to(torch.bfloat16))

        calls = []
        _spy_extension(monkeypatch, calls, fused)
        r3 = _run_layer(bank, "3", torch.bfloat16, x, route, weight, g)
        monkeypatch.undo()
        ran = {n for n in calls if n.startswith(("moe_", "grouped_glu_"))}
        glu = {"grouped_glu_fwd", "grouped_glu_dgrad"} if fused else set()
        assert ran == glu | {"moe_combine_bwd", "moe_combine_fwd",
                             "moe_permute_bwd", "moe_permute_fwd",
                             "moe_route_plan"}, calls

        r_loop = _run_layer(loop, None, torch.bfloat16, x, route, weight, g)
        r_ref = _run_layer(oracle, None, torch.float32, x, route, weight, g)
        errs = {}
        for name, ref in r_ref.items():
            e3 = (r3[name].float() - ref).abs().max().item()
            e_loop = (r_loop[name].float() - ref).abs().max().item()
            print(f"top{topk} zeroed={zeroed} fused={fused} {name}: "
                  f"=3 {e3:.4g} loop {e_loop:.4g}")
            errs[name] = (e3, e_loop)
        bad = {n: v for n, v in errs.items() if not v[0] <= 2 * v[1]}
        assert not bad, bad
    finally:
        ctx.destroy()


@pytest.mark.parametrize("fused", [True, False])
def test_gated_layer_never_synchronises_the_host(fused, monkeypatch):
    """Forward + backward of the gated layer under PG_MOE_GROUPED=3 inside
    torch.cuda.set_sync_debug_mode("error"), on the fused GLU kernels and
    on the composed route; a known synchronising call must raise under the
    same mode, so the check cannot pass vacuously."""
    _dist_env()
    import pipegoose_amd.ops.grouped_gemm as gg
    monkeypatch.setattr(gg, "FUSED_FWD_DEFAULT", fused)
    monkeypatch.setattr(gg, "FUSED_DGRAD_DEFAULT", fused)
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.nn.expert_parallel import GatedExpertMLP
    from pipegoose_amd.nn.expert_parallel.experts import Experts

    ctx = ParallelContext.from_torch()
    os.environ["PG_MOE_GROUPED"] = "3"
    try:
        torch.manual_seed(31)
        H, I, E, T = 128, 512, 8, 600
        mod = Experts(E, GatedExpertMLP(H, I), enable_tensor_parallel=False,
                      parallel_context=ctx).to("cuda", torch.bfloat16)
        cases = []
        for topk in (1, 2):
            x, route, weight, g = _layer_inputs(E, T, H, topk, True)
            weight = weight.bfloat16()
            assert mod._fused_applies(x.reshape(-1, H), weight)
            cases.append((x.requires_grad_(True),
                          route, weight.requires_grad_(True), g))
        for x, route, weight, g in cases:          # warm-up
            mod(x, route, weight).backward(g)
        ones = torch.ones(4, device="cuda")
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                ones.nonzero()
            outs = []
            for x, route, weight, g in cases:
                out = mod(x, route, weight)
                out.backward(g)
                outs.append(out)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        for out in outs:
            assert torch.isfinite(out.float()).all()
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)
        ctx.destroy()


def test_llama_moe_trains_a_step(monkeypatch):
    """A 2-layer llama wrapped by ExpertParallel(expert=GatedExpertMLP):
    one training step under PG_MOE_GROUPED=3 on the fused kernels."""
    _dist_env()
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from pipegoose_amd.nn import ExpertParallel
    from pipegoose_amd.nn.expert_parallel import (ExpertLoss, GatedExpertMLP,
                                                  SwitchNoisePolicy,
                                                  Top2Router)
    from pipegoose_amd.nn.expert_parallel.layers import ExpertLayer

    ctx = ParallelContext.from_torch()
    os.environ["PG_MOE_GROUPED"] = "3"
    try:
        torch.manual_seed(37)
        cfg = LlamaConfig(vocab_size=256, hidden_size=128,
                          intermediate_size=256, n_layer=2, n_head=4)
        model = LlamaForCausalLM(cfg, ctx)
        model = ExpertParallel(
            model, 4, expert=GatedExpertMLP(128, 256),
            router=Top2Router(SwitchNoisePolicy(), 4, 128),
            parallel_context=ctx).parallelize().to("cuda", torch.bfloat16)
        layers = [m for m in model.modules() if isinstance(m, ExpertLayer)]
        assert len(layers) == 2
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        ids = torch.randint(0, 256, (2, 64), device="cuda")
        calls = []
        _spy_extension(monkeypatch, calls)
        loss = ExpertLoss(lambda: model(ids, labels=ids))()
        loss.backward()
        monkeypatch.undo()
        assert torch.isfinite(loss.float()).item(), loss
        assert calls.count("grouped_glu_fwd") == 2, calls
        assert calls.count("grouped_glu_dgrad") == 2, calls
        assert calls.count("moe_route_plan") == 2, calls
        for m in layers:
            for name, p in m._experts.named_parameters():
                assert p.grad is not None, name
                assert torch.isfinite(p.grad.float()).all(), name
        opt.step()
    finally:
        os.environ.pop("PG_MOE_GROUPED", None)
        ctx.destroy()
