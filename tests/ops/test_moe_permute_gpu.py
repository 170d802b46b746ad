"""csrc/moe_permute.hip on the GPU: the routing plan and the four row movers
against the torch reference of ops/moe_permute.py, the grouped GEMM kernels
on a buffer whose tail rows are dead, the Experts layer under
PG_MOE_GROUPED=3, and the property the feature exists for: forward and
backward of that layer without a host synchronisation.

The plan kernel works in chunks of 1024 slots (256 threads x 4 slots), so
N = 2125 gives S = 2125 / 4250 / 6375 slots for k = 1 / 2 / 3: at least
two full chunks and a ragged last one (77, 154 and 231 slots)."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 1024
N_CHUNKS = 2 * CHUNK + 77            # 2125: three chunks at k = 1
PATTERNS = ["one_expert", "empty_experts", "zeroed", "all_dropped", "offset"]


def _ext():
    from pipegoose_amd.ops import get_extension
    return get_extension(required=True)


def _mp():
    import pipegoose_amd.ops.moe_permute as mp
    return mp


def _uniform_nonzero(shape, gen):
    """bf16 uniform in [-1, 1] with no zeros, so a leak from a dead or a
    neighbouring row always shows."""
    t = torch.rand(shape, generator=gen, device="cuda") * 2 - 1
    t = torch.where(t.abs() < 1e-2, torch.full_like(t, 0.5), t)
    return t.to(torch.bfloat16)


def _routes(pattern, N, k, E, gen):
    """(order int64 [N,k], weight fp32 [N,E_tot], e0); ids may repeat
    inside a token -- the plan treats slots independently."""
    e0, E_tot = 0, E
    if pattern == "offset":           # local range strictly inside the ids
        e0, E_tot = 2, E + 4
    order = torch.randint(0, E_tot, (N, k), generator=gen, device="cuda")
    weight = torch.rand(N, E_tot, generator=gen, device="cuda") + 0.1
    if pattern == "one_expert":
        order = torch.full_like(order, E - 1)
    elif pattern == "empty_experts":
        order = order % 2 * (E - 1)   # only the first and the last expert
    elif pattern == "zeroed":         # ~30 % of the weights zeroed
        weight = weight * (torch.rand(N, E_tot, generator=gen,
                                      device="cuda") >= 0.3)
    elif pattern == "all_dropped":
        weight = torch.zeros_like(weight)
    return order, weight, e0


def _same_plan(got, ref):
    for g, r, name in zip(got, ref, ("offsets", "row_of_slot",
                                     "slot_of_row")):
        assert g.dtype == torch.int32 and g.shape == r.shape, name
        assert torch.equal(g, r), name


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, N_CHUNKS])
@pytest.mark.parametrize("E", [1, 8, 64])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_plan_matches_reference(k, E, N):
    ext, mp = _ext(), _mp()
    gen = torch.Generator(device="cuda").manual_seed(1000 * k + 10 * E + N)
    for pattern in PATTERNS:
        order, weight, e0 = _routes(pattern, N, k, E, gen)
        for wdt in (torch.float32, torch.bfloat16):
            w = weight.to(wdt)
            ref = mp.route_plan_reference(order, w, e0, E)
            got = ext.moe_route_plan(order, w, e0, E)
            _same_plan(got, ref)
            again = ext.moe_route_plan(order, w, e0, E)
            for a, b in zip(got, again):
                assert torch.equal(a, b)            # two runs, same bits
            M = ref[0][-1].item()
            if pattern == "all_dropped":
                assert M == 0
            if pattern == "one_expert":
                assert M == N * k
        _same_plan(ext.moe_route_plan(order, None, e0, E),
                   mp.route_plan_reference(order, None, e0, E))


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
def test_plan_drops_bad_ids_and_nan(wdt):
    ext, mp = _ext(), _mp()
    N, k, E = 300, 2, 8
    gen = torch.Generator(device="cuda").manual_seed(77)
    order, weight, _ = _routes("zeroed", N, k, E, gen)
    order.view(-1)[0::5] = E + 1000000        # far outside [0, E_tot)
    order.view(-1)[1::7] = -3
    order.view(-1)[2::11] = 1 << 40
    weight[3::4, :] = float("nan")
    w = weight.to(wdt)
    ref = mp.route_plan_reference(order, w, 0, E)
    got = ext.moe_route_plan(order, w, 0, E)
    _same_plan(got, ref)
    ros = got[1].view(N, k)
    assert ros[3::4].eq(-1).all()              # NaN weights: dropped
    assert got[1][0::5].eq(-1).all() and got[1][1::7].eq(-1).all()
    # with a wide local range the bad ids pass the range test on e0/E and
    # must still be stopped by the [0, E_tot) check before indexing weight
    wide = ext.moe_route_plan(order.clamp(max=E + 50), w, 0, 64)
    _same_plan(wide, mp.route_plan_reference(order.clamp(max=E + 50), w,
                                             0, 64))


def test_public_route_plan_uses_the_kernels():
    mp = _mp()
    gen = torch.Generator(device="cuda").manual_seed(3)
    order, weight, e0 = _routes("zeroed", 65, 2, 8, gen)
    plan = mp.route_plan(order, weight, e0, 8)
    assert (plan.num_tokens, plan.k) == (65, 2)
    _same_plan(plan[:3], mp.route_plan_reference(order, weight, e0, 8))
    assert mp.supported(torch.zeros(4, 8, device="cuda",
                                    dtype=torch.bfloat16), 8)
    assert not mp.supported(torch.zeros(4, 12, device="cuda",
                                        dtype=torch.bfloat16), 8)
    assert not mp.supported(torch.zeros(4, 8, device="cuda"), 8)
    assert not mp.supported(torch.zeros(4, 8, device="cuda",
                                        dtype=torch.bfloat16), 65)


# ------------------------------------------------------------- row movers
MOVER_CASES = [(0, 2, "zeroed"), (1, 1, "zeroed"), (65, 1, "zeroed"),
               (65, 2, "zeroed"), (63, 3, "offset"), (64, 2, "all_dropped"),
               (300, 2, "zeroed")]


@functools.lru_cache(maxsize=None)
def _mover_case(N, k, pattern, H):
    """Plan, inputs and references of one case; built once, never modified."""
    mp = _mp()
    gen = torch.Generator(device="cuda").manual_seed(N * 7 + k * 3 + H)
    E = 8
    order, weight, e0 = _routes(pattern, N, k, E, gen)
    off, ros, sor = mp.route_plan_reference(order, weight, e0, E)
    S, M = N * k, off[-1].item()
    x = _uniform_nonzero((N, H), gen)
    ys = _uniform_nonzero((S, H), gen)
    dxs = _uniform_nonzero((S, H), gen)
    dout = _uniform_nonzero((N, H), gen)
    gates = (torch.rand(S, generator=gen, device="cuda") + 0.25).float()
    rows = ros.view(N, k).long()
    ok = rows >= 0
    safe = rows.clamp(min=0)
    # fp64 combine and the magnitude sum of its terms
    terms = gates.double().view(N, k, 1) * ys.double()[safe] * ok.unsqueeze(-1)
    comb64, comb_abs = terms.sum(1), terms.abs().sum(1)
    terms1 = ys.double()[safe] * ok.unsqueeze(-1)
    comb64_1, comb_abs_1 = terms1.sum(1), terms1.abs().sum(1)
    # sequential fp32 sum in ascending j, rounded once
    acc = torch.zeros(N, H, device="cuda")
    for j in range(k):
        acc = torch.where(ok[:, j:j + 1], acc + dxs.float()[safe[:, j]], acc)
    dx_ref = acc.to(torch.bfloat16)
    # combine backward
    live = sor >= 0
    slots = sor.clamp(min=0).long()
    d_rows = dout.float()[slots // k]
    dys_ref = ((gates[slots].unsqueeze(-1) * d_rows).to(torch.bfloat16)
               * live.unsqueeze(-1))
    dys_ref1 = d_rows.to(torch.bfloat16) * live.unsqueeze(-1)
    prod = d_rows.double() * ys.double() * live.unsqueeze(-1)
    dgate64 = torch.zeros(S, device="cuda", dtype=torch.float64)
    dgate_abs = torch.zeros(S, device="cuda", dtype=torch.float64)
    dgate64[slots[live]] = prod.sum(1)[live]
    dgate_abs[slots[live]] = prod.abs().sum(1)[live]
    return dict(ros=ros, sor=sor, M=M, S=S, x=x, ys=ys, dxs=dxs, dout=dout,
                gates=gates, comb64=comb64, comb_abs=comb_abs,
                comb64_1=comb64_1, comb_abs_1=comb_abs_1, dx_ref=dx_ref,
                dys_ref=dys_ref, dys_ref1=dys_ref1, dgate64=dgate64,
                dgate_abs=dgate_abs, none_kept=~ok.any(1),
                xs_ref=mp.permute_fwd_reference(x, sor, k))


def _run_movers(ext, c, N, k, ys, dxs):
    xs = ext.moe_permute_fwd(c["x"], c["sor"], k)
    dx = ext.moe_permute_bwd(dxs, c["ros"], N, k)
    out = ext.moe_combine_fwd(ys, c["gates"], c["ros"], N, k)
    out1 = ext.moe_combine_fwd(ys, None, c["ros"], N, k)
    dys, dgate = ext.moe_combine_bwd(c["dout"], ys, c["gates"], c["sor"], k,
                                     True)
    dys1, none = ext.moe_combine_bwd(c["dout"], ys, None, c["sor"], k, False)
    assert none.numel() == 0
    return dict(xs=xs, dx=dx, out=out, out1=out1, dys=dys, dgate=dgate,
                dys1=dys1)


@pytest.mark.parametrize("H", [8, 72, 520])
@pytest.mark.parametrize("N,k,pattern", MOVER_CASES)
def test_row_movers(N, k, pattern, H):
    ext = _ext()
    c = _mover_case(N, k, pattern, H)
    S, M = c["S"], c["M"]
    r = _run_movers(ext, c, N, k, c["ys"], c["dxs"])
    for name in ("xs", "dys", "dys1"):
        assert r[name].shape == (S, H) and r[name].dtype == torch.bfloat16
    for name in ("dx", "out", "out1"):
        assert r[name].shape == (N, H) and r[name].dtype == torch.bfloat16
    assert r["dgate"].shape == (S,) and r["dgate"].dtype == torch.float32

    assert torch.equal(r["xs"], c["xs_ref"])           # dead rows: zeros
    assert torch.count_nonzero(r["xs"][M:]) == 0
    assert torch.equal(r["dys"], c["dys_ref"])         # one product each
    assert torch.equal(r["dys1"], c["dys_ref1"])
    assert torch.equal(r["dx"], c["dx_ref"])           # same order, one round

    # combine: one bf16 rounding (2^-8 |ref|, with margin) plus the fp32
    # accumulate of k terms, contracted to FMA or not (k 2^-22 sum|g y|)
    for got, ref, mag in ((r["out"], c["comb64"], c["comb_abs"]),
                          (r["out1"], c["comb64_1"], c["comb_abs_1"])):
        err = (got.double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -22 * mag
        print(f"combine N={N} k={k} H={H}: max err "
              f"{err.max().item() if N else 0:.3g}")
        assert (err <= bound).all()
    # dgate: worst-case fp32 summation bound for any order
    err = (r["dgate"].double() - c["dgate64"]).abs()
    assert (err <= H * 2.0 ** -24 * c["dgate_abs"]).all()
    assert torch.count_nonzero(r["dgate"][c["ros"] < 0]) == 0

    # tokens with nothing kept: exact zeros
    nk = c["none_kept"]
    for name in ("out", "out1", "dx"):
        assert torch.count_nonzero(r[name][nk]) == 0
    if pattern == "all_dropped":
        assert M == 0 and nk.all()

    # two runs: same bits
    r2 = _run_movers(ext, c, N, k, c["ys"], c["dxs"])
    for name in r:
        assert torch.equal(r[name], r2[name]), name

    # dead rows are never read: NaN there changes nothing
    if M < S:
        ys_nan, dxs_nan = c["ys"].clone(), c["dxs"].clone()
        ys_nan[M:] = float("nan")
        dxs_nan[M:] = float("nan")
        r3 = _run_movers(ext, c, N, k, ys_nan, dxs_nan)
        for name in r:
            assert torch.isfinite(r3[name].float()).all(), name
            assert torch.equal(r[name], r3[name]), name


def test_autograd_ops_run_the_kernels():
    """permute/combine end to end on device tensors: forward and backward
    equal the raw kernels' results."""
    mp, ext = _mp(), _ext()
    N, k, H = 65, 2, 72
    c = _mover_case(N, k, "zeroed", H)
    plan = mp.RoutePlan(None, c["ros"], c["sor"], N, k)
    x = c["x"].clone().requires_grad_(True)
    xs = mp.permute(x, plan)
    xs.backward(c["dxs"])
    assert torch.equal(xs, c["xs_ref"]) and torch.equal(x.grad, c["dx_ref"])
    ys = c["ys"].clone().requires_grad_(True)
    g = c["gates"].clone().requires_grad_(True)
    out = mp.combine(ys, g, plan)
    out.backward(c["dout"])
    assert torch.equal(out, ext.moe_combine_fwd(c["ys"], c["gates"],
                                                c["ros"], N, k))
    dys, dgate = ext.moe_combine_bwd(c["dout"], c["ys"], c["gates"],
                                     c["sor"], k, True)
    assert torch.equal(ys.grad, dys) and torch.equal(g.grad, dgate)


# ------------------------------------------- grouped GEMM, short offsets
def test_grouped_gemm_ignores_rows_past_offsets_end():
    """T = S rows, offsets[E] = M < S, NaN in the rows >= M: live rows of Y
    and dX and all of dW / db are bitwise those of the M-row call."""
    ext = _ext()
    K, N = 192, 384
    counts = (0, 1, 127, 128, 129, 0, 300, 37)
    E, M, dead = len(counts), sum(counts), 150
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = _uniform_nonzero((M, K), gen)
    dy = _uniform_nonzero((M, N), gen)
    ws = [_uniform_nonzero((N, K), gen) for _ in range(E)]
    bias = _uniform_nonzero((E, N), gen)
    off = [0]
    for n in counts:
        off.append(off[-1] + n)
    off = torch.tensor(off, dtype=torch.int32, device="cuda")

    def padded(t):
        nan = torch.full((dead, t.size(1)), float("nan"), device="cuda",
                         dtype=t.dtype)
        return torch.cat([t, nan])

    y = ext.grouped_gemm_fwd(x, ws, off, bias)
    dx = ext.grouped_gemm_dgrad(dy, ws, off)
    dw, db = ext.grouped_gemm_wgrad(dy, x, off, E, True)
    y_s = ext.grouped_gemm_fwd(padded(x), ws, off, bias)
    dx_s = ext.grouped_gemm_dgrad(padded(dy), ws, off)
    dw_s, db_s = ext.grouped_gemm_wgrad(padded(dy), padded(x), off, E, True)
    assert y_s.shape == (M + dead, N) and dx_s.shape == (M + dead, K)
    assert torch.equal(y_s[:M], y)
    assert torch.equal(dx_s[:M], dx)
    assert torch.equal(dw_s, dw) and torch.equal(db_s, db)
    assert torch.isfinite(dw_s.float()).all() and torch.isfinite(db_s).all()


# ------------------------------------------------------------------ layer
def _dist_env():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29894")
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


@pytest.mark.parametrize("zeroed", [False, True])
@pytest.mark.parametrize("topk", [1, 2])
def test_experts_layer_fused_vs_loop(topk, zeroed):
    """Experts under PG_MOE_GROUPED=3 may be at most 2x as far from the
    fp32-parameter oracle as the default bf16 loop (out, x.grad, the grad
    reaching `weight`, every parameter grad); for top-1 it is bitwise the
    PG_MOE_GROUPED=2 result: same row order, same roundings."""
    _dist_env()
    from torch import nn
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.nn.expert_parallel.experts import Experts

    ctx = ParallelContext.from_torch()
    try:
        torch.manual_seed(19 + topk + 2 * zeroed)
        H, I, E, T = 128, 512, 8, 600
        proto = nn.Sequential(nn.Linear(H, I), nn.GELU(), nn.Linear(I, H))
        fused = Experts(E, proto, enable_tensor_parallel=False,
                        parallel_context=ctx).to("cuda", torch.bfloat16)
        # the ParallelContext holds process groups: share it, don't copy
        mode2 = copy.deepcopy(fused, {id(ctx): ctx})
        loop = copy.deepcopy(fused, {id(ctx): ctx})
        oracle = copy.deepcopy(fused, {id(ctx): ctx}).float()
        x, route, weight, g = _layer_inputs(E, T, H, topk, zeroed)
        assert fused._fused_applies(x.reshape(-1, H),
                                    weight.to(torch.bfloat16))

        import pipegoose_amd.ops.moe_permute as mp
        calls, real = [], mp.get_extension

        class _Spy:
            def __getattr__(self, name):
                if name.startswith("moe_"):
                    calls.append(name)
                return getattr(real(required=True), name)
        mp.get_extension = lambda required=False: _Spy()
        try:
            r3 = _run_layer(fused, "3", torch.bfloat16, x, route, weight, g)
        finally:
            mp.get_extension = real
        assert sorted(calls) == ["moe_combine_bwd", "moe_combine_fwd",
                                 "moe_permute_bwd", "moe_permute_fwd",
                                 "moe_route_plan"], calls
        r2 = _run_layer(mode2, "2", torch.bfloat16, x, route, weight, g)
        r_loop = _run_layer(loop, None, torch.bfloat16, x, route, weight, g)
        r_ref = _run_layer(oracle, None, torch.float32, x, route, weight, g)

        errs = {}
        for name, ref in r_ref.items():
            e3 = (r3[name].float() - ref).abs().max().item()
            e_loop = (r_loop[name].float() - ref).abs().max().item()
            print(f"top{topk} zeroed={zeroed} {name}: fused {e3:.4g} "
                  f"loop {e_loop:.4g}")
            errs[name] = (e3, e_loop)
        bad = {n: v for n, v in errs.items() if not v[0] <= 2 * v[1]}
        assert not bad, bad
        if topk == 1:
            differ = [n for n in r3 if n != "weight.grad"
                      and not torch.equal(r3[n], r2[n])]
            assert not differ, differ
    finally:
        ctx.destroy()


def test_fused_layer_never_synchronises_the_host():
    """Forward + backward of the layer under PG_MOE_GROUPED=3 inside
    torch.cuda.set_sync_debug_mode("error"); a known synchronising call
    must raise under the same mode, so the check cannot pass vacuously."""
    _dist_env()
    from torch import nn
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.nn.expert_parallel.experts import Experts

    ctx = ParallelContext.from_torch()
    os.environ["PG_MOE_GROUPED"] = "3"
    try:
        torch.manual_seed(23)
        H, I, E, T = 128, 512, 8, 600
        proto = nn.Sequential(nn.Linear(H, I), nn.GELU(), nn.Linear(I, H))
        mod = Experts(E, proto, enable_tensor_parallel=False,
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
