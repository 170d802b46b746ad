"""Native grouped expert GEMM (csrc/grouped_gemm.hip) on the GPU: the three
kernels against an fp32 per-segment oracle, bitwise repeatability, the
edge cases (empty experts, partial tiles, T == 0, unsupported shapes), and
the Experts layer under PG_MOE_GROUPED=2 against the per-expert loop."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 128), (192, 384)]          # (K, N)
COUNT_SETS = [(0, 1, 127, 128, 129, 0, 300, 37), (5,), (0, 0, 200, 0)]
CASES = [(k, n, c) for (k, n) in SHAPES for c in COUNT_SETS]


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


@functools.lru_cache(maxsize=None)
def _case(K, N, counts):
    """Inputs and fp32 oracle for one (K, N, counts); built once, shared by
    every test of that case and never modified."""
    gen = torch.Generator(device="cuda").manual_seed(1000 + K + N + len(counts))
    E, T = len(counts), sum(counts)
    x = _uniform_nonzero((T, K), gen)
    dy = _uniform_nonzero((T, N), gen)
    ws = [_uniform_nonzero((N, K), gen) for _ in range(E)]
    bias = _uniform_nonzero((E, N), gen)
    y = torch.empty(T, N, device="cuda")
    dx = torch.empty(T, K, device="cuda")
    dw = torch.empty(E, N, K, device="cuda")
    db = torch.empty(E, N, device="cuda")
    s = 0
    for e, c in enumerate(counts):
        xe, dye, we = x[s:s + c].float(), dy[s:s + c].float(), ws[e].float()
        y[s:s + c] = xe @ we.t()
        dx[s:s + c] = dye @ we
        dw[e] = dye.t() @ xe
        db[e] = dye.sum(0)
        s += c
    return dict(x=x, dy=dy, ws=ws, bias=bias, off=_offsets(counts), y=y,
                dx=dx, dw=dw, db=db, counts=counts)


def _check(got, ref, what):
    err = (got.float() - ref).abs().max().item() if ref.numel() else 0.0
    scale = max(1.0, ref.abs().max().item() if ref.numel() else 0.0)
    print(f"{what}: max|err|={err:.4g} bound={0.02 * scale:.4g}")
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    assert err < 0.02 * scale, f"{what}: {err} vs {0.02 * scale}"


@pytest.mark.parametrize("K,N,counts", CASES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_fwd(K, N, counts, with_bias):
    c = _case(K, N, counts)
    y = _ext().grouped_gemm_fwd(c["x"], c["ws"], c["off"],
                                c["bias"] if with_bias else None)
    ref = c["y"]
    if with_bias:
        seg = torch.repeat_interleave(
            torch.arange(len(counts), device="cuda"),
            torch.tensor(counts, device="cuda"))
        ref = ref + c["bias"].float()[seg]
    assert y.dtype == torch.bfloat16
    _check(y, ref, "fwd")


@pytest.mark.parametrize("K,N,counts", CASES)
def test_dgrad(K, N, counts):
    c = _case(K, N, counts)
    dx = _ext().grouped_gemm_dgrad(c["dy"], c["ws"], c["off"])
    assert dx.dtype == torch.bfloat16
    _check(dx, c["dx"], "dgrad")


@pytest.mark.parametrize("K,N,counts", CASES)
def test_wgrad_and_db(K, N, counts):
    c = _case(K, N, counts)
    E = len(counts)
    dw, db = _ext().grouped_gemm_wgrad(c["dy"], c["x"], c["off"], E, True)
    assert dw.dtype == torch.bfloat16 and db.dtype == torch.float32
    _check(dw, c["dw"], "wgrad")
    _check(db, c["db"], "db")
    for e, n in enumerate(counts):
        if n == 0:  # empty experts: exact zeros, not garbage
            assert torch.count_nonzero(dw[e]) == 0
            assert torch.count_nonzero(db[e]) == 0
    dw2, db2 = _ext().grouped_gemm_wgrad(c["dy"], c["x"], c["off"], E, False)
    assert torch.equal(dw2, dw) and db2.numel() == 0


@pytest.mark.parametrize("K,N,counts", CASES)
def test_bitwise_repeatable(K, N, counts):
    c, ext, E = _case(K, N, counts), _ext(), len(counts)
    runs = []
    for _ in range(2):
        y = ext.grouped_gemm_fwd(c["x"], c["ws"], c["off"], c["bias"])
        dx = ext.grouped_gemm_dgrad(c["dy"], c["ws"], c["off"])
        dw, db = ext.grouped_gemm_wgrad(c["dy"], c["x"], c["off"], E, True)
        runs.append((y, dx, dw, db))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_zero_rows():
    ext, E, K, N = _ext(), 3, 64, 128
    gen = torch.Generator(device="cuda").manual_seed(5)
    ws = [_uniform_nonzero((N, K), gen) for _ in range(E)]
    off = _offsets((0, 0, 0))
    x = torch.empty(0, K, device="cuda", dtype=torch.bfloat16)
    dy = torch.empty(0, N, device="cuda", dtype=torch.bfloat16)
    assert ext.grouped_gemm_fwd(x, ws, off, None).shape == (0, N)
    assert ext.grouped_gemm_dgrad(dy, ws, off).shape == (0, K)
    dw, db = ext.grouped_gemm_wgrad(dy, x, off, E, True)
    assert dw.shape == (E, N, K) and db.shape == (E, N)
    assert torch.count_nonzero(dw) == 0 and torch.count_nonzero(db) == 0

    from pipegoose_amd.ops.grouped_gemm import grouped_linear
    params = [w.clone().requires_grad_(True) for w in ws]
    xr = x.clone().requires_grad_(True)
    y = grouped_linear(xr, off, params)
    assert y.shape == (0, N)
    y.sum().backward()
    assert xr.grad.shape == (0, K)
    for p in params:
        assert p.grad is not None and torch.count_nonzero(p.grad) == 0


def test_rows_past_int32_elements():
    """T*N > 2^31 elements: addresses must be 64-bit.  Only the last
    expert's few rows (at the far end of the buffers) are compared."""
    ext, K, N, tail = _ext(), 64, 128, 200
    T = (1 << 31) // N + 1000
    gen = torch.Generator(device="cuda").manual_seed(6)
    ws = [_uniform_nonzero((N, K), gen) for _ in range(2)]
    x = torch.full((T, K), 0.5, device="cuda", dtype=torch.bfloat16)
    x[T - tail:] = _uniform_nonzero((tail, K), gen)
    off = torch.tensor([0, T - tail, T], dtype=torch.int32, device="cuda")
    y = ext.grouped_gemm_fwd(x, ws, off, None)
    _check(y[T - tail:], x[T - tail:].float() @ ws[1].float().t(), "fwd-far")
    _check(y[:128], x[:128].float() @ ws[0].float().t(), "fwd-near")


@pytest.mark.parametrize("K,N,E", [(96, 128, 4), (64, 128, 65)])
def test_unsupported_shapes_fall_back(K, N, E):
    from pipegoose_amd.ops.grouped_gemm import grouped_linear, supported
    gen = torch.Generator(device="cuda").manual_seed(7)
    counts = tuple(3 + (e % 4) for e in range(E))
    T = sum(counts)
    x = _uniform_nonzero((T, K), gen).requires_grad_(True)
    ws = [_uniform_nonzero((N, K), gen).requires_grad_(True)
          for _ in range(E)]
    bs = [_uniform_nonzero((N,), gen).requires_grad_(True) for _ in range(E)]
    assert not supported(x, ws)
    y = grouped_linear(x, _offsets(counts), ws, bs)
    g = _uniform_nonzero((T, N), gen)
    y.backward(g)
    s = 0
    for e, c in enumerate(counts):
        xe, ge, we = x[s:s + c].float(), g[s:s + c].float(), ws[e].float()
        _check(y[s:s + c], xe @ we.t() + bs[e].float(), f"y[{e}]")
        _check(x.grad[s:s + c], ge @ we, f"dx[{e}]")
        _check(ws[e].grad, ge.t() @ xe, f"dw[{e}]")
        _check(bs[e].grad, ge.sum(0), f"db[{e}]")
        s += c


def test_autograd_op_matches_oracle():
    """grouped_linear end to end (native path) with biases."""
    from pipegoose_amd.ops.grouped_gemm import grouped_linear, supported
    c = _case(192, 384, COUNT_SETS[0])
    E = len(c["counts"])
    x = c["x"].clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in c["ws"]]
    bs = [c["bias"][e].clone().requires_grad_(True) for e in range(E)]
    assert supported(x, ws)
    y = grouped_linear(x, c["off"], ws, bs)
    y.backward(c["dy"])
    _check(x.grad, c["dx"], "dx")
    for e in range(E):
        _check(ws[e].grad, c["dw"][e], f"dw[{e}]")
        _check(bs[e].grad, c["db"][e], f"db[{e}]")


class _CountingExt:
    """Counts calls into the extension's grouped entry points."""

    def __init__(self, ext):
        self._ext, self.calls = ext, {}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if not name.startswith("grouped_gemm_"):
            return fn

        def counted(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **kw)
        return counted


@pytest.mark.parametrize("topk", [1, 2])
def test_experts_layer_hip_vs_loop(topk, monkeypatch):
    """Experts under PG_MOE_GROUPED=2 vs the default bf16 loop, both
    measured against the loop on fp32 copies of the same parameters: the
    hip path may be at most 2x as far from the oracle as the bf16 loop
    (they differ in summation order and in where the bias is added)."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29893")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    from torch import nn
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.nn.expert_parallel.experts import Experts
    import pipegoose_amd.ops.grouped_gemm as gg

    ctx = ParallelContext.from_torch()
    try:
        torch.manual_seed(19)
        H, I, E, T = 128, 512, 8, 600
        proto = nn.Sequential(nn.Linear(H, I), nn.GELU(), nn.Linear(I, H))
        hip = Experts(E, proto, enable_tensor_parallel=False,
                      parallel_context=ctx).to("cuda", torch.bfloat16)
        # the ParallelContext holds process groups: share it, don't copy
        loop = copy.deepcopy(hip, {id(ctx): ctx})
        oracle = copy.deepcopy(hip, {id(ctx): ctx}).float()
        assert hip._grouped is not None

        x = torch.randn(2, T // 2, H, device="cuda", dtype=torch.bfloat16)
        route = torch.stack([torch.randperm(E, device="cuda")[:topk]
                             for _ in range(T)])
        weight = torch.zeros(T, E, device="cuda")
        weight.scatter_(1, route, torch.rand(T, topk, device="cuda") + 0.1)
        g = torch.randn(2, T // 2, H, device="cuda", dtype=torch.bfloat16)

        def run(mod, mode, dtype):
            xi = x.detach().to(dtype).clone().requires_grad_(True)
            if mode is None:
                os.environ.pop("PG_MOE_GROUPED", None)
            else:
                os.environ["PG_MOE_GROUPED"] = mode
            try:
                out = mod(xi, route, weight.to(dtype))
                out.backward(g.to(dtype))
            finally:
                os.environ.pop("PG_MOE_GROUPED", None)
            res = {"out": out.detach(), "x.grad": xi.grad}
            for name, p in mod.named_parameters():
                assert p.grad is not None, name
                res[name] = p.grad
            return res

        spy = _CountingExt(gg.get_extension(required=True))
        monkeypatch.setattr(gg, "get_extension", lambda required=False: spy)
        r_hip = run(hip, "2", torch.bfloat16)
        monkeypatch.undo()
        # fwd twice, dgrad twice; wgrad twice (two linears)
        assert spy.calls == {"grouped_gemm_fwd": 2, "grouped_gemm_dgrad": 2,
                             "grouped_gemm_wgrad": 2}, spy.calls

        r_loop = run(loop, None, torch.bfloat16)
        r_ref = run(oracle, None, torch.float32)
        errs = {}
        for name, ref in r_ref.items():
            e_hip = (r_hip[name].float() - ref).abs().max().item()
            e_loop = (r_loop[name].float() - ref).abs().max().item()
            print(f"top{topk} {name}: hip {e_hip:.4g} loop {e_loop:.4g}")
            errs[name] = (e_hip, e_loop)
        bad = {n: v for n, v in errs.items() if not v[0] <= 2 * v[1]}
        assert not bad, bad
    finally:
        ctx.destroy()
