"""The fp64 references and input generators of tests/ops/_rowwise_refs.py are
sound: each reference agrees with the torch functional op evaluated in fp64,
every generator yields a finite reference, and every generator yields the tie,
mask and ignore patterns it promises.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as TF

from tests.ops import _rowwise_refs as R

TIGHT = dict(rtol=1e-11, atol=1e-11)


def _leaf(t):
    return t.double().detach().requires_grad_(True)


def test_layer_norm_ref_matches_torch_fp64():
    inp = R.norm_inputs(7, 41, "m0_s1", torch.float32, seed=1)
    ref = R.layer_norm_ref(inp["x"], inp["w"], inp["b"], 1e-5, inp["dy"])
    x, w, b = _leaf(inp["x"]), _leaf(inp["w"]), _leaf(inp["b"])
    y, mean, rstd = torch.native_layer_norm(x, (41,), w, b, 1e-5)
    y.backward(inp["dy"].double())
    for got, want in ((ref["y"], y), (ref["mean"], mean.reshape(-1)),
                      (ref["rstd"], rstd.reshape(-1)), (ref["dx"], x.grad),
                      (ref["dw"], w.grad), (ref["db"], b.grad)):
        assert torch.allclose(got, want.detach(), **TIGHT)


def test_rms_norm_ref_matches_torch_fp64():
    inp = R.norm_inputs(7, 41, "m0_s1", torch.float32, seed=2)
    ref = R.rms_norm_ref(inp["x"], inp["w"], 1e-6, inp["dy"])
    x, w = _leaf(inp["x"]), _leaf(inp["w"])
    y = TF.rms_norm(x, (41,), w, 1e-6)
    y.backward(inp["dy"].double())
    rstd = torch.rsqrt(x.detach().pow(2).mean(-1) + 1e-6)
    for got, want in ((ref["y"], y), (ref["rstd"], rstd), (ref["dx"], x.grad),
                      (ref["dw"], w.grad)):
        assert torch.allclose(got, want.detach(), **TIGHT)


def test_cross_entropy_ref_matches_torch_fp64():
    inp = R.ce_inputs(6, 53, "randn", torch.float32, seed=3)
    targets = inp["targets"].clone()
    targets[2] = -100
    ref = R.cross_entropy_ref(inp["logits"], targets, gscale=inp["gscale"])
    x = _leaf(inp["logits"])
    loss = TF.cross_entropy(x, targets, reduction="none", ignore_index=-100)
    loss.backward(inp["gscale"].double())
    assert torch.allclose(ref["loss"], loss.detach(), **TIGHT)
    assert torch.allclose(ref["grad"], x.grad, **TIGHT)
    assert ref["loss"][2] == 0 and (ref["grad"][2] == 0).all()


def test_cross_entropy_ref_shards_tile_the_row():
    """The reference over a shard uses global ids; the gradient of the full
    row restricted to a shard needs the full row's statistics, so the sharded
    tests compare against the unsharded reference.  Here: vocab_start only
    shifts the ids."""
    inp = R.ce_inputs(5, 43, "randn", torch.float32, seed=4)
    full = R.cross_entropy_ref(inp["logits"], inp["targets"], gscale=inp["gscale"])
    shifted = R.cross_entropy_ref(inp["logits"], inp["targets"] + 100, 100, 143,
                                  gscale=inp["gscale"])
    assert torch.equal(full["loss"], shifted["loss"])
    assert torch.equal(full["grad"], shifted["grad"])


@pytest.mark.parametrize("pos_offset", [0, 37])
def test_rope_ref_matches_complex_rotation_fp64(pos_offset):
    """Against an independent formulation: multiply (x1 + i x2) by e^{i ang}."""
    x = R.rope_input((2, 3, 9, 16), torch.float32, seed=5)
    ref = R.rope_ref(x, 10000.0, pos_offset)
    d = torch.arange(8, dtype=torch.float64)
    freq = torch.tensor(10000.0, dtype=torch.float64) ** (-2.0 * d / 16)
    pos = torch.arange(pos_offset, pos_offset + 9, dtype=torch.float64)
    rot = torch.polar(torch.ones(9, 8, dtype=torch.float64), pos[:, None] * freq)
    z = torch.complex(x[..., :8].double(), x[..., 8:].double()) * rot
    assert torch.allclose(ref, torch.cat([z.real, z.imag], -1), **TIGHT)
    back = R.rope_ref(ref, 10000.0, pos_offset, inverse=True)
    assert torch.allclose(back, x.double(), **TIGHT)


def test_rope_ref_matches_op_cpu_path():
    from pipegoose_amd.ops.rope import _rope_ref
    x = R.rope_input((1, 2, 12, 32), torch.float32, seed=6)
    assert torch.allclose(R.rope_ref(x, 10000.0, 3),
                          _rope_ref(x, 10000.0, 3).double(), atol=1e-5)


@pytest.mark.parametrize("k", [1, 2])
def test_router_ref_matches_torch_fp64(k):
    logits = R.router_logits(40, 9, "randn", torch.float32, seed=7)
    ref = R.router_ref(logits, k)
    probs = torch.softmax(logits.double(), -1)
    val, idx = probs.topk(k, dim=-1)
    assert not R.router_tied(logits, k).any()
    assert torch.allclose(ref["probs"], probs, **TIGHT)
    assert torch.equal(ref["idx"], idx)
    assert torch.allclose(ref["val"], val, **TIGHT)
    assert torch.allclose(ref["colsum"], probs.sum(0), **TIGHT)
    assert torch.allclose(ref["lse"], torch.logsumexp(logits.double(), -1), **TIGHT)
    assert torch.equal(ref["count"], torch.bincount(idx[:, 0], minlength=9))


def test_router_ref_lowest_index_wins():
    logits = torch.tensor([[1.0, 3.0, 3.0, 3.0], [2.0, 2.0, 5.0, 2.0],
                           [0.0, 1.0, 2.0, 3.0]])
    ref = R.router_ref(logits, 2)
    assert ref["idx"].tolist() == [[1, 2], [2, 0], [3, 2]]
    assert R.router_tied(logits, 2).tolist() == [[True, True], [False, True],
                                                 [False, False]]
    assert ref["count"].tolist() == [0, 1, 1, 1]


# ------------------------------------------------------- generators are sound
def _norm_cases(extra=False):
    fams = dict(R.NORM_FAMILIES, **(R.RMS_EXTRA_FAMILIES if extra else {}))
    return [(N, H, f, dt) for (N, H) in R.NORM_SHAPES
            for f, (_, _, dts) in fams.items() for dt in dts]


@pytest.mark.parametrize("N,H,family,dtype", _norm_cases(extra=True))
def test_norm_generators_finite_and_as_promised(N, H, family, dtype):
    inp = R.norm_inputs(N, H, family, dtype)
    assert all(v.numel() * v.element_size() < 2 ** 20 for v in inp.values())
    mean, std, _ = {**R.NORM_FAMILIES, **R.RMS_EXTRA_FAMILIES}[family]
    s = inp["x_res"] + inp["r"]
    for x in (inp["x"], s):
        xd = x.double()
        # rounding to dtype moves an element by at most half a spacing
        half = 0.5 * R.ulp_out(dtype, max(abs(mean), 4 * std)) + 1e-300
        assert (xd.mean(-1) - mean).abs().max() <= 0.5 * std + 2 * half
        if std == 0.0:
            assert (xd == mean).all()
        else:
            # bf16 is spaced 4 apart at 1000: such a row may round to a constant
            assert (xd.std(-1) > 0).all() or 2 * half > std
            assert (xd.std(-1) <= 1.5 * std + 2 * half).all()
        if family in R.NORM_FAMILIES:
            ref = R.layer_norm_ref(x, inp["w"], inp["b"], 1e-5, inp["dy"])
            assert all(torch.isfinite(v).all() for v in ref.values())
            assert (ref["rstd"] > 0).all()
        ref = R.rms_norm_ref(x, inp["w"], 1e-6, inp["dy"])
        assert all(torch.isfinite(v).all() for v in ref.values())
        assert (ref["rstd"] > 0).all()


@pytest.mark.parametrize("N,V", R.CE_SHAPES)
@pytest.mark.parametrize("family", R.CE_FAMILIES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ce_generators_finite_and_as_promised(N, V, family, dtype):
    inp = R.ce_inputs(N, V, family, dtype)
    x, t = inp["logits"], inp["targets"]
    body_end = V - V % 8
    assert (t == 0).any() and (t >= body_end).any()
    assert ((t > 0) & (t < body_end)).any()
    assert (inp["gscale"] > 0).all()
    if family == "neg_inf":
        masked = torch.isinf(x)
        frac = masked.double().mean(-1)
        assert (frac > 0.05).all() and (frac < 0.15).all()
        assert not masked.gather(-1, t[:, None]).any()      # never the target
        assert masked[:, 8].all()            # first element of a thread's packet
        assert torch.isfinite(x[~masked]).all()
    else:
        assert torch.isfinite(x).all()
    if family == "equal_row":
        assert (x[1] == x[1, 0]).all()
    ref = R.cross_entropy_ref(x, t, gscale=inp["gscale"])
    assert torch.isfinite(ref["loss"]).all() and torch.isfinite(ref["grad"]).all()
    if family == "equal_row":
        assert abs(ref["loss"][1].item() - math.log(V)) < 1e-12
    if family == "neg_inf":
        assert (ref["grad"][torch.isinf(x)] == 0).all()
    # with ignored rows: loss and gradient exactly zero there
    ti = t.clone()
    ti[1::2] = -100
    ref = R.cross_entropy_ref(x, ti, gscale=inp["gscale"])
    assert (ref["loss"][1::2] == 0).all() and (ref["grad"][1::2] == 0).all()
    assert (ref["loss"][0::2] > 0).all()


@pytest.mark.parametrize("D", R.ROPE_DIMS)
@pytest.mark.parametrize("pos_offset", R.ROPE_OFFSETS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_generator_finite(D, pos_offset, dtype):
    x = R.rope_input((1, 2, 64, D), dtype)
    y = R.rope_ref(x, 10000.0, pos_offset)
    assert torch.isfinite(y).all()
    # a rotation: pair norms are kept
    h = D // 2
    n_in = x.double()[..., :h] ** 2 + x.double()[..., h:] ** 2
    n_out = y[..., :h] ** 2 + y[..., h:] ** 2
    assert torch.allclose(n_in, n_out, **TIGHT)


def test_rope_offsets_straddle_the_hardware_sine_domain():
    """256 revolutions = 1608.5 rad: the offsets put 64 positions below,
    across and above it."""
    lim = 256 * 2 * math.pi
    assert 1500 + 63 < lim
    assert 1580 < lim < 1580 + 63
    assert all(o > lim for o in (4096, 32704))
    assert 32704 + 64 == 32768


@pytest.mark.parametrize("N,E", R.ROUTER_SHAPES)
@pytest.mark.parametrize("family", R.ROUTER_FAMILIES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_router_generators_finite_and_as_promised(N, E, family, dtype):
    x = R.router_logits(N, E, family, dtype)
    assert torch.isfinite(x).all()
    xd = x.double()
    spread = (xd.max(-1).values - xd.min(-1).values).max().item()
    assert spread < R.ROUTER_SPREAD
    if family == "snapped":
        assert (xd * 2 == torch.round(xd * 2)).all()
    if family == "randn15" and E > 1:
        assert spread > 15.0
    for k in (1, 2):
        if k > E:
            continue
        ref = R.router_ref(x, k)
        assert all(torch.isfinite(v.double()).all() for v in ref.values())
        assert (ref["probs"] > 0).all()             # nothing underflows
        assert ref["count"].sum().item() == N
        if k == 2:
            assert (ref["idx"][:, 0] != ref["idx"][:, 1]).all()
        tied = R.router_tied(x, k)
        if family == "snapped" and E >= 8:
            assert tied[:, 0].any()                 # exact ties at the top
        if dtype == torch.bfloat16 and N * E > 30000:
            assert tied.any()                       # bf16: ties without snapping
        # the lowest-index rule, checked against the definition
        top = xd.gather(-1, ref["idx"][:, :1])
        assert (top == xd.max(-1, keepdim=True).values).all()
        lowest = torch.where(xd == top, torch.arange(E).expand(N, E),
                             torch.full((N, E), E)).min(-1).values
        assert torch.equal(ref["idx"][:, 0], lowest)
