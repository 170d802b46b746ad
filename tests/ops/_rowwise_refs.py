"""fp64 references, seeded input generators and the comparison helper for the
row-wise kernels (LayerNorm, residual-LayerNorm, RMSNorm, cross-entropy, RoPE,
router).  Plain helpers: imported by test_rowwise_refs_cpu.py (which checks
that the references and generators are sound) and test_rowwise_edges_gpu.py.

Every reference is written out explicitly in float64 from the definition of
the operation; none calls the torch functional op it stands in for.
"""
import math

import torch

EPS_OUT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8}
F_DEFAULT = 4.0
F_MAX = 16.0


# ------------------------------------------------------------------ comparison
def ulp_out(dtype, magnitude: float) -> float:
    """Spacing of ``dtype`` at ``magnitude``: 2^-23 (fp32) or 2^-8 (bf16) times
    the power of two at or below it."""
    if magnitude == 0.0 or not math.isfinite(magnitude):
        return 0.0
    return EPS_OUT[dtype] * 2.0 ** math.floor(math.log2(magnitude))


RATIOS = {}     # kernel name -> (largest measured ratio, case that gave it)


def check_close(kernel, what, got, base, ref, out_dtype, F=F_DEFAULT):
    """Assert  max|got - ref| <= F * max|base - ref| + 2 * ulp_out(max|ref|).

    got: the kernel's output; base: the stock torch result on the same inputs
    in the same dtype; ref: the fp64 reference.  Prints, and returns, the
    measured ratio: the smallest F with which the assertion would hold."""
    assert F <= F_MAX
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    base = base.detach().double().cpu()
    assert got.shape == ref.shape and base.shape == ref.shape, \
        (what, got.shape, base.shape, ref.shape)
    assert torch.isfinite(ref).all(), f"{what}: reference is not finite"
    assert torch.isfinite(got).all(), f"{kernel} {what}: kernel output is not finite"
    if ref.numel() == 0:
        return 0.0
    err = (got - ref).abs().max().item()
    base_err = (base - ref).abs().max().item()
    floor = 2.0 * ulp_out(out_dtype, ref.abs().max().item())
    over = max(0.0, err - floor)
    ratio = 0.0 if over == 0.0 else (over / base_err if base_err > 0 else math.inf)
    print(f"[ratio] {kernel} {what}: err={err:.3e} base={base_err:.3e} "
          f"floor={floor:.3e} ratio={ratio:.3g} (F={F:g})")
    if ratio > RATIOS.get(kernel, (-1.0, ""))[0]:
        RATIOS[kernel] = (ratio, what)
    assert err <= F * base_err + floor, \
        f"{kernel} {what}: err {err:.3e} > {F:g} * {base_err:.3e} + {floor:.3e} (ratio {ratio:.3g})"
    return ratio


# ------------------------------------------------------------------ references
def layer_norm_ref(x, w, b, eps, dy=None):
    """x [N, H], w/b [H] -> dict of float64 y, mean, rstd (+ dx, dw, db)."""
    xd, wd, bd = x.double(), w.double(), b.double()
    H = xd.size(-1)
    mean = xd.sum(-1, keepdim=True) / H
    xc = xd - mean
    var = (xc * xc).sum(-1, keepdim=True) / H
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = xc * rstd
    out = {"y": xhat * wd + bd, "mean": mean.squeeze(-1), "rstd": rstd.squeeze(-1)}
    if dy is not None:
        dyd = dy.double()
        dyw = dyd * wd
        c1 = dyw.sum(-1, keepdim=True) / H
        c2 = (dyw * xhat).sum(-1, keepdim=True) / H
        out["dx"] = rstd * (dyw - c1 - xhat * c2)
        out["dw"] = (dyd * xhat).sum(0)
        out["db"] = dyd.sum(0)
    return out


def rms_norm_ref(x, w, eps, dy=None):
    """x [N, H], w [H] -> dict of float64 y, rstd (+ dx, dw)."""
    xd, wd = x.double(), w.double()
    H = xd.size(-1)
    rstd = 1.0 / torch.sqrt((xd * xd).sum(-1, keepdim=True) / H + eps)
    xhat = xd * rstd
    out = {"y": xhat * wd, "rstd": rstd.squeeze(-1)}
    if dy is not None:
        dyd = dy.double()
        dyw = dyd * wd
        c = (dyw * xhat).sum(-1, keepdim=True) / H
        out["dx"] = rstd * (dyw - xhat * c)
        out["dw"] = (dyd * xhat).sum(0)
    return out


def cross_entropy_ref(logits, targets, vocab_start=0, vocab_end=None, gscale=None):
    """Per-row loss over the FULL row of ``logits`` [N, V] (global vocab ids
    ``vocab_start + column``), targets [N]; a negative target is ignored: loss
    0 and gradient 0.  With ``gscale`` [N] also the gradient
    (softmax - onehot) * gscale.  ``-inf`` logits have probability 0."""
    xd = logits.double()
    N, V = xd.shape
    if vocab_end is None:
        vocab_end = vocab_start + V
    assert vocab_end - vocab_start == V
    m = xd.max(-1, keepdim=True).values
    e = torch.exp(xd - m)
    s = e.sum(-1, keepdim=True)
    valid = targets >= 0
    local = (targets - vocab_start).clamp(0, V - 1)
    assert ((targets[valid] >= vocab_start) & (targets[valid] < vocab_end)).all()
    t = xd.gather(-1, local[:, None])
    loss = (torch.log(s) - (t - m)).squeeze(-1)
    out = {"loss": torch.where(valid, loss, torch.zeros_like(loss))}
    if gscale is not None:
        onehot = torch.zeros_like(xd)
        onehot.scatter_(-1, local[:, None], 1.0)
        grad = (e / s - onehot) * gscale.double()[:, None]
        out["grad"] = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return out


def rope_ref(x, theta_base, pos_offset=0, inverse=False):
    """Half-split RoPE on [B, H, S, D] with the angle formed in float64."""
    xd = x.double()
    S, D = xd.shape[-2:]
    half = D // 2
    d = torch.arange(half, device=x.device, dtype=torch.float64)
    freq = torch.exp(-2.0 * d / D * math.log(theta_base))
    pos = torch.arange(pos_offset, pos_offset + S, device=x.device,
                       dtype=torch.float64)
    ang = pos[:, None] * freq
    cos, sin = torch.cos(ang), torch.sin(ang)
    if inverse:
        sin = -sin
    x1, x2 = xd[..., :half], xd[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def router_ref(logits, k):
    """logits [N, E] -> float64 probs, top-k (idx, val) where among equal
    logits the lowest index wins, colsum, top-1 count, lse."""
    xd = logits.double()
    N, E = xd.shape
    m = xd.max(-1, keepdim=True).values
    e = torch.exp(xd - m)
    s = e.sum(-1, keepdim=True)
    probs = e / s
    lse = (m + torch.log(s)).squeeze(-1)
    ar = torch.arange(E, device=xd.device).expand(N, E)
    work = xd.clone()
    idx = []
    for _ in range(k):
        is_max = work == work.max(-1, keepdim=True).values
        pick = torch.where(is_max, ar, torch.full_like(ar, E)).min(-1).values
        idx.append(pick)
        work.scatter_(-1, pick[:, None], -math.inf)
    idx = torch.stack(idx, -1)
    return {"probs": probs, "idx": idx, "val": probs.gather(-1, idx),
            "colsum": probs.sum(0),
            "count": torch.bincount(idx[:, 0], minlength=E), "lse": lse}


def router_tied(logits, k):
    """[N, k] bool: the logit at rank kk (descending) equals a neighbour in
    rank, so the index at that rank is decided by the lowest-index rule."""
    v = logits.double().sort(-1, descending=True).values
    E = v.size(-1)
    cols = []
    for kk in range(k):
        tie = torch.zeros(v.size(0), dtype=torch.bool, device=v.device)
        if kk > 0:
            tie |= v[:, kk] == v[:, kk - 1]
        if kk + 1 < E:
            tie |= v[:, kk] == v[:, kk + 1]
        cols.append(tie)
    return torch.stack(cols, -1)


# ------------------------------------------------------------------ generators
# All draws are float64 on the CPU from a seeded generator, then rounded to
# the dtype under test, so a case is the same tensor on every machine.
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


NORM_SHAPES = [(5, 1001), (3, 40), (2, 8204), (64, 1024)]

# name -> (row mean, row std, dtypes)
_BOTH = (torch.float32, torch.bfloat16)
NORM_FAMILIES = {
    "m0_s1": (0.0, 1.0, _BOTH),
    "m100_s1": (100.0, 1.0, _BOTH),
    "m1000_s1": (1000.0, 1.0, _BOTH),
    "const100": (100.0, 0.0, _BOTH),
    "m100_s1e-3": (100.0, 1e-3, (torch.float32,)),
    "m30_s1e-2": (30.0, 1e-2, (torch.float32,)),
}
RMS_EXTRA_FAMILIES = {
    "m0_s1e-3": (0.0, 1e-3, _BOTH),
    "m0_s1e3": (0.0, 1e3, _BOTH),
}


def norm_inputs(N, H, family, dtype, seed=0):
    """x, r, w, b, dy for the norm kernels.  x has the family's row mean and
    std; r is a small zero-mean residual (exactly 0 for constant rows) and
    x_res = x - r, so that x_res + r has the family's distribution too."""
    mean, std, dtypes = {**NORM_FAMILIES, **RMS_EXTRA_FAMILIES}[family]
    assert dtype in dtypes
    g = _gen(seed)
    x = mean + std * _randn((N, H), g)
    r = 0.5 * std * _randn((N, H), g)
    return {"x": x.to(dtype), "r": r.to(dtype), "x_res": (x - r).to(dtype),
            "w": _randn((H,), g).to(dtype), "b": _randn((H,), g).to(dtype),
            "dy": _randn((N, H), g).to(dtype)}


CE_SHAPES = [(5, 1003), (5, 4099)]
CE_FAMILIES = ["randn", "randn30", "equal_row", "neg_inf"]


def ce_targets(N, V):
    """Targets with the true class at index 0, in the 8-wide vector body, and
    in the scalar tail (the last V % 8 columns), repeating over the rows."""
    tail = V - (V % 8)
    assert V % 8 >= 2
    pattern = [0, 17, V - 1, tail, V // 2 - 3]
    return torch.tensor([pattern[i % len(pattern)] for i in range(N)],
                        dtype=torch.int64)


def ce_inputs(N, V, family, dtype, seed=0):
    """logits [N, V] in dtype, targets [N], gscale [N] (fp32)."""
    g = _gen(seed)
    targets = ce_targets(N, V)
    x = _randn((N, V), g)
    if family == "randn30":
        x = 30.0 * x
    elif family == "equal_row":
        x[1, :] = 3.0
    elif family == "neg_inf":
        mask = torch.rand((N, V), generator=g, dtype=torch.float64) < 0.1
        # also an element that opens a thread's 8-wide packet
        mask[:, 8] = True
        mask[:, 16] = True
        mask.scatter_(-1, targets[:, None], False)
        x = x.masked_fill(mask, -math.inf)
    else:
        assert family == "randn"
    # exact in bf16, so that the stock op in bf16 scales by the same numbers
    gscale = (0.5 + torch.rand((N,), generator=g, dtype=torch.float64)) \
        .bfloat16().float()
    return {"logits": x.to(dtype), "targets": targets, "gscale": gscale}


ROPE_DIMS = [64, 80, 128, 256]
ROPE_OFFSETS = [0, 1500, 1580, 4096, 32704]


def rope_input(shape, dtype, seed=0):
    return _randn(shape, _gen(seed)).to(dtype)


ROUTER_SHAPES = [(4097, 8), (37, 64), (50, 3), (33, 1), (64, 60)]
ROUTER_FAMILIES = ["randn", "snapped", "randn15"]
ROUTER_SPREAD = 60.0


def router_logits(N, E, family, dtype, seed=0):
    x = _randn((N, E), _gen(seed))
    if family == "snapped":
        x = torch.round(x * 2.0) / 2.0          # multiples of 0.5: exact ties
    elif family == "randn15":
        # spread of every row under ROUTER_SPREAD: no probability underflows
        x = (15.0 * x).clamp(-29.0, 29.0)
    else:
        assert family == "randn"
    return x.to(dtype)
