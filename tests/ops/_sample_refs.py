"""Plain helpers for the sampling tests: an fp64 reference of the semantics in
pipegoose_amd/ops/sampling.py, a builder of bf16 rows whose outcome is far
from every rounding decision, and the case table both test files share."""
import math

import numpy as np
import torch

MARGIN = 1e-3   # see exact_cases
NEG_INF = float("-inf")
ALMOST_ONE = float(np.nextafter(np.float32(1), np.float32(0)))


def split_chunk(V, splits):
    """The chunk length of ``sample_logits(..., splits=splits)``."""
    return -(-(-(-V // splits)) // 8) * 8


def head_indices(V):
    """0, V-1, either side of an 8-element boundary and of both chunk
    boundaries of ``splits=3``."""
    chunk = split_chunk(V, 3)
    cand = [0, V - 1, 7, 8, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk]
    return sorted({i for i in cand if 0 <= i < V})


def make_row(V, heads, tail_top=None, seed=0):
    """bf16 [V]: ``heads`` {index: logit}; everything else a random tail in
    ``[tail_top - 4, tail_top]`` (default: 6 + ln V below the lowest head, so
    that the whole tail weighs under e^-6 of it at T = 1) with some -inf."""
    g = torch.Generator().manual_seed(seed)
    if tail_top is None:
        tail_top = min(heads.values()) - 6.0 - math.log(V)
    row = tail_top - 4.0 * torch.rand(V, generator=g, dtype=torch.float64)
    row[torch.rand(V, generator=g) < 1 / 16] = NEG_INF
    for i, z in heads.items():
        row[i] = z
    return row.to(torch.bfloat16)


def default_heads(V, top=10.0, gap=0.5):
    idx = head_indices(V)
    n = len(idx)            # 1, 2 or 8: 3 * i % n permutes them
    return {j: top - gap * (3 * i % n) for i, j in enumerate(idx)}


def reference(row, T, k, p):
    """fp64.  Returns (keep [V] bool, lo [V], hi [V], margin): the kept set,
    every token's interval of the normalised CDF in index order, and the
    distance of ``top_p`` from the nearest cumulative mass it is compared
    with."""
    z = row.double()
    V = z.numel()
    w = torch.exp((z - z.max()) / T)
    zs, order = z.sort(descending=True, stable=True)
    t_k = float(zs[k - 1]) if 0 < k < V else NEG_INF
    w = w * (z >= t_k)
    t_p, margin = NEG_INF, math.inf
    if p < 1:
        cum = w[order].cumsum(0)
        ends = torch.ones(V, dtype=torch.bool)
        ends[:-1] = zs[:-1] != zs[1:]
        mass = cum[ends] / w.sum()          # mass(z >= t), one per value t
        j = int((mass >= p).nonzero()[0])
        t_p = float(zs[ends][j])
        margin = float((mass - p).abs().min())
    keep = (z >= max(t_k, t_p)) & (z > NEG_INF)
    kw = w * keep
    hi = kw.cumsum(0) / kw.sum()
    return keep, hi - kw / kw.sum(), hi, margin


def exact_cases(row, heads, T, k, p):
    """(u fp32 [n], expected token [n]): the midpoint of every kept head's
    interval, u = 0 and u = nextafter(1, 0).

    Asserts, on the reference alone, that every interval used is at least
    MARGIN wide and that top_p is MARGIN away from the masses it is compared
    with.  With fixed-point masses the kernel's CDF is off by at most
    V * 2^-41 plus a few ulp of exp2f per term (1e-7 relative); an fp32
    cumsum over 2^18 terms stays near 1e-6: 1000x below MARGIN."""
    keep, lo, hi, margin = reference(row, T, k, p)
    assert margin >= MARGIN, f"top_p sits {margin} from a cumulative mass"
    us, want = [], []
    for j in heads:
        if keep[j]:
            us.append(float(lo[j] + hi[j]) / 2)
            want.append(j)
    for u in (0.0, ALMOST_ONE):
        us.append(u)
        want.append(int((hi > u).nonzero()[0]))
    for j in want:
        assert hi[j] - lo[j] >= MARGIN, f"token {j}: interval too narrow"
    return torch.tensor(us, dtype=torch.float32), torch.tensor(want)


def _case(V, T=1.0, k=0, p=1.0, heads=None, **row):
    heads = default_heads(V) if heads is None else heads
    return make_row(V, heads, **row), heads, T, k, p


def _spread(V, values):
    """``values`` on the first head indices of V."""
    return dict(zip(head_indices(V), values))


# name -> (row, heads, T, k, p); one axis at a time
CASES = {
    **{f"V{V}": _case(V) for V in (1, 7, 255, 257, 4104, 250880)},
    "T0.7_k5": _case(4104, 0.7, 5),
    "p0.9": _case(4104, 1.0, 0, 0.9),
    "T1.3_k50_p0.8": _case(4104, 1.3, 50, 0.8),
    "T0.05": _case(4104, 0.05,      # bf16 neighbours: 1.25 apart after 1/T
                   heads=_spread(4104, [9.875, 10.0, 9.8125, 9.9375])),
    "T100_p0.95": _case(257, 100.0, 0, 0.95),
    "k1": _case(4104, 1.0, 1),
    "k_above_V": _case(4104, 1.0, 4104 + 3),
    "tie_at_kth": _case(4104, 1.0, 3,
                        heads=_spread(4104, [9.0, 10.0, 9.0, 8.0, 9.5, 9.0])),
    "tie_at_top_p": _case(4104, 1.0, 0, 0.7,
                          heads=_spread(4104, [9.0, 8.0, 10.0, 9.0])),
    "extreme": _case(4104, heads=_spread(4104, [3e38] * 8), tail_top=-3e38),
}
