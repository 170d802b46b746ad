"""Token sampling: temperature, top-k and top-p with per-row parameters.

``sample_logits(logits [R, V], u [R], temperature, top_k, top_p) -> int64 [R]``
picks one token per row.  With ``z`` the row's logits and ``T`` its
temperature:

- ``T == 0`` (greedy): the lowest index of the row maximum; ``u``, ``top_k``
  and ``top_p`` are ignored.  A batch may mix greedy and sampled rows.
- otherwise the weights are ``w_i = exp((z_i - z_max) / T)``;
- top-k keeps ``z_i >= t_k``, the k-th largest logit value — every token tied
  at the threshold survives; ``top_k <= 0`` or ``>= V`` turns it off;
- top-p is applied after top-k, on the survivors: ``t_p`` is the largest logit
  value ``t`` with ``mass(z_i >= t) >= top_p * mass(survivors)``; ties at the
  threshold are kept, the row maximum is always kept, ``top_p >= 1`` turns it
  off;
- the kept set is ``z_i >= max(t_k, t_p)`` with total weight ``M``, and the
  token is the smallest index ``j`` whose running kept weight **in vocabulary
  index order** exceeds ``u * M`` (the last kept index if rounding leaves
  none).  ``u`` is uniform in [0, 1).

``-inf`` logits are never kept.  Rows that hold NaN or are all ``-inf`` are
unspecified (the result is some index in ``[0, V)``).

GPU, bf16 contiguous logits: one HIP sampler (csrc/sampling.hip) — radix
selection of the thresholds on 16-bit keys, fixed-point masses that make the
token independent of ``splits`` and of scheduling, no host sync, capturable
into a hipGraph.  ``splits`` cuts a row into that many chunks of
``ceil(ceil(V / splits) / 8) * 8`` elements (0: a plan from the shapes).
fp32 / fp16 logits, the CPU and ``PIPEGOOSE_DISABLE_EXT=1`` run the torch
reference below with the same semantics in fp32.
"""
import os

import torch

from pipegoose_amd.ops import get_extension


def _per_row(x, rows: int, dtype, device) -> torch.Tensor:
    if torch.is_tensor(x):
        assert x.numel() == rows, f"expected one value per row ({rows})"
        return x.to(device=device, dtype=dtype).reshape(rows).contiguous()
    return torch.full((rows,), x, dtype=dtype, device=device)


def _first_true(cond: torch.Tensor) -> torch.Tensor:
    """Lowest index at which ``cond [R, V]`` holds, V where it never does."""
    V = cond.size(-1)
    idx = torch.arange(V, device=cond.device).expand_as(cond)
    return torch.where(cond, idx, V).min(-1).values


def _sample_ref(logits, u, temperature, top_k, top_p) -> torch.Tensor:
    z = logits.float()
    R, V = z.shape
    neg_inf = float("-inf")
    zmax = z.max(-1, keepdim=True).values
    greedy = ~(temperature > 0)
    T = torch.where(greedy, torch.ones_like(temperature), temperature)[:, None]

    zs = z.sort(-1, descending=True).values
    k_on = (top_k > 0) & (top_k < V)
    kth = torch.where(k_on, top_k, V).long().clamp(1, V) - 1
    t_k = zs.gather(1, kth[:, None])                        # [R, 1]

    # mass(z >= t) for t = zs[j] is the running sum at the END of j's run of
    # equal values
    ws = torch.exp((zs - zmax) / T) * (zs >= t_k)
    cum = ws.cumsum(-1)
    run_end = torch.ones_like(zs, dtype=torch.bool)
    run_end[:, :-1] = zs[:, :-1] != zs[:, 1:]
    reached = run_end & (cum > 0) & (cum >= top_p[:, None] * cum[:, -1:])
    at = _first_true(reached).clamp(max=V - 1)
    t_p = zs.gather(1, at[:, None])
    t_p = torch.where((top_p < 1)[:, None], t_p, torch.full_like(t_p, neg_inf))

    keep = (z >= torch.maximum(t_k, t_p)) & (z > neg_inf)
    kw = torch.exp((z - zmax) / T) * keep
    run = kw.cumsum(-1)
    tok = _first_true(run > u[:, None] * run[:, -1:])
    last = V - 1 - _first_true(keep.flip(-1))
    tok = torch.where(tok < V, tok, last)
    tok = torch.where(greedy, _first_true(z == zmax), tok)
    return tok.clamp(0, V - 1)


def sample_logits(logits: torch.Tensor, u: torch.Tensor, temperature=1.0,
                  top_k=0, top_p=1.0, splits: int = 0) -> torch.Tensor:
    """One token per row of ``logits [R, V]`` (module docstring).  ``u`` holds
    one uniform per row; ``temperature``, ``top_k`` and ``top_p`` are scalars
    or tensors with one value per row."""
    assert logits.dim() == 2, "logits must be [R, V]"
    R, dev = logits.size(0), logits.device
    u = _per_row(u, R, torch.float32, dev)
    temperature = _per_row(temperature, R, torch.float32, dev)
    top_k = _per_row(top_k, R, torch.int32, dev)
    top_p = _per_row(top_p, R, torch.float32, dev)
    if (logits.is_cuda and logits.dtype == torch.bfloat16
            and os.environ.get("PIPEGOOSE_DISABLE_EXT") != "1"):
        ext = get_extension(required=True)
        return ext.sample_logits(logits.contiguous(), u, temperature, top_k,
                                 top_p, splits)
    return _sample_ref(logits, u, temperature, top_k, top_p)
