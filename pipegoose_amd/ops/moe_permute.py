"""Sync-free MoE dispatch/combine around the grouped expert GEMMs.

``N`` tokens, router fan-out ``k``, ``S = N*k`` *slots*; slot ``s = t*k + j``
is token ``t``'s ``j``-th choice.  ``route_plan`` sorts the kept slots by
(local expert, slot) -- a stable counting sort, the order
``torch.argsort(stable=True)`` gives -- into the first ``M`` rows of a fixed
``S``-row buffer and returns

    offsets      int32 [E+1]  first row of each local expert, offsets[E] = M
    row_of_slot  int32 [S]    row of slot s, -1 when the slot was dropped
    slot_of_row  int32 [S]    slot at row r, -1 for the dead rows r >= M

``permute(x, plan)`` gathers the token rows into that buffer (dead rows are
zeros) and ``combine(ys, gates, plan)`` sums each token's gate-weighted
expert outputs back (fp32 accumulate in ascending ``j``, one rounding).
Both are differentiable and go through the plan only, so rows ``>= M`` of
anything computed in between are never read.

On gfx950 with bf16 rows all five functions are kernels of
csrc/moe_permute.hip: no host read-back, no atomics, no fp32 ``[N,H]``
scratch, bitwise repeatable.  Everything else (CPU, other dtypes) runs the
``*_reference`` functions below, which have identical semantics -- fixed
``S``-row buffer, ``-1`` conventions, zeroed dead rows -- but may
synchronise the host.
"""
from typing import NamedTuple, Optional

import torch

from pipegoose_amd.ops import get_extension

MAX_EXPERTS = 64  # the plan kernel matches expert ids on six ballot bits


class RoutePlan(NamedTuple):
    offsets: torch.Tensor       # int32 [E+1]
    row_of_slot: torch.Tensor   # int32 [S]
    slot_of_row: torch.Tensor   # int32 [S]
    num_tokens: int             # N
    k: int                      # router fan-out


def supported(x: torch.Tensor, num_local: int = 1) -> bool:
    """True when the native kernels take rows like ``x``: a 2-D bf16 device
    tensor with H % 8 == 0, and 1 <= E <= 64 local experts.  On such inputs
    a missing extension is an error, not a reason to fall back."""
    if num_local < 1 or num_local > MAX_EXPERTS:
        return False
    if not x.is_cuda or x.dim() != 2 or x.dtype != torch.bfloat16:
        return False
    if x.size(1) == 0 or x.size(1) % 8:
        return False
    get_extension(required=True)
    return True


def _plan_native(order: torch.Tensor, weight, num_local: int) -> bool:
    if not order.is_cuda or num_local < 1 or num_local > MAX_EXPERTS:
        return False
    if weight is not None and (
            not weight.is_cuda
            or weight.dtype not in (torch.bfloat16, torch.float32)):
        return False
    get_extension(required=True)
    return True


# ------------------------------------------------------------- reference
def route_plan_reference(order: torch.Tensor, weight: Optional[torch.Tensor],
                         expert_offset: int, num_local: int):
    """(offsets, row_of_slot, slot_of_row) in eager torch (synchronises)."""
    N, k = order.shape
    S, dev = N * k, order.device
    ids = order.reshape(-1).to(torch.int64)
    keep = (ids >= expert_offset) & (ids < expert_offset + num_local)
    if weight is not None:
        e_tot = weight.size(-1)
        # range first: a bad id is a dropped slot, never an index
        keep = keep & (ids >= 0) & (ids < e_tot)
        tok = torch.arange(S, device=dev) // k
        w = weight.reshape(N, e_tot)[tok, ids.clamp(0, max(e_tot - 1, 0))]
        keep = keep & (w > 0)           # NaN > 0 is False
    slots = keep.nonzero(as_tuple=True)[0]
    local = ids[slots] - expert_offset
    slots = slots[torch.argsort(local, stable=True)]
    M = slots.numel()
    slot_of_row = torch.full((S,), -1, dtype=torch.int32, device=dev)
    slot_of_row[:M] = slots.to(torch.int32)
    row_of_slot = torch.full((S,), -1, dtype=torch.int32, device=dev)
    row_of_slot[slots] = torch.arange(M, dtype=torch.int32, device=dev)
    offsets = torch.zeros(num_local + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(
        torch.bincount(local, minlength=num_local), 0).to(torch.int32)
    return offsets, row_of_slot, slot_of_row


def _acc_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.promote_types(dtype, torch.float32)


def _valid(idx: torch.Tensor, bound: int) -> torch.Tensor:
    return (idx >= 0) & (idx < bound)


def permute_fwd_reference(x, slot_of_row, k):
    S = x.size(0) * k
    xs = x.new_zeros(S, x.size(1))
    live = _valid(slot_of_row, S)
    xs[live] = x[slot_of_row[live].long() // k]
    return xs


def _gather_sum_reference(src, gates, row_of_slot, N, k):
    S = N * k
    acc = torch.zeros(N, src.size(1), device=src.device,
                      dtype=_acc_dtype(src.dtype))
    rows = row_of_slot.reshape(N, k).long()
    for j in range(k):                      # ascending j, one rounding
        ok = _valid(rows[:, j], S)
        term = src[rows[ok, j]].to(acc.dtype)
        if gates is not None:
            g = gates.reshape(N, k)[ok, j].to(acc.dtype)
            term = g.unsqueeze(-1) * term
        acc[ok] += term
    return acc.to(src.dtype)


def permute_bwd_reference(dxs, row_of_slot, N, k):
    return _gather_sum_reference(dxs, None, row_of_slot, N, k)


def combine_fwd_reference(ys, gates, row_of_slot, N, k):
    return _gather_sum_reference(ys, gates, row_of_slot, N, k)


def combine_bwd_reference(dout, ys, gates, slot_of_row, k, want_dgate=True):
    S = dout.size(0) * k
    acc = _acc_dtype(dout.dtype)
    live = _valid(slot_of_row, S)
    slots = slot_of_row[live].long()
    d = dout[slots // k].to(acc)
    dys = torch.zeros_like(ys)
    if gates is None:
        dys[live] = d.to(dout.dtype)
    else:
        dys[live] = (gates[slots].to(acc).unsqueeze(-1) * d).to(dout.dtype)
    if not want_dgate:
        return dys, dout.new_empty(0, dtype=acc)
    dgate = torch.zeros(S, device=dout.device, dtype=acc)
    dgate[slots] = (d * ys[live].to(acc)).sum(-1)
    return dys, dgate


# ---------------------------------------------------------------- public
def route_plan(order: torch.Tensor, weight: Optional[torch.Tensor],
               expert_offset: int, num_local: int) -> RoutePlan:
    """order: int64 [N,k] (or [N]) global expert ids; weight: None or
    [N, E_tot] routing weights (bf16 or fp32).  A slot is kept iff its id is
    in ``[expert_offset, expert_offset + num_local)`` and, with a weight, in
    ``[0, E_tot)`` with ``weight[t, id] > 0``."""
    if order.dim() == 1:
        order = order.unsqueeze(-1)
    N, k = order.shape
    if weight is not None:
        weight = weight.reshape(N, weight.size(-1))
    if _plan_native(order, weight, num_local):
        order = order.to(torch.int64).contiguous()
        if weight is not None:
            weight = weight.detach().contiguous()
        off, ros, sor = get_extension(required=True).moe_route_plan(
            order, weight, expert_offset, num_local)
    else:
        off, ros, sor = route_plan_reference(order, weight, expert_offset,
                                             num_local)
    return RoutePlan(off, ros, sor, N, k)


class _Permute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, row_of_slot, slot_of_row, k):
        ctx.save_for_backward(row_of_slot)
        ctx.N, ctx.k = x.size(0), k
        if supported(x):
            return get_extension(required=True).moe_permute_fwd(
                x.contiguous(), slot_of_row, k)
        return permute_fwd_reference(x, slot_of_row, k)

    @staticmethod
    def backward(ctx, dxs):
        row_of_slot, = ctx.saved_tensors
        if supported(dxs):
            dx = get_extension(required=True).moe_permute_bwd(
                dxs.contiguous(), row_of_slot, ctx.N, ctx.k)
        else:
            dx = permute_bwd_reference(dxs, row_of_slot, ctx.N, ctx.k)
        return dx, None, None, None


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ys, gates, row_of_slot, slot_of_row, N, k):
        ys = ys.contiguous()
        g = None
        if gates is not None:
            g = gates.detach()
            if supported(ys):
                g = g.float().contiguous()
        ctx.save_for_backward(ys, g, slot_of_row)
        ctx.k = k
        ctx.gate_dtype = None if gates is None else gates.dtype
        if supported(ys):
            return get_extension(required=True).moe_combine_fwd(
                ys, g, row_of_slot, N, k)
        return combine_fwd_reference(ys, g, row_of_slot, N, k)

    @staticmethod
    def backward(ctx, dout):
        ys, g, slot_of_row = ctx.saved_tensors
        want_dgate = g is not None and ctx.needs_input_grad[1]
        if supported(ys):
            dys, dgate = get_extension(required=True).moe_combine_bwd(
                dout.contiguous(), ys, g, slot_of_row, ctx.k, want_dgate)
        else:
            dys, dgate = combine_bwd_reference(dout, ys, g, slot_of_row,
                                               ctx.k, want_dgate)
        dgate = dgate.to(ctx.gate_dtype) if want_dgate else None
        if not ctx.needs_input_grad[0]:
            dys = None
        return dys, dgate, None, None, None, None


def permute(x: torch.Tensor, plan: RoutePlan) -> torch.Tensor:
    """x [N,H] -> xs [N*k,H] with ``xs[r] = x[slot_of_row[r] // k]`` and
    zeros in the dead rows.  Differentiable in x."""
    if x.dim() != 2 or x.size(0) != plan.num_tokens:
        raise ValueError("permute: x must be [N,H] with the plan's N")
    return _Permute.apply(x, plan.row_of_slot, plan.slot_of_row, plan.k)


def combine(ys: torch.Tensor, gates: Optional[torch.Tensor],
            plan: RoutePlan) -> torch.Tensor:
    """ys [N*k,H], gates None or [N*k] (per slot) -> out [N,H] with
    ``out[t] = sum_j gates[t*k+j] * ys[row_of_slot[t*k+j]]`` over the kept
    slots; tokens with nothing kept get zeros.  Differentiable in ys and
    gates (dropped slots get a zero gate gradient)."""
    S = plan.num_tokens * plan.k
    if ys.dim() != 2 or ys.size(0) != S:
        raise ValueError("combine: ys must be [N*k,H] for the plan")
    if gates is not None and gates.shape != (S,):
        raise ValueError("combine: gates must be [N*k]")
    return _Combine.apply(ys, gates, plan.row_of_slot, plan.slot_of_row,
                          plan.num_tokens, plan.k)
