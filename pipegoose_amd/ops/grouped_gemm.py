"""Grouped expert linear over an expert-sorted, ragged token buffer.

``grouped_linear(x, offsets, weights, biases)`` computes, for every expert
``e`` and every row ``r`` in ``offsets[e] .. offsets[e+1]-1``::

    y[r] = x[r] @ weights[e].T (+ biases[e])

On gfx950 with bf16 operands the three passes (forward, input grad, weight
and bias grad) are one MFMA kernel each (csrc/grouped_gemm.hip): segments
are walked unpadded, every expert's ``[N,K]`` weight is read in place (the
``nn.Linear.weight`` storages are never stacked or transposed), there is no
host sync, and the weight grad is deterministic.  Everything else (CPU,
fp32, unaligned shapes, more than 64 experts) runs an eager per-segment
``F.linear`` through the same function, so callers need one code path.

``grouped_glu(x, offsets, w_gate, w_up)`` is the gated first projection of
SwiGLU experts on the same buffer::

    h[r] = silu(x[r] @ w_gate[e].T) * (x[r] @ w_up[e].T)

with one fused kernel for the forward and one for the input grad (or the
same result composed from the plain kernels), and the same eager path
elsewhere.
"""
from typing import List, Optional, Sequence

import torch
import torch.nn.functional as TF

from pipegoose_amd.ops import get_extension

MAX_EXPERTS = 64  # compile-time cap of the kernarg pointer table


def supported(x: torch.Tensor, weights: Sequence[torch.Tensor]) -> bool:
    """True when the native kernels take this call: device tensors, all
    bf16, E <= 64, K % 64 == 0 and N % 128 == 0.  On such inputs a missing
    extension is an error, not a reason to fall back."""
    E = len(weights)
    if E < 1 or E > MAX_EXPERTS:
        return False
    if not x.is_cuda or x.dim() != 2 or x.dtype != torch.bfloat16:
        return False
    N, K = weights[0].shape
    if K % 64 or N % 128 or x.size(1) != K:
        return False
    for w in weights:
        if (not w.is_cuda or w.dtype != torch.bfloat16 or w.dim() != 2
                or tuple(w.shape) != (N, K)):
            return False
    get_extension(required=True)
    return True


def _segments(offsets: torch.Tensor, E: int, T: int):
    """Host copy of the segment bounds, sanitised the way the kernel does
    (clamped to [0, T], monotone).  Fallback path only."""
    off = offsets.tolist()
    bounds, lo = [], min(max(off[0], 0), T)
    for e in range(E):
        hi = max(min(max(off[e + 1], 0), T), lo)
        bounds.append((lo, hi))
        lo = hi
    return bounds


class _GroupedLinearHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offsets, E, has_bias, *params):
        ext = get_extension(required=True)
        weights = [w.detach() for w in params[:E]]
        weights = [w if w.is_contiguous() else w.contiguous() for w in weights]
        bias = None
        if has_bias:
            bias = torch.stack([b.detach() for b in params[E:]])  # [E, N]
        x = x.contiguous()
        ctx.save_for_backward(x, offsets, *weights)
        ctx.E, ctx.has_bias = E, has_bias
        ctx.bias_dtype = params[E].dtype if has_bias else None
        return ext.grouped_gemm_fwd(x, weights, offsets, bias)

    @staticmethod
    def backward(ctx, dy):
        ext = get_extension(required=True)
        x, offsets, *weights = ctx.saved_tensors
        E = ctx.E
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ext.grouped_gemm_dgrad(dy, weights, offsets)
        need_w = any(ctx.needs_input_grad[4:4 + E])
        need_b = ctx.has_bias and any(ctx.needs_input_grad[4 + E:])
        gw: List[Optional[torch.Tensor]] = [None] * E
        gb: List[Optional[torch.Tensor]] = [None] * (E if ctx.has_bias else 0)
        if need_w or need_b:
            # one [E,N,K] bank; each weight's gradient is a view of it
            bank, db = ext.grouped_gemm_wgrad(dy, x, offsets, E, need_b)
            gw = [bank[e] for e in range(E)]
            if need_b:
                db = db.to(ctx.bias_dtype)
                gb = [db[e] for e in range(E)]
        return (dx, None, None, None, *gw, *gb)


def _grouped_linear_eager(x, offsets, weights, biases):
    E, T = len(weights), x.size(0)
    outs = []
    for e, (lo, hi) in enumerate(_segments(offsets, E, T)):
        # empty segments still run (on a 0-row batch) so that every expert
        # parameter receives a (zero) gradient
        b = biases[e] if biases is not None else None
        outs.append(TF.linear(x[lo:hi], weights[e].to(x.dtype),
                              None if b is None else b.to(x.dtype)))
    covered = sum(o.size(0) for o in outs)
    if covered != T:
        raise ValueError(
            f"grouped_linear: offsets cover {covered} of {T} rows")
    return torch.cat(outs, dim=0)


def grouped_linear(x: torch.Tensor, offsets: torch.Tensor,
                   weights: Sequence[torch.Tensor],
                   biases: Optional[Sequence[torch.Tensor]] = None
                   ) -> torch.Tensor:
    """x: [T, K] sorted by expert; offsets: int32 [E+1] on x's device with
    ``offsets[0] == 0`` and ``offsets[E] == T``; weights: E tensors [N, K];
    biases: None or E tensors [N].  Returns [T, N].  Differentiable in x,
    every weight and every bias; experts with no rows get zero gradients."""
    weights = list(weights)
    E = len(weights)
    if biases is not None:
        biases = list(biases)
        if len(biases) != E or any(b is None for b in biases):
            raise ValueError("grouped_linear: need one bias per expert")
    if offsets.numel() != E + 1:
        raise ValueError("grouped_linear: offsets must have E+1 entries")
    if supported(x, weights):
        if offsets.dtype != torch.int32 or offsets.device != x.device:
            offsets = offsets.to(device=x.device, dtype=torch.int32)
        params = weights + (biases if biases is not None else [])
        return _GroupedLinearHip.apply(x, offsets.contiguous(), E,
                                       biases is not None, *params)
    return _grouped_linear_eager(x, offsets, weights, biases)


# ------------------------------------------------------------ gated bank
# Which passes of ``grouped_glu`` run the fused kernels when the caller
# does not say.  A fused kernel is the default for its pass only if its
# slowest run beat the composed route's fastest in the same job
# (profiles/moe_grouped_gemm.md §5): on the MI355X neither did -- forward
# 1.99 vs 1.80 ms, dgrad 1.65 vs 1.63 ms at T=16384, K=2048, I=8192 -- so
# both passes default to the composed route and the fused kernels stay
# selectable with ``fused=True`` or ``fused=(fwd, dgrad)``.
FUSED_FWD_DEFAULT = False
FUSED_DGRAD_DEFAULT = False


def supported_glu(x: torch.Tensor, w_gate: Sequence[torch.Tensor],
                  w_up: Sequence[torch.Tensor]) -> bool:
    """True when the native gated-bank kernels take this call: device bf16
    tensors, 1 <= E <= 64, every gate and up weight ``[I,K]`` with
    K % 64 == 0 and I % 128 == 0 (what the weight grad and the down
    projection need).  On such inputs a missing extension is an error."""
    if len(w_gate) != len(w_up) or not supported(x, w_gate):
        return False
    return supported(x, w_up) and w_up[0].shape == w_gate[0].shape


class _GroupedGluHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offsets, E, fused_fwd, fused_dgrad, *params):
        ext = get_extension(required=True)
        ws = [w.detach() for w in params]
        ws = [w if w.is_contiguous() else w.contiguous() for w in ws]
        wg, wu = ws[:E], ws[E:]
        x = x.contiguous()
        need_grad = any(ctx.needs_input_grad)
        if fused_fwd:
            h, g, u = ext.grouped_glu_fwd(x, wg, wu, offsets, need_grad)
        else:
            g = ext.grouped_gemm_fwd(x, wg, offsets, None)
            u = ext.grouped_gemm_fwd(x, wu, offsets, None)
            # silu_mul launches no empty grid
            h = ext.silu_mul_fwd(g, u) if g.numel() else torch.empty_like(g)
        if need_grad:
            ctx.save_for_backward(x, offsets, g, u, *ws)
        ctx.E, ctx.fused_dgrad = E, fused_dgrad
        return h

    @staticmethod
    def backward(ctx, dh):
        ext = get_extension(required=True)
        x, offsets, g, u, *ws = ctx.saved_tensors
        E = ctx.E
        wg, wu = ws[:E], ws[E:]
        dh = dh.contiguous()
        if dh.numel():
            dg, du = ext.silu_mul_bwd(dh, g, u)
        else:
            dg, du = torch.empty_like(g), torch.empty_like(u)
        dx = None
        if ctx.needs_input_grad[0]:
            if ctx.fused_dgrad:
                dx = ext.grouped_glu_dgrad(dg, du, wg, wu, offsets)
            else:
                dx = ext.grouped_gemm_dgrad(dg, wg, offsets) \
                    + ext.grouped_gemm_dgrad(du, wu, offsets)
        gw: List[Optional[torch.Tensor]] = [None] * (2 * E)
        if any(ctx.needs_input_grad[5:5 + E]):
            # one [E,I,K] bank per matrix; each grad is a view of it
            bank, _ = ext.grouped_gemm_wgrad(dg, x, offsets, E, False)
            gw[:E] = [bank[e] for e in range(E)]
        if any(ctx.needs_input_grad[5 + E:]):
            bank, _ = ext.grouped_gemm_wgrad(du, x, offsets, E, False)
            gw[E:] = [bank[e] for e in range(E)]
        return (dx, None, None, None, None, *gw)


def _grouped_glu_eager(x, offsets, w_gate, w_up):
    E, T = len(w_gate), x.size(0)
    outs = []
    for e, (lo, hi) in enumerate(_segments(offsets, E, T)):
        # empty segments still run so every weight receives a (zero) grad
        g = TF.linear(x[lo:hi], w_gate[e].to(x.dtype))
        u = TF.linear(x[lo:hi], w_up[e].to(x.dtype))
        outs.append(TF.silu(g) * u)
    covered = sum(o.size(0) for o in outs)
    if covered != T:
        raise ValueError(f"grouped_glu: offsets cover {covered} of {T} rows")
    return torch.cat(outs, dim=0)


def grouped_glu(x: torch.Tensor, offsets: torch.Tensor,
                w_gate: Sequence[torch.Tensor], w_up: Sequence[torch.Tensor],
                fused=None) -> torch.Tensor:
    """Gated expert projection: for the rows ``r`` of expert ``e``,
    ``h[r] = silu(x[r] @ w_gate[e].T) * (x[r] @ w_up[e].T)``.

    x: [T, K] sorted by expert; offsets: int32 [E+1] as in
    ``grouped_linear``; w_gate, w_up: E tensors [I, K] each.  Returns
    [T, I].  Differentiable in x and all 2E weights; experts with no rows
    get zero gradients.

    On the native path the bf16-rounded gate and up products are what the
    activation sees and what is saved for backward.  ``fused=True`` runs
    the fused kernels (csrc/grouped_gemm.hip: both products from one read
    of x with silu*mul in the epilogue; both input-grad products in one
    accumulator); ``fused=False`` composes the same result from two grouped
    GEMMs and the silu_mul kernels; ``fused=(fwd, dgrad)`` picks per pass;
    ``None`` takes the measured defaults (``FUSED_FWD_DEFAULT``,
    ``FUSED_DGRAD_DEFAULT``).  The forward result and the weight grads do
    not depend on the choice; the input grad differs in one rounding."""
    w_gate, w_up = list(w_gate), list(w_up)
    E = len(w_gate)
    if len(w_up) != E:
        raise ValueError("grouped_glu: need one up weight per gate weight")
    if offsets.numel() != E + 1:
        raise ValueError("grouped_glu: offsets must have E+1 entries")
    if supported_glu(x, w_gate, w_up):
        if fused is None:
            fused_fwd, fused_dgrad = FUSED_FWD_DEFAULT, FUSED_DGRAD_DEFAULT
        elif isinstance(fused, (tuple, list)):
            fused_fwd, fused_dgrad = (bool(f) for f in fused)
        else:
            fused_fwd = fused_dgrad = bool(fused)
        if offsets.dtype != torch.int32 or offsets.device != x.device:
            offsets = offsets.to(device=x.device, dtype=torch.int32)
        return _GroupedGluHip.apply(x, offsets.contiguous(), E, fused_fwd,
                                    fused_dgrad, *w_gate, *w_up)
    return _grouped_glu_eager(x, offsets, w_gate, w_up)
