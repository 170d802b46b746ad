"""Grouped expert FFN: all local experts over one expert-sorted buffer.

The per-expert loop launches E small GEMMs (plus mask, gather and
``index_put``) that each underfill the 256-CU chip.  ``grouped_mlp_forward``
runs the whole bank of identical ``Sequential(Linear, act, Linear)`` experts
on the expert-sorted token buffer instead, with two implementations:

``impl="hip"``
    ``grouped_linear -> act -> grouped_linear`` (ops/grouped_gemm.py): one
    hand-written MFMA kernel per pass (csrc/grouped_gemm.hip) that walks the
    ragged segments unpadded and reads every expert's ``[N,K]`` weight in
    place.  No ``zeros``/pad, no ``stack``, no ``cat``, no host sync; takes
    device ``offsets`` instead of a Python ``counts`` list.  The activation
    stays one elementwise torch op on the unpadded ``[T, I]`` buffer.

``impl="bmm"``
    the earlier batched path: every segment padded to the largest expert's
    row count, all weights stacked per call, two ``torch.bmm`` with
    contiguous transposed weight copies on both passes (the ROCm batched
    GEMM faults on batch-strided operands, tools/moe_repro.py).  Those
    copies are why it measured slower than the loop (16.5k vs 41.3k tok/s
    on bloom-1b7 with 8 experts); it is kept for comparison.

Measurements of both against the loop: profiles/moe_grouped_gemm.md.

Gated experts (``GatedExpertMLP``: ``down(silu(gate(x)) * up(x))``, the
llama / Mixtral shape) have a bank of their own on the ``hip`` route only:
``grouped_glu_mlp_forward`` is ``grouped_glu -> grouped_linear``
(ops/grouped_gemm.py; the gate and up products and the activation can run
as one kernel, opt-in -- profiles/moe_grouped_gemm.md §5).  There is no
bmm form of it.

MI355X-native replacement for the reference's per-expert Python loop
(nn/expert_parallel/experts.py:41-82; SURVEY §2.5 'grouped-GEMM HIP kernel').
"""
from typing import List, Optional

import torch
from torch import nn


_SUPPORTED_ACTS = (nn.GELU, nn.SiLU, nn.ReLU, nn.Tanh)


class GatedExpertMLP(nn.Module):
    """Dense gated (SwiGLU) expert: ``down_proj(silu(gate_proj(x)) *
    up_proj(x))`` with three bias-free linears named as in the llama family
    (models/llama.py::LlamaMLP).  A bank of identical ones runs on the
    grouped and sync-free MoE paths (PG_MOE_GROUPED=2/3)."""

    def __init__(self, hidden: int, intermediate: int,
                 out: Optional[int] = None):
        super().__init__()
        out = hidden if out is None else out
        self.gate_proj = nn.Linear(hidden, intermediate, bias=False)
        self.up_proj = nn.Linear(hidden, intermediate, bias=False)
        self.down_proj = nn.Linear(intermediate, out, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from pipegoose_amd.ops.silu_mul import silu_mul
        return self.down_proj(silu_mul(self.gate_proj(x), self.up_proj(x)))


def match_grouped_mlp(experts: nn.ModuleList):
    """If every expert is Sequential(Linear, act, Linear) with identical
    shapes, return (w1s, b1s, w2s, b2s, act) views; else None."""
    w1, b1, w2, b2 = [], [], [], []
    act = None
    for e in experts:
        if not isinstance(e, nn.Sequential) or len(e) != 3:
            return None
        lin1, a, lin2 = e[0], e[1], e[2]
        if not (isinstance(lin1, nn.Linear) and isinstance(lin2, nn.Linear)
                and isinstance(a, _SUPPORTED_ACTS)):
            return None
        if act is None:
            act = a
        elif type(a) is not type(act):
            return None
        w1.append(lin1.weight); b1.append(lin1.bias)
        w2.append(lin2.weight); b2.append(lin2.bias)
    if any(b is None for b in b1) != all(b is None for b in b1):
        return None
    return w1, b1, w2, b2, act


def match_grouped_glu(experts: nn.ModuleList):
    """If every expert is a GatedExpertMLP (three bias-free linears) of
    identical shapes, return (w_gate, w_up, w_down) lists; else None."""
    wg, wu, wd = [], [], []
    for e in experts:
        if not isinstance(e, GatedExpertMLP):
            return None
        lins = (e.gate_proj, e.up_proj, e.down_proj)
        if not all(isinstance(m, nn.Linear) and m.bias is None
                   for m in lins):
            return None
        wg.append(e.gate_proj.weight)
        wu.append(e.up_proj.weight)
        wd.append(e.down_proj.weight)
    if not wg:
        return None
    for ws in (wg, wu, wd):
        if any(w.shape != ws[0].shape for w in ws):
            return None
    if wu[0].shape != wg[0].shape or wd[0].size(1) != wg[0].size(0):
        return None
    return wg, wu, wd


def grouped_glu_mlp_forward(tokens: torch.Tensor, offsets: torch.Tensor,
                            wg: List[torch.Tensor], wu: List[torch.Tensor],
                            wd: List[torch.Tensor]) -> torch.Tensor:
    """tokens: [N, H] sorted by local expert; offsets: int32 [E+1] device
    tensor of segment bounds.  Returns [N, H_out] in the same order."""
    from pipegoose_amd.ops.grouped_gemm import grouped_glu, grouped_linear
    return grouped_linear(grouped_glu(tokens, offsets, wg, wu), offsets, wd)


class _GroupedLinear(torch.autograd.Function):
    """Batched y = x @ W^T with CONTIGUOUS-operand bmms on both passes.

    torch.bmm with a transposed (batch-strided) operand mem-faults in the
    ROCm GEMM backend at the 1b7-MoE shapes (bisected: tools/moe_repro.py)
    — and autograd's built-in bmm backward issues exactly such transposed
    views, so the workaround must own the backward too: dx = dy·W and
    dW = dy^T·x with explicit contiguous copies.
    """

    @staticmethod
    def forward(ctx, x, W):              # x [E, M, K], W [E, N, K]
        ctx.save_for_backward(x, W)
        return torch.bmm(x.contiguous(), W.transpose(1, 2).contiguous())

    @staticmethod
    def backward(ctx, dy):               # dy [E, M, N]
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.bmm(dy, W.contiguous())                    # [E, M, K]
        dW = torch.bmm(dy.transpose(1, 2).contiguous(), x.contiguous())
        return dx, dW


def grouped_mlp_hip(tokens: torch.Tensor, offsets: torch.Tensor,
                    w1: List[torch.Tensor], b1, w2: List[torch.Tensor], b2,
                    act: nn.Module) -> torch.Tensor:
    """tokens: [N, H] sorted by local expert; offsets: int32 [E+1] device
    tensor of segment bounds.  Returns [N, H_out] in the same order."""
    from pipegoose_amd.ops.grouped_gemm import grouped_linear
    h = grouped_linear(tokens, offsets, w1,
                       None if b1[0] is None else b1)
    h = act(h)
    return grouped_linear(h, offsets, w2, None if b2[0] is None else b2)


def grouped_mlp_forward(tokens: torch.Tensor, counts: Optional[List[int]],
                        w1: List[torch.Tensor], b1, w2: List[torch.Tensor],
                        b2, act: nn.Module, impl: str = "bmm",
                        offsets: Optional[torch.Tensor] = None
                        ) -> torch.Tensor:
    """tokens: [N, H] sorted by local expert with ``counts[i]`` rows each.
    Returns [N, H_out] in the same order.  Differentiable.

    ``impl="bmm"`` (stack + pad + bmm) needs the Python ``counts`` list;
    ``impl="hip"`` needs the device ``offsets`` tensor instead (``counts``
    is ignored and may be None)."""
    if impl == "hip":
        if offsets is None:
            raise ValueError("grouped_mlp_forward(impl='hip') needs offsets")
        return grouped_mlp_hip(tokens, offsets, w1, b1, w2, b2, act)
    if impl != "bmm":
        raise ValueError(f"unknown grouped impl {impl!r}")
    E = len(counts)
    H = tokens.size(-1)
    max_n = max(max(counts), 1)
    dev, dt = tokens.device, tokens.dtype

    padded = torch.zeros(E, max_n, H, device=dev, dtype=dt)
    start = 0
    for i, c in enumerate(counts):
        if c:
            padded[i, :c] = tokens[start:start + c]
        start += c

    W1 = torch.stack(w1).to(dt)          # [E, I, H]
    W2 = torch.stack(w2).to(dt)          # [E, H_out, I]
    h = _GroupedLinear.apply(padded, W1)
    if b1[0] is not None:
        h = h + torch.stack(b1).to(dt).unsqueeze(1)
    h = act(h)
    out = _GroupedLinear.apply(h, W2)
    if b2[0] is not None:
        out = out + torch.stack(b2).to(dt).unsqueeze(1)

    segs = [out[i, :c] for i, c in enumerate(counts) if c]
    if not segs:
        return tokens[:0]
    return torch.cat(segs, dim=0)
