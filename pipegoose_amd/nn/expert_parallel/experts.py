"""Expert bank sharded over the TENSOR axis.

Reference parity: nn/expert_parallel/experts.py:41-102 (mask-select dispatch,
all-reduce combine over the TENSOR group; expert params tagged ``is_expert``
so DataParallel reduces them over the EXPERT_DATA group).

MI355X path: when every rank holds >1 expert the local experts run as a
grouped GEMM (one kernel for all local experts) via pipegoose_amd.ops; the
cross-rank combine stays a single RCCL all-reduce over xGMI.  Token
all-to-all dispatch is used by the EP=8 config (see expert_parallel.py).
With PG_MOE_GROUPED=3 an unsharded bank also dispatches and combines with
kernels (ops/moe_permute.py): the layer runs forward and backward without
a host synchronisation.
"""
import copy

import torch
from torch import nn

from pipegoose_amd.distributed import functional as F
from pipegoose_amd.distributed.parallel_context import ParallelContext
from pipegoose_amd.distributed.parallel_mode import ParallelMode


class Experts(nn.Module):
    def __init__(self, num_experts: int, expert: nn.Module,
                 enable_tensor_parallel: bool, parallel_context: ParallelContext,
                 dispatch: str = "mask"):
        super().__init__()
        assert dispatch in ("mask", "alltoall")
        self.parallel_context = parallel_context
        self.dispatch = dispatch
        tp_size = parallel_context.get_world_size(ParallelMode.TENSOR)
        if enable_tensor_parallel and tp_size > 1:
            assert num_experts % tp_size == 0
            self.num_local_experts = num_experts // tp_size
            rank = parallel_context.get_local_rank(ParallelMode.TENSOR)
            self.expert_offset = rank * self.num_local_experts
        else:
            self.num_local_experts = num_experts
            self.expert_offset = 0
        self.num_experts = num_experts
        self.enable_tensor_parallel = enable_tensor_parallel and tp_size > 1

        # share (don't copy) the ParallelContext a prototype module may hold:
        # ProcessGroups aren't picklable and must stay process-wide singletons
        memo = {id(parallel_context): parallel_context}
        self.experts = nn.ModuleList(
            [copy.deepcopy(expert, dict(memo)) for _ in range(self.num_local_experts)]
        )
        if self.enable_tensor_parallel:
            # An expert must be a DENSE local module: the EP axis reuses the
            # TENSOR group, so a TP-sharded expert would fire its internal
            # all-reduces with per-rank-different token counts → collective
            # mismatch.  (Native models build TP layers at construction;
            # pass a plain nn.Module via ExpertParallel(expert=...).)
            from pipegoose_amd.nn.tensor_parallel.linear import (
                ColumnParallelLinear, RowParallelLinear)
            for m in self.experts.modules():
                if isinstance(m, (ColumnParallelLinear, RowParallelLinear)):
                    raise TypeError(
                        "expert prototype contains tensor-parallel layers; "
                        "pass a dense expert module to ExpertParallel(expert=...)")
        for p in self.experts.parameters():
            setattr(p, "is_expert", True)
        # grouped-GEMM fast path: identical Sequential(Linear, act, Linear)
        # experts run as one batched MFMA GEMM over the expert-sorted tokens
        from pipegoose_amd.nn.expert_parallel.grouped import (
            match_grouped_glu, match_grouped_mlp)
        self._grouped = match_grouped_mlp(self.experts)
        # identical GatedExpertMLP experts: the gated bank of the native
        # kernels (PG_MOE_GROUPED=2/3); the bmm bank has no gated form
        self._grouped_glu = match_grouped_glu(self.experts)

    def forward(self, inputs: torch.Tensor, dispatch_order: torch.Tensor,
                weight: torch.Tensor = None, *args, **kwargs):
        # inputs: [B, S, H]; dispatch_order: [N] (top-1) or [N, k] global
        # expert ids; weight: optional [N, num_experts] routing weights
        # (capacity-dropped entries are 0).  With a weight matrix the output
        # is the gate-weighted combine (Switch semantics — this also gives
        # the router a gradient through the main path, which the reference's
        # unweighted scatter never did); without it, top-1 unweighted
        # (reference parity).
        shape = inputs.shape
        flat = inputs.reshape(-1, shape[-1])
        if self.dispatch == "alltoall" and self.enable_tensor_parallel:
            return self._forward_alltoall(flat, dispatch_order,
                                          weight).reshape(shape)
        k = 1 if dispatch_order.dim() == 1 else dispatch_order.size(-1)
        order2d = dispatch_order.reshape(-1, k)
        mode = _grouped_mode()
        if self._bank_modes(mode):
            # measured SLOWER than the per-expert loop on the 1b7-MoE bench
            # (16.5k vs 41.3k tok/s): the ROCm transposed-bmm fault forces
            # contiguous weight copies every call (grouped.py), which
            # dominate.  Kept opt-in for re-evaluation when the backend bug
            # is fixed; the a2a path still uses the grouped bank (tokens/ep
            # per rank makes the copies proportionally cheaper there).
            # PG_MOE_GROUPED=2 runs the same dispatch through the native
            # grouped kernels instead (no padding, no weight copies; 47.9k
            # tok/s on that bench, profiles/moe_grouped_gemm.md).
            # PG_MOE_GROUPED=3 additionally replaces the eager dispatch and
            # combine around those kernels (two host syncs, an argsort, an
            # fp32 [N,H] atomic index_put for top-k) by the routing-plan,
            # permute and combine kernels of ops/moe_permute.py: no host
            # sync in forward or backward, deterministic.  Where that path
            # does not apply (CPU, fp32, odd shapes, expert-sharded bank)
            # mode 3 is mode 2.
            if mode == "3" and self._fused_applies(flat, weight):
                return self._forward_local_fused(flat, order2d,
                                                 weight).reshape(shape)
            outputs = self._forward_local_grouped(
                flat, order2d, weight, impl="bmm" if mode == "1" else "hip")
            if self.enable_tensor_parallel:
                outputs = _AllReduceCombine.apply(outputs,
                                                  self.parallel_context)
            return outputs.reshape(shape)
        outputs = torch.zeros_like(flat)
        for local_idx, expert in enumerate(self.experts):
            global_idx = self.expert_offset + local_idx
            token_mask = (order2d == global_idx).any(dim=-1)
            if weight is not None:
                # capacity-dropped tokens (weight 0) are not computed
                token_mask = token_mask & (
                    weight.reshape(-1, self.num_experts)[:, global_idx] > 0)
            # A zero-token expert still runs (on a 0-row batch) so every
            # expert param gets a grad every step: DP ranks route different
            # tokens, and a rank that skipped an expert its EXPERT_DATA peer
            # ran would launch a different bucket-reduce sequence → hang.
            selected = flat[token_mask]
            # experts receive ONLY their tokens; block-level extras such
            # as HF Bloom's residual are handled by ExpertLayer
            expert_out = expert(selected)
            if isinstance(expert_out, tuple):
                expert_out = expert_out[0]
            expert_out = expert_out.to(outputs.dtype)
            if weight is not None:
                w = weight.reshape(-1, self.num_experts)[token_mask,
                                                         global_idx]
                expert_out = expert_out * w.unsqueeze(-1).to(outputs.dtype)
                idx = token_mask.nonzero(as_tuple=True)[0]
                outputs = outputs.index_put((idx,), expert_out,
                                            accumulate=True)  # top-2 sums
            else:
                outputs[token_mask] = expert_out
        if self.enable_tensor_parallel:
            outputs = _AllReduceCombine.apply(outputs, self.parallel_context)
        return outputs.reshape(shape)

    def _bank_modes(self, mode: str) -> bool:
        """Whether PG_MOE_GROUPED=`mode` runs the experts as one bank:
        Sequential(Linear, act, Linear) experts in modes 1-3, gated experts
        in modes 2 and 3 (native kernels only)."""
        if self._grouped is not None:
            return mode in ("1", "2", "3")
        return self._grouped_glu is not None and mode in ("2", "3")

    def _bank_hip(self, tokens: torch.Tensor,
                  offsets: torch.Tensor) -> torch.Tensor:
        """The whole local bank over an expert-sorted buffer through the
        native grouped kernels: tokens [S, H], device offsets [E+1]."""
        from pipegoose_amd.nn.expert_parallel.grouped import (
            grouped_glu_mlp_forward, grouped_mlp_forward)
        if self._grouped is not None:
            w1, b1, w2, b2, act = self._grouped
            return grouped_mlp_forward(tokens, None, w1, b1, w2, b2, act,
                                       impl="hip", offsets=offsets)
        wg, wu, wd = self._grouped_glu
        return grouped_glu_mlp_forward(tokens, offsets, wg, wu, wd)

    def _forward_local_grouped(self, flat: torch.Tensor,
                               order2d: torch.Tensor,
                               weight: torch.Tensor = None,
                               impl: str = "bmm") -> torch.Tensor:
        """Mask-dispatch semantics via one grouped GEMM over the tokens
        routed to THIS rank's experts (all of them when EP is off)."""
        from pipegoose_amd.nn.expert_parallel.grouped import (
            grouped_mlp_forward)
        N, k = order2d.shape
        dev = flat.device
        tok = torch.arange(N, device=dev).repeat_interleave(k)
        ridx = order2d.reshape(-1)
        keep = (ridx >= self.expert_offset) & \
               (ridx < self.expert_offset + self.num_local_experts)
        if weight is not None:
            wvals = weight.reshape(N, self.num_experts)[tok, ridx]
            keep = keep & (wvals > 0)
        tok, ridx = tok[keep], ridx[keep] - self.expert_offset
        perm = torch.argsort(ridx, stable=True)
        tok, ridx = tok[perm], ridx[perm]
        counts = torch.bincount(ridx, minlength=self.num_local_experts)
        if impl == "hip":  # device offsets: no host sync on the counts
            expert_out = self._bank_hip(
                flat[tok], _offsets_from_counts(counts)).to(flat.dtype)
        else:
            w1, b1, w2, b2, act = self._grouped
            expert_out = grouped_mlp_forward(flat[tok], counts.tolist(), w1,
                                             b1, w2, b2, act).to(flat.dtype)
        if weight is not None:
            expert_out = expert_out * wvals[keep][perm].unsqueeze(-1) \
                .to(flat.dtype)
        if k == 1:
            # top-1: each token appears at most once — plain scatter
            outputs = torch.zeros_like(flat)
            return outputs.index_put((tok,), expert_out)
        # top-k: a token can receive k contributions; accumulate in fp32
        # (bf16 scattered atomics are neither precise nor reliable here)
        out32 = torch.zeros(flat.shape, device=flat.device,
                            dtype=torch.float32)
        out32 = out32.index_put((tok,), expert_out.float(), accumulate=True)
        return out32.to(flat.dtype)

    def _fused_applies(self, flat: torch.Tensor, weight) -> bool:
        """PG_MOE_GROUPED=3 takes the call: local (unsharded) bank, rows the
        permute kernels and every grouped projection accept natively."""
        from pipegoose_amd.ops import grouped_gemm, moe_permute
        if self.enable_tensor_parallel or not self._bank_modes("3"):
            return False
        if self._grouped is not None:
            w1, _, w2, _, _ = self._grouped
            wu = None
        else:  # gated bank: gate and up share the first projection's shape
            w1, wu, w2 = self._grouped_glu
        if weight is not None and (
                not weight.is_cuda
                or weight.dtype not in (torch.bfloat16, torch.float32)):
            return False
        if not moe_permute.supported(flat, self.num_local_experts):
            return False
        if not (grouped_gemm.supported(flat, w1) if wu is None
                else grouped_gemm.supported_glu(flat, w1, wu)):
            return False
        I, H_out = w1[0].size(0), w2[0].size(0)
        # the last linear sees [S, I] rows; the combine moves [S, H_out]
        return (H_out % 8 == 0 and all(
            w.is_cuda and w.dtype == torch.bfloat16
            and tuple(w.shape) == (H_out, I) for w in w2)
            and I % 64 == 0 and H_out % 128 == 0)

    def _forward_local_fused(self, flat: torch.Tensor, order2d: torch.Tensor,
                             weight: torch.Tensor = None) -> torch.Tensor:
        """The mask-dispatch semantics of ``_forward_local_grouped`` with no
        host synchronisation: the routing plan, the gather into the
        expert-sorted buffer and the gate-weighted combine are kernels
        (ops/moe_permute.py).  The buffer always has N*k rows; rows past
        ``offsets[E]`` are dead -- the grouped kernels walk only the rows
        ``offsets`` covers, and permute/combine go through the plan."""
        from pipegoose_amd.ops.moe_permute import (combine, permute,
                                                   route_plan)
        N = order2d.size(0)
        plan = route_plan(order2d, weight, self.expert_offset,
                          self.num_local_experts)
        xs = permute(flat, plan)                           # [N*k, H]
        ys = self._bank_hip(xs, plan.offsets).to(flat.dtype)
        gates = None
        if weight is not None:
            # tiny [N,k] gather; its autograd carries dgate into `weight`
            gates = weight.reshape(N, self.num_experts) \
                .gather(1, order2d).reshape(-1).float()
        return combine(ys, gates, plan)

    def _forward_alltoall(self, flat: torch.Tensor,
                          dispatch_order: torch.Tensor,
                          weight: torch.Tensor = None):
        """EP dispatch over xGMI.  The activation is replicated across the EP
        group, so first each rank takes its 1/ep chunk of the token set (no
        redundant expert FLOPs — the mask path recomputes every token on every
        rank), all-to-alls its chunk to the expert-owner ranks, computes, and
        all-to-alls back; a final dim-0 all-gather rebuilds the replicated
        output.  Backward mirrors: chunk the output grad, reverse exchanges,
        all-gather input grads — every rank ends with the FULL input gradient
        (the mask path leaves per-rank partials that are only correct after a
        downstream TP sum).

        With a routing-weight matrix: capacity-dropped tokens are NOT put on
        the wire (their output row stays 0 — the residual path carries them,
        Switch semantics), top-2 tokens ship once per selected expert, and
        the combine is gate-weighted (giving the router main-path gradient).
        """
        from pipegoose_amd.nn.expert_parallel.dispatch import AllToAllDispatcher
        from pipegoose_amd.nn.tensor_parallel._functional import (
            _Gather, _Scatter)
        if not hasattr(self, "_dispatcher"):
            self._dispatcher = AllToAllDispatcher(
                self.num_experts, self.parallel_context, ParallelMode.TENSOR)
        ep = self.parallel_context.get_world_size(ParallelMode.TENSOR)
        rank = self.parallel_context.get_local_rank(ParallelMode.TENSOR)
        assert flat.size(0) % ep == 0, \
            f"token count {flat.size(0)} not divisible by ep={ep}"
        k = 1 if dispatch_order.dim() == 1 else dispatch_order.size(-1)
        chunk = _Scatter.apply(flat, 0, self.parallel_context)
        n = chunk.size(0)
        route_chunk = dispatch_order.reshape(-1, k).chunk(ep, dim=0)[rank]

        if weight is None and k == 1:
            send_tokens, send_routes = chunk, route_chunk.reshape(-1)
            tok_idx = None
        else:
            w_chunk = weight.reshape(-1, self.num_experts).chunk(ep, dim=0)[rank]
            tok_rep = torch.arange(n, device=chunk.device) \
                .repeat_interleave(k)
            ridx = route_chunk.reshape(-1)
            wvals = w_chunk[tok_rep, ridx]
            keep = wvals > 0  # capacity-dropped entries never hit the wire
            tok_idx = tok_rep[keep]
            send_tokens = chunk[tok_idx]
            send_routes = ridx[keep]
            wkeep = wvals[keep]

        recv, local_idx, state = self._dispatcher.dispatch(send_tokens,
                                                           send_routes)
        counts = torch.bincount(local_idx, minlength=self.num_local_experts)
        # mode 3 is mode 2 here: the split sizes need the host anyway
        use_hip = _grouped_mode() in ("2", "3") and self._bank_modes("2")
        counts = counts if use_hip else counts.tolist()
        if use_hip:  # device offsets: no host sync on the counts
            expert_out = self._bank_hip(
                recv, _offsets_from_counts(counts)).to(recv.dtype)
        elif self._grouped is not None and recv.size(0) > 0:
            from pipegoose_amd.nn.expert_parallel.grouped import (
                grouped_mlp_forward)
            w1, b1, w2, b2, act = self._grouped
            expert_out = grouped_mlp_forward(recv, counts, w1, b1, w2, b2, act)
        else:
            outs = []
            start = 0
            for i, expert in enumerate(self.experts):
                seg = recv[start:start + counts[i]]
                out = expert(seg)
                if isinstance(out, tuple):
                    out = out[0]
                outs.append(out.to(recv.dtype))
                start += counts[i]
            expert_out = torch.cat(outs, dim=0) if outs else recv
        combined = self._dispatcher.combine(expert_out, state)
        if tok_idx is not None:
            combined = combined * wkeep.unsqueeze(-1).to(combined.dtype)
            if k == 1:  # no per-token overlap: plain scatter
                outc = torch.zeros_like(chunk)
                combined = outc.index_put((tok_idx,), combined)
            else:       # top-k sums accumulate in fp32 (see grouped path)
                out32 = torch.zeros(chunk.shape, device=chunk.device,
                                    dtype=torch.float32)
                out32 = out32.index_put((tok_idx,), combined.float(),
                                        accumulate=True)
                combined = out32.to(chunk.dtype)
        return _Gather.apply(combined, 0, self.parallel_context)


def _grouped_mode() -> str:
    """PG_MOE_GROUPED: unset/0 = per-expert loop, 1 = padded bmm bank,
    2 = native grouped-GEMM kernels, 3 = those plus the sync-free
    routing-plan/permute/combine kernels around them (mode 2 wherever the
    fused path does not apply)."""
    import os
    return os.environ.get("PG_MOE_GROUPED", "0")


def _offsets_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """[E] device counts -> int32 [E+1] segment bounds, no host sync."""
    offsets = torch.zeros(counts.numel() + 1, device=counts.device,
                          dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets


class _AllReduceCombine(torch.autograd.Function):
    """Sum expert-sharded outputs across the TENSOR group (each token was
    computed on exactly one rank, zeros elsewhere)."""

    @staticmethod
    def forward(ctx, tensor, parallel_context):
        ctx.parallel_context = parallel_context
        tensor = tensor.contiguous()
        F.all_reduce(tensor, parallel_context=parallel_context,
                     parallel_mode=ParallelMode.TENSOR)
        return tensor

    @staticmethod
    def backward(ctx, grad):
        return grad, None
