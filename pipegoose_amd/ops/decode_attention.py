"""Decode attention: one query row per sequence against the KV cache.

    o[b,h,:] = softmax_j(scale * q[b,h,:]·k[b,h//G,j,:] + slopes[h]*(j-p))
               @ v[b,h//G,j,:]        j in [0, p] inclusive, p = pos[b]

GPU path: the split-KV HIP kernels of csrc/decode_attention.hip — causal cut,
ALiBi bias and the GQA head mapping in-kernel, fp32 softmax, the position
read ON THE DEVICE (so a captured hipGraph replays with it as data), and
nothing beyond ``p`` ever read: cache slots ``j > p`` may hold anything.
Everything else (CPU, fp32, other head dims, ``PG_DECODE_ATTN=0``) runs the
pure-torch reference.  Inference only — there is no backward.
"""
import os

import torch

from pipegoose_amd.ops import get_extension


def decode_attention_reference(q, k, v, slopes, scale, pos=None):
    """Pure-torch definition, in the dtype of ``q`` (fp64 in, fp64 oracle out).

    q [B,H,1,D]; k, v [B,Hkv,Skv,D]; slopes [H]; pos a 1- or B-element integer
    tensor, or None for ``Skv - 1``.  Returns [B,H,1,D]."""
    B, H, _, D = q.shape
    Hkv, Skv = k.size(1), k.size(2)
    G = H // Hkv
    if pos is None:
        p = torch.full((B,), Skv - 1, dtype=torch.long, device=q.device)
    else:
        p = pos.to(device=q.device, dtype=torch.long).reshape(-1).expand(B)
    j = torch.arange(Skv, device=q.device)
    rel = j[None, :] - p[:, None]                               # [B, Skv]
    # GQA by head index: q heads viewed as [Hkv, G] against the Hkv-head
    # cache, no expanded copy of the cache
    qg = q.reshape(B, Hkv, G, D)
    s = torch.einsum("bkgd,bkjd->bkgj", qg, k.to(q.dtype)) * scale
    bias = slopes.to(device=q.device, dtype=q.dtype).reshape(1, Hkv, G, 1) \
        * rel.to(q.dtype)[:, None, None, :]
    s = (s + bias).masked_fill((rel > 0)[:, None, None, :], float("-inf"))
    w = torch.softmax(s, dim=-1)
    # masked slots get weight exactly 0; keep whatever they hold out of 0*v
    vv = v.to(q.dtype).masked_fill((rel > 0)[:, None, :, None], 0)
    o = torch.einsum("bkgj,bkjd->bkgd", w, vv)
    return o.reshape(B, H, 1, D)


def decode_kernel_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    """Whether the HIP decode kernels take (q, k): bf16 on the GPU, extension
    present, one query row, D in {64, 128}, and not opted out with
    ``PG_DECODE_ATTN=0`` (read on every call, so one process can A/B).

    Measured (profiles/decode_attn.md): no slower than the sdpa path at any
    (shape, filled length) recorded there, so no shape region is excluded."""
    if os.environ.get("PG_DECODE_ATTN", "1") == "0":
        return False
    if not (q.is_cuda and k.is_cuda) or q.dtype != torch.bfloat16 \
            or k.dtype != torch.bfloat16:
        return False
    if get_extension() is None:   # not built, or PIPEGOOSE_DISABLE_EXT=1
        return False
    return q.dim() == 4 and q.size(-2) == 1 and q.size(-1) in (64, 128)


def decode_attention(q, k, v, slopes, scale, pos=None):
    """The kernel when ``decode_kernel_supported``, else the reference.
    Logical [B,H,1,D]; the kernel's result is physically [B,1,H,D]."""
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (q, k, v, slopes)):
        raise RuntimeError(
            "decode_attention is inference-only (no backward): call it under "
            "torch.no_grad() or with tensors that do not require grad")
    if not decode_kernel_supported(q, k):
        return decode_attention_reference(q, k, v, slopes, scale, pos)
    ext = get_extension(required=True)
    return ext.decode_attn(
        q, k, v, slopes.to(device=q.device, dtype=torch.float32), scale,
        pos, 0)
