"""Paged KV cache ops: decode and prefill attention and cache writes through a
block table.

K and V live in pools ``[n_pages, Hkv, PAGE, D]`` shared by all sequences.
``block_table`` (int32 ``[B, max_pages]``) names the pages of each sequence
in logical order: key row ``j`` of batch row ``b`` is

    pool[block_table[b, j // PAGE], h // G, j % PAGE, :]

GPU path: ``paged_decode_attn`` and ``paged_kv_write`` of
csrc/decode_attention.hip — the decode kernel's maths with the row address
taken through the table, positions read ON THE DEVICE, page ids clamped into
the pool, nothing beyond the position (table entries included) ever read, and
rows written past ``max_pages * PAGE`` dropped — and ``paged_prefill_attn`` of
csrc/paged_prefill_attention.hip for ``Sq > 1`` query rows at positions
``start[b] + i`` (chunked prefill, prefix reuse) under the same rules, rows
outside ``[0, max_pages * PAGE)`` giving zeros.  Everything else (CPU, fp32,
other head dims, ``PG_DECODE_ATTN=0``) runs the pure-torch references.
Inference only — there is no backward.
"""
import torch

from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.decode_attention import (decode_attention_reference,
                                                decode_kernel_supported)


def paged_gather(pool: torch.Tensor, block_table: torch.Tensor,
                 n_rows: int) -> torch.Tensor:
    """Materialise the first ``n_rows`` logical rows of every sequence:
    ``[B, Hkv, n_rows, D]`` from ``pool`` [n_pages, Hkv, PAGE, D]."""
    page = pool.size(2)
    n = -(-n_rows // page)
    pages = pool[block_table[:, :n].long()]            # [B, n, Hkv, PAGE, D]
    B, _, Hkv, _, D = pages.shape
    rows = pages.permute(0, 2, 1, 3, 4).reshape(B, Hkv, n * page, D)
    return rows[:, :, :n_rows]


def paged_decode_attention_reference(q, k_pool, v_pool, block_table, slopes,
                                     scale, pos):
    """``decode_attention_reference`` on the gathered cache, in the dtype of
    ``q`` (fp64 in, fp64 oracle out)."""
    n_rows = block_table.size(1) * k_pool.size(2)
    return decode_attention_reference(
        q, paged_gather(k_pool, block_table, n_rows),
        paged_gather(v_pool, block_table, n_rows), slopes, scale, pos)


def paged_prefill_attention_reference(q, k_pool, v_pool, block_table, slopes,
                                      scale, start):
    """Pure-torch definition of prefill attention over the paged cache, in the
    dtype of ``q`` (fp64 in, fp64 oracle out).

    q [B,H,Sq,D]; row ``i`` of batch row ``b`` sits at ``p = start[b] + i``
    and sees keys ``0..p`` of the gathered cache with bias
    ``slopes[h] * (j - p)``.  Rows with ``p`` outside
    ``[0, max_pages * PAGE)`` give zeros.  Returns [B,H,Sq,D]."""
    B, H, Sq, D = q.shape
    Hkv = k_pool.size(1)
    G = H // Hkv
    cap = block_table.size(1) * k_pool.size(2)
    k = paged_gather(k_pool, block_table, cap).to(q.dtype)
    v = paged_gather(v_pool, block_table, cap).to(q.dtype)
    st = start.to(device=q.device, dtype=torch.long).reshape(-1).expand(B)
    p = st[:, None] + torch.arange(Sq, device=q.device)            # [B, Sq]
    in_range = (p >= 0) & (p < cap)
    j = torch.arange(cap, device=q.device)
    rel = j[None, None, :] - p[:, :, None]                         # [B, Sq, cap]
    qg = q.reshape(B, Hkv, G, Sq, D)
    s = torch.einsum("bkgid,bkjd->bkgij", qg, k) * scale
    bias = slopes.to(device=q.device, dtype=q.dtype).reshape(1, Hkv, G, 1, 1) \
        * rel.to(q.dtype)[:, None, None]
    s = (s + bias).masked_fill((rel > 0)[:, None, None], float("-inf"))
    # out-of-range rows (all masked, or a bias of any size): weight 0
    w = torch.softmax(s, dim=-1).masked_fill(
        ~in_range[:, None, None, :, None], 0)
    # slots no in-range row sees get weight exactly 0; keep whatever they
    # hold out of 0*v
    p_max = torch.where(in_range, p, torch.full_like(p, -1)).amax(dim=1)
    vv = v.masked_fill((j[None, :] > p_max[:, None])[:, None, :, None], 0)
    o = torch.einsum("bkgij,bkjd->bkgid", w, vv)
    return o.reshape(B, H, Sq, D)


def paged_kv_write_reference(k_new, v_new, k_pool, v_pool, block_table, start):
    """Pure-torch definition of the write: row ``s`` of batch row ``b`` goes
    to logical position ``start[b] + s``; rows outside
    ``[0, max_pages * PAGE)`` are dropped.  Writes the pools in place."""
    B, _, S_new, _ = k_new.shape
    page = k_pool.size(2)
    capacity = block_table.size(1) * page
    st = start.to(device=k_new.device, dtype=torch.long).reshape(-1).expand(B)
    row = st[:, None] + torch.arange(S_new, device=k_new.device)   # [B, S]
    keep = (row >= 0) & (row < capacity)
    safe = row.clamp(0, capacity - 1)
    ids = block_table.long().gather(1, safe // page)[keep]         # [n]
    slot = (safe % page)[keep]
    # [B, S, Hkv, D] rows of the kept positions
    k_pool[ids, :, slot] = k_new.transpose(1, 2)[keep].to(k_pool.dtype)
    v_pool[ids, :, slot] = v_new.transpose(1, 2)[keep].to(v_pool.dtype)


def paged_kernel_supported(q: torch.Tensor, k_pool: torch.Tensor) -> bool:
    """Whether the HIP paged kernels take these operands: the conditions of
    ``decode_kernel_supported`` (GPU, bf16, extension present, D in
    {64, 128}, ``PG_DECODE_ATTN != "0"``) and a page size the kernel knows.
    ``q`` may hold any number of rows (the write's new rows, a prefill chunk):
    only its first row is shown to the decode condition.

    Measured (profiles/paged_decode_attn.md, profiles/paged_prefill_attn.md):
    the paged decode kernel is 0.82-1.05x the contiguous one, and the prefill
    kernel 0.15-0.96x the time of gather + sdpa at every (shape, Sq 128/512,
    context 0/1024/3584, page 16/64) recorded there, the closest row 4 %
    apart at a spread of 0.4 %, so no shape region is excluded."""
    return decode_kernel_supported(q[:, :, :1], k_pool) \
        and k_pool.size(2) in (16, 32, 64, 128)


def _inference_only(name, tensors):
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(
            f"{name} is inference-only (no backward): call it under "
            "torch.no_grad() or with tensors that do not require grad")


def paged_decode_attention(q, k_pool, v_pool, block_table, slopes, scale, pos):
    """The kernel when ``paged_kernel_supported``, else the reference.
    Logical [B,H,1,D]; the kernel's result is physically [B,1,H,D]."""
    _inference_only("paged_decode_attention", (q, k_pool, v_pool, slopes))
    if not (q.size(-2) == 1 and paged_kernel_supported(q, k_pool)):
        return paged_decode_attention_reference(
            q, k_pool, v_pool, block_table, slopes, scale, pos)
    ext = get_extension(required=True)
    return ext.paged_decode_attn(
        q, k_pool, v_pool, block_table,
        slopes.to(device=q.device, dtype=torch.float32), scale, pos, 0)


def paged_prefill_attention(q, k_pool, v_pool, block_table, slopes, scale,
                            start):
    """Attention of the ``Sq >= 1`` rows of ``q`` [B,H,Sq,D] at positions
    ``start[b] + i`` over the pools, which already hold the rows' own K/V:
    the kernel when ``paged_kernel_supported``, else the reference.  The
    kernel's result is physically [B,Sq,H,D]."""
    _inference_only("paged_prefill_attention", (q, k_pool, v_pool, slopes))
    if not paged_kernel_supported(q, k_pool):
        return paged_prefill_attention_reference(
            q, k_pool, v_pool, block_table, slopes, scale, start)
    ext = get_extension(required=True)
    return ext.paged_prefill_attn(
        q, k_pool, v_pool, block_table,
        slopes.to(device=q.device, dtype=torch.float32), scale, start)


def paged_kv_write(k_new, v_new, k_pool, v_pool, block_table, start):
    """Write the new rows into the pools (in place): the kernel when
    ``paged_kernel_supported``, else the reference."""
    _inference_only("paged_kv_write", (k_new, v_new, k_pool, v_pool))
    if not paged_kernel_supported(k_new, k_pool):
        return paged_kv_write_reference(k_new, v_new, k_pool, v_pool,
                                        block_table, start)
    get_extension(required=True).paged_kv_write(
        k_new, v_new, k_pool, v_pool, block_table, start)
