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

``paged_varlen_attn`` of csrc/paged_varlen_attention.hip is the same
attention over a TOKEN-PACKED ragged batch ``q`` [T,H,D]: sequence ``b`` owns
the rows ``cu_q[b] .. cu_q[b+1]-1`` at positions ``start[b] + i`` over
``block_table[b]``, all read on the device, in one launch whose M tiles hold
``64/G`` tokens x the ``G`` heads of one kv head.

fp8 cache (``k_scale`` / ``v_scale`` given): the pools are
``torch.float8_e4m3fn`` and every cached row of every kv head has an fp32
scale in ``[n_pages, Hkv, PAGE]`` tensors indexed by the same page ids; a row
is quantised when it is written (``scale = amax / 448``, no calibration) and
reads back as ``float(byte) * scale``.  GPU path: ``paged_kv_write_fp8`` and
``paged_decode_attn_fp8`` of csrc/paged_fp8_attention.hip and
``paged_prefill_attn_fp8`` of csrc/paged_fp8_prefill_attention.hip and, for
the token-packed batch, ``paged_varlen_attn_fp8`` of
csrc/paged_fp8_varlen_attention.hip (each K/V tile converted from bytes once
per GQA group) and its split-KV form ``paged_varlen_split_attn_fp8`` of
csrc/paged_fp8_varlen_split_attention.hip, under the same conditions and
rules as the bf16 kernels; no scale beyond the last visible row is read
either.

``paged_rope_write`` is the LLaMA step's rotary embedding fused with the
cache write: q and the new K rows rotated at ``start[b] + s`` (half-split
convention, position read on the device), the rotated K and V written through
the table, one launch of csrc/paged_rope_write.hip for bf16 and for fp8
caches.
"""
import math
import os

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


def paged_gather_dequant(pool: torch.Tensor, scale: torch.Tensor,
                         block_table: torch.Tensor, n_rows: int,
                         dtype: torch.dtype) -> torch.Tensor:
    """``paged_gather`` of an fp8 pool with its scales [n_pages, Hkv, PAGE],
    dequantised: ``float(byte) * scale`` in ``dtype`` or wider (the product
    with the fp32 scale is not rounded down to a narrower ``dtype``)."""
    # gathered as bytes: indexing lacks fp8 on some devices
    rows = paged_gather(pool.view(torch.uint8), block_table, n_rows)
    return rows.view(pool.dtype).to(dtype) \
        * paged_gather(scale[..., None], block_table, n_rows)


def _gathered(pool, scale, block_table, n_rows, dtype):
    if scale is None:
        return paged_gather(pool, block_table, n_rows)
    return paged_gather_dequant(pool, scale, block_table, n_rows, dtype)


def paged_decode_attention_reference(q, k_pool, v_pool, block_table, slopes,
                                     scale, pos, k_scale=None, v_scale=None):
    """``decode_attention_reference`` on the gathered cache (dequantised when
    the scales of an fp8 cache are given), in the dtype of ``q`` (fp64 in,
    fp64 oracle out)."""
    n_rows = block_table.size(1) * k_pool.size(2)
    return decode_attention_reference(
        q, _gathered(k_pool, k_scale, block_table, n_rows, q.dtype),
        _gathered(v_pool, v_scale, block_table, n_rows, q.dtype), slopes,
        scale, pos)


def paged_prefill_attention_reference(q, k_pool, v_pool, block_table, slopes,
                                      scale, start, k_scale=None,
                                      v_scale=None):
    """Pure-torch definition of prefill attention over the paged cache, in the
    dtype of ``q`` (fp64 in, fp64 oracle out).

    q [B,H,Sq,D]; row ``i`` of batch row ``b`` sits at ``p = start[b] + i``
    and sees keys ``0..p`` of the gathered cache with bias
    ``slopes[h] * (j - p)``.  Rows with ``p`` outside
    ``[0, max_pages * PAGE)`` give zeros.  With the scales of an fp8 cache
    the gather is dequantised.  Returns [B,H,Sq,D]."""
    B, H, Sq, D = q.shape
    Hkv = k_pool.size(1)
    G = H // Hkv
    cap = block_table.size(1) * k_pool.size(2)
    k = _gathered(k_pool, k_scale, block_table, cap, q.dtype).to(q.dtype)
    v = _gathered(v_pool, v_scale, block_table, cap, q.dtype).to(q.dtype)
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


def paged_varlen_attention_reference(q, k_pool, v_pool, block_table, slopes,
                                     scale, cu_q, start, k_scale=None,
                                     v_scale=None):
    """Pure-torch definition of attention over a token-packed ragged batch,
    in the dtype of ``q`` (fp64 in, fp64 oracle out):
    ``paged_prefill_attention_reference`` applied per sequence.

    q [T,H,D]; sequence ``b`` owns the packed rows ``cu_q[b] .. cu_q[b+1]-1``,
    its row ``i`` sits at ``start[b] + i`` and sees the keys of
    ``block_table[b]``.  Rows ``t >= cu_q[B]`` are padding and give zeros.
    Returns [T,H,D]."""
    cu = cu_q.tolist()
    B = len(cu) - 1
    st = start.to(device=q.device, dtype=torch.long).reshape(-1).expand(B)
    o = torch.zeros_like(q)
    for b in range(B):
        if cu[b + 1] > cu[b]:
            rows = slice(cu[b], cu[b + 1])
            o[rows] = paged_prefill_attention_reference(
                q[rows].transpose(0, 1)[None], k_pool, v_pool,
                block_table[b:b + 1], slopes, scale, st[b:b + 1], k_scale,
                v_scale)[0].transpose(0, 1)
    return o


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


def quantize_rows_fp8(x: torch.Tensor):
    """The cache format's quantiser on the rows ``x[..., :]``: e4m3fn bytes
    of ``clamp(x * (448 / amax), -448, 448)`` and the fp32 scales
    ``amax / 448`` (shape of ``x`` without its last dim); an all-zero row
    gives scale 0 and zero bytes."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    inv = torch.where(amax > 0, 448.0 / amax, torch.zeros_like(amax))
    q = (xf * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q, (amax / 448.0).squeeze(-1)


def paged_kv_write_fp8_reference(k_new, v_new, k_pool, v_pool, k_scale,
                                 v_scale, block_table, start):
    """``paged_kv_write_reference`` into an fp8 cache: every kept row of
    every kv head is quantised on its own (``quantize_rows_fp8``) and its
    bytes and scale are written in place."""
    B, _, S_new, _ = k_new.shape
    page = k_pool.size(2)
    capacity = block_table.size(1) * page
    st = start.to(device=k_new.device, dtype=torch.long).reshape(-1).expand(B)
    row = st[:, None] + torch.arange(S_new, device=k_new.device)   # [B, S]
    keep = (row >= 0) & (row < capacity)
    safe = row.clamp(0, capacity - 1)
    ids = block_table.long().gather(1, safe // page)[keep]         # [n]
    slot = (safe % page)[keep]
    for new, pool, scales in ((k_new, k_pool, k_scale),
                              (v_new, v_pool, v_scale)):
        q, sc = quantize_rows_fp8(new.transpose(1, 2)[keep])  # [n, Hkv, D]
        # assigned as bytes: indexed assignment lacks fp8 on some devices
        pool.view(torch.uint8)[ids, :, slot] = q.view(torch.uint8)
        scales[ids, :, slot] = sc


def _rotate_exact(x, theta, p):
    """Half-split rotation of ``x`` [B,Hx,S,D] at positions ``p`` [B,S], the
    angle ``p * theta^(-2d/D)`` in fp64, the arithmetic in the dtype of
    ``x``."""
    half = x.size(-1) // 2
    d = torch.arange(half, device=x.device, dtype=torch.float64)
    ang = p.double()[:, None, :, None] * theta ** (-2.0 * d / x.size(-1))
    cos, sin = ang.cos().to(x.dtype), ang.sin().to(x.dtype)
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def paged_rope_write_reference(q, k_new, v_new, k_pool, v_pool, block_table,
                               start, theta, k_scale=None, v_scale=None):
    """Pure-torch definition of ``paged_rope_write``, in the dtype of ``q``
    (fp64 in, fp64 oracle out): q [B,H,S,D] and k_new [B,Hkv,S,D] rotated at
    ``p = start[b] + s`` with the exact angle, the rotated K and v_new written
    by ``paged_kv_write_reference`` (``paged_kv_write_fp8_reference`` with the
    scales of an fp8 cache).  Returns the rotated q, rows with ``p`` outside
    ``[0, max_pages * PAGE)`` zero."""
    B, _, S, _ = q.shape
    cap = block_table.size(1) * k_pool.size(2)
    st = start.to(device=q.device, dtype=torch.long).reshape(-1).expand(B)
    p = st[:, None] + torch.arange(S, device=q.device)             # [B, S]
    k_rot = _rotate_exact(k_new, theta, p)
    if k_scale is None:
        paged_kv_write_reference(k_rot, v_new, k_pool, v_pool, block_table,
                                 start)
    else:
        paged_kv_write_fp8_reference(k_rot, v_new, k_pool, v_pool, k_scale,
                                     v_scale, block_table, start)
    in_range = (p >= 0) & (p < cap)
    return _rotate_exact(q, theta, p).masked_fill(
        ~in_range[:, None, :, None], 0)


_FREQ_TABS = {}


def rope_freq_table(theta: float, D: int, device) -> torch.Tensor:
    """The kernel's frequency table for ``(theta, D)`` on ``device``, built
    once: fp32 [D/2, 2], row ``j`` the hi/lo pair of
    ``theta^(-2j/D) / (2 pi)`` (revolutions per position), from fp64."""
    key = (float(theta), D, torch.device(device))
    tab = _FREQ_TABS.get(key)
    if tab is None:
        j = torch.arange(D // 2, dtype=torch.float64)
        f = float(theta) ** (-2.0 * j / D) / (2.0 * math.pi)
        hi = f.float()
        lo = (f - hi.double()).float()
        tab = torch.stack([hi, lo], dim=1).contiguous().to(device)
        _FREQ_TABS[key] = tab
    return tab


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


def paged_fp8_kernel_supported(q: torch.Tensor, k_pool: torch.Tensor) -> bool:
    """``paged_kernel_supported`` for an fp8 cache: the same conditions on
    ``q`` (GPU, bf16, extension present, D in {64, 128},
    ``PG_DECODE_ATTN != "0"``) and on the page size, with e4m3fn pools on the
    GPU.  ``q`` may hold any number of rows: the write and the prefill
    kernel use the same condition.  Not gated on speed: fp8 is opt-in, and
    what it buys is capacity (twice the tokens per pool byte) and, for
    prefill, activation memory bounded by the chunk — the reference
    materialises the dequantised cache at full capacity and a score tensor
    over it — and both hold whatever the kernels time
    (profiles/paged_fp8_decode_attn.md, profiles/paged_fp8_prefill_attn.md)."""
    q1 = q[:, :, :1]
    # q1 also stands in for the bf16 cache operand of the decode condition
    return k_pool.dtype == torch.float8_e4m3fn and k_pool.is_cuda \
        and decode_kernel_supported(q1, q1) \
        and k_pool.size(2) in (16, 32, 64, 128)


def _check_scales(name, k_pool, k_scale, v_scale):
    if (k_scale is None) != (v_scale is None):
        raise ValueError(f"{name}: k_scale and v_scale go together")
    if k_scale is not None and k_pool.dtype != torch.float8_e4m3fn:
        raise ValueError(f"{name}: scales are for float8_e4m3fn pools, got "
                         f"{k_pool.dtype}")
    return k_scale is not None


def _inference_only(name, tensors):
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(
            f"{name} is inference-only (no backward): call it under "
            "torch.no_grad() or with tensors that do not require grad")


def paged_decode_attention(q, k_pool, v_pool, block_table, slopes, scale, pos,
                           k_scale=None, v_scale=None):
    """The kernel when ``paged_kernel_supported``, else the reference.
    Logical [B,H,1,D]; the kernel's result is physically [B,1,H,D].  With
    ``k_scale`` / ``v_scale`` the pools are an fp8 cache: the fp8 kernel when
    ``paged_fp8_kernel_supported``, else the reference on the dequantised
    gather."""
    _inference_only("paged_decode_attention", (q, k_pool, v_pool, slopes))
    if _check_scales("paged_decode_attention", k_pool, k_scale, v_scale):
        if not (q.size(-2) == 1 and paged_fp8_kernel_supported(q, k_pool)):
            return paged_decode_attention_reference(
                q, k_pool, v_pool, block_table, slopes, scale, pos,
                k_scale, v_scale)
        return get_extension(required=True).paged_decode_attn_fp8(
            q, k_pool, v_pool, k_scale, v_scale, block_table,
            slopes.to(device=q.device, dtype=torch.float32), scale, pos, 0)
    if not (q.size(-2) == 1 and paged_kernel_supported(q, k_pool)):
        return paged_decode_attention_reference(
            q, k_pool, v_pool, block_table, slopes, scale, pos)
    ext = get_extension(required=True)
    return ext.paged_decode_attn(
        q, k_pool, v_pool, block_table,
        slopes.to(device=q.device, dtype=torch.float32), scale, pos, 0)


def paged_prefill_attention(q, k_pool, v_pool, block_table, slopes, scale,
                            start, k_scale=None, v_scale=None):
    """Attention of the ``Sq >= 1`` rows of ``q`` [B,H,Sq,D] at positions
    ``start[b] + i`` over the pools, which already hold the rows' own K/V:
    the kernel when ``paged_kernel_supported``, else the reference.  The
    kernel's result is physically [B,Sq,H,D].

    With ``k_scale`` / ``v_scale`` the pools are an fp8 cache: the fp8
    kernel when ``paged_fp8_kernel_supported``, else the reference on the
    dequantised gather, in the dtype of ``q``."""
    _inference_only("paged_prefill_attention", (q, k_pool, v_pool, slopes))
    if _check_scales("paged_prefill_attention", k_pool, k_scale, v_scale):
        if not paged_fp8_kernel_supported(q, k_pool):
            return paged_prefill_attention_reference(
                q, k_pool, v_pool, block_table, slopes, scale, start,
                k_scale, v_scale)
        return get_extension(required=True).paged_prefill_attn_fp8(
            q, k_pool, v_pool, k_scale, v_scale, block_table,
            slopes.to(device=q.device, dtype=torch.float32), scale, start)
    if not paged_kernel_supported(q, k_pool):
        return paged_prefill_attention_reference(
            q, k_pool, v_pool, block_table, slopes, scale, start)
    ext = get_extension(required=True)
    return ext.paged_prefill_attn(
        q, k_pool, v_pool, block_table,
        slopes.to(device=q.device, dtype=torch.float32), scale, start)


def paged_varlen_attention(q, k_pool, v_pool, block_table, slopes, scale,
                           cu_q, start, k_scale=None, v_scale=None,
                           n_splits=None):
    """Attention of a token-packed ragged batch ``q`` [T,H,D] over the pools,
    which already hold the rows' own K/V: sequence ``b`` owns the rows
    ``cu_q[b] .. cu_q[b+1]-1`` (int32 [B+1]) at positions ``start[b] + i``
    (int64 [B]) over ``block_table[b]``; rows ``t >= cu_q[B]`` give zeros.
    One launch of ``paged_varlen_attn`` (csrc/paged_varlen_attention.hip, the
    GQA group sharing each staged K/V tile) when ``paged_kernel_supported``,
    else the reference.  Returns [T,H,D].

    With ``k_scale`` / ``v_scale`` the pools are an fp8 cache: one launch of
    ``paged_varlen_attn_fp8`` (csrc/paged_fp8_varlen_attention.hip) when
    ``paged_fp8_kernel_supported``, else the reference on the dequantised
    gather, in the dtype of ``q``.  Not gated on speed, as stated there
    (measured: profiles/paged_fp8_varlen_attn.md).

    Measured (profiles/paged_varlen_attn.md): 0.39-0.65x the time of the
    eight B = 1 ``paged_prefill_attn`` launches it replaces on 8 ragged
    prompts (spreads <= 5 %).  It is NOT the faster kernel for an
    equal-length batch without a GQA group (1.01-1.05x
    ``paged_prefill_attn``) or for length-1 rows behind a context (2.0-2.3x
    ``paged_decode_attn``); callers keep those on their kernels.

    ``n_splits`` (an int; ``None`` is the call above, bit for bit) selects
    ``paged_varlen_split_attn`` (csrc/paged_varlen_split_attention.hip) when
    ``paged_kernel_supported``: the same attention with every tile's visible
    keys divided among ``n_splits`` workgroups (0 = the shapes-only auto
    plan, 1..64 forced) and a body for tiles of decode rows, which is what a
    packed forward that mixes decode rows with prefill pieces wants
    (profiles/paged_mixed_attn.md).  Elsewhere it runs the same reference,
    which takes no plan.  With ``k_scale`` / ``v_scale`` it selects
    ``paged_varlen_split_attn_fp8``
    (csrc/paged_fp8_varlen_split_attention.hip) when
    ``paged_fp8_kernel_supported``: the same plan and combine kernel over the
    fp8 cache, decode rows converted from bytes in registers
    (profiles/paged_fp8_mixed_attn.md)."""
    _inference_only("paged_varlen_attention", (q, k_pool, v_pool, slopes))
    if n_splits is not None and not 0 <= int(n_splits) <= 64:
        raise ValueError("paged_varlen_attention: n_splits must be None, 0 "
                         f"(auto) or 1..64, got {n_splits}")
    if _check_scales("paged_varlen_attention", k_pool, k_scale, v_scale):
        if not paged_fp8_kernel_supported(q[None], k_pool):
            return paged_varlen_attention_reference(
                q, k_pool, v_pool, block_table, slopes, scale, cu_q, start,
                k_scale, v_scale)
        if n_splits is not None:
            return get_extension(required=True).paged_varlen_split_attn_fp8(
                q, k_pool, v_pool, k_scale, v_scale, block_table,
                slopes.to(device=q.device, dtype=torch.float32), scale, cu_q,
                start, int(n_splits))
        return get_extension(required=True).paged_varlen_attn_fp8(
            q, k_pool, v_pool, k_scale, v_scale, block_table,
            slopes.to(device=q.device, dtype=torch.float32), scale, cu_q,
            start)
    if not paged_kernel_supported(q[None], k_pool):
        return paged_varlen_attention_reference(
            q, k_pool, v_pool, block_table, slopes, scale, cu_q, start)
    if n_splits is not None:
        return get_extension(required=True).paged_varlen_split_attn(
            q, k_pool, v_pool, block_table,
            slopes.to(device=q.device, dtype=torch.float32), scale, cu_q,
            start, int(n_splits))
    return get_extension(required=True).paged_varlen_attn(
        q, k_pool, v_pool, block_table,
        slopes.to(device=q.device, dtype=torch.float32), scale, cu_q, start)


def paged_kv_write(k_new, v_new, k_pool, v_pool, block_table, start,
                   k_scale=None, v_scale=None):
    """Write the new rows into the pools (in place): the kernel when
    ``paged_kernel_supported``, else the reference.  With ``k_scale`` /
    ``v_scale`` (fp8 cache) the rows are quantised and their scales written
    too: the fp8 kernel when ``paged_fp8_kernel_supported``, else
    ``paged_kv_write_fp8_reference``."""
    _inference_only("paged_kv_write", (k_new, v_new, k_pool, v_pool))
    if _check_scales("paged_kv_write", k_pool, k_scale, v_scale):
        if not paged_fp8_kernel_supported(k_new, k_pool):
            return paged_kv_write_fp8_reference(
                k_new, v_new, k_pool, v_pool, k_scale, v_scale, block_table,
                start)
        return get_extension(required=True).paged_kv_write_fp8(
            k_new, v_new, k_pool, v_pool, k_scale, v_scale, block_table,
            start)
    if not paged_kernel_supported(k_new, k_pool):
        return paged_kv_write_reference(k_new, v_new, k_pool, v_pool,
                                        block_table, start)
    get_extension(required=True).paged_kv_write(
        k_new, v_new, k_pool, v_pool, block_table, start)


def paged_rope_write(q, k_new, v_new, k_pool, v_pool, block_table, start,
                     theta, k_scale=None, v_scale=None):
    """Rotate q [B,H,S,D] and k_new [B,Hkv,S,D] at positions ``start[b] + s``
    and write the rotated K and v_new into the pools (in place); returns the
    rotated q.  One kernel launch when ``paged_kernel_supported`` (bf16
    cache) or ``paged_fp8_kernel_supported`` (fp8 cache, ``k_scale`` /
    ``v_scale`` given) and ``PG_PAGED_ROPE != "0"``; the kernel's result is
    physically [B,S,H,D] and its rows outside ``[0, max_pages * PAGE)`` are
    zeros.  Otherwise ``rope_at_position`` twice and ``paged_kv_write``.

    Measured (profiles/paged_rope_write.md): the fused call takes 0.05x the
    time of the unfused sequence at every recorded row (llama-7b and GQA
    heads, B 1/8 at S 1, S 512, bf16 and fp8; spreads under 10 %), so no
    shape region is excluded."""
    _inference_only("paged_rope_write", (q, k_new, v_new, k_pool, v_pool))
    fp8 = _check_scales("paged_rope_write", k_pool, k_scale, v_scale)
    supported = paged_fp8_kernel_supported if fp8 else paged_kernel_supported
    if os.environ.get("PG_PAGED_ROPE", "1") == "0" \
            or not supported(q, k_pool):
        from pipegoose_amd.ops.rope import rope_at_position
        q = rope_at_position(q, theta, start)
        k_new = rope_at_position(k_new, theta, start)
        paged_kv_write(k_new, v_new, k_pool, v_pool, block_table, start,
                       k_scale=k_scale, v_scale=v_scale)
        return q
    ext = get_extension(required=True)
    tab = rope_freq_table(theta, q.size(-1), q.device)
    if fp8:
        return ext.paged_rope_write_fp8(q, k_new, v_new, k_pool, v_pool,
                                        k_scale, v_scale, block_table, start,
                                        float(theta), tab)
    return ext.paged_rope_write(q, k_new, v_new, k_pool, v_pool, block_table,
                                start, float(theta), tab)
