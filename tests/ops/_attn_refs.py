"""fp64 references, seeded input generators and the stock-torch baselines for
the causal + ALiBi attention kernels (csrc/attention.hip).  Plain helpers:
imported by test_attn_refs_cpu.py (which checks that the references and the
generators are sound, and that the tolerance rule rejects wrong kernels) and
by test_attn_edges_gpu.py.  The comparison itself is _rowwise_refs.check_close.

Conventions: q, do [B, H, S, D]; k, v [B, Hkv, S, D] with H % Hkv == 0 (q
head h reads kv head h // (H // Hkv)); slopes [H]; key j of the block sits at
position j + kv_off relative to the block's queries, is visible to row i when
j + kv_off <= i, and carries the bias slope_h * (j + kv_off - i).

The references are written out in float64 from the definition; none calls
scaled_dot_product_attention, softmax or logsumexp.
"""
import math

import torch
import torch.nn.functional as TF

TILE = 64       # kv rows per tile in every forward kernel


# ------------------------------------------------------------------ references
def _expand_kv(t, H):
    """[B, Hkv, S, D] -> [B, H, S, D], each kv head repeated for its group."""
    B, Hkv, S, D = t.shape
    assert H % Hkv == 0
    return t[:, :, None].expand(B, Hkv, H // Hkv, S, D).reshape(B, H, S, D)


def _reduce_kv(t, Hkv):
    """[B, H, S, D] -> [B, Hkv, S, D], summed over each kv head's group."""
    B, H, S, D = t.shape
    return t.reshape(B, Hkv, H // Hkv, S, D).sum(2)


def visible(Sq, Sk, kv_off, device=None):
    """[Sq, Sk] bool: key j is visible to row i."""
    i = torch.arange(Sq, device=device)[:, None]
    j = torch.arange(Sk, device=device)[None, :]
    return j + kv_off <= i


def scores(q, k, slopes, scale, kv_off, dtype=torch.float64):
    """[B, H, Sq, Sk] scores in ``dtype`` with -inf at the masked positions."""
    H, Sq, Sk = q.size(1), q.size(2), k.size(2)
    qd, kd = q.to(dtype), _expand_kv(k.to(dtype), H)
    i = torch.arange(Sq, device=q.device)[:, None]
    j = torch.arange(Sk, device=q.device)[None, :]
    rel = (j + kv_off - i).to(dtype)
    s = scale * (qd @ kd.transpose(-1, -2)) \
        + slopes.to(device=q.device, dtype=dtype)[:, None, None] * rel
    return torch.where(visible(Sq, Sk, kv_off, q.device), s,
                       torch.full_like(s, -math.inf))


def attn_ref(q, k, v, slopes, scale, kv_off):
    """float64 (o [B, H, S, D], lse [B, H, S]); lse is the natural log of the
    row's sum of exp(score).  Every row must see at least one key."""
    s = scores(q, k, slopes, scale, kv_off)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    o = (e @ _expand_kv(v.double(), q.size(1))) / l
    return o, (m + torch.log(l)).squeeze(-1)


def attn_bwd_ref(do, q, k, v, o, lse, slopes, scale, kv_off):
    """float64 (dq, dk, dv) from a GIVEN o and lse: p = exp(s - lse),
    delta = rowsum(do * o), ds = p * (dp - delta) * scale.  With the block's
    own o and lse this is the gradient of attn_ref; with the merged o and lse
    of several blocks it is this block's share of the whole gradient."""
    H, Hkv = q.size(1), k.size(1)
    dod, qd, od = do.double(), q.double(), o.double()
    kd, vd = _expand_kv(k.double(), H), _expand_kv(v.double(), H)
    p = torch.exp(scores(q, k, slopes, scale, kv_off) - lse.double()[..., None])
    dp = dod @ vd.transpose(-1, -2)
    delta = (dod * od).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = ds @ kd
    dk = _reduce_kv(ds.transpose(-1, -2) @ qd, Hkv)
    dv = _reduce_kv(p.transpose(-1, -2) @ dod, Hkv)
    return dq, dk, dv


def merge_blocks(parts):
    """Log-sum-exp merge of (o, lse) pairs of one q block over several kv
    blocks, in float64: the (o, lse) of attention over their union."""
    os_ = [o.double() for o, _ in parts]
    ls = [l.double() for _, l in parts]
    m = ls[0]
    for l in ls[1:]:
        m = torch.maximum(m, l)
    ws = [torch.exp(l - m) for l in ls]
    wsum = sum(ws)
    o = sum(w[..., None] * o for w, o in zip(ws, os_)) / wsum[..., None]
    return o, m + torch.log(wsum)


def zero_q_facts(v, H, kv_off):
    """What q = 0 with slope 0 must give: o_i the mean of the keys row i sees,
    lse_i the log of their number.  float64 (o, lse)."""
    S = v.size(2)
    jmax = last_visible(S, kv_off).to(v.device)
    n = (jmax + 1).double()
    o = _expand_kv(v.double(), H).cumsum(2)[:, :, jmax, :] / n[:, None]
    return o, torch.log(n).expand(v.size(0), H, S)


def ring_cp2(fwd, bwd, c, acc_dtype, out_dtype):
    """Context parallelism over two ranks, on one device: the sequence of case
    ``c`` (length 2 S) in two halves, through the block primitives
        fwd(q, k, v, kv_off) -> (o, lse)
        bwd(do, q, k, v, o, lse, kv_off) -> (dq, dk, dv)
    in the order and with the arithmetic of _RingAttentionRotate: rank 1 runs
    (q1, kv1, 0) then (q1, kv0, -S) and merges in ``acc_dtype``; the backward
    hands every block the MERGED o (rounded to ``out_dtype``) and lse, and
    partial grads are summed in ``acc_dtype``.  Returns the whole sequence's
    o, lse, dq, dk, dv."""
    S = c["q"].size(2) // 2
    q0, q1 = c["q"][:, :, :S], c["q"][:, :, S:]
    k0, k1 = c["k"][:, :, :S], c["k"][:, :, S:]
    v0, v1 = c["v"][:, :, :S], c["v"][:, :, S:]
    do0, do1 = c["do"][:, :, :S], c["do"][:, :, S:]

    def merged(blocks):
        o_num = w_sum = m_run = None
        for o_r, lse_r in blocks:
            o_r, lse_r = o_r.to(acc_dtype), lse_r.to(acc_dtype)[..., None]
            if o_num is None:
                m_run, o_num, w_sum = lse_r, o_r, torch.ones_like(lse_r)
            else:
                m_new = torch.maximum(m_run, lse_r)
                o_num = o_num * torch.exp(m_run - m_new) \
                    + o_r * torch.exp(lse_r - m_new)
                w_sum = w_sum * torch.exp(m_run - m_new) \
                    + torch.exp(lse_r - m_new)
                m_run = m_new
        return (o_num / w_sum).to(out_dtype), \
            (m_run + torch.log(w_sum)).squeeze(-1)

    o0, l0 = merged([fwd(q0, k0, v0, 0)])
    o1, l1 = merged([fwd(q1, k1, v1, 0), fwd(q1, k0, v0, -S)])
    g00 = bwd(do0, q0, k0, v0, o0, l0, 0)
    g11 = bwd(do1, q1, k1, v1, o1, l1, 0)
    g10 = bwd(do1, q1, k0, v0, o1, l1, -S)
    a = lambda t: t.to(acc_dtype)
    dq = torch.cat([a(g00[0]), a(g11[0]) + a(g10[0])], 2)
    dk = torch.cat([a(g00[1]) + a(g10[1]), a(g11[1])], 2)
    dv = torch.cat([a(g00[2]) + a(g10[2]), a(g11[2])], 2)
    return {"o": torch.cat([o0, o1], 2), "lse": torch.cat([l0, l1], 2),
            "dq": dq.to(out_dtype), "dk": dk.to(out_dtype),
            "dv": dv.to(out_dtype)}


# ------------------------------------------------------------------- baselines
def mask_bias(Sq, Sk, slopes, kv_off, device, dtype):
    """The explicit additive mask [1, H, Sq, Sk] that the sdpa fallback of
    alibi_attention is given: bias formed in fp32, -inf above the diagonal,
    then cast to the dtype of q."""
    i = torch.arange(Sq, device=device)[:, None]
    j = torch.arange(Sk, device=device)[None, :]
    rel = (j + kv_off - i).float()
    bias = slopes.to(device=device, dtype=torch.float32)[:, None, None] * rel
    bias = bias.masked_fill(~visible(Sq, Sk, kv_off, device), -math.inf)
    return bias.to(dtype)[None]


def sdpa_base(q, k, v, do, slopes, scale, kv_off):
    """Stock torch on the same tensors in their own dtype: (o, dq, dk, dv)
    from scaled_dot_product_attention with the explicit mask, plus autograd;
    GQA through repeat_interleave."""
    H, Hkv = q.size(1), k.size(1)
    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    bias = mask_bias(q.size(2), k.size(2), slopes, kv_off, q.device, q.dtype)
    o = TF.scaled_dot_product_attention(
        ql, kl.repeat_interleave(H // Hkv, dim=1),
        vl.repeat_interleave(H // Hkv, dim=1), attn_mask=bias, scale=scale)
    o.backward(do)
    return o.detach(), ql.grad, kl.grad, vl.grad


def lse_base(q, k, slopes, scale, kv_off):
    """torch.logsumexp of the fp32 scores formed from the given inputs."""
    return torch.logsumexp(
        scores(q, k, slopes, scale, kv_off, dtype=torch.float32), dim=-1)


# ------------------------------------------------------------------ generators
# All draws are float64 on the CPU from a seeded generator, then rounded to
# bf16, so a case is the same tensor on every machine.
SLOPE_SETS = {
    "zero": [0.0, 0.0],             # Llama and ring attention pass zeros
    "mild": [2.0 ** -8, 0.5],
    "steep": [4.0, 0.0625],         # slope 4: keys ~25 positions back underflow
}
PEAKED = ["peaked_first", "peaked_diag", "peaked_last"]
FAMILIES = ["randn"] + PEAKED + ["rising", "falling", "zero_q", "v_offset",
                                 "do_zero"]
PEAK_SCORE, PEAK_NOISE = 60.0, 9.7
RAMP_LO, RAMP_SPAN = 0.25, 6.0


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def last_visible(S, kv_off):
    """[S] index of the last key each row sees."""
    return (torch.arange(S) - kv_off).clamp(max=S - 1)


def peak_targets(family, S, kv_off):
    """[S] the key planted to dominate each row: in the first kv tile, on the
    mask edge (the block diagonal for rows whose edge lies past the block),
    or in the last tile that the row sees."""
    i = torch.arange(S)
    jmax = last_visible(S, kv_off)
    if family == "peaked_first":
        return (7 * i) % torch.minimum(jmax + 1, torch.tensor(TILE))
    if family == "peaked_diag":
        edge = i - kv_off
        return torch.where(edge <= S - 1, edge, i)
    assert family == "peaked_last"
    tile0 = (jmax // TILE) * TILE
    return tile0 + (5 * i) % (jmax - tile0 + 1)


def attn_case(family, slope_set, H, Hkv, S, D, kv_off=0, B=1, seed=0):
    """dict of bf16 q, k, v, do, fp32 slopes and the scale D**-0.5 (CPU)."""
    assert H == 2 and family in FAMILIES
    g = _gen(seed)
    q, do = _randn((B, H, S, D), g), _randn((B, H, S, D), g)
    k, v = _randn((B, Hkv, S, D), g), _randn((B, Hkv, S, D), g)
    if family in PEAKED:
        # k = 3 g;  q_i = (PEAK_SCORE / 3) * unit(k_t(i)) + PEAK_NOISE / 3 g'.
        # With scale D**-0.5 and |k_t| ~ 3 sqrt(D) the planted score is
        # PEAK_SCORE +- PEAK_NOISE and the others are N(0, PEAK_SCORE^2 / D +
        # PEAK_NOISE^2): std 12.3 at D=64, 11 at D=128.  Their maximum over a
        # few hundred keys is near 40, so nearly every row is one-hot on the
        # planted key and a few have a real competitor
        k = 3.0 * k
        t = peak_targets(family, S, kv_off)
        kt = _expand_kv(k, H)[:, :, t, :]                    # [B, H, S, D]
        q = (PEAK_SCORE / 3.0) * kt / kt.norm(dim=-1, keepdim=True) \
            + (PEAK_NOISE / 3.0) * q
    elif family in ("rising", "falling"):
        # all rows near one direction u, |k_j| a linear ramp in j: the scores
        # of a row rise (fall) by RAMP_SPAN * sqrt(D) over the block
        u = torch.where(_randn((D,), g) >= 0, 1.0, -1.0).double()
        ramp = torch.arange(S, dtype=torch.float64) / S
        if family == "falling":
            ramp = 1.0 - ramp
        amp = RAMP_LO + RAMP_SPAN * ramp
        k = amp[:, None] * (u + 0.15 * k)
        q = u + 0.15 * q
    elif family == "zero_q":
        q = torch.zeros_like(q)
    elif family == "v_offset":
        v = 100.0 + v
        do = 10.0 + do
    elif family == "do_zero":
        do = torch.zeros_like(do)
    return {"q": q.bfloat16(), "k": k.bfloat16(), "v": v.bfloat16(),
            "do": do.bfloat16(),
            "slopes": torch.tensor(SLOPE_SETS[slope_set], dtype=torch.float32),
            "scale": D ** -0.5}


# --------------------------------------------------------------- mask positions
def mask_offsets(S):
    """kv_off values of the mask-position tests: every multiple of 64 strictly
    inside (-S, 0), the non-multiples -1, -63, -65 where they lie inside it,
    and three fully visible ones.  Each leaves every row a visible key."""
    inside = list(range(-S + 64, 0, 64)) + [o for o in (-1, -63, -65) if o > -S]
    return sorted(inside, reverse=True) + [-S, -S - 64, -2 * S]
