"""Attention backward (v2 kernels) vs an fp32 torch oracle, at the smallest
shapes that reach each path of the softmax/dS phase: diagonal (masked) and
off-diagonal (mask-free) sub-tiles, 4- and 8-wave builds, D=64 and D=128,
GQA restaging, kv offsets (ring attention), the exp2 flush path, and the
strided fused-QKV inputs.

Error measure: max-abs error over the reference's max-abs (floored at 1),
the project's normalisation.  Two bounds per gradient:
  * HARD = 5e-2, the project's existing limit;
  * a tight one: twice the error of the previous kernels (the build before
    the softmax-phase rewrite) on the same seeds and shapes, listed in
    _PARENT_ERR.  Both builds are dominated by the bf16 rounding of P and
    dS, so moving one rounding shifts a tensor-wide max by tens of percent;
    a real defect (lost scale, wrong row statistic, unmasked element) gives
    errors of order one.
The rewritten phase keeps every rounding where the previous kernels had it,
and on an MI355X it reproduced their gradients bit for bit on all of these
cases, so the measured errors are the listed ones.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HARD = 5e-2

# case id -> (B, H, Hkv, S, D, kv_off, slopes)
#   slopes: "bloom" = BLOOM's own for the head count, or a float for all heads
CASES = {
    "d64_w8_diag":      (1, 2, 2, 256, 64, 0, "bloom"),   # every tile diagonal
    "d64_w8_offdiag":   (1, 2, 2, 512, 64, 0, "bloom"),   # + mask-free body
    "d64_w4_s128":      (1, 2, 2, 128, 64, 0, "bloom"),
    "d64_w4_s384":      (1, 2, 2, 384, 64, 0, "bloom"),
    "d128_w8_s256":     (1, 1, 1, 256, 128, 0, "bloom"),
    "d128_w8_s512":     (1, 1, 1, 512, 128, 0, "bloom"),
    "d128_w4_s384":     (1, 1, 1, 384, 128, 0, "bloom"),
    "gqa_s512":         (1, 4, 2, 512, 64, 0, "bloom"),   # gq loop restages
    "kvoff_m256":       (1, 2, 2, 256, 64, -256, "bloom"),  # fully visible
    "kvoff_ring":       (1, 2, 2, 256, 64, -256 * 7, "bloom"),  # large offset
    "slope07_flush":    (1, 2, 2, 512, 64, 0, 0.7),       # far keys < 2^-126
}

# Normalised errors (dq, dk, dv) of the previous kernels on these cases,
# measured on an MI355X; the tight bound is twice each.
_PARENT_ERR = {
    "d128_w4_s384": (2.8224e-03, 2.4397e-03, 2.3326e-03),
    "d128_w8_s256": (4.3538e-03, 3.2322e-03, 2.2523e-03),
    "d128_w8_s512": (5.9196e-03, 3.9792e-03, 1.5748e-03),
    "d64_w4_s128": (2.8613e-03, 2.9157e-03, 1.5759e-03),
    "d64_w4_s384": (3.3504e-03, 2.5488e-03, 2.6272e-03),
    "d64_w8_diag": (2.8204e-03, 3.7861e-03, 2.6379e-03),
    "d64_w8_offdiag": (2.8825e-03, 2.9772e-03, 2.6442e-03),
    "fused_qkv_s256": (5.4612e-03, 3.2066e-03, 3.5384e-03),
    "gqa_s512": (3.6252e-03, 3.8502e-03, 3.4177e-03),
    "kvoff_m256": (3.4865e-03, 3.2362e-03, 2.0828e-03),
    "kvoff_ring": (3.8348e-03, 2.6815e-03, 2.7796e-03),
    "slope07_flush": (3.7320e-03, 3.5665e-03, 3.7073e-03),
}


def _ext():
    from pipegoose_amd.ops import get_extension
    return get_extension(required=True)


def _slopes(kind, H):
    if kind == "bloom":
        from pipegoose_amd.models.bloom import alibi_slopes
        return alibi_slopes(H).float().cuda()
    return torch.full((H,), float(kind), device="cuda")


def _oracle_grads(q, k, v, do, slopes, scale, kv_off):
    """fp32 attention with ALiBi and the causal mask at shifted kv
    positions (as nn.ring_attention._block_attention_ref), GQA by expanding
    kv heads; returns fp32 (dq, dk, dv)."""
    H, Hkv = q.size(1), k.size(1)
    q2 = q.detach().float().requires_grad_(True)
    k2 = k.detach().float().requires_grad_(True)
    v2 = v.detach().float().requires_grad_(True)
    ke = k2.repeat_interleave(H // Hkv, dim=1)
    ve = v2.repeat_interleave(H // Hkv, dim=1)
    iq = torch.arange(q.size(2), device=q.device)
    jk = torch.arange(k.size(2), device=q.device) + kv_off
    rel = jk[None, :] - iq[:, None]
    bias = slopes[:, None, None] * rel[None].float()
    bias = bias.masked_fill(rel[None] > 0, float("-inf"))
    scores = (q2 @ ke.transpose(-1, -2)) * scale + bias[None]
    o = torch.softmax(scores, dim=-1) @ ve
    o.backward(do.float())
    return q2.grad, k2.grad, v2.grad


def _norm_err(got, want):
    return ((got.float() - want).abs().max()
            / want.abs().max().clamp_min(1.0)).item()


def _inputs(case):
    B, H, Hkv, S, D, kv_off, kind = CASES[case]
    torch.manual_seed(20 + sorted(CASES).index(case))
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn_like(k)
    do = torch.randn_like(q)
    return q, k, v, do, _slopes(kind, H), D ** -0.5, kv_off


@functools.lru_cache(maxsize=None)
def _run(case):
    """One forward + backward of the kernels and one oracle per case,
    shared by the tests below; returns the kernel gradients and the
    normalised errors."""
    ext = _ext()
    q, k, v, do, slopes, scale, kv_off = _inputs(case)
    o, lse = ext.attn_fwd(q, k, v, slopes, scale, kv_off)
    got = ext.attn_bwd(do, q, k, v, o, lse, slopes, scale, kv_off)
    want = _oracle_grads(q, k, v, do, slopes, scale, kv_off)
    errs = tuple(_norm_err(g, w) for g, w in zip(got, want))
    return got, errs


def _check(case, errs, got):
    print(f"{case}: dq {errs[0]:.3e} dk {errs[1]:.3e} dv {errs[2]:.3e}")
    for g in got:
        assert torch.isfinite(g.float()).all(), case
    for name, e, pe in zip(("dq", "dk", "dv"), errs, _PARENT_ERR[case]):
        assert e < HARD, f"{case} {name}: {e}"
        assert e <= 2 * pe, f"{case} {name}: {e} vs previous kernels {pe}"


@pytest.mark.parametrize("case", sorted(CASES))
def test_attn_bwd_softmax_vs_oracle(case):
    got, errs = _run(case)
    _check(case, errs, got)


def test_attn_bwd_softmax_fused_qkv():
    """The kernels read q/k/v at the interleaved strides of the fused QKV
    buffer and write into the slices of one d(fused)."""
    from pipegoose_amd.ops.attention import alibi_attention_qkv
    case = "fused_qkv_s256"
    B, S, H, D = 1, 256, 2, 64
    torch.manual_seed(40)
    fused = torch.randn(B, S, H, 3, D, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
    slopes = _slopes("bloom", H)
    scale = D ** -0.5
    o = alibi_attention_qkv(fused, slopes, scale)
    do = torch.randn_like(o)
    o.backward(do)
    q, k, v = (fused.detach()[:, :, :, i, :].permute(0, 2, 1, 3)
               for i in range(3))
    want = _oracle_grads(q, k, v, do, slopes, scale, 0)
    got = tuple(fused.grad[:, :, :, i, :].permute(0, 2, 1, 3)
                for i in range(3))
    errs = tuple(_norm_err(g, w) for g, w in zip(got, want))
    _check(case, errs, got)


def test_attn_bwd_softmax_deterministic():
    """No atomics, fixed accumulation order: the same backward twice is
    bitwise equal."""
    ext = _ext()
    case = "d64_w8_offdiag"
    first, _ = _run(case)
    q, k, v, do, slopes, scale, kv_off = _inputs(case)
    o, lse = ext.attn_fwd(q, k, v, slopes, scale, kv_off)
    again = ext.attn_bwd(do, q, k, v, o, lse, slopes, scale, kv_off)
    for a, b, name in zip(first, again, ("dq", "dk", "dv")):
        assert torch.equal(a, b), name
