"""The v2 attention kernels under their workgroup order (attn_work_order.h):
forward and backward through the extension's entry points on grids with
nx = 2 and 3 blocks along S (S 512 and 768, 8 waves; S 384, 4 waves), group
counts B*H that are and are not multiples of 8 (the XCD-pinned and the plain
heaviest-first branch), GQA (the dkdv grid's y is then the KV head count) and
causal, shifted-causal and fully visible launches.

The oracle and the tolerances are those of test_attn_variants_gpu: fp32 sdpa
with the additive ALiBi bias, forward < 3e-2 absolute, gradients
err / max(1, |ref|max) < 4e-2.

A wrong map either computes a tile twice and another never, or indexes outside
the grid.  A tile that no workgroup computed must not pass on what the memory
held before: the forward runs right after tensors of o's and lse's sizes were
NaN-filled and freed, so the caching allocator hands that storage back, and
the backward writes into NaN-filled gradient buffers (the d(fused) buffer of
the model where q and kv heads match).  Two runs must be bitwise equal.
"""
import functools

import pytest
import torch

from tests.ops.test_attn_variants_gpu import _oracle as _variants_oracle

pytestmark = pytest.mark.gpu

FWD_TOL = 3e-2   # test_attn_variants_gpu / test_attn_fwd_kernel
BWD_TOL = 4e-2   # test_attn_variants_gpu / test_attn_bwd_kernel

SHIFT = -256     # the shifted-causal kv_off; "full" stands for -S

# case id -> (B, H, Hkv, S, D, kv_off)
CASES = {}
for _S in (512, 768, 384):
    for _D in (64, 128):
        for _B, _H in ((2, 4), (1, 3), (3, 5)):
            for _name, _off in (("causal", 0), ("full", -_S), ("shift", SHIFT)):
                CASES[f"s{_S}_d{_D}_b{_B}h{_H}_{_name}"] = (
                    _B, _H, _H, _S, _D, _off)
for _D in (64, 128):
    for _name, _off in (("causal", 0), ("full", -512), ("shift", SHIFT)):
        CASES[f"gqa_s512_d{_D}_{_name}"] = (4, 4, 2, 512, _D, _off)


def _ext():
    from pipegoose_amd.ops import get_extension
    return get_extension(required=True)


def _oracle(q, k, v, slopes, scale, kv_off):
    """test_attn_variants_gpu's oracle; for an offset strictly between -S and
    0 the same fp32 sdpa with the bias at the shifted kv positions and the
    keys with j + kv_off > i masked."""
    S = q.size(-2)
    if kv_off in (0, -S):
        return _variants_oracle(q, k, v, slopes, scale, kv_off)
    pos = torch.arange(S, device=q.device)
    rel = pos[None, :] + kv_off - pos[:, None]
    bias = slopes.float()[:, None, None] * rel[None].float()
    bias = bias.masked_fill(rel[None] > 0, float("-inf"))
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=bias[None], scale=scale)


def _inputs(case):
    B, H, Hkv, S, D, kv_off = CASES[case]
    torch.manual_seed(100 + sorted(CASES).index(case))
    if H == Hkv:
        # the model's layout: q, k, v are strided views of the fused projection
        fused = torch.randn(B, S, H, 3, D, device="cuda", dtype=torch.bfloat16)
        q, k, v = (fused[:, :, :, i, :].permute(0, 2, 1, 3) for i in range(3))
    else:
        q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn_like(k)
    do = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    slopes = torch.rand(H, device="cuda") * 0.5
    return q, k, v, do, slopes, 1.0 / D ** 0.5, kv_off


def _nan_grads(q, k):
    """NaN-filled gradient buffers as [B, H, S, D] views: the slices of one
    d(fused) where the head counts match, three [B, S, H, D] buffers under
    GQA."""
    B, H, S, D = q.shape
    nan = float("nan")
    if k.size(1) == H:
        dfused = torch.full((B, S, H, 3, D), nan, device="cuda",
                            dtype=torch.bfloat16)
        return tuple(dfused[:, :, :, i, :].permute(0, 2, 1, 3)
                     for i in range(3))
    return tuple(torch.full((B, S, heads, D), nan, device="cuda",
                            dtype=torch.bfloat16).permute(0, 2, 1, 3)
                 for heads in (H, k.size(1), k.size(1)))


def _kernels(case):
    ext = _ext()
    q, k, v, do, slopes, scale, kv_off = _inputs(case)
    B, H, S, D = q.shape
    # poison the storage that attn_fwd's two allocations are about to reuse
    poison_o = torch.full((B, S, H, D), float("nan"), device="cuda",
                          dtype=torch.bfloat16)
    poison_lse = torch.full((B, H, S), float("nan"), device="cuda",
                            dtype=torch.float32)
    del poison_o, poison_lse
    o, lse = ext.attn_fwd(q, k, v, slopes, scale, kv_off)
    dq, dk, dv = _nan_grads(q, k)
    ext.attn_bwd_into(do, q, k, v, o, lse, slopes, scale, dq, dk, dv, kv_off)
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _run(case):
    """One run of the kernels per case, shared by the tests below."""
    return _kernels(case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_work_order_fwd_bwd_vs_oracle(case):
    ext = _ext()
    B, H, Hkv, S, D, kv_off = CASES[case]
    assert ext.attn_variant(S, D) == ("v2", 8 if S % 256 == 0 else 4)
    o, lse, dq, dk, dv = _run(case)
    q, k, v, do, slopes, scale, _ = _inputs(case)

    q2 = q.float().requires_grad_(True)
    k2 = k.float().requires_grad_(True)
    v2 = v.float().requires_grad_(True)
    ref = _oracle(q2, k2.repeat_interleave(H // Hkv, dim=1),
                  v2.repeat_interleave(H // Hkv, dim=1), slopes, scale, kv_off)
    ref.backward(do.float())

    err = (o.float() - ref).abs().max().item()
    print(f"{case}: o err {err:.3e}")
    assert err < FWD_TOL, err
    assert torch.isfinite(lse).all()
    for got, want, name in ((dq, q2.grad, "dq"), (dk, k2.grad, "dk"),
                            (dv, v2.grad, "dv")):
        assert got.shape == want.shape
        e = (got.float() - want).abs().max().item()
        ref_max = max(want.abs().max().item(), 1.0)
        print(f"{case}: {name} err {e:.3e} / {ref_max:.3e}")
        assert e / ref_max < BWD_TOL, f"{name}: {e} vs {ref_max}"


@pytest.mark.parametrize("case", sorted(CASES))
def test_work_order_repeats_bitwise(case):
    first = _run(case)
    again = _kernels(case)
    for a, b, name in zip(first, again, ("o", "lse", "dq", "dk", "dv")):
        assert torch.equal(a, b), name
