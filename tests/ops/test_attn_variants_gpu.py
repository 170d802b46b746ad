"""The attention selection table (ext.attn_variant) and every kernel
instantiation it can reach, forward and backward, against the fp32 oracle of
test_kernels_gpu; plus the host-side argument check of the backward.

Per family the smaller S is the smallest it accepts and the larger one gives
at least two workgroups along S and crosses a causal tile boundary.
Tolerances are the project's own: forward < 3e-2 absolute
(test_attn_fwd_kernel), backward err / max(1, |ref|max) < 4e-2
(test_attn_bwd_kernel).
"""
import pytest
import torch

from tests.ops.test_kernels_gpu import _attn_oracle

pytestmark = pytest.mark.gpu

# family -> (S of one workgroup, S of several)
FAMILY_S = {("v1", 4): (64, 192), ("v2", 4): (128, 384), ("v2", 8): (256, 512)}

# case id -> (family, H, Hkv, S, D, fully visible)
CASES = {}
for (_fam, _w), _ss in FAMILY_S.items():
    for _D in (64, 128):
        for _S in _ss:
            CASES[f"{_fam}w{_w}_d{_D}_s{_S}"] = ((_fam, _w), 2, 2, _S, _D, False)
    CASES[f"{_fam}w{_w}_gqa"] = ((_fam, _w), 2, 1, _ss[1], 64, False)
    CASES[f"{_fam}w{_w}_visible"] = ((_fam, _w), 2, 2, _ss[1], 64, True)


def _ext():
    from pipegoose_amd.ops import get_extension
    return get_extension(required=True)


def _oracle(q, k, v, slopes, scale, kv_off):
    """fp32 reference on fp32 leaves with H kv heads.  kv_off == 0 is the
    causal _attn_oracle; kv_off == -S shifts every kv position S to the left
    of the q block, so all of them are visible and only the bias remains."""
    if kv_off == 0:
        return _attn_oracle(q, k, v, slopes, scale)
    S = q.size(-2)
    assert kv_off == -S
    pos = torch.arange(S, device=q.device)
    rel = (pos[None, :] + kv_off - pos[:, None]).float()
    bias = slopes.float()[:, None, None] * rel[None]
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=bias[None], scale=scale)


def test_attn_variant_table():
    ext = _ext()
    for D in (64, 128):
        for S in range(64, 1024 + 1, 64):
            got = ext.attn_variant(S, D)
            assert (got == ("v1", 4)) == (S % 128 == 64), (S, D, got)
            assert (got == ("v2", 4)) == (S % 256 == 128), (S, D, got)
            assert (got == ("v2", 8)) == (S % 256 == 0), (S, D, got)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ext.attn_variant(96, 64)
    with pytest.raises(RuntimeError, match="head dim"):
        ext.attn_variant(128, 96)


@pytest.mark.parametrize("case", sorted(CASES))
def test_attn_variant_fwd_bwd(case):
    ext = _ext()
    family, H, Hkv, S, D, visible = CASES[case]
    assert ext.attn_variant(S, D) == family
    B, kv_off = 1, (-S if visible else 0)
    torch.manual_seed(21)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    do = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    slopes = torch.rand(H, device="cuda") * 0.5
    scale = 1.0 / D ** 0.5

    o, lse = ext.attn_fwd(q, k, v, slopes, scale, kv_off)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse, slopes, scale, kv_off)

    q2 = q.float().requires_grad_(True)
    k2 = k.float().requires_grad_(True)
    v2 = v.float().requires_grad_(True)
    ref = _oracle(q2, k2.repeat_interleave(H // Hkv, dim=1),
                  v2.repeat_interleave(H // Hkv, dim=1), slopes, scale, kv_off)
    ref.backward(do.float())

    err = (o.float() - ref).abs().max().item()
    print(f"{case}: o err {err:.3e}")
    assert err < 3e-2, err
    assert torch.isfinite(lse).all()
    for got, want, name in ((dq, q2.grad, "dq"), (dk, k2.grad, "dk"),
                            (dv, v2.grad, "dv")):
        assert got.shape == want.shape
        e = (got.float() - want).abs().max().item()
        ref_max = max(want.abs().max().item(), 1.0)
        print(f"{case}: {name} err {e:.3e} / {ref_max:.3e}")
        assert e / ref_max < 4e-2, f"{name}: {e} vs {ref_max}"


@pytest.mark.parametrize("S,D,msg", [(96, 64, "multiple of 64"),
                                     (128, 96, "head dim")])
def test_attn_bwd_rejects_unsupported_shape(S, D, msg):
    """attn_bwd used to check strides only: S=96 ran a grid of S/64 blocks
    whose loops step past the end.  The message shows that the host check
    raised, which happens before anything is launched."""
    ext = _ext()
    B, H = 1, 2
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k, v, do = torch.randn_like(q), torch.randn_like(q), torch.randn_like(q)
    o = torch.zeros_like(q)
    lse = torch.zeros(B, H, S, device="cuda", dtype=torch.float32)
    slopes = torch.rand(H, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        ext.attn_bwd(do, q, k, v, o, lse, slopes, 0.125, 0)
    torch.cuda.synchronize()
