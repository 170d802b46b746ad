"""Attention forward/backward HIP kernels at mask edges and hostile values,
against fp64.

Every kernel family of csrc/attention.hip (v1, v2 with 4 waves, v2 with 8
waves) at D = 64 and 128, with and without GQA, on inputs that break a naive
flash kernel (near one-hot rows planted in the first, the diagonal and the
last visible tile, a row maximum that moves at every tile, late tiles that
underflow, q = 0, v and do with a large common offset, slope 0 and a slope
steep enough to underflow everything but the nearest keys), at every position
of a shifted causal mask (kv_off inside (-S, 0), multiples of the tile and
not), through the ring-attention flow on one GPU (block backwards fed the
merged o and lse), and through the strided views of the fused-QKV path.

Every value check is  max|got - ref| <= F * max|base - ref| + 2 ulp_out(max|ref|)
(tests/ops/_rowwise_refs.py: ref is the fp64 reference of tests/ops/_attn_refs.py,
base is bf16 scaled_dot_product_attention with the explicit additive mask plus
autograd on the GPU, for lse torch.logsumexp of the fp32 scores), over whole
tensors.  The measured ratio (smallest F that would pass) is printed per check.

Largest measured ratio per output on an MI355X, F = 4 everywhere (no check
needed a raised F).  A ratio of 0 means every error lay inside the 2 ulp term:
    o          0
    lse        0.40  peaked_last, slopes [2^-8, 0.5], S=512 D=64 kv_off=-192
    dq         1.95  peaked_diag, slopes [4, 0.0625], S=512 D=128
    dk         1.95  the same case
    dv         0
    ring o     0
    ring lse   0
    ring dq    0.80  rising, slopes [2^-8, 0.5], Hkv=1, 2 x 256 D=64
    ring dk    0.15  randn, slopes [0, 0], 2 x 128 D=128
    ring dv    0.25  rising, slopes [0, 0], 2 x 128 D=128
In the peaked and v_offset cases the kernel's and the baseline's gradient
errors are nearly equal and far above the 2 ulp term (v_offset dq: 17.9 both):
both backwards form delta = rowsum(do * o) from the bf16 o, and that rounding
is the error.  The hardware exp2/log2 of the v2 kernels costs lse nothing
that shows next to an fp32 logsumexp.

What the kernels gave before this file's fixes:
    v1 dk/dv (attn_bwd_dkdv_kernel, S % 128 == 64) with a kv_off that is no
        multiple of 32: the q chunks started at kv block start + kv_off
        unrounded, so the last chunk of 32 rows ran up to 31 rows past S,
        reading q, do, lse and delta out of bounds and adding those rows to
        dk and dv.  Found by reading the kernel while choosing these cases
        and fixed (chunk start rounded down) before anything ran; the
        unfixed kernel was not run on such an offset.  The v1 cases of
        test_attn_mask_positions at kv_off -1, -63 and -65 cover it now.
    Everything else passed as it was: no other kernel body changed.
    attn_fwd / attn_bwd accepted kv_off > 0 and returned o = 0 * inf for the
        rows without a visible key; the host check rejects it now.
"""
import pytest
import torch

from tests.ops import _attn_refs as A
from tests.ops import _rowwise_refs as R

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
H = 2
# variant -> (what attn_variant reports, S of one workgroup, S of several)
VARIANTS = {"v1": (("v1", 4), 64, 192), "v2w4": (("v2", 4), 128, 384),
            "v2w8": (("v2", 8), 256, 512)}
DS = [64, 128]
OUT_DTYPE = {"o": BF16, "lse": FP32, "dq": BF16, "dk": BF16, "dv": BF16}


def _ext():
    from pipegoose_amd.ops import get_extension
    return get_extension(required=True)


@pytest.fixture(scope="module", autouse=True)
def _report_largest_ratios():
    yield
    for kernel, (ratio, what) in sorted(R.RATIOS.items()):
        print(f"[largest] {kernel}: {ratio:.3g} at {what}")


_CASES = {}


def _case(family, slope_set, Hkv, S, D, kv_off=0):
    """The case's inputs on the GPU with its fp64 reference and its stock
    torch baseline, never written to.  The cases that several tests use
    (randn, mild slopes, kv_off 0) are computed once and kept."""
    key = (family, slope_set, Hkv, S, D, kv_off)
    shared = (family, slope_set, kv_off) == ("randn", "mild", 0)
    if key not in _CASES:
        c = {n: t.cuda() if torch.is_tensor(t) else t for n, t in
             A.attn_case(family, slope_set, H, Hkv, S, D, kv_off=kv_off).items()}
        args = (c["q"], c["k"], c["v"], c["slopes"], c["scale"], kv_off)
        ro, rl = A.attn_ref(*args)
        ref = dict(zip(("dq", "dk", "dv"), A.attn_bwd_ref(
            c["do"], c["q"], c["k"], c["v"], ro, rl, c["slopes"], c["scale"],
            kv_off)), o=ro, lse=rl)
        base = dict(zip(("o", "dq", "dk", "dv"), A.sdpa_base(
            c["q"], c["k"], c["v"], c["do"], c["slopes"], c["scale"], kv_off)),
            lse=A.lse_base(c["q"], c["k"], c["slopes"], c["scale"], kv_off))
        c.update(ref=ref, base=base, kv_off=kv_off,
                 tag=f"{family} {slope_set} Hkv={Hkv} S={S} D={D} off={kv_off}")
        if not shared:
            return c
        _CASES[key] = c
    return _CASES[key]


def _run(c):
    """The kernels on case c: dict of o, lse, dq, dk, dv."""
    ext = _ext()
    o, lse = ext.attn_fwd(c["q"], c["k"], c["v"], c["slopes"], c["scale"],
                          c["kv_off"])
    dq, dk, dv = ext.attn_bwd(c["do"], c["q"], c["k"], c["v"], o, lse,
                              c["slopes"], c["scale"], c["kv_off"])
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _check_all(kernel, c, got):
    for name, dtype in OUT_DTYPE.items():
        R.check_close(f"{kernel} {name}", c["tag"], got[name], c["base"][name],
                      c["ref"][name], dtype)


def _variant_S(variant, D, larger=True):
    want, s_small, s_large = VARIANTS[variant]
    S = s_large if larger else s_small
    assert _ext().attn_variant(S, D) == want
    return S


# --------------------------------------------------------------------- values
@pytest.mark.parametrize("slope_set", sorted(A.SLOPE_SETS))
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_attn_values(variant, D, family, slope_set):
    S = _variant_S(variant, D)
    c = _case(family, slope_set, H, S, D)
    got = _run(c)
    _check_all("attn", c, got)
    if family == "do_zero":
        for name in ("dq", "dk", "dv"):
            assert (got[name] == 0).all(), name
    if family == "zero_q" and slope_set == "zero":
        # o the running mean of v, lse = log(i + 1)
        fo, fl = A.zero_q_facts(c["v"], H, 0)
        R.check_close("attn o", f"{c['tag']} mean of v", got["o"],
                      c["base"]["o"], fo, BF16)
        R.check_close("attn lse", f"{c['tag']} log(i+1)", got["lse"],
                      c["base"]["lse"], fl, FP32)


@pytest.mark.parametrize("family,slope_set", [
    ("randn", "mild"), ("peaked_diag", "mild"), ("v_offset", "zero"),
    ("rising", "steep")])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_attn_values_gqa(variant, D, family, slope_set):
    c = _case(family, slope_set, 1, _variant_S(variant, D), D)
    _check_all("attn", c, _run(c))


@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_attn_values_one_workgroup(variant, D, Hkv):
    c = _case("randn", "mild", Hkv, _variant_S(variant, D, larger=False), D)
    _check_all("attn", c, _run(c))


# ------------------------------------------------------------- mask positions
def _mask_params():
    out = []
    for variant in sorted(VARIANTS):
        for kv_off in A.mask_offsets(VARIANTS[variant][2]):
            for D in DS:
                for family, Hkv in (("randn", 2), ("randn", 1),
                                    ("peaked_diag", 2), ("peaked_last", 2),
                                    ("peaked_first", 2)):
                    out.append(pytest.param(
                        variant, D, family, Hkv, kv_off,
                        id=f"{variant}-d{D}-{family}-kv{Hkv}-off{kv_off}"))
    return out


@pytest.mark.parametrize("variant,D,family,Hkv,kv_off", _mask_params())
def test_attn_mask_positions(variant, D, family, Hkv, kv_off):
    """Shifted causal masks: kv_off inside (-S, 0) at and off the tile
    boundaries, and the fully visible offsets."""
    c = _case(family, "mild", Hkv, _variant_S(variant, D), D, kv_off=kv_off)
    _check_all("attn", c, _run(c))


# -------------------------------------------------------------- ring emulation
@pytest.mark.parametrize("family,slope_set,Hkv", [
    ("randn", "zero", 2), ("randn", "mild", 1), ("rising", "zero", 2),
    ("rising", "mild", 1)])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_attn_ring_cp2(variant, D, family, slope_set, Hkv):
    """Context parallelism over two ranks on one GPU: three block forwards,
    the fp32 merge of _RingAttentionRotate, three block backwards fed the
    MERGED o and lse (P = exp(s - lse_global) sums to less than 1 per block),
    partial grads summed in fp32; against the whole 2 S sequence."""
    ext = _ext()
    S_local = _variant_S(variant, D, larger=False)
    c = _case(family, slope_set, Hkv, 2 * S_local, D)
    sl, sc = c["slopes"], c["scale"]
    got = A.ring_cp2(
        lambda q, k, v, off: ext.attn_fwd(
            q.contiguous(), k.contiguous(), v.contiguous(), sl, sc, off),
        lambda do, q, k, v, o, lse, off: ext.attn_bwd(
            do.contiguous(), q.contiguous(), k.contiguous(), v.contiguous(),
            o, lse.contiguous(), sl, sc, off),
        c, FP32, BF16)
    _check_all("ring", c, got)


# --------------------------------------------------------------------- layout
@pytest.mark.parametrize("S,D", [(128, 64), (192, 128)])
def test_attn_strided_views_and_bwd_into(S, D):
    """q, k, v as views of one fused [B, S, H, 3, D] buffer, do as a permuted
    view, grads written by attn_bwd_into into three slots of a [B, S, H, 4, D]
    buffer: bit-identical to the contiguous call, the fourth slot untouched,
    and a repeated call bit-identical (fixed summation order, no atomics)."""
    ext = _ext()
    B, SENTINEL = 2, 12288.0
    g = torch.Generator(device="cpu").manual_seed(17)
    fused = torch.randn(B, S, H, 3, D, generator=g).bfloat16().cuda()
    do = torch.randn(B, S, H, D, generator=g).bfloat16().cuda().permute(0, 2, 1, 3)
    slopes = torch.tensor(A.SLOPE_SETS["mild"], device="cuda")
    scale = D ** -0.5
    q, k, v = (fused[:, :, :, n, :].permute(0, 2, 1, 3) for n in range(3))
    assert not q.is_contiguous() and not do.is_contiguous()

    o, lse = ext.attn_fwd(q, k, v, slopes, scale, 0)
    out = torch.full((B, S, H, 4, D), SENTINEL, device="cuda", dtype=BF16)
    slots = [out[:, :, :, n, :].permute(0, 2, 1, 3) for n in range(3)]
    ext.attn_bwd_into(do, q, k, v, o, lse, slopes, scale, *slots, 0)

    qc, kc, vc, doc = (t.contiguous() for t in (q, k, v, do))
    oc, lsec = ext.attn_fwd(qc, kc, vc, slopes, scale, 0)
    grads_c = ext.attn_bwd(doc, qc, kc, vc, oc, lsec, slopes, scale, 0)
    assert torch.equal(o, oc) and torch.equal(lse, lsec)
    for slot, want, name in zip(slots, grads_c, ("dq", "dk", "dv")):
        assert torch.equal(slot, want), name
    assert (out[:, :, :, 3, :] == SENTINEL).all()

    o2, lse2 = ext.attn_fwd(q, k, v, slopes, scale, 0)
    out2 = torch.full_like(out, SENTINEL)
    slots2 = [out2[:, :, :, n, :].permute(0, 2, 1, 3) for n in range(3)]
    ext.attn_bwd_into(do, q, k, v, o2, lse2, slopes, scale, *slots2, 0)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(out, out2)


# ---------------------------------------------------------------- exact facts
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_attn_row_zero_sees_one_key(variant, D, Hkv):
    """kv_off = 0: row 0 sees key 0 alone, so o is v[0] (to one bf16 ulp) and
    lse the one score scale * q0.k0 (its bias is 0)."""
    c = _case("randn", "mild", Hkv, _variant_S(variant, D), D)
    ext = _ext()
    o, lse = ext.attn_fwd(c["q"], c["k"], c["v"], c["slopes"], c["scale"], 0)
    v0 = A._expand_kv(c["v"], H)[:, :, 0, :].double()
    k0 = A._expand_kv(c["k"], H)[:, :, 0, :].double()
    ulp = 2.0 ** -8 * torch.exp2(torch.floor(torch.log2(v0.abs())))
    assert ((o[:, :, 0, :].double() - v0).abs() <= ulp).all()
    s00 = c["scale"] * (c["q"][:, :, 0, :].double() * k0).sum(-1)
    R.check_close("attn lse", f"{c['tag']} row 0", lse[:, :, 0],
                  c["base"]["lse"][:, :, 0], s00, FP32)


# ------------------------------------------------------------ rejected offset
@pytest.mark.parametrize("S,D", [(64, 64), (128, 128), (256, 64)])
def test_attn_rejects_positive_kv_off(S, D):
    """A positive kv_off leaves the first rows without a visible key (l = 0).
    The message shows that the host check raised, which happens before
    anything is launched."""
    ext = _ext()
    c = _case("randn", "mild", H, S, D)
    o = torch.zeros_like(c["q"])
    lse = torch.zeros(1, H, S, device="cuda", dtype=FP32)
    with pytest.raises(RuntimeError, match="kv_off must be"):
        ext.attn_fwd(c["q"], c["k"], c["v"], c["slopes"], c["scale"], 64)
    with pytest.raises(RuntimeError, match="kv_off must be"):
        ext.attn_bwd(c["do"], c["q"], c["k"], c["v"], o, lse, c["slopes"],
                     c["scale"], 64)
    with pytest.raises(RuntimeError, match="kv_off must be"):
        ext.attn_fwd(c["q"], c["k"], c["v"], c["slopes"], c["scale"], 1)
    torch.cuda.synchronize()
