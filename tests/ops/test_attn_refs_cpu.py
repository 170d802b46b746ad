"""The fp64 attention references and input generators of tests/ops/_attn_refs.py
are sound, and the tolerance rule of test_attn_edges_gpu.py has teeth: a CPU
emulation of a correct bf16 flash kernel passes it at F = 4, and five
deliberately wrong variants of that emulation each fail it.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as TF

from tests.ops import _attn_refs as A
from tests.ops import _rowwise_refs as R

TIGHT = dict(rtol=1e-10, atol=1e-11)
BF16, FP32 = torch.bfloat16, torch.float32


def _case(family="randn", slope_set="mild", Hkv=2, S=128, D=64, kv_off=0,
          seed=0):
    return A.attn_case(family, slope_set, 2, Hkv, S, D, kv_off=kv_off,
                       seed=seed)


def _leaf(t):
    return t.double().detach().requires_grad_(True)


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("kv_off", [0, -64, -128, -256])
def test_attn_ref_matches_sdpa_fp64(kv_off, Hkv):
    c = _case(Hkv=Hkv, kv_off=kv_off, seed=1)
    o, lse = A.attn_ref(c["q"], c["k"], c["v"], c["slopes"], c["scale"], kv_off)
    q, k, v = (c[n].double() for n in "qkv")
    bias = A.mask_bias(128, 128, c["slopes"], kv_off, "cpu", torch.float64)
    want = TF.scaled_dot_product_attention(
        q, k.repeat_interleave(2 // Hkv, 1), v.repeat_interleave(2 // Hkv, 1),
        attn_mask=bias, scale=c["scale"])
    assert torch.allclose(o, want, **TIGHT)
    s = c["scale"] * q @ k.repeat_interleave(2 // Hkv, 1).transpose(-1, -2)
    assert torch.allclose(lse, torch.logsumexp(s + bias[0], -1), **TIGHT)


@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("kv_off", [0, -65, -128])
def test_attn_bwd_ref_matches_autograd_fp64(kv_off, Hkv):
    c = _case(Hkv=Hkv, kv_off=kv_off, seed=2)
    q, k, v = _leaf(c["q"]), _leaf(c["k"]), _leaf(c["v"])
    o, lse = A.attn_ref(q, k, v, c["slopes"], c["scale"], kv_off)
    o.backward(c["do"].double())
    got = A.attn_bwd_ref(c["do"], c["q"], c["k"], c["v"], o.detach(),
                         lse.detach(), c["slopes"], c["scale"], kv_off)
    for g, want in zip(got, (q.grad, k.grad, v.grad)):
        assert g.shape == want.shape
        assert torch.allclose(g, want, **TIGHT)


def _ref_fwd(c):
    return lambda q, k, v, off: A.attn_ref(q, k, v, c["slopes"], c["scale"], off)


def _ref_bwd(c):
    return lambda do, q, k, v, o, lse, off: A.attn_bwd_ref(
        do, q, k, v, o, lse, c["slopes"], c["scale"], off)


@pytest.mark.parametrize("family,slope_set,Hkv", [
    ("randn", "mild", 2), ("randn", "steep", 1), ("rising", "zero", 2)])
def test_ring_identity_cp2_fp64(family, slope_set, Hkv):
    """Block forwards (q0,kv0,0), (q1,kv1,0), (q1,kv0,-S), merged; block
    backwards with the merged o and lse, summed: the whole 2S sequence."""
    c = _case(family, slope_set, Hkv=Hkv, S=128, seed=3)
    got = A.ring_cp2(_ref_fwd(c), _ref_bwd(c), c, torch.float64, torch.float64)
    q, k, v = _leaf(c["q"]), _leaf(c["k"]), _leaf(c["v"])
    o, lse = A.attn_ref(q, k, v, c["slopes"], c["scale"], 0)
    o.backward(c["do"].double())
    want = {"o": o.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad,
            "dv": v.grad}
    for name in want:
        assert torch.allclose(got[name], want[name], **TIGHT), name


def test_merge_blocks_is_attention_over_the_union():
    c = _case(S=128, seed=4)
    q1 = c["q"][:, :, 64:]
    parts = [A.attn_ref(q1, c["k"][:, :, :64], c["v"][:, :, :64], c["slopes"],
                        c["scale"], -64),
             A.attn_ref(q1, c["k"][:, :, 64:], c["v"][:, :, 64:], c["slopes"],
                        c["scale"], 0)]
    o, lse = A.merge_blocks(parts)
    wo, wl = A.attn_ref(c["q"], c["k"], c["v"], c["slopes"], c["scale"], 0)
    assert torch.allclose(o, wo[:, :, 64:], **TIGHT)
    assert torch.allclose(lse, wl[:, :, 64:], **TIGHT)


# ------------------------------------------------------------------ generators
@pytest.mark.parametrize("S", [192, 384, 512])
def test_mask_offsets_leave_every_row_a_key(S):
    offs = A.mask_offsets(S)
    assert len(set(offs)) == len(offs) and all(o < 0 for o in offs)
    assert set(range(-S + 64, 0, 64)) <= set(offs)
    assert {-1, -63, -65, -S, -S - 64, -2 * S} <= set(offs)
    for off in offs + [0]:
        assert A.visible(S, S, off).any(-1).all(), off
    # and a positive offset does not: what the host check rejects
    assert not A.visible(S, S, 64).any(-1).all()


@pytest.mark.parametrize("slope_set", sorted(A.SLOPE_SETS))
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("D,Hkv,kv_off", [(64, 2, 0), (128, 1, -65)])
def test_generators_give_a_finite_reference(family, slope_set, D, Hkv, kv_off):
    c = A.attn_case(family, slope_set, 2, Hkv, 256, D, kv_off=kv_off)
    for n in ("q", "do"):
        assert c[n].shape == (1, 2, 256, D) and c[n].dtype == BF16
    for n in ("k", "v"):
        assert c[n].shape == (1, Hkv, 256, D) and c[n].dtype == BF16
    assert c["slopes"].dtype == FP32
    again = A.attn_case(family, slope_set, 2, Hkv, 256, D, kv_off=kv_off)
    assert all(torch.equal(c[n], again[n]) for n in ("q", "k", "v", "do"))
    o, lse = A.attn_ref(c["q"], c["k"], c["v"], c["slopes"], c["scale"], kv_off)
    grads = A.attn_bwd_ref(c["do"], c["q"], c["k"], c["v"], o, lse,
                           c["slopes"], c["scale"], kv_off)
    for t in (o, lse) + grads:
        assert torch.isfinite(t).all()
    if family == "do_zero":
        assert all((g == 0).all() for g in grads)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kv_off", [0, -65, -256])
@pytest.mark.parametrize("family", A.PEAKED)
def test_peaked_rows_are_near_one_hot_in_the_intended_tile(family, kv_off, D):
    S = 256
    c = A.attn_case(family, "zero", 2, 2, S, D, kv_off=kv_off)
    s = A.scores(c["q"], c["k"], c["slopes"], c["scale"], kv_off)
    _, lse = A.attn_ref(c["q"], c["k"], c["v"], c["slopes"], c["scale"], kv_off)
    pmax, arg = torch.exp(s - lse[..., None]).max(-1)
    t = A.peak_targets(family, S, kv_off)
    assert A.visible(S, S, kv_off)[torch.arange(S), t].all()
    assert (arg == t).float().mean() > 0.95
    assert (pmax > 0.9).float().mean() > 0.9
    jmax = A.last_visible(S, kv_off)
    if family == "peaked_first":
        assert (t < A.TILE).all()
    elif family == "peaked_last":
        assert (t // A.TILE == jmax // A.TILE).all()
    elif kv_off > -S:
        assert (t == jmax)[: S + kv_off].all()     # on the mask edge
    # the scores besides the planted one have the advertised spread
    rest = s[0, 0, S - 1, :S]
    rest = rest[torch.isfinite(rest)]
    assert 6.0 < rest.std().item() < 16.0


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [192, 512])
def test_rising_moves_the_row_max_at_every_tile(S, D):
    c = A.attn_case("rising", "zero", 2, 2, S, D)
    s = A.scores(c["q"], c["k"], c["slopes"], c["scale"], 0)
    tiles = s.reshape(1, 2, S, S // A.TILE, A.TILE).amax(-1)   # [1,2,S,T]
    # tiles that a row sees whole: t with 64 t + 63 <= i
    i = torch.arange(S)[:, None]
    whole = (torch.arange(S // A.TILE)[None, :] * A.TILE + A.TILE - 1) <= i
    pair = whole[:, 1:]                   # tile t+1 whole implies tile t whole
    assert pair.any()
    assert (tiles[..., 1:] > tiles[..., :-1])[..., pair].all()
    # falling is the mirror image: the first tile holds the maximum and the
    # last tile's weights are below the smallest normal fp32
    c = A.attn_case("falling", "zero", 2, 2, S, D)
    s = A.scores(c["q"], c["k"], c["slopes"], c["scale"], 0)
    tiles = s.reshape(1, 2, S, S // A.TILE, A.TILE).amax(-1)
    assert (tiles[..., 1:] < tiles[..., :-1])[..., pair].all()
    if S == 512:
        assert (tiles[..., S - 1, -1] - tiles[..., S - 1, 0]).max() \
            < math.log(2.0 ** -24)


def test_zero_q_analytic_facts():
    """q = 0, slope 0: o is the running mean of v, lse the log of the number
    of visible keys."""
    for kv_off in (0, -65, -128):
        c = _case("zero_q", "zero", kv_off=kv_off)
        o, lse = A.attn_ref(c["q"], c["k"], c["v"], c["slopes"], c["scale"],
                            kv_off)
        wo, wl = A.zero_q_facts(c["v"], 2, kv_off)
        assert torch.allclose(o, wo, **TIGHT) and torch.allclose(lse, wl, **TIGHT)


# ------------------------------------------------------- sensitivity (mutants)
# A correct bf16 flash kernel in the small: bf16 inputs, fp32 scores and
# statistics, 64-key tiles with the online-softmax rescale, P rounded to bf16
# before P.V, outputs rounded to bf16 (lse fp32); the backward recomputes P
# from (q, k, lse) and rounds P and dS to bf16 before their products.
MUTANTS = ["strict_mask", "bias_plus_one", "skip_last_tile", "local_lse",
           "bias_without_kv_off"]


def _emul_scores(q, k, slopes, scale, kv_off, mutant):
    """fp32 scores [B,H,S,S] and the visibility mask [S,S] that a (mutant)
    kernel would use."""
    H, S = q.size(1), q.size(2)
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    pos = j + kv_off
    vis = pos < i if mutant == "strict_mask" else pos <= i
    if mutant == "skip_last_tile":
        last = A.last_visible(S, kv_off)[:, None] // A.TILE
        vis = vis & ~((j // A.TILE == last) & (last >= 1))
    rel = pos - i
    if mutant == "bias_plus_one":
        rel = rel + 1
    elif mutant == "bias_without_kv_off":
        rel = j - i
    s = (q.float() @ A._expand_kv(k.float(), H).transpose(-1, -2)) * scale \
        + slopes.float()[:, None, None] * rel.float()
    return s, vis


def emul_fwd(q, k, v, slopes, scale, kv_off, mutant=None):
    B, H, S, D = q.shape
    s, vis = _emul_scores(q, k, slopes, scale, kv_off, mutant)
    vf = A._expand_kv(v.float(), H)
    m = torch.full((B, H, S, 1), -1e30)
    l = torch.zeros(B, H, S, 1)
    acc = torch.zeros(B, H, S, D)
    for t0 in range(0, S, A.TILE):
        vt = vis[:, t0:t0 + A.TILE]
        if not vt.any():
            continue
        st = torch.where(vt, s[..., t0:t0 + A.TILE], torch.tensor(-1e30))
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        p = torch.where(vt, torch.exp(st - m_new), torch.tensor(0.0))
        alpha = torch.exp(m - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + p.bfloat16().float() @ vf[:, :, t0:t0 + A.TILE]
        m = m_new
    return (acc / l).bfloat16(), (m + torch.log(l)).squeeze(-1)


def emul_bwd(do, q, k, v, o, lse, slopes, scale, kv_off, mutant=None):
    H, Hkv = q.size(1), k.size(1)
    if mutant == "local_lse":
        lse = emul_fwd(q, k, v, slopes, scale, kv_off)[1]
    s, vis = _emul_scores(q, k, slopes, scale, kv_off, mutant)
    kf, vf = A._expand_kv(k.float(), H), A._expand_kv(v.float(), H)
    p = torch.where(vis, torch.exp(s - lse.float()[..., None]),
                    torch.tensor(0.0))
    delta = (do.float() * o.float()).sum(-1, keepdim=True)
    ds = p * (do.float() @ vf.transpose(-1, -2) - delta) * scale
    p16, ds16 = p.bfloat16().float(), ds.bfloat16().float()
    dq = ds16 @ kf
    dk = A._reduce_kv(ds16.transpose(-1, -2) @ q.float(), Hkv)
    dv = A._reduce_kv(p16.transpose(-1, -2) @ do.float(), Hkv)
    return dq.bfloat16(), dk.bfloat16(), dv.bfloat16()


# (family, slope set, Hkv, kv_off) at S=128, D=64; "ring" = the cp=2 emulation
# with S_local = 64
BLOCK_CASES = [("randn", "mild", 2, 0), ("peaked_diag", "mild", 2, 0),
               ("randn", "mild", 1, -64), ("peaked_last", "mild", 2, -65),
               ("v_offset", "zero", 2, 0)]
RING_CASES = [("randn", "zero", 2), ("rising", "zero", 2), ("randn", "mild", 1)]


def _check_block(case, mutant):
    family, slope_set, Hkv, kv_off = case
    c = _case(family, slope_set, Hkv=Hkv, kv_off=kv_off, seed=5)
    args = (c["q"], c["k"], c["v"], c["slopes"], c["scale"], kv_off)
    tag = f"{mutant or 'correct'} {case}"
    o, lse = emul_fwd(*args, mutant=mutant)
    dq, dk, dv = emul_bwd(c["do"], c["q"], c["k"], c["v"], o, lse,
                          c["slopes"], c["scale"], kv_off, mutant=mutant)
    ro, rl = A.attn_ref(*args)
    rq, rk, rv = A.attn_bwd_ref(c["do"], c["q"], c["k"], c["v"], ro, rl,
                                c["slopes"], c["scale"], kv_off)
    bo, bq, bk, bv = A.sdpa_base(c["q"], c["k"], c["v"], c["do"], c["slopes"],
                                 c["scale"], kv_off)
    bl = A.lse_base(c["q"], c["k"], c["slopes"], c["scale"], kv_off)
    R.check_close("emul", f"{tag} o", o, bo, ro, BF16)
    R.check_close("emul", f"{tag} lse", lse, bl, rl, FP32)
    R.check_close("emul", f"{tag} dq", dq, bq, rq, BF16)
    R.check_close("emul", f"{tag} dk", dk, bk, rk, BF16)
    R.check_close("emul", f"{tag} dv", dv, bv, rv, BF16)


def _check_ring(case, mutant):
    family, slope_set, Hkv = case
    c = _case(family, slope_set, Hkv=Hkv, S=128, seed=6)
    sl, sc = c["slopes"], c["scale"]
    got = A.ring_cp2(
        lambda q, k, v, off: emul_fwd(q, k, v, sl, sc, off, mutant=mutant),
        lambda do, q, k, v, o, lse, off: emul_bwd(do, q, k, v, o, lse, sl, sc,
                                                  off, mutant=mutant),
        c, torch.float32, BF16)
    ro, rl = A.attn_ref(c["q"], c["k"], c["v"], sl, sc, 0)
    ref = dict(zip(("dq", "dk", "dv"), A.attn_bwd_ref(
        c["do"], c["q"], c["k"], c["v"], ro, rl, sl, sc, 0)), o=ro, lse=rl)
    base = dict(zip(("o", "dq", "dk", "dv"), A.sdpa_base(
        c["q"], c["k"], c["v"], c["do"], sl, sc, 0)),
        lse=A.lse_base(c["q"], c["k"], sl, sc, 0))
    for name in ("o", "lse", "dq", "dk", "dv"):
        R.check_close("emul ring", f"{mutant or 'correct'} {case} {name}",
                      got[name], base[name], ref[name],
                      FP32 if name == "lse" else BF16)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=str)
def test_correct_emulation_passes_block(case):
    _check_block(case, None)


@pytest.mark.parametrize("case", RING_CASES, ids=str)
def test_correct_emulation_passes_ring(case):
    _check_ring(case, None)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_is_rejected(mutant):
    """Each wrong variant fails check_close on at least one listed case."""
    failed = []
    for check, cases in ((_check_block, BLOCK_CASES), (_check_ring, RING_CASES)):
        for case in cases:
            try:
                check(case, mutant)
            except AssertionError:
                failed.append(case)
    print(f"{mutant}: rejected on {failed}")
    assert failed, f"{mutant} passed every case"


def test_bias_plus_one_shows_in_lse_only():
    """A bias off by a constant per row cancels in o and every gradient: the
    reason lse is compared at all."""
    c = _case("randn", "mild", seed=5)
    args = (c["q"], c["k"], c["v"], c["slopes"], c["scale"], 0)
    o, lse = emul_fwd(*args)
    o2, lse2 = emul_fwd(*args, mutant="bias_plus_one")
    assert (o.float() - o2.float()).abs().max() <= 2.0 ** -6
    assert torch.allclose(lse2 - lse, c["slopes"][None, :, None].expand_as(lse),
                          atol=1e-4)
