"""fp8 paged cache kernels (csrc/paged_fp8_attention.hip) against fp64.

Decode: pools built with the torch reference quantiser in the shuffled page
layout of tests/ops/test_paged_attn_gpu.py (its shapes, plans, positions and
bound check are imported); the reference is the fp64 paged reference on the
dequantised gather of the same bytes and scales.  fp8 -> fp32 is exact and
the scale multiply is one fp32 rounding, so the bound carries over:
|out - ref| <= 2^-7*|ref| + 2^-7*vmax, vmax the largest dequantised live |v|.
Rows beyond p, pages outside a live prefix and table entries beyond the live
count are poison: K byte 0x7E (+448), V byte 0xFE (-448), scale 1e30.

Write: scale == amax/448 within 2^-22 relative (one fp32 rounding);
|y - x| <= max(|x|*2^-4, scale*2^-10) * (1 + 2^-10) for each dequantised y
(half-ulp of e4m3fn, normal and subnormal; the factor for the fp32 scale
arithmetic); bytes and scales outside the addressed rows keep a sentinel.
"""
import pytest
import torch

from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_decode_attention_reference, paged_gather, paged_gather_dequant,
    quantize_rows_fp8)
from tests.ops.test_paged_attn_gpu import (B, CAP, H, SHAPES, SPLITS, _check,
                                           _chunk, _layout, _pos_tensor,
                                           _positions, _qkv, _slopes)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
POISON_K, POISON_V, POISON_SCALE = 0x7E, 0xFE, 1e30


def _ext():
    return get_extension(required=True)


def _build(k_log, v_log, PAGE, pos_rows):
    """fp8 pools, scales and table holding the quantised logical rows 0..p of
    every sequence, all the rest poison (module docstring)."""
    assign, spare, n_pool = _layout(PAGE)
    Hkv, D = k_log.size(1), k_log.size(3)
    max_pages = CAP // PAGE
    live = torch.arange(max_pages)[None, :] <= \
        (torch.tensor(pos_rows) // PAGE)[:, None]
    table = torch.where(live, assign, torch.tensor(spare[0]))
    out = []
    for logical, poison in ((k_log, POISON_K), (v_log, POISON_V)):
        q8, sc = quantize_rows_fp8(logical)
        q8, sc = q8.view(torch.uint8).clone(), sc.clone()
        for b, pb in enumerate(pos_rows):
            q8[b, :, pb + 1:] = poison
            sc[b, :, pb + 1:] = POISON_SCALE
        pool = torch.full((n_pool, Hkv, PAGE, D), poison, device="cuda",
                          dtype=torch.uint8)
        scale = torch.full((n_pool, Hkv, PAGE), POISON_SCALE, device="cuda")
        pool[assign[live].cuda()] = q8.view(
            B, Hkv, max_pages, PAGE, D).permute(0, 2, 1, 3, 4)[live.cuda()]
        scale[assign[live].cuda()] = sc.view(
            B, Hkv, max_pages, PAGE).permute(0, 2, 1, 3)[live.cuda()]
        out += [pool.view(FP8), scale]
    return out[0], out[2], out[1], out[3], table.to("cuda", torch.int32)


def _vmax(v_pool, v_scale, table, pos_rows):
    vg = paged_gather_dequant(v_pool, v_scale, table, CAP, torch.float64)
    return max(vg[b, :, :p + 1].abs().max().item()
               for b, p in enumerate(pos_rows))


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_decode_random_inputs(D, Hkv, PAGE):
    ext = _ext()
    q, k_log, v_log = _qkv(D, Hkv)
    scale = D ** -0.5
    for n in SPLITS:
        c = _chunk(n, Hkv, D)
        for rows in [[p] * B for p in _positions(c, PAGE)] + \
                [[min(c + 1, CAP - 1), 0]]:
            kp, vp, ks, vs, table = _build(k_log, v_log, PAGE, rows)
            pos, vmax = _pos_tensor(rows), _vmax(vp, vs, table, rows)
            for kind in ("alibi", "zero"):
                slopes = _slopes(kind)
                out = ext.paged_decode_attn_fp8(q, kp, vp, ks, vs, table,
                                                slopes, scale, pos, n)
                assert out.dtype == torch.bfloat16
                assert out.transpose(1, 2).is_contiguous()
                ref = paged_decode_attention_reference(
                    q.double(), kp, vp, table, slopes.double(), scale, pos,
                    ks, vs)
                _check(out, ref, vmax,
                       f"{kind} n_splits={n} chunk={c} pos={rows}")


@pytest.mark.parametrize("D,Hkv,PAGE", SHAPES)
def test_decode_every_index_is_reachable(D, Hkv, PAGE):
    """K is zero except row j*, aligned with the group's first q head
    strongly enough that softmax puts all weight there: out == the
    dequantised v[j*]."""
    ext = _ext()
    q, _, v_log = _qkv(D, Hkv)
    G, scale = H // Hkv, D ** -0.5
    q0 = q[:, ::G, 0].float()                                  # [B, Hkv, D]
    krow = ((30 + 0.25 * CAP) * q0
            / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    for n in SPLITS:
        c = _chunk(n, Hkv, D)
        for p in _positions(c, PAGE):
            for js in sorted({min(j, p)
                              for j in (0, p, PAGE - 1, PAGE, c - 1, c)}):
                k_log = torch.zeros_like(v_log)
                k_log[:, :, js] = krow
                kp, vp, ks, vs, table = _build(k_log, v_log, PAGE, [p] * B)
                vg = paged_gather_dequant(vp, vs, table, CAP, torch.float64)
                vmax = vg[:, :, :p + 1].abs().max().item()
                for kind in ("alibi", "zero"):
                    out = ext.paged_decode_attn_fp8(
                        q, kp, vp, ks, vs, table, _slopes(kind), scale,
                        _pos_tensor([p] * B), n)
                    _check(out[:, ::G, 0], vg[:, :, js], vmax,
                           f"{kind} n_splits={n} chunk={c} pos={p} j*={js}")


# ------------------------------------------------------------------ kv write

BYTE_SENTINEL, SCALE_SENTINEL = 0x5A, 0x3F9D70A5     # an odd fp32 bit pattern


def _sentinel_cache(PAGE, Hkv, D):
    n_pool = _layout(PAGE)[2]
    pool = lambda: torch.full((n_pool, Hkv, PAGE, D), BYTE_SENTINEL,
                              device="cuda", dtype=torch.uint8).view(FP8)
    scale = lambda: torch.full((n_pool, Hkv, PAGE), SCALE_SENTINEL,
                               device="cuda",
                               dtype=torch.int32).view(torch.float32)
    return pool(), pool(), scale(), scale()


def _check_written(pool, scales, table, new, lo, kept, b):
    x = new[b, :, :kept].double()                          # [Hkv, kept, D]
    sc = paged_gather(scales[..., None], table, CAP)[b, :, lo:lo + kept, 0]
    y = paged_gather_dequant(pool, scales, table, CAP,
                             torch.float64)[b, :, lo:lo + kept]
    want = x.abs().amax(-1) / 448
    assert ((sc.double() - want).abs() <= 2.0 ** -22 * want).all()
    bound = torch.maximum(x.abs() * 2.0 ** -4,
                          sc.double()[..., None] * 2.0 ** -10)
    assert ((y - x).abs() <= bound * (1 + 2.0 ** -10)).all()


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (64, 1, 64),
                                        (128, 2, 16), (128, 4, 64)])
def test_kv_write(D, Hkv, PAGE):
    ext = _ext()
    table = _layout(PAGE)[0].to("cuda", torch.int32)
    g = torch.Generator(device="cuda").manual_seed(5000 + D + Hkv + PAGE)
    for s_new, start in [(1, [PAGE - 1]), (1, [PAGE]), (37, [0]), (37, [5]),
                         (37, [5, PAGE]),
                         (5, [CAP - 2])]:    # the last three rows are dropped
        kp, vp, ks, vs = _sentinel_cache(PAGE, Hkv, D)
        # transposed views of a wider buffer: strided in every dim but the last
        mk = lambda: torch.randn(
            B, s_new, Hkv, D + 8, device="cuda",
            generator=g).bfloat16()[..., 8:].transpose(1, 2)
        k_new, v_new = mk(), mk()
        if s_new >= 5:
            k_new[:, :, 3] = 0                 # amax == 0
            v_new[:, :, 4] = 1e-3              # flushed to zero next to 3e4
            v_new[:, :, 4, D // 2] = 3e4
        assert not k_new.is_contiguous() and k_new.stride(3) == 1
        ext.paged_kv_write_fp8(k_new, v_new, kp, vp, ks, vs, table,
                               torch.tensor(start, device="cuda"))
        touched = torch.zeros(kp.size(0), PAGE, dtype=torch.bool)
        for b in range(B):
            lo = start[b % len(start)]
            kept = min(s_new, CAP - lo)
            _check_written(kp, ks, table, k_new, lo, kept, b)
            _check_written(vp, vs, table, v_new, lo, kept, b)
            for j in range(lo, lo + kept):
                touched[table[b, j // PAGE].item(), j % PAGE] = True
        if s_new >= 5 and start != [CAP - 2]:
            zero = paged_gather(ks[..., None], table, CAP)[0, :, start[0] + 3]
            assert (zero == 0).all()
        keep = ~touched.cuda()[:, None, :]                 # [n_pool, 1, PAGE]
        for pool, scales in ((kp, ks), (vp, vs)):
            assert (pool.view(torch.uint8)[keep.expand(-1, Hkv, -1)]
                    == BYTE_SENTINEL).all(), (s_new, start)
            assert (scales.view(torch.int32)[keep.expand(-1, Hkv, -1)]
                    == SCALE_SENTINEL).all(), (s_new, start)


@pytest.mark.parametrize("D,Hkv,PAGE", [(64, 4, 16), (128, 2, 64)])
def test_graph_capture_write_then_decode(D, Hkv, PAGE):
    """One captured write + decode replays at the start / pos in the tensor
    at replay time, across a page and a split boundary, bit for bit as the
    eager calls and within the fp64 bound."""
    ext = _ext()
    n = 4
    c = _chunk(n, Hkv, D)
    p1, p2 = c - 1, c
    assert p1 // PAGE != p2 // PAGE
    q, k_log, v_log = _qkv(D, Hkv)
    kp, vp, ks, vs, table = _build(k_log, v_log, PAGE, [p2] * B)
    new = torch.randn(B, Hkv, 1, D, device="cuda").bfloat16()
    scale, slopes, pos = D ** -0.5, _slopes("alibi"), _pos_tensor([p1])

    def step():
        ext.paged_kv_write_fp8(new, new, kp, vp, ks, vs, table, pos)
        return ext.paged_decode_attn_fp8(q, kp, vp, ks, vs, table, slopes,
                                         scale, pos, n)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    pos.fill_(p2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, step())
    row = paged_gather_dequant(kp, ks, table, CAP, torch.float64)[:, :, p2]
    assert (row - new[:, :, 0].double()).abs().max() \
        <= new.double().abs().max() * 2.0 ** -3          # the replay wrote p2
    ref = paged_decode_attention_reference(
        q.double(), kp, vp, table, slopes.double(), scale, pos, ks, vs)
    _check(out, ref, _vmax(vp, vs, table, [p2] * B), "replay at p2")


def test_host_checks():
    ext = _ext()
    D, Hkv, PAGE = 64, 2, 16
    q = torch.zeros(B, H, 1, D, device="cuda", dtype=torch.bfloat16)
    new = torch.zeros(B, Hkv, 3, D, device="cuda", dtype=torch.bfloat16)
    table = _layout(PAGE)[0].to("cuda", torch.int32)
    kp, vp, ks, vs = _sentinel_cache(PAGE, Hkv, D)
    slopes, pos = _slopes("alibi"), _pos_tensor([4])
    decode = lambda kp=kp, vp=vp, ks=ks, vs=vs, table=table: \
        ext.paged_decode_attn_fp8(q, kp, vp, ks, vs, table, slopes, 0.125,
                                  pos, 0)
    write = lambda kp=kp, vp=vp, ks=ks, vs=vs, table=table: \
        ext.paged_kv_write_fp8(new, new, kp, vp, ks, vs, table, pos)
    for call in (decode, write):
        with pytest.raises(RuntimeError, match="k_pool must be float8_e4m3fn"):
            call(kp=kp.view(torch.uint8).bfloat16())
        with pytest.raises(RuntimeError, match="v_scale must be fp32"):
            call(vs=vs.double())
        with pytest.raises(RuntimeError, match="k_scale has sizes"):
            call(ks=ks[:, :, :8].contiguous())
        with pytest.raises(RuntimeError, match="v_scale must be on the GPU"):
            call(vs=vs.cpu())
        with pytest.raises(RuntimeError, match="block_table must be an int32 "
                                               "GPU tensor"):
            call(table=table.cpu())
    for t in (kp, vp):                                     # nothing launched
        assert (t.view(torch.uint8) == BYTE_SENTINEL).all()
    for t in (ks, vs):
        assert (t.view(torch.int32) == SCALE_SENTINEL).all()
