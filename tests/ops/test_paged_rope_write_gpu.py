"""paged_rope_write kernels (csrc/paged_rope_write.hip) against the fp64
reference on the same bf16 inputs.  With r the norm of a rotation pair of the
input: rotated bf16 values (q_rot, cached K) are within ROT * r, ROT = 2^-8
(bf16 half-ulp of a value up to r) + 2^-11 (angle and fp32 arithmetic); the
bf16 V row is bit-equal; an fp8 element is within the write bound of
tests/ops/test_paged_fp8_attn_gpu.py on top (K) or alone (V); pool bytes and
scales outside the addressed rows keep a sentinel."""
import pytest
import torch

from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.paged_attention import (
    paged_decode_attention, paged_rope_write, paged_rope_write_reference,
    rope_freq_table)

pytestmark = pytest.mark.gpu

B, N_POOL, FP8 = 2, 9, torch.float8_e4m3fn
ROT, Q8 = 2.0 ** -8 + 2.0 ** -11, 1 + 2.0 ** -10
BYTE, WORD = 0x5A, 0x3F9D70A5                       # sentinels
SHAPES = [(64, 4, 2, 16), (64, 2, 1, 128), (128, 4, 4, 16), (128, 4, 2, 128)]


def _cache(Hkv, PAGE, D, fp8, max_pages=4, seed=0):
    """Sentinel pools [+ scales] and a shuffled table whose last column is
    real whatever ``max_pages`` (every other entry of a long table is 0)."""
    g = torch.Generator().manual_seed(seed + PAGE)
    ids = (torch.randperm(N_POOL - 1, generator=g) + 1)[:B * 4].view(B, 4)
    table = torch.zeros(B, max_pages, dtype=torch.int32)
    table[:, :3], table[:, -1] = ids[:, :3], ids[:, 3]
    n = N_POOL * Hkv * PAGE * D
    mk = (lambda: torch.full((n,), BYTE, dtype=torch.uint8).view(FP8)) if fp8 \
        else (lambda: torch.full((n // 2,), BYTE * 0x01010101,
                                 dtype=torch.int32).view(torch.bfloat16))
    pools = [mk().view(N_POOL, Hkv, PAGE, D).cuda() for _ in range(2)]
    scales = [torch.full((N_POOL, Hkv, PAGE), WORD, dtype=torch.int32)
              .view(torch.float32).cuda() for _ in range(2 * fp8)]
    return pools, scales, table.cuda()


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("D,H,Hkv,PAGE", SHAPES)
def test_against_fp64(D, H, Hkv, PAGE, theta, fp8):
    g = torch.Generator(device="cuda").manual_seed(D + H + PAGE)
    cases = [(1, [0], 4), (1, [PAGE - 1, PAGE], 4), (5, [PAGE - 2], 4),
             (37, [5, PAGE], 4), (5, [4 * PAGE - 2], 4), (3, [-1], 4)]
    if PAGE == 128:                                  # capacity 2^17
        cases += [(1, [131071 - 4], 1024), (5, [131071 - 4], 1024)]
    for S, start, max_pages in cases:
        pools, scales, table = _cache(Hkv, PAGE, D, fp8, max_pages)
        # transposed views of a wider buffer: strided in all dims but the last
        mk = lambda h: torch.randn(B, S, h, D + 8, device="cuda", generator=g
                                   ).bfloat16()[..., 8:].transpose(1, 2)
        q, k, v = mk(H), mk(Hkv), mk(Hkv)
        k[:, :, min(1, S - 1)] = 0                   # amax == 0
        st = torch.tensor(start, device="cuda")
        q_rot = paged_rope_write(q, k, v, *pools, table, st, theta,
                                 *scales).double()
        ref = [torch.zeros(N_POOL, Hkv, PAGE, D, device="cuda",
                           dtype=torch.float64) for _ in range(2)]
        q_ref = paged_rope_write_reference(q.double(), k.double(), v.double(),
                                           *ref, table, st, theta)
        p = st.expand(B)[:, None] + torch.arange(S, device="cuda")
        keep = (p >= 0) & (p < max_pages * PAGE)                   # [B, S]
        ids = table.long().gather(1, p.clamp(0, max_pages * PAGE - 1)
                                  // PAGE)[keep]
        slot = (p % PAGE)[keep]
        pair = lambda x: (x[..., :D // 2] ** 2 + x[..., D // 2:] ** 2
                          ).sqrt().repeat(1, 1, 2)
        what = f"S={S} start={start}"

        qk = q.double().transpose(1, 2)[keep]
        err = (q_rot.transpose(1, 2)[keep] - q_ref.transpose(1, 2)[keep]).abs()
        print(what, "q worst err/r", (err / pair(qk)).nan_to_num(0).max().item())
        assert (err <= ROT * pair(qk)).all(), what
        assert (q_rot.transpose(1, 2)[~keep] == 0).all(), what

        x = v.double().transpose(1, 2)[keep]
        r = pair(k.double().transpose(1, 2)[keep])
        yb = ref[0][ids, :, slot]                                  # [n, Hkv, D]
        if not fp8:
            err = (pools[0][ids, :, slot].double() - yb).abs()
            print(what, "k worst err/r", (err / r).nan_to_num(0).max().item())
            assert (err <= ROT * r).all(), what
            assert torch.equal(pools[1][ids, :, slot].double(), x), what
        else:
            deq = lambda i: pools[i].view(torch.uint8)[ids, :, slot].view(
                FP8).double() * scales[i][ids, :, slot].double()[..., None]
            sk, sv = (s[ids, :, slot].double() for s in scales)
            assert ((sk - yb.abs().amax(-1) / 448).abs()
                    <= ROT * r.amax(-1) / 448 + 2.0 ** -22 * sk).all(), what
            assert ((deq(0) - yb).abs() <= ROT * r + Q8 * torch.maximum(
                yb.abs() * 2.0 ** -4, sk[..., None] * 2.0 ** -10)).all(), what
            want = x.abs().amax(-1) / 448
            assert ((sv - want).abs() <= 2.0 ** -22 * want).all(), what
            assert ((deq(1) - x).abs() <= Q8 * torch.maximum(
                x.abs() * 2.0 ** -4, sv[..., None] * 2.0 ** -10)).all(), what
            zero = (k.transpose(1, 2)[keep] == 0).all(-1)          # [n, Hkv]
            assert zero.any() and (sk[zero] == 0).all() and \
                (pools[0].view(torch.uint8)[ids, :, slot][zero] == 0).all()
        untouched = torch.ones(N_POOL, PAGE, dtype=torch.bool, device="cuda")
        untouched[ids, slot] = False
        mask = untouched[:, None, :].expand(-1, Hkv, -1)
        for pool in pools:
            assert (pool.view(torch.uint8)[mask] == BYTE).all(), what
        for scale in scales:
            assert (scale.view(torch.int32)[mask] == WORD).all(), what


@pytest.mark.parametrize("D,H,Hkv,PAGE,fp8", [(64, 4, 2, 16, False),
                                              (128, 4, 2, 128, True)])
def test_graph_capture_with_decode(D, H, Hkv, PAGE, fp8):
    """One captured rope-write + decode replays at the position in the tensor
    at replay time, across a page edge, bit for bit as the eager calls."""
    pools, scales, table = _cache(Hkv, PAGE, D, fp8)
    for t in pools + scales:                         # a readable cache
        t.view(torch.uint8).fill_(0x38 if t.dim() == 4 else 0)
    mk = lambda h: torch.randn(B, h, 1, D, device="cuda").bfloat16()
    q, k, v = mk(H), mk(Hkv), mk(Hkv)
    pos = torch.tensor([PAGE - 1], device="cuda")
    slopes = torch.zeros(H, device="cuda")

    def step():
        q_rot = paged_rope_write(q, k, v, *pools, table, pos, 1e4, *scales)
        return paged_decode_attention(q_rot, *pools, table, slopes,
                                      D ** -0.5, pos, *scales)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    pos.fill_(PAGE)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, step())
    ref = [torch.zeros(N_POOL, Hkv, PAGE, D, device="cuda",
                       dtype=torch.float64) for _ in range(2)]
    paged_rope_write_reference(q.double(), k.double(), v.double(), *ref,
                               table, pos, 1e4)
    ids = table[:, 1].long()
    yb = ref[0][ids, :, 0]                                         # [B, Hkv, D]
    sk = scales[0][ids, :, 0].double()[..., None] if fp8 else 1
    got = pools[0].view(torch.uint8)[ids, :, 0].view(FP8).double() * sk \
        if fp8 else pools[0][ids, :, 0].double()
    kd = k[:, :, 0].double()
    r = (kd[..., :D // 2] ** 2 + kd[..., D // 2:] ** 2).sqrt().repeat(1, 1, 2)
    bound = ROT * r + (Q8 * torch.maximum(yb.abs() * 2.0 ** -4,
                                          sk * 2.0 ** -10) if fp8 else 0)
    assert ((got - yb).abs() <= bound).all()         # the replay wrote PAGE


def test_host_checks():
    ext = get_extension(required=True)
    (kp, vp), _, table = _cache(2, 16, 64, False)
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    q, k, st = z(B, 4, 3, 64), z(B, 2, 3, 64), torch.zeros(1, device="cuda",
                                                           dtype=torch.long)
    tab = rope_freq_table(1e4, 64, "cuda")
    call = lambda q=q, k=k, kp=kp, st=st, tab=tab: ext.paged_rope_write(
        q, k, k, kp, vp, table, st, 1e4, tab)
    for bad in (dict(q=q.float()), dict(k=k.cpu()), dict(tab=tab.cpu()),
                dict(q=z(B, 4, 3, 32), k=z(B, 2, 3, 32)),
                dict(kp=kp[:, :, :8].contiguous()),
                dict(st=torch.zeros(3, device="cuda", dtype=torch.long))):
        with pytest.raises(RuntimeError, match="paged_rope_write: "):
            call(**bad)
    for t in (kp, vp):                               # nothing launched
        assert (t.view(torch.uint8) == BYTE).all()
