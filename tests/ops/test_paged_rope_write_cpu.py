"""paged_rope_write on the CPU: the fp64 reference against the unfused fp64
pair it replaces, and the dispatcher's fallback against today's sequence."""
import pytest
import torch

from pipegoose_amd.ops.paged_attention import (
    paged_kv_write, paged_kv_write_reference, paged_rope_write,
    paged_rope_write_reference)
from pipegoose_amd.ops.rope import rope_at_position

B, H, HKV, D, PAGE, MAX_PAGES, N_POOL = 2, 4, 2, 16, 4, 3, 7
CAP = MAX_PAGES * PAGE
TABLE = torch.tensor([[5, 0, 3], [1, 6, 2]], dtype=torch.int32)
CASES = [(1, [0]), (1, [3, 4]), (5, [2, 6]), (5, [CAP - 2])]   # last: 3 dropped


def _inputs(S, dtype):
    g = torch.Generator().manual_seed(S)
    mk = lambda h: torch.randn(B, S, h, D, generator=g,
                               dtype=torch.float64).to(dtype).transpose(1, 2)
    return mk(H), mk(HKV), mk(HKV)


@pytest.mark.parametrize("S,start", CASES)
def test_reference_is_the_unfused_pair_in_fp64(S, start):
    q, k, v = _inputs(S, torch.float64)
    st = torch.tensor(start)
    got = [torch.full((N_POOL, HKV, PAGE, D), -7.0, dtype=torch.float64)
           for _ in range(2)]
    want = [p.clone() for p in got]
    q_rot = paged_rope_write_reference(q, k, v, *got, TABLE, st, 5e5)
    paged_kv_write_reference(rope_at_position(k, 5e5, st), v, *want, TABLE,
                             st)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[0] != -7.0).any()
    q_want = rope_at_position(q, 5e5, st)
    p = st.expand(B)[:, None] + torch.arange(S)
    dropped = (p >= CAP)[:, None, :, None].expand_as(q_rot)
    assert (q_rot[dropped] == 0).all()
    assert (q_rot - q_want)[~dropped].abs().max() <= 1e-12


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("S,start", CASES)
def test_cpu_dispatch_is_the_unfused_sequence(S, start, fp8):
    q, k, v = _inputs(S, torch.bfloat16)
    st = torch.tensor(start)
    pools, scales = [], []
    for _ in range(2):
        kp = torch.zeros(N_POOL, HKV, PAGE, D, dtype=torch.bfloat16)
        pools.append([kp.to(torch.float8_e4m3fn) if fp8 else kp,
                      kp.to(torch.float8_e4m3fn) if fp8 else kp.clone()])
        scales.append(dict(k_scale=torch.ones(N_POOL, HKV, PAGE),
                           v_scale=torch.ones(N_POOL, HKV, PAGE))
                      if fp8 else {})
    q_rot = paged_rope_write(q, k, v, *pools[0], TABLE, st, 1e4, **scales[0])
    paged_kv_write(rope_at_position(k, 1e4, st), v, *pools[1], TABLE, st,
                   **scales[1])
    assert torch.equal(q_rot, rope_at_position(q, 1e4, st))
    for a, b in zip(pools[0] + list(scales[0].values()),
                    pools[1] + list(scales[1].values())):
        assert torch.equal(a.view(torch.uint8) if fp8 and a.dim() == 4 else a,
                           b.view(torch.uint8) if fp8 and b.dim() == 4 else b)
