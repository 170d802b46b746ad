"""Decode attention kernel (csrc/decode_attention.hip) against the fp64
reference, at op level and through both model families.

Oracle: decode_attention_reference on the fp64 upcast of the same bf16
inputs.  In every case the cache tail j > p holds +1e30 (K) / -1e30 (V): a
finite result that meets the bound shows that nothing beyond p leaks.

Tolerance |out - ref| <= 2^-7*|ref| + 2^-7*max|v|: the output is a convex
combination of V rows, so its bf16 rounding is <= 2^-9*|out|; an
implementation that rounds P to bf16 adds <= 2^-9*max|v|; fp32 accumulation
over <= 320 terms and the exp2 approximation are orders of magnitude below
that.  The bound is the sum of the two with a 4x margin.  With these shapes
max|v| ~ 4.5 (absolute term ~ 0.035) while dropping the single key j = p
moves the output by ~ 0.8, so an off-by-one at the causal edge cannot hide.
"""
import dataclasses
import functools
import os

import pytest
import torch

from pipegoose_amd.models.bloom import alibi_slopes
from pipegoose_amd.ops import get_extension
from pipegoose_amd.ops.decode_attention import (decode_attention,
                                                decode_attention_reference,
                                                decode_kernel_supported)

pytestmark = pytest.mark.gpu

B, H = 2, 4
TILE = 64          # keys per workgroup iteration (decode_attention.hip header)
SHAPES = [(D, Hkv, Skv) for D in (64, 128) for Hkv in (4, 2, 1)
          for Skv in (320, 77)]
SPLITS = (1, 4, 0)  # forced, forced, auto


def _ext():
    return get_extension(required=True)


def _chunk(n_splits, Hkv, Skv, D):
    """The plan rule of the kernel's file header."""
    if n_splits == 0:
        return _ext().decode_attn_plan(B, Hkv, Skv, D)[1]
    per_split = (Skv + n_splits - 1) // n_splits
    return (per_split + TILE - 1) // TILE * TILE


def _positions(c, Skv):
    return sorted({min(max(p, 0), Skv - 1)
                   for p in (0, 1, c - 1, c, c + 1, Skv - 1)})


def _slopes(kind):
    s = alibi_slopes(H) if kind == "alibi" else torch.zeros(H)
    return s.to("cuda", torch.float32)


@functools.lru_cache(maxsize=None)
def _qkv(D, Hkv, Skv):
    """One set of random inputs per shape, shared and never modified."""
    g = torch.Generator(device="cuda").manual_seed(1000 + D + 7 * Hkv + Skv)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    return mk(B, H, 1, D), mk(B, Hkv, Skv, D), mk(B, Hkv, Skv, D)


def _poison_tail(k, v, pos_rows):
    k, v = k.clone(), v.clone()
    for b, p in enumerate(pos_rows):
        k[b, :, p + 1:] = 1e30
        v[b, :, p + 1:] = -1e30
    return k, v


def _pos_tensor(pos_rows):
    rows = pos_rows if len(set(pos_rows)) > 1 else pos_rows[:1]
    return torch.tensor(rows, device="cuda", dtype=torch.long)


def _check(out, ref, vmax, what):
    assert out.shape == ref.shape, what
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out.double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -7 * vmax
    worst = (err - bound).max().item()
    assert worst <= 0, (f"{what}: max err {err.max().item():.4g}, exceeds "
                        f"the bound by {worst:.4g}")


def _cases(D, Hkv, Skv):
    """(n_splits, chunk, pos_rows) over the plans and the edge positions,
    plus one per-row case per plan."""
    for n in SPLITS:
        c = _chunk(n, Hkv, Skv, D)
        for p in _positions(c, Skv):
            yield n, c, [p] * B
        yield n, c, [min(c + 1, Skv - 1), 0]


@pytest.mark.parametrize("D,Hkv,Skv", SHAPES)
def test_random_inputs(D, Hkv, Skv):
    ext = _ext()
    q, k0, v0 = _qkv(D, Hkv, Skv)
    scale = D ** -0.5
    vmax = v0.double().abs().max().item()
    for kind in ("alibi", "zero"):
        slopes = _slopes(kind)
        for n, c, rows in _cases(D, Hkv, Skv):
            k, v = _poison_tail(k0, v0, rows)
            pos = _pos_tensor(rows)
            out = ext.decode_attn(q, k, v, slopes, scale, pos, n)
            assert out.dtype == torch.bfloat16
            # physically [B, 1, H, D]: the model's reshape is free
            assert out.transpose(1, 2).is_contiguous()
            ref = decode_attention_reference(
                q.double(), k.double(), v.double(), slopes.double(), scale,
                pos)
            _check(out, ref, vmax,
                   f"{kind} n_splits={n} chunk={c} pos={rows}")


@pytest.mark.parametrize("D,Hkv,Skv", SHAPES)
def test_pos_none_is_last_slot(D, Hkv, Skv):
    """pos=None (eager incremental path) means p = Skv-1, on the full buffer
    and on the [:, :, :len] prefix view of a longer one, with no copy."""
    ext = _ext()
    q, k, v = _qkv(D, Hkv, Skv)
    scale, slopes = D ** -0.5, _slopes("alibi")
    vmax = v.double().abs().max().item()
    for length in (Skv, Skv - 13, 1):
        kk, vv = k[:, :, :length], v[:, :, :length]
        out = ext.decode_attn(q, kk, vv, slopes, scale, None, 0)
        ref = decode_attention_reference(q.double(), kk.double(), vv.double(),
                                         slopes.double(), scale)
        _check(out, ref, vmax, f"pos=None len={length}")
        assert torch.equal(out, decode_attention(q, kk, vv, slopes, scale))


@pytest.mark.parametrize("D,Hkv,Skv", SHAPES)
def test_every_index_is_reachable(D, Hkv, Skv):
    """K is zero except row j*, which is aligned with the group's first q
    head strongly enough that softmax puts all weight there: out == v[j*].
    A split boundary that is dropped or counted twice shows here, where a
    diffuse random softmax hides it."""
    ext = _ext()
    q, _, v0 = _qkv(D, Hkv, Skv)
    G = H // Hkv
    scale = D ** -0.5
    gain = 30 + 0.25 * Skv
    vmax = v0.double().abs().max().item()
    q0 = q[:, ::G, 0].float()                                  # [B, Hkv, D]
    krow = (gain * q0 / (scale * (q0 * q0).sum(-1, keepdim=True))).bfloat16()
    for kind in ("alibi", "zero"):
        slopes = _slopes(kind)
        for n in SPLITS:
            c = _chunk(n, Hkv, Skv, D)
            for p in _positions(c, Skv):
                for js in sorted({min(j, p) for j in (0, p, c - 1, c)}):
                    k = torch.zeros_like(v0)
                    k[:, :, js] = krow
                    k, v = _poison_tail(k, v0, [p] * B)
                    out = ext.decode_attn(q, k, v, slopes, scale,
                                          _pos_tensor([p] * B), n)
                    assert torch.isfinite(out).all()
                    _check(out[:, ::G, 0], v[:, :, js].double(), vmax,
                           f"{kind} n_splits={n} chunk={c} pos={p} j*={js}")


@pytest.mark.parametrize("D,Hkv,Skv", [(64, 2, 320), (128, 1, 77)])
def test_deterministic(D, Hkv, Skv):
    ext = _ext()
    q, k, v = _qkv(D, Hkv, Skv)
    pos = _pos_tensor([Skv - 1, Skv // 2])
    for n in SPLITS:
        a = ext.decode_attn(q, k, v, _slopes("alibi"), D ** -0.5, pos, n)
        b = ext.decode_attn(q, k, v, _slopes("alibi"), D ** -0.5, pos, n)
        assert torch.equal(a, b)


@pytest.mark.parametrize("D,Hkv", [(64, 4), (128, 2)])
def test_graph_capture_reads_pos_on_device(D, Hkv):
    """A captured call replays at the position that is in ``pos`` at replay
    time; a position baked in at capture time fails this."""
    ext = _ext()
    Skv, n = 320, 4
    c = _chunk(n, Hkv, Skv, D)
    p1, p2 = c - 1, c + 1              # replay crosses a split boundary
    q, k0, v0 = _qkv(D, Hkv, Skv)
    k, v = _poison_tail(k0, v0, [p1] * B)
    scale, slopes = D ** -0.5, _slopes("alibi")
    pos = _pos_tensor([p1])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.decode_attn(q, k, v, slopes, scale, pos, n)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext.decode_attn(q, k, v, slopes, scale, pos, n)

    pos.fill_(p2)
    k[:, :, p1 + 1:p2 + 1] = k0[:, :, p1 + 1:p2 + 1]
    v[:, :, p1 + 1:p2 + 1] = v0[:, :, p1 + 1:p2 + 1]
    graph.replay()
    torch.cuda.synchronize()
    eager = ext.decode_attn(q, k, v, slopes, scale, _pos_tensor([p2]), n)
    assert torch.equal(out, eager)
    ref = decode_attention_reference(q.double(), k.double(), v.double(),
                                     slopes.double(), scale, pos)
    _check(out, ref, v0.double().abs().max().item(), "replay at p2")


def test_plan():
    ext = _ext()
    for D, Hkv, Skv in SHAPES + [(128, 8, 4096), (64, 16, 1)]:
        n, c = ext.decode_attn_plan(8, Hkv, Skv, D)
        assert 1 <= n <= 64 and c % TILE == 0
        assert (n - 1) * c < Skv <= n * c      # covers Skv, no empty split
    with pytest.raises(RuntimeError):
        ext.decode_attn_plan(2, 4, 320, 32)
    with pytest.raises(RuntimeError):
        ext.decode_attn_plan(2, 4, 0, 64)


def test_host_checks():
    ext = _ext()
    q, k, v = _qkv(64, 2, 77)
    slopes, scale = _slopes("alibi"), 0.125
    ok_pos = _pos_tensor([5])
    with pytest.raises(RuntimeError, match="bf16"):
        ext.decode_attn(q.float(), k, v, slopes, scale, ok_pos, 0)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.decode_attn(q, k, v.half(), slopes, scale, ok_pos, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.decode_attn(q, k.cpu(), v, slopes, scale, ok_pos, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.decode_attn(q, k, v, slopes.cpu(), scale, ok_pos, 0)
    with pytest.raises(RuntimeError, match="64 or 128"):
        ext.decode_attn(q[..., :32].contiguous(), k[..., :32].contiguous(),
                        v[..., :32].contiguous(), slopes, scale, ok_pos, 0)
    q3 = torch.zeros(B, 3, 1, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of kv heads"):
        ext.decode_attn(q3, k, v, slopes[:3].contiguous(), scale, ok_pos, 0)
    with pytest.raises(RuntimeError, match="pos"):
        ext.decode_attn(q, k, v, slopes, scale, _pos_tensor([1, 2, 3]), 0)
    with pytest.raises(RuntimeError, match="pos"):
        ext.decode_attn(q, k, v, slopes, scale, ok_pos.int(), 0)
    with pytest.raises(RuntimeError, match="n_splits"):
        ext.decode_attn(q, k, v, slopes, scale, ok_pos, 65)
    with pytest.raises(RuntimeError, match="q must be"):
        ext.decode_attn(q[:, :, 0], k, v, slopes, scale, ok_pos, 0)
    with pytest.raises(RuntimeError, match="sizes"):
        ext.decode_attn(q.expand(B, H, 2, 64), k, v, slopes, scale, ok_pos, 0)


def test_opt_out_and_dispatch(monkeypatch):
    q, k, v = _qkv(64, 2, 77)
    assert decode_kernel_supported(q, k)
    assert not decode_kernel_supported(q.float(), k.float())
    assert not decode_kernel_supported(q.expand(B, H, 2, 64), k)
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    assert not decode_kernel_supported(q, k)
    monkeypatch.setenv("PG_DECODE_ATTN", "1")
    assert decode_kernel_supported(q, k)


# ---------------------------------------------------------------- model level

def _ctx():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29893")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    from pipegoose_amd import ParallelContext
    return ParallelContext.from_torch()


def _bloom():
    from pipegoose_amd.models.bloom import BloomConfig, BloomForCausalLM
    cfg = BloomConfig(vocab_size=256, hidden_size=128, n_layer=2, n_head=2)
    return BloomForCausalLM(cfg, _ctx())


def _llama():
    from pipegoose_amd.models.llama import LlamaForCausalLM, llama_tiny
    cfg = dataclasses.replace(llama_tiny(), hidden_size=256,
                              intermediate_size=512, n_head=4, n_kv_head=2)
    return LlamaForCausalLM(cfg, _ctx())


def _build(family):
    return (_bloom() if family == "bloom" else _llama()).eval()


def _fp32_cpu_copy(model, family):
    """The same model in fp32 on the CPU: same weights and buffers (the
    bf16-rounded ALiBi slopes included), sdpa attention."""
    twin = _build(family)
    twin.load_state_dict(model.state_dict())
    buffers = dict(model.named_buffers())
    with torch.no_grad():
        for name, buf in twin.named_buffers():
            buf.copy_(buffers[name])
    return twin


N_STEPS, MAX_LEN = 6, 48


@torch.no_grad()
def _step_logits(model, prompt, forced):
    """Prefill, then N_STEPS graph-mode steps run eagerly on the given
    (teacher-forced) tokens; returns the logits of those steps."""
    cache = model.new_graph_kv_cache(prompt.size(0), MAX_LEN)
    model(prompt, past=cache, use_cache=True)
    cache.enter_graph_mode()
    steps = []
    for t in range(N_STEPS):
        logits, _ = model(forced[:, t:t + 1], past=cache, use_cache=True)
        cache.advance()
        steps.append(logits[:, -1].float().cpu())
    return torch.stack(steps)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_model_decode_uses_the_kernel(family, monkeypatch):
    torch.manual_seed(90)
    model = _build(family).to("cuda", torch.bfloat16)
    n_layer = model.config.n_layer
    oracle = _fp32_cpu_copy(model, family)
    g = torch.Generator().manual_seed(91)
    prompt = torch.randint(0, 256, (2, 16), generator=g)
    forced = torch.randint(0, 256, (2, N_STEPS), generator=g)

    ext = _ext()
    real, calls = ext.decode_attn, []

    def counting(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ext, "decode_attn", counting)

    want = _step_logits(oracle, prompt, forced)
    assert not calls
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    old = _step_logits(model, prompt.cuda(), forced.cuda())
    assert not calls, "PG_DECODE_ATTN=0 must keep the sdpa path"
    monkeypatch.setenv("PG_DECODE_ATTN", "1")
    new = _step_logits(model, prompt.cuda(), forced.cuda())
    assert len(calls) == n_layer * N_STEPS, \
        f"{len(calls)} kernel calls, expected {n_layer} per step"

    e_old = (old - want).abs().max().item()
    e_new = (new - want).abs().max().item()
    print(f"{family}: e_old={e_old:.4g} e_new={e_new:.4g}")
    assert torch.isfinite(new).all()
    assert e_new <= 2 * e_old, (e_new, e_old)

    # eager incremental path (sampling / eos / TP serving): q_len 1 against
    # the growing prefix view, pos=None
    calls.clear()
    with torch.no_grad():
        past = model.new_kv_cache(2, MAX_LEN)
        model(prompt.cuda(), past=past, use_cache=True)
        logits, _ = model(forced[:, :1].cuda(), past=past, use_cache=True)
    assert len(calls) == n_layer
    e_inc = (logits[:, -1].float().cpu() - want[0]).abs().max().item()
    print(f"{family}: e_incremental={e_inc:.4g}")
    assert e_inc <= 2 * e_old, (e_inc, e_old)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_graph_decoder_matches_eager(family, monkeypatch):
    from pipegoose_amd.models.graph_decode import GraphDecoder
    torch.manual_seed(92)
    model = _build(family).to("cuda", torch.bfloat16)
    prompt = torch.randint(0, 256, (2, 16), device="cuda")

    ext = _ext()
    real, calls = ext.decode_attn, []

    def counting(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ext, "decode_attn", counting)
    ref = GraphDecoder(model, 2, MAX_LEN, use_graph=False).generate(prompt, 12)
    assert len(calls) == model.config.n_layer * 11
    dec = GraphDecoder(model, 2, MAX_LEN)
    out = dec.generate(prompt, 12)
    assert dec._graph is not None, "hipGraph capture failed"
    assert torch.equal(out, ref), (out, ref)
