"""decode_attention on the CPU: the pure-torch reference equals what the
models' graph-mode / incremental decode branches compute today (sdpa with the
bias of BloomAttention._alibi_bias_graph, or llama's -inf position mask over
repeat_interleave'd kv heads), and the dispatcher falls back to it."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as TF

from pipegoose_amd.models.bloom import BloomAttention, alibi_slopes
from pipegoose_amd.ops.decode_attention import (decode_attention,
                                                decode_attention_reference,
                                                decode_kernel_supported)

B, H, D, SKV = 2, 4, 16, 37
SCALE = D ** -0.5


def _inputs(Hkv, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, 1, D, generator=g)
    k = torch.randn(B, Hkv, SKV, D, generator=g)
    v = torch.randn(B, Hkv, SKV, D, generator=g)
    return q, k, v


def _sdpa_bloom(q, k, v, slopes, pos_rows):
    """Today's graph-mode computation, one batch row at a time (the models
    share one position; per-row positions are rows of that)."""
    G = q.size(1) // k.size(1)
    ke, ve = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    outs = []
    for b, p in enumerate(pos_rows):
        attn = SimpleNamespace(alibi_slopes=slopes)
        bias = BloomAttention._alibi_bias_graph(
            attn, SKV, torch.tensor([p]), q.dtype)
        outs.append(TF.scaled_dot_product_attention(
            q[b:b + 1], ke[b:b + 1], ve[b:b + 1], attn_mask=bias,
            scale=SCALE))
    return torch.cat(outs)


def _sdpa_llama(q, k, v, pos_rows):
    """LlamaAttention's graph-mode branch: expanded heads, -inf beyond pos."""
    G = q.size(1) // k.size(1)
    ke, ve = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    kpos = torch.arange(SKV)
    outs = []
    for b, p in enumerate(pos_rows):
        bias = torch.zeros(1, 1, 1, SKV, dtype=q.dtype)
        bias = bias.masked_fill((kpos > p)[None, None, None], float("-inf"))
        outs.append(TF.scaled_dot_product_attention(
            q[b:b + 1], ke[b:b + 1], ve[b:b + 1], attn_mask=bias,
            scale=SCALE))
    return torch.cat(outs)


POS_CASES = [([0], [0, 0]), ([17], [17, 17]), ([36], [36, 36]),
             ([5, 30], [5, 30]), (None, [SKV - 1, SKV - 1])]


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("pos,rows", POS_CASES)
def test_reference_matches_bloom_graph_path(Hkv, pos, rows):
    q, k, v = _inputs(Hkv)
    slopes = alibi_slopes(H)
    pos_t = None if pos is None else torch.tensor(pos)
    out = decode_attention_reference(q, k, v, slopes, SCALE, pos_t)
    assert out.shape == (B, H, 1, D) and out.dtype == torch.float32
    torch.testing.assert_close(out, _sdpa_bloom(q, k, v, slopes, rows),
                               atol=1e-5, rtol=0)


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("pos,rows", POS_CASES)
def test_reference_matches_llama_graph_path(Hkv, pos, rows):
    q, k, v = _inputs(Hkv, seed=1)
    pos_t = None if pos is None else torch.tensor(pos)
    out = decode_attention_reference(q, k, v, torch.zeros(H), SCALE, pos_t)
    torch.testing.assert_close(out, _sdpa_llama(q, k, v, rows),
                               atol=1e-5, rtol=0)


def test_reference_ignores_the_cache_tail():
    """Slots beyond pos may hold any finite value, bf16-max included."""
    q, k, v = _inputs(2, seed=2)
    pos = torch.tensor([5, 30])
    clean = decode_attention_reference(q, k, v, alibi_slopes(H), SCALE, pos)
    k2, v2 = k.clone(), v.clone()
    for b, p in enumerate(pos.tolist()):
        k2[b, :, p + 1:] = 1e30
        v2[b, :, p + 1:] = -1e30
    dirty = decode_attention_reference(q, k2, v2, alibi_slopes(H), SCALE, pos)
    assert torch.equal(clean, dirty)


def test_reference_keeps_fp64():
    q, k, v = (t.double() for t in _inputs(2, seed=3))
    out = decode_attention_reference(q, k, v, alibi_slopes(H), SCALE,
                                     torch.tensor([17]))
    assert out.dtype == torch.float64


def test_cpu_dispatch_is_the_reference():
    q, k, v = _inputs(2, seed=4)
    slopes, pos = alibi_slopes(H), torch.tensor([5, 30])
    assert not decode_kernel_supported(q, k)
    assert not decode_kernel_supported(q.bfloat16(), k.bfloat16())
    assert torch.equal(decode_attention(q, k, v, slopes, SCALE, pos),
                       decode_attention_reference(q, k, v, slopes, SCALE, pos))
    assert torch.equal(decode_attention(q, k, v, slopes, SCALE),
                       decode_attention_reference(q, k, v, slopes, SCALE))


def test_inference_only():
    q, k, v = _inputs(2, seed=5)
    q.requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        decode_attention(q, k, v, alibi_slopes(H), SCALE)
    with torch.no_grad():
        decode_attention(q, k, v, alibi_slopes(H), SCALE)
