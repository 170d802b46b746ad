"""Ragged decode over the paged cache on the GPU, both model families, bf16,
the tiny configs of tests/ops/test_decode_attn_gpu.py.

Oracle: the fp32 CPU twin, each prompt alone.  ``e_old`` is the error of the
bf16 path that exists without this feature (each prompt alone,
``PG_DECODE_ATTN=0``), ``e_paged`` the error of the ragged batch through
PagedKVCache; the project's rule is e_paged <= 2 * e_old, both measured
here.
"""
import dataclasses
import os

import pytest
import torch

from pipegoose_amd.ops import get_extension

pytestmark = pytest.mark.gpu

LENGTHS, N_STEPS, PAGE, MAX_LEN = (5, 16, 23), 6, 16, 48


def _ctx():
    """A single-rank context; the rendezvous variables go back to what they
    were, so that tests that start further processes do not inherit them."""
    from pipegoose_amd import ParallelContext
    env = {"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29894", "RANK": "0",
           "WORLD_SIZE": "1"}
    saved = {name: os.environ.get(name) for name in env}
    for name, value in env.items():
        os.environ.setdefault(name, value)
    try:
        return ParallelContext.from_torch()
    finally:
        for name, value in saved.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value


def _build(family):
    if family == "bloom":
        from pipegoose_amd.models.bloom import BloomConfig, BloomForCausalLM
        cfg = BloomConfig(vocab_size=256, hidden_size=128, n_layer=2,
                          n_head=2)
        return BloomForCausalLM(cfg, _ctx()).eval()
    from pipegoose_amd.models.llama import LlamaForCausalLM, llama_tiny
    cfg = dataclasses.replace(llama_tiny(), hidden_size=256,
                              intermediate_size=512, n_head=4, n_kv_head=2)
    return LlamaForCausalLM(cfg, _ctx()).eval()


def _fp32_cpu_copy(model, family):
    """The same model in fp32 on the CPU: same weights and buffers."""
    twin = _build(family)
    twin.load_state_dict(model.state_dict())
    buffers = dict(model.named_buffers())
    with torch.no_grad():
        for name, buf in twin.named_buffers():
            buf.copy_(buffers[name])
    return twin


@torch.no_grad()
def _alone(model, prompts, forced):
    """[steps, n, V]: every prompt alone through the contiguous cache."""
    dev = next(model.parameters()).device
    per_prompt = []
    for i, prompt in enumerate(prompts):
        past = model.new_kv_cache(1, MAX_LEN)
        model(prompt[None].to(dev), past=past, use_cache=True)
        steps = []
        for t in range(N_STEPS):
            logits, _ = model(forced[i:i + 1, t:t + 1].to(dev), past=past,
                              use_cache=True)
            steps.append(logits[0, -1].float().cpu())
        per_prompt.append(torch.stack(steps))
    return torch.stack(per_prompt, dim=1)


@torch.no_grad()
def _paged(model, prompts, forced):
    """[steps, n, V]: the ragged batch through PagedKVCache."""
    n = len(prompts)
    need = sum(-(-(p.numel() + N_STEPS) // PAGE) for p in prompts)
    cache = model.new_paged_kv_cache(n, need + 1, PAGE, MAX_LEN)
    for i, prompt in enumerate(prompts):
        cache.allocate(i, prompt.numel() + N_STEPS)
    for i, prompt in enumerate(prompts):
        rows = cache.rows(i, i + 1)
        model(prompt[None].cuda(), past=rows, use_cache=True)
        rows.advance(prompt.numel())
    rows = cache.rows(0, n)
    steps = []
    for t in range(N_STEPS):
        logits, _ = model(forced[:, t:t + 1].cuda(), past=rows,
                          use_cache=True)
        rows.advance(1)
        steps.append(logits[:, -1].float().cpu())
    return torch.stack(steps)


def _count(monkeypatch, name):
    ext = get_extension(required=True)
    real, calls = getattr(ext, name), []

    def counting(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ext, name, counting)
    return calls


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_ragged_paged_decode(family, monkeypatch):
    torch.manual_seed(93)
    model = _build(family).to("cuda", torch.bfloat16)
    n_layer = model.config.n_layer
    oracle = _fp32_cpu_copy(model, family)
    g = torch.Generator().manual_seed(94)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    forced = torch.randint(0, 256, (len(LENGTHS), N_STEPS), generator=g)
    calls = _count(monkeypatch, "paged_decode_attn")

    want = _alone(oracle, prompts, forced)
    monkeypatch.setenv("PG_DECODE_ATTN", "0")
    old = _alone(model, prompts, forced)
    monkeypatch.setenv("PG_DECODE_ATTN", "1")
    assert not calls
    new = _paged(model, prompts, forced)
    assert len(calls) == n_layer * N_STEPS, \
        f"{len(calls)} paged kernel calls, expected {n_layer} per step"

    e_old = (old - want).abs().max().item()
    e_paged = (new - want).abs().max().item()
    print(f"{family}: e_old={e_old:.4g} e_paged={e_paged:.4g}")
    assert torch.isfinite(new).all()
    assert e_paged <= 2 * e_old, (e_paged, e_old)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_paged_decoder_graph_matches_eager(family, monkeypatch):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    torch.manual_seed(95)
    model = _build(family).to("cuda", torch.bfloat16)
    prompts = [torch.randint(0, 256, (n,), device="cuda") for n in LENGTHS]
    new = 12
    need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
    calls = _count(monkeypatch, "paged_decode_attn")
    ref = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN,
                       use_graph=False).generate(prompts, new)
    assert len(calls) == model.config.n_layer * (new - 1)
    dec = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN)
    out = dec.generate(prompts, new)
    assert dec._graph is not None, "hipGraph capture failed"
    assert dec.cache.n_free_pages == need
    for a, b in zip(out, ref):
        assert a.shape == (new,) and torch.equal(a, b), (out, ref)
    # a second call gets the freed pages in another order and replays the
    # captured step against the rewritten table rows
    assert not dec.cache.block_table.any()      # every slot was freed
    again = dec.generate(prompts, new)
    for a, b in zip(again, ref):
        assert torch.equal(a, b)
