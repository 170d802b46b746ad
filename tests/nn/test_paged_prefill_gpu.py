"""Chunked prefill and prefix sharing over the paged cache on the GPU, both
model families, bf16, the tiny configs of tests/nn/test_paged_decode_gpu.py.

Oracle: the fp32 CPU twin, the whole prompt at once.  ``e_old`` is the error
of the bf16 path that exists without this feature (the whole prompt prefilled
into an empty slot of the paged cache), ``e_new`` the error of the same
prompt in chunks of 16 and, separately, behind the forked pages of another
prompt; the project's rule is e_new <= 2 * e_old, all measured here, over the
logits of the tokens each run computes and of 4 forced decode steps after.
"""
import pytest
import torch

from tests.nn.test_paged_decode_gpu import _build, _count, _fp32_cpu_copy

pytestmark = pytest.mark.gpu

PROMPT, CHUNK, N_STEPS, PAGE, MAX_LEN = 45, 16, 4, 16, 64
SHARED = 32             # two whole pages of the 37-token common prefix


@torch.no_grad()
def _run(model, prompt, forced, chunk, fork_from=None):
    """Logits [len(prompt) - done + N_STEPS, V] of the tokens run and of the
    forced decode steps.  ``fork_from``: another prompt that is prefilled
    first and whose first SHARED tokens' pages the run reuses."""
    dev = next(model.parameters()).device
    cache = model.new_paged_kv_cache(2, 9, PAGE, MAX_LEN)
    done = 0
    if fork_from is not None:
        cache.allocate(1, fork_from.numel())
        other = cache.rows(1, 2)
        model(fork_from[None].to(dev), past=other, use_cache=True)
        other.advance(fork_from.numel())
        done = cache.fork(1, 0, SHARED)
        assert done == SHARED
    cache.allocate(0, prompt.numel() + N_STEPS)
    rows = cache.rows(0, 1)
    out = []
    for lo in range(done, prompt.numel(), chunk):
        piece = prompt[lo:lo + chunk]
        logits, _ = model(piece[None].to(dev), past=rows, use_cache=True)
        rows.advance(piece.numel())
        out.append(logits[0].float().cpu())
    for t in range(N_STEPS):
        logits, _ = model(forced[None, t:t + 1].to(dev), past=rows,
                          use_cache=True)
        rows.advance(1)
        out.append(logits[0].float().cpu())
    return torch.cat(out)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_chunked_and_shared_prefill(family, monkeypatch):
    torch.manual_seed(193)
    model = _build(family).to("cuda", torch.bfloat16)
    n_layer = model.config.n_layer
    oracle = _fp32_cpu_copy(model, family)
    g = torch.Generator().manual_seed(194)
    system = torch.randint(0, 256, (37,), generator=g)
    prompt = torch.cat([system, torch.randint(0, 256, (PROMPT - 37,),
                                              generator=g)])
    other = torch.cat([system, torch.randint(0, 256, (3,), generator=g)])
    forced = torch.randint(0, 256, (N_STEPS,), generator=g)
    prefill_calls = _count(monkeypatch, "paged_prefill_attn")
    decode_calls = _count(monkeypatch, "paged_decode_attn")

    want = _run(oracle, prompt, forced, PROMPT)
    assert not prefill_calls and not decode_calls
    old = _run(model, prompt, forced, PROMPT)
    assert not prefill_calls, "a whole-prompt prefill must stay on its path"
    assert len(decode_calls) == n_layer * N_STEPS
    chunked = _run(model, prompt, forced, CHUNK)
    chunks = -(-PROMPT // CHUNK)
    assert len(prefill_calls) == n_layer * (chunks - 1), \
        f"{len(prefill_calls)} paged prefill kernel calls, expected " \
        f"{n_layer} per chunk after the first"
    assert len(decode_calls) == 2 * n_layer * N_STEPS
    shared = _run(model, prompt, forced, PROMPT, fork_from=other)
    assert len(prefill_calls) == n_layer * chunks   # one more forward

    e_old = (old - want).abs().max().item()
    e_chunked = (chunked - want).abs().max().item()
    e_old_tail = (old[SHARED:] - want[SHARED:]).abs().max().item()
    e_shared = (shared - want[SHARED:]).abs().max().item()
    print(f"{family}: e_old={e_old:.4g} e_chunked={e_chunked:.4g} "
          f"e_old(tokens {SHARED}..)={e_old_tail:.4g} e_shared={e_shared:.4g}")
    assert torch.isfinite(chunked).all() and torch.isfinite(shared).all()
    assert e_chunked <= 2 * e_old, (e_chunked, e_old)
    assert e_shared <= 2 * e_old, (e_shared, e_old)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_paged_decoder_chunked_graph_matches_eager(family):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    torch.manual_seed(195)
    model = _build(family).to("cuda", torch.bfloat16)
    system = torch.randint(0, 256, (37,), device="cuda")
    prompts = [torch.cat([system, torch.randint(0, 256, (n,), device="cuda")])
               for n in (8, 3, 1)]
    new = 8
    need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
    ref = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN, use_graph=False,
                       prefill_chunk=CHUNK).generate(prompts, new)
    dec = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN,
                       prefill_chunk=CHUNK)
    out = dec.generate(prompts, new)
    assert dec._graph is not None, "hipGraph capture failed"
    assert dec.cache.n_free_pages == need
    for a, b in zip(out, ref):
        assert a.shape == (new,) and torch.equal(a, b), (out, ref)
    # with shared prefix pages the captured step replays over table rows
    # that name the same pages; everything is returned afterwards
    again = dec.generate(prompts, new, share_prefix=True)
    assert dec.cache.n_free_pages == need and not any(dec.cache.refcount)
    assert all(a.shape == (new,) for a in again)
