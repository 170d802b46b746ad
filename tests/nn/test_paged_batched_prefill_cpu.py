"""Ragged batched prefill through ``PagedKVCache.packed`` on the CPU (fp32,
both families): prompts of 45, 8 and 1 tokens as ONE packed forward and in
rounds of 16, then forced decode steps, against every prompt prefilled alone.
Configs and tolerance (atol 1e-5) are those of
tests/nn/test_paged_prefill_cpu.py."""
import pytest
import torch

from pipegoose_amd.testing.utils import spawn
from tests.nn.test_paged_prefill_cpu import (ATOL, CHUNK, MAX_LEN, N_STEPS,
                                             PAGE, _model)

LENGTHS = (45, 8, 1)


@torch.no_grad()
def run_prompts(model, prompts, forced, chunk=None):
    """Logits of every prompt token, prompt by prompt, then of N_STEPS forced
    decode steps over all prompts.  ``chunk=None``: each prompt alone, whole;
    else packed forwards of up to ``chunk`` tokens of every unfinished one."""
    dev = next(model.parameters()).device
    n = len(prompts)
    need = sum(-(-(p.numel() + N_STEPS) // PAGE) for p in prompts)
    cache = model.new_paged_kv_cache(n, need + 1, PAGE, MAX_LEN)
    for i, p in enumerate(prompts):
        cache.allocate(i, p.numel() + N_STEPS)
    out, done = [[] for _ in prompts], [0] * n
    while min(d - p.numel() for d, p in zip(done, prompts)) < 0:
        slots = [i for i in range(n) if done[i] < prompts[i].numel()]
        slots = slots if chunk else slots[:1]
        lens = [min(chunk or MAX_LEN, prompts[i].numel() - done[i])
                for i in slots]
        rows = cache.packed(slots, lens) if chunk \
            else cache.rows(slots[0], slots[0] + 1)
        ids = torch.cat([prompts[i][done[i]:done[i] + m]
                         for i, m in zip(slots, lens)])
        logits, _ = model(ids[None].to(dev), past=rows, use_cache=True)
        rows.advance() if chunk else rows.advance(lens[0])
        for i, piece in zip(slots, logits[0].float().cpu().split(lens)):
            out[i].append(piece)
            done[i] += piece.size(0)
    rows = cache.rows(0, n)
    for t in range(N_STEPS):
        logits, _ = model(forced[:, t:t + 1].to(dev), past=rows,
                          use_cache=True)
        rows.advance(1)
        out.append([logits[:, -1].float().cpu()])
    assert cache.pos_t.tolist() == cache.filled == [
        p.numel() + N_STEPS for p in prompts]
    return torch.cat([piece for pieces in out for piece in pieces])


def _run(rank, world_size, port):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    g = torch.Generator().manual_seed(173)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    forced = torch.randint(0, 256, (len(prompts), N_STEPS), generator=g)
    system = torch.randint(0, 256, (37,), generator=g)
    related = [torch.cat([system, torch.randint(0, 256, (n,), generator=g)])
               for n in (8, 3, 1)]
    new = 5
    need = sum(-(-(p.numel() + new) // PAGE) for p in related)
    for family in ("bloom", "llama"):
        model = _model(family, ctx)
        alone = run_prompts(model, prompts, forced)
        for chunk in (max(LENGTHS), CHUNK):
            packed = run_prompts(model, prompts, forced, chunk)
            err = (packed - alone).abs().max().item()
            print(f"{family}: rounds of {chunk}: max |dlogit| = {err:.3g}")
            assert torch.isfinite(packed).all() and err <= ATOL, (chunk, err)
        # a packed forward that would run past a slot's pages is refused
        cache = model.new_paged_kv_cache(2, 5, PAGE, MAX_LEN)
        cache.allocate(0, 16)
        with pytest.raises(AssertionError, match="runs past the pages"):
            cache.packed([0], [17])

        args = (model, 3, need + 1, PAGE, MAX_LEN)
        want = PagedDecoder(*args, use_graph=False).generate(related, new)
        for chunk in (None, CHUNK):
            dec = PagedDecoder(*args, use_graph=False, prefill_chunk=chunk,
                               batched_prefill=True)
            for share in (False, True):
                out = dec.generate(related, new, share_prefix=share)
                assert all(map(torch.equal, out, want)), (chunk, share)
                assert dec.cache.n_free_pages == need    # all pages back
                assert not any(dec.cache.refcount)
        with pytest.raises(NotImplementedError, match="batched_prefill"):
            PagedDecoder(*args, kv_dtype=torch.float8_e4m3fn,
                         batched_prefill=True)
    ctx.destroy()


def test_batched_prefill_matches_per_prompt_prefill():
    spawn(_run, world_size=1)
