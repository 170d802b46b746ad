"""Chunked prefill and prefix sharing through PagedKVCache on the CPU (fp32,
both families, the tiny configs of tests/nn/test_paged_decode_gpu.py).

A prompt of 45 tokens in chunks of 16 (pages of 16: the chunks end on page
edges, the last is ragged), then 6 forced decode steps, against the same
prompt prefilled whole.  atol 1e-5: logits are O(1); fp32 with two layers and
hidden <= 256 leaves GEMM-shape-dependent summation order at about 1e-6,
while a wrong position, page or causal edge moves logits by O(0.1).
"""
import dataclasses

import pytest
import torch

from pipegoose_amd.models.kv_cache import PagedKVCache
from pipegoose_amd.testing.utils import spawn

PROMPT, CHUNK, N_STEPS, PAGE, MAX_LEN = 45, 16, 6, 16, 64
ATOL = 1e-5


def _model(family, ctx):
    torch.manual_seed(170)
    if family == "bloom":
        from pipegoose_amd.models.bloom import BloomConfig, BloomForCausalLM
        cfg = BloomConfig(vocab_size=256, hidden_size=128, n_layer=2,
                          n_head=2)
        return BloomForCausalLM(cfg, ctx).eval()
    from pipegoose_amd.models.llama import LlamaForCausalLM, llama_tiny
    cfg = dataclasses.replace(llama_tiny(), hidden_size=256,
                              intermediate_size=512, n_head=4, n_kv_head=2)
    return LlamaForCausalLM(cfg, ctx).eval()


def _prefill_and_decode(model, cache, slot, prompt, forced, chunk, done=0):
    """Logits of the prompt's last token and of the forced decode steps,
    [1 + N_STEPS, V]; tokens ``done..`` are run, in pieces of ``chunk``."""
    rows = cache.rows(slot, slot + 1)
    for lo in range(done, prompt.numel(), chunk):
        piece = prompt[lo:lo + chunk]
        logits, _ = model(piece[None], past=rows, use_cache=True)
        rows.advance(piece.numel())
    out = [logits[0, -1]]
    for t in range(N_STEPS):
        logits, _ = model(forced[None, t:t + 1], past=rows, use_cache=True)
        rows.advance(1)
        out.append(logits[0, -1])
    return torch.stack(out)


def _run_chunked(rank, world_size, port):
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    g = torch.Generator().manual_seed(171)
    prompt = torch.randint(0, 256, (PROMPT,), generator=g)
    forced = torch.randint(0, 256, (N_STEPS,), generator=g)
    with torch.no_grad():
        for family in ("bloom", "llama"):
            model = _model(family, ctx)
            cache = model.new_paged_kv_cache(2, 9, PAGE, MAX_LEN)
            for slot in (0, 1):
                cache.allocate(slot, PROMPT + N_STEPS)
            whole = _prefill_and_decode(model, cache, 0, prompt, forced,
                                        PROMPT)
            pieces = _prefill_and_decode(model, cache, 1, prompt, forced,
                                         CHUNK)
            err = (pieces - whole).abs().max().item()
            print(f"{family}: chunked vs whole prefill, max |dlogit| = "
                  f"{err:.3g}")
            assert torch.isfinite(pieces).all()
            assert err <= ATOL, (family, err)
            assert cache.filled == [PROMPT + N_STEPS] * 2

            # a chunk that would run past the slot's pages is refused on
            # the host
            cache.free(1)
            cache.allocate(1, 20)
            rows = cache.rows(1, 2)
            model(prompt[None, :20], past=rows, use_cache=True)
            rows.advance(20)
            with pytest.raises(AssertionError, match="runs past the pages"):
                model(prompt[None, 20:40], past=rows, use_cache=True)
    ctx.destroy()


def test_chunked_prefill_matches_whole_prompt():
    spawn(_run_chunked, world_size=1)


def _cache():
    return PagedKVCache(n_layers=1, max_seqs=3, n_pages=12, page_size=PAGE,
                        max_len=MAX_LEN, Hkv=1, D=16, dtype=torch.float32,
                        device="cpu")


def test_fork_shares_whole_pages():
    cache = _cache()
    cache.allocate(0, 45)                       # 3 pages
    cache.rows(0, 1).advance(45)
    src_pages = list(cache.pages[0])
    assert cache.n_free_pages == 8
    assert cache.fork(0, 1, 40) == 32           # whole pages only
    assert cache.n_free_pages == 8              # sharing takes no page
    assert cache.pages[1] == src_pages[:2]
    assert [cache.refcount[p] for p in src_pages] == [2, 2, 1]
    assert cache.filled[1] == 32 and cache.pos_t[1].item() == 32
    assert cache.block_table[1].tolist() == src_pages[:2] + [0, 0]
    assert torch.equal(cache.block_table, cache.table_host)
    cache.allocate(1, 50)                       # fresh pages AFTER the shared
    assert cache.n_free_pages == 6
    assert cache.pages[1][:2] == src_pages[:2]
    fresh = cache.pages[1][2:]
    assert len(fresh) == 2 and not set(fresh) & set(src_pages)
    assert cache.block_table[1].tolist() == cache.pages[1]
    assert [cache.refcount[p] for p in fresh] == [1, 1]

    # a third holder, then free in either order
    assert cache.fork(1, 2, 16) == 16
    assert cache.refcount[src_pages[0]] == 3
    cache.free(0)                               # the source first
    assert cache.n_free_pages == 7              # only its unshared page
    assert [cache.refcount[p] for p in src_pages] == [2, 1, 0]
    assert cache.pages[1][:2] == src_pages[:2]  # the fork still holds them
    assert cache.block_table[1].tolist() == cache.pages[1]
    assert not cache.block_table[0].any() and cache.filled[0] == 0
    cache.free(2)
    assert cache.n_free_pages == 7 and cache.refcount[src_pages[0]] == 1
    cache.free(1)
    assert cache.n_free_pages == 11
    assert not any(cache.refcount) and not cache.block_table.any()
    assert sorted(cache._free) == list(range(1, 12))    # each page once

    cache.allocate(0, 45)
    cache.rows(0, 1).advance(45)
    cache.fork(0, 1, 45)
    cache.free(1)                               # the fork first
    assert cache.n_free_pages == 8
    assert [cache.refcount[p] for p in cache.pages[0]] == [1, 1, 1]
    cache.free(0)
    assert cache.n_free_pages == 11


def test_fork_refusals_and_unforked_behaviour():
    cache = _cache()
    cache.allocate(0, 45)
    cache.rows(0, 1).advance(45)
    cache.allocate(1, 5)
    with pytest.raises(AssertionError, match="empty slot"):
        cache.fork(0, 1, 32)                    # owns a page
    cache.rows(1, 2).advance(5)
    with pytest.raises(AssertionError, match="empty slot"):
        cache.fork(0, 1, 32)                    # holds tokens
    with pytest.raises(AssertionError, match="holds 45"):
        cache.fork(0, 2, 46)                    # more than the source has
    with pytest.raises(AssertionError):
        cache.fork(0, 0, 16)
    assert cache.fork(0, 2, 15) == 0            # less than a page: nothing
    assert cache.pages[2] == [] and cache.filled[2] == 0
    assert cache.n_free_pages == 7
    # without fork, pages come and go as before: lowest id first, and a
    # freed slot's pages are handed out again in the same order
    fresh = _cache()
    fresh.allocate(0, 33)
    assert fresh.pages[0] == [1, 2, 3]
    fresh.free(0)
    fresh.allocate(1, 33)
    assert fresh.pages[1] == [1, 2, 3] and fresh.n_free_pages == 8


def _run_share_prefix(rank, world_size, port):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    g = torch.Generator().manual_seed(172)
    system = torch.randint(0, 256, (37,), generator=g)  # 2 whole pages + 5
    prompts = [torch.cat([system, torch.randint(0, 256, (n,), generator=g)])
               for n in (8, 3)]
    forced = torch.randint(0, 256, (N_STEPS,), generator=g)
    new = 5
    with torch.no_grad():
        for family in ("bloom", "llama"):
            model = _model(family, ctx)
            # logits: the second prompt behind the forked pages of the
            # first against the same prompt prefilled whole
            cache = model.new_paged_kv_cache(3, 12, PAGE, MAX_LEN)
            cache.allocate(0, prompts[0].numel())
            rows = cache.rows(0, 1)
            model(prompts[0][None], past=rows, use_cache=True)
            rows.advance(prompts[0].numel())
            cache.allocate(1, prompts[1].numel() + N_STEPS)
            whole = _prefill_and_decode(model, cache, 1, prompts[1], forced,
                                        PROMPT)
            free_before = cache.n_free_pages
            assert cache.fork(0, 2, 37) == 32
            cache.allocate(2, prompts[1].numel() + N_STEPS)
            assert free_before - cache.n_free_pages == 1    # not 3
            shared = _prefill_and_decode(model, cache, 2, prompts[1], forced,
                                         PROMPT, done=32)
            err = (shared - whole).abs().max().item()
            print(f"{family}: shared-prefix vs whole prefill, max |dlogit| "
                  f"= {err:.3g}")
            assert torch.isfinite(shared).all()
            assert err <= ATOL, (family, err)

            # PagedDecoder: same tokens, fewer pages
            need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
            used = {}
            for share in (False, True):
                dec = PagedDecoder(model, max_seqs=2, n_pages=need + 1,
                                   page_size=PAGE, max_len=MAX_LEN,
                                   use_graph=False, prefill_chunk=CHUNK)
                low = []
                real = dec.cache.allocate

                def allocate(slot, n_tokens, real=real, dec=dec, low=low):
                    real(slot, n_tokens)
                    low.append(dec.cache.n_free_pages)

                dec.cache.allocate = allocate
                out = dec.generate(prompts, new, share_prefix=share)
                used[share] = (out, need - min(low))
                assert dec.cache.n_free_pages == need       # all pages back
                assert not any(dec.cache.refcount)
                assert not dec.cache.block_table.any()
            assert used[False][1] == need
            assert used[True][1] == need - 2    # two whole pages shared
            for a, b in zip(used[True][0], used[False][0]):
                assert a.shape == (new,) and torch.equal(a, b), family
            # a pool two pages short serves the run only when shared
            small = PagedDecoder(model, max_seqs=2, n_pages=need - 1,
                                 page_size=PAGE, max_len=MAX_LEN,
                                 use_graph=False)
            out = small.generate(prompts, new, share_prefix=True)
            for a, b in zip(out, used[False][0]):
                assert torch.equal(a, b), family
            with pytest.raises(RuntimeError, match="out of pages"):
                small.generate(prompts, new)
            assert small.cache.n_free_pages == need - 2
    ctx.destroy()


def test_share_prefix_matches_unshared_on_fewer_pages():
    spawn(_run_share_prefix, world_size=1)
