"""Ragged decode through PagedKVCache on the CPU (fp32, tiny models, both
families) against each prompt run ALONE through new_kv_cache.

Prompts of 5, 16 and 23 tokens with 16-token pages: the first decode step of
the 16-token prompt opens a new page and the 23-token one crosses 32 within
the 10 steps.  atol 1e-4: logits are O(1); fp32 with two layers and hidden
<= 256 leaves batch-size-dependent GEMM ordering at about 1e-6, while a wrong
page or position moves logits by O(0.1).
"""
import dataclasses

from pipegoose_amd.testing.utils import spawn

LENGTHS, N_STEPS, PAGE = (5, 16, 23), 10, 16


def _model(family, ctx):
    import torch
    torch.manual_seed(70)
    if family == "bloom":
        from pipegoose_amd.models.bloom import BloomForCausalLM, bloom_tiny
        return BloomForCausalLM(bloom_tiny(), ctx).eval()
    from pipegoose_amd.models.llama import LlamaForCausalLM, llama_tiny
    cfg = dataclasses.replace(llama_tiny(), n_kv_head=2)      # GQA
    return LlamaForCausalLM(cfg, ctx).eval()


def _inputs():
    import torch
    g = torch.Generator().manual_seed(71)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    forced = torch.randint(0, 256, (len(LENGTHS), N_STEPS), generator=g)
    return prompts, forced


def _run_ragged_matches_alone(rank, world_size, port):
    import torch
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    prompts, forced = _inputs()
    n = len(prompts)
    with torch.no_grad():
        for family in ("bloom", "llama"):
            model = _model(family, ctx)
            # each prompt alone through the contiguous cache
            want = []
            for i, prompt in enumerate(prompts):
                past = model.new_kv_cache(1, 64)
                model(prompt[None], past=past, use_cache=True)
                steps = []
                for t in range(N_STEPS):
                    logits, _ = model(forced[i:i + 1, t:t + 1], past=past,
                                      use_cache=True)
                    steps.append(logits[0, -1])
                want.append(torch.stack(steps))
            want = torch.stack(want, dim=1)                  # [steps, n, V]

            # a pool for the tokens actually held (+ the null page), far
            # below max_seqs * max_len = 4 * 64 tokens = 16 pages
            need = sum(-(-(p.numel() + N_STEPS) // PAGE) for p in prompts)
            assert need + 1 < 4 * 64 // PAGE
            cache = model.new_paged_kv_cache(4, need + 1, PAGE, 64)
            for i, prompt in enumerate(prompts):
                cache.allocate(i, prompt.numel() + N_STEPS)
            assert cache.n_free_pages == 0
            for i, prompt in enumerate(prompts):
                rows = cache.rows(i, i + 1)
                model(prompt[None], past=rows, use_cache=True)
                rows.advance(prompt.numel())
            assert cache.pos_t.tolist() == list(LENGTHS) + [0]
            rows = cache.rows(0, n)
            got = []
            for t in range(N_STEPS):
                logits, _ = model(forced[:, t:t + 1], past=rows,
                                  use_cache=True)
                rows.advance(1)
                got.append(logits[:, -1])
            got = torch.stack(got)
            err = (got - want).abs().max().item()
            print(f"{family}: ragged paged vs alone, max |dlogit| = {err:.3g}")
            assert torch.isfinite(got).all()
            assert err <= 1e-4, (family, err)

            # a second prefill into a slot that holds tokens is refused
            try:
                model(prompts[0][None], past=cache.rows(0, 1), use_cache=True)
            except AssertionError as e:
                assert "empty" in str(e)
            else:
                raise AssertionError("prefill into a filled slot went through")
    ctx.destroy()


def test_ragged_paged_decode_matches_each_prompt_alone():
    spawn(_run_ragged_matches_alone, world_size=1)


def _run_paged_decoder(rank, world_size, port):
    import torch
    from pipegoose_amd.models.paged_decode import PagedDecoder
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    prompts, _ = _inputs()
    new = 7
    for family in ("bloom", "llama"):
        model = _model(family, ctx)
        need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
        dec = PagedDecoder(model, max_seqs=4, n_pages=need + 1,
                           page_size=PAGE, max_len=64, use_graph=False)
        outs = dec.generate(prompts, new)
        assert len(outs) == len(prompts)
        assert dec.cache.n_free_pages == need               # all pages back
        assert not dec.cache.block_table.any()
        assert dec.cache.pos_t.tolist() == [0] * 4
        for prompt, out in zip(prompts, outs):
            assert out.shape == (new,)
            # greedy, so it is model.generate() on that prompt alone
            alone = model.generate(prompt[None], max_new_tokens=new)
            assert torch.equal(out, alone[0, prompt.numel():]), family
        # a second call reuses the freed pages; a pool too small raises on
        # the host and leaves nothing allocated
        again = dec.generate(prompts[::-1], new)
        assert all(torch.equal(a, b) for a, b in zip(again, outs[::-1]))
        small = PagedDecoder(model, max_seqs=4, n_pages=need, page_size=PAGE,
                             max_len=64, use_graph=False)
        try:
            small.generate(prompts, new)
        except RuntimeError as e:
            assert "out of pages" in str(e)
        else:
            raise AssertionError("an exhausted pool did not raise")
        assert small.cache.n_free_pages == need - 1
    ctx.destroy()


def test_paged_decoder_generates_and_frees():
    spawn(_run_paged_decoder, world_size=1)
