"""``PagedDecoder.generate_continuous`` on the CPU, both families: 5 ragged
prompts through 2 slots, pieces of 4, 5 tokens per forward and a pool that
holds the longest prompt plus one more, against ``generate`` with a slot per
prompt.  The models run in fp64 (both families do), where regrouping the
batch moves a logit by ~1e-15 and cannot move an argmax: the tokens must be
equal."""
import pytest
import torch

from pipegoose_amd.testing.utils import spawn
from tests.nn.test_paged_prefill_cpu import MAX_LEN, PAGE, _model

LENGTHS, MAX_SEQS, CHUNK, BUDGET, NEW = (1, 20, 7, 13, 4), 2, 4, 5, 6


def count_steps(lengths, max_seqs, chunk, budget, new):
    """Forwards ``generate_continuous`` runs when pages never run short."""
    waiting, flight, steps = list(lengths), [], 0
    while waiting or flight:
        while waiting and len(flight) < max_seqs:
            flight.append([waiting.pop(0), 0])      # prompt left, tokens held
        sampled = [s for s in flight if s[0] == 0]
        room = budget - len(sampled)
        for s in flight:
            if s[0] and room:
                k = min(s[0], chunk, room)
                s[0], room = s[0] - k, room - k
                if s[0] == 0:
                    sampled.append(s)
        for s in sampled:
            s[1] += 1
        flight = [s for s in flight if s[1] < new]
        steps += 1
    return steps


def _run(rank, world_size, port):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    g = torch.Generator().manual_seed(211)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    need = sum(-(-(n + NEW) // PAGE) for n in LENGTHS)
    for family in ("bloom", "llama"):
        model = _model(family, ctx).double()
        want = PagedDecoder(model, len(LENGTHS), need + 1, PAGE, MAX_LEN,
                            use_graph=False).generate(prompts, NEW)
        dec = PagedDecoder(model, MAX_SEQS, 4, PAGE, MAX_LEN, use_graph=False,
                           prefill_chunk=CHUNK)
        forwards = []
        hook = model.register_forward_pre_hook(
            lambda *_: forwards.append(1))
        out = dec.generate_continuous(prompts, NEW, token_budget=BUDGET)
        assert len(forwards) >= count_steps(LENGTHS, MAX_SEQS, CHUNK, BUDGET,
                                            NEW)        # pages can only delay
        for a, b in zip(out, want):
            assert a.shape == (NEW,) and torch.equal(a, b), (family, out, want)
        cache = dec.cache
        assert cache.n_free_pages == 3 and not any(cache.refcount)
        assert not any(cache.filled) and not cache.pos_t.any()

        # a prompt that can never fit raises before any forward
        del forwards[:]
        long = torch.zeros(MAX_LEN - NEW + 1, dtype=torch.long)
        with pytest.raises(RuntimeError, match="exceed max_len"):
            dec.generate_continuous([prompts[0], long], NEW)
        with pytest.raises(RuntimeError, match="out of pages"):
            dec.generate_continuous([prompts[0], long[:3 * PAGE]], NEW)
        assert not forwards and cache.n_free_pages == 3
        hook.remove()
    ctx.destroy()


def test_continuous_batching_matches_generate():
    spawn(_run, world_size=1)
