"""Sampled decoding on the CPU path, both families: ``top_k=1`` is greedy, and
per-prompt parameter lists leave a greedy prompt's tokens what they were."""
import torch

from pipegoose_amd.testing.utils import spawn
from tests.nn.test_paged_prefill_cpu import MAX_LEN, PAGE, _model

LENGTHS, NEW = (5, 16, 23), 6


def _run(rank, world_size, port):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    from pipegoose_amd.testing.utils import init_parallel_context
    ctx = init_parallel_context(rank, world_size, port)
    g = torch.Generator().manual_seed(311)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    need = sum(-(-(n + NEW) // PAGE) for n in LENGTHS)
    for family in ("bloom", "llama"):
        dec = PagedDecoder(_model(family, ctx), 3, need + 1, PAGE, MAX_LEN,
                           use_graph=False)
        greedy = dec.generate(prompts, NEW)
        runs = {
            "top_k=1": dec.generate(prompts, NEW, temperature=0.8, top_k=1),
            "continuous": dec.generate_continuous(prompts, NEW,
                                                  temperature=0.8, top_k=1),
        }
        for name, out in runs.items():
            for a, b in zip(out, greedy):
                assert torch.equal(a, b), (family, name, out, greedy)
        mixed = dec.generate(prompts, NEW, temperature=[0.9, 0.0, 1.1],
                             top_k=[20, 0, 0], top_p=[1.0, 1.0, 0.9],
                             generator=torch.Generator().manual_seed(5))
        assert torch.equal(mixed[1], greedy[1]), (family, mixed, greedy)
        assert all(m.shape == (NEW,) for m in mixed)
    ctx.destroy()


def test_top_k_1_is_greedy_and_per_prompt_parameters():
    spawn(_run, world_size=1)
