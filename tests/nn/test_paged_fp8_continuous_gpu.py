"""``PagedDecoder.generate_continuous`` over an fp8 cache on the GPU, both
families: tests/nn/test_paged_continuous_gpu.py with
``kv_dtype=torch.float8_e4m3fn``.  Every step is one packed forward whose
attention is the fp8 split-KV ragged kernel
(csrc/paged_fp8_varlen_split_attention.hip), decode rows included.  As there,
no token-for-token equality: a prompt no longer than the chunk is one pure
prefill piece in both runs, and its first token must agree."""
import pytest
import torch

from tests.nn.test_paged_continuous_cpu import (BUDGET, CHUNK, LENGTHS,
                                                MAX_SEQS, NEW, count_steps)
from tests.nn.test_paged_decode_gpu import _build, _count
from tests.nn.test_paged_prefill_cpu import MAX_LEN, PAGE

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_continuous_batching_fp8(family, monkeypatch):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    torch.manual_seed(212)
    model = _build(family).to("cuda", torch.bfloat16)
    g = torch.Generator().manual_seed(211)
    prompts = [torch.randint(0, 256, (n,), generator=g).cuda()
               for n in LENGTHS]
    need = sum(-(-(n + NEW) // PAGE) for n in LENGTHS)
    want = PagedDecoder(model, len(LENGTHS), need + 1, PAGE, MAX_LEN,
                        use_graph=False, prefill_chunk=CHUNK,
                        batched_prefill=True, kv_dtype=FP8
                        ).generate(prompts, NEW)

    split_calls = _count(monkeypatch, "paged_varlen_split_attn_fp8")
    other = [_count(monkeypatch, name)
             for name in ("paged_varlen_attn_fp8", "paged_decode_attn_fp8",
                          "paged_decode_attn", "paged_varlen_split_attn")]
    dec = PagedDecoder(model, MAX_SEQS, need + 1, PAGE, MAX_LEN,
                       prefill_chunk=CHUNK, kv_dtype=FP8)
    out = dec.generate_continuous(prompts, NEW, token_budget=BUDGET)
    steps = count_steps(LENGTHS, MAX_SEQS, CHUNK, BUDGET, NEW)
    assert len(split_calls) == model.config.n_layer * steps and \
        not any(other), (len(split_calls), steps, [len(c) for c in other])
    for n, a, b in zip(LENGTHS, out, want):
        assert a.shape == (NEW,) and a.dtype == torch.long
        if n <= CHUNK:
            assert a[0] == b[0], (n, a, b)
    cache = dec.cache
    assert cache.kv_dtype == FP8
    assert cache.n_free_pages == need and not any(cache.filled)
    assert not any(cache.refcount) and not cache.pos_t.any()
