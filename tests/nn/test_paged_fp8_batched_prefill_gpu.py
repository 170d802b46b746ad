"""Ragged batched prefill over the fp8 paged cache on the GPU, both families,
bf16 models, the setting of tests/nn/test_paged_batched_prefill_gpu.py.

Oracle: the fp32 CPU twin, every prompt prefilled alone.  ``e_old`` is the
error of the fp8 path that exists without this feature (every prompt alone
over the fp8 cache), ``e_new`` that of the three prompts as one packed forward
and, separately, in rounds of 16, each through one ``paged_varlen_attn_fp8``
launch per layer and round; the project's rule is e_new <= 2 * e_old."""
import functools

import pytest
import torch

from tests.nn.test_paged_batched_prefill_cpu import LENGTHS, run_prompts
from tests.nn.test_paged_decode_gpu import _build, _count, _fp32_cpu_copy
from tests.nn.test_paged_prefill_cpu import CHUNK, MAX_LEN, N_STEPS, PAGE

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_packed_prefill_over_fp8_cache(family, monkeypatch):
    torch.manual_seed(296)
    model = _build(family).to("cuda", torch.bfloat16)
    n_layer = model.config.n_layer
    oracle = _fp32_cpu_copy(model, family)
    g = torch.Generator().manual_seed(297)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    forced = torch.randint(0, 256, (len(prompts), N_STEPS), generator=g)
    want = run_prompts(oracle, prompts, forced)

    monkeypatch.setattr(model, "new_paged_kv_cache", functools.partial(
        model.new_paged_kv_cache, kv_dtype=FP8))
    e_old = (run_prompts(model, prompts, forced) - want).abs().max().item()
    varlen_calls = _count(monkeypatch, "paged_varlen_attn_fp8")
    prefill_calls = _count(monkeypatch, "paged_prefill_attn_fp8")
    for chunk, rounds in ((max(LENGTHS), 1), (CHUNK, 3)):
        new = run_prompts(model, prompts, forced, chunk)
        assert len(varlen_calls) == n_layer * rounds and not prefill_calls, \
            f"{len(varlen_calls)} fp8 varlen kernel calls in {rounds} rounds"
        del varlen_calls[:]
        e_new = (new - want).abs().max().item()
        print(f"{family}: rounds of {chunk}: e_old={e_old:.4g} "
              f"e_new={e_new:.4g}")
        assert torch.isfinite(new).all()
        assert e_new <= 2 * e_old, (chunk, e_new, e_old)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_paged_decoder_fp8_batched_prefill_graph_matches_eager(family):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    torch.manual_seed(298)
    model = _build(family).to("cuda", torch.bfloat16)
    system = torch.randint(0, 256, (37,), device="cuda")
    prompts = [torch.cat([system, torch.randint(0, 256, (n,), device="cuda")])
               for n in (8, 3, 1)]
    new = 8
    need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
    args = (model, 3, need + 1, PAGE, MAX_LEN)
    kw = dict(kv_dtype=FP8, prefill_chunk=CHUNK, batched_prefill=True)
    ref = PagedDecoder(*args, use_graph=False, **kw).generate(prompts, new)
    dec = PagedDecoder(*args, **kw)
    out = dec.generate(prompts, new)
    assert dec._graph is not None, "hipGraph capture failed"
    assert dec.cache.n_free_pages == need
    for a, b in zip(out, ref):
        assert a.shape == (new,) and torch.equal(a, b), (out, ref)
    again = dec.generate(prompts, new, share_prefix=True)
    assert dec.cache.n_free_pages == need and not any(dec.cache.refcount)
    assert all(a.shape == (new,) for a in again)
