"""Decode over the fp8 paged cache, both model families, bf16 models, the tiny
configs, prompts and steps of tests/nn/test_paged_decode_gpu.py.

Oracle: the fp32 CPU twin, each prompt alone, teacher-forced.  ``e_bf16`` is
the max abs logit error of the bf16 paged cache, ``e_fp8`` that of
``PagedDecoder(kv_dtype=torch.float8_e4m3fn)``'s cache in the same test.  An
e4m3 element carries 2^-4 relative error against bf16's 2^-8; 16 is that
ratio propagated linearly, a ceiling: e_fp8 <= 16 * e_bf16.
"""
import pytest
import torch

from pipegoose_amd.models.paged_decode import PagedDecoder
from pipegoose_amd.ops.paged_attention import paged_fp8_kernel_supported
from tests.nn.test_paged_decode_gpu import (LENGTHS, MAX_LEN, N_STEPS, PAGE,
                                            _alone, _build, _fp32_cpu_copy)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


@torch.no_grad()
def _paged(model, prompts, forced, kv_dtype, chunk=None, share=False):
    """[steps, n, V]: the ragged batch through a PagedDecoder's cache,
    prefilled as ``generate`` does it, then teacher-forced."""
    n = len(prompts)
    need = sum(-(-(p.numel() + N_STEPS) // PAGE) for p in prompts)
    dec = PagedDecoder(model, n, need + 1, PAGE, MAX_LEN, use_graph=False,
                       prefill_chunk=chunk, kv_dtype=kv_dtype)
    cache = dec.cache
    if kv_dtype == FP8:     # the steps below run the fp8 kernels
        view = cache.rows(0, n)[0]
        assert view.k_pool.dtype == FP8 and view.v_scale is not None
        assert paged_fp8_kernel_supported(
            torch.empty(n, 1, 1, view.k_pool.size(-1), device="cuda",
                        dtype=torch.bfloat16), view.k_pool)
    shared = dec._shared_prefixes(prompts) if share else [(None, 0)] * n
    for i, prompt in enumerate(prompts):
        if shared[i][1]:
            cache.fork(shared[i][0], i, shared[i][1])
        cache.allocate(i, prompt.numel() + N_STEPS)
        dec._prefill(i, prompt, done=shared[i][1])
    rows = cache.rows(0, n)
    steps = []
    for t in range(N_STEPS):
        logits, _ = model(forced[:, t:t + 1].cuda(), past=rows,
                          use_cache=True)
        rows.advance(1)
        steps.append(logits[:, -1].float().cpu())
    return torch.stack(steps), shared


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    prompts[2][:LENGTHS[1]] = prompts[1]        # one whole page in common
    return prompts, torch.randint(0, 256, (len(LENGTHS), N_STEPS),
                                  generator=g)


@pytest.mark.parametrize("family", ["bloom", "llama"])
@pytest.mark.parametrize("chunk,share", [(None, False), (8, True)])
def test_logit_error_against_fp32(family, chunk, share):
    torch.manual_seed(97)
    model = _build(family).to("cuda", torch.bfloat16)
    prompts, forced = _inputs(98)
    want = _alone(_fp32_cpu_copy(model, family), prompts, forced)
    bf16, _ = _paged(model, prompts, forced, None, chunk, share)
    fp8, shared = _paged(model, prompts, forced, FP8, chunk, share)
    assert not share or shared[2] == (1, PAGE)
    e_bf16 = (bf16 - want).abs().max().item()
    e_fp8 = (fp8 - want).abs().max().item()
    print(f"{family} chunk={chunk} share={share}: e_bf16={e_bf16:.4g} "
          f"e_fp8={e_fp8:.4g}")
    assert torch.isfinite(fp8).all()
    assert e_fp8 <= 16 * e_bf16, (e_fp8, e_bf16)


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_captured_step_returns_the_eager_tokens(family):
    torch.manual_seed(99)
    model = _build(family).to("cuda", torch.bfloat16)
    prompts = [torch.randint(0, 256, (n,), device="cuda") for n in LENGTHS]
    new = 12
    need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
    ref = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN, use_graph=False,
                       kv_dtype=FP8).generate(prompts, new)
    dec = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN, kv_dtype=FP8)
    assert dec.cache.k_pools[0].dtype == FP8
    for _ in range(2):          # the second call replays the captured step
        out = dec.generate(prompts, new)
        assert dec._graph is not None, "hipGraph capture failed"
        for a, b in zip(out, ref):
            assert a.shape == (new,) and torch.equal(a, b), (out, ref)
