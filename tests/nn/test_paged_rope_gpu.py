"""LLaMA over the paged cache with the fused rope + cache-write kernel
(csrc/paged_rope_write.hip): the config, prompts and method of
tests/nn/test_paged_decode_gpu.py.  ``e_unfused`` is the error of the same
run with ``PG_PAGED_ROPE=0`` (rope_at_position twice + paged_kv_write)
against the fp32 CPU twin; the project's rule is e_fused <= 2 * e_unfused."""
import pytest
import torch

from tests.nn.test_paged_decode_gpu import (LENGTHS, MAX_LEN, N_STEPS, PAGE,
                                            _alone, _build, _count,
                                            _fp32_cpu_copy, _paged)

pytestmark = pytest.mark.gpu


def test_decode_steps_use_the_fused_kernel(monkeypatch):
    torch.manual_seed(93)
    model = _build("llama").to("cuda", torch.bfloat16)
    oracle = _fp32_cpu_copy(model, "llama")
    g = torch.Generator().manual_seed(94)
    prompts = [torch.randint(0, 256, (n,), generator=g) for n in LENGTHS]
    forced = torch.randint(0, 256, (len(LENGTHS), N_STEPS), generator=g)
    want = _alone(oracle, prompts, forced)

    monkeypatch.setenv("PG_PAGED_ROPE", "0")
    e_unfused = (_paged(model, prompts, forced) - want).abs().max().item()
    monkeypatch.setenv("PG_PAGED_ROPE", "1")
    fused = _count(monkeypatch, "paged_rope_write")
    writes = _count(monkeypatch, "paged_kv_write")
    new = _paged(model, prompts, forced)
    # the prompts go into empty slots in one chunk each: apply_rope + write
    assert len(fused) == model.config.n_layer * N_STEPS
    assert len(writes) == model.config.n_layer * len(LENGTHS)

    e_fused = (new - want).abs().max().item()
    print(f"e_unfused={e_unfused:.4g} e_fused={e_fused:.4g}")
    assert torch.isfinite(new).all()
    assert e_fused <= 2 * e_unfused, (e_fused, e_unfused)


@pytest.mark.parametrize("kv_dtype", [None, torch.float8_e4m3fn])
def test_chunked_prefill_graph_matches_eager(kv_dtype, monkeypatch):
    from pipegoose_amd.models.paged_decode import PagedDecoder
    torch.manual_seed(95)
    model = _build("llama").to("cuda", torch.bfloat16)
    prompts = [torch.randint(0, 256, (n,), device="cuda") for n in LENGTHS]
    new = 12
    need = sum(-(-(p.numel() + new) // PAGE) for p in prompts)
    fused = _count(monkeypatch, "paged_rope_write_fp8" if kv_dtype
                   else "paged_rope_write")
    kwargs = dict(prefill_chunk=7, kv_dtype=kv_dtype)
    ref = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN, use_graph=False,
                       **kwargs).generate(prompts, new)
    assert fused                     # chunks behind a prefix and decode steps
    dec = PagedDecoder(model, 3, need + 1, PAGE, MAX_LEN, **kwargs)
    out = dec.generate(prompts, new)
    assert dec._graph is not None, "hipGraph capture failed"
    for a, b in zip(out, ref):
        assert a.shape == (new,) and torch.equal(a, b), (out, ref)
