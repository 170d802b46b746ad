"""Chunked prefill with prefix sharing over the fp8 paged cache runs the fp8
prefill kernel (csrc/paged_fp8_prefill_attention.hip) in both model families:
the setting, oracle and ceiling ``e_fp8 <= 16 * e_bf16`` of
tests/nn/test_paged_fp8_decode_gpu.py, with the kernel's calls counted.
"""
import pytest
import torch

from tests.nn.test_paged_decode_gpu import (_alone, _build, _count,
                                            _fp32_cpu_copy)
from tests.nn.test_paged_fp8_decode_gpu import FP8, _inputs, _paged

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", ["bloom", "llama"])
def test_chunked_shared_prefill_runs_the_fp8_kernel(family, monkeypatch):
    torch.manual_seed(97)
    model = _build(family).to("cuda", torch.bfloat16)
    prompts, forced = _inputs(98)
    want = _alone(_fp32_cpu_copy(model, family), prompts, forced)
    bf16, _ = _paged(model, prompts, forced, None, chunk=8, share=True)
    calls = _count(monkeypatch, "paged_prefill_attn_fp8")
    fp8, _ = _paged(model, prompts, forced, FP8, chunk=8, share=True)
    assert len(calls) > 0 and len(calls) % model.config.n_layer == 0, \
        f"{len(calls)} fp8 prefill kernel calls"
    e_bf16 = (bf16 - want).abs().max().item()
    e_fp8 = (fp8 - want).abs().max().item()
    print(f"{family}: e_bf16={e_bf16:.4g} e_fp8={e_fp8:.4g}")
    assert torch.isfinite(fp8).all()
    assert e_fp8 <= 16 * e_bf16, (e_fp8, e_bf16)
