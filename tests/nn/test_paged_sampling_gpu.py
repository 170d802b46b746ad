"""Sampled decoding through the HIP sampler on the GPU, both families, the tiny
bf16 configs of tests/nn/test_paged_decode_gpu.py."""
import pytest
import torch

from pipegoose_amd.models.graph_decode import GraphDecoder
from pipegoose_amd.models.paged_decode import PagedDecoder
from tests.nn.test_paged_decode_gpu import LENGTHS, MAX_LEN, PAGE, _build
from tests.ops._sample_refs import reference

pytestmark = pytest.mark.gpu

NEW = 12
NEED = sum(-(-(n + NEW) // PAGE) for n in LENGTHS)


@pytest.fixture(scope="module", params=["bloom", "llama"])
def setup(request):
    torch.manual_seed(401)
    model = _build(request.param).to("cuda", torch.bfloat16)
    prompts = [torch.randint(0, 256, (n,), device="cuda") for n in LENGTHS]
    return model, prompts


def _decoder(model, **kwargs):
    return PagedDecoder(model, 3, NEED + 1, PAGE, MAX_LEN, **kwargs)


def _seeded():
    return torch.Generator(device="cuda").manual_seed(7)


def _same(outs, wants):
    return all(torch.equal(a, b) for a, b in zip(outs, wants))


def test_graph_and_eager_draw_the_same_tokens(setup):
    model, prompts = setup
    args = dict(temperature=0.8, top_k=20, top_p=0.9)
    ref = _decoder(model, use_graph=False).generate(
        prompts, NEW, generator=_seeded(), **args)
    dec = _decoder(model)
    out = dec.generate(prompts, NEW, generator=_seeded(), **args)
    assert dec._graph is not None, "hipGraph capture failed"
    assert _same(out, ref), (out, ref)
    # the captured step serves other parameters without a new capture
    graphs = dict(dec._graphs)
    dec.generate(prompts, NEW, temperature=1.2, top_k=0, top_p=0.5)
    assert dec._graphs == graphs


@pytest.mark.parametrize("batched", [False, True])
def test_top_k_1_and_greedy_rows_are_greedy(setup, batched):
    model, prompts = setup
    dec = _decoder(model, batched_prefill=batched)
    greedy = dec.generate(prompts, NEW)
    assert _same(dec.generate(prompts, NEW, temperature=0.8, top_k=1), greedy)
    assert _same(dec.generate_continuous(prompts, NEW, temperature=0.8,
                                         top_k=1), greedy)
    mixed = dec.generate(prompts, NEW, temperature=[0.9, 0.0, 1.1],
                         top_k=[20, 0, 0], top_p=[1.0, 1.0, 0.9])
    assert torch.equal(mixed[1], greedy[1]), (mixed, greedy)


def test_graph_decoder_and_model_generate(setup):
    model, prompts = setup
    ids = torch.stack([p[:5] for p in prompts])
    dec = GraphDecoder(model, batch_size=3, max_len=MAX_LEN)
    greedy = dec.generate(ids, NEW)
    assert torch.equal(dec.generate(ids, NEW, temperature=0.8, top_k=1),
                       greedy)
    out = model.generate(ids, max_new_tokens=NEW, temperature=0.8, top_p=0.9)
    assert out.shape == (3, 5 + NEW) and torch.equal(out[:, :5], ids)
    with torch.no_grad():
        logits = model(ids)[:, -1].cpu()
    for row, token in zip(logits, out[:, 5].tolist()):
        assert reference(row, 0.8, 0, 0.9)[0][token], token
