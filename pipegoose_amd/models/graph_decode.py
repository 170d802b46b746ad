"""hipGraph-captured decode loop, greedy or sampled.

Decode at batch 8 is launch-bound (~8 ms/step on BLOOM-560M, ROADMAP.md §4):
hundreds of tiny kernel launches per step dwarf the actual compute.  A
hipGraph replays the whole step as ONE launch.  The requirements, and how
they are met here:

- constant shapes/addresses: ``GraphKVCache`` (models/kv_cache.py) — attention
  always runs over the full preallocated cache length, unfilled slots masked;
- no host values in the step: the write position is a device tensor
  (``pos_t``) advanced in-graph (`add_`); the ALiBi bias is computed from it
  (`BloomAttention._alibi_bias_graph`); token selection is an in-graph argmax,
  or the in-graph sampler (ops/sampling.py) reading its parameters and its
  uniforms from static device buffers, written back into the input buffer —
  the loop is fully self-advancing;
- every HIP kernel launches on the capture stream: all csrc bindings use
  ``at::cuda::getCurrentCUDAStream()``.

Beyond-reference capability (the reference had no decode path at all).
Falls back to eager static-cache stepping when capture is unavailable
(CPU, or ``use_graph=False``) — numerics are identical by construction and
tested (tests/nn/test_bloom_model.py, tests/ops/test_kernels_gpu.py).
"""
from typing import Optional

import torch

from pipegoose_amd.distributed.parallel_mode import ParallelMode


class GraphDecoder:
    """Decoder for a (tp=1) causal LM with ``new_graph_kv_cache``.

    Usage::

        dec = GraphDecoder(model, batch_size=8, max_len=512)
        out = dec.generate(prompt_ids, max_new_tokens=128)   # [B, 128]
        out = dec.generate(prompt_ids, 128, temperature=0.8, top_p=0.9)
    """

    def __init__(self, model, batch_size: int, max_len: int,
                 use_graph: Optional[bool] = None):
        ctx = getattr(model, "parallel_context", None)
        if ctx is not None and ctx.get_world_size(ParallelMode.TENSOR) > 1:
            raise NotImplementedError(
                "GraphDecoder is single-GPU (tp=1): RCCL collectives inside "
                "graph capture are a round-2 item; use model.generate() for "
                "TP serving")
        self.model = model
        self.max_len = max_len
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.cache = model.new_graph_kv_cache(batch_size, max_len)
        self.ids = torch.zeros(batch_size, 1, dtype=torch.long,
                               device=self.device)
        self.use_graph = (p.device.type == "cuda") if use_graph is None \
            else use_graph
        self._graph = None          # the one generate() used last
        self._graphs = {}           # sampled? -> captured step
        # what the sampled step reads: one graph serves any parameters
        self._sampled = False
        f32 = dict(dtype=torch.float32, device=self.device)
        self._temperature = torch.zeros(batch_size, **f32)
        self._top_k = torch.zeros(batch_size, dtype=torch.int32,
                                  device=self.device)
        self._top_p = torch.ones(batch_size, **f32)
        self._u = torch.zeros(batch_size, **f32)
        self._generator = None

    def _select(self, logits: torch.Tensor) -> torch.Tensor:
        """The next token of every row of ``logits [B, V]``, as [B, 1]."""
        if not self._sampled:
            return logits.argmax(-1, keepdim=True)
        from pipegoose_amd.ops.sampling import sample_logits
        return sample_logits(logits, self._u, self._temperature, self._top_k,
                             self._top_p).unsqueeze(-1)

    # ------------------------------------------------------------------ step

    @torch.no_grad()
    def _step(self):
        """One self-advancing decode step (the captured region)."""
        logits, _ = self.model(self.ids, past=self.cache, use_cache=True)
        self.ids.copy_(self._select(logits[:, -1]))
        self.cache.advance()

    @torch.no_grad()
    def _capture(self):
        """Run ONE real warmup step (allocator priming), then record the
        graph.  Always returns the warmup step's token — even when capture
        fails, that step advanced the state and its token must be kept."""
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
        except Exception:       # no device: nothing ran, nothing to return
            self.use_graph = False
            self._graph = None
            return None
        with torch.cuda.stream(s):
            self._step()
        torch.cuda.current_stream().wait_stream(s)
        warmup_token = self.ids.clone()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):   # records, does not execute
                self._step()
            self._graph = g
        except Exception:
            # capture unsupported here: permanent eager fallback
            self.use_graph = False
            self._graph = None
        return warmup_token

    # -------------------------------------------------------------- generate

    @torch.no_grad()
    def generate(self, prompt_ids: torch.Tensor, max_new_tokens: int,
                 temperature: float = 0.0, top_k: int = 0,
                 top_p: float = 1.0, generator=None) -> torch.Tensor:
        """Decode ``max_new_tokens`` tokens after ``prompt_ids`` [B, P];
        returns [B, max_new_tokens].  ``temperature == 0`` is greedy (the
        argmax step, a graph of its own); otherwise every token is drawn by ``sample_logits``
        from uniforms of ``generator`` (a ``torch.Generator`` on the model's
        device; the decoder's own, freshly seeded, by default), all drawn
        before the first step: a graph run and an eager run of one seed give
        the same tokens."""
        B, P = prompt_ids.shape
        assert B == self.ids.size(0), "batch size fixed at construction"
        assert P + max_new_tokens <= self.max_len, "raise max_len"
        self.model.eval()
        self.cache.reset()
        self._sampled = temperature > 0
        uniforms = None
        if self._sampled:
            self._temperature.fill_(temperature)
            self._top_k.fill_(top_k)
            self._top_p.fill_(top_p)
            if generator is None:
                if self._generator is None:
                    self._generator = torch.Generator(device=self.device)
                    self._generator.seed()
                generator = self._generator
            uniforms = torch.rand(max_new_tokens, B, generator=generator,
                                  device=self.device)
            self._u.copy_(uniforms[0])

        # eager prefill fills cache slots 0..P-1
        logits, _ = self.model(prompt_ids.to(self.device), past=self.cache,
                               use_cache=True)
        self.ids.copy_(self._select(logits[:, -1]))
        self.cache.enter_graph_mode()

        tokens = [self.ids.clone()]
        remaining = max_new_tokens - 1
        self._graph = self._graphs.get(self._sampled)
        if self.use_graph and remaining > 1 and self._graph is None:
            if uniforms is not None:
                self._u.copy_(uniforms[1])
            warmup_token = self._capture()
            if self._graph is not None:
                self._graphs[self._sampled] = self._graph
            if warmup_token is not None:  # the warmup step really ran
                tokens.append(warmup_token)
                remaining -= 1
        # a previously captured graph replays against the CURRENT buffer
        # contents — no re-capture needed across calls
        for _ in range(remaining):
            if uniforms is not None:      # async copy into the static buffer
                self._u.copy_(uniforms[len(tokens)])
            if self._graph is not None:
                self._graph.replay()
            else:
                self._step()
            tokens.append(self.ids.clone())
        return torch.cat(tokens, dim=1)
