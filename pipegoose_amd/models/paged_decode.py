"""Greedy decode of a RAGGED batch over a paged KV cache.

The sibling of ``GraphDecoder`` (models/graph_decode.py) for prompts of
different lengths: K/V live in a page pool shared by all sequences
(``PagedKVCache``, models/kv_cache.py), every sequence has a block-table row
and a device position of its own, and the decode step — cache write through
the table, paged decode attention, argmax, advance — runs batched over all
live rows with per-row positions (ops/paged_attention.py,
csrc/decode_attention.hip).

``generate`` allocates every slot's pages for prompt + new tokens up front,
so the step has static shapes and addresses and is captured into a hipGraph
exactly as ``GraphDecoder._capture`` does, keyed by the number of live rows;
CPU, ``use_graph=False`` or a failed capture step eagerly with identical
numerics.  Greedy, tp=1.

``DEFAULT_PAGE_SIZE`` comes from profiles/paged_decode_attn.md.
"""
from typing import List, Optional

import torch

from pipegoose_amd.distributed.parallel_mode import ParallelMode

DEFAULT_PAGE_SIZE = 16


class PagedDecoder:
    """Usage::

        dec = PagedDecoder(model, max_seqs=8, n_pages=257, max_len=512)
        outs = dec.generate(prompts, max_new_tokens=128)

    ``prompts`` is a list of up to ``max_seqs`` 1-D long tensors of any
    lengths; ``outs[i]`` holds the ``max_new_tokens`` tokens after
    ``prompts[i]``.  ``n_pages`` counts the reserved null page 0."""

    def __init__(self, model, max_seqs: int, n_pages: int,
                 page_size: int = DEFAULT_PAGE_SIZE, max_len: int = 2048,
                 use_graph: Optional[bool] = None):
        ctx = getattr(model, "parallel_context", None)
        if ctx is not None and ctx.get_world_size(ParallelMode.TENSOR) > 1:
            raise NotImplementedError(
                "PagedDecoder is single-GPU (tp=1); use model.generate() for "
                "TP serving")
        self.model = model
        p = next(model.parameters())
        self.device = p.device
        self.cache = model.new_paged_kv_cache(max_seqs, n_pages, page_size,
                                              max_len)
        self.ids = torch.zeros(max_seqs, 1, dtype=torch.long,
                               device=self.device)
        self.use_graph = (p.device.type == "cuda") if use_graph is None \
            else use_graph
        self._graphs = {}           # live rows -> captured step
        self._graph = None          # the one generate() used last
        self._rows = {}             # live rows -> PagedRows over [0, n)

    def _live_rows(self, n: int):
        if n not in self._rows:
            self._rows[n] = self.cache.rows(0, n)
        return self._rows[n]

    # ------------------------------------------------------------------ step

    @torch.no_grad()
    def _step(self, n: int):
        """One self-advancing decode step over slots [0, n) (the captured
        region)."""
        rows = self._live_rows(n)
        ids = self.ids[:n]
        logits, _ = self.model(ids, past=rows, use_cache=True)
        ids.copy_(logits[:, -1].argmax(-1, keepdim=True))
        rows.advance(1)

    @torch.no_grad()
    def _capture(self, n: int):
        """Run ONE real warmup step (allocator priming), then record the
        graph for ``n`` live rows.  Returns the warmup step's tokens — even
        when capture fails, that step advanced the state — or None when
        nothing ran."""
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
        except Exception:       # no device: nothing ran, nothing to return
            self.use_graph = False
            return None
        with torch.cuda.stream(s):
            self._step(n)
        torch.cuda.current_stream().wait_stream(s)
        warmup_tokens = self.ids[:n].clone()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):   # records, does not execute
                self._step(n)
            self._graphs[n] = g
        except Exception:
            # capture unsupported here: permanent eager fallback
            self.use_graph = False
            self._graphs.clear()
        return warmup_tokens

    # -------------------------------------------------------------- generate

    @torch.no_grad()
    def generate(self, prompts: List[torch.Tensor], max_new_tokens: int
                 ) -> List[torch.Tensor]:
        n = len(prompts)
        cache = self.cache
        assert 1 <= n <= cache.max_seqs, "more prompts than max_seqs"
        assert max_new_tokens >= 1
        self.model.eval()
        try:
            # every page the run needs, before anything is launched: running
            # out raises here, and the decode steps have static addresses
            for i, prompt in enumerate(prompts):
                assert prompt.dim() == 1 and prompt.numel() >= 1
                cache.allocate(i, prompt.numel() + max_new_tokens)

            # prefill each prompt alone into its slot
            for i, prompt in enumerate(prompts):
                rows = cache.rows(i, i + 1)
                logits, _ = self.model(prompt.to(self.device)[None],
                                       past=rows, use_cache=True)
                self.ids[i].copy_(logits[0, -1].argmax(-1, keepdim=True))
                rows.advance(prompt.numel())

            tokens = [self.ids[:n].clone()]
            remaining = max_new_tokens - 1
            if self.use_graph and remaining > 1 and n not in self._graphs:
                warmup_tokens = self._capture(n)
                if warmup_tokens is not None:   # the warmup step really ran
                    tokens.append(warmup_tokens)
                    remaining -= 1
            # a captured graph replays against the CURRENT table, positions
            # and pools — no re-capture across calls
            self._graph = self._graphs.get(n)
            rows = self._live_rows(n)
            for _ in range(remaining):
                if self._graph is not None:
                    self._graph.replay()
                    rows.host_advance(1)
                else:
                    self._step(n)
                tokens.append(self.ids[:n].clone())
            out = torch.cat(tokens, dim=1)
            return [out[i] for i in range(n)]
        finally:
            for i in range(n):
                cache.free(i)
