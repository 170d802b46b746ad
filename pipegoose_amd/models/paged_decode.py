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

``prefill_chunk`` feeds a prompt in pieces of at most that many tokens (the
later pieces attend over the pages behind them: paged prefill attention,
csrc/paged_prefill_attention.hip), which bounds the activation memory and the
latency of one forward.  ``share_prefix`` lets a prompt reuse the whole pages
of the longest token prefix it has in common with an earlier prompt of the
same call (``PagedKVCache.fork``) and prefills only the rest.

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
    ``prompts[i]``.  ``n_pages`` counts the reserved null page 0.
    ``prefill_chunk=None`` prefills every prompt in one forward."""

    def __init__(self, model, max_seqs: int, n_pages: int,
                 page_size: int = DEFAULT_PAGE_SIZE, max_len: int = 2048,
                 use_graph: Optional[bool] = None,
                 prefill_chunk: Optional[int] = None):
        assert prefill_chunk is None or prefill_chunk >= 1
        self.prefill_chunk = prefill_chunk
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

    def _shared_prefixes(self, prompts: List[torch.Tensor]):
        """For every prompt, (earlier prompt, shared tokens): the longest
        common token prefix with an earlier prompt, rounded down to whole
        pages and capped at ``len - 1`` so that at least one token is run;
        (None, 0) where nothing is shared.  Compared on the host."""
        page = self.cache.page_size
        host = [p.tolist() for p in prompts]
        plan = []
        for i, tokens in enumerate(host):
            best_src, best = None, 0
            for j in range(i):
                other = host[j]
                common = 0
                limit = min(len(tokens) - 1, len(other))
                while common < limit and tokens[common] == other[common]:
                    common += 1
                common = common // page * page
                if common > best:
                    best_src, best = j, common
            plan.append((best_src, best))
        return plan

    @torch.no_grad()
    def _prefill(self, slot: int, prompt: torch.Tensor, done: int = 0):
        """Run tokens ``done..`` of ``prompt`` into ``slot`` (which holds the
        first ``done``), whole or in pieces of ``prefill_chunk``; leaves the
        first new token in ``ids[slot]``."""
        rows = self.cache.rows(slot, slot + 1)
        prompt = prompt.to(self.device)
        step = self.prefill_chunk or prompt.numel()
        logits = None
        for lo in range(done, prompt.numel(), step):
            piece = prompt[lo:lo + step]
            logits, _ = self.model(piece[None], past=rows, use_cache=True)
            rows.advance(piece.numel())
        self.ids[slot].copy_(logits[0, -1].argmax(-1, keepdim=True))

    @torch.no_grad()
    def generate(self, prompts: List[torch.Tensor], max_new_tokens: int,
                 share_prefix: bool = False) -> List[torch.Tensor]:
        n = len(prompts)
        cache = self.cache
        assert 1 <= n <= cache.max_seqs, "more prompts than max_seqs"
        assert max_new_tokens >= 1
        self.model.eval()
        try:
            for prompt in prompts:
                assert prompt.dim() == 1 and prompt.numel() >= 1
            shared = self._shared_prefixes(prompts) if share_prefix \
                else [(None, 0)] * n
            # every page the run needs (shared pages count once), before
            # anything is launched: running out raises here, and the decode
            # steps have static addresses
            page = cache.page_size
            longest = max(p.numel() for p in prompts) + max_new_tokens
            if longest > cache.max_len:
                raise RuntimeError(
                    f"PagedKVCache: {longest} tokens exceed max_len "
                    f"{cache.max_len}")
            fresh = sum(-(-(p.numel() + max_new_tokens) // page) - sh // page
                        for p, (_, sh) in zip(prompts, shared))
            if fresh > cache.n_free_pages:
                raise RuntimeError(
                    f"PagedKVCache: out of pages: the run needs {fresh}, "
                    f"{cache.n_free_pages} of {cache.n_pages - 1} are free")

            # prefill each prompt alone into its slot, behind the pages it
            # shares with an earlier one
            for i, prompt in enumerate(prompts):
                src, sh = shared[i]
                if sh:
                    cache.fork(src, i, sh)
                cache.allocate(i, prompt.numel() + max_new_tokens)
                self._prefill(i, prompt, done=sh)

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
