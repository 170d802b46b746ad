"""Decode of a RAGGED batch over a paged KV cache, greedy or sampled.

The sibling of ``GraphDecoder`` (models/graph_decode.py) for prompts of
different lengths: K/V live in a page pool shared by all sequences
(``PagedKVCache``, models/kv_cache.py), every sequence has a block-table row
and a device position of its own, and the decode step — cache write through
the table, paged decode attention, token selection, advance — runs batched
over all live rows with per-row positions (ops/paged_attention.py,
csrc/decode_attention.hip).

``generate`` allocates every slot's pages for prompt + new tokens up front,
so the step has static shapes and addresses and is captured into a hipGraph
exactly as ``GraphDecoder._capture`` does, keyed by the number of live rows;
CPU, ``use_graph=False`` or a failed capture step eagerly with identical
numerics.  tp=1.

Token selection is greedy (``temperature == 0``, the default: an argmax) or
sampled with temperature, top-k and top-p, each a scalar or one value per
prompt (ops/sampling.py, csrc/sampling.hip).  The sampled step reads its
parameters and its uniforms from static per-slot device buffers, so one graph
per live-row count serves any parameters; the greedy step is a graph of its
own and is what it was.  The uniforms of a call are drawn on the device before
its first step, ``[steps, rows]`` from a ``torch.Generator`` (``generator``,
or the decoder's own freshly seeded one), and copied step by step into the
static buffer ahead of the replay: a graph run and an eager run of one seed
give the same tokens.

``prefill_chunk`` feeds a prompt in pieces of at most that many tokens (the
later pieces attend over the pages behind them: paged prefill attention,
csrc/paged_prefill_attention.hip), which bounds the activation memory and the
latency of one forward.  ``share_prefix`` lets a prompt reuse the whole pages
of the longest token prefix it has in common with an earlier prompt of the
same call (``PagedKVCache.fork``) and prefills only the rest.

``batched_prefill=True`` prefills all prompts of a call together instead of
one at a time: every round packs the next ``prefill_chunk`` tokens of every
unfinished prompt (or the rest) into one forward ``ids [1, T]`` over
``PagedKVCache.packed``, with one ragged-batch attention launch per layer
(csrc/paged_varlen_attention.hip, profiles/paged_varlen_attn.md; over an fp8
cache csrc/paged_fp8_varlen_attention.hip, profiles/paged_fp8_varlen_attn.md).
With an fp8 cache it needs the fp8 kernels (``paged_fp8_kernel_supported``: a
bf16 model on the GPU, head dim 64 or 128, a page size of 16/32/64/128, the
extension, ``PG_DECODE_ATTN != "0"``) and is refused elsewhere, where the
packed forward would run the pure-torch reference over the dequantised cache
at full capacity.  The decode step and its graphs are the same.

``kv_dtype=torch.float8_e4m3fn`` keeps the cache in fp8 with one fp32 scale
per cached row and kv head (csrc/paged_fp8_attention.hip): twice the tokens
per pool byte, about half the bytes read per decode step, at e4m3 precision
of the cached K/V (profiles/paged_fp8_decode_attn.md).  Chunked prefill and
shared prefixes attend over the fp8 pages in a kernel as well
(csrc/paged_fp8_prefill_attention.hip, profiles/paged_fp8_prefill_attn.md).
The default is the model dtype.

``generate_continuous`` is continuous batching on the same cache: any number
of prompts through ``max_seqs`` slots, every step one packed forward of the
decoding sequences' rows and the next pieces of the prefilling ones
(csrc/paged_varlen_split_attention.hip, profiles/paged_mixed_attn.md; over an
fp8 cache csrc/paged_fp8_varlen_split_attention.hip,
profiles/paged_fp8_mixed_attn.md); eager, opt-in.

``DEFAULT_PAGE_SIZE`` comes from profiles/paged_decode_attn.md.
"""
from typing import List, Optional, Sequence, Union

import torch

from pipegoose_amd.distributed.parallel_mode import ParallelMode
from pipegoose_amd.models.kv_cache import PagedPacked
from pipegoose_amd.ops.paged_attention import paged_fp8_kernel_supported
from pipegoose_amd.ops.sampling import sample_logits

DEFAULT_PAGE_SIZE = 16


class PagedDecoder:
    """Usage::

        dec = PagedDecoder(model, max_seqs=8, n_pages=257, max_len=512)
        outs = dec.generate(prompts, max_new_tokens=128)

    ``prompts`` is a list of up to ``max_seqs`` 1-D long tensors of any
    lengths; ``outs[i]`` holds the ``max_new_tokens`` tokens after
    ``prompts[i]``.  ``n_pages`` counts the reserved null page 0.
    ``prefill_chunk=None`` prefills every prompt in one forward.
    ``kv_dtype=None`` caches in the model dtype, ``torch.float8_e4m3fn`` in
    fp8."""

    def __init__(self, model, max_seqs: int, n_pages: int,
                 page_size: int = DEFAULT_PAGE_SIZE, max_len: int = 2048,
                 use_graph: Optional[bool] = None,
                 prefill_chunk: Optional[int] = None, kv_dtype=None,
                 batched_prefill: bool = False):
        assert prefill_chunk is None or prefill_chunk >= 1
        self.prefill_chunk = prefill_chunk
        self.batched_prefill = batched_prefill
        ctx = getattr(model, "parallel_context", None)
        if ctx is not None and ctx.get_world_size(ParallelMode.TENSOR) > 1:
            raise NotImplementedError(
                "PagedDecoder is single-GPU (tp=1); use model.generate() for "
                "TP serving")
        self.model = model
        p = next(model.parameters())
        self.device = p.device
        self.cache = model.new_paged_kv_cache(max_seqs, n_pages, page_size,
                                              max_len, kv_dtype=kv_dtype)
        if batched_prefill and kv_dtype == torch.float8_e4m3fn:
            pool = self.cache.k_pools[0]
            q = torch.empty(1, 1, 1, pool.size(-1), dtype=p.dtype,
                            device=p.device)
            if not paged_fp8_kernel_supported(q, pool):
                raise NotImplementedError(
                    "PagedDecoder: batched_prefill over an fp8 cache needs "
                    "the fp8 ragged-batch attention kernel (a bf16 model on "
                    "the GPU, head dim 64 or 128, page size 16/32/64/128, "
                    "the HIP extension, PG_DECODE_ATTN != 0); elsewhere "
                    "kv_dtype=torch.float8_e4m3fn prefills one prompt at a "
                    "time")
        self.ids = torch.zeros(max_seqs, 1, dtype=torch.long,
                               device=self.device)
        self.use_graph = (p.device.type == "cuda") if use_graph is None \
            else use_graph
        self._graphs = {}           # (live rows, sampled?) -> captured step
        self._graph = None          # the one generate() used last
        self._rows = {}             # live rows -> PagedRows over [0, n)
        # what the sampled step reads, per slot
        self._sampled = False
        f32 = dict(dtype=torch.float32, device=self.device)
        self._temperature = torch.zeros(max_seqs, **f32)
        self._top_k = torch.zeros(max_seqs, dtype=torch.int32,
                                  device=self.device)
        self._top_p = torch.ones(max_seqs, **f32)
        self._u = torch.zeros(max_seqs, **f32)
        self._generator = None

    def _live_rows(self, n: int):
        if n not in self._rows:
            self._rows[n] = self.cache.rows(0, n)
        return self._rows[n]

    # ------------------------------------------------------------- sampling

    def _set_sampling(self, n: int, temperature, top_k, top_p, generator):
        """Loads the per-prompt parameters (scalars or sequences of ``n``)
        into device tensors of ``n`` and returns them with the generator to
        draw from; ``_sampled`` says whether any prompt samples at all."""
        def per_prompt(x):
            vals = list(x) if isinstance(x, (Sequence, torch.Tensor)) \
                else [x] * n
            assert len(vals) == n, "one sampling parameter per prompt"
            return [float(v) for v in vals]
        t, k, p = map(per_prompt, (temperature, top_k, top_p))
        self._sampled = any(v > 0 for v in t)
        if not self._sampled:
            return None
        if generator is None:
            if self._generator is None:
                self._generator = torch.Generator(device=self.device)
                self._generator.seed()
            generator = self._generator
        return (torch.tensor(t, dtype=torch.float32, device=self.device),
                torch.tensor(k, dtype=torch.int32, device=self.device),
                torch.tensor(p, dtype=torch.float32, device=self.device),
                generator)

    def _select(self, logits: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
        """The next token of slots [lo, hi) from ``logits [hi - lo, V]``, as
        [hi - lo, 1]."""
        if not self._sampled:
            return logits.argmax(-1, keepdim=True)
        return sample_logits(logits, self._u[lo:hi],
                             self._temperature[lo:hi], self._top_k[lo:hi],
                             self._top_p[lo:hi]).unsqueeze(-1)

    # ------------------------------------------------------------------ step

    @torch.no_grad()
    def _step(self, n: int):
        """One self-advancing decode step over slots [0, n) (the captured
        region)."""
        rows = self._live_rows(n)
        ids = self.ids[:n]
        logits, _ = self.model(ids, past=rows, use_cache=True)
        ids.copy_(self._select(logits[:, -1], 0, n))
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
            self._graphs[n, self._sampled] = g
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
        self.ids[slot:slot + 1].copy_(
            self._select(logits[:, -1], slot, slot + 1))

    @torch.no_grad()
    def _prefill_batched(self, prompts: List[torch.Tensor], shared,
                         max_new_tokens: int):
        """Prefill all prompts together: every round packs the next
        ``prefill_chunk`` tokens (or the rest) of every unfinished prompt
        into ONE forward ``ids [1, T]`` (``PagedKVCache.packed``,
        csrc/paged_varlen_attention.hip).  A prompt that shares a prefix
        joins once its source holds the shared tokens.  Leaves every
        prompt's first new token in ``ids``."""
        cache = self.cache
        prompts = [p.to(self.device) for p in prompts]
        done: List[Optional[int]] = [None] * len(prompts)   # None: no pages
        step = self.prefill_chunk
        while True:
            for i, (src, sh) in enumerate(shared):
                if done[i] is None and (not sh or (done[src] or 0) >= sh):
                    if sh:
                        cache.fork(src, i, sh)
                    cache.allocate(i, prompts[i].numel() + max_new_tokens)
                    done[i] = sh
            slots, lens, room = [], [], PagedPacked.MAX_TOKENS
            for i, p in enumerate(prompts):
                if done[i] is not None and done[i] < p.numel() and room:
                    n = min(p.numel() - done[i], step or room, room)
                    slots.append(i), lens.append(n)
                    room -= n
            if not slots:
                return
            rows = cache.packed(slots, lens)
            ids = torch.cat([prompts[i][done[i]:done[i] + n]
                             for i, n in zip(slots, lens)])
            logits, _ = self.model(ids[None], past=rows, use_cache=True)
            rows.advance()
            end = 0
            for i, n in zip(slots, lens):
                end += n
                done[i] += n
                if done[i] == prompts[i].numel():
                    self.ids[i:i + 1].copy_(
                        self._select(logits[:, end - 1], i, i + 1))

    @torch.no_grad()
    def generate(self, prompts: List[torch.Tensor], max_new_tokens: int,
                 share_prefix: bool = False,
                 temperature: Union[float, Sequence[float]] = 0.0,
                 top_k: Union[int, Sequence[int]] = 0,
                 top_p: Union[float, Sequence[float]] = 1.0,
                 generator=None) -> List[torch.Tensor]:
        n = len(prompts)
        cache = self.cache
        assert 1 <= n <= cache.max_seqs, "more prompts than max_seqs"
        assert max_new_tokens >= 1
        self.model.eval()
        sampling = self._set_sampling(n, temperature, top_k, top_p, generator)
        uniforms = None
        if sampling is not None:
            self._temperature[:n].copy_(sampling[0])
            self._top_k[:n].copy_(sampling[1])
            self._top_p[:n].copy_(sampling[2])
            uniforms = torch.rand(max_new_tokens, n, generator=sampling[3],
                                  device=self.device)
            self._u[:n].copy_(uniforms[0])
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
            # shares with an earlier one — or all of them together
            if self.batched_prefill:
                self._prefill_batched(prompts, shared, max_new_tokens)
            else:
                for i, prompt in enumerate(prompts):
                    src, sh = shared[i]
                    if sh:
                        cache.fork(src, i, sh)
                    cache.allocate(i, prompt.numel() + max_new_tokens)
                    self._prefill(i, prompt, done=sh)

            tokens = [self.ids[:n].clone()]
            remaining = max_new_tokens - 1
            key = (n, self._sampled)
            if self.use_graph and remaining > 1 and key not in self._graphs:
                if uniforms is not None:
                    self._u[:n].copy_(uniforms[1])
                warmup_tokens = self._capture(n)
                if warmup_tokens is not None:   # the warmup step really ran
                    tokens.append(warmup_tokens)
                    remaining -= 1
            # a captured graph replays against the CURRENT table, positions
            # and pools — no re-capture across calls
            self._graph = self._graphs.get(key)
            rows = self._live_rows(n)
            for _ in range(remaining):
                if uniforms is not None:    # async, into the static buffer
                    self._u[:n].copy_(uniforms[len(tokens)])
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

    # ------------------------------------------------- continuous batching

    @torch.no_grad()
    def generate_continuous(self, prompts: List[torch.Tensor],
                            max_new_tokens: int,
                            token_budget: Optional[int] = None,
                            temperature: Union[float, Sequence[float]] = 0.0,
                            top_k: Union[int, Sequence[int]] = 0,
                            top_p: Union[float, Sequence[float]] = 1.0,
                            generator=None) -> List[torch.Tensor]:
        """Decode of ANY number of prompts with at most ``max_seqs``
        in flight: a prompt is admitted (first come, first served) as soon as
        a slot and the pages for ``len + max_new_tokens`` are free, and a
        sequence that holds its ``max_new_tokens`` tokens frees its slot at
        once.  Every step is ONE packed forward of at most ``token_budget``
        tokens (default ``PagedPacked.MAX_TOKENS``): one row for every
        decoding sequence, in slot order, then the next piece (at most
        ``prefill_chunk`` tokens) of every admitted sequence still
        prefilling, in admission order.  Its attention is one launch of the
        split-KV ragged kernel per layer
        (csrc/paged_varlen_split_attention.hip; over an fp8 cache
        csrc/paged_fp8_varlen_split_attention.hip, measured at 0.24-0.59x
        ``paged_varlen_attn_fp8`` on decode rows behind 1024 tokens or more,
        profiles/paged_fp8_mixed_attn.md), which serves decode rows and
        prefill pieces alike.  T varies from step to step, so
        the step is eager: no graph.  Returns what ``generate`` returns;
        ``share_prefix`` is not offered here.  The sampling arguments are
        those of ``generate``; the uniforms are drawn step by step, one per
        slot, and a sequence takes the one of the slot it was admitted to."""
        cache = self.cache
        budget = PagedPacked.MAX_TOKENS if token_budget is None \
            else token_budget
        n = len(prompts)
        assert n >= 1 and max_new_tokens >= 1
        assert cache.max_seqs <= budget <= PagedPacked.MAX_TOKENS, (
            f"token_budget must lie in [max_seqs = {cache.max_seqs}, "
            f"{PagedPacked.MAX_TOKENS}]: every decoding sequence needs its "
            f"row, got {budget}")
        page = cache.page_size
        need = []                       # pages per prompt
        for prompt in prompts:
            assert prompt.dim() == 1 and prompt.numel() >= 1
            total = prompt.numel() + max_new_tokens
            if total > cache.max_len:
                raise RuntimeError(
                    f"PagedKVCache: {total} tokens exceed max_len "
                    f"{cache.max_len}")
            need.append(-(-total // page))
            if need[-1] > cache.n_pages - 1:
                raise RuntimeError(
                    f"PagedKVCache: out of pages: a prompt needs "
                    f"{need[-1]}, the pool has {cache.n_pages - 1}")
        self.model.eval()
        sampling = self._set_sampling(n, temperature, top_k, top_p, generator)
        prompts = [p.to(self.device) for p in prompts]
        free_slots = [s for s in range(cache.max_seqs) if not cache.pages[s]]
        waiting = list(range(n))
        slot_of = {}                    # in flight: prompt -> slot,
        done = {}                       # in admission order; tokens fed
        outs: List[List[torch.Tensor]] = [[] for _ in range(n)]
        try:
            while waiting or slot_of:
                while waiting and free_slots \
                        and need[waiting[0]] <= cache.n_free_pages:
                    i = waiting.pop(0)
                    slot_of[i] = free_slots.pop(0)
                    cache.allocate(slot_of[i],
                                   prompts[i].numel() + max_new_tokens)
                    done[i] = 0
                if not slot_of:
                    raise RuntimeError(
                        "PagedKVCache: out of pages: nothing is in flight "
                        f"and the next prompt needs {need[waiting[0]]} of "
                        f"{cache.n_free_pages} free pages")
                # decode rows in slot order, then pieces in admission order
                seqs = sorted((i for i in slot_of
                               if done[i] == prompts[i].numel()),
                              key=slot_of.get)
                lens = [1] * len(seqs)
                pieces = [outs[i][-1] for i in seqs]
                room = budget - len(seqs)
                for i in slot_of:
                    left = prompts[i].numel() - done[i]
                    if left and room:
                        k = min(left, self.prefill_chunk or room, room)
                        seqs.append(i), lens.append(k)
                        pieces.append(prompts[i][done[i]:done[i] + k])
                        room -= k
                rows = cache.packed([slot_of[i] for i in seqs], lens,
                                    split_kv=True)
                logits, _ = self.model(torch.cat(pieces)[None], past=rows,
                                       use_cache=True)
                rows.advance()
                # the last row of every sequence that decoded or whose piece
                # ended its prompt
                last, end = [], 0
                for i, k in zip(seqs, lens):
                    end += k
                    done[i] = min(done[i] + k, prompts[i].numel())
                    if done[i] == prompts[i].numel():
                        last.append((i, end - 1))
                if not last:
                    continue
                at = torch.tensor([t for _, t in last], device=self.device)
                if sampling is None:
                    tokens = logits[0, at].argmax(-1)
                else:
                    who = torch.tensor([i for i, _ in last],
                                       device=self.device)
                    slots = torch.tensor([slot_of[i] for i, _ in last],
                                         device=self.device)
                    u = torch.rand(cache.max_seqs, generator=sampling[3],
                                   device=self.device)
                    tokens = sample_logits(logits[0, at], u[slots],
                                           sampling[0][who], sampling[1][who],
                                           sampling[2][who])
                for j, (i, _) in enumerate(last):
                    outs[i].append(tokens[j:j + 1])
                    if len(outs[i]) == max_new_tokens:
                        cache.free(slot_of[i])
                        free_slots.append(slot_of.pop(i))
                        free_slots.sort()
            return [torch.cat(o) for o in outs]
        finally:
            for slot in slot_of.values():
                cache.free(slot)
