"""Static KV cache for incremental decode.

The naive cache re-`cat`s the whole [B, H, S, D] history every step and
layer (O(S) copies per token).  A StaticKVCache preallocates
[B, H, max_len, D] once and index-writes the new step — no growth copies,
stable addresses (hipGraph-friendly for a future captured decode step).

A PagedKVCache instead shares one pool of fixed-size pages among all
sequences through a block table, so memory follows the tokens actually held
and prompts of different lengths decode in one batch (models/paged_decode.py).

Beyond-reference capability (the reference had no decode path at all).
"""
from typing import List, Tuple

import torch


class LayerKVCache:
    def __init__(self, B: int, H: int, max_len: int, D: int,
                 dtype: torch.dtype, device: torch.device):
        self.k = torch.empty(B, H, max_len, D, dtype=dtype, device=device)
        self.v = torch.empty(B, H, max_len, D, dtype=dtype, device=device)
        self.len = 0

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Write the new steps and return views of the filled prefix."""
        s = k_new.size(2)
        assert self.len + s <= self.k.size(2), "KV cache overflow"
        self.k[:, :, self.len:self.len + s] = k_new
        self.v[:, :, self.len:self.len + s] = v_new
        self.len += s
        return self.k[:, :, :self.len], self.v[:, :, :self.len]


class StaticKVCache:
    """Per-layer static caches; duck-types the (k, v) tuple list the model's
    ``past=`` plumbing expects via __getitem__."""

    def __init__(self, n_layers: int, B: int, H: int, max_len: int, D: int,
                 dtype: torch.dtype, device):
        self.layers: List[LayerKVCache] = [
            LayerKVCache(B, H, max_len, D, dtype, torch.device(device))
            for _ in range(n_layers)]

    def __getitem__(self, i: int) -> "LayerKVCache":
        return self.layers[i]

    def __len__(self):
        return len(self.layers)

    @property
    def seq_len(self) -> int:
        return self.layers[0].len


class GraphLayerKVCache(LayerKVCache):
    """LayerKVCache whose decode write is shape-static: in graph mode
    ``append`` index-writes at a DEVICE position tensor and returns the FULL
    buffers, so a captured hipGraph replays with constant shapes/addresses
    while the position advances as data (models/graph_decode.py)."""

    def __init__(self, B, H, max_len, D, dtype, device, pos_t: torch.Tensor):
        super().__init__(B, H, max_len, D, dtype, device)
        # full-length attention reads UNFILLED slots (masked by -inf bias);
        # they must be finite — inf garbage in q·k would make inf + (-inf)
        # = NaN and poison the whole softmax row
        self.k.zero_()
        self.v.zero_()
        self.pos_t = pos_t          # int64 [1], shared across layers
        self.graph_mode = False

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor):
        if not self.graph_mode:     # eager prefill: normal growing prefix
            return super().append(k_new, v_new)
        # decode step: k_new is [B, H, 1, D]; write at pos_t, return full S_max
        self.k.index_copy_(2, self.pos_t, k_new)
        self.v.index_copy_(2, self.pos_t, v_new)
        return self.k, self.v


class GraphKVCache:
    """Static cache bank for graph-captured decode: one shared device
    position scalar, per-layer static buffers.  ``graph_mode`` off = behaves
    like StaticKVCache (eager prefill fills the prefix); on = every layer
    writes at ``pos_t`` and attention runs full-length with a position mask."""

    def __init__(self, n_layers: int, B: int, H: int, max_len: int, D: int,
                 dtype: torch.dtype, device):
        device = torch.device(device)
        self.pos_t = torch.zeros(1, dtype=torch.long, device=device)
        self.max_len = max_len
        self.layers: List[GraphLayerKVCache] = [
            GraphLayerKVCache(B, H, max_len, D, dtype, device, self.pos_t)
            for _ in range(n_layers)]

    def __getitem__(self, i: int) -> GraphLayerKVCache:
        return self.layers[i]

    def __len__(self):
        return len(self.layers)

    @property
    def seq_len(self) -> int:
        return self.layers[0].len

    def enter_graph_mode(self):
        """Call after prefill: freeze shapes, position = filled length."""
        self.pos_t.fill_(self.layers[0].len)
        for layer in self.layers:
            layer.graph_mode = True

    def advance(self):
        self.pos_t.add_(1)  # capture-safe: device-side increment

    def reset(self):
        """Back to eager-prefill state (buffer addresses unchanged, so a
        previously captured graph stays valid)."""
        self.pos_t.zero_()
        for layer in self.layers:
            layer.graph_mode = False
            layer.len = 0


class PagedLayerView:
    """What ``past[i]`` is for a forward over slots ``[lo, hi)`` of a
    PagedKVCache: one layer's pools plus views (no copies) of the shared
    block table and positions.  ``paged = True`` selects the paged branch of
    the attentions."""
    paged = True

    def __init__(self, k_pool, v_pool, block_table, pos_t, rows):
        self.k_pool, self.v_pool = k_pool, v_pool
        self.block_table, self.pos_t = block_table, pos_t
        self._rows = rows

    def assert_empty(self):
        """Raise unless every slot of the range is empty (host mirror)."""
        self._rows.assert_empty()

    def has_prefix(self, n_new: int = 0) -> bool:
        """Whether any slot of the range already holds tokens (host mirror):
        a multi-token forward then attends over the pools behind ``pos_t``
        (chunked prefill, prefix reuse) instead of over its fresh rows, and
        its ``n_new`` tokens must fit the pages every slot has."""
        return self._rows.has_prefix(n_new)


class PagedRows:
    """The ``past=`` object for the contiguous slot range ``[lo, hi)``."""

    def __init__(self, cache: "PagedKVCache", lo: int, hi: int):
        assert 0 <= lo < hi <= cache.max_seqs, (lo, hi)
        self.cache, self.lo, self.hi = cache, lo, hi
        self.block_table = cache.block_table[lo:hi]
        self.pos_t = cache.pos_t[lo:hi]
        self.layers = [PagedLayerView(k, v, self.block_table, self.pos_t, self)
                       for k, v in zip(cache.k_pools, cache.v_pools)]

    def __getitem__(self, i: int) -> PagedLayerView:
        return self.layers[i]

    def __len__(self):
        return len(self.layers)

    def assert_empty(self):
        filled = self.cache.filled[self.lo:self.hi]
        assert not any(filled), (
            f"paged prefill needs empty slots, slots {self.lo}..{self.hi - 1} "
            f"hold {filled} tokens")

    def has_prefix(self, n_new: int = 0) -> bool:
        cache = self.cache
        if not any(cache.filled[self.lo:self.hi]):
            return False
        # rows written past a slot's pages would land in the null page and
        # be read back as if they were the sequence
        for slot in range(self.lo, self.hi):
            room = len(cache.pages[slot]) * cache.page_size
            assert cache.filled[slot] + n_new <= room, (
                f"paged prefill of {n_new} tokens runs past the pages of "
                f"slot {slot} ({cache.filled[slot]} tokens held, pages for "
                f"{room}): allocate() first, or free() the slot and prefill "
                f"it empty")
        return True

    def advance(self, n: int = 1):
        """The forward just run wrote ``n`` tokens per row: move the device
        positions (capture-safe) and, unless the call is only being recorded
        into a graph, the host mirror."""
        self.pos_t.add_(n)
        if not (self.pos_t.is_cuda
                and torch.cuda.is_current_stream_capturing()):
            self.host_advance(n)

    def host_advance(self, n: int = 1):
        """Host mirror only: after replaying a captured step that advances."""
        cache = self.cache
        for slot in range(self.lo, self.hi):
            cache.filled[slot] += n
            assert cache.filled[slot] <= \
                len(cache.pages[slot]) * cache.page_size, \
                f"slot {slot} ran past its allocated pages"


class PagedKVCache:
    """Paged cache bank: per layer one K and one V pool
    ``[n_pages, Hkv, page_size, D]`` shared by all sequences; one int32
    ``block_table`` [max_seqs, max_pages] and one int64 ``pos_t`` [max_seqs]
    (filled length = position of the next token) shared by all layers, both on
    the device, the table with a host mirror.

    Page 0 is a reserved null page: it is never handed out and the table is
    initialised to 0, so a stale entry can only ever name the null page.
    Pages are handed out from a host free list with a per-page reference
    count, and running out raises before anything is launched.  A page is
    held by two slots only through ``fork``, which shares WHOLE pages of a
    prefix: a shared page is full and lies below ``filled`` of every holder,
    so nobody ever writes it and no copy-on-write is needed.  Every other
    page has exactly one holder."""

    def __init__(self, n_layers: int, max_seqs: int, n_pages: int,
                 page_size: int, max_len: int, Hkv: int, D: int,
                 dtype: torch.dtype, device):
        assert page_size in (16, 32, 64, 128), \
            f"page_size must be 16, 32, 64 or 128, got {page_size}"
        assert n_pages >= 2, "page 0 is reserved: n_pages must be >= 2"
        device = torch.device(device)
        self.max_seqs, self.n_pages = max_seqs, n_pages
        self.page_size = page_size
        self.max_pages = -(-max_len // page_size)
        self.max_len = self.max_pages * page_size
        # zeros, not empty: the reference path gathers whole pages
        self.k_pools = [torch.zeros(n_pages, Hkv, page_size, D, dtype=dtype,
                                    device=device) for _ in range(n_layers)]
        self.v_pools = [torch.zeros(n_pages, Hkv, page_size, D, dtype=dtype,
                                    device=device) for _ in range(n_layers)]
        self.block_table = torch.zeros(max_seqs, self.max_pages,
                                       dtype=torch.int32, device=device)
        self.table_host = torch.zeros(max_seqs, self.max_pages,
                                      dtype=torch.int32)
        self.pos_t = torch.zeros(max_seqs, dtype=torch.long, device=device)
        self.filled: List[int] = [0] * max_seqs        # host mirror of pos_t
        self.pages: List[List[int]] = [[] for _ in range(max_seqs)]
        self._free: List[int] = list(range(n_pages - 1, 0, -1))
        self.refcount: List[int] = [0] * n_pages

    @property
    def n_free_pages(self) -> int:
        return len(self._free)

    def allocate(self, slot: int, n_tokens: int):
        """Grow the slot's page list to cover ``n_tokens`` tokens and upload
        the changed table row."""
        want = -(-n_tokens // self.page_size)
        if want > self.max_pages:
            raise RuntimeError(
                f"PagedKVCache: {n_tokens} tokens exceed max_len "
                f"{self.max_len}")
        need = want - len(self.pages[slot])
        if need <= 0:
            return
        if need > len(self._free):
            raise RuntimeError(
                f"PagedKVCache: out of pages: slot {slot} needs {need} more "
                f"for {n_tokens} tokens, {len(self._free)} of "
                f"{self.n_pages - 1} are free")
        for _ in range(need):
            page = self._free.pop()
            self.refcount[page] = 1
            self.table_host[slot, len(self.pages[slot])] = page
            self.pages[slot].append(page)
        self.block_table[slot].copy_(self.table_host[slot])

    def free(self, slot: int):
        """Drop the slot's hold on its pages, returning those nobody else
        holds; zero its table row and position."""
        for page in reversed(self.pages[slot]):
            self.refcount[page] -= 1
            if self.refcount[page] == 0:
                self._free.append(page)
        self.pages[slot] = []
        self.table_host[slot].zero_()
        self.block_table[slot].zero_()
        self.pos_t[slot] = 0
        self.filled[slot] = 0

    def fork(self, src: int, dst: int, n_tokens: int) -> int:
        """Share the first ``n_tokens // page_size`` WHOLE pages of ``src``
        with the empty slot ``dst`` and set ``dst``'s table row, position and
        ``filled`` to the shared token count, which is returned.  ``allocate``
        then appends fresh pages after the shared ones."""
        assert src != dst, "fork needs two different slots"
        assert self.filled[dst] == 0 and not self.pages[dst], (
            f"fork needs an empty slot that owns no pages, slot {dst} holds "
            f"{self.filled[dst]} tokens on {len(self.pages[dst])} pages")
        assert 0 <= n_tokens <= self.filled[src], (
            f"fork of {n_tokens} tokens, slot {src} holds {self.filled[src]}")
        n_shared = n_tokens // self.page_size
        shared = self.pages[src][:n_shared]
        for i, page in enumerate(shared):
            self.refcount[page] += 1
            self.table_host[dst, i] = page
        self.pages[dst] = list(shared)
        tokens = n_shared * self.page_size
        self.block_table[dst].copy_(self.table_host[dst])
        self.pos_t[dst] = tokens
        self.filled[dst] = tokens
        return tokens

    def rows(self, lo: int, hi: int) -> PagedRows:
        return PagedRows(self, lo, hi)
