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
        """Multi-token forwards are prefills from empty slots only (no
        prefix reuse, no chunked prefill); checked on the host mirror."""
        self._rows.assert_empty()


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
    Pages are handed out from a host free list; no page is ever owned by two
    slots, and running out raises before anything is launched."""

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
            self.table_host[slot, len(self.pages[slot])] = page
            self.pages[slot].append(page)
        self.block_table[slot].copy_(self.table_host[slot])

    def free(self, slot: int):
        """Return the slot's pages; zero its table row and position."""
        self._free.extend(reversed(self.pages[slot]))
        self.pages[slot] = []
        self.table_host[slot].zero_()
        self.block_table[slot].zero_()
        self.pos_t[slot] = 0
        self.filled[slot] = 0

    def rows(self, lo: int, hi: int) -> PagedRows:
        return PagedRows(self, lo, hi)
