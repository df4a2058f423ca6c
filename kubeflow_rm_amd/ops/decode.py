"""KV-cache decode: the cache, the append and attention over it (``kernels/attn_kv.hip``).

``KVCache`` holds the per-layer K / V tensors ``[B, H, capacity, D]`` and the device-side ``lens``
(``int32 [B]``): every kernel reads positions from ``lens``, so a decode step captured into a hipGraph
replays while the position advances (``lens.add_(1)`` is part of the step). ``t_bound`` is the host-side
upper bound of ``lens`` that sizes the attention grid; a step meant for capture sets it to the capacity.

``kv_append(qkv, cache, layer)`` copies the K and V rows of a fused QKV activation ``[B, T, 3*H*D]``
to rows ``lens[b] .. lens[b]+T-1``; ``attention_decode(q, cache, layer)`` attends one query row per
head over keys ``0 .. lens[b]-1`` (or an explicit ``lens`` / ``t_bound``). Neither advances ``lens``. A
model step that appends T rows passes its attention ``lens=cache.lens_after(T)`` (a device tensor
``lens + T``: the rows it just appended are attended too) with ``t_bound=cache.bound_after(T)``, and
calls ``cache.advance(T)`` (``lens.add_(T)``) once, after the last layer. The cache keeps no record of
a step in flight.

``attention_extend(q, cache, layer)`` is the multi-token form (``attn_extend_split``, up to 8 row slots):
T <= 16 new query rows per head, already appended, each attending the cache up to its own row; with
``KVCache.rewind(n)`` (drop the last n rows) it carries ``GPT.extend`` and draft-and-verify decoding.

``attention_chunk(q, cache, layer)`` is the same contract without the row limit, on MFMA query tiles
(``attn_chunk_split`` in ``kernels/attn_kv_mfma.hip``: K / V read once per 128 new rows): 1 <= T <= capacity
new rows, which carries ``GPT.extend(chunk=N)`` and ``GPT.generate(prefill_chunk=N)`` — a follow-up turn or a
long prompt over a cache that is not empty, N rows of activations at a time.

On CPU tensors the same functions run plain torch (index copy, masked fp32 SDPA): the CPU model path
and its tests. On a GPU there is no fallback: a shape the kernels reject raises.

``KVCache(..., dtype=torch.float8_e4m3fn)`` is the 8-bit cache (the kernels' ``Fp8Rows`` format): ``k`` /
``v`` hold OCP e4m3fn codes ``[B, H, capacity, D]`` and ``k_scale`` / ``v_scale`` one fp32 scale per stored row
``[B, H, capacity]``. ``kv_append`` quantises each K / V row on the way in (``quantize_rows``: ``scale =
amax / 448``, ``code = RNE_e4m3(clamp(x / scale, -448, 448))``, an all-zero row stores ``scale = 1``); the
attention kernels multiply the scales in (``(q . codes_k[j]) * k_scale[j]``, ``p * v_scale[j]``) and never
write a dequantised tensor. The three functions dispatch on the cache's dtype; everything else about the
cache (``lens``, ``t_bound``, ``advance``, ``rewind``, the workspaces) is the same. ``KVCache.nbytes`` is
what a cache holds in device memory.

Grouped-query attention: the cache's ``H`` counts K / V heads; ``attention_decode`` / ``attention_extend`` /
``attention_chunk`` take a ``q`` of ``Hq = G * cache.H`` heads and infer G from the shapes: query head ``h`` reads
K / V head ``h // G`` (the Llama convention). ``kv_append(qkv, cache, layer, q_heads=Hq)`` reads a fused activation
``[B, T, (Hq + 2 * cache.H) * D]`` laid out ``q: Hq * D | k: H * D | v: H * D``. On a GPU G is one of ``GROUP_SIZES``
(any other ratio raises ``ValueError``) and the kernels see ``T * G`` rows per (batch, K / V head): token-major,
row ``t * G + g`` with the limit of token ``t``, so K / V are streamed once for the whole group. ``attention_decode``
with G > 1 is ``attention_extend`` at T = 1; ``attention_extend`` takes ``T * G <= MAX_EXTEND_ROWS`` rows and, for
G > 1, runs the extend kernel's row slots below ``GQA_MFMA_MIN_ROWS`` rows and ``attention_chunk``'s MFMA kernel from
there on (faster from 8 rows: profiles/gqa; the results then agree with the VALU form within the kernels' bounds,
not bit for bit). The CPU /
``ops.torch_reference()`` forms take any divisor and expand K / V with ``repeat_interleave(G, dim=1)``. Not built:
G outside ``GROUP_SIZES`` on a GPU.

Rotary position embeddings: ``kv_append(..., rope=table)`` (``ops.rope_table``; the rule is ``ops/rope.py``'s) is the
append of a rotary layer. It rotates the q and k slices of ``qkv`` in place at positions ``lens[b] + t``, read on the
device, and stores the rotated K (``kernels/rope_bf16.hip``: one launch, bf16 and FP8 caches); the attention call
after it reads the rotated q slice of the same buffer. The attention kernels know nothing of it: the cache simply
holds rotated keys.

Sliding-window attention: ``attention_decode`` / ``attention_extend`` / ``attention_chunk`` take ``window=W``, a local
causal mask. THE RULE (the kernels and the references point here): a query row whose causal limit is ``L`` sees key
``j`` iff ``max(0, L - W) <= j < L``. ``L = lens[b] - T + i + 1`` for row ``i`` of the ``T`` new rows (``lens[b]`` for
``attention_decode``); a grouped row takes the ``L`` of its token. The row therefore sees itself and the ``W - 1`` keys
before it; with one token per position that is Hugging Face Mistral's ``q_pos - k_pos < W``. ``W >= 1`` is a host
``int`` (not a ``bool``), the same for every row of a call; anything else raises. ``window=None`` is the call without
a window, on the kernels without one. A key below a row's lower bound is excluded as a key at or beyond its limit is:
cache rows outside every row's window may hold NaN (bf16) or ``0x7F`` codes and NaN scales (FP8). The launch grid
still comes from ``t_bound`` (``lens`` stays on the device, the step stays capturable); workgroups whose keys all lie
below the window write the empty split record and load nothing, so the K / V stream is bounded by about ``W`` keys
per row block whatever the position. ``W >= t_bound`` can remove no key and launches the kernels without a window.
The routing between the VALU and MFMA forms does not depend on the window. A flat ``KVCache`` still holds every position.

Ring-buffer cache: ``KVCache(..., ring=True)`` holds the last ``capacity`` positions of every row, so a windowed
sequence runs in O(window) memory and to any position. THE RING RULE (the kernels and the references point here):
``capacity`` (``C``) is a positive multiple of ``SPLIT_KEYS`` (256; anything else raises ``ValueError``); ``lens[b]`` is
the ABSOLUTE number of tokens of row ``b`` and is not bounded by ``C``; key ``j`` lives in slot ``j % C``, for K, V and
the FP8 scales alike; the live keys of row ``b`` are ``max(0, lens[b] - C) <= j < lens[b]``, and anything else a slot
might stand for is gone. ``kv_append`` writes position ``lens[b] + t`` to slot ``(lens[b] + t) % C`` and never drops a
row; it needs ``T <= C``; ``rope=table`` rotates by the absolute position, so the table needs ``_bound + T`` rows (not
``capacity``), and the FP8 append still stores exactly ``quantize_rows`` of the (rotated) row. The three attention ops
on a ring require ``window=W`` and ``W + T - 1 <= C`` (``T`` new tokens of the call, 1 for ``attention_decode``), on
every path; either failing raises ``ValueError`` naming both numbers. That condition is the whole safety argument: a
step that appends positions ``L .. L+T-1`` overwrites positions ``L-C .. L+T-1-C``, row 0 of the step sees keys down to
``L + 1 - W``, so nothing seen is overwritten iff ``C >= W + T - 1``. The window rule itself is unchanged. An explicit
``t_bound=`` raises: the grid of a ring launch is a function of ``(W, T, G, B, H)`` only, never of the position. The
kernels keep the absolute 256-aligned split partition and rebase it per batch row on the device at ``base_b =
(max(lens[b] - T + 1 - W, 0) // 256) * 256`` (``lens[b]`` including the new rows): split ``s`` covers absolute keys from
``base_b + 256 s``, and ``ceil((W + T - 1) / 256) + 1`` splits always suffice; the MFMA form applies its ``nsplit`` /
``split_keys`` formula to that span. Every split and every 64-key tile is one contiguous run of slots, so no kernel
takes a modulo per key. A captured step needs no ``pin_bound()`` and carries no empty splits from the position.
``set_lens`` accepts any lengths ``>= 0`` (the slots are taken to hold the last ``C`` positions before each length),
``advance`` does not clamp, ``rewind(n)`` raises for ``n > C - W + 1`` (``W``: the ``window=`` the cache was built with,
as ``GPT.new_cache`` does; 1 without it, the widest limit any window allows), where the needed keys are certainly gone,
and is valid for ``n <= T`` of the step before it (draft-and-verify). ``t_bound`` / ``bound_after`` / ``pin_bound`` keep working for callers that read
them; nothing on the ring path depends on them. The torch path gathers the live slots into absolute order and applies
the masked softmax above. Positions up to 2^24 are covered. ``ring=False`` is the cache as it was: same launches, same
bits. Not built: a ring without a window, a capacity that is no multiple of 256.

Paged cache: ``KVCache(..., pool=PagePool(...))`` keeps its rows in pages of a pool that several caches share, so memory
follows the use, not the capacity, and sequences can share a prefix. THE PAGE RULE (the kernels, ``kfamd_kernels.h`` and
the documents point here): a page holds ``PAGE = 256`` consecutive positions of one sequence, for all K / V heads of one
layer (``PAGE`` is the kernels' ``SPLIT_KEYS``). ``PagePool(n_layers, H, D, n_pages, device, dtype)`` owns per layer
``k`` / ``v`` ``[n_pages, H, 256, D]`` (an FP8 pool also ``k_scale`` / ``v_scale`` ``[n_pages, H, 256]``), a host free
list and a host reference count per page. ``capacity`` of a paged cache is a positive multiple of 256 (anything else
raises ``ValueError``): the longest a row may grow, not memory. ``cache.page_table`` is a device ``int32 [B, capacity //
256]`` with ``-1`` for "no page"; the host keeps an exact mirror of it and of every row's length, which ``advance``,
``rewind``, ``set_lens`` and ``reset`` keep exact (so: no device-side change of ``lens`` behind the cache's back, except
a captured step's, whose replay wrapper tells the mirror). Key ``j`` of row ``b`` lives in page ``page_table[b, j //
256]`` at row ``j % 256``, for K, V and the FP8 scales alike. ``lens``, ``t_bound``, ``lens_after``, ``bound_after``,
``pin_bound`` and the split workspaces mean exactly what they mean on a flat cache. ``cache.reserve(T)`` makes positions
``0 .. len + T - 1`` present and the last T of them writable (a page shared with another cache is copied first);
``GPT.prefill`` / ``decode_step`` / ``extend`` and the graphed steps call it, a direct user of ``kv_append`` calls it
themselves: ``kv_append`` drops a position at or beyond the capacity or without a page, without a store (the rotary
form then leaves that row unrotated). ``cache.fork(S)`` gives ``B * S`` rows that share the full pages; ``release()``
gives the pages back. The kernels keep the flat launch's absolute 256-aligned split partition, tile order and
arithmetic: a VALU workgroup reads its one page id as a block-uniform scalar after the empty-split return, the MFMA
form the page of each 64-key tile, whose buffer descriptors end at the row that holds key ``len - 1`` (rows beyond read
as zeros). So a paged launch equals the flat launch bit for bit on the same logical contents. A page id read on the
device is clamped into ``[0, n_pages - 1]`` before a load and checked before a store. Pages no row owns, and rows at or
beyond ``len`` in an owned page, may hold NaN (bf16) or ``0x7F`` codes and NaN scales (FP8). ``window=`` on a paged cache
raises ``ValueError``, and so does ``ring=True`` with ``pool=``. The torch path gathers each row's pages into a ``[B, H,
capacity, D]`` view (absent pages as zeros) and runs the flat references. ``pool=None`` is the cache as it was: same
launches, same bits. Not built: paged with a window or a ring, page sizes other than 256.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib

HEAD_DIMS = (64, 128)
FP8 = torch.float8_e4m3fn  # the 8-bit cache's code type (OCP e4m3fn: finite maximum 448, code 0x7E)
FP8_MAX = 448.0
CACHE_DTYPES = (torch.bfloat16, FP8)  # what the kernels read
MAX_EXTEND_ROWS = 16  # query ROWS per attention_extend call and (batch, K / V head): T * G of them, T tokens at G = 1
GROUP_SIZES = (1, 2, 4, 8, 16)  # query heads per K / V head the kernels take
# attention_decode / attention_extend with G > 1 query heads per K / V head: from this many rows (T * G) per K / V
# head on they run the MFMA form (attention_chunk's kernel) instead of the VALU form; None: never. G = 1 never
# moves. Measured (profiles/gqa; tools/decode_bench.py --steps gqa; D = 128, 8 x 16 query heads, 2048 / 4096 keys,
# bf16 and FP8): at 8 rows the MFMA form is 1.5 - 2.0x faster, at 16 rows 2.5 - 3.7x, every case beyond the
# blocks' spread; below 8 rows the forms were not compared and the VALU form stays.
GQA_MFMA_MIN_ROWS: int | None = 8
PAGE = 256  # positions per page of a paged cache: the kernels' SPLIT_KEYS
RING_ALIGN = 256  # a ring's capacity is a multiple of the kernels' SPLIT_KEYS (a constant: importing needs no library)


def _gqa_mfma(T: int, G: int) -> bool:
    return G > 1 and GQA_MFMA_MIN_ROWS is not None and T * G >= GQA_MFMA_MIN_ROWS


_split_keys: int | None = None


def split_keys() -> int:
    """Keys per split of the decode attention kernel (``SPLIT_KEYS``)."""
    global _split_keys
    if _split_keys is None:
        _split_keys = int(_lib.lib().kfamd_attn_decode_split_keys())
    return _split_keys


def __getattr__(name):  # SPLIT_KEYS: read from the library on first use (importing needs no GPU)
    if name == "SPLIT_KEYS":
        return split_keys()
    raise AttributeError(name)


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _native(t: torch.Tensor) -> bool:
    """GPU tensors run the HIP kernels unless ops.torch_reference() is active (the A/B baseline)."""
    from . import native_enabled
    return t.is_cuda and native_enabled()


def _ll(*vals) -> "ctypes.Array":
    return (ctypes.c_longlong * len(vals))(*(int(v) for v in vals))


def _group(what: str, q_heads: int, cache: "KVCache", native: bool) -> int:
    """G = q_heads / cache.H of a call; on the kernels' path one of GROUP_SIZES."""
    G, rem = divmod(int(q_heads), cache.H)
    if rem or G < 1:
        raise ValueError(f"{what}: the query head count must be a multiple of the cache's {cache.H} K / V heads, "
                         f"got {q_heads}")
    if native and G not in GROUP_SIZES:
        raise ValueError(f"{what}: {G} query heads per K / V head; one of {GROUP_SIZES} expected on a GPU")
    return G


def _expand_kv(k, v, G: int):
    """K, V ``[B, Hkv, ...]`` with every head repeated G times: what the torch reference attends."""
    return (k, v) if G == 1 else (k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1))


def _entry(name: str, cache: "KVCache", layer: int):
    """The entry point ``name`` for the cache's dtype: (function, the scale tensors an FP8 cache adds to the
    pointers and strides, the tag of its error messages)."""
    if cache.fp8:
        return getattr(_lib.lib(), name + "_fp8"), (cache.k_scale[layer], cache.v_scale[layer]), "fp8 "
    return getattr(_lib.lib(), name + "_bf16"), (), ""


def quantize_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The FP8 cache's format in plain torch: rows ``x [..., D]`` -> ``(codes [..., D] float8_e4m3fn, scale
    [...] fp32)`` with ``scale = max|x| / 448`` in fp32 (1 for an all-zero row) and ``code =
    RNE_e4m3(clamp(x / scale, -448, 448))``. A non-finite input is out of contract."""
    x = x.float()
    amax = x.abs().amax(-1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    codes = (x / scale.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return codes, scale


def dequantize_rows(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``codes * scale`` in fp32: the values an FP8 cache row stands for."""
    return codes.float() * scale.float().unsqueeze(-1)


class PagePool:
    """The memory of paged caches (the module docstring's page rule): per layer ``k`` / ``v`` ``[n_pages, H, 256, D]``
    (``dtype=torch.float8_e4m3fn``: codes, and ``k_scale`` / ``v_scale`` ``[n_pages, H, 256]`` fp32), a host free list
    and a host reference count per page. Pages are handed out lowest id first. Every ``KVCache(..., pool=pool)`` on it
    must match ``n_layers``, ``H``, ``D``, the dtype and the device."""

    def __init__(self, n_layers: int, H: int, D: int, n_pages: int, device=None, dtype: torch.dtype = torch.bfloat16):
        if min(n_layers, H, D, n_pages) < 1:
            raise ValueError("PagePool: positive sizes expected")
        self.n_layers, self.H, self.D, self.n_pages = n_layers, H, D, n_pages
        self.device, self.dtype = torch.device(device if device is not None else "cpu"), dtype
        self.k = [torch.zeros(n_pages, H, PAGE, D, device=self.device, dtype=dtype) for _ in range(n_layers)]
        self.v = [torch.zeros(n_pages, H, PAGE, D, device=self.device, dtype=dtype) for _ in range(n_layers)]
        self.k_scale = self.v_scale = None
        if dtype == FP8:
            self.k_scale = [torch.zeros(n_pages, H, PAGE, device=self.device) for _ in range(n_layers)]
            self.v_scale = [torch.zeros(n_pages, H, PAGE, device=self.device) for _ in range(n_layers)]
        self._free = list(range(n_pages))  # taken from the front
        self._ref = [0] * n_pages

    @property
    def pages_total(self) -> int:
        return self.n_pages

    @property
    def pages_free(self) -> int:
        return len(self._free)

    @property
    def page_bytes(self) -> int:
        """Bytes of one page over all layers: K and V, and the scales of an FP8 pool."""
        per = self.H * PAGE * (self.D * self.k[0].element_size() + (4 if self.dtype == FP8 else 0))
        return 2 * self.n_layers * per

    @property
    def nbytes(self) -> int:
        """Bytes of device memory the pool holds, whatever is in use."""
        return self.n_pages * self.page_bytes

    def _take(self, n: int) -> list[int]:
        """n pages from the free list, each with one reference; the caller has checked ``pages_free``."""
        pages, self._free = self._free[:n], self._free[n:]
        for p in pages:
            self._ref[p] = 1
        return pages

    def _drop(self, page: int) -> None:
        self._ref[page] -= 1
        if self._ref[page] == 0:
            self._free.append(page)

    def _copy(self, src: int, dst: int) -> None:
        """The device copy of page ``src`` into page ``dst`` in every layer, scales included."""
        for ts in (self.k, self.v, self.k_scale or [], self.v_scale or []):
            for t in ts:
                if t.dtype == FP8:
                    t.view(torch.uint8)[dst].copy_(t.view(torch.uint8)[src])
                else:
                    t[dst].copy_(t[src])


class KVCache:
    """Per-layer K / V ``[B, H, capacity, D]``, device ``lens`` (int32 [B]), host ``t_bound``. ``H`` is the
    number of K / V heads: a grouped-query model's cache holds ``n_kv_heads`` and the attention functions take a
    ``q`` of ``G * H`` heads.
    ``dtype=torch.float8_e4m3fn``: ``k`` / ``v`` hold codes and ``k_scale`` / ``v_scale`` ``[B, H, capacity]``
    fp32 the per-row scales (``None`` for every other dtype).
    ``ring=True``: a ring buffer of the last ``capacity`` positions (the module docstring's ring rule): ``capacity`` a
    multiple of 256, ``lens`` absolute and unbounded, key ``j`` in slot ``j % capacity``. ``window``: optional, the
    window the cache will be attended with: only ``rewind`` reads it, for its limit ``capacity - window + 1`` (without
    it the limit is ``capacity``, what a window of 1 allows). No call changes it.
    ``pool=PagePool(...)``: a paged cache on that pool (the module docstring's page rule): ``capacity`` is a multiple of
    256 and bounds a row's length, not memory; ``k`` / ``v`` (and the scales) ARE the pool's tensors ``[n_pages, H, 256,
    D]``, ``page_table`` the device ``int32 [B, capacity // 256]``; the device and the dtype are the pool's. ``reserve``,
    ``fork`` and ``release`` exist on a paged cache only."""

    def __init__(self, n_layers: int, B: int, H: int, D: int, capacity: int, device=None,
                 dtype: torch.dtype | None = None, ring: bool = False, window: int | None = None,
                 pool: "PagePool | None" = None):
        if min(n_layers, B, H, D, capacity) < 1:
            raise ValueError("KVCache: positive sizes expected")
        if ring and capacity % RING_ALIGN:
            raise ValueError(f"KVCache(ring=True): the capacity must be a multiple of {RING_ALIGN}, got {capacity}")
        if pool is not None:
            if ring:
                raise ValueError("KVCache: ring=True cannot be combined with pool= (a paged ring is not built)")
            if capacity % PAGE:
                raise ValueError(f"KVCache(pool=...): the capacity must be a multiple of {PAGE}, got {capacity}")
            if (pool.n_layers, pool.H, pool.D) != (n_layers, H, D):
                raise ValueError(f"KVCache(pool=...): the pool holds {pool.n_layers} layers of {pool.H} heads x {pool.D}, "
                                 f"got {n_layers} layers of {H} x {D}")
            if dtype is not None and dtype != pool.dtype:
                raise ValueError(f"KVCache(pool=...): the pool's dtype is {pool.dtype}, got {dtype}")
            if device is not None and torch.device(device).type != pool.device.type:
                raise ValueError(f"KVCache(pool=...): the pool lives on {pool.device}, got {device}")
            device, dtype = pool.device, pool.dtype
        dtype = torch.bfloat16 if dtype is None else dtype
        self.ring, self.pool = bool(ring), pool
        self.window = _check_window("KVCache", window) if ring else None
        self.n_layers, self.B, self.H, self.D, self.capacity = n_layers, B, H, D, capacity
        self.device, self.dtype = torch.device(device if device is not None else "cpu"), dtype
        self.k_scale = self.v_scale = None
        if pool is not None:  # the pool's tensors: the page stride stands where the batch stride stands
            self.k, self.v, self.k_scale, self.v_scale = pool.k, pool.v, pool.k_scale, pool.v_scale
            self.page_table = torch.full((B, capacity // PAGE), -1, device=self.device, dtype=torch.int32)
            self._table = [[-1] * (capacity // PAGE) for _ in range(B)]  # the host mirror of page_table
            self._hlen = [0] * B  # and of lens
        else:
            self.k = [torch.zeros(B, H, capacity, D, device=self.device, dtype=dtype) for _ in range(n_layers)]
            self.v = [torch.zeros(B, H, capacity, D, device=self.device, dtype=dtype) for _ in range(n_layers)]
            if dtype == FP8:
                self.k_scale = [torch.zeros(B, H, capacity, device=self.device) for _ in range(n_layers)]
                self.v_scale = [torch.zeros(B, H, capacity, device=self.device) for _ in range(n_layers)]
        self.lens = torch.zeros(B, device=self.device, dtype=torch.int32)
        self._lens_after = torch.zeros(B, device=self.device, dtype=torch.int32)  # lens_after()'s buffer
        self._bound, self._pinned = 0, False
        self.workspace = None
        self.extend_workspace = None  # attention_extend's, allocated on its first use
        self.chunk_workspace = None  # attention_chunk's, allocated on its first use, grown when a call needs more
        if self.ring:  # the ring's workspaces follow the window: all three are allocated on first use
            return
        if self.device.type == "cuda" and dtype in CACHE_DTYPES and D in HEAD_DIMS:  # the kernels' shapes
            nbytes = _lib.lib().kfamd_attn_decode_workspace(B, H, D, capacity)
            self.workspace = torch.empty(max(int(nbytes), 16), device=self.device, dtype=torch.uint8)

    @property
    def fp8(self) -> bool:
        return self.dtype == FP8

    @property
    def nbytes(self) -> int:
        """Bytes this cache holds: K / V (codes), the scales of an FP8 cache, and the attention workspaces
        allocated so far. ``lens`` and its step buffer (8 bytes per batch row) are not counted. A paged cache: the page
        table, the workspaces and ``pages_held * pool.page_bytes``; a page shared between caches (or between rows of
        one) is counted once in each cache that holds it, so the sum over caches can exceed ``pool.nbytes``."""
        if self.pool is not None:
            ts = [self.page_table, self.workspace, self.extend_workspace, self.chunk_workspace]
            return (sum(t.numel() * t.element_size() for t in ts if t is not None)
                    + self.pages_held * self.pool.page_bytes)
        ts = [*self.k, *self.v, *(self.k_scale or []), *(self.v_scale or []), self.workspace, self.extend_workspace,
              self.chunk_workspace]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    @property
    def t_bound(self) -> int:
        """Host-side upper bound of every ``lens[b]`` (sizes the attention grid)."""
        return self.capacity if self._pinned else min(self._bound, self.capacity)

    def lens_after(self, T: int = 1) -> torch.Tensor:
        """``lens + T`` on the device (one buffer per cache, capturable): the lengths a step that
        appends T rows per batch row hands to its attention."""
        return torch.add(self.lens, T, out=self._lens_after)

    def bound_after(self, T: int = 1) -> int:
        """The host bound that goes with ``lens_after(T)``."""
        return self.capacity if self._pinned else min(self._bound + T, self.capacity)

    def advance(self, T: int = 1) -> None:
        """``lens += T`` on the device (capturable); the host bound follows."""
        self.lens.add_(T)
        self._bound = self._bound + T if self.ring else min(self._bound + T, self.capacity)
        if self.pool is not None:
            self._hlen = [n + T for n in self._hlen]

    def set_lens(self, lens) -> None:
        """Set per-row lengths from the host (a sync: not for a captured step)."""
        vals = [int(x) for x in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
        if self.ring:  # absolute lengths: the slots are taken to hold the last `capacity` positions before each
            if len(vals) != self.B or min(vals) < 0 or max(vals) >= 2 ** 31:
                raise ValueError(f"set_lens: {self.B} lengths >= 0 expected")
        elif len(vals) != self.B or min(vals) < 0 or max(vals) > self.capacity:
            raise ValueError(f"set_lens: {self.B} lengths in 0..{self.capacity} expected")
        self.lens.copy_(torch.tensor(vals, dtype=torch.int32))
        self._bound = max(vals)
        if self.pool is not None:  # pages are not touched: reserve(0) makes the new lengths present
            self._hlen = vals

    def pin_bound(self) -> None:
        """Size the attention grid for the whole capacity: what a step captured once must use."""
        self._pinned = True

    def rewind(self, n: int) -> None:
        """``lens -= n`` on the device, clamped at 0 (capturable); the host bound follows (a pinned bound
        stays pinned). The rows beyond ``lens`` stay in memory: dead by the kernels' contract, overwritten
        by the next append."""
        if n < 0:
            raise ValueError("rewind: n >= 0 expected")
        if self.ring and n > self.capacity - (self.window or 1) + 1:
            raise ValueError(f"rewind: on a ring of capacity {self.capacity} with window {self.window or 1} at most "
                             f"{self.capacity - (self.window or 1) + 1} rows can be dropped (the keys before them are "
                             f"overwritten), got {n}")
        self.lens.sub_(n).clamp_(min=0)
        self._bound = max(self._bound - n, 0)
        if self.pool is not None:  # the pages stay held; a shared one is copied by the reserve before the next append
            self._hlen = [max(m - n, 0) for m in self._hlen]

    def reset(self) -> None:
        """Lengths to 0. A paged cache also gives its pages back (``release``)."""
        if self.pool is not None:
            self.release()
            return
        self.lens.zero_()
        self._bound = 0

    # ---- a paged cache's pages (the module docstring's page rule): plain host code, no kernel ----------------------
    def _paged(self, what: str) -> "PagePool":
        if self.pool is None:
            raise ValueError(f"{what}: a paged cache expected (KVCache(..., pool=PagePool(...)))")
        return self.pool

    @property
    def pages_held(self) -> int:
        """Table entries that name a page (a page two rows share counts twice)."""
        self._paged("pages_held")
        return sum(p >= 0 for row in self._table for p in row)

    def _push_table(self) -> None:
        """The host mirror to the device: one host-to-device copy."""
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("KVCache: the page table cannot change inside a stream capture: reserve the whole "
                               "length before capturing")
        self.page_table.copy_(torch.tensor(self._table, dtype=torch.int32))

    def reserve(self, T: int = 1) -> None:
        """Make positions ``0 .. len[b] + T - 1`` of every row present (clamped to the capacity) and the T positions
        from ``len[b]`` on writable: missing pages come from the pool's free list, and a page about to be written that
        another holder shares (reference count above 1) is replaced by a private copy first (copy-on-write: a device
        copy of that page in every layer, scales included). Raises ``RuntimeError`` naming the pages needed and the
        pages free when the pool is short, and changes nothing then. Inside a stream capture it raises if it would
        have to change the table: a captured generation reserves its whole length before the capture. The lengths are
        the host mirror's (``advance`` / ``rewind`` / ``set_lens`` / ``reset`` keep it exact)."""
        pool = self._paged("reserve")
        if T < 0:
            raise ValueError("reserve: T >= 0 expected")
        missing, shared = [], []  # (row, column) without a page; with a shared page about to be written
        for b, n in enumerate(self._hlen):
            end = min(n + T, self.capacity)
            first_w = min(n, self.capacity) // PAGE  # the first column the step writes
            for c in range(-(-end // PAGE)):
                p = self._table[b][c]
                if p < 0:
                    missing.append((b, c))
                elif T > 0 and c >= first_w and n < end and pool._ref[p] > 1:
                    shared.append((b, c))
        need = len(missing) + len(shared)
        if need == 0:
            return
        if need > pool.pages_free:
            raise RuntimeError(f"KVCache.reserve: {need} pages needed, {pool.pages_free} free (pool of "
                               f"{pool.pages_total})")
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("KVCache.reserve: the page table would change inside a stream capture: reserve the "
                               "whole length before capturing")
        pages = pool._take(need)
        for (b, c), p in zip(missing, pages):
            self._table[b][c] = p
        for (b, c), p in zip(shared, pages[len(missing):]):
            old = self._table[b][c]
            pool._copy(old, p)
            pool._drop(old)
            self._table[b][c] = p
        self._push_table()

    def fork(self, S: int, release: bool = False) -> "KVCache":
        """A new cache of ``B * S`` rows on the same pool, row ``b * S + s`` holding the contents of row ``b``: the full
        pages are shared (reference count + 1 per child), the last partial page, if any, is copied into a fresh page per
        child; ``lens`` is copied. The parent stays valid; whoever appends to a shared page next gets a private copy from
        ``reserve``. Raises ``RuntimeError`` (nothing changed) when the pool lacks the pages for the partial copies.
        ``release=True``: fork and release the parent in one move: each row's last child takes over the parent's own
        references (its partial page included, no copy), so ``S - 1`` partial copies per row suffice and no page is
        held twice meanwhile; the parent ends empty, as after ``release()``."""
        pool = self._paged("fork")
        if isinstance(S, bool) or not isinstance(S, int) or S < 1:
            raise ValueError(f"fork: S >= 1 expected, got {S!r}")
        partial = [b for b, n in enumerate(self._hlen) if n % PAGE and n < self.capacity]
        for b, n in enumerate(self._hlen):
            if any(p < 0 for p in self._table[b][:-(-min(n, self.capacity) // PAGE)]):
                raise RuntimeError(f"fork: row {b} has positions without a page (reserve(0) after set_lens)")
        copies = len(partial) * (S - 1 if release else S)
        if copies > pool.pages_free:
            raise RuntimeError(f"KVCache.fork: {copies} pages needed, {pool.pages_free} free (pool of "
                               f"{pool.pages_total})")
        child = KVCache(self.n_layers, self.B * S, self.H, self.D, self.capacity, pool=pool)
        fresh = iter(pool._take(copies))
        for b, n in enumerate(self._hlen):
            n = min(n, self.capacity)
            for s in range(S - 1 if release else S):
                row = child._table[b * S + s]
                for c in range(n // PAGE):
                    row[c] = self._table[b][c]
                    pool._ref[row[c]] += 1
                if n % PAGE:
                    row[n // PAGE] = next(fresh)
                    pool._copy(self._table[b][n // PAGE], row[n // PAGE])
            if release:  # the parent's row, pages reserved ahead included, passes to the last child as it is
                child._table[b * S + S - 1], self._table[b] = self._table[b], [-1] * len(self._table[b])
        child._hlen = [n for n in self._hlen for _ in range(S)]
        child.lens.copy_(self.lens.repeat_interleave(S))
        child._bound, child._pinned = self._bound, self._pinned
        child._push_table()
        if release:
            self.release()  # nothing left to drop: lengths to 0, the empty table to the device
        return child

    def release(self) -> None:
        """Drop the cache's references (a page whose count reaches 0 returns to the pool's free list) and set the
        lengths to 0. The cache can be filled again."""
        pool = self._paged("release")
        for row in self._table:
            for c, p in enumerate(row):
                if p >= 0:
                    pool._drop(p)
                    row[c] = -1
        self._hlen = [0] * self.B
        self.lens.zero_()
        self._bound = 0
        self._push_table()

    def _ring_ws(self, attr: str, nbytes: int, what: str) -> torch.Tensor:
        """A ring's workspace ``attr`` of at least ``nbytes`` (the size follows the window and the row count, never the
        position): allocated on first use, replaced by a larger one when a call needs more, never inside a capture."""
        ws = getattr(self, attr)
        if ws is None or ws.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{what}: run one step before capturing (the workspace is allocated on first use)")
            ws = torch.empty(max(int(nbytes), 16), device=self.device, dtype=torch.uint8)
            setattr(self, attr, ws)
        return ws

    def _extend_ws(self, window: int | None = None) -> torch.Tensor:
        """attention_extend's split workspace: MAX_EXTEND_ROWS times decode's (rows of a K / V head, whatever
        the group size), allocated on first use (outside any capture) and kept. A ring's: for the splits of
        ``window`` and MAX_EXTEND_ROWS tokens."""
        if self.ring:
            return self._ring_ws("extend_workspace", _lib.lib().kfamd_attn_extend_ring_workspace(
                self.B, self.H, 1, self.D, MAX_EXTEND_ROWS, window), "attention_extend")
        if self.extend_workspace is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("attention_extend: run one step before capturing (the workspace is allocated "
                                   "on first use)")
            nbytes = _lib.lib().kfamd_attn_extend_workspace(self.B, self.H, self.D, MAX_EXTEND_ROWS, self.capacity)
            self.extend_workspace = torch.empty(max(int(nbytes), 16), device=self.device, dtype=torch.uint8)
        return self.extend_workspace

    def _chunk_ws(self, T: int, G: int = 1, window: int | None = None) -> torch.Tensor:
        """attention_chunk's split workspace for T tokens of G query heads per K / V head:
        ``kfamd_attn_chunk_gqa_workspace`` at the capacity (the split count does not fall when t_bound grows, so
        it serves every t_bound), allocated on first use and replaced by a larger one when a later call needs
        more, never inside a capture."""
        L = _lib.lib()
        if self.ring:  # the split count comes from the window and T
            return self._ring_ws("chunk_workspace", L.kfamd_attn_chunk_ring_workspace(self.B, self.H, G, self.D, T,
                                                                                      window), "attention_chunk")
        nbytes = int(L.kfamd_attn_chunk_workspace(self.B, self.H, self.D, T, self.capacity) if G == 1 else
                     L.kfamd_attn_chunk_gqa_workspace(self.B, self.H, G, self.D, T, self.capacity))
        if self.chunk_workspace is None or self.chunk_workspace.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"attention_chunk: run one step of T = {T} rows before capturing (the workspace "
                                   "is allocated on first use)")
            self.chunk_workspace = torch.empty(max(nbytes, 16), device=self.device, dtype=torch.uint8)
        return self.chunk_workspace


def kv_append(qkv: torch.Tensor, cache: KVCache, layer: int, q_heads: int | None = None,
              rope: torch.Tensor | None = None) -> None:
    """K, V rows of the fused QKV activation ``[B, T, 3*H*D]`` -> cache rows ``lens[b] .. lens[b]+T-1``
    (rows at or beyond the capacity are dropped). ``lens`` is not advanced. ``q_heads=Hq`` (default: the
    cache's H): a grouped-query layer's activation ``[B, T, (Hq + 2*H)*D]``, ``q: Hq*D | k: H*D | v: H*D``.

    ``rope=table`` (``ops.rope_table``, fp32 ``[max_pos >= capacity, D]``): the append of a rotary layer. The q and k
    slices of ``qkv`` are rotated IN PLACE for positions ``lens[b] + t`` (the rule of ``ops/rope.py``), and the
    rotated K row and the V row are stored; an FP8 cache quantises the rotated K as rounded to the activation's
    dtype. Rows at or beyond the capacity are neither appended nor rotated. On a GPU it is one launch
    (``kfamd_kv_append_rope_*``); on the torch path rotate, then the append below. ``rope=None``: no rotation."""
    B, H, D = cache.B, cache.H, cache.D
    Hq = H if q_heads is None else int(q_heads)
    native = _native(qkv)
    G = _group("kv_append", Hq, cache, native)
    if qkv.dim() != 3 or qkv.shape[0] != B or qkv.shape[2] != (Hq + 2 * H) * D:
        raise ValueError(f"kv_append: qkv [B={B}, T, {(Hq + 2 * H) * D}] expected, got {tuple(qkv.shape)}")
    if cache.ring and qkv.shape[1] > cache.capacity:
        raise ValueError(f"kv_append: T = {qkv.shape[1]} rows exceed the ring's capacity {cache.capacity}")
    if rope is not None:
        # a ring rotates by the absolute position: a table row for every position of the step, whatever the capacity
        # (a paged cache's capacity is rounded up to whole pages: the table covers the positions of the step)
        need = (cache._bound + qkv.shape[1] if cache.ring else
                min(cache._bound + qkv.shape[1], cache.capacity) if cache.pool is not None else cache.capacity)
        if rope.dim() != 2 or rope.shape[1] != D or rope.shape[0] < need or rope.dtype != torch.float32:
            raise ValueError(f"kv_append: rope must be an fp32 [max_pos >= {need}, {D}] table, got "
                             f"{tuple(rope.shape)} {rope.dtype}")
        if native:
            _kv_append_rope_native(qkv, cache, layer, Hq, rope)
            return
        from .rope import rotate_torch  # rows at or beyond the capacity have no table row here: left as they are
        qkv.copy_(rotate_torch(qkv, rope if cache.ring else rope[:cache.capacity], Hq, H, positions=cache.lens))
        # (a paged row without a page is left unrotated by the kernel and rotated here: reserve() first, either way)
    if native:
        _kv_append_native(qkv, cache, layer, Hq, G)
    else:
        _kv_append_torch(qkv, cache, layer, Hq)


def _kv_append_torch(qkv, cache: KVCache, layer: int, Hq: int) -> None:
    """The append on torch ops (CPU tensors / ops.torch_reference()); a rotary layer's qkv is already rotated."""
    B, H, D, T = cache.B, cache.H, cache.D, qkv.shape[1]
    k, v = cache.k[layer], cache.v[layer]
    # [B, T, 3, H, D]: slot 0 the last H query heads (unused), slots 1 and 2 k and v
    x = qkv[:, :, (Hq - H) * D:].reshape(B, T, 3, H, D)
    if cache.pool is not None:
        _kv_append_paged_torch(x, cache, layer)
        return
    if cache.fp8:
        _kv_append_fp8_torch(x, cache, layer)
        return
    rows = cache.lens.long().unsqueeze(1) + torch.arange(T, device=qkv.device).unsqueeze(0)  # [B, T]
    if cache.ring:
        rows = rows % cache.capacity  # T <= capacity: no slot twice
    if cache.ring or cache._bound + T <= cache.capacity:  # no row can fall off the end: one index_put per tensor
        bidx = torch.arange(B, device=qkv.device).unsqueeze(1).expand(B, T)
        k[bidx, :, rows] = x[:, :, 1].to(k.dtype)
        v[bidx, :, rows] = x[:, :, 2].to(v.dtype)
        return
    for b in range(B):
        keep = rows[b] < cache.capacity
        k[b].index_copy_(1, rows[b][keep], x[b, keep, 1].transpose(0, 1).to(k.dtype))
        v[b].index_copy_(1, rows[b][keep], x[b, keep, 2].transpose(0, 1).to(v.dtype))


def _page_args(cache: KVCache) -> tuple:
    """What a paged entry point takes before the stream: the device table, its row stride, the pool's page count."""
    return cache.page_table.data_ptr(), cache.page_table.stride(0), cache.pool.n_pages


def _kv_append_paged_torch(x, cache: KVCache, layer: int) -> None:
    """The torch form of the paged append (the page rule): position ``lens[b] + t`` to page ``page_table[b, p // 256]``,
    row ``p % 256``; a position at or beyond the capacity or without a page is dropped. ``x [B, T, 3, H, D]``."""
    B, T = x.shape[:2]
    pos = cache.lens.long().unsqueeze(1) + torch.arange(T, device=x.device).unsqueeze(0)  # [B, T]
    page = cache.page_table.long().gather(1, (pos // PAGE).clamp(0, cache.page_table.shape[1] - 1))
    keep = (pos >= 0) & (pos < cache.capacity) & (page >= 0)
    pg, row = page[keep], (pos % PAGE)[keep]  # [N]
    for s, t, sc in ((1, cache.k[layer], cache.k_scale), (2, cache.v[layer], cache.v_scale)):
        rows = x[:, :, s][keep]  # [N, H, D]
        if cache.fp8:
            codes, scale = quantize_rows(rows)
            t.view(torch.uint8)[pg, :, row] = codes.view(torch.uint8)
            sc[layer][pg, :, row] = scale
        else:
            t[pg, :, row] = rows.to(t.dtype)


def _kv_append_native(qkv, cache: KVCache, layer: int, Hq: int, G: int) -> None:
    """The append launch without rotation (``kernels/attn_kv.hip``)."""
    B, H, D, T = cache.B, cache.H, cache.D, qkv.shape[1]
    k, v = cache.k[layer], cache.v[layer]
    if qkv.dtype != torch.bfloat16 or qkv.stride(2) != 1:
        raise ValueError("kv_append: bf16 qkv with a contiguous last dim expected")
    if cache.fp8 and D not in HEAD_DIMS:
        raise ValueError(f"kv_append: head dim in {HEAD_DIMS} expected for an FP8 cache on a GPU, got {D}")
    paged = cache.pool is not None
    fn, scales, tag = _entry("kfamd_kv_append_paged" if paged else "kfamd_kv_append_ring" if cache.ring else
                             "kfamd_kv_append" if G == 1 else "kfamd_kv_append_gqa", cache, layer)
    # the ring and paged forms take the grouped signature; a paged cache's first stride is the page stride
    rc = fn(qkv.data_ptr(), k.data_ptr(), v.data_ptr(), *(s.data_ptr() for s in scales), cache.lens.data_ptr(), B, T,
            *((H,) if G == 1 and not cache.ring and not paged else (Hq, H)), D, cache.capacity, qkv.stride(0),
            qkv.stride(1), _ll(*k.stride()[:3], *v.stride()[:3], *(n for s in scales for n in s.stride()[:2])),
            *(_page_args(cache) if paged else ()), _stream_ptr(qkv))
    _lib.check(rc, f"kv_append[{tag}B={B} T={T} Hq={Hq} H={H} D={D}]")


def _kv_append_rope_native(qkv, cache: KVCache, layer: int, Hq: int, rope: torch.Tensor) -> None:
    """The fused rotate-and-append launch (``kernels/rope_bf16.hip``); the grouped signature covers G = 1."""
    B, H, D, T = cache.B, cache.H, cache.D, qkv.shape[1]
    k, v = cache.k[layer], cache.v[layer]
    if qkv.dtype != torch.bfloat16 or qkv.stride(2) != 1:
        raise ValueError("kv_append: bf16 qkv with a contiguous last dim expected")
    if D not in HEAD_DIMS or k.dtype not in CACHE_DTYPES:
        raise ValueError(f"kv_append(rope=...): head dim in {HEAD_DIMS} and a bf16 or float8_e4m3fn cache expected on "
                         f"a GPU, got {D}, {k.dtype}")
    if not rope.is_cuda or rope.device != qkv.device or not rope.is_contiguous():
        raise ValueError("kv_append: rope must be a contiguous table on the activation's device")
    paged = cache.pool is not None
    fn, scales, tag = _entry("kfamd_kv_append_rope_paged" if paged else "kfamd_kv_append_rope_ring" if cache.ring else
                             "kfamd_kv_append_rope", cache, layer)
    rc = fn(qkv.data_ptr(), k.data_ptr(), v.data_ptr(), *(s.data_ptr() for s in scales), cache.lens.data_ptr(),
            rope.data_ptr(), rope.shape[0], B, T, Hq, H, D, cache.capacity, qkv.stride(0), qkv.stride(1),
            _ll(*k.stride()[:3], *v.stride()[:3], *(n for s in scales for n in s.stride()[:2])),
            *(_page_args(cache) if paged else ()), _stream_ptr(qkv))
    _lib.check(rc, f"kv_append[rope {tag}B={B} T={T} Hq={Hq} H={H} D={D}]")


def _kv_append_fp8_torch(x, cache: KVCache, layer: int) -> None:
    """The torch form of the quantising append: ``quantize_rows`` of the K / V rows, written through uint8
    views (torch has no index_copy for float8). Rows at or beyond the capacity are dropped."""
    B, T = x.shape[:2]
    rows = cache.lens.long().unsqueeze(1) + torch.arange(T, device=x.device).unsqueeze(0)  # [B, T]
    if cache.ring:
        rows = rows % cache.capacity  # every row has a slot
    for s, codes, scales in ((1, cache.k[layer], cache.k_scale[layer]), (2, cache.v[layer], cache.v_scale[layer])):
        c, sc = quantize_rows(x[:, :, s])  # [B, T, H, D], [B, T, H]
        c = c.view(torch.uint8)
        for b in range(B):
            keep = rows[b] < cache.capacity
            codes[b].view(torch.uint8).index_copy_(1, rows[b][keep], c[b, keep].transpose(0, 1))
            scales[b].index_copy_(1, rows[b][keep], sc[b, keep].transpose(0, 1))


def _dequantized_prefix(cache: KVCache, layer: int, lens, n: int, dtype, kv=None):
    """K, V of an FP8 cache's first n rows as ``dtype`` tensors, the rows at or beyond ``lens[b]`` zeroed
    (dead codes and scales may be NaN): what the torch reference attends. ``kv``: ``(k, v, k_scale, v_scale)`` in flat
    ``[B, H, capacity, ...]`` order instead of the cache's own tensors (a paged cache's gathered view)."""
    ck, cv, cks, cvs = kv if kv is not None else (cache.k[layer], cache.v[layer], cache.k_scale[layer],
                                                  cache.v_scale[layer])
    live = (torch.arange(n, device=lens.device).view(1, 1, n) < lens.view(-1, 1, 1)).unsqueeze(-1)
    zero = torch.zeros((), device=lens.device)
    k = torch.where(live, dequantize_rows(ck[:, :, :n], cks[:, :, :n]), zero)
    v = torch.where(live, dequantize_rows(cv[:, :, :n], cvs[:, :, :n]), zero)
    return k.to(dtype), v.to(dtype)


def _paged_view(cache: KVCache, layer: int):
    """The torch path's view of a paged cache (the page rule): ``(k, v, k_scale, v_scale)`` with every row's pages
    gathered into flat ``[B, H, capacity, D]`` / ``[B, H, capacity]`` order (the scales ``None`` for a bf16 cache).
    Positions without a page read as zeros (codes 0, scale 0). Also what a test compares a flat cache with."""
    B, H, C, D = cache.B, cache.H, cache.capacity, cache.D
    table = cache.page_table.long()  # [B, C // 256]
    absent = (table < 0).repeat_interleave(PAGE, dim=1).view(B, 1, C)
    idx = table.clamp(min=0)

    def gather(t):
        if t is None:
            return None
        u = t.view(torch.uint8) if t.dtype == FP8 else t
        g = u[idx]  # [B, C // 256, H, 256, (D)]
        g = g.transpose(1, 2).reshape(B, H, C, *g.shape[4:])
        g = g.masked_fill(absent.unsqueeze(-1) if g.dim() == 4 else absent, 0)
        return g.view(FP8) if t.dtype == FP8 else g
    sc = (cache.k_scale[layer], cache.v_scale[layer]) if cache.fp8 else (None, None)
    return gather(cache.k[layer]), gather(cache.v[layer]), gather(sc[0]), gather(sc[1])


def _ring_view(cache: KVCache, layer: int, lens, dtype):
    """The torch path's view of a ring (the ring rule): ``(k, v, lens')`` with the slots gathered into absolute order
    from ``off[b] = max(lens[b] - C, 0)`` on, index ``i`` standing for key ``off[b] + i`` (slot ``(off[b] + i) % C``),
    and ``lens' = lens - off`` (at most C). Every key of a row's window keeps its distance to the row's limit, so the
    masked softmax of the flat references applies unchanged. An FP8 ring is dequantised to ``dtype``, the rows at or
    beyond ``lens'`` zeroed (dead codes and scales may be NaN)."""
    C = cache.capacity
    off = (lens.long() - C).clamp(min=0)  # [B]
    slot = (off.view(-1, 1) + torch.arange(C, device=lens.device).view(1, C)) % C  # [B, C]
    rows = slot.view(cache.B, 1, C).expand(cache.B, cache.H, C)

    def gather(t):
        if t.dim() == 3:
            return t.gather(2, rows)
        idx = rows.unsqueeze(-1).expand(cache.B, cache.H, C, cache.D)
        if t.dtype == FP8:
            return t.view(torch.uint8).gather(2, idx).view(FP8)
        return t.gather(2, idx)
    k, v = gather(cache.k[layer]), gather(cache.v[layer])
    lens_g = (lens.long() - off).to(lens.dtype)
    if cache.fp8:
        live = (torch.arange(C, device=lens.device).view(1, 1, C) < lens_g.view(-1, 1, 1)).unsqueeze(-1)
        zero = torch.zeros((), device=lens.device)
        k = torch.where(live, dequantize_rows(k, gather(cache.k_scale[layer])), zero).to(dtype)
        v = torch.where(live, dequantize_rows(v, gather(cache.v_scale[layer])), zero).to(dtype)
    return k, v, lens_g


def _ring_check(what: str, cache: KVCache, window, T: int, t_bound) -> int:
    """The ring rule's conditions on an attention call of T new tokens, on every path; returns the window."""
    if window is None:
        raise ValueError(f"{what}: a ring cache needs window=W (capacity {cache.capacity}, window None)")
    if window + T - 1 > cache.capacity:
        raise ValueError(f"{what}: W + T - 1 <= capacity expected on a ring, got W = {window}, T = {T} "
                         f"(W + T - 1 = {window + T - 1}) and capacity {cache.capacity}")
    if t_bound is not None:
        raise ValueError(f"{what}: t_bound= cannot be given on a ring cache (the grid comes from the window, "
                         f"got t_bound = {t_bound})")
    return window


def _check_window(what: str, window, cache: "KVCache | None" = None) -> int | None:
    """``window`` as the ops take it: ``None`` or an ``int >= 1`` (``bool`` rejected); none on a paged ``cache``."""
    if window is not None and cache is not None and cache.pool is not None:
        raise ValueError(f"{what}: window= cannot be given on a paged cache (paged with a window is not built), got "
                         f"{window!r}")
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{what}: window must be None or an int >= 1, got {window!r}")
    return window


def _attention_decode_torch(q, k, v, lens, scale, window=None):
    """Masked SDPA of one query row over keys 0 .. lens[b]-1 (``window``: the module docstring's rule, the last
    ``window`` of them): fp32 on the CPU, the tensors' own dtype on a GPU (the torch_reference() baseline reads
    the cache as it is stored)."""
    Tcap = k.shape[2]
    idx = torch.arange(Tcap, device=q.device).view(1, 1, 1, Tcap)
    mask = idx < lens.view(-1, 1, 1, 1)
    if window is not None:
        mask = mask & (idx >= lens.view(-1, 1, 1, 1) - window)
        v = torch.where(mask.transpose(2, 3), v, torch.zeros((), device=v.device, dtype=v.dtype))  # may hold NaN
    if not q.is_cuda:
        q, k, v = q.float(), k.float(), v.float()
    return F.scaled_dot_product_attention(q.unsqueeze(2), k, v, attn_mask=mask, scale=scale).squeeze(2)


def _attention_extend_torch(q, k, v, lens, scale, window=None):
    """Masked fp32 SDPA of T query rows per head, row i over keys 0 .. lens[b]-T+i (``window``: the module
    docstring's rule, the last ``window`` of them). A row with no key gives zeros and lse = -inf. Returns
    (o [B, T, H, D] fp32, lse [B, T, H])."""
    T, Tcap = q.shape[1], k.shape[2]
    limit = lens.view(-1, 1).long() - T + torch.arange(T, device=q.device).view(1, T)  # last visible key
    idx = torch.arange(Tcap, device=q.device).view(1, 1, 1, Tcap)
    mask = idx <= limit.view(-1, 1, T, 1)  # [B, 1, T, Tcap]
    if window is not None:
        mask = mask & (idx > limit.view(-1, 1, T, 1) - window)
    s = (q.transpose(1, 2).float() @ k.float().transpose(-1, -2)) * scale  # [B, H, T, Tcap]
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.masked_fill(lse == float("-inf"), 0.0).unsqueeze(-1))  # a dead row: all zeros
    seen = mask.any(2).view(-1, 1, Tcap, 1)  # the cache beyond lens may hold NaN: those V rows are zeroed
    o = p @ torch.where(seen, v.float(), torch.zeros((), device=q.device))
    return o.transpose(1, 2), lse.transpose(1, 2)


# ---- the front end the three attention ops share ----------------------------------------------------------------
# Each op is: _attend_args -> (torch path: _attend_torch) -> its own row limit -> _attend_contract -> its launch.
# The front end comes in two halves because the row limits fire between them. ``what`` names the public function in
# every message; ``q`` is ``[B, T, H, D]``, or attention_decode's ``[B, H, D]`` (T = 1), and ``out`` has q's shape.

def _attend_args(what: str, q, cache: KVCache, scale, lens, t_bound, rank: int = 4):
    """The checks of every device and the defaults -> ``(T, G, scale, lens, t_bound)``."""
    B, D = cache.B, cache.D
    if q.dim() != rank or q.shape[0] != B or q.shape[-1] != D:
        raise ValueError(f"{what}: q [{B}, {'T, ' if rank == 4 else ''}G * {cache.H}, {D}] expected, got "
                         f"{tuple(q.shape)}")
    T = q.shape[1] if rank == 4 else 1
    G = _group(what, q.shape[-2], cache, _native(q))
    if T < 1:
        raise ValueError(f"{what}: at least one query row expected")
    return (T, G, float(scale) if scale is not None else 1.0 / math.sqrt(D), cache.lens if lens is None else lens,
            cache.t_bound if t_bound is None else int(t_bound))


def _attend_torch(reference, q, cache: KVCache, layer: int, G: int, scale, out, lens, t_bound, return_lse, dtype,
                  window=None):
    """The torch path (CPU tensors / ops.torch_reference()): ``reference(q, k, v, lens, scale, window) -> (o, lse)``
    over the cache's K / V expanded to q's heads, an FP8 cache's as its visible rows dequantised to ``dtype``."""
    k, v = cache.k[layer], cache.v[layer]
    if cache.ring:  # the live slots in absolute order, then the same masked softmax
        k, v, lens = _ring_view(cache, layer, lens, dtype)
    elif cache.pool is not None:  # every row's pages in flat order, then the flat references
        k, v, ks, vs = _paged_view(cache, layer)
        if cache.fp8:
            k, v = _dequantized_prefix(cache, layer, lens, max(min(t_bound, cache.capacity), 1), dtype, (k, v, ks, vs))
    elif cache.fp8:
        k, v = _dequantized_prefix(cache, layer, lens, max(min(t_bound, cache.capacity), 1), dtype)
    o, lse = reference(q, *_expand_kv(k, v, G), lens, scale, window)
    o = o.to(q.dtype)
    if out is not None:
        out.copy_(o)
        o = out
    return (o, lse) if return_lse else o


def _attend_contract(what: str, q, cache: KVCache, layer: int, lens, t_bound, out):
    """The kernels' contract on a GPU; returns ``out``, allocated when not given."""
    B, D = cache.B, cache.D
    if D not in HEAD_DIMS:
        raise ValueError(f"{what}: head dim in {HEAD_DIMS} expected on a GPU, got {D}")
    if q.dtype != torch.bfloat16 or q.stride(-1) != 1 or cache.k[layer].dtype not in CACHE_DTYPES:
        raise ValueError(f"{what}: bf16 q (contiguous head dim) and a bf16 or float8_e4m3fn cache expected")
    if lens.dtype != torch.int32 or not lens.is_cuda or lens.numel() != B or not lens.is_contiguous():
        raise ValueError(f"{what}: lens must be a device int32 [B] tensor")
    if not 1 <= t_bound <= cache.capacity:
        raise ValueError(f"{what}: 1 <= t_bound <= capacity ({cache.capacity}) expected, got {t_bound}")
    if out is None:
        return torch.empty(q.shape, device=q.device, dtype=q.dtype)
    if out.shape != q.shape or out.dtype != torch.bfloat16 or out.stride(-1) != 1 or not out.is_cuda:
        raise ValueError(f"{what}: out must be a bf16 GPU {list(q.shape)} view with a contiguous head dim")
    return out


def _attend_launch(what: str, name: str, q, cache: KVCache, layer: int, out, lens, ws, G: int, t_bound: int,
                   scale: float, return_lse: bool, window: int | None = None):
    """``name[_gqa]_{bf16,fp8}(q, k, v, *scales, lens, out, lse, ws, B, (H | Hkv, G), D, T, t_bound, scale, strides,
    stream)``: the extend and chunk entry points. A rank-3 ``q`` / ``out`` (attention_decode's G rows of a group) is
    T = 1 with a zero t stride. With a window: ``name_win_{bf16,fp8}``, the grouped signature (G = 1 included) with
    ``window`` after ``t_bound``."""
    B, D, k, v = cache.B, cache.D, cache.k[layer], cache.v[layer]
    if q.dim() == 4:
        T, qs, os, dims = q.shape[1], q.stride()[:3], out.stride()[:3], f"T={q.shape[1]} H={q.shape[2]}"
    else:
        T, qs, os, dims = 1, (q.stride(0), 0, q.stride(1)), (out.stride(0), 0, out.stride(1)), f"H={q.shape[1]} G={G}"
    lse = torch.empty(q.shape[:-1], device=q.device, dtype=torch.float32) if return_lse else None
    paged = cache.pool is not None  # the grouped signature with the page table before the stream
    grouped = G > 1 or window is not None or paged
    fn, scales, tag = _entry(name + ("_paged" if paged else "_ring" if cache.ring else "_win" if window is not None
                                     else "_gqa" if grouped else ""), cache, layer)  # a ring: t_bound is the capacity
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), *(s.data_ptr() for s in scales), lens.data_ptr(), out.data_ptr(),
            lse.data_ptr() if lse is not None else None, ws.data_ptr(), B, *((cache.H, G) if grouped else (cache.H,)),
            D, T, t_bound, *(() if window is None else (min(window, cache.capacity),)), scale,
            _ll(*qs, *k.stride()[:3], *v.stride()[:3], *os, *(n for s in scales for n in s.stride()[:2])),
            *(_page_args(cache) if paged else ()), _stream_ptr(q))
    _lib.check(rc, f"{what}[{tag}B={B} {dims} D={D} t_bound={t_bound}{'' if window is None else f' window={window}'}]")
    return (out, lse) if return_lse else out


def attention_decode(q: torch.Tensor, cache: KVCache, layer: int, scale: float | None = None,
                     out: torch.Tensor | None = None, lens: torch.Tensor | None = None,
                     t_bound: int | None = None, return_lse: bool = False, window: int | None = None):
    """softmax(scale * q k^T) v for one query row per head: q ``[B, H, D]`` (any b / h strides, e.g. a
    view of the fused QKV output), keys ``0 .. lens[b]-1`` of ``cache`` layer ``layer``. ``out``:
    optional ``[B, H, D]`` view to write (e.g. of a ``[B, 1, H*D]`` buffer). ``lens`` / ``t_bound``
    default to the cache's. Grouped-query attention: ``H = G * cache.H`` query heads, head h on K / V head
    ``h // G``; on a GPU G > 1 runs the group's G rows as ``attention_extend`` does at T = 1: the extend kernel's
    row slots for G < ``GQA_MFMA_MIN_ROWS``, the MFMA kernel for G = 8 and 16 (K / V streamed once per group; the
    extend / chunk workspace, allocated on first use and never inside a capture). ``window=W``: the last W of those
    keys only (the module docstring's rule), on the windowed kernels of the same routing."""
    what = "attention_decode"
    window = _check_window(what, window, cache)
    if cache.ring:
        window, t_bound = _ring_check(what, cache, window, 1, t_bound), cache.capacity
    _, G, scale, lens, t_bound = _attend_args(what, q, cache, scale, lens, t_bound, rank=3)
    if not _native(q):
        def reference(q, k, v, lens, scale, window):  # its own SDPA, not attention_extend's at T = 1; lse on request
            o = _attention_decode_torch(q, k, v, lens, scale, window)
            if not return_lse:
                return o, None
            s = (q.float().unsqueeze(2) @ k.float().transpose(-1, -2)).squeeze(2) * scale
            idx = torch.arange(k.shape[2], device=q.device).view(1, 1, -1)
            dead = idx >= lens.view(-1, 1, 1)
            if window is not None:
                dead = dead | (idx < lens.view(-1, 1, 1) - window)
            return o, torch.logsumexp(s.masked_fill(dead, float("-inf")), -1)
        return _attend_torch(reference, q, cache, layer, G, scale, out, lens, t_bound, return_lse,
                             q.dtype if q.is_cuda else torch.float32, window)
    out = _attend_contract(what, q, cache, layer, lens, t_bound, out)
    if _gqa_mfma(1, G):  # the group's G rows on an MFMA tile
        res = attention_chunk(q.unsqueeze(1), cache, layer, scale=scale, out=out.unsqueeze(1), lens=lens,
                              t_bound=None if cache.ring else t_bound, return_lse=return_lse, window=window)
        return (out, res[1].squeeze(1)) if return_lse else out
    if G > 1:  # the group's G rows on the extend kernel's row slots: T = 1, no t stride
        return _attend_launch(what, "kfamd_attn_extend", q, cache, layer, out, lens, cache._extend_ws(window), G,
                              t_bound, scale, return_lse, window)
    B, H, D = q.shape
    k, v = cache.k[layer], cache.v[layer]
    lse = torch.empty(B, H, device=q.device, dtype=torch.float32) if return_lse else None
    paged = cache.pool is not None
    fn, scales, tag = _entry("kfamd_attn_decode_paged" if paged else "kfamd_attn_decode_ring" if cache.ring else
                             "kfamd_attn_decode" if window is None else "kfamd_attn_decode_win", cache, layer)
    ws = cache.workspace if not cache.ring else cache._ring_ws(
        "workspace", _lib.lib().kfamd_attn_decode_ring_workspace(B, H, D, window), what)
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), *(s.data_ptr() for s in scales), lens.data_ptr(), out.data_ptr(),
            lse.data_ptr() if lse is not None else None, ws.data_ptr(), B, H, D, t_bound,
            *(() if window is None else (min(window, cache.capacity),)), scale,
            _ll(q.stride(0), q.stride(1), *k.stride()[:3], *v.stride()[:3], out.stride(0), out.stride(1),
                *(n for s in scales for n in s.stride()[:2])), *(_page_args(cache) if paged else ()), _stream_ptr(q))
    _lib.check(rc, f"attention_decode[{tag}B={B} H={H} D={D} t_bound={t_bound}]")
    return (out, lse) if return_lse else out


def attention_extend(q: torch.Tensor, cache: KVCache, layer: int, scale: float | None = None,
                     out: torch.Tensor | None = None, lens: torch.Tensor | None = None,
                     t_bound: int | None = None, return_lse: bool = False, window: int | None = None):
    """softmax(scale * q k^T) v for T new query rows per head (1 <= T <= 16 on a GPU): q ``[B, T, H, D]``
    (any b / t / h strides, e.g. ``qkv.view(B, T, 3, H, D)[:, :, 0]``), already appended to ``cache``
    layer ``layer``. ``lens[b]`` counts the keys INCLUDING the T new rows; row i attends keys
    ``0 .. lens[b] - T + i`` (a row whose limit is negative gives zeros, lse = -inf). ``out``: optional
    ``[B, T, H, D]`` view to write. ``lens`` / ``t_bound`` default to the cache's. K and V are read once
    per 8 query rows (``kernels/attn_kv.hip``). Grouped-query attention: ``H = G * cache.H`` query heads; the
    rows of a K / V head are then the ``T * G`` (token, head-in-group) pairs, and the GPU limit is
    ``T * G <= MAX_EXTEND_ROWS``; with G > 1, ``GQA_MFMA_MIN_ROWS`` rows or more run ``attention_chunk``'s kernel.
    ``window=W``: each row sees the last W keys up to its own only (the module docstring's rule)."""
    what = "attention_extend"
    window = _check_window(what, window, cache)
    if cache.ring:
        window, t_bound = _ring_check(what, cache, window, q.shape[1] if q.dim() == 4 else 1, t_bound), cache.capacity
    T, G, scale, lens, t_bound = _attend_args(what, q, cache, scale, lens, t_bound)
    if not _native(q):
        return _attend_torch(_attention_extend_torch, q, cache, layer, G, scale, out, lens, t_bound, return_lse,
                             torch.float32, window)
    if T * G > MAX_EXTEND_ROWS:
        raise ValueError(f"attention_extend: 1 <= T * G <= {MAX_EXTEND_ROWS} query rows per K / V head expected on a "
                         f"GPU, got T = {T}, G = {G}")
    out = _attend_contract(what, q, cache, layer, lens, t_bound, out)
    if _gqa_mfma(T, G):
        return attention_chunk(q, cache, layer, scale=scale, out=out, lens=lens,
                               t_bound=None if cache.ring else t_bound, return_lse=return_lse, window=window)
    return _attend_launch(what, "kfamd_attn_extend", q, cache, layer, out, lens, cache._extend_ws(window), G, t_bound,
                          scale, return_lse, window)


def attention_chunk(q: torch.Tensor, cache: KVCache, layer: int, scale: float | None = None,
                    out: torch.Tensor | None = None, lens: torch.Tensor | None = None,
                    t_bound: int | None = None, return_lse: bool = False, window: int | None = None):
    """``attention_extend`` without the row limit: softmax(scale * q k^T) v for T new query rows per head
    (1 <= T <= capacity on a GPU), q ``[B, T, H, D]`` (any b / t / h strides), already appended to ``cache``
    layer ``layer``; ``lens[b]`` counts the keys INCLUDING the T new rows, row i attends keys
    ``0 .. lens[b] - T + i`` (a negative limit gives zeros, lse = -inf). ``out``, ``lens``, ``t_bound`` and
    ``return_lse`` as there. On a GPU it always runs the MFMA kernel (``kernels/attn_kv_mfma.hip``: 128-row
    query tiles, K / V read once per tile and split, P rounded to bf16 for the P.V product), whatever T is:
    for T <= 16 it agrees with ``attention_extend`` within the kernels' bounds, not bit for bit. On CPU
    tensors and under ``ops.torch_reference()`` it is the same torch code as ``attention_extend``. Grouped-query
    attention: ``H = G * cache.H`` query heads; the kernel tiles the ``T * G`` rows of a K / V head
    (``T * G <= 65535``). ``window=W``: each row sees the last W keys up to its own only (the module docstring's
    rule); the key tiles below the lowest lower bound of a query tile's rows are not read."""
    what = "attention_chunk"
    window = _check_window(what, window, cache)
    if cache.ring:
        window, t_bound = _ring_check(what, cache, window, q.shape[1] if q.dim() == 4 else 1, t_bound), cache.capacity
    T, G, scale, lens, t_bound = _attend_args(what, q, cache, scale, lens, t_bound)
    if not _native(q):
        return _attend_torch(_attention_extend_torch, q, cache, layer, G, scale, out, lens, t_bound, return_lse,
                             torch.float32, window)
    if T > cache.capacity:
        raise ValueError(f"attention_chunk: 1 <= T <= capacity ({cache.capacity}) query rows expected on a GPU, "
                         f"got {T}")
    out = _attend_contract(what, q, cache, layer, lens, t_bound, out)
    if G > 1 and T * G > 65535:
        raise ValueError(f"attention_chunk: T * G <= 65535 query rows per K / V head expected, got T = {T}, G = {G}")
    return _attend_launch(what, "kfamd_attn_chunk", q, cache, layer, out, lens, cache._chunk_ws(T, G, window), G,
                          t_bound, scale, return_lse, window)
