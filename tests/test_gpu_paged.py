"""The paged KV cache on the GPU kernels (the page rule: the docstring of ``ops/decode.py``).

The oracle is bit equality: a paged launch keeps the flat launch's split partition, tile order and arithmetic, only the
addresses differ, so O, the LSE and the cache contents after an append equal the flat cache's with ``torch.equal``.
Shapes: B = 2, 2 K / V heads, G in {1, 4}, D in {64, 128}, bf16 and FP8, capacity 768 (three pages) on a pool of 8 pages
with a scrambled table (descending within a row, interleaved between the rows). Every page no row owns and every row at
or beyond ``len`` inside an owned page holds NaN (bf16) or ``0x7F`` codes and NaN scales (FP8), in the flat cache too."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP, NPAGES, P = 2, 2, 768, 8, 256
FP8 = torch.float8_e4m3fn
ORDER = [5, 3, 1, 4, 2, 0, 6, 7]  # the free list's order: row 0 takes 5, 3, 1 and row 1 takes 4, 2, 0
KINDS = ["bf16", "fp8"]
LENS = [(1, 255), (256, 257), (600, None), (768, 513)]  # None: the T new rows only (an empty row beside a long one)


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _bits(t):
    """The tensor's bytes as integers: NaN-safe equality."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _poison(ts, scales):
    for t in ts:
        if t.dtype == FP8:
            t.view(torch.uint8).fill_(0x7F)
        else:
            t.fill_(float("nan"))
    for t in scales or []:
        t.fill_(float("nan"))


_ROWS: dict = {}


def _rows(D, kind):
    """K, V rows [B, HKV, CAP, D] (and FP8: their scales) in the cache's format, drawn once per shape, never changed."""
    from kubeflow_rm_amd.ops.decode import quantize_rows
    if (D, kind) not in _ROWS:
        k, v = _randn(B, HKV, CAP, D, seed=D), _randn(B, HKV, CAP, D, seed=D + 1)
        if kind == "fp8":
            (k, ks), (v, vs) = quantize_rows(k), quantize_rows(v)
            _ROWS[D, kind] = (k, v, ks, vs)
        else:
            _ROWS[D, kind] = (k, v, None, None)
    return _ROWS[D, kind]


def _caches(D, kind, lens, layers=1, share=False):
    """A flat and a paged cache that hold the same ``lens[b]`` rows per batch row and poison everywhere else. ``share``:
    both rows are forks of one sequence (``lens[0] == lens[1]``), so they share its full pages."""
    from kubeflow_rm_amd import ops
    dtype = FP8 if kind == "fp8" else torch.bfloat16
    k, v, ks, vs = _rows(D, kind)
    flat = ops.KVCache(layers, B, HKV, D, CAP, device=DEV, dtype=dtype)
    pool = ops.PagePool(layers, HKV, D, NPAGES, device=DEV, dtype=dtype)
    pool._free = list(ORDER)
    if share:
        one = ops.KVCache(layers, 1, HKV, D, CAP, pool=pool)
        one.set_lens(lens[:1])
        one.reserve(0)
        paged = one.fork(2, release=True)
        src = [0, 0]
    else:
        paged = ops.KVCache(layers, B, HKV, D, CAP, pool=pool)
        paged.set_lens(lens)
        paged.reserve(0)
        src = [0, 1]
    flat.set_lens(lens)
    _poison(flat.k + flat.v, (flat.k_scale or []) + (flat.v_scale or []))
    _poison(pool.k + pool.v, (pool.k_scale or []) + (pool.v_scale or []))
    for layer in range(layers):
        for b, n in enumerate(lens):
            for dst_f, dst_p, rows in ((flat.k, pool.k, k), (flat.v, pool.v, v), (flat.k_scale, pool.k_scale, ks),
                                       (flat.v_scale, pool.v_scale, vs)):
                if rows is None:
                    continue
                _bits(dst_f[layer])[b, :, :n] = _bits(rows)[src[b], :, :n]
                for c in range(-(-n // P)):
                    m = min(P, n - c * P)
                    _bits(dst_p[layer])[paged._table[b][c], :, :m] = _bits(rows)[src[b], :, c * P:c * P + m]
    return flat, paged


def _lens(case, T):
    return [case[0], T if case[1] is None else case[1]]


def test_the_table_is_scrambled_and_a_strict_subset():
    flat, paged = _caches(64, "bf16", [768, 513])
    assert paged._table == [[5, 3, 1], [4, 2, 0]] and paged.pool.pages_free == 2
    assert torch.equal(paged.page_table.cpu(), torch.tensor(paged._table, dtype=torch.int32))
    k = paged.pool.k[0]
    assert torch.isnan(k[6:].float()).all() and torch.isnan(k[0, :, 1:].float()).all()  # key 512 of row 1 is page 0's row 0
    assert not torch.isnan(k[0, :, 0].float()).any()


@pytest.mark.parametrize("case", LENS, ids=str)
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_equals_flat(kind, D, G, case):
    from kubeflow_rm_amd import ops
    flat, paged = _caches(D, kind, _lens(case, 1))
    q = _randn(B, G * HKV, D, seed=7)
    o1, l1 = ops.attention_decode(q, flat, 0, return_lse=True)
    o2, l2 = ops.attention_decode(q, paged, 0, return_lse=True)
    assert not torch.isnan(o1.float()).any() and torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("case", LENS, ids=str)
@pytest.mark.parametrize("T,G", [(1, 1), (3, 1), (8, 1), (16, 1), (1, 4), (3, 4)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_paged_extend_equals_flat(kind, D, T, G, case):
    """T * G = 1 .. 16 rows: every row-slot kernel and both split launches of 16 rows; (3, 4) is 12 grouped rows, which
    ``attention_extend`` routes to the MFMA form."""
    from kubeflow_rm_amd import ops
    flat, paged = _caches(D, kind, _lens(case, T))
    q = _randn(B, T, G * HKV, D, seed=T)
    o1, l1 = ops.attention_extend(q, flat, 0, return_lse=True)
    o2, l2 = ops.attention_extend(q, paged, 0, return_lse=True)
    assert not torch.isnan(o1.float()).any() and torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("prior", [0, 300])
@pytest.mark.parametrize("T,G", [(16, 1), (130, 1), (300, 1), (130, 4)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_paged_chunk_equals_flat(kind, D, T, G, prior):
    """A padding wave (16), a second query tile (130), rows whose limits fall in different pages (300); row 1 always
    starts empty."""
    from kubeflow_rm_amd import ops
    flat, paged = _caches(D, kind, [prior + T, T])
    q = _randn(B, T, G * HKV, D, seed=T + 1)
    o1, l1 = ops.attention_chunk(q, flat, 0, return_lse=True)
    o2, l2 = ops.attention_chunk(q, paged, 0, return_lse=True)
    assert not torch.isnan(o1.float()).any() and torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_that_share_pages_through_fork(kind, D):
    from kubeflow_rm_amd import ops
    flat, paged = _caches(D, kind, [513, 513], share=True)
    assert paged._table[0][:2] == paged._table[1][:2] and paged._table[0][2] != paged._table[1][2]
    q = _randn(B, 3, HKV, D, seed=3)
    for op, qq in ((ops.attention_decode, q[:, 0]), (ops.attention_extend, q), (ops.attention_chunk, q)):
        o1, l1 = op(qq, flat, 0, return_lse=True)
        o2, l2 = op(qq, paged, 0, return_lse=True)
        assert torch.equal(o1, o2) and torch.equal(l1, l2)


def _tensors(c):
    return [*c.k, *c.v, *(c.k_scale or []), *(c.v_scale or [])]


def _expected_pool(paged, flat, start, T, before):
    """The pool's tensors after a correct append of positions ``start[b] .. start[b] + T - 1``: ``before`` with the flat
    cache's rows at those positions scattered to their pages; positions at or beyond the capacity or without a page
    change nothing."""
    want = [t.clone() for t in before]
    for w, f in zip(want, _tensors(flat)):
        for b in range(B):
            for p in range(start[b], min(start[b] + T, CAP)):
                page = paged._table[b][p // P]
                if page >= 0:
                    _bits(w)[page, :, p % P] = _bits(f)[b, :, p]
    return want


@pytest.mark.parametrize("T", [1, 16, 300])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", ["plain", "rope", "rope-gqa"])
@pytest.mark.parametrize("kind", KINDS)
def test_paged_appends_equal_flat_and_touch_nothing_else(kind, mode, D, T):
    """From position 250: across one page edge (T = 16) and two (T = 300)."""
    from kubeflow_rm_amd import ops
    G = 4 if mode == "rope-gqa" else 1
    rope = ops.rope_table(CAP, D, device=DEV) if mode != "plain" else None
    start = [250, 250]
    flat, paged = _caches(D, kind, start)
    paged.reserve(T)
    before = [t.clone() for t in _tensors(paged)]
    qkv = _randn(B, T, (G + 2) * HKV * D, seed=T + D)
    qf, qp = qkv.clone(), qkv.clone()
    ops.kv_append(qf, flat, 0, q_heads=G * HKV, rope=rope)
    ops.kv_append(qp, paged, 0, q_heads=G * HKV, rope=rope)
    assert torch.equal(qf, qp) and (rope is None) == torch.equal(qp, qkv)  # the rotation in place
    want = _expected_pool(paged, flat, start, T, before)
    for got, w in zip(_tensors(paged), want):
        assert torch.equal(_bits(got), _bits(w))
    touched = {paged._table[b][p // P] for b in range(B) for p in range(250, 250 + T)}
    assert len(touched) == 2 * (1 if T == 1 else 2 if T == 16 else 3)


@pytest.mark.parametrize("mode", ["plain", "rope"])
@pytest.mark.parametrize("kind", KINDS)
def test_appends_drop_rows_at_the_capacity_and_rows_without_a_page(kind, mode):
    """Row 0 runs into the capacity; row 1's next page is absent because ``reserve`` is skipped on purpose: both drop
    those rows without a store (the documented contract, on a valid table)."""
    from kubeflow_rm_amd import ops
    D, T = 64, 16
    rope = ops.rope_table(CAP + T, D, device=DEV) if mode == "rope" else None
    start = [760, 250]
    flat, paged = _caches(D, kind, start)
    assert paged._table[1] == [4, -1, -1]
    before = [t.clone() for t in _tensors(paged)]
    qkv = _randn(B, T, 3 * HKV * D, seed=5)
    qf, qp = qkv.clone(), qkv.clone()
    ops.kv_append(qf, flat, 0, rope=rope)
    ops.kv_append(qp, paged, 0, rope=rope)
    want = _expected_pool(paged, flat, start, T, before)  # row 0: 760 .. 767; row 1: 250 .. 255
    for got, w in zip(_tensors(paged), want):
        assert torch.equal(_bits(got), _bits(w))
    assert torch.equal(qf[0], qp[0]) and torch.equal(qf[1, :6], qp[1, :6])
    if rope is not None:  # a dropped row is not rotated either
        assert torch.equal(qp[0, 8:], qkv[0, 8:]) and torch.equal(qp[1, 6:], qkv[1, 6:])


def test_errors_on_the_gpu():
    from kubeflow_rm_amd import ops
    flat, paged = _caches(64, "bf16", [10, 10])
    q = _randn(B, 1, HKV, 64, seed=1)
    for op, qq in ((ops.attention_decode, q[:, 0]), (ops.attention_extend, q), (ops.attention_chunk, q)):
        with pytest.raises(ValueError, match="paged"):
            op(qq, paged, 0, window=4)
    with pytest.raises(ValueError, match="ring"):
        ops.KVCache(1, B, HKV, 64, CAP, pool=paged.pool, ring=True, window=4)


# ---- the model ------------------------------------------------------------------------------------------------------
_MODEL = []


def _small():
    from kubeflow_rm_amd.models import GPT, GPTConfig
    if not _MODEL:
        cfg = GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=512, max_seq=2048, pos="rope",
                        n_kv_heads=2, norm="rms", mlp="swiglu")
        _MODEL.append(GPT(cfg, device=DEV).eval())
    return _MODEL[0]


def _prompt(T0, seed=0):
    return torch.randint(0, 512, (2, T0), generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("kv_dtype", [None, FP8], ids=KINDS)
def test_model_steps_on_a_paged_cache_equal_the_flat_caches(kv_dtype):
    m = _small()
    idx = _prompt(250)
    logits = []
    for paged in (False, True):
        c = m.new_cache(2, 512, kv_dtype=kv_dtype, paged=paged)
        out = [m.prefill(idx, c), m.decode_step(idx[:, 0], c), m.extend(idx[:, :3], c),
               m.extend(idx[:, :40], c, chunk=32)]  # 250 -> 251 -> 254 -> 294: over the page edge
        g = m.graphed_decode_step(c)
        out += [g(idx[:, 1]).clone(), g(idx[:, 2]).clone()]
        assert c.lens.tolist() == [296, 296] and (not paged or c._hlen == [296, 296])
        logits.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*logits))
    assert c.pages_held == 4 and c.pool.pages_total == 4


def test_generate_paged_graph_fused_fp8_equals_flat_and_replays():
    m = _small()
    idx = _prompt(250, seed=1)
    kw = dict(graph=True, sampler="fused", kv_dtype=FP8, temperature=0.8, top_k=50, top_p=0.9)
    gen = lambda: torch.Generator().manual_seed(11)  # noqa: E731
    want = m.generate(idx, 12, generator=gen(), **kw)
    got = m.generate(idx, 12, generator=gen(), paged=True, **kw)
    assert torch.equal(got, want)
    assert torch.equal(m.generate(idx, 12, generator=gen(), paged=True, **kw), got)


def _flat_samples(m, idx, n_new, S, temperature, top_k, generator):
    """``generate(num_samples=S)`` by hand on a flat cache: prefill B rows, copy the K / V rows S-fold into a flat cache
    of B * S rows, decode with the same sampler."""
    from kubeflow_rm_amd.models.gpt import _sample
    Bp, T0 = idx.shape
    c0 = m.new_cache(Bp, T0 + n_new)
    logits = m.prefill(idx, c0).repeat_interleave(S, 0)
    c = m.new_cache(Bp * S, T0 + n_new)
    for layer in range(c.n_layers):
        c.k[layer].copy_(c0.k[layer].repeat_interleave(S, 0))
        c.v[layer].copy_(c0.v[layer].repeat_interleave(S, 0))
    c.set_lens([T0] * (Bp * S))
    out = [idx.repeat_interleave(S, 0)]
    for i in range(n_new):
        nxt = _sample(logits, temperature, top_k, generator)
        out.append(nxt.view(Bp * S, 1))
        if i + 1 < n_new:
            logits = m.decode_step(nxt, c)
    return torch.cat(out, 1)


def test_num_samples_equals_the_hand_built_flat_run_and_shares_the_prompt():
    m = _small()
    idx = _prompt(300, seed=2)
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)  # noqa: E731
    got, cache = m.generate(idx, 8, num_samples=4, temperature=1.0, top_k=40, generator=gen(), return_cache=True)
    want = _flat_samples(m, idx, 8, 4, 1.0, 40, gen())
    assert got.shape == (8, 308) and torch.equal(got, want)
    pool = cache.pool  # one full prompt page per prompt, shared 4 ways; one page per sample for the tail and the tokens
    assert pool.pages_total == 2 * 1 + 2 * 4 * 1 and pool.pages_total - pool.pages_free == 10
    assert sorted(pool._ref) == [1] * 8 + [4] * 2
    cache.release()
    assert pool.pages_free == pool.pages_total
