"""The paged KV cache on the torch path (the page rule: the docstring of ``ops/decode.py``): the allocator (reserve,
exhaustion, release / reset, fork, copy-on-write, set_lens), the errors, and the CPU model: ``generate(paged=True)``
against ``generate()`` and ``generate(num_samples=S)`` against a hand-built flat run. Everything is compared with
``torch.equal``: a paged cache holds the flat cache's values at other addresses."""
import pytest
import torch

from kubeflow_rm_amd import ops
from kubeflow_rm_amd.models import GPT, GPTConfig
from kubeflow_rm_amd.ops.decode import PAGE, _paged_view

L, H, D = 2, 2, 16


def _pool(n_pages=8, dtype=torch.float32):
    return ops.PagePool(L, H, D, n_pages, dtype=dtype)


def _cache(pool, B=2, capacity=768):
    return ops.KVCache(L, B, H, D, capacity, pool=pool)


def _state(cache):
    return ([list(r) for r in cache._table], list(cache.pool._free), list(cache.pool._ref), cache.page_table.clone())


def _fill(cache, lens, seed=0):
    """Append ``max(lens)`` random rows to every layer of an empty cache, then set the lengths."""
    T = max(lens)
    qkv = torch.randn(cache.B, T, 3 * H * D, generator=torch.Generator().manual_seed(seed))
    if T:
        cache.reserve(T)
        for layer in range(L):
            ops.kv_append(qkv, cache, layer)
    cache.set_lens(lens)
    return qkv


def _gathered(cache, layer=0):
    k, v, _, _ = _paged_view(cache, layer)
    return k.clone(), v.clone()


def test_reserve_allocates_exactly_the_missing_pages():
    pool = _pool()
    c = _cache(pool)
    c.reserve(1)
    assert c._table == [[0, -1, -1], [1, -1, -1]] and pool.pages_free == 6
    c.advance(1)
    c.reserve(255)  # positions 1 .. 255: the same page
    assert pool.pages_free == 6
    c.advance(255)
    c.reserve(1)  # position 256: one more page per row
    assert c._table == [[0, 2, -1], [1, 3, -1]] and pool.pages_free == 4
    assert torch.equal(c.page_table, torch.tensor(c._table, dtype=torch.int32))
    assert pool.pages_total == 8 and c.pages_held == 4
    assert pool.nbytes == 8 * pool.page_bytes == 8 * 2 * L * H * PAGE * D * 4
    assert c.nbytes == c.page_table.numel() * 4 + 4 * pool.page_bytes


def test_exhaustion_raises_and_changes_nothing():
    pool = _pool(3)
    c = _cache(pool)
    c.reserve(256)
    before = _state(c)
    with pytest.raises(RuntimeError, match=r"4 pages needed, 1 free"):
        c.reserve(768)
    after = _state(c)
    assert before[:3] == after[:3] and torch.equal(before[3], after[3])


@pytest.mark.parametrize("how", ["release", "reset"])
def test_release_and_reset_return_the_pages(how):
    pool = _pool()
    c = _cache(pool)
    c.reserve(600)
    c.advance(600)
    assert pool.pages_free == 2
    getattr(c, how)()
    assert pool.pages_free == 8 and sorted(pool._free) == list(range(8)) and pool._ref == [0] * 8
    assert c._hlen == [0, 0] and c.lens.tolist() == [0, 0] and c.t_bound == 0
    assert (c.page_table == -1).all() and c.pages_held == 0
    c.reserve(1)  # and it can be filled again
    assert c.pages_held == 2


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 512])
def test_fork_shares_full_pages_and_copies_the_partial_one(n):
    pool = _pool(12)
    c = _cache(pool, B=1)
    _fill(c, [n])
    held = c.pages_held
    assert held == -(-n // PAGE)
    free = pool.pages_free
    k0, v0 = _gathered(c)
    ch = c.fork(3)
    full, part = n // PAGE, int(n % PAGE != 0)
    assert pool.pages_free == free - 3 * part  # no copy at a multiple of 256
    assert ch.B == 3 and ch.lens.tolist() == [n] * 3 and ch._hlen == [n] * 3 and ch.t_bound == n
    for s in range(3):
        assert ch._table[s][:full] == c._table[0][:full]
        if part:
            assert ch._table[s][full] not in c._table[0] and ch._table[s][full] >= 0
        assert ch._table[s][full + part:] == [-1] * (3 - full - part)
    for p in c._table[0][:full]:
        assert pool._ref[p] == 4
    k1, v1 = _gathered(ch)
    for s in range(3):
        assert torch.equal(k1[s, :, :n], k0[0, :, :n]) and torch.equal(v1[s, :, :n], v0[0, :, :n])
    kp, vp = _gathered(c)  # the parent stays valid
    assert torch.equal(kp, k0) and torch.equal(vp, v0) and c.lens.tolist() == [n]
    ch.release()
    c.release()
    assert pool.pages_free == 12


def test_fork_release_moves_the_parents_pages():
    pool = _pool(5)
    c = _cache(pool, B=1)
    _fill(c, [300])
    k0, _ = _gathered(c)
    ch = c.fork(3, release=True)  # 2 held + 2 copies of the partial page: a plain fork would need 3
    assert pool.pages_free == 1 and c.pages_held == 0 and c._hlen == [0]
    k1, _ = _gathered(ch)
    assert all(torch.equal(k1[s, :, :300], k0[0, :, :300]) for s in range(3))


def test_copy_on_write_after_fork_rewind_and_append():
    pool = _pool(12)
    c = _cache(pool, B=1)
    _fill(c, [512])
    w, sib = c.fork(1), c.fork(1)  # the writer and a sibling: three holders of both pages
    parent, sibling = _gathered(c), _gathered(sib)
    w.rewind(212)  # to 300: inside the shared second page
    assert w._hlen == [300] and w.lens.tolist() == [300]
    shared = w._table[0][1]
    assert shared == sib._table[0][1] == c._table[0][1] and pool._ref[shared] == 3
    free = pool.pages_free
    w.reserve(4)
    assert w._table[0][1] != shared and w._table[0][0] == c._table[0][0]  # the page written is private now
    assert pool._ref[shared] == 2 and pool.pages_free == free - 1
    assert torch.equal(w.page_table, torch.tensor(w._table, dtype=torch.int32))
    new = torch.randn(1, 4, 3 * H * D)
    for layer in range(L):
        ops.kv_append(new, w, layer)
    w.advance(4)
    k, v = _gathered(w)
    assert torch.equal(k[0, :, 300:304], new[0].view(4, 3, H, D)[:, 1].transpose(0, 1))
    assert torch.equal(k[0, :, :300], parent[0][0, :, :300])  # the writer kept the prefix
    for cache, (k0, v0) in ((sib, sibling), (c, parent)):  # the sibling and the parent are untouched
        k1, v1 = _gathered(cache)
        assert torch.equal(k1, k0) and torch.equal(v1, v0)
    w.reserve(1)  # private already: nothing more to take
    assert pool.pages_free == free - 1


def test_set_lens_then_reserve_zero():
    pool = _pool()
    c = _cache(pool)
    c.set_lens([257, 0])
    assert c.pages_held == 0 and c._hlen == [257, 0]
    c.reserve(0)
    assert c._table == [[0, 1, -1], [-1, -1, -1]]
    c.reserve(0)
    assert pool.pages_free == 6


def test_appends_without_a_page_or_beyond_the_capacity_are_dropped():
    pool = _pool()
    c = _cache(pool, capacity=256)
    c.reserve(250)
    c.set_lens([250, 250])
    before = [t.clone() for t in pool.k + pool.v]
    qkv = torch.randn(2, 10, 3 * H * D)
    ops.kv_append(qkv, c, 0)  # rows 250 .. 255 stored, 256 .. 259 beyond the capacity
    k, _ = _gathered(c)
    assert torch.equal(k[:, :, 250:256], qkv.view(2, 10, 3, H, D)[:, :6, 1].transpose(1, 2))
    c2 = _cache(pool)  # no reserve: every entry is -1
    mid = [t.clone() for t in pool.k + pool.v]
    ops.kv_append(qkv, c2, 0)
    assert all(torch.equal(a, b) for a, b in zip(mid, pool.k + pool.v))
    assert not all(torch.equal(a, b) for a, b in zip(before, mid))


def test_fp8_pool_round_trips_quantize_rows():
    pool = _pool(dtype=ops.decode.FP8)
    c, f = _cache(pool), ops.KVCache(L, 2, H, D, 768, dtype=ops.decode.FP8)
    qkv = torch.randn(2, 300, 3 * H * D)
    c.reserve(300)
    for cache in (c, f):
        ops.kv_append(qkv, cache, 1)
        cache.advance(300)
    k, v, ks, vs = _paged_view(c, 1)
    assert torch.equal(k.view(torch.uint8)[:, :, :300], f.k[1].view(torch.uint8)[:, :, :300])
    assert torch.equal(vs[:, :, :300], f.v_scale[1][:, :, :300])
    q = torch.randn(2, 3, H, D)
    for op in (ops.attention_extend, ops.attention_chunk):
        a, la = op(q, c, 1, return_lse=True)
        b, lb = op(q, f, 1, return_lse=True)
        assert torch.equal(a, b) and torch.equal(la, lb)
    assert torch.equal(ops.attention_decode(q[:, 0], c, 1), ops.attention_decode(q[:, 0], f, 1))


def test_errors():
    pool = _pool()
    with pytest.raises(ValueError, match="multiple of 256"):
        ops.KVCache(L, 2, H, D, 300, pool=pool)
    with pytest.raises(ValueError, match="ring"):
        ops.KVCache(L, 2, H, D, 768, pool=pool, ring=True, window=8)
    with pytest.raises(ValueError, match="pool holds"):
        ops.KVCache(L, 2, H + 1, D, 768, pool=pool)
    c = _cache(pool)
    c.reserve(4)
    c.advance(4)
    q = torch.randn(2, 1, H, D)
    for op, qq in ((ops.attention_decode, q[:, 0]), (ops.attention_extend, q), (ops.attention_chunk, q)):
        with pytest.raises(ValueError, match="paged"):
            op(qq, c, 0, window=4)
    with pytest.raises(ValueError, match="paged cache expected"):
        ops.KVCache(L, 2, H, D, 768).reserve(1)


def _model(**kw):
    cfg = GPTConfig(vocab_size=64, d_model=32, n_layers=2, n_heads=4, d_ff=64, max_seq=600, dtype=torch.float32, **kw)
    return GPT(cfg).eval()


def test_model_errors():
    m = _model()
    idx = torch.randint(0, 64, (1, 5))
    for kw in ({"paged": True}, {"num_samples": 2}):
        with pytest.raises(NotImplementedError, match="not built"):
            m.generate(idx, 4, draft=m, **kw)
    with pytest.raises(ValueError, match="num_samples"):
        m.generate(idx, 4, num_samples=0)
    w = _model(window=8)
    with pytest.raises(ValueError, match="not built"):
        w.new_cache(1, 256, paged=True)
    with pytest.raises(ValueError, match="not built"):
        w.generate(idx, 4, paged=True)
    assert m.new_cache(2, 300, paged=True).capacity == 512  # rounded up to whole pages
    assert m.new_cache(2, 300, paged=True).pool.pages_total == 4
    with pytest.raises(RuntimeError, match="pages needed"):
        m.prefill(torch.randint(0, 64, (2, 300)), m.new_cache(2, 300, paged=True, n_pages=3))


@pytest.mark.parametrize("kw", [{}, {"pos": "rope", "n_kv_heads": 2}], ids=["learned", "rope-gqa"])
def test_generate_paged_equals_generate(kw):
    m = _model(**kw)
    idx = torch.randint(0, 64, (2, 250), generator=torch.Generator().manual_seed(1))
    assert torch.equal(m.generate(idx, 12), m.generate(idx, 12, paged=True))  # crosses a page edge at 256
    gen = lambda: torch.Generator().manual_seed(5)  # noqa: E731
    a = m.generate(idx, 6, temperature=0.9, top_k=10, generator=gen(), prefill_chunk=100)
    b = m.generate(idx, 6, temperature=0.9, top_k=10, generator=gen(), prefill_chunk=100, paged=True)
    assert torch.equal(a, b)
    # logit for logit: the same steps by hand on both caches
    cf, cp = m.new_cache(2, 512), m.new_cache(2, 512, paged=True)  # the same key count in the masked softmax
    for c in (cf, cp):
        c.logits = [m.prefill(idx, c), m.decode_step(idx[:, 0], c), m.extend(idx[:, :7], c),
                    m.extend(idx[:, :40], c, chunk=20)]
    assert all(torch.equal(x, y) for x, y in zip(cf.logits, cp.logits))


def _flat_samples(m, idx, n_new, S, **sample):
    """``generate(num_samples=S)`` by hand on a flat cache: prefill B rows, copy the K / V rows S-fold into a flat cache
    of B * S rows, decode with the same sampler."""
    from kubeflow_rm_amd.models.gpt import _sample
    B, T0 = idx.shape
    c0 = m.new_cache(B, T0 + n_new)
    logits = m.prefill(idx, c0).repeat_interleave(S, 0)
    c = m.new_cache(B * S, T0 + n_new)
    for layer in range(c.n_layers):
        c.k[layer].copy_(c0.k[layer].repeat_interleave(S, 0))
        c.v[layer].copy_(c0.v[layer].repeat_interleave(S, 0))
    c.set_lens([T0] * (B * S))
    out = [idx.repeat_interleave(S, 0)]
    for i in range(n_new):
        nxt = _sample(logits, sample.get("temperature", 0.0), sample.get("top_k"), sample.get("generator"))
        out.append(nxt.view(B * S, 1))
        if i + 1 < n_new:
            logits = m.decode_step(nxt, c)
    return torch.cat(out, 1)


@pytest.mark.parametrize("T0", [250, 256, 300])
def test_num_samples_equals_the_hand_built_flat_run(T0):
    m = _model()
    idx = torch.randint(0, 64, (2, T0), generator=torch.Generator().manual_seed(2))
    got = m.generate(idx, 10, num_samples=3, temperature=1.0, top_k=20, generator=torch.Generator().manual_seed(9))
    want = _flat_samples(m, idx, 10, 3, temperature=1.0, top_k=20, generator=torch.Generator().manual_seed(9))
    assert got.shape == (6, T0 + 10) and torch.equal(got, want)
    assert not torch.equal(got[0], got[1])  # the samples differ
    assert torch.equal(m.generate(idx, 5, num_samples=1), m.generate(idx, 5, paged=True))


def test_greedy_samples_are_equal_rows_and_the_pool_follows_the_sharing_rule():
    m = _model()
    idx = torch.randint(0, 64, (2, 300), generator=torch.Generator().manual_seed(3))
    out, cache = m.generate(idx, 8, num_samples=3, return_cache=True)
    ref = m.generate(idx, 8)
    for b in range(2):
        for s in range(3):
            assert torch.equal(out[b * 3 + s], ref[b])
    pool = cache.pool  # 1 full prompt page per prompt, 1 tail page per sample
    assert pool.pages_total == 2 * 1 + 2 * 3 * 1 and pool.pages_free == 0
    assert sorted(pool._ref) == [1] * 6 + [3] * 2
    cache.release()
    assert pool.pages_free == pool.pages_total
    mine = ops.PagePool(2, 4, 8, 20, dtype=torch.float32)  # a caller's pool gets its pages back
    assert torch.equal(m.generate(idx, 8, num_samples=3, pool=mine), out) and mine.pages_free == 20
