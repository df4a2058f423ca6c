"""Chunked-prefill attention on the gfx950 kernels: ops.attention_chunk (kernels/attn_kv_mfma.hip: MFMA query
tiles of any row count over a bf16 or FP8 KV cache), GPT.extend(chunk=) and generate(prefill_chunk=), against
per-row fp32 SDPA and the fp32 model. The bounds are those of tests/test_gpu_extend.py's _check, which
tests/test_gpu_attention.py also holds the MFMA flash kernel to (it rounds P to bf16 as this kernel does):
max-abs < 2e-2, rel-l2 < 8e-3, lse within 1e-3."""
from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 3
FP8 = torch.float8_e4m3fn
KINDS = ["bf16", "fp8"]
ABS, REL, LSE = 2e-2, 8e-3, 1e-3


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _randn(*shape, seed, dev=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev or DEV, torch.bfloat16)


def _S():
    from kubeflow_rm_amd.ops import decode
    return decode.SPLIT_KEYS


def _R():
    from kubeflow_rm_amd.ops import _lib
    return int(_lib.lib().kfamd_attn_chunk_tile_rows())


def _nsplit(Tq, t_bound, Bc=B, Hc=H):
    from kubeflow_rm_amd.ops import _lib
    return int(_lib.lib().kfamd_attn_chunk_nsplit(Bc, Hc, Tq, t_bound))


def _store(cache, k, v):
    """k, v [B, H, cap, D] bf16 into rows 0 .. cap-1 of layer 0: a copy, or for an FP8 cache the quantising
    append. Returns the values the cache then stands for (fp32 for FP8: dequantize_rows of the stored codes)."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.decode import dequantize_rows
    if not cache.fp8:
        cache.k[0].copy_(k)
        cache.v[0].copy_(v)
        return cache.k[0], cache.v[0]
    Bc, Hc, cap, D = k.shape
    qkv = torch.stack([torch.zeros_like(k), k, v], 0).permute(1, 3, 0, 2, 4).reshape(Bc, cap, 3 * Hc * D).contiguous()
    cache.reset()
    ops.kv_append(qkv, cache, 0)
    return dequantize_rows(cache.k[0], cache.k_scale[0]), dequantize_rows(cache.v[0], cache.v_scale[0])


def _cache(D, seed, kind="bf16", Bc=B, Hc=H, cap=None, dev=None):
    """(cache, k, v): k, v are what the reference attends."""
    from kubeflow_rm_amd import ops
    dev = dev or DEV
    cap = 3 * _S() + 8 if cap is None else cap
    c = ops.KVCache(1, Bc, Hc, D, cap, device=dev, dtype=FP8 if kind == "fp8" else torch.bfloat16)
    k, v = _store(c, _randn(Bc, Hc, cap, D, seed=seed, dev=dev), _randn(Bc, Hc, cap, D, seed=seed + 1, dev=dev))
    return c, k, v


def _poison(cache, lens):
    """Everything at or beyond lens[b]: NaN, or for an FP8 cache code 0x7F and NaN scales."""
    for b, n in enumerate(lens):
        if cache.fp8:
            cache.k[0].view(torch.uint8)[b, :, n:] = 0x7F
            cache.v[0].view(torch.uint8)[b, :, n:] = 0x7F
            cache.k_scale[0][b, :, n:] = float("nan")
            cache.v_scale[0][b, :, n:] = float("nan")
        else:
            cache.k[0][b, :, n:] = float("nan")
            cache.v[0][b, :, n:] = float("nan")


def _ref(q, k, v, lens, extra=0):
    """fp32 SDPA per (b, row) over that row's own key prefix 0 .. lens[b]-Tq+i; a row with no key gives zeros,
    lse = -inf. ``extra``: keys past the limit each row attends too, capped at lens[b] (the leak a test wants
    to be able to see). Returns (o [B, Tq, H, D], lse [B, Tq, H])."""
    Bq, Tq, Hq, D = q.shape
    o = torch.zeros(Bq, Tq, Hq, D, device=q.device)
    lse = torch.full((Bq, Tq, Hq), float("-inf"), device=q.device)
    for b, n in enumerate(lens):
        for i in range(Tq):
            nk = min(n - Tq + i + 1 + extra, n)
            if nk <= 0:
                continue
            kk, vv = k[b:b + 1, :, :nk].float(), v[b:b + 1, :, :nk].float()
            o[b, i] = F.scaled_dot_product_attention(q[b:b + 1, i].float().unsqueeze(2), kk, vv)[0, :, 0]
            s = (q[b, i].float().unsqueeze(1) @ kk[0].transpose(-1, -2)).squeeze(1) / math.sqrt(D)
            lse[b, i] = torch.logsumexp(s, -1)
    return o, lse


def _check(o, ref, what=""):
    err = (o.float() - ref).abs().max().item()
    rel = _rel(o, ref)
    print(f"chunk attention {what}: max-abs {err:.3e} rel-l2 {rel:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < ABS, err
    assert rel < REL, rel


def _edge_rows():
    R = _R()
    return [1, 17, 32, 33, R - 1, R, R + 1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("ti", range(7))
def test_chunk_attention_tile_and_split_edges(D, ti, kind):
    """T around the wave and tile sizes; the new block before, on and across a split boundary and across a
    64-key tile boundary, ragged lens; the tight grid (one split for the first case) and the whole capacity
    (several); the LSE; two calls bitwise equal; with lens == T on a bf16 cache row 0 returns V row 0."""
    from kubeflow_rm_amd import ops
    S, Tq = _S(), _edge_rows()[ti]
    cache, k, v = _cache(D, seed=100 + D, kind=kind)
    q = _randn(B, Tq, H, D, seed=Tq)
    seen = set()
    for lens in ([Tq, S - 1], [S, S + 1], [S + Tq - 1, 2 * S + 3], [64 + Tq // 2, cache.capacity]):
        cache.set_lens(lens)
        ref, ref_lse = _ref(q, k, v, lens)
        for t_bound in (max(lens), cache.capacity):
            seen.add(min(_nsplit(Tq, t_bound), 2))
            o, lse = ops.attention_chunk(q, cache, 0, t_bound=t_bound, return_lse=True)
            assert o.shape == (B, Tq, H, D) and lse.shape == (B, Tq, H)
            _check(o, ref, f"{kind} D={D} Tq={Tq} lens={lens} t_bound={t_bound} nsplit={_nsplit(Tq, t_bound)}")
            live = torch.isfinite(ref_lse)
            assert torch.equal(torch.isfinite(lse), live)
            assert (lse[live] - ref_lse[live]).abs().max().item() < LSE
            again, lse2 = ops.attention_chunk(q, cache, 0, t_bound=t_bound, return_lse=True)
            assert torch.equal(again, o) and torch.equal(lse2, lse)
            if lens[0] == Tq and kind == "bf16":  # softmax of one key is exactly 1
                assert torch.equal(o[0, 0], cache.v[0][0, :, 0])
    assert seen == {1, 2}  # the direct store and the split records + combine were both exercised


def test_chunk_attention_splits_of_several_chunks():
    """Enough (b, h) pairs that the split count falls below the number of kSplitKeys chunks: a split covers two
    chunks and the last split is empty for every row."""
    from kubeflow_rm_amd import ops
    Hc, D, Tq = 48, 64, 33
    cache, k, v = _cache(D, seed=77, Hc=Hc)
    assert _nsplit(Tq, cache.capacity, Hc=Hc) == 3 < math.ceil(cache.capacity / _S())
    q = _randn(B, Tq, Hc, D, seed=78)
    lens = [2 * _S() + 5, 3 * _S() + 1]
    cache.set_lens(lens)
    ref, ref_lse = _ref(q, k, v, lens)
    o, lse = ops.attention_chunk(q, cache, 0, t_bound=cache.capacity, return_lse=True)
    _check(o, ref, "H=48 nsplit=3")
    assert (lse - ref_lse).abs().max().item() < LSE


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_chunk_attention_rows_before_the_sequence_start(D, kind):
    """lens < T, 0 included: the leading rows have no key: exactly 0 and lse = -inf; the others match."""
    from kubeflow_rm_amd import ops
    S, Tq = _S(), 40
    cache, k, v = _cache(D, seed=110 + D, kind=kind)
    q = _randn(B, Tq, H, D, seed=7)
    for lens, t_bound in (([2, 0], 2), ([33, S + 2], S + 2), ([0, 39], cache.capacity)):
        cache.set_lens(lens)
        ref, ref_lse = _ref(q, k, v, lens)
        o, lse = ops.attention_chunk(q, cache, 0, t_bound=t_bound, return_lse=True)
        _check(o, ref, f"{kind} lens={lens}")
        for b, n in enumerate(lens):
            dead = max(Tq - n, 0)
            assert (o[b, :dead] == 0).all() and (lse[b, :dead] == float("-inf")).all()
            assert torch.isfinite(lse[b, dead:]).all()
            if dead < Tq:
                assert (lse[b, dead:] - ref_lse[b, dead:]).abs().max().item() < LSE


def _leak_case(D, Tq, kind, dev=None):
    """The block across a split boundary (row 0) and ending a split (row 1); the K rows of the new block scaled
    so that a row attending one key past its causal limit moves far; everything at or beyond lens poisoned.
    Returns (cache, q, lens, ref, moved [B, Tq - 1])."""
    from kubeflow_rm_amd import ops
    dev = dev or DEV
    S = _S()
    cap = 3 * S + 8
    lens = [S + 2, 2 * S + Tq - 1]
    q = _randn(B, Tq, H, D, seed=9, dev=dev)
    k, v = _randn(B, H, cap, D, seed=120 + D, dev=dev), _randn(B, H, cap, D, seed=121 + D, dev=dev)
    for b, n in enumerate(lens):
        for j in range(1, Tq):  # the key of block row j is aligned with the query of row j - 1
            p = n - Tq + j
            k[b, :, p] = (k[b, :, p].float().abs() * torch.sign(q[b, j - 1].float()) * 30).to(torch.bfloat16)
    cache = ops.KVCache(1, B, H, D, cap, device=dev, dtype=FP8 if kind == "fp8" else torch.bfloat16)
    ks, vs = _store(cache, k, v)
    ks, vs = ks.clone(), vs.clone()  # what the reference reads stays clean
    _poison(cache, lens)
    cache.set_lens(lens)
    ref, _ = _ref(q, ks, vs, lens)
    leaky, _ = _ref(q, ks, vs, lens, extra=1)
    moved = (leaky - ref)[:, :Tq - 1].abs().amax(dim=(2, 3))  # per (b, row) but the last, which has no next key
    return cache, q, lens, ref, moved


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("big", [False, True], ids=["T17", "Tile+1"])
def test_chunk_attention_does_not_leak(D, big, kind):
    """Cache rows at or beyond lens hold NaN (FP8: code 0x7F, NaN scales): the outputs stay finite and in
    bounds, although one key past a row's limit would move it by >= 10x the bound (shown on the reference)."""
    from kubeflow_rm_amd import ops
    Tq = _R() + 1 if big else 17
    cache, q, lens, ref, moved = _leak_case(D, Tq, kind)
    assert moved.min().item() >= 10 * ABS, moved.min().item()
    for t_bound in (max(lens), cache.capacity):
        o, lse = ops.attention_chunk(q, cache, 0, t_bound=t_bound, return_lse=True)
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
        _check(o, ref, f"{kind} D={D} Tq={Tq} spiked block keys, NaN beyond lens, t_bound={t_bound}")


@pytest.mark.parametrize("D", [64, 128])
def test_chunk_attention_strided_q_and_out_no_stray_writes(D):
    """q read in place from the fused QKV output [B, T, 3, H, D]; o written into a view inside a larger
    sentinel-filled buffer, by the combine launch (several splits) and by the split kernel itself (one)."""
    from kubeflow_rm_amd import ops
    S, Tq = _S(), 37
    cache, k, v = _cache(D, seed=130 + D)
    qkv = _randn(B, Tq, 3, H, D, seed=61)
    q = qkv[:, :, 0]
    assert not q.is_contiguous()
    seen = set()
    for lens in ([S + 9, 40], [40, 37]):
        cache.set_lens(lens)
        seen.add(min(_nsplit(Tq, max(lens)), 2))
        want = ops.attention_chunk(q.contiguous(), cache, 0)
        buf = torch.full((B + 2, Tq + 1, H * D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
        out = buf[1:B + 1, :Tq, 8:].view(B, Tq, H, D)
        got = ops.attention_chunk(q, cache, 0, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out, want)
        _check(got, _ref(q, k, v, lens)[0], f"strided lens={lens}")
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:B + 1, :Tq, 8:] = False
        assert (buf[keep] == 7.0).all()  # every element outside the view is unchanged
    assert seen == {1, 2}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_chunk_agrees_with_the_valu_form_up_to_16_rows(D, kind):
    """attention_extend runs the same rows on fp32 VALU arithmetic: the two agree within the bounds (not bit
    for bit), and both match the reference."""
    from kubeflow_rm_amd import ops
    S = _S()
    cache, k, v = _cache(D, seed=140 + D, kind=kind)
    for Tq, lens in ((1, [S + 1, 5]), (5, [S + 2, 2 * S + 4]), (16, [16, 3 * S])):
        q = _randn(B, Tq, H, D, seed=20 + Tq)
        cache.set_lens(lens)
        a, la = ops.attention_chunk(q, cache, 0, return_lse=True)
        e, le = ops.attention_extend(q, cache, 0, return_lse=True)
        _check(a, e.float(), f"{kind} D={D} Tq={Tq} chunk against extend")
        assert (la - le).abs().max().item() < LSE
        _check(a, _ref(q, k, v, lens)[0], f"{kind} D={D} Tq={Tq} chunk against fp32")


def test_chunk_attention_contract():
    import ctypes
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    cache, _, _ = _cache(64, seed=1, cap=64)
    cache.set_lens([20, 20])
    with pytest.raises(ValueError):
        ops.attention_chunk(_randn(B, 0, H, 64, seed=1), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_chunk(_randn(B, 65, H, 64, seed=1), cache, 0)  # T > capacity
    q = _randn(B, 20, H, 64, seed=1)
    with pytest.raises(ValueError):
        ops.attention_chunk(q, cache, 0, lens=cache.lens.long())
    with pytest.raises(ValueError):
        ops.attention_chunk(q, cache, 0, lens=cache.lens.cpu())
    for t_bound in (0, 65):
        with pytest.raises(ValueError):
            ops.attention_chunk(q, cache, 0, t_bound=t_bound)
    with pytest.raises(ValueError):
        ops.attention_chunk(q.float(), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_chunk(q, cache, 0, out=torch.empty(B, 20, H, 64, device=DEV))
    c96 = ops.KVCache(1, 1, 2, 96, 64, device=DEV)
    c96.set_lens([8])
    q96 = _randn(1, 4, 2, 96, seed=1)
    with pytest.raises(ValueError):
        ops.attention_chunk(q96, c96, 0)
    # nbytes grows by exactly the workspace on first use, and not again for a call that needs no more
    L = _lib.lib()
    big = ops.KVCache(1, B, H, 64, 3 * _S() + 8, device=DEV)
    big.set_lens([300, 300])
    before = big.nbytes
    ops.attention_chunk(_randn(B, 40, H, 64, seed=2), big, 0)
    ws = L.kfamd_attn_chunk_workspace(B, H, 64, 40, big.capacity)
    nsplit = L.kfamd_attn_chunk_nsplit(B, H, 40, big.capacity)
    assert nsplit == 4 and ws == B * H * 40 * nsplit * (64 + 2) * 4
    assert big.nbytes - before == ws
    ops.attention_chunk(_randn(B, 17, H, 64, seed=2), big, 0)
    assert big.nbytes - before == ws
    ops.attention_chunk(_randn(B, 80, H, 64, seed=2), big, 0)  # grows
    assert big.nbytes - before == L.kfamd_attn_chunk_workspace(B, H, 64, 80, big.capacity) == 2 * ws
    # the library itself
    assert L.kfamd_attn_chunk_tile_rows() == 128
    assert L.kfamd_attn_chunk_workspace(1, 2, 96, 4, 64) == 0
    assert L.kfamd_attn_chunk_workspace(1, 2, 64, 0, 64) == 0
    assert L.kfamd_attn_chunk_workspace(1, 2, 64, 65536, 64) == 0
    assert L.kfamd_attn_chunk_workspace(1, 2, 64, 4, 0) == 0
    assert L.kfamd_attn_chunk_workspace(0, 2, 64, 4, 64) == 0
    assert L.kfamd_attn_chunk_workspace(1, 2, 64, 17, 64) == 16  # one split: unused
    assert L.kfamd_attn_chunk_nsplit(1, 2, 0, 64) == 0
    assert L.kfamd_attn_chunk_nsplit(1, 2, 129, 4096) == 16 and L.kfamd_attn_chunk_nsplit(4, 32, 512, 4096) == 1
    o = torch.empty_like(q)

    def call(qt, c, D, Tq, t_bound, ws=None, q_off=0, kt=None):
        ks = list(c.k[0].stride()[:3])
        ks[2] = ks[2] if kt is None else kt
        st = (ctypes.c_longlong * 12)(*qt.stride()[:3], *ks, *c.v[0].stride()[:3], *qt.stride()[:3])
        return L.kfamd_attn_chunk_bf16(qt.data_ptr() + q_off, c.k[0].data_ptr(), c.v[0].data_ptr(), c.lens.data_ptr(),
                                       o.data_ptr(), None, ws, qt.shape[0], qt.shape[2], D, Tq, t_bound, 1.0, st, None)

    assert call(q96, c96, 96, 4, 8) == -1
    assert call(q, cache, 64, 0, 20) == -1
    assert call(q, cache, 64, 65536, 20) == -1
    assert call(q, cache, 64, 20, 0) == -1
    assert call(q, cache, 64, 20, _S() + 1) == -1  # two splits need the workspace
    assert call(q, cache, 64, 20, 20, q_off=2) == -2
    assert call(q, cache, 64, 20, 20, kt=68) == -2  # a cache stride that is no multiple of 16 bytes
    assert call(q, cache, 96, 20, 20, q_off=2) == -1  # an invalid shape is reported before the alignment


# ---- model -------------------------------------------------------------------------------------

def _cfg(n_heads, dtype, n_layers=2):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=n_layers, n_heads=n_heads, d_ff=1024, max_seq=256,
                     dtype=dtype)


@pytest.fixture(scope="module", params=[4, 2], ids=["D64", "D128"])
def models(request):
    from kubeflow_rm_amd.models import GPT
    return (GPT(_cfg(request.param, torch.bfloat16), device=DEV).eval(), GPT(_cfg(request.param, torch.float32)).eval(),
            request.param)


def test_chunked_extend_matches_fp32_full_forward(models):
    """prefill 40 tokens, then extend(chunk=32) of 50 tokens (steps of 32 + 18) and of 100 (32 + 32 + 32 + 4) at
    B = 2: every position within 0.1 of the fp32 full forward."""
    gpu, ref, _ = models
    Bm, T0, steps = 2, 40, (50, 100)
    total = T0 + sum(steps)
    seq = torch.randint(0, 512, (Bm, total), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)
    cache = gpu.new_cache(Bm, total)
    got, at = [gpu.prefill(seq[:, :T0].to(DEV), cache).view(Bm, 1, -1)], T0
    for T in steps:
        lg = gpu.extend(seq[:, at:at + T].to(DEV), cache, chunk=32)
        assert lg.shape == (Bm, T, 512)
        got.append(lg)
        at += T
        assert cache.lens.tolist() == [at] * Bm
    got = torch.cat(got, 1).float().cpu()
    errs = (got - want[:, T0 - 1:]).abs().amax(dim=(0, 2))
    print(f"chunked extend per-position max-abs: max {errs.max().item():.4f}")
    assert errs.max().item() < 0.1, errs.tolist()
    for bad in (16, 257):
        with pytest.raises(ValueError):
            gpu.extend(seq[:, :1].to(DEV), gpu.new_cache(Bm, 256), chunk=bad)


def test_chunked_extend_on_an_fp8_cache_matches_extend(models):
    gpu, _, _ = models
    Bm, T0 = 2, 40
    seq = torch.randint(0, 512, (Bm, T0 + 150), generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = gpu.new_cache(Bm, 190, kv_dtype=FP8), gpu.new_cache(Bm, 190, kv_dtype=FP8)
    gpu.prefill(seq[:, :T0], a)
    gpu.prefill(seq[:, :T0], b)
    at = T0
    for T in (50, 100):
        want = gpu.extend(seq[:, at:at + T], a)
        got = gpu.extend(seq[:, at:at + T], b, chunk=32)
        err = (got.float() - want.float()).abs().max().item()
        print(f"fp8 cache, chunked against 16-row extend, T={T}: max-abs {err:.4f}")
        assert err < 0.1, err
        at += T


def test_chunked_extend_from_an_empty_cache_and_ragged_rows(models):
    gpu, ref, _ = models
    seq = torch.randint(0, 512, (2, 120), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = ref(seq)
    cache = gpu.new_cache(2, 120)
    first = gpu.extend(seq[:, :50].to(DEV), cache, chunk=32).float().cpu()  # like a prefill
    assert (first - want[:, :50]).abs().max().item() < 0.1
    last = gpu.extend(seq[:, 50:70].to(DEV), cache, last_only=True, chunk=32).float().cpu()
    assert last.shape == (2, 512) and (last - want[:, 69]).abs().max().item() < 0.1
    cache.set_lens([70, 21])  # row 1 goes back to position 21: positions come from cache.lens per row
    nxt = torch.stack([seq[0, 70:110], seq[1, 21:61]]).to(DEV)
    lg = gpu.extend(nxt, cache, chunk=32).float().cpu()
    assert (lg[0] - want[0, 70:110]).abs().max().item() < 0.1
    assert (lg[1] - want[1, 21:61]).abs().max().item() < 0.1
    assert cache.lens.tolist() == [110, 61]


def test_graphed_chunked_extend_equals_eager(models):
    """extend(chunk=32) at T = 32 captured once on a pinned cache and replayed at three positions: logits
    bit-identical to the eager step."""
    from kubeflow_rm_amd import ops
    gpu, _, _ = models
    Bm, T, cap = 2, 32, 128
    cache = gpu.new_cache(Bm, cap)
    cache.pin_bound()  # the captured attention grid covers the whole capacity
    step = ops.GraphedCallable(lambda t: gpu.extend(t, cache, chunk=32),
                               torch.zeros(Bm, T, dtype=torch.long, device=DEV), warmup=1)
    torch.cuda.synchronize()
    for seed, T0 in ((1, 40), (2, 65), (3, 17)):
        seq = torch.randint(0, 512, (Bm, T0 + T), generator=torch.Generator().manual_seed(seed)).to(DEV)
        eager = gpu.new_cache(Bm, cap)
        gpu.prefill(seq[:, :T0], eager)
        want = gpu.extend(seq[:, T0:], eager, chunk=32)
        cache.reset()
        gpu.prefill(seq[:, :T0], cache)
        got = step(seq[:, T0:])
        torch.testing.assert_close(got, want, rtol=0, atol=0)
        assert cache.lens.tolist() == [T0 + T] * Bm


def test_generate_with_a_chunked_prefill(models):
    """Greedy generate(prefill_chunk=32): the right shape and prompt, and every emitted token within 0.2 of the
    best fp32 logit at its position (twice the 0.1 logit bound: the emitted and the best may both be off)."""
    gpu, ref, _ = models
    T0, new = 70, 16
    idx = torch.randint(0, 512, (2, T0), generator=torch.Generator().manual_seed(1)).to(DEV)
    out = gpu.generate(idx, new, prefill_chunk=32)
    assert out.shape == (2, T0 + new) and torch.equal(out[:, :T0], idx)
    with torch.no_grad():
        want = ref(out.cpu())  # logits[t] predict token t + 1
    toks = out.cpu()
    for b in range(2):
        for t in range(T0 - 1, T0 + new - 1):
            gap = (want[b, t].max() - want[b, t, toks[b, t + 1]]).item()
            assert gap <= 0.2, (b, t, gap)
    with pytest.raises(ValueError):
        gpu.generate(idx[:1], 4, prefill_chunk=32, draft=gpu)
