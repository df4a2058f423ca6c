"""Multi-token KV-cache steps on the gfx950 kernels: attention_extend (kernels/attn_kv.hip: Tq <= 16
new query rows per head over the cache, causal inside the new block), KVCache.rewind, GPT.extend and
draft-and-verify generate, against fp32 references."""
from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 3


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _S():
    from kubeflow_rm_amd.ops import decode
    return decode.SPLIT_KEYS


def _cache(D, seed, Bc=B, Hc=H, cap=None):
    from kubeflow_rm_amd import ops
    cap = 3 * _S() + 8 if cap is None else cap
    c = ops.KVCache(1, Bc, Hc, D, cap, device=DEV)
    c.k[0].copy_(_randn(Bc, Hc, cap, D, seed=seed))
    c.v[0].copy_(_randn(Bc, Hc, cap, D, seed=seed + 1))
    return c


def _ref_extend(q, k, v, lens, extra=0):
    """fp32 SDPA per (b, row) over that row's own key prefix 0 .. lens[b]-Tq+i (same bf16 inputs); a row
    with no key gives zeros, lse = -inf. ``extra``: keys past the limit each row attends too (the leak
    a test wants to be able to see), capped at lens[b]. Returns (o [B, Tq, H, D], lse [B, Tq, H])."""
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
    """The bounds of the single-query decode attention (tests/test_gpu_decode.py _check_decode): every
    query row is a single-query attention over its own prefix, on the same fp32 VALU arithmetic."""
    err = (o.float() - ref).abs().max().item()
    rel = _rel(o, ref)
    print(f"extend attention {what}: max-abs {err:.3e} rel-l2 {rel:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < 2e-2, err
    assert rel < 8e-3, rel


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tq", [1, 2, 5, 16])
def test_extend_attention_split_edges_and_causal_diagonal(D, Tq):
    """The new block before, on and across a split boundary, with several splits; the LSE; two calls
    bitwise equal; with lens == Tq row 0 sees one key and returns V row 0 bit for bit."""
    from kubeflow_rm_amd import ops
    S = _S()
    cache = _cache(D, seed=100 + D)
    q = _randn(B, Tq, H, D, seed=Tq)
    for lens in ([Tq, S - 1], [S, S + 1], [S + Tq - 1, 2 * S + 3]):
        cache.set_lens(lens)
        ref, ref_lse = _ref_extend(q, cache.k[0], cache.v[0], lens)
        for t_bound in (max(lens), cache.capacity):  # the tight grid, and one with empty trailing splits
            o, lse = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
            assert o.shape == (B, Tq, H, D) and lse.shape == (B, Tq, H)
            _check(o, ref, f"Tq={Tq} lens={lens} t_bound={t_bound}")
            assert (lse - ref_lse).abs().max().item() < 1e-3
            again, lse2 = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
            assert torch.equal(again, o) and torch.equal(lse2, lse)
            if lens[0] == Tq:  # softmax of one key is exactly 1
                assert torch.equal(o[0, 0], cache.v[0][0, :, 0])


@pytest.mark.parametrize("D", [64, 128])
def test_extend_attention_rows_before_the_sequence_start(D):
    """lens < Tq: the leading rows have no key: zeros and lse = -inf; the others match the reference."""
    from kubeflow_rm_amd import ops
    S = _S()
    Tq = 5
    cache = _cache(D, seed=110 + D)
    q = _randn(B, Tq, H, D, seed=7)
    for lens, t_bound in (([2, 0], 2), ([3, S + 2], S + 2), ([0, 4], cache.capacity)):
        cache.set_lens(lens)
        ref, ref_lse = _ref_extend(q, cache.k[0], cache.v[0], lens)
        o, lse = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
        _check(o, ref, f"lens={lens}")
        for b, n in enumerate(lens):
            dead = max(Tq - n, 0)
            assert (o[b, :dead] == 0).all() and (lse[b, :dead] == float("-inf")).all()
            assert torch.isfinite(lse[b, dead:]).all()
            if dead < Tq:
                assert (lse[b, dead:] - ref_lse[b, dead:]).abs().max().item() < 1e-3


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tq", [5, 16])
def test_extend_attention_does_not_leak(D, Tq):
    """Cache rows at or beyond lens hold NaN: the outputs stay finite and in bounds. The K rows of the
    new block are scaled so that a row attending one key past its causal limit would move its output
    by far more than the bound (shown on the reference itself)."""
    from kubeflow_rm_amd import ops
    S = _S()
    lens = [S + 2, 2 * S + Tq - 1]  # the block across a split boundary; the block ending a split
    cache = _cache(D, seed=120 + D)
    q = _randn(B, Tq, H, D, seed=9)
    k = cache.k[0]
    for b, n in enumerate(lens):
        for j in range(1, Tq):  # the key of block row j is aligned with the query of row j - 1
            p = n - Tq + j
            k[b, :, p] = (k[b, :, p].float().abs() * torch.sign(q[b, j - 1].float()) * 30).to(torch.bfloat16)
        k[b, :, n:] = float("nan")
        cache.v[0][b, :, n:] = float("nan")
    cache.set_lens(lens)
    ref, _ = _ref_extend(q, k, cache.v[0], lens)
    leaky, _ = _ref_extend(q, k, cache.v[0], lens, extra=1)
    moved = (leaky - ref)[:, :Tq - 1].abs().amax(dim=(2, 3))  # per (b, row) but the last, which has no next key
    assert moved.min().item() >= 10 * 2e-2, moved
    o = ops.attention_extend(q, cache, 0, t_bound=cache.capacity)
    assert torch.isfinite(o.float()).all()
    _check(o, ref, f"Tq={Tq} spiked block keys, NaN beyond lens")


@pytest.mark.parametrize("D", [64, 128])
def test_extend_attention_strided_q_and_out_no_stray_writes(D):
    """q read in place from the fused QKV output [B, T, 3, H, D]; o written into a view inside a larger
    sentinel-filled buffer, by the combine launch (two splits) and by the split kernel itself (one)."""
    from kubeflow_rm_amd import ops
    S = _S()
    Tq = 5
    cache = _cache(D, seed=130 + D)
    qkv = _randn(B, Tq, 3, H, D, seed=61)
    q = qkv[:, :, 0]
    assert not q.is_contiguous()
    for lens in ([S + 9, 40], [40, 17]):
        cache.set_lens(lens)
        want = ops.attention_extend(q.contiguous(), cache, 0)
        buf = torch.full((B + 2, Tq + 1, H * D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
        out = buf[1:B + 1, :Tq, 8:].view(B, Tq, H, D)
        got = ops.attention_extend(q, cache, 0, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out, want)
        _check(got, _ref_extend(q, cache.k[0], cache.v[0], lens)[0], f"strided lens={lens}")
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:B + 1, :Tq, 8:] = False
        assert (buf[keep] == 7.0).all()  # every element outside the view is unchanged


def test_extend_attention_contract_violations_raise():
    import ctypes
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    cache = _cache(64, seed=1, cap=64)
    cache.set_lens([20, 20])
    with pytest.raises(ValueError):
        ops.attention_extend(_randn(B, 0, H, 64, seed=1), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_extend(_randn(B, 17, H, 64, seed=1), cache, 0)
    q = _randn(B, 4, H, 64, seed=1)
    with pytest.raises(ValueError):
        ops.attention_extend(q, cache, 0, lens=cache.lens.long())
    with pytest.raises(ValueError):
        ops.attention_extend(q, cache, 0, lens=cache.lens.cpu())
    for t_bound in (0, 65):
        with pytest.raises(ValueError):
            ops.attention_extend(q, cache, 0, t_bound=t_bound)
    with pytest.raises(ValueError):
        ops.attention_extend(q.float(), cache, 0)
    c96 = ops.KVCache(1, 1, 2, 96, 64, device=DEV)
    c96.set_lens([8])
    q96 = _randn(1, 4, 2, 96, seed=1)
    with pytest.raises(ValueError):
        ops.attention_extend(q96, c96, 0)
    # the library itself
    L = _lib.lib()
    assert L.kfamd_attn_extend_workspace(1, 2, 96, 4, 64) == 0
    assert L.kfamd_attn_extend_workspace(1, 2, 64, 17, 64) == 0
    assert L.kfamd_attn_extend_workspace(2, 3, 64, 5, 600) == 5 * L.kfamd_attn_decode_workspace(2, 3, 64, 600)
    o = torch.empty_like(q)

    def call(qt, c, D, Tq, t_bound, ws=None, q_off=0):
        st = (ctypes.c_longlong * 12)(*qt.stride()[:3], *c.k[0].stride()[:3], *c.v[0].stride()[:3], *qt.stride()[:3])
        return L.kfamd_attn_extend_bf16(qt.data_ptr() + q_off, c.k[0].data_ptr(), c.v[0].data_ptr(), c.lens.data_ptr(),
                                        o.data_ptr(), None, ws, qt.shape[0], qt.shape[2], D, Tq, t_bound, 1.0, st, None)

    assert call(q96, c96, 96, 4, 8) == -1
    assert call(q, cache, 64, 0, 20) == -1
    assert call(q, cache, 64, 17, 20) == -1
    assert call(q, cache, 64, 4, 0) == -1
    assert call(q, cache, 64, 4, _S() + 1) == -1  # two splits need the workspace
    assert call(q, cache, 64, 4, 20, q_off=2) == -2


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


def test_teacher_forced_extend_matches_fp32_full_forward(models):
    """prefill, then extend with M = B * T = 2, 6, 32, 8 rows (the weight-streaming GEMM up to 16 rows,
    the "auto" route above) and one call of 20 tokens (chunks of 16 + 4): the bound of the decode test."""
    gpu, ref, _ = models
    Bm, T0, steps = 2, 40, (1, 3, 16, 4, 20)
    total = T0 + sum(steps)
    seq = torch.randint(0, 512, (Bm, total), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)  # fp32 CPU logits at every position
    cache = gpu.new_cache(Bm, total)
    got, at = [gpu.prefill(seq[:, :T0].to(DEV), cache).view(Bm, 1, -1)], T0
    for T in steps:
        lg = gpu.extend(seq[:, at:at + T].to(DEV), cache)
        assert lg.shape == (Bm, T, 512)
        got.append(lg)
        at += T
        assert cache.lens.tolist() == [at] * Bm
    got = torch.cat(got, 1).float().cpu()
    errs = (got - want[:, T0 - 1:]).abs().amax(dim=(0, 2))
    print(f"extend per-position max-abs: max {errs.max().item():.4f} {[round(e, 3) for e in errs.tolist()]}")
    assert errs.max().item() < 0.1, errs.tolist()
    assert cache.lens.tolist() == [total] * Bm
    with pytest.raises(ValueError):
        gpu.extend(seq[:, :1].to(DEV), cache)  # the cache is full


def test_extend_from_an_empty_cache_and_ragged_rows(models):
    gpu, ref, _ = models
    seq = torch.randint(0, 512, (2, 40), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = ref(seq)
    cache = gpu.new_cache(2, 40)
    first = gpu.extend(seq[:, :12].to(DEV), cache).float().cpu()  # like a prefill
    assert (first - want[:, :12]).abs().max().item() < 0.1
    last = gpu.extend(seq[:, 12:14].to(DEV), cache, last_only=True).float().cpu()
    assert last.shape == (2, 512) and (last - want[:, 13]).abs().max().item() < 0.1
    cache.set_lens([14, 7])  # row 1 goes back to position 7: positions come from cache.lens per row
    nxt = torch.stack([seq[0, 14:19], seq[1, 7:12]]).to(DEV)
    lg = gpu.extend(nxt, cache).float().cpu()
    assert (lg[0] - want[0, 14:19]).abs().max().item() < 0.1
    assert (lg[1] - want[1, 7:12]).abs().max().item() < 0.1
    assert cache.lens.tolist() == [19, 12]
    step = gpu.decode_step(torch.stack([seq[0, 19], seq[1, 12]]).to(DEV), cache).float().cpu()
    assert (step[0] - want[0, 19]).abs().max().item() < 0.1 and (step[1] - want[1, 12]).abs().max().item() < 0.1


def test_rewind_then_extend_is_bit_identical(models):
    gpu, _, _ = models
    seq = torch.randint(0, 512, (2, 30), generator=torch.Generator().manual_seed(3)).to(DEV)
    junk = torch.randint(0, 512, (2, 4), generator=torch.Generator().manual_seed(4)).to(DEV)
    a, b = gpu.new_cache(2, 40), gpu.new_cache(2, 40)
    gpu.prefill(seq[:, :20], a)
    gpu.prefill(seq[:, :20], b)
    want = gpu.extend(seq[:, 20:24], a)
    gpu.extend(junk, b)
    b.rewind(4)
    assert b.lens.tolist() == [20, 20] and b.t_bound == 20
    got = gpu.extend(seq[:, 20:24], b)
    assert torch.equal(got, want)
    assert torch.equal(gpu.extend(seq[:, 24:30], b), gpu.extend(seq[:, 24:30], a))


def test_graphed_extend_equals_eager(models):
    """extend at T = 4 captured once (nothing in it depends on a host-side position) and replayed at
    three positions: logits bit-identical to the eager step."""
    from kubeflow_rm_amd import ops
    gpu, _, _ = models
    Bm, T, cap = 2, 4, 64
    cache = gpu.new_cache(Bm, cap)
    cache.pin_bound()  # the captured attention grid covers the whole capacity
    step = ops.GraphedCallable(lambda t: gpu.extend(t, cache), torch.zeros(Bm, T, dtype=torch.long, device=DEV),
                               warmup=1)
    torch.cuda.synchronize()
    for seed, T0 in ((1, 40), (2, 33), (3, 17)):
        seq = torch.randint(0, 512, (Bm, T0 + T), generator=torch.Generator().manual_seed(seed)).to(DEV)
        eager = gpu.new_cache(Bm, cap)
        gpu.prefill(seq[:, :T0], eager)
        want = gpu.extend(seq[:, T0:], eager)
        cache.reset()
        gpu.prefill(seq[:, :T0], cache)
        got = step(seq[:, T0:])
        torch.testing.assert_close(got, want, rtol=0, atol=0)
        assert cache.lens.tolist() == [T0 + T] * Bm


def test_draft_and_verify_generate(models):
    """Greedy draft decoding on bf16: each emitted token is within 0.2 of the best fp32 logit at its
    position (twice the 0.1 logit bound: the emitted and the best logit may both be off by it). The
    acceptance rate of an untrained one-layer draft is printed, not asserted."""
    from kubeflow_rm_amd.models import GPT
    gpu, ref, n_heads = models
    draft = GPT(_cfg(n_heads, torch.bfloat16, n_layers=1), device=DEV).eval()
    T0, new = 24, 24
    idx = torch.randint(0, 512, (1, T0), generator=torch.Generator().manual_seed(1)).to(DEV)
    out, stats = gpu.generate(idx, new, draft=draft, lookahead=4, return_stats=True)
    print(f"draft decoding stats: {stats}")
    assert out.shape == (1, T0 + new) and torch.equal(out[:, :T0], idx)
    assert stats["target_steps"] >= math.ceil(new / 5) and 0 <= stats["accepted"] <= stats["proposed"]

    def check_tokens(seq):
        with torch.no_grad():
            want = ref(seq.cpu())[0]  # logits[t] predict token t + 1
        toks = seq[0].cpu()
        for t in range(T0 - 1, T0 + new - 1):
            gap = (want[t].max() - want[t, toks[t + 1]]).item()
            assert gap <= 0.2, (t, gap)

    check_tokens(out)
    self_out, self_stats = gpu.generate(idx, new, draft=gpu, lookahead=4, return_stats=True)
    print(f"self-draft stats: {self_stats}")
    assert self_out.shape == (1, T0 + new) and torch.equal(self_out[:, :T0], idx)
    check_tokens(self_out)
    for kw in ({"temperature": 0.8}, {"graph": True}):
        with pytest.raises(ValueError):
            gpu.generate(idx, 4, draft=draft, **kw)
    with pytest.raises(ValueError):
        gpu.generate(torch.cat([idx, idx]), 4, draft=draft)  # B = 2
