"""Sliding-window attention on the gfx950 KV-cache kernels: attention_decode / attention_extend / attention_chunk
with ``window=W`` (plain and grouped rows, bf16 and FP8 caches) against an fp32 masked softmax written from the rule
of ``ops/decode.py`` (a row of causal limit L sees key j iff max(0, L - W) <= j < L), row by row; poison outside
every row's window; guard rows around ``out``; bit equality with the unwindowed launch when nothing is removed;
splits that hold no key; and a windowed GPT through prefill / decode_step / extend / generate.

Bounds: ABS / REL / LSE are those tests/test_gpu_extend.py (_check), test_gpu_attn_chunk.py, test_gpu_kv_fp8.py
(_check_attn) and test_gpu_gqa.py assert for the same ops against the same kind of reference (fp32 SDPA per row on
the stored values): max-abs < 2e-2, rel-l2 < 8e-3, lse within 1e-3. LOGITS is the 0.1 of tests/test_gpu_decode.py /
test_gpu_extend.py on bf16 logits."""
from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV = 3, 2
FP8 = torch.float8_e4m3fn
KINDS = ["bf16", "fp8"]
ABS, REL, LSE = 2e-2, 8e-3, 1e-3  # tests/test_gpu_gqa.py, test_gpu_attn_chunk.py (ABS, REL, LSE); test_gpu_extend.py _check
LOGITS = 0.1  # tests/test_gpu_decode.py, test_gpu_extend.py: bf16 logits


def _S():
    from kubeflow_rm_amd.ops import decode
    return decode.SPLIT_KEYS


def _cap():
    return 2 * _S() + 40


def _windows():
    S = _S()
    return [1, 5, 64, S - 1, S + 3, _cap()]


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


_CACHES: dict = {}


def _cache(D, kind):
    """(cache, k, v) of capacity 2 S + 40, the source rows drawn once per (D, kind): k, v [B, HKV, cap, D] are what the
    reference attends (for FP8 the dequantised stored codes), clean copies. Tests poison the cache, so every use
    refills it."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.decode import dequantize_rows
    cap = _cap()
    if (D, kind) not in _CACHES:
        c = ops.KVCache(1, B, HKV, D, cap, device=DEV, dtype=FP8 if kind == "fp8" else torch.bfloat16)
        k, v = _randn(B, HKV, cap, D, seed=D), _randn(B, HKV, cap, D, seed=D + 1)
        qkv = torch.stack([torch.zeros_like(k), k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, cap, 3 * HKV * D)
        _CACHES[D, kind] = (c, qkv.contiguous())
    c, qkv = _CACHES[D, kind]
    c.reset()
    ops.kv_append(qkv, c, 0)
    if c.fp8:
        return c, dequantize_rows(c.k[0], c.k_scale[0]), dequantize_rows(c.v[0], c.v_scale[0])
    return c, c.k[0].clone(), c.v[0].clone()


def _limits(lens, T):
    """L [B, T]: the causal limit of row i, lens[b] - T + i + 1."""
    return torch.tensor(lens, device=DEV).view(-1, 1) - T + torch.arange(T, device=DEV).view(1, T) + 1


def _seen(lens, T, W, cap):
    """[B, T, cap] bool, straight from the rule: key j for row i iff max(0, L - W) <= j < L."""
    L = _limits(lens, T).unsqueeze(-1)
    j = torch.arange(cap, device=DEV).view(1, 1, cap)
    lo = torch.zeros_like(L) if W is None else (L - W).clamp_min(0)
    return (j >= lo) & (j < L)


def _ref(q, k, v, lens, W):
    """fp32 masked softmax over the clean k, v [B, HKV, cap, D], query head h on K / V head h // G; a row with no
    key gives zeros, lse = -inf. q [B, T, Hq, D] -> (o [B, T, Hq, D], lse [B, T, Hq])."""
    T, Hq, D = q.shape[1:]
    G = Hq // k.shape[1]
    kf, vf = k.float().repeat_interleave(G, dim=1), v.float().repeat_interleave(G, dim=1)
    s = torch.einsum("bthd,bhjd->bhtj", q.float(), kf) / math.sqrt(D)
    s = s.masked_fill(~_seen(lens, T, W, k.shape[2]).unsqueeze(1), float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.masked_fill(lse == float("-inf"), 0.0).unsqueeze(-1))
    return (p @ vf).transpose(1, 2), lse.transpose(1, 2)


def _poison(cache, lens, T, W):
    """Every cache position outside every row's window, and every position at or beyond lens[b]: NaN, or for an FP8
    cache code 0x7F and NaN scales."""
    dead = ~_seen(lens, T, W, cache.capacity).any(1)  # [B, cap]
    for b in range(cache.B):
        rows = dead[b].nonzero().flatten()
        if cache.fp8:
            cache.k[0].view(torch.uint8)[b, :, rows] = 0x7F
            cache.v[0].view(torch.uint8)[b, :, rows] = 0x7F
            cache.k_scale[0][b, :, rows] = float("nan")
            cache.v_scale[0][b, :, rows] = float("nan")
        else:
            cache.k[0][b, :, rows] = float("nan")
            cache.v[0][b, :, rows] = float("nan")


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _check(o, lse, ref, ref_lse, what):
    err, rel = (o.float() - ref).abs().max().item(), _rel(o, ref)
    live = torch.isfinite(ref_lse)
    lerr = (lse[live] - ref_lse[live]).abs().max().item() if live.any() else 0.0
    print(f"window {what}: max-abs {err:.3e} rel-l2 {rel:.3e} lse {lerr:.3e}")
    assert torch.isfinite(o.float()).all(), what
    assert err < ABS and rel < REL, (what, err, rel)
    assert torch.equal(torch.isfinite(lse), live) and lerr < LSE, (what, lerr)


SENTINEL = 123.0


def _guarded(q):
    """(buffer, out): ``out`` of q's shape as a strided view inside a larger sentinel-filled buffer, one guard row
    of heads before and after every token's and every batch row's rows."""
    if q.dim() == 4:
        Bq, T, Hq, D = q.shape
        buf = torch.full((Bq, T + 2, Hq + 2, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
        return buf, buf[:, 1:T + 1, 1:Hq + 1]
    Bq, Hq, D = q.shape
    buf = torch.full((Bq, Hq + 2, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    return buf, buf[:, 1:Hq + 1]


def _guards_intact(buf, out):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep.as_strided(out.shape, out.stride(), out.storage_offset() - buf.storage_offset()).fill_(False)
    return bool((buf[keep] == SENTINEL).all())


def _run(op, q, cache, k, v, lens, W, what, t_bounds=None):
    """One (lens, W) case of an op: poison, the call with ``out=`` into guarded memory and the returning call, both
    against the reference, for the tight grid and the capacity's."""
    T = q.shape[1] if q.dim() == 4 else 1
    cache.set_lens(lens)
    _poison(cache, lens, T, W)
    ref, ref_lse = _ref(q if q.dim() == 4 else q.unsqueeze(1), k, v, lens, W)
    if q.dim() == 3:
        ref, ref_lse = ref[:, 0], ref_lse[:, 0]
    for t_bound in t_bounds or (max(lens), cache.capacity):
        o, lse = op(q, cache, 0, t_bound=t_bound, return_lse=True, window=W)
        assert o.shape == q.shape and lse.shape == q.shape[:-1]
        _check(o, lse, ref, ref_lse, f"{what} lens={lens} W={W} t_bound={t_bound}")
        buf, out = _guarded(q)
        assert op(q, cache, 0, t_bound=t_bound, out=out, window=W) is out
        assert torch.equal(out, o), what  # the same launch: the same bits
        assert _guards_intact(buf, out), what


def _lens_cases(T):
    S = _S()
    return [[T, S - 1, 2 * S + 7], [S + 2, 2 * S + 7, S - 1]]


# ---- the three ops, plain rows -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_window(D, kind):
    from kubeflow_rm_amd import ops
    q = _randn(B, HKV, D, seed=3)
    for W in _windows():
        for lens in _lens_cases(1):
            cache, k, v = _cache(D, kind)
            _run(ops.attention_decode, q, cache, k, v, lens, W, f"decode D={D} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tq", [2, 3, 8, 11, 16])
def test_extend_window(Tq, D, kind):
    from kubeflow_rm_amd import ops
    q = _randn(B, Tq, HKV, D, seed=10 + Tq)
    for W in _windows():
        for lens in _lens_cases(Tq):
            cache, k, v = _cache(D, kind)
            _run(ops.attention_extend, q, cache, k, v, lens, W, f"extend Tq={Tq} D={D} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [17, 130])
def test_chunk_window(T, D, kind):
    from kubeflow_rm_amd import ops
    S = _S()
    q = _randn(B, T, HKV, D, seed=30 + T)
    lens = [T, 50 + T, S + 9 + T]  # 0, 50 and S + 9 prior keys
    for W in _windows():
        cache, k, v = _cache(D, kind)
        _run(ops.attention_chunk, q, cache, k, v, lens, W, f"chunk T={T} D={D} {kind}")


# ---- grouped rows, on both sides of the cut-over -----------------------------------------------------
GT_VALU = [(2, 1), (2, 3), (4, 1)]  # fewer than GQA_MFMA_MIN_ROWS rows: the extend kernel's row slots as routed
GT_MFMA = [(2, 4), (4, 2), (8, 1), (4, 4), (8, 2)]  # from 8 rows on: the MFMA kernel as routed


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G,T,forced", [(g, t, False) for g, t in GT_VALU + GT_MFMA] + [(8, 1, True), (8, 2, True),
                                                                                       (4, 3, True)])
def test_grouped_window(G, T, forced, D, kind, monkeypatch):
    """``forced``: the VALU form at a row count the routing gives to the MFMA form (G = 8 has no other way there)."""
    from kubeflow_rm_amd import ops
    assert ops.decode.GQA_MFMA_MIN_ROWS == 8
    if forced:
        monkeypatch.setattr(ops.decode, "GQA_MFMA_MIN_ROWS", None)
    q = _randn(B, T, G * HKV, D, seed=50 + 7 * G + T)
    for W in _windows():
        for lens in _lens_cases(T):
            cache, k, v = _cache(D, kind)
            _run(ops.attention_extend, q, cache, k, v, lens, W, f"grouped extend G={G} T={T} D={D} {kind}",
                 t_bounds=(cache.capacity,))
            if T == 1:  # decode with G > 1 is the same launch on the group's G rows
                cache, k, v = _cache(D, kind)
                _run(ops.attention_decode, q[:, 0], cache, k, v, lens, W, f"grouped decode G={G} D={D} {kind}",
                     t_bounds=(cache.capacity,))
    cache, k, v = _cache(D, kind)  # and the MFMA kernel on grouped rows that cross a 32-row wave: 40 tokens
    qc = _randn(B, 40, G * HKV, D, seed=90 + G)
    for W in (5, _S() + 3):
        cache, k, v = _cache(D, kind)
        _run(ops.attention_chunk, qc, cache, k, v, [40, _S() + 2, 2 * _S() + 7], W, f"grouped chunk G={G} D={D} {kind}",
             t_bounds=(cache.capacity,))


# ---- nothing but removal -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_a_window_that_removes_nothing_changes_no_bit(D, kind):
    """W >= every row's limit: only keys were to be removed, and none were. W = capacity - 1 under the capacity's
    grid runs the windowed kernels (W < t_bound); W = capacity the unwindowed ones."""
    from kubeflow_rm_amd import ops
    S, cap = _S(), _cap()
    lens = [S - 1, S + 2, 2 * S + 7]
    calls = [(ops.attention_decode, _randn(B, HKV, D, seed=1), lens),
             (ops.attention_decode, _randn(B, 4 * HKV, D, seed=2), lens),
             (ops.attention_extend, _randn(B, 3, HKV, D, seed=3), lens),
             (ops.attention_extend, _randn(B, 11, HKV, D, seed=4), lens),
             (ops.attention_extend, _randn(B, 3, 2 * HKV, D, seed=5), lens),
             (ops.attention_chunk, _randn(B, 17, HKV, D, seed=6), lens),
             (ops.attention_chunk, _randn(B, 130, HKV, D, seed=7), [130, 180, S + 139]),
             (ops.attention_chunk, _randn(B, 40, 4 * HKV, D, seed=8), lens)]
    for op, q, ls in calls:
        cache, _, _ = _cache(D, kind)
        cache.set_lens(ls)
        o, lse = op(q, cache, 0, t_bound=cap, return_lse=True)
        for W in (cap - 1, cap, 2 * S + 7):
            ow, lsew = op(q, cache, 0, t_bound=cap, return_lse=True, window=W)
            assert torch.equal(ow, o) and torch.equal(lsew, lse), (op.__name__, tuple(q.shape), W)


# ---- splits that hold no key ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_splits_below_the_window_are_empty(D, kind):
    """lens = 2 S + 7, W = 5: the first two splits hold no key for any row (Tq = 1: the single-row kernel; Tq = 8:
    eight row slots; and the MFMA kernel)."""
    from kubeflow_rm_amd import ops
    lens = [2 * _S() + 7] * B
    for op, q in ((ops.attention_decode, _randn(B, HKV, D, seed=1)),
                  (ops.attention_extend, _randn(B, 1, HKV, D, seed=2)),
                  (ops.attention_extend, _randn(B, 8, HKV, D, seed=3)),
                  (ops.attention_chunk, _randn(B, 8, HKV, D, seed=4))):
        cache, k, v = _cache(D, kind)
        _run(op, q, cache, k, v, lens, 5, f"empty splits {op.__name__} {tuple(q.shape)} D={D} {kind}")


def test_bad_windows_raise_on_the_gpu():
    from kubeflow_rm_amd import ops
    cache, _, _ = _cache(64, "bf16")
    cache.set_lens([9] * B)
    q = _randn(B, 2, HKV, 64, seed=1)
    for bad in (0, -1, True, 3.0):
        for call in (lambda: ops.attention_decode(q[:, 0], cache, 0, window=bad),
                     lambda: ops.attention_extend(q, cache, 0, window=bad),
                     lambda: ops.attention_chunk(q, cache, 0, window=bad)):
            with pytest.raises(ValueError):
                call()


# ---- the model -----------------------------------------------------------------------------------
W_MODEL = 7


def _cfg(n_heads, window, **kw):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=n_heads, d_ff=1024, max_seq=256,
                     dtype=torch.bfloat16, window=window, **kw)


@pytest.fixture(scope="module", params=[4, 2], ids=["D64", "D128"])
def model(request):
    from kubeflow_rm_amd.models import GPT
    return GPT(_cfg(request.param, W_MODEL), device=DEV).eval()


def _steps(m, seq, T0, cache):
    """decode_step, extend(T = 4), extend(chunk = 32) over 40 tokens, after the prompt: the three logits."""
    at = T0
    a = m.decode_step(seq[:, at], cache)
    b = m.extend(seq[:, at + 1:at + 5], cache)
    c = m.extend(seq[:, at + 5:at + 45], cache, chunk=32)
    assert cache.lens.tolist() == [at + 45] * seq.shape[0]
    return [a.float(), b.float(), c.float()]


@pytest.mark.parametrize("T0", [1, 9, 40])
def test_windowed_model_matches_the_torch_reference_path(model, T0):
    from kubeflow_rm_amd import ops
    Bm = 2
    seq = torch.randint(0, 512, (Bm, T0 + 45), generator=torch.Generator().manual_seed(T0)).to(DEV)
    cache = model.new_cache(Bm, T0 + 45)
    got = [model.prefill(seq[:, :T0], cache).float()] + _steps(model, seq, T0, cache)
    with ops.torch_reference():
        rc = model.new_cache(Bm, T0 + 45)
        want = [model.prefill(seq[:, :T0], rc).float()] + _steps(model, seq, T0, rc)
    for name, g, w in zip(("prefill", "decode_step", "extend(4)", "extend(chunk=32)"), got, want):
        err = (g - w).abs().max().item()
        print(f"windowed model T0={T0} {name}: max-abs {err:.4f}")
        assert g.shape == w.shape and err < LOGITS, (name, err)
    # the FP8 cache: both caches filled by the reference prefill (the windowed GPU prefill attends the quantised
    # rows, so its logits are not the reference's, and it is left out), then the same three steps
    with ops.torch_reference():
        c8, r8 = model.new_cache(Bm, T0 + 45, kv_dtype=FP8), model.new_cache(Bm, T0 + 45, kv_dtype=FP8)
        model.prefill(seq[:, :T0], c8)
        model.prefill(seq[:, :T0], r8)
        want8 = _steps(model, seq, T0, r8)
    got8 = _steps(model, seq, T0, c8)
    for name, g, w in zip(("decode_step", "extend(4)", "extend(chunk=32)"), got8, want8):
        err = (g - w).abs().max().item()
        print(f"windowed model fp8 cache T0={T0} {name}: max-abs {err:.4f}")
        assert err < LOGITS, (name, err)


def test_windowed_generate_graph_fused_sampler_and_the_rest(model):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT
    idx = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    eager = model.generate(idx, 10)
    assert eager.shape == (2, 22) and torch.equal(eager[:, :12], idx)
    assert torch.equal(model.generate(idx, 10, graph=True), eager)  # graphed_decode_step needs no other change
    kw = dict(sampler="fused", temperature=0.8, top_k=20, top_p=0.9)
    a = model.generate(idx, 10, generator=torch.Generator().manual_seed(3), graph=True, **kw)
    b_ = model.generate(idx, 10, generator=torch.Generator().manual_seed(3), **kw)
    assert a.shape == (2, 22) and torch.equal(a, b_)
    for extra in (dict(kv_dtype=FP8), dict(weight_dtype=FP8), dict(prefill_chunk=17)):
        a = model.generate(idx, 10, generator=torch.Generator().manual_seed(3), graph=True, **kw, **extra)
        b_ = model.generate(idx, 10, generator=torch.Generator().manual_seed(3), **kw, **extra)
        assert torch.equal(a, b_), extra
    # a draft with no window of its own, and one with another window: the target decides. As in
    # tests/test_gpu_extend.py's draft test, every emitted token is within 2 * LOGITS of the best logit of the
    # windowed torch-reference forward at its position (the emitted and the best logit may both be off by LOGITS)
    for dw in (None, 3):
        draft = GPT(_cfg(model.cfg.n_heads, dw), device=DEV).eval()
        out = model.generate(idx[:1], 10, draft=draft, lookahead=3)
        assert out.shape == (1, 22) and torch.equal(out[:, :12], idx[:1])
        with ops.torch_reference(), torch.no_grad():
            want = model(out)[0].float()  # logits[t] predict token t + 1
        for t in range(11, 21):
            assert want[t].max().item() - want[t, out[0, t + 1]].item() < 2 * LOGITS, (dw, t)


def test_windowed_llama_style_model_generates(model):
    """GQA + rotary + RMSNorm / SwiGLU compose by shapes only: graph replay equals the eager call."""
    from kubeflow_rm_amd.models import GPT
    m = GPT(_cfg(4, W_MODEL, n_kv_heads=2, pos="rope", norm="rms", mlp="swiglu"), device=DEV).eval()
    idx = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(2)).to(DEV)
    eager = m.generate(idx, 10)
    assert torch.equal(m.generate(idx, 10, graph=True), eager)
    kw = dict(sampler="fused", temperature=0.8, top_k=20, top_p=0.9, kv_dtype=FP8)
    assert torch.equal(m.generate(idx, 10, generator=torch.Generator().manual_seed(3), graph=True, **kw),
                       m.generate(idx, 10, generator=torch.Generator().manual_seed(3), **kw))


def test_unwindowed_generation_is_repeatable():
    from kubeflow_rm_amd.models import GPT
    m = GPT(_cfg(4, None), device=DEV).eval()
    idx = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(m.generate(idx, 10), m.generate(idx, 10))
    assert torch.equal(m.generate(idx, 10, graph=True), m.generate(idx, 10, graph=True))


def test_native_training_forward_of_a_windowed_model_raises(model):
    from kubeflow_rm_amd import ops
    idx = torch.randint(0, 512, (2, 16), generator=torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(NotImplementedError, match="flash"):
        model(idx)
    with ops.torch_reference(), torch.no_grad():  # the torch path applies the mask
        assert model(idx).shape == (2, 16, 512)
