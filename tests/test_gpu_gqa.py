"""Grouped-query attention on the gfx950 kernels: the VALU form (attn_extend_split on T * G row slots), the MFMA
form (attn_chunk_split tiling the T * G rows), the grouped append, the refusals and a GQA GPT through prefill /
extend / generate. The reference is per-row fp32 SDPA over the K / V of head h // G (tests/test_gpu_attn_chunk.py's
_ref on the expanded K / V); the bounds are the project's for these kernels: max-abs < 2e-2, rel-l2 < 8e-3, lse
within 1e-3, and 0.1 on bf16 logits against the fp32 CPU model."""
from __future__ import annotations

import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV = 2, 3
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


_CACHES: dict = {}


def _cache(D, kind):
    """(cache, k, v) of capacity 3 * S + 8, filled once per (D, kind) and shared: k, v [B, HKV, cap, D] are what
    the reference attends (for FP8 the dequantised stored codes). Tests poison the tail, so every use refills."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.decode import dequantize_rows
    cap = 3 * _S() + 8
    if (D, kind) not in _CACHES:
        c = ops.KVCache(1, B, HKV, D, cap, device=DEV, dtype=FP8 if kind == "fp8" else torch.bfloat16)
        k, v = _randn(B, HKV, cap, D, seed=D), _randn(B, HKV, cap, D, seed=D + 1)
        qkv = torch.stack([torch.zeros_like(k), k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, cap, 3 * HKV * D)
        _CACHES[D, kind] = (c, qkv.contiguous())
    c, qkv = _CACHES[D, kind]
    c.reset()
    ops.kv_append(qkv, c, 0)  # the G = 1 append: a copy, or the quantising one
    if c.fp8:
        return c, dequantize_rows(c.k[0], c.k_scale[0]), dequantize_rows(c.v[0], c.v_scale[0])
    return c, c.k[0].clone(), c.v[0].clone()


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
    """fp32 SDPA per (b, token) over the token's own key prefix 0 .. lens[b]-T+i, query head h on K / V head
    h // G; a token with no key gives zeros, lse = -inf. ``extra``: keys past the limit each token attends too,
    capped at lens[b]. Returns (o [B, T, Hq, D], lse [B, T, Hq])."""
    Bq, T, Hq, D = q.shape
    G = Hq // k.shape[1]
    k, v = k.float().repeat_interleave(G, dim=1), v.float().repeat_interleave(G, dim=1)
    o = torch.zeros(Bq, T, Hq, D, device=q.device)
    lse = torch.full((Bq, T, Hq), float("-inf"), device=q.device)
    for b, n in enumerate(lens):
        for i in range(T):
            nk = min(n - T + i + 1 + extra, n)
            if nk <= 0:
                continue
            kk, vv = k[b:b + 1, :, :nk], v[b:b + 1, :, :nk]
            o[b, i] = F.scaled_dot_product_attention(q[b:b + 1, i].float().unsqueeze(2), kk, vv)[0, :, 0]
            s = (q[b, i].float().unsqueeze(1) @ kk[0].transpose(-1, -2)).squeeze(1) / math.sqrt(D)
            lse[b, i] = torch.logsumexp(s, -1)
    return o, lse


def _check(o, lse, ref, ref_lse, what):
    err, rel = (o.float() - ref).abs().max().item(), _rel(o, ref)
    live = torch.isfinite(ref_lse)
    lerr = (lse[live] - ref_lse[live]).abs().max().item() if live.any() else 0.0
    print(f"gqa {what}: max-abs {err:.3e} rel-l2 {rel:.3e} lse {lerr:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < ABS and rel < REL, (what, err, rel)
    assert torch.equal(torch.isfinite(lse), live) and lerr < LSE, (what, lerr)


def _lens_cases(T):
    S = _S()
    return [[T, S - 1], [S, S + 1], [S + T - 1, 2 * S + 3]]


# ---- the VALU form ------------------------------------------------------------------------------
GT = [(2, 1), (4, 1), (8, 1), (16, 1), (2, 3), (2, 5), (4, 3), (4, 4), (8, 2)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G,T", GT)
def test_valu_form_edges(G, T, D, kind, monkeypatch):
    from kubeflow_rm_amd import ops
    monkeypatch.setattr(ops.decode, "GQA_MFMA_MIN_ROWS", None)  # the VALU form at every row count
    q = _randn(B, T, G * HKV, D, seed=7 * G + T)
    for lens in _lens_cases(T):
        cache, k, v = _cache(D, kind)  # refilled: the last case's poison lies inside this one's lens
        cache.set_lens(lens)
        _poison(cache, lens)
        ref, ref_lse = _ref(q, k, v, lens)
        for t_bound in (max(lens), cache.capacity):
            o, lse = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
            _check(o, lse, ref, ref_lse, f"extend G={G} T={T} D={D} {kind} lens={lens} t_bound={t_bound}")
            o2, lse2 = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
            assert torch.equal(o, o2) and torch.equal(lse, lse2)
            if T == 1:  # decode with G > 1 is this body on G row slots
                od, lsed = ops.attention_decode(q[:, 0], cache, 0, t_bound=t_bound, return_lse=True)
                assert torch.equal(od, o[:, 0]) and torch.equal(lsed, lse[:, 0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G,T", [(4, 4), (2, 5)])
def test_limit_follows_the_token_not_the_row(G, T, kind, monkeypatch):
    """A reference in which every row sees one key too many differs from the right one, and from the kernel, by
    more than the bound on every token but the last (whose limit is lens[b] either way): the limit is r / G, not
    r. Few keys per row (lens = T + 2, T + 5), so one more key moves a row by far more than 2e-2; that gap is
    asserted on the fp32 references alone first."""
    from kubeflow_rm_amd import ops
    monkeypatch.setattr(ops.decode, "GQA_MFMA_MIN_ROWS", None)  # attention_extend: the VALU form
    D = 64
    cache, k, v = _cache(D, kind)
    q = _randn(B, T, G * HKV, D, seed=100 + G)
    lens = [T + 2, T + 5]
    cache.set_lens(lens)
    _poison(cache, lens)
    ref, ref_lse = _ref(q, k, v, lens)
    leak, _ = _ref(q, k, v, lens, extra=1)
    gap = (ref - leak).abs().amax(dim=(0, 2, 3))  # per token
    assert (gap[:-1] > 5 * ABS).all() and gap[-1] == 0, gap.tolist()
    for fn in (ops.attention_extend, ops.attention_chunk):
        o, lse = fn(q, cache, 0, return_lse=True)
        _check(o, lse, ref, ref_lse, f"leak G={G} T={T} {kind} {fn.__name__}")
        off = (o.float() - leak).abs().amax(dim=(0, 3))  # [T, Hq]
        assert (off[:-1].amax(1) > ABS).all(), off.tolist()


# ---- the MFMA form ------------------------------------------------------------------------------
def _mfma_cases():
    return [(G, rows // G) for G in (2, 8, 16) for base in (32, 128) for rows in (base - G, base, base + G)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G,T", _mfma_cases())
def test_mfma_form_tiles_of_grouped_rows(G, T, D, kind):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    S = _S()
    cache = _cache(D, kind)[0]
    q = _randn(B, T, G * HKV, D, seed=11 * G + T)
    # across a split boundary (S) and across a 64-key tile boundary inside a split; rows before the start (T > 64)
    for lens, t_bound in (([S + T // 2, 64 + T // 2 + 1], cache.capacity), ([T + 60, 64], T + 64)):
        nsplit = _lib.lib().kfamd_attn_chunk_gqa_nsplit(B, HKV, G, T, t_bound)
        assert nsplit == (1 if t_bound <= S else min(math.ceil(256 / (math.ceil(T * G / 128) * HKV * B)),
                                                     math.ceil(t_bound / S)))
        cache, k, v = _cache(D, kind)  # refilled: the last case's poison lies inside this one's lens
        cache.set_lens(lens)
        _poison(cache, lens)
        ref, ref_lse = _ref(q, k, v, lens)
        o, lse = ops.attention_chunk(q, cache, 0, t_bound=t_bound, return_lse=True)
        _check(o, lse, ref, ref_lse, f"chunk G={G} T={T} D={D} {kind} lens={lens} nsplit={nsplit}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G,T", [(2, 5), (4, 4), (16, 1)])
def test_mfma_form_agrees_with_the_valu_form_up_to_16_rows(G, T, kind, monkeypatch):
    from kubeflow_rm_amd import ops
    monkeypatch.setattr(ops.decode, "GQA_MFMA_MIN_ROWS", None)  # attention_extend: the VALU form
    cache, k, v = _cache(128, kind)
    q = _randn(B, T, G * HKV, 128, seed=3 * G)
    lens = [_S() + 2, 70]
    cache.set_lens(lens)
    _poison(cache, lens)
    a, la = ops.attention_extend(q, cache, 0, return_lse=True)
    c, lc = ops.attention_chunk(q, cache, 0, return_lse=True)
    _check(c, lc, a.float(), la, f"chunk vs extend G={G} T={T} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_routing_between_the_forms(kind):
    """For G > 1, attention_decode / attention_extend run the MFMA kernel from GQA_MFMA_MIN_ROWS = 8 rows per
    K / V head on (bit for bit attention_chunk) and the VALU form below it; both within the bounds."""
    from kubeflow_rm_amd import ops
    assert ops.decode.GQA_MFMA_MIN_ROWS == 8
    D = 128
    lens = [_S() + 5, 70]
    for G, T, mfma in ((2, 1, False), (4, 1, False), (2, 3, False), (8, 1, True), (16, 1, True), (4, 2, True),
                       (2, 5, True), (4, 4, True)):
        cache, k, v = _cache(D, kind)
        cache.set_lens(lens)
        _poison(cache, lens)
        q = _randn(B, T, G * HKV, D, seed=50 + G + T)
        ref, ref_lse = _ref(q, k, v, lens)
        o, lse = ops.attention_extend(q, cache, 0, return_lse=True)
        _check(o, lse, ref, ref_lse, f"routed extend G={G} T={T} {kind}")
        c, lc = ops.attention_chunk(q, cache, 0, return_lse=True)
        if mfma:
            assert torch.equal(o, c) and torch.equal(lse, lc)
        if T == 1:
            od, lsed = ops.attention_decode(q[:, 0], cache, 0, return_lse=True)
            assert torch.equal(od, o[:, 0]) and torch.equal(lsed, lse[:, 0])


# ---- views, append, refusals --------------------------------------------------------------------
@pytest.mark.parametrize("form", ["extend", "chunk", "decode"])
@pytest.mark.parametrize("kind", KINDS)
def test_strided_q_and_out_no_stray_writes(kind, form, monkeypatch):
    """q read in place from the fused activation [B, T, (Hq + 2 Hkv) D]; o written into a view inside a larger
    sentinel-filled buffer, by the combine launch (several splits) and by the split kernel itself (one)."""
    from kubeflow_rm_amd import ops
    monkeypatch.setattr(ops.decode, "GQA_MFMA_MIN_ROWS", None)  # "extend" and "decode": the VALU form's stores
    D, G, T = 64, 4, 1 if form == "decode" else 3
    Hq, S = G * HKV, _S()
    cache, k, v = _cache(D, kind)
    qkv = _randn(B, T, (Hq + 2 * HKV) * D, seed=61)
    q = qkv[..., :Hq * D].view(B, T, Hq, D)
    assert not q.is_contiguous()
    fn = {"extend": ops.attention_extend, "chunk": ops.attention_chunk, "decode": ops.attention_decode}[form]
    for lens, t_bound in (([S + 9, 40], S + 9), ([40, 17], 40)):
        cache.set_lens(lens)
        buf = torch.full((B + 2, T + 1, Hq * D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
        out = buf[1:B + 1, :T, 8:].view(B, T, Hq, D)
        if form == "decode":
            got = fn(q[:, 0], cache, 0, out=out[:, 0], t_bound=t_bound).unsqueeze(1)
            want = fn(q[:, 0].contiguous(), cache, 0, t_bound=t_bound).unsqueeze(1)
        else:
            got = fn(q, cache, 0, out=out, t_bound=t_bound)
            want = fn(q.contiguous(), cache, 0, t_bound=t_bound)
        assert torch.equal(out, want) and got.data_ptr() == out.data_ptr()
        ref, _ = _ref(q, k, v, lens)
        assert (got.float() - ref).abs().max().item() < ABS and _rel(got, ref) < REL
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:B + 1, :T, 8:] = False
        assert (buf[keep] == 7.0).all()  # every element outside the view is unchanged


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [1, 5])
def test_grouped_append_equals_the_cpu_form(T, kind):
    from kubeflow_rm_amd import ops
    D, G, cap = 64, 4, 40
    Hq = G * HKV
    dt = FP8 if kind == "fp8" else torch.bfloat16
    gpu, cpu = ops.KVCache(1, B, HKV, D, cap, device=DEV, dtype=dt), ops.KVCache(1, B, HKV, D, cap, dtype=dt)
    lens = [7, cap - T + 2] if T > 1 else [7, cap]  # row 1 ends at (T = 1: beyond) the capacity: rows dropped
    qkv = _randn(B, T, (Hq + 2 * HKV) * D, seed=5 + T, dev="cpu")
    for c in (gpu, cpu):
        c.set_lens(lens)
        for t in (c.k[0], c.v[0]):
            t.view(torch.uint8).fill_(0x11)
    ops.kv_append(qkv.to(DEV), gpu, 0, q_heads=Hq)
    ops.kv_append(qkv, cpu, 0, q_heads=Hq)
    assert gpu.k[0].shape == (B, HKV, cap, D)  # heads >= Hkv do not exist
    for a, b_ in ((gpu.k[0], cpu.k[0]), (gpu.v[0], cpu.v[0])):
        assert torch.equal(a.view(torch.uint8).cpu(), b_.view(torch.uint8))  # untouched rows included
    if kind == "fp8":
        kx = qkv[..., Hq * D:].view(B, T, 2, HKV, D)
        for s_, codes_t, scale_t in ((0, gpu.k[0], gpu.k_scale[0]), (1, gpu.v[0], gpu.v_scale[0])):
            for b, n0 in enumerate(lens):  # the ragged row at the capacity included: only the rows that fit
                n = max(min(T, cap - n0), 0)
                codes, scale = ops.decode.quantize_rows(kx[b, :n, s_].transpose(0, 1))
                assert torch.equal(codes_t[b, :, n0:n0 + n].view(torch.uint8).cpu(), codes.view(torch.uint8))
                assert torch.equal(scale_t[b, :, n0:n0 + n].cpu(), scale)
        live = torch.zeros(B, HKV, cap, dtype=torch.bool)
        for b, n0 in enumerate(lens):
            live[b, :, n0:min(n0 + T, cap)] = True
        for a, b_ in ((gpu.k_scale[0], cpu.k_scale[0]), (gpu.v_scale[0], cpu.v_scale[0])):
            assert torch.equal(a.cpu()[live], b_[live]) and (a.cpu()[~live] == 0).all()


def test_contract_violations():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    D, cap = 64, 64
    cache = ops.KVCache(1, B, HKV, D, cap, device=DEV)
    cache.set_lens([20, 20])
    with pytest.raises(ValueError):  # G = 3
        ops.attention_extend(_randn(B, 1, 3 * HKV, D, seed=1), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_decode(_randn(B, 3 * HKV, D, seed=1), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_chunk(_randn(B, 1, 3 * HKV, D, seed=1), cache, 0)
    with pytest.raises(ValueError):
        ops.kv_append(_randn(B, 1, (3 + 2) * HKV * D, seed=1), cache, 0, q_heads=3 * HKV)
    with pytest.raises(ValueError):  # T * G = 17 rows... the next multiple: 9 * 2 = 18 > 16, and 17 * 1 at G = 1
        ops.attention_extend(_randn(B, 9, 2 * HKV, D, seed=1), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_extend(_randn(B, 17, HKV, D, seed=1), cache, 0)
    big = _randn(B, 2, 2 * HKV, D + 4, seed=1)
    with pytest.raises(_lib.NativeLibraryError):  # misaligned q: rows of D + 4 elements begin 8 bytes off
        ops.attention_extend(big[..., 4:], cache, 0)
    # the library itself
    L = _lib.lib()
    G, T = 2, 4
    q = _randn(B, T, G * HKV, D, seed=1)
    o = torch.empty_like(q)
    ws = torch.empty(L.kfamd_attn_extend_gqa_workspace(B, HKV, 16, D, 1, cap), device=DEV, dtype=torch.uint8)

    def st(qt):
        return (ctypes.c_longlong * 12)(*qt.stride()[:3], *cache.k[0].stride()[:3], *cache.v[0].stride()[:3],
                                        *o.stride()[:3])

    def call(name, g, t, t_bound=20, q_off=0, w=ws):
        fn = getattr(L, name)
        return fn(q.data_ptr() + q_off, cache.k[0].data_ptr(), cache.v[0].data_ptr(), cache.lens.data_ptr(),
                  o.data_ptr(), None, w.data_ptr() if w is not None else None, B, HKV, g, D, t, t_bound, 0.125, st(q),
                  None)

    for name in ("kfamd_attn_extend_gqa_bf16", "kfamd_attn_chunk_gqa_bf16"):
        assert call(name, G, T) == 0
        assert call(name, 3, T) == -1 and call(name, 0, T) == -1 and call(name, 32, 1) == -1
        assert call(name, G, 0) == -1 and call(name, G, T, t_bound=0) == -1
        assert call(name, 3, T, q_off=2) == -1  # EINVAL before EALIGN
        assert call(name, G, T, q_off=2) == -2
    assert call("kfamd_attn_extend_gqa_bf16", 2, 9) == -1  # 18 rows
    assert call("kfamd_attn_extend_gqa_bf16", 16, 2) == -1  # 32 rows
    assert call("kfamd_attn_extend_gqa_bf16", G, T, t_bound=_S() + 1, w=None) == -1  # two splits need the workspace
    assert call("kfamd_attn_chunk_gqa_bf16", 16, 4096) == -1  # 65536 rows
    assert L.kfamd_attn_extend_gqa_workspace(B, HKV, 3, D, 1, cap) == 0
    assert L.kfamd_attn_extend_gqa_workspace(B, HKV, 2, D, 9, cap) == 0
    assert (L.kfamd_attn_extend_gqa_workspace(B, HKV, 4, D, 3, 600)
            == 12 * L.kfamd_attn_decode_workspace(B, HKV, D, 600))
    assert L.kfamd_attn_chunk_gqa_workspace(B, HKV, 3, D, 8, cap) == 0
    assert L.kfamd_attn_chunk_gqa_workspace(B, HKV, 16, D, 4096, cap) == 0
    assert L.kfamd_attn_chunk_gqa_nsplit(B, HKV, 5, 8, cap) == 0
    assert (L.kfamd_attn_chunk_gqa_workspace(1, 1, 8, D, 40, 1024)
            == L.kfamd_attn_chunk_workspace(1, 1, D, 320, 1024) == 320 * 4 * (D + 2) * 4)
    qkv = _randn(B, 1, (G + 2) * HKV * D, seed=2)
    cs = (ctypes.c_longlong * 6)(*cache.k[0].stride()[:3], *cache.v[0].stride()[:3])

    def app(hq, hkv, off=0):
        return L.kfamd_kv_append_gqa_bf16(qkv.data_ptr() + off, cache.k[0].data_ptr(), cache.v[0].data_ptr(),
                                          cache.lens.data_ptr(), B, 1, hq, hkv, D, cap, qkv.stride(0), qkv.stride(1), cs,
                                          None)

    assert app(G * HKV, HKV) == 0
    assert app(3 * HKV, HKV) == -1 and app(HKV + 1, HKV) == -1 and app(HKV, 0) == -1 and app(1, HKV) == -1
    assert app(3 * HKV, HKV, off=2) == -1 and app(G * HKV, HKV, off=2) == -2
    torch.cuda.synchronize()


# ---- model --------------------------------------------------------------------------------------
def _cfg(n_heads, n_kv_heads, dtype):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=n_heads, d_ff=1024, max_seq=256, dtype=dtype,
                     n_kv_heads=n_kv_heads)


@pytest.fixture(scope="module", params=[(4, 2), (4, 1), (2, 1)], ids=["D64-G2", "D64-G4", "D128-G2"])
def models(request):
    from kubeflow_rm_amd.models import GPT
    h, hkv = request.param
    return GPT(_cfg(h, hkv, torch.bfloat16), device=DEV).eval(), GPT(_cfg(h, hkv, torch.float32)).eval()


def _teacher_forced(gpu, seq, T0, steps, chunk_tail, kv_dtype=None):
    Bm = seq.shape[0]
    cache = gpu.new_cache(Bm, seq.shape[1], kv_dtype=kv_dtype)
    assert cache.H == gpu.cfg.kv_heads and cache.k[0].shape[1] == gpu.cfg.kv_heads
    got, at = [gpu.prefill(seq[:, :T0].to(DEV), cache).view(Bm, 1, -1)], T0
    for T in steps:
        got.append(gpu.extend(seq[:, at:at + T].to(DEV), cache))
        at += T
    got.append(gpu.extend(seq[:, at:at + chunk_tail].to(DEV), cache, chunk=24))
    assert cache.lens.tolist() == [seq.shape[1]] * Bm
    return torch.cat(got, 1).float().cpu()


def test_gqa_model_cache_paths_match_the_fp32_full_forward(models):
    gpu, ref = models
    Bm, T0, steps, tail = 2, 40, (1, 3, 16, 20), 30
    seq = torch.randint(0, 512, (Bm, T0 + sum(steps) + tail), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)[:, T0 - 1:]
    errs = (_teacher_forced(gpu, seq, T0, steps, tail) - want).abs().amax(dim=(0, 2))
    print(f"gqa extend per-position max-abs: max {errs.max().item():.4f}")
    assert errs.max().item() < 0.1, errs.tolist()
    # the FP8 cache: tests/test_gpu_kv_fp8.py's bound, 0.1 + 2 E_q with E_q the fp32 model's own fp8-cache error
    c8, c32 = ref.new_cache(Bm, seq.shape[1], kv_dtype=FP8), ref.new_cache(Bm, seq.shape[1])
    with torch.no_grad():
        e_q = (ref.extend(seq, c8) - ref.extend(seq, c32)).abs().max().item()
    errs8 = (_teacher_forced(gpu, seq, T0, steps, tail, kv_dtype=FP8) - want).abs().amax(dim=(0, 2))
    print(f"gqa fp8-cache per-position max-abs: max {errs8.max().item():.4f}, E_q {e_q:.4f}")
    assert e_q > 0 and errs8.max().item() < 0.1 + 2 * e_q, (errs8.tolist(), e_q)


def test_gqa_generate_graph_and_fused_sampler(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    eager = gpu.generate(idx, 8)
    assert torch.equal(gpu.generate(idx, 8, graph=True), eager)
    kw = dict(sampler="fused", temperature=0.8, top_k=20, top_p=0.9, weight_dtype=FP8)
    a = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), graph=True, **kw)
    b_ = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), **kw)
    assert a.shape == (2, 20) and torch.equal(a, b_)


def test_gqa_training_step_sums_kv_gradients_over_the_group(models):
    """loss.backward() through ops.flash_attention on the expanded K / V against the torch-reference mode on the
    same weights: tests/test_gpu_attention.py's bounds (loss within 2e-2, QKV weight gradient rel-l2 < 5e-2)."""
    from unittest import mock
    from kubeflow_rm_amd import ops
    gpu, _ = models
    gpu.train()
    try:
        idx = torch.randint(0, 512, (2, 128), generator=torch.Generator().manual_seed(2)).to(DEV)
        tgt = torch.randint(0, 512, (2, 128), generator=torch.Generator().manual_seed(3)).to(DEV)
        gpu.zero_grad(set_to_none=True)
        with mock.patch.object(F, "scaled_dot_product_attention", side_effect=AssertionError("SDPA called")):
            _, loss = gpu(idx, tgt)
            loss.backward()
        g_native = gpu.blocks[0].qkv.weight.grad.clone()
        gpu.zero_grad(set_to_none=True)
        with ops.torch_reference():
            _, loss_ref = gpu(idx, tgt)
            loss_ref.backward()
        g_ref = gpu.blocks[0].qkv.weight.grad
        hq = gpu.cfg.n_heads * gpu.cfg.head_dim
        print(f"gqa train: loss {loss.item():.4f} / {loss_ref.item():.4f}, qkv grad rel {_rel(g_native, g_ref):.3e}, "
              f"kv rows rel {_rel(g_native[hq:], g_ref[hq:]):.3e}")
        assert abs(loss.item() - loss_ref.item()) < 2e-2
        assert _rel(g_native, g_ref) < 5e-2 and _rel(g_native[hq:], g_ref[hq:]) < 5e-2
    finally:
        gpu.zero_grad(set_to_none=True)
        gpu.eval()
