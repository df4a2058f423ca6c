"""The FP8 KV cache on the gfx950 kernels (kernels/attn_kv.hip): the quantising append against the
torch reference of the format, decode and extend attention against fp32 SDPA over the DEQUANTISED cache
(which isolates the kernels from the quantisation error: the project's bf16 bounds apply unchanged), and
GPT.prefill / decode_step / extend / generate with kv_dtype=torch.float8_e4m3fn."""
from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_kv_fp8_cpu import check_format, format_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _S():
    from kubeflow_rm_amd.ops import decode
    return decode.SPLIT_KEYS


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _raw(t):
    return t.view(torch.uint8)


def _compare_codes(got, got_scale, x):
    """GPU codes / scales of rows x [..., D] (bf16, CPU) against quantize_rows of the same rows: scales
    within 1e-6 relative; codes equal on >= 99 % of the elements, the rest exactly one code step away (a
    1-ulp difference in the scale can flip a tie). Returns the fraction of equal codes."""
    from kubeflow_rm_amd.ops import decode
    ref, ref_scale = decode.quantize_rows(x)
    got, got_scale = _raw(got).cpu(), got_scale.cpu()
    rel = ((got_scale - ref_scale).abs() / ref_scale).max().item()
    assert rel <= 1e-6, rel
    diff = (got.int() - _raw(ref).int()).abs()
    same = (diff == 0).float().mean().item()
    assert same >= 0.99, same
    assert (diff <= 1).all(), diff.max().item()
    return same


# ---- format and append -------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
def test_gpu_append_stores_the_format(D):
    """The CPU format test's inputs as K and V rows of two heads: the stored rows meet every property of
    the format, and agree with quantize_rows."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    H = 2
    sets = [format_rows(D, seed=10 * D + i) for i in range(2 * H)]  # k h0, k h1, v h0, v h1
    N = sets[0].shape[0]
    qkv = torch.randn(1, N, 3, H, D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    for i, rows in enumerate(sets):
        qkv[0, :, 1 + i // H, i % H] = rows
    cache = ops.KVCache(1, 1, H, D, N + 3, device=DEV, dtype=FP8)
    ops.kv_append(qkv.view(1, N, 3 * H * D).to(DEV), cache, 0)
    torch.cuda.synchronize()
    assert cache.lens.tolist() == [0]
    for i, rows in enumerate(sets):
        codes = (cache.k if i < H else cache.v)[0][0, i % H, :N].cpu()
        scale = (cache.k_scale if i < H else cache.v_scale)[0][0, i % H, :N].cpu()
        check_format(rows, codes, scale)
        same = _compare_codes(codes, scale, rows)
        print(f"D={D} set {i}: codes equal to the reference on {100 * same:.3f} %")
    ref, ref_scale = decode.quantize_rows(sets[0])
    assert _compare_codes(ref, ref_scale, sets[0]) == 1.0  # the reference against itself: the cap hides nothing


def _append_case(D, B, H, cap, lens, T, strided=False):
    """Append T rows at `lens` into a sentinel-filled cache; every written row agrees with quantize_rows,
    every other byte and scale is untouched (rows before lens, rows past the block, rows past the capacity)."""
    from kubeflow_rm_amd import ops
    cache = ops.KVCache(1, B, H, D, cap, device=DEV, dtype=FP8)
    for t in (cache.k[0], cache.v[0]):
        _raw(t).fill_(0x55)
    for t in (cache.k_scale[0], cache.v_scale[0]):
        t.fill_(-7.0)
    cache.set_lens(lens)
    if strided:  # a slice of a wider activation buffer: row stride 3 * H * D + 64, 16-B aligned start
        wide = _randn(B, T, 3 * H * D + 64, seed=T + D)
        qkv = wide[:, :, 8:8 + 3 * H * D]
        assert not qkv.is_contiguous()
    else:
        qkv = _randn(B, T, 3 * H * D, seed=T + D)
    ops.kv_append(qkv, cache, 0)
    torch.cuda.synchronize()
    assert cache.lens.tolist() == list(lens)
    x = qkv.cpu().view(B, T, 3, H, D)
    for s, codes, scales in ((1, cache.k[0], cache.k_scale[0]), (2, cache.v[0], cache.v_scale[0])):
        raw, scales = _raw(codes).cpu(), scales.cpu()
        for b, n in enumerate(lens):
            kept = max(min(T, cap - n), 0)
            if kept:
                _compare_codes(codes[b, :, n:n + kept], scales[b, :, n:n + kept], x[b, :kept, s].transpose(0, 1))
            assert (raw[b, :, :n] == 0x55).all() and (scales[b, :, :n] == -7.0).all()
            assert (raw[b, :, n + kept:] == 0x55).all() and (scales[b, :, n + kept:] == -7.0).all()


@pytest.mark.parametrize("D", [64, 128])
def test_gpu_append_edges(D):
    _append_case(D, 3, 3, 40, [0, 7, 33], 1)                  # T = 1 at ragged lens
    _append_case(D, 3, 3, 40, [0, 7, 33], 5)                  # T = 5 at ragged lens
    _append_case(D, 2, 2, 320, [0, 0], 300)                   # a prefill-sized call from empty
    _append_case(D, 2, 3, 40, [3, 20], 5, strided=True)       # a slice of a wider buffer
    _append_case(D, 3, 2, 24, [22, 24, 10], 5)                # crosses the capacity; starts at it; fits


# ---- attention -----------------------------------------------------------------------------------

def _filled(B, H, D, cap, seed, edit=None):
    """An fp8 cache of `cap` rows appended from random bf16 QKV (`edit(x [B, cap, 3, H, D])` first), and
    its dequantised K, V (fp32, on the GPU) read back from the cache."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    qkv = torch.randn(B, cap, 3, H, D, generator=torch.Generator().manual_seed(seed))
    if edit is not None:
        edit(qkv)
    cache = ops.KVCache(1, B, H, D, cap, device=DEV, dtype=FP8)
    ops.kv_append(qkv.view(B, cap, 3 * H * D).to(DEV, torch.bfloat16), cache, 0)
    torch.cuda.synchronize()
    kd = decode.dequantize_rows(cache.k[0].cpu(), cache.k_scale[0].cpu()).to(DEV)
    vd = decode.dequantize_rows(cache.v[0].cpu(), cache.v_scale[0].cpu()).to(DEV)
    return cache, kd, vd


def _ref_decode(q, k, v, lens):
    outs, lses = [], []
    for b, n in enumerate(lens):
        kk, vv = k[b:b + 1, :, :n], v[b:b + 1, :, :n]
        outs.append(F.scaled_dot_product_attention(q[b:b + 1].float().unsqueeze(2), kk, vv).squeeze(2))
        s = (q[b].float().unsqueeze(1) @ kk[0].transpose(-1, -2)).squeeze(1) / math.sqrt(q.shape[-1])
        lses.append(torch.logsumexp(s, -1))
    return torch.cat(outs, 0), torch.stack(lses, 0)


def _ref_extend(q, k, v, lens):
    Bq, Tq, Hq, D = q.shape
    o = torch.zeros(Bq, Tq, Hq, D, device=q.device)
    lse = torch.full((Bq, Tq, Hq), float("-inf"), device=q.device)
    for b, n in enumerate(lens):
        for i in range(Tq):
            nk = n - Tq + i + 1
            if nk <= 0:
                continue
            kk, vv = k[b:b + 1, :, :nk], v[b:b + 1, :, :nk]
            o[b, i] = F.scaled_dot_product_attention(q[b:b + 1, i].float().unsqueeze(2), kk, vv)[0, :, 0]
            s = (q[b, i].float().unsqueeze(1) @ kk[0].transpose(-1, -2)).squeeze(1) / math.sqrt(D)
            lse[b, i] = torch.logsumexp(s, -1)
    return o, lse


def _check(o, ref, what=""):
    """The project's bf16 bounds (tests/test_gpu_decode.py _check_decode), unchanged."""
    err = (o.float() - ref).abs().max().item()
    rel = _rel(o, ref)
    print(f"fp8 attention {what}: max-abs {err:.3e} rel-l2 {rel:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < 2e-2, err
    assert rel < 8e-3, rel


@pytest.fixture(scope="module", params=[64, 128], ids=["D64", "D128"])
def boundary(request):
    D = request.param
    return (D, *_filled(2, 3, D, 2 * _S(), seed=10 + D))


@pytest.mark.parametrize("which", ["one", "S-1", "S", "S+1"])
def test_decode_split_boundary(boundary, which):
    from kubeflow_rm_amd import ops
    D, cache, kd, vd = boundary
    S = _S()
    n = {"one": 1, "S-1": S - 1, "S": S, "S+1": S + 1}[which]
    q = _randn(2, 3, D, seed=n)
    cache.set_lens([n] * 2)
    ref, _ = _ref_decode(q, kd, vd, [n] * 2)
    for t_bound in (n, cache.capacity):
        o = ops.attention_decode(q, cache, 0, t_bound=t_bound)
        _check(o, ref, f"decode n={n} t_bound={t_bound}")
        assert torch.equal(ops.attention_decode(q, cache, 0, t_bound=t_bound), o)  # repeatable


@pytest.mark.parametrize("D", [64, 128])
def test_decode_ragged_rows_lse_and_dead_rows(D):
    """Ragged rows with empty later splits and the LSE; then codes beyond lens set to 0x7F (NaN) and scales
    to NaN: finite, and bit-identical to the clean cache's result."""
    from kubeflow_rm_amd import ops
    S = _S()
    B, H, lens = 3, 5, [1, S + 1, 3 * S - 1]
    cache, kd, vd = _filled(B, H, D, 3 * S, seed=20 + D)
    q = _randn(B, H, D, seed=21)
    cache.set_lens(lens)
    o, lse = ops.attention_decode(q, cache, 0, t_bound=3 * S, return_lse=True)
    ref, ref_lse = _ref_decode(q, kd, vd, lens)
    _check(o, ref, "decode ragged")
    assert (lse - ref_lse).abs().max().item() < 1e-3
    clean, clean_lse = o.clone(), lse.clone()
    for b, n in enumerate(lens):
        _raw(cache.k[0])[b, :, n:] = 0x7F
        _raw(cache.v[0])[b, :, n:] = 0x7F
        cache.k_scale[0][b, :, n:] = float("nan")
        cache.v_scale[0][b, :, n:] = float("nan")
    o, lse = ops.attention_decode(q, cache, 0, t_bound=3 * S, return_lse=True)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(o, clean) and torch.equal(lse, clean_lse)


@pytest.mark.parametrize("D", [64, 128])
def test_decode_many_splits(D):
    from kubeflow_rm_amd import ops
    cache, kd, vd = _filled(1, 2, D, 4096, seed=30 + D)
    q = _randn(1, 2, D, seed=31)
    cache.set_lens([4095])
    o = ops.attention_decode(q, cache, 0, t_bound=4096)
    _check(o, _ref_decode(q, kd, vd, [4095])[0], "decode 4095 of 4096")


@pytest.mark.parametrize("D", [64, 128])
def test_scale_wiring_and_cross_split_rescale(D):
    """Head 0's K rows x 64 and head 1's V rows / 64 before the append: a kernel that ignores or swaps the
    two scale tensors misses the bounds. Head 2 carries a key spiked x 30 in a later split (the rescale
    inside a split and the max hand-over in the combine)."""
    from kubeflow_rm_amd import ops
    S = _S()
    B, H, n, Tq = 1, 3, 3 * S, 4
    q = _randn(B, Tq, H, D, seed=51)

    def edit(x):  # x [B, n, 3, H, D] fp32
        x[:, :, 1, 0] *= 64
        x[:, :, 2, 1] /= 64
        x[0, 2 * S + 17, 1, 2] = x[0, 2 * S + 17, 1, 2].abs() * torch.sign(q[0, -1, 2].float().cpu()) * 30

    cache, kd, vd = _filled(B, H, D, n, seed=50 + D, edit=edit)
    ks, vs = cache.k_scale[0], cache.v_scale[0]
    assert ks[0, 0].mean() > 16 * ks[0, 1].mean() and vs[0, 1].mean() * 16 < vs[0, 0].mean()  # the scales differ
    cache.set_lens([n])
    o, lse = ops.attention_decode(q[:, -1], cache, 0, return_lse=True)
    ref, ref_lse = _ref_decode(q[:, -1], kd, vd, [n])
    _check(o, ref, "decode scale wiring")
    assert (lse - ref_lse).abs().max().item() < 1e-3
    oe, lse_e = ops.attention_extend(q, cache, 0, return_lse=True)
    ref, ref_lse = _ref_extend(q, kd, vd, [n])
    _check(oe, ref, "extend scale wiring")
    assert (lse_e - ref_lse).abs().max().item() < 1e-3


@pytest.fixture(scope="module", params=[64, 128], ids=["D64", "D128"])
def extend_cache(request):
    D = request.param
    return (D, *_filled(2, 3, D, 2 * _S() + 8, seed=100 + D))


@pytest.mark.parametrize("Tq", [1, 3, 8, 9, 16])
def test_extend_split_straddle_and_rows_before_the_start(extend_cache, Tq):
    """Row 0: the new block straddles a split boundary (lens = S + 2). Row 1: lens < Tq, so its early rows
    see no key: zeros and lse = -inf. Then dead codes / scales set to NaN: bit-identical."""
    from kubeflow_rm_amd import ops
    D, cache, kd, vd = extend_cache
    S = _S()
    lens = [S + 2, max(Tq - 2, 0)]
    q = _randn(2, Tq, 3, D, seed=Tq)
    cache.set_lens(lens)
    ref, ref_lse = _ref_extend(q, kd, vd, lens)
    dead = Tq - lens[1]
    for t_bound in (S + 2, cache.capacity):
        o, lse = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
        _check(o, ref, f"extend Tq={Tq} t_bound={t_bound}")
        assert (o[1, :dead] == 0).all() and (lse[1, :dead] == float("-inf")).all()
        live = torch.isfinite(ref_lse)
        assert torch.equal(torch.isfinite(lse), live)
        assert (lse[live] - ref_lse[live]).abs().max().item() < 1e-3
        again, lse2 = ops.attention_extend(q, cache, 0, t_bound=t_bound, return_lse=True)
        assert torch.equal(again, o) and torch.equal(lse2, lse)  # repeatable
    saved = [(_raw(t) if t.dtype == FP8 else t).clone() for t in (cache.k[0], cache.v[0], cache.k_scale[0],
                                                                  cache.v_scale[0])]
    for b, n in enumerate(lens):
        _raw(cache.k[0])[b, :, n:] = 0x7F
        _raw(cache.v[0])[b, :, n:] = 0x7F
        cache.k_scale[0][b, :, n:] = float("nan")
        cache.v_scale[0][b, :, n:] = float("nan")
    o2, lse2 = ops.attention_extend(q, cache, 0, t_bound=cache.capacity, return_lse=True)
    for t, s in zip((cache.k[0], cache.v[0], cache.k_scale[0], cache.v_scale[0]), saved):  # a shared fixture
        (_raw(t) if t.dtype == FP8 else t).copy_(s)
    assert torch.isfinite(o2.float()).all()
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


def test_launcher_contract():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    from kubeflow_rm_amd.ops.decode import _ll
    L = _lib.lib()
    B, H, D, cap = 1, 2, 64, 32
    c = ops.KVCache(1, B, H, D, cap, device=DEV, dtype=FP8)
    k, v, ks, vs = c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]
    q = _randn(B, 1, H, D, seed=1)
    o = torch.empty_like(q)
    c.set_lens([4])
    qkv = _randn(B, 1, 3 * H * D, seed=2)

    def decode(k_off=0, D_=D):
        return L.kfamd_attn_decode_fp8(
            q.data_ptr(), k.data_ptr() + k_off, v.data_ptr(), ks.data_ptr(), vs.data_ptr(), c.lens.data_ptr(),
            o.data_ptr(), None, c.workspace.data_ptr(), B, H, D_, cap, 0.125,
            _ll(H * D_, D_, *k.stride()[:3], *v.stride()[:3], H * D_, D_, *ks.stride()[:2], *vs.stride()[:2]), None)

    def extend(k_off=0, D_=D, Tq=1):
        return L.kfamd_attn_extend_fp8(
            q.data_ptr(), k.data_ptr() + k_off, v.data_ptr(), ks.data_ptr(), vs.data_ptr(), c.lens.data_ptr(),
            o.data_ptr(), None, c._extend_ws().data_ptr(), B, H, D_, Tq, cap, 0.125,
            _ll(H * D_, H * D_, D_, *k.stride()[:3], *v.stride()[:3], H * D_, H * D_, D_, *ks.stride()[:2],
                *vs.stride()[:2]), None)

    def append(k_off=0, D_=D):
        return L.kfamd_kv_append_fp8(
            qkv.data_ptr(), k.data_ptr() + k_off, v.data_ptr(), ks.data_ptr(), vs.data_ptr(), c.lens.data_ptr(), B, 1,
            H, D_, cap, 3 * H * D_, 3 * H * D_, _ll(*k.stride()[:3], *v.stride()[:3], *ks.stride()[:2], *vs.stride()[:2]),
            None)

    for fn in (decode, extend, append):
        assert fn() == 0
        assert fn(k_off=8) == -2   # KFAMD_EALIGN: a misaligned code pointer
        assert fn(D_=96) == -1     # KFAMD_EINVAL
    assert extend(Tq=17) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.attention_decode(q[:, 0].float(), c, 0)
    with pytest.raises(ValueError):
        ops.attention_decode(q[:, 0], c, 0, t_bound=cap + 1)


def test_cache_nbytes_and_workspaces_on_the_gpu():
    from kubeflow_rm_amd import ops
    for D in (64, 128):
        bf = ops.KVCache(2, 2, 4, D, 512, device=DEV)
        f8 = ops.KVCache(2, 2, 4, D, 512, device=DEV, dtype=FP8)
        assert f8.workspace is not None and f8.workspace.numel() == bf.workspace.numel()
        kv_bf, kv_f8 = bf.nbytes - bf.workspace.numel(), f8.nbytes - f8.workspace.numel()
        assert kv_f8 / kv_bf == (D + 4) / (2 * D)
        before = f8.nbytes
        f8._extend_ws()
        assert f8.nbytes == before + f8.extend_workspace.numel()


# ---- model -------------------------------------------------------------------------------------

def _cfg(n_heads, dtype):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=n_heads, d_ff=1024, max_seq=256, dtype=dtype)


@pytest.fixture(scope="module", params=[4, 2], ids=["D64", "D128"])
def models(request):
    from kubeflow_rm_amd.models import GPT
    return GPT(_cfg(request.param, torch.bfloat16), device=DEV).eval(), GPT(_cfg(request.param, torch.float32)).eval()


def test_prefill_logits_do_not_depend_on_the_cache_dtype(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 40), generator=torch.Generator().manual_seed(0)).to(DEV)
    a = gpu.prefill(idx, gpu.new_cache(2, 48))
    c8 = gpu.new_cache(2, 48, kv_dtype=FP8)
    assert c8.dtype == FP8 and c8.k_scale[0].is_cuda
    assert torch.equal(gpu.prefill(idx, c8), a)
    assert c8.lens.tolist() == [40, 40]


def test_teacher_forced_decode_on_an_fp8_cache(models):
    """E_q: the max-abs logit difference, on the CPU, between the fp32 model on an fp8 cache and on an fp32
    cache: a quantity of the torch reference alone. The GPU's fp8-cache logits stay within 0.1 + 2 * E_q
    of the fp32 full forward: 0.1 is the bf16 bound, and the GPU quantises bf16-computed K / V where the
    CPU quantises fp32-computed ones (two independent rounding patterns)."""
    gpu, ref = models
    B, T0, steps = 2, 40, 24
    seq = torch.randint(0, 512, (B, T0 + steps), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)
    rows = slice(T0 - 1, T0 + steps)
    c8, c32 = ref.new_cache(B, T0 + steps, kv_dtype=FP8), ref.new_cache(B, T0 + steps)
    ref.prefill(seq[:, :T0], c8)
    ref.prefill(seq[:, :T0], c32)
    e_q = max((ref.decode_step(seq[:, T0 + i], c8) - ref.decode_step(seq[:, T0 + i], c32)).abs().max().item()
              for i in range(steps))
    cache = gpu.new_cache(B, T0 + steps, kv_dtype=FP8)
    logits = [gpu.prefill(seq[:, :T0].to(DEV), cache)]
    for i in range(steps):
        logits.append(gpu.decode_step(seq[:, T0 + i].to(DEV), cache))
    got = torch.stack([x.float().cpu() for x in logits], 1)
    errs = (got - want[:, rows]).abs().amax(dim=(0, 2))
    print(f"E_q {e_q:.4f}; fp8-cache per-step max-abs {[round(e, 4) for e in errs.tolist()]}")
    assert e_q > 0
    assert errs.max().item() < 0.1 + 2 * e_q, (errs.tolist(), e_q)
    assert cache.lens.tolist() == [T0 + steps] * B


@pytest.mark.parametrize("T", [1, 5, 16, 20])
def test_extend_on_an_fp8_cache_equals_decode_steps(models, T):
    """extend(T) against T decode_steps, both on fp8 caches: within the 0.1 logit bound that
    tests/test_gpu_extend.py holds bf16 extend to."""
    gpu, _ = models
    seq = torch.randint(0, 512, (2, 30 + T), generator=torch.Generator().manual_seed(3)).to(DEV)
    a, b = gpu.new_cache(2, 30 + T, kv_dtype=FP8), gpu.new_cache(2, 30 + T, kv_dtype=FP8)
    gpu.prefill(seq[:, :30], a)
    gpu.prefill(seq[:, :30], b)
    lg = gpu.extend(seq[:, 30:], a).float()
    steps = torch.stack([gpu.decode_step(seq[:, 30 + i], b).float() for i in range(T)], 1)
    err = (lg - steps).abs().max().item()
    print(f"extend({T}) against decode steps on fp8: max-abs {err:.4f}")
    assert lg.shape == steps.shape and err < 0.1, err
    assert a.lens.tolist() == b.lens.tolist() == [30 + T] * 2


def _hand_loop(model, idx, new, cache=None):
    cache = cache if cache is not None else model.new_cache(idx.shape[0], idx.shape[1] + new, kv_dtype=FP8)
    logits = [model.prefill(idx, cache).clone()]
    toks = [idx, logits[0].argmax(-1).view(-1, 1)]
    for _ in range(new - 1):
        logits.append(model.decode_step(toks[-1].view(-1), cache).clone())
        toks.append(logits[-1].argmax(-1).view(-1, 1))
    return torch.cat(toks, 1), logits


def test_generate_on_fp8_equals_hand_loop_and_graph(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(1)).to(DEV)
    out = gpu.generate(idx, 16, kv_dtype=FP8)
    assert out.shape == (2, 40) and torch.equal(out[:, :24], idx)
    assert torch.equal(out, _hand_loop(gpu, idx, 16)[0])
    assert torch.equal(gpu.generate(idx, 16, graph=True, kv_dtype=FP8), out)


def test_graphed_fp8_step_equals_eager(models):
    """One captured decode step on an fp8 cache replayed over two prompts of different lengths: logits
    bit-identical to the eager steps at every position."""
    gpu, _ = models
    B, new, cap = 2, 10, 64
    cache = gpu.new_cache(B, cap, kv_dtype=FP8)
    step = None
    for seed, T0 in ((1, 40), (2, 17)):
        idx = torch.randint(0, 512, (B, T0), generator=torch.Generator().manual_seed(seed)).to(DEV)
        want_toks, want_logits = _hand_loop(gpu, idx, new)
        cache.reset()
        logits = gpu.prefill(idx, cache)
        if step is None:
            step = gpu.graphed_decode_step(cache)
        toks = [idx]
        for i in range(new):
            torch.testing.assert_close(logits, want_logits[i], rtol=0, atol=0)
            toks.append(logits.argmax(-1).view(-1, 1))
            if i + 1 < new:
                logits = step(toks[-1].view(-1))
        assert torch.equal(torch.cat(toks, 1), want_toks)


def test_self_draft_on_fp8_accepts_every_proposal(models):
    gpu, _ = models
    T0, new, lookahead = 24, 24, 4
    idx = torch.randint(0, 512, (1, T0), generator=torch.Generator().manual_seed(1)).to(DEV)
    plain = gpu.generate(idx, new, kv_dtype=FP8)
    out, stats = gpu.generate(idx, new, draft=gpu, lookahead=lookahead, return_stats=True, kv_dtype=FP8)
    print(f"self-draft on fp8 caches: {stats}")
    assert stats["accepted"] == stats["proposed"], stats
    assert stats["target_steps"] == math.ceil(new / (lookahead + 1)), stats
    assert torch.equal(out, plain)
