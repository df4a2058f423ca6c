"""KV-cache decode on the gfx950 kernels: single-query split-KV attention and the KV append
(kernels/attn_kv.hip), the M <= 16 weight-streaming GEMM (kernels/gemm_skinny_bf16.hip),
and GPT.prefill / decode_step / generate built on them, against fp32 references."""
from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _cache(B, H, D, Tcap, seed):
    from kubeflow_rm_amd import ops
    c = ops.KVCache(1, B, H, D, Tcap, device=DEV)
    c.k[0].copy_(_randn(B, H, Tcap, D, seed=seed))
    c.v[0].copy_(_randn(B, H, Tcap, D, seed=seed + 1))
    return c


def _ref_decode(q, k, v, lens):
    """fp32 SDPA of the 1-row query over k[:, :, :len], per batch row (same bf16 inputs)."""
    outs = []
    for b, n in enumerate(lens):
        outs.append(F.scaled_dot_product_attention(q[b:b + 1].float().unsqueeze(2), k[b:b + 1, :, :n].float(),
                                                   v[b:b + 1, :, :n].float()).squeeze(2))
    return torch.cat(outs, 0)


def _check_decode(o, ref):
    err = (o.float() - ref).abs().max().item()
    rel = _rel(o, ref)
    print(f"decode attention: max-abs {err:.3e} rel-l2 {rel:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err < 2e-2, err
    assert rel < 8e-3, rel


def _S():
    from kubeflow_rm_amd.ops import decode
    return decode.SPLIT_KEYS


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("which", ["one", "S-1", "S", "S+1"])
def test_decode_attention_split_boundary(D, which):
    from kubeflow_rm_amd import ops
    S = _S()
    n = {"one": 1, "S-1": S - 1, "S": S, "S+1": S + 1}[which]
    B, H, Tcap = 2, 3, 2 * S
    cache = _cache(B, H, D, Tcap, seed=10 + D)
    q = _randn(B, H, D, seed=n)
    cache.set_lens([n] * B)
    ref = _ref_decode(q, cache.k[0], cache.v[0], [n] * B)
    for t_bound in (n, Tcap):  # the tight grid, and a grid with an empty / 1-key trailing split
        o = ops.attention_decode(q, cache, 0, t_bound=t_bound)
        _check_decode(o, ref)


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_ragged_rows_and_lse(D):
    """Rows whose later splits are entirely empty; the log-sum-exp output."""
    from kubeflow_rm_amd import ops
    S = _S()
    B, H = 3, 5
    lens = [1, S + 1, 3 * S - 1]
    cache = _cache(B, H, D, 3 * S, seed=20 + D)
    q = _randn(B, H, D, seed=21)
    cache.set_lens(lens)
    o, lse = ops.attention_decode(q, cache, 0, t_bound=3 * S, return_lse=True)
    _check_decode(o, _ref_decode(q, cache.k[0], cache.v[0], lens))
    for b, n in enumerate(lens):
        s = (q[b].float().unsqueeze(1) @ cache.k[0][b, :, :n].float().transpose(-1, -2)).squeeze(1) / math.sqrt(D)
        assert (lse[b] - torch.logsumexp(s, -1)).abs().max().item() < 1e-3


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_many_splits(D):
    from kubeflow_rm_amd import ops
    cache = _cache(1, 2, D, 4096, seed=30 + D)
    q = _randn(1, 2, D, seed=31)
    cache.set_lens([4095])
    o = ops.attention_decode(q, cache, 0, t_bound=4096)
    _check_decode(o, _ref_decode(q, cache.k[0], cache.v[0], [4095]))


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_masks_by_select(D):
    """Cache rows at or beyond len hold NaN: the result is bit-identical to the clean cache's, and finite."""
    from kubeflow_rm_amd import ops
    S = _S()
    B, H = 2, 2
    lens = [S // 2 + 3, S + 5]
    cache = _cache(B, H, D, 3 * S, seed=40 + D)
    q = _randn(B, H, D, seed=41)
    cache.set_lens(lens)
    clean = ops.attention_decode(q, cache, 0, t_bound=3 * S).clone()
    for b, n in enumerate(lens):
        cache.k[0][b, :, n:] = float("nan")
        cache.v[0][b, :, n:] = float("nan")
    o = ops.attention_decode(q, cache, 0, t_bound=3 * S)
    assert torch.isfinite(o.float()).all()
    assert torch.equal(o, clean)
    _check_decode(o, _ref_decode(q, cache.k[0], cache.v[0], lens))


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_rescale_and_cross_split_combine(D):
    """A key spiked x30 in a later split than the running max forces the online-softmax rescale inside a
    split's lane groups and the max hand-over in the combine (cdna_hip_programming.md §5.4 rule 26);
    another head's max grows at every key."""
    from kubeflow_rm_amd import ops
    S = _S()
    B, H, n = 1, 3, 3 * S
    cache = _cache(B, H, D, n, seed=50 + D)
    q = _randn(B, H, D, seed=51)
    k = cache.k[0]
    for idx, h in ((2 * S + 17, 0), (S // 2 + 1, 2)):  # later split; later key of the first split
        k[0, h, idx] = (k[0, h, idx].float().abs() * torch.sign(q[0, h].float()) * 30).to(torch.bfloat16)
    q[0, 1] = 0.5
    ramp = torch.linspace(0.0, 3.0 / math.sqrt(D / 64), n, device=DEV).view(n, 1)
    k[0, 1] = (k[0, 1].float() * 0.1 + ramp / 8).to(torch.bfloat16)
    cache.set_lens([n])
    o = ops.attention_decode(q, cache, 0)
    ref = _ref_decode(q, k, cache.v[0], [n])
    _check_decode(o, ref)
    # the spiked key owns its head's softmax
    assert (o[0, 0].float() - cache.v[0][0, 0, 2 * S + 17].float()).abs().max().item() < 2e-2


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_strided_q_and_out(D):
    """q read in place from the fused QKV output [B, 1, 3, H, D]; o written into [B, 1, H * D]."""
    from kubeflow_rm_amd import ops
    S = _S()
    B, H = 2, 3
    cache = _cache(B, H, D, 2 * S, seed=60 + D)
    cache.set_lens([S + 9, 40])
    qkv = _randn(B, 1, 3, H, D, seed=61)
    q = qkv[:, 0, 0]
    assert not q.is_contiguous()
    want = ops.attention_decode(q.contiguous(), cache, 0)
    buf = torch.full((B, 1, H * D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
    out = buf[:, 0, :H * D].view(B, H, D)
    got = ops.attention_decode(q, cache, 0, out=out)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, 0, :H * D].reshape(B, H, D), want)
    assert (buf[:, 0, H * D:] == 7.0).all()
    _check_decode(got, _ref_decode(q, cache.k[0], cache.v[0], [S + 9, 40]))


def test_decode_attention_rejects_head_dim_96():
    from kubeflow_rm_amd import ops
    cache = ops.KVCache(1, 1, 2, 96, 64, device=DEV)
    cache.set_lens([8])
    with pytest.raises(ValueError):
        ops.attention_decode(_randn(1, 2, 96, seed=1), cache, 0)
    import ctypes
    from kubeflow_rm_amd.ops import _lib
    q = _randn(1, 2, 96, seed=1)
    st = (ctypes.c_longlong * 10)(192, 96, 2 * 64 * 96, 64 * 96, 96, 2 * 64 * 96, 64 * 96, 96, 192, 96)
    assert _lib.lib().kfamd_attn_decode_workspace(1, 2, 96, 64) == 0
    rc = _lib.lib().kfamd_attn_decode_bf16(q.data_ptr(), cache.k[0].data_ptr(), cache.v[0].data_ptr(),
                                           cache.lens.data_ptr(), q.data_ptr(), None, None, 1, 2, 96, 8, 1.0, st, None)
    assert rc == -1


@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_bit_exact(D):
    from kubeflow_rm_amd import ops
    B, H, Tcap = 3, 2, 48
    cache = ops.KVCache(2, B, H, D, Tcap, device=DEV)
    sent = torch.tensor(-3.5, dtype=torch.bfloat16)
    for t in (*cache.k, *cache.v):
        t.fill_(sent)
    want_k = torch.full((B, H, Tcap, D), -3.5, device=DEV, dtype=torch.bfloat16)
    want_v = want_k.clone()

    def put(qkv, pos):
        x = qkv.view(B, qkv.shape[1], 3, H, D)
        for b in range(B):
            for t in range(qkv.shape[1]):
                if pos[b] + t < Tcap:
                    want_k[b, :, pos[b] + t] = x[b, t, 1]
                    want_v[b, :, pos[b] + t] = x[b, t, 2]

    steps = [(40, [0, 0, 0]),       # a prefill-sized append
             (1, [40, 7, 0]),       # one decode row at per-row positions
             (2, [47, 48, 46])]     # rows that would land at or beyond Tcap are dropped
    for i, (T, pos) in enumerate(steps):
        qkv = _randn(B, T, 3 * H * D, seed=70 + i)
        cache.set_lens(pos)
        ops.kv_append(qkv, cache, 1)
        put(qkv, pos)
        assert torch.equal(cache.k[1], want_k) and torch.equal(cache.v[1], want_v), (T, pos)
        assert cache.lens.tolist() == pos  # the append does not advance the position
    assert (cache.k[0] == sent).all() and (cache.v[0] == sent).all()  # the other layer is untouched


# ---- skinny GEMM -------------------------------------------------------------------------------

def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)


def _ref_gemm(a, b, bias=None, act="none", residual=None, alpha=1.0):
    c = alpha * (a.float() @ b.float().transpose(-1, -2))
    if bias is not None:
        c = c + bias.float()
    if act == "relu":
        c = torch.relu(c)
    elif act in ("gelu", "gelu_tanh"):
        c = torch.nn.functional.gelu(c, approximate="tanh")
    elif act == "silu":
        c = torch.nn.functional.silu(c)
    if residual is not None:
        c = c + residual.float()
    return c


def _assert_close(out, ref, K):
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    # bf16 output rounding (2^-8 relative) + fp32 accumulation order
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


@pytest.fixture(scope="module")
def weights():
    return {(N, K): _rand(N, K, seed=N + K, scale=0.5) for N, K in [(128, 64), (136, 2056), (1000, 8192),
                                                                      (2048, 2048)]}


@pytest.mark.parametrize("N,K", [(128, 64), (136, 2056), (1000, 8192), (2048, 2048)])
@pytest.mark.parametrize("M", [1, 3, 8, 16])
def test_skinny_gemm_epilogues(M, N, K, weights):
    """Every epilogue on the M-selected kernel and on each arithmetic pattern forced (VALU: M <= 8)."""
    from kubeflow_rm_amd.ops import gemm_nt
    w = weights[(N, K)]
    a = _rand(M, K, seed=M)
    bias = _rand(N, seed=2, scale=2.0)
    res = _rand(M, N, seed=3, scale=4.0)
    for variant in ["skinny", "skinny_mfma"] + (["skinny_valu"] if M <= 8 else []):
        for kw in ({"bias": bias}, {"bias": bias, "act": "gelu_tanh"}, {"bias": bias, "residual": res},
                   {"alpha": 0.37}):
            out = gemm_nt(a, w, variant=variant, **kw)
            assert out.shape == (M, N) and out.dtype == torch.bfloat16
            _assert_close(out, _ref_gemm(a, w, **kw), K)


@pytest.mark.parametrize("M", [3, 16])
def test_skinny_gemm_strided_rows_and_determinism(M):
    from kubeflow_rm_amd.ops import gemm_nt
    N, K = 136, 2056
    w = _rand(N, K, seed=5, scale=0.5)
    abig = _rand(M, K + 64, seed=6)
    a = abig[:, 8:8 + K]                                  # lda = K + 64, 16-B aligned start
    cbig = torch.full((M, N + 24), 9.0, device=DEV, dtype=torch.bfloat16)
    out = gemm_nt(a, w, out=cbig[:, :N], variant="skinny")
    assert out.data_ptr() == cbig.data_ptr()
    _assert_close(cbig[:, :N], _ref_gemm(a, w), K)
    assert (cbig[:, N:] == 9.0).all()
    again = gemm_nt(a.contiguous(), w, variant="skinny")
    assert torch.equal(again, cbig[:, :N])               # two runs, bit-identical
    assert torch.equal(gemm_nt(a.contiguous(), w, variant="skinny"), again)


def test_skinny_gemm_contract_violations_raise():
    from kubeflow_rm_amd.ops import gemm_nt
    w = _rand(128, 64, seed=1)
    with pytest.raises(ValueError):
        gemm_nt(_rand(17, 64, seed=2), w, variant="skinny")
    with pytest.raises(ValueError):
        gemm_nt(_rand(4, 60, seed=3), _rand(128, 60, seed=4), variant="skinny")
    from kubeflow_rm_amd.ops import _lib
    a = _rand(16, 64, seed=2)
    c = torch.empty(17, 128, device=DEV, dtype=torch.bfloat16)
    L = _lib.lib()
    assert L.kfamd_gemm_nt_skinny_bf16(a.data_ptr(), w.data_ptr(), c.data_ptr(), None, None, 17, 128, 64, 64, 64,
                                       128, 0, 1.0, 0, None) == -1
    assert L.kfamd_gemm_nt_skinny_bf16(a.data_ptr() + 2, w.data_ptr(), c.data_ptr(), None, None, 4, 128, 56, 64, 64,
                                       128, 0, 1.0, 0, None) == -2


# ---- model -------------------------------------------------------------------------------------

def _cfg(n_heads, dtype):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=n_heads, d_ff=1024, max_seq=256, dtype=dtype)


@pytest.fixture(scope="module", params=[4, 2], ids=["D64", "D128"])
def models(request):
    from kubeflow_rm_amd.models import GPT
    return GPT(_cfg(request.param, torch.bfloat16), device=DEV).eval(), GPT(_cfg(request.param, torch.float32)).eval()


def test_teacher_forced_decode_matches_fp32_full_forward(models):
    gpu, ref = models
    B, T0, steps = 2, 40, 24
    seq = torch.randint(0, 512, (B, T0 + steps), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)                                   # fp32 CPU logits at every position
        full = gpu(seq.to(DEV)).float().cpu()             # the bf16 GPU full forward
    rows = slice(T0 - 1, T0 + steps)                      # the prefill's position and the 24 steps'
    full_err = (full[:, rows] - want[:, rows]).abs().max().item()
    cache = gpu.new_cache(B, T0 + steps)
    logits = [gpu.prefill(seq[:, :T0].to(DEV), cache)]
    for i in range(steps):                                # fed from the fixed sequence, not argmax-chained
        logits.append(gpu.decode_step(seq[:, T0 + i].to(DEV), cache))
    got = torch.stack([x.float().cpu() for x in logits], 1)
    errs = (got - want[:, rows]).abs().amax(dim=(0, 2))
    print(f"full-forward max-abs {full_err:.4f}; cached per-step max-abs {[round(e, 4) for e in errs.tolist()]}")
    assert full_err < 0.1, full_err
    assert errs.max().item() < 0.1, errs.tolist()
    assert cache.lens.tolist() == [T0 + steps] * B


def _hand_loop(model, idx, new, step=None):
    cache = model.new_cache(idx.shape[0], idx.shape[1] + new)
    logits = [model.prefill(idx, cache).clone()]
    toks = [idx, logits[0].argmax(-1).view(-1, 1)]
    for _ in range(new - 1):
        logits.append(model.decode_step(toks[-1].view(-1), cache).clone())
        toks.append(logits[-1].argmax(-1).view(-1, 1))
    return torch.cat(toks, 1), logits


def test_generate_greedy_equals_hand_loop(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(1)).to(DEV)
    out = gpu.generate(idx, 16)
    assert out.shape == (2, 40) and torch.equal(out[:, :24], idx)
    assert torch.equal(out, _hand_loop(gpu, idx, 16)[0])
    assert torch.equal(gpu.generate(idx, 16, temperature=1.0, top_k=1), out)
    a = gpu.generate(idx, 16, temperature=1.0, generator=torch.Generator(DEV).manual_seed(3))
    b = gpu.generate(idx, 16, temperature=1.0, generator=torch.Generator(DEV).manual_seed(3))
    assert torch.equal(a, b) and torch.equal(a[:, :24], idx)
    with pytest.raises(ValueError):
        gpu.generate(torch.zeros(1, 250, dtype=torch.long, device=DEV), 7)  # 257 > max_seq


def test_graphed_decode_equals_eager(models):
    """One captured decode step replayed over three prompts of different lengths: logits bit-identical
    to the eager steps at every position; generate(graph=True) equals generate(graph=False)."""
    gpu, _ = models
    B, new, cap = 2, 12, 64
    cache = gpu.new_cache(B, cap)
    step = None
    for seed, T0 in ((1, 40), (2, 33), (3, 17)):
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
        assert torch.equal(gpu.generate(idx, new, graph=True), gpu.generate(idx, new, graph=False))


def test_graphed_step_counts_replays_and_bf16_cache_is_required(models):
    """A captured step keeps decode_step's capacity check: the replay that would push lens past the
    capacity raises on the host, and lens stays inside the position table."""
    from kubeflow_rm_amd import ops
    gpu, _ = models
    B, T0 = 1, 20
    idx = torch.randint(0, 512, (B, T0), generator=torch.Generator().manual_seed(4)).to(DEV)
    cache = gpu.new_cache(B, T0 + 2)
    tok = gpu.prefill(idx, cache).argmax(-1)
    step = gpu.graphed_decode_step(cache)
    assert cache.lens.tolist() == [T0]
    step(tok)
    step(tok)
    with pytest.raises(ValueError):
        step(tok)
    with pytest.raises(ValueError):
        gpu.decode_step(tok, cache)
    assert cache.lens.tolist() == [T0 + 2]
    f32 = ops.KVCache(1, 1, 2, 64, 32, device=DEV, dtype=torch.float32)
    f32.set_lens([4])
    with pytest.raises(ValueError):
        ops.attention_decode(_randn(1, 2, 64, seed=2), f32, 0)
