"""FP8 decode weights on the gfx950 kernels: the W8A16 weight-streaming GEMM (kernels/gemm_skinny_w8.hip)
against fp32 GEMMs on the dequantised weights, and GPT.decode_step / extend / graphed_decode_step / generate
on GPT.decode_weights() against an fp32 CPU model built from the same codes."""
from __future__ import annotations

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn

# (N, K): the bf16 kernel's sweep moved to the K % 16 contract (N = 133: a partial row tile; K = 2064 =
# 16 * 129: a partial chunk), then one small-K shape just above each N threshold of the launcher, so that
# every tile-count instantiation runs: MFMA TILES = 2 from 4096, 4 from 16384; VALU 4 rows per wave from 8192.
SHAPES = [(128, 64), (133, 2064), (1000, 8192), (2048, 2048), (4100, 64), (8196, 64), (16388, 128)]


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
    # bf16 output rounding (2^-8 relative) + fp32 accumulation order; the products on codes are exact
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


def _quantised(N, K, seed):
    """quantize_weight of uniform(-0.5, 0.5) with per-row gains spread over 2^-4 .. 2^4: the row scales differ,
    so a scale applied to the wrong row or at the wrong place shows."""
    from kubeflow_rm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.rand(N, K, generator=g, device="cuda") - 0.5)
    gains = torch.exp2(torch.rand(N, generator=g, device="cuda") * 8 - 4)
    return ops.quantize_weight(w * gains.unsqueeze(1))


@pytest.fixture(scope="module")
def weights():
    out = {}
    for N, K in SHAPES:
        qw = _quantised(N, K, seed=N + K)
        out[(N, K)] = (qw, qw.dequantize())  # the fp32 reference weight, computed once
    return out


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 3, 8, 16])
def test_w8_gemm_epilogues(M, N, K, weights):
    """Every epilogue on the M-selected kernel and on each arithmetic form forced (VALU: M <= 8)."""
    from kubeflow_rm_amd.ops import gemm_nt
    qw, wref = weights[(N, K)]
    a = _rand(M, K, seed=M)
    bias = _rand(N, seed=2, scale=2.0)  # magnitude 2: a scaled bias would show
    res = _rand(M, N, seed=3, scale=4.0)
    for variant in ["skinny", "skinny_mfma"] + (["skinny_valu"] if M <= 8 else []):
        for kw in ({"bias": bias}, {"bias": bias, "act": "gelu_tanh"}, {"bias": bias, "residual": res},
                   {"alpha": 0.37}):
            out = gemm_nt(a, qw, variant=variant, **kw)
            assert out.shape == (M, N) and out.dtype == torch.bfloat16
            _assert_close(out, _ref_gemm(a, wref, **kw), K)


def test_w8_every_code_decodes_exactly():
    """codes[n][k] = byte 16 n + k (NaN codes replaced by 0), unit scales, A = identity: the output is the
    code table itself, bit for bit: subnormals, -0, +-448, and K = 16 (less than one chunk)."""
    from kubeflow_rm_amd import ops
    raw = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    raw[0x7F] = 0
    raw[0xFF] = 0
    codes = raw.view(16, 16).to(DEV).view(FP8)
    qw = ops.QuantizedWeight(codes, torch.ones(16, device=DEV))
    want = codes.float().T.contiguous()  # out[m][n] = codes[n][m]
    assert want.abs().max().item() == 448.0 and (want.abs() == 2.0 ** -9).any()
    eye = torch.eye(16, device=DEV, dtype=torch.bfloat16)
    for variant in ("skinny", "skinny_mfma"):
        got = ops.gemm_nt(eye, qw, variant=variant)
        assert torch.equal(got.float(), want), variant
    for half in (slice(0, 8), slice(8, 16)):
        got = ops.gemm_nt(eye[half].contiguous(), qw, variant="skinny_valu")
        assert torch.equal(got.float(), want[half]), half


@pytest.mark.parametrize("M", [3, 16])
def test_w8_strided_rows_sentinels_determinism_and_graph(M):
    from kubeflow_rm_amd import ops
    N, K = 133, 2064
    qw = _quantised(N, K, seed=5)
    abig = _rand(M, K + 64, seed=6)
    a = abig[:, 8:8 + K]                                  # lda = K + 64, 16-B aligned start
    cbig = torch.full((M, N + 27), 9.0, device=DEV, dtype=torch.bfloat16)
    out = ops.gemm_nt(a, qw, out=cbig[:, :N], variant="skinny")
    assert out.data_ptr() == cbig.data_ptr()
    _assert_close(cbig[:, :N], _ref_gemm(a, qw.dequantize()), K)
    assert (cbig[:, N:] == 9.0).all()
    ac = a.contiguous()
    again = ops.gemm_nt(ac, qw, variant="skinny")
    assert torch.equal(again, cbig[:, :N])               # two runs, bit-identical
    assert torch.equal(ops.gemm_nt(ac, qw, variant="skinny"), again)
    graphed = ops.GraphedCallable(lambda x: ops.gemm_nt(x, qw, variant="skinny"), ac.clone(), warmup=1)
    assert torch.equal(graphed(ac), again)               # a captured launch replays bit-identically
    assert torch.equal(graphed(ac), again)


def test_w8_contract_violations_raise():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    qw = _quantised(128, 64, seed=1)
    with pytest.raises(ValueError):
        ops.gemm_nt(_rand(17, 64, seed=2), qw, variant="skinny")
    with pytest.raises(ValueError):
        ops.gemm_nt(_rand(4, 24, seed=3), _quantised(128, 24, seed=4), variant="skinny")
    for variant in ("auto", "w4"):
        with pytest.raises(ValueError):
            ops.gemm_nt(_rand(4, 64, seed=2), qw, variant=variant)
    wide = _quantised(128, 128, seed=5)
    with pytest.raises(ValueError):  # a non-unit inner stride
        ops.gemm_nt(_rand(4, 64, seed=2), ops.QuantizedWeight(wide.codes[:, ::2], wide.scale), variant="skinny")
    # the launcher itself, before any launch; the buffers are large enough for what the calls claim
    a = _rand(17, 64, seed=2)
    c = torch.empty(17, 128, device=DEV, dtype=torch.bfloat16)
    big = _quantised(128, 80, seed=6)
    L = _lib.lib()
    assert L.kfamd_gemm_nt_skinny_w8(a.data_ptr(), qw.codes.data_ptr(), qw.scale.data_ptr(), c.data_ptr(), None, None,
                                     17, 128, 64, 64, 64, 128, 0, 1.0, 0, None) == -1
    assert L.kfamd_gemm_nt_skinny_w8(a.data_ptr(), big.codes.data_ptr() + 4, big.scale.data_ptr(), c.data_ptr(), None,
                                     None, 4, 128, 64, 64, 80, 128, 0, 1.0, 0, None) == -2
    assert L.kfamd_gemm_nt_skinny_w8_path(1, a.data_ptr(), qw.codes.data_ptr(), qw.scale.data_ptr(), c.data_ptr(), None,
                                          None, 9, 128, 64, 64, 64, 128, 0, 1.0, 0, None) == -1  # VALU: M <= 8


# ---- model -------------------------------------------------------------------------------------

def _cfg(n_heads, dtype):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=n_heads, d_ff=1024, max_seq=256, dtype=dtype)


@pytest.fixture(scope="module", params=[4, 2], ids=["D64", "D128"])
def models(request):
    from kubeflow_rm_amd.models import GPT
    return GPT(_cfg(request.param, torch.bfloat16), device=DEV).eval(), GPT(_cfg(request.param, torch.float32)).eval()


def _cpu(qw):
    from kubeflow_rm_amd import ops
    return ops.QuantizedWeight(qw.codes.cpu(), qw.scale.cpu())


def test_teacher_forced_decode_on_fp8_weights_matches_fp32_dequantised_forward(models):
    """extend (T = 8, B = 2: 16 rows) then decode_steps, all on the 8-bit weights, against the fp32 CPU model
    whose block linears hold the SAME codes dequantised and whose head is h @ head.dequantize().T: the
    quantisation error is excluded by construction, the bound is the bf16 cached path's own."""
    gpu, ref = models
    B, T, steps = 2, 8, 16
    W = gpu.decode_weights()
    seq = torch.randint(0, 512, (B, T + steps), generator=torch.Generator().manual_seed(0))
    deq = copy.deepcopy(ref)
    with torch.no_grad():
        for blk, qb in zip(deq.blocks, W.blocks):
            for name in ("qkv", "proj", "fc1", "fc2"):
                getattr(blk, name).weight.copy_(_cpu(qb[name]).dequantize())
        x = F.embedding(seq, deq.tok) + deq.pos[:seq.shape[1]]
        for blk in deq.blocks:
            x = blk(x)
        want = deq.ln_f(x) @ _cpu(W.head).dequantize().T
    cache = gpu.new_cache(B, T + steps)
    got = [gpu.extend(seq[:, :T].to(DEV), cache, weights=W).float().cpu()]
    for i in range(steps):
        got.append(gpu.decode_step(seq[:, T + i].to(DEV), cache, weights=W).float().cpu().unsqueeze(1))
    got = torch.cat(got, 1)
    errs = (got - want).abs().amax(dim=(0, 2))
    print(f"fp8 weights, cached per-position max-abs {[round(e, 4) for e in errs.tolist()]}")
    assert errs.max().item() < 0.1, errs.tolist()
    assert cache.lens.tolist() == [T + steps] * B


def test_steps_read_the_quantised_tensors(models):
    """A DecodeWeights whose head codes are all zero gives zero logits; with more than 16 rows the head is
    the model's own again."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models.gpt import DecodeWeights
    gpu, _ = models
    W = gpu.decode_weights()
    zero_head = ops.QuantizedWeight(torch.zeros_like(W.head.codes.view(torch.uint8)).view(FP8), W.head.scale)
    Z = DecodeWeights(W.blocks, zero_head, W._key)
    tok = torch.randint(0, 512, (2,), generator=torch.Generator().manual_seed(1)).to(DEV)
    cache = gpu.new_cache(2, 40)
    assert (gpu.decode_step(tok, cache, weights=Z) == 0).all()
    assert (gpu.extend(tok.view(2, 1).repeat(1, 8), cache, weights=Z) == 0).all()           # 16 rows
    cache.reset()
    many = tok.view(2, 1).repeat(1, 16)                                                     # 32 rows
    c2 = gpu.new_cache(2, 40)
    assert torch.equal(gpu.extend(many, cache, weights=Z), gpu.extend(many, c2))


def _hand_loop(model, idx, new, W, kv_dtype=None):
    cache = model.new_cache(idx.shape[0], idx.shape[1] + new, kv_dtype=kv_dtype)
    logits = [model.prefill(idx, cache).clone()]
    toks = [idx, logits[0].argmax(-1).view(-1, 1)]
    for _ in range(new - 1):
        logits.append(model.decode_step(toks[-1].view(-1), cache, weights=W).clone())
        toks.append(logits[-1].argmax(-1).view(-1, 1))
    return torch.cat(toks, 1), logits


def test_graphed_fp8_weight_step_equals_eager(models):
    gpu, _ = models
    B, T0, new = 2, 21, 10
    W = gpu.decode_weights()
    idx = torch.randint(0, 512, (B, T0), generator=torch.Generator().manual_seed(2)).to(DEV)
    want_toks, want_logits = _hand_loop(gpu, idx, new, W)
    cache = gpu.new_cache(B, 64)
    logits = gpu.prefill(idx, cache)
    step = gpu.graphed_decode_step(cache, weights=W)
    toks = [idx]
    for i in range(new):
        torch.testing.assert_close(logits, want_logits[i], rtol=0, atol=0)
        toks.append(logits.argmax(-1).view(-1, 1))
        if i + 1 < new:
            logits = step(toks[-1].view(-1))
    assert torch.equal(torch.cat(toks, 1), want_toks)


def test_generate_on_fp8_weights_and_cache_graphed_equals_hand_loop(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(3)).to(DEV)
    want, _ = _hand_loop(gpu, idx, 12, gpu.decode_weights(), kv_dtype=FP8)
    out = gpu.generate(idx, 12, weight_dtype=FP8, kv_dtype=FP8, graph=True)
    assert out.shape == (2, 36) and torch.equal(out, want)
    assert torch.equal(gpu.generate(idx, 12, weight_dtype=FP8, kv_dtype=FP8), want)
    with pytest.raises(ValueError):
        gpu.generate(idx, 4, weight_dtype=torch.int8)


def test_decode_weights_bytes(models):
    gpu, _ = models
    W = gpu.decode_weights()
    assert gpu.decode_weights() is W
    srcs = [getattr(blk, n).weight for blk in gpu.blocks for n in ("qkv", "proj", "fc1", "fc2")] + [gpu.tok]
    assert W.nbytes == sum(p.shape[0] * p.shape[1] + 4 * p.shape[0] for p in srcs)
    # (K + 4) / 2K with K >= 256 is at most 0.5078
    assert W.nbytes < 0.51 * sum(p.numel() * 2 for p in srcs)
    assert all(q.codes.is_cuda and q.codes.dtype == FP8 for q in W.matrices())
    assert not any(k.startswith("_decode") for k in gpu.state_dict())
