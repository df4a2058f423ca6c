"""MXFP4 decode weights on the gfx950 kernels: the MXFP4 weight-streaming GEMM (kernels/gemm_skinny_mx4.hip) against
fp64 GEMMs on the dequantised weights, exact decoding of every code, and GPT.decode_step / extend /
graphed_decode_step / generate on GPT.decode_weights("mxfp4") against the same model on the dequantised bf16 copies."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (N, K). K = 32: less than one chunk (byte-loaded scales); 288: one chunk + a one-piece tail (the moved scale
# window); 2080: every wave + a tail; N = 1, 7: a partial 8-row tile; then one small-K shape just above each N threshold
# of the launcher: MFMA TILES = 2 from 4096, 4 from 16384; VALU 4 rows per wave from 8192.
SHAPES = [(1, 32), (7, 288), (133, 2080), (4100, 64), (8196, 64), (16388, 64)]
# (variant, forced tiles / rows per wave, largest M)
FORMS = [("skinny", 0, 16), ("skinny_mfma", 1, 16), ("skinny_mfma", 2, 16), ("skinny_mfma", 4, 16),
         ("skinny_valu", 2, 8), ("skinny_valu", 4, 4)]


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)


def _quantised(N, K, seed):
    """As tests/test_gpu_w8.py: uniform(-0.5, 0.5) with per-row gains over 2^-4 .. 2^4, so a misplaced scale shows."""
    from kubeflow_rm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.rand(N, K, generator=g, device="cuda") - 0.5)
    gains = torch.exp2(torch.rand(N, generator=g, device="cuda") * 8 - 4)
    return ops.quantize_weight(w * gains.unsqueeze(1), dtype="mxfp4")


def _ref_gemm(a, wref, bias=None, act="none", residual=None, alpha=1.0, glu=False):
    c = alpha * (a.double() @ wref.double().T)
    if bias is not None:
        c = c + bias.double()
    if glu:
        return torch.nn.functional.silu(c[:, 0::2]) * c[:, 1::2]
    if act == "gelu_tanh":
        c = torch.nn.functional.gelu(c, approximate="tanh")
    if residual is not None:
        c = c + residual.double()
    return c


def _assert_close(out, ref, K):
    err = (out.double() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    # tests/test_gpu_w8.py's bound: bf16 output rounding (2^-8 relative) + fp32 accumulation order; the products exact
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


def _gemm(a, qw, variant, tiles, **kw):
    from kubeflow_rm_amd.ops import gemm
    kw = {"bias": None, "residual": None, "alpha": 1.0, "act": "none", "out": None, **kw}
    if kw["act"] == "swiglu":
        return gemm._gemm_nt_swiglu(a, qw, kw["bias"], None, kw["alpha"], kw["out"], variant, tiles=tiles)
    return gemm._gemm_nt_mx4(a, qw, kw["bias"], kw["residual"], kw["alpha"], kw["act"], kw["out"], variant, tiles=tiles)


@pytest.fixture(scope="module")
def weights():
    out = {}
    for N, K in SHAPES:
        qw = _quantised(N, K, seed=N + K)
        out[(N, K)] = (qw, qw.dequantize())  # the reference weight, computed once
    return out


@pytest.mark.parametrize("variant,tiles,max_m", FORMS)
def test_mx4_every_code_decodes_exactly(variant, tiles, max_m):
    """19 rows x K = 64: every group has its own scale byte and holds the 16 codes in both nibble positions. A = 16
    rows of the identity at column offset c: out[m][n] is dequantize()[n][c + m], bit for bit."""
    from kubeflow_rm_amd import ops
    N, K = 19, 64
    n, k = torch.arange(N).view(N, 1), torch.arange(K).view(1, K)
    code = ((k + n + k // 16) % 16).to(torch.uint8)
    qw = ops.MXFP4Weight((code[:, 0::2] | (code[:, 1::2] << 4)).to(DEV), (105 + 2 * n + k[:, ::32] // 32).to(torch.uint8)
                         .to(DEV))
    want = qw.dequantize()
    for c in (0, 16, 32, 48):
        a = torch.zeros(16, K, device=DEV, dtype=torch.bfloat16)
        a[torch.arange(16), c + torch.arange(16)] = 1.0
        for m0 in range(0, 16, max_m):
            got = _gemm(a[m0:m0 + max_m], qw, variant, tiles)
            assert torch.equal(got.float(), want[:, c + m0:c + m0 + max_m].T), (c, m0)
    if variant == "skinny_valu":  # the one- and two-row instantiations
        for M in (1, 2):
            assert torch.equal(_gemm(a[:M], qw, variant, tiles).float(), want[:, 48:48 + M].T)


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8, 9, 16])
def test_mx4_gemm_epilogues(M, N, K, weights):
    from kubeflow_rm_amd.ops import gemm_nt
    qw, wref = weights[(N, K)]
    a = _rand(M, K, seed=M)
    bias = _rand(N, seed=2, scale=2.0)
    res = _rand(M, N, seed=3, scale=4.0)
    for variant in ["skinny", "skinny_mfma"] + (["skinny_valu"] if M <= 8 else []):
        for kw in ({"bias": bias}, {"bias": bias, "act": "gelu_tanh"}, {"bias": bias, "residual": res},
                   {"alpha": 0.37}):
            _assert_close(gemm_nt(a, qw, variant=variant, **kw), _ref_gemm(a, wref, **kw), K)


@pytest.mark.parametrize("variant,tiles,max_m", FORMS[1:])
@pytest.mark.parametrize("N,K", [(7, 288), (133, 2080)])
def test_mx4_forced_tile_counts(variant, tiles, max_m, N, K, weights):
    qw, wref = weights[(N, K)]
    bias = _rand(N, seed=2, scale=2.0)
    for M in (1, 3, max_m):
        a = _rand(M, K, seed=M)
        _assert_close(_gemm(a, qw, variant, tiles, bias=bias), _ref_gemm(a, wref, bias=bias), K)


@pytest.mark.parametrize("Fd", [4, 66])
@pytest.mark.parametrize("M", [1, 4, 16])
def test_mx4_gated_form(M, Fd):
    from kubeflow_rm_amd import ops
    K = 288
    qw = _quantised(2 * Fd, K, seed=Fd)
    wref = qw.dequantize()
    a = _rand(M, K, seed=M)
    bias = _rand(2 * Fd, seed=2)
    assert ops.gemm_nt(a, qw, bias=bias, act="swiglu", variant="skinny").shape == (M, Fd)
    for variant, tiles, max_m in FORMS:
        if M <= max_m:
            for kw in ({"bias": bias}, {"alpha": 0.37}):
                _assert_close(_gemm(a, qw, variant, tiles, act="swiglu", **kw), _ref_gemm(a, wref, glu=True, **kw), K)


@pytest.mark.parametrize("M", [3, 16])
def test_mx4_strided_rows_sentinels_determinism_and_graph(M):
    from kubeflow_rm_amd import ops
    N, K = 133, 2080
    qw = _quantised(N, K, seed=5)
    abig = _rand(M, K + 64, seed=6)
    a = abig[:, 8:8 + K]                                  # lda = K + 64, 16-B aligned start
    cbig = torch.full((M + 2, N + 27), 9.0, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt(a, qw, out=cbig[:M, :N], variant="skinny")
    _assert_close(cbig[:M, :N], _ref_gemm(a, qw.dequantize()), K)
    assert (cbig[:, N:] == 9.0).all() and (cbig[M:] == 9.0).all()
    ac = a.contiguous()
    again = ops.gemm_nt(ac, qw, variant="skinny")
    assert torch.equal(again, cbig[:M, :N])              # two runs, bit-identical
    graphed = ops.GraphedCallable(lambda x: ops.gemm_nt(x, qw, variant="skinny"), ac.clone(), warmup=1)
    assert torch.equal(graphed(ac), again)               # a captured launch replays bit-identically
    assert torch.equal(graphed(ac), again)


def test_mx4_contract_violations_raise():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    qw = _quantised(128, 64, seed=1)
    with pytest.raises(ValueError):
        ops.gemm_nt(_rand(17, 64, seed=2), qw, variant="skinny")
    with pytest.raises(ValueError):
        ops.gemm_nt(_rand(4, 64, seed=2), qw, variant="auto")
    with pytest.raises(ValueError):  # K mismatch
        ops.gemm_nt(_rand(4, 96, seed=2), qw, variant="skinny")
    wide = _quantised(128, 128, seed=5)
    with pytest.raises(ValueError):  # a non-unit inner stride
        ops.gemm_nt(_rand(4, 64, seed=2), ops.MXFP4Weight(wide.codes[:, ::2], qw.scales), variant="skinny")
    # the launcher itself, before any launch
    a = _rand(17, 64, seed=2)
    c = torch.full((17, 128), 9.0, device=DEV, dtype=torch.bfloat16)
    L = _lib.lib()
    args = (a.data_ptr(), qw.codes.data_ptr(), qw.scales.data_ptr(), c.data_ptr(), None, None)
    assert L.kfamd_gemm_nt_skinny_mx4(*args, 17, 128, 64, 64, 32, 2, 128, 0, 1.0, 0, None) == -1
    assert L.kfamd_gemm_nt_skinny_mx4(*args, 4, 128, 48, 64, 32, 2, 128, 0, 1.0, 0, None) == -1       # K % 32
    assert L.kfamd_gemm_nt_skinny_mx4(*args, 4, 128, 64, 64, 32, 1, 128, 0, 1.0, 0, None) == -1       # lds < K / 32
    assert L.kfamd_gemm_nt_skinny_mx4(a.data_ptr(), wide.codes.data_ptr() + 4, qw.scales.data_ptr(), c.data_ptr(), None,
                                      None, 4, 127, 64, 64, 64, 2, 128, 0, 1.0, 0, None) == -2
    assert L.kfamd_gemm_nt_skinny_mx4_path(1, *args, 9, 128, 64, 64, 32, 2, 128, 0, 1.0, 0, None) == -1  # VALU: M <= 8
    assert L.kfamd_gemm_nt_skinny_mx4_glu_tiles(2, 3, *args[:5], 4, 128, 64, 64, 32, 2, 64, 1.0, None) == -1
    torch.cuda.synchronize()
    assert (c == 9.0).all()


# ---- model -------------------------------------------------------------------------------------

CONFIGS = {"default": {}, "llama": dict(norm="rms", mlp="swiglu", pos="rope", n_kv_heads=2, d_ff=352)}


@pytest.fixture(scope="module", params=list(CONFIGS))
def model(request):
    from kubeflow_rm_amd.models import GPT, GPTConfig
    cfg = GPTConfig(**{**dict(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024, max_seq=128),
                       **CONFIGS[request.param]})
    return GPT(cfg, device=DEV).eval()


def test_mx4_steps_match_the_dequantised_bf16_copies(model):
    """decode_step, extend(T = 4) and graphed_decode_step on the MXFP4 weights against the same model reading
    dequantize().to(bf16) (an exact copy) in every block linear and the tied head: summation order apart."""
    from kubeflow_rm_amd.models.gpt import DecodeWeights
    W = model.decode_weights("mxfp4")
    srcs = [getattr(blk, n).weight for blk in model.blocks for n in ("qkv", "proj", "fc1", "fc2")] + [model.tok]
    assert W.unquantized == [] and W.nbytes == sum(p.numel() // 2 + p.numel() // 32 for p in srcs)
    bf = [q.dequantize().to(torch.bfloat16) for q in W.matrices()]
    assert all(torch.equal(b.float(), q.dequantize()) for b, q in zip(bf, W.matrices()))
    plain = DecodeWeights([dict(zip(("qkv", "proj", "fc1", "fc2"), bf[4 * i:4 * i + 4])) for i in range(2)], bf[-1],
                          W._key)
    B = 2
    idx = torch.randint(0, 512, (B, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    got, want = [], []
    for weights, outs in ((W, got), (plain, want)):
        cache = model.new_cache(B, 32)
        model.prefill(idx[:, :6], cache)
        outs.append(model.extend(idx[:, 6:10], cache, weights=weights)[:, -1])
        outs.append(model.decode_step(idx[:, 10], cache, weights=weights))
        outs.append(model.graphed_decode_step(cache, weights=weights)(idx[:, 11]).clone())
    for g, w in zip(got, want):
        err = (g.float() - w.float()).abs().max().item()
        assert err < 0.1, err  # tests/test_gpu_w8.py's bound for its like-for-like model comparison


def test_mx4_generate_graphed_fused_equals_eager(model):
    idx = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(weight_dtype="mxfp4", sampler="fused")
    assert torch.equal(model.generate(idx, 10, graph=True, **kw), model.generate(idx, 10, **kw))
