"""The wide weight-streaming GEMM (kernels/gemm_stream_wide.hip, ops.gemm_nt(variant="stream")), 17 .. 128 rows on
bf16, FP8 and MXFP4 weights: bit-exact on integer operands at every tile count, the inexact epilogues against fp64,
determinism under capture, and the contract."""
from __future__ import annotations

import pytest
import torch

from tests.exact import BF16, FP8, assert_bits_equal, assert_window_bits_equal, exact_ref, framed, int_operand

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMATS = ["bf16", "fp8", "mxfp4"]
_cache: dict = {}


def _weight(fmt, N, K, seed=70, ints=True):
    """(the weight gemm_nt takes, what the references multiply by), made once per (fmt, N, K)."""
    from kubeflow_rm_amd import ops
    key = (fmt, N, K, seed, ints)
    if key not in _cache:
        if fmt == "fp8" and ints:
            w = int_operand(N, K, seed=seed, dtype=FP8)
            _cache[key] = (w, w)
        else:
            v = int_operand(N, K, seed=seed)
            if not ints:  # per-row gains over 2^-3 .. 2^3: a scale at the wrong row shows
                g = torch.Generator().manual_seed(seed)
                v = ((torch.rand(N, K, generator=g) - 0.5) * torch.exp2(torch.rand(N, 1, generator=g) * 6 - 3)).to(BF16).to(DEV)
            if fmt == "bf16":
                _cache[key] = (v, v)
            else:
                q = ops.quantize_weight(v, dtype="mxfp4" if fmt == "mxfp4" else None)
                d = q.dequantize()
                if ints:  # values up to 3 under the group's power-of-two scale lie on e2m1's grid
                    assert torch.equal(d, v.float())
                _cache[key] = (q, d)
    return _cache[key]


# (24, 64): a partial second tile, one chunk (three waves idle); (136, 320): five chunks over four waves; (264, 2080):
# K % 64 == 32, a half-chunk tail; K = 72 is on the bf16 grid only
EXACT = [(f, N, K) for f in FORMATS for N, K in [(24, 64), (136, 320), (264, 2080)]] + [("bf16", 24, 72)]


@pytest.mark.parametrize("M", [17, 32, 33, 128])
@pytest.mark.parametrize("fmt,N,K", EXACT)
def test_stream_bit_exact_on_integer_operands(fmt, M, N, K):
    from kubeflow_rm_amd.ops import gemm_nt, gemm_nt_stream
    w, wref = _weight(fmt, N, K)
    abig = int_operand(M, K + 64, seed=71 + M)
    a = abig[:, 8:8 + K]  # lda = K + 64, a 16-B aligned start
    bias, res = int_operand(N, seed=72, lo=-8, hi=8), int_operand(M, N, seed=73, lo=-8, hi=8)
    for name, kw, rkw in (("residual", {"residual": res}, {"residual": res}), ("relu", {"act": "relu"}, {"relu": True})):
        ref = exact_ref(a, wref, trans_b=True, bias=bias, alpha=0.5, **rkw)
        for tiles in (0, 1, 2, 4):
            big, win = framed(M, N, ld=N + 27, pad_rows=1)
            gemm_nt_stream(a, w, bias=bias, alpha=0.5, out=win, tiles=tiles, **kw)
            assert_window_bits_equal(big, ref, tile=(16, 16), what=f"{fmt} {name} tiles={tiles}")
        out = gemm_nt(a, w, bias=bias, alpha=0.5, variant="stream", **kw)  # ldc = N: the 8-byte stores
        assert_bits_equal(out, ref, tile=(16, 16), what=f"{fmt} {name} gemm_nt")


def _assert_close(out, ref, K):  # the bound of tests/test_gpu_decode.py::_assert_close
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


@pytest.mark.parametrize("fmt,N,K", [("bf16", 136, 2056), ("fp8", 134, 2064), ("mxfp4", 134, 2080)])
def test_stream_inexact_epilogues_against_fp64(fmt, N, K):
    from kubeflow_rm_amd.ops import gemm_nt
    M = 33
    w, wref = _weight(fmt, N, K, seed=74, ints=False)
    g = torch.Generator().manual_seed(75)
    a, bias, res = ((torch.rand(*s, generator=g) * 2 - 1).to(BF16).to(DEV) for s in ((M, K), (N,), (M, N)))
    z = 0.125 * (a.double() @ wref.double().T) + bias.double()
    F = torch.nn.functional
    for act, want in (("gelu", F.gelu(z, approximate="tanh")), ("silu", F.silu(z)), ("none", z + res.double())):
        out = gemm_nt(a, w, bias=bias, alpha=0.125, act=act, residual=res if act == "none" else None, variant="stream")
        _assert_close(out, want, K)
    out = gemm_nt(a, w, bias=bias, alpha=0.125, act="swiglu", variant="stream")
    assert out.shape == (M, N // 2)
    _assert_close(out, F.silu(z[:, 0::2]) * z[:, 1::2], K)


def test_stream_is_deterministic_and_replays_bit_for_bit():
    from kubeflow_rm_amd import ops
    w, _ = _weight("fp8", 264, 2080)
    a, bias = int_operand(33, 2080, seed=76).mul_(0.37), int_operand(264, seed=77)
    run = lambda x: ops.gemm_nt(x, w, bias=bias, act="gelu", variant="stream")  # noqa: E731
    first = run(a).clone()
    assert torch.equal(run(a), first)
    g = ops.GraphedCallable(run, a, warmup=1)
    for _ in range(3):
        assert torch.equal(g(a), first)


def test_stream_contract():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    w = int_operand(32, 64, seed=78)
    with pytest.raises(ValueError):
        ops.gemm_nt(int_operand(129, 64, seed=79), w, variant="stream")
    with pytest.raises(ValueError):  # K = 72 is off the FP8 grid
        ops.gemm_nt(int_operand(20, 72, seed=79), int_operand(32, 72, seed=78, dtype=FP8), variant="stream")
    with pytest.raises(ValueError):
        ops.gemm_nt(int_operand(20, 128, seed=79)[:, ::2], w, variant="stream")
    a, c, L = int_operand(20, 72, seed=79), torch.empty(20, 32, dtype=BF16, device=DEV), _lib.lib()
    call = lambda M, K, lda, p=0: L.kfamd_gemm_nt_stream_bf16(  # noqa: E731
        0, a.data_ptr() + p, w.data_ptr(), c.data_ptr(), None, None, M, 32, K, lda, 64, 32, 0, 1.0, 0, None)
    assert call(129, 64, 72) == -1 and call(0, 64, 72) == -1 and call(20, 60, 72) == -1
    assert call(20, 64, 72, p=2) == -2 and call(20, 64, 68) == -2
    assert L.kfamd_gemm_nt_stream_bf16(3, a.data_ptr(), w.data_ptr(), c.data_ptr(), None, None, 20, 32, 64, 72, 64, 32,
                                       0, 1.0, 0, None) == -1
