"""The dense W8A8 FP8 GEMM (kernels/gemm_fp8.hip, gemm_nt(variant="w8a8")) and its activation quantiser
(ops.quantize_act): bit-exact on integer operands at every tile edge of both plans, nothing read beyond M, N, K,
the quantiser against ops.decode.quantize_rows bit for bit, random data against the rule in fp64."""
from __future__ import annotations

import pytest
import torch

from tests.exact import (FP8, assert_bits_equal, assert_window_bits_equal, exact_ref, framed, int_operand)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = (16, 112, 128, 144, 400)  # below, on and across the 128-byte K step


def _expected(a, b, **kw):
    """exact_ref on a's integer codes, times a's power-of-two row scales (which commute with the one rounding)."""
    return (exact_ref(a.codes.float(), b, trans_b=True, **kw).float() * a.scale[:, None]).to(torch.bfloat16)


@pytest.mark.parametrize("plan", ["large", "small"])
@pytest.mark.parametrize("N", [1, 33, 136, 257])
@pytest.mark.parametrize("M", [1, 31, 100, 257])
def test_w8a8_bit_exact_on_integer_operands(M, N, plan):
    from kubeflow_rm_amd.ops import gemm_nt_w8a8
    for K in KS:
        a = int_operand(M, K, dtype=FP8, seed=M + K)
        b = int_operand(N, K, dtype=FP8, seed=N + K + 1)
        what = f"M={M} N={N} K={K} {plan}"
        assert_bits_equal(gemm_nt_w8a8(a, b, plan=plan), _expected(a, b), what=what)
        assert_bits_equal(gemm_nt_w8a8(a, b, alpha=0.5, act="relu", plan=plan),
                          _expected(a, b, alpha=0.5, relu=True), what=what + " alpha relu")
        a1 = type(a)(a.codes, torch.ones_like(a.scale))  # with a bias or a residual the row scale no longer commutes
        bias = int_operand(N, seed=3, lo=-8, hi=8)
        res = int_operand(M, N, seed=4, lo=-8, hi=8)
        assert_bits_equal(gemm_nt_w8a8(a1, b, bias=bias, residual=res, act="relu", plan=plan),
                          _expected(a1, b, bias=bias, residual=res, relu=True), what=what + " bias relu residual")


@pytest.mark.parametrize("plan", ["large", "small"])
@pytest.mark.parametrize("M,N,K", [(31, 33, 112), (257, 136, 400)])
def test_w8a8_reads_nothing_beyond_m_n_k_and_writes_only_its_window(M, N, K, plan):
    """Operands as views into NaN-filled buffers (code 0x7F after every row's K bytes and in the rows after M / N, NaN
    in the spare scales); the output a window at an odd column of a sentinel frame with an odd row stride."""
    from kubeflow_rm_amd import ops

    def embedded(q):
        rows = q.codes.shape[0]
        codes = torch.full((rows + 5, K + 48), 0x7F, dtype=torch.uint8, device=DEV)
        scale = torch.full((rows + 5,), float("nan"), device=DEV)
        codes[:rows, :K] = q.codes.view(torch.uint8)
        scale[:rows] = q.scale
        return ops.QuantizedWeight(codes[:rows, :K].view(FP8), scale[:rows])
    a, b = int_operand(M, K, dtype=FP8, seed=5), int_operand(N, K, dtype=FP8, seed=6)
    big, win = framed(M, N, ld=N + 13, col0=5, pad_rows=3)
    ops.gemm_nt_w8a8(embedded(a), embedded(b), out=win, plan=plan)
    assert_window_bits_equal(big, _expected(a, b), col0=5, what=f"{M}x{N}x{K} {plan}")


@pytest.mark.parametrize("K", [16, 2048, 4112])
@pytest.mark.parametrize("M", [1, 5, 130])
def test_quantize_act_is_quantize_rows(M, K):
    from kubeflow_rm_amd import ops
    g = torch.Generator(device=DEV).manual_seed(M + K)
    big = (torch.randn(M, K + 24, generator=g, device=DEV) * 3).to(torch.bfloat16)
    big[M // 2] = 0                      # an all-zero row
    big[0, :K] *= 0.25
    big[0, K - 1] = 50.0                 # the amax is the row's last element
    for x in (big[:, :K].contiguous(), big[:, :K], big[:, 4:4 + K]):  # contiguous, strided, strided off the 16-B grid
        # the rule's divisions are IEEE: quantize_rows on the CPU copy, as tests/test_gpu_kv_fp8.py takes it (torch's
        # GPU division by a host scalar multiplies by the reciprocal)
        got, (codes, scale) = ops.quantize_act(x), ops.decode.quantize_rows(x.cpu())
        assert torch.equal(got.scale.cpu(), scale)
        assert torch.equal(got.codes.view(torch.uint8).cpu(), codes.view(torch.uint8))


@pytest.mark.parametrize("M,N,K", [(100, 136, 400), (300, 515, 2064)])
def test_w8a8_random_bf16_activation_against_the_rule_in_fp64(M, N, K):
    from kubeflow_rm_amd import ops
    g = torch.Generator(device=DEV).manual_seed(N)
    a = (torch.rand(M, K, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16)
    gains = torch.exp2(torch.rand(N, 1, generator=g, device=DEV) * 8 - 4)  # row scales that differ
    qw = ops.quantize_weight((torch.rand(N, K, generator=g, device=DEV) - 0.5) * gains * 0.05)
    bias = (torch.rand(N, generator=g, device=DEV) * 4 - 2).to(torch.bfloat16)
    codes, scale = (t.to(DEV) for t in ops.decode.quantize_rows(a.cpu()))  # the CPU's IEEE divisions
    z = (codes.double() * scale.double()[:, None]) @ qw.dequantize().double().T + bias.double()
    ref = torch.nn.functional.gelu(z, approximate="tanh").float()
    # tests/test_gpu_w8.py's _assert_close, restated: bf16 output rounding (2^-8 relative) + fp32 accumulation order;
    # the products on codes are exact
    err = (ops.gemm_nt(a, qw, variant="w8a8", act="gelu", bias=bias).float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


def test_w8a8_argument_errors_raise_before_a_launch():
    from kubeflow_rm_amd import ops
    from tests.test_w8a8_cpu import bad_calls
    for a, b, kw, why in bad_calls(DEV):
        with pytest.raises(ValueError, match=f"w8a8.*{why}"):
            ops.gemm_nt(a, b, variant="w8a8", **kw)
