"""The w4 GEMM at the edges of a grid of more than 256 tiles (more tiles than the chip has CUs, so blocks
follow one another on a CU): interior tiles leave as whole 128-B lines with non-temporal stores
(gemm_w4.h emit_fullline) right next to the masked stores of the shifted last tile row and column.
These are the smallest shapes with more than 256 tiles of 256 x 256, against an fp32 reference with
test_gpu_kernels.py's gemm_nt tolerance. The shapes come from the successor prefetch they were first
written for (profiles/w4_prefetch; that code is gone): a shifted last tile row and column, a partial
first K-tile, a single K-tile, and operands that end where their allocations end."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(*shape, generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)


def _ref_gemm(a, b, bias=None, residual=None):
    c = a.float() @ b.float().transpose(-1, -2)
    if bias is not None:
        c = c + bias.float()
    if residual is not None:
        c = c + residual.float()
    return c


def _assert_close(out, ref, K):
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    # bf16 output rounding (2^-8 relative) + fp32 accumulation order
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


# 4352 x 4096: 17 x 16 = 272 tiles, 16 more than one wave of 256 CUs
# 4392 x 4136 x 200: shifted last tile row and column, partial first K-tile (koff = -56)
# K = 64: one K-tile, no second one for the prologue to stage
@pytest.mark.parametrize("M,N,K", [(4352, 4096, 192), (4392, 4136, 200), (4352, 4096, 64)])
def test_grid_edges(M, N, K):
    from kubeflow_rm_amd.ops import gemm_nt
    a, b = _rand(M, K, seed=41), _rand(N, K, seed=42)
    out = gemm_nt(a, b, variant="w4")
    torch.cuda.synchronize()
    _assert_close(out, _ref_gemm(a, b), K)


@pytest.mark.parametrize("batch", [1, 2])
def test_grid_edges_with_bias_and_residual(batch):
    """The bias and residual loads of the full-line residual epilogue, with and without a batch."""
    from kubeflow_rm_amd.ops import gemm_nt
    M, N, K = 4352, 4096, 64
    lead = (batch,) if batch > 1 else ()
    a, b = _rand(*lead, M, K, seed=43), _rand(*lead, N, K, seed=44)
    bias, r = _rand(N, seed=45), _rand(*lead, M, N, seed=46)
    out = gemm_nt(a, b, bias=bias, residual=r, variant="w4")
    torch.cuda.synchronize()
    _assert_close(out, _ref_gemm(a, b, bias, r), K)


def test_operands_at_the_end_of_their_allocation():
    """A and B end where their allocations end (no load may reach past an operand's last element),
    and the elements after `out` keep their pattern."""
    from kubeflow_rm_amd.ops import gemm_nt
    M, N, K = 4392, 4136, 200
    abuf, bbuf = _rand(4096 + M * K, seed=47), _rand(4096 + N * K, seed=48)
    a, b = abuf[-M * K:].view(M, K), bbuf[-N * K:].view(N, K)
    guard = 1 << 16
    obuf = torch.full((M * N + guard,), -3.0, device="cuda", dtype=torch.bfloat16)
    out = obuf[:M * N].view(M, N)
    assert gemm_nt(a, b, out=out, variant="w4") is out
    torch.cuda.synchronize()
    assert bool((obuf[M * N:] == -3.0).all()), "elements after the output were written"
    _assert_close(out, _ref_gemm(a, b), K)
