"""RMSNorm backward on the HIP kernel (kfamd_rmsnorm_bwd_bf16: the LayerNorm backward's kernels with mean = 0, no c2
term, no dbeta): dx and dgamma against the fp32 formula, with and without the residual gradient folded into the dx
store, with bf16 and fp32 gamma, on every launch path. Tolerances: tests/test_gpu_layernorm_residual.py's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# rows x hidden: the W = 4 wave form (256, 768), the fused one-pass form up to its limit (2048), the dx + partials
# split (4096), the block fallback (1000); odd row counts leave partial workgroups and row chunks
SHAPES = [(7, 256), (64, 768), (130, 2048), (33, 4096), (96, 1000)]
EPS = 1e-6


def _inputs(rows, H, gamma_dtype):
    g = torch.Generator(device="cpu").manual_seed(rows + H)
    x = torch.randn(rows, H, generator=g).to("cuda", torch.bfloat16)
    # bf16-representable in either dtype, so the fp32 parameter and the bf16 copy the kernels read are one value
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16).to("cuda", gamma_dtype)
    gy = torch.randn(rows, H, generator=g).to("cuda", torch.bfloat16)
    gr = torch.randn(rows, H, generator=g).to("cuda", torch.bfloat16)
    return x, w, gy, gr


def _rel(a, b):
    return ((a.float() - b).norm() / b.norm()).item()


@pytest.mark.parametrize("gamma_dtype", [torch.bfloat16, torch.float32], ids=["gamma_bf16", "gamma_fp32"])
@pytest.mark.parametrize("rows,H", SHAPES)
def test_rmsnorm_backward_matches_fp32(rows, H, gamma_dtype):
    from kubeflow_rm_amd import ops
    x0, w0, gy, gr = _inputs(rows, H, gamma_dtype)
    # the fp32 formula, through autograd; the residual path adds gr to dx
    xf, wf = x0.float().requires_grad_(True), w0.detach().clone().float().requires_grad_(True)
    yf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS) * wf
    yf.backward(gy.float())
    dx_ref, dw_ref = xf.grad, wf.grad

    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = ops.rms_norm(x, w, EPS)
    y.backward(gy)
    assert torch.allclose(y.float(), yf, atol=3e-2, rtol=2e-2)
    assert x.grad.dtype == torch.bfloat16 and w.grad.dtype == gamma_dtype
    assert _rel(x.grad, dx_ref) < 1e-2 and _rel(w.grad, dw_ref) < 1e-2

    xr, wr = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y2, r = ops.rms_norm_residual(xr, wr, EPS)
    assert torch.equal(y2, y) and torch.equal(r, x0)
    torch.autograd.backward([y2, r], [gy, gr])
    assert _rel(xr.grad, dx_ref + gr.float()) < 1e-2 and _rel(wr.grad, dw_ref) < 1e-2
    assert torch.equal(wr.grad, w.grad)
    # the dres form is dres + the plain form, to bf16 rounding: with t the fp32 gradient, the plain store is rn(t)
    # and this one rn(dres + t); a bf16 rounding moves a value by at most half an ulp, 2^-8 of it (8 significand
    # bits), so the two differ by at most 2^-8 (|t| + |dres + t|) (1 % for taking the rounded values in the bound;
    # 1e-6 for the fused multiply-add of the dres store)
    plain, withres = x.grad.float(), xr.grad.float()
    bound = 1.01 * 2.0 ** -8 * (plain.abs() + withres.abs()) + 1e-6
    assert ((withres - (gr.float() + plain)).abs() <= bound).all()
    # only the residual output used: its gradient passes through
    x3 = x0.clone().requires_grad_(True)
    ops.rms_norm_residual(x3, w0, EPS)[1].backward(gr)
    assert torch.equal(x3.grad, gr)


def test_rmsnorm_backward_launcher_contract():
    from kubeflow_rm_amd.ops import _lib
    L = _lib.lib()
    x, w, gy, _ = _inputs(8, 256, torch.bfloat16)
    rstd = torch.ones(8, device="cuda")
    dx = torch.full_like(x, 9.0)
    dg = torch.empty(256, device="cuda")
    # dgamma without a workspace, dres aliasing dx, no rstd
    assert L.kfamd_rmsnorm_bwd_bf16(gy.data_ptr(), None, x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                    dg.data_ptr(), 0, None, 8, 256, None) == -1
    assert L.kfamd_rmsnorm_bwd_bf16(gy.data_ptr(), dx.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(),
                                    dx.data_ptr(), None, 0, None, 8, 256, None) == -1
    assert L.kfamd_rmsnorm_bwd_bf16(gy.data_ptr(), None, x.data_ptr(), w.data_ptr(), None, dx.data_ptr(), None, 0, None,
                                    8, 256, None) == -1
    torch.cuda.synchronize()
    assert (dx == 9.0).all()


def test_rmsnorm_backward_sees_an_in_place_update_of_gamma():
    """The backward reads the bf16 gamma the forward read; it is saved through autograd, so an in-place update of
    the parameter between forward and backward raises instead of giving gradients of another gamma."""
    from kubeflow_rm_amd import ops
    x0, w0, gy, _ = _inputs(8, 256, torch.bfloat16)
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = ops.rms_norm(x, w, EPS)
    with torch.no_grad():
        w.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(gy)
