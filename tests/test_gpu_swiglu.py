"""SwiGLU on the gfx950 kernels: the gated weight-streaming GEMM (gemm_skinny_bf16.hip / gemm_skinny_w8.hip with GLU)
and the elementwise gate with its backward (swiglu_bf16.hip), against fp32 torch on the same bf16 (or dequantised)
inputs. The rule under test is the docstring of kubeflow_rm_amd/ops/swiglu.py."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (N = 2F, K). (134, 2064): 67 pairs, a partial tile with a pair count off the 4- and 2-grids, and a partial K chunk
# in both kernels (K = 16 * 129). Then one small-K shape just above each N threshold of the launchers, so that every
# tile count the launchers select runs: MFMA TILES = 2 from 4096, 4 from 16384 (the gated launchers also move to 1 / 4
# by M from 8192); VALU 4 rows per wave from 8192 on 8-bit weights. test_gated_gemm_every_tile_count_forced then
# forces every instantiation. Every K is a multiple of 16, the 8-bit kernel's contract.
SHAPES = [(128, 64), (134, 2064), (2048, 2048), (4100, 64), (8196, 64), (16388, 128)]


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(*shape, generator=g, device="cuda") * 2 - 1) * scale).to(torch.bfloat16)


def _assert_close(out, ref, K):
    """tests/test_gpu_w8.py's bound."""
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= 1e-2 * scale + 1e-2, f"max err {err} vs scale {scale} (K={K})"


def _quantised(N, K, seed):
    """As tests/test_gpu_w8.py: per-row gains spread over 2^-4 .. 2^4, so gate and up rows have different scales."""
    from kubeflow_rm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.rand(N, K, generator=g, device="cuda") - 0.5)
    gains = torch.exp2(torch.rand(N, generator=g, device="cuda") * 8 - 4)
    return ops.quantize_weight(w * gains.unsqueeze(1))


def _ref_glu(a, wf, bias=None, alpha=1.0):
    z = alpha * (a.float() @ wf.t())
    if bias is not None:
        z = z + bias.float()
    return F.silu(z[:, 0::2]) * z[:, 1::2]


@pytest.fixture(scope="module")
def weights():
    out = {}
    for N, K in SHAPES:
        w = _rand(N, K, seed=N + K)
        qw = _quantised(N, K, seed=N + K + 1)
        out[("bf16", N, K)] = (w, w.float())
        out[("w8", N, K)] = (qw, qw.dequantize())  # the fp32 reference weights, computed once
    return out


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 3, 8, 16])
@pytest.mark.parametrize("fmt", ["bf16", "w8"])
def test_gated_skinny_gemm(fmt, M, N, K, weights):
    """The M-selected kernel and each arithmetic form forced (VALU: M <= 8); no bias, a bias of magnitude 2 and
    alpha = 0.37; the output a strided view of a poisoned [M, F + 8] buffer whose padding must stay untouched."""
    from kubeflow_rm_amd.ops import gemm_nt
    w, wref = weights[(fmt, N, K)]
    Fd = N // 2
    a = _rand(M, K, seed=M)
    bias = _rand(N, seed=2, scale=2.0)
    refs = [({}, _ref_glu(a, wref)), ({"bias": bias}, _ref_glu(a, wref, bias)),
            ({"alpha": 0.37}, _ref_glu(a, wref, alpha=0.37))]
    for variant in ["skinny", "skinny_mfma"] + (["skinny_valu"] if M <= 8 else []):
        for kw, ref in refs:
            buf = torch.full((M, Fd + 8), 9.0, device=DEV, dtype=torch.bfloat16)
            out = gemm_nt(a, w, act="swiglu", variant=variant, out=buf[:, :Fd], **kw)
            assert out.data_ptr() == buf.data_ptr() and out.shape == (M, Fd)
            _assert_close(buf[:, :Fd], ref, K)
            assert (buf[:, Fd:] == 9.0).all(), (variant, kw.keys())
    fresh = gemm_nt(a, w, act="swiglu", variant="skinny", bias=bias)  # the allocating form
    assert fresh.shape == (M, Fd) and fresh.dtype == torch.bfloat16
    _assert_close(fresh, refs[1][1], K)


@pytest.mark.parametrize("N,K", [(134, 2064), (8196, 64)])
@pytest.mark.parametrize("fmt", ["bf16", "w8"])
def test_gated_gemm_every_tile_count_forced(fmt, N, K, weights):
    """The launchers pick tile counts and rows per wave by M and N; here every one is forced (MFMA 1 / 2 / 4 tiles
    = 4 / 8 / 16 pairs per workgroup, VALU 2 / 4 rows = 1 / 2 pairs per wave) at a pair count off every grid."""
    from kubeflow_rm_amd.ops.gemm import _gemm_nt_swiglu
    w, wref = weights[(fmt, N, K)]
    bias = _rand(N, seed=2, scale=2.0)
    for M in (1, 3, 4, 16):
        a = _rand(M, K, seed=M)
        ref = _ref_glu(a, wref, bias)
        forced = [("skinny_mfma", t) for t in (1, 2, 4)] + ([("skinny_valu", r) for r in (2, 4)] if M <= 4 else [])
        for variant, tiles in forced:
            buf = torch.full((M, N // 2 + 8), 9.0, device=DEV, dtype=torch.bfloat16)
            _gemm_nt_swiglu(a, w, bias, None, 1.0, buf[:, :N // 2], variant, tiles)
            _assert_close(buf[:, :N // 2], ref, K)
            assert (buf[:, N // 2:] == 9.0).all(), (variant, tiles)


def test_gated_gemm_equals_gemm_then_gate_to_bf16_rounding():
    """The one-launch form against z (fp32 would be exact; z is rounded to bf16 between the two launches) -> the gate
    kernel: same inputs, so the two differ by z's rounding only; here only the shapes and the rule are tied together."""
    from kubeflow_rm_amd import ops
    a, w, b = _rand(4, 256, seed=1), _rand(688, 256, seed=2, scale=0.1), _rand(688, seed=3)
    one = ops.gemm_nt(a, w, bias=b, act="swiglu", variant="skinny")
    two = ops.swiglu(ops.gemm_nt(a, w, bias=b, variant="skinny"))
    assert one.shape == two.shape == (4, 344)
    _assert_close(one, two.float(), 256)
    with ops.torch_reference():
        ref = ops.gemm_nt(a, w, bias=b, act="swiglu", variant="skinny")
    _assert_close(one, ref.float(), 256)


def test_gated_gemm_errors_raise_and_launch_nothing():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    a, w = _rand(4, 64, seed=1), _rand(128, 64, seed=2)
    qw = _quantised(128, 64, seed=3)
    sentinel = torch.full((4, 64), 9.0, device=DEV, dtype=torch.bfloat16)
    for wt in (w, qw):
        with pytest.raises(ValueError):  # odd N
            odd = wt[:127] if wt is w else ops.QuantizedWeight(qw.codes[:127], qw.scale[:127].contiguous())
            ops.gemm_nt(a, odd, act="swiglu", variant="skinny")
        with pytest.raises(ValueError):  # a residual
            ops.gemm_nt(a, wt, act="swiglu", variant="skinny", residual=_rand(4, 64, seed=4), out=sentinel)
        with pytest.raises(ValueError):  # M = 17
            ops.gemm_nt(_rand(17, 64, seed=5), wt, act="swiglu", variant="skinny")
        for variant in ("auto", "w4", "generic"):
            with pytest.raises(ValueError):
                ops.gemm_nt(a, wt, act="swiglu", variant=variant, out=sentinel)
        with pytest.raises(ValueError):  # out of the ungated width
            ops.gemm_nt(a, wt, act="swiglu", variant="skinny", out=torch.empty(4, 128, device=DEV, dtype=torch.bfloat16))
    torch.cuda.synchronize()
    assert (sentinel == 9.0).all()
    # the launchers themselves, before any launch
    L = _lib.lib()
    c = torch.full((17, 64), 9.0, device=DEV, dtype=torch.bfloat16)
    a17 = _rand(17, 64, seed=5)
    assert L.kfamd_gemm_nt_skinny_bf16_glu(a.data_ptr(), w.data_ptr(), c.data_ptr(), None, 4, 127, 64, 64, 64, 64, 1.0,
                                           None) == -1
    assert L.kfamd_gemm_nt_skinny_bf16_glu(a17.data_ptr(), w.data_ptr(), c.data_ptr(), None, 17, 128, 64, 64, 64, 64,
                                           1.0, None) == -1
    assert L.kfamd_gemm_nt_skinny_bf16_glu(a.data_ptr(), w.data_ptr(), c.data_ptr(), None, 4, 128, 64, 64, 64, 63, 1.0,
                                           None) == -1  # ldc < F
    assert L.kfamd_gemm_nt_skinny_bf16_glu_path(1, a17.data_ptr(), w.data_ptr(), c.data_ptr(), None, 9, 128, 64, 64, 64,
                                                64, 1.0, None) == -1  # VALU: M <= 8
    assert L.kfamd_gemm_nt_skinny_w8_glu(a.data_ptr(), qw.codes.data_ptr(), qw.scale.data_ptr(), c.data_ptr(), None, 4,
                                         127, 64, 64, 64, 64, 1.0, None) == -1
    assert L.kfamd_gemm_nt_skinny_w8_glu_tiles(2, 3, a.data_ptr(), qw.codes.data_ptr(), qw.scale.data_ptr(), c.data_ptr(),
                                               None, 4, 128, 64, 64, 64, 64, 1.0, None) == -1
    torch.cuda.synchronize()
    assert (c == 9.0).all()


# ---- the elementwise gate ---------------------------------------------------------------------------------
ELEMENTWISE = [(1, 8), (5, 67), (33, 1024), (300, 136)]  # (5, 67): the scalar path; the others 16-B vectors


def _gate_inputs(rows, Fd, seed):
    """z with gates spread over [-30, 30] (exp saturates both ways, the extremes included) and dh."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(rows, 2 * Fd, generator=g, device=DEV) * 3
    gate = (torch.rand(rows, Fd, generator=g, device=DEV) * 2 - 1) * 30
    wide = torch.rand(rows, Fd, generator=g, device=DEV) < 0.3
    z[:, 0::2] = torch.where(wide, gate, z[:, 0::2])
    z.view(-1)[0], z.view(-1)[2 * min(Fd - 1, 1)] = 30.0, -30.0
    dh = torch.randn(rows, Fd, generator=g, device=DEV)
    return z.to(torch.bfloat16), dh.to(torch.bfloat16)


def _gate_refs(z, dh):
    gf, uf, df = z.float()[:, 0::2], z.float()[:, 1::2], dh.float()
    s = torch.sigmoid(gf)
    return gf * s * uf, df * uf * s * (1 + gf * (1 - s)), df * gf * s, (df * uf).abs()


def _check_gate(h, dz, z, dh):
    """Per element: one bf16 ulp of the fp32 reference, 2^-8 |ref|; plus 1e-5 |dh u| on dz[2j] for the cancellation
    near 1 + g (1 - s) = 0. (Half an ulp, the rounding of an exact result, reaches 2^-8 |ref| only just above a
    power of two; elsewhere the rest of the bound covers the fast exp's and the reference's own fp32 error.)"""
    h_ref, dg_ref, du_ref, dhu = _gate_refs(z, dh)
    ulp = 2.0 ** -8
    if h is not None:
        assert ((h.float() - h_ref).abs() <= ulp * h_ref.abs()).all(), (h.float() - h_ref).abs().max().item()
    if dz is not None:
        dg, du = dz.float()[:, 0::2], dz.float()[:, 1::2]
        assert ((dg - dg_ref).abs() <= ulp * dg_ref.abs() + 1e-5 * dhu).all(), (dg - dg_ref).abs().max().item()
        assert ((du - du_ref).abs() <= ulp * du_ref.abs()).all(), (du - du_ref).abs().max().item()


@pytest.mark.parametrize("rows,Fd", ELEMENTWISE)
def test_swiglu_forward_backward(rows, Fd):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.swiglu import swiglu_bwd, swiglu_fwd
    z, dh = _gate_inputs(rows, Fd, seed=rows + Fd)
    assert z.float()[:, 0::2].abs().max().item() >= 29.0
    _check_gate(swiglu_fwd(z), swiglu_bwd(dh, z), z, dh)
    # a strided z view and a strided output, the padding poisoned (NaN in z's, a sentinel in the output's)
    pad = 8
    zbig = torch.full((rows, 2 * Fd + pad), float("nan"), device=DEV, dtype=torch.bfloat16)
    zbig[:, :2 * Fd] = z
    hbig = torch.full((rows, Fd + pad), 9.0, device=DEV, dtype=torch.bfloat16)
    swiglu_fwd(zbig[:, :2 * Fd], out=hbig[:, :Fd])
    dz = swiglu_bwd(dh, zbig[:, :2 * Fd])
    _check_gate(hbig[:, :Fd], dz, z, dh)
    assert (hbig[:, Fd:] == 9.0).all() and zbig[:, 2 * Fd:].isnan().all()
    assert torch.equal(hbig[:, :Fd], swiglu_fwd(z)) and torch.equal(dz, swiglu_bwd(dh, z))
    # through autograd: ops.swiglu against the torch rule
    zg = z.clone().requires_grad_(True)
    h = ops.swiglu(zg)
    h.backward(dh)
    zr = z.float().requires_grad_(True)
    from kubeflow_rm_amd.ops.swiglu import swiglu_reference
    swiglu_reference(zr).backward(dh.float())
    _check_gate(h.detach(), zg.grad, z, dh)
    dg, dg_t = zg.grad.float()[:, 0::2], zr.grad[:, 0::2]
    assert ((dg - dg_t).abs() <= 2.0 ** -8 * dg_t.abs() + 1e-5 * (dh.float() * z.float()[:, 1::2]).abs()).all()
    assert ((zg.grad.float()[:, 1::2] - zr.grad[:, 1::2]).abs() <= 2.0 ** -8 * zr.grad[:, 1::2].abs()).all()


def test_swiglu_3d_and_torch_reference():
    from kubeflow_rm_amd import ops
    z, _ = _gate_inputs(24, 40, seed=7)
    z3 = z.view(2, 12, 80)
    h = ops.swiglu(z3)
    assert h.shape == (2, 12, 40) and torch.equal(h.view(24, 40), ops.swiglu(z))
    with ops.torch_reference():
        ref = ops.swiglu(z3)
    assert ((h.float() - ref.float()).abs() <= 2.0 ** -7 * ref.float().abs()).all()  # two bf16 roundings apart
    with pytest.raises(ValueError):
        ops.swiglu(z[:, :79])


def test_swiglu_backward_takes_a_broadcast_gradient():
    """``h.sum().backward()`` hands the backward an expanded dh (strides (0, 0)), and a row-broadcast one has strides
    (0, 1): neither is a row-strided view the kernel can read in place; both equal the materialised gradient."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.swiglu import swiglu_bwd
    z, dh = _gate_inputs(6, 24, seed=11)
    row = dh[:1].expand(6, 24)
    assert row.stride() == (0, 1)
    assert torch.equal(swiglu_bwd(row, z), swiglu_bwd(row.contiguous(), z))
    zg = z.clone().requires_grad_(True)
    ops.swiglu(zg).sum().backward()
    assert torch.equal(zg.grad, swiglu_bwd(torch.ones_like(dh), z))
