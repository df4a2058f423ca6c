"""tests/norm_ref.py against torch's float64 autograd, and the claims made for its input families (no GPU)."""
from __future__ import annotations

import pytest
import torch

from tests import norm_ref as R

SHAPES = [(5, 512), (3, 7), (4, 1), (9, 1000)]


def _close(a, b, scale):
    """float64 against float64: 1e-12 of the result's natural scale (torch's own result is not exactly 0 where the
    terms cancel, as dgamma does at hidden 1: a floor of 1e-12 on operands of size 1)."""
    return bool(((a - b).abs() <= 1e-12 * scale + 1e-12).all())


@pytest.mark.parametrize("rows,H", SHAPES)
@pytest.mark.parametrize("eps", [1e-5, 0.5])
@pytest.mark.parametrize("with_beta", [True, False])
def test_layernorm_reference_matches_float64_autograd(rows, H, eps, with_beta):
    x = R.offset_rows(rows, H, 1) if H > 1 else R.unit_rows(rows, H, 1)
    gamma, beta = R.params(H, 2, with_beta)
    dy, dres = R.correlated_dy(x, eps, 3), R.plain_dy(rows, H, 4)
    xa, ga = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    ba = beta.double().requires_grad_(True) if with_beta else None
    ya = torch.nn.functional.layer_norm(xa, (H,), ga, ba, eps)
    torch.autograd.backward((ya, xa * 1.0), (dy.double(), dres.double()))
    f = R.forward(x, gamma, beta, eps)
    b = R.backward(dy, x, gamma, f.mean, f.rstd, dres)
    assert _close(f.y, ya.detach(), f.y_scale)
    assert _close(f.mean, x.double().mean(1), x.double().abs().mean(1))
    assert _close(f.rstd, 1 / torch.sqrt(x.double().var(1, unbiased=False) + eps), f.rstd)
    assert _close(b.dx, xa.grad, b.dx_scale + dres.double().abs())
    assert _close(b.dgamma, ga.grad, b.dgamma_scale)
    if with_beta:
        assert _close(b.dbeta, ba.grad, b.dbeta_scale)
    # without dres
    xa.grad = None
    torch.nn.functional.layer_norm(xa, (H,), ga, ba, eps).backward(dy.double())
    assert _close(R.backward(dy, x, gamma, f.mean, f.rstd).dx, xa.grad, b.dx_scale)


@pytest.mark.parametrize("rows,H", SHAPES)
@pytest.mark.parametrize("eps", [1e-6, 0.5])
def test_rmsnorm_reference_matches_float64_autograd(rows, H, eps):
    x = R.offset_rows(rows, H, 5) if H > 1 else R.unit_rows(rows, H, 5)
    gamma, _ = R.params(H, 6)
    dy, dres = R.correlated_dy(x, eps, 7, rms=True), R.plain_dy(rows, H, 8)
    xa, ga = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    ya = xa * torch.rsqrt(xa.pow(2).mean(1, keepdim=True) + eps) * ga
    torch.autograd.backward((ya, xa * 1.0), (dy.double(), dres.double()))
    f = R.forward(x, gamma, None, eps, rms=True)
    b = R.backward(dy, x, gamma, None, f.rstd, dres, rms=True)
    assert bool((f.mean == 0).all()) and bool((b.c2 == 0).all())
    assert _close(f.y, ya.detach(), f.y_scale)
    assert _close(f.rstd, torch.rsqrt(x.double().pow(2).mean(1) + eps), f.rstd)
    assert _close(b.dx, xa.grad, b.dx_scale + dres.double().abs())
    assert _close(b.dgamma, ga.grad, b.dgamma_scale)


def test_rms_ignores_beta_and_mean():
    x, (gamma, beta) = R.unit_rows(3, 64, 9), R.params(64, 10)
    assert torch.equal(R.forward(x, gamma, beta, 1e-6, rms=True).y, R.forward(x, gamma, None, 1e-6, rms=True).y)


@pytest.mark.parametrize("lo,hi,lost", [(48, 80, 32), (240, 255, 1024)])
@pytest.mark.parametrize("H", [256, 512, 768, 4096, 8192, 16384])
def test_offset_rows_are_exact_and_defeat_a_one_pass_variance(H, lo, hi, lost):
    """bf16-exact integers whose row sums are exact in fp32 in any order. In fp32 the two-pass variance is within 8
    roundings (2^-24 relative) of the truth; E[x^2] - mean^2 rounds E[x^2] and mean^2, each var-times larger than their
    difference: [48, 80] (4190 - 4100 = 90) is off by more than 32 roundings on some row of 64, [240, 255]
    (61280 - 61260 = 21) by more than 1024."""
    x = R.offset_rows(64, H, 11 + H, lo, hi)
    xd = x.double()
    assert bool((xd == xd.round()).all()) and lo <= xd.min() and xd.max() <= hi
    assert float(xd.sum(1).max()) < 2 ** 24
    f = R.forward(x, torch.ones(H), None, 1e-5)
    mid, spread = (lo + hi) / 2, ((hi - lo + 1) ** 2 - 1) ** 0.5 / 12 ** 0.5
    assert bool(((f.mean - mid).abs() < 3).all()) and bool(((1 / f.rstd - spread).abs() < 0.15 * spread).all())
    xf = x.float()
    mean32 = xf.sum(1) / H
    assert bool(((mean32.double() - f.mean).abs() <= R.ulp32(f.mean)).all())
    var = xd.var(1, unbiased=False)
    two_pass = ((xf - mean32[:, None]) ** 2).sum(1) / H
    one_pass = (xf * xf).sum(1) / H - mean32 * mean32
    e2, e1 = ((two_pass.double() - var).abs() / var).max(), ((one_pass.double() - var).abs() / var).max()
    assert e2 <= 8 * 2.0 ** -24 and e1 > lost * 2.0 ** -24, (float(e1), float(e2))


def test_large_eps_is_visible():
    """eps = 0.5 on unit-variance rows moves rstd by about 18 %: dozens of bf16 ulps of y."""
    x, (gamma, beta) = R.unit_rows(6, 512, 12), R.params(512, 13)
    with_eps, without = R.forward(x, gamma, beta, 0.5), R.forward(x, gamma, beta, 0.0)
    assert bool((with_eps.rstd / without.rstd < 0.85).all())
    moved = (with_eps.y - without.y).abs() > 8 * R.ulp_bf16(R.to_bf16(with_eps.y))
    assert float(moved.double().mean()) > 0.5


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("rows,H", [(5, 256), (4, 512), (3, 8192), (9, 1000)])
def test_correlated_gradients_make_c1_and_c2_visible(rows, H, rms):
    x = R.unit_rows(rows, H, 14)
    gamma, _ = R.params(H, 15)
    eps = 1e-6 if rms else 1e-5
    dy = R.correlated_dy(x, eps, 16, rms=rms)
    f = R.forward(x, gamma, None, eps, rms)
    b = R.backward(dy, x, gamma, f.mean, f.rstd, rms=rms)
    rms_gd = b.gd.pow(2).mean(1).sqrt()
    assert bool((b.c1.abs() >= 0.25 * rms_gd).all()), (b.c1, rms_gd)
    if not rms:
        assert bool((b.c2.abs() >= 0.25 * rms_gd).all()), (b.c2, rms_gd)
    # dropping either term moves most elements of dx by more than a bf16 rounding
    ulp = R.ulp_bf16(R.to_bf16(b.dx))
    assert float(((f.rstd * b.c1)[:, None] * f.xhat).abs().gt(2 * ulp).double().mean()) > 0.5
    if not rms:
        assert float((f.rstd * b.c2)[:, None].abs().expand_as(ulp).gt(2 * ulp).double().mean()) > 0.9


def test_degenerate_rows():
    gamma, beta = R.params(64, 17)
    const = torch.full((2, 64), 3.0, dtype=torch.bfloat16)
    f = R.forward(const, gamma, beta, 1e-5)
    assert torch.equal(f.y, beta.double().expand(2, 64)) and bool((f.xhat == 0).all())
    assert torch.equal(f.rstd, torch.full((2,), 1e-5, dtype=torch.float64).rsqrt())
    b = R.backward(R.plain_dy(2, 64, 18), const, gamma, f.mean, f.rstd)
    assert bool(torch.isfinite(b.dx).all()) and bool((b.dgamma == 0).all())
    zero = torch.zeros(2, 64, dtype=torch.bfloat16)
    assert bool((R.forward(zero, gamma, None, 1e-6, rms=True).y == 0).all())
    one = R.forward(torch.tensor([[2.5]], dtype=torch.bfloat16), gamma[:1], beta[:1], 1e-5)
    assert torch.equal(one.y, beta[:1].double()[None]) and float(one.mean) == 2.5


def test_ulp_helpers():
    v = torch.tensor([0.0, 1.0, 1.5, -2.0, 0.99609375, 3.0e38], dtype=torch.float64)
    assert R.ulp_bf16(v).tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** 120]
    assert R.ulp32(v)[:4].tolist() == [2.0 ** -149, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
    nxt = torch.nextafter(torch.tensor([1.0, 1.5], dtype=torch.bfloat16).float(), torch.tensor(9.0))
    assert torch.equal(R.to_bf16(torch.tensor([1.0 + 2.0 ** -9, 1.5 + 2.0 ** -10], dtype=torch.float64)),
                       torch.tensor([1.0, 1.5], dtype=torch.float64)) and bool((nxt > 1).all())
    assert R.rel_err(torch.tensor([1.0, 0.0]), torch.tensor([1.5, 0.0], dtype=torch.float64),
                     torch.tensor([2.0, 0.0], dtype=torch.float64)) == 0.25
