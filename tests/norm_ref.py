"""LayerNorm / RMSNorm in plain float64 on the CPU (a helper module, not a conftest), and the input families of
tests/test_gpu_norm_rows.py.

Inputs are bf16 (or already float64) CPU tensors; every value is widened exactly, so the results are those of the
real-number formulas on the kernels' own operands, to float64 rounding:

    mean = mean_j x        (RMS: 0)          var = mean_j (x - mean)^2        rstd = 1 / sqrt(var + eps)
    xhat = (x - mean) * rstd                 y = xhat * gamma (+ beta)
    gd = gamma * dy    c1 = mean_j gd * xhat    c2 = mean_j gd   (RMS: 0)
    dx = rstd * (gd - xhat * c1 - c2) (+ dres)      dgamma = sum_r dy * xhat      dbeta = sum_r dy

Beside each result stands its *natural scale*, the sum of the absolute values of what was added up to make it: the
unit in which an fp32 evaluation's error is measured (an element that cancels to 0 still carries the rounding of its
terms). ``rel_err`` expresses an error in that unit.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

BF16 = torch.bfloat16


class Fwd(NamedTuple):
    y: torch.Tensor        # [rows, H]
    mean: torch.Tensor     # [rows] (zeros for RMS)
    rstd: torch.Tensor     # [rows]
    xhat: torch.Tensor     # [rows, H]
    y_scale: torch.Tensor  # |xhat * gamma| + |beta| + |mean| * rstd * |gamma|


class Bwd(NamedTuple):
    dx: torch.Tensor         # [rows, H]
    dgamma: torch.Tensor     # [H]
    dbeta: torch.Tensor      # [H] (sum_r dy also for RMS, where no kernel writes it)
    dx_scale: torch.Tensor   # |rstd gd| + |rstd xhat c1| + |rstd c2|
    dgamma_scale: torch.Tensor  # sum_r (|dy * xhat| + |dy| * |mean| * rstd)
    dbeta_scale: torch.Tensor   # sum_r |dy|
    c1: torch.Tensor         # [rows]
    c2: torch.Tensor         # [rows]
    gd: torch.Tensor         # [rows, H]


def _d(t):
    return None if t is None else t.detach().cpu().double()


def forward(x, gamma, beta=None, eps=1e-5, rms=False) -> Fwd:
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    mean = torch.zeros(x.shape[0], dtype=torch.float64) if rms else x.mean(1)
    xc = x - mean[:, None]
    var = (xc * xc).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = xc * rstd[:, None]
    y = xhat * gamma
    scale = y.abs() + (mean.abs() * rstd)[:, None] * gamma.abs()
    if beta is not None and not rms:
        y = y + beta
        scale = scale + beta.abs()
    return Fwd(y, mean, rstd, xhat, scale)


def backward(dy, x, gamma, mean, rstd, dres=None, rms=False) -> Bwd:
    """From the statistics given (float64 tensors: the reference's own, or the fp32 values a kernel was handed)."""
    dy, x, gamma, dres, mean, rstd = _d(dy), _d(x), _d(gamma), _d(dres), _d(mean), _d(rstd)
    if rms:
        mean = torch.zeros_like(rstd)
    xhat = (x - mean[:, None]) * rstd[:, None]
    gd = gamma * dy
    c1 = (gd * xhat).mean(1)
    c2 = torch.zeros_like(c1) if rms else gd.mean(1)
    t1, t2, t3 = rstd[:, None] * gd, rstd[:, None] * xhat * c1[:, None], (rstd * c2)[:, None].expand_as(gd)
    dx = t1 - t2 - t3
    if dres is not None:
        dx = dx + dres
    p = dy * xhat
    # dgamma's terms: dy x rstd and dy mean rstd, as y's (xhat alone cancels where x is close to the mean, and any fp32
    # evaluation from an fp32 mean is then off by the mean's rounding, which |dy xhat| does not carry)
    dg_scale = (p.abs() + dy.abs() * (mean.abs() * rstd)[:, None]).sum(0)
    return Bwd(dx, p.sum(0), dy.sum(0), t1.abs() + t2.abs() + t3.abs(), dg_scale, dy.abs().sum(0), c1, c2, gd)


def ulp32(v):
    """Spacing of fp32 at |v| (float64 in, float64 out)."""
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def ulp_bf16(v):
    """Spacing of bf16 at v (a float64 tensor of bf16 values); 0 at 0."""
    _, e = torch.frexp(v)
    ulp = torch.ldexp(torch.ones_like(v), (e - 8).clamp(min=-133))
    return torch.where(v == 0, torch.zeros_like(v), ulp)


def to_bf16(v):
    """float64 -> the nearest bf16, as float64."""
    return v.to(BF16).double()


def rel_err(got, ref, scale):
    """max |got - ref| / scale over the elements (0 / 0 counts as 0; a non-zero error on a zero scale as inf)."""
    err = (_d(got) - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / scale)
    return float(q.max()) if q.numel() else 0.0


# ---- input families -----------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def unit_rows(rows, H, seed):
    """randn rows: mean about 0, variance about 1."""
    return torch.randn(rows, H, generator=_gen(seed)).to(BF16)


def offset_rows(rows, H, seed, lo=48, hi=80):
    """Integers in [lo, hi] (at most 255): exact in bf16, every partial sum of a row exact in fp32 (< 2^24 up to
    H = 2^16). [48, 80]: mean about 64 against a spread of 9.5, so E[x^2] - mean^2 in fp32 cancels 4190 against 4100;
    [240, 255]: 61280 against 61260."""
    assert 0 <= lo <= hi <= 255
    return torch.randint(lo, hi + 1, (rows, H), generator=_gen(seed)).to(BF16)


def params(H, seed, beta=True):
    """gamma = 1 + 0.25 * noise, beta = noise (bf16)."""
    g = _gen(seed)
    gamma = (1.0 + 0.25 * torch.randn(H, generator=g)).to(BF16)
    b = torch.randn(H, generator=g).to(BF16)
    return gamma, (b if beta else None)


def correlated_dy(x, eps, seed, a=0.75, b=0.5, rms=False):
    """dy = a * xhat + b + noise: with gamma = 1 + 0.25 * noise, c1 is about a and c2 about b against
    rms(gd) of about sqrt(a^2 + b^2 + 1) * 1.03 = 1.39, so each term of dx that a wrong kernel could drop is at least
    a quarter of the gradient it is subtracted from."""
    xhat = forward(x, torch.ones(x.shape[1]), None, eps, rms).xhat
    noise = torch.randn(x.shape, generator=_gen(seed)).double()
    return (a * xhat + b + noise).to(BF16)


def plain_dy(rows, H, seed):
    return torch.randn(rows, H, generator=_gen(seed)).to(BF16)
