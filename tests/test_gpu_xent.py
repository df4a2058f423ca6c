"""Softmax cross-entropy on the gfx950 kernels (kernels/xent_bf16.hip) against a float64 CPU reference, row by row.

The contract, for bf16 logits x[rows, V] (row stride ld), int64 targets t, an upstream gradient g and the counted-row
total ``count``; a row is *counted* unless t == ignore_index, t < 0 or t >= V:

    lse[r]   = logsumexp(x[r])                                            (-inf logits add 0)
    loss[r]  = lse[r] - x[r, t[r]]            0 where the row is not counted, +inf where x[r, t[r]] = -inf
    dx[r, j] = (exp(x[r, j] - lse[r]) - [j == t[r]]) * g / count          +0 (by bits) where the row is not counted

and nothing outside [0, V) of the ``rows`` gradient rows, loss[0:rows] and lse[0:rows] is written; the logits and the
targets are only read. Two levels: the C entries (kfamd_xent_fwd_bf16 / kfamd_xent_bwd_bf16) on buffers, strides and
base offsets the test owns, so that every launch path runs and stray writes show against a sentinel; then
ops.cross_entropy through autograd for what the wrapper adds (reshape, count, empty_like, view).

Launch paths (the ids name them): the 16-B vector loop alone; the vector loop plus its element tail (ld % 8 == 0,
ld > V, V % 8 != 0); the element loop because the stride is off the 16-B grid; the element loop because the base is;
and, backward only, logits eligible for the vector loop with a gradient that is not, and the reverse.

Bounds.
  lse, loss: |kernel - float64| <= max(16 * FP32_LSE_ERR, 4 fp32 ulps of |lse|). FP32_LSE_ERR is the largest error
    of torch's own fp32 ``logsumexp`` on the device against the float64 reference over the inputs of this file (wide
    row included: torch is exact there, and its own bound is 4 ulps of 1e30); it measures the reference and fp32
    arithmetic, not the kernel. The factor 16 is for the kernel's fast exponential and its different reduction order.
    Every check prints its figures (``pytest -s``); see MEASURED below.
  dx, per element: |kernel - bf16(float64)| <= ulp_bf16(ref) + 2^-18 * |g / count|: one flipped rounding, plus the fp32
    error of exp(x - lse) for |x - lse| up to about 28, which is what is left at the target where p - 1 cancels.

The wide row holds one 1e30 (the target) among -1e30 and 0: with a single maximum, exp(x - lse) is the softmax also
in float64, where lse = 1e30 swallows log(count of maxima).

MEASURED (MI355X, all 47 row sets of this file): torch's fp32 logsumexp is off by at most 5.94e-7 (|lse| about 13;
0 on the wide row), so FP32_LSE_ERR = 5.94e-7 and the bound is max(9.5e-6, 4 ulps). The kernel's largest lse error
is 7.77e-7 and its largest loss error 9.56e-7 (both V = 50257, |lse| = 15.3); through ops.cross_entropy the mean loss
is off by at most 1.2e-6. No gradient element is outside its bound; the largest error is 7.6e-6, one bf16 rounding.
On the kernel as it was before -inf logits were handled, the masked rows give a NaN lse and loss on every path, and an
ignore_index inside the vocabulary gives -0 at that index: test_masked_*, test_op_masked_*, test_an_ignore_index_*
and test_op_uncounted_*[ignore5] fail there.
"""
from __future__ import annotations

from typing import NamedTuple

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
IGN = -100
EINVAL = -1
NEG = float("-inf")
BF16_SENTINEL = 0x7FA5      # a NaN: a kernel that read padding as logits would show it
F32_SENTINEL = 0x7FC5A5A5
GUARD = 4                   # loss / lse slots after ``rows``
FP32_LSE_ERR = 5.94e-7      # measured, see the module docstring


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _filled(n, dtype):
    t = torch.empty(n, dtype=dtype, device=DEV)
    _bits_view(t).fill_(BF16_SENTINEL if dtype == torch.bfloat16 else F32_SENTINEL)
    return t


def _bits_view(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the float64 reference --------------------------------------------------------------------------
def _reference(x, t, g, count, ignore=IGN):
    """x bf16 [rows, V], t int [rows] on the CPU -> loss, lse, dx (float64) and the counted-row mask."""
    xd, t = x.double(), t.to(torch.int64)
    rows, V = xd.shape
    lse = torch.logsumexp(xd, dim=1)
    counted = (t != ignore) & (t >= 0) & (t < V)
    at = xd.gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(counted, lse - at, torch.zeros_like(lse))
    onehot = torch.zeros_like(xd)
    onehot[counted.nonzero()[:, 0], t[counted]] = 1.0
    scale = counted.double() * (g / count if count > 0 else 0.0)
    dx = (torch.exp(xd - lse[:, None]) - onehot) * scale[:, None]
    return loss, lse, dx, counted


def _ulp32(v):
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _ulp_bf16(v):
    """Spacing of bf16 at v (a float64 tensor of bf16 values); 0 at 0."""
    _, e = torch.frexp(v)
    ulp = torch.ldexp(torch.ones_like(v), (e - 8).clamp(min=-133))
    return torch.where(v == 0, torch.zeros_like(v), ulp)


def _check_rows(name, x, loss, lse, ref_loss, ref_lse):
    """Per-row lse and loss (fp32, CPU) against float64; rows whose reference loss is +inf must be +inf."""
    fin = torch.isfinite(ref_loss)
    e32 = (torch.logsumexp(x.to(DEV).float(), dim=1).cpu().double() - ref_lse).abs()
    tol = torch.maximum(torch.full_like(ref_lse, 16 * FP32_LSE_ERR), 4 * _ulp32(ref_lse))
    e_lse = (lse.double() - ref_lse).abs()
    e_loss = (loss.double() - ref_loss).abs()[fin]
    print(f"XENT-FIG {name}: rows={x.shape[0]} max|lse|={ref_lse.abs().max().item():.4g} "
          f"fp32_torch_err={e32.max().item():.3e} kernel_lse_err={e_lse.max().item():.3e} "
          f"kernel_loss_err={(e_loss.max().item() if e_loss.numel() else 0.0):.3e} tol_min={tol.min().item():.3e}")
    assert bool(torch.isfinite(lse).all()), (name, lse)
    assert bool((e_lse <= tol).all()), (name, "lse", e_lse.tolist(), tol.tolist())
    assert bool((e_loss <= tol[fin]).all()), (name, "loss", e_loss.tolist(), tol[fin].tolist())
    assert bool((loss[~fin] == float("inf")).all()), (name, loss)
    return tol


def _check_grad(name, grad, ref_dx, counted, g, count):
    """Per-element gradient (bf16, CPU) against the float64 result rounded to bf16; uncounted rows +0 by bits."""
    ref = ref_dx.to(torch.bfloat16).double()
    scale = counted.double() * (abs(g / count) if count > 0 else 0.0)
    bound = _ulp_bf16(ref) + 2.0 ** -18 * scale[:, None]
    err = (grad.double() - ref).abs()
    worst = (err - bound).max().item()
    print(f"XENT-FIG {name}: grad max_err={err.max().item():.3e} max(err-bound)={worst:.3e}")
    assert bool(torch.isfinite(grad.float()).all()), name
    assert bool((err <= bound).all()), (name, "grad", err.max().item(), worst, (err > bound).nonzero()[:4].tolist())
    dead = _bits(grad)[~counted]
    assert bool((dead == 0).all()), (name, "an uncounted row's gradient is not +0 by bits")


# ---- the C entries ----------------------------------------------------------------------------------
class Case(NamedTuple):
    path: str
    V: int
    ld: int
    ldg: int
    xoff: int = 0   # elements between the 16-B aligned buffer and the first logit
    goff: int = 0
    rows: int = 0   # 0: the test's own row set

    @property
    def id(self):
        off = ("-xbase+%d" % self.xoff if self.xoff else "") + ("-gbase+%d" % self.goff if self.goff else "")
        return f"{self.path}-V{self.V}-ld{self.ld}-ldg{self.ldg}{off}"

    @property
    def fwd_vec(self):
        return self.xoff % 8 == 0 and self.ld % 8 == 0

    @property
    def bwd_vec(self):
        return self.fwd_vec and self.goff % 8 == 0 and self.ldg % 8 == 0


def _pad8(V):
    return -(-V // 8) * 8


CASES = (
    [Case("vector", V, V, V) for V in (8, 2048, 2056, 4096)]
    + [Case("vector+tail", V, _pad8(V), _pad8(V)) for V in (1, 7, 9, 255, 257, 1001, 2049, 2055)]
    + [Case("scalar-stride", 1000, 1001, 1001), Case("scalar-stride", 1001, 1001, 1001),
       Case("scalar-stride", 50257, 50257, 50257, rows=2)]
    + [Case("scalar-base", V, V, V, xoff=1, goff=1) for V in (1000, 2048)]
    + [Case("bwd-xvector-gscalar", 1000, 1000, 1001), Case("bwd-xscalar-gvector", 1000, 1001, 1000),
       Case("bwd-xvector-gscalar", 1000, 1000, 1000, goff=1), Case("bwd-xscalar-gvector", 1000, 1000, 1000, xoff=1)]
)


def test_the_ids_name_the_path_each_case_takes():
    for c in CASES:
        tail = c.V % 8 != 0
        want = {"vector": (True, True, False), "vector+tail": (True, True, True),
                "bwd-xvector-gscalar": (True, False, False), "bwd-xscalar-gvector": (False, False, False)}.get(c.path)
        if want is None:
            assert not c.fwd_vec and not c.bwd_vec and (c.xoff % 8 != 0) == (c.path == "scalar-base"), c.id
        else:
            assert (c.fwd_vec, c.bwd_vec, tail) == want, c.id
        assert c.ld >= c.V and c.ldg >= c.V
    # the reverse mixed case: the gradient alone would take the vector loop
    assert all(c.goff % 8 == 0 and c.ldg % 8 == 0 for c in CASES if c.path == "bwd-xscalar-gvector")


def _call(case, x, t, g, count, ignore=IGN):
    """Forward and backward through the C entries on sentinel-filled buffers laid out as ``case`` says; returns loss,
    lse (fp32) and the gradient rows (bf16) on the CPU after checking that nothing else was written."""
    from kubeflow_rm_amd.ops import _lib
    L = _lib.lib()
    rows, V = x.shape
    assert V == case.V
    xbuf = _filled(case.xoff + (rows + 1) * case.ld + 8, torch.bfloat16)
    gbuf = _filled(case.goff + (rows + 1) * case.ldg + 8, torch.bfloat16)
    assert xbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    xbuf[case.xoff:case.xoff + rows * case.ld].view(rows, case.ld)[:, :V].copy_(x)
    loss, lse = _filled(rows + GUARD, torch.float32), _filled(rows + GUARD, torch.float32)
    td = t.to(torch.int64).to(DEV)
    gd = torch.tensor([g], dtype=torch.float32, device=DEV)
    cd = torch.tensor([count], dtype=torch.float32, device=DEV)
    x0, g0 = _bits(xbuf).clone(), _bits(gbuf).clone()
    xp, gp = xbuf.data_ptr() + 2 * case.xoff, gbuf.data_ptr() + 2 * case.goff
    rc = L.kfamd_xent_fwd_bf16(xp, case.ld, td.data_ptr(), loss.data_ptr(), lse.data_ptr(), rows, V, ignore, _stream())
    assert rc == 0, rc
    rc = L.kfamd_xent_bwd_bf16(xp, case.ld, td.data_ptr(), lse.data_ptr(), gp, case.ldg, rows, V, ignore,
                               gd.data_ptr(), cd.data_ptr(), _stream())
    assert rc == 0, rc
    _sync()
    assert torch.equal(_bits(xbuf), x0), "the logits (or their padding) were written"
    assert torch.equal(td.cpu(), t.to(torch.int64)), "the targets were written"
    assert gd.item() == g and cd.item() == count
    for name, buf in (("loss", loss), ("lse", lse)):
        assert bool((_bits(buf)[rows:] == F32_SENTINEL).all()), f"{name} written beyond row {rows}"
    g1 = _bits(gbuf)
    keep = torch.ones_like(g1, dtype=torch.bool)
    keep[case.goff:case.goff + rows * case.ldg].view(rows, case.ldg)[:, :V] = False
    assert torch.equal(g1[keep], g0[keep]), "gradient bytes outside [0, V) of the rows were written"
    grad = gbuf[case.goff:case.goff + rows * case.ldg].view(rows, case.ldg)[:, :V].cpu().contiguous()
    return loss[:rows].cpu(), lse[:rows].cpu(), grad


def _probes(V):
    """0, 7, 8, the last element of the vector body, the first of the tail, V - 1, 2047, 2048: those below V."""
    body = V // 8 * 8
    return sorted({p for p in (0, 7, 8, body - 1, body, V - 1, 2047, 2048) if 0 <= p < V})


def _gen(case, salt):
    return torch.Generator().manual_seed(case.V * 131 + case.ld * 7 + case.xoff + salt)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_probe_rows_count_every_element_once(case):
    """Every logit is -60 except the probes at 0, so lse = log|S| to within V e^-60 and a dropped or doubled probe
    moves it by about 1/|S|; the target walks over the probes."""
    V, S = case.V, _probes(case.V)
    targets = S[-case.rows:] if case.rows else S
    x = torch.full((len(targets), V), -60.0, dtype=torch.bfloat16)
    x[:, S] = 0.0
    t = torch.tensor(targets)
    g, count = 0.75, float(len(targets))
    loss, lse, grad = _call(case, x, t, g, count)
    ref_loss, ref_lse, ref_dx, counted = _reference(x, t, g, count)
    assert bool((ref_lse - torch.log(torch.tensor(float(len(S)), dtype=torch.float64))).abs().max() < 1e-20)
    _check_rows(case.id, x, loss, lse, ref_loss, ref_lse)
    _check_grad(case.id, grad, ref_dx, counted, g, count)


def _wide_row(V, gen):
    """{-1e30, 0} at random with one 1e30, the target."""
    row = torch.where(torch.rand(V, generator=gen) < 0.5, torch.tensor(-1e30), torch.tensor(0.0))
    hot = V // 2
    row[hot] = 1e30
    return row.to(torch.bfloat16), hot


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_random_wide_and_uncounted_rows(case):
    """randn * 3 rows with the target on the last element, inside the tail, ignored, >= V, negative and anywhere,
    then the wide row; uncounted rows have loss 0 and a +0 gradient and are left out of count."""
    V, gen = case.V, _gen(case, 1)
    body = V // 8 * 8
    kinds = ["last", "any"] if case.rows else ["last", "tail", "ignore", "geV", "neg", "any", "wide"]
    x = (torch.randn(len(kinds), V, generator=gen) * 3).to(torch.bfloat16)
    t = torch.zeros(len(kinds), dtype=torch.int64)
    for r, kind in enumerate(kinds):
        if kind == "wide":
            x[r], t[r] = _wide_row(V, gen)
        else:
            t[r] = {"last": V - 1, "tail": body + (V - body) // 2 if body < V else V // 3, "ignore": IGN, "geV": V,
                    "neg": -5, "any": int(torch.randint(0, V, (1,), generator=gen))}[kind]
    ref_loss, ref_lse, ref_dx, counted = _reference(x, t, 0.75, 1.0)
    assert counted.tolist() == [k not in ("ignore", "geV", "neg") for k in kinds]
    g, count = 0.75, float(counted.sum())
    loss, lse, grad = _call(case, x, t, g, count)
    ref_loss, ref_lse, ref_dx, counted = _reference(x, t, g, count)
    _check_rows(case.id, x, loss, lse, ref_loss, ref_lse)
    _check_grad(case.id, grad, ref_dx, counted, g, count)
    assert bool((_bits(loss)[~counted] == 0).all()), "an uncounted row's loss is not 0"


def test_an_ignore_index_inside_the_vocabulary_and_a_zero_count():
    """ignore_index = 5 (a pad token): the row's gradient is +0 at index 5 too; count = 0 zeroes every row."""
    case = Case("vector+tail", 1001, 1008, 1008)
    x = (torch.randn(3, 1001, generator=_gen(case, 2)) * 3).to(torch.bfloat16)
    t = torch.tensor([5, 7, 5])
    loss, lse, grad = _call(case, x, t, 0.75, 1.0, ignore=5)
    ref_loss, ref_lse, ref_dx, counted = _reference(x, t, 0.75, 1.0, ignore=5)
    assert counted.tolist() == [False, True, False]
    _check_rows(case.id, x, loss, lse, ref_loss, ref_lse)
    _check_grad(case.id, grad, ref_dx, counted, 0.75, 1.0)
    assert bool((_bits(loss)[~counted] == 0).all())
    loss, lse, grad = _call(case, x, t, 0.75, 0.0)
    assert bool((_bits(grad) == 0).all())


# ---- masked (-inf) logits ---------------------------------------------------------------------------
MASKED = [Case("scalar-stride", 1001, 1001, 1001), Case("vector", 4096, 4096, 4096),
          Case("vector+tail", 2055, 2056, 2056), Case("scalar-stride", 50257, 50257, 50257, rows=2)]
LANE = 3  # the thread whose visits are masked


def _visits(case):
    """What thread LANE of the 256 reads from a row, in order, as index lists: 8-element vectors, then elements."""
    V = case.V
    nv = V // 8 if case.fwd_vec else 0
    return ([list(range(8 * i, 8 * i + 8)) for i in range(LANE, nv, 256)]
            + [[j] for j in range(nv * 8 + LANE, V, 256)])


def _masked_rows(case, kinds):
    V = case.V
    x = (torch.randn(len(kinds), V, generator=_gen(case, 3)) * 3).to(torch.bfloat16)
    t = torch.full((len(kinds),), V - 1, dtype=torch.int64)
    visits = _visits(case)
    assert len(visits) >= 2 and V - 1 not in sum(visits, [])
    for r, kind in enumerate(kinds):
        if kind == "first":
            x[r, 0] = NEG
        elif kind == "first8":
            x[r, 0:8] = NEG
        elif kind == "before-first-finite":   # everything the thread reads before its last visit
            x[r, sum(visits[:-1], [])] = NEG
        elif kind == "whole-thread":          # the thread never sees a finite value
            x[r, sum(visits, [])] = NEG
        elif kind == "all-but-one":
            x[r] = NEG
            x[r, V // 2], t[r] = 1.5, V // 2
        elif kind == "target":                # loss +inf, as in torch
            x[r, 5], t[r] = NEG, 5
    return x, t


@pytest.mark.parametrize("case", MASKED, ids=lambda c: c.id)
def test_masked_logits_stay_finite_and_match(case):
    """-inf logits: at the row's first element, over its first vector, at everything one thread reads before its first
    finite value (vectors LANE, LANE + 256 / elements LANE, LANE + 256, ...), at everything it reads, everywhere but
    one element, and on the target (loss +inf, finite gradient)."""
    kinds = ["first", "before-first-finite"] if case.rows else \
        ["first", "first8", "before-first-finite", "whole-thread", "all-but-one", "target"]
    x, t = _masked_rows(case, kinds)
    g, count = 0.75, float(len(kinds))
    loss, lse, grad = _call(case, x, t, g, count)
    ref_loss, ref_lse, ref_dx, counted = _reference(x, t, g, count)
    assert bool(torch.isfinite(ref_lse).all()) and bool(torch.isfinite(ref_dx).all())
    assert torch.isinf(ref_loss).tolist() == [k == "target" for k in kinds]
    _check_rows(case.id, x, loss, lse, ref_loss, ref_lse)
    _check_grad(case.id, grad, ref_dx, counted, g, count)
    masked = torch.isinf(x)
    masked[torch.arange(len(kinds)), t] = False  # a masked target's gradient is -g / count
    assert bool((_bits(grad)[masked] == 0).all()), "a masked logit has a non-zero gradient"


# ---- ops.cross_entropy through autograd -------------------------------------------------------------
def _torch_reference(x, t, ignore):
    """F.cross_entropy in float64 with every uncounted target mapped to ignore_index."""
    V = x.shape[-1]
    t = t.to(torch.int64)
    mapped = torch.where((t < 0) | (t >= V), torch.full_like(t, ignore), t)
    return torch.nn.functional.cross_entropy(x.double().reshape(-1, V), mapped.reshape(-1), ignore_index=ignore)


def _through_op(name, x, t, upstream=1.0, ignore=IGN, leaf=None, narrow=None):
    """ops.cross_entropy(x, t) and its backward on the device against the float64 reference; ``leaf`` / ``narrow``:
    x is leaf[..., :narrow] and the gradient is taken at the leaf. Returns the leaf's gradient on the CPU."""
    from kubeflow_rm_amd import ops
    V = x.shape[-1]
    xd = (x if leaf is None else leaf).to(DEV).requires_grad_(True)
    loss = ops.cross_entropy(xd if leaf is None else xd[..., :narrow], t.to(DEV), ignore_index=ignore)
    loss.backward(torch.tensor(upstream, dtype=loss.dtype, device=DEV))
    _sync()
    assert loss.dtype == torch.float32 and xd.grad.shape == xd.shape and xd.grad.dtype == torch.bfloat16
    x2, t2 = x.reshape(-1, V), t.reshape(-1)
    count = float(((t2 != ignore) & (t2 >= 0) & (t2 < V)).sum())
    ref_loss, ref_lse, ref_dx, counted = _reference(x2, t2, upstream, count, ignore)
    grad = xd.grad.cpu()
    g2 = (grad if leaf is None else grad[..., :narrow]).reshape(-1, V)
    if count == 0:
        assert bool(torch.isnan(loss).item()), loss  # 0 / 0, as F.cross_entropy
    else:
        ref = ref_loss.sum() / count
        want = _torch_reference(x, t, ignore)
        assert ref == want or abs(ref - want) <= 1e-12 * abs(want), (ref, want)  # the reference against torch's own
        if torch.isfinite(ref):
            # the rows' own bound, then an fp32 sum of the rows and one division
            tol = torch.maximum(torch.full_like(ref_lse, 16 * FP32_LSE_ERR), 4 * _ulp32(ref_lse))
            tol = tol[counted].sum() / count + (x2.shape[0] + 1) * 2.0 ** -24 * abs(ref)
            err = abs(loss.double().item() - ref.item())
            print(f"XENT-FIG {name}: mean loss {ref.item():.6f} err={err:.3e} tol={tol.item():.3e}")
            assert err <= tol.item(), (name, loss.item(), ref.item(), tol.item())
        else:
            assert loss.item() == ref.item(), (loss, ref)
    _check_grad(name, g2, ref_dx, counted, upstream, count)
    return grad


def test_op_3d_logits_int32_targets_and_an_upstream_gradient():
    B, T, V = 2, 3, 1001
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(B, T, V, generator=gen) * 3).to(torch.bfloat16)
    t = torch.randint(0, V, (B, T), generator=gen).to(torch.int32)
    t[0, 1], t[1, 2] = IGN, V - 1
    _through_op("op-3d-int32", x, t, upstream=0.375)


@pytest.mark.parametrize("ignore", [IGN, 5], ids=["ignore-100", "ignore5"])
def test_op_uncounted_rows_are_left_out_of_count(ignore):
    """Targets >= V and negative targets that are not ignore_index count as ignored, as the kernel treats them."""
    V = 1000
    x = (torch.randn(7, V, generator=torch.Generator().manual_seed(12)) * 3).to(torch.bfloat16)
    t = torch.tensor([5, ignore, V, V + 7, -3, V - 1, 17])
    grad = _through_op(f"op-uncounted-{ignore}", x, t, upstream=1.0, ignore=ignore)
    dead = (t == ignore) | (t < 0) | (t >= V)
    assert int(dead.sum()) in (4, 5) and bool((_bits(grad)[dead] == 0).all())


def test_op_all_rows_ignored_is_nan_with_a_zero_gradient():
    V = 1000
    x = (torch.randn(4, V, generator=torch.Generator().manual_seed(13)) * 3).to(torch.bfloat16)
    grad = _through_op("op-all-ignored", x, torch.tensor([IGN, V, -1, IGN]))
    assert bool((_bits(grad) == 0).all())


@pytest.mark.parametrize("rows,V,padded", [(4, 1001, 1008), (2, 50257, 50304)], ids=["1001of1008", "50257of50304"])
def test_op_padded_vocabulary_slice(rows, V, padded):
    """The loss on full[:, :V] of a padded head: the logits keep their stride, the gradient buffer is dense, and the
    padding's gradient is exactly zero."""
    gen = torch.Generator().manual_seed(V)
    full = (torch.randn(rows, padded, generator=gen) * 3).to(torch.bfloat16)
    t = torch.randint(0, V, (rows,), generator=gen)
    t[0] = V - 1
    grad = _through_op(f"op-slice-{V}of{padded}", full[:, :V], t, upstream=0.5, leaf=full, narrow=V)
    assert grad.shape == (rows, padded) and bool((_bits(grad)[:, V:] == 0).all())


def test_op_masked_logits_match_torch():
    case = MASKED[0]
    kinds = ["first", "first8", "before-first-finite", "whole-thread", "all-but-one"]
    x, t = _masked_rows(case, kinds)
    _through_op("op-masked", x, t)
    x, t = _masked_rows(case, kinds + ["target"])  # +inf, as F.cross_entropy (checked in _through_op)
    _through_op("op-masked-target", x, t)


# ---- argument checks --------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_before_any_launch():
    from kubeflow_rm_amd.ops import _lib
    L = _lib.lib()
    rows, V = 2, 16
    x, grad = _filled(rows * V, torch.bfloat16), _filled(rows * V, torch.bfloat16)
    loss, lse = _filled(rows, torch.float32), _filled(rows, torch.float32)
    t = torch.zeros(rows, dtype=torch.int64, device=DEV)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    s = _stream()

    def fwd(xp=x.data_ptr(), ld=V, tp=t.data_ptr(), lp=loss.data_ptr(), sp=lse.data_ptr(), r=rows, v=V):
        return L.kfamd_xent_fwd_bf16(xp, ld, tp, lp, sp, r, v, IGN, s)

    def bwd(xp=x.data_ptr(), ld=V, tp=t.data_ptr(), sp=lse.data_ptr(), gp=grad.data_ptr(), ldg=V, r=rows, v=V,
            up=one.data_ptr(), cp=one.data_ptr()):
        return L.kfamd_xent_bwd_bf16(xp, ld, tp, sp, gp, ldg, r, v, IGN, up, cp, s)

    bad = [fwd(ld=V - 1), fwd(r=0), fwd(r=-1), fwd(v=0), fwd(xp=None), fwd(tp=None), fwd(lp=None), fwd(sp=None),
           bwd(ld=V - 1), bwd(ldg=V - 1), bwd(r=0), bwd(r=-1), bwd(v=0), bwd(xp=None), bwd(tp=None), bwd(sp=None),
           bwd(gp=None), bwd(up=None), bwd(cp=None)]
    assert bad == [EINVAL] * len(bad), bad
    _sync()
    for buf in (x, grad):
        assert bool((_bits(buf) == BF16_SENTINEL).all())
    for buf in (loss, lse):
        assert bool((_bits(buf) == F32_SENTINEL).all())
