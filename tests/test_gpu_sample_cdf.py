"""The fused sampler (kernels/sample_bf16.hip) token by token: its whole kept set and its whole CDF at 2^-24
resolution, recovered by bisection over u (tests/sample_cdf.py), on rows built to put the cuts where the kernel's
integer logic works hardest.

Families A (all-equal rows), B (a plateau over a floor) and C (V = 2^20) are made of tie groups: equal keys weigh
the same integer, so the expected step function is exact whatever the kernel's exp2 returns, and every assertion is
``==``. D (a staircase on the key-bin edges) and E (random rows with natural ties) have unequal weights: the token
set is still exact, the boundaries are held to TOL = 2^-15 of the kept mass, which follows from the accuracy the
kernel's header states (sample_cdf.TOL) and not from what the kernel returns.

Measured on an MI355X: the largest |first_q - reference| / 2^24 over D and E is 6.97e-8 of W = 2^-23.8, 1.2 grid
steps (random row 0 at V = 1025, plain), against TOL = 3.05e-5; the staircase's worst is 6.15e-8. Every test prints
its own figure before it asserts. The whole file takes 2.2 s.
"""
from __future__ import annotations

import pytest
import torch

from tests import sample_cdf as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
Q = sc.Q
TOL = sc.TOL
_worst = {"dev": 0.0}


def _steps(x, temperature, k, p):
    return sc.step_function(x, temperature, k, p, DEV)


def _within_tol(got, ref_q, what):
    dev = sc.max_deviation(got, ref_q)
    _worst["dev"] = max(_worst["dev"], dev)
    print(f"{what}: boundary deviation {dev:.3e} of W (TOL {TOL:.3e}); worst so far {_worst['dev']:.3e}")
    assert dev <= TOL, f"{what}: a boundary is {dev:.3e} of W away from the fp64 reference (TOL {TOL:.3e})"


# ---- A: all-equal rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.EQUAL_KINDS)
@pytest.mark.parametrize("V", sc.EQUAL_V)
def test_all_equal_rows(V, kind):
    """The kept tokens are the lowest n indices, n = min(k, V), then ceil(p * n), and token i starts at exactly
    ceil(i * 2^24 / n). The +0 / -0 row is one tie group."""
    x = sc.equal_row(V, kind)
    for k, p, n in sc.equal_settings(V):
        assert _steps(x, 1.0, k, p) == sc.equal_steps(range(V), n), f"top_k={k} top_p={p}: {n} tokens expected"


# ---- B: a plateau over a floor ---------------------------------------------------------------------------
@pytest.mark.parametrize("floor", sc.PLATEAU_FLOORS)
@pytest.mark.parametrize("V", sc.PLATEAU_V)
def test_plateau_over_a_floor(V, floor):
    """The plateau's lowest n indices, each 2^40 heavy, whether the cut falls inside the plateau, exactly at its
    end or inside the zero-weight floor (whose tokens are kept and must never be drawn)."""
    x = sc.plateau_row(V, floor)
    idx = sc.plateau_indices(V)
    for k, p, n in sc.plateau_settings(V):
        got = _steps(x, 1.0, k, p)
        assert got == sc.equal_steps(idx, n), f"top_k={k} top_p={p}: {n} plateau tokens expected"
        assert got[idx[0]] == 0 and max(got) == idx[n - 1]  # u = 0 and u = 1 - 2^-24


# ---- C: the greatest V -----------------------------------------------------------------------------------
@pytest.mark.parametrize("V", sc.BIG_V)
def test_greatest_v(V):
    """All-equal rows at the contract's limit (seg = 65536, the mass V * 2^40 = 2^60): token == floor(n * q / 2^24)
    at tokens 0, n - 1 and both sides of three wave-segment edges, plain and under top_k = V / 2 + 1."""
    from kubeflow_rm_amd import ops
    x = torch.full((8, V), 1.5, dtype=sc.BF16, device=DEV)
    for k, n in ((None, V), (V // 2 + 1, V // 2 + 1)):
        pairs = sc.big_queries(n)
        u = (torch.tensor([q for q, _ in pairs], dtype=torch.float64) / Q).float().to(DEV)
        out = torch.full((8,), -1, dtype=torch.int64, device=DEV)
        ops.sample(x, u, 1.0, k, None, out=out)
        assert out.tolist() == [t for _, t in pairs], f"top_k={k}"


# ---- D: a staircase on the bin edges ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def staircase():
    return sc.staircase_row()


def test_staircase_top_k_sweep(staircase):
    """Every top_k from 2 to past the last finite token: the token set is the reference kept set of non-zero
    weight (the order and the tie admission at every bin edge; +0 / -0 one group), the boundaries within TOL."""
    x, count = staircase
    for k in range(2, count + 3):
        got = _steps(x, 1.0, k, None)
        _, ref_q = sc.reference(x, 1.0, k, None)
        assert set(got) == set(ref_q), f"top_k={k}: {sorted(set(got) ^ set(ref_q))} differ"
        _within_tol(got, ref_q, f"staircase top_k={k}")


@pytest.mark.parametrize("case", sc.STAIR_TOP_P, ids=lambda c: f"k{c[0]}-{c[1]:04x}-{c[3]}")
def test_staircase_top_p(staircase, case):
    """top_p ending inside a chosen tie group, alone and over a top-k cut in a lower, the same, and the very
    bin. The fp64 count of members needed is at least 0.1 away from an integer, and by more than TOL * Z in mass, so
    the expected count does not hinge on rounding."""
    x, _ = staircase
    k, bits, members, relation = case
    p = sc.top_p_into(x, 1.0, k, bits, members)
    assert sc.classify(x, k, p).relation == relation
    c = sc.cut_of(x, 1.0, k, p)
    frac = c.needed % 1.0
    assert 0.1 <= frac <= 0.9 and min(frac, 1 - frac) * c.w_cp > TOL * c.Z, (c.needed, c.w_cp, c.Z)
    got = _steps(x, 1.0, k, p)
    _, ref_q = sc.reference(x, 1.0, k, p)
    assert set(got) == set(ref_q), f"{sorted(set(got) ^ set(ref_q))} differ"
    _within_tol(got, ref_q, f"staircase top_k={k} top_p={p}")


# ---- E: random rows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", sc.PLATEAU_V)
def test_random_rows(V):
    """randn * 4 rows at temperature 0.8 under the four settings of tests/test_gpu_sample.py. The top-p cut is
    unambiguous at TOL; the top-k cut is left as it falls, and at least one row has a tie group across it."""
    rows = sc.random_rows(V, sc.RANDOM_SEEDS[V])
    assert any(sc.straddles_top_k(x, 40) for x in rows)
    for b, x in enumerate(rows):
        for name, (k, p) in sc.RANDOM_SETTINGS.items():
            got = _steps(x, sc.RANDOM_T, k, p)
            wk, ref_q = sc.reference(x, sc.RANDOM_T, k, p)
            assert set(got) <= set((wk > 0).nonzero().flatten().tolist()), f"row {b} {name}: outside the kept set"
            missing = [t for t in ref_q if wk[t] >= 2.0 ** -20 * wk.sum() and t not in got]
            assert not missing, f"row {b} {name}: kept tokens {missing[:8]} are never drawn"
            assert set(got) <= set(ref_q)
            _within_tol(got, ref_q, f"random V={V} row {b} {name}")
