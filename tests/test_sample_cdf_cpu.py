"""tests/sample_cdf.py against ops.sample's torch form: the bisection, the exact identities, the row builders and
the branch coverage of the case tables that tests/test_gpu_sample_cdf.py runs on the kernel."""
from __future__ import annotations

import math

import pytest
import torch

from tests import sample_cdf as sc

Q = sc.Q


@pytest.mark.parametrize("V", [1, 2, 9, 1025])
def test_all_equal_identity(V):
    """first_q[i] = ceil(i * 2^24 / n) over the lowest n indices, under plain, top-k, top-p and both."""
    for kind in ("1.5", "zeros"):
        x = sc.equal_row(V, kind)
        for k, p, n in ((None, None, V), (max(1, V // 2), None, max(1, V // 2)), (None, 0.3125, math.ceil(0.3125 * V)),
                        (V + 9, 0.75, math.ceil(0.75 * V)), (max(1, V - 1), 0.5, math.ceil(0.5 * max(1, V - 1)))):
            got = sc.step_function(x, 1.0, k, p)
            assert got == sc.equal_steps(range(V), n), (kind, k, p)
            assert got == {i: math.ceil(i * Q / n) for i in range(n)}


def test_equal_settings_cover_the_issue():
    sets = sc.equal_settings(1025)
    assert {k for k, p, _ in sets if p is None} == {None, 2, 63, 64, 65, 1024, 1025, 1034}
    assert (65, 0.75, 49) in sets and (None, 0.3125, 321) in sets and (1034, None, 1025) in sets
    assert all(1 <= n <= 1 for _, _, n in sc.equal_settings(1))


def test_bisection_rejects_a_decreasing_token(monkeypatch):
    """A sampler whose token falls with q fails inside step_function."""
    from kubeflow_rm_amd import ops
    real = ops.sample

    def backwards(rows, u, *a, **kw):
        kw.pop("out", None)
        return rows.shape[1] - 1 - real(rows, u, *a, **kw)

    monkeypatch.setattr(ops, "sample", backwards)
    with pytest.raises(AssertionError):
        sc.step_function(sc.equal_row(9, "1.5"), 1.0, None, None)


@pytest.mark.parametrize("floor", sc.PLATEAU_FLOORS)
def test_plateau_family(floor):
    V = 257
    x = sc.plateau_row(V, floor)
    idx = sc.plateau_indices(V)
    for k, p, n in sc.plateau_settings(V):
        got = sc.step_function(x, 1.0, k, p)
        _, ref_q = sc.reference(x, 1.0, k, p)
        assert set(got) == set(ref_q), (k, p)
        assert set(got) <= set(idx)
        assert sc.max_deviation(got, ref_q) <= 2.0 ** -24
        if floor == "-inf":  # exact masses in fp64 too: the expectation the kernel is held to
            assert got == sc.equal_steps(idx, n), (k, p)
        assert got[idx[0]] == 0 and max(got) == max(ref_q)


def test_staircase_family():
    V = 300
    x, count = sc.staircase_row(V)
    assert count == 25 and int((x != float("-inf")).sum()) == 25
    for k in range(2, count + 3):
        got = sc.step_function(x, 1.0, k, None)
        _, ref_q = sc.reference(x, 1.0, k, None)
        assert set(got) == set(ref_q) and len(got) == min(k, count), k
        assert sc.max_deviation(got, ref_q) <= 2.0 ** -24
    for k, bits, members, relation in sc.STAIR_TOP_P:
        p = sc.top_p_into(x, 1.0, k, bits, members)
        assert sc.classify(x, k, p).relation == relation
        got = sc.step_function(x, 1.0, k, p)
        _, ref_q = sc.reference(x, 1.0, k, p)
        assert set(got) == set(ref_q), (k, hex(bits))
        assert sc.max_deviation(got, ref_q) <= 2.0 ** -24


def test_staircase_places_each_value_in_different_waves():
    x, _ = sc.staircase_row()
    keys, s = sc.keys_of(x), sc.seg(sc.STAIR_V)
    assert s == 320
    for b in sc.STAIR_BITS:
        idx = (keys == sc.keys_of(sc.from_bits([b]))[0]).nonzero()[0]
        assert len(set((idx // s).tolist())) == idx.size
    zeros = (keys == 0x8000).nonzero()[0]
    assert zeros.size == 5  # +0 and -0: one group


def test_random_family():
    V = 257
    for x in sc.random_rows(V, sc.RANDOM_SEEDS[V]):
        for k, p in sc.RANDOM_SETTINGS.values():
            got = sc.step_function(x, sc.RANDOM_T, k, p)
            wk, ref_q = sc.reference(x, sc.RANDOM_T, k, p)
            assert set(got) <= set(ref_q)
            assert all(t in got for t in ref_q if wk[t] >= 2.0 ** -20 * wk.sum())
            assert sc.max_deviation(got, ref_q) <= 2.0 ** -24


@pytest.mark.parametrize("V", sc.PLATEAU_V)
def test_random_seeds_put_a_tie_group_across_the_top_k_cut(V):
    rows = sc.random_rows(V, sc.RANDOM_SEEDS[V])
    assert any(sc.straddles_top_k(x, 40) for x in rows)


def test_key_map():
    x = sc.from_bits([0x0000, 0x8000, 0x0080, 0x8080, 0x3F80, 0xBF80, 0x7F80, 0xFF80])
    assert sc.keys_of(x).tolist() == [0x8000, 0x8000, 0x8080, 0x7F7F, 0xBF80, 0x407F, 0xFF80, 0x007F]
    v = torch.randn(4096, generator=torch.Generator().manual_seed(0)).mul(4).to(sc.BF16)
    order = sorted(range(4096), key=lambda i: (-float(v[i]), i))
    keys = sc.keys_of(v)
    assert order == sorted(range(4096), key=lambda i: (-int(keys[i]), i))
    assert [sc.seg(V) for V in (1, 1024, 1025, 4097, 1 << 20, (1 << 20) - 65)] == [64, 64, 128, 320, 65536, 65536]


def test_case_tables_reach_every_branch():
    """Over the cases the GPU file runs: each of the four relations of the top-p cut to the top-k cut, and cut tie
    groups that span steps of one wave and that span waves, so that an edit cannot quietly lose a branch."""
    seen, steps, waves = {}, set(), set()

    def note(family, x, k, p, temperature=1.0):
        b = sc.classify(x, k, p, temperature)
        seen.setdefault(b.relation, set()).add(family)
        if b.spans_steps:
            steps.add(family)
        if b.spans_waves:
            waves.add(family)
        return b

    for V in sc.EQUAL_V:
        for kind in sc.EQUAL_KINDS:
            for k, p, _ in sc.equal_settings(V):
                note("A", sc.equal_row(V, kind), k, p)
    for V in sc.PLATEAU_V:
        for floor in sc.PLATEAU_FLOORS:
            for k, p, _ in sc.plateau_settings(V):
                note("B", sc.plateau_row(V, floor), k, p)
    x, count = sc.staircase_row()
    for k in range(2, count + 3):
        note("D", x, k, None)
    for k, bits, members, relation in sc.STAIR_TOP_P:
        assert note("D", x, k, sc.top_p_into(x, 1.0, k, bits, members)).relation == relation
    for V in sc.PLATEAU_V:
        for row in sc.random_rows(V, sc.RANDOM_SEEDS[V]):
            for k, p in sc.RANDOM_SETTINGS.values():
                note("E", row, k, p, sc.RANDOM_T)
    for relation in ("no-k", "Hp>Hk", "Hp==Hk, cp>ck", "cp==ck"):
        assert seen.get(relation), f"no case reaches {relation}"
    # the exact families reach them all but Hp == Hk with cp > ck (two values in one bin); the staircase all four
    assert {"A", "B"} <= seen["no-k"] and "B" in seen["Hp>Hk"] and {"A", "B"} <= seen["cp==ck"]
    assert all("D" in seen[r] for r in ("no-k", "Hp>Hk", "Hp==Hk, cp>ck", "cp==ck"))
    assert {"A", "B"} <= steps and {"A", "B", "D"} <= waves
    # the plateau's floor as the cut tie group: every wave
    b = sc.classify(sc.plateau_row(4097, "-inf"), len(sc.plateau_indices(4097)) + 5, None)
    assert b.spans_steps and b.spans_waves and b.Hk == 0x00
