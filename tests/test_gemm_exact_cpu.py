"""The bit-exact GEMM scheme of tests/exact.py, proved on the CPU: integer operands make every fp32
accumulation order give the fp64 result, three small kernel faults emulated in torch each change the output's
bits, and the same faults on the tolerance tests' uniform(-1, 1) operands fall inside ``_assert_close``'s own
bound (tests/test_gpu_kernels.py)."""
import pytest
import torch

from tests import exact
from tests.exact import BF16, assert_bits_equal, exact_ref, int_operand, mismatch_report
from tests.test_gpu_kernels import _assert_close, _ref_gemm

TABLED = [(1000, 1000, 1001), (512, 512, 4096), (512, 768, 1024)]


def _ints(*shape, seed, **kw):
    return int_operand(*shape, seed=seed, device="cpu", **kw)


def _rand(*shape, seed):
    """The tolerance tests' operand distribution (their ``_rand``), drawn on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(BF16)


# ---- the three faults, on fp32 operands a [M, K], b [N, K]; each returns the bf16 a faulty kernel would store ----

def _fault_last_k(af, bf, bias):
    """The last k element dropped everywhere (a K tail masked one element short)."""
    c = af[:, :-1] @ bf[:, :-1].t()
    return (c + bias if bias is not None else c).to(BF16)


def _fault_bf16_partial(af, bf, bias):
    """One of two K halves rounded to bf16 before the sum (a split's partial kept in bf16)."""
    h = af.shape[1] // 2
    c = (af[:, :h] @ bf[:, :h].t()).to(BF16).to(af.dtype) + af[:, h:] @ bf[:, h:].t()
    return (c + bias if bias is not None else c).to(BF16)


def _fault_no_bias(af, bf, bias):
    return (af @ bf.t()).to(BF16)


FAULTS = {"last_k": _fault_last_k, "bf16_partial": _fault_bf16_partial, "no_bias": _fault_no_bias}


def test_int_operand_is_seeded_integer_and_exact():
    a = _ints(5, 33, 70, seed=3)
    assert a.dtype == BF16 and a.shape == (5, 33, 70) and torch.equal(a, _ints(5, 33, 70, seed=3))
    assert not torch.equal(a, _ints(5, 33, 70, seed=4))
    assert sorted(a.float().unique().tolist()) == [-3, -2, -1, 0, 1, 2, 3]
    r = _ints(64, 64, seed=1, lo=-8, hi=8)
    assert r.float().min().item() == -8 and r.float().max().item() == 8 and torch.equal(r.float(), r.float().round())
    qw = _ints(96, 64, seed=5, dtype=exact.FP8)
    assert qw.codes.dtype == exact.FP8 and qw.codes.shape == (96, 64) and qw.scale.dtype == torch.float32
    assert sorted(qw.codes.float().unique().tolist()) == [-3, -2, -1, 0, 1, 2, 3]
    assert set(qw.scale.tolist()) == set(exact.W8_SCALES)  # more than one scale: a misplaced one would show
    assert torch.equal(qw.dequantize(), qw.codes.float() * qw.scale[:, None])


def test_integer_sums_are_exact_in_fp32_in_any_order():
    """At 256 x 384 x 8192: the fp32 product equals fp64 as computed, with K permuted, and accumulated in 64-wide
    chunks (a tiled kernel's order); every partial sum is bounded by 9 K < 2^24; a good share of the outputs is
    not representable in bf16 and some are exact ties, so the one rounding and its tie rule are exercised."""
    M, N, K = 256, 384, 8192
    a, b = _ints(M, K, seed=11), _ints(N, K, seed=12)
    c64 = a.double() @ b.double().t()
    af, bf = a.float(), b.float()
    assert torch.equal((af @ bf.t()).double(), c64)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(13))
    assert torch.equal((af[:, perm] @ bf[:, perm].t()).double(), c64)
    acc = torch.zeros(M, N)
    for k0 in reversed(range(0, K, 64)):
        acc += af[:, k0:k0 + 64] @ bf[:, k0:k0 + 64].t()
    assert torch.equal(acc.double(), c64)
    assert c64.abs().max().item() <= 9 * K < 2 ** 24
    ref = exact_ref(a, b, trans_b=True)
    inexact = ref.double() != c64
    assert inexact.float().mean().item() > 0.1
    mid = (c64.abs() >= 256) & (c64.abs() < 512)  # bf16 spacing 2: every odd integer is a tie
    ties = mid & (c64.abs() % 2 == 1)
    assert ties.sum().item() > 100
    assert torch.equal(ref.double()[ties].abs() % 4, torch.zeros(int(ties.sum().item()), dtype=torch.float64))  # to even
    assert (ref.double() - c64)[~inexact].abs().max().item() == 0


def test_exact_ref_epilogue_and_layouts():
    a, b = _ints(40, 72, seed=21), _ints(56, 72, seed=22)
    bias, res = _ints(56, seed=23, lo=-8, hi=8), _ints(40, 56, seed=24, lo=-8, hi=8)
    want = (torch.relu(0.5 * (a.double() @ b.double().t()) + bias.double())).float()
    assert_bits_equal(exact_ref(a, b, trans_b=True, bias=bias, alpha=0.5, relu=True), want.to(BF16))
    want = (0.5 * (a.double() @ b.double().t()) + bias.double() + res.double()).float().to(BF16)
    assert_bits_equal(exact_ref(a, b, trans_b=True, bias=bias, residual=res, alpha=0.5), want)
    at, bt = a.t().contiguous(), b.t().contiguous()
    plain = exact_ref(a, b, trans_b=True)
    for ta, tb, x, y in ((False, False, a, bt), (True, False, at, bt), (True, True, at, b)):
        assert_bits_equal(exact_ref(x, y, trans_a=ta, trans_b=tb), plain)
    qw = _ints(56, 64, seed=25, dtype=exact.FP8)
    a2 = _ints(3, 64, seed=26)
    want = (0.5 * (a2.double() @ qw.dequantize().double().t()) + bias.double()).float().to(BF16)
    assert_bits_equal(exact_ref(a2, qw, trans_b=True, bias=bias, alpha=0.5), want)


def test_exact_ref_refuses_to_leave_the_exact_regime():
    a, b = _ints(8, 64, seed=31), _ints(8, 64, seed=32)
    with pytest.raises(AssertionError, match="integer"):
        exact_ref(a * 0.5, b, trans_b=True)
    with pytest.raises(AssertionError, match="power of two"):
        exact_ref(a, b, trans_b=True, alpha=0.3)
    with pytest.raises(AssertionError, match="integer"):
        exact_ref(a, b, trans_b=True, bias=torch.full((8,), 0.5))
    with pytest.raises(AssertionError, match="2\\^24"):  # 4096 * 4096 * 64 = 2^30: partial sums past fp32's integers
        exact_ref(a * 4096, b * 4096, trans_b=True)
    with pytest.raises(AssertionError, match="2\\^24"):
        exact.exact_colsum(torch.full((2 ** 12, 4), float(2 ** 12), dtype=torch.float64))


@pytest.mark.parametrize("M,N,K", TABLED)
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_each_fault_changes_the_bits_on_integer_operands(fault, M, N, K):
    a, b, bias = _ints(M, K, seed=41), _ints(N, K, seed=42), _ints(N, seed=43, lo=-8, hi=8)
    ref = exact_ref(a, b, trans_b=True, bias=bias)
    assert_bits_equal((a.float() @ b.float().t() + bias.float()).to(BF16), ref)  # the sound fp32 kernel passes
    out = FAULTS[fault](a.float(), b.float(), bias.float())
    with pytest.raises(AssertionError, match="elements differ in their bits"):
        assert_bits_equal(out, ref, what=fault)
    d = (out.double() - ref.double())[out != ref]
    if fault == "last_k":  # the difference is the dropped product, up to the output's rounding step
        assert d.abs().min().item() >= 1
    if fault == "no_bias":
        assert d.abs().max().item() >= 8


# (shape, seed) at which each fault, final bf16 rounding included, is inside _assert_close's bound. A partial kept in
# bf16 is inside it at every tabled shape and seed tried (0.18 - 0.41 against 0.49 - 1.23). A dropped k element and a
# dropped bias are one product / one bias value (up to 1) plus the output's rounding: about 1.05 - 1.25, above the
# bound at K ~ 1000 (0.5 - 0.6) and at it at K = 4096 (1.0 - 1.2, by the seed's largest output): asserted at a seed
# where it holds; at the other seeds tried they miss the bound by a few per cent.
WITHIN = {"bf16_partial": [(s, 71) for s in TABLED], "last_k": [((512, 512, 4096), 735)],
          "no_bias": [((512, 512, 4096), 735)]}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_each_fault_is_inside_the_tolerance_bound_on_uniform_operands(fault):
    """What the tolerance tests cannot see: ``_assert_close`` (their own function) accepts the faulty output."""
    for (M, N, K), seed in WITHIN[fault]:
        a, b, bias = _rand(M, K, seed=seed), _rand(N, K, seed=seed + 1), _rand(N, seed=seed + 2)
        ref = _ref_gemm(a, b, bias)
        # fp64 products: the faulty output's roundings do not hang on this CPU's fp32 summation order
        out = FAULTS[fault](a.double(), b.double(), bias.double())
        err, bound = (out.float() - ref).abs().max().item(), 1e-2 * (ref.abs().max().item() + 1e-6) + 1e-2
        print(f"{fault} {M}x{N}x{K} seed {seed}: max err {err:.3f}, bound {bound:.3f}")
        assert not torch.equal(out, ref.to(BF16))  # the fault did change the output
        _assert_close(out, ref, K)


def test_mismatch_report_format():
    ref = torch.zeros(2, 600, 520, dtype=BF16)
    out = ref.clone()
    assert mismatch_report(out, ref) is None
    out[1, 300, 7] = 4.0
    out[1, 599, 519] = -6.0
    out[0, 5, 300] = -0.0
    msg = mismatch_report(out, ref)
    assert msg.startswith("3 of 624000 elements differ in their bits; first at (batch, row, col) = (0, 5, 300); ")
    assert "3 differing 256x256 tiles (batch, tile row, tile col): (0, 0, 1), (1, 1, 0), (1, 2, 2); " in msg
    assert "out - ref over the mismatches: min -6, max 4" in msg
    assert msg.endswith("1 of them differ only in the sign of zero")
    with pytest.raises(AssertionError, match=r"^w4 3x: 3 of 624000 elements differ"):
        assert_bits_equal(out, ref, what="w4 3x")
    assert "2 differing 128x128 tiles" in mismatch_report(out[1], ref[1], tile=(128, 128))
    with pytest.raises(AssertionError):
        assert_bits_equal(out.float(), ref)  # dtypes must agree: bits are compared
    # 1-D (a bias gradient) and fp32
    v = torch.arange(8, dtype=torch.float32)
    w = v.clone()
    w[6] += 1
    assert "first at (batch, row, col) = (0, 0, 6)" in mismatch_report(w, v)


def test_framed_window_check():
    big, win = exact.framed(40, 24, ld=35, col0=3, pad_rows=2, device="cpu")
    assert win.shape == (40, 24) and win.stride() == (35, 1) and win.data_ptr() == big.data_ptr() + 6
    ref = _ints(40, 24, seed=51)
    win.copy_(ref)
    exact.assert_window_bits_equal(big, ref, col0=3)
    big[40, 0] = 1.0  # a stray write below the window
    with pytest.raises(AssertionError, match=r"first at \(batch, row, col\) = \(0, 40, 0\)"):
        exact.assert_window_bits_equal(big, ref, col0=3)
    big3, win3 = exact.framed(8, 16, ld=24, batch=2, device="cpu")
    assert win3.shape == (2, 8, 16)
    win3.copy_(_ints(2, 8, 16, seed=52))
    exact.assert_window_bits_equal(big3, _ints(2, 8, 16, seed=52))
    win3[1, 2, 3] += 1
    with pytest.raises(AssertionError, match=r"first at \(batch, row, col\) = \(1, 2, 3\)"):
        exact.assert_window_bits_equal(big3, _ints(2, 8, 16, seed=52))
