"""Every bf16 GEMM kernel and plan, bit for bit, on small-integer operands (tests/exact.py).

Integer operands in [-3, 3] make every fp32 partial sum exact in any order, so each kernel's output has one right
bit pattern: the fp64 result rounded once (RNE) to bf16. A stale LDS buffer, an accumulator cleared a step early, a
K tail masked one element short, a split's partial kept in bf16 or a dropped bias each change bits here, where the
tolerance tests (test_gpu_kernels.py, test_gpu_decode.py, test_gpu_w8.py) cannot see them. Linear epilogues only
(alpha in {1, 0.5}, integer bias / residual in [-8, 8], relu); the transcendental ones stay with the tolerance tests.
No kernel takes an activation together with a residual (the library refuses it), so relu and the residual run as
two epilogues of the same operands."""
import pytest
import torch

from tests.exact import (BF16, FP8, assert_bits_equal, assert_window_bits_equal, exact_colsum, exact_ref, framed,
                         int_operand)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_cache: dict = {}


def _ints(*shape, seed, **kw):
    return int_operand(*shape, seed=seed, device=DEV, **kw)


def _ints8(*shape, seed):
    return _ints(*shape, seed=seed, lo=-8, hi=8)


def _nt(M, N, K, batch=None):
    """Operands, bias and residual of an NT problem, made once per shape."""
    key = (M, N, K, batch)
    if key not in _cache:
        lead = () if batch is None else (batch,)
        _cache[key] = (_ints(*lead, M, K, seed=1), _ints(*lead, N, K, seed=2), _ints8(N, seed=3),
                       _ints8(*lead, M, N, seed=4))
    return _cache[key]


def _epilogues(bias, res):
    """(name, gemm_nt's keywords, exact_ref's keywords) of every linear epilogue."""
    return [("plain", {}, {}),
            ("alpha", {"alpha": 0.5}, {"alpha": 0.5}),
            ("bias+relu", {"bias": bias, "act": "relu", "alpha": 0.5}, {"bias": bias, "relu": True, "alpha": 0.5}),
            ("bias+residual", {"bias": bias, "residual": res}, {"bias": bias, "residual": res}),
            ("alpha+residual", {"residual": res, "alpha": 0.5}, {"residual": res, "alpha": 0.5})]


def _w4_variants(M, N):
    """The tiled variants that take a shape with edge tiles: the 256 tile needs M, N >= 256."""
    return (["w4"] if M >= 256 and N >= 256 else []) + ["w4s", "auto"]


# ---- the NT kernels on the tile grid ------------------------------------------------------------------------------

NT_VARIANTS = ["fast", "pipe", "pipe_sched", "w4", "w4s", "auto"]


@pytest.mark.parametrize("variant", NT_VARIANTS)
@pytest.mark.parametrize("kt", [1, 2, 3, 4, 5, 9])
def test_nt_k_loop_depths(kt, variant):
    """K / 64 in {1, 2, 3, 4, 5, 9}: prologue, steady state and tail of any pipeline depth, M, N in {256, 512}.
    (kt = 1 is one aligned MFMA k-step per tile: it also confirms that MFMA accumulates integers exactly.)"""
    from kubeflow_rm_amd.ops import gemm_nt
    K = 64 * kt
    for M in (256, 512):
        for N in (256, 512):
            a, b, bias, _ = _nt(M, N, K)
            what = f"{variant} {M}x{N}x{K}"
            assert_bits_equal(gemm_nt(a, b, variant=variant), exact_ref(a, b, trans_b=True), what=what)
            out = gemm_nt(a, b, bias=bias, act="relu", alpha=0.5, variant=variant)
            assert_bits_equal(out, exact_ref(a, b, trans_b=True, bias=bias, relu=True, alpha=0.5), what=what + " relu")


@pytest.mark.parametrize("variant", NT_VARIANTS + ["generic"])
def test_nt_epilogues(variant):
    from kubeflow_rm_amd.ops import gemm_nt
    M, N, K = 512, 768, 192
    a, b, bias, res = _nt(M, N, K)
    for name, kw, rkw in _epilogues(bias, res):
        assert_bits_equal(gemm_nt(a, b, variant=variant, **kw), exact_ref(a, b, trans_b=True, **rkw),
                          what=f"{variant} {name}")
    with pytest.raises(RuntimeError):  # the contract the split above rests on
        gemm_nt(a, b, bias=bias, act="relu", residual=res, variant=variant)


@pytest.mark.parametrize("variant", NT_VARIANTS + ["generic"])
def test_nt_batched(variant):
    from kubeflow_rm_amd.ops import gemm_nt
    a, b, bias, res = _nt(256, 512, 128, batch=3)
    for name, kw, rkw in _epilogues(bias, res):
        assert_bits_equal(gemm_nt(a, b, variant=variant, **kw), exact_ref(a, b, trans_b=True, **rkw),
                          what=f"{variant} batched {name}")


@pytest.mark.parametrize("variant", NT_VARIANTS + ["generic"])
def test_nt_strided_operands_and_framed_output(variant):
    """lda = ldb = K + 64, and the output as a window (16-B aligned) of a sentinel-filled wider buffer: the window
    and the whole frame bit for bit."""
    from kubeflow_rm_amd.ops import gemm_nt
    M, N, K = 512, 256, 192
    abig, bbig = _ints(M, K + 64, seed=5), _ints(N, K + 64, seed=6)
    a, b = abig[:, :K], bbig[:, :K]
    assert a.stride(0) == K + 64 and b.stride(0) == K + 64
    bias, res = _ints8(N, seed=7), _ints8(M, N, seed=8)
    for name, kw, rkw in _epilogues(bias, res):
        ref = exact_ref(a, b, trans_b=True, **rkw)
        big, win = framed(M, N, ld=N + 64, col0=8, pad_rows=1)
        assert gemm_nt(a, b, out=win, variant=variant, **kw) is win
        assert_window_bits_equal(big, ref, col0=8, what=f"{variant} {name}")


# ---- edge tiles in the kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(264, 392, 200), (383, 136, 72), (511, 1001, 136)])
def test_edge_tiles_in_kernel(M, N, K):
    """Shifted last tiles, masked stores, a zero-filled K tail and (N = 1001) the element-wise epilogue, with every
    linear epilogue and the in-place residual (a double store would add it twice)."""
    from kubeflow_rm_amd.ops import gemm, gemm_nt
    assert gemm._w4_nt_shape(M, N, K) and gemm.splitk_plan(M, N, K) is None and gemm.fixk_plan(M, N, K) is None
    a, b, bias, res = _nt(M, N, K)
    for name, kw, rkw in _epilogues(bias, res):
        ref = exact_ref(a, b, trans_b=True, **rkw)
        for v in _w4_variants(M, N):
            assert_bits_equal(gemm_nt(a, b, variant=v, **kw), ref, what=f"{v} {name}")
    ref = exact_ref(a, b, trans_b=True, bias=bias, residual=res)
    for v in _w4_variants(M, N):
        c = res.clone()
        gemm_nt(a, b, bias=bias, residual=c, out=c, variant=v)
        assert_bits_equal(c, ref, what=f"{v} in-place residual")


def test_edge_tiles_odd_output_stride_frame():
    """(640, 1496, 256) into a column window of an ldc = 1503 buffer (rows off 16 B): exactly the window is written."""
    from kubeflow_rm_amd.ops import gemm_nt
    M, N, K = 640, 1496, 256
    a, b, bias, res = _nt(M, N, K)
    for name, kw, rkw in _epilogues(bias, res):
        ref = exact_ref(a, b, trans_b=True, **rkw)
        for v in _w4_variants(M, N):
            big, win = framed(M, N, ld=1503, col0=3, pad_rows=1)
            gemm_nt(a, b, out=win, variant=v, **kw)
            assert_window_bits_equal(big, ref, col0=3, what=f"{v} {name}")


# ---- the generic kernel, and K off the 8-grid through pad_k ---------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (17, 33, 65), (129, 127, 130)])
def test_generic_kernel(M, N, K):
    from kubeflow_rm_amd.ops import gemm_nt
    a, b, bias, res = _nt(M, N, K)
    for name, kw, rkw in _epilogues(bias, res):
        ref = exact_ref(a, b, trans_b=True, **rkw)
        for v in ("generic", "auto"):  # auto: below the tiled contract and the padding threshold
            assert_bits_equal(gemm_nt(a, b, variant=v, **kw), ref, tile=(128, 128), what=f"{v} {name}")


@pytest.mark.parametrize("M,N,K,batch", [(257, 300, 77, None), (384, 256, 1001, None), (256, 384, 77, 2)])
def test_k_off_grid_through_pad_k(M, N, K, batch):
    """K % 8 != 0: pad_k's own output (the copy and its zero tail) and the GEMM on it."""
    from kubeflow_rm_amd.ops import gemm, gemm_nt
    a, b, bias, res = _nt(M, N, K, batch)
    Kp = (K + 7) // 8 * 8
    assert not gemm._w4_nt_shape(M, N, K) and M >= 128 and N >= 128  # the packed route of gemm_nt
    ap, bp = gemm.pad_k(a, b, Kp)
    F = torch.nn.functional
    assert_bits_equal(ap, F.pad(a, (0, Kp - K)), what="pad_k a")
    assert_bits_equal(bp, F.pad(b, (0, Kp - K)), what="pad_k b")
    only, none = gemm.pad_k(a, None, Kp)
    assert none is None
    assert_bits_equal(only, ap, what="pad_k of one operand")
    for name, kw, rkw in _epilogues(bias, res):
        assert_bits_equal(gemm_nt(a, b, **kw), exact_ref(a, b, trans_b=True, **rkw), what=name)


# ---- mm: the four operand layouts -----------------------------------------------------------------------------------

LAYOUTS = [(False, False), (True, False), (True, True), (False, True)]


def _mm_operands(M, N, K, ta, tb, batch=None, seed=11):
    lead = () if batch is None else (batch,)
    a = _ints(*lead, *((K, M) if ta else (M, K)), seed=seed)
    b = _ints(*lead, *((N, K) if tb else (K, N)), seed=seed + 1)
    return a, b


def _check_mm(M, N, K, ta, tb, batch=None):
    from kubeflow_rm_amd.ops import mm
    a, b = _mm_operands(M, N, K, ta, tb, batch)
    what = f"mm ta={ta} tb={tb} {M}x{N}x{K}"
    out = mm(a, b, trans_a=ta, trans_b=tb)
    assert_bits_equal(out, exact_ref(a, b, trans_a=ta, trans_b=tb), what=what)
    res = _ints8(*out.shape, seed=13)
    assert_bits_equal(mm(a, b, trans_a=ta, trans_b=tb, residual=res, alpha=0.5),
                      exact_ref(a, b, trans_a=ta, trans_b=tb, residual=res, alpha=0.5), what=what + " residual")
    # accumulate in place: out = 0.5 * op(a) op(b) + out
    acc = res.clone()
    mm(a, b, trans_a=ta, trans_b=tb, out=acc, residual=acc, alpha=0.5)
    assert_bits_equal(acc, exact_ref(a, b, trans_a=ta, trans_b=tb, residual=res, alpha=0.5), what=what + " accumulate")
    return a, b, out


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K,batch", [(256, 256, 64, None), (392, 264, 200, None), (1496, 1000, 776, None),
                                         (256, 384, 128, 2)])
def test_mm_layouts(M, N, K, batch, ta, tb):
    """k-major operands through the transposing LDS reads: the plain w4 launch of each layout (no split plan)."""
    from kubeflow_rm_amd.ops import gemm
    b_ = batch or 1
    assert gemm._w4_shape(M, N, K) and gemm.splitk_plan(M, N, K, b_) is None and gemm.fixk_plan(M, N, K, b_) is None
    _check_mm(M, N, K, ta, tb, batch)


# ---- split-K: fp32 partials + the reduce launch ---------------------------------------------------------------------

def _without(flag, fn):
    from kubeflow_rm_amd.ops import gemm
    old = getattr(gemm, flag)
    setattr(gemm, flag, False)
    try:
        return fn()
    finally:
        setattr(gemm, flag, old)


@pytest.mark.parametrize("M,N,K,batch", [(384, 512, 2056, None), (136, 128, 2120, None), (256, 256, 4096, 2)])
def test_splitk_nt_epilogues_and_unsplit(M, N, K, batch):
    """Bias / relu / residual in the reduce; a K that leaves the last split partial; bitwise the unsplit kernel."""
    from kubeflow_rm_amd.ops import gemm, gemm_nt
    splits, kper = gemm.splitk_plan(M, N, K, batch or 1)
    assert splits >= 2 and kper % 64 == 0 and (splits - 1) * kper < K <= splits * kper
    assert gemm.fixk_plan(M, N, K, batch or 1) is None
    a, b, bias, res = _nt(M, N, K, batch)
    for name, kw, rkw in _epilogues(bias, res):
        out = gemm_nt(a, b, **kw)
        assert_bits_equal(out, exact_ref(a, b, trans_b=True, **rkw), what=f"split-K {name}")
        assert_bits_equal(out, _without("SPLITK", lambda: gemm_nt(a, b, **kw)), what=f"split-K vs unsplit {name}")


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K,batch", [(384, 512, 2056, None), (136, 128, 2120, None), (256, 256, 4096, 2)])
def test_splitk_mm_layouts_and_unsplit(M, N, K, batch, ta, tb):
    from kubeflow_rm_amd.ops import gemm, mm
    assert gemm.splitk_plan(M, N, K, batch or 1) is not None and gemm.fixk_plan(M, N, K, batch or 1) is None
    a, b, out = _check_mm(M, N, K, ta, tb, batch)
    assert_bits_equal(out, _without("SPLITK", lambda: mm(a, b, trans_a=ta, trans_b=tb)), what="split-K vs unsplit")


# ---- the pre-activation output ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["gelu_tanh", "silu"])
@pytest.mark.parametrize("M,N,K", [(512, 768, 192), (511, 1001, 136), (384, 512, 2056)])
def test_preact_output_z(M, N, K, act):
    """gemm_nt_preact's second output, the pre-activation z = a b^T + bias (linear, so exact), from the same GEMM
    as y: on the grid, through the element-wise epilogue, and from the split-K reduce. (The kernels emit z only
    next to gelu / silu; y itself stays with the tolerance tests.)"""
    from kubeflow_rm_amd.ops import gemm
    assert (gemm.splitk_plan(M, N, K) is not None) == (K == 2056)
    a, b, bias, _ = _nt(M, N, K)
    for bb in (bias, None):
        y, z = gemm.gemm_nt_preact(a, b, bb, act)
        assert_bits_equal(z, exact_ref(a, b, trans_b=True, bias=bb), what=f"z ({act}, bias={bb is not None})")
        assert y.shape == z.shape and torch.isfinite(y.float()).all().item()


# ---- split-K with the in-kernel fixup -------------------------------------------------------------------------------

def _fixk_counters_zero():
    from kubeflow_rm_amd.ops import gemm
    torch.cuda.synchronize()
    assert gemm._fixk_ws
    for _, cnt in gemm._fixk_ws.values():
        assert int(cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("S", [2, 3, 5, 16])
def test_fixk_forced_splits(S):
    """mm(trans_a=True) of 2 x (4096 x 512, 4096 x 768) at S splits: three launches over one workspace, each
    bitwise the exact result and the run without the fixup; the arrival counters back at zero."""
    from kubeflow_rm_amd.ops import gemm, mm
    a, b = _mm_operands(512, 768, 4096, True, False, batch=2, seed=21)
    ref = exact_ref(a, b, trans_a=True)
    whole = _without("FIXK", lambda: mm(a, b, trans_a=True))
    assert_bits_equal(whole, ref, what="FIXK = False")
    gemm.FIXK_SPLITS = S
    try:
        assert gemm.fixk_plan(512, 768, 4096, 2)[0] == S
        for i in range(3):
            out = mm(a, b, trans_a=True)
            assert_bits_equal(out, ref, what=f"fix-K S={S} launch {i}")
            assert_bits_equal(out, whole, what=f"fix-K S={S} launch {i} vs FIXK = False")
        res = _ints8(2, 512, 768, seed=23)
        acc = res.clone()
        mm(a, b, trans_a=True, out=acc, residual=acc, alpha=0.5)
        assert_bits_equal(acc, exact_ref(a, b, trans_a=True, residual=res, alpha=0.5), what=f"fix-K S={S} accumulate")
    finally:
        gemm.FIXK_SPLITS = None
    _fixk_counters_zero()


def test_fixk_nt_planned():
    """An NT shape fixk_plan takes by itself (90 tiles of 256, edge tiles in M, a partial last split)."""
    from kubeflow_rm_amd.ops import gemm, gemm_nt
    M, N, K = 2300, 2560, 4104
    splits, kper = gemm.fixk_plan(M, N, K)
    assert splits >= 2 and kper % 64 == 0 and (splits - 1) * kper < K <= splits * kper
    a, b, _, res = _nt(M, N, K)
    for name, kw, rkw in (("plain", {}, {}), ("alpha+residual", {"residual": res, "alpha": 0.5},
                                              {"residual": res, "alpha": 0.5})):
        out = gemm_nt(a, b, **kw)
        assert_bits_equal(out, exact_ref(a, b, trans_b=True, **rkw), what=f"fix-K NT {name}")
        assert_bits_equal(out, _without("FIXK", lambda: gemm_nt(a, b, **kw)), what=f"fix-K NT {name} vs FIXK = False")
    _fixk_counters_zero()


# ---- stream-K ---------------------------------------------------------------------------------------------------------

@pytest.fixture
def streamk_on():
    from kubeflow_rm_amd.ops import gemm
    old = gemm.STREAMK
    gemm.STREAMK = True
    yield
    gemm.STREAMK = old


@pytest.mark.parametrize("M,N,K", [(2304, 2304, 1024), (1000, 5000, 3000)])
def test_streamk_epilogues_and_plain(M, N, K, streamk_on):
    """The owner's epilogue after adding the producers' fp32 partials: bitwise the exact result and the plain
    kernel, on the grid and with edge tiles in M and N and K % 64 != 0."""
    from kubeflow_rm_amd.ops import gemm, gemm_nt
    grid, splits = gemm.streamk_plan(M, N, K)
    assert grid == 256 and splits >= 2
    assert gemm.splitk_plan(M, N, K) is None and gemm.fixk_plan(M, N, K) is None  # nothing takes it first
    a, b, bias, res = _nt(M, N, K)
    for name, kw, rkw in _epilogues(bias, res):
        out = gemm_nt(a, b, **kw)
        assert_bits_equal(out, exact_ref(a, b, trans_b=True, **rkw), what=f"stream-K {name}")
        assert_bits_equal(out, _without("STREAMK", lambda: gemm_nt(a, b, **kw)), what=f"stream-K vs plain {name}")


def test_streamk_deadline_path_and_epochs():
    """The plan sequence of test_gpu_kernels.py::test_streamk_deadline_path_and_epochs, at its shape, bit for bit:
    owners that recompute their producers' splits after the deadline, a grid of 4x the CUs, new epochs over the
    same flag words."""
    from kubeflow_rm_amd.ops import gemm
    M, N, K = 2304, 2304, 2048
    a, b, _, _ = _nt(M, N, K)
    ref = exact_ref(a, b, trans_b=True)
    c = torch.empty(M, N, dtype=BF16, device=DEV)
    for plan, force in (((256, 3), True), ((256, 3), False), ((1024, 8), False), ((256, 4), False), ((256, 3), False)):
        c.zero_()
        rc = gemm._streamk(a, b, c, M, N, K, K, K, N, plan, bias=None, r_ptr=None, ldr=0, aux=None, alpha=1.0,
                           act="none", _force_deadline=force)
        assert rc == 0
        assert_bits_equal(c, ref, what=f"stream-K plan {plan} deadline={force}")


# ---- the paired weight gradient and the fused dgrad-through-activation -----------------------------------------------

@pytest.mark.parametrize("M1,M2,N,N2", [(768, 256, 512, 512), (768, 256, 256, 768)])
@pytest.mark.parametrize("plan", [None, (2, 256), (3, 192)])
def test_wgrad_pair(plan, M1, M2, N, N2):
    """Two weight gradients in one launch, whole K and K split 2 and 3 ways by the in-kernel fixup, a second
    problem of the same and of its own width: both outputs bit for bit."""
    from kubeflow_rm_amd import ops
    K = 512
    if plan is not None:
        assert (plan[0] - 1) * plan[1] < K <= plan[0] * plan[1]
    g1, x1 = _ints(K, M1, seed=31), _ints(K, N, seed=32)
    g2, x2 = _ints(K, M2, seed=33), _ints(K, N2, seed=34)
    for i in range(2):  # twice: the arrival counters of the first launch are reused
        out = ops.wgrad_pair(g1, x1, g2, x2, force=True, plan=plan)
        assert out is not None, "the pair kernel refused a shape inside its contract"
        assert_bits_equal(out[0], exact_ref(g1, x1, trans_a=True), what=f"pair output 1 plan {plan} launch {i}")
        assert_bits_equal(out[1], exact_ref(g2, x2, trans_a=True), what=f"pair output 2 plan {plan} launch {i}")


@pytest.mark.parametrize("M,K,N", [(512, 256, 768), (256, 2048, 1024)])
def test_dgrad_act_relu(M, K, N):
    """g = (gy @ W) * (z > 0) bit for bit on an integer z with many exact zeros; the bias gradient (column sums of
    the unrounded fp32 g) exact as fp32, and as bf16 the RNE of that exact sum."""
    from kubeflow_rm_amd import ops
    gy, w, z = _ints(M, K, seed=41), _ints(K, N, seed=42), _ints(M, N, seed=43)
    assert (z == 0).float().mean().item() > 0.1
    out = ops.dgrad_act(gy, w, z, "relu", True, torch.float32)
    assert out is not None, "the fused kernel refused a 256-multiple shape"
    g, db = out
    ref = exact_ref(gy, w, gate=z)
    assert_bits_equal(g, ref, what="g")
    col = exact_colsum((gy.double() @ w.double()) * (z.double() > 0).double())
    assert_bits_equal(db, col, what="db fp32")
    g2, db2 = ops.dgrad_act(gy, w, z, "relu", True, BF16)
    assert_bits_equal(g2, ref, what="g (bf16 db)")
    assert_bits_equal(db2, col.to(BF16), what="db bf16")
    g3, db3 = ops.dgrad_act(gy, w, z, "relu", False)
    assert db3 is None
    assert_bits_equal(g3, ref, what="g (no db)")


# ---- the weight-streaming kernels (M <= 16) -------------------------------------------------------------------------

SKINNY_M = [1, 3, 8, 9, 16]


def _skinny_variants(M):
    return ["skinny", "skinny_mfma"] + (["skinny_valu"] if M <= 8 else [])


def _check_skinny(M, N, K, weight, run):
    """Every linear epilogue on every arithmetic form, contiguous, then a strided A into a framed C."""
    a, bias, res = _ints(M, K, seed=51 + M), _ints8(N, seed=52), _ints8(M, N, seed=53)
    abig = _ints(M, K + 64, seed=54 + M)
    a_strided = abig[:, 8:8 + K]  # lda = K + 64, a 16-B aligned start
    for name, kw, rkw in _epilogues(bias, res):
        ref = exact_ref(a, weight, trans_b=True, **rkw)
        ref_s = exact_ref(a_strided, weight, trans_b=True, **rkw)
        for v in _skinny_variants(M):
            out = run(a, v, kw, None)
            assert out.shape == (M, N) and out.dtype == BF16
            assert_bits_equal(out, ref, tile=(16, 128), what=f"{v} {name}")
            big, win = framed(M, N, ld=N + 27, pad_rows=1)
            run(a_strided, v, kw, win)
            assert_window_bits_equal(big, ref_s, tile=(16, 128), what=f"{v} {name} strided")


@pytest.mark.parametrize("N,K", [(128, 64), (136, 2056), (1001, 264)])
@pytest.mark.parametrize("M", SKINNY_M)
def test_skinny_bf16(M, N, K):
    from kubeflow_rm_amd.ops import gemm_nt
    w = _ints(N, K, seed=55)
    _check_skinny(M, N, K, w, lambda a, v, kw, out: gemm_nt(a, w, variant=v, out=out, **kw))


@pytest.mark.parametrize("N,K", [(128, 64), (136, 2064), (1001, 272)])
@pytest.mark.parametrize("M", SKINNY_M)
def test_skinny_w8(M, N, K):
    """W8A16: integer e4m3 codes and power-of-two row scales keep alpha * wscale[n] * acc + bias exact."""
    from kubeflow_rm_amd.ops import gemm_nt
    qw = _ints(N, K, seed=56, dtype=FP8)
    _check_skinny(M, N, K, qw, lambda a, v, kw, out: gemm_nt(a, qw, variant=v, out=out, **kw))


@pytest.mark.parametrize("N,K", [(128, 64), (1001, 272)])
@pytest.mark.parametrize("M", SKINNY_M)
def test_skinny_w8_every_tiles_value(M, N, K):
    """Every ``tiles`` value the entry point takes: the MFMA form's 1 / 2 / 4 tiles per wave, the VALU form's 2 / 4
    weight rows per wave ("skinny" is the VALU form for M <= 2 at these N); any other value is refused."""
    from kubeflow_rm_amd.ops.gemm import _gemm_nt_w8
    qw = _ints(N, K, seed=57, dtype=FP8)
    a, bias, res = _ints(M, K, seed=58 + M), _ints8(N, seed=59), _ints8(M, N, seed=60)
    ref = exact_ref(a, qw, trans_b=True, bias=bias, residual=res, alpha=0.5)
    ref_relu = exact_ref(a, qw, trans_b=True, bias=bias, relu=True, alpha=0.5)
    for v in _skinny_variants(M):
        valu = v == "skinny_valu" or (v == "skinny" and M <= 2)
        for tiles in ((0, 2, 4) if valu else (0, 1, 2, 4)):
            out = _gemm_nt_w8(a, qw, bias, res, 0.5, "none", None, v, tiles)
            assert_bits_equal(out, ref, tile=(16, 128), what=f"{v} tiles={tiles} residual")
            out = _gemm_nt_w8(a, qw, bias, None, 0.5, "relu", None, v, tiles)
            assert_bits_equal(out, ref_relu, tile=(16, 128), what=f"{v} tiles={tiles} relu")
        with pytest.raises(RuntimeError):
            _gemm_nt_w8(a, qw, bias, None, 0.5, "none", None, v, 1 if valu else 3)
