"""Bit-exact GEMM checks on small-integer operands (a plain helper module, not a conftest).

Operands are integers, uniform in [lo, hi] (default [-3, 3]): exact in bf16 and in e4m3. Every product is
an integer of magnitude <= 9, every partial sum in any order an integer below 2^24, so every fp32
accumulation is exact whatever the MFMA order, split count, tile raster or pipelining. The linear epilogue
(alpha a power of two, power-of-two weight scales, integer bias, relu, integer residual) is exact as well,
and the kernels round once, RNE, to bf16: the expected output is ONE bit pattern, the fp64 result rounded
once. ``exact_ref`` computes it and asserts that the case stays inside that regime; ``assert_bits_equal``
compares every element's bits and says where and by how much a result differs.
"""
from __future__ import annotations

import math

import torch

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
LIMIT = float(2 ** 24)          # integers (in units of the result's grid) below this are exact in fp32
W8_SCALES = (0.25, 0.5, 1.0, 2.0)
SENTINEL_BITS = 0x5A5A          # a finite bf16 pattern (about 1.5e16) no exact-regime result can take


def _default_device() -> str:
    return "cuda" if torch.cuda.is_available() else "cpu"


def int_operand(*shape, seed: int, lo: int = -3, hi: int = 3, dtype=BF16, device: str | None = None):
    """A seeded integer-valued tensor, uniform in [lo, hi]: the same values on every device (drawn on the
    CPU). ``dtype=torch.float8_e4m3fn`` with a 2-D shape returns a ``QuantizedWeight`` whose codes are those
    integers and whose per-row scales are powers of two drawn from ``W8_SCALES``."""
    device = device or _default_device()
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int32).float()
    if dtype == FP8:
        from kubeflow_rm_amd.ops.gemm import QuantizedWeight
        assert len(shape) == 2, "an FP8 operand is a weight [N, K]"
        pick = torch.randint(0, len(W8_SCALES), (shape[0],), generator=g)
        scale = torch.tensor(W8_SCALES, dtype=torch.float32)[pick]
        codes = v.to(FP8)
        assert torch.equal(codes.float(), v), "integer codes must be exact in e4m3"
        return QuantizedWeight(codes.to(device), scale.to(device))
    t = v.to(dtype)
    assert torch.equal(t.float(), v), f"integers in [{lo}, {hi}] must be exact in {dtype}"
    return t.to(device)


def _pow2(x: float) -> bool:
    return x != 0 and math.frexp(abs(float(x)))[0] == 0.5


def _integral(t: torch.Tensor) -> bool:
    return bool(torch.equal(t, t.round()))


def _check_stage(v: torch.Tensor, unit: float, what: str) -> None:
    """Every value a multiple of ``unit`` (a power of two) and below 2^24 units: exact in fp32."""
    if v.numel() == 0:
        return
    q = v / unit
    assert _integral(q), f"exact_ref: {what} is off the {unit} grid"
    m = q.abs().max().item()
    assert m < LIMIT, f"exact_ref: {what} reaches {m} units of {unit}, not below 2^24: outside the exact regime"


def exact_ref(a, b, *, trans_a: bool = False, trans_b: bool = False, bias=None, residual=None, alpha: float = 1.0,
              relu: bool = False, gate=None) -> torch.Tensor:
    """bf16(RNE) of ``relu?(alpha * wscale[n] * (op(a) @ op(b)) + bias[n]) (* (gate > 0)) (+ residual)`` computed in
    fp64 on the operands' device and rounded ONCE. op = transpose of the last two dims when the flag is set
    (``gemm_nt(a, b)`` is ``trans_b=True``). ``b`` may be a ``QuantizedWeight`` ([N, K] codes with per-row scales,
    ``trans_b=True``). ``gate`` is the pre-activation of a fused relu backward (``dgrad_act``).

    Asserts the exact regime: integer operands, bias and residual; alpha and the scales powers of two; the bound on
    any partial sum (max|a| * max|b| * K, times |alpha| * max scale) and every intermediate result below 2^24
    units of the result's grid. A case that passes these asserts has exactly one right answer."""
    wscale = None
    if hasattr(b, "codes"):
        assert trans_b, "a QuantizedWeight is stored [N, K]"
        b, wscale = b.codes.float(), b.scale
    a64, b64 = a.double(), b.double()
    assert _integral(a64) and _integral(b64), "exact_ref: operands must be integer-valued"
    assert _pow2(alpha), f"exact_ref: alpha must be a power of two, got {alpha}"
    if trans_a:
        a64 = a64.transpose(-1, -2)
    if trans_b:
        b64 = b64.transpose(-1, -2)
    K = a64.shape[-1]
    assert b64.shape[-2] == K, (tuple(a64.shape), tuple(b64.shape))
    smax = smin = 1.0
    if wscale is not None:
        s64 = wscale.double()
        assert all(_pow2(s) for s in s64.unique().tolist()), "exact_ref: weight scales must be powers of two"
        smax, smin = s64.max().item(), s64.min().item()
    # the unscaled partial sums of any k subset in any order, then the scaled accumulator
    part = a64.abs().max().item() * b64.abs().max().item() * K
    assert part < LIMIT and part * abs(alpha) * smax < LIMIT * min(1.0, abs(alpha) * smin), (
        f"exact_ref: partial sums bounded by {part} (x |alpha| {abs(alpha)} x scale {smax}) are not below 2^24")
    unit = min(1.0, abs(alpha) * smin)
    v = a64 @ b64
    _check_stage(v, 1.0, "the accumulator")
    v = v * alpha
    if wscale is not None:
        v = v * wscale.double()
    _check_stage(v, unit, "the scaled accumulator")
    if bias is not None:
        b1 = bias.double()
        assert _integral(b1), "exact_ref: bias must be integer-valued"
        v = v + b1
        _check_stage(v, unit, "accumulator + bias")
    if relu:
        v = torch.relu(v)
    if gate is not None:
        v = v * (gate.double() > 0).double()
    if residual is not None:
        r = residual.double()
        assert _integral(r), "exact_ref: residual must be integer-valued"
        v = v + r
        _check_stage(v, unit, "result + residual")
    f = v.float()
    assert torch.equal(f.double(), v), "exact_ref: the result is not exact in fp32"
    return f.to(BF16)  # the one rounding, RNE


def exact_colsum(g64: torch.Tensor) -> torch.Tensor:
    """fp32 column sums of an integer-valued fp64 matrix, asserted exact (rows * max|g| < 2^24)."""
    assert _integral(g64)
    bound = g64.shape[0] * (g64.abs().max().item() if g64.numel() else 0.0)
    assert bound < LIMIT, f"exact_colsum: rows * max|g| = {bound} is not below 2^24"
    return g64.sum(0).float()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def mismatch_report(out: torch.Tensor, ref: torch.Tensor, tile=(256, 256)) -> str | None:
    """None when ``out`` and ``ref`` agree in every bit, else the description ``assert_bits_equal`` raises with."""
    assert out.dtype == ref.dtype and out.element_size() in (2, 4), (out.dtype, ref.dtype)
    assert tuple(out.shape) == tuple(ref.shape), (tuple(out.shape), tuple(ref.shape))
    ob, rb = _bits(out), _bits(ref)
    if torch.equal(ob, rb):
        return None
    shape = tuple(out.shape)
    cols = shape[-1] if len(shape) >= 1 else 1
    rows = shape[-2] if len(shape) >= 2 else 1
    ne = (ob != rb).reshape(-1, rows, cols)
    idx = ne.nonzero()
    count = idx.shape[0]
    first = tuple(idx[0].tolist())
    tiles = torch.unique(torch.stack([idx[:, 0], idx[:, 1] // tile[0], idx[:, 2] // tile[1]], 1), dim=0).tolist()
    d = (out.double() - ref.double()).reshape(-1, rows, cols)[ne]
    zeros = int(((out.double() == 0) & (ref.double() == 0)).reshape(-1, rows, cols)[ne].sum().item())
    shown = ", ".join(str(tuple(t)) for t in tiles[:16]) + (", ..." if len(tiles) > 16 else "")
    return (f"{count} of {ne.numel()} elements differ in their bits; first at (batch, row, col) = {first}; "
            f"{len(tiles)} differing {tile[0]}x{tile[1]} tiles (batch, tile row, tile col): {shown}; "
            f"out - ref over the mismatches: min {d.min().item():g}, max {d.max().item():g}"
            + (f"; {zeros} of them differ only in the sign of zero" if zeros else ""))


def assert_bits_equal(out: torch.Tensor, ref: torch.Tensor, tile=(256, 256), what: str = "") -> None:
    """Every element of ``out`` has ``ref``'s bit pattern (``torch.equal`` on the raw bits: no tolerance, no
    element skipped, -0 != +0). On failure: the mismatch count, the first (batch, row, col), the set of
    differing output tiles and min / max of out - ref over the mismatches (on integer operands an integer
    combination of dropped or doubled products, which points at the k range)."""
    msg = mismatch_report(out, ref, tile)
    assert msg is None, (what + ": " if what else "") + msg


def framed(rows: int, cols: int, *, ld: int, col0: int = 0, batch: int | None = None, pad_rows: int = 0,
           device: str | None = None):
    """(big, window): a sentinel-filled bf16 buffer [(batch,) rows + pad_rows, ld] and its [rows, cols] window
    at column ``col0`` (row stride ld), for an ``out=`` argument."""
    device = device or _default_device()
    shape = (rows + pad_rows, ld) if batch is None else (batch, rows + pad_rows, ld)
    big = torch.empty(shape, dtype=BF16, device=device)
    big.view(torch.int16).fill_(SENTINEL_BITS)
    return big, big[..., :rows, col0:col0 + cols]


def assert_window_bits_equal(big: torch.Tensor, ref: torch.Tensor, *, col0: int = 0, tile=(256, 256),
                             what: str = "") -> None:
    """The window of ``big`` at (row 0, column col0) equals ``ref`` and the whole frame around it still holds the
    sentinel, bit for bit (one comparison of the full buffer)."""
    want = torch.empty_like(big)
    want.view(torch.int16).fill_(SENTINEL_BITS)
    want[..., :ref.shape[-2], col0:col0 + ref.shape[-1]] = ref
    assert_bits_equal(big, want, tile, what=(what + " (window + frame)").strip())
