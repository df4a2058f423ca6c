"""LayerNorm / RMSNorm on the gfx950 kernels (kernels/layernorm_bf16.hip) against tests/norm_ref.py (float64, CPU), element
by element, on every launch path.

Two levels. The C entries kfamd_norm_fwd_bf16_path / kfamd_norm_bwd_bf16_path run on buffers the test owns: the path is
forced (forward 1 wave per row, 2 streaming, 3 block; backward 1 fused, 2 dx wave + column partials, 3 dx block +
partials), NaN sentinels stand 4 rows before and after y / dx, 4 slots round mean / rstd / dgamma / dbeta and behind
the kfamd_layernorm_bwd_workspace bytes of a NaN-filled workspace, and every input is compared by bits before and
after. Then ops.layer_norm, layer_norm_residual, rms_norm and rms_norm_residual run through autograd.

Bounds, per element, none excluded. With ref the float64 result and A the fp32 allowance of that output (below):
    bf16 outputs (y, dx, bf16 dgamma / dbeta):  |kernel - bf16(ref)| <= ulp_bf16(bf16(ref)) + 16 * A * scale
    fp32 outputs (mean, rstd, fp32 dgamma / dbeta):  |kernel - ref| <= 16 * A * scale
scale is the output's natural scale (norm_ref.py): y: |xhat gamma| + |beta| + |mean| rstd |gamma|; mean: mean_j |x|;
rstd: rstd; dx: |rstd gd| + |rstd xhat c1| + |rstd c2|; dgamma: sum_r (|dy xhat| + |dy| |mean| rstd); dbeta: sum_r |dy|. A is the largest
error, in that unit, of torch's own fp32 evaluation on the device (torch.native_layer_norm and its autograd; the RMS
formula in fp32 and its autograd) against the float64 reference over the inputs of this file: it measures fp32
arithmetic, not the kernel. The factor 16 is for the hardware rsqrt and another reduction order. The backward kernels
are handed the reference's statistics rounded to fp32. Every check prints its figures (``pytest -s``, NORM-FIG lines).

MEASURED (MI355X, every check of this file; units of each output's scale). torch's fp32 evaluation, which is ALLOW:
y 1.40e-5 (one element of a no-beta row at hidden 2560; 7.1e-7 otherwise), mean 7.13e-7, rstd 2.53e-7, dx 7.08e-6,
dgamma 6.09e-7, dbeta 5.98e-8; the offset rows give the largest of each but y's. The kernels' largest error, for bf16
outputs what is left beyond one bf16 rounding:
    forward    wave-per-row  y 3.5e-8  mean 7.9e-8  rstd 6.6e-7     streaming  y 7.0e-8  mean 7.9e-8  rstd 8.1e-7
               block         y 3.0e-8  mean 5.7e-8  rstd 3.5e-7     (rstd: the offset rows at hidden 8192, where a
               lane adds 128 squares in turn; an fp32 emulation of that order on the CPU gives 8.4e-7)
    backward   fused         dx 1.5e-7  dgamma 2.2e-7  dbeta 5.8e-8     dx wave + partials  dx 1.5e-7  dgamma 2.5e-7
               dbeta 5.7e-8     dx block + partials  dx 1.9e-6 (offset rows, hidden 3)  dgamma 2.7e-7  dbeta 4.4e-8
    every bf16 dgamma / dbeta within one rounding; through the ops: dx 5.6e-8, fp32 dgamma 2.1e-7, y within one rounding.
No test of this file fails on the kernels as they are. Arithmetic-only variants of layernorm_bf16.hip (none committed):
eps left out of rstd fails 111 of the 259 tests here (every forward test) and none of the earlier norm tests; c2 left out
of dx 61 (earlier tests: 5); the variance as E[x^2] - mean^2 35 (every forward path, on the offset rows; earlier: 0);
dres not added 118 (earlier: 21); the finalize leaving out one of its four chunk lanes 34 (earlier: 17).
"""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import pytest
import torch

from tests import norm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
EINVAL = -1
BF16_SENTINEL = 0x7FA5      # NaNs: a kernel that read a guard as data would show it
F32_SENTINEL = 0x7FC5A5A5
GUARD = 4                   # rows round y / dx, slots round the vectors
MARGIN = 16
# the fp32 allowances A (measured: torch's fp32 evaluation against float64, in units of each output's scale)
ALLOW = {"y": 1.40e-05, "mean": 7.14e-07, "rstd": 2.53e-07, "dx": 7.09e-06, "dgamma": 6.09e-07, "dbeta": 5.99e-08}
FIG: dict = {}

WAVE8 = [512 * v for v in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)]
WAVE4 = [256, 768, 1280]
STREAM = [512 * v for v in (1, 2, 3, 4, 5, 6, 8, 16)]
FUSED = [512, 1024, 1536, 2048] + WAVE4
BLOCK_ONLY = [1, 3, 7, 1000, 3584, 4608, 8200, 16384]
FWD_NAMES = {0: "auto", 1: "wave", 2: "stream", 3: "block"}
BWD_NAMES = {0: "auto", 1: "fused", 2: "dxwave+partials", 3: "dxblock+partials"}


def _L():
    from kubeflow_rm_amd.ops import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _bits_view(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _bits(t):
    return _bits_view(t.detach().contiguous()).cpu()


def _sentinel(dtype):
    return BF16_SENTINEL if dtype == BF16 else F32_SENTINEL


class Slot:
    """n elements at ``off`` bytes past a 16-B boundary of a sentinel-filled device buffer, at least ``guard`` sentinel
    elements before and after them."""

    def __init__(self, n, dtype, off=0, guard=8, data=None):
        es = 2 if dtype == BF16 else 4
        self.n, self.start = n, -(-guard // 8) * 8 + off // es
        self.buf = torch.empty(self.start + n + guard + 8, dtype=dtype, device=DEV)
        _bits_view(self.buf).fill_(_sentinel(dtype))
        if data is not None:
            self.buf[self.start:self.start + n].copy_(data.reshape(-1))
        self.ptr = self.buf.data_ptr() + es * self.start
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == off % 16
        self.before = _bits(self.buf).clone()

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.before)

    def guards_intact(self):
        now = _bits(self.buf)
        keep = torch.ones_like(now, dtype=torch.bool)
        keep[self.start:self.start + self.n] = False
        return torch.equal(now[keep], self.before[keep])

    def fully_written(self):
        return not bool((_bits(self.buf)[self.start:self.start + self.n] == _sentinel(self.buf.dtype)).any())

    def get(self, *shape):
        return self.buf[self.start:self.start + self.n].cpu().view(*shape)


# ---- inputs and their references, computed once ---------------------------------------------------------
FAMILY_SEED = {"unit": 1, "eps": 2, "offset": 3, "narrow": 4}


@functools.lru_cache(maxsize=6)
def _case(family, rows, H, rms, with_beta=True):
    """unit: randn rows at the default eps; eps: the same at eps = 0.5; offset / narrow: integers in [48, 80] /
    [240, 255]. gamma = 1 + 0.25 noise, beta = noise, dy = 0.75 xhat + 0.5 + noise, dres = noise."""
    seed = FAMILY_SEED[family] + 10 * rows + 100003 * H + (50000 if rms else 0)
    if family == "offset":
        x = R.offset_rows(rows, H, seed)
    elif family == "narrow":
        x = R.offset_rows(rows, H, seed, 240, 255)
    else:
        x = R.unit_rows(rows, H, seed)
    eps = 0.5 if family == "eps" else (1e-6 if rms else 1e-5)
    gamma, beta = R.params(H, seed + 1, with_beta and not rms)
    dy, dres = R.correlated_dy(x, eps, seed + 2, rms=rms), R.plain_dy(rows, H, seed + 3)
    f = R.forward(x, gamma, beta, eps, rms)
    b = R.backward(dy, x, gamma, f.mean, f.rstd, None, rms)
    c = SimpleNamespace(name=f"{family}-{rows}x{H}-{'rms' if rms else 'ln'}", x=x, gamma=gamma, beta=beta, dy=dy,
                        dres=dres, eps=eps, rms=rms, f=f, b=b, rows=rows, H=H)
    c.torch = _torch_fp32(c)
    return c


def _torch_fp32(c):
    """torch's own fp32 evaluation on the device against the reference, in units of each output's scale."""
    x = c.x.to(DEV).float().requires_grad_(True)
    g = c.gamma.to(DEV).float().requires_grad_(True)
    out = {}
    if c.rms:
        inv = torch.rsqrt(x.pow(2).mean(1, keepdim=True) + c.eps)
        y, rstd, params = x * inv * g, inv[:, 0], [x, g]
    else:
        b = c.beta.to(DEV).float().requires_grad_(True) if c.beta is not None else None
        y, mean, rstd = torch.native_layer_norm(x, (c.H,), g, b, c.eps)
        out["mean"] = R.rel_err(mean.reshape(-1), c.f.mean, c.x.double().abs().mean(1))
        params = [x, g] + ([b] if b is not None else [])
    out["y"] = R.rel_err(y, c.f.y, c.f.y_scale)
    out["rstd"] = R.rel_err(rstd.reshape(-1), c.f.rstd, c.f.rstd)
    grads = torch.autograd.grad(y, params, c.dy.to(DEV).float())
    out["dx"] = R.rel_err(grads[0], c.b.dx, c.b.dx_scale)
    out["dgamma"] = R.rel_err(grads[1], c.b.dgamma, c.b.dgamma_scale)
    if len(grads) > 2:
        out["dbeta"] = R.rel_err(grads[2], c.b.dbeta, c.b.dbeta_scale)
    return out


def _rows(c, n):
    """The first n rows of a case as a case of its own (rows are independent; the column sums are taken again)."""
    if n == c.rows:
        return c
    f = R.Fwd(c.f.y[:n], c.f.mean[:n], c.f.rstd[:n], c.f.xhat[:n], c.f.y_scale[:n])
    b = R.backward(c.dy[:n], c.x[:n], c.gamma, f.mean, f.rstd, None, c.rms)
    s = SimpleNamespace(name=f"{c.name}[:{n}]", x=c.x[:n], gamma=c.gamma, beta=c.beta, dy=c.dy[:n], dres=c.dres[:n],
                        eps=c.eps, rms=c.rms, f=f, b=b, rows=n, H=c.H)
    s.torch = _torch_fp32(s)
    return s


# ---- the bounds -------------------------------------------------------------------------------------------
def _check(tag, what, got, ref, scale, torch_fig=None):
    """One output against the reference under the module's bound; records and prints the figures."""
    got = got.detach().cpu()
    bf = got.dtype == BF16
    target = R.to_bf16(ref) if bf else ref
    allow = MARGIN * ALLOW[what] * scale
    bound = (R.ulp_bf16(target) + allow) if bf else allow
    err = (got.double() - target).abs()
    beyond = (err - (R.ulp_bf16(target) if bf else 0.0)).clamp(min=0)
    rel = float(torch.where(beyond == 0, torch.zeros_like(beyond), beyond / scale).max()) if err.numel() else 0.0
    if torch_fig is not None:
        FIG[("torch-fp32", what)] = max(FIG.get(("torch-fp32", what), 0.0), torch_fig)
    key = (tag.split(" ")[0], what + ("/bf16" if bf else ""))
    FIG[key] = max(FIG.get(key, 0.0), rel)
    print(f"NORM-FIG {tag} {what}{'/bf16' if bf else ''}: max_err={float(err.max()):.3e} "
          f"beyond_rounding/scale={rel:.3e} allowed={MARGIN * ALLOW[what]:.3e}"
          + (f" torch_fp32/scale={torch_fig:.3e}" if torch_fig is not None else ""))
    assert bool(torch.isfinite(got.float()).all()), (tag, what, "not finite")
    ok = err <= bound
    assert bool(ok.all()), (tag, what, "elements outside the bound", int((~ok).sum()), "first", (~ok).nonzero()[:3].tolist(),
                            "err", float(err[~ok].max()), "bound there", float(bound[~ok].min()), "rel", rel)


def _check_fwd(tag, c, out, stats=True):
    y, mean, rstd = out
    _check(tag, "y", y, c.f.y, c.f.y_scale, c.torch.get("y"))
    if stats:
        if not c.rms:
            _check(tag, "mean", mean, c.f.mean, c.x.double().abs().mean(1), c.torch.get("mean"))
        _check(tag, "rstd", rstd, c.f.rstd, c.f.rstd, c.torch.get("rstd"))


def _check_bwd(tag, c, out, dres):
    dx, dg, db = out
    ref_dx = c.b.dx + (c.dres.double() if dres else 0.0)
    _check(tag, "dx", dx, ref_dx, c.b.dx_scale, c.torch.get("dx"))
    if dg is not None:
        _check(tag, "dgamma", dg, c.b.dgamma, c.b.dgamma_scale, c.torch.get("dgamma"))
    if db is not None:
        _check(tag, "dbeta", db, c.b.dbeta, c.b.dbeta_scale, c.torch.get("dbeta"))


# ---- the C entries on buffers the test owns ---------------------------------------------------------------
def _fwd(c, path, blocks=0, stats=True, beta=True, offs=None, x=None):
    """kfamd_norm_fwd_bf16_path on sentinel-guarded buffers. Returns (y, mean, rstd) on the CPU, or None after checking
    that a KFAMD_EINVAL wrote nothing. An RMS launch is handed a NaN beta and a mean buffer, which it must ignore."""
    offs = offs or {}
    x = c.x if x is None else x
    rows, H = x.shape
    sx = Slot(rows * H, BF16, offs.get("x", 0), 8, x)
    sg = Slot(H, BF16, offs.get("gamma", 0), 8, c.gamma)
    use_beta = beta and (c.rms or c.beta is not None)
    sb = Slot(H, BF16, offs.get("beta", 0), 8, None if c.rms else c.beta) if use_beta else None
    sy = Slot(rows * H, BF16, offs.get("y", 0), GUARD * H)
    sm = Slot(rows, F32, 0, GUARD) if stats else None
    sr = Slot(rows, F32, 0, GUARD) if stats else None
    rc = _L().kfamd_norm_fwd_bf16_path(int(c.rms), path, blocks, sx.ptr, sg.ptr, sb.ptr if sb else None, sy.ptr,
                                       sm.ptr if sm else None, sr.ptr if sr else None, rows, H, c.eps, _stream())
    _sync()
    slots = [s for s in (sx, sg, sb, sy, sm, sr) if s is not None]
    if rc != 0:
        assert rc == EINVAL, rc
        assert all(s.unchanged() for s in slots), "a rejected launch wrote something"
        return None
    assert sx.unchanged() and sg.unchanged() and (sb is None or sb.unchanged()), "an input (or its padding) was written"
    assert sy.guards_intact(), "y written outside its rows"
    assert sy.fully_written() or bool(torch.isnan(x.float()).any()), "y not fully written"
    if stats:
        assert sr.guards_intact() and sr.fully_written(), "rstd written outside its rows, or not fully"
        assert sm.unchanged() if c.rms else (sm.guards_intact() and sm.fully_written()), "mean"
    return sy.get(rows, H), (sm.get(rows) if stats and not c.rms else None), (sr.get(rows) if stats else None)


def _bwd(c, path, dres=True, want=("dgamma", "dbeta"), dgb_bf16=False, offs=None, ws=True, x=None, twice=False):
    """kfamd_norm_bwd_bf16_path likewise, from the reference's statistics rounded to fp32. Returns (dx, dgamma, dbeta).
    twice: the launch is repeated on the same buffers and must give the same bits."""
    offs = offs or {}
    x = c.x if x is None else x
    rows, H = x.shape
    L = _L()
    sdy = Slot(rows * H, BF16, offs.get("dy", 0), 8, c.dy)
    sres = Slot(rows * H, BF16, offs.get("dres", 0), 8, c.dres) if dres else None
    sx = Slot(rows * H, BF16, offs.get("x", 0), 8, x)
    sg = Slot(H, BF16, offs.get("gamma", 0), 8, c.gamma)
    smean = Slot(rows, F32, 0, GUARD, c.f.mean.float())   # RMS: handed over and ignored
    srstd = Slot(rows, F32, 0, GUARD, c.f.rstd.float())
    sdx = Slot(rows * H, BF16, offs.get("dx", 0), GUARD * H)
    pdt = BF16 if dgb_bf16 else F32
    sdg = Slot(H, pdt, 0, GUARD) if "dgamma" in want else None
    sdb = Slot(H, pdt, 0, GUARD) if "dbeta" in want else None   # RMS: handed over and ignored
    nws = L.kfamd_layernorm_bwd_workspace(rows, H)
    assert nws % 4 == 0 and nws >= 2 * 4 * H * max(256, -(-rows // 64))
    sws = Slot(nws // 4, F32, 0, 64) if ws else None
    args = (int(c.rms), path, sdy.ptr, sres.ptr if sres else None, sx.ptr, sg.ptr, smean.ptr, srstd.ptr, sdx.ptr,
            sdg.ptr if sdg else None, sdb.ptr if sdb else None, int(dgb_bf16), sws.ptr if sws else None, rows, H,
            _stream())
    rc = L.kfamd_norm_bwd_bf16_path(*args)
    _sync()
    ins = [s for s in (sdy, sres, sx, sg, smean, srstd) if s is not None]
    outs = [s for s in (sdx, sdg, sdb, sws) if s is not None]
    if rc != 0:
        assert rc == EINVAL, rc
        assert all(s.unchanged() for s in ins + outs), "a rejected launch wrote something"
        return None
    assert all(s.unchanged() for s in ins), "an input (or its padding) was written"
    assert all(s.guards_intact() for s in outs), "dx / dgamma / dbeta / workspace written outside their extent"
    poisoned = bool((~torch.isfinite(x.float())).any())
    assert sdx.fully_written() or poisoned, "dx not fully written"
    assert sdg is None or sdg.fully_written() or poisoned, "dgamma not fully written"
    if c.rms:
        assert sdb is None or sdb.unchanged(), "the RMS backward wrote dbeta"
    else:
        assert sdb is None or sdb.fully_written() or poisoned, "dbeta not fully written"
    if twice:
        first = [_bits(s.buf) for s in (sdx, sdg, sdb) if s is not None]
        assert L.kfamd_norm_bwd_bf16_path(*args) == 0
        _sync()
        again = [_bits(s.buf) for s in (sdx, sdg, sdb) if s is not None]
        assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs on the same buffers differ"
    return (sdx.get(rows, H), sdg.get(H) if sdg else None, sdb.get(H) if sdb and not c.rms else None)


# ---- forward ------------------------------------------------------------------------------------------------
def _fwd_suite(rms, path, blocks, H, row_counts, families=("unit", "eps", "offset", "narrow")):
    nmax = max(row_counts)
    tag = f"fwd-{FWD_NAMES[path]}" + (f"-b{blocks}" if blocks else "")
    for fam in families:
        full = _case(fam, nmax, H, rms)
        for n in (row_counts if fam == "offset" else [nmax]):
            c = _rows(full, n)
            out = _fwd(c, path, blocks)
            assert out is not None, (tag, c.name, "KFAMD_EINVAL")
            _check_fwd(f"{tag} {c.name}", c, out)
    c = _case("unit", nmax, H, rms)
    plain = _fwd(c, path, blocks)
    nostats = _fwd(c, path, blocks, stats=False)
    assert torch.equal(_bits(nostats[0]), _bits(plain[0])), "y depends on whether the statistics are saved"
    if not rms:
        nb = _case("unit", nmax, H, rms, with_beta=False)
        _check_fwd(f"{tag} {nb.name}-nobeta", nb, _fwd(nb, path, blocks, beta=False))


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", WAVE8 + WAVE4)
def test_forward_wave_per_row_every_width(H, rms):
    """norm_fwd_wave: ten 16-byte widths (8192 with gamma / beta prefetched), three 8-byte widths; 1, 3, 4, 5 rows on
    4 rows per workgroup."""
    _fwd_suite(rms, 1, 0, H, [1, 3, 4, 5])


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", BLOCK_ONLY + [512, 768])
def test_forward_block_kernel(H, rms):
    _fwd_suite(rms, 3, 0, H, [1, 5])


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("H", [512, 4096, 8192])
def test_forward_streaming_small_grids(H, blocks, rms):
    """norm_fwd_stream on 4, 8 and 12 waves: 1 .. 41 rows leave waves without a row, end the double-buffered loop at
    its first exit (an odd number of sweeps) and at its second, and make the last sweep ragged."""
    nw = 4 * blocks
    sweeps = {-(-n // nw) for n in (1, 5, 8, 9, 37, 41)}
    assert any(s % 2 for s in sweeps) and any(s % 2 == 0 for s in sweeps) and nw > 1
    _fwd_suite(rms, 2, blocks, H, [1, 5, 8, 9, 37, 41], families=("unit", "offset", "narrow", "eps"))


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", [h for h in STREAM if h not in (512, 4096, 8192)])
def test_forward_streaming_other_widths(H, rms):
    _fwd_suite(rms, 2, 2, H, [37], families=("unit", "offset"))


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", WAVE8 + WAVE4 + BLOCK_ONLY)
def test_forward_auto_launch_names_its_path(H, rms):
    """One launch by the launcher's own rule per width; kfamd_norm_fwd_path_for says which kernel that was."""
    rows = 37
    took = _L().kfamd_norm_fwd_path_for(int(rms), rows, H)
    want = 3 if H in BLOCK_ONLY else (2 if H == 8192 else 1)  # 37 rows: below one generation; 8192 streams up to two
    assert took == want, (H, rows, "path", took, FWD_NAMES.get(took))
    for fam in ("unit", "offset"):
        c = _case(fam, rows, H, rms)
        auto = _fwd(c, 0)
        _check_fwd(f"fwd-auto(took:{FWD_NAMES[took]}) {c.name}", c, auto)
        forced = _fwd(c, took)
        for a, b, what in zip(auto, forced, ("y", "mean", "rstd")):
            assert (a is None and b is None) or torch.equal(_bits(a), _bits(b)), \
                (what, "auto differs from the forced path", FWD_NAMES[took])


def test_forward_path_for_contract():
    L = _L()
    assert L.kfamd_norm_fwd_path_for(0, 0, 512) == EINVAL and L.kfamd_norm_fwd_path_for(1, 4, 0) == EINVAL
    for rms in (0, 1):
        assert L.kfamd_norm_fwd_path_for(rms, 4, 1000) == 3 and L.kfamd_norm_fwd_path_for(rms, 4, 5120) == 1
        assert L.kfamd_norm_fwd_path_for(rms, 4, 768) == 1 and L.kfamd_norm_fwd_path_for(rms, 1, 8192) == 2
        assert L.kfamd_norm_fwd_path_for(rms, 1 << 30, 8192) == 1 and L.kfamd_norm_fwd_path_for(rms, 1 << 30, 512) == 1


# ---- backward -----------------------------------------------------------------------------------------------
def _bwd_suite(rms, path, H, row_counts, every_option_at=None):
    nmax = max(row_counts)
    tag = f"bwd-{BWD_NAMES[path]}"
    for fam in ("unit", "offset"):
        full = _case(fam, nmax, H, rms)
        for n in (row_counts if fam == "unit" else [nmax]):
            c = _rows(full, n)
            out = _bwd(c, path, dres=True, twice=(n == nmax))
            assert out is not None, (tag, c.name, "KFAMD_EINVAL")
            _check_bwd(f"{tag} {c.name}", c, out, dres=True)
            out = _bwd(c, path, dres=False, dgb_bf16=True)
            _check_bwd(f"{tag} {c.name}-nodres", c, out, dres=False)
    c = _rows(_case("unit", nmax, H, rms), every_option_at or nmax)
    for want, bf in ((("dgamma",), False), (("dbeta",), False), (("dgamma",), True), (("dbeta",), True)):
        if rms and want == ("dbeta",):
            continue
        out = _bwd(c, path, dres=True, want=want, dgb_bf16=bf)
        assert out is not None, (tag, want)
        _check_bwd(f"{tag} {c.name}-{want[0]}-only", c, out, dres=True)
    if path != 1:  # no column sums asked for: no workspace needed (the fused kernel is for the column sums)
        out = _bwd(c, path, dres=False, want=(), ws=False)
        _check_bwd(f"{tag} {c.name}-dx-only", c, out, dres=False)
    else:
        assert _bwd(c, path, dres=False, want=(), ws=True) is None


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", FUSED)
def test_backward_fused(H, rms):
    """ln_bwd_fused, seven instantiations: 8 waves per block, one row per wave at a time."""
    _bwd_suite(rms, 1, H, [1, 7, 8, 9, 300], every_option_at=9)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("rows", [2049, 2100])
@pytest.mark.parametrize("H", [256, 512])
def test_backward_fused_many_rows(H, rows, rms):
    """Above 2048 rows the grid stops at 256 blocks: 9 rows per block, so the first wave takes two and the last block
    is short."""
    c = _case("unit", rows, H, rms)
    _check_bwd(f"bwd-fused {c.name}", c, _bwd(c, 1, dres=True, twice=True), dres=True)
    _check_bwd(f"bwd-fused {c.name}-bf16", c, _bwd(c, 1, dres=False, dgb_bf16=True), dres=False)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", WAVE8 + WAVE4)
def test_backward_dx_wave_and_column_partials(H, rms):
    """ln_bwd_dx_wave (registers; packed at 8192) on 4 rows per workgroup, ln_bwd_dgb_partial on 64-row chunks and 4
    row lanes, ln_bwd_dgb_finalize (300 rows: 5 chunks, so each of its 4 chunk lanes has one)."""
    _bwd_suite(rms, 2, H, [1, 3, 4, 5, 63, 64, 65, 131, 300] if H <= 1024 else [1, 3, 4, 5, 65], every_option_at=5)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", BLOCK_ONLY + [512, 768])
def test_backward_dx_block_and_column_partials(H, rms):
    """ln_bwd_dx_block; hidden 7 and 1000 put the column strip's edge (64 columns per block) inside a block."""
    _bwd_suite(rms, 3, H, [1, 63, 64, 65, 131, 300] if H in (7, 1000) else [1, 5, 65], every_option_at=5)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", [512, 768, 2048, 4096, 1000])
def test_backward_auto_is_one_of_the_forced_paths(H, rms):
    c = _case("unit", 9, H, rms)
    auto = _bwd(c, 0, dres=True)
    _check_bwd(f"bwd-auto {c.name}", c, auto, dres=True)
    want = 1 if H in FUSED else (2 if H == 4096 else 3)
    if os.environ.get("KFAMD_LN_BWD_SPLIT") == "1" and want == 1:
        want = 2
    forced = _bwd(c, want, dres=True)
    for a, b in zip(auto, forced):
        assert (a is None and b is None) or torch.equal(_bits(a), _bits(b)), ("auto differs from", BWD_NAMES[want])


# ---- alignment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("off", [2, 4, 8])
@pytest.mark.parametrize("H", [512, 768, 2048])
def test_pointers_off_the_vector_grid(H, off, rms):
    """Each operand in turn 2, 4 or 8 bytes off the 16-byte grid: 8 bytes off at hidden 768 stays on the 8-byte wave
    kernels, everything else falls to the block kernels (the wave, streaming and fused paths refuse), same bounds."""
    c = _case("unit", 5, H, rms)
    wave_ok = H == 768 and off == 8
    for which in ("x", "gamma", "beta", "y"):
        if rms and which == "beta":
            continue
        offs = {which: off}
        tag = f"fwd-auto-{which}+{off} {c.name}"
        _check_fwd(tag, c, _fwd(c, 0, offs=offs))
        assert (_fwd(c, 1, offs=offs) is not None) == wave_ok, (tag, "forced wave path")
        assert _fwd(c, 2, offs=offs) is None, (tag, "forced streaming path")
        _check_fwd(tag + "-block", c, _fwd(c, 3, offs=offs))
    for which in ("dy", "dres", "x", "gamma", "dx"):
        offs = {which: off}
        tag = f"bwd-auto-{which}+{off} {c.name}"
        _check_bwd(tag, c, _bwd(c, 0, offs=offs), dres=True)
        assert (_bwd(c, 1, offs=offs) is not None) == wave_ok, (tag, "forced fused path")
        assert (_bwd(c, 2, offs=offs) is not None) == wave_ok, (tag, "forced dx wave path")
        if which == "dres":  # without a dres its alignment cannot matter
            assert _bwd(c, 2, offs=offs, dres=False) is not None


# ---- degenerate and poisoned rows ----------------------------------------------------------------------------
FWD_PATHS_AT = {512: [(1, 0), (2, 1), (3, 0)], 768: [(1, 0), (3, 0)], 8192: [(1, 0), (2, 1), (3, 0)], 1: [(3, 0)],
                7: [(3, 0)]}
BWD_PATHS_AT = {512: [1, 2, 3], 768: [1, 2, 3], 8192: [2, 3], 1: [3], 7: [3]}


@pytest.mark.parametrize("H", [512, 768, 8192, 7])
def test_constant_rows_give_beta_exactly(H):
    """Variance 0: y is bf16(beta) exactly (the two-pass mean of a constant row is that constant), rstd = 1 / sqrt(eps),
    dx finite and inside the bound."""
    c = _case("unit", 5, H, False)
    x = c.x.clone()
    x[1], x[3] = 3.0, -80.0
    f = R.forward(x, c.gamma, c.beta, c.eps)
    b = R.backward(c.dy, x, c.gamma, f.mean, f.rstd, None)
    cc = SimpleNamespace(**{**c.__dict__, "x": x, "f": f, "b": b, "name": c.name + "-const"})
    cc.torch = _torch_fp32(cc)
    for path, blocks in FWD_PATHS_AT[H]:
        y, mean, rstd = _fwd(cc, path, blocks)
        for r in (1, 3):
            assert torch.equal(y[r].float(), c.beta.float()), (FWD_NAMES[path], "row", r)
            assert float(mean[r]) == float(x[r, 0])
        _check_fwd(f"fwd-{FWD_NAMES[path]} {cc.name}", cc, (y, mean, rstd))
    for path in BWD_PATHS_AT[H]:
        _check_bwd(f"bwd-{BWD_NAMES[path]} {cc.name}", cc, _bwd(cc, path, dres=True), dres=True)


@pytest.mark.parametrize("H", [512, 768, 8192, 7])
def test_all_zero_rows_under_rmsnorm(H):
    c = _case("unit", 5, H, True)
    x = c.x.clone()
    x[0], x[4] = 0.0, 0.0
    f = R.forward(x, c.gamma, None, c.eps, True)
    b = R.backward(c.dy, x, c.gamma, None, f.rstd, None, True)
    cc = SimpleNamespace(**{**c.__dict__, "x": x, "f": f, "b": b, "name": c.name + "-zero"})
    cc.torch = _torch_fp32(cc)
    for path, blocks in FWD_PATHS_AT[H]:
        out = _fwd(cc, path, blocks)
        assert bool((out[0][0] == 0).all()) and bool((out[0][4] == 0).all())
        _check_fwd(f"fwd-{FWD_NAMES[path]} {cc.name}", cc, out)
    for path in BWD_PATHS_AT[H]:
        _check_bwd(f"bwd-{BWD_NAMES[path]} {cc.name}", cc, _bwd(cc, path, dres=True), dres=True)


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_hidden_one(rms):
    """LayerNorm: xhat = 0, y = beta, dx = dres; RMSNorm: y = x / sqrt(x^2 + eps) * gamma."""
    c = _case("unit", 5, 1, rms)
    out = _fwd(c, 3)
    _check_fwd(f"fwd-block {c.name}", c, out)
    if not rms:
        assert torch.equal(out[0].float(), c.beta.float().expand(5, 1))
    got = _bwd(c, 3, dres=True)
    _check_bwd(f"bwd-dxblock+partials {c.name}", c, got, dres=True)
    if not rms:
        assert torch.equal(_bits(got[0]), _bits(c.dres))
    assert _fwd(c, 1) is None and _fwd(c, 2) is None and _bwd(c, 1) is None and _bwd(c, 2) is None


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("H", [512, 768, 8192, 7])
def test_a_poisoned_row_touches_no_other(H, rms):
    """A NaN in row 2 and +inf in row 5 of 9: every other row's y, mean, rstd and dx keeps its bits; forward, a row run
    as a batch of one on the same path gives the same bits."""
    c = _case("unit", 9, H, rms)
    bad = c.x.clone()
    bad[2, H // 3], bad[5, H - 1] = float("nan"), float("inf")
    keep = torch.tensor([r not in (2, 5) for r in range(9)])
    for path, blocks in FWD_PATHS_AT[H]:
        clean, dirty = _fwd(c, path, blocks), _fwd(c, path, blocks, x=bad)
        for a, b, what in zip(clean, dirty, ("y", "mean", "rstd")):
            if a is not None:
                assert torch.equal(_bits(a)[keep], _bits(b)[keep]), (FWD_NAMES[path], what)
        assert bool(torch.isnan(dirty[0][2].float()).all())
        for r in (0, 8):
            one = _fwd(_rows(c, 9), path, blocks, x=c.x[r:r + 1])
            assert torch.equal(_bits(one[0][0]), _bits(clean[0][r])), (FWD_NAMES[path], "row", r, "alone")
            assert torch.equal(_bits(one[2]), _bits(clean[2][r:r + 1]))
    for path in BWD_PATHS_AT[H]:
        clean, dirty = _bwd(c, path, dres=True), _bwd(c, path, dres=True, x=bad)
        assert torch.equal(_bits(clean[0])[keep], _bits(dirty[0])[keep]), (BWD_NAMES[path], "dx")


# ---- contract of the forcing entries -------------------------------------------------------------------------
def test_impossible_paths_are_rejected_and_write_nothing():
    for rms in (False, True):
        for H in (1000, 3584, 8200):
            c = _case("unit", 5, H, rms)
            assert _fwd(c, 1) is None and _fwd(c, 2) is None and _bwd(c, 1) is None and _bwd(c, 2) is None
        for H in (768, 5120, 6144):  # wave widths that do not stream; 5120 / 6144 do not fuse either
            c = _case("unit", 5, H, rms)
            assert _fwd(c, 2) is None and _fwd(c, 1) is not None
            assert (_bwd(c, 1) is None) == (H != 768)
        c = _case("unit", 5, 512, rms)
        for path in (-1, 4):
            assert _fwd(c, path) is None and _bwd(c, path) is None
        assert _fwd(c, 2, blocks=-1) is None
        assert _bwd(c, 1, want=()) is None          # fused without a column sum to write
        assert _bwd(c, 2, ws=False) is None         # column sums without a workspace


# ---- the ops through autograd ----------------------------------------------------------------------------------
def _through_op(kind, H, param_dtype, with_bias=True):
    from kubeflow_rm_amd import ops
    rms = kind.startswith("rms")
    c = _case("unit", 6, H, rms, with_beta=with_bias)
    x = c.x.view(2, 3, H).to(DEV).requires_grad_(True)
    w = c.gamma.to(DEV).to(param_dtype).requires_grad_(True)
    b = c.beta.to(DEV).to(param_dtype).requires_grad_(True) if c.beta is not None else None
    gy, gres = c.dy.view(2, 3, H).to(DEV), c.dres.view(2, 3, H).to(DEV)
    residual = kind.endswith("residual")
    fn = getattr(ops, kind)
    out = fn(x, w, c.eps) if rms else fn(x, w, b, c.eps)
    if residual:
        y, r = out
        assert torch.equal(_bits(r), _bits(c.x.view(2, 3, H)))
        torch.autograd.backward((y, r), (gy, gres))
    else:
        y = out
        y.backward(gy)
    _sync()
    assert y.shape == x.shape and y.dtype == BF16 and x.grad.shape == x.shape and x.grad.dtype == BF16
    assert w.grad.dtype == param_dtype and (b is None or b.grad.dtype == param_dtype)
    tag = f"op-{kind}-{str(param_dtype).split('.')[-1]}"
    _check(f"{tag} {c.name}", "y", y.reshape(6, H), c.f.y, c.f.y_scale)
    _check_bwd(f"{tag} {c.name}", c, (x.grad.reshape(6, H), w.grad, b.grad if b is not None else None), dres=residual)


@pytest.mark.parametrize("H", [768, 2048, 4096, 1000])
@pytest.mark.parametrize("kind", ["layer_norm", "layer_norm_residual"])
def test_op_layer_norm(kind, H):
    _through_op(kind, H, BF16)
    _through_op(kind, H, BF16, with_bias=False)


@pytest.mark.parametrize("H", [768, 2048, 4096, 1000])
@pytest.mark.parametrize("param_dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["rms_norm", "rms_norm_residual"])
def test_op_rms_norm(kind, param_dtype, H):
    """An fp32 weight is rounded to bf16 once (exact here: the values are bf16) and gets an fp32 gradient."""
    _through_op(kind, H, param_dtype)


def test_op_rejects_a_bias_or_weight_the_kernel_cannot_read():
    from kubeflow_rm_amd import ops
    c = _case("unit", 5, 512, False)
    x, w, b = c.x.to(DEV), c.gamma.to(DEV), c.beta.to(DEV)
    with pytest.raises(TypeError):
        ops.layer_norm(x, w, b.float())
    with pytest.raises(ValueError):
        ops.layer_norm(x, w, c.beta)          # a CPU bias
    with pytest.raises(TypeError):
        ops.layer_norm_fwd(x, w, b.float())
    with pytest.raises(TypeError):
        ops.rms_norm_fwd(x, w.float())
    with pytest.raises(ValueError):
        ops.rms_norm_fwd(x, c.gamma)          # a CPU weight
    with pytest.raises(TypeError):
        ops.layer_norm(x, w.float(), b)
    assert ops.layer_norm(x, w, None).shape == x.shape


def test_op_zero_rows_raise():
    """What an empty batch does today: the kernels' rows >= 1 contract surfaces as the library's error."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops._lib import NativeLibraryError
    c = _case("unit", 5, 512, False)
    x0 = torch.empty(0, 512, dtype=BF16, device=DEV)
    w, b = c.gamma.to(DEV), c.beta.to(DEV)
    for call in (lambda: ops.layer_norm(x0, w, b), lambda: ops.layer_norm_fwd(x0, w, b), lambda: ops.rms_norm(x0, w),
                 lambda: ops.rms_norm_fwd(x0, w), lambda: ops.layer_norm_residual(x0, w, b),
                 lambda: ops.rms_norm_residual(x0, w)):
        with pytest.raises(NativeLibraryError):
            call()


def test_zz_figures():
    """Prints the largest figure per path and output of the whole run (``pytest -s``)."""
    for key in sorted(FIG):
        print(f"NORM-SUM {key[0]:28s} {key[1]:12s} {FIG[key]:.3e}")
