"""Flash attention (kernels/attention_bf16.hip) row by row: masks, tile edges, stray writes.

tests/test_gpu_attention.py judges the training kernels by one norm over a whole tensor of random
inputs, into ``torch.empty`` outputs. Here every row is judged on its own, against torch in fp32 /
fp64 with an explicit ``S = scale * q k^T``, the mask, ``softmax`` and autograd on the same
bf16-rounded inputs:

1. steep-ramp inputs make every row's softmax geometric in the key index, so a mask that is off by
   one key moves every row far past the bound (checked on the reference alone, in the test);
2. inputs and outputs are carved out of NaN-filled buffers: every output row below T is written,
   no guard row is written, no guard row of an input is used;
3. per-row errors on random inputs (``scale_in`` 1 and 4) at T in {1 .. 321} around every tile edge;
4. two calls agree bit for bit (the backward is atomic-free);
5. mixed layouts through the autograd entry point, and contract violations that must raise.

Bounds. Forward: ``|o - ref| <= 2^-7 max|v|`` elementwise: o is a convex combination of v rows; the
bf16 roundings of P and of O and the mismatch between the fp32 row sum and the bf16 P cost at most
2^-9 each, one more 2^-9 allows for fp32 order and exp2. ``lse`` to 1e-3. Backward, per row
(b, h, t): ``|got - ref|_2 / max(|ref|_2, median row norm of ref)`` within 4x the largest such
value of a torch emulation of the algorithm's roundings (``_emulate``) against fp64, for that tensor
and case, and never more than 5e-2; the factor 4 allows for accumulation order, v_exp_f32 and the
fp32 lse. For dq and dk the denominator has a third term, 4 / 5e-2 times the row's unavoidable
rounding noise (``_Ref._noise``): where the softmax is nearly one-hot the exact row cancels to far
below what the bf16 O and dS leave in it, and without that term the emulation alone is off by up to
2.7 (dq) and 0.4 (dk) per row at 4 * randn inputs. That 4x the emulation's error needs no cap is
asserted for dv; for dq and dk it does not hold (the emulation reaches 0.017, 0.03 along the ramp),
so there the tolerance is the cap itself. Where the reference is identically zero (T = 1: one key,
dS = 0, so dq = dk = 0) the ratio is undefined, and the rows are held to the absolute bound of
``_zero_ref_bound`` instead.

lse has no guard rows between (b, h) slices (it is contiguous [B, H, T]): only the end of the
allocation is guarded. A write past row T of one slice lands in the next slice and shows only if it
survives there: one that the right value overwrites later is not seen.
"""
from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 24          # guard rows behind every tensor of the poisoned-buffer tests
TOL_CAP = 5e-2
NAMES = ("dq", "dk", "dv")
NAN = float("nan")

# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _randn_inputs(B, H, T, D, seed, scale_in=1.0, device=DEV):
    """q, k, v (randn * scale_in) and do (randn), bf16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q, k, v = (torch.randn(B, H, T, D, generator=g) * scale_in for _ in range(3))
    do = torch.randn(B, H, T, D, generator=g)
    return [x.to(device, torch.bfloat16) for x in (q, k, v, do)]


RAMP_SCALE = 0.125


def _ramp_inputs(B, H, T, D, seed, causal, device=DEV):
    """Scaled score of (query, key j) ~ j (causal) or -(j + 50) (non-causal): adjacent keys are one
    nat apart, so each row's weight sits on the last few keys its mask lets through."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q, k = (0.05 * torch.randn(B, H, T, D, generator=g) for _ in range(2))
    v, do = (torch.randn(B, H, T, D, generator=g) for _ in range(2))
    j = torch.arange(T, dtype=torch.float32)
    q[..., 0] = 8.0
    k[..., 0] = j if causal else -(j + 50.0)
    return [x.to(device, torch.bfloat16) for x in (q, k, v, do)]


# ------------------------------------------------------------------------------------------------
# references (run on the inputs' device; the CPU serves to check seeds without a GPU)
# ------------------------------------------------------------------------------------------------
def _reference(q, k, v, do, scale, causal, dtype=torch.float32, leak=False):
    """o, lse, dq, dk, dv by autograd in ``dtype``. ``leak``: the mask off by one key: causal
    key <= query + 1; non-causal key < T + 1 with one zero key (and value) row appended."""
    qf, kf, vf = (x.detach().to(dtype).requires_grad_(True) for x in (q, k, v))
    B, H, T, D = q.shape
    kk, vv = kf, vf
    if leak and not causal:
        z = torch.zeros(B, H, 1, D, dtype=dtype, device=q.device)
        kk, vv = torch.cat([kf, z], 2), torch.cat([vf, z], 2)
    s = scale * (qf @ kk.transpose(-1, -2))
    if causal:
        t = torch.arange(T, device=q.device)
        s = s.masked_fill(t[None, :] > t[:, None] + (1 if leak else 0), float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.softmax(s, -1) @ vv
    o.backward(do.to(dtype))
    return o.detach(), lse.detach(), qf.grad, kf.grad, vf.grad


def _emulate(q, k, v, do, scale, causal):
    """dq, dk, dv with the kernels' roundings: fp32 S and lse; P in bf16 before P V and dO^T P;
    delta from the bf16 O; dS = P (dP - delta) in bf16 before the dK / dQ products; bf16 outputs."""
    qf, kf, vf, dof = (x.float() for x in (q, k, v, do))
    T = q.shape[2]
    s = scale * (qf @ kf.transpose(-1, -2))
    if causal:
        t = torch.arange(T, device=q.device)
        s = s.masked_fill(t[None, :] > t[:, None], float("-inf"))
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    pb = p.bfloat16().float()
    o = (pb @ vf).bfloat16().float()
    delta = (dof * o).sum(-1, keepdim=True)
    ds = (p * (dof @ vf.transpose(-1, -2) - delta)).bfloat16().float()
    dv = pb.transpose(-1, -2) @ dof
    dk = scale * (ds.transpose(-1, -2) @ qf)
    dq = scale * (ds @ kf)
    return [x.bfloat16() for x in (dq, dk, dv)]


def _row_err(got, ref, noise=None):
    """Per row (b, h, t): |got - ref|_2 / max(|ref|_2, median row norm of ref[, 4 / TOL_CAP noise]).
    ``noise``: _Ref.noise, the size of the rounding the algorithm cannot avoid in that row. [B, H, T]"""
    g, r = got.double(), ref.double()
    rn = r.norm(dim=-1)
    den = torch.maximum(rn, rn.median())
    if noise is not None:
        den = torch.maximum(den, noise.double() * (4 / TOL_CAP))
    return (g - r).norm(dim=-1) / den.clamp_min(1e-300)


def _zero_ref_bound(name, q, k, v, do, scale):
    """Row-norm bound for a gradient whose reference is identically zero (T = 1). dS = P (dP - delta)
    with dP = do . v and delta = do . o two fp32 dot products of D terms that cancel: what is left is
    at most D 2^-23 |do| |v| <= 2^-16 |do| |v|; times scale |k| (dq) or scale |q| (dk). 2^-12 of
    that natural size leaves 16x for the order of the sums and is far below one bf16 step (2^-8)
    of any gradient that is not zero."""
    other = k if name == "dq" else q
    nat = scale * do.float().norm(dim=-1).max() * v.float().norm(dim=-1).max() * other.float().norm(dim=-1).max()
    return 2.0 ** -12 * nat.item()


class _Ref:
    """The references of one case, computed once: fp32 (what the kernels are compared with), the
    rounding noise of every dq / dk row, and the backward tolerances from the emulation against fp64."""

    def __init__(self, q, k, v, do, scale, causal, ramp=False):
        self.args = (q, k, v, do)
        self.scale, self.causal = scale, causal
        self.o, self.lse, self.dq, self.dk, self.dv = _reference(q, k, v, do, scale, causal)
        r64 = dict(zip(NAMES, _reference(q, k, v, do, scale, causal, torch.float64)[2:]))
        emu = dict(zip(NAMES, _emulate(q, k, v, do, scale, causal)))
        # what is judged: (label, tensor, columns). The ramp inputs put 8 and the key index j into
        # coordinate 0 of q and k. Along it dq[t, 0] = scale sum_j dS[t, j] j with sum_j dS[t, j] = 0
        # exactly, so the bf16 rounding of dS leaves about 2^-9 T times the value, and dk[j, 0] =
        # sum_t dS[t, j] is one scalar that cancels by chance: coordinate 0 is judged against that
        # noise (below) and cannot see a leaked key. Coordinates 1.. (D - 1 random directions, as
        # well-conditioned as random inputs) are judged on their own, and do see it: _leak_visible.
        self.parts = []
        for name in NAMES:
            if ramp and name != "dv":
                self.parts += [(f"{name}[1:]", name, slice(1, None)), (f"{name}[0]", name, slice(0, 1))]
            else:
                self.parts.append((name, name, slice(None)))
        self._noise_terms()
        self.floor, self.zero, self.noise = {}, {}, {}
        for label, name, cols in self.parts:
            self.noise[label] = self._noise(name, cols)
            self.zero[label] = not bool(r64[name][..., cols].any())
            self.floor[label] = 0.0 if self.zero[label] else self.row_err(label, emu[name], r64[name]).max().item()
        del self._p, self._p2, self._ds2, self._a2
        self.fwd_bound = 2.0 ** -7 * v.float().abs().max().item()

    def _noise_terms(self):
        """P^2, dS^2 [B, H, T, T] and a^2 = |do o|_2^2 [B, H, T, 1] (elementwise product) in fp32."""
        q, k, v, do = (x.float() for x in self.args)
        T = q.shape[2]
        s = self.scale * (q @ k.transpose(-1, -2))
        if self.causal:
            t = torch.arange(T, device=q.device)
            s = s.masked_fill(t[None, :] > t[:, None], float("-inf"))
        p = torch.softmax(s, -1)
        ds = p * (do @ v.transpose(-1, -2) - (do * self.o).sum(-1, keepdim=True))
        self._p, self._p2, self._ds2 = p, p * p, ds * ds
        self._a2 = ((do * self.o) ** 2).sum(-1, keepdim=True)

    def _noise(self, name, cols):
        """One-sigma size, per row, of what two roundings no bf16 flash backward avoids leave in dq /
        dk: O is stored in bf16, so delta = sum_d do o is off by about 2^-9 |do o|_2 =: 2^-9 a_t, which
        dS = P (dP - delta) carries into dq[t] = -scale ddelta_t (P k)[t] and, independently per t,
        into dk[j] = -scale sum_t P[t, j] ddelta_t q[t]; and dS enters the dQ / dK products in bf16,
        each entry off by up to 2^-9 of itself, independently. Where the softmax is nearly one-hot
        (or along the ramp) the exact row cancels to far below this, and the issue's ratio to the
        row's own norm or the median measures the noise, not the kernel. _row_err therefore judges
        a row against at least 4 / TOL_CAP times its noise: what cannot be avoided then counts for
        TOL_CAP / 4 at the most, and everything else as the issue sets it."""
        if name == "dv":
            return None
        q, k = (x.float()[..., cols] for x in self.args[:2])
        if name == "dq":
            via_delta = self._a2.squeeze(-1) * (self._p @ k).pow(2).sum(-1)
            via_ds = self._ds2 @ k.pow(2).sum(-1, keepdim=True)
        else:
            qn2 = q.pow(2).sum(-1, keepdim=True)
            via_delta = self._p2.transpose(-1, -2) @ (self._a2 * qn2)
            via_ds = self._ds2.transpose(-1, -2) @ qn2
            via_delta = via_delta.squeeze(-1)
        return 4 * self.scale * 2.0 ** -9 * (via_delta + via_ds.squeeze(-1)).sqrt()

    def row_err(self, label, got, ref):
        cols = next(p[2] for p in self.parts if p[0] == label)
        return _row_err(got[..., cols], ref[..., cols], self.noise[label])

    def tol(self, label):
        if label == "dv":  # the cap is never needed; for dq and dk it is (module docstring), and holds
            assert 4 * self.floor[label] <= TOL_CAP, (label, self.floor[label])
        return min(4 * self.floor[label], TOL_CAP)

    def check_fwd(self, o, lse, what):
        assert o.dtype == torch.bfloat16 and torch.isfinite(o.float()).all(), what
        err = (o.float() - self.o).abs().max().item()
        lerr = (lse - self.lse).abs().max().item()
        print(f"EDGE {what} o: max-abs {err:.3e} bound {self.fwd_bound:.3e}; lse: max-abs {lerr:.3e}")
        assert torch.isfinite(lse).all(), what
        assert err <= self.fwd_bound, (what, err, self.fwd_bound)
        assert lerr < 1e-3, (what, lerr)

    def check_bwd(self, grads, what):
        got_by_name = dict(zip(NAMES, grads))
        for label, name, cols in self.parts:
            got = got_by_name[name]
            assert got.dtype == torch.bfloat16 and torch.isfinite(got.float()).all(), (what, name)
            if self.zero[label]:
                worst, bound = got.float().norm(dim=-1).max().item(), _zero_ref_bound(name, *self.args, self.scale)
                print(f"EDGE {what} {label}: zero reference, max row norm {worst:.3e} bound {bound:.3e}")
                assert worst <= bound, (what, label, worst, bound)
                continue
            worst, tol = self.row_err(label, got, getattr(self, name)).max().item(), self.tol(label)
            print(f"EDGE {what} {label}: floor {self.floor[label]:.3e} worst {worst:.3e} "
                  f"ratio {worst / max(self.floor[label], 1e-300):.2f}")
            assert worst <= tol, (what, label, worst, tol)


def _leak_visible(ref: _Ref):
    """On the references alone: the mask off by one key moves every row of o and dv it can reach by
    at least 10x the bound the kernels are held to (of dq and dk: half the rows by 10x, 95 % past the
    bound), so these inputs cannot hide that bug. Causal: rows below
    T - 1 of o and dq (row T - 1 has no key T to leak) and key rows from 1 up of dk and dv (key 0 is
    in every row's mask already). Non-causal: the leaked zero key takes all the weight, every row of
    o and dq moves by its own size; of dk and dv the rows that carry weight (row norm at least the
    largest row's 2^-20: key j holds e^-j of it, later rows are below any bound in both references)."""
    q, k, v, do = ref.args
    T = q.shape[2]
    lo, _, ldq, ldk, ldv = _reference(q, k, v, do, ref.scale, ref.causal, leak=True)
    rows = slice(0, T - 1) if ref.causal else slice(0, T)
    move = (lo - ref.o).abs().amax(-1)[..., rows]
    assert move.min().item() >= 10 * ref.fwd_bound, ("o", move.min().item(), ref.fwd_bound)
    leaked = dict(zip(NAMES, (ldq, ldk, ldv)))
    for label, name, cols in ref.parts:
        if label.endswith("[0]"):  # the ramp coordinate of dq / dk: judged against its noise, blind to a leak
            continue
        want = getattr(ref, name)
        move = ref.row_err(label, leaked[name], want)
        if name == "dq":
            move = move[..., rows]
        elif ref.causal:
            move = move[..., 1:]
        else:
            rn = want[..., cols].norm(dim=-1)
            move = move[rn >= 2.0 ** -20 * rn.max()]
        print(f"EDGE leak {label}: moves rows by {move.min().item() / ref.tol(label):.1f}x (least), "
              f"{move.median().item() / ref.tol(label):.1f}x (median) the tolerance {ref.tol(label):.3e}")
        assert move.numel() > 0, label
        if name == "dv":
            assert move.min().item() >= 10 * ref.tol(label), (label, move.min().item(), ref.tol(label))
        else:
            # a single row's dS can move little by chance (whatever the seed, a few rows in a
            # thousand stay within the tolerance): 95 % of the rows move past it, and half of them by 10x
            q05 = torch.quantile(move.flatten().float(), 0.05).item()
            print(f"EDGE leak {label}: 5th percentile {q05 / ref.tol(label):.1f}x")
            assert q05 >= ref.tol(label), (label, q05, ref.tol(label))
            assert move.median().item() >= 10 * ref.tol(label), (label, move.median().item(), ref.tol(label))


# ------------------------------------------------------------------------------------------------
# kernel calls
# ------------------------------------------------------------------------------------------------
def _fwd_into(q, k, v, o, lse, causal, scale):
    """ops.attention._fwd with the caller's lse buffer ([B, H, T] f32, contiguous)."""
    from kubeflow_rm_amd.ops import _lib, attention as A
    B, H, T, D = q.shape
    rc = _lib.lib().kfamd_attn_fwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                        B, H, T, D, float(scale), int(causal), A._strides(q, k, v, o), A._stream_ptr(q))
    _lib.check(rc, f"attn_fwd[B={B} H={H} T={T} D={D}]")


def _carve(B, H, T, D, layout, src=None):
    """A [B, H, T, D] view with GUARD more rows behind every (b, h) slice, out of a NaN-filled
    [B, H, T + GUARD, D] or (permuted) [B, T + GUARD, H, D] buffer. Returns (view, guard rows)."""
    if layout == "bhtd":
        buf = torch.full((B, H, T + GUARD, D), NAN, device=DEV, dtype=torch.bfloat16)
    else:
        buf = torch.full((B, T + GUARD, H, D), NAN, device=DEV, dtype=torch.bfloat16).permute(0, 2, 1, 3)
    view, guard = buf[:, :, :T], buf[:, :, T:]
    if src is not None:
        view.copy_(src)
    return view, guard


def _run_poisoned(q, k, v, do, causal, scale, layout):
    """Forward and backward with every tensor carved out of a NaN-filled buffer. Returns
    (o, lse, (dq, dk, dv)) and asserts that every guard row is still NaN."""
    from kubeflow_rm_amd.ops import attention as A
    B, H, T, D = q.shape
    ins = [_carve(B, H, T, D, layout, x) for x in (q, k, v, do)]
    outs = [_carve(B, H, T, D, layout) for _ in range(4)]  # o, dq, dk, dv
    lse_buf = torch.full((B * H * (T + GUARD),), NAN, device=DEV, dtype=torch.float32)
    lse = lse_buf[:B * H * T].view(B, H, T)
    (qv, _), (kv, _), (vv, _), (dov, _) = ins
    (o, _), (dq, _), (dk, _), (dv, _) = outs
    _fwd_into(qv, kv, vv, o, lse, causal, scale)
    A._bwd(qv, kv, vv, o, dov, lse, dq, dk, dv, causal, scale)
    torch.cuda.synchronize()
    for name, (_, guard) in zip(("q", "k", "v", "do", "o", "dq", "dk", "dv"), ins + outs):
        assert torch.isnan(guard).all(), f"{name}: a guard row past T was written ({layout})"
    assert torch.isnan(lse_buf[B * H * T:]).all(), f"lse: written past its end ({layout})"
    return o, lse, (dq, dk, dv)


def _fwd_grid(B, H, T, D, causal):
    """(kernel, paired, grid) of the forward launcher (kfamd_attn_fwd_bf16): attn_fwd_pp (256 query
    rows per workgroup) at D = 128 where its grid fills the device's compute units, else attn_fwd
    (128 rows); causal passes with an even number of query blocks run two blocks per workgroup.
    A copy of the rule in kfamd_attn_fwd_bf16 (kernels/attention_bf16.hip: nq, nq4, pair4, g4 and the
    ``g4 >= device_cus()`` branch): if the launcher's rule changes, change this with it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nq, nq4 = (T + 127) // 128, (T + 255) // 256
    pair4 = causal and nq4 % 2 == 0
    g4 = (nq4 // 2 if pair4 else nq4) * H * B
    if D == 128 and g4 >= cus:
        return "attn_fwd_pp", pair4, g4
    pair = causal and nq % 2 == 0
    return "attn_fwd", pair, (nq // 2 if pair else nq) * H * B


# ------------------------------------------------------------------------------------------------
# 1. steep-ramp masks
# ------------------------------------------------------------------------------------------------
def _ramp_case(B, H, T, D, causal, seed, kernel, paired):
    q, k, v, do = _ramp_inputs(B, H, T, D, seed, causal)
    ref = _Ref(q, k, v, do, RAMP_SCALE, causal, ramp=True)
    _leak_visible(ref)
    got = _fwd_grid(B, H, T, D, causal)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if kernel == "attn_fwd_pp":  # the path taken is a checked fact: the launcher's rule, on this device
        nq4 = (T + 255) // 256
        assert cus <= (nq4 // 2 if paired else nq4) * H * B
    assert got[:2] == (kernel, paired), (got, cus)
    what = f"ramp[{B}x{H}x{T}x{D} {'causal' if causal else 'full'} {got[0]}{' paired' if got[1] else ''} grid {got[2]}]"
    o, lse, grads = _run_poisoned(q, k, v, do, causal, RAMP_SCALE, "bhtd")
    ref.check_fwd(o, lse, what)
    ref.check_bwd(grads, what)


# seeds: any for which _leak_visible holds (it is asserted, on the references, in every run)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,T,paired", [(3, 200, True), (3, 321, False), (8, 321, False)])
def test_ramp_causal_mask_every_row(H, T, paired, D):
    """Causal diagonal tiles of every query block (T = 200: two blocks in one workgroup; 321: three
    blocks and a partial tail; H = 8: the longest-first block order)."""
    _ramp_case(1, H, T, D, True, 11 + T + D + H, "attn_fwd", paired)


@pytest.mark.parametrize("T,paired,seed", [(300, True, 305), (600, False, 606)])
def test_ramp_causal_mask_fwd_pp(T, paired, seed):
    """attn_fwd_pp (256 heads fill the device): T = 300 pairs its two 256-row blocks, the last one
    partial; T = 600 is three blocks, unpaired."""
    _ramp_case(2, 128, T, 128, True, seed, "attn_fwd_pp", paired)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [40, 65, 129])
def test_ramp_key_tail_mask(T, D):
    """Non-causal: every real score is <= -50, so a zero-filled key past T that escapes the
    key >= T mask (score 0) would take all the weight."""
    _ramp_case(1, 3, T, D, False, 23 + T + D, "attn_fwd", False)


# ------------------------------------------------------------------------------------------------
# 2 + 3. poisoned buffers and per-row error on random inputs
# ------------------------------------------------------------------------------------------------
EDGE_T = [1, 31, 33, 63, 65, 127, 129, 191, 257, 321]
EDGE_CASES = [(2, 3, T, D, causal) for D in (64, 128) for causal in (True, False) for T in EDGE_T]
EDGE_CASES += [(1, 8, 321, 64, True), (1, 8, 321, 128, True)]  # (B H) % 8 == 0: the longest-first block order


@pytest.mark.parametrize("B,H,T,D,causal", EDGE_CASES)
def test_rows_written_guards_untouched_and_per_row_error(B, H, T, D, causal):
    """Every row below T of o, lse, dq, dk, dv is written (NaN-prefilled outputs come back finite)
    and right to the per-row bounds; no row past T is written; NaN rows past T of the inputs are
    never used. Both storage orders; randn inputs and 4 * randn (a near-one-hot softmax)."""
    scale = 1.0 / math.sqrt(D)
    for scale_in in (1.0, 4.0):
        q, k, v, do = _randn_inputs(B, H, T, D, seed=1000 * int(scale_in) + 2 * T + D + int(causal), scale_in=scale_in)
        ref = _Ref(q, k, v, do, scale, causal)
        for layout in ("bhtd", "bthd"):
            what = f"rows[{B}x{H}x{T}x{D} {'causal' if causal else 'full'} x{scale_in:g} {layout}]"
            o, lse, grads = _run_poisoned(q, k, v, do, causal, scale, layout)
            ref.check_fwd(o, lse, what)
            ref.check_bwd(grads, what)


# ------------------------------------------------------------------------------------------------
# 4. bitwise repeatability
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,T,D", [(2, 3, 321, 64), (2, 3, 321, 128), (2, 128, 300, 128)])
def test_two_calls_agree_bit_for_bit(B, H, T, D):
    """No atomics anywhere in the forward or the backward: a second call on the same inputs, into
    other buffers, gives the same bits (a race between the LDS buffers would not)."""
    from kubeflow_rm_amd.ops import attention as A
    q, k, v, do = _randn_inputs(B, H, T, D, seed=T + D + H)
    scale = 1.0 / math.sqrt(D)
    if H == 128:
        assert _fwd_grid(B, H, T, D, True)[:2] == ("attn_fwd_pp", True)

    def call():
        o, dq, dk, dv = (A._bhtd(torch.full((B, T, H, D), NAN, device=DEV, dtype=torch.bfloat16)) for _ in range(4))
        lse = torch.full((B, H, T), NAN, device=DEV, dtype=torch.float32)
        _fwd_into(q, k, v, o, lse, True, scale)
        A._bwd(q, k, v, o, do, lse, dq, dk, dv, True, scale)
        return o, lse, dq, dk, dv
    first = call()
    second = call()
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), first, second):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------
# 5. layouts and contract
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("do_pad", [8, 4])  # row stride D + 8: read in place; D + 4: the .contiguous() branch
def test_mixed_layouts_through_autograd(D, do_pad):
    """q a view of a fused [B, T, 3, H, D] buffer, k contiguous [B, H, T, D], v [B, T, H, D]
    permuted, do with padded rows; a scale that is no head dim's default."""
    from kubeflow_rm_amd import ops
    B, H, T, scale = 2, 3, 129, 0.1
    q0, k0, v0, do0 = _randn_inputs(B, H, T, D, seed=77 + D)
    ref = _Ref(q0, k0, v0, do0, scale, True)
    fused = torch.zeros(B, T, 3, H, D, device=DEV, dtype=torch.bfloat16)
    fused[:, :, 0].copy_(q0.permute(0, 2, 1, 3))
    q = fused[:, :, 0].permute(0, 2, 1, 3).requires_grad_(True)
    k = k0.clone().requires_grad_(True)
    v = v0.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3).requires_grad_(True)
    do = torch.zeros(B, H, T, D + do_pad, device=DEV, dtype=torch.bfloat16)[..., :D]
    do.copy_(do0)
    assert not q.is_contiguous() and k.is_contiguous() and not v.is_contiguous() and not do.is_contiguous()
    assert (do.stride(2) % 8 == 0) == (do_pad == 8)
    o = ops.flash_attention(q, k, v, causal=True, scale=scale)
    o.backward(do)
    what = f"layouts[D={D} do row stride D+{do_pad}]"
    err = (o.float() - ref.o).abs().max().item()
    assert err <= ref.fwd_bound, (what, err, ref.fwd_bound)
    ref.check_bwd((q.grad, k.grad, v.grad), what)


def _contract_args(B, H, T, D):
    q, k, v, do = _randn_inputs(B, H, T, D, seed=3)
    o, dq, dk, dv = (torch.full((B, H, T, D), NAN, device=DEV, dtype=torch.bfloat16) for _ in range(4))
    lse = torch.full((B, H, T), NAN, device=DEV, dtype=torch.float32)
    return dict(q=q, k=k, v=v, do=do, o=o, dq=dq, dk=dk, dv=dv, lse=lse)


@pytest.mark.parametrize("violation", ["q_row_stride", "q_pointer", "head_dim_96"])
def test_contract_violations_raise_and_write_nothing(violation):
    from kubeflow_rm_amd.ops import _lib, attention as A
    B, H, T = 2, 3, 65
    D = 96 if violation == "head_dim_96" else 64
    a = _contract_args(B, H, T, D)
    if violation == "q_row_stride":  # rows D + 4 elements apart: not on the 16-byte grid
        q = torch.zeros(B, H, T, D + 4, device=DEV, dtype=torch.bfloat16)[..., :D]
        q.copy_(a["q"])
        assert q.stride(2) % 8 == 4
        a["q"] = q
    elif violation == "q_pointer":  # 8 bytes off the 16-byte alignment
        flat = torch.zeros(B * H * T * D + 8, device=DEV, dtype=torch.bfloat16)
        q = flat[4:4 + B * H * T * D].view(B, H, T, D)
        q.copy_(a["q"])
        assert q.data_ptr() % 16 == 8
        a["q"] = q
    with pytest.raises(_lib.NativeLibraryError):
        _fwd_into(a["q"], a["k"], a["v"], a["o"], a["lse"], True, 0.125)
    lse = torch.zeros(B, H, T, device=DEV, dtype=torch.float32)
    o = torch.zeros(B, H, T, D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(_lib.NativeLibraryError):
        A._bwd(a["q"], a["k"], a["v"], o, a["do"], lse, a["dq"], a["dk"], a["dv"], True, 0.125)
    torch.cuda.synchronize()
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert torch.isnan(a[name]).all(), name


def test_empty_sequence_raises():
    """T = 0 reaches the launcher through the Python layer, which rejects it."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    q, k, v = (torch.zeros(2, 3, 0, 64, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    with pytest.raises(_lib.NativeLibraryError):
        ops.flash_attention(q, k, v)
