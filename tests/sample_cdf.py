"""The sampler's whole kept set and CDF, recovered token by token (a plain helper module, not a conftest).

``ops.sample`` cuts ``u`` to 24 bits, ``uq = floor(u * 2^24)``, and emits the first kept token in index order whose
running sum exceeds ``floor(W * uq / 2^24)``. For a fixed row and setting ``uq -> token`` is therefore a
non-decreasing step function on ``[0, 2^24)``, and ``step_function`` recovers it completely by bisection: every
round samples the midpoints of all intervals whose ends still differ, one launch with one materialised copy of the
row per midpoint (``u = q / 2^24`` is exact in fp32). The result ``{token: first_q}`` is the sampler's kept set and
its CDF at 2^-24 resolution, on the HIP kernel and on the torch form alike.

Rows made of tie groups need no tolerance: equal keys weigh the same integer ``w``, so ``n`` kept tokens of one
value have ``W = n * w`` and token ``i`` of them starts at exactly ``ceil(i * 2^24 / n)``, whatever the kernel's
``exp2`` returns (``equal_steps``). Rows with unequal weights are compared with ``reference`` (fp64, by sorting)
within ``TOL``.

``classify`` names the kernel branch a case exercises, from the bf16 keys by the kernel's own key map, so that the
case tables at the end of this file can be checked for the branches they are meant to reach.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

BF16 = torch.bfloat16
Q = 1 << 24            # grid points of u
WAVES = 16             # waves of the kernel's workgroup: wave w owns [w * seg, (w + 1) * seg)
STEP = 64              # tokens a wave reads per step
NINF_BITS = 0xFF80
# A boundary of the CDF is a ratio of two sums of weights, each weight good to 2^-17 relative plus a 2^-20 share of
# the 2^-40 quantum (the accuracy kernels/sample_bf16.hip states): at most 2 * (2^-17 + 2^-20) = 2^-15.83 of W.
# One 2^-24 grid step comes on top. 2^-15 covers both.
TOL = 2.0 ** -15
assert 2 * (2.0 ** -17 + 2.0 ** -20) + 2.0 ** -24 <= TOL
LIVE = 2.0 ** -40      # a weight below this share of the maximum is 0 in the kernel's fixed point


def seg(V: int) -> int:
    """Tokens per wave: whole 64-token steps."""
    return (-(-V // WAVES) + STEP - 1) // STEP * STEP


def from_bits(bits) -> torch.Tensor:
    """bf16 tensor with the given 16-bit patterns."""
    return torch.from_numpy(np.asarray(bits, dtype=np.uint16).view(np.int16).copy()).view(BF16)


def keys_of(x_row: torch.Tensor) -> np.ndarray:
    """The kernel's 16-bit keys: -0 -> +0; negative values have all bits flipped; others have the sign bit set."""
    b = x_row.to(BF16).contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


# ---- the step function -------------------------------------------------------------------------------------
def step_function(x_row: torch.Tensor, temperature: float, top_k, top_p, device="cpu") -> dict:
    """{token: the lowest q in [0, 2^24) that draws it} for every token that owns a grid point, through
    ``ops.sample`` on ``device`` (CPU tensors: the torch form). Asserts that the token never decreases with q."""
    from kubeflow_rm_amd import ops
    x = x_row.to(device)
    V = x.numel()

    def draw(qs):
        u = (torch.tensor(qs, dtype=torch.float64) / Q).float()
        assert torch.equal(u.double() * Q, torch.tensor(qs, dtype=torch.float64))
        rows = x.unsqueeze(0).expand(len(qs), V).contiguous()  # the kernel takes no stride-0 batch
        out = torch.full((len(qs),), -1, dtype=torch.int64, device=device)
        tok = ops.sample(rows, u.to(device), temperature, top_k, top_p, out=out).cpu().tolist()
        assert all(0 <= t < V for t in tok), f"q={qs[tok.index(min(tok))]}: no token in [0, {V}) was emitted"
        return tok

    t_lo, t_hi = draw([0, Q - 1])
    assert t_lo <= t_hi, f"token {t_lo} at q=0 but {t_hi} at q=2^24-1"
    first = {t_lo: 0}
    open_ = [(0, Q - 1, t_lo, t_hi)] if t_lo != t_hi else []
    rounds = 0
    while open_:
        split = [iv for iv in open_ if iv[1] - iv[0] > 1]
        for lo, hi, _, th in open_:
            if hi - lo == 1:
                assert th not in first, f"token {th} drawn again at q={hi} after a higher token"
                first[th] = hi
        open_ = []
        if not split:
            break
        rounds += 1
        assert rounds <= 24  # the interval [0, 2^24 - 1] halves to length 1 in 24 rounds
        mids = draw([(lo + hi) // 2 for lo, hi, _, _ in split])
        for (lo, hi, tl, th), tm in zip(split, mids):
            mid = (lo + hi) // 2
            assert tl <= tm <= th, f"token {tm} at q={mid} between {tl} at q={lo} and {th} at q={hi}"
            if tl != tm:
                open_.append((lo, mid, tl, tm))
            if tm != th:
                open_.append((mid, hi, tm, th))
    qs = [first[t] for t in sorted(first)]
    assert qs == sorted(qs) and len(set(qs)) == len(qs)
    return first


def equal_steps(indices, n: int) -> dict:
    """The step function of n kept tokens of one weight at the lowest n of ``indices``: no tolerance."""
    idx = sorted(indices)[:n]
    return {t: -(-(i * Q) // n) for i, t in enumerate(idx)}


# ---- the fp64 reference ------------------------------------------------------------------------------------
def reference(x_row: torch.Tensor, temperature: float, top_k, top_p):
    """(kept weights fp64 [V] in index order, {token: 2^24 * cdf_before[token] / W} over the kept tokens whose
    weight the kernel's fixed point does not flush to 0) from ``ops.sample.kept_weights`` on the row's exact
    values, with top_p rounded to fp32 as the kernel receives it."""
    from kubeflow_rm_amd.ops.sample import kept_weights
    p = None if top_p is None else float(np.float32(top_p))
    wk = kept_weights(x_row.double().unsqueeze(0), temperature, top_k, p)[0]  # top_k == 1: the greedy token alone
    W = wk.sum()
    before = wk.cumsum(0) - wk
    live = (wk >= LIVE).nonzero().flatten().tolist()
    return wk, {t: float(Q * before[t] / W) for t in live}


def max_deviation(steps: dict, ref_q: dict) -> float:
    """max |first_q - reference| / 2^24 over the tokens of ``steps`` (all of them must be in the reference)."""
    return max(abs(q - ref_q[t]) for t, q in steps.items()) / Q


class Cut(NamedTuple):
    ck: int | None        # key of the top-k cut, members of its tie group inside the top k
    ak: int | None
    cp: int | None        # key of the top-p cut
    needed: float | None  # members of cp's tie group the top-p prefix needs, as a real number
    w_cp: float | None    # weight of one such member, and the mass of the top-k set
    Z: float | None
    members: np.ndarray   # indices of the tie group at the final cut (empty where nothing is cut)


def cut_of(x_row: torch.Tensor, temperature: float, top_k, top_p) -> Cut:
    """Where the cuts fall, in fp64 on the kernel's keys."""
    keys = keys_of(x_row)
    V = keys.size
    xd = x_row.double().numpy()
    with np.errstate(invalid="ignore"):
        w = np.exp((xd - xd.max()) / temperature)
    order = np.lexsort((np.arange(V), -keys))  # key descending, index ascending
    K = top_k if top_k is not None and top_k < V else None
    ck = ak = cp = needed = w_cp = Z = None
    kept = order
    if K is not None:
        kept = order[:K]
        ck = int(keys[order[K - 1]])
        ak = K - int((keys > ck).sum())
    if top_p is not None and top_p < 1.0:
        p = float(np.float32(top_p))
        wo, ko = w[kept], keys[kept]
        Z = float(wo.sum())
        n = min(int((np.cumsum(wo) < p * Z).sum()) + 1, kept.size)
        cp = int(ko[n - 1])
        w_cp = float(wo[n - 1])
        needed = (p * Z - float(wo[ko > cp].sum())) / w_cp if w_cp > 0 else None
    cut = cp if cp is not None else ck
    members = np.flatnonzero(keys == cut) if cut is not None else np.zeros(0, dtype=np.int64)
    return Cut(ck, ak, cp, needed, w_cp, Z, members)


class Branch(NamedTuple):
    Hk: int | None        # high key byte of the top-k cut (None: no top-k cut)
    Hp: int | None        # high key byte of the top-p cut (None: no top-p cut)
    relation: str | None  # "no-k", "Hp>Hk", "Hp==Hk, cp>ck", "cp==ck" where top-p cuts; "greedy"; None
    spans_steps: bool     # the cut tie group has members in more than one 64-token step of one wave
    spans_waves: bool     # ... in more than one wave segment


def classify(x_row: torch.Tensor, top_k, top_p, temperature: float = 1.0) -> Branch:
    if temperature == 0 or top_k == 1:
        return Branch(None, None, "greedy", False, False)
    c = cut_of(x_row, temperature, top_k, top_p)
    Hk = None if c.ck is None else c.ck >> 8
    Hp = None if c.cp is None else c.cp >> 8
    relation = None
    if c.cp is not None:
        relation = "no-k" if c.ck is None else "Hp>Hk" if Hp > Hk else "Hp==Hk, cp>ck" if c.cp > c.ck else "cp==ck"
        assert c.ck is None or c.cp >= c.ck
    s = seg(x_row.numel())
    waves, steps = c.members // s, c.members // STEP
    spans_steps = any(len(set(steps[waves == w])) > 1 for w in set(waves.tolist()))
    return Branch(Hk, Hp, relation, spans_steps, len(set(waves.tolist())) > 1)


def top_p_clear(x_row: torch.Tensor, temperature: float, top_k, top_p, tol: float = TOL) -> bool:
    """The top-p cut is unambiguous: the masses of the prefix that reaches top_p * Z, and of the one a token
    shorter, are more than tol * Z away from top_p * Z."""
    if top_p is None or top_p >= 1.0:
        return True
    xd = x_row.double()
    w = torch.exp((xd - xd.max()) / temperature).sort(descending=True).values
    if top_k is not None:
        w[top_k:] = 0
    Z, cum = w.sum(), w.cumsum(0)
    n = min(int((cum < top_p * Z).sum()) + 1, w.numel())
    return bool(cum[n - 1] - top_p * Z > tol * Z and (n == 1 or top_p * Z - cum[n - 2] > tol * Z))


def straddles_top_k(x_row: torch.Tensor, top_k: int) -> bool:
    """A tie group lies on both sides of the top-k cut."""
    c = cut_of(x_row, 1.0, top_k, None)
    return c.ck is not None and c.ak < c.members.size


# ---- row builders and the case tables ----------------------------------------------------------------------
# A. all-equal rows
EQUAL_KINDS = ("1.5", "-3.0", "zeros")
EQUAL_V = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)  # 1024 -> 1025: seg 64 -> 128, waves 9..15 become empty


def equal_row(V: int, kind: str) -> torch.Tensor:
    if kind == "zeros":  # +0 / -0 alternating: one tie group
        return from_bits([0x0000 if i % 2 == 0 else 0x8000 for i in range(V)])
    return torch.full((V,), float(kind), dtype=BF16)


def equal_settings(V: int):
    """(top_k, top_p, the number of tokens kept: min(k, V), then ceil(p * n))."""
    ks = sorted({k for k in (2, 63, 64, 65, V - 1, V, V + 9) if k >= 1})
    sets = [(None, None)] + [(k, None) for k in ks] + [(None, 0.3125), (None, 0.8125)]
    sets += [(k, p) for k, p in ((2, 0.5), (65, 0.75), (V - 1, 0.3125), (V + 9, 0.8125)) if k >= 1]
    out = []
    for k, p in sets:
        n = V if k is None else min(k, V)
        out.append((k, p, n if p is None else math.ceil(p * n)))  # p * n is exact: p has 4 fractional bits
    return out


# B. a plateau over a floor
PLATEAU_V = (257, 1025, 4097)
PLATEAU_FLOORS = ("-inf", "a-64")
PLATEAU_A = 2.0


def plateau_indices(V: int):
    """The first and last index, both sides of a 64-step edge and of a wave-segment edge, a run of 70."""
    s = seg(V)
    idx = sorted({0, V - 1, 63, 64, 2 * s - 1, 2 * s} | set(range(2 * s + 12, 2 * s + 82)))
    assert idx[-1] == V - 1 and len(idx) == 76
    return idx


def plateau_row(V: int, floor: str) -> torch.Tensor:
    """n_hi tokens at a = 2.0 (weight exactly 2^40 each); the rest at -inf, or at a - 64, whose weight
    e^-64 = 2^-92 is 0 in units of 2^-40 at temperature 1."""
    x = torch.full((V,), float("-inf") if floor == "-inf" else PLATEAU_A - 64.0, dtype=BF16)
    x[plateau_indices(V)] = PLATEAU_A
    return x


def plateau_settings(V: int):
    """(top_k, top_p, plateau members kept)."""
    n = len(plateau_indices(V))
    out = [(None, None, n)]
    out += [(k, None, k) for k in (1, 2, n // 2, n - 1, n)]       # inside the plateau (1: greedy), exactly n_hi
    out += [(k, None, n) for k in (n + 5, V - 1)]                 # inside the floor: zero-weight kept tokens
    out += [(None, p, math.ceil(p * n)) for p in (0.3125, 0.75)]  # p * 76 = 23.75, 57
    out += [(j, p, math.ceil(p * j)) for j, p in ((40, 0.75), (41, 0.3125), (n - 1, 0.5))]  # cp == ck: avail = ak
    out += [(n + 5, 0.5, n // 2), (n + 5, 0.8125, math.ceil(0.8125 * n))]  # top-p above a top-k cut in the floor
    return out


# C. the greatest V
BIG_V = ((1 << 20), (1 << 20) - 65)  # the second: last wave and last step partly filled; seg = 65536 for both


def big_queries(n: int):
    """8 (q, token) pairs over n equally weighted kept tokens 0..n-1: tokens 0 and n - 1 and both sides of three
    wave-segment edges; token == floor(n * q / 2^24)."""
    last = (n - 1) // 65536
    toks = [0]
    for w in (1, max(2, last // 2), last):
        toks += [65536 * w - 1, 65536 * w]
    pairs = [(-(-(t * Q) // n), t) for t in toks] + [(Q - 1, n - 1)]
    assert len(pairs) == 8 and all(t == n * q // Q and 0 <= q < Q for q, t in pairs)
    return pairs


# D. a staircase on bin edges
STAIR_V = 4097
# low key bytes at 0x00, 0x7F / 0x80 and 0xFF, adjacent high bytes, both sides of the sign, no denormals
STAIR_BITS = (0x4100, 0x40FF, 0x4080, 0x4000, 0x3FFF, 0x3F80, 0x0080, 0x0000, 0x8000, 0x8080, 0xBF80, 0xBFFF, 0xC000)


def staircase_row(V: int = STAIR_V):
    """Value i of STAIR_BITS 1 + i % 3 times, the members of one value in different waves, the rest -inf.
    Returns (row, the number of non-floor tokens)."""
    s = seg(V)
    nw = -(-V // s)
    stride = max(1, nw // 3)
    bits = [NINF_BITS] * V
    count = 0
    for i, b in enumerate(STAIR_BITS):
        for j in range(1 + i % 3):
            wave = (i + j * stride) % nw
            width = min(s, V - wave * s)
            off = (37 * i + 101 * j + 7) % width
            while bits[wave * s + off] != NINF_BITS:  # taken: the next free index of the wave
                off = (off + 1) % width
            idx = wave * s + off
            bits[idx] = b
            count += 1
    return from_bits(bits), count


# (top_k, bit pattern of the top-p cut's tie group, its members the prefix needs, the relation this reaches).
# In key order the row holds 1, 2, 3, 1, 2, 3, 1, 5 (+0 and -0), 1, 2, 3, 1 tokens: top_k = 16 cuts 3 into the 5
# zeros (Hk = 0x80), top_k = 11 cuts 2 into the 3 at 1.0 (Hk = 0xBF).
STAIR_TOP_P = (
    (None, 0x4080, 1.5, "no-k"), (None, 0x3F80, 2.5, "no-k"), (None, 0x0000, 2.5, "no-k"),
    (16, 0x4080, 2.5, "Hp>Hk"), (16, 0x3FFF, 1.5, "Hp>Hk"), (16, 0x0080, 0.5, "Hp==Hk, cp>ck"),
    (16, 0x0000, 1.5, "cp==ck"),
    (11, 0x40FF, 1.5, "Hp>Hk"), (11, 0x3FFF, 1.5, "Hp==Hk, cp>ck"), (11, 0x3F80, 1.5, "cp==ck"),
)


def top_p_into(x_row: torch.Tensor, temperature: float, top_k, cut_bits: int, members: float) -> float:
    """The top_p (rounded to fp32) whose prefix of the top-k set ends ``members`` tokens into the tie group of
    ``cut_bits``."""
    keys = keys_of(x_row)
    c = cut_of(x_row, temperature, top_k, 0.5)  # for Z
    xd = x_row.double().numpy()
    w = np.exp((xd - xd.max()) / temperature)
    ckey = int(keys_of(from_bits([cut_bits]))[0])
    hit = np.flatnonzero(keys == ckey)
    assert hit.size and (c.ck is None or ckey >= c.ck)
    return float(np.float32((w[keys > ckey].sum() + members * w[hit[0]]) / c.Z))


# E. random rows
RANDOM_SETTINGS = {"plain": (None, None), "top_k": (40, None), "top_p": (None, 0.9), "both": (40, 0.9)}
RANDOM_T = 0.8
# V -> seed: chosen (on the CPU) so that at least one of the 3 rows has a tie group across the top-k cut
RANDOM_SEEDS = {257: 1, 1025: 1, 4097: 1}


def random_rows(V: int, seed: int, B: int = 3):
    """bf16 rows randn * 4 (natural ties), each redrawn until its top-p cut is unambiguous at TOL under every
    setting. The top-k cut is not filtered."""
    rows = []
    for b in range(B):
        for attempt in range(400):
            g = torch.Generator().manual_seed(100003 * seed + 401 * b + attempt)
            x = (torch.randn(V, generator=g) * 4).to(BF16)
            if all(top_p_clear(x, RANDOM_T, k, p) for k, p in RANDOM_SETTINGS.values()):
                break
        else:
            raise AssertionError(f"no unambiguous row found for V={V} row {b}")
        rows.append(x)
    return rows
