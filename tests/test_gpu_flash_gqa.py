"""Flash attention on grouped K / V heads (kernels/attention_bf16.hip with Hkv < H), kernel to model.

The forward and dQ kernels keep their grids in query heads and change only the K / V base offsets, so O, LSE and
dQ of a grouped call must equal, bit for bit, the ungrouped call of the same build on K / V expanded to H heads.
dK / dV sweeps a group inside one workgroup (``group_split`` = GS query heads per workgroup; GS < G goes through
fp32 parts and a reduce kernel): head routing is checked bit for bit against the ungrouped kernel with all but one
head of a group silenced (dO = 0: dP, delta and dS are exact zeros), the values against fp32 SDPA on expanded K / V
summed over the group in fp32. Bounds are those of tests/test_gpu_attention.py.
"""
from __future__ import annotations

import functools
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _feature():
    """The feature exists: the grouped entry points and the ``kv_heads`` keyword. Fails (does not skip) before any
    launch, so nothing hands fewer K / V heads to a launcher that does not know about them."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    L = _lib.lib()
    for sym in ("kfamd_attn_fwd_gqa_bf16", "kfamd_attn_bwd_gqa_bf16", "kfamd_attn_bwd_gqa_workspace",
                "kfamd_attn_bwd_gqa_group_split"):
        assert hasattr(L, sym), f"{sym}: not in the kernel library"
    for fn in (ops.attention_qkv, ops.attn_block):
        assert "kv_heads" in inspect.signature(fn).parameters, f"{fn.__name__}: no kv_heads keyword"


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]


def _splits(G):
    """group_split = G, 1 and (where G has one) a middle divisor."""
    mid = [d for d in _divisors(G) if 1 < d < G]
    return sorted({G, 1, *mid[len(mid) // 2:len(mid) // 2 + 1]}, reverse=True)


HEADS = [(2, 8, 2), (1, 8, 1), (1, 6, 2), (2, 8, 8)]
CASES = [(B, H, Hkv, T, D) for D in (64, 128) for T in (128, 200, 300) for (B, H, Hkv) in HEADS]
IDS = [f"{B}x{H}/{Hkv}x{T}x{D}" for (B, H, Hkv, T, D) in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Hkv, T, D):
    """q, k, v views [B, H | Hkv, T, D] and do [B, H, T, D]. T != 128: views of one fused activation
    [B, T, (H + 2 Hkv) D] (the model's layout: row stride (H + 2 Hkv) D, head stride D); T == 128: [B, T, H, D]
    storage per tensor. Never written by a test."""
    from kubeflow_rm_amd.ops import attention as A
    g = torch.Generator(device="cpu").manual_seed(1000 * T + 10 * D + H + Hkv)
    if T != 128:
        qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g).to(DEV, torch.bfloat16)
        q, k, v = A._qkv_views(qkv, H, Hkv, D)
    else:
        q, k, v = (A._bhtd(torch.randn(B, T, n, D, generator=g).to(DEV, torch.bfloat16)) for n in (H, Hkv, Hkv))
    do = A._bhtd(torch.randn(B, T, H, D, generator=g).to(DEV, torch.bfloat16))
    return q, k, v, do


def _expand(x, G):
    """[B, Hkv, T, D] -> a materialised [B, Hkv G, T, D] (head h <- h // G), [B, T, H, D] storage."""
    from kubeflow_rm_amd.ops import attention as A
    return A._bhtd(x.repeat_interleave(G, dim=1).permute(0, 2, 1, 3).contiguous())


def _empty_like_heads(x):
    from kubeflow_rm_amd.ops import attention as A
    B, n, T, D = x.shape
    return A._bhtd(torch.full((B, T, n, D), NAN, device=DEV, dtype=torch.bfloat16))


def _forward(q, k, v, causal):
    from kubeflow_rm_amd.ops import attention as A
    o = _empty_like_heads(q)
    lse = A._fwd(q, k, v, o, causal, 1.0 / math.sqrt(q.shape[-1]))
    return o, lse


def _backward(q, k, v, o, do, lse, causal, gs=0):
    from kubeflow_rm_amd.ops import attention as A
    dq, dk, dv = _empty_like_heads(q), _empty_like_heads(k), _empty_like_heads(v)
    A._bwd(q, k, v, o, do, lse, dq, dk, dv, causal, 1.0 / math.sqrt(q.shape[-1]), gs)
    return dq, dk, dv


@functools.lru_cache(maxsize=None)
def _grouped(B, H, Hkv, T, D, causal):
    """The grouped forward and, per group_split, the grouped backward of a case (computed once, left unchanged)."""
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    o, lse = _forward(q, k, v, causal)
    return o, lse, {gs: _backward(q, k, v, o, do, lse, causal, gs) for gs in _splits(H // Hkv)}


@functools.lru_cache(maxsize=None)
def _reference(B, H, Hkv, T, D, causal):
    """fp32 SDPA on expanded K / V; dk / dv summed over the group in fp32. Returns o, lse, dq, dk, dv."""
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    G = H // Hkv
    qf, kf, vf = (x.detach().float().requires_grad_(True) for x in (q, k, v))
    ke, ve = (x.repeat_interleave(G, dim=1) for x in (kf, vf))  # autograd sums the group in fp32
    o = F.scaled_dot_product_attention(qf, ke, ve, is_causal=causal)
    o.backward(do.float())
    s = (qf.detach() @ ke.detach().transpose(-1, -2)) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool, device=DEV), 1), float("-inf"))
    return o.detach(), torch.logsumexp(s, -1), qf.grad, kf.grad, vf.grad


# ------------------------------------------------------------------------------------------------
# 1. forward and dQ, bit for bit against the ungrouped call on expanded K / V
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,H,Hkv,T,D", CASES, ids=IDS)
def test_forward_and_dq_equal_the_expanded_call(B, H, Hkv, T, D, causal):
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    G = H // Hkv
    o, lse, grads = _grouped(B, H, Hkv, T, D, causal)
    ke, ve = _expand(k, G), _expand(v, G)
    o1, lse1 = _forward(q, ke, ve, causal)
    assert torch.equal(o, o1) and torch.equal(lse, lse1)
    dq1, _, _ = _backward(q, ke, ve, o1, do, lse1, causal)
    for gs, (dq, _, _) in grads.items():
        assert torch.equal(dq, dq1), f"dq, group_split {gs}"


def test_forward_fwd_pp_route():
    """B = 2, H = 128, Hkv = 16, T = 300, D = 128: the one-workgroup-per-CU forward (attn_fwd_pp, paired), by the
    launcher's rule as tests/test_gpu_attention_edges.py mirrors it (kfamd_attn_fwd_bf16: nq4, pair4, g4 and the
    ``g4 >= device_cus()`` branch). Grids stay in query heads, so the rule is the ungrouped one."""
    B, H, Hkv, T, D = 2, 128, 16, 300, 128
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nq4 = (T + 255) // 256
    assert nq4 % 2 == 0 and (nq4 // 2) * H * B >= cus, "attn_fwd_pp (paired) is not the route on this device"
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    o, lse = _forward(q, k, v, True)
    ke, ve = _expand(k, H // Hkv), _expand(v, H // Hkv)
    o1, lse1 = _forward(q, ke, ve, True)
    assert torch.equal(o, o1) and torch.equal(lse, lse1)
    ro, rlse, rdq, rdk, rdv = _reference(B, H, Hkv, T, D, True)
    assert (o.float() - ro).abs().max().item() < 2e-2 and _rel(o, ro) < 8e-3
    assert (lse - rlse).abs().max().item() < 1e-3
    dq1, _, _ = _backward(q, ke, ve, o1, do, lse1, True)
    for gs in _splits(H // Hkv):
        dq, dk, dv = _backward(q, k, v, o, do, lse, True, gs)
        assert torch.equal(dq, dq1), gs
        for name, got, want in (("dk", dk, rdk), ("dv", dv, rdv)):
            assert torch.isfinite(got.float()).all() and _rel(got, want) < 2e-2, (name, gs, _rel(got, want))


# ------------------------------------------------------------------------------------------------
# 2. dK / dV head routing, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,H,Hkv,T,D", CASES, ids=IDS)
def test_dkdv_head_routing(B, H, Hkv, T, D, causal):
    """dO = 0 for every query head of a group but the one at position j: grouped dK / dV == the ungrouped kernel's
    for those heads alone (H' = Hkv heads, the same K / V). Every j, every group_split."""
    from kubeflow_rm_amd.ops import attention as A
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    G = H // Hkv
    o, lse, _ = _grouped(B, H, Hkv, T, D, causal)
    for j in range(G):
        dom = torch.zeros_like(do)
        dom[:, j::G] = do[:, j::G]
        sel = [A._bhtd(x[:, j::G].permute(0, 2, 1, 3).contiguous()) for x in (q, o, do)]
        _, dk1, dv1 = _backward(sel[0], k, v, sel[1], sel[2], lse[:, j::G].contiguous(), causal)
        for gs in _splits(G):
            _, dk, dv = _backward(q, k, v, o, dom, lse, causal, gs)
            assert torch.equal(dk, dk1), f"dk: kept head {j} of its group, group_split {gs}"
            assert torch.equal(dv, dv1), f"dv: kept head {j} of its group, group_split {gs}"


# ------------------------------------------------------------------------------------------------
# 3. values against fp32, determinism of each route
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,H,Hkv,T,D", CASES, ids=IDS)
def test_values_match_fp32_and_routes_are_deterministic(B, H, Hkv, T, D, causal):
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    o, lse, grads = _grouped(B, H, Hkv, T, D, causal)
    ro, rlse, rdq, rdk, rdv = _reference(B, H, Hkv, T, D, causal)
    err = (o.float() - ro).abs().max().item()
    print(f"o max-abs {err:.4g} rel {_rel(o, ro):.4g}; lse {(lse - rlse).abs().max().item():.4g}")
    assert err < 2e-2 and _rel(o, ro) < 8e-3
    assert (lse - rlse).abs().max().item() < 1e-3
    for gs, (dq, dk, dv) in grads.items():
        assert dk.shape == k.shape and dv.shape == v.shape
        for name, got, want in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
            print(f"group_split {gs} {name}: rel-l2 {_rel(got, want):.4g}")
            assert torch.isfinite(got.float()).all(), (name, gs)
            assert _rel(got, want) < 2e-2, (name, gs, _rel(got, want))
        again = _backward(q, k, v, o, do, lse, causal, gs)
        assert all(torch.equal(a, b) for a, b in zip(again, (dq, dk, dv))), f"group_split {gs}: not deterministic"


def test_launcher_rule_and_default_route():
    """kfamd_attn_bwd_gqa_group_split: the largest divisor GS of G whose grid ceil(T / 128) Hkv B (G / GS) has 1.5
    workgroups per slot (compute units x 2 at D = 64), else 1 (a copy of gqa_group_split in attention_bf16.hip);
    group_split = 0 runs that route (same bits as asking for it)."""
    from kubeflow_rm_amd.ops import _lib
    L = _lib.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (B, H, Hkv, T, D) in [(2, 8, 2, 200, 64), (1, 6, 2, 300, 128), (2, 128, 16, 300, 128), (4, 16, 4, 2048, 128),
                              (4, 16, 2, 2048, 128), (16, 12, 3, 2048, 64), (16, 12, 2, 2048, 64), (1, 8, 2, 2048, 128)]:
        G, nkv, slots = H // Hkv, -(-T // 128) * Hkv * B, cus * (2 if D == 64 else 1)
        want = next((gs for gs in sorted(_divisors(G), reverse=True) if gs > 1 and 2 * nkv * (G // gs) >= 3 * slots), 1)
        assert L.kfamd_attn_bwd_gqa_group_split(B, H, Hkv, T, D) == want
    B, H, Hkv, T, D = 2, 8, 2, 200, 64
    q, k, v, do = _inputs(B, H, Hkv, T, D)
    o, lse, grads = _grouped(B, H, Hkv, T, D, True)
    rule = L.kfamd_attn_bwd_gqa_group_split(B, H, Hkv, T, D)
    assert all(torch.equal(a, b) for a, b in zip(_backward(q, k, v, o, do, lse, True, 0), grads[rule]))


# ------------------------------------------------------------------------------------------------
# 4. stray writes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Hkv,T,D", [(2, 8, 2, 200, 64), (1, 6, 2, 300, 128), (1, 8, 1, 128, 128)])
def test_no_stray_writes_and_no_reads_past_T(B, H, Hkv, T, D):
    """dq / dk / dv in the (h + 2 hkv) hd gradient layout and O, each inside a NaN-filled buffer with guard columns
    and guard rows past T; the K / V (and Q) rows past T of the input hold NaN. Guards stay NaN, outputs finite."""
    from kubeflow_rm_amd.ops import attention as A
    GR, GC = 3, 16
    W = (H + 2 * Hkv) * D
    src = _inputs(B, H, Hkv, T, D)
    xin = torch.full((B, T + GR, W), NAN, device=DEV, dtype=torch.bfloat16)
    q, k, v = A._qkv_views(xin[:, :T], H, Hkv, D)
    for dst, s in zip((q, k, v), src[:3]):
        dst.copy_(s)
    do = src[3]
    scale = 1.0 / math.sqrt(D)
    obuf = torch.full((B, T + GR, H * D + GC), NAN, device=DEV, dtype=torch.bfloat16)
    o = A._bhtd(obuf[:, :T, :H * D].view(B, T, H, D))
    lse = A._fwd(q, k, v, o, True, scale)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.isnan(obuf[:, T:]).all() and torch.isnan(obuf[:, :, H * D:]).all()
    want = _grouped(B, H, Hkv, T, D, True)
    assert torch.equal(o, want[0]) and torch.equal(lse, want[1])
    for gs in _splits(H // Hkv):
        gbuf = torch.full((B, T + GR, W + GC), NAN, device=DEV, dtype=torch.bfloat16)
        dq, dk, dv = A._qkv_views(gbuf[:, :T, :W], H, Hkv, D)
        A._bwd(q, k, v, o, do, lse, dq, dk, dv, True, scale, gs)
        assert torch.isfinite(gbuf[:, :T, :W].float()).all(), gs
        assert torch.isnan(gbuf[:, T:]).all() and torch.isnan(gbuf[:, :, W:]).all(), f"group_split {gs}: a guard was written"
        assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), want[2][gs])), gs


# ------------------------------------------------------------------------------------------------
# 5. ops layer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,hd,h,hkv", [(200, 64, 8, 2), (300, 128, 6, 2)])
def test_attention_qkv_kv_heads_matches_view_entry_point(T, hd, h, hkv):
    from kubeflow_rm_amd import ops
    B = 2
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(B, T, (h + 2 * hkv) * hd, generator=g).to(DEV, torch.bfloat16).requires_grad_(True)
    y = ops.attention_qkv(qkv, h, hd, kv_heads=hkv)
    dy = torch.randn(B, T, h * hd, generator=g).to(DEV, torch.bfloat16)
    y.backward(dy)
    x = qkv.detach()
    q = x[..., :h * hd].view(B, T, h, hd).transpose(1, 2).clone().requires_grad_(True)
    k, v = (t.transpose(1, 2).clone().requires_grad_(True) for t in x[..., h * hd:].view(B, T, 2, hkv, hd).unbind(2))
    o = ops.flash_attention(q, k, v)
    o.backward(dy.view(B, T, h, hd).transpose(1, 2))
    assert o.shape == (B, h, T, hd) and k.grad.shape == (B, hkv, T, hd) and v.grad.shape == (B, hkv, T, hd)
    assert torch.equal(y.view(B, T, h, hd).transpose(1, 2), o)
    want = torch.cat([t.grad.transpose(1, 2).reshape(B, T, -1) for t in (q, k, v)], -1)
    assert torch.equal(qkv.grad, want)


def test_attn_block_kv_heads_with_rope_matches_composition():
    """ops.attn_block(kv_heads=, rope=): loss and every gradient against the same computation from ops.linear (the
    autograd form of gemm_nt), rope_qkv, flash_attention on expanded K / V and autograd."""
    from kubeflow_rm_amd import ops
    B, T, Dm, h, hkv, hd = 2, 200, 512, 8, 2, 64
    G = h // hkv
    g = torch.Generator(device="cpu").manual_seed(11)

    def mk(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).to(DEV, torch.bfloat16)
    x0, wq0, bq0 = mk(B, T, Dm), mk((h + 2 * hkv) * hd, Dm, s=Dm ** -0.5), mk((h + 2 * hkv) * hd, s=0.1)
    wp0, bp0, tgt = mk(Dm, h * hd, s=(h * hd) ** -0.5), mk(Dm, s=0.1), mk(B, T, Dm)
    rope = ops.rope_table(256, hd, device=DEV)

    def leaves():
        return [t.clone().requires_grad_(True) for t in (x0, wq0, bq0, wp0, bp0)]

    x, wq, bq, wp, bp = a = leaves()
    out = ops.attn_block(x, wq, bq, wp, bp, h, hd, residual=x, rope=rope, kv_heads=hkv)
    loss = (out.float() * tgt.float()).mean() * 100
    loss.backward()

    x, wq, bq, wp, bp = b = leaves()
    qkv = ops.rope_qkv(ops.linear(x, wq, bq), rope, h, hkv)
    q = qkv[..., :h * hd].view(B, T, h, hd).transpose(1, 2)
    k, v = (t.repeat_interleave(G, dim=2).transpose(1, 2) for t in qkv[..., h * hd:].view(B, T, 2, hkv, hd).unbind(2))
    y = ops.flash_attention(q, k, v).transpose(1, 2).reshape(B, T, h * hd)
    ref = ops.linear(y, wp, bp, residual=x)
    rloss = (ref.float() * tgt.float()).mean() * 100
    rloss.backward()
    print(f"loss {loss.item():.5f} / {rloss.item():.5f}")
    assert abs(loss.item() - rloss.item()) < 2e-2
    for name, got, want in zip(("x", "wqkv", "bqkv", "wproj", "bproj"), a, b):
        r = _rel(got.grad, want.grad)
        print(f"  d{name}: rel {r:.4g}")
        assert got.grad.shape == want.grad.shape and torch.isfinite(got.grad.float()).all() and r < 5e-2, (name, r)


# ------------------------------------------------------------------------------------------------
# 6. model
# ------------------------------------------------------------------------------------------------
def _cfg(n_kv, dtype):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=512, n_layers=2, n_heads=8, d_ff=688, max_seq=256, dtype=dtype,
                     n_kv_heads=n_kv, pos="rope", norm="rms", mlp="swiglu")


class _Spy:
    """Records the head counts of q and k / v that reach ops.attention._fwd / _bwd."""

    def __init__(self, monkeypatch):
        from kubeflow_rm_amd.ops import attention as A
        self.fwd, self.bwd = [], []
        f0, b0 = A._fwd, A._bwd

        def fwd(q, k, v, *a, **kw):
            self.fwd.append((q.shape[1], k.shape[1], v.shape[1]))
            return f0(q, k, v, *a, **kw)

        def bwd(q, k, v, o, do, lse, dq, dk, dv, *a, **kw):
            self.bwd.append((q.shape[1], k.shape[1], v.shape[1], dk.shape[1], dv.shape[1]))
            return b0(q, k, v, o, do, lse, dq, dk, dv, *a, **kw)
        monkeypatch.setattr(A, "_fwd", fwd)
        monkeypatch.setattr(A, "_bwd", bwd)


@pytest.mark.parametrize("n_kv", [2, None], ids=["gqa2", "mha"])
def test_model_training_step_reads_grouped_heads_in_place(n_kv, monkeypatch):
    """One training step against the fp32 CPU model (bounds of tests/test_gpu_llama.py); K / V reach the launchers
    with Hkv heads (H for the default model), and SDPA is never called."""
    from kubeflow_rm_amd.models import GPT
    spy = _Spy(monkeypatch)
    hkv = 8 if n_kv is None else n_kv
    torch.manual_seed(0)
    idx = torch.randint(0, 512, (2, 128))
    tgt = torch.randint(0, 512, (2, 128))
    gpu = GPT(_cfg(n_kv, torch.bfloat16), device=DEV)
    with monkeypatch.context() as m:
        m.setattr(F, "scaled_dot_product_attention", lambda *a, **k: pytest.fail("SDPA called"))
        logits, loss = gpu(idx.cuda(), tgt.cuda())
        loss.backward()
    assert spy.fwd == [(8, hkv, hkv)] * 2 and spy.bwd == [(8, hkv, hkv, hkv, hkv)] * 2
    ref = GPT(_cfg(n_kv, torch.float32))
    rlogits, rloss = ref(idx, tgt)
    rloss.backward()
    err = (logits.float().cpu() - rlogits.detach()).abs().max().item()
    print(f"loss {loss.item():.4f} / {rloss.item():.4f}, logits max-abs {err:.4f}")
    assert abs(loss.item() - rloss.item()) < 2e-2 * abs(rloss.item())
    assert err < 0.1, err
    for name in ("ln1.weight", "qkv.weight", "proj.weight", "ln2.weight", "fc1.weight"):
        gr = gpu.blocks[0].get_parameter(name).grad.float().cpu()
        r = ref.blocks[0].get_parameter(name).grad
        print(f"  blocks[0].{name}.grad: max-abs error / max |reference| {((gr - r).abs().max() / r.abs().max()).item():.4f}")
        assert torch.allclose(gr, r, atol=5e-2 * r.abs().max().item() + 1e-3), name


def test_model_forced_unfused_path_reads_grouped_heads(monkeypatch):
    """Block._attention_gqa (the path off ops.attn_block) on the GPU: ops.attention_qkv(kv_heads=), same loss as the
    fused node within the block test's bound."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT
    spy = _Spy(monkeypatch)
    torch.manual_seed(0)
    gpu = GPT(_cfg(2, torch.bfloat16), device=DEV)
    blk = gpu.blocks[0]
    x = torch.randn(2, 128, 512, device=DEV).to(torch.bfloat16)
    with monkeypatch.context() as m:
        m.setattr(F, "scaled_dot_product_attention", lambda *a, **k: pytest.fail("SDPA called"))
        y = blk._attention_gqa(x, x, gpu.rope_table)
    want = blk.attention(x, x, gpu.rope_table)
    assert spy.fwd == [(8, 2, 2)] * 2
    assert _rel(y, want) < 8e-3  # the same kernels on the same values: the forward test's bound for O


@pytest.mark.parametrize("kv_dtype", [None, torch.float8_e4m3fn], ids=["bf16", "fp8"])
def test_model_prefill_equals_the_expanded_prefill(kv_dtype, monkeypatch):
    """prefill logits == those of a prefill whose attention is computed as before this kernel knew groups: split the
    rotated activation, repeat K / V over the group, ungrouped flash kernel."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT
    from kubeflow_rm_amd.ops import attention as A
    gpu = GPT(_cfg(2, torch.bfloat16), device=DEV).eval()
    torch.manual_seed(1)
    idx = torch.randint(0, 512, (2, 200), device=DEV)

    def run():
        cache = gpu.new_cache(2, 256, **({"kv_dtype": kv_dtype} if kv_dtype is not None else {}))
        return gpu.prefill(idx, cache)
    spy = _Spy(monkeypatch)
    got = run()
    assert spy.fwd == [(8, 2, 2)] * 2

    def old_attention(qkv, h, hd, causal=True, scale=None, kv_heads=None):
        assert kv_heads == 2
        q, k, v = GPT._split_gqa(qkv, h, kv_heads, hd)
        assert k.shape[1] == h
        B, T = qkv.shape[:2]
        return ops.flash_attention(q, k, v, causal=causal).transpose(1, 2).reshape(B, T, h * hd)
    monkeypatch.setattr(ops, "attention_qkv", old_attention)
    want = run()
    assert spy.fwd[2:] == [(8, 8, 8)] * 2
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib, attention as A
    B, T, D = 1, 128, 64
    scale = 1.0 / math.sqrt(D)

    def t(n, fill=None):
        x = torch.randn(B, T, n, D, device=DEV).to(torch.bfloat16) if fill is None else \
            torch.full((B, T, n, D), fill, device=DEV, dtype=torch.bfloat16)
        return A._bhtd(x)
    q, do = t(8), t(8)
    o, dq = t(8, 7.0), t(8, 7.0)
    for hkv in (3, 5):  # H % Hkv != 0
        k, v, dk, dv = t(hkv), t(hkv), t(hkv, 7.0), t(hkv, 7.0)
        with pytest.raises(ValueError):
            A._fwd(q, k, v, o, True, scale)
        with pytest.raises(ValueError):
            ops.flash_attention(q, k, v)
        with pytest.raises(ValueError):
            A._bwd(q, k, v, o, do, torch.zeros(B, 8, T, device=DEV), dq, dk, dv, True, scale)
        assert all((x == 7.0).all() for x in (o, dq, dk, dv))
    k0 = A._bhtd(torch.empty(B, T, 0, D, device=DEV, dtype=torch.bfloat16))  # Hkv = 0
    with pytest.raises(ValueError):
        A._fwd(q, k0, k0, o, True, scale)
    with pytest.raises(ValueError):
        ops.flash_attention(q, k0, k0)
    k, v, dk, dv = t(2), t(2), t(2, 7.0), t(2, 7.0)
    lse = A._fwd(q, k, v, t(8), True, scale)
    with pytest.raises(ValueError):  # G = 4: 3 does not divide it
        A._bwd(q, k, v, o, do, lse, dq, dk, dv, True, scale, 3)
    assert all((x == 7.0).all() for x in (o, dq, dk, dv))
    # the C entry points themselves: KFAMD_EINVAL (-1), nothing launched
    L = _lib.lib()
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    st8 = A._strides(q, k, v, o, do, dq, dk, dv)
    for H, Hkv, gs in ((8, 3, 0), (8, 0, 0), (8, 2, 3)):
        if gs == 0:
            assert L.kfamd_attn_fwd_gqa_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B,
                                             H, Hkv, T, D, scale, 1, A._strides(q, k, v, o), A._stream_ptr(q)) == -1
        assert L.kfamd_attn_bwd_gqa_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(),
                                         lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), B,
                                         H, Hkv, T, D, scale, 1, gs, st8, A._stream_ptr(q)) == -1
        assert L.kfamd_attn_bwd_gqa_workspace(B, H, Hkv, T, D, gs) < 0
    assert L.kfamd_attn_bwd_gqa_group_split(B, 8, 3, T, D) < 0 and L.kfamd_attn_bwd_gqa_group_split(B, 8, 0, T, D) < 0
    torch.cuda.synchronize()
    assert all((x == 7.0).all() for x in (o, dq, dk, dv))
    # a wrong QKV width
    bad = torch.zeros(B, T, (8 + 2 * 2) * D + 8, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.attention_qkv(bad, 8, D, kv_heads=2)
    with pytest.raises(ValueError):
        ops.attention_qkv(torch.zeros(B, T, 3 * 8 * D, device=DEV, dtype=torch.bfloat16), 8, D, kv_heads=2)
    x = torch.zeros(B, T, 512, device=DEV, dtype=torch.bfloat16)
    wp = torch.zeros(512, 8 * D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.attn_block(x, torch.zeros(3 * 8 * D, 512, device=DEV, dtype=torch.bfloat16), None, wp, None, 8, D, kv_heads=2)
    with pytest.raises(ValueError):
        ops.attn_block(x, torch.zeros((8 + 6) * D, 512, device=DEV, dtype=torch.bfloat16), None, wp, None, 8, D, kv_heads=3)
