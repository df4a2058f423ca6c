"""The ring-buffer KV cache on the GPU kernels (the ring rule: the docstring of ``ops/decode.py``): the ring appends slot
by slot, the RING attention kernels row by row at laps, wraps, split boundaries and positions up to 2^20, with every
slot no row may see poisoned (the slots after key ``lens[b] - 1`` above all) and guard rows around ``out``; ring against
flat; a grid that does not depend on the position, through a captured step replayed across the wrap; rewind; the model.

Reference: an fp32 masked softmax written from the rule over the token stream itself, never over the cache: row ``b``'s
stream is kept as its last C positions, index ``i`` standing for absolute key ``lens[b] - C + i``. For FP8 the stream is
``dequantize_rows(quantize_rows(stream))``. Bounds (tests/test_gpu_window.py): max-abs < 2e-2, rel-l2 < 8e-3, lse within
1e-3, bf16 logits within 0.1."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV = 3, 2
FP8 = torch.float8_e4m3fn
ABS, REL, LSE, LOGITS = 2e-2, 8e-3, 1e-3, 0.1
SENTINEL = 123.0
FAR = 2 ** 20 + 5


def _S():
    from kubeflow_rm_amd.ops import decode
    return decode.SPLIT_KEYS


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


_STREAMS: dict = {}


def _stream(D, C, kind):
    """(k, v [B, HKV, C, D] bf16, and what a cache of ``kind`` stands for: themselves, or the dequantised codes), drawn
    once per shape and never changed."""
    from kubeflow_rm_amd.ops.decode import dequantize_rows, quantize_rows
    if (D, C, kind) not in _STREAMS:
        k, v = _randn(B, HKV, C, D, seed=D + C), _randn(B, HKV, C, D, seed=D + C + 1)
        kr, vr = (k, v) if kind == "bf16" else (dequantize_rows(*quantize_rows(k)), dequantize_rows(*quantize_rows(v)))
        _STREAMS[D, C, kind] = (k, v, kr.float(), vr.float())
    return _STREAMS[D, C, kind]


def _new_ring(D, C, kind, layers=1):
    from kubeflow_rm_amd import ops
    return ops.KVCache(layers, B, HKV, D, C, device=DEV, dtype=FP8 if kind == "fp8" else torch.bfloat16, ring=True)


def _positions(lens, C):
    """[B, C]: the absolute key that index i of row b's stream stands for (negative: before the sequence's start)."""
    return torch.tensor(lens, device=DEV).view(-1, 1) - C + torch.arange(C, device=DEV).view(1, C)


def _seen(lens, T, W, C):
    """[B, T, C] bool over the stream's indices, straight from the rule: key j for row i iff max(0, L - W) <= j < L."""
    L = (torch.tensor(lens, device=DEV).view(-1, 1) - T + torch.arange(T, device=DEV).view(1, T) + 1).unsqueeze(-1)
    j = _positions(lens, C).unsqueeze(1)
    return (j >= (L - W).clamp_min(0)) & (j < L) & (j >= 0)


def _ref(q, kr, vr, lens, W):
    """q [B, T, Hq, D] -> (o [B, T, Hq, D] fp32, lse [B, T, Hq]); a row with no key gives zeros, lse = -inf."""
    T, Hq, D = q.shape[1:]
    G = Hq // HKV
    kf, vf = kr.repeat_interleave(G, dim=1), vr.repeat_interleave(G, dim=1)
    s = torch.einsum("bthd,bhjd->bhtj", q.float(), kf) / math.sqrt(D)
    s = s.masked_fill(~_seen(lens, T, W, kr.shape[2]).unsqueeze(1), float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.masked_fill(lse == float("-inf"), 0.0).unsqueeze(-1))
    return (p @ vf).transpose(1, 2), lse.transpose(1, 2)


def _fill(cache, k, v, lens, T, W, poison=True):
    """Slot j % C <- key j of the stream for every key some row of the call sees; every other slot (stale positions
    below every window, negative positions, and the slots after key lens[b] - 1) NaN, or 0x7F codes and NaN scales."""
    from kubeflow_rm_amd.ops.decode import quantize_rows
    C = cache.capacity
    slot = (_positions(lens, C) % C).view(B, 1, C, 1)
    live = _seen(lens, T, W, C).any(1).view(B, 1, C, 1) if poison else (_positions(lens, C) >= 0).view(B, 1, C, 1)
    idx = slot.expand(B, HKV, C, k.shape[-1])
    for src, dst, sc in ((k, cache.k[0], cache.k_scale), (v, cache.v[0], cache.v_scale)):
        if cache.fp8:
            codes, scale = quantize_rows(src)
            codes = torch.where(live, codes.view(torch.uint8), torch.full_like(codes.view(torch.uint8), 0x7F))
            scale = torch.where(live[..., 0], scale, torch.full_like(scale, float("nan")))
            dst.view(torch.uint8).scatter_(2, idx, codes)
            sc[0].scatter_(2, slot[..., 0].expand(B, HKV, C), scale)
        else:
            dst.scatter_(2, idx, torch.where(live, src, torch.full_like(src, float("nan"))))
    cache.set_lens(lens)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _check(o, lse, ref, ref_lse, what):
    err, rel = (o.float() - ref).abs().max().item(), _rel(o, ref)
    live = torch.isfinite(ref_lse)
    lerr = (lse[live] - ref_lse[live]).abs().max().item() if live.any() else 0.0
    print(f"ring {what}: max-abs {err:.3e} rel-l2 {rel:.3e} lse {lerr:.3e}")
    assert torch.isfinite(o.float()).all(), what
    assert err < ABS and rel < REL, (what, err, rel)
    assert torch.equal(torch.isfinite(lse), live) and lerr < LSE, (what, lerr)


def _guarded(q):
    if q.dim() == 4:
        Bq, T, Hq, D = q.shape
        buf = torch.full((Bq, T + 2, Hq + 2, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
        return buf, buf[:, 1:T + 1, 1:Hq + 1]
    Bq, Hq, D = q.shape
    buf = torch.full((Bq, Hq + 2, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    return buf, buf[:, 1:Hq + 1]


def _guards_intact(buf, out):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep.as_strided(out.shape, out.stride(), out.storage_offset() - buf.storage_offset()).fill_(False)
    return bool((buf[keep] == SENTINEL).all())


def _run(op, q, cache, D, kind, lens, W, what):
    """One (lens, W) case: fill and poison, the returning call and the call with ``out=`` into guarded memory."""
    k, v, kr, vr = _stream(D, cache.capacity, kind)
    T = q.shape[1] if q.dim() == 4 else 1
    assert W + T - 1 <= cache.capacity
    _fill(cache, k, v, lens, T, W)
    ref, ref_lse = _ref(q if q.dim() == 4 else q.unsqueeze(1), kr, vr, lens, W)
    if q.dim() == 3:
        ref, ref_lse = ref[:, 0], ref_lse[:, 0]
    o, lse = op(q, cache, 0, return_lse=True, window=W)
    assert o.shape == q.shape and lse.shape == q.shape[:-1]
    _check(o, lse, ref, ref_lse, f"{what} C={cache.capacity} lens={lens} W={W}")
    buf, out = _guarded(q)
    assert op(q, cache, 0, out=out, window=W) is out
    assert torch.equal(out, o), what  # the same launch: the same bits
    assert _guards_intact(buf, out), what


def _cases(C, T):
    """(lens, W) of one capacity and token count: laps, the wrap, W + T - 1 == C, a lower bound on a split boundary."""
    S = _S()
    out = []
    for W in (1, 5, 64, S - 1, S + 3, C - T + 1):
        if W < 1 or W + T - 1 > C:
            continue
        out.append(([W - 1, C, 2 * C + 17], W))
        out.append(([C - 1, C + 1, 3 * C + S], W))
        # a far position; lens - T + 1 - W on a split boundary; a window across the physical end of the buffer
        out.append(([FAR, 3 * S + W + T - 1, 2 * C + max(W // 2, 1)], W))
    return out


# ---- 1. the appends --------------------------------------------------------------------------------------

@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_ring_append_writes_its_slots_and_nothing_else(D, kind, rope):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.decode import quantize_rows
    from kubeflow_rm_amd.ops.rope import rotate_torch
    S, Hq = _S(), 2 * HKV
    for C in (S, 2 * S):
        cache = _new_ring(D, C, kind)
        table = ops.rope_table(4 * C + 200, D, device=DEV) if rope else None
        for T, lens in ((1, [C - 1, 2 * C, 5]), (7, [C - 3, C + 9, 3 * C - 7]), (16, [0, 2 * C - 3, C]),
                        (100, [C - 3, 3 * C + 1, 17]), (7, [FAR, C - 3, 2 * C])):
            if rope and max(lens) + T > table.shape[0]:
                lens = [n % (3 * C) for n in lens]  # the table bounds a rotary position
            for t in (cache.k[0], cache.v[0]):
                t.view(torch.uint8).random_(0, 120)  # finite in both formats
            if cache.fp8:
                cache.k_scale[0].uniform_(), cache.v_scale[0].uniform_()
            cache.set_lens(lens)
            qkv = _randn(B, T, (Hq + 2 * HKV) * D, seed=T + C)
            want = qkv.clone()
            if rope:
                want = rotate_torch(qkv, table, Hq, HKV, positions=cache.lens)
            before = [t.clone() for t in (cache.k[0], cache.v[0], *((cache.k_scale[0], cache.v_scale[0]) if cache.fp8
                                                                     else ()))]
            ops.kv_append(qkv, cache, 0, q_heads=Hq, rope=table)
            if rope:  # q and k rotated in place
                assert torch.equal(qkv, want)
            x = want[:, :, Hq * D:].view(B, T, 2, HKV, D)
            slot = (torch.tensor(lens, device=DEV).view(-1, 1) + torch.arange(T, device=DEV).view(1, T)) % C  # [B, T]
            bidx = torch.arange(B, device=DEV).view(-1, 1).expand(B, T)
            touched = torch.zeros(B, C, dtype=torch.bool, device=DEV)
            touched[bidx, slot] = True
            for s, (codes, scales) in enumerate(((cache.k[0], cache.k_scale), (cache.v[0], cache.v_scale))):
                got = (codes.view(torch.uint8) if cache.fp8 else codes)[bidx, :, slot]  # [B, T, HKV, D]
                if cache.fp8:
                    c, sc = (t.to(DEV) for t in quantize_rows(x[:, :, s].cpu()))  # the CPU's IEEE division
                    assert torch.equal(got, c.view(torch.uint8)), (C, T, lens, s)
                    assert torch.equal(scales[0][bidx, :, slot], sc), (C, T, lens, s)
                else:
                    assert torch.equal(got, x[:, :, s]), (C, T, lens, s)
            after = [cache.k[0], cache.v[0], *((cache.k_scale[0], cache.v_scale[0]) if cache.fp8 else ())]
            for a, b0 in zip(after, before):  # nothing outside the T target slots changed
                keep = ~touched.view(B, 1, C, *([1] * (a.dim() - 3))).expand_as(a)
                a8, b8 = (a.view(torch.uint8), b0.view(torch.uint8)) if a.dtype == FP8 else (a, b0)
                assert torch.equal(a8[keep], b8[keep]), (C, T, lens)
            assert cache.lens.tolist() == lens  # not advanced


# ---- 2 - 4. attention: positions, poison, guard rows ---------------------------------------------------------

@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_ring_decode(D, kind):
    from kubeflow_rm_amd import ops
    for C in (_S(), 2 * _S()):
        cache, q = _new_ring(D, C, kind), _randn(B, HKV, D, seed=3)
        for lens, W in _cases(C, 1):
            _run(ops.attention_decode, q, cache, D, kind, lens, W, "decode")


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [2, 8, 16])
def test_ring_extend(T, D, kind):
    from kubeflow_rm_amd import ops
    for C in (_S(), 2 * _S()):
        cache, q = _new_ring(D, C, kind), _randn(B, T, HKV, D, seed=T)
        for lens, W in _cases(C, T):
            _run(ops.attention_extend, q, cache, D, kind, lens, W, f"extend T={T}")


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [16, 129, 200])
def test_ring_chunk(T, D, kind):
    from kubeflow_rm_amd import ops
    for C in (_S(), 2 * _S()):
        cache, q = _new_ring(D, C, kind), _randn(B, T, HKV, D, seed=T)
        for lens, W in _cases(C, T):
            _run(ops.attention_chunk, q, cache, D, kind, lens, W, f"chunk T={T}")


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G,T,forced", [(4, 1, None), (4, 2, "valu"), (4, 4, "valu"), (4, 4, None), (8, 1, None),
                                        (8, 2, None), (8, 25, "chunk")])
def test_ring_grouped(G, T, forced, D, kind, monkeypatch):
    """G = 4 below 8 rows and with the MFMA route switched off: the grouped VALU form; G = 8: the MFMA route."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    if forced == "valu":
        monkeypatch.setattr(decode, "GQA_MFMA_MIN_ROWS", None)
    for C in (_S(), 2 * _S()):
        cache = _new_ring(D, C, kind)
        q = _randn(B, T, G * HKV, D, seed=G + T)
        for lens, W in _cases(C, T):
            if T == 1:
                _run(ops.attention_decode, q[:, 0], cache, D, kind, lens, W, f"decode G={G}")
            op = ops.attention_chunk if forced == "chunk" else ops.attention_extend
            _run(op, q, cache, D, kind, lens, W, f"{op.__name__} G={G} T={T} {forced}")


# ---- 5. ring against flat ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_ring_against_the_flat_cache(D, kind):
    from kubeflow_rm_amd import ops
    S = _S()
    C, lens = 2 * S, [2 * S + 17, 4 * S + 3, 3 * S]
    k, v, _, _ = _stream(D, C, kind)
    ring = _new_ring(D, C, kind)
    flat = ops.KVCache(1, B, HKV, D, max(lens), device=DEV, dtype=ring.dtype)
    for W in (5, S - 1, S + 3):
        for name, T, G in (("attention_decode", 1, 1), ("attention_extend", 8, 1), ("attention_extend", 1, 4),
                           ("attention_chunk", 129, 1), ("attention_extend", 2, 8)):
            _fill(ring, k, v, lens, T, W, poison=False)
            # the flat cache holds the same stream at its absolute rows (the last C positions of each row)
            pos = _positions(lens, C)  # all >= 0 here
            for src, dst, sc, rsc in ((ring.k[0], flat.k[0], flat.k_scale, ring.k_scale),
                                      (ring.v[0], flat.v[0], flat.v_scale, ring.v_scale)):
                for b in range(B):
                    if ring.fp8:
                        dst.view(torch.uint8)[b][:, pos[b]] = src.view(torch.uint8)[b][:, pos[b] % C]
                        sc[0][b][:, pos[b]] = rsc[0][b][:, pos[b] % C]
                    else:
                        dst[b][:, pos[b]] = src[b][:, pos[b] % C]
            flat.set_lens(lens)
            q = _randn(B, T, G * HKV, D, seed=T + G)
            q = q[:, 0] if name == "attention_decode" else q
            op = getattr(ops, name)
            o, lse = op(q, ring, 0, return_lse=True, window=W)
            fo, flse = op(q, flat, 0, return_lse=True, window=W)
            _check(o, lse, fo.float(), flse, f"ring vs flat {name} T={T} G={G} W={W}")
            print(f"ring vs flat {name} T={T} G={G} W={W} {kind} D={D}: bit-equal o {torch.equal(o, fo)}, "
                  f"lse {torch.equal(lse, flse)}")  # reported, not asserted


# ---- 6. the grid does not depend on the position -----------------------------------------------------------

def test_ring_grid_entry_points_take_no_position():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import _lib
    L, S = _lib.lib(), _S()
    assert L.kfamd_attn_ring_nsplit(1, 1) == 2 and L.kfamd_attn_ring_nsplit(S, 1) == 2
    assert L.kfamd_attn_ring_nsplit(S, 2) == 3 and L.kfamd_attn_ring_nsplit(1000, 16) == 5
    cache = _new_ring(64, 2 * S, "bf16")
    q, sizes = _randn(B, 4, HKV, 64, seed=1), []
    k, v, _, _ = _stream(64, 2 * S, "bf16")
    for lens in ([0, 1, 2], [S, 2 * S, 3 * S + 1], [FAR, FAR + 1, 7]):
        _fill(cache, k, v, lens, 4, 200, poison=False)
        ops.attention_decode(q[:, 0], cache, 0, window=200)
        ops.attention_extend(q, cache, 0, window=200)
        ops.attention_chunk(q, cache, 0, window=200)
        sizes.append((cache.workspace.data_ptr(), cache.extend_workspace.data_ptr(), cache.chunk_workspace.data_ptr(),
                      cache.nbytes, L.kfamd_attn_ring_nsplit(200, 4), L.kfamd_attn_chunk_ring_nsplit(B, HKV, 1, 4, 200),
                      L.kfamd_attn_decode_ring_workspace(B, HKV, 64, 200),
                      L.kfamd_attn_extend_ring_workspace(B, HKV, 1, 64, 4, 200),
                      L.kfamd_attn_chunk_ring_workspace(B, HKV, 1, 64, 4, 200)))
    assert sizes[0] == sizes[1] == sizes[2]  # the same workspaces and counts whatever lens is
    assert cache.workspace.numel() == L.kfamd_attn_decode_ring_workspace(B, HKV, 64, 200)


def _small(window=200, **kw):
    from kubeflow_rm_amd.models import GPT, GPTConfig
    cfg = GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=512, max_seq=2048, window=window,
                    pos="rope", n_kv_heads=2, norm="rms", mlp="swiglu", **kw)
    return GPT(cfg, device=DEV).eval()


def test_captured_ring_step_replays_across_the_wrap():
    S = _S()
    m = _small()
    g = torch.Generator(device="cpu").manual_seed(5)
    toks = torch.randint(0, 512, (2, 100 + S + 40), generator=g).to(DEV)
    graphed_cache, eager_cache = m.new_cache(2, S, ring=True), m.new_cache(2, S, ring=True)
    for c in (graphed_cache, eager_cache):
        for t0 in range(0, 100, 50):
            m.extend(toks[:, t0:t0 + 50], c, last_only=True, chunk=50)  # 200 + 50 - 1 <= 256
    step = m.graphed_decode_step(graphed_cache)
    assert not graphed_cache._pinned
    for i in range(S + 40):
        lg = step(toks[:, 100 + i])
        le = m.decode_step(toks[:, 100 + i], eager_cache)
        if i % 50 == 0 or i == S + 39:
            err = (lg.float() - le.float()).abs().max().item()
            print(f"ring graphed step {i}: logits max-abs {err:.3e}")
            assert torch.isfinite(lg.float()).all() and err < LOGITS, (i, err)
    assert graphed_cache.lens.tolist() == [100 + S + 40] * 2 == eager_cache.lens.tolist()
    assert graphed_cache._bound == 100 + S + 40


def test_captured_fp8_ring_step_matches_the_eager_ring_step():
    """What generate(ring=True, graph=True, kv_dtype=FP8) replays: the captured step on an FP8 ring against the eager step
    on a twin ring, across the wrap, every 50th step and the last."""
    S = _S()
    m = _small()
    toks = torch.randint(0, 512, (2, 100 + S + 40), generator=torch.Generator(device="cpu").manual_seed(8)).to(DEV)
    graphed_cache, eager_cache = m.new_cache(2, S, kv_dtype=FP8, ring=True), m.new_cache(2, S, kv_dtype=FP8, ring=True)
    for c in (graphed_cache, eager_cache):
        for t0 in range(0, 100, 50):
            m.extend(toks[:, t0:t0 + 50], c, last_only=True, chunk=50)
    step = m.graphed_decode_step(graphed_cache)
    for i in range(S + 40):
        lg = step(toks[:, 100 + i])
        le = m.decode_step(toks[:, 100 + i], eager_cache)
        if i % 50 == 0 or i == S + 39:
            err = (lg.float() - le.float()).abs().max().item()
            print(f"ring graphed fp8 step {i}: logits max-abs {err:.3e}")
            assert torch.isfinite(lg.float()).all() and err < LOGITS, (i, err)
    assert graphed_cache.lens.tolist() == [100 + S + 40] * 2 == eager_cache.lens.tolist()
    for a, b in zip(graphed_cache.k + graphed_cache.k_scale, eager_cache.k + eager_cache.k_scale):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))  # the same codes and scales in every slot


# ---- 7. rewind -----------------------------------------------------------------------------------------

def test_ring_rewind_after_an_extend():
    S = _S()
    m = _small()
    g = torch.Generator(device="cpu").manual_seed(6)
    toks = torch.randint(0, 512, (2, S + 64), generator=g).to(DEV)
    a, b = m.new_cache(2, S, ring=True), m.new_cache(2, S, ring=True)
    n = S + 30  # past the wrap
    for c in (a, b):
        for t0 in range(0, n, 50):
            m.extend(toks[:, t0:min(t0 + 50, n)], c, last_only=True, chunk=50)
    m.extend(toks[:, n:n + 4], a)  # four rows, three of them dropped again
    a.rewind(3)
    m.extend(toks[:, n:n + 1], b)  # the path that never appended the three
    assert a.lens.tolist() == b.lens.tolist() == [n + 1] * 2
    la, lb = m.decode_step(toks[:, n + 10], a), m.decode_step(toks[:, n + 10], b)
    err = (la.float() - lb.float()).abs().max().item()
    print(f"ring rewind: logits max-abs {err:.3e}")
    assert err < LOGITS


# ---- 8. the model ---------------------------------------------------------------------------------------

def _model_case(kv_dtype, new):
    """The flat cache's greedy tokens fed to a flat cache and to the ring ``generate(ring=True, prefill_chunk=17)``
    makes (W = 200: 256 slots): the worst per-step logit difference, and the ring."""
    m = _small()
    idx = torch.randint(0, 512, (2, 300), generator=torch.Generator(device="cpu").manual_seed(7)).to(DEV)
    assert m._ring_capacity(17) == 256
    flat, ring = m.new_cache(2, 300 + new, kv_dtype=kv_dtype), m.new_cache(2, 256, kv_dtype=kv_dtype, ring=True)
    lf = m.extend(idx, flat, last_only=True, chunk=17)
    lr = m.extend(idx, ring, last_only=True, chunk=17)
    worst = 0.0
    for _ in range(new):
        worst = max(worst, (lf.float() - lr.float()).abs().max().item())
        tok = lf.argmax(-1)
        lf, lr = m.decode_step(tok, flat), m.decode_step(tok, ring)
    print(f"ring model {kv_dtype}: per-step logits max-abs {worst:.3e} over {new} steps")
    assert worst < LOGITS and ring.lens.tolist() == [300 + new] * 2 and ring.nbytes < flat.nbytes
    return m, idx, ring


def _workspaces(c):
    return sum(t.numel() for t in (c.workspace, c.extend_workspace, c.chunk_workspace) if t is not None)


def test_ring_model_generates_past_the_capacity_twice():
    new = 2 * 256 + 20  # the ring of 256 slots is passed twice after the prompt
    m, idx, ring = _model_case(None, new)
    h, hd = m.blocks[0].local_kv_heads, m.cfg.head_dim
    assert ring.nbytes == 2 * 2 * 2 * h * 256 * hd * 2 + _workspaces(ring)  # K and V, layers, B, heads, slots, D, bf16
    out = m.generate(idx, new, ring=True, prefill_chunk=17)
    assert out.shape == (2, 300 + new) and torch.equal(out[:, :300], idx)
    assert int(out.max()) < 512 and int(out.min()) >= 0
    assert torch.equal(out, m.generate(idx, new, ring=True, prefill_chunk=17))  # repeatable


def test_ring_model_graph_fused_sampler_fp8_cache():
    new = 2 * 256 + 20
    m, idx, ring = _model_case(FP8, 256 + 20)
    h, hd = m.blocks[0].local_kv_heads, m.cfg.head_dim
    assert ring.nbytes == 2 * 2 * 2 * h * 256 * (hd + 4) + _workspaces(ring)  # codes and one fp32 scale per row
    out = m.generate(idx, new, ring=True, prefill_chunk=17, graph=True, sampler="fused", kv_dtype=FP8, temperature=0.8,
                     top_k=40, generator=torch.Generator(device="cpu").manual_seed(1))
    assert out.shape == (2, 300 + new) and torch.equal(out[:, :300], idx)
    assert int(out.max()) < 512 and int(out.min()) >= 0


def test_ring_errors_on_the_gpu():
    from kubeflow_rm_amd import ops
    S = _S()
    ring = _new_ring(64, S, "bf16")
    ring.set_lens([S, 2 * S, 5])
    q = _randn(B, 4, HKV, 64, seed=2)
    for op, x in ((ops.attention_decode, q[:, 0]), (ops.attention_extend, q), (ops.attention_chunk, q)):
        with pytest.raises(ValueError):
            op(x, ring, 0)  # no window
        with pytest.raises(ValueError):
            op(x, ring, 0, window=8, t_bound=S)
        if x.dim() == 4:
            with pytest.raises(ValueError):
                op(x, ring, 0, window=S)  # W + T - 1 > C
    with pytest.raises(ValueError):
        ops.attention_decode(q[:, 0], ring, 0, window=S + 1)
    with pytest.raises(ValueError):
        ops.KVCache(1, B, HKV, 64, S + 64, device=DEV, ring=True)
