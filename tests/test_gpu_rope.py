"""Rotary position embeddings on the gfx950 kernels (kernels/rope_bf16.hip): the standalone rotation and the fused
rotate-and-append against the rule written out here in torch fp32 ops on the same table (EXACT equality: the
kernels switch FMA contraction off), then a rotary GPT in training and through prefill / decode_step / extend /
generate against the fp32 CPU rotary model, at the bounds tests/test_gpu_models.py and tests/test_gpu_kv_fp8.py
hold the learned-position model to (0.1 on bf16 logits; 0.1 + 2 E_q on an FP8 cache)."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
B = 2


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.uint8)


def _rule(x, table, Hq, Hkv, first, sign=1.0, limit=None):
    """The rule on CPU tensors: x bf16 [B, T, (Hq + 2 Hkv) D], row (b, t) at position first[b] + t; rows at or
    beyond ``limit`` (default: the table's row count) stay. Products and sums are separate fp32 torch ops."""
    Bx, T, _ = x.shape
    D = table.shape[1]
    limit = table.shape[0] if limit is None else limit
    out = x.clone()
    for b in range(Bx):
        for t in range(T):
            p = first[b] + t
            if p >= limit:
                continue
            c, s = table[p, :D // 2], table[p, D // 2:] * sign
            for h in range(Hq + Hkv):
                lo = x[b, t, h * D:h * D + D // 2].float()
                hi = x[b, t, h * D + D // 2:(h + 1) * D].float()
                out[b, t, h * D:h * D + D // 2] = ((lo * c) - (hi * s)).to(torch.bfloat16)
                out[b, t, h * D + D // 2:(h + 1) * D] = ((hi * c) + (lo * s)).to(torch.bfloat16)
    return out


# ---- the standalone rotation ----------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv", [(3, 3), (4, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_qkv_forward_and_backward_equal_the_rule_exactly(D, Hq, Hkv):
    from kubeflow_rm_amd import ops
    T, first = 5, [0, 37]
    W = (Hq + 2 * Hkv) * D
    table = ops.rope_table(64, D)
    x, gy = _randn(B, T, W, seed=D + Hq), _randn(B, T, W, seed=D + Hq + 1)
    pos = torch.tensor(first, dtype=torch.int32, device=DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = ops.rope_qkv(xg, table.to(DEV), Hq, Hkv, pos)
    y.backward(gy.to(DEV))
    assert torch.equal(_bits(y), _bits(_rule(x, table, Hq, Hkv, first)))
    assert torch.equal(_bits(xg.grad), _bits(_rule(gy, table, Hq, Hkv, first, sign=-1.0)))
    assert torch.equal(_bits(xg), _bits(x))  # a leaf is rotated out of place
    assert not torch.equal(_bits(y)[..., :Hq * D], _bits(x)[..., :Hq * D])
    # anything else in place; positions=None is position 0
    z = x.to(DEV)
    out = ops.rope_qkv(z, table.to(DEV), Hq, Hkv)
    assert out.data_ptr() == z.data_ptr() and torch.equal(_bits(z), _bits(_rule(x, table, Hq, Hkv, [0, 0])))
    # the torch_reference() switch runs the same rule, out of place
    with ops.torch_reference():
        r = ops.rope_qkv(x.to(DEV), table.to(DEV), Hq, Hkv, pos)
    assert torch.equal(_bits(r), _bits(y))


@pytest.mark.parametrize("D", [64, 128])
def test_rope_qkv_strided_view_poisoned_padding_and_the_table_end(D):
    from kubeflow_rm_amd import ops
    Hq, Hkv, T, first, pad = 4, 2, 5, [0, 37], 24
    W = (Hq + 2 * Hkv) * D
    table = ops.rope_table(40, D)  # rows 40, 41 of batch row 1 have no table row
    x = _randn(B, T, W, seed=3 * D)
    buf = torch.full((B + 1, T + 1, W + pad), float("nan"), dtype=torch.bfloat16, device=DEV)
    view = buf[:B, :T, 8:8 + W]
    view.copy_(x.to(DEV))
    before = _bits(buf).clone()
    out = ops.rope_qkv(view, table.to(DEV), Hq, Hkv, torch.tensor(first, dtype=torch.int32, device=DEV))
    assert out.data_ptr() == view.data_ptr()
    want = _rule(x, table, Hq, Hkv, first)
    assert torch.equal(_bits(want[1, 3:]), _bits(x[1, 3:]))  # the reference left them too
    assert torch.equal(_bits(view), _bits(want))
    after = _bits(buf)
    keep = torch.ones_like(after, dtype=torch.bool)
    keep[:B, :T, 8:8 + (Hq + Hkv) * D] = False
    assert torch.equal(after[keep], before[keep])  # v and every byte of padding
    from kubeflow_rm_amd.ops import _lib
    with pytest.raises(_lib.NativeLibraryError):  # rows that begin 8 bytes off
        ops.rope_qkv(buf[:B, :T, 4:4 + W], table.to(DEV), Hq, Hkv)
    with pytest.raises(ValueError):
        ops.rope_qkv(view, table.to(DEV), Hq, Hkv + 1)


# ---- the fused rotate-and-append --------------------------------------------------------------------
HKV, CAP = 3, 64


def _caches(kind, D, lens):
    from kubeflow_rm_amd import ops
    c = ops.KVCache(1, B, HKV, D, CAP, device=DEV, dtype=FP8 if kind == "fp8" else torch.bfloat16)
    c.set_lens(lens)
    for t in (c.k[0], c.v[0]):
        t.view(torch.uint8).fill_(0x11)
    if c.fp8:
        c.k_scale[0].fill_(-7.0)
        c.v_scale[0].fill_(-7.0)
    return c


def _check_append(cache, qkv0, qkv1, table, Hq, lens):
    """cache after kv_append(rope=table) of qkv0 (CPU, before) -> qkv1 (device, after)."""
    from kubeflow_rm_amd.ops.decode import quantize_rows
    D, T = cache.D, qkv0.shape[1]
    want = _rule(qkv0, table, Hq, HKV, lens, limit=CAP)
    assert torch.equal(_bits(qkv1), _bits(want))  # q, k rotated where the row fits; v and dropped rows as they were
    assert torch.equal(_bits(want[..., (Hq + HKV) * D:]), _bits(qkv0[..., (Hq + HKV) * D:]))
    kv = want[..., Hq * D:].view(B, T, 2, HKV, D)
    for s, codes_t, scale_t in ((0, cache.k[0], cache.k_scale[0] if cache.fp8 else None),
                                (1, cache.v[0], cache.v_scale[0] if cache.fp8 else None)):
        live = torch.zeros(B, HKV, CAP, dtype=torch.bool)
        for b, n0 in enumerate(lens):
            n = max(min(T, CAP - n0), 0)
            live[b, :, n0:n0 + n] = True
            rows = kv[b, :n, s].transpose(0, 1)  # [HKV, n, D]
            if cache.fp8:
                codes, scale = quantize_rows(rows)
                assert torch.equal(_bits(codes_t[b, :, n0:n0 + n]), _bits(codes))
                assert torch.equal(scale_t[b, :, n0:n0 + n].cpu(), scale)
            else:
                assert torch.equal(_bits(codes_t[b, :, n0:n0 + n]), _bits(rows))
        assert (codes_t.view(torch.uint8).cpu()[~live] == 0x11).all()  # every other row keeps its poison
        if cache.fp8:
            assert (scale_t.cpu()[~live] == -7.0).all()


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5, 11])  # threads: B * T * (G + 2) * HKV * D / 16; every T leaves the last block partial
def test_fused_append_equals_rotate_then_append_exactly(T, D, G, kind):
    from kubeflow_rm_amd import ops
    Hq = G * HKV
    table = ops.rope_table(CAP + 8, D)
    qkv0 = _randn(B, T, (Hq + 2 * HKV) * D, seed=T + D + G)
    assert (B * T * (Hq + 2 * HKV) * D // 16) % 256
    lens = [0, 37]
    cache = _caches(kind, D, lens)
    qkv1 = qkv0.to(DEV)
    ops.kv_append(qkv1, cache, 0, q_heads=Hq, rope=table.to(DEV))
    assert cache.lens.tolist() == lens
    _check_append(cache, qkv0, qkv1, table, Hq, lens)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_fused_append_at_the_capacity_and_strided(D, kind):
    """Rows past the capacity are dropped and left unrotated; the activation is a row-strided view."""
    from kubeflow_rm_amd import ops
    G, T = 4, 5
    Hq = G * HKV
    W = (Hq + 2 * HKV) * D
    table = ops.rope_table(CAP, D)
    qkv0 = _randn(B, T, W, seed=D + 9)
    lens = [CAP - 2, CAP]
    cache = _caches(kind, D, lens)
    buf = torch.full((B, T, W + 16), float("nan"), dtype=torch.bfloat16, device=DEV)
    view = buf[..., :W]
    view.copy_(qkv0.to(DEV))
    ops.kv_append(view, cache, 0, q_heads=Hq, rope=table.to(DEV))
    _check_append(cache, qkv0, view, table, Hq, lens)
    assert torch.isnan(buf[..., W:].float()).all()
    with pytest.raises(ValueError):  # a table shorter than the cache
        ops.kv_append(view, cache, 0, q_heads=Hq, rope=table[:CAP - 1].to(DEV))


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_append_without_rope_is_the_plain_append(kind):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.decode import quantize_rows
    D, T, lens = 64, 5, [0, 37]
    qkv0 = _randn(B, T, 3 * HKV * D, seed=21)
    cache = _caches(kind, D, lens)
    qkv1 = qkv0.to(DEV)
    ops.kv_append(qkv1, cache, 0, rope=None)
    assert torch.equal(_bits(qkv1), _bits(qkv0))
    kv = qkv0.view(B, T, 3, HKV, D)
    for b, n0 in enumerate(lens):
        for s, t in ((1, cache.k[0]), (2, cache.v[0])):
            rows = kv[b, :, s].transpose(0, 1)
            assert torch.equal(_bits(t[b, :, n0:n0 + T]), _bits(quantize_rows(rows)[0] if cache.fp8 else rows))


# ---- the model: training ----------------------------------------------------------------------------
def _cfg(n_heads, n_kv_heads, dtype, pos="rope"):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=n_heads, d_ff=1024, max_seq=256, dtype=dtype,
                     n_kv_heads=n_kv_heads, pos=pos)


MODELS = [(4, None), (2, None), (4, 2)]
IDS = ["D64", "D128", "D64-G2"]


@pytest.mark.parametrize("n_heads,n_kv", MODELS, ids=IDS)
def test_rotary_gpt_forward_backward_matches_fp32_reference(n_heads, n_kv):
    """tests/test_gpu_models.py's check and bounds, on the rotary model."""
    from kubeflow_rm_amd.models import GPT
    torch.manual_seed(0)
    idx = torch.randint(0, 512, (2, 128))
    tgt = torch.randint(0, 512, (2, 128))
    gpu = GPT(_cfg(n_heads, n_kv, torch.bfloat16), device=DEV)
    assert gpu.pos is None and gpu.rope_table.is_cuda and gpu.rope_table.dtype == torch.float32
    logits, loss = gpu(idx.cuda(), tgt.cuda())
    loss.backward()
    ref = GPT(_cfg(n_heads, n_kv, torch.float32))
    rlogits, rloss = ref(idx, tgt)
    rloss.backward()
    err = (logits.float().cpu() - rlogits.detach()).abs().max().item()
    print(f"rotary gpt: loss {loss.item():.4f} / {rloss.item():.4f}, logits max-abs {err:.4f}")
    assert abs(loss.item() - rloss.item()) < 2e-2 * abs(rloss.item())
    assert err < 0.1, err
    for name in ("ln1.weight", "qkv.weight"):
        g = gpu.blocks[0].get_parameter(name).grad.float().cpu()
        r = ref.blocks[0].get_parameter(name).grad
        worst = ((g - r).abs().max() / r.abs().max()).item()
        print(f"  blocks[0].{name}.grad: max-abs error / max |reference| {worst:.4f}")
        assert torch.allclose(g, r, atol=5e-2 * r.abs().max().item() + 1e-3), name


@pytest.mark.parametrize("hd,h", [(64, 4), (128, 2)])
def test_attn_block_with_rope_equals_the_separate_ops_bit_for_bit(hd, h):
    from kubeflow_rm_amd import ops
    Bm, T, d = 2, 72, h * hd
    x = _randn(Bm, T, d, seed=1).to(DEV)
    wqkv, wproj = (_randn(3 * d, d, seed=2) * 0.05).to(DEV), (_randn(d, d, seed=3) * 0.05).to(DEV)
    bqkv, bproj = (_randn(3 * d, seed=4) * 0.1).to(DEV), (_randn(d, seed=5) * 0.1).to(DEV)
    table = ops.rope_table(128, hd, device=DEV)
    with torch.no_grad():
        fused = ops.attn_block(x, wqkv, bqkv, wproj, bproj, h, hd, residual=x, rope=table)
        qkv = ops.rope_qkv(ops.linear(x, wqkv, bqkv), table, h, h)
        sep = ops.linear(ops.attention_qkv(qkv, h, hd, causal=True), wproj, bproj, residual=x)
        plain = ops.attn_block(x, wqkv, bqkv, wproj, bproj, h, hd, residual=x)
    assert torch.equal(_bits(fused), _bits(sep)) and not torch.equal(_bits(fused), _bits(plain))
    # backward: the fused node against autograd through the separate ops
    leaves = [t.clone().requires_grad_(True) for t in (x, wqkv, bqkv, wproj, bproj)]
    ops.attn_block(*leaves, h, hd, rope=table).float().square().sum().backward()
    leaves2 = [t.clone().requires_grad_(True) for t in (x, wqkv, bqkv, wproj, bproj)]
    q2 = ops.rope_qkv(ops.linear(leaves2[0], leaves2[1], leaves2[2]), table, h, h)
    ops.linear(ops.attention_qkv(q2, h, hd, causal=True), leaves2[3], leaves2[4]).float().square().sum().backward()
    for a, b_ in zip(leaves, leaves2):
        rel = ((a.grad.float() - b_.grad.float()).norm() / b_.grad.float().norm()).item()
        assert rel < 1e-2, rel  # the same kernels in another order of launches (the pair wgrad): bf16 rounding


# ---- the model: generation --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=MODELS, ids=IDS)
def models(request):
    from kubeflow_rm_amd.models import GPT
    h, hkv = request.param
    return GPT(_cfg(h, hkv, torch.bfloat16), device=DEV).eval(), GPT(_cfg(h, hkv, torch.float32)).eval()


def _teacher_forced(gpu, seq, T0, kv_dtype=None):
    """prefill(T0) + 4 decode steps + extend(T = 3) + extend(40 tokens, chunk=32): logits from row T0 - 1 on."""
    Bm, total = seq.shape
    cache = gpu.new_cache(Bm, total, kv_dtype=kv_dtype)
    got, at = [gpu.prefill(seq[:, :T0].to(DEV), cache).view(Bm, 1, -1)], T0
    for _ in range(4):
        got.append(gpu.decode_step(seq[:, at].to(DEV), cache).view(Bm, 1, -1))
        at += 1
    got.append(gpu.extend(seq[:, at:at + 3].to(DEV), cache))
    got.append(gpu.extend(seq[:, at + 3:].to(DEV), cache, chunk=32))
    assert cache.lens.tolist() == [total] * Bm
    return torch.cat(got, 1).float().cpu()


def test_rotary_cache_paths_match_the_fp32_full_forward(models):
    gpu, ref = models
    Bm, T0 = 2, 40
    seq = torch.randint(0, 512, (Bm, T0 + 4 + 3 + 40), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)[:, T0 - 1:]
    errs = (_teacher_forced(gpu, seq, T0) - want).abs().amax(dim=(0, 2))
    print(f"rotary cache paths, per-position max-abs: max {errs.max().item():.4f}")
    assert errs.max().item() < 0.1, errs.tolist()
    # the FP8 cache: tests/test_gpu_kv_fp8.py's bound, 0.1 + 2 E_q with E_q the fp32 model's own fp8-cache error
    c8, c32 = ref.new_cache(Bm, seq.shape[1], kv_dtype=FP8), ref.new_cache(Bm, seq.shape[1])
    with torch.no_grad():
        e_q = (ref.extend(seq, c8) - ref.extend(seq, c32)).abs().max().item()
    errs8 = (_teacher_forced(gpu, seq, T0, kv_dtype=FP8) - want).abs().amax(dim=(0, 2))
    print(f"rotary fp8-cache per-position max-abs: max {errs8.max().item():.4f}, E_q {e_q:.4f}")
    assert e_q > 0 and errs8.max().item() < 0.1 + 2 * e_q, (errs8.tolist(), e_q)


def _hand_loop(model, idx, new, kv_dtype=None):
    cache = model.new_cache(idx.shape[0], idx.shape[1] + new, kv_dtype=kv_dtype)
    logits = [model.prefill(idx, cache).clone()]
    toks = [idx, logits[0].argmax(-1).view(-1, 1)]
    for _ in range(new - 1):
        logits.append(model.decode_step(toks[-1].view(-1), cache).clone())
        toks.append(logits[-1].argmax(-1).view(-1, 1))
    return torch.cat(toks, 1), logits


@pytest.mark.parametrize("kv_dtype", [None, FP8], ids=["bf16", "fp8"])
def test_graphed_rotary_step_equals_eager(models, kv_dtype):
    """One captured decode step replayed over two prompts of different lengths: the position comes from the
    device-side lens, so the logits are bit-identical to the eager steps at every position."""
    gpu, _ = models
    Bm, new, cap = 2, 8, 64
    cache = gpu.new_cache(Bm, cap, kv_dtype=kv_dtype)
    step = None
    for seed, T0 in ((1, 40), (2, 17)):
        idx = torch.randint(0, 512, (Bm, T0), generator=torch.Generator().manual_seed(seed)).to(DEV)
        want_toks, want_logits = _hand_loop(gpu, idx, new, kv_dtype)
        cache.reset()
        logits = gpu.prefill(idx, cache)
        if step is None:
            step = gpu.graphed_decode_step(cache)
        toks = [idx]
        for i in range(new):
            torch.testing.assert_close(logits, want_logits[i], rtol=0, atol=0)
            toks.append(logits.argmax(-1).view(-1, 1))
            if i + 1 < new:
                logits = step(toks[-1].view(-1))
        assert torch.equal(torch.cat(toks, 1), want_toks)


def test_rotary_generate_graph_fused_sampler_and_the_rest(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    eager = gpu.generate(idx, 8)
    assert torch.equal(eager, _hand_loop(gpu, idx, 8)[0])
    assert torch.equal(gpu.generate(idx, 8, graph=True), eager)
    kw = dict(sampler="fused", temperature=0.8, top_k=20, top_p=0.9)
    a = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), graph=True, **kw)
    b_ = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), **kw)
    assert a.shape == (2, 20) and torch.equal(a, b_)
    # everything at once: graph, fused sampler, FP8 cache, FP8 weights, a chunked prefill
    kw.update(kv_dtype=FP8, weight_dtype=FP8, prefill_chunk=17)
    c = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), graph=True, **kw)
    d = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), **kw)
    assert torch.equal(c, d) and torch.equal(c[:, :12], idx)
    # draft-and-verify with rewinds: a self-draft accepts every proposal
    one = idx[:1]
    out, stats = gpu.generate(one, 12, draft=gpu, lookahead=4, return_stats=True)
    assert stats["accepted"] == stats["proposed"] and torch.equal(out, gpu.generate(one, 12))
