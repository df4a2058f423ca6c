"""The FP8 KV cache on the torch path (CPU tensors): the storage format (quantize_rows / dequantize_rows),
the quantising kv_append, attention over the dequantised rows, KVCache.nbytes, and GPT.generate /
extend / rewind / drafting with kv_dtype=torch.float8_e4m3fn on an fp32 model."""
import math

import pytest
import torch
import torch.nn.functional as F

FP8 = torch.float8_e4m3fn


def format_rows(D, seed):
    """The format's test inputs: randn bf16 rows, rows with one element x 100, rows scaled by 1e-3, and an
    all-zero row (the last one). [N, D] bf16."""
    g = torch.Generator().manual_seed(seed)
    plain = torch.randn(24, D, generator=g)
    spiked = torch.randn(24, D, generator=g)
    spiked[torch.arange(24), torch.randint(0, D, (24,), generator=g)] *= 100
    small = torch.randn(24, D, generator=g) * 1e-3
    return torch.cat([plain, spiked, small, torch.zeros(1, D)]).to(torch.bfloat16)


def check_format(x, codes, scale):
    """Every property the format fixes, for rows x [N, D] (bf16) stored as codes [N, D] / scale [N]."""
    from kubeflow_rm_amd.ops import decode
    x = x.float()
    amax = x.abs().amax(-1)
    zero = amax == 0
    # scale == amax / 448 (1 for an all-zero row)
    want = torch.where(zero, torch.ones_like(amax), amax / 448)
    rel = ((scale - want).abs() / want).max().item()
    print(f"scale: max relative difference {rel:.3e}")
    assert rel <= 1e-6, rel
    # dequantisation error: half an e4m3 ulp of a normal value, or half the smallest subnormal (2^-9)
    deq = decode.dequantize_rows(codes, scale)
    bound = torch.maximum(x.abs() * 2.0 ** -4, scale.unsqueeze(-1) * 2.0 ** -10) * 1.001
    ratio = ((deq - x).abs() / bound.clamp_min(1e-45)).max().item()
    print(f"dequantisation: worst error / bound {ratio:.7f}")
    assert ((deq - x).abs() <= bound).all(), ratio
    # the element that holds the row's amax takes the largest finite code; a zero row is all zero codes
    raw = codes.view(torch.uint8)
    top = raw.gather(1, x.abs().argmax(-1, keepdim=True)).squeeze(1)
    assert ((top[~zero] & 0x7F) == 0x7E).all(), top
    assert (raw[zero] == 0).all() and (scale[zero] == 1).all()
    assert zero.any() and (~zero).any()


@pytest.mark.parametrize("D", [64, 128])
def test_quantize_rows_format(D):
    from kubeflow_rm_amd.ops import decode
    x = format_rows(D, seed=D)
    codes, scale = decode.quantize_rows(x)
    assert codes.dtype == FP8 and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    check_format(x, codes, scale)
    # leading dims are kept; dequantize_rows is codes * scale
    c2, s2 = decode.quantize_rows(x.view(1, -1, D))
    assert torch.equal(c2.view(torch.uint8)[0], codes.view(torch.uint8)) and torch.equal(s2[0], scale)
    assert torch.equal(decode.dequantize_rows(codes, scale), codes.float() * scale.unsqueeze(-1))


def test_cache_fields_nbytes_and_value_errors():
    from kubeflow_rm_amd import ops
    for D in (64, 128):
        bf = ops.KVCache(2, 3, 4, D, 40, device="cpu", dtype=torch.bfloat16)
        f8 = ops.KVCache(2, 3, 4, D, 40, device="cpu", dtype=FP8)
        assert bf.k_scale is None and bf.v_scale is None
        assert len(f8.k) == len(f8.k_scale) == len(f8.v_scale) == 2
        assert f8.k[0].dtype == FP8 and f8.k[0].shape == (3, 4, 40, D) and f8.k[0].stride(2) == D
        assert f8.k_scale[0].dtype == torch.float32 and f8.v_scale[1].shape == (3, 4, 40)
        rows = 2 * 2 * 3 * 4 * 40  # layers * (k, v) * B * H * capacity; no workspace on the CPU
        assert bf.nbytes == rows * D * 2
        assert f8.nbytes == rows * (D + 4)
        assert f8.nbytes / bf.nbytes == (D + 4) / (2 * D)
    assert round(68 / 128, 2) == 0.53 and round(132 / 256, 2) == 0.52
    # the bookkeeping is the cache's, whatever it stores
    c = ops.KVCache(1, 2, 2, 64, 10, device="cpu", dtype=FP8)
    c.set_lens([3, 7])
    c.k[0].view(torch.uint8).fill_(0x31)
    c.k_scale[0].fill_(2.0)
    c.rewind(2)
    assert c.lens.tolist() == [1, 5] and c.t_bound == 5
    assert (c.k[0].view(torch.uint8) == 0x31).all() and (c.k_scale[0] == 2.0).all()  # dead rows stay in place
    c.advance(4)
    assert c.lens.tolist() == [5, 9] and c.lens_after(1).tolist() == [6, 10] and c.bound_after(1) == 10
    c.pin_bound()
    assert c.t_bound == 10
    c.reset()
    assert c.lens.tolist() == [0, 0]
    with pytest.raises(ValueError):
        ops.KVCache(1, 2, 2, 64, 0, device="cpu", dtype=FP8)
    with pytest.raises(ValueError):
        c.set_lens([11, 0])
    with pytest.raises(ValueError):
        c.rewind(-1)
    with pytest.raises(ValueError):
        ops.kv_append(torch.zeros(2, 1, 3 * 2 * 32), c, 0)  # another head dim
    with pytest.raises(ValueError):
        ops.attention_decode(torch.zeros(2, 2, 32), c, 0)
    with pytest.raises(ValueError):
        ops.attention_extend(torch.zeros(2, 1, 2, 32), c, 0)


@pytest.mark.parametrize("D", [64, 128])
def test_cpu_append_quantises_by_the_formula_and_keeps_other_rows(D):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    B, H, cap, T = 2, 3, 12, 5
    g = torch.Generator().manual_seed(7)
    cache = ops.KVCache(1, B, H, D, cap, device="cpu", dtype=FP8)
    cache.k[0].view(torch.uint8).fill_(0x55)
    cache.v[0].view(torch.uint8).fill_(0x55)
    cache.k_scale[0].fill_(-7.0)
    cache.v_scale[0].fill_(-7.0)
    lens = [2, 9]  # row 1 crosses the capacity: 9 + 5 > 12
    cache.set_lens(lens)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16)
    qkv[0, 1].view(3, H, D)[1, 2] = 0  # an all-zero K row
    ops.kv_append(qkv, cache, 0)
    assert cache.lens.tolist() == lens  # not advanced
    x = qkv.view(B, T, 3, H, D)
    for s, codes, scales in ((1, cache.k[0], cache.k_scale[0]), (2, cache.v[0], cache.v_scale[0])):
        raw = codes.view(torch.uint8)
        for b, n in enumerate(lens):
            kept = min(T, cap - n)
            c, sc = decode.quantize_rows(x[b, :kept, s].transpose(0, 1))  # [H, kept, D]
            assert torch.equal(raw[b, :, n:n + kept], c.view(torch.uint8))
            assert torch.equal(scales[b, :, n:n + kept], sc)
            assert (raw[b, :, :n] == 0x55).all() and (scales[b, :, :n] == -7.0).all()
            assert (raw[b, :, n + kept:] == 0x55).all() and (scales[b, :, n + kept:] == -7.0).all()
    assert (cache.k[0].view(torch.uint8)[0, 2, 3] == 0).all() and cache.k_scale[0][0, 2, 3] == 1


def test_cpu_attention_reads_the_dequantised_visible_rows():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    B, H, D, cap, T = 3, 2, 64, 12, 4
    g = torch.Generator().manual_seed(3)
    cache = ops.KVCache(1, B, H, D, cap, device="cpu", dtype=FP8)
    lens = [4, 9, 2]
    qkv = torch.randn(B, 9, 3 * H * D, generator=g)
    ops.kv_append(qkv, cache, 0)
    cache.set_lens(lens)
    for b, n in enumerate(lens):  # dead rows: NaN codes and NaN scales
        cache.k[0].view(torch.uint8)[b, :, n:] = 0x7F
        cache.v[0].view(torch.uint8)[b, :, n:] = 0x7F
        cache.k_scale[0][b, :, n:] = float("nan")
        cache.v_scale[0][b, :, n:] = float("nan")
    kd = decode.dequantize_rows(cache.k[0], cache.k_scale[0])
    vd = decode.dequantize_rows(cache.v[0], cache.v_scale[0])
    q = torch.randn(B, T, H, D, generator=g)
    o, lse = ops.attention_extend(q, cache, 0, return_lse=True)
    assert torch.isfinite(o).all()
    for b, n in enumerate(lens):
        for i in range(T):
            nk = n - T + i + 1
            if nk <= 0:
                assert (o[b, i] == 0).all() and (lse[b, i] == float("-inf")).all()
                continue
            ref = F.scaled_dot_product_attention(q[b:b + 1, i].unsqueeze(2), kd[b:b + 1, :, :nk],
                                                 vd[b:b + 1, :, :nk]).squeeze(2)
            assert torch.allclose(o[b:b + 1, i], ref, atol=1e-5), (b, i)
            s = (q[b, i].unsqueeze(1) @ kd[b, :, :nk].transpose(-1, -2)).squeeze(1) / math.sqrt(D)
            assert torch.allclose(lse[b, i], torch.logsumexp(s, -1), atol=1e-5)
    od, lsed = ops.attention_decode(q[:, -1], cache, 0, return_lse=True)
    assert torch.isfinite(od).all()
    assert torch.allclose(od, o[:, -1], atol=1e-5) and torch.allclose(lsed, lse[:, -1], atol=1e-5)
    out = torch.zeros(B, H * D)
    ops.attention_decode(q[:, -1], cache, 0, out=out.view(B, H, D))
    assert torch.equal(out.view(B, H, D), od)


# ---- the model ------------------------------------------------------------------------------------

def _cfg(n_layers=2, max_seq=64):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=128, d_model=256, n_layers=n_layers, n_heads=4, d_ff=256, max_seq=max_seq,
                     dtype=torch.float32)  # head dim 64


def _perturbed(cfg, seed):
    from kubeflow_rm_amd.models import GPT
    m = GPT(cfg).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # the seeded init has zero biases and unit LayerNorm gains
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return m


@pytest.fixture(scope="module")
def model():
    return _perturbed(_cfg(), 11)


def _prompt(B, T, seed):
    return torch.randint(0, 128, (B, T), generator=torch.Generator().manual_seed(seed))


def test_new_cache_kv_dtype_and_prefill_logits(model):
    idx = _prompt(2, 12, seed=1)
    c32 = model.new_cache(2, 20)
    c8 = model.new_cache(2, 20, kv_dtype=FP8)
    assert c32.dtype == torch.float32 and c8.dtype == FP8 and c8.k_scale[0].shape == (2, 4, 20)
    assert model.new_cache(2, 20, kv_dtype=torch.bfloat16).dtype == torch.bfloat16
    # prefill's attention never reads the cache: same logits whatever the cache stores
    assert torch.equal(model.prefill(idx, c32), model.prefill(idx, c8))
    assert c8.lens.tolist() == [12, 12]
    with pytest.raises(ValueError):
        model.new_cache(2, 65, kv_dtype=FP8)


def test_generate_fp8_equals_hand_loop_and_quantisation_is_real(model):
    B, T0, new = 2, 9, 14
    idx = _prompt(B, T0, seed=2)
    out = model.generate(idx, new, kv_dtype=FP8)
    cache = model.new_cache(B, T0 + new, kv_dtype=FP8)
    logits = model.prefill(idx, cache)
    ref_cache = model.new_cache(B, T0 + new)
    model.prefill(idx, ref_cache)
    toks, e_q = [idx], 0.0
    for i in range(new):
        nxt = logits.argmax(-1)
        toks.append(nxt.view(B, 1))
        if i + 1 < new:
            logits = model.decode_step(nxt, cache)
            e_q = max(e_q, (logits - model.decode_step(nxt, ref_cache)).abs().max().item())
    assert torch.equal(out, torch.cat(toks, 1))
    assert cache.lens.tolist() == [T0 + new - 1] * B
    print(f"fp8 against fp32 cache, max-abs logit difference {e_q:.4f}")
    assert 0 < e_q < 0.5, e_q  # quantisation really happens, and stays a perturbation
    # sampling goes through the same cache
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    a = model.generate(idx, 6, temperature=0.8, top_k=20, generator=g1, kv_dtype=FP8)
    b = model.generate(idx, 6, temperature=0.8, top_k=20, generator=g2, kv_dtype=FP8)
    assert torch.equal(a, b) and a.shape == (B, T0 + 6)
    with pytest.raises(ValueError):
        model.generate(idx, 4, graph=True, kv_dtype=FP8)  # CPU tensors


def test_extend_and_rewind_on_an_fp8_cache_match_decode_steps(model):
    """extend(T) stores the same rows as T decode_steps, so its logits agree to fp32 rounding; after a
    rewind the dead codes and scales are overwritten."""
    B, total = 2, 40
    seq = _prompt(B, total, seed=4)
    a = model.new_cache(B, total, kv_dtype=FP8)
    b = model.new_cache(B, total, kv_dtype=FP8)
    model.prefill(seq[:, :7], a)
    model.prefill(seq[:, :7], b)
    at = 7
    for T in (1, 5, 16, 11):
        lg = model.extend(seq[:, at:at + T], a)
        steps = torch.stack([model.decode_step(seq[:, at + i], b) for i in range(T)], 1)
        assert lg.shape == steps.shape and (lg - steps).abs().max().item() < 1e-4
        at += T
    assert a.lens.tolist() == b.lens.tolist() == [total] * B
    for li in range(len(a.k)):
        same = (a.k[li].view(torch.uint8) == b.k[li].view(torch.uint8)).float().mean().item()
        assert same > 0.999, same
    a.rewind(6)
    again = model.extend(seq[:, total - 6:], a)
    assert (again - steps[:, -6:]).abs().max().item() < 1e-4
    with pytest.raises(ValueError):
        model.extend(seq[:, :1], a)  # full


def _greedy_margin_fp8(model, idx, new):
    """Top-2 logit gap of the greedy run on an fp8 cache, minimum over the steps."""
    cache = model.new_cache(idx.shape[0], idx.shape[1] + new, kv_dtype=FP8)
    logits, margin = model.prefill(idx, cache), float("inf")
    for i in range(new):
        top2 = logits.topk(2, -1).values
        margin = min(margin, (top2[:, 0] - top2[:, 1]).min().item())
        if i + 1 < new:
            logits = model.decode_step(logits.argmax(-1), cache)
    return margin


@pytest.mark.parametrize("new,lookahead", [(24, 4), (11, 3)])
def test_draft_generate_on_fp8_caches_equals_plain_greedy_on_fp8(model, new, lookahead):
    idx = _prompt(1, 7, seed=5)
    # extend and decode_step store the same codes (a flipped tie moves a logit by ~1e-3 at most)
    assert _greedy_margin_fp8(model, idx, new) > 1e-2
    plain = model.generate(idx, new, kv_dtype=FP8)
    out, stats = model.generate(idx, new, draft=model, lookahead=lookahead, return_stats=True, kv_dtype=FP8)
    assert torch.equal(out, plain)
    assert stats["target_steps"] == math.ceil(new / (lookahead + 1)), stats
    assert stats["accepted"] == stats["proposed"] == new - stats["target_steps"], stats
    small = _perturbed(_cfg(n_layers=1), 12)
    out, stats = model.generate(idx, new, draft=small, lookahead=lookahead, return_stats=True, kv_dtype=FP8)
    assert torch.equal(out, plain)
    assert 0 <= stats["accepted"] <= stats["proposed"]
