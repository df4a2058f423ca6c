"""Chunked prefill on the torch path (CPU tensors): ops.attention_chunk against attention_extend and a per-row
fp32 SDPA loop on bf16-valued and FP8 caches, GPT.extend(chunk=) against the default path,
generate(prefill_chunk=) against plain generate, and the argument errors."""
import pytest
import torch
import torch.nn.functional as F


def _cache(kind, B, H, D, cap, seed):
    """A cache filled through kv_append (so an FP8 one holds real codes and scales), then NaN beyond nothing:
    the callers set lens and poison what lies beyond them."""
    from kubeflow_rm_amd import ops
    g = torch.Generator().manual_seed(seed)
    dtype = torch.float8_e4m3fn if kind == "fp8" else torch.bfloat16
    cache = ops.KVCache(1, B, H, D, cap, device="cpu", dtype=dtype)
    ops.kv_append(torch.randn(B, cap, 3 * H * D, generator=g), cache, 0)
    return cache, g


def _poison(cache, lens):
    for b, n in enumerate(lens):
        if cache.fp8:
            cache.k[0].view(torch.uint8)[b, :, n:] = 0x7F
            cache.v[0].view(torch.uint8)[b, :, n:] = 0x7F
            cache.k_scale[0][b, :, n:] = float("nan")
            cache.v_scale[0][b, :, n:] = float("nan")
        else:
            cache.k[0][b, :, n:] = float("nan")
            cache.v[0][b, :, n:] = float("nan")
    cache.set_lens(lens)


def _kv(cache):
    from kubeflow_rm_amd.ops import decode
    if cache.fp8:
        return (decode.dequantize_rows(cache.k[0], cache.k_scale[0]),
                decode.dequantize_rows(cache.v[0], cache.v_scale[0]))
    return cache.k[0], cache.v[0]


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_chunk_equals_extend_up_to_16_rows(kind):
    from kubeflow_rm_amd import ops
    B, H, D, cap = 2, 2, 16, 40
    cache, g = _cache(kind, B, H, D, cap, seed=1)
    _poison(cache, [23, 9])
    for T in (1, 5, 16):
        q = torch.randn(B, T, H, D, generator=g)
        o, lse = ops.attention_chunk(q, cache, 0, return_lse=True)
        o2, lse2 = ops.attention_extend(q, cache, 0, return_lse=True)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)
        out = torch.zeros(B, T, H * D)
        assert torch.equal(ops.attention_chunk(q, cache, 0, out=out.view(B, T, H, D)), o)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("T", [17, 40])
def test_chunk_matches_per_row_sdpa(kind, T):
    from kubeflow_rm_amd import ops
    B, H, D, cap = 3, 2, 16, 64
    cache, g = _cache(kind, B, H, D, cap, seed=2 + T)
    lens = [T, 61, T - 6]  # the block is the whole sequence; has a prefix; starts before the sequence
    _poison(cache, lens)
    k, v = _kv(cache)
    q = torch.randn(B, T, H, D, generator=g)
    o, lse = ops.attention_chunk(q, cache, 0, return_lse=True)
    assert o.shape == (B, T, H, D) and lse.shape == (B, T, H)
    for b, n in enumerate(lens):
        for i in range(T):
            nk = n - T + i + 1
            if nk <= 0:
                assert (o[b, i] == 0).all() and (lse[b, i] == float("-inf")).all()
                continue
            kk, vv = k[b:b + 1, :, :nk].float(), v[b:b + 1, :, :nk].float()
            ref = F.scaled_dot_product_attention(q[b:b + 1, i].unsqueeze(2), kk, vv).squeeze(2)
            assert torch.allclose(o[b:b + 1, i], ref, atol=1e-5), (b, i)
            s = (q[b, i].unsqueeze(1) @ kk[0].transpose(-1, -2)).squeeze(1) / D ** 0.5
            assert torch.allclose(lse[b, i], torch.logsumexp(s, -1), atol=1e-5)


def _model(max_seq=128):
    from kubeflow_rm_amd.models import GPT, GPTConfig
    cfg = GPTConfig(vocab_size=128, d_model=64, n_layers=2, n_heads=4, d_ff=128, max_seq=max_seq, dtype=torch.float32)
    m = GPT(cfg).eval()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # the seeded init has zero biases and unit LayerNorm gains
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return m


@pytest.fixture(scope="module")
def model():
    return _model()


def test_extend_chunk_equals_extend(model):
    B, T0, T = 2, 9, 75
    seq = torch.randint(0, 128, (B, T0 + T), generator=torch.Generator().manual_seed(1))
    a, b = model.new_cache(B, T0 + T), model.new_cache(B, T0 + T)
    model.prefill(seq[:, :T0], a)
    model.prefill(seq[:, :T0], b)
    want = model.extend(seq[:, T0:], a)
    got = model.extend(seq[:, T0:], b, chunk=32)  # 32 + 32 + 11
    assert got.shape == (B, T, 128) and (got - want).abs().max().item() < 1e-5
    assert b.lens.tolist() == [T0 + T] * B and b.t_bound == T0 + T
    # from an empty cache, the last position only, on an FP8 cache too
    for kv in (None, torch.float8_e4m3fn):
        a, b = model.new_cache(B, 80, kv_dtype=kv), model.new_cache(B, 80, kv_dtype=kv)
        want = model.extend(seq[:, :70], a, last_only=True)
        got = model.extend(seq[:, :70], b, last_only=True, chunk=32)
        assert got.shape == (B, 128) and (got - want).abs().max().item() < 1e-5


def test_generate_prefill_chunk_equals_generate(model):
    idx = torch.randint(0, 128, (2, 45), generator=torch.Generator().manual_seed(5))
    plain = model.generate(idx, 12)
    # cached logits of the two paths agree to 1e-5: the comparison cannot turn on a tie
    cur, margin = idx, float("inf")
    with torch.no_grad():
        for _ in range(12):
            top2 = model(cur)[:, -1].topk(2, -1).values
            margin = min(margin, (top2[:, 0] - top2[:, 1]).min().item())
            cur = torch.cat([cur, model(cur)[:, -1].argmax(-1, keepdim=True)], 1)
    assert margin > 1e-3
    got = model.generate(idx, 12, prefill_chunk=32)
    assert got.shape == (2, 57) and torch.equal(got, plain)
    assert torch.equal(model.generate(idx, 12, prefill_chunk=32, sampler="fused"), plain)


def test_argument_errors(model):
    from kubeflow_rm_amd import ops
    cache, g = _cache("bf16", 2, 2, 16, 40, seed=3)
    cache.set_lens([20, 20])
    with pytest.raises(ValueError):
        ops.attention_chunk(torch.randn(2, 0, 2, 16), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_chunk(torch.randn(2, 20, 1, 16), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_chunk(torch.randn(1, 20, 2, 16), cache, 0)
    idx = torch.randint(0, 128, (1, 40), generator=torch.Generator().manual_seed(6))
    for bad in (16, 0, -32, 65, 32.0, True):  # not above 16; above the capacity; not an int
        with pytest.raises(ValueError):
            model.extend(idx, model.new_cache(1, 64), chunk=bad)
    with pytest.raises(ValueError):
        model.generate(idx, 8, prefill_chunk=16)
    with pytest.raises(ValueError):
        model.generate(idx, 8, prefill_chunk=49)  # the cache holds 48 rows
    with pytest.raises(ValueError):
        model.generate(idx, 8, prefill_chunk=32, draft=model)
    assert model.generate(idx, 8, prefill_chunk=48).shape == (1, 48)
