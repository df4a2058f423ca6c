"""Grouped-query attention on the CPU / torch path: GPTConfig.n_kv_heads, the cache paths of a GQA model against
its own full forward, ops.attention_decode / extend / chunk and kv_append(q_heads=) against a cache expanded by
hand, and the refusals. The bounds of the cache-path tests are tests/test_extend_cpu.py's (1e-4 on fp32 logits)."""
from __future__ import annotations

import pytest
import torch

FP8 = torch.float8_e4m3fn


def _cfg(n_kv_heads=None, n_heads=4):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=128, d_model=64, n_layers=2, n_heads=n_heads, d_ff=128, max_seq=64, dtype=torch.float32,
                     n_kv_heads=n_kv_heads)


def _prompt(B, T, seed):
    return torch.randint(0, 128, (B, T), generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module", params=[2, 1], ids=["kv2", "kv1"])
def gqa(request):
    from kubeflow_rm_amd.models import GPT
    return GPT(_cfg(request.param)).eval()


def test_default_config_is_unchanged():
    from kubeflow_rm_amd.models import GPT, CONFIGS
    assert all(c.n_kv_heads is None and c.kv_heads == c.n_heads for c in CONFIGS.values())
    a, b = GPT(_cfg(None)), GPT(_cfg(4))
    assert a.blocks[0].qkv.weight.shape == (3 * 64, 64)
    for (n, p), (_, p2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(p, p2), n
    assert GPT(_cfg(2)).blocks[0].qkv.weight.shape == ((4 + 2 * 2) * 16, 64)
    assert GPT(_cfg(2)).flops_per_token(32) < a.flops_per_token(32)


def test_gqa_model_equals_the_mha_model_with_repeated_kv_rows(gqa):
    """An MHA model whose QKV weight / bias repeat every K and V head's rows G times computes the same function."""
    from kubeflow_rm_amd.models import GPT
    h, hkv, hd = 4, gqa.cfg.kv_heads, 16
    G = h // hkv
    mha = GPT(_cfg(None)).eval()
    sd = {k: v.clone() for k, v in gqa.state_dict().items()}
    for name, t in list(sd.items()):
        if ".qkv." in name:
            q, kv = t[:h * hd], t[h * hd:].view(2, hkv, hd, *t.shape[1:])
            kv = kv.repeat_interleave(G, dim=1).reshape(2 * h * hd, *t.shape[1:])
            sd[name] = torch.cat([q, kv], 0)
    mha.load_state_dict(sd)
    idx = _prompt(2, 24, seed=0)
    with torch.no_grad():
        assert (gqa(idx) - mha(idx)).abs().max().item() < 1e-5


def test_cache_paths_reproduce_the_full_forward(gqa):
    from kubeflow_rm_amd.models import GPT
    B, hkv = 2, gqa.cfg.kv_heads
    seq = _prompt(B, 48, seed=1)
    with torch.no_grad():
        full = gqa(seq)
    cache = gqa.new_cache(B, 48)
    assert cache.k[0].shape[1] == hkv and cache.H == hkv
    mha_cache = GPT(_cfg(None)).new_cache(B, 48)
    kv_bytes = lambda c: sum(t.numel() * t.element_size() for t in (*c.k, *c.v))  # noqa: E731
    assert kv_bytes(cache) * (4 // hkv) == kv_bytes(mha_cache)
    assert cache.nbytes * (4 // hkv) == mha_cache.nbytes  # no workspaces on the CPU: K / V is all of it
    got = [gqa.prefill(seq[:, :10], cache).unsqueeze(1), gqa.decode_step(seq[:, 10], cache).unsqueeze(1)]
    at = 11
    for T in (1, 3, 7):
        got.append(gqa.extend(seq[:, at:at + T], cache))
        at += T
    got.append(gqa.extend(seq[:, at:48], cache, chunk=17))
    assert (torch.cat(got, 1) - full[:, 9:]).abs().max().item() < 1e-4
    assert cache.lens.tolist() == [48, 48]
    out = gqa.generate(seq[:, :6], 5)
    with torch.no_grad():
        assert torch.equal(out[:, 6:], torch.stack([gqa(out[:, :6 + i])[:, -1].argmax(-1) for i in range(5)], 1))
    c8 = gqa.new_cache(B, 48, kv_dtype=FP8)
    assert c8.k_scale[0].shape == (B, hkv, 48)
    lg = gqa.extend(seq[:, :20], c8)
    assert (lg - full[:, :20]).abs().max().item() < 0.1  # a quantised cache: close, not equal


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("G", [2, 3, 4])
def test_ops_equal_the_same_calls_on_a_hand_expanded_cache(G, kind):
    from kubeflow_rm_amd import ops
    B, Hkv, D, cap, T = 2, 2, 16, 24, 5
    Hq = G * Hkv
    g = torch.Generator().manual_seed(10 * G)
    dt = FP8 if kind == "fp8" else torch.bfloat16
    small, big = ops.KVCache(1, B, Hkv, D, cap, dtype=dt), ops.KVCache(1, B, Hq, D, cap, dtype=dt)
    pre = torch.randn(B, 12, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    sentinel = [t.clone() for t in (small.k[0].view(torch.uint8), small.v[0].view(torch.uint8))]
    small.set_lens([3, 0])
    ops.kv_append(pre, small, 0, q_heads=Hq)
    # exactly the Hkv heads' rows lens[b] .. lens[b] + 11 were written, with the activation's k / v slices
    kx = pre[..., Hq * D:].view(B, 12, 2, Hkv, D)
    for b, n in enumerate((3, 0)):
        for s, t in ((0, small.k[0]), (1, small.v[0])):
            want = kx[b, :, s].transpose(0, 1)
            if kind == "fp8":
                codes, scale = ops.decode.quantize_rows(want)
                assert torch.equal(t[b, :, n:n + 12].view(torch.uint8), codes.view(torch.uint8))
                assert torch.equal((small.k_scale if s == 0 else small.v_scale)[0][b, :, n:n + 12], scale)
            else:
                assert torch.equal(t[b, :, n:n + 12], want)
            assert torch.equal(t.view(torch.uint8)[b, :, n + 12:], sentinel[s][b, :, n + 12:])
            assert torch.equal(t.view(torch.uint8)[b, :, :n], sentinel[s][b, :, :n])
    small.set_lens([15, 12])
    big.set_lens([15, 12])
    for src, dst in ((small.k, big.k), (small.v, big.v), (small.k_scale, big.k_scale), (small.v_scale, big.v_scale)):
        if src is not None:
            dst[0].view(torch.uint8 if src[0].dtype == FP8 else src[0].dtype).copy_(
                src[0].view(torch.uint8 if src[0].dtype == FP8 else src[0].dtype).repeat_interleave(G, dim=1))
    q = torch.randn(B, T, Hq, D, generator=g).bfloat16()
    for fn in (ops.attention_extend, ops.attention_chunk):
        o, lse = fn(q, small, 0, return_lse=True)
        o2, lse2 = fn(q, big, 0, return_lse=True)
        assert o.shape == (B, T, Hq, D) and torch.equal(o, o2) and torch.equal(lse, lse2)
    o, lse = ops.attention_decode(q[:, 0], small, 0, return_lse=True)
    o2, lse2 = ops.attention_decode(q[:, 0], big, 0, return_lse=True)
    assert o.shape == (B, Hq, D) and torch.equal(o, o2) and torch.equal(lse, lse2)


def test_refusals(monkeypatch):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT
    from kubeflow_rm_amd.parallel import tp as tpl
    with pytest.raises(ValueError):
        _cfg(3)
    with pytest.raises(ValueError):
        _cfg(0)
    cache = ops.KVCache(1, 1, 2, 16, 8)
    cache.set_lens([4])
    with pytest.raises(ValueError):
        ops.attention_decode(torch.zeros(1, 3, 16), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_extend(torch.zeros(1, 2, 5, 16), cache, 0)
    with pytest.raises(ValueError):
        ops.attention_chunk(torch.zeros(1, 2, 1, 16), cache, 0)
    with pytest.raises(ValueError):
        ops.kv_append(torch.zeros(1, 1, 3 * 2 * 16), cache, 0, q_heads=4)  # the width of q_heads = 2
    with pytest.raises(ValueError):
        ops.kv_append(torch.zeros(1, 1, (4 + 4) * 16), cache, 0)  # the width of q_heads = 4
    with pytest.raises(ValueError):
        ops.kv_append(torch.zeros(1, 1, (3 + 4) * 16), cache, 0, q_heads=3)
    monkeypatch.setattr(tpl, "_world", lambda group: 2)  # a two-rank group, as far as Block.__init__ looks
    with pytest.raises(NotImplementedError):
        GPT(_cfg(2))
