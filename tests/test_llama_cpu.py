"""Llama-style blocks on the CPU: GPTConfig(norm="rms", mlp="swiglu") against an independent torch Llama block
written here from two separate gate / up matrices, the SwiGLU rule of ops/swiglu.py, the KV-cache paths against the
full forward, and the default config's parameters, which must be exactly what they were."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from kubeflow_rm_amd import ops
from kubeflow_rm_amd.models import GPT, GPTConfig


def _cfg(**kw):
    base = dict(vocab_size=128, d_model=64, n_layers=2, n_heads=4, d_ff=88, max_seq=64, dtype=torch.float32,
                norm="rms", mlp="swiglu", pos="rope")
    base.update(kw)
    return GPTConfig(**base)


def _randomise(model, seed=0):
    """Non-trivial norm weights and biases (the constructor gives ones / zeros, which would hide a misplaced one)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif ".ln" in name or name.startswith("ln_f"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
    return model


def test_config_validation():
    for kw in ({"norm": "batch"}, {"mlp": "geglu"}, {"mlp": "silu"}, {"norm_eps": 0.0}, {"norm_eps": -1e-5}):
        with pytest.raises(ValueError):
            GPTConfig(**kw)
    c = GPTConfig()
    assert (c.norm, c.mlp, c.norm_eps, c.eps) == ("layer", "gelu", None, 1e-5)
    assert GPTConfig(norm="rms").eps == 1e-6 and GPTConfig(norm="rms", norm_eps=1e-5).eps == 1e-5


def test_swiglu_interleave_round_trip():
    g = torch.Generator().manual_seed(1)
    gate, up = torch.randn(5, 7, generator=g), torch.randn(5, 7, generator=g)
    w = ops.swiglu_interleave(gate, up)
    assert w.shape == (10, 7) and torch.equal(w[0::2], gate) and torch.equal(w[1::2], up)
    g2, u2 = ops.swiglu_deinterleave(w)
    assert torch.equal(g2, gate) and torch.equal(u2, up)
    b = ops.swiglu_interleave(gate[:, 0], up[:, 0])  # a bias [F]
    assert b.shape == (10,) and torch.equal(b[0::2], gate[:, 0]) and torch.equal(b[1::2], up[:, 0])
    with pytest.raises(ValueError):
        ops.swiglu_interleave(gate, up[:4])
    with pytest.raises(ValueError):
        ops.swiglu_deinterleave(w[:9])


def test_cpu_rule_against_separate_gate_and_up_matrices():
    g = torch.Generator().manual_seed(2)
    M, K, Fd = 5, 32, 11
    x = torch.randn(M, K, generator=g)
    wg, wu = torch.randn(Fd, K, generator=g), torch.randn(Fd, K, generator=g)
    bg, bu = torch.randn(Fd, generator=g), torch.randn(Fd, generator=g)
    w, b = ops.swiglu_interleave(wg, wu), ops.swiglu_interleave(bg, bu)
    want = F.silu(0.37 * (x @ wg.T) + bg) * (0.37 * (x @ wu.T) + bu)
    got = ops.gemm_nt(x, w, bias=b, alpha=0.37, act="swiglu", variant="skinny")
    assert got.shape == (M, Fd)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ops.swiglu(0.37 * (x @ w.T) + b), want, rtol=1e-5, atol=1e-5)
    # a QuantizedWeight enters as its dequantised value; the pair keeps its two row scales
    qw = ops.quantize_weight(w)
    dg, du = ops.swiglu_deinterleave(qw.dequantize())
    torch.testing.assert_close(ops.gemm_nt(x, qw, bias=b, act="swiglu", variant="skinny_mfma"),
                               F.silu(x @ dg.T + bg) * (x @ du.T + bu), rtol=1e-5, atol=1e-5)
    # through autograd
    zf = torch.randn(3, 2 * Fd, generator=g, requires_grad=True)
    ops.swiglu(zf).sum().backward()
    gg, uu = zf.detach()[:, 0::2], zf.detach()[:, 1::2]
    s = torch.sigmoid(gg)
    torch.testing.assert_close(zf.grad[:, 0::2], uu * s * (1 + gg * (1 - s)), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(zf.grad[:, 1::2], gg * s, rtol=1e-5, atol=1e-6)
    # the argument checks hold on the CPU too
    for bad in (dict(variant="auto"), dict(variant="w4"), dict(residual=torch.zeros(M, Fd))):
        kw = dict(act="swiglu", variant="skinny")
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.gemm_nt(x, w, **kw)
    with pytest.raises(ValueError):
        ops.gemm_nt(x, w[:-1], act="swiglu", variant="skinny")
    with pytest.raises(ValueError):
        ops.gemm_nt(x, w, act="swiglu", variant="skinny", out=torch.empty(M, 2 * Fd))
    with pytest.raises(ValueError):  # more rows than the weight-streaming kernel takes
        ops.gemm_nt(torch.randn(17, K), w, act="swiglu", variant="skinny")
    with pytest.raises(ValueError):  # K off the 8-bit kernel's 16-grid
        ops.gemm_nt(x[:, :24], ops.quantize_weight(w[:, :24].contiguous()), act="swiglu", variant="skinny")


def _llama_reference(model, idx):
    """An independent Llama forward from the model's parameters, fc1 split into its gate and up matrices."""
    c = model.cfg
    h, hkv, hd = c.n_heads, c.kv_heads, c.head_dim
    B, T = idx.shape

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c.eps) * w

    half = hd // 2
    inv = c.rope_theta ** (-torch.arange(half, dtype=torch.float64) * 2 / hd)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
    cos, sin = ang.cos().float()[None, :, None], ang.sin().float()[None, :, None]  # [1, T, 1, half]

    def rot(t):  # [B, T, heads, hd], rotate-half
        a, b = t[..., :half], t[..., half:]
        return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)

    x = F.embedding(idx, model.tok)
    for blk in model.blocks:
        y = rms(x, blk.ln1.weight)
        qkv = y @ blk.qkv.weight.T + blk.qkv.bias
        q = rot(qkv[..., :h * hd].view(B, T, h, hd))
        k = rot(qkv[..., h * hd:(h + hkv) * hd].view(B, T, hkv, hd))
        v = qkv[..., (h + hkv) * hd:].view(B, T, hkv, hd)
        k, v = (t.repeat_interleave(h // hkv, dim=2) for t in (k, v))
        att = torch.einsum("bthd,bshd->bhts", q, k) / hd ** 0.5
        att = att.masked_fill(torch.ones(T, T).triu(1).bool(), float("-inf")).softmax(-1)
        a = torch.einsum("bhts,bshd->bthd", att, v).reshape(B, T, h * hd)
        x = x + a @ blk.proj.weight.T + blk.proj.bias
        y = rms(x, blk.ln2.weight)
        wg, wu = blk.fc1.weight[0::2], blk.fc1.weight[1::2]
        bg, bu = blk.fc1.bias[0::2], blk.fc1.bias[1::2]
        x = x + (F.silu(y @ wg.T + bg) * (y @ wu.T + bu)) @ blk.fc2.weight.T + blk.fc2.bias
    return rms(x, model.ln_f.weight) @ model.tok.T


@pytest.mark.parametrize("n_kv", [None, 2])
def test_model_forward_matches_an_independent_llama_block(n_kv):
    model = _randomise(GPT(_cfg(n_kv_heads=n_kv))).eval()
    assert model.blocks[0].fc1.weight.shape == (176, 64) and model.blocks[0].fc1.act == "none"
    idx = torch.randint(0, 128, (2, 19), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        got, want = model(idx), _llama_reference(model, idx)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    keys = list(model.state_dict())
    assert "pos" not in keys and not [k for k in keys if ".ln" in k and k.endswith("bias")]
    assert "ln_f.weight" in keys and "ln_f.bias" not in keys


@pytest.mark.parametrize("n_kv", [None, 2])
def test_cache_paths_equal_the_full_forward(n_kv):
    model = _randomise(GPT(_cfg(n_kv_heads=n_kv))).eval()
    B, T0 = 2, 9
    seq = torch.randint(0, 128, (B, T0 + 3 + 5 + 20), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = model(seq)
        cache = model.new_cache(B, seq.shape[1])
        got, at = [model.prefill(seq[:, :T0], cache).view(B, 1, -1)], T0
        for _ in range(3):
            got.append(model.decode_step(seq[:, at], cache).view(B, 1, -1))
            at += 1
        got.append(model.extend(seq[:, at:at + 5], cache))
        got.append(model.extend(seq[:, at + 5:], cache, chunk=17))
    torch.testing.assert_close(torch.cat(got, 1), want[:, T0 - 1:], rtol=1e-4, atol=1e-4)
    # the 8-bit decode weights: fc1 is quantised row by row in its interleaved order
    # (fc2 has K = d_ff = 88, off the 8-bit kernel's 16-grid: it stays bf16, and the call says so)
    with pytest.warns(UserWarning, match="keep bf16 weights"):
        W = model.decode_weights()
    assert W.unquantized == ["blocks.0.fc2", "blocks.1.fc2"]
    q = W.blocks[0]["fc1"]
    assert q.codes.shape == (176, 64) and q.scale.shape == (176,)
    ref = ops.quantize_weight(model.blocks[0].fc1.weight.detach())
    assert torch.equal(q.codes.view(torch.uint8), ref.codes.view(torch.uint8)) and torch.equal(q.scale, ref.scale)
    with torch.no_grad():
        c8 = model.new_cache(B, 16)
        out = model.decode_step(seq[:, 0], c8, weights=W)
    assert out.shape == (B, 128) and torch.isfinite(out).all()


def test_flops_per_token():
    for mlp, k in (("gelu", 2), ("swiglu", 3)):
        c = _cfg(mlp=mlp, n_kv_heads=2)
        kv = 2 * 2 * c.head_dim
        dense = 2 * ((2 * 64 + kv) * 64 + k * 64 * 88) * 2 + 2 * 64 * 128
        assert GPT(c).flops_per_token(32) == 3.0 * (dense + 2 * 2 * 32 * 64 * 2)


def test_default_config_parameters_are_exactly_as_before():
    cfg = GPTConfig(vocab_size=128, d_model=64, n_layers=1, n_heads=4, d_ff=96, max_seq=32, dtype=torch.float32)
    model = GPT(cfg)
    want = [("tok", (128, 64)), ("pos", (32, 64)),
            ("blocks.0.ln1.weight", (64,)), ("blocks.0.ln1.bias", (64,)),
            ("blocks.0.qkv.weight", (192, 64)), ("blocks.0.qkv.bias", (192,)),
            ("blocks.0.proj.weight", (64, 64)), ("blocks.0.proj.bias", (64,)),
            ("blocks.0.ln2.weight", (64,)), ("blocks.0.ln2.bias", (64,)),
            ("blocks.0.fc1.weight", (96, 64)), ("blocks.0.fc1.bias", (96,)),
            ("blocks.0.fc2.weight", (64, 96)), ("blocks.0.fc2.bias", (64,)),
            ("ln_f.weight", (64,)), ("ln_f.bias", (64,))]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    assert model.blocks[0].fc1.act == "gelu_tanh" and not model.blocks[0].swiglu
    # and the default forward is LayerNorm + GELU
    idx = torch.randint(0, 128, (1, 8), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        x = F.embedding(idx, model.tok) + model.pos[:8]
        blk = model.blocks[0]
        y = F.layer_norm(x, (64,), blk.ln1.weight, blk.ln1.bias, 1e-5)
        q, k, v = (t.view(1, 8, 4, 16).transpose(1, 2) for t in (y @ blk.qkv.weight.T + blk.qkv.bias).chunk(3, -1))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(1, 8, 64)
        x = x + a @ blk.proj.weight.T + blk.proj.bias
        y = F.layer_norm(x, (64,), blk.ln2.weight, blk.ln2.bias, 1e-5)
        x = x + F.gelu(y @ blk.fc1.weight.T + blk.fc1.bias, approximate="tanh") @ blk.fc2.weight.T + blk.fc2.bias
        want_logits = F.layer_norm(x, (64,), model.ln_f.weight, model.ln_f.bias, 1e-5) @ model.tok.T
        torch.testing.assert_close(model(idx), want_logits, rtol=1e-4, atol=1e-4)
