"""Grouped K / V heads on the flash-attention ops: the argument checks that run before any device work, and the
grouped CPU model, which the GPU kernels leave as it was (SDPA on K / V repeated over the group)."""
from __future__ import annotations

import inspect

import pytest
import torch
import torch.nn.functional as F


def test_kv_heads_keywords_exist():
    from kubeflow_rm_amd import ops
    for fn in (ops.attention_qkv, ops.attn_block):
        p = inspect.signature(fn).parameters
        assert "kv_heads" in p and p["kv_heads"].default is None, fn.__name__


@pytest.mark.parametrize("h,hkv", [(8, 3), (8, 0), (6, 4), (4, 8), (8, -2)])
def test_head_counts_that_do_not_divide_raise(h, hkv):
    """ValueError from the head-count check itself, before dtype / device / layout are looked at."""
    from kubeflow_rm_amd import ops
    B, T, hd = 1, 16, 64
    kv = max(hkv, 0)
    q = torch.zeros(B, h, T, hd)
    k = torch.zeros(B, kv, T, hd)
    with pytest.raises(ValueError, match="K / V heads"):
        ops.flash_attention(q, k, k)
    with pytest.raises(ValueError, match="K / V heads"):
        ops.attention_qkv(torch.zeros(B, T, (h + 2 * kv) * hd), h, hd, kv_heads=hkv)
    with pytest.raises(ValueError, match="K / V heads"):
        ops.attn_block(torch.zeros(B, T, 32), torch.zeros((h + 2 * kv) * hd, 32), None, torch.zeros(32, h * hd), None,
                       h, hd, kv_heads=hkv)


def test_flash_attention_shape_checks():
    from kubeflow_rm_amd import ops
    q = torch.zeros(1, 8, 16, 64)
    with pytest.raises(ValueError):  # k and v disagree
        ops.flash_attention(q, torch.zeros(1, 2, 16, 64), torch.zeros(1, 4, 16, 64))
    with pytest.raises(ValueError):  # another T
        ops.flash_attention(q, torch.zeros(1, 2, 8, 64), torch.zeros(1, 2, 8, 64))
    with pytest.raises(ValueError):  # not 4-d
        ops.flash_attention(q, torch.zeros(2, 16, 64), torch.zeros(2, 16, 64))
    with pytest.raises(ValueError):  # divisible heads, but no bf16 GPU views: still refused, never a fallback
        ops.flash_attention(q, torch.zeros(1, 2, 16, 64), torch.zeros(1, 2, 16, 64))


def test_qkv_width_checks():
    from kubeflow_rm_amd import ops
    B, T, h, hkv, hd = 1, 16, 8, 2, 64
    with pytest.raises(ValueError, match="kv_heads"):  # the ungrouped width with kv_heads
        ops.attention_qkv(torch.zeros(B, T, 3 * h * hd), h, hd, kv_heads=hkv)
    with pytest.raises(ValueError, match="kv_heads"):  # the grouped width without it
        ops.attention_qkv(torch.zeros(B, T, (h + 2 * hkv) * hd), h, hd)
    with pytest.raises(ValueError, match="head dim"):  # the right width on the CPU: no fallback
        ops.attention_qkv(torch.zeros(B, T, (h + 2 * hkv) * hd), h, hd, kv_heads=hkv)
    x, wp = torch.zeros(B, T, 32), torch.zeros(32, h * hd)
    with pytest.raises(ValueError, match="wqkv"):
        ops.attn_block(x, torch.zeros(3 * h * hd, 32), None, wp, None, h, hd, kv_heads=hkv)
    with pytest.raises(ValueError, match="wqkv"):
        ops.attn_block(x, torch.zeros((h + 2 * hkv) * hd, 32), None, wp, None, h, hd)
    with pytest.raises(ValueError, match="head dim"):
        ops.attn_block(x, torch.zeros((h + 2 * hkv) * hd, 32), None, wp, None, h, hd, kv_heads=hkv)
    # kv_heads == h is the ungrouped call: its width is 3 h hd
    with pytest.raises(ValueError, match="head dim"):
        ops.attention_qkv(torch.zeros(B, T, 3 * h * hd), h, hd, kv_heads=h)


def _cfg(**kw):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=128, d_model=128, n_layers=1, n_heads=8, d_ff=172, max_seq=32, dtype=torch.float32,
                     n_kv_heads=2, pos="rope", norm="rms", mlp="swiglu", **kw)


def test_grouped_cpu_model_is_unchanged():
    """The CPU attention of a grouped block: q | k | v split of the (h + 2 hkv) hd projection, rotary, K / V head
    j serving query heads j G .. j G + G - 1, SDPA — computed here from F.scaled_dot_product_attention. The
    state dict keeps its names and the (h + 2 hkv) hd QKV shape."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT
    torch.manual_seed(0)
    model = GPT(_cfg()).eval()
    sd = model.state_dict()
    h, hkv, hd = 8, 2, 16
    assert sd["blocks.0.qkv.weight"].shape == ((h + 2 * hkv) * hd, 128)
    assert "pos" not in sd and not [k for k in sd if "rope" in k]
    assert sorted(k for k in sd if k.startswith("blocks.0.")) == sorted(
        "blocks.0." + n for n in ("ln1.weight", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "ln2.weight",
                                  "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))
    blk = model.blocks[0]
    B, T = 2, 24
    x = torch.randn(B, T, 128)
    with torch.no_grad():
        got = blk.attention(x, residual=x, rope=model.rope_table)
        qkv = ops.rope_qkv(F.linear(x, blk.qkv.weight, blk.qkv.bias), model.rope_table, h, hkv)
        q = qkv[..., :h * hd].view(B, T, h, hd).transpose(1, 2)
        k = qkv[..., h * hd:(h + hkv) * hd].view(B, T, hkv, hd).transpose(1, 2)
        v = qkv[..., (h + hkv) * hd:].view(B, T, hkv, hd).transpose(1, 2)
        heads = [F.scaled_dot_product_attention(q[:, i:i + 1], k[:, i // 4:i // 4 + 1], v[:, i // 4:i // 4 + 1],
                                                is_causal=True) for i in range(h)]
        y = torch.cat(heads, 1).transpose(1, 2).reshape(B, T, h * hd)
        want = x + F.linear(y, blk.proj.weight, blk.proj.bias)
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), (got - want).abs().max().item()
    idx = torch.randint(0, 128, (B, T))
    with torch.no_grad():
        logits, _ = model(idx, idx)
        cache = model.new_cache(B, 32)
        last = model.prefill(idx, cache)
    assert torch.allclose(last, logits[:, -1], atol=1e-4, rtol=1e-4)
