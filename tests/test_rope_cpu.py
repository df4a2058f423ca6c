"""Rotary position embeddings on the torch path: the table, the rule against an independent complex form, the
relative-position property, the backward, and a rotary GPT (fp32 CPU) through prefill / decode_step / extend /
generate against its own full forward. Bounds: 1e-4 on cached-vs-full fp32 logits and 0 < E_q < 0.5 for an FP8
cache, as tests/test_generate_cpu.py and tests/test_kv_fp8_cpu.py hold the learned-position model to."""
import math

import pytest
import torch

FP8 = torch.float8_e4m3fn


def _angles(max_pos, D, theta=10000.0):
    """p * f_i in float64, written with python floats: independent of ops.rope_table's tensor code."""
    f = [theta ** (-2.0 * i / D) for i in range(D // 2)]
    return torch.tensor([[p * fi for fi in f] for p in range(max_pos)], dtype=torch.float64)


def _complex_rope(x, pos, theta=10000.0):
    """x [B, T, H, D] float64 rotated as D/2 complex numbers (x[i] + 1j x[i + D/2]) * exp(1j pos f_i); pos [B, T]."""
    D = x.shape[-1]
    ang = _angles(int(pos.max()) + 1, D, theta)[pos]  # [B, T, D/2]
    z = torch.complex(x[..., :D // 2], x[..., D // 2:]) * torch.polar(torch.ones_like(ang), ang).unsqueeze(2)
    return torch.cat([z.real, z.imag], -1)


@pytest.mark.parametrize("D,theta", [(64, 10000.0), (128, 10000.0), (16, 500000.0)])
def test_table_is_the_float64_values_rounded_once(D, theta):
    from kubeflow_rm_amd import ops
    t = ops.rope_table(300, D, theta)
    assert t.shape == (300, D) and t.dtype == torch.float32
    ang = _angles(300, D, theta)
    want = torch.cat([ang.cos(), ang.sin()], 1).to(torch.float32)
    assert torch.equal(t, want)
    assert torch.equal(t[0], torch.cat([torch.ones(D // 2), torch.zeros(D // 2)]))
    assert torch.equal(ops.rope_table(300, D, theta=theta), t) and torch.equal(ops.rope_table(10, D, theta), t[:10])
    with pytest.raises(ValueError):
        ops.rope_table(8, 7)


@pytest.mark.parametrize("Hq,Hkv", [(3, 3), (4, 2)])
def test_rule_matches_the_complex_form(Hq, Hkv):
    from kubeflow_rm_amd import ops
    B, T, D = 2, 5, 64
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, (Hq + 2 * Hkv) * D, generator=g)
    positions = torch.tensor([0, 37], dtype=torch.int32)
    y = ops.rope_qkv(x, ops.rope_table(64, D), Hq, Hkv, positions)
    assert y.dtype == torch.float32 and y.shape == x.shape and y.data_ptr() != x.data_ptr()
    nr = (Hq + Hkv) * D
    pos = positions.long().view(B, 1) + torch.arange(T)
    want = _complex_rope(x[..., :nr].double().view(B, T, Hq + Hkv, D), pos).view(B, T, nr)
    err = (y[..., :nr].double() - want).abs().max().item()
    print(f"rope rule against the complex form: max-abs {err:.3e}")
    assert err < 1e-6
    assert torch.equal(y[..., nr:], x[..., nr:])  # v
    # positions=None is position 0 for every row's first token
    assert torch.equal(ops.rope_qkv(x[:1], ops.rope_table(64, D), Hq, Hkv), y[:1])
    # a row at or beyond the table's end is left as it is
    short = ops.rope_qkv(x, ops.rope_table(40, D), Hq, Hkv, positions)
    assert torch.equal(short[1, 3:], x[1, 3:]) and torch.equal(short[1, :3], y[1, :3]) and torch.equal(short[0], y[0])


def test_scores_depend_on_the_relative_position_only():
    from kubeflow_rm_amd import ops
    D, H = 64, 2
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 1, 3 * H * D, generator=g)
    table = ops.rope_table(512, D)

    def score(m, n):
        q = ops.rope_qkv(x, table, H, H, torch.tensor([m], dtype=torch.int32))[0, 0, :H * D].view(H, D)
        k = ops.rope_qkv(x, table, H, H, torch.tensor([n], dtype=torch.int32))[0, 0, H * D:2 * H * D].view(H, D)
        return (q * k).sum(-1) / math.sqrt(D)

    base = score(7, 3)
    for shift in (1, 50, 400):
        assert (score(7 + shift, 3 + shift) - base).abs().max().item() < 1e-4
    assert (score(8, 3) - base).abs().max().item() > 1e-3  # and it does depend on the difference


def test_backward_is_the_inverse_rotation():
    from kubeflow_rm_amd import ops
    B, T, D, Hq, Hkv = 2, 5, 64, 4, 2
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, T, (Hq + 2 * Hkv) * D, generator=g, requires_grad=True)
    gy = torch.randn(B, T, (Hq + 2 * Hkv) * D, generator=g)
    positions = torch.tensor([0, 37], dtype=torch.int32)
    table = ops.rope_table(64, D)
    y = ops.rope_qkv(x, table, Hq, Hkv, positions)
    y.backward(gy)
    nr = (Hq + Hkv) * D
    assert torch.equal(x.grad[..., nr:], gy[..., nr:])  # the v gradient passes through
    pos = positions.long().view(B, 1) + torch.arange(T)
    ang = _angles(64, D)[pos]
    gq = gy[..., :nr].double().view(B, T, Hq + Hkv, D)
    z = torch.complex(gq[..., :D // 2], gq[..., D // 2:]) * torch.polar(torch.ones_like(ang), -ang).unsqueeze(2)
    want = torch.cat([z.real, z.imag], -1).view(B, T, nr)
    assert (x.grad[..., :nr].double() - want).abs().max().item() < 1e-6
    # rotating the gradient forward again gives it back: the backward is the inverse map
    again = ops.rope_qkv(x.grad.detach(), table, Hq, Hkv, positions)
    assert (again - gy).abs().max().item() < 1e-5


def _cfg(pos="rope", n_heads=4, **kw):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=128, d_model=64, n_layers=2, n_heads=n_heads, d_ff=128, max_seq=64, dtype=torch.float32,
                     pos=pos, **kw)


def _model(**kw):
    from kubeflow_rm_amd.models import GPT
    m = GPT(_cfg(**kw)).eval()
    g = torch.Generator().manual_seed(11)  # zero biases and unit gains otherwise: perturb so every term is exercised
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def test_parameters_and_state_dict():
    from kubeflow_rm_amd.models import GPT, GPTConfig
    from kubeflow_rm_amd.models.gpt import num_params
    rope, learned = GPT(_cfg()), GPT(_cfg(pos="learned"))
    c = learned.cfg
    assert GPTConfig().pos == "learned" and GPTConfig().rope_theta == 10000.0
    assert "pos" not in rope.state_dict() and "rope_table" not in rope.state_dict()
    assert "pos" not in dict(rope.named_parameters())
    assert rope.rope_table.shape == (c.max_seq, c.head_dim) and rope.rope_table.dtype == torch.float32
    assert [n for n, _ in rope.named_buffers()] == ["rope_table"]
    # the default model: the keys and the count it has always had
    per_block = (3 * c.d_model * c.d_model + 3 * c.d_model) + (c.d_model * c.d_model + c.d_model) \
        + 2 * c.d_model * c.d_ff + c.d_ff + c.d_model + 4 * c.d_model
    want = c.vocab_size * c.d_model + c.max_seq * c.d_model + c.n_layers * per_block + 2 * c.d_model
    assert num_params(learned) == want and num_params(rope) == want - c.max_seq * c.d_model
    keys = set(learned.state_dict())
    assert keys == set(rope.state_dict()) | {"pos"}
    names = {f"blocks.{i}.{m}.{p}" for i in range(2) for m in ("ln1", "qkv", "proj", "ln2", "fc1", "fc2")
             for p in ("weight", "bias")}
    assert keys == names | {"tok", "pos", "ln_f.weight", "ln_f.bias"}
    assert list(learned.named_buffers()) == []
    # the weights the two share are seeded alike
    assert torch.equal(rope.tok, learned.tok) and torch.equal(rope.blocks[1].fc2.weight, learned.blocks[1].fc2.weight)
    rope.load_state_dict({k: v for k, v in learned.state_dict().items() if k != "pos"})
    for bad in ("alibi", "", None):
        with pytest.raises(ValueError):
            _cfg(pos=bad)


def test_position_matters():
    """The rotary model is not position-blind: swapping two prompt tokens changes the last logits."""
    m = _model()
    a = torch.tensor([[5, 9, 17, 3, 44]])
    b = torch.tensor([[9, 5, 17, 3, 44]])
    with torch.no_grad():
        assert (m(a)[:, -1] - m(b)[:, -1]).abs().max().item() > 1e-3


@pytest.mark.parametrize("kw", [dict(), dict(n_heads=2), dict(n_kv_heads=2)], ids=["D16", "D32", "gqa"])
def test_cached_logits_equal_the_full_forward(kw):
    m = _model(**kw)
    B, T0, steps, T = 2, 9, 12, 7
    total = T0 + steps + T
    seq = torch.randint(0, 128, (B, total), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        full = m(seq)
    cache = m.new_cache(B, total)
    logits = m.prefill(seq[:, :T0], cache)
    assert (logits - full[:, T0 - 1]).abs().max().item() < 1e-4
    for i in range(steps):
        logits = m.decode_step(seq[:, T0 + i], cache)
        assert (logits - full[:, T0 + i]).abs().max().item() < 1e-4, i
    at = T0 + steps
    lg = m.extend(seq[:, at:], cache)
    assert lg.shape == (B, T, 128) and (lg - full[:, at:]).abs().max().item() < 1e-4
    assert cache.lens.tolist() == [total] * B
    cache.rewind(5)  # the dead rows are rotated again on the way in
    again = m.extend(seq[:, total - 5:], cache)
    assert (again - full[:, total - 5:]).abs().max().item() < 1e-4
    cache.rewind(total - 3)
    lg = m.extend(seq[:, 3:30], cache, chunk=20)  # the chunked path
    assert (lg - full[:, 3:30]).abs().max().item() < 1e-4
    with pytest.raises(ValueError):
        m.extend(seq, cache)  # does not fit


@pytest.mark.parametrize("kw", [dict(), dict(n_kv_heads=2)], ids=["mha", "gqa"])
def test_cached_logits_on_an_fp8_cache(kw):
    m = _model(**kw)
    B, T0, steps = 2, 9, 14
    seq = torch.randint(0, 128, (B, T0 + steps + 6), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        full = m(seq)
    c8 = m.new_cache(B, seq.shape[1], kv_dtype=FP8)
    # prefill attends the unquantised rows: the full forward's logits
    assert (m.prefill(seq[:, :T0], c8) - full[:, T0 - 1]).abs().max().item() < 1e-4
    e_q = 0.0
    for i in range(steps):
        e_q = max(e_q, (m.decode_step(seq[:, T0 + i], c8) - full[:, T0 + i]).abs().max().item())
    lg = m.extend(seq[:, T0 + steps:], c8)
    e_q = max(e_q, (lg - full[:, T0 + steps:]).abs().max().item())
    c8.rewind(4)
    e_q = max(e_q, (m.extend(seq[:, -4:], c8) - full[:, -4:]).abs().max().item())
    print(f"rotary model, fp8 cache against the full forward: max-abs {e_q:.4f}")
    assert 0 < e_q < 0.5, e_q
    # what is stored is quantize_rows of the rotated K: the codes of a bf16-free fp32 run dequantise to the fp32 cache
    c32 = m.new_cache(B, seq.shape[1])
    m.prefill(seq[:, :T0], c32)
    from kubeflow_rm_amd.ops.decode import quantize_rows
    codes, scale = quantize_rows(c32.k[0][:, :, :T0])
    assert torch.equal(codes.view(torch.uint8), c8.k[0][:, :, :T0].view(torch.uint8))
    assert torch.equal(scale, c8.k_scale[0][:, :, :T0])


def test_greedy_generate_equals_naive_full_forward_loop():
    m = _model()
    B, T0, new = 2, 7, 20
    idx = torch.randint(0, 128, (B, T0), generator=torch.Generator().manual_seed(5))
    naive, margin = idx, float("inf")
    with torch.no_grad():
        for _ in range(new):
            last = m(naive)[:, -1]
            top2 = last.topk(2, -1).values
            margin = min(margin, (top2[:, 0] - top2[:, 1]).min().item())
            naive = torch.cat([naive, last.argmax(-1, keepdim=True)], 1)
    assert margin > 1e-3, margin  # cached and full-forward logits agree to 1e-4: no tie decides
    assert torch.equal(m.generate(idx, new), naive)
    assert torch.equal(m.generate(idx, new, prefill_chunk=20), naive)


def test_kv_append_rope_on_the_torch_path():
    """rotate, then the existing append; rows past the capacity neither appended nor rotated; rope=None unchanged."""
    from kubeflow_rm_amd import ops
    B, H, D, cap, T = 2, 2, 16, 12, 4
    g = torch.Generator().manual_seed(3)
    table = ops.rope_table(cap, D)
    qkv = torch.randn(B, T, 3 * H * D, generator=g)
    plain, rot = ops.KVCache(1, B, H, D, cap, dtype=torch.float32), ops.KVCache(1, B, H, D, cap, dtype=torch.float32)
    for c in (plain, rot):
        c.set_lens([3, cap - 2])
        c.k[0].fill_(7.0)
    a = qkv.clone()
    ops.kv_append(a, plain, 0, rope=None)
    assert torch.equal(a, qkv) and torch.equal(plain.k[0][0, :, 3:7], qkv[0].view(T, 3, H, D)[:, 1].transpose(0, 1))
    b = qkv.clone()
    ops.kv_append(b, rot, 0, rope=table)
    want = ops.rope_qkv(qkv, table, H, H, rot.lens)
    assert torch.equal(b[0], want[0]) and torch.equal(b[1, :2], want[1, :2])
    assert torch.equal(b[1, 2:], qkv[1, 2:])  # past the capacity: not rotated
    assert torch.equal(rot.k[0][0, :, 3:7], want[0].view(T, 3, H, D)[:, 1].transpose(0, 1))
    assert torch.equal(rot.k[0][1, :, cap - 2:], want[1, :2].view(2, 3, H, D)[:, 1].transpose(0, 1))
    assert torch.equal(rot.v[0], plain.v[0]) and (rot.k[0][0, :, 7:] == 7.0).all() and (rot.k[0][0, :, :3] == 7.0).all()
    with pytest.raises(ValueError):
        ops.kv_append(qkv.clone(), rot, 0, rope=table[:cap - 1])
