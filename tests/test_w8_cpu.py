"""FP8 decode weights on the torch path (fp32 CPU model): the QuantizedWeight format, GPT.decode_weights,
the <= 16-row routing rule of decode_step / extend, and generate(weight_dtype=...)."""
import copy

import pytest
import torch
import torch.nn.functional as F

FP8 = torch.float8_e4m3fn


def _cfg(n_layers=2, max_seq=64):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=128, d_model=64, n_layers=n_layers, n_heads=4, d_ff=128, max_seq=max_seq,
                     dtype=torch.float32)


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


# ---- format ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_weight_is_quantize_rows(dtype):
    from kubeflow_rm_amd import ops
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(24, 48, generator=g) * torch.logspace(-3, 2, 24).unsqueeze(1)).to(dtype)
    w[5] = 0
    w[7, 3] = w[7].float().abs().max() * 2          # +amax
    w[9, 11] = -w[9].float().abs().max() * 2        # -amax
    qw = ops.quantize_weight(w)
    codes, scale = ops.decode.quantize_rows(w)
    assert isinstance(qw, ops.QuantizedWeight)
    assert qw.codes.dtype == FP8 and qw.scale.dtype == torch.float32
    assert torch.equal(qw.codes.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(qw.scale, scale)
    assert qw.shape == (24, 48) and qw.device == w.device
    assert qw.nbytes == 24 * 48 + 4 * 24
    # a zero row: scale 1, zero codes
    assert qw.scale[5].item() == 1.0 and (qw.codes[5].float() == 0).all()
    # a row's +-amax is stored as +-448
    assert qw.codes[7, 3].float().item() == 448.0 and qw.codes[9, 11].float().item() == -448.0
    # RNE to 3 mantissa bits (2^-4 relative), subnormal spacing 2^-9 code units (half: 2^-10), fp32 division slack
    wf = w.float()
    err = (qw.dequantize() - wf).abs()
    bound = torch.maximum(wf.abs() * 2.0 ** -4, qw.scale.unsqueeze(1) * 2.0 ** -10) * (1 + 1e-6)
    assert qw.dequantize().dtype == torch.float32
    assert (err <= bound).all(), (err - bound).max().item()
    assert torch.equal(qw.dequantize(), ops.decode.dequantize_rows(codes, scale))


def test_quantized_weight_constructor_checks():
    from kubeflow_rm_amd import ops
    codes = torch.zeros(4, 16, dtype=torch.uint8).view(FP8)
    qw = ops.QuantizedWeight(codes, torch.ones(4))
    assert qw.nbytes == 4 * 16 + 16 and (qw.dequantize() == 0).all()
    with pytest.raises(ValueError):
        ops.QuantizedWeight(torch.zeros(4, 16), torch.ones(4))
    with pytest.raises(ValueError):
        ops.QuantizedWeight(codes, torch.ones(5))
    with pytest.raises(ValueError):
        ops.quantize_weight(torch.zeros(4))


# ---- model -------------------------------------------------------------------------------------

def _dequantised_reference(model, W, seq):
    """Logits of every position from a full fp32 forward of a copy whose block linears hold the dequantised
    weights, the head applied to its final-LayerNorm output as h @ head.dequantize().T."""
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for blk, qb in zip(ref.blocks, W.blocks):
            for name in ("qkv", "proj", "fc1", "fc2"):
                getattr(blk, name).weight.copy_(qb[name].dequantize())
        x = F.embedding(seq, ref.tok) + ref.pos[:seq.shape[1]]
        for blk in ref.blocks:
            x = blk(x)
        return ref.ln_f(x) @ W.head.dequantize().T


def test_cached_steps_on_quantised_weights_match_the_dequantised_full_forward(model):
    B, T, steps = 2, 8, 8
    seq = _prompt(B, T + steps, seed=1)
    W = model.decode_weights()
    want = _dequantised_reference(model, W, seq)
    cache = model.new_cache(B, T + steps)
    got = [model.extend(seq[:, :T], cache, weights=W)]                       # 16 rows: every linear quantised
    for i in range(steps):
        got.append(model.decode_step(seq[:, T + i], cache, weights=W).unsqueeze(1))
    got = torch.cat(got, 1)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-4
    # the quantisation is really in: the original weights give visibly different logits
    with torch.no_grad():
        assert (model(seq) - want).abs().max().item() > 1e-3


def test_steps_of_more_than_16_rows_read_the_original_weights(model):
    B, T = 2, 16  # B * T = 32
    seq = _prompt(B, T, seed=2)
    W = model.decode_weights()
    c0, c1 = model.new_cache(B, T), model.new_cache(B, T)
    assert torch.equal(model.extend(seq, c0, weights=W), model.extend(seq, c1))
    # last_only: the linears take 32 rows (original weights), the head 2 rows (quantised)
    c0.reset(), c1.reset()
    a, b = model.extend(seq, c0, last_only=True, weights=W), model.extend(seq, c1, last_only=True)
    assert not torch.equal(a, b)
    with torch.no_grad():  # exactly the quantised head on the original blocks' output
        h = F.embedding(seq, model.tok) + model.pos[:T]
        for blk in model.blocks:
            h = blk(h)
        want = model.ln_f(h[:, -1]) @ W.head.dequantize().T
    assert (a - want).abs().max().item() < 1e-4


def test_generate_weight_dtype(model):
    idx = _prompt(2, 9, seed=3)
    new = 10
    W = model.decode_weights()
    out = model.generate(idx, new, weight_dtype=FP8)
    cache = model.new_cache(2, 9 + new)
    toks = [idx, model.prefill(idx, cache).argmax(-1).view(-1, 1)]
    for _ in range(new - 1):
        toks.append(model.decode_step(toks[-1].view(-1), cache, weights=W).argmax(-1).view(-1, 1))
    assert torch.equal(out, torch.cat(toks, 1))
    both = model.generate(idx, new, weight_dtype=FP8, kv_dtype=FP8)  # combines with the FP8 KV cache
    assert both.shape == out.shape and torch.equal(both[:, :9], idx)
    for bad in (torch.int8, torch.bfloat16, torch.float8_e5m2):
        with pytest.raises(ValueError):
            model.generate(idx, new, weight_dtype=bad)
    with pytest.raises(ValueError):
        model.decode_weights(torch.int8)


def test_generate_weight_dtype_with_a_draft(model):
    draft = _perturbed(_cfg(n_layers=1), 12)
    idx = _prompt(1, 7, seed=5)
    out, stats = model.generate(idx, 12, draft=draft, lookahead=3, return_stats=True, weight_dtype=FP8)
    assert out.shape == (1, 19) and torch.equal(out[:, :7], idx)
    assert stats["target_steps"] > 0 and stats["proposed"] >= stats["accepted"] >= 0
    # the target as its own draft on the same quantised weights: every proposal is accepted
    _, self_stats = model.generate(idx, 12, draft=model, lookahead=3, return_stats=True, weight_dtype=FP8)
    assert self_stats["accepted"] == self_stats["proposed"]
    assert "_decode_weights" in draft.__dict__  # the draft decoded on its own quantised weights


def test_decode_weights_memo_requantises_after_an_update():
    m = _perturbed(_cfg(), 13)
    keys = list(m.state_dict().keys())
    nparams = len(list(m.parameters()))
    W = m.decode_weights()
    assert m.decode_weights() is W
    assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == nparams
    assert not list(m.buffers())
    mats = W.matrices()
    assert len(mats) == 4 * len(m.blocks) + 1
    assert W.nbytes == sum(q.nbytes for q in mats) == sum(q.shape[0] * q.shape[1] + 4 * q.shape[0] for q in mats)
    assert W.head.shape == m.tok.shape and W.blocks[0]["qkv"].shape == m.blocks[0].qkv.weight.shape
    with torch.no_grad():
        m.blocks[1].fc1.weight.add_(0.01)
    W2 = m.decode_weights()
    assert W2 is not W and m.decode_weights() is W2
    old, new = W.blocks[1]["fc1"], W2.blocks[1]["fc1"]
    assert not torch.equal(old.codes.view(torch.uint8), new.codes.view(torch.uint8))
    from kubeflow_rm_amd import ops
    fresh = ops.quantize_weight(m.blocks[1].fc1.weight)  # the new codes are those of the updated weight
    assert torch.equal(new.codes.view(torch.uint8), fresh.codes.view(torch.uint8)) and torch.equal(new.scale, fresh.scale)
    assert torch.equal(W2.blocks[0]["qkv"].codes.view(torch.uint8), W.blocks[0]["qkv"].codes.view(torch.uint8))
