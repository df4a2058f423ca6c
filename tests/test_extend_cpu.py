"""Multi-token KV-cache steps on the torch path (fp32 CPU model): attention_extend against direct masked
SDPA, GPT.extend against the full forward, KVCache.rewind, and draft-and-verify generate against plain
greedy generate."""
import math

import pytest
import torch
import torch.nn.functional as F


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


def test_cpu_attention_extend_matches_direct_masked_sdpa():
    from kubeflow_rm_amd import ops
    B, H, D, cap, T = 3, 2, 16, 12, 4
    g = torch.Generator().manual_seed(3)
    cache = ops.KVCache(1, B, H, D, cap, device="cpu", dtype=torch.float32)
    cache.k[0].copy_(torch.randn(B, H, cap, D, generator=g))
    cache.v[0].copy_(torch.randn(B, H, cap, D, generator=g))
    lens = [4, 9, 2]  # the block is the whole sequence; has a prefix; starts before the sequence (2 < T)
    for b, n in enumerate(lens):  # rows no query may see
        cache.k[0][b, :, n:] = float("nan")
        cache.v[0][b, :, n:] = float("nan")
    cache.set_lens(lens)
    q = torch.randn(B, T, H, D, generator=g)
    o, lse = ops.attention_extend(q, cache, 0, return_lse=True)
    assert o.shape == (B, T, H, D) and lse.shape == (B, T, H)
    for b, n in enumerate(lens):
        for i in range(T):
            nk = n - T + i + 1
            if nk <= 0:
                assert (o[b, i] == 0).all() and (lse[b, i] == float("-inf")).all()
                continue
            k, v = cache.k[0][b:b + 1, :, :nk], cache.v[0][b:b + 1, :, :nk]
            ref = F.scaled_dot_product_attention(q[b:b + 1, i].unsqueeze(2), k, v).squeeze(2)
            assert torch.allclose(o[b:b + 1, i], ref, atol=1e-5), (b, i)
            s = (q[b, i].unsqueeze(1) @ k[0].transpose(-1, -2)).squeeze(1) / math.sqrt(D)
            assert torch.allclose(lse[b, i], torch.logsumexp(s, -1), atol=1e-5)
    out = torch.zeros(B, T, H * D)
    ops.attention_extend(q, cache, 0, out=out.view(B, T, H, D))
    assert torch.equal(out.view(B, T, H, D), o)
    # one row is attention_decode (whose torch path multiplies the dead rows by zero: clean them first)
    cache.k[0].nan_to_num_(0.0)
    cache.v[0].nan_to_num_(0.0)
    one = ops.attention_extend(q[:, :1], cache, 0)
    assert torch.allclose(one[:, 0], ops.attention_decode(q[:, 0], cache, 0), atol=1e-6)
    with pytest.raises(ValueError):
        ops.attention_extend(q[:, :, :1], cache, 0)


def test_rewind_bookkeeping():
    from kubeflow_rm_amd import ops
    c = ops.KVCache(1, 2, 2, 16, 10, device="cpu", dtype=torch.float32)
    c.set_lens([3, 7])
    c.k[0].fill_(5.0)
    c.rewind(2)
    assert c.lens.tolist() == [1, 5] and c.t_bound == 5 and c.lens.dtype == torch.int32
    assert (c.k[0] == 5.0).all()  # rows stay in memory
    c.rewind(3)
    assert c.lens.tolist() == [0, 2] and c.t_bound == 2  # clamped at 0 per row
    c.rewind(0)
    assert c.lens.tolist() == [0, 2]
    c.advance(4)
    assert c.lens.tolist() == [4, 6] and c.t_bound == 6
    c.pin_bound()
    c.rewind(5)
    assert c.lens.tolist() == [0, 1] and c.t_bound == 10 and c.bound_after(1) == 10  # a pinned bound stays
    with pytest.raises(ValueError):
        c.rewind(-1)


def test_extend_in_chunks_matches_full_forward(model):
    B, total = 2, 50
    seq = _prompt(B, total, seed=1)
    with torch.no_grad():
        full = model(seq)
    cache = model.new_cache(B, total)
    got, at = [], 0
    for T in (1, 3, 20, 16, 10):  # from an empty cache; 20 runs as 16 + 4
        lg = model.extend(seq[:, at:at + T], cache)
        assert lg.shape == (B, T, 128)
        got.append(lg)
        at += T
        assert cache.lens.tolist() == [at] * B and cache.t_bound == at
    assert at == total
    assert (torch.cat(got, 1) - full).abs().max().item() < 1e-4
    with pytest.raises(ValueError):  # the cache is full
        model.extend(seq[:, :1], cache)
    # last_only; prefill + extend; extend + decode_step
    cache.reset()
    model.prefill(seq[:, :9], cache)
    last = model.extend(seq[:, 9:30], cache, last_only=True)
    assert last.shape == (B, 128) and (last - full[:, 29]).abs().max().item() < 1e-4
    step = model.decode_step(seq[:, 30], cache)
    assert (step - full[:, 30]).abs().max().item() < 1e-4
    # rewind: dead rows are overwritten
    cache.rewind(6)
    again = model.extend(seq[:, 25:31], cache)
    assert (again - full[:, 25:31]).abs().max().item() < 1e-4
    with pytest.raises(ValueError):
        model.extend(seq[:, :0], cache)


def test_extend_ragged_rows(model):
    """Rows at different positions: extend reads every position from cache.lens."""
    seq = _prompt(2, 30, seed=2)
    with torch.no_grad():
        full = model(seq)
    cache = model.new_cache(2, 30)
    model.extend(seq[:, :12], cache)
    cache.set_lens([12, 7])  # row 1 goes back to position 7
    nxt = torch.stack([seq[0, 12:17], seq[1, 7:12]])
    lg = model.extend(nxt, cache)
    assert (lg[0] - full[0, 12:17]).abs().max().item() < 1e-4
    assert (lg[1] - full[1, 7:12]).abs().max().item() < 1e-4
    assert cache.lens.tolist() == [17, 12]


def _greedy_margin(model, idx, new):
    """Top-2 logit gap of the plain greedy run (full forwards), minimum over the steps."""
    cur, margin = idx, float("inf")
    with torch.no_grad():
        for _ in range(new):
            last = model(cur)[:, -1]
            top2 = last.topk(2, -1).values
            margin = min(margin, (top2[:, 0] - top2[:, 1]).min().item())
            cur = torch.cat([cur, last.argmax(-1, keepdim=True)], 1)
    return margin


@pytest.mark.parametrize("new,lookahead", [(24, 4), (11, 3), (1, 4)])
def test_draft_generate_equals_plain_greedy(model, new, lookahead):
    idx = _prompt(1, 7, seed=5)
    # cached and full-forward logits agree to 1e-4: the comparisons below cannot turn on a tie
    assert _greedy_margin(model, idx, new) > 1e-3
    plain = model.generate(idx, new)
    # the target as its own draft: every proposal is accepted
    out, stats = model.generate(idx, new, draft=model, lookahead=lookahead, return_stats=True)
    assert out.shape == plain.shape and torch.equal(out, plain)
    assert stats["target_steps"] == math.ceil(new / (lookahead + 1)), stats
    assert stats["accepted"] == stats["proposed"] == new - stats["target_steps"], stats
    # a one-layer draft: some proposals are rejected, the output is the target's greedy sequence anyway
    small = _perturbed(_cfg(n_layers=1), 12)
    out, stats = model.generate(idx, new, draft=small, lookahead=lookahead, return_stats=True)
    assert torch.equal(out, plain)
    assert 0 <= stats["accepted"] <= stats["proposed"] and stats["target_steps"] >= math.ceil(new / (lookahead + 1))
    assert torch.equal(model.generate(idx, new, draft=small, lookahead=lookahead), plain)
    assert torch.equal(model.generate(idx, new, temperature=1.0, top_k=1, draft=small), plain)


def test_draft_generate_one_token_prompt_and_refusals(model):
    idx = _prompt(1, 1, seed=6)
    assert _greedy_margin(model, idx, 9) > 1e-3
    assert torch.equal(model.generate(idx, 9, draft=model, lookahead=2), model.generate(idx, 9))
    out, stats = model.generate(idx, 0, draft=model, return_stats=True)
    assert torch.equal(out, idx) and stats == {"target_steps": 0, "proposed": 0, "accepted": 0}
    with pytest.raises(ValueError):
        model.generate(_prompt(2, 4, seed=1), 4, draft=model)  # B = 2
    with pytest.raises(ValueError):
        model.generate(idx, 4, temperature=0.7, draft=model)
    with pytest.raises(ValueError):
        model.generate(idx, 4, graph=True, draft=model)
    with pytest.raises(ValueError):
        model.generate(idx, 4, draft=model, lookahead=0)
    with pytest.raises(ValueError):
        model.generate(idx, 4, return_stats=True)  # stats describe draft decoding
    from kubeflow_rm_amd.models import GPT, GPTConfig
    other = GPT(GPTConfig(vocab_size=64, d_model=64, n_layers=1, n_heads=4, d_ff=128, max_seq=64,
                          dtype=torch.float32)).eval()
    with pytest.raises(ValueError):
        model.generate(idx, 4, draft=other)  # another vocabulary


def test_tensor_parallel_group_raises_on_extend(model, monkeypatch):
    from kubeflow_rm_amd.parallel import tp as tpl
    idx = _prompt(1, 4, seed=1)
    cache = model.new_cache(1, 8)
    monkeypatch.setattr(tpl, "_collective", lambda group: True)
    with pytest.raises(NotImplementedError):
        model.extend(idx, cache)
    with pytest.raises(NotImplementedError):
        model.generate(idx, 2, draft=model)
    assert cache.lens.tolist() == [0]
