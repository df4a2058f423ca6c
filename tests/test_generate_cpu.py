"""KV-cache generation on the torch path (fp32 CPU model): prefill + decode_step against the full
forward, generate against the naive re-run-everything loop, and the cache ops against direct SDPA."""
import math

import pytest
import torch
import torch.nn.functional as F


def _cfg(n_heads=4, max_seq=64):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=128, d_model=64, n_layers=2, n_heads=n_heads, d_ff=128, max_seq=max_seq,
                     dtype=torch.float32)


@pytest.fixture(scope="module")
def model():
    from kubeflow_rm_amd.models import GPT
    m = GPT(_cfg()).eval()
    # the seeded init has zero biases and unit LayerNorm gains: perturb them so every term is exercised
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def _prompt(B, T, seed):
    return torch.randint(0, 128, (B, T), generator=torch.Generator().manual_seed(seed))


def test_kvcache_bookkeeping():
    from kubeflow_rm_amd import ops
    c = ops.KVCache(3, 2, 4, 16, 10, device="cpu", dtype=torch.float32)
    assert len(c.k) == len(c.v) == 3 and c.k[0].shape == (2, 4, 10, 16)
    assert c.lens.dtype == torch.int32 and c.lens.tolist() == [0, 0] and c.t_bound == 0
    after = c.lens_after(4)  # what a step that appends 4 rows hands to its attention; lens itself stays
    assert after.tolist() == [4, 4] and c.bound_after(4) == 4 and c.lens.tolist() == [0, 0] and c.t_bound == 0
    c.advance(4)
    assert c.lens.tolist() == [4, 4] and c.t_bound == 4
    c.advance(1)
    assert c.lens.tolist() == [5, 5] and c.t_bound == 5
    c.set_lens([2, 9])
    assert c.lens.tolist() == [2, 9] and c.t_bound == 9
    assert c.bound_after(5) == 10  # clamped to the capacity
    c.pin_bound()
    assert c.t_bound == 10 and c.bound_after(1) == 10
    c.reset()
    assert c.lens.tolist() == [0, 0]
    with pytest.raises(ValueError):
        c.set_lens([0, 11])


def test_cpu_kv_append_and_attention_decode_match_direct_sdpa():
    from kubeflow_rm_amd import ops
    B, H, D, cap = 3, 2, 16, 12
    g = torch.Generator().manual_seed(3)
    cache = ops.KVCache(1, B, H, D, cap, device="cpu", dtype=torch.float32)
    cache.k[0].fill_(7.0)
    cache.v[0].fill_(7.0)
    qkv = torch.randn(B, 5, 3 * H * D, generator=g)
    ops.kv_append(qkv, cache, 0)
    cache.advance(5)
    x = qkv.view(B, 5, 3, H, D)
    assert torch.equal(cache.k[0][:, :, :5], x[:, :, 1].transpose(1, 2))
    assert torch.equal(cache.v[0][:, :, :5], x[:, :, 2].transpose(1, 2))
    assert (cache.k[0][:, :, 5:] == 7.0).all() and (cache.v[0][:, :, 5:] == 7.0).all()
    # per-row positions; the row that would land at the capacity is dropped
    cache.set_lens([5, 2, cap])
    one = torch.randn(B, 1, 3 * H * D, generator=g)
    before = cache.k[0].clone()
    ops.kv_append(one, cache, 0)
    y = one.view(B, 1, 3, H, D)
    assert torch.equal(cache.k[0][0, :, 5], y[0, 0, 1]) and torch.equal(cache.k[0][1, :, 2], y[1, 0, 1])
    assert torch.equal(cache.k[0][2], before[2])
    # attention over keys 0 .. lens[b]-1 against SDPA on the sliced cache
    lens = [6, 3, cap]
    cache.set_lens(lens)
    q = torch.randn(B, H, D, generator=g)
    o, lse = ops.attention_decode(q, cache, 0, return_lse=True)
    for b, n in enumerate(lens):
        k, v = cache.k[0][b:b + 1, :, :n], cache.v[0][b:b + 1, :, :n]
        ref = F.scaled_dot_product_attention(q[b:b + 1].unsqueeze(2), k, v).squeeze(2)
        assert torch.allclose(o[b:b + 1], ref, atol=1e-5)
        s = (q[b].unsqueeze(1) @ k[0].transpose(-1, -2)).squeeze(1) / math.sqrt(D)
        assert torch.allclose(lse[b], torch.logsumexp(s, -1), atol=1e-5)
    out = torch.zeros(B, 1, H * D)
    ops.attention_decode(q, cache, 0, out=out.view(B, H, D))
    assert torch.equal(out.view(B, H, D), o)


@pytest.mark.parametrize("n_heads", [4, 2])
def test_prefill_and_decode_step_match_full_forward(n_heads):
    from kubeflow_rm_amd.models import GPT
    m = GPT(_cfg(n_heads)).eval()
    B, T0, steps = 2, 9, 12
    seq = _prompt(B, T0 + steps, seed=1)
    with torch.no_grad():
        full = m(seq)  # [B, T, vocab]
    cache = m.new_cache(B, T0 + steps)
    logits = m.prefill(seq[:, :T0], cache)
    assert logits.shape == (B, 128)
    assert (logits - full[:, T0 - 1]).abs().max().item() < 1e-4
    for i in range(steps):
        logits = m.decode_step(seq[:, T0 + i], cache)
        assert (logits - full[:, T0 + i]).abs().max().item() < 1e-4, i
    assert cache.lens.tolist() == [T0 + steps] * B
    with pytest.raises(ValueError):  # the cache is full
        m.decode_step(seq[:, 0], cache)


def test_greedy_generate_equals_naive_full_forward_loop(model):
    B, T0, new = 2, 7, 20
    idx = _prompt(B, T0, seed=5)
    naive, margin = idx, float("inf")
    with torch.no_grad():
        for _ in range(new):
            last = model(naive)[:, -1]
            top2 = last.topk(2, -1).values
            margin = min(margin, (top2[:, 0] - top2[:, 1]).min().item())
            naive = torch.cat([naive, last.argmax(-1, keepdim=True)], 1)
    # the comparison below cannot turn on a tie: cached and full-forward logits agree to 1e-4
    assert margin > 1e-3, margin
    out = model.generate(idx, new)
    assert out.shape == (B, T0 + new)
    assert torch.equal(out[:, :T0], idx)
    assert torch.equal(out, naive)


def test_generate_capacity_error_and_zero_tokens(model):
    idx = _prompt(1, 60, seed=2)
    with pytest.raises(ValueError):
        model.generate(idx, 5)  # 65 > max_seq 64
    assert model.generate(idx, 4).shape == (1, 64)
    assert torch.equal(model.generate(idx, 0), idx)
    with pytest.raises(ValueError):
        model.generate(idx, 2, graph=True)  # hipGraph capture needs GPU tensors


def test_sampling_top_k_and_seed(model):
    idx = _prompt(2, 6, seed=9)
    greedy = model.generate(idx, 10)
    assert torch.equal(model.generate(idx, 10, temperature=1.0, top_k=1), greedy)
    a = model.generate(idx, 10, temperature=1.0, generator=torch.Generator().manual_seed(4))
    b = model.generate(idx, 10, temperature=1.0, generator=torch.Generator().manual_seed(4))
    c = model.generate(idx, 10, temperature=1.0, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)
    assert not torch.equal(a, c)  # 128-way sampling at temperature 1: 20 draws do not all coincide
    assert not torch.equal(a, greedy)
    k5 = model.generate(idx, 10, temperature=1.0, top_k=5, generator=torch.Generator().manual_seed(4))
    assert torch.equal(k5[:, :6], idx) and int(k5.max()) < 128


def test_top_k_sampling_stays_inside_the_top_k_set(model):
    """Every sampled token lies among the top_k logits of its step (recomputed by a full forward on the
    generated prefix), and the sampling is not greedy in disguise."""
    B, T0, new, k = 2, 6, 24, 3
    idx = _prompt(B, T0, seed=13)
    out = model.generate(idx, new, temperature=2.0, top_k=k, generator=torch.Generator().manual_seed(8))
    assert torch.equal(out[:, :T0], idx)
    ranks = []
    with torch.no_grad():
        full = model(out)  # logits[:, t] predict token t + 1
    for t in range(T0 - 1, T0 + new - 1):
        vals, top = full[:, t].topk(k + 1, -1)
        # the cached logits agree with these to 1e-4: the k-th / (k+1)-th gap decides membership
        assert (vals[:, k - 1] - vals[:, k]).min().item() > 1e-3
        hit = top[:, :k] == out[:, t + 1].unsqueeze(1)
        assert hit.any(-1).all(), t
        ranks += hit.float().argmax(-1).tolist()
    assert set(ranks) == {0, 1, 2}, ranks  # 48 draws at temperature 2: every rank of the top 3 shows up


def test_sample_top_k_path_directly():
    """The topk / softmax / multinomial / gather path itself (generate's top_k == 1 takes argmax)."""
    from kubeflow_rm_amd.models.gpt import _sample, _sample_top_k
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(64, 50, generator=g)
    # one candidate: the argmax, whatever the temperature
    assert torch.equal(_sample_top_k(logits, 1.0, 1, g), logits.argmax(-1))
    assert torch.equal(_sample_top_k(logits, 7.0, 1, g), logits.argmax(-1))
    # two candidates at a vanishing temperature: the larger one, always
    assert torch.equal(_sample(logits, 1e-6, 2, g), logits.argmax(-1))
    # k = 4: only the four largest are drawn, each of them at some point, in proportion to softmax
    row = torch.tensor([[0.0, 3.0, 1.0, 2.5, -1.0, 2.0, 0.5]]).expand(4000, 7)
    draws = _sample(row, 1.0, 4, g)
    counts = torch.bincount(draws, minlength=7).float()
    assert counts[[0, 4, 6]].sum().item() == 0
    want = torch.softmax(torch.tensor([3.0, 1.0, 2.5, 2.0]), 0)
    got = counts[[1, 2, 3, 5]] / 4000
    assert (got - want).abs().max().item() < 0.03, got  # 4 sigma of a 4000-draw frequency is < 0.032
    # top_k above the vocabulary is the whole vocabulary
    assert int(_sample(row, 1.0, 50, g).max()) < 7


def test_tensor_parallel_group_raises_on_every_path(model, monkeypatch):
    """A TP group that would issue collectives is refused on the torch path too: F.linear on the row
    shards without the all-reduce would return wrong logits silently."""
    from kubeflow_rm_amd.parallel import tp as tpl
    idx = _prompt(1, 4, seed=1)
    cache = model.new_cache(1, 8)
    monkeypatch.setattr(tpl, "_collective", lambda group: True)
    with pytest.raises(NotImplementedError):
        model.prefill(idx, cache)
    with pytest.raises(NotImplementedError):
        model.decode_step(idx[:, 0], cache)
    with pytest.raises(NotImplementedError):
        model.generate(idx, 2)
    assert cache.lens.tolist() == [0]
