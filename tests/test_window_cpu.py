"""Sliding-window attention on the torch path (fp32 CPU): the three cache attention ops against a masked softmax
written here from the rule of ``ops/decode.py`` (a row of causal limit L sees key j iff max(0, L - W) <= j < L), and
the windowed GPT (prefill / decode_step / extend / extend(chunk=) / generate) against its own full-sequence forward.
Tolerances: those of the unwindowed counterparts in test_generate_cpu.py / test_extend_cpu.py / test_attn_chunk_cpu.py
(ops atol 1e-5, model logits 1e-4)."""
import math

import pytest
import torch

B, H, D, CAP = 4, 2, 64, 40


def _cache(seed=0, G=1):
    """A full fp32 cache of random rows (every position finite) and a q source."""
    from kubeflow_rm_amd import ops
    g = torch.Generator().manual_seed(seed)
    cache = ops.KVCache(1, B, H, D, CAP, device="cpu", dtype=torch.float32)
    cache.k[0].copy_(torch.randn(B, H, CAP, D, generator=g))
    cache.v[0].copy_(torch.randn(B, H, CAP, D, generator=g))
    return cache, g


def _direct(q, cache, lens, W):
    """fp32 masked softmax, row by row, straight from the rule. q [B, T, Hq, D] -> (o [B, T, Hq, D], lse [B, T, Hq])."""
    Bq, T, Hq, _ = q.shape
    G = Hq // cache.H
    o = torch.zeros(Bq, T, Hq, D)
    lse = torch.full((Bq, T, Hq), float("-inf"))
    for b in range(Bq):
        for i in range(T):
            L = lens[b] - T + i + 1
            lo = max(0, L - W) if W is not None else 0
            if L <= lo:
                continue  # no key: zeros, lse = -inf
            for h in range(Hq):
                k, v = cache.k[0][b, h // G, lo:L], cache.v[0][b, h // G, lo:L]
                s = (k @ q[b, i, h]) / math.sqrt(D)
                lse[b, i, h] = torch.logsumexp(s, 0)
                o[b, i, h] = torch.softmax(s, 0) @ v
    return o, lse


@pytest.mark.parametrize("W", [1, 5, 17, CAP - 1])
def test_decode_reference_follows_the_rule(W):
    from kubeflow_rm_amd import ops
    cache, g = _cache(1)
    lens = [1, 3, W + 4 if W + 4 <= CAP else CAP, CAP]  # lens < W, lens > W, the full cache
    cache.set_lens(lens)
    q = torch.randn(B, H, D, generator=g)
    o, lse = ops.attention_decode(q, cache, 0, return_lse=True, window=W)
    ro, rl = _direct(q.unsqueeze(1), cache, lens, W)
    assert torch.allclose(o, ro[:, 0], atol=1e-5)
    assert torch.allclose(lse, rl[:, 0], atol=1e-5)
    out = torch.zeros(B, H, D)
    assert ops.attention_decode(q, cache, 0, out=out, window=W) is out and torch.equal(out, o)


@pytest.mark.parametrize("op", ["attention_extend", "attention_chunk"])
@pytest.mark.parametrize("W", [1, 5, 17])
@pytest.mark.parametrize("G", [1, 2])
def test_extend_and_chunk_references_follow_the_rule(op, W, G):
    from kubeflow_rm_amd import ops
    cache, g = _cache(2)
    T = 6
    lens = [T, 3, W + 2 if W + 2 >= T else T + 1, CAP]  # lens == Tq, lens < Tq (rows before the start), lens < / > W
    cache.set_lens(lens)
    q = torch.randn(B, T, G * H, D, generator=g)
    o, lse = getattr(ops, op)(q, cache, 0, return_lse=True, window=W)
    ro, rl = _direct(q, cache, lens, W)
    assert torch.allclose(o, ro, atol=1e-5)
    finite = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), finite) and torch.allclose(lse[finite], rl[finite], atol=1e-5)
    assert (o[~finite] == 0).all()


def test_window_at_or_beyond_the_capacity_is_no_window():
    from kubeflow_rm_amd import ops
    cache, g = _cache(3)
    lens = [6, 9, 23, CAP]
    cache.set_lens(lens)
    q = torch.randn(B, 6, H, D, generator=g)
    for W in (CAP, CAP + 1, 10 ** 6):
        for op in (ops.attention_extend, ops.attention_chunk):
            a, la = op(q, cache, 0, return_lse=True)
            b, lb = op(q, cache, 0, return_lse=True, window=W)
            assert torch.equal(a, b) and torch.equal(la, lb)
        a, la = ops.attention_decode(q[:, 0], cache, 0, return_lse=True)
        b, lb = ops.attention_decode(q[:, 0], cache, 0, return_lse=True, window=W)
        assert torch.equal(a, b) and torch.equal(la, lb)


@pytest.mark.parametrize("bad", [0, -3, True, False, 2.0, "4"])
def test_bad_window_raises(bad):
    from kubeflow_rm_amd import ops
    cache, g = _cache(4)
    cache.set_lens([8] * B)
    q = torch.randn(B, 2, H, D, generator=g)
    with pytest.raises(ValueError):
        ops.attention_decode(q[:, 0], cache, 0, window=bad)
    with pytest.raises(ValueError):
        ops.attention_extend(q, cache, 0, window=bad)
    with pytest.raises(ValueError):
        ops.attention_chunk(q, cache, 0, window=bad)


# ---- the model ---------------------------------------------------------------------------------------------

W_MODEL = 5


def _cfg(kind, window=W_MODEL):
    from kubeflow_rm_amd.models import GPTConfig
    extra = {} if kind == "learned" else {"pos": "rope", "n_kv_heads": 2, "norm": "rms", "mlp": "swiglu"}
    return GPTConfig(vocab_size=128, d_model=64, n_layers=2, n_heads=4, d_ff=128, max_seq=64, dtype=torch.float32,
                     window=window, **extra)


def _model(kind, window=W_MODEL):
    from kubeflow_rm_amd.models import GPT
    m = GPT(_cfg(kind, window)).eval()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # zero biases and unit gains in the seeded init: perturb them so every term is exercised
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def _prompt(Bm, T, seed):
    return torch.randint(0, 128, (Bm, T), generator=torch.Generator().manual_seed(seed))


def _forward_by_hand(m, seq, W):
    """The windowed full-sequence forward on the model's own weights with an explicit mask: the learned-position
    model only (no rotary, LayerNorm, GELU), so that ``forward`` itself has an oracle written here."""
    import torch.nn.functional as F
    Bm, T = seq.shape
    c = m.cfg
    h, hd = c.n_heads, c.head_dim
    i = torch.arange(T)
    seen = (i.view(T, 1) >= i.view(1, T)) & (i.view(T, 1) - i.view(1, T) < W)
    x = F.embedding(seq, m.tok) + m.pos[:T]
    for blk in m.blocks:
        y = F.layer_norm(x, (c.d_model,), blk.ln1.weight, blk.ln1.bias, c.eps)
        q, k, v = F.linear(y, blk.qkv.weight, blk.qkv.bias).view(Bm, T, 3, h, hd).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        a = torch.softmax(s.masked_fill(~seen, float("-inf")), -1) @ v
        x = x + F.linear(a.transpose(1, 2).reshape(Bm, T, h * hd), blk.proj.weight, blk.proj.bias)
        y = F.layer_norm(x, (c.d_model,), blk.ln2.weight, blk.ln2.bias, c.eps)
        y = F.gelu(F.linear(y, blk.fc1.weight, blk.fc1.bias), approximate="tanh")
        x = x + F.linear(y, blk.fc2.weight, blk.fc2.bias)
    x = F.layer_norm(x, (c.d_model,), m.ln_f.weight, m.ln_f.bias, c.eps)
    return F.linear(x, m.tok)


def test_forward_applies_the_windowed_mask():
    m = _model("learned")
    seq = _prompt(2, 23, seed=1)
    with torch.no_grad():
        full = m(seq)
        assert (full - _forward_by_hand(m, seq, W_MODEL)).abs().max().item() < 1e-4
        # and it is not the causal forward: a window at the sequence length is
        causal = _model("learned", window=None)(seq)
        assert (full - causal).abs().max().item() > 1e-3
        assert (_model("learned", window=23)(seq) - causal).abs().max().item() < 1e-5


@pytest.mark.parametrize("kind", ["learned", "llama"])
def test_prefill_decode_extend_chunk_match_the_windowed_forward(kind):
    m = _model(kind)
    Bm, T0, steps = 2, 9, 12
    seq = _prompt(Bm, 40, seed=2)
    with torch.no_grad():
        full = m(seq)  # [B, 40, vocab], the windowed mask
    cache = m.new_cache(Bm, 40)
    logits = m.prefill(seq[:, :T0], cache)
    assert logits.shape == (Bm, 128) and (logits - full[:, T0 - 1]).abs().max().item() < 1e-4
    for i in range(steps):
        logits = m.decode_step(seq[:, T0 + i], cache)
        assert (logits - full[:, T0 + i]).abs().max().item() < 1e-4, i
    at = T0 + steps
    for T in (1, 3, 15):  # extend(T) on a cache longer than the window; 9 + 12 + 1 + 3 + 15 = the 40 positions
        lg = m.extend(seq[:, at:at + T], cache)
        assert lg.shape == (Bm, T, 128) and (lg - full[:, at:at + T]).abs().max().item() < 1e-4, T
        at += T
    assert cache.lens.tolist() == [at] * Bm
    # extend from an empty cache, more rows than one step takes, and in chunks of 17 (19 + 17 + 4 ... rows)
    cache = m.new_cache(Bm, 40)
    lg = m.extend(seq[:, :19], cache)
    assert (lg - full[:, :19]).abs().max().item() < 1e-4
    lg = m.extend(seq[:, 19:], cache, chunk=17)
    assert lg.shape == (Bm, 21, 128) and (lg - full[:, 19:]).abs().max().item() < 1e-4
    cache = m.new_cache(Bm, 40)
    last = m.extend(seq, cache, last_only=True, chunk=17)
    assert (last - full[:, -1]).abs().max().item() < 1e-4


@pytest.mark.parametrize("kind", ["learned", "llama"])
def test_greedy_generate_equals_recomputation_from_scratch(kind):
    m = _model(kind)
    Bm, T0, new = 2, 7, 20
    idx = _prompt(Bm, T0, seed=7)  # a prompt whose greedy steps are no near-ties in either model (the margin below)
    naive, margin = idx, float("inf")
    with torch.no_grad():
        for _ in range(new):
            last = m(naive)[:, -1]
            top2 = last.topk(2, -1).values
            margin = min(margin, (top2[:, 0] - top2[:, 1]).min().item())
            naive = torch.cat([naive, last.argmax(-1, keepdim=True)], 1)
    assert margin > 1e-3, margin  # cached and full-forward logits agree to 1e-4: no comparison turns on a tie
    assert torch.equal(m.generate(idx, new), naive)
    assert torch.equal(m.generate(idx, new, prefill_chunk=17), naive)
    # a draft with no window of its own proposes, the windowed target decides: the target's tokens
    draft = _model(kind, window=None)
    assert torch.equal(m.generate(idx[:1], new, draft=draft, lookahead=3), naive[:1])


@pytest.mark.parametrize("bad", [0, -1, True, 2.5])
def test_config_rejects_a_bad_window(bad):
    from kubeflow_rm_amd.models import GPTConfig
    with pytest.raises(ValueError):
        GPTConfig(window=bad)
    assert GPTConfig(window=None).window is None and GPTConfig(window=1).window == 1
