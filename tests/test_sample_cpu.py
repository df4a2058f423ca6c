"""ops.sample's torch form (the fp64 reference of the sampling rule) against a brute-force oracle that sorts
in Python, and the GPT.generate plumbing of sampler="fused" on the CPU."""
from __future__ import annotations

import math

import pytest
import torch

from kubeflow_rm_amd import ops
from kubeflow_rm_amd.models import gpt
from kubeflow_rm_amd.models.gpt import _sample

NINF = float("-inf")


def oracle(x, u, temperature=1.0, top_k=None, top_p=None):
    """The rule, one row, with Python floats: (token, the kept token set)."""
    x = [float(v) for v in x]
    V = len(x)
    order = sorted(range(V), key=lambda i: (-x[i], i))
    if temperature == 0 or top_k == 1:
        return order[0], {order[0]}
    kept = order[:min(top_k, V)] if top_k is not None else order
    w = {i: math.exp((x[i] - x[order[0]]) / temperature) for i in kept}
    if top_p is not None and top_p < 1.0:
        Z, run, n = math.fsum(w.values()), 0.0, 0
        for i in kept:
            run += w[i]
            n += 1
            if run >= top_p * Z:
                break
        kept = kept[:n]
    W = math.fsum(w[i] for i in kept)
    run, tok = 0.0, None
    for i in sorted(kept):
        run += w[i]
        if run > u * W:
            tok = i
            break
    if tok is None:
        tok = max(i for i in kept if w[i] > 0)
    return tok, set(kept)


def sample1(x, u, *a, **kw):
    return int(ops.sample(torch.tensor([x], dtype=torch.float32), torch.tensor([u], dtype=torch.float32), *a, **kw)[0])


def drawn(x, *a, n=64, **kw):
    """The tokens a sweep of uniforms draws."""
    return {sample1(x, (i + 0.5) / n, *a, **kw) for i in range(n)}


def test_all_equal_logits():
    V = 9
    x = [1.5] * V
    assert drawn(x, 1.0, 3) == {0, 1, 2}
    assert drawn(x, 1.0, None, 0.5) == set(range(math.ceil(V / 2)))
    assert sample1(x, 0.3, 0.0) == 0 and sample1(x, 0.3, 1.0, 1) == 0
    for u in (0.0, 0.49, 1 - 2.0 ** -24):
        assert sample1(x, u, 1.0, 3) == oracle(x, u, 1.0, 3)[0]


def test_tie_group_straddling_both_cuts():
    # order: 4 (3.0), then the tie group {1, 2, 5, 7} at 2.0, then 0, 3, 6
    x = [0.0, 2.0, 2.0, -1.0, 3.0, 2.0, -2.0, 2.0]
    assert drawn(x, 1.0, 3) == {4, 1, 2}  # top_k cuts inside the group: lowest indices first
    w4, w2 = 1.0, math.exp(-1.0)
    p = (w4 + 1.5 * w2) / (w4 + 3 * w2)  # top_p inside the top-4 set needs two members of the group
    assert drawn(x, 1.0, 4, p) == {4, 1, 2}
    assert drawn(x, 1.0, None, (w4 + 0.5 * w2) / sum(math.exp(v - 3.0) for v in x)) == {4, 1}
    for u in (0.0, 0.2, 0.5, 0.77, 0.999):
        for k, pp in ((3, None), (4, p), (None, 0.8), (5, 0.99)):
            assert sample1(x, u, 1.0, k, pp) == oracle(x, u, 1.0, k, pp)[0]


def test_minus_inf_is_never_drawn():
    x = [NINF, 0.5, NINF, 0.25, NINF]
    assert drawn(x, 1.0) == {1, 3}
    assert drawn(x, 1.0, 4) == {1, 3}  # the top-k set holds an -inf token: still never drawn
    assert sample1(x, 1 - 2.0 ** -24, 1.0, 5) == 3
    assert sample1(x, 0.0, 1.0) == 1
    assert sample1([NINF, 2.0], 0.9, 0.0) == 1


@pytest.mark.parametrize("seed", range(4))
def test_random_rows_against_the_oracle(seed):
    g = torch.Generator().manual_seed(seed)
    V = 37
    x = (torch.randn(V, generator=g) * 4).to(torch.bfloat16).float().tolist()  # bf16 values: natural ties
    for u in (0.0, 0.013, 0.4, 0.8, 1 - 2.0 ** -24):
        for temperature in (0.7, 1.0):
            for k, p in ((None, None), (5, None), (V, None), (V + 9, None), (None, 1.0), (None, 0.9), (8, 0.6)):
                assert sample1(x, u, temperature, k, p) == oracle(x, u, temperature, k, p)[0], (u, temperature, k, p)


def test_v_equals_one_and_batches():
    assert sample1([0.3], 0.99, 1.0, 4, 0.2) == 0
    x = torch.tensor([[0.0, 5.0, 1.0], [7.0, 0.0, 7.0]])
    assert ops.sample(x, torch.tensor([0.5, 0.9]), 0.0).tolist() == [1, 0]
    assert ops.sample(x.to(torch.bfloat16), torch.tensor([0.999, 0.999]), 1.0, 2).tolist() == [2, 2]


def test_schedule_step_out_seq_done():
    x = torch.tensor([[0.0, 9.0, 0.0], [9.0, 0.0, 0.0]])
    u = torch.rand(4, 2, generator=torch.Generator().manual_seed(0))
    step = torch.tensor([2], dtype=torch.int32)
    out = torch.full((2,), -1, dtype=torch.int64)
    seq = torch.full((2, 4), -1, dtype=torch.int64)
    done = torch.zeros(2, dtype=torch.int32)
    got = ops.sample(x, u, 0.0, step=step, out=out, seq=seq, done=done, stop_token=1)
    assert got is out and out.tolist() == [1, 0] and done.tolist() == [1, 0]
    assert seq.tolist() == [[-1, -1, 1, -1], [-1, -1, 0, -1]] and step.item() == 2
    x[0] = torch.tensor([9.0, 0.0, 0.0])
    assert ops.sample(x, u, 0.0, step=step, done=done, stop_token=1).tolist() == [1, 0]  # row 0 stays finished


def test_sample_value_errors():
    x, u = torch.zeros(2, 4), torch.zeros(2)
    for bad in (0.0, -0.5, 1.0001):
        with pytest.raises(ValueError):
            ops.sample(x, u, top_p=bad)
    with pytest.raises(ValueError):
        ops.sample(x, u, top_k=0)
    with pytest.raises(ValueError):
        ops.sample(x, u, temperature=-1.0)
    with pytest.raises(ValueError):
        ops.sample(x, torch.zeros(3, 2))  # a schedule without step
    with pytest.raises(ValueError):
        ops.sample(x, u, stop_token=1)  # no done
    with pytest.raises(ValueError):
        ops.sample(x, u.double())


@pytest.fixture(scope="module")
def model():
    cfg = gpt.GPTConfig(vocab_size=61, d_model=32, n_layers=2, n_heads=2, d_ff=64, max_seq=48, dtype=torch.float32)
    return gpt.build(cfg).eval()


ARGS = dict(temperature=0.9, top_k=12, top_p=0.85)


def _hand_loop(model, idx, S, seed, **args):
    B, T0 = idx.shape
    u = torch.rand(S, B, generator=torch.Generator().manual_seed(seed))
    cache = model.new_cache(B, T0 + S)
    logits = model.prefill(idx, cache)
    toks = [idx]
    for s in range(S):
        tok = ops.sample(logits, u[s].contiguous(), **args)
        toks.append(tok.view(B, 1))
        if s + 1 < S:
            logits = model.decode_step(tok, cache)
    return torch.cat(toks, 1)


def test_generate_fused_equals_the_hand_loop_and_is_seeded(model):
    idx = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(2))
    a = model.generate(idx, 10, generator=torch.Generator().manual_seed(7), sampler="fused", **ARGS)
    assert a.shape == (3, 15) and a.dtype == torch.int64
    assert torch.equal(a, _hand_loop(model, idx, 10, 7, **ARGS))
    assert torch.equal(a, model.generate(idx, 10, generator=torch.Generator().manual_seed(7), sampler="fused", **ARGS))
    assert not torch.equal(a, model.generate(idx, 10, generator=torch.Generator().manual_seed(8), sampler="fused",
                                             **ARGS))
    greedy = model.generate(idx, 6, sampler="fused")  # temperature 0: the argmax, as the torch sampler's
    assert torch.equal(greedy, model.generate(idx, 6))


def test_generate_stop_token_pads_finished_rows(model):
    idx = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(2))
    free = model.generate(idx, 12, generator=torch.Generator().manual_seed(7), sampler="fused", **ARGS)
    stop = int(free[1, 5 + 4])  # row 1 emits it mid-way
    out = model.generate(idx, 12, generator=torch.Generator().manual_seed(7), sampler="fused", stop_token=stop, **ARGS)
    assert out.shape == free.shape
    for b in range(3):
        hits = (free[b, 5:] == stop).nonzero()
        n = 5 + (int(hits[0, 0]) if len(hits) else 12)
        assert torch.equal(out[b, :n], free[b, :n])  # the uniforms are per step and row: unchanged until the stop
        assert (out[b, n:] == stop).all()
    assert (out[1, 9:] == stop).all()
    assert any(not (out[b, 5:] == stop).any() or (free[b, 5:] == stop).nonzero()[0, 0] > 4 for b in (0, 2))


def test_generate_value_errors(model):
    idx = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        model.generate(idx, 2, temperature=1.0, top_p=0.9)  # sampler="torch"
    with pytest.raises(ValueError):
        model.generate(idx, 2, stop_token=3)
    with pytest.raises(ValueError):
        model.generate(idx, 2, sampler="other")
    with pytest.raises(ValueError):
        model.generate(idx, 2, sampler="fused", draft=model)
    with pytest.raises(ValueError):
        model.generate(idx, 2, temperature=1.0, sampler="fused", top_p=1.5)
    with pytest.raises(ValueError):
        model.generate(idx, 2, sampler="fused", graph=True)  # CPU tensors


def test_torch_sampler_is_unchanged(model):
    """sampler="torch" with default arguments: the parent's loop of prefill / _sample / decode_step."""
    idx = torch.randint(0, 61, (2, 4), generator=torch.Generator().manual_seed(3))
    for temperature, top_k in ((0.0, None), (1.0, None), (0.8, 7)):
        got = model.generate(idx, 8, temperature=temperature, top_k=top_k, generator=torch.Generator().manual_seed(11))
        g = torch.Generator().manual_seed(11)
        cache = model.new_cache(2, 12)
        logits = model.prefill(idx, cache)
        toks = [idx]
        for i in range(8):
            nxt = _sample(logits, temperature, top_k, g)
            toks.append(nxt.view(2, 1))
            if i + 1 < 8:
                logits = model.decode_step(nxt, cache)
        assert torch.equal(got, torch.cat(toks, 1))
