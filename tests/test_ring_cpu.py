"""The ring-buffer KV cache on the torch path (fp32 CPU): ``KVCache(..., ring=True)`` against a flat cache that holds
every position, fed the same token stream (the ring rule: the docstring of ``ops/decode.py``), its errors, and the
windowed GPT generating on a ring against the same model on a flat cache. Tolerances: those of test_window_cpu.py
(ops atol 1e-5, model logits 1e-4)."""
import pytest
import torch

B, H, D, C = 3, 2, 64, 256
P = 3 * C + 40  # positions the furthest row reaches: past three laps
START = [0, 100, 300]  # the rows of the batch sit at different laps


def _stream(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, P, D, generator=g), torch.randn(B, H, P, D, generator=g), g


def _pair(ks, vs):
    """A flat cache of capacity P and a ring of capacity C that both hold positions 0 .. START[b] - 1 of the stream."""
    from kubeflow_rm_amd import ops
    flat = ops.KVCache(1, B, H, D, P, device="cpu", dtype=torch.float32)
    ring = ops.KVCache(1, B, H, D, C, device="cpu", dtype=torch.float32, ring=True)
    for b, n in enumerate(START):
        flat.k[0][b, :, :n], flat.v[0][b, :, :n] = ks[b, :, :n], vs[b, :, :n]
        for j in range(max(0, n - C), n):
            ring.k[0][b, :, j % C], ring.v[0][b, :, j % C] = ks[b, :, j], vs[b, :, j]
    flat.set_lens(START)
    ring.set_lens(START)
    return flat, ring


def _slots_hold_the_stream(ring, ks, vs, lens):
    for b, n in enumerate(lens):
        j = torch.arange(max(0, n - C), n)
        assert torch.equal(ring.k[0][b][:, j % C], ks[b][:, j]) and torch.equal(ring.v[0][b][:, j % C], vs[b][:, j])


@pytest.mark.parametrize("T", [1, 3, 16, 57])
@pytest.mark.parametrize("W", [1, 5, 200])
def test_ring_ops_equal_the_flat_windowed_ops(W, T):
    from kubeflow_rm_amd import ops
    assert W + T - 1 <= C
    ks, vs, g = _stream(100 * W + T)
    flat, ring = _pair(ks, vs)
    lens = list(START)
    step, Tfull = 0, T
    while max(lens) < P:
        T = min(Tfull, P - max(lens))  # the last step is shorter: the furthest row ends at P exactly
        qkv = torch.randn(B, T, 3 * H * D, generator=g)
        x = qkv.view(B, T, 3, H, D)
        for b in range(B):
            x[b, :, 1] = ks[b, :, lens[b]:lens[b] + T].transpose(0, 1)
            x[b, :, 2] = vs[b, :, lens[b]:lens[b] + T].transpose(0, 1)
        ops.kv_append(qkv, flat, 0)
        ops.kv_append(qkv, ring, 0)
        q = x[:, :, 0]
        for op in (ops.attention_extend, ops.attention_chunk):  # after every step
            a, la = op(q, flat, 0, lens=flat.lens_after(T), t_bound=flat.bound_after(T), return_lse=True, window=W)
            r, lr = op(q, ring, 0, lens=ring.lens_after(T), return_lse=True, window=W)
            assert torch.allclose(r, a, atol=1e-5), (op.__name__, lens)
            assert torch.allclose(lr, la, atol=1e-5), (op.__name__, lens)
        flat.advance(T)
        ring.advance(T)
        lens = [n + T for n in lens]
        a, la = ops.attention_decode(q[:, -1], flat, 0, return_lse=True, window=W)
        r, lr = ops.attention_decode(q[:, -1], ring, 0, return_lse=True, window=W)
        assert torch.allclose(r, a, atol=1e-5) and torch.allclose(lr, la, atol=1e-5), lens
        if step % 5 == 0:
            _slots_hold_the_stream(ring, ks, vs, lens)
        step += 1
    assert max(lens) == P and ring.lens.tolist() == lens and ring._bound == max(lens)
    _slots_hold_the_stream(ring, ks, vs, lens)


def test_fp8_ring_stores_quantize_rows_and_equals_the_flat_cache():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.decode import FP8, quantize_rows
    ks, vs, g = _stream(7)
    flat = ops.KVCache(1, B, H, D, P, device="cpu", dtype=FP8)
    ring = ops.KVCache(1, B, H, D, C, device="cpu", dtype=FP8, ring=True)
    T, W, n = 57, 200, 0
    while n + T <= 2 * C + 30:
        qkv = torch.randn(B, T, 3 * H * D, generator=g)
        x = qkv.view(B, T, 3, H, D)
        x[:, :, 1], x[:, :, 2] = ks[:, :, n:n + T].transpose(1, 2), vs[:, :, n:n + T].transpose(1, 2)
        ops.kv_append(qkv, flat, 0)
        ops.kv_append(qkv, ring, 0)
        a = ops.attention_extend(x[:, :, 0], flat, 0, lens=flat.lens_after(T), t_bound=flat.bound_after(T), window=W)
        r = ops.attention_extend(x[:, :, 0], ring, 0, lens=ring.lens_after(T), window=W)
        assert torch.allclose(r, a, atol=1e-5)
        flat.advance(T)
        ring.advance(T)
        n += T
    j = torch.arange(n - C, n)
    codes, scale = quantize_rows(ks[:, :, j])
    assert torch.equal(ring.k[0][:, :, j % C].view(torch.uint8), codes.view(torch.uint8))
    assert torch.equal(ring.k_scale[0][:, :, j % C], scale)


def test_ring_errors():
    from kubeflow_rm_amd import ops
    for cap in (100, 255, 257, 384):
        with pytest.raises(ValueError):
            ops.KVCache(1, B, H, D, cap, device="cpu", dtype=torch.float32, ring=True)
    ops.KVCache(1, B, H, D, 384, device="cpu", dtype=torch.float32)  # a flat cache takes any capacity
    ring = ops.KVCache(1, B, H, D, C, device="cpu", dtype=torch.float32, ring=True)
    ring.set_lens([5, 700, 2 ** 24])
    q = torch.randn(B, 4, H, D)
    for op, x in ((ops.attention_decode, q[:, 0]), (ops.attention_extend, q), (ops.attention_chunk, q)):
        with pytest.raises(ValueError, match="window"):
            op(x, ring, 0)  # window=None
        with pytest.raises(ValueError, match="t_bound"):
            op(x, ring, 0, window=8, t_bound=C)
    with pytest.raises(ValueError, match="257.*256|256.*257"):
        ops.attention_decode(q[:, 0], ring, 0, window=C + 1)
    with pytest.raises(ValueError, match=str(C - 2)):
        ops.attention_extend(q, ring, 0, window=C - 2)  # W + 4 - 1 = C + 1
    with pytest.raises(ValueError, match=str(C - 2)):
        ops.attention_chunk(q, ring, 0, window=C - 2)
    ops.attention_extend(q, ring, 0, window=C - 3)  # W + T - 1 == C: no dead slot, still fine
    with pytest.raises(ValueError):
        ops.kv_append(torch.randn(B, C + 1, 3 * H * D), ring, 0)  # T > C
    # rewind: beyond C - W + 1 rows the keys before them are overwritten
    ring = ops.KVCache(1, B, H, D, C, device="cpu", dtype=torch.float32, ring=True, window=200)
    ring.set_lens([900] * B)
    with pytest.raises(ValueError):
        ring.rewind(C - 200 + 2)
    ring.rewind(C - 200 + 1)
    assert ring.lens.tolist() == [900 - 57] * B
    # the rope table must hold the absolute positions, not the capacity
    ring.set_lens([900] * B)
    with pytest.raises(ValueError):
        ops.kv_append(torch.randn(B, 2, 3 * H * D), ring, 0, rope=ops.rope_table(901, D))
    ops.kv_append(torch.randn(B, 2, 3 * H * D), ring, 0, rope=ops.rope_table(902, D))


def test_ring_cache_methods():
    from kubeflow_rm_amd import ops
    ring = ops.KVCache(2, B, H, D, C, device="cpu", dtype=torch.float32, ring=True)
    flat = ops.KVCache(2, B, H, D, 4 * C, device="cpu", dtype=torch.float32)
    assert ring.nbytes * 4 == flat.nbytes and ring.nbytes == 2 * 2 * B * H * C * D * 4
    ring.set_lens([0, C, 5 * C + 3])
    ring.advance(C - 1)  # no clamp
    assert ring.lens.tolist() == [C - 1, 2 * C - 1, 6 * C + 2] and ring._bound == 6 * C + 2
    assert ring.t_bound == C and ring.bound_after(3) == C  # still readable, never past the capacity
    ring.pin_bound()
    assert ring.t_bound == C
    ring.rewind(2)
    assert ring.lens.tolist() == [C - 3, 2 * C - 3, 6 * C]
    ring.reset()
    assert ring.lens.tolist() == [0, 0, 0] and ring._bound == 0
    with pytest.raises(ValueError):
        ring.set_lens([1, 2, -1])


# ---- the model ---------------------------------------------------------------------------------------------

W_MODEL, T0, NEW = 40, 300, 400


def _model(kind, window=W_MODEL, n_layers=2):
    from kubeflow_rm_amd.models import GPT, GPTConfig
    extra = {} if kind == "learned" else {"pos": "rope", "n_kv_heads": 2, "norm": "rms", "mlp": "swiglu"}
    torch.manual_seed(3)
    model = GPT(GPTConfig(vocab_size=128, d_model=64, n_layers=n_layers, n_heads=4, d_ff=128, max_seq=1024,
                          dtype=torch.float32, window=window, **extra))
    with torch.no_grad():  # enough weight on the tokens that greedy decoding does not sit on ties
        model.tok.mul_(20.0)
    return model.eval()


def _prompt():
    return torch.randint(0, 128, (2, T0), generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("kind", ["rope", "learned"])
def test_generate_on_a_ring_equals_the_flat_cache(kind):
    model, idx = _model(kind), _prompt()
    # step by step on both caches, the flat cache's greedy tokens fed to both: the logits at every step
    flat = model.new_cache(2, T0 + NEW)
    ring = model.new_cache(2, 512, ring=True)
    assert ring.ring and ring.capacity == 512 and ring.nbytes < flat.nbytes
    lf = model.extend(idx, flat, last_only=True, chunk=17)
    lr = model.extend(idx, ring, last_only=True, chunk=17)
    margin = []
    for _ in range(NEW):
        assert torch.allclose(lr, lf, atol=1e-4), (ring.lens.tolist(), (lr - lf).abs().max().item())
        top = lf.topk(2, -1).values
        margin.append((top[:, 0] - top[:, 1]).min().item())
        tok = lf.argmax(-1)
        lf, lr = model.decode_step(tok, flat), model.decode_step(tok, ring)
    assert ring.lens.tolist() == [T0 + NEW] * 2 and flat.lens.tolist() == [T0 + NEW] * 2
    # generate: the same tokens up to the first step at which the two caches' logits could pick differently
    a = model.generate(idx, NEW, prefill_chunk=17)
    r = model.generate(idx, NEW, prefill_chunk=17, ring=True)
    assert r.shape == a.shape == (2, T0 + NEW)
    sure = next((i for i, m in enumerate(margin) if m <= 2e-4), NEW)
    assert sure > 0 and torch.equal(r[:, :T0 + sure], a[:, :T0 + sure])
    assert torch.equal(model.generate(idx, 8, ring=True), a[:, :T0 + 8]) or sure < 8  # the default chunk of 256


@pytest.mark.parametrize("draft_window", [W_MODEL, None])
def test_draft_and_verify_on_a_ring_equals_the_flat_cache(draft_window):
    model, draft = _model("rope"), _model("learned", window=draft_window, n_layers=1)
    idx = _prompt()[:1]
    a, sa = model.generate(idx, NEW, draft=draft, lookahead=3, return_stats=True)
    r, sr = model.generate(idx, NEW, draft=draft, lookahead=3, return_stats=True, ring=True, prefill_chunk=17)
    assert r.shape == a.shape == (1, T0 + NEW)
    # the trusted prefix comes from the flat cache alone: the target's greedy tokens step by step on a flat cache, up to
    # the first step whose top-2 logit margin is within reach of the paths' fp32 differences (2e-4, twice the bound)
    flat = model.new_cache(1, T0 + NEW)
    logits, greedy, sure = model.extend(idx, flat, last_only=True, chunk=17), [], None
    for i in range(NEW):
        top = logits.topk(2, -1).values
        if sure is None and (top[:, 0] - top[:, 1]).min().item() <= 2e-4:
            sure = i
        greedy.append(logits.argmax(-1))
        logits = model.decode_step(greedy[-1], flat)
    sure = NEW if sure is None else sure
    want = torch.cat([idx, torch.stack(greedy, 1)], 1)
    assert sure >= NEW // 2, sure  # the models' margins are wide: most of the run is trusted
    # draft-and-verify emits the target's greedy tokens: both caches, over the whole trusted prefix
    assert torch.equal(a[:, :T0 + sure], want[:, :T0 + sure])
    assert torch.equal(r[:, :T0 + sure], want[:, :T0 + sure])
    if sure == NEW:
        assert sr == sa


def test_model_ring_errors():
    model = _model("rope")
    with pytest.raises(ValueError):
        _model("rope", window=None).new_cache(1, 256, ring=True)  # ring=True without cfg.window
    with pytest.raises(ValueError):
        _model("rope", window=None).generate(_prompt(), 4, ring=True)
    with pytest.raises(ValueError):
        model.new_cache(1, 300, ring=True)  # not a multiple of 256
    ring = model.new_cache(2, 256, ring=True)  # the capacity need not reach max_seq, nor the prompt
    with pytest.raises(ValueError, match="chunk"):
        model.prefill(_prompt(), ring)  # 40 + 300 - 1 > 256: names extend(chunk=)
    model.prefill(_prompt()[:, :217], ring)  # 40 + 217 - 1 == 256
    assert ring.lens.tolist() == [217, 217]
    with pytest.raises(ValueError):
        model.extend(_prompt(), ring, chunk=218)  # a step of 218 does not fit the ring
    model.extend(_prompt(), ring, last_only=True, chunk=217)
    ring.set_lens([1024, 1024])
    with pytest.raises(ValueError, match="max_seq"):
        model.decode_step(torch.zeros(2, dtype=torch.long), ring)  # positions are still bounded by max_seq
