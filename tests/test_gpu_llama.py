"""GPTConfig(norm="rms", mlp="swiglu", pos="rope") on the GPU: training forward / backward against an fp32 CPU copy,
every KV-cache path against the fp32 full forward (bf16 and FP8 cache + FP8 weights), graphs and generate."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _cfg(n_kv, dtype):
    from kubeflow_rm_amd.models import GPTConfig
    return GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=344, max_seq=256, dtype=dtype,
                     n_kv_heads=n_kv, pos="rope", norm="rms", mlp="swiglu")


KV = [None, 2]
IDS = ["mha", "gqa2"]


@pytest.mark.parametrize("n_kv", KV, ids=IDS)
def test_llama_forward_backward_matches_fp32_reference(n_kv):
    """test_rotary_gpt_forward_backward_matches_fp32_reference's check and bounds, plus fc1's gradient (the gate's
    backward kernel) and ln_f's (the RMSNorm backward without a residual)."""
    from kubeflow_rm_amd.models import GPT
    torch.manual_seed(0)
    idx = torch.randint(0, 512, (2, 128))
    tgt = torch.randint(0, 512, (2, 128))
    gpu = GPT(_cfg(n_kv, torch.bfloat16), device=DEV)
    keys = list(gpu.state_dict())
    assert "pos" not in keys and not [k for k in keys if k.endswith("ln1.bias") or k.endswith("ln2.bias")]
    assert "ln_f.bias" not in keys and gpu.blocks[0].fc1.weight.shape == (688, 256)
    logits, loss = gpu(idx.cuda(), tgt.cuda())
    loss.backward()
    ref = GPT(_cfg(n_kv, torch.float32))
    rlogits, rloss = ref(idx, tgt)
    rloss.backward()
    err = (logits.float().cpu() - rlogits.detach()).abs().max().item()
    print(f"llama gpt: loss {loss.item():.4f} / {rloss.item():.4f}, logits max-abs {err:.4f}")
    assert abs(loss.item() - rloss.item()) < 2e-2 * abs(rloss.item())
    assert err < 0.1, err
    for name in ("ln1.weight", "qkv.weight", "ln2.weight", "fc1.weight"):
        g = gpu.blocks[0].get_parameter(name).grad.float().cpu()
        r = ref.blocks[0].get_parameter(name).grad
        worst = ((g - r).abs().max() / r.abs().max()).item()
        print(f"  blocks[0].{name}.grad: max-abs error / max |reference| {worst:.4f}")
        assert torch.allclose(g, r, atol=5e-2 * r.abs().max().item() + 1e-3), name
    g, r = gpu.ln_f.weight.grad.float().cpu(), ref.ln_f.weight.grad
    assert torch.allclose(g, r, atol=5e-2 * r.abs().max().item() + 1e-3)


@pytest.fixture(scope="module", params=KV, ids=IDS)
def models(request):
    from kubeflow_rm_amd.models import GPT
    return (GPT(_cfg(request.param, torch.bfloat16), device=DEV).eval(),
            GPT(_cfg(request.param, torch.float32)).eval())


def _teacher_forced(model, seq, T0, kv_dtype=None, weights=None):
    """prefill(T0) + 4 decode steps + extend(T = 5) + extend(40 tokens, chunk=32): logits from row T0 - 1 on. With
    B = 2 the decode steps (2 rows) and the T = 5 extend (10 rows) take the weight-streaming route, i.e. the gated
    GEMM (and ``weights``); the prefill and the chunked extend (64 rows) take GEMM + the gate kernel."""
    dev = model.tok.device
    Bm, total = seq.shape
    cache = model.new_cache(Bm, total, kv_dtype=kv_dtype)
    got, at = [model.prefill(seq[:, :T0].to(dev), cache).view(Bm, 1, -1)], T0
    for _ in range(4):
        got.append(model.decode_step(seq[:, at].to(dev), cache, weights=weights).view(Bm, 1, -1))
        at += 1
    got.append(model.extend(seq[:, at:at + 5].to(dev), cache, weights=weights))
    got.append(model.extend(seq[:, at + 5:].to(dev), cache, chunk=32, weights=weights))
    assert cache.lens.tolist() == [total] * Bm
    return torch.cat(got, 1).float().cpu()


def test_llama_cache_paths_match_the_fp32_full_forward(models):
    gpu, ref = models
    Bm, T0 = 2, 40
    seq = torch.randint(0, 512, (Bm, T0 + 4 + 5 + 40), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = ref(seq)[:, T0 - 1:]
        plain = _teacher_forced(ref, seq, T0)
    assert (plain - want).abs().max().item() < 1e-3  # the fp32 model's own cache paths
    errs = (_teacher_forced(gpu, seq, T0) - want).abs().amax(dim=(0, 2))
    print(f"llama cache paths, per-position max-abs: max {errs.max().item():.4f}")
    assert errs.max().item() < 0.1, errs.tolist()
    # FP8 cache and FP8 weights: 0.1 + 2 E_q, E_q the fp32 model's own error on the same quantised cache and weights
    # over the same sequence of steps (tests/test_gpu_rope.py / test_gpu_kv_fp8.py apply the allowance this way)
    with torch.no_grad():
        e_q = (_teacher_forced(ref, seq, T0, kv_dtype=FP8, weights=ref.decode_weights()) - plain).abs().max().item()
    errs8 = (_teacher_forced(gpu, seq, T0, kv_dtype=FP8, weights=gpu.decode_weights()) - want).abs().amax(dim=(0, 2))
    print(f"llama fp8 cache + weights per-position max-abs: max {errs8.max().item():.4f}, E_q {e_q:.4f}")
    assert e_q > 0 and errs8.max().item() < 0.1 + 2 * e_q, (errs8.tolist(), e_q)


def _hand_loop(model, idx, new, weights=None, kv_dtype=None):
    cache = model.new_cache(idx.shape[0], idx.shape[1] + new, kv_dtype=kv_dtype)
    logits = [model.prefill(idx, cache).clone()]
    toks = [idx, logits[0].argmax(-1).view(-1, 1)]
    for _ in range(new - 1):
        logits.append(model.decode_step(toks[-1].view(-1), cache, weights=weights).clone())
        toks.append(logits[-1].argmax(-1).view(-1, 1))
    return torch.cat(toks, 1), logits


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_llama_graphed_decode_step_equals_eager(models, fp8):
    gpu, _ = models
    Bm, T0, new = 2, 21, 8
    W = gpu.decode_weights() if fp8 else None
    kvd = FP8 if fp8 else None
    idx = torch.randint(0, 512, (Bm, T0), generator=torch.Generator().manual_seed(2)).to(DEV)
    want_toks, want_logits = _hand_loop(gpu, idx, new, W, kvd)
    cache = gpu.new_cache(Bm, 64, kv_dtype=kvd)
    logits = gpu.prefill(idx, cache)
    step = gpu.graphed_decode_step(cache, weights=W)
    toks = [idx]
    for i in range(new):
        torch.testing.assert_close(logits, want_logits[i], rtol=0, atol=0)
        toks.append(logits.argmax(-1).view(-1, 1))
        if i + 1 < new:
            logits = step(toks[-1].view(-1))
    assert torch.equal(torch.cat(toks, 1), want_toks)


def test_llama_generate_graph_fused_sampler_fp8(models):
    gpu, _ = models
    idx = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    eager = gpu.generate(idx, 8)
    assert torch.equal(eager, _hand_loop(gpu, idx, 8)[0]) and torch.equal(gpu.generate(idx, 8, graph=True), eager)
    kw = dict(sampler="fused", temperature=0.8, top_k=20, top_p=0.9, kv_dtype=FP8, weight_dtype=FP8)
    a = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), graph=True, **kw)
    b = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), **kw)
    assert a.shape == (2, 20) and torch.equal(a, b) and torch.equal(a[:, :12], idx)
    c = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), graph=True, prefill_chunk=17, **kw)
    d = gpu.generate(idx, 8, generator=torch.Generator().manual_seed(3), prefill_chunk=17, **kw)
    assert torch.equal(c, d)
    # draft-and-verify: a self-draft accepts every proposal
    one = idx[:1]
    out, stats = gpu.generate(one, 12, draft=gpu, lookahead=4, return_stats=True)
    assert stats["accepted"] == stats["proposed"] and torch.equal(out, gpu.generate(one, 12))


def test_llama_steps_launch_the_gated_gemm(models, monkeypatch):
    """A decode step (B <= 16 rows) calls gemm_nt(act="swiglu") once per layer and never the gate kernel; a step of
    more rows runs the ungated GEMM and ops.swiglu."""
    from kubeflow_rm_amd import ops
    gpu, _ = models
    calls = {"glu": 0, "gate": 0}
    real_gemm, real_gate = ops.gemm_nt, ops.swiglu

    def gemm(*a, **kw):
        calls["glu"] += kw.get("act") == "swiglu"
        return real_gemm(*a, **kw)

    def gate(z):
        calls["gate"] += 1
        return real_gate(z)

    monkeypatch.setattr(ops, "gemm_nt", gemm)
    monkeypatch.setattr(ops, "swiglu", gate)
    cache = gpu.new_cache(2, 64)
    tok = torch.randint(0, 512, (2,), generator=torch.Generator().manual_seed(4)).to(DEV)
    gpu.decode_step(tok, cache)
    assert calls == {"glu": 2, "gate": 0}
    gpu.extend(tok.view(2, 1).repeat(1, 20), cache, chunk=20)  # 40 rows
    assert calls == {"glu": 2, "gate": 2}


@pytest.mark.parametrize("mlp", ["gelu", "swiglu"])
def test_short_prefill_keeps_the_auto_route(mlp, monkeypatch):
    """``prefill`` runs every linear on the "auto" GEMM route whatever the prompt's length: a prompt of 16 rows or
    fewer does not switch fc1 (or anything else) to the weight-streaming kernel, so the default model's prefill
    launches what it always did. The gated one-launch form belongs to decode_step / extend."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT, GPTConfig
    kw = dict(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=344 if mlp == "swiglu" else 1024, max_seq=64,
              mlp=mlp, norm="rms" if mlp == "swiglu" else "layer")
    model = GPT(GPTConfig(**kw), device=DEV).eval()
    seen, real = [], ops.gemm_nt

    def spy(*a, **kw):
        seen.append((kw.get("variant", "auto"), kw.get("act", "none")))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "gemm_nt", spy)
    idx = torch.randint(0, 512, (2, 8), generator=torch.Generator().manual_seed(5)).to(DEV)
    logits = model.prefill(idx, model.new_cache(2, 16))
    assert len(seen) == 2 * 4 + 1 and {v for v, _ in seen} == {"auto"} and "swiglu" not in {a for _, a in seen}
    with torch.no_grad():  # the bound of the cache-path tests above: the fp32 full forward within 0.1
        want = GPT(GPTConfig(**kw, dtype=torch.float32)).eval()(idx.cpu())[:, -1]
    assert (logits.float().cpu() - want).abs().max().item() < 0.1
