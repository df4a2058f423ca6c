"""GPT prompt and chunk steps on the dense FP8 GEMM (w8a8=True) against the same calls on a CPU copy of the model,
which computes the W8A8 rule in torch on the SAME codes."""
from __future__ import annotations

import copy

import pytest
import torch

from tests.test_w8a8_cpu import FP8, small_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 0.1  # tests/test_gpu_w8.py's bound between the native and the torch path for W8A16 logits


@pytest.fixture(scope="module")
def pair():
    """(gpu model, its FP8 weights, cpu copy, the same codes on the CPU)."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models.gpt import DecodeWeights
    gpu = small_model(DEV)
    W = gpu.decode_weights()
    host = lambda q: ops.QuantizedWeight(q.codes.cpu(), q.scale.cpu())  # noqa: E731
    Wc = DecodeWeights([{n: host(q) for n, q in b.items()} for b in W.blocks], host(W.head), W._key)
    return gpu, W, copy.deepcopy(gpu).cpu(), Wc


def _idx(B, T, seed):
    return torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(seed))


def _step(m, step, i, **kw):
    if step == "prefill":
        return m.prefill(i, m.new_cache(2, 128), **kw)
    return m.extend(i, m.new_cache(2, 128), chunk=32, **kw)  # chunks of 32, 32 and 6 tokens: 64, 64 and 12 rows


@pytest.mark.parametrize("step", ["prefill", "extend"])
def test_w8a8_steps_match_the_cpu_rule(pair, step):
    gpu, W, cpu, Wc = pair
    idx = _idx(2, 70, 0)
    got = _step(gpu, step, idx.to(DEV), weights=W, w8a8=True).float().cpu()
    err = (got - _step(cpu, step, idx, weights=Wc, w8a8=True).float()).abs().max().item()
    print(f"w8a8 {step}: GPU vs CPU rule, max-abs logit difference {err:.4f}")
    assert err < TOL, err
    # the FP8 route is really taken (the bf16 route's logits differ by the quantisation); w8a8=False is the model as
    # it was, bit for bit
    plain = _step(gpu, step, idx.to(DEV), **({} if step == "prefill" else {"weights": W}))
    assert not torch.equal(plain.float().cpu(), got)
    assert torch.equal(_step(gpu, step, idx.to(DEV), weights=W, w8a8=False), plain)


@pytest.mark.parametrize("chunk", [None, 32])
def test_generate_w8a8_graphed_is_repeatable(pair, chunk):
    gpu = pair[0]
    idx = _idx(2, 40, 2).to(DEV)
    kw = dict(weight_dtype=FP8, w8a8=True, graph=True, prefill_chunk=chunk)
    out = gpu.generate(idx, 8, **kw)
    assert out.shape == (2, 48) and torch.equal(gpu.generate(idx, 8, **kw), out)
