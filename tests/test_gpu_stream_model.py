"""GPT decode steps of 17 .. 128 rows: ``stream_rows`` takes them to the wide weight-streaming GEMM
(ops.gemm_nt(variant="stream")) on the bf16, FP8 or MXFP4 weights; with the default they run the "auto" route."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
B = 20
LINEARS = ("qkv", "proj", "fc1", "fc2")
CONFIGS = {"D64": dict(n_heads=4), "D128": dict(n_heads=2),
           "llama": dict(n_heads=4, norm="rms", mlp="swiglu", pos="rope", n_kv_heads=2, d_ff=352)}
_models: dict = {}


def _model(name):
    """(the bf16 GPU model, an fp32 CPU model holding its parameters), made once per config."""
    from kubeflow_rm_amd.models import GPT, GPTConfig
    if name not in _models:
        kw = {**dict(vocab_size=512, d_model=256, n_layers=2, d_ff=1024, max_seq=256), **CONFIGS[name]}
        gpu = GPT(GPTConfig(**kw), device=DEV).eval()
        ref = GPT(GPTConfig(**kw, dtype=torch.float32)).eval()
        ref.load_state_dict({k: v.float().cpu() for k, v in gpu.state_dict().items()})
        _models[name] = (gpu, ref)
    return _models[name]


def _weights(gpu, fmt):
    return None if fmt is None else gpu.decode_weights("mxfp4" if fmt == "mxfp4" else FP8)


@pytest.mark.parametrize("name,stream_rows,fmt", [(n, r, f) for n in ("D64", "D128") for r in (16, 32)
                                                  for f in (None, "fp8", "mxfp4")]
                         + [("llama", 32, f) for f in (None, "fp8", "mxfp4")])
def test_teacher_forced_wide_decode_matches_fp32_forward(name, stream_rows, fmt):
    """B = 20 rows, teacher-forced, against the fp32 CPU model holding the weights the steps read: the dequantised
    ones when ``weights`` is given and 20 <= stream_rows, else the model's own (then the prompt runs through
    ``prefill``; on quantised weights, which a prefill never reads, every position is a ``decode_step`` from the empty
    cache). The bound is the teacher-forced one of tests/test_gpu_w8.py: per-position max-abs < 0.1."""
    import copy
    gpu, ref = _model(name)
    W = _weights(gpu, fmt)
    quant = W is not None and B <= stream_rows
    T0, T = (0, 8) if quant else (4, 10)
    seq = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(0))
    deq, head = ref, ref.tok
    with torch.no_grad():
        if quant:
            deq, head = copy.deepcopy(ref), W.head.dequantize().cpu()
            for blk, qb in zip(deq.blocks, W.blocks):
                for n in LINEARS:
                    getattr(blk, n).weight.copy_(qb[n].dequantize().cpu())
        x = F.embedding(seq, deq.tok)
        if deq.pos is not None:
            x = x + deq.pos[:T]
        for blk in deq.blocks:
            x = blk(x, deq.rope_table)
        want = deq.ln_f(x) @ head.T
    cache = gpu.new_cache(B, T)
    got = [gpu.prefill(seq[:, :T0].to(DEV), cache).float().cpu().unsqueeze(1)] if T0 else []
    for t in range(T0, T):
        got.append(gpu.decode_step(seq[:, t].to(DEV), cache, weights=W, stream_rows=stream_rows).float().cpu().unsqueeze(1))
    got = torch.cat(got, 1)
    errs = (got - want[:, max(T0 - 1, 0):]).abs().amax(dim=(0, 2))
    print(f"{name} stream_rows={stream_rows} weights={fmt}: per-position max-abs {[round(e, 4) for e in errs.tolist()]}")
    assert errs.max().item() < 0.1, errs.tolist()
    assert cache.lens.tolist() == [T] * B


def test_wide_steps_read_the_quantised_head_only_with_stream_rows():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models.gpt import DecodeWeights
    gpu, _ = _model("D64")
    W = gpu.decode_weights()
    Z = DecodeWeights(W.blocks, ops.QuantizedWeight(torch.zeros_like(W.head.codes.view(torch.uint8)).view(FP8),
                                                    W.head.scale), W._key)
    tok = torch.randint(0, 512, (B,), generator=torch.Generator().manual_seed(1)).to(DEV)
    assert (gpu.decode_step(tok, gpu.new_cache(B, 8), weights=Z, stream_rows=32) == 0).all()
    assert torch.equal(gpu.decode_step(tok, gpu.new_cache(B, 8), weights=Z), gpu.decode_step(tok, gpu.new_cache(B, 8)))


def test_graphed_wide_step_equals_eager():
    gpu, _ = _model("D128")
    W = gpu.decode_weights()
    idx = torch.randint(0, 512, (B, 9), generator=torch.Generator().manual_seed(2)).to(DEV)
    toks = torch.randint(0, 512, (5, B), generator=torch.Generator().manual_seed(3)).to(DEV)
    ce, cg = gpu.new_cache(B, 32), gpu.new_cache(B, 32)
    gpu.prefill(idx, ce), gpu.prefill(idx, cg)
    step = gpu.graphed_decode_step(cg, weights=W, stream_rows=32)
    for t in toks:
        torch.testing.assert_close(step(t), gpu.decode_step(t, ce, weights=W, stream_rows=32), rtol=0, atol=0)


def test_num_samples_on_a_paged_cache_streams_24_rows():
    gpu, _ = _model("D64")
    idx = torch.randint(0, 512, (8, 11), generator=torch.Generator().manual_seed(4)).to(DEV)
    out = gpu.generate(idx, 6, num_samples=3, paged=True, stream_rows=32)
    assert out.shape == (24, 17)
    assert torch.equal(out, gpu.generate(idx.repeat_interleave(3, 0), 6, stream_rows=32))
