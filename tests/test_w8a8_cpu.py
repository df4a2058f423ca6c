"""The W8A8 rule on the CPU (ops.gemm_nt(variant="w8a8") in torch) and the model's routing rule."""
from __future__ import annotations

import pytest
import torch

from kubeflow_rm_amd import ops
from kubeflow_rm_amd.models import GPT, GPTConfig
from kubeflow_rm_amd.parallel.launch import spawn

FP8 = torch.float8_e4m3fn


def small_model(device=None, **kw):
    """The small test model of tests/test_gpu_w8.py, bf16."""
    cfg = dict(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024, max_seq=256, dtype=torch.bfloat16)
    return GPT(GPTConfig(**{**cfg, **kw}), device=device).eval()


def test_rule_against_explicit_fp64():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(9, 48, generator=g).to(torch.bfloat16)
    qw = ops.quantize_weight(torch.randn(13, 48, generator=g))
    bias = torch.randn(13, generator=g).to(torch.bfloat16)
    res = torch.randn(9, 13, generator=g).to(torch.bfloat16)
    ca, sa = ops.decode.quantize_rows(a)
    z = 0.5 * sa.double()[:, None] * qw.scale.double() * (ca.double() @ qw.codes.double().T) + bias.double()
    want = torch.nn.functional.silu(z) + res.double()
    q = ops.quantize_act(a)
    assert torch.equal(q.scale, sa) and torch.equal(q.codes.view(torch.uint8), ca.view(torch.uint8))
    for x in (a, q):  # a bf16 activation, and one already quantised
        got = ops.gemm_nt(x, qw, variant="w8a8", alpha=0.5, bias=bias, act="silu", residual=res)
        # one bf16 rounding (2^-9 relative) plus the fp32 matmul's error, far below it at K = 48
        assert got.dtype == torch.bfloat16 and (got.double() - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item()


def bad_calls(dev="cpu"):
    """(a, b, keywords, a word of the refusal) of every call the rule refuses."""
    a = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    q = lambda n, k, **kw: ops.quantize_weight(torch.ones(n, k, device=dev), **kw)  # noqa: E731
    w, wide = q(8, 64), q(8, 128)
    return [(a, q(8, 64, dtype="mxfp4"), {}, "MXFP4"), (a.view(1, 4, 64), w, {}, "non-batched"),
            (a, w, {"act": "swiglu"}, "swiglu"),
            (a, ops.QuantizedWeight(wide.codes[:, ::2], wide.scale), {}, "inner stride"),
            (torch.zeros(4, 128, dtype=torch.bfloat16, device=dev)[:, ::2], w, {}, "inner stride"),
            (a[:, :8], q(8, 8), {}, "K >= 16"), (a[:, :24], q(8, 24), {}, "K % 16")]


def test_argument_errors():
    for a, b, kw, why in bad_calls():
        with pytest.raises(ValueError, match=f'w8a8.*{why}'):
            ops.gemm_nt(a, b, variant="w8a8", **kw)


def test_model_routing_and_errors():
    model = small_model()
    W = model.decode_weights()
    idx = torch.randint(0, 512, (2, 40), generator=torch.Generator().manual_seed(0))
    run = lambda i, **kw: model.prefill(i, model.new_cache(2, 64), **kw)  # noqa: E731
    plain = run(idx)
    assert torch.equal(run(idx, weights=W, w8a8=False), plain)
    fp8 = run(idx, weights=W, w8a8=True)  # 80 rows: the FP8 route
    assert not torch.equal(fp8, plain) and (fp8.float() - plain.float()).abs().max().item() < 0.5
    few = idx[:, :8]  # 16 rows <= max(16, stream_rows): the keyword changes nothing
    assert torch.equal(run(few, weights=W, w8a8=True), run(few))
    assert torch.equal(model.extend(few, model.new_cache(2, 64), weights=W, w8a8=True),
                       model.extend(few, model.new_cache(2, 64), weights=W))
    for kw, why in (({"weights": None}, "decode_weights"), ({"weights": model.decode_weights("mxfp4")}, "MXFP4")):
        with pytest.raises(ValueError, match=f"w8a8.*{why}"):
            model.extend(idx, model.new_cache(2, 64), chunk=32, w8a8=True, **kw)
    with pytest.raises(ValueError, match="w8a8"):
        model.generate(idx, 2, w8a8=True)
    assert model.generate(idx, 2, weight_dtype=FP8, w8a8=True).shape == (2, 42)


def _tp_worker(rank):
    import torch.distributed as dist
    from kubeflow_rm_amd import parallel
    parallel.init(backend="gloo")
    model = GPT(GPTConfig(vocab_size=64, d_model=32, n_layers=1, n_heads=2, d_ff=64, max_seq=64,
                          dtype=torch.bfloat16), tp_group=dist.group.WORLD).eval()
    W, idx, refused = model.decode_weights(), torch.randint(0, 64, (1, 24)), []
    for call in (lambda: model.prefill(idx, model.new_cache(1, 32), weights=W, w8a8=True),
                 lambda: model.extend(idx, model.new_cache(1, 32), chunk=20, weights=W, w8a8=True),
                 lambda: model.generate(idx, 2, weight_dtype=FP8, w8a8=True)):
        try:
            call()
            refused.append("ran")
        except ValueError as e:
            refused.append(str(e))
    parallel.shutdown()
    return refused


def test_tensor_parallel_group_is_refused():
    assert all("w8a8" in r and "tensor-parallel" in r for refused in spawn(_tp_worker, 2) for r in refused)
