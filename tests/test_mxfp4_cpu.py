"""MXFP4 decode weights on the torch path: the MXFP4Weight format and the OCP MX v1.0 quantiser
(ops.quantize_weight(dtype="mxfp4")), and CPU generation on GPT.decode_weights("mxfp4")."""
import pytest
import torch

MAGS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _value(code):
    return torch.where(code >= 8, -MAGS[code & 7], MAGS[code & 7])


def _pack(code):
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)


def test_every_code_round_trips_under_several_scales():
    """Every group holds the 16 codes twice, rotated by group so that each code meets each nibble position; the
    scale bytes vary across groups and rows. e = 252 is the largest scale a finite fp32 group can produce (amax <
    2^128), so the round trip stops there; e = 254 is checked through dequantize() alone."""
    from kubeflow_rm_amd import ops
    scales = torch.tensor([[1, 127, 252, 100], [130, 2, 64, 200], [127, 251, 1, 90]], dtype=torch.uint8)
    N, G = scales.shape
    code = torch.stack([torch.stack([(torch.arange(32) + 3 * g + n) % 16 for g in range(G)]).reshape(-1)
                        for n in range(N)])
    want = (_value(code).view(N, G, 32) * torch.exp2(scales.float() - 127).unsqueeze(-1)).view(N, G * 32)
    qw = ops.MXFP4Weight(_pack(code), scales)
    assert qw.shape == (N, G * 32) and qw.nbytes == N * G * 16 + N * G and qw.device == scales.device
    deq = qw.dequantize()
    assert deq.dtype == torch.float32 and torch.equal(deq, want) and (deq.abs() == 2.0 ** -127).any()
    assert torch.equal(torch.signbit(deq), code >= 8)  # -0 is a code of its own
    back = ops.quantize_weight(want, dtype="mxfp4")
    assert isinstance(back, ops.MXFP4Weight)
    assert torch.equal(back.codes, qw.codes) and torch.equal(back.scales, scales)
    assert torch.equal(back.dequantize().view(torch.int32), want.view(torch.int32))
    # the float4 / e8m0 dtypes are views of the same bytes, and torch.float4_e2m1fn_x2 is the same request
    same = ops.MXFP4Weight(qw.codes.view(torch.float4_e2m1fn_x2), scales.view(torch.float8_e8m0fnu))
    assert torch.equal(same.dequantize(), want)
    assert torch.equal(ops.quantize_weight(want, dtype=torch.float4_e2m1fn_x2).codes, qw.codes)
    top = ops.MXFP4Weight(_pack(torch.tensor([[1, 2, 3, 11] * 8])), torch.tensor([[254]], dtype=torch.uint8))
    assert torch.equal(top.dequantize(), torch.tensor([[0.5, 1.0, 1.5, -1.5] * 8]) * 2.0 ** 127)


def test_ties_saturation_zero_group_and_negative_zero():
    from kubeflow_rm_amd import ops
    w = torch.zeros(3, 64)
    # group 0 of row 0: amax 6 -> e = 127; the seven ties and their negatives
    w[0, :16] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0,
                              -0.0])
    w[0, 32:34] = torch.tensor([7.9, 1.0])        # amax in (6, 8): e = 127, clamps to 6
    w[1, :32] = -0.0                              # a zero group: e = 127, the sign kept
    w[2, :3] = torch.tensor([7.9, 1.0, -5.1]) * 2.0 ** -10
    qw = ops.quantize_weight(w, dtype="mxfp4")
    assert qw.scales.tolist() == [[127, 127], [127, 127], [117, 127]]
    deq = qw.dequantize()
    assert deq[0, :16].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0,
                                    -0.0]
    assert torch.signbit(deq[0, 8:16]).all() and deq[0, 32:34].tolist() == [6.0, 1.0]
    assert (qw.codes[1, :16] == 0x88).all() and (qw.codes[1, 16:] == 0).all()
    assert (deq[2, :3] * 2.0 ** 10).tolist() == [6.0, 1.0, -6.0]


def test_default_is_unchanged_and_contract_violations_raise():
    from kubeflow_rm_amd import ops
    w = torch.randn(8, 48, generator=torch.Generator().manual_seed(0))
    codes, scale = ops.decode.quantize_rows(w)
    for qw in (ops.quantize_weight(w), ops.quantize_weight(w, dtype=torch.float8_e4m3fn)):
        assert isinstance(qw, ops.QuantizedWeight)
        assert torch.equal(qw.codes.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(qw.scale, scale)
    u8 = torch.uint8
    for bad in (lambda: ops.quantize_weight(w, dtype="mxfp4"),                       # K % 32
                lambda: ops.quantize_weight(w, dtype=torch.int8),
                lambda: ops.quantize_weight(torch.zeros(64), dtype="mxfp4"),
                lambda: ops.MXFP4Weight(torch.zeros(4, 24, dtype=u8), torch.zeros(4, 1, dtype=u8)),   # K = 48
                lambda: ops.MXFP4Weight(torch.zeros(4, 16, dtype=u8), torch.zeros(4, 2, dtype=u8)),   # scale shape
                lambda: ops.MXFP4Weight(torch.zeros(4, 16, dtype=u8), torch.zeros(4, 1)),             # scale dtype
                lambda: ops.MXFP4Weight(torch.zeros(4, 16), torch.zeros(4, 1, dtype=u8)),             # code dtype
                lambda: ops.MXFP4Weight(torch.zeros(64, dtype=u8), torch.zeros(4, 1, dtype=u8))):
        with pytest.raises(ValueError):
            bad()


def test_cpu_generation_on_mxfp4_weights_equals_the_dequantised_model():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT, GPTConfig
    from kubeflow_rm_amd.models.gpt import DecodeWeights
    cfg = GPTConfig(vocab_size=128, d_model=64, n_layers=2, n_heads=4, d_ff=128, max_seq=64, dtype=torch.float32)
    model = GPT(cfg).eval()
    W = model.decode_weights("mxfp4")
    assert model.decode_weights(torch.float4_e2m1fn_x2) is W and W.unquantized == []
    W8 = model.decode_weights()                                    # the other format's memo is its own
    assert isinstance(W8.head, ops.QuantizedWeight) and model.decode_weights("mxfp4") is W
    assert model.decode_weights() is W8 and all(isinstance(q, ops.MXFP4Weight) for q in W.matrices())
    assert W.nbytes == sum(q.shape[0] * q.shape[1] * 17 // 32 for q in W.matrices())
    # the same model, every linear and the tied head replaced by the plain dequantised tensor
    plain = DecodeWeights([{n: q.dequantize() for n, q in b.items()} for b in W.blocks], W.head.dequantize(), W._key)
    idx = torch.randint(0, 128, (2, 9), generator=torch.Generator().manual_seed(3))
    cache = model.new_cache(2, 19)
    toks = [idx, model.prefill(idx, cache).argmax(-1).view(-1, 1)]  # the prompt reads the original weights
    for _ in range(9):
        toks.append(model.decode_step(toks[-1].view(-1), cache, weights=plain).argmax(-1).view(-1, 1))
    assert torch.equal(model.generate(idx, 10, weight_dtype="mxfp4"), torch.cat(toks, 1))
