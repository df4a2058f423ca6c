"""Packed documents on the torch path (the rule: ops/attention.py): doc_bounds, the mask, the position restart."""
import pytest
import torch


def test_doc_bounds_of_a_hand_written_row():
    from kubeflow_rm_amd import ops
    ids = torch.tensor([[7, 7, 7, 2, 9, 9, 9, 9], [4, 4, 4, 4, 4, 4, 4, 5]])
    start, end = ops.doc_bounds(ids)
    assert start.dtype == end.dtype == torch.int32
    assert start.tolist() == [[0, 0, 0, 3, 4, 4, 4, 4], [0, 0, 0, 0, 0, 0, 0, 7]]
    assert end.tolist() == [[3, 3, 3, 4, 8, 8, 8, 8], [7, 7, 7, 7, 7, 7, 7, 8]]


def test_torch_path_is_causal_attention_per_document():
    from kubeflow_rm_amd import ops
    torch.manual_seed(0)
    q, k, v = (torch.randn(2, 3, 20, 16) for _ in range(3))
    cuts = [0, 5, 6, 20]
    ids = torch.bucketize(torch.arange(20), torch.tensor(cuts[1:]), right=True).expand(2, 20)
    o = ops.flash_attention(q, k, v, doc_start=ops.doc_bounds(ids)[0])
    want = torch.cat([torch.nn.functional.scaled_dot_product_attention(q[:, :, a:b], k[:, :, a:b], v[:, :, a:b],
                                                                       is_causal=True) for a, b in zip(cuts, cuts[1:])], 2)
    assert torch.allclose(o, want, atol=1e-5)


def test_model_document_in_a_packed_row_equals_the_document_alone():
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT, GPTConfig
    model = GPT(GPTConfig(vocab_size=64, d_model=32, n_layers=2, n_heads=2, d_ff=64, max_seq=32, dtype=torch.float32))
    torch.manual_seed(0)
    idx = torch.randint(0, 64, (1, 24))
    ids = (torch.arange(24) >= 9).long()[None]
    with torch.no_grad():
        packed = model(idx, doc_start=ops.doc_bounds(ids)[0])
        alone = model(idx[:, 9:])
    assert torch.allclose(packed[:, 9:], alone, atol=1e-5)


def test_doc_start_needs_causal():
    from kubeflow_rm_amd import ops
    q = torch.randn(1, 1, 8, 16)
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, causal=False, doc_start=torch.zeros(1, 8, dtype=torch.int32))
