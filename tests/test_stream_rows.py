"""The weight a cached step reads, by its row count and ``stream_rows`` (the rule in GPT.extend's docstring)."""
import pytest
import torch

from kubeflow_rm_amd.models import GPT, GPTConfig


def test_stream_rows_moves_the_quantised_weight_cut_over():
    m = GPT(GPTConfig(vocab_size=64, d_model=32, n_layers=1, n_heads=2, d_ff=64, max_seq=16, dtype=torch.float32)).eval()
    W, own = m.decode_weights(), m.blocks[0].qkv.weight
    for rows, sr, quant in ((16, 16, True), (17, 16, False), (20, 32, True), (33, 32, False), (128, 128, True)):
        assert (m._weight_selector(W, rows, sr)(0, "qkv") is W.blocks[0]["qkv"]) == quant
        assert (m._head_weight(W, rows, sr) is W.head) == quant
    assert m._weight_selector(None, 20, 32)(0, "qkv") is own and m._weight_selector(W, 20)(0, "qkv") is own
    tok = torch.zeros(20, dtype=torch.long)
    for bad in (15, 129, True, 32.0):
        with pytest.raises(ValueError):
            m.decode_step(tok, m.new_cache(20, 4), stream_rows=bad)
    wide = m.decode_step(tok, m.new_cache(20, 4), weights=W, stream_rows=32)  # the torch path follows the rule
    assert not torch.equal(wide, m.decode_step(tok, m.new_cache(20, 4), weights=W))
