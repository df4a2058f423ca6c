"""attention_decode is attention_extend with one query row: the single-row kernel and its combine
(attn_decode_split, attn_decode_combine in kernels/attn_kv.hip) do what attn_extend_split at R = 1, Tq = 1,
row0 = 0 and attn_kv_combine do, operation for operation, so o and lse of the two calls are equal bit for
bit: for both cache dtypes, at the split edges, with a tight and a capacity-sized grid, and with the rows
beyond lens poisoned.

The two calls run different kernels. The test keeps them from drifting apart (a fix to the key-validity rule
or to a merge made in one body and not in the other); the property already held between the kernels that
attn_kv.hip replaced."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
B, H = 2, 3


def _randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _cache(D, dtype, cap, lens, poison):
    """A cache of seeded rows (an FP8 one holds quantize_rows of them); with ``poison`` the rows at or
    beyond lens[b] hold NaN (bf16), or code 0x7F and NaN scales (FP8)."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    c = ops.KVCache(1, B, H, D, cap, device=DEV, dtype=dtype)
    for i, (t, sc) in enumerate(((c.k[0], c.k_scale), (c.v[0], c.v_scale))):
        rows = _randn(B, H, cap, D, seed=200 + D + i)
        if dtype == FP8:
            codes, scale = decode.quantize_rows(rows.cpu())
            t.view(torch.uint8).copy_(codes.view(torch.uint8))
            sc[0].copy_(scale)
        else:
            t.copy_(rows)
        if poison:
            for b, n in enumerate(lens):
                if dtype == FP8:
                    t.view(torch.uint8)[b, :, n:] = 0x7F
                    sc[0][b, :, n:] = float("nan")
                else:
                    t[b, :, n:] = float("nan")
    c.set_lens(lens)
    return c


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
def test_decode_is_extend_with_one_row_bit_for_bit(dtype, D, poison):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    S = decode.SPLIT_KEYS
    cap = 3 * S
    q = _randn(B, H, D, seed=D)
    for lens in ((0, 1), (S - 1, S), (S + 1, 2 * S + 3)):
        cache = _cache(D, dtype, cap, list(lens), poison)
        for t_bound in (max(lens), cap):  # the tight grid, and one with empty trailing splits
            o1, lse1 = ops.attention_decode(q, cache, 0, t_bound=t_bound, return_lse=True)
            o2, lse2 = ops.attention_extend(q.unsqueeze(1), cache, 0, t_bound=t_bound, return_lse=True)
            what = f"lens={lens} t_bound={t_bound}"
            assert o2.shape == (B, 1, H, D) and lse2.shape == (B, 1, H), what
            assert torch.equal(o1, o2[:, 0]), what
            assert torch.equal(lse1, lse2[:, 0]), what
            for b, n in enumerate(lens):  # and it is a result: finite where a key exists, 0 / -inf where none does
                if n == 0:
                    assert (o1[b] == 0).all() and (lse1[b] == float("-inf")).all(), what
                else:
                    assert torch.isfinite(o1[b].float()).all() and torch.isfinite(lse1[b]).all(), what
