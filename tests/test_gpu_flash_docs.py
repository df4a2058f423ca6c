"""Flash attention over packed documents (the DOC kernels of kernels/attention_bf16.hip; the rule: ops/attention.py)
against fp32 SDPA under the rule's boolean mask on the same bf16-rounded inputs. Bounds: test_gpu_attention.py's."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (B, H, Hkv, T, D, document starts per batch row)
CASES = [
    (1, 2, 2, 40, 128, [0, 1, 17]),                                # less than one tile; a one-token document
    (2, 3, 3, 300, 64, [[0, 70, 71, 200], [0, 128, 256]]),         # boundaries inside a tile and on the grid; a wave
    (1, 4, 2, 300, 128, [0, 70, 71, 200]),                         # whose rows start at different tiles; grouped K / V
    (8, 32, 32, 512, 128, [0, 130, 300, 301, 448]),                # attn_fwd_pp, paired blocks
    (2, 64, 64, 700, 128, [0, 130, 300, 301, 448]),                # attn_fwd_pp, an odd block count
]


def _doc_start(B, T, starts):
    from kubeflow_rm_amd import ops
    ids = torch.zeros(B, T, dtype=torch.int64)
    for b, row in enumerate(starts if isinstance(starts[0], list) else [starts] * B):
        for s in row[1:]:
            ids[b, s:] += 1
    return ops.doc_bounds(ids.to(DEV))[0]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the fp32 reference (o, lse, dq, dk, dv) of CASES[i]: computed once, left unchanged."""
    B, H, Hkv, T, D, starts = CASES[i]
    g = torch.Generator(device="cpu").manual_seed(11 * T + D)
    q, do = (torch.randn(B, H, T, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    k, v = (torch.randn(B, Hkv, T, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    ds = _doc_start(B, T, starts)
    return (q, k, v, do, ds) + _ref(q, k, v, do, ds)


def _ref(q, k, v, do, ds):
    from kubeflow_rm_amd import ops
    G = q.shape[1] // k.shape[1]
    qf, kf, vf = (x.float().requires_grad_(True) for x in (q, k, v))
    ke, ve = kf.repeat_interleave(G, 1), vf.repeat_interleave(G, 1)
    mask = ops.doc_mask(ds)
    o = torch.nn.functional.scaled_dot_product_attention(qf, ke, ve, attn_mask=mask)
    o.backward(do.float())
    s = (qf.detach() @ ke.detach().transpose(-1, -2)) / math.sqrt(q.shape[-1])
    lse = torch.logsumexp(s.masked_fill(~mask, float("-inf")), -1)
    return o.detach(), lse, qf.grad, kf.grad, vf.grad


@pytest.mark.parametrize("i", range(len(CASES)))
def test_doc_forward_matches_fp32(i):
    from kubeflow_rm_amd.ops import attention as A
    q, k, v, _, ds, ref, ref_lse = _case(i)[:7]
    B, H, T, D = q.shape
    o = A._bhtd(torch.empty(B, T, H, D, device=DEV, dtype=torch.bfloat16))
    lse = A._fwd(q, k, v, o, True, 1.0 / math.sqrt(D), ds)
    err, rel, lerr = (o.float() - ref).abs().max().item(), _rel(o, ref), (lse - ref_lse).abs().max().item()
    print(f"max-abs {err:.4g} rel {rel:.4g} lse {lerr:.4g}")
    assert err < 2e-2 and rel < 8e-3 and lerr < 1e-3  # (a NaN fails each)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_doc_backward_matches_fp32(i):
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import attention as A
    q, k, v, do, ds, _, _, *want = _case(i)
    qs, ks, vs = (x.clone().requires_grad_(True) for x in (q, k, v))
    o = ops.flash_attention(qs, ks, vs, doc_start=ds)
    o.backward(do)
    runs = [("rule", (qs.grad, ks.grad, vs.grad))]
    G, scale = q.shape[1] // k.shape[1], 1.0 / math.sqrt(q.shape[-1])
    for gs in (1, G) if G > 1 else ():  # grouped K / V: every query head its own workgroup (the reduce path), one sweep
        lse = A._fwd(q, k, v, torch.empty_like(o), True, scale, ds)
        grads = [torch.empty_like(x) for x in (q, k, v)]
        A._bwd(q, k, v, o.detach(), do, lse, *grads, True, scale, group_split=gs, doc=(ds, A._doc_end(ds)))
        runs.append((f"group_split {gs}", grads))
    for what, grads in runs:
        for name, got, ref in zip(("dq", "dk", "dv"), grads, want):
            print(f"{what} {name}: rel {_rel(got, ref):.4g}")
            assert torch.isfinite(got.float()).all(), (what, name)
            assert _rel(got, ref) < 2e-2, (what, name, _rel(got, ref))


def test_doc_rescale_inside_a_late_document():
    """A row's running maximum first moves at a tile that is not the block's first (bound: test_gpu_attention.py's)."""
    from kubeflow_rm_amd import ops
    B, H, T, D = 1, 2, 1000, 128
    g = torch.Generator(device="cpu").manual_seed(3)
    q, k, v = (torch.randn(B, H, T, D, generator=g).to(DEV, torch.bfloat16) for _ in range(3))
    k[:, :, 950] = 4.0
    q[:, :, 990] = 0.5
    ds = _doc_start(B, T, [0, 900])
    o = ops.flash_attention(q, k, v, doc_start=ds)
    ref = _ref(q, k, v, torch.zeros_like(q), ds)[0]
    assert (o.float() - ref).abs().max().item() < 3e-2


@pytest.mark.parametrize("B,H,T,D", [(2, 3, 300, 64), (8, 32, 512, 128)])
def test_one_document_is_the_causal_kernel_bit_for_bit(B, H, T, D):
    from kubeflow_rm_amd.ops import attention as A
    g = torch.Generator(device="cpu").manual_seed(T)
    q, k, v, do = (torch.randn(B, H, T, D, generator=g).to(DEV, torch.bfloat16) for _ in range(4))
    ds = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    outs = []
    for doc in (None, (ds, A._doc_end(ds))):
        o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
        lse = A._fwd(q, k, v, o, True, 1.0 / math.sqrt(D), doc and doc[0])
        A._bwd(q, k, v, o, do, lse, dq, dk, dv, True, 1.0 / math.sqrt(D), doc=doc)
        outs.append((o, lse, dq, dk, dv))
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), *outs):
        assert torch.equal(a, b), name


def test_attention_qkv_doc_matches_view_entry_point():
    from kubeflow_rm_amd import ops
    B, T, h, hd = 2, 256, 3, 64
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(B, T, 3 * h * hd, generator=g).to(DEV, torch.bfloat16).requires_grad_(True)
    dy = torch.randn(B, T, h * hd, generator=g).to(DEV, torch.bfloat16)
    ds = _doc_start(B, T, [[0, 70, 71, 200], [0, 128]])
    y = ops.attention_qkv(qkv, h, hd, doc_start=ds)
    y.backward(dy)
    q, k, v = (t.clone().requires_grad_(True) for t in qkv.detach().view(B, T, 3, h, hd).permute(2, 0, 3, 1, 4))
    o = ops.flash_attention(q, k, v, doc_start=ds)
    o.backward(dy.view(B, T, h, hd).permute(0, 2, 1, 3))
    assert torch.equal(y.view(B, T, h, hd).permute(0, 2, 1, 3), o)
    want = torch.stack([q.grad, k.grad, v.grad], 0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * h * hd)
    assert torch.equal(qkv.grad, want)


def test_gpt_packed_row_matches_reference_and_the_document_alone():
    """A packed row [docA | docB], native against ops.torch_reference() (test_gpu_models.py's bounds), and docB's logits
    against the model on docB alone: positions restart and nothing leaks."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT, GPTConfig
    cfg = GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024, max_seq=128)
    torch.manual_seed(0)
    model = GPT(cfg, device=DEV)
    la, lb = 37, 91
    idx = torch.randint(0, 512, (1, la + lb), device=DEV)
    tgt = torch.randint(0, 512, (1, la + lb), device=DEV)
    tgt[0, la - 1] = tgt[0, -1] = -100
    ds = _doc_start(1, la + lb, [0, la])
    logits, loss = model(idx, tgt, doc_start=ds)
    loss.backward()
    g_native = model.blocks[0].qkv.weight.grad.clone()
    model.zero_grad(set_to_none=True)
    with ops.torch_reference():
        ref_logits, ref_loss = model(idx, tgt, doc_start=ds)
        ref_loss.backward()
    alone = model(idx[:, la:]).detach()
    bound = lambda ref: 5e-2 * ref.float().abs().max().item() + 5e-2  # noqa: E731
    assert abs(loss.item() - ref_loss.item()) < 2e-2 * abs(ref_loss.item())
    assert (logits.float() - ref_logits.float()).abs().max().item() < bound(ref_logits)
    assert (logits[:, la:].float() - alone.float()).abs().max().item() < bound(alone)
    assert _rel(g_native, model.blocks[0].qkv.weight.grad) < 5e-2  # as test_gpt_attention_runs_on_the_flash_kernel
