#!/usr/bin/env python3
"""Flash attention over packed documents (``doc_start=``) against the plain causal kernels and the torch path
(profiles/flash_docs).

All forms run in ONE process, interleaved block by block; medians of ``--blocks`` blocks with min / max.

  kernels  forward and backward per shape and layout: n equal documents per row (n = 1, 2, 8, 32) and one ragged
           layout. "causal": the ``doc_start=None`` call (documents leak). "doc": the DOC kernels. "torch": SDPA in
           bf16 under the dense boolean mask of the rule (the mask built outside the timed region), its backward by
           autograd (``torch_bwd`` is the backward alone).
  model    one training step (forward + backward) of a gpt-1b-sized model on a packed 4 x 2048 batch, native against
           ``ops.torch_reference()``.

One JSON line per row on stdout.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.flash_gqa_bench import time_blocks, verdict  # noqa: E402

KERNEL_SHAPES = [(4, 16, 2048, 128), (16, 12, 2048, 64)]  # gpt-1b, gpt-small attention: B, H, T, D
RAGGED = [0, 37, 300, 301, 1100, 1950]                    # document starts of the ragged layout, every row


def layouts(T: int) -> dict:
    out = {f"n{n}": [i * (T // n) for i in range(n)] for n in (1, 2, 8, 32)}
    out["ragged"] = RAGGED
    return out


def doc_start_of(B: int, T: int, starts, dev):
    import torch
    from kubeflow_rm_amd import ops
    ids = torch.zeros(B, T, dtype=torch.int64)
    for s in starts[1:]:
        ids[:, s:] += 1
    return ops.doc_bounds(ids.to(dev))[0]


def kernels(args) -> None:
    import torch
    import torch.nn.functional as F
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import attention as A
    dev = "cuda"
    for (B, H, T, D) in KERNEL_SHAPES:
        torch.manual_seed(0)
        qkv = torch.randn(B, T, 3 * H * D, device=dev).to(torch.bfloat16)
        q, k, v = A._qkv_views(qkv, H, H, D)
        do = A._bhtd(torch.randn(B, T, H, D, device=dev).to(torch.bfloat16))
        scale = 1.0 / math.sqrt(D)
        o, dq, dk, dv = (A._bhtd(torch.empty(B, T, H, D, device=dev, dtype=torch.bfloat16)) for _ in range(4))
        lse = A._fwd(q, k, v, o, True, scale)
        base = {"fwd": lambda: A._fwd(q, k, v, o, True, scale),
                "bwd": lambda: A._bwd(q, k, v, o, do, lse, dq, dk, dv, True, scale)}
        for name, starts in layouts(T).items():
            ds = doc_start_of(B, T, starts, dev)
            doc = (ds, A._doc_end(ds))
            od = A._bhtd(torch.empty(B, T, H, D, device=dev, dtype=torch.bfloat16))
            lsed = A._fwd(q, k, v, od, True, scale, ds)
            mask = ops.doc_mask(ds)
            qt, kt, vt = (x.detach().clone().requires_grad_(True) for x in (q, k, v))

            def torch_fwd_bwd():
                F.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask).backward(do)
                qt.grad = kt.grad = vt.grad = None
            with torch.no_grad():
                r = time_blocks({"causal_fwd": base["fwd"], "causal_bwd": base["bwd"],
                                 "doc_fwd": lambda: A._fwd(q, k, v, od, True, scale, ds),
                                 "doc_bwd": lambda: A._bwd(q, k, v, od, do, lsed, dq, dk, dv, True, scale, doc=doc),
                                 "torch_fwd": lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask)},
                                args.blocks, args.iters)
            r.update(time_blocks({"torch_fwd_bwd": torch_fwd_bwd}, args.blocks, max(1, args.iters // 4)))
            print(json.dumps({"step": "kernels", "B": B, "H": H, "T": T, "D": D, "layout": name, "docs": len(starts), **r,
                              "torch_bwd_median_us": round(r["torch_fwd_bwd"]["median_us"] - r["torch_fwd"]["median_us"], 1),
                              "doc_vs_causal_fwd": verdict(r["doc_fwd"], r["causal_fwd"]),
                              "doc_vs_causal_bwd": verdict(r["doc_bwd"], r["causal_bwd"]),
                              "doc_vs_torch_fwd": verdict(r["doc_fwd"], r["torch_fwd"])}), flush=True)


def model(args) -> None:
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT, GPTConfig
    cfg = GPTConfig(vocab_size=32000, d_model=2048, n_layers=args.layers, n_heads=16, d_ff=8192, max_seq=2048)
    torch.manual_seed(0)
    m = GPT(cfg, device="cuda")
    B, T = 4, 2048
    idx = torch.randint(0, cfg.vocab_size, (B, T), device="cuda")
    tgt = torch.randint(0, cfg.vocab_size, (B, T), device="cuda")
    ds = doc_start_of(B, T, RAGGED, "cuda")
    tgt[:, [s - 1 for s in RAGGED[1:]] + [T - 1]] = -100

    def step():
        m.zero_grad(set_to_none=True)
        _, loss = m(idx, tgt, doc_start=ds)
        loss.backward()

    def ref():
        with ops.torch_reference():
            step()
    r = time_blocks({"train_native": step, "train_torch_reference": ref}, args.blocks, 1)
    print(json.dumps({"step": "model", "layers": args.layers, "d_model": 2048, "heads": 16, "batch": "4x2048",
                      "docs_per_row": len(RAGGED), **r,
                      "reference_over_native": round(r["train_torch_reference"]["median_us"] / r["train_native"]["median_us"], 3),
                      "native_vs_reference": verdict(r["train_native"], r["train_torch_reference"])}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default="kernels,model")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="calls per block (kernels)")
    ap.add_argument("--layers", type=int, default=24, help="layers of the gpt-1b-sized model")
    args = ap.parse_args()
    for step in args.steps.split(","):
        {"kernels": kernels, "model": model}[step](args)


if __name__ == "__main__":
    main()
