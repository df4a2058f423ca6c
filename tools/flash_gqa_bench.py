#!/usr/bin/env python3
"""Flash attention on grouped K / V heads against the expand-and-sum form it replaces (profiles/flash_gqa).

Both forms run in ONE process, interleaved block by block; medians of ``--blocks`` blocks with min / max.

  kernels  forward and backward per shape and group size G. "expand": K / V repeated to H heads (a materialised
           copy, part of the forward's time), the ungrouped kernels, dK / dV summed over the group in bf16 (part of
           the backward's time) — what autograd did. "grouped": the kernels on Hkv heads; the backward once per
           ``group_split`` (GS query heads per dK / dV workgroup) and with the launcher's rule (gs0).
  model    a gpt-1b-sized rms / swiglu / rope model with 4 K / V heads: training forward + backward at 4 x 2048 and
           ``prefill`` of 2048 tokens, new path against the old one (Block.attention / ops.attention_qkv patched to
           expand K / V as before), with the peak memory of the training step and whether the fused weight-gradient
           pair (ops.wgrad_pair) took the grouped width.

One JSON line per row on stdout.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

KERNEL_SHAPES = [(4, 16, 2048, 128, (2, 4, 8)), (16, 12, 2048, 64, (2, 4, 6)), (1, 8, 2048, 128, (4,))]  # B, H, T, D, Gs


def time_blocks(fns: dict, blocks: int, iters: int) -> dict:
    import torch
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in times.items()}


def verdict(a: dict, b: dict) -> str:
    """a against b: 'tie' when the min-max ranges overlap."""
    if a["min_us"] <= b["max_us"] and b["min_us"] <= a["max_us"]:
        return "tie"
    return "wins" if a["median_us"] < b["median_us"] else "loses"


def kernels(args) -> None:
    import torch
    from kubeflow_rm_amd.ops import _lib, attention as A
    dev = "cuda"
    for (B, H, T, D, Gs) in KERNEL_SHAPES:
        for G in Gs:
            Hkv = H // G
            torch.manual_seed(0)
            qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
            q, k, v = A._qkv_views(qkv, H, Hkv, D)
            do = A._bhtd(torch.randn(B, T, H, D, device=dev).to(torch.bfloat16))
            scale = 1.0 / math.sqrt(D)

            def new(n):
                return A._bhtd(torch.empty(B, T, n, D, device=dev, dtype=torch.bfloat16))
            o, dq, dke, dve, dk, dv = new(H), new(H), new(H), new(H), new(Hkv), new(Hkv)

            def expand():
                return [A._bhtd(x.permute(0, 2, 1, 3).unsqueeze(3).expand(B, T, Hkv, G, D).reshape(B, T, H, D))
                        for x in (k, v)]
            ke, ve = expand()
            lse = A._fwd(q, k, v, o, True, scale)

            def fwd_expand():
                a, b = expand()
                A._fwd(q, a, b, o, True, scale)

            def bwd_expand():
                A._bwd(q, ke, ve, o, do, lse, dq, dke, dve, True, scale)
                for g in (dke, dve):  # autograd's backward of the expansion: the group sum, in bf16
                    g.permute(0, 2, 1, 3).reshape(B, T, Hkv, G, D).sum(3)
            fns = {"fwd_expand": fwd_expand, "fwd_grouped": lambda: A._fwd(q, k, v, o, True, scale),
                   "bwd_expand": bwd_expand}
            splits = [d for d in range(1, G + 1) if G % d == 0]
            for gs in [0, *splits]:
                fns[f"bwd_grouped_gs{gs}"] = (lambda gs=gs: A._bwd(q, k, v, o, do, lse, dq, dk, dv, True, scale, gs))
            r = time_blocks(fns, args.blocks, args.iters)
            rule = _lib.lib().kfamd_attn_bwd_gqa_group_split(B, H, Hkv, T, D)
            best = min(splits, key=lambda s: r[f"bwd_grouped_gs{s}"]["median_us"])
            print(json.dumps({"step": "kernels", "B": B, "H": H, "Hkv": Hkv, "G": G, "T": T, "D": D, **r,
                              "rule_gs": rule, "best_gs": best,
                              "rule_vs_best": verdict(r[f"bwd_grouped_gs{rule}"], r[f"bwd_grouped_gs{best}"]),
                              "fwd_grouped_vs_expand": verdict(r["fwd_grouped"], r["fwd_expand"]),
                              "bwd_grouped_vs_expand": verdict(r["bwd_grouped_gs0"], r["bwd_expand"])}), flush=True)


def model(args) -> None:
    import torch
    import torch.nn.functional as F  # noqa: F401
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import GPT, GPTConfig
    from kubeflow_rm_amd.models import gpt as G
    from kubeflow_rm_amd.ops import gemm
    cfg = GPTConfig(vocab_size=32000, d_model=2048, n_layers=args.layers, n_heads=16, d_ff=5504, max_seq=2048,
                    n_kv_heads=4, pos="rope", norm="rms", mlp="swiglu")
    torch.manual_seed(0)
    m = GPT(cfg, device="cuda")
    idx = torch.randint(0, cfg.vocab_size, (4, 2048), device="cuda")
    tgt = torch.randint(0, cfg.vocab_size, (4, 2048), device="cuda")
    new_attention, new_qkv = G.Block.attention, ops.attention_qkv

    def old_attention(self, x, residual=None, rope=None):  # the block's attention before the kernels knew groups
        B, T, _ = x.shape
        h, hkv, hd = self.local_heads, self.local_kv_heads, self.cfg.head_dim
        qkv = self.qkv(x)
        qkv = ops.rope_qkv(qkv, rope, h, hkv)
        q = qkv[..., :h * hd].view(B, T, h, hd)
        k, v = qkv[..., h * hd:].view(B, T, 2, hkv, hd).unbind(2)
        k = k.unsqueeze(3).expand(B, T, hkv, h // hkv, hd).reshape(B, T, h, hd)
        v = v.unsqueeze(3).expand(B, T, hkv, h // hkv, hd).reshape(B, T, h, hd)
        y = ops.flash_attention(*(t.transpose(1, 2) for t in (q, k, v)), causal=True)
        return self.proj(y.transpose(1, 2).reshape(B, T, h * hd), residual=residual)

    def old_qkv(qkv, h, hd, causal=True, scale=None, kv_heads=None):
        q, k, v = GPT._split_gqa(qkv, h, kv_heads, hd)
        B, T = qkv.shape[:2]
        return ops.flash_attention(q, k, v, causal=causal).transpose(1, 2).reshape(B, T, h * hd)

    def train(attention):
        def f():
            G.Block.attention = attention
            try:
                m.zero_grad(set_to_none=True)
                _, loss = m(idx, tgt)
                loss.backward()
            finally:
                G.Block.attention = new_attention
        return f

    def prefill(fn):
        def f():
            ops.attention_qkv = fn
            try:
                m.prefill(idx[:1], m.new_cache(1, 2048))
            finally:
                ops.attention_qkv = new_qkv
        return f
    pair, real = [], gemm.wgrad_pair

    def spy(*a, **kw):
        out = real(*a, **kw)
        pair.append((tuple(a[0].shape), out is not None))
        return out
    gemm.wgrad_pair = spy
    train(new_attention)()
    gemm.wgrad_pair = real
    peak = {}
    for name, att in (("old", old_attention), ("new", new_attention)):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        train(att)()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
    r = time_blocks({"train_old": train(old_attention), "train_new": train(new_attention),
                     "prefill_old": prefill(old_qkv), "prefill_new": prefill(new_qkv)}, args.blocks, 1)
    print(json.dumps({"step": "model", "layers": args.layers, "d_model": 2048, "heads": 16, "kv_heads": 4, "batch": "4x2048",
                      **r, "train_old_over_new": round(r["train_old"]["median_us"] / r["train_new"]["median_us"], 4),
                      "train_new_vs_old": verdict(r["train_new"], r["train_old"]),
                      "prefill_old_over_new": round(r["prefill_old"]["median_us"] / r["prefill_new"]["median_us"], 4),
                      "prefill_new_vs_old": verdict(r["prefill_new"], r["prefill_old"]),
                      "peak_bytes_old": peak["old"], "peak_bytes_new": peak["new"],
                      "wgrad_pair_qkv_dgrad_shape": pair[0][0] if pair else None,
                      "wgrad_pair_ran": bool(pair) and all(p[1] for p in pair)}), flush=True)


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
