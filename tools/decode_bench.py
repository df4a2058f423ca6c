#!/usr/bin/env python3
"""Decode benchmark: the M <= 16 weight-streaming GEMM, single-query attention and GPT.generate.

    python tools/decode_bench.py [--out decode_bench.json] [--steps gemm,attn,e2e,extend] [--quick]

The parent process never touches the GPU: every step runs as a child process of its own under a time
limit, and a step that fails or times out ends the run (nothing more is started on the GPU).

  gemm  gemm_nt(variant="skinny") (and each arithmetic pattern forced) against variant="auto" — the
        route these shapes took before — at M in {1, 2, 4, 8, 16} x the gpt-1b projection shapes. The two are
        interleaved block by block; medians over the blocks; the weights rotate through copies that
        together exceed the 256 MiB last-level cache, as a model's layers do.
  attn  ops.attention_decode against torch SDPA (bf16, masked) on the same cache: B*H in {16, 128,
        256}, D = 128, lens in {128, 2048, 4096}.
  e2e   gpt-small and gpt-1b, B in {1, 8, 16}, prompt 2048 - 128, 128 new tokens: native eager, native
        graphed and the torch-reference cached path of the same model, interleaved; ms/token and
        (weights + KV bytes read per token) / time as a fraction of the 6.29 TB/s copy roof.
  extend  multi-token steps. Kernel: ops.attention_extend at Tq in {1, 2, 4, 8, 16} against Tq calls of
        ops.attention_decode on the same cache (D = 128, capacity 4096, B*H in {16, 128}, lens in {128,
        2048, 4096}; caches rotated as in attn). Model: gpt-small and gpt-1b, B = 1, position 1920:
        one GPT.extend of T tokens against T decode_steps, each eager and as a hipGraph, interleaved.
  kv8   (not in the default list) the FP8 KV cache against the bf16 one, in the same process and in
        interleaved blocks with rotated caches: ops.attention_decode and ops.attention_extend at Tq in
        {4, 8} (D = 128, capacity 4096, B*H in {16, 128}, lens in {128, 2048, 4096}); ops.kv_append at T in
        {1, 2048}; gpt-1b (gpt-small with --quick) end to end in ms/token at B in {1, 16}, eager and
        graphed; KVCache.nbytes of both caches.
  w8    (not in the default list) FP8 decode weights against bf16 ones, same process, interleaved blocks,
        weights rotated past the last-level cache. Kernel: gemm_nt on a QuantizedWeight ("skinny", each form
        forced, and every tile count of each form forced) against the bf16 weight-streaming kernel on the
        gpt-1b projection shapes at M in {1, 2, 4, 8, 16}: us, bytes/s of W, ratio. Model: ms/token near
        position 2048 for gpt-small B = 1 and gpt-1b B in {1, 16} (gpt-small only with --quick), bf16 / FP8
        weights x bf16 / FP8 KV cache x eager / graphed; one extend of T in {4, 16} tokens at B = 1;
        DecodeWeights.nbytes against the bf16 bytes of the same matrices; the max-abs logit difference of
        one step on FP8 against bf16 weights (gpt-tiny and gpt-1b; reported, not judged).
  sample  (not in the default list) the fused sampler. Kernel: ops.sample against the model's torch _sample
        at V = 32000, B in {1, 16}, interleaved blocks: greedy, top_k = 50, top_p = 0.9 and both (_sample has
        no top_p: those two rows time it at the nearest setting it has, named in the row). Model: gpt-small
        and gpt-1b (gpt-small only with --quick), B in {1, 16}, temperature 1, top_k = 50, graphed, ms/token:
        the torch sampler between replays of graphed_decode_step against graphed_generate_step (step,
        sampler and token feedback in one graph), interleaved runs.
  chunk   (not in the default list) chunked prefill. Kernel: ops.attention_chunk at T in {16, 32, 64, 128, 256,
        512} new rows over 128 / 2048 / 4096 prior keys (D = 128, capacity 4096, B*H in {16, 128}, bf16 and FP8
        caches, rotated) against the only other way to do the same work, ceil(T / 16) calls of
        ops.attention_extend on 16-row slices with lens stepped, and against the ceiling, ops.attention_qkv
        (the flash kernel, causal) on T rows with no prior keys. Model: gpt-small and gpt-1b, B = 1, a
        512-token turn on a cache of 1536: extend(chunk=128 / 256 / 512) against extend without chunk, eager.
        Medians of 7 interleaved blocks with min and max.
  gqa   (not in the default list) grouped-query attention. Kernel: D = 128, capacity 4096, B = 8 x 16 query
        heads, 2048 and 4096 keys, bf16 and FP8 caches of 16 / G K / V heads (rotated past the last-level cache):
        ops.attention_decode at G in {1, 2, 4, 8, 16} interleaved in one process (time against G = 1 and
        against the K / V bytes), and at T * G in {8, 16} rows the VALU form (attn_extend_split) against the
        MFMA form (ops.attention_chunk) on the same cache: what ops.decode.GQA_MFMA_MIN_ROWS is set from.
        Model: the gpt-1b shape with n_kv_heads in {16, 4, 2} (random weights), B in {1, 16}, position about
        2048, bf16 and FP8 caches, eager and graphed, interleaved runs: ms/token and KVCache.nbytes.
  rope  (not in the default list) rotary position embeddings. Append: ops.kv_append(rope=table) (one launch)
        against kv_append alone and against rope_qkv + kv_append (two launches), the gpt-1b layer (B = 8, 16
        heads, D = 128), T in {1, 2048}, bf16 and FP8 caches, 7 interleaved blocks. Decode: gpt-1b with
        pos="rope" against pos="learned" in one process, B in {1, 16}, position about 2048, graphed and eager,
        7 interleaved runs: ms/token. Train: forward + backward of 4 x 2048 tokens (no optimiser), rotary
        against learned, 7 interleaved blocks.
  glu   (not in the default list) SwiGLU. Kernel: gemm_nt(act="swiglu") (one launch; "skinny", each arithmetic form
        forced, and every tile count / rows-per-wave of each form forced) against the two-launch form, the ungated
        weight-streaming GEMM to [M, 2F] then ops.swiglu, at M in {1, 2, 4, 8, 16}, d_model 2048, F in {8192, 5504},
        bf16 and FP8 weights, weights rotated past the last-level cache, 7 interleaved blocks: us, min - max. Model:
        a gpt-1b-sized norm="rms", mlp="swiglu", pos="rope", n_kv_heads=4 model (gpt-small-sized with --quick), the
        gated GEMM against the two-launch MLP in the same model (its _fc1 shadowed by this tool), B in {1, 16}, position
        about 2048, graphed and eager, 7 interleaved runs: ms/token. RMSNorm backward with dres at 8192 x 2048: the
        kernel against the fp32 torch arithmetic it replaced.
  window (not in the default list) sliding-window attention. Kernel: D = 128, capacity 4096, 4096 keys, B x 16 heads
        with B in {1, 8} (B * H = 16, 128), bf16 and FP8 caches rotated past the last-level cache: ops.attention_decode,
        ops.attention_extend at Tq = 4 and ops.attention_chunk at T = 128, each with window in {256, 1024, 4095, 4096}
        against window=None (the kernels without a window) interleaved in one process, medians of 7 blocks with min
        and max. 4096 removes nothing and, being t_bound, launches the kernels without a window; 4095 removes one key
        and runs the windowed ones. Model: gpt-1b (gpt-small with --quick), B in {1, 8}, a graphed decode step at
        position about 4000 with GPTConfig(window=1024) against none, 7 interleaved runs: ms/token.
  ring  (not in the default list) the ring-buffer KV cache. Kernel: D = 128, B x 16 heads for B in {1, 8}, position
        4000, W in {256, 1024}, bf16 and FP8, decode / extend Tq = 4 / chunk T = 128: the flat windowed launch, the
        ring launch at the same position and the ring launch at position 2^20 + 5 (no flat cache exists there),
        interleaved in one process, medians of 7 blocks with min and max. Model: a graphed gpt-1b step (gpt-small
        with --quick) at position about 4000 with W = 1024, flat against ring, B in {1, 8}, 7 interleaved runs.
        nbytes: both caches for gpt-1b shapes at max_seq = 32768, W = 4096, B in {1, 16} (meta device, no timing).
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

ROOF = 6.29e12
STEP_LIMIT_S = {"gemm": 300, "attn": 150, "e2e": 420, "extend": 600, "kv8": 420, "w8": 900, "sample": 420,
                "chunk": 900, "gqa": 1000, "rope": 600, "glu": 600, "window": 600, "ring": 900}
WINDOW_WS = (256, 1024, 4095, 4096)
GQA_GS = (1, 2, 4, 8, 16)
GQA_FORMS = ((8, 1), (4, 2), (2, 4), (16, 1), (8, 2), (4, 4), (2, 8))  # (G, T) with T * G in {8, 16}
CHUNK_TS = (16, 32, 64, 128, 256, 512)
KV8_TS = (4, 8)
EXTEND_TS = (1, 2, 4, 8, 16)
GEMM_MS = (1, 2, 4, 8, 16)  # 2 and 4: where the VALU / MFMA cut-over of the skinny kernel is decided
GEMM_SHAPES = [(6144, 2048), (2048, 2048), (8192, 2048), (2048, 8192), (32000, 2048)]  # (N, K)


def _time_blocks(fns: dict, blocks: int, iters: int):
    """Interleaved blocks: for each block, each candidate runs `iters` calls between two events."""
    import torch
    for f in fns.values():  # warm-up
        for i in range(3):
            f(i)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for b in range(blocks):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                f(b * iters + i)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / iters)  # us per call
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def step_gemm(quick: bool):
    import torch
    from kubeflow_rm_amd.ops import gemm_nt
    rows = []
    for N, K in GEMM_SHAPES:
        wbytes = N * K * 2
        ncopy = max(2, -(-(512 << 20) // wbytes)) if not quick else 2
        ws = [torch.randn(N, K, device="cuda").mul_(0.02).to(torch.bfloat16) for _ in range(ncopy)]
        bias = torch.randn(N, device="cuda").to(torch.bfloat16)
        for M in GEMM_MS:
            a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            variants = ["auto", "skinny", "skinny_mfma"] + (["skinny_valu"] if M <= 8 else [])
            fns = {v: (lambda i, v=v: gemm_nt(a, ws[i % ncopy], bias=bias, out=out, variant=v)) for v in variants}
            r = _time_blocks(fns, blocks=5 if quick else 7, iters=ncopy)
            row = {"M": M, "N": N, "K": K, "weight_copies": ncopy}
            for v, t in r.items():
                row[v] = {**t, "weight_GBps": wbytes / t["median_us"] / 1e3}
            row["auto_over_skinny"] = r["auto"]["median_us"] / r["skinny"]["median_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_attn(quick: bool):
    import torch
    import torch.nn.functional as F
    from kubeflow_rm_amd import ops
    rows = []
    D, cap = 128, 4096
    for BH in (16, 128, 256):
        B, H = BH // 16, 16
        ncopy = 1 if quick else max(1, min(4, (512 << 20) // (2 * B * H * cap * D * 2)))
        cache = ops.KVCache(ncopy, B, H, D, cap, device="cuda")
        for t in (*cache.k, *cache.v):
            t.normal_()
        q = torch.randn(B, H, D, device="cuda").to(torch.bfloat16)
        out = torch.empty(B, H, D, device="cuda", dtype=torch.bfloat16)
        for n in (128, 2048, 4096):
            cache.set_lens([n] * B)
            mask = torch.arange(cap, device="cuda").view(1, 1, 1, cap) < n

            def native(i):
                ops.attention_decode(q, cache, i % ncopy, out=out, t_bound=n)

            def sdpa_sliced(i):  # the best case for torch: the host knows the length and slices
                F.scaled_dot_product_attention(q.unsqueeze(2), cache.k[i % ncopy][:, :, :n], cache.v[i % ncopy][:, :, :n])

            def sdpa_masked(i):  # what a graph-capturable torch step has to do: mask the whole capacity
                F.scaled_dot_product_attention(q.unsqueeze(2), cache.k[i % ncopy], cache.v[i % ncopy], attn_mask=mask)

            r = _time_blocks({"native": native, "sdpa_sliced": sdpa_sliced, "sdpa_masked": sdpa_masked},
                             blocks=5 if quick else 7, iters=20)
            kv = 2 * B * H * n * D * 2
            row = {"B": B, "H": H, "D": D, "len": n, "kv_bytes": kv, **r,
                   "native_KV_GBps": kv / r["native"]["median_us"] / 1e3,
                   "sdpa_sliced_over_native": r["sdpa_sliced"]["median_us"] / r["native"]["median_us"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_e2e(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import CONFIGS, GPT, num_params
    rows = []
    prompt, new = 2048 - 128, 128
    for name in (("gpt-small",) if quick else ("gpt-small", "gpt-1b")):
        cfg = CONFIGS[name]
        model = GPT(cfg, device="cuda").eval()
        wbytes = num_params(model) * 2 - cfg.max_seq * cfg.d_model * 2  # every weight once; pos: one row
        for B in ((1, 8) if quick else (1, 8, 16)):
            idx = torch.randint(0, cfg.vocab_size, (B, prompt), device="cuda")
            toks = torch.randint(0, cfg.vocab_size, (new, B), device="cuda")

            def run(mode):
                cache = model.new_cache(B, prompt + new)
                model.prefill(idx, cache)
                step = (lambda t: model.decode_step(t, cache)) if mode != "graph" else model.graphed_decode_step(cache)
                step(toks[0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(1, new):
                    step(toks[i])
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / (new - 1)

            def run_ref():
                with ops.torch_reference():
                    return run("eager")

            res = {"native_eager": [], "native_graph": [], "torch_reference": []}
            for _ in range(3 if quick else 5):  # interleaved
                res["native_eager"].append(run("eager"))
                res["native_graph"].append(run("graph"))
                res["torch_reference"].append(run_ref())
            kv = 2 * cfg.n_layers * B * cfg.d_model * (prompt + new / 2) * 2
            row = {"model": name, "B": B, "prompt": prompt, "new": new, "bytes_per_token": wbytes + kv}
            for k, v in res.items():
                med = statistics.median(v)
                row[k] = {"ms_per_token": med, "min": min(v), "max": max(v),
                          "roof_fraction": (wbytes + kv) / (med * 1e-3) / ROOF}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()
    return rows


def _extend_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    D, cap = 128, 4096
    for BH in (16, 128):
        B, H = BH // 16, 16
        ncopy = 1 if quick else max(1, min(4, (512 << 20) // (2 * B * H * cap * D * 2)))
        cache = ops.KVCache(ncopy, B, H, D, cap, device="cuda")
        for t in (*cache.k, *cache.v):
            t.normal_()
        for n in (128, 2048, 4096):
            cache.set_lens([n] * B)
            for Tq in EXTEND_TS:
                q = torch.randn(B, Tq, H, D, device="cuda").to(torch.bfloat16)
                out = torch.empty(B, Tq, H, D, device="cuda", dtype=torch.bfloat16)

                def extend(i):
                    ops.attention_extend(q, cache, i % ncopy, out=out, t_bound=n)

                def decode_x_tq(i):  # what a cache that grows one token at a time costs for the same rows
                    for t in range(Tq):
                        ops.attention_decode(q[:, t], cache, i % ncopy, out=out[:, t], t_bound=n)

                r = _time_blocks({"extend": extend, "decode_x_tq": decode_x_tq}, blocks=5 if quick else 7, iters=20)
                kv = 2 * B * H * n * D * 2
                row = {"B": B, "H": H, "D": D, "len": n, "Tq": Tq, "kv_bytes": kv, "cache_copies": ncopy, **r,
                       "extend_KV_GBps": kv / r["extend"]["median_us"] / 1e3,
                       "decode_x_tq_over_extend": r["decode_x_tq"]["median_us"] / r["extend"]["median_us"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def _extend_model_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import CONFIGS, GPT
    rows = []
    pos, cap, iters = 1920, 2048, 4  # iters * 16 rows fit between the position and the capacity
    for name in (("gpt-small",) if quick else ("gpt-small", "gpt-1b")):
        cfg = CONFIGS[name]
        model = GPT(cfg, device="cuda").eval()
        eager, pinned = model.new_cache(1, cap), model.new_cache(1, cap)  # a captured step pins the grid to the capacity
        for c in (eager, pinned):
            for t in (*c.k, *c.v):
                t.normal_()
            c.set_lens([pos])
        dstep = model.graphed_decode_step(pinned)
        for T in EXTEND_TS:
            toks = torch.randint(0, cfg.vocab_size, (1, T), device="cuda")
            pinned.set_lens([pos])
            gstep = ops.GraphedCallable(lambda t: model.extend(t, pinned), toks.clone(), warmup=1)
            torch.cuda.synchronize()

            def decode_graph():
                for t in range(T):
                    dstep(toks[:, t])

            def decode_eager():
                for t in range(T):
                    model.decode_step(toks[:, t], eager)

            cands = {"extend_eager": (eager, lambda: model.extend(toks, eager)), "decode_eager": (eager, decode_eager),
                     "extend_graph": (pinned, lambda: gstep(toks)), "decode_graph": (pinned, decode_graph)}
            times = {k: [] for k in cands}
            for b in range(-1, 5 if quick else 7):  # block -1: warm-up, not recorded
                for k, (c, f) in cands.items():
                    c.set_lens([pos])  # a sync, outside the timed region: every block starts at the same position
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        f()
                    e1.record()
                    e1.synchronize()
                    if b >= 0:
                        times[k].append(e0.elapsed_time(e1) / iters)  # ms per T tokens
            row = {"model": name, "B": 1, "T": T, "position": pos, "capacity": cap}
            for k, v in times.items():
                row[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            row["decode_over_extend_eager"] = row["decode_eager"]["median_ms"] / row["extend_eager"]["median_ms"]
            row["decode_over_extend_graph"] = row["decode_graph"]["median_ms"] / row["extend_graph"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del gstep
        del model, eager, pinned, dstep
        torch.cuda.empty_cache()
    return rows


def step_extend(quick: bool):
    return {"kernel": _extend_kernel_rows(quick), "model": _extend_model_rows(quick)}


def _chunk_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    D, cap = 128, 4096
    for BH in ((16,) if quick else (16, 128)):
        B, H = BH // 16, 16
        ncopy = 1 if quick else max(1, min(4, (512 << 20) // (2 * B * H * cap * D * 2)))
        caches = _kv8_caches(B, H, D, cap, ncopy)
        for prior in (128, 2048, 4096):
            for T in CHUNK_TS:
                n = prior + T
                if n > cap:  # 4096 prior keys: the block is the cache's last T rows
                    n, prior = cap, cap - T
                qkv = torch.randn(B, T, 3 * H * D, device="cuda").to(torch.bfloat16)
                q = qkv.view(B, T, 3, H, D)[:, :, 0]
                out = torch.empty(B, T, H, D, device="cuda", dtype=torch.bfloat16)
                lens16 = [torch.full((B,), prior + min(t0 + 16, T), device="cuda", dtype=torch.int32)
                          for t0 in range(0, T, 16)]
                fns = {"flash_no_prior": lambda i: ops.attention_qkv(qkv, H, D, causal=True)}
                for kind, cache in caches.items():
                    cache.set_lens([n] * B)

                    def chunk(i, c=cache):
                        ops.attention_chunk(q, c, i % ncopy, out=out, t_bound=n)

                    def extend16(i, c=cache):  # the same rows, 16 at a time, each slice up to its own last row
                        for j, t0 in enumerate(range(0, T, 16)):
                            ops.attention_extend(q[:, t0:t0 + 16], c, i % ncopy, out=out[:, t0:t0 + 16], lens=lens16[j],
                                                 t_bound=n)

                    fns[f"chunk_{kind}"], fns[f"extend16_{kind}"] = chunk, extend16
                r = _time_blocks(fns, blocks=5 if quick else 7, iters=10)
                row = {"B": B, "H": H, "D": D, "prior": prior, "T": T, "cache_copies": ncopy, **r}
                for kind in caches:
                    a, b = r[f"chunk_{kind}"], r[f"extend16_{kind}"]
                    row[f"extend16_over_chunk_{kind}"] = b["median_us"] / a["median_us"]
                    row[f"verdict_{kind}"] = ("tie" if a["min_us"] <= b["max_us"] and b["min_us"] <= a["max_us"]
                                              else "chunk wins" if a["median_us"] < b["median_us"] else "chunk loses")
                rows.append(row)
                print(json.dumps(row), flush=True)
        del caches
        torch.cuda.empty_cache()
    return rows


def _chunk_model_rows(quick: bool):
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    rows = []
    pos, T, cap = 1536, 512, 2048
    for name in (("gpt-small",) if quick else ("gpt-small", "gpt-1b")):
        cfg = CONFIGS[name]
        model = GPT(cfg, device="cuda").eval()
        cache = model.new_cache(1, cap)
        for t in (*cache.k, *cache.v):
            t.normal_()
        toks = torch.randint(0, cfg.vocab_size, (1, T), device="cuda")
        cands = {"extend16": lambda: model.extend(toks, cache, last_only=True)}
        for N in (128, 256, 512):
            cands[f"chunk{N}"] = lambda N=N: model.extend(toks, cache, last_only=True, chunk=N)
        times = {k: [] for k in cands}
        for b in range(-1, 5 if quick else 7):  # block -1: warm-up, not recorded
            for k, f in cands.items():
                cache.set_lens([pos])  # a sync, outside the timed region: every run starts at the same position
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if b >= 0:
                    times[k].append(e0.elapsed_time(e1))  # ms per turn of T tokens
        row = {"model": name, "B": 1, "T": T, "position": pos, "capacity": cap}
        for k, v in times.items():
            row[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        for N in (128, 256, 512):
            row[f"extend16_over_chunk{N}"] = row["extend16"]["median_ms"] / row[f"chunk{N}"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del model, cache
        torch.cuda.empty_cache()
    return rows


def step_chunk(quick: bool):
    return {"kernel": _chunk_kernel_rows(quick), "model": _chunk_model_rows(quick)}


def _kv8_caches(B, H, D, cap, ncopy):
    """A bf16 and an FP8 cache holding the same random rows (the FP8 one through the quantising append)."""
    import torch
    from kubeflow_rm_amd import ops
    caches = {"bf16": ops.KVCache(ncopy, B, H, D, cap, device="cuda"),
              "fp8": ops.KVCache(ncopy, B, H, D, cap, device="cuda", dtype=torch.float8_e4m3fn)}
    chunk = 512
    for layer in range(ncopy):
        for c in caches.values():
            c.reset()
        for t0 in range(0, cap, chunk):
            qkv = torch.randn(B, min(chunk, cap - t0), 3 * H * D, device="cuda").to(torch.bfloat16)
            for c in caches.values():
                ops.kv_append(qkv, c, layer)
            for c in caches.values():
                c.advance(qkv.shape[1])
    return caches


def _kv8_ratio(row, r):
    for k, t in r.items():
        row[k] = t
    row["bf16_over_fp8"] = r["bf16"]["median_us"] / r["fp8"]["median_us"]
    # a win or a loss only beyond the blocks' spread
    row["separated"] = r["fp8"]["max_us"] < r["bf16"]["min_us"] or r["bf16"]["max_us"] < r["fp8"]["min_us"]
    return row


def _kv8_attention_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    D, cap = 128, 4096
    blocks = 5 if quick else 7
    for BH in (16, 128):
        B, H = BH // 16, 16
        ncopy = 1 if quick else max(1, min(4, (512 << 20) // (2 * B * H * cap * D * 2)))
        caches = _kv8_caches(B, H, D, cap, ncopy)
        for n in (128, 2048, 4096):
            for c in caches.values():
                c.set_lens([n] * B)
            q = torch.randn(B, H, D, device="cuda").to(torch.bfloat16)
            out = torch.empty(B, H, D, device="cuda", dtype=torch.bfloat16)
            fns = {k: (lambda i, c=c: ops.attention_decode(q, c, i % ncopy, out=out, t_bound=n))
                   for k, c in caches.items()}
            r = _time_blocks(fns, blocks=blocks, iters=20)
            row = _kv8_ratio({"op": "decode", "B": B, "H": H, "D": D, "len": n, "cache_copies": ncopy}, r)
            row["bf16_KV_GBps"] = 2 * B * H * n * D * 2 / r["bf16"]["median_us"] / 1e3
            row["fp8_KV_GBps"] = 2 * B * H * n * (D + 4) / r["fp8"]["median_us"] / 1e3
            rows.append(row)
            print(json.dumps(row), flush=True)
            for Tq in KV8_TS:
                qe = torch.randn(B, Tq, H, D, device="cuda").to(torch.bfloat16)
                oe = torch.empty(B, Tq, H, D, device="cuda", dtype=torch.bfloat16)
                fns = {k: (lambda i, c=c: ops.attention_extend(qe, c, i % ncopy, out=oe, t_bound=n))
                       for k, c in caches.items()}
                r = _time_blocks(fns, blocks=blocks, iters=20)
                row = _kv8_ratio({"op": "extend", "Tq": Tq, "B": B, "H": H, "D": D, "len": n, "cache_copies": ncopy}, r)
                row["bf16_KV_GBps"] = 2 * B * H * n * D * 2 / r["bf16"]["median_us"] / 1e3
                row["fp8_KV_GBps"] = 2 * B * H * n * (D + 4) / r["fp8"]["median_us"] / 1e3
                rows.append(row)
                print(json.dumps(row), flush=True)
        del caches
        torch.cuda.empty_cache()
    return rows


def _kv8_append_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    B, H, D, cap, ncopy = 8, 16, 128, 4096, 2
    caches = {"bf16": ops.KVCache(ncopy, B, H, D, cap, device="cuda"),
              "fp8": ops.KVCache(ncopy, B, H, D, cap, device="cuda", dtype=torch.float8_e4m3fn)}
    for T in (1, 2048):
        qkv = torch.randn(B, T, 3 * H * D, device="cuda").to(torch.bfloat16)
        for c in caches.values():
            c.set_lens([cap - T] * B)  # lens is not advanced by the append: every call writes the same rows
        fns = {k: (lambda i, c=c: ops.kv_append(qkv, c, i % ncopy)) for k, c in caches.items()}
        r = _time_blocks(fns, blocks=5 if quick else 7, iters=20)
        row = _kv8_ratio({"op": "kv_append", "B": B, "H": H, "D": D, "T": T}, r)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _kv8_model_rows(quick: bool):
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    rows = []
    prompt, new = 2048 - 128, 128
    name = "gpt-small" if quick else "gpt-1b"
    cfg = CONFIGS[name]
    model = GPT(cfg, device="cuda").eval()
    kinds = {"bf16": None, "fp8": torch.float8_e4m3fn}
    for B in (1, 16):
        idx = torch.randint(0, cfg.vocab_size, (B, prompt), device="cuda")
        toks = torch.randint(0, cfg.vocab_size, (new, B), device="cuda")
        nbytes = {}

        def run(kind, mode):
            cache = model.new_cache(B, prompt + new, kv_dtype=kinds[kind])
            model.prefill(idx, cache)
            step = (lambda t: model.decode_step(t, cache)) if mode != "graph" else model.graphed_decode_step(cache)
            step(toks[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(1, new):
                step(toks[i])
            torch.cuda.synchronize()
            nbytes[kind] = cache.nbytes
            return (time.perf_counter() - t0) * 1e3 / (new - 1)

        res = {f"{k}_{m}": [] for k in kinds for m in ("eager", "graph")}
        for _ in range(3 if quick else 5):  # interleaved
            for key in res:
                res[key].append(run(*key.split("_")))
        row = {"model": name, "B": B, "prompt": prompt, "new": new, "cache_nbytes": dict(nbytes),
               "nbytes_fp8_over_bf16": nbytes["fp8"] / nbytes["bf16"]}
        for k, v in res.items():
            row[k] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
        for m in ("eager", "graph"):
            row[f"bf16_over_fp8_{m}"] = row[f"bf16_{m}"]["ms_per_token"] / row[f"fp8_{m}"]["ms_per_token"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_kv8(quick: bool):
    return {"attention": _kv8_attention_rows(quick), "append": _kv8_append_rows(quick),
            "model": _kv8_model_rows(quick)}


def _sep(a, b):
    """A win or a loss only beyond the blocks' spread (a, b: {"min", "max"} in any unit)."""
    return a["max"] < b["min"] or b["max"] < a["min"]


def _w8_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.gemm import _gemm_nt_w8
    rows = []
    for N, K in GEMM_SHAPES:
        ncopy = 2 if quick else max(2, -(-(512 << 20) // (N * K)))  # the 8-bit copies alone exceed the cache
        ws = [torch.randn(N, K, device="cuda").mul_(0.02).to(torch.bfloat16) for _ in range(ncopy)]
        qs = [ops.quantize_weight(w) for w in ws]
        bias = torch.randn(N, device="cuda").to(torch.bfloat16)
        for M in GEMM_MS:
            a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)

            def w8(variant, tiles=0):
                return lambda i: _gemm_nt_w8(a, qs[i % ncopy], bias, None, 1.0, "none", out, variant, tiles)

            fns = {"bf16": lambda i: ops.gemm_nt(a, ws[i % ncopy], bias=bias, out=out, variant="skinny"),
                   "w8": w8("skinny"), "w8_mfma": w8("skinny_mfma"),
                   **{f"w8_mfma_t{t}": w8("skinny_mfma", t) for t in (1, 2, 4)}}
            if M <= 8:
                fns.update({"w8_valu": w8("skinny_valu"), "w8_valu_r2": w8("skinny_valu", 2),
                            "w8_valu_r4": w8("skinny_valu", 4)})
            r = _time_blocks(fns, blocks=5 if quick else 7, iters=ncopy)
            row = {"M": M, "N": N, "K": K, "weight_copies": ncopy}
            for v, t in r.items():
                row[v] = {**t, "weight_GBps": N * K * (2 if v == "bf16" else 1) / t["median_us"] / 1e3}
            row["bf16_over_w8"] = r["bf16"]["median_us"] / r["w8"]["median_us"]
            row["separated"] = _sep({"min": r["w8"]["min_us"], "max": r["w8"]["max_us"]},
                                    {"min": r["bf16"]["min_us"], "max": r["bf16"]["max_us"]})
            rows.append(row)
            print(json.dumps(row), flush=True)
        del ws, qs
        torch.cuda.empty_cache()
    return rows


def _w8_model_rows(model, name: str, B: int, quick: bool):
    """ms/token around position 2048: bf16 / FP8 weights x bf16 / FP8 KV cache x eager / graphed, interleaved."""
    import torch
    cfg = model.cfg
    prompt, new = 2048 - 128, 64 if quick else 128
    weights = {"wbf16": None, "wfp8": model.decode_weights()}
    kvs = {"kvbf16": None, "kvfp8": torch.float8_e4m3fn}
    idx = torch.randint(0, cfg.vocab_size, (B, prompt), device="cuda")
    toks = torch.randint(0, cfg.vocab_size, (new, B), device="cuda")

    def run(w, kv, mode):
        cache = model.new_cache(B, prompt + new, kv_dtype=kvs[kv])
        model.prefill(idx, cache)
        W = weights[w]
        step = ((lambda t: model.decode_step(t, cache, weights=W)) if mode != "graph"
                else model.graphed_decode_step(cache, weights=W))
        step(toks[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, new):
            step(toks[i])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (new - 1)

    res = {f"{w}_{kv}_{m}": [] for w in weights for kv in kvs for m in ("eager", "graph")}
    for _ in range(3 if quick else 7):  # interleaved
        for key in res:
            res[key].append(run(*key.split("_")))
    row = {"model": name, "B": B, "prompt": prompt, "new": new}
    for k, v in res.items():
        row[k] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
    for kv in kvs:
        for m in ("eager", "graph"):
            b, f = row[f"wbf16_{kv}_{m}"], row[f"wfp8_{kv}_{m}"]
            row[f"bf16_over_fp8_weights_{kv}_{m}"] = b["ms_per_token"] / f["ms_per_token"]
            row[f"separated_{kv}_{m}"] = _sep(b, f)
    print(json.dumps(row), flush=True)
    return row


def _w8_extend_rows(model, name: str, quick: bool):
    """One extend of T tokens at B = 1, position 1920: bf16 against FP8 weights, eager and as a hipGraph."""
    import torch
    from kubeflow_rm_amd import ops
    cfg = model.cfg
    pos, cap, iters = 1920, 2048, 4
    W = model.decode_weights()
    eager, pinned = model.new_cache(1, cap), model.new_cache(1, cap)
    for c in (eager, pinned):
        for t in (*c.k, *c.v):
            t.normal_()
        c.set_lens([pos])
    pinned.pin_bound()
    rows = []
    for T in (4, 16):
        toks = torch.randint(0, cfg.vocab_size, (1, T), device="cuda")
        graphs = {}
        for k, w in (("wbf16", None), ("wfp8", W)):
            pinned.set_lens([pos])
            graphs[k] = ops.GraphedCallable(lambda t, w=w: model.extend(t, pinned, weights=w), toks.clone(), warmup=1)
        torch.cuda.synchronize()
        cands = {"wbf16_eager": (eager, lambda: model.extend(toks, eager)),
                 "wfp8_eager": (eager, lambda: model.extend(toks, eager, weights=W)),
                 "wbf16_graph": (pinned, lambda: graphs["wbf16"](toks)),
                 "wfp8_graph": (pinned, lambda: graphs["wfp8"](toks))}
        times = {k: [] for k in cands}
        for b in range(-1, 5 if quick else 7):  # block -1: warm-up, not recorded
            for k, (c, f) in cands.items():
                c.set_lens([pos])  # a sync, outside the timed region: every block starts at the same position
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    f()
                e1.record()
                e1.synchronize()
                if b >= 0:
                    times[k].append(e0.elapsed_time(e1) / iters)  # ms per extend of T tokens
        row = {"model": name, "B": 1, "T": T, "position": pos, "capacity": cap}
        for k, v in times.items():
            row[k] = {"median_ms": statistics.median(v), "min": min(v), "max": max(v)}
        for m in ("eager", "graph"):
            row[f"bf16_over_fp8_weights_{m}"] = row[f"wbf16_{m}"]["median_ms"] / row[f"wfp8_{m}"]["median_ms"]
            row[f"separated_{m}"] = _sep(row[f"wbf16_{m}"], row[f"wfp8_{m}"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del graphs
    return rows


def _w8_logit_row(model, name: str):
    """max-abs logit difference of one decode step on FP8 against bf16 weights (one prompt; reported only)."""
    import torch
    cfg = model.cfg
    T0 = min(128, cfg.max_seq - 2)
    idx = torch.randint(0, cfg.vocab_size, (1, T0), device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    outs = []
    for W in (None, model.decode_weights()):
        cache = model.new_cache(1, T0 + 1)
        tok = model.prefill(idx, cache).argmax(-1)
        outs.append(model.decode_step(tok, cache, weights=W).float())
    row = {"model": name, "prompt": T0, "max_abs_logit_diff": (outs[0] - outs[1]).abs().max().item(),
           "max_abs_logit": outs[0].abs().max().item(), "argmax_equal": bool((outs[0].argmax(-1) == outs[1].argmax(-1)).all())}
    print(json.dumps(row), flush=True)
    return row


def step_w8(quick: bool):
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    result = {"kernel": _w8_kernel_rows(quick), "model": [], "extend": [], "nbytes": [], "logits": []}
    plan = [("gpt-tiny", ()), ("gpt-small", (1,))] + ([] if quick else [("gpt-1b", (1, 16))])
    for name, batches in plan:
        model = GPT(CONFIGS[name], device="cuda").eval()
        W = model.decode_weights()
        bf16 = sum(q.shape[0] * q.shape[1] * 2 for q in W.matrices())
        row = {"model": name, "decode_weights_nbytes": W.nbytes, "bf16_nbytes": bf16, "ratio": W.nbytes / bf16}
        print(json.dumps(row), flush=True)
        result["nbytes"].append(row)
        if name != "gpt-small":  # the test model and gpt-1b
            result["logits"].append(_w8_logit_row(model, name))
        for B in batches:
            result["model"].append(_w8_model_rows(model, name, B, quick))
        if batches:
            result["extend"] += _w8_extend_rows(model, name, quick)
        del model, W
        torch.cuda.empty_cache()
    return result


def _sample_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models.gpt import _sample
    rows, V, ncopy = [], 32000, 8
    settings = {"greedy": (0.0, None, None), "top_k50": (1.0, 50, None), "top_p0.9": (1.0, None, 0.9),
                "top_k50_top_p0.9": (1.0, 50, 0.9)}
    for B in (1, 16):
        logits = [(torch.randn(B, V, device="cuda") * 4).to(torch.bfloat16) for _ in range(ncopy)]
        u = torch.rand(ncopy, B, device="cuda")
        out = torch.empty(B, dtype=torch.long, device="cuda")
        for name, (temp, k, p) in settings.items():
            fns = {"fused": lambda i: ops.sample(logits[i % ncopy], u[i % ncopy], temp, k, p, out=out),
                   "torch": lambda i: _sample(logits[i % ncopy], temp, k, None)}
            r = _time_blocks(fns, 5 if quick else 15, 50)
            row = {"B": B, "V": V, "setting": name, "torch_setting": "greedy" if temp == 0 else f"top_k={k}", **r,
                   "torch_over_fused": r["torch"]["median_us"] / r["fused"]["median_us"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _sample_model_rows(model, name: str, B: int, quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models.gpt import _sample
    cfg = model.cfg
    prompt, new, temp, k = 512 - 128, 128, 1.0, 50
    idx = torch.randint(0, cfg.vocab_size, (B, prompt), device="cuda")

    def run(kind):
        cache = model.new_cache(B, prompt + new)
        logits = model.prefill(idx, cache)
        if kind == "torch_between_replays":  # generate(graph=True): the parent's token loop
            step = model.graphed_decode_step(cache)
            logits = step(_sample(logits, temp, k, None))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(new - 2):
                logits = step(_sample(logits, temp, k, None))
        else:  # generate(graph=True, sampler="fused")
            u = torch.rand(new, B, device="cuda")
            tok = torch.empty(B, dtype=torch.long, device="cuda")
            seq = torch.empty(B, new, dtype=torch.long, device="cuda")
            pos = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.sample(logits, u, temp, k, step=pos, out=tok, seq=seq)
            pos.add_(1)
            g = model.graphed_generate_step(cache, tok=tok, u=u, step=pos, seq=seq, temperature=temp, top_k=k)
            g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(new - 2):
                g.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (new - 2)

    res = {"torch_between_replays": [], "fused_in_graph": []}
    for _ in range(3 if quick else 7):  # interleaved
        for key in res:
            res[key].append(run(key))
    row = {"model": name, "B": B, "prompt": prompt, "new": new, "temperature": temp, "top_k": k}
    for key, v in res.items():
        row[key] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
    row["torch_over_fused"] = row["torch_between_replays"]["ms_per_token"] / row["fused_in_graph"]["ms_per_token"]
    print(json.dumps(row), flush=True)
    return row


def step_sample(quick: bool):
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    result = {"kernel": _sample_kernel_rows(quick), "model": []}
    for name in ("gpt-small",) if quick else ("gpt-small", "gpt-1b"):
        model = GPT(CONFIGS[name], device="cuda").eval()
        for B in (1, 16):
            result["model"].append(_sample_model_rows(model, name, B, quick))
        del model
        torch.cuda.empty_cache()
    return result


def _gqa_caches(B, Hq, Hkv, D, cap, quick: bool):
    """A bf16 and an FP8 cache of Hkv heads, full of random rows (the grouped append), with enough layers that
    a rotation through them exceeds the 256 MiB last-level cache (at most 32)."""
    import torch
    from kubeflow_rm_amd import ops
    ncopy = 1 if quick else max(2, min(32, -(-(512 << 20) // (2 * B * Hkv * cap * D * 2))))
    caches = {"bf16": ops.KVCache(ncopy, B, Hkv, D, cap, device="cuda"),
              "fp8": ops.KVCache(ncopy, B, Hkv, D, cap, device="cuda", dtype=torch.float8_e4m3fn)}
    for layer in range(ncopy):
        for c in caches.values():
            c.reset()
        for t0 in range(0, cap, 512):
            qkv = torch.randn(B, min(512, cap - t0), (Hq + 2 * Hkv) * D, device="cuda").to(torch.bfloat16)
            for c in caches.values():
                ops.kv_append(qkv, c, layer, q_heads=Hq)
                c.advance(qkv.shape[1])
    return caches, ncopy


def _gqa_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops import decode
    rows = {"decode": [], "forms": []}
    B, Hq, D, cap = 8, 16, 128, 4096
    blocks = 5 if quick else 7
    caches, ncopy = {}, {}
    for G in GQA_GS:
        caches[G], ncopy[G] = _gqa_caches(B, Hq, Hq // G, D, cap, quick)
    q = torch.randn(B, Hq, D, device="cuda").to(torch.bfloat16)
    out = torch.empty(B, Hq, D, device="cuda", dtype=torch.bfloat16)
    routed = decode.GQA_MFMA_MIN_ROWS

    def valu(fn, *a, **kw):  # the VALU form whatever the routing says
        decode.GQA_MFMA_MIN_ROWS = None
        try:
            return fn(*a, **kw)
        finally:
            decode.GQA_MFMA_MIN_ROWS = routed

    for n in (2048, 4096):
        for kind in ("bf16", "fp8"):
            for G in GQA_GS:
                caches[G][kind].set_lens([n] * B)
            # decode as routed (what a model step runs), every G interleaved with G = 1
            fns = {f"G{G}": (lambda i, G=G: ops.attention_decode(q, caches[G][kind], i % ncopy[G], out=out, t_bound=n))
                   for G in GQA_GS}
            r = _time_blocks(fns, blocks=blocks, iters=20)
            row = {"op": "decode", "kind": kind, "B": B, "Hq": Hq, "D": D, "len": n, "cache_copies": dict(ncopy)}
            for G in GQA_GS:
                t = r[f"G{G}"]
                kv = 2 * B * (Hq // G) * n * (D * 2 if kind == "bf16" else D + 4)
                row[f"G{G}"] = {**t, "KV_GBps": kv / t["median_us"] / 1e3,
                                "G1_over_this": r["G1"]["median_us"] / t["median_us"],
                                "separated_from_G1": G > 1 and _sep({"min": t["min_us"], "max": t["max_us"]},
                                                                    {"min": r["G1"]["min_us"],
                                                                     "max": r["G1"]["max_us"]})}
            rows["decode"].append(row)
            print(json.dumps(row), flush=True)
            # the two forms at 8 and 16 rows per K / V head
            for G, T in GQA_FORMS:
                c, nc = caches[G][kind], ncopy[G]
                c.set_lens([n] * B)
                qe = torch.randn(B, T, Hq, D, device="cuda").to(torch.bfloat16)
                oe = torch.empty(B, T, Hq, D, device="cuda", dtype=torch.bfloat16)
                fns = {"valu": (lambda i: valu(ops.attention_extend, qe, c, i % nc, out=oe, t_bound=n)),
                       "mfma": (lambda i: ops.attention_chunk(qe, c, i % nc, out=oe, t_bound=n))}
                r = _time_blocks(fns, blocks=blocks, iters=20)
                row = {"op": "forms", "kind": kind, "G": G, "T": T, "rows": G * T, "B": B, "Hq": Hq, "D": D, "len": n,
                       **r, "valu_over_mfma": r["valu"]["median_us"] / r["mfma"]["median_us"],
                       "separated": _sep({"min": r["valu"]["min_us"], "max": r["valu"]["max_us"]},
                                         {"min": r["mfma"]["min_us"], "max": r["mfma"]["max_us"]})}
                rows["forms"].append(row)
                print(json.dumps(row), flush=True)
    return rows


def _gqa_model_rows(quick: bool):
    import dataclasses
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    rows = []
    prompt, new = 2048 - 64, 64
    base = CONFIGS["gpt-small" if quick else "gpt-1b"]
    kvs = (base.n_heads, 4, 2)
    models = {kv: GPT(dataclasses.replace(base, n_kv_heads=kv), device="cuda").eval() for kv in kvs}
    kinds = {"bf16": None, "fp8": torch.float8_e4m3fn}
    for B in (1, 16):
        idx = torch.randint(0, base.vocab_size, (B, prompt), device="cuda")
        toks = torch.randint(0, base.vocab_size, (new, B), device="cuda")
        nbytes = {}

        def run(kv, kind, mode):
            model = models[kv]
            cache = model.new_cache(B, prompt + new, kv_dtype=kinds[kind])
            model.prefill(idx, cache)
            step = (lambda t: model.decode_step(t, cache)) if mode != "graph" else model.graphed_decode_step(cache)
            step(toks[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(1, new):
                step(toks[i])
            torch.cuda.synchronize()
            nbytes[f"kv{kv}_{kind}"] = cache.nbytes
            return (time.perf_counter() - t0) * 1e3 / (new - 1)

        keys = [(kv, kind, mode) for kv in kvs for kind in kinds for mode in ("eager", "graph")]
        res = {k: [] for k in keys}
        for _ in range(3):  # interleaved
            for k in keys:
                res[k].append(run(*k))
        row = {"model": f"{'gpt-small' if quick else 'gpt-1b'} shape", "n_heads": base.n_heads, "B": B, "prompt": prompt,
               "new": new, "cache_nbytes": dict(nbytes)}
        for (kv, kind, mode), v in res.items():
            row[f"kv{kv}_{kind}_{mode}"] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_gqa(quick: bool):
    return {"kernel": _gqa_kernel_rows(quick), "model": _gqa_model_rows(quick)}


def _rope_append_rows(quick: bool):
    """(a) the fused rotate-and-append against kv_append alone and against kv_append + a separate rope_qkv launch."""
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    B, H, D, cap, ncopy = 8, 16, 128, 4096, 2  # the gpt-1b layer
    table = ops.rope_table(cap, D, device="cuda")
    for kind, dt in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
        cache = ops.KVCache(ncopy, B, H, D, cap, device="cuda", dtype=dt)
        for T in (1, 2048):
            qkv = torch.randn(B, T, 3 * H * D, device="cuda").to(torch.bfloat16)
            cache.set_lens([cap - T] * B)  # lens is not advanced by the append: every call writes the same rows

            def two(i):
                ops.rope_qkv(qkv, table, H, H, cache.lens)
                ops.kv_append(qkv, cache, i % ncopy)

            fns = {"append": lambda i: ops.kv_append(qkv, cache, i % ncopy),
                   "fused": lambda i: ops.kv_append(qkv, cache, i % ncopy, rope=table),
                   "rope_then_append": two}
            r = _time_blocks(fns, blocks=5 if quick else 7, iters=20)
            row = {"op": "kv_append", "cache": kind, "B": B, "H": H, "D": D, "T": T, **r,
                   "fused_over_append": r["fused"]["median_us"] / r["append"]["median_us"],
                   "two_launches_over_fused": r["rope_then_append"]["median_us"] / r["fused"]["median_us"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _rope_models(quick: bool):
    import dataclasses
    from kubeflow_rm_amd.models import CONFIGS, GPT
    base = CONFIGS["gpt-small" if quick else "gpt-1b"]
    return base, {p: GPT(dataclasses.replace(base, pos=p), device="cuda") for p in ("learned", "rope")}


def _rope_decode_rows(quick: bool, base, models):
    """(b) graphed (and eager) decode, ms/token around position 2048: pos="rope" against pos="learned"."""
    import torch
    rows = []
    prompt, new = 2048 - 64, 64
    for B in (1, 16):
        idx = torch.randint(0, base.vocab_size, (B, prompt), device="cuda")
        toks = torch.randint(0, base.vocab_size, (new, B), device="cuda")

        def run(p, mode):
            model = models[p].eval()
            cache = model.new_cache(B, prompt + new)
            model.prefill(idx, cache)
            step = (lambda t: model.decode_step(t, cache)) if mode != "graph" else model.graphed_decode_step(cache)
            step(toks[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(1, new):
                step(toks[i])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (new - 1)

        keys = [(p, mode) for mode in ("graph", "eager") for p in ("learned", "rope")]
        res = {k: [] for k in keys}
        for _ in range(3 if quick else 7):  # interleaved
            for k in keys:
                res[k].append(run(*k))
        row = {"model": f"{'gpt-small' if quick else 'gpt-1b'}", "B": B, "prompt": prompt, "new": new}
        for (p, mode), v in res.items():
            row[f"{p}_{mode}"] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
        for mode in ("graph", "eager"):
            a, b = row[f"rope_{mode}"], row[f"learned_{mode}"]
            row[f"rope_over_learned_{mode}"] = a["ms_per_token"] / b["ms_per_token"]
            row[f"separated_{mode}"] = a["max"] < b["min"] or b["max"] < a["min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _rope_train_rows(quick: bool, base, models):
    """(c) the training step's forward + backward (no optimiser), 4 x 2048 tokens: rotary against learned."""
    import torch
    Bt, T = (2, 512) if quick else (4, 2048)
    idx = torch.randint(0, base.vocab_size, (Bt, T), device="cuda")
    tgt = torch.randint(0, base.vocab_size, (Bt, T), device="cuda")

    def fb(p):
        def f(i):
            m = models[p].train()
            _, loss = m(idx, tgt)
            loss.backward()
            for q in m.parameters():
                q.grad = None
        return f

    r = _time_blocks({p: fb(p) for p in ("learned", "rope")}, blocks=5 if quick else 7, iters=3)
    row = {"model": f"{'gpt-small' if quick else 'gpt-1b'}", "B": Bt, "T": T, "what": "forward + backward", **r,
           "rope_minus_learned_us": r["rope"]["median_us"] - r["learned"]["median_us"],
           "separated": r["rope"]["max_us"] < r["learned"]["min_us"] or r["learned"]["max_us"] < r["rope"]["min_us"]}
    print(json.dumps(row), flush=True)
    return [row]


def step_rope(quick: bool):
    out = {"append": _rope_append_rows(quick)}
    base, models = _rope_models(quick)
    out["decode"] = _rope_decode_rows(quick, base, models)
    out["train"] = _rope_train_rows(quick, base, models)
    return out


GLU_FS = (8192, 5504)


def _glu_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.ops.gemm import _gemm_nt_swiglu
    from kubeflow_rm_amd.ops.swiglu import swiglu_fwd
    rows = []
    K = 2048
    for Fd in GLU_FS:
        N = 2 * Fd
        for fmt in ("bf16", "fp8"):
            ncopy = 2 if quick else max(2, -(-(512 << 20) // (N * K * (2 if fmt == "bf16" else 1))))
            ws = [torch.randn(N, K, device="cuda").mul_(0.02).to(torch.bfloat16) for _ in range(ncopy)]
            if fmt == "fp8":
                ws = [ops.quantize_weight(w) for w in ws]
            bias = torch.randn(N, device="cuda").to(torch.bfloat16)
            for M in GEMM_MS:
                a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
                out = torch.empty(M, Fd, device="cuda", dtype=torch.bfloat16)
                z = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)

                def glu(variant, tiles=0):
                    return lambda i: _gemm_nt_swiglu(a, ws[i % ncopy], bias, None, 1.0, out, variant, tiles)

                def two(i):
                    ops.gemm_nt(a, ws[i % ncopy], bias=bias, out=z, variant="skinny")
                    swiglu_fwd(z, out=out)

                fns = {"two_launch": two, "glu": glu("skinny"), "glu_mfma": glu("skinny_mfma"),
                       **{f"glu_mfma_t{t}": glu("skinny_mfma", t) for t in (1, 2, 4)}}
                if M <= 8:
                    fns.update({"glu_valu": glu("skinny_valu"), "glu_valu_r2": glu("skinny_valu", 2)})
                    if M <= 4:  # 8 activation rows always take 2 weight rows per wave
                        fns["glu_valu_r4"] = glu("skinny_valu", 4)
                r = _time_blocks(fns, blocks=5 if quick else 7, iters=ncopy)
                row = {"M": M, "F": Fd, "N": N, "K": K, "weights": fmt, "weight_copies": ncopy, **r}
                row["two_launch_over_glu"] = r["two_launch"]["median_us"] / r["glu"]["median_us"]
                row["separated"] = (r["glu"]["max_us"] < r["two_launch"]["min_us"]
                                    or r["two_launch"]["max_us"] < r["glu"]["min_us"])
                rows.append(row)
                print(json.dumps(row), flush=True)
            del ws
            torch.cuda.empty_cache()
    return rows


def _glu_model_rows(quick: bool):
    """Graphed (and eager) decode, ms/token around position 2048: the gated GEMM against the two-launch MLP."""
    import dataclasses
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    from kubeflow_rm_amd import ops
    name = "gpt-small" if quick else "gpt-1b"
    # 4 K / V heads under gpt-1b's 16 query heads; gpt-small has 12, and groups of 3 are no kernel instantiation: 6
    cfg = dataclasses.replace(CONFIGS[name], norm="rms", mlp="swiglu", pos="rope", n_kv_heads=6 if quick else 4)
    model = GPT(cfg, device="cuda").eval()
    rows = []
    prompt, new = 2048 - 64, 64
    for B in (1, 16):
        idx = torch.randint(0, cfg.vocab_size, (B, prompt), device="cuda")
        toks = torch.randint(0, cfg.vocab_size, (new, B), device="cuda")

        def run(form, mode):
            if form != "fused":  # shadow GPT._fc1 on this instance: ungated GEMM to [rows, 2 d_ff], then the gate kernel
                model._fc1 = lambda lin, y, w, blk: ops.swiglu(lin(y, w, blk.fc1.bias))
            try:
                cache = model.new_cache(B, prompt + new)
                model.prefill(idx, cache)
                step = (lambda t: model.decode_step(t, cache)) if mode != "graph" else model.graphed_decode_step(cache)
                step(toks[0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(1, new):
                    step(toks[i])
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / (new - 1)
            finally:
                model.__dict__.pop("_fc1", None)

        keys = [(f, mode) for mode in ("graph", "eager") for f in ("two", "fused")]
        res = {k: [] for k in keys}
        for _ in range(3 if quick else 7):  # interleaved
            for k in keys:
                res[k].append(run(*k))
        row = {"model": f"{name} rms / swiglu / rope / {cfg.n_kv_heads} kv heads", "B": B, "prompt": prompt, "new": new}
        for (f, mode), v in res.items():
            row[f"{f}_{mode}"] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
        for mode in ("graph", "eager"):
            a, b = row[f"fused_{mode}"], row[f"two_{mode}"]
            row[f"two_over_fused_{mode}"] = b["ms_per_token"] / a["ms_per_token"]
            row[f"separated_{mode}"] = a["max"] < b["min"] or b["max"] < a["min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _glu_rmsnorm_rows(quick: bool):
    """RMSNorm backward with the residual gradient, 8192 x 2048: the kernel against the torch arithmetic it replaced."""
    import torch
    from kubeflow_rm_amd import ops
    rows_, H = (1024, 2048) if quick else (8192, 2048)
    x = torch.randn(rows_, H, device="cuda").to(torch.bfloat16)
    w = torch.ones(H, device="cuda", dtype=torch.bfloat16)
    gy, gr = (torch.randn(rows_, H, device="cuda").to(torch.bfloat16) for _ in range(2))
    _, rstd = ops.rms_norm_fwd(x, w, 1e-6, save_stats=True)

    def torch_bwd(i):  # the previous _RMSNorm.backward, plus autograd's add of the residual gradient
        r = rstd.unsqueeze(-1)
        xhat = x.float() * r
        gyf = gy.float()
        gdy = gyf * w.float()
        dx = (r * (gdy - xhat * (gdy * xhat).mean(-1, keepdim=True))).to(torch.bfloat16) + gr
        return dx, (gyf * xhat).sum(0).to(torch.bfloat16)

    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y, r = ops.rms_norm_residual(xg, wg, 1e-6)

    def kernel_bwd(i):
        torch.autograd.backward([y, r], [gy, gr], retain_graph=True)
        xg.grad = wg.grad = None

    t = _time_blocks({"torch": torch_bwd, "kernel": kernel_bwd}, blocks=5 if quick else 7, iters=10)
    row = {"op": "rmsnorm backward + dres", "rows": rows_, "hidden": H, **t,
           "torch_over_kernel": t["torch"]["median_us"] / t["kernel"]["median_us"]}
    print(json.dumps(row), flush=True)
    return [row]


def step_glu(quick: bool):
    return {"kernel": _glu_kernel_rows(quick), "rmsnorm_bwd": _glu_rmsnorm_rows(quick), "model": _glu_model_rows(quick)}


def _window_kernel_rows(quick: bool):
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    H, D, cap, n = 16, 128, 4096, 4096
    blocks = 5 if quick else 7
    for B in (1, 8):
        caches, ncopy = _gqa_caches(B, H, H, D, cap, quick)
        shapes = {"decode": (B, H, D), "extend_T4": (B, 4, H, D), "chunk_T128": (B, 128, H, D)}
        calls = {"decode": ops.attention_decode, "extend_T4": ops.attention_extend, "chunk_T128": ops.attention_chunk}
        for kind, c in caches.items():
            c.set_lens([n] * B)
            for name, shape in shapes.items():
                q = torch.randn(*shape, device="cuda").to(torch.bfloat16)
                out = torch.empty_like(q)
                fn = calls[name]
                fns = {"none": (lambda i: fn(q, c, i % ncopy, out=out, t_bound=n))}
                for W in WINDOW_WS:
                    fns[f"W{W}"] = (lambda i, W=W: fn(q, c, i % ncopy, out=out, t_bound=n, window=W))
                r = _time_blocks(fns, blocks=blocks, iters=20)
                row = {"op": name, "kind": kind, "B": B, "H": H, "D": D, "len": n, "cache_copies": ncopy, "none": r["none"]}
                for W in WINDOW_WS:
                    t = r[f"W{W}"]
                    sep = _sep({"min": t["min_us"], "max": t["max_us"]},
                               {"min": r["none"]["min_us"], "max": r["none"]["max_us"]})
                    row[f"W{W}"] = {**t, "none_over_this": r["none"]["median_us"] / t["median_us"], "separated": sep}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del caches
        torch.cuda.empty_cache()
    return rows


def _window_model_rows(quick: bool):
    import dataclasses
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    rows = []
    base = CONFIGS["gpt-small" if quick else "gpt-1b"]
    new = 64
    prompt = base.max_seq - 2 * new
    models = {"none": GPT(base, device="cuda").eval(),
              "W1024": GPT(dataclasses.replace(base, window=1024), device="cuda").eval()}
    for B in (1, 8):
        idx = torch.randint(0, base.vocab_size, (B, prompt), device="cuda")
        toks = torch.randint(0, base.vocab_size, (new, B), device="cuda")

        def run(key):
            model = models[key]
            cache = model.new_cache(B, prompt + new)
            model.prefill(idx, cache)
            step = model.graphed_decode_step(cache)
            step(toks[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(1, new):
                step(toks[i])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (new - 1)

        res = {k: [] for k in models}
        for _ in range(3 if quick else 7):  # interleaved
            for k in models:
                res[k].append(run(k))
        row = {"model": "gpt-small" if quick else "gpt-1b", "B": B, "position": f"{prompt + 1} .. {prompt + new - 1}",
               "mode": "graph"}
        for k, v in res.items():
            row[k] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
        row["none_over_W1024"] = row["none"]["ms_per_token"] / row["W1024"]["ms_per_token"]
        row["separated"] = _sep(row["none"], row["W1024"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


RING_WS = (256, 1024)
RING_FAR = 2 ** 20 + 5


def _ring_kernel_rows(quick: bool):
    """Ring against the flat windowed launch at the same position and W, and the ring at a position no flat cache
    reaches: three candidates interleaved per cell. Both read the same keys; the ring's grid comes from W and T."""
    import torch
    from kubeflow_rm_amd import ops
    rows = []
    H, D, cap, n = 16, 128, 4096, 4000
    blocks = 5 if quick else 7
    shapes = {"decode": (1, lambda B: (B, H, D)), "extend_T4": (4, lambda B: (B, 4, H, D)),
              "chunk_T128": (128, lambda B: (B, 128, H, D))}
    calls = {"decode": ops.attention_decode, "extend_T4": ops.attention_extend, "chunk_T128": ops.attention_chunk}
    for B in (1, 8):
        flats, ncopy = _gqa_caches(B, H, H, D, cap, quick)
        near = torch.full((B,), n, device="cuda", dtype=torch.int32)
        far = torch.full((B,), RING_FAR, device="cuda", dtype=torch.int32)
        for W in RING_WS:
            C = -(-(W + 128 - 1) // 256) * 256  # the largest step here is 128 tokens
            for kind, flat in flats.items():
                flat.set_lens([n] * B)
                ring = ops.KVCache(ncopy, B, H, D, C, device="cuda", dtype=flat.dtype, ring=True, window=W)
                for layer in range(ncopy):  # every slot holds a finite row
                    ring.reset()
                    for t0 in range(0, C, 256):
                        ops.kv_append(torch.randn(B, 256, 3 * H * D, device="cuda").to(torch.bfloat16), ring, layer)
                        ring.advance(256)
                for name, (T, shape) in shapes.items():
                    q = torch.randn(*shape(B), device="cuda").to(torch.bfloat16)
                    out = torch.empty_like(q)
                    fn = calls[name]
                    fns = {"flat": (lambda i: fn(q, flat, i % ncopy, out=out, t_bound=n, window=W)),
                           "ring": (lambda i: fn(q, ring, i % ncopy, out=out, lens=near, window=W)),
                           "ring_far": (lambda i: fn(q, ring, i % ncopy, out=out, lens=far, window=W))}
                    r = _time_blocks(fns, blocks=blocks, iters=20)
                    mm = {k: {"min": v["min_us"], "max": v["max_us"]} for k, v in r.items()}
                    row = {"op": name, "kind": kind, "B": B, "H": H, "D": D, "W": W, "position": n, "ring_capacity": C,
                           "far_position": RING_FAR, "cache_copies": ncopy, **r,
                           "flat_over_ring": r["flat"]["median_us"] / r["ring"]["median_us"],
                           "ring_vs_flat_separated": _sep(mm["ring"], mm["flat"]),
                           "far_over_near": r["ring_far"]["median_us"] / r["ring"]["median_us"],
                           "far_vs_near_separated": _sep(mm["ring_far"], mm["ring"])}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del ring
        del flats
        torch.cuda.empty_cache()
    return rows


def _ring_model_rows(quick: bool):
    """A graphed decode step of the windowed model at position about 4000 (about 2000 with --quick), on a flat cache
    (pinned bound) against a ring, interleaved runs: ms/token."""
    import dataclasses
    import torch
    from kubeflow_rm_amd.models import CONFIGS, GPT
    rows = []
    base = CONFIGS["gpt-small" if quick else "gpt-1b"]
    W, new = (256 if quick else 1024), 64
    prompt = base.max_seq - 2 * new
    model = GPT(dataclasses.replace(base, window=W), device="cuda").eval()
    for B in (1, 8):
        idx = torch.randint(0, base.vocab_size, (B, prompt), device="cuda")
        toks = torch.randint(0, base.vocab_size, (new, B), device="cuda")
        nbytes = {}

        def run(key):
            if key == "flat":
                cache = model.new_cache(B, prompt + new)
            else:
                cache = model.new_cache(B, model._ring_capacity(256), ring=True)
            model.extend(idx, cache, last_only=True, chunk=256)  # the same prompt path for both
            step = model.graphed_decode_step(cache)
            step(toks[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(1, new):
                step(toks[i])
            torch.cuda.synchronize()
            nbytes[key] = cache.nbytes
            return (time.perf_counter() - t0) * 1e3 / (new - 1)

        res = {"flat": [], "ring": []}
        for _ in range(3 if quick else 7):  # interleaved
            for k in res:
                res[k].append(run(k))
        row = {"model": "gpt-small" if quick else "gpt-1b", "B": B, "W": W, "mode": "graph",
               "position": f"{prompt + 1} .. {prompt + new - 1}", "nbytes": dict(nbytes)}
        for k, v in res.items():
            row[k] = {"ms_per_token": statistics.median(v), "min": min(v), "max": max(v)}
        row["flat_over_ring"] = row["flat"]["ms_per_token"] / row["ring"]["ms_per_token"]
        row["separated"] = _sep(row["flat"], row["ring"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _ring_nbytes_rows():
    """K / V bytes of a flat cache and of a ring for gpt-1b shapes at max_seq = 32768, W = 4096 (a ring of 4352 slots:
    steps of up to 256 tokens), from ``KVCache.nbytes`` of caches built on the meta device (nothing is allocated; the
    attention workspaces, allocated on first use on a GPU, are not in these figures)."""
    from kubeflow_rm_amd import ops
    from kubeflow_rm_amd.models import CONFIGS
    c = CONFIGS["gpt-1b"]
    rows = []
    W, max_seq = 4096, 32768
    C = -(-(W + 256 - 1) // 256) * 256
    for B in (1, 16):
        flat = ops.KVCache(c.n_layers, B, c.kv_heads, c.head_dim, max_seq, device="meta")
        ring = ops.KVCache(c.n_layers, B, c.kv_heads, c.head_dim, C, device="meta", ring=True, window=W)
        row = {"model": "gpt-1b", "B": B, "max_seq": max_seq, "W": W, "ring_capacity": C, "flat_nbytes": flat.nbytes,
               "ring_nbytes": ring.nbytes, "flat_over_ring": flat.nbytes / ring.nbytes,
               "bytes_per_position_and_row": flat.nbytes // (B * max_seq)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_ring(quick: bool):
    return {"nbytes": _ring_nbytes_rows(), "kernel": _ring_kernel_rows(quick), "model": _ring_model_rows(quick)}


def step_window(quick: bool):
    return {"kernel": _window_kernel_rows(quick), "model": _window_model_rows(quick)}


STEPS = {"ring": step_ring, "window": step_window, "glu": step_glu, "rope": step_rope, "gqa": step_gqa,"chunk": step_chunk, "sample": step_sample, "gemm": step_gemm, "attn": step_attn, "e2e": step_e2e, "extend": step_extend, "kv8": step_kv8, "w8": step_w8}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="decode_bench.json")
    ap.add_argument("--steps", default="gemm,attn,e2e,extend")
    ap.add_argument("--quick", action="store_true", help="fewer blocks / shapes (a smoke run of the tool)")
    ap.add_argument("--child", choices=sorted(STEPS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:  # one step, in a process of its own
        Path(args.out).write_text(json.dumps(STEPS[args.child](args.quick)))
        return 0
    result = {}
    part = Path(args.out + ".part")
    for name in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, str(Path(__file__).resolve()),
               "--child", name, "--out", str(part), *(["--quick"] if args.quick else [])]
        rc = subprocess.run(cmd).returncode  # the child's rows stream to this process's stdout
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping", file=sys.stderr)
            Path(args.out).write_text(json.dumps(result, indent=1))
            return rc
        result[name] = json.loads(part.read_text())
        part.unlink()
        Path(args.out).write_text(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
