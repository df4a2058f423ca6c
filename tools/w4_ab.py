#!/usr/bin/env python3
"""A/B of the w4 GEMM header (kernels/gemm_w4.h) on one GPU: tools/w4_ab.hip built once per variant.
`prod` is the working tree's kernels/, `head` the committed kernels/ (git HEAD, extracted into the
build directory), which is how an experiment on the header is measured against what is committed:
edit kernels/gemm_w4.h, build both, run. The header has no build knobs; a schedule that is to be
tried is written into the working tree.

  python tools/w4_ab.py --build            # on the host: compile both variants into kubeflow_rm_amd/lib/w4ab/
  python tools/w4_ab.py --sizes 4096,8192   # on the GPU: bitwise check vs the loaded kernel library, interleaved
                                            # timing rounds vs that library (`ops`) and torch.matmul, then the
                                            # variants' cheap K-loop stamps (cycles per 64-k tile by segment)

Prints one JSON line per measurement. Every variant carries KFW4_CHEAP_STAMPS=1, which only touches its
diag kernel (s_memtime with no wait of its own, read after the loop's own lgkmcnt(0)).
"""
import argparse
import ctypes
import io
import json
import statistics
import subprocess
import sys
import tarfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "kubeflow_rm_amd" / "lib" / "w4ab"

VARIANTS = {"prod": None, "head": "HEAD"}  # name -> git revision of kernels/ (None: the working tree)


def build(names):
    from concurrent.futures import ThreadPoolExecutor
    OUT.mkdir(parents=True, exist_ok=True)

    def one(name):
        so = OUT / f"libw4ab_{name}.so"
        kernels = ROOT / "kernels"
        if VARIANTS[name]:  # the committed kernels/ of that revision, extracted beside the libraries
            tar = subprocess.run(["git", "-C", str(ROOT), "archive", VARIANTS[name], "kernels"],
                                 capture_output=True, check=True).stdout
            tarfile.open(fileobj=io.BytesIO(tar)).extractall(OUT / name)
            kernels = OUT / name / "kernels"
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-mcode-object-version=5", f"-I{kernels}", "-DKFW4_CHEAP_STAMPS=1",
               str(ROOT / "tools" / "w4_ab.hip"), "-o", str(so)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            raise SystemExit(f"{name}: {p.stderr[-2000:]}")
        nm = subprocess.run(["nm", "-D", "--undefined-only", str(so)], capture_output=True, text=True).stdout
        if "device_stub" in nm:  # hipcc 7.2 dropped the launch stubs (gemm_w4.h notes)
            raise SystemExit(f"{name}: launch stubs missing")
        return name
    with ThreadPoolExecutor(4) as ex:
        for n in ex.map(one, names):
            print("built", n, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--sizes", default="4096,8192,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--diag", default="8192")
    ap.add_argument("--launches", type=int, default=0,
                    help="profiling mode (under rocprofv3): only launch each variant N times at the first size, "
                         "in --variants order (the kernel name is the same in every library)")
    a = ap.parse_args()
    names = [v for v in a.variants.split(",") if v]
    if a.build:
        build(names)
        return
    import torch
    from kubeflow_rm_amd import ops
    vp, i = ctypes.c_void_p, ctypes.c_int
    libs = {}
    for n in names:
        L = ctypes.CDLL(str(OUT / f"libw4ab_{n}.so"))
        L.w4ab_nt.restype = i
        L.w4ab_nt.argtypes = [vp, vp, vp, i, i, i, vp]
        L.w4ab_diag.restype = i
        L.w4ab_diag.argtypes = [vp, vp, vp, i, i, i, vp, vp]
        libs[n] = L
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for spec in [x for x in a.sizes.split(",") if x]:
        # s (s^3) or MxNxK
        M, N, K = (int(v) for v in spec.split("x")) if "x" in spec else (int(spec),) * 3
        s = spec
        A = (torch.rand(M, K, device=dev) * 2 - 1).to(torch.bfloat16)
        B = (torch.rand(N, K, device=dev) * 2 - 1).to(torch.bfloat16)
        ref = ops.gemm_nt(A, B)
        C = torch.empty_like(ref)
        if a.launches:
            for n, L in libs.items():
                for _ in range(a.launches):
                    assert L.w4ab_nt(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, st) == 0
                torch.cuda.synchronize()
            print(json.dumps({"size": s, "launches": a.launches, "order": list(libs)}), flush=True)
            return
        same = {}
        for n, L in libs.items():
            assert L.w4ab_nt(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, st) == 0
            torch.cuda.synchronize()
            same[n] = bool(torch.equal(C, ref))
        flop = 2.0 * M * N * K
        iters = max(5, int(3e13 / flop))
        # `ops`: the kernel library the package loaded (KFAMD_KERNEL_LIB or the in-tree build)
        fns = {"ops": lambda: ops.gemm_nt(A, B, out=C), "torch": lambda: torch.matmul(A, B.t())}
        for n, L in libs.items():
            fns[n] = (lambda L=L: L.w4ab_nt(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, st))
        for fn in fns.values():  # first calls (hipBLASLt picks its algorithm) stay out of the rounds
            fn()
        torch.cuda.synchronize()
        t_end = time.perf_counter() + 1.0  # settle: 1 s of back-to-back GEMMs before round 1
        while time.perf_counter() < t_end:
            fns["ops"]()
        tf = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                tf[k].append(flop * iters / (time.perf_counter() - t0) / 1e12)
        print(json.dumps({"size": s, "bitwise_equal_to_ops": same,
                          "median_tf": {k: round(statistics.median(v), 1) for k, v in tf.items()},
                          "best_tf": {k: round(max(v), 1) for k, v in tf.items()},
                          # (max - min) / median of each build's own rounds: what a difference has to beat
                          "spread": {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in tf.items()},
                          "rounds_tf": {k: [round(x, 1) for x in v] for k, v in tf.items()}}), flush=True)
        del A, B, C, ref
    for spec in [x for x in a.diag.split(",") if x]:
        # s (s^3) or MxNxK: e.g. 1024x1024x8192 puts 16 blocks on 16 CUs (no chip-wide store burst)
        M_, N_, K_ = (int(v) for v in spec.split("x")) if "x" in spec else (int(spec),) * 3
        A = (torch.rand(M_, K_, device=dev) * 2 - 1).to(torch.bfloat16)
        B = (torch.rand(N_, K_, device=dev) * 2 - 1).to(torch.bfloat16)
        C = torch.empty(M_, N_, device=dev, dtype=torch.bfloat16)
        nblk = (M_ // 256) * (N_ // 256)
        diag = torch.zeros(nblk * 4 * 16, dtype=torch.int64, device=dev)
        nk = K_ // 64
        s = spec
        for n, L in libs.items():
            for _ in range(3):
                assert L.w4ab_diag(A.data_ptr(), B.data_ptr(), C.data_ptr(), M_, N_, K_, diag.data_ptr(), st) == 0
            torch.cuda.synchronize()
            d = diag.view(nblk, 4, 16).double()
            seg = (d[..., :4].sum(dim=(0, 1)) / (nblk * 4 * (nk - 1))).tolist()  # cycles per 64-k tile
            clk = ((d[:, 0, 7]) / (d[:, 0, 9] - d[:, 0, 8]).clamp(min=1) * 100).median().item()
            print(json.dumps({"diag_size": s, "variant": n,
                              "cycles_per_ktile": {"substep0": round(seg[0]), "mid_wait_barrier": round(seg[1]),
                                                   "substep1": round(seg[2]), "end_wait_rotate": round(seg[3]),
                                                   "total": round(sum(seg))},
                              "prologue_cycles": round(d[..., 4].mean().item()),
                              "epilogue_cycles": round(d[..., 5].mean().item()),
                              "block_cycles": round(d[..., 7].mean().item()), "clock_mhz_median": round(clk)}),
                  flush=True)


if __name__ == "__main__":
    main()
