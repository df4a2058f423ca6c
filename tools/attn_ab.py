#!/usr/bin/env python3
"""Flash-attention build A/B: the kernel library re-linked with another build of kernels/attention_bf16.hip,
one library per variant (kubeflow_rm_amd/lib/attnab/): `prod` is the working tree under the production
flags, `head` the committed source (git HEAD) under the same flags, which is how an experiment on the
kernel file is measured against what is committed, and `agprform` the working tree without the MFMA
VGPR-form flag.

  python tools/attn_ab.py --build [--variants a,b]   # host: compile + link every variant
  KFAMD_KERNEL_LIB=kubeflow_rm_amd/lib/attnab/libkfamd_kernels_<v>.so python tools/attn_bench.py ...

The GPU side is the ordinary tooling with ``KFAMD_KERNEL_LIB`` pointing at a variant (ops/_lib.py), so
a variant runs the same numerics tests and the same interleaved bench as production
(tools/runs/r5n_attn_ab.sh).
"""
from __future__ import annotations

import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "kubeflow_rm_amd" / "lib" / "attnab"


def _variants():
    from kubeflow_rm_amd import _build as B
    prod = B.TU_FLAGS.get("attention_bf16.hip", [])
    return {
        "prod": prod,  # the working tree with the production flags
        "head": prod,  # git HEAD's attention source with the production flags
        # the compiler's default AGPR form: S / dP shuttled through v_accvgpr moves
        "agprform": [],
    }


VARIANTS = _variants()


def build(names):
    from kubeflow_rm_amd import _build as B
    B.build_kernels()
    # the objects of the current sources (build/kernels also keeps objects of retired ones)
    srcs = sorted(B.KERNEL_DIR.glob("*.hip")) + sorted((B.KERNEL_DIR / "tu").glob("*.hip"))
    others = [B.BUILD_DIR / "kernels" / (s.stem + ".o") for s in srcs if s.stem != "attention_bf16"]
    OUT.mkdir(parents=True, exist_ok=True)
    for n in names:
        obj = OUT / f"attention_bf16_{n}.o"
        src = B.KERNEL_DIR / "attention_bf16.hip"
        if n == "head":  # the committed source (git HEAD), for an A/B against the working tree
            src = OUT / "attention_bf16_head.hip"
            src.write_text(subprocess.run(["git", "-C", str(ROOT), "show", "HEAD:kernels/attention_bf16.hip"],
                                          capture_output=True, text=True, check=True).stdout)
        subprocess.run([B.HIPCC, *B.HIP_FLAGS, *VARIANTS[n], "-I", str(B.KERNEL_DIR), "-c", str(src), "-o", str(obj)],
                       check=True)
        lib = OUT / f"libkfamd_kernels_{n}.so"
        subprocess.run([B.HIPCC, f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", str(lib), str(obj),
                        *map(str, others)], check=True)
        B.check_kernel_library(lib)
        print("built", lib.relative_to(ROOT), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    a = ap.parse_args()
    names = [v for v in a.variants.split(",") if v]
    if a.build:
        build(names)


if __name__ == "__main__":
    main()
