#!/usr/bin/env python3
"""Compare the kernels of two builds instruction for instruction, and list a build's VGPR counts.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I kernels --cuda-device-only -S kernels/attn_kv.hip -o new/attn_kv.s
    (the same for the other revision into old/)
    python tools/kernel_isa_diff.py old new [--vgprs SUBSTRING]

Every kernel of ``old/*.s`` is looked up in ``new/*.s`` by its demangled name, also with one more trailing ``false``
template argument (a kernel that gained a compile-time flag), and the two instruction streams are compared with labels
and symbol names normalised. Prints the kernels that differ or are missing and the count compared / identical; exits 1
when any differs. ``--vgprs S``: also print ``.amdhsa_next_free_vgpr`` of the new build's kernels whose name holds S."""
import re
import subprocess
import sys
from pathlib import Path


def functions(path):
    out, cur = {}, None
    for ln in Path(path).read_text().splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if ln.startswith("\t.end_amdhsa_kernel") or re.match(r"^\.Lfunc_end", ln):
            cur = None
            continue
        s = re.sub(r";.*", "", ln).strip()
        if not s or s.startswith("."):
            continue
        out[cur].append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", s)))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    out = []
    for d in res.stdout.splitlines():  # the name with its template arguments, without return type and parameter list
        d = re.sub(r"\s+", "", d.replace("(anonymous namespace)::", ""))
        out.append(re.sub(r"^void", "", d.split("(")[0]))
    return out


def vgprs(path):
    out, cur = {}, None
    for ln in Path(path).read_text().splitlines():
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        cur = m.group(1) if m else cur
        m = re.match(r"\s*\.amdhsa_next_free_vgpr (\d+)", ln)
        if m and cur:
            out[cur] = int(m.group(1))
    return out


def main():
    old_dir, new_dir = Path(sys.argv[1]), Path(sys.argv[2])
    want = sys.argv[sys.argv.index("--vgprs") + 1] if "--vgprs" in sys.argv else None
    total = same = 0
    for old_s in sorted(old_dir.glob("*.s")):
        new_s = new_dir / old_s.name
        if not new_s.exists():
            print(f"missing file {new_s}")
            continue
        old, new = functions(old_s), functions(new_s)
        by_name = dict(zip(demangle(list(new)), new))
        for name, key in zip(demangle(list(old)), old):
            flagged = name[:-1] + ",false>" if name.endswith(">") else name + "<false>"
            hit = by_name.get(name) or by_name.get(flagged)
            if hit is None:  # a name c++filt does not know (a __bf16 parameter): the flag in the mangled name
                alt = key.replace("EEEv", "ELb0EEEv", 1)
                hit = alt if alt in new else None
            total += 1
            if hit is not None and new[hit] == old[key]:
                same += 1
            else:
                print(f"{old_s.name}: {name}: {'missing' if hit is None else 'differs'}")
        if want is not None:
            v = vgprs(new_s)
            for name, key in sorted(zip(demangle(list(v)), v)):
                if want in name:
                    print(f"{old_s.name}: {name}: {v[key]} VGPRs")
    print(f"compared {total}, identical {same}")
    return 0 if total == same else 1


if __name__ == "__main__":
    sys.exit(main())
