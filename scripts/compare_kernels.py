#!/usr/bin/env python
"""Kernel by kernel, what a source change did to the gfx950 device code of two builds of betty_amd/csrc.

    python scripts/compare_kernels.py OTHER_CSRC [--object bhg_vector.o] [--markdown]

OTHER_CSRC is the betty_amd/csrc directory of another checkout that was built with `make` (its build/ and build_ab/).
For every object of both builds: whether the device code (.hip_fatbin) is byte-identical.  For the kernels of --object:
the resource notes (VGPR / AGPR / SGPR counts, LDS and scratch bytes, spill counts) and the per-opcode instruction counts of
`llvm-objdump -d`, with s_nop and s_waitcnt set aside (they move with instruction order alone).  A refactor that keeps the
arithmetic and the access pattern shows equal notes and equal counts for every opcode; exit status 1 otherwise.
"""
import argparse
import collections
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count")
SET_ASIDE = ("s_nop", "s_waitcnt")


def fatbin(obj, tmp):
    fat = os.path.join(tmp, "fat")
    if os.path.exists(fat):
        os.remove(fat)
    if not os.path.exists(obj):
        return None
    r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    return open(fat, "rb").read()


def demangle(names):
    out = list(names)
    for tool in (f"{LLVM}/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.check_output([tool] + list(names), text=True).splitlines()
            break
        except OSError:
            continue
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void bhg::\(anonymous namespace\)::", "", d)
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        short[n] = re.sub(r"\(.*$", "", d)   # drop the argument list
    return short


def kernels(obj, tmp):
    """{mangled name: (notes dict, Counter of opcodes)} of the object's gfx950 code object."""
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    if fatbin(obj, tmp) is None:   # (leaves the section in `fat`)
        sys.exit(f"compare_kernels: no device code in {obj}")
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}",
                           f"--output={co}"])
    # a kernel's keys come in alphabetical order: .agpr_count opens its entry, .name sits in the middle, .vgpr_spill_count is
    # the last one wanted here
    notes, name, cur = {}, None, {}
    for line in subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True).splitlines():
        s = line.strip().lstrip("- ").strip()
        if s.startswith(".agpr_count:"):
            name, cur = None, {}
        if s.startswith(".name:") and line.startswith("    .name:"):   # (deeper .name lines belong to the arguments)
            name = s.split(":", 1)[1].strip()
        for key in NOTE_KEYS:
            if s.startswith(key + ":"):
                cur[key] = int(s.split(":", 1)[1])
        if s.startswith(".vgpr_spill_count:") and name is not None:
            notes[name] = cur
    seq, cur = {}, None
    for line in subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", co], text=True).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            seq.setdefault(cur, [])
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            seq[cur].append(line.split()[0])
    ops = {}
    for n, s in seq.items():   # what follows the last s_endpgm is padding (zero words disassemble as instructions or "...")
        last = max((i for i, o in enumerate(s) if o == "s_endpgm"), default=len(s) - 1)
        ops[n] = collections.Counter(s[:last + 1])
    return {n: (notes[n], ops.get(n, collections.Counter())) for n in notes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--object", default="bhg_vector.o")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    here = os.path.join(ROOT, "betty_amd", "csrc")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for build in ("build", "build_ab"):
            print(f"## {build}: device code of every object, other against this tree")
            for o in sorted(glob.glob(os.path.join(here, build, "*.o"))):
                base = os.path.basename(o)
                a, b = fatbin(os.path.join(args.other, build, base), tmp), fatbin(o, tmp)
                if a is None and b is None:
                    continue
                same = a == b
                ha, hb = (hashlib.sha256(d).hexdigest()[:16] if d is not None else "(none)".ljust(16) for d in (a, b))
                print(f"{base:22s} {ha} {hb} {'identical' if same else 'DIFFERENT'}")
                if not same and base != args.object:
                    bad += 1
            ka = kernels(os.path.join(args.other, build, args.object), tmp)
            kb = kernels(os.path.join(here, build, args.object), tmp)
            if set(ka) != set(kb):
                print("kernel symbols differ:", sorted(set(ka) ^ set(kb)))
                bad += 1
            short = demangle(sorted(set(ka) | set(kb)))
            print(f"\n## {build}/{args.object}: {len(kb)} kernels (other -> this where they differ)")
            sep = " | " if args.markdown else "  "
            head = ["kernel", "vgpr", "agpr", "sgpr", "lds", "scratch", "vspill", "sspill", "instr", "opcodes that differ"]
            if args.markdown:
                print("| " + sep.join(head) + " |\n|" + "---|" * len(head))
            else:
                print(sep.join(head))
            for n in sorted(set(ka) & set(kb), key=lambda n: short[n]):
                (na, oa), (nb, ob) = ka[n], kb[n]
                cells = [short[n]]
                for key in NOTE_KEYS:
                    va, vb = na.get(key), nb.get(key)
                    cells.append(str(vb) if va == vb else f"{va}->{vb}")
                    bad += va != vb
                ca = sum(v for k, v in oa.items() if k not in SET_ASIDE)
                cb = sum(v for k, v in ob.items() if k not in SET_ASIDE)
                cells.append(str(cb) if ca == cb else f"{ca}->{cb}")
                diff = [f"{k} {oa[k]}->{ob[k]}" for k in sorted(set(oa) | set(ob)) if oa[k] != ob[k]]
                counted = [d for d in diff if d.split()[0] not in SET_ASIDE]
                bad += len(counted)
                cells.append(", ".join(diff) if diff else "none")
                print(("| " + sep.join(cells) + " |") if args.markdown else sep.join(cells))
            print()
    print("compare_kernels:", "equal notes and opcode counts" if not bad else f"{bad} difference(s)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
