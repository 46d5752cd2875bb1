#!/usr/bin/env python3
"""Instruction counts of the march kernels' loops, from the compiler's assembly.

Compiles percolation_amd/csrc/perc_solve.hip to gfx950 assembly with the
library's own flags (hipcc --cuda-device-only -S; no GPU needed) and prints,
for each named k_cg_march instantiation, the kernel's VGPRs, SGPRs, LDS bytes,
ScratchSize and occupancy as the compiler reports them, and for every loop
(a label that a later branch jumps back to) its instructions by class:

  VALU   v_*            of these: cndmask (v_cndmask*), fp64 (v_*_f64)
  SALU   s_* other than the three classes below (branches included)
  SMEM   s_load*, s_buffer_load*
  waits  s_waitcnt*
  LDS    ds_*
  VMEM   buffer_*, global_*, flat_*, scratch_*

Classes go by mnemonic prefix and nothing else.  A loop's count is every
instruction between its label and its back branch: all paths through the
body, taken or not, and inner loops' instructions too (inner loops are
indented).  The walk loops hold D steps (the kernel's third template
argument): divide by D for one step.  The open-lattice
instantiations (last template argument true) hold the open-square path
alone, so a walk loop's count is D steps of it.  The strip-major nibble
kernels with the last argument false run under pbc and hold the
run-time-mask, map and general paths.

  python tools/march_isa.py                       # the default kernels
  python tools/march_isa.py -D PERC_MARCH_DYNMASK # the run-time mask (also: PERC_MARCH_FIRST_RT)
  python tools/march_isa.py --kernel '<1, true, 3, 2, false, true, true, false, 0, true>'
  python tools/march_isa.py --asm perc_solve.s    # an assembly file made before
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "percolation_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

# k_cg_march<MODE, SM, D, PAUX, TR, TAG, PK, LIT, ESR, OPEN>: the L = 4096
# pair (strip-major, nibble codes, tagged, open lattice), its pbc pair and the
# L = 8192 pair (row-major, nibble codes)
DEFAULT = [
    ("strip-major P", r"k_cg_march<1, true, 3, 2, false, true, true, false, 0, true>"),
    ("strip-major B", r"k_cg_march<2, true, 3, 2, false, true, true, false, 64, true>"),
    ("strip-major P, pbc", r"k_cg_march<1, true, 3, 2, false, true, true, false, 0, false>"),
    ("strip-major B, pbc", r"k_cg_march<2, true, 3, 2, false, true, true, false, 64, false>"),
    ("row-major nibble P", r"k_cg_march<1, false, 2, 0, false, false, true, false, 0, false>"),
    ("row-major nibble B", r"k_cg_march<2, false, 2, 2, false, false, true, false, 16, false>"),
]

CLASSES = ("VALU", "cndmask", "fp64", "SALU", "SMEM", "waits", "LDS", "VMEM")


def classify(mn):
    """classes of one mnemonic (by prefix)"""
    if mn.startswith("v_"):
        c = ["VALU"]
        if mn.startswith("v_cndmask"):
            c.append("cndmask")
        if mn.endswith("_f64") or "_f64_" in mn:
            c.append("fp64")
        return c
    if mn.startswith("s_waitcnt"):
        return ["waits"]
    if mn.startswith("s_load") or mn.startswith("s_buffer_load"):
        return ["SMEM"]
    if mn.startswith("s_"):
        return ["SALU"]
    if mn.startswith("ds_"):
        return ["LDS"]
    if mn.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return ["VMEM"]
    return []


def hipflags():
    """HIPFLAGS of the library's Makefile (without the include path)"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, re.M)
    flags = m.group(1).replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if not f.startswith("-I")]


def compile_asm(src_dir, defines, out):
    cmd = [os.path.join(ROCM, "bin", "hipcc")] + hipflags() + ["-I", os.path.join(src_dir, "..", "..", "include")]
    cmd += ["-D" + d for d in defines]
    cmd += ["--cuda-device-only", "-S", os.path.join(src_dir, "perc_solve.hip"), "-o", out]
    subprocess.run(cmd, check=True)


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or os.path.join(ROCM, "lib", "llvm", "bin", "llvm-cxxfilt")
    r = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def functions(path):
    """mangled kernel name -> (body lines, the comment lines after its end)"""
    out, name, body, tail = {}, None, [], None
    for line in open(path):
        s = line.rstrip("\n")
        m = re.match(r"^(_Z\w+):", s)
        if m:
            if name is not None and tail is not None:
                out[name] = (body, tail)
            name, body, tail = m.group(1), [], None
        elif name is None:
            continue
        elif tail is None:
            if s.startswith(".Lfunc_end"):
                tail = []
            else:
                body.append(s)
        elif s.strip().startswith(";"):
            tail.append(s.strip())
    if name is not None and tail is not None:
        out[name] = (body, tail)
    return out


def loops(body):
    """[(label, first line, last line, counts)] of the function's loops"""
    label_at, insts = {}, []
    for i, s in enumerate(body):
        t = s.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label_at[m.group(1)] = i
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        insts.append((i, t.split()[0], t))
    found = {}
    for i, mn, t in insts:
        if mn.startswith("s_cbranch") or mn == "s_branch":
            tgt = t.split()[-1]
            if tgt in label_at and label_at[tgt] < i:
                lo = label_at[tgt]
                found[tgt] = (lo, max(i, found.get(tgt, (0, 0))[1]))
    res = []
    for lab, (lo, hi) in sorted(found.items(), key=lambda kv: kv[1]):
        cnt = dict.fromkeys(CLASSES, 0)
        cnt["all"] = 0
        for i, mn, _ in insts:
            if lo < i <= hi:
                cnt["all"] += 1
                for c in classify(mn):
                    cnt[c] += 1
        res.append((lab, lo, hi, cnt))
    return res


def meta(tail):
    keys = ("NumVgprs", "NumAgprs", "TotalNumVgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
    out = {}
    for s in tail:
        m = re.match(r"^;\s*(\w+):\s*(\d+)", s)
        if m and m.group(1) in keys:
            out[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=CSRC, help="the csrc directory to compile (default: this tree's)")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra macro of the compile")
    ap.add_argument("--kernel", action="append", default=[],
                    help="substring of a demangled kernel name (default: the default march kernels)")
    ap.add_argument("--keep", default=None, help="also write the assembly to this file")
    ap.add_argument("--min", type=int, default=150, help="skip loops of fewer instructions")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if not path:
            path = os.path.join(tmp, "perc_solve.s")
            compile_asm(a.src, a.defines, path)
            if a.keep:
                shutil.copyfile(path, a.keep)
        fns = functions(path)
    names = demangle(list(fns))
    want = [(k, k) for k in a.kernel] or DEFAULT
    print("# march_isa: %s" % ("assembly file " + a.asm if a.asm else "defines " + (" ".join(a.defines) or "(none)")))
    missing = 0
    for title, pat in want:
        hits = [n for n in fns if pat in names[n]]
        if not hits:
            print("%s: no kernel matches %s" % (title, pat))
            missing += 1
        for n in hits:
            body, tail = fns[n]
            m = meta(tail)
            print("%s: %s" % (title, re.sub(r"\(.*", "", names[n].replace("perc::(anonymous namespace)::", "").replace("void ", ""))))
            print("  " + "  ".join("%s %d" % kv for kv in m.items()))
            ls = loops(body)
            for lab, lo, hi, cnt in ls:
                if cnt["all"] < a.min:
                    continue
                depth = sum(1 for _, l2, h2, _ in ls if l2 <= lo and hi <= h2) - 1
                print("  %sloop %-10s lines %5d-%5d  all %4d | " % ("  " * depth, lab, lo, hi, cnt["all"])
                      + "  ".join("%s %d" % (c, cnt[c]) for c in CLASSES))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
