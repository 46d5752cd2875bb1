#!/usr/bin/env python3
"""Are k_batch_clusters' plain instantiations the instructions they were?
Two device assembly listings of perc_batch_clusters.hip (one per tree):

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Iinclude \\
        --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \\
        percolation_amd/csrc/perc_batch_clusters.hip -o TREE.s 2> TREE.res

  python tools/cluster_isa_diff.py PARENT.s THIS.s [PARENT.res THIS.res]

Per (threads, kind) of the instantiations without the geometry: the body from
the symbol's label to its .Lfunc_end, with the symbol's own name, the basic
block labels' function number and every comment normalised, compared line for
line; with the two resource listings, their remarks too.  Exit status: the
number of instantiations that differ."""
import difflib
import re
import sys

SYM = r"_ZN4perc12_GLOBAL__N_116k_batch_clustersILi(\d+)ELi(\d)E(?:Lb([01])E)?"


def kernels(path):
    out = {}
    txt = open(path).read()
    for m in re.finditer(r"^(" + SYM + r"[^\n:]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S):
        name, nt, kd, geom, body = m.groups()
        if geom == "1":
            continue
        body = body.replace(name, "KERNEL")
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
        body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)
        out[(int(nt), int(kd))] = [ln for ln in body.splitlines() if ln.strip()]
    return out


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*) \[-Rpass", line)
        if not m:
            continue
        f = re.match(r"\s*Function Name: (\S+)", m.group(1))
        if f:
            g = re.search(SYM, f.group(1))
            cur = (int(g.group(1)), int(g.group(2))) if g and g.group(3) != "1" else None
            if cur:
                out[cur] = []
        elif cur:
            out[cur].append(m.group(1).strip())
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    assert sorted(a) == sorted(b) and len(a) == 9, (sorted(a), sorted(b))
    ra, rb = (remarks(sys.argv[3]), remarks(sys.argv[4])) if len(sys.argv) > 4 else ({}, {})
    bad = 0
    for k in sorted(a):
        d = list(difflib.unified_diff(a[k], b[k], lineterm="", n=0))
        same = not d and ra.get(k) == rb.get(k)
        bad += not same
        print("threads %4d kind %d: %d lines, %s%s" % (k[0], k[1], len(a[k]), "identical" if not d else "DIFFERENT",
                                                       "" if not ra else ", resources " +
                                                       ("identical" if ra.get(k) == rb.get(k) else "DIFFERENT")))
        for ln in d[:20]:
            print("    " + ln)
    return bad


if __name__ == "__main__":
    sys.exit(main())
