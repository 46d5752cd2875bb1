#!/usr/bin/env python3
"""Per-kernel means of the SQ counter passes of tools/gpu/pmc_march.sh.

For every pass directory (rocprofv3 -f csv output) and each k_cg_march
instantiation (named by its first template argument: <1 the march P, <2 the
march B), average each counter over the kernel's last `--last` dispatches
(tools/pmc_probe.py's whole-iteration launches, every one doing work), then
print the counters and the ratios the march's issue estimate needs: VALU and
SALU instructions per wave, and the share of the waves' cycles in which a
VALU / scalar instruction was issuing.

  python tools/pmc_march_summary.py DIR [DIR ...] [--last 64]
"""
import argparse
import sys

from pmc_reconcile import load


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--last", type=int, default=64)
    a = ap.parse_args()
    ctr = {}
    for d in a.dirs:
        for k, cs in load(d).items():
            if not k.startswith("k_cg_march"):
                continue
            for c, v in cs.items():
                v = v[-a.last:]
                ctr.setdefault(k, {})[c] = (sum(v) / len(v), len(v))
    if not ctr:
        sys.exit("no k_cg_march dispatches in %s" % " ".join(a.dirs))
    for k in sorted(ctr):
        c = ctr[k]
        print(k)
        for name in sorted(c):
            print("  %-22s %16.1f  (mean of %d dispatches)" % (name, c[name][0], c[name][1]))
        g = lambda n: c[n][0] if n in c else None  # noqa: E731
        waves, wc = g("SQ_WAVES"), g("SQ_WAVE_CYCLES")
        if waves:
            for n in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS"):
                if g(n) is not None:
                    print("  %-22s %16.1f" % (n + " / wave", g(n) / waves))
        # (SQ_WAVE_CYCLES and the SQ_ACTIVE_INST_* / SQ_WAIT_* counters are in
        # the same unit when collected by the same tool: their ratio is the
        # share of the resident waves' time with such an instruction issuing)
        if wc:
            for n in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_SCA", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_INST_ANY",
                      "SQ_WAIT_ANY", "SQ_BUSY_CYCLES"):
                if g(n) is not None:
                    print("  %-22s %16.4f" % (n + " / wave cycles", g(n) / wc))


if __name__ == "__main__":
    main()
