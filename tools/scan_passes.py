#!/usr/bin/env python3
"""Labelings per trial and hook / flatten passes per labeling of k_batch_scan,
from a probe build that returns the counters in place of the sizes:

  make -C percolation_amd/csrc probe TAG=passes PFLAGS=-DPERC_SCAN_PASSES
  PERC_LIBPERC=percolation_amd/probe/libperc_passes.so python tools/scan_passes.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from percolation_amd import _lib as L  # noqa: E402
from percolation_amd import api  # noqa: E402

for lat, Ls, trials in ((0, 50, 256), (1, 50, 256), (0, 128, 64)):
    for kind in (L.BOND, L.SITE):
        with api.Context(lat, Ls, Ls, 0) as ctx:
            N = ctx.nb if kind == L.BOND else ctx.t
            seeds = api.trial_seeds(58302, trials, scale=1000000)
            orders = np.stack([api.shuffled_ids(N, int(s)) for s in seeds])
            r = ctx.batch_scan(kind, **{"bond_orders" if kind == L.BOND else "site_orders": orders})
        p = np.array([x["maxcs"] for x in r], float)
        n = np.array([x["span_size"] for x in r], float)
        print(json.dumps(dict(lattice=lat, L=Ls, kind=int(kind), trials=trials, labelings_per_trial=round(float(n.mean()), 2),
                              passes_per_labeling=round(float(p.sum() / n.sum()), 2),
                              max_passes_per_labeling_of_a_trial=round(float((p / n).max()), 2))), flush=True)
