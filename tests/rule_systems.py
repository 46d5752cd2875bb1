"""Named test systems over the conductance rules (bond, site, mixed), both
lattices, pbc and non-unit Va / g0 / leak -- TEST INFRASTRUCTURE ONLY, the
helper of test_rule_value_parity.py (and of test_batch.py's value sets).

A system is (rule, lattice, m, n, pbc, Va, g0, leak).  build() gives the GPU's
occupancy arguments (Context.occupy) and the oracle's side of the same
realisation: the bond list, the replay labels, the spanning label by the
reference's rule and the rule's bond values (or_bond_values).  Occupation is
by the reference shuffles the other tests use:

  bond    shuffled_ids(nb, 21), square 0.60 (open) / 0.58 (pbc), triangular 0.42
  site    shuffled_ids(t, 1080115) (site.f's seed), square 0.66, triangular 0.58
  mixed   sites 143285, bonds 43716 (sitebond.f's seeds), square ps 0.90 pb 0.80,
          triangular ps 0.85 pb 0.60

The spanning rule is bondc.f:413-456 (bond), site.f:309-344 with size n
(site) and sitebond.f:423-458 with size 2n-1 (mixed), as
test_literal_dot.mixed_system and golden/make_config_golden.py.

oracle_solve() is the oracle's literal linbcg of a system (tol 1e-8 and
1e-13, itmax 100000) with the terminal currents under both current rules,
computed once per process and shared by every test that needs it.
"""
import collections
import ctypes as C

import numpy as np

import oracle_lib as O
from percolation_amd import _lib as PL
from percolation_amd import api

System = collections.namedtuple("System", "rule lattice m n pbc Va g0 leak")

RULE_NAME = {PL.RULE_BOND: "bond", PL.RULE_SITE: "site", PL.RULE_MIXED: "mixed"}
TOLS = (1e-8, 1e-13)
ITMAX = 100000
CUR_THRESH = {PL.CUR_FORTRAN: 1e-10, PL.CUR_MATLAB: 0.0}  # sprsin's threshold, bondc.f:547

# (Va, g0, leak): the reference's values; two sets whose g0 and Va are no
# powers of two (no product g0 * x or gval * Va is exact), with the leak
# below (its terms dropped from the Fortran-rule currents) and above (kept)
# the 1e-10 current threshold
UNIT = (1.0, 1.0, 1e-12)
LEAK_DROPPED = (2.5, 0.7, 3e-11)
LEAK_KEPT = (0.3, 13.0, 3e-9)
NONUNIT = (LEAK_DROPPED, LEAK_KEPT)

# the smallest lattices that still select each kernel family
# (perc_solve.hip: select_format, res_geometry)
G_OPEN_SQ = (0, 128, 99, 0)    # N = 12416 > 8192: one march strip, the narrow resident grid
G_PBC_SQ = (0, 256, 150, 1)    # pbc wrap forms, two strips, no resident grid
G_OPEN_TRI = (1, 128, 99, 0)   # triangular forms
G_PBC_TRI = (1, 256, 120, 1)   # triangular + pbc
G_TILE_SQ = (0, 130, 70, 0)    # N = 8840, m % 128 != 0: LDS tiles, narrow resident with 192 threads
G_TILE_TRI = (1, 130, 70, 1)   # LDS tiles with wrapped triangular forms
G_SMALL_SQ = (0, 50, 50, 0)    # N <= 8192: k_cg_small under PERC_FMT_AUTO
G_SMALL_TRI = (1, 48, 48, 1)
GEOMETRIES = (G_OPEN_SQ, G_PBC_SQ, G_OPEN_TRI, G_PBC_TRI, G_TILE_SQ, G_TILE_TRI, G_SMALL_SQ,
              G_SMALL_TRI)


def matrix():
    """the 36 systems: site and mixed on every geometry at the unit values and
    on G_OPEN_SQ at both non-unit sets; bond on every geometry at both non-unit
    sets (bond at the unit values is test_gpu_parity's / test_literal_dot's)"""
    out = []
    for rule in (PL.RULE_SITE, PL.RULE_MIXED):
        out += [System(rule, *g, *UNIT) for g in GEOMETRIES]
        out += [System(rule, *G_OPEN_SQ, *v) for v in NONUNIT]
    out += [System(PL.RULE_BOND, *g, *v) for g in GEOMETRIES for v in NONUNIT]
    return out


def name(s):
    return "%s-%s%dx%d%s-Va%g-g%g-l%g" % (RULE_NAME[s.rule], "tri" if s.lattice else "sq", s.m, s.n,
                                            "p" if s.pbc else "", s.Va, s.g0, s.leak)


def geometry(s):
    return (s.lattice, s.m, s.n, s.pbc)


def nonunit(s):
    return (s.Va, s.g0, s.leak) != UNIT


def natural_cur_rule(s):
    """bondc.f's currents for the bond rule, ConductCalc.m's for the others"""
    return PL.CUR_FORTRAN if s.rule == PL.RULE_BOND else PL.CUR_MATLAB


_BUILT = {}


def build(s):
    """dict(occ: Context.occupy's arguments; b1, b2, gval: the oracle's bond
    list and the rule's bond values; blabel, slabel, perccln: the oracle's
    labels and spanning label (0: nothing spans, gval is None); nspan: how
    many labels span).  The labeling is shared by the value sets of a
    (rule, geometry)."""
    key = (s.rule,) + geometry(s)
    if key not in _BUILT:
        _BUILT[key] = _label(s.rule, *geometry(s))
    d = dict(_BUILT[key])
    if d["perccln"] > 0:
        nb = len(d["b1"])
        gval = O.f64(nb)
        O.lib().or_bond_values(s.rule, nb, d["b1"], d["b2"], d["blabel"], d["slabel"], d["perccln"],
                               s.g0, s.leak, gval)
        d["gval"] = gval
    else:
        d["gval"] = None
    return d


def _label(rule, lat, m, n, pbc):
    lib = O.lib()
    t = m * n
    if rule == PL.RULE_BOND:
        seed = 21
        p = 0.42 if lat else (0.58 if pbc else 0.60)
        b1, b2, o1, o2 = O.bond_order(lat, m, n, pbc, seed)
        nb = len(b1)
        tb = int(p * nb)
        bl, csize, cln, _, _ = O.label_bonds(lat, m, n, pbc, b1, b2, o1, o2, tb, literal=False)
        sl = O.i32(1)
        perccln = lib.or_span_bonds(m, n, nb, b1, b2, bl, csize, cln)
        occ_ = bl > 0
        bot = set(bl[occ_ & (b1 <= m)].tolist())
        top = set(bl[occ_ & (b2 > t - m)].tolist())
        spanning = [l for l in bot & top if csize[l] >= n - 1]
        occ = dict(kind=PL.BOND, bond_order=api.shuffled_ids(nb, seed), nbonds_=tb)
    elif rule == PL.RULE_SITE:
        seed = 1080115
        ps = 0.58 if lat else 0.66
        b1, b2 = O.bond_list(lat, m, n, pbc)
        ts = int(ps * t)
        sl, csize, cln, _, _ = O.label_sites(lat, m, n, pbc, O.site_order(t, seed), ts, literal=False)
        bl = O.i32(len(b1))
        minsize = n
        occ = dict(kind=PL.SITE, site_order=api.shuffled_ids(t, seed), nsites=ts)
    else:
        sseed, bseed = 143285, 43716
        ps, pb = (0.85, 0.60) if lat else (0.90, 0.80)
        b1, b2, o1, o2 = O.bond_order(lat, m, n, pbc, bseed)
        nb = len(b1)
        ts, tb = int(ps * t), int(pb * nb)
        sl, bl, csize, cln, _, _ = O.label_sitebond(lat, m, n, pbc, b1, b2, O.site_order(t, sseed), ts,
                                                    o1, o2, tb, literal=False)
        minsize = 2 * n - 1
        occ = dict(kind=PL.SITEBOND, site_order=api.shuffled_ids(t, sseed), nsites=ts,
                   bond_order=api.shuffled_ids(nb, bseed), nbonds_=tb)
    if rule != PL.RULE_BOND:
        perccln = lib.or_span_sites(m, n, sl, csize, cln, minsize)
        bot = set(sl[:m][sl[:m] > 0].tolist())
        top = set(sl[t - m:][sl[t - m:] > 0].tolist())
        spanning = [l for l in bot & top if csize[l] >= minsize]
    assert (perccln > 0) == bool(spanning) and (not spanning or perccln == min(spanning))
    return dict(occ=occ, b1=b1, b2=b2, blabel=bl, slabel=sl, perccln=int(perccln), nspan=len(spanning))


def oracle_currents(s, d, oc, cur_rule, gval=None):
    """(Gtop, Gbot) of the oracle solve oc's voltages under a current rule
    (or_currents: bondc.f:554-592 with sprsin's 1e-10 threshold, or
    ConductCalc.m:178-196 without one)"""
    gt, gb = C.c_double(), C.c_double()
    O.lib().or_currents(s.lattice, s.m, s.n, s.pbc, len(d["b1"]), d["b1"], d["b2"],
                        d["gval"] if gval is None else gval, oc["diag"], oc["vint"], s.Va,
                        CUR_THRESH[cur_rule], cur_rule, C.byref(gt), C.byref(gb))
    return gt.value, gb.value


def oracle_conductance(s, d, tol, gval=None):
    """the oracle's assembly + literal linbcg + currents of a system (both
    current rules: dict cur[cur_rule] = (Gtop, Gbot)); gval: other bond values
    than the rule's (per-bond weights)"""
    g = d["gval"] if gval is None else gval
    oc = O.conductance(s.lattice, s.m, s.n, s.pbc, d["b1"], d["b2"], g, Va=s.Va, tol=tol, itmax=ITMAX,
                       cur_rule=PL.CUR_FORTRAN, cur_thresh=CUR_THRESH[PL.CUR_FORTRAN])
    oc["cur"] = {PL.CUR_FORTRAN: (oc["gtop"], oc["gbot"]),
                 PL.CUR_MATLAB: oracle_currents(s, d, oc, PL.CUR_MATLAB, g)}
    return oc


_ORACLE = {}


def oracle_solve(s, tol):
    """oracle_conductance of a spanning system, computed once (a solve takes
    up to 2 s of CPU)"""
    if (s, tol) not in _ORACLE:
        d = build(s)
        assert d["perccln"] > 0, "%s does not span" % name(s)
        _ORACLE[s, tol] = oracle_conductance(s, d, tol)
    return _ORACLE[s, tol]
