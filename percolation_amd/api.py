"""Host-side mirror of the reference drivers over the libperc C-ABI.

The drop-in host is Fortran (percolation_amd/fortran/); this module mirrors
the same programs for tests and the benchmark, with the reference's
parameter names and semantics:

  bondc      Fortran/Square/bondc.f, Fortran/Triangular/bondc.f
  site       Fortran/*/site.f (+ MATLAB/ConductCalc.m site rule)
  sitebond   Fortran/*/sitebond.f (+ ConductCalc.m mixed rule)
  bond_cond  Fortran/*/bond_cond.f grid-point conductances
  cond_curve site / sitebond realisations over trials and a grid of ps or
             (ps, pb): the mean ConductCalc.m conductance curve (no reference
             program; the batch kernel's ensemble, Context.batch_cond)
  current_curve  the same trials' bond-current statistics over a grid of p:
             backbone fraction, current moments, histogram
             (Context.batch_cond(currents=True))

Every compute step runs in libperc on the GPU; there is no fallback.
"""
import ctypes as C

import numpy as np

from . import _lib as L

LEAK = 1.0e-12  # bondc.f:487


def _i32(n):
    return np.zeros(n, dtype=np.int32)


def nbonds(lattice, m, n, pbc=0):
    return L.lib().perc_nbonds(lattice, m, n, pbc)


def bond_list(lattice, m, n, pbc=0):
    """(b1, b2) in reference order (bondc.f:137-154)."""
    nb = nbonds(lattice, m, n, pbc)
    b1, b2 = _i32(nb), _i32(nb)
    got = L.lib().perc_bond_list(lattice, m, n, pbc, b1, b2)
    assert got == nb
    return b1, b2


def nearestn(lattice, m, n, pbc, rn):
    nn = _i32(6)
    scn = L.lib().perc_nearestn(lattice, m, n, pbc, rn, nn)
    return nn[:scn]


def shuffled_ids(N, seed):
    """1-based id permutation after srand(seed) + REAL*4 Fisher-Yates;
    N+1 slots, slot N is the H2 spill slot (bondc.f:162-174)."""
    order = _i32(N + 1)
    order[:N] = np.arange(1, N + 1, dtype=np.int32)
    lib = L.lib()
    lib.perc_srand(seed)
    lib.perc_shuffle(N, order)
    return order


def random_order(n, count, seed, kind=L.BOND):
    """The order perc_occupy_random's occupancy is the prefix of: the first
    `count` ids (1-based) in ascending counter-based key order (host)."""
    out = _i32(max(count, 1))
    L.check(L.lib().perc_random_order(int(n), int(count), int(seed), int(kind), out),
            "perc_random_order")
    return out[:count]


def trial_seeds(master, k=1000, scale=10000000):
    """tseed(1..k) = int(rand(0)*scale)+1 after srand(master): scale 1e7 in
    bond_cond.f:65-70, 1e6 in bond_perc.f / site_perc.f:70-74."""
    ts = _i32(k)
    if scale == 10000000:
        L.lib().perc_trial_seeds(master, k, ts)
    else:
        L.lib().perc_trial_seeds_scaled(master, k, scale, ts)
    return ts


def replay_labels(lattice, m, n, pbc, kind, site_order=None, nsites=0, bond_order=None,
                  nbond=0):
    """Reference label numbering of an explicit occupancy (host replay, no
    device): dict(bond_label, site_label, csize, cln, maxcn, maxcs, perccln)."""
    t = m * n
    nb = nbonds(lattice, m, n, pbc)
    cap = {L.BOND: nb + 2, L.SITE: t + 2}.get(kind, t + nb + 2)
    bl = _i32(nb) if kind != L.SITE else None
    sl = _i32(t) if kind != L.BOND else None
    cs, st = _i32(cap), _i32(4)
    so = None if site_order is None else np.ascontiguousarray(site_order, dtype=np.int32)
    bo = None if bond_order is None else np.ascontiguousarray(bond_order, dtype=np.int32)
    L.check(L.lib().perc_replay_labels(lattice, m, n, pbc, kind, nsites, L.ptr(so), nbond,
                                       L.ptr(bo), L.ptr(bl), L.ptr(sl), L.ptr(cs), cap,
                                       L.ptr(st)), "perc_replay_labels")
    return dict(bond_label=bl, site_label=sl, csize=cs, cln=int(st[0]), maxcn=int(st[1]),
                maxcs=int(st[2]), perccln=int(st[3]))


def batch_supported(lattice, m, n, pbc=0):
    """perc_batch_supported (host-only): True when the batch kernel can run
    this lattice -- n >= 3, (n-2)*m <= 8192 interior rows, stencil operator."""
    return bool(L.lib().perc_batch_supported(lattice, m, n, pbc))


def batch_cond_supported(kind, lattice, m, n, pbc=0):
    """perc_batch_cond_supported (host-only): True when the batch kernel can
    run this kind (BOND / SITE / SITEBOND) on this lattice -- batch_supported
    for BOND, the same checks with the kind's own LDS layout for the others."""
    return bool(L.lib().perc_batch_cond_supported(int(kind), lattice, m, n, pbc))


def batch_large_supported(kind, lattice, m, n, pbc=0):
    """perc_batch_large_supported (host-only): True when the large batch
    kernel (Context.set_batch_large) can run this kind on this lattice --
    m, n >= 3, m * n <= 16384 sites (128 x 128), stencil operator, the kind's
    LDS arena; every lattice batch_cond_supported accepts."""
    return bool(L.lib().perc_batch_large_supported(int(kind), lattice, m, n, pbc))


def batch_weighted_supported(kind, lattice, m, n, pbc=0):
    """perc_batch_weighted_supported (host-only): True when the weighted batch
    kernel (Context.batch_cond with weights / item_wseed) can run this kind on
    this lattice -- m, n >= 3, at most 4096 interior rows, stencil operator,
    the slot values of every row within the workgroup's LDS; every lattice of
    10 x 10 .. 50 x 50."""
    return bool(L.lib().perc_batch_weighted_supported(int(kind), lattice, m, n, pbc))


KIND_RULE = {L.BOND: L.RULE_BOND, L.SITE: L.RULE_SITE, L.SITEBOND: L.RULE_MIXED}


def natural_cur_rule(kind):
    """the reference's own pairing: bondc.f's currents for the bond kind,
    ConductCalc.m's for the site and mixed kinds"""
    return L.CUR_FORTRAN if kind == L.BOND else L.CUR_MATLAB


def scan_supported(lattice, m, n, pbc=0):
    """perc_scan_supported (host-only): True when the scan kernel can run this
    lattice -- m, n >= 3 and m * n <= 16384 sites."""
    return bool(L.lib().perc_scan_supported(lattice, m, n, pbc))


def shuffle_device_supported(N):
    """perc_shuffle_device_supported (host-only): True when the shuffle kernel
    can take a list of N ids -- 1 <= N <= 65534 (16-bit entries in LDS)."""
    return bool(L.lib().perc_shuffle_device_supported(int(N)))


def batch_clusters_supported(lattice, m, n, pbc=0, nexact=0):
    """perc_batch_clusters_supported (host-only): True when the cluster kernel
    (Context.batch_clusters) can run this lattice with this exact range --
    what scan_supported accepts, and 0 <= nexact <= 1024."""
    return bool(L.lib().perc_batch_clusters_supported(lattice, m, n, pbc, int(nexact)))


def batch_geometry_supported(lattice, m, n, pbc=0, nexact=0):
    """perc_batch_geometry_supported (host-only): True when
    Context.batch_clusters(geometry=True) can run this lattice --
    batch_clusters_supported with pbc == 0."""
    return bool(L.lib().perc_batch_geometry_supported(lattice, m, n, pbc, int(nexact)))


def batch_currents_supported(kind, lattice, m, n, pbc=0):
    """perc_batch_currents_supported (host-only): True when
    Context.batch_cond(currents=True) can run this kind on this lattice --
    exactly batch_cond_supported (the default kernel only, at most 8192
    interior rows; set_batch_large is not read)."""
    return bool(L.lib().perc_batch_currents_supported(int(kind), lattice, m, n, pbc))


def _currents_dict(rec):
    """one CURRENTS_DTYPE record as the keys Context.batch_cond adds"""
    d = {k: rec[k].item() for k in L.CURRENTS_KEYS[:-1]}
    d["hist"] = np.array(rec["hist"], dtype=np.int32)
    return d


def current_stats_host(lattice, m, n, pbc, conducting, vint, Va=1.0, g0=1.0, cut=1e-6):
    """perc_current_stats_host (host-only, no device): the bond-current record
    of one realisation -- over the conducting bonds (conducting[id - 1] != 0,
    nb entries by bond id) with an interior end site, |i| = |g0 (V[b2] -
    V[b1])| with V = 0 on the bottom row, Va on the top row and vint (t - 2m)
    between: dict(nbonds, nabove, imax, s1, s2, s4, s6, hist), the sums in
    bond-id order, nabove the bonds with |i| >= cut * imax, hist[64] the
    octaves below g0 Va."""
    nb = nbonds(lattice, m, n, pbc) if m >= 1 and n >= 1 else 0
    c = np.ascontiguousarray(conducting, dtype=np.uint8).reshape(-1)
    v = np.ascontiguousarray(vint, dtype=np.float64).reshape(-1)
    if len(c) != nb or len(v) != max(m * n - 2 * m, 0):
        raise ValueError("current_stats_host: conducting has nb entries, vint t - 2m")
    rec = np.zeros(1, dtype=L.CURRENTS_DTYPE)
    L.check(L.lib().perc_current_stats_host(lattice, m, n, pbc, L.ptr(c), L.ptr(v), float(Va), float(g0),
                                            float(cut), L.ptr(rec)), "perc_current_stats_host")
    return _currents_dict(rec[0])


def conducting_bonds(kind, b1, b2, site_occ, bond_occ, canon, root):
    """The conducting bonds of a labeled realisation (uint8, nb entries by bond
    id): the bonds the kind's rule gives g0 -- BOND: the bond is occupied;
    SITE: both end sites are; SITEBOND: the bond and both end sites are -- and
    whose end sites lie in the chosen spanning cluster (canon[s - 1] == root,
    Context.label(canon=True); root 0: none).  b1, b2: bond_list; site_occ,
    bond_occ: Context.occupancy()."""
    kind = int(kind)
    if kind not in (L.BOND, L.SITE, L.SITEBOND):
        raise ValueError("conducting_bonds: kind BOND, SITE or SITEBOND")
    b1, b2 = np.asarray(b1, dtype=np.int64) - 1, np.asarray(b2, dtype=np.int64) - 1
    so, bo, canon = np.asarray(site_occ) != 0, np.asarray(bond_occ) != 0, np.asarray(canon)
    occ = np.ones(len(b1), dtype=bool)
    if kind != L.SITE:
        occ &= bo
    if kind != L.BOND:
        occ &= so[b1] & so[b2]
    return (occ & (int(root) > 0) & (canon[b1] == int(root))).astype(np.uint8)


def _whole_prefix(order, count, N):
    """(order, count) as replay_labels takes them: a count of N + 1 is the
    whole order with the spill slot dropped"""
    if order is None:
        return None, 0
    o = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
    count = int(count)
    if count > N:
        o = np.ascontiguousarray(o[:count][o[:count] != 0][:N])
        count = len(o)
    return o, count


def cluster_stats_host(lattice, m, n, pbc, kind, site_order=None, nsites=0, bond_order=None, nbonds=0,
                       nexact=0):
    """The record and histogram row of Context.batch_clusters for one item, on
    the host (no device): from replay_labels' label arrays -- a cluster's size
    is the number of bonds and sites that carry its label (bonds for BOND,
    sites for SITE, both for SITEBOND), never csize, so the phantom label of
    the shuffle's spill slot (H2) does not enter; spanning from the labels of
    the bottom and top rows (BOND: of the bonds with an end site there).
    Returns (record, hist): a CLUSTER_DTYPE scalar and nexact + 32 int32."""
    kind, nexact = int(kind), int(nexact)
    if kind not in (L.BOND, L.SITE, L.SITEBOND):
        raise ValueError("cluster_stats_host: kind BOND, SITE or SITEBOND")
    if not 0 <= nexact <= 1024:
        raise ValueError("cluster_stats_host: nexact outside 0..1024")
    t = m * n
    b1, b2 = bond_list(lattice, m, n, pbc)
    nb = len(b1)
    so, ns = _whole_prefix(site_order if kind != L.BOND else None, nsites, t)
    bo, nbo = _whole_prefix(bond_order if kind != L.SITE else None, nbonds, nb)
    r = replay_labels(lattice, m, n, pbc, kind, site_order=so, nsites=ns, bond_order=bo, nbond=nbo)
    sl, bl = r["site_label"], r["bond_label"]
    nlab = 1 + max(int(sl.max()) if sl is not None and len(sl) else 0,
                   int(bl.max()) if bl is not None and len(bl) else 0)
    nsite = np.bincount(sl, minlength=nlab) if sl is not None else np.zeros(nlab, np.int64)
    nbond = np.bincount(bl, minlength=nlab) if bl is not None else np.zeros(nlab, np.int64)
    size = (nsite + nbond).astype(np.int64)
    size[0] = 0  # (label 0: not occupied)
    # the member sites of a label: its sites (SITE, SITEBOND), its bonds' end sites (BOND)
    minsite = np.full(nlab, t + 1, dtype=np.int64)
    bot = np.zeros(nlab, dtype=bool)
    top = np.zeros(nlab, dtype=bool)
    if kind == L.BOND:
        for end in (b1, b2):
            np.minimum.at(minsite, bl, end)
            bot[bl[end <= m]] = True
            top[bl[end > t - m]] = True
    else:
        np.minimum.at(minsite, sl, np.arange(1, t + 1))
        bot[sl[:m]] = True
        top[sl[t - m:]] = True
    labels = np.nonzero(size)[0]
    span = labels[bot[labels] & top[labels]]
    s = size[labels]
    rec = np.zeros((), dtype=L.CLUSTER_DTYPE)
    rec["nclusters"] = len(labels)
    rec["nlone"] = int(np.count_nonzero(nsite[labels] == 0)) if kind == L.SITEBOND else 0
    rec["nspan"] = len(span)
    if len(span):
        first = span[np.argmin(minsite[span])]
        rec["span_root"] = minsite[first]
        rec["span_size"] = size[first]
    rec["maxcs"] = s.max() if len(s) else 0
    rec["s1"], rec["s2"] = s.sum(), (s * s).sum()
    rec["span_s1"], rec["span_s2"] = size[span].sum(), (size[span] ** 2).sum()
    hist = np.zeros(nexact + 32, dtype=np.int32)
    if len(s):
        np.add.at(hist, s[s <= nexact] - 1, 1)
        np.add.at(hist, nexact + np.frexp(s)[1].astype(np.int64) - 1, 1)  # floor(log2 s), exactly
    return rec, hist


def site_positions(lattice, m, n):
    """The integer embedding of include/perc.h's cluster geometry: (x, y, wx,
    unit) with d2(i, j) = wx (x_i - x_j)^2 + (y_i - y_j)^2 = unit x the squared
    distance of sites i and j (0-based, row-major from the bottom row) --
    square: x = column, y = row, wx = 1, unit = 1; triangular: y = 2 row -
    (column & 1), wx = 3, unit = 4."""
    s = np.arange(m * n, dtype=np.int64)
    r, c = s // m, s % m
    if lattice == L.TRIANGULAR:
        return c, 2 * r - (c & 1), 3, 4
    return c, r, 1, 1


def cluster_geometry_host(lattice, m, n, pbc, kind, site_order=None, nsites=0, bond_order=None, nbonds=0,
                          nexact=0):
    """The geometry record and octave rows of Context.batch_clusters(geometry=
    True) for one item, on the host (no device): from replay_labels' label
    arrays -- a cluster's member sites are the sites that carry its label
    (SITE, SITEBOND) or the end sites of the bonds that do (BOND), G_c = n_c
    sum |r_i|^2 - |sum r_i|^2 over site_positions in int64, spanning as in
    cluster_stats_host.  pbc = 0 only; nexact is not read (cluster_stats_host's
    arguments).  Returns (record, rows): a GEOM_DTYPE scalar and 96 int64."""
    kind = int(kind)
    if kind not in (L.BOND, L.SITE, L.SITEBOND):
        raise ValueError("cluster_geometry_host: kind BOND, SITE or SITEBOND")
    if pbc != 0:
        raise ValueError("cluster_geometry_host: pbc = 0 only")
    t = m * n
    b1, b2 = bond_list(lattice, m, n, pbc)
    so, ns = _whole_prefix(site_order if kind != L.BOND else None, nsites, t)
    bo, nbo = _whole_prefix(bond_order if kind != L.SITE else None, nbonds, len(b1))
    r = replay_labels(lattice, m, n, pbc, kind, site_order=so, nsites=ns, bond_order=bo, nbond=nbo)
    if kind == L.BOND:  # every occupied bond of a site carries one label
        lab = np.zeros(t + 1, dtype=np.int64)
        bl = r["bond_label"].astype(np.int64)
        lab[b1[bl > 0]] = bl[bl > 0]
        lab[b2[bl > 0]] = bl[bl > 0]
        lab = lab[1:]
    else:
        lab = r["site_label"].astype(np.int64)
    nlab = int(lab.max()) + 1 if t else 1
    x, y, wx, _ = site_positions(lattice, m, n)

    def per_label(w):
        out = np.zeros(nlab, dtype=np.int64)
        np.add.at(out, lab, w)
        out[0] = 0  # (label 0: no member site)
        return out

    nc = per_label(np.ones(t, dtype=np.int64))
    sx, sy = per_label(x), per_label(y)
    G = nc * per_label(wx * x * x + y * y) - wx * sx * sx - sy * sy
    minsite = np.full(nlab, t + 1, dtype=np.int64)
    np.minimum.at(minsite, lab, np.arange(1, t + 1))
    bot, top = np.zeros(nlab, dtype=bool), np.zeros(nlab, dtype=bool)
    bot[lab[:m]] = True
    top[lab[t - m:]] = True
    labels = np.nonzero(nc)[0]
    span = labels[bot[labels] & top[labels]]
    rec = np.zeros((), dtype=L.GEOM_DTYPE)
    rows = np.zeros(L.GEOM_ROW, dtype=np.int64)
    if len(labels):
        n_, g_ = nc[labels], G[labels]
        rec["n1"], rec["n2"], rec["g2"] = n_.sum(), (n_ * n_).sum(), g_.sum()
        rec["span_n1"], rec["span_n2"], rec["span_g2"] = nc[span].sum(), (nc[span] ** 2).sum(), G[span].sum()
        big = labels[np.lexsort((minsite[labels], -n_))[0]]  # the most member sites; tie: the smallest root
        rec["big_root"], rec["big_n"], rec["big_g2"] = minsite[big], nc[big], G[big]
        if len(span):
            first = span[np.argmin(minsite[span])]
            rec["root_n"], rec["root_g2"] = nc[first], G[first]
        b = np.frexp(n_)[1].astype(np.int64) - 1  # floor(log2 n_c), exactly
        np.add.at(rows, b, 1)
        np.add.at(rows, 32 + b, n_ * n_)
        np.add.at(rows, 64 + b, g_)
    return rec, rows


def _device_shuffle_ok(ctx, kind):
    """every list `kind` reads on ctx's lattice fits the shuffle kernel"""
    return ((kind == L.BOND or shuffle_device_supported(ctx.t))
            and (kind == L.SITE or shuffle_device_supported(ctx.nb)))


class Context:
    """One libperc context (one lattice on one device)."""

    def __init__(self, lattice, m, n, pbc=0, device=0):
        self.lattice, self.m, self.n, self.pbc = lattice, m, n, pbc
        self.device = device
        self.t = m * n
        self.nb = nbonds(lattice, m, n, pbc)
        self.N = self.t - 2 * m
        h = C.c_void_p()
        L.check(L.lib().perc_ctx_create(device, lattice, m, n, pbc, C.byref(h)),
                "perc_ctx_create")
        self.h = h

    def close(self):
        if self.h:
            L.lib().perc_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- occupancy ---------------------------------------------------------
    def occupy(self, kind, site_order=None, nsites=0, bond_order=None, nbonds_=0):
        so = None if site_order is None else np.ascontiguousarray(site_order, dtype=np.int32)
        bo = None if bond_order is None else np.ascontiguousarray(bond_order, dtype=np.int32)
        L.check(L.lib().perc_occupy(self.h, kind, nsites, L.ptr(so), nbonds_, L.ptr(bo)),
                "perc_occupy")

    def occupy_random(self, kind, nsites=0, nbonds_=0, seed=1):
        """perc_occupy_random: the nsites / nbonds_ smallest counter-based
        keys occupied, drawn on the device (no order array)."""
        L.check(L.lib().perc_occupy_random(self.h, kind, int(nsites), int(nbonds_), int(seed)),
                "perc_occupy_random")

    def occupancy(self):
        """perc_occupancy: (site_occ[t], bond_occ[nb]) uint8 arrays of the
        device occupancy (site / bond ids 1.. at index 0..)."""
        so = np.zeros(self.t, dtype=np.uint8)
        bo = np.zeros(self.nb, dtype=np.uint8)
        L.check(L.lib().perc_occupancy(self.h, so.ctypes.data, bo.ctypes.data), "perc_occupancy")
        return so, bo

    def occupy_device(self, kind, site_ptr=None, nsites=0, bond_ptr=None, nbonds_=0):
        """perc_occupy_device: order lists already in device memory (int
        addresses of device int32 arrays on this context's device)."""
        sp = C.c_void_p(site_ptr) if site_ptr else None
        bp = C.c_void_p(bond_ptr) if bond_ptr else None
        L.check(L.lib().perc_occupy_device(self.h, kind, nsites, sp, nbonds_, bp),
                "perc_occupy_device")

    def label(self, canon=False):
        info = L.LabelInfo()
        out = _i32(self.t) if canon else None
        L.check(L.lib().perc_label(self.h, C.byref(info), L.ptr(out)), "perc_label")
        res = {k: getattr(info, k) for k, _ in L.LabelInfo._fields_}
        if canon:
            res["canon"] = out
        return res

    def label_numbers(self, kind):
        if kind == L.BOND:
            cap = self.nb + 2
        elif kind == L.SITE:
            cap = self.t + 2
        else:
            cap = self.t + self.nb + 2
        bl = _i32(self.nb) if kind != L.SITE else None
        sl = _i32(self.t) if kind != L.BOND else None
        cs, st = _i32(cap), _i32(4)
        L.check(L.lib().perc_label_numbers(self.h, L.ptr(bl), L.ptr(sl), L.ptr(cs), cap,
                                           L.ptr(st)), "perc_label_numbers")
        return dict(bond_label=bl, site_label=sl, csize=cs, cln=int(st[0]), maxcn=int(st[1]),
                    maxcs=int(st[2]), perccln=int(st[3]))

    # -- conductance -------------------------------------------------------
    def conductance(self, rule=L.RULE_BOND, cur_rule=L.CUR_FORTRAN, Va=1.0, g0=1.0, leak=LEAK,
                    itol=2, tol=1e-8, itmax=2500, vint=False):
        res = L.CondResult()
        v = np.zeros(self.N, dtype=np.float64) if vint else None
        L.check(L.lib().perc_conductance(self.h, rule, cur_rule, Va, g0, leak, itol, tol, itmax,
                                         C.byref(res), L.ptr(v)), "perc_conductance")
        out = {k: getattr(res, k) for k, _ in L.CondResult._fields_}
        if vint:
            out["vint"] = v
        return out

    def system(self):
        n, nnz = C.c_int(), C.c_int()
        L.check(L.lib().perc_get_system(self.h, None, None, None, None, None, C.byref(n),
                                        C.byref(nnz)), "perc_get_system")
        rp, col = _i32(n.value + 1), _i32(nnz.value)
        val, diag, rhs = (np.zeros(k, np.float64) for k in (nnz.value, n.value, n.value))
        L.check(L.lib().perc_get_system(self.h, L.ptr(rp), L.ptr(col), L.ptr(val), L.ptr(diag),
                                        L.ptr(rhs), C.byref(n), C.byref(nnz)),
                "perc_get_system")
        return dict(rowptr=rp, col=col, val=val, diag=diag, rhs=rhs)

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        L.check(L.lib().perc_spmv_host(self.h, x, y), "perc_spmv_host")
        return y

    def bench_kernel(self, which, reps):
        ms = C.c_double()
        L.check(L.lib().perc_bench_kernel(self.h, which, reps, C.byref(ms)), "perc_bench_kernel")
        return ms.value

    def set_kernel_timing(self, enable=True):
        L.check(L.lib().perc_set_kernel_timing(self.h, int(enable)), "perc_set_kernel_timing")

    def kernel_stats(self, reset=True):
        st = np.zeros(6)
        L.check(L.lib().perc_kernel_stats(self.h, st, int(reset)), "perc_kernel_stats")
        return dict(spmv_ms=st[0], spmv_n=int(st[1]), resid_ms=st[2], resid_n=int(st[3]),
                    xp_ms=st[4], xp_n=int(st[5]))

    def set_matrix_format(self, fmt):
        """PERC_FMT_AUTO / _CSR / _STENCIL (fused) / _STENCIL_SPLIT / _STENCIL_TILED (perc.h)."""
        L.check(L.lib().perc_set_matrix_format(self.h, int(fmt)), "perc_set_matrix_format")

    def set_full_voltages(self, enable=True):
        """Keep every interior voltage up to date during the solve (perc.h)."""
        L.check(L.lib().perc_set_full_voltages(self.h, int(enable)), "perc_set_full_voltages")

    def cluster_sizes(self):
        """(maxcs, span_size) of the labeled bond / site occupancy on the
        GPU (perc_cluster_sizes)."""
        mx, sp = C.c_int(), C.c_int()
        L.check(L.lib().perc_cluster_sizes(self.h, C.byref(mx), C.byref(sp)), "perc_cluster_sizes")
        return mx.value, sp.value

    def set_slabs(self, nslab=1):
        """Row-slab decomposition of the CG solve (perc_set_slabs)."""
        L.check(L.lib().perc_set_slabs(self.h, int(nslab)), "perc_set_slabs")

    def set_march_rows(self, rows=0):
        """Band height of the register-march kernel (0: auto; perc.h)."""
        L.check(L.lib().perc_set_march_rows(self.h, int(rows)), "perc_set_march_rows")

    def set_march_mode(self, mode):
        """PERC_MARCH_* bits of the register-march loop (perc.h)."""
        L.check(L.lib().perc_set_march_mode(self.h, int(mode)), "perc_set_march_mode")

    def set_band_weights(self, which=None, weights=None):
        """Per-round weights of the slot-weighted bands (perc_set_band_weights;
        which 0: strip-major P, 1: its B, 2: row-major P).  No arguments:
        the defaults."""
        if which is None:
            L.check(L.lib().perc_set_band_weights(self.h, 0, 0, None), "perc_set_band_weights")
            return
        w = np.ascontiguousarray(weights, dtype=np.int32)
        L.check(L.lib().perc_set_band_weights(self.h, int(which), len(w), w.ctypes.data),
                "perc_set_band_weights")

    def set_dot_order(self, order):
        """PERC_DOT_FAST / PERC_DOT_LITERAL: the association of linbcg's dot
        products (perc_set_dot_order; LITERAL reproduces the reference solver
        bitwise)."""
        L.check(L.lib().perc_set_dot_order(self.h, int(order)), "perc_set_dot_order")

    def set_batch_large(self, enable=True):
        """perc_set_batch_large: batch_bondc / batch_cond on the large kernel
        (p alone in LDS; lattices up to 128 x 128, batch_large_supported) while
        set; False: the default batch kernel again."""
        L.check(L.lib().perc_set_batch_large(self.h, int(bool(enable))), "perc_set_batch_large")

    def batch_large(self):
        """the flag of set_batch_large (perc_batch_large)"""
        return bool(L.lib().perc_batch_large(self.h))

    def err_history(self):
        """err of every iteration of the last solve (perc_err_history)."""
        n = L.lib().perc_err_history(self.h, None, 0)
        if n < 0:
            L.check(n, "perc_err_history")
        out = np.zeros(n, dtype=np.float64)
        m = L.lib().perc_err_history(self.h, out.ctypes.data, n)
        if m < 0:
            L.check(m, "perc_err_history")
        return out

    def set_conductcalc_weights(self, rule, seed=1838534):
        """ConductCalc.m condtype 2 inside libperc (perc_set_conductcalc_weights):
        the spanning cluster's -g0 bonds of the last labeling get
        -g0*rand('twister', seed), one draw per bond in bond-list order --
        conductcalc_weights + set_bond_weights without the host replay."""
        L.check(L.lib().perc_set_conductcalc_weights(self.h, rule, int(seed) & 0xFFFFFFFF),
                "perc_set_conductcalc_weights")

    def set_bond_weights(self, w=None):
        """Per-bond conductance multipliers for the spanning cluster's bonds
        (ConductCalc.m condtype 2; None: fixed g0).  perc_set_bond_weights."""
        if w is None:
            L.check(L.lib().perc_set_bond_weights(self.h, None, 0), "perc_set_bond_weights")
            return
        w = np.ascontiguousarray(w, dtype=np.float64)
        L.check(L.lib().perc_set_bond_weights(self.h, w.ctypes.data, len(w)),
                "perc_set_bond_weights")

    def march_info(self):
        """The solver loop of the assembled system (perc_march_info)."""
        out = np.zeros(5, dtype=np.int32)
        L.check(L.lib().perc_march_info(self.h, out.ctypes.data), "perc_march_info")
        return dict(kernel=("none", "wave", "", "resident", "small")[out[0]],
                    qfree=bool(out[1] & 1), strips=bool(out[1] & 2), slots=bool(out[1] & 8), tag=bool(out[1] & 16),
                    nibble=bool(out[1] & 32),
                    alt=bool(out[2]), band_rows=int(out[3]), strip_cols=int(out[4]))

    def last_solve(self):
        """What the last solve actually ran (perc_last_solve): the kernel
        family ('other', 'march', 'slabs', 'resident', 'small'), its flags and
        the iteration count.  lit_terms: the literal folds summed the terms
        the solve kernels themselves stored (the production kernels ran).
        open: the strip-major nibble march ran its open-lattice kernels.
        front / front_iters: the march skipped the bands the Krylov front had
        not reached, in that many iterations."""
        out = np.zeros(4, dtype=np.int32)
        L.check(L.lib().perc_last_solve(self.h, out.ctypes.data), "perc_last_solve")
        f = int(out[1])
        return dict(kernel=("other", "march", "slabs", "resident", "small")[out[0]],
                    literal=bool(f & L.RAN_LITERAL), lit_terms=bool(f & L.RAN_LIT_TERMS),
                    qfree=bool(f & L.RAN_QFREE), strips=bool(f & L.RAN_STRIPS),
                    nibble=bool(f & L.RAN_NIBBLE), tag=bool(f & L.RAN_TAG),
                    host_fold=bool(f & L.RAN_HOST_FOLD), xcd_grouped=bool(f & L.RAN_XCD_GROUPED),
                    open=bool(f & L.RAN_OPEN), front=bool(f & L.RAN_FRONT), front_iters=int(out[3]),
                    iter=int(out[2]))

    def matrix_format(self):
        rc = L.lib().perc_matrix_format(self.h)
        if rc < 0:
            L.check(rc, "perc_matrix_format")
        return rc

    def system_size(self):
        out = np.zeros(2, dtype=np.int64)
        L.check(L.lib().perc_system_size(self.h, out), "perc_system_size")
        return int(out[0]), int(out[1])

    def _trial_lists(self, site_orders, bond_orders, site_seeds, bond_seeds):
        """The order lists (ntrials, N + 1) or seed lists (ntrials) of a batch
        call as libperc takes them: (so, bo, ntrials, seeded); ntrials None
        where no list is given."""
        so = bo = ntrials = None
        seeded = site_seeds is not None or bond_seeds is not None
        if seeded and (site_orders is not None or bond_orders is not None):
            raise ValueError("orders or seeds, not both")
        if site_seeds is not None:
            so = np.ascontiguousarray(site_seeds, dtype=np.int32).reshape(-1)
            ntrials = len(so)
        if bond_seeds is not None:
            bo = np.ascontiguousarray(bond_seeds, dtype=np.int32).reshape(-1)
            if ntrials is not None and len(bo) != ntrials:
                raise ValueError("site_seeds and bond_seeds differ in trials")
            ntrials = len(bo)
        if site_orders is not None:
            so = np.ascontiguousarray(site_orders, dtype=np.int32).reshape(-1, self.t + 1)
            ntrials = so.shape[0]
        if bond_orders is not None:
            bo = np.ascontiguousarray(bond_orders, dtype=np.int32).reshape(-1, self.nb + 1)
            if ntrials is not None and bo.shape[0] != ntrials:
                raise ValueError("site_orders and bond_orders differ in trials")
            ntrials = bo.shape[0]
        return so, bo, ntrials, seeded

    @staticmethod
    def _item_lists(item_trial, item_nsites, item_nbonds):
        """The items of a batch call as libperc takes them: (it, ns, nbc)."""
        it = np.ascontiguousarray(item_trial, dtype=np.int32).reshape(-1)
        ns = nbc = None
        if item_nsites is not None:
            ns = np.ascontiguousarray(item_nsites, dtype=np.int32).reshape(-1)
        if item_nbonds is not None:
            nbc = np.ascontiguousarray(item_nbonds, dtype=np.int32).reshape(-1)
        for c in (ns, nbc):
            if c is not None and c.shape != it.shape:
                raise ValueError("item_trial and the count lists differ in length")
        return it, ns, nbc

    def batch_bondc(self, orders, item_trial, item_count, solve=True, Va=1.0, g0=1.0, leak=LEAK,
                    itol=2, tol=1e-8, itmax=2500):
        """perc_batch_bondc: many small bond realisations in one launch, one
        workgroup each.  orders: (ntrials, nb + 1) shuffled id arrays (one
        array of nb + 1 for one trial); item i occupies the first
        item_count[i] entries of trial item_trial[i]'s order.  Returns one
        dict per item (gtop, gbot, err, iter, status, nclusters, nspan,
        span_root, span_sites, fallback); solve=False stops after the
        spanning test.  The dot order is the context's."""
        o = np.ascontiguousarray(orders, dtype=np.int32).reshape(-1, self.nb + 1)
        it = np.ascontiguousarray(item_trial, dtype=np.int32).reshape(-1)
        ic = np.ascontiguousarray(item_count, dtype=np.int32).reshape(-1)
        if it.shape != ic.shape:
            raise ValueError("item_trial and item_count differ in length")
        out = (L.BatchItem * max(len(it), 1))()
        L.check(L.lib().perc_batch_bondc(self.h, o.shape[0], o.reshape(-1), len(it), it, ic,
                                         1 if solve else 0, Va, g0, leak, itol, tol, itmax,
                                         C.cast(out, C.c_void_p)), "perc_batch_bondc")
        return [{k: getattr(out[i], k) for k, _ in L.BatchItem._fields_} for i in range(len(it))]

    def batch_shuffle(self, list, seeds, orders=False, ranks=False, n=None):
        """perc_batch_shuffle: the reference shuffle of one trial per seed on
        the device, one wave each, the ranks left in the context's batch rank
        buffers.  list BOND (N = nb) or SITE (N = t).  Returns (orders, ranks):
        the (ntrials, N + 1) orders as shuffled_ids gives them and the
        (ntrials, N) positions of ids 1..N in them, each None unless asked
        for.  n (list=None): perc_batch_shuffle_n, a list of n ids that is no
        list of the lattice -- the outputs only, the rank buffers left alone."""
        sd = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        if n is not None:
            if list is not None:
                raise ValueError("list or n, not both")
            N = int(n)
        else:
            N = self.nb if int(list) == L.BOND else self.t
        o = np.zeros((len(sd), max(N, 0) + 1), dtype=np.int32) if orders else None
        r = np.zeros((len(sd), max(N, 0)), dtype=np.int32) if ranks else None
        if n is not None:
            L.check(L.lib().perc_batch_shuffle_n(self.h, N, len(sd), L.ptr(sd), L.ptr(o), L.ptr(r)),
                    "perc_batch_shuffle_n")
        else:
            L.check(L.lib().perc_batch_shuffle(self.h, int(list), len(sd), L.ptr(sd), L.ptr(o), L.ptr(r)),
                    "perc_batch_shuffle")
        return o, r

    def batch_cond(self, kind, item_trial, site_orders=None, bond_orders=None, item_nsites=None,
                   item_nbonds=None, rule=None, cur_rule=None, solve=True, Va=1.0, g0=1.0, leak=LEAK,
                   itol=2, tol=1e-8, itmax=2500, site_seeds=None, bond_seeds=None, weights=None,
                   item_wset=None, item_wseed=None, currents=False, cut=1e-6, voltages=False):
        """perc_batch_cond: many small bond, site or mixed realisations in one
        launch, one workgroup each.  kind BOND: bond_orders (ntrials, nb + 1)
        and item_nbonds; SITE: site_orders (ntrials, t + 1) and item_nsites;
        SITEBOND: both.  Item i occupies the first item_nsites[i] sites and
        item_nbonds[i] bonds of trial item_trial[i]'s orders.  rule=None: the
        kind's rule (the only one the kernel runs); cur_rule=None: the
        reference's own pairing (CUR_FORTRAN for BOND, CUR_MATLAB for SITE and
        SITEBOND).  Returns one dict per item with batch_bondc's keys;
        solve=False stops after the spanning test.  The dot order is the
        context's.  site_seeds / bond_seeds (one seed per trial) in place of
        the order lists: perc_batch_cond_seeded, the orders shuffled on the
        device -- the same items.  With any of weights / item_wset / item_wseed
        given: perc_batch_cond_weighted (ConductCalc.m condtype 2), the kernel
        that keeps the rows' values -- weights (nwsets, nb) per-bond multipliers
        with item_wset[i] the row item i uses (set_bond_weights(row) per item),
        or item_wseed[i] the rand('twister') seed item i draws with
        (set_conductcalc_weights(rule, seed) per item); order lists only.
        currents=True: perc_batch_cond_currents (or its seeded form) -- every
        item's dict gains the bond-current record of current_stats_host
        (nbonds, nabove at `cut`, imax, s1, s2, s4, s6, hist as an int array;
        all zero where nothing spans) and, with voltages=True, vint (N
        doubles).  The default kernel only (batch_currents_supported); not
        with weights, not with solve=False.  cut must sit above the solver's
        noise on the dangling ends: about 1e-9 of imax at tol=1e-8."""
        kind = int(kind)
        weighted = weights is not None or item_wset is not None or item_wseed is not None
        if currents and weighted:
            raise ValueError("currents=True does not go with weights / item_wset / item_wseed")
        if currents and not solve:
            raise ValueError("currents=True always solves (no solve=False)")
        if voltages and not currents:
            raise ValueError("voltages=True goes with currents=True")
        if rule is None:
            rule = KIND_RULE.get(kind, -1)  # (an unknown kind: libperc reports it)
        if cur_rule is None:
            cur_rule = natural_cur_rule(kind)
        it = np.ascontiguousarray(item_trial, dtype=np.int32).reshape(-1)
        so, bo, ntrials, seeded = self._trial_lists(site_orders, bond_orders, site_seeds, bond_seeds)
        if ntrials is None:
            ntrials = int(it.max()) + 1 if len(it) else 0  # (no list at all: libperc reports it)
        it, ns, nbc = self._item_lists(it, item_nsites, item_nbonds)
        out = (L.BatchItem * max(len(it), 1))()
        if weights is not None or item_wset is not None or item_wseed is not None:
            if seeded:
                raise ValueError("weights go with order lists, not seeds")
            w = ws = wd = None
            if weights is not None:
                w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, self.nb)
            if item_wset is not None:
                ws = np.ascontiguousarray(item_wset, dtype=np.int32).reshape(-1)
            if item_wseed is not None:
                wd = np.ascontiguousarray(np.asarray(item_wseed, dtype=np.int64) & 0xFFFFFFFF,
                                          dtype=np.uint32).reshape(-1)
            for c in (ws, wd):
                if c is not None and c.shape != it.shape:
                    raise ValueError("item_trial and item_wset / item_wseed differ in length")
            L.check(L.lib().perc_batch_cond_weighted(
                self.h, kind, int(rule), int(cur_rule), ntrials, L.ptr(so), L.ptr(bo), len(it), L.ptr(it),
                L.ptr(ns), L.ptr(nbc), 0 if w is None else w.shape[0], L.ptr(w), L.ptr(ws), L.ptr(wd),
                1 if solve else 0, Va, g0, leak, itol, tol, itmax, C.cast(out, C.c_void_p)),
                "perc_batch_cond_weighted")
            return [{k: getattr(out[i], k) for k, _ in L.BatchItem._fields_} for i in range(len(it))]
        if currents:
            name = "perc_batch_cond_currents_seeded" if seeded else "perc_batch_cond_currents"
            cur = np.zeros(max(len(it), 1), dtype=L.CURRENTS_DTYPE)
            vint = np.zeros((max(len(it), 1), self.N), dtype=np.float64) if voltages else None
            L.check(getattr(L.lib(), name)(self.h, kind, int(rule), int(cur_rule), ntrials, L.ptr(so),
                                           L.ptr(bo), len(it), L.ptr(it), L.ptr(ns), L.ptr(nbc), Va, g0, leak,
                                           itol, tol, itmax, C.cast(out, C.c_void_p), float(cut), L.ptr(cur),
                                           L.ptr(vint)), name)
            cols = [(k, cur[k].tolist()) for k in L.CURRENTS_KEYS[:-1]]  # (columns at once: no per-item numpy)
            hist = cur["hist"].copy()
            res = []
            for i in range(len(it)):
                d = {k: getattr(out[i], k) for k, _ in L.BatchItem._fields_}
                for k, col in cols:
                    d[k] = col[i]
                d["hist"] = hist[i]
                if voltages:
                    d["vint"] = vint[i]
                res.append(d)
            return res
        name = "perc_batch_cond_seeded" if seeded else "perc_batch_cond"
        L.check(getattr(L.lib(), name)(self.h, kind, int(rule), int(cur_rule), ntrials, L.ptr(so),
                                       L.ptr(bo), len(it), L.ptr(it), L.ptr(ns), L.ptr(nbc),
                                       1 if solve else 0, Va, g0, leak, itol, tol, itmax,
                                       C.cast(out, C.c_void_p)), name)
        return [{k: getattr(out[i], k) for k, _ in L.BatchItem._fields_} for i in range(len(it))]

    def batch_twister(self, seeds, n):
        """perc_batch_twister: n draws of rand('twister', seed) per seed on the
        device (k_twister_stream, one wave per seed), bit for bit
        twister_uniform(seed, n).  Returns (len(seeds), n) doubles."""
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32).reshape(-1)
        n = int(n)
        out = np.zeros((len(sd), max(n, 0)))
        L.check(L.lib().perc_batch_twister(self.h, len(sd), L.ptr(sd), n, L.ptr(out)), "perc_batch_twister")
        return out

    def batch_scan(self, kind, site_orders=None, bond_orders=None, scan=L.BOND, fixed=None):
        """perc_batch_scan: many small threshold-scan trials in one launch,
        one workgroup bisecting each.  kind BOND / SITE: the scanned list's
        orders, (ntrials, N + 1) shuffled id arrays (one array for one
        trial); kind SITEBOND: both lists, scan names the scanned one and
        fixed (an int or one per trial) the occupied entries of the other.
        Returns one dict per trial (first, maxcs, span_size, nspan).
        batch_scan_seeded takes seeds in place of the order lists."""
        return self._batch_scan(kind, site_orders, bond_orders, scan, fixed, None, None, False)

    def batch_scan_seeded(self, kind, site_seeds=None, bond_seeds=None, scan=L.BOND, fixed=None):
        """perc_batch_scan_seeded: batch_scan with site_seeds / bond_seeds
        (one seed per trial) in place of the order lists, the orders shuffled
        on the device (one wave per trial) -- the same records."""
        return self._batch_scan(kind, None, None, scan, fixed, site_seeds, bond_seeds, True)

    def _batch_scan(self, kind, site_orders, bond_orders, scan, fixed, site_seeds, bond_seeds, seeded):
        fx = None
        so, bo, ntrials, _ = self._trial_lists(site_orders, bond_orders, site_seeds, bond_seeds)
        if fixed is not None:
            fx = np.ascontiguousarray(fixed, dtype=np.int32).reshape(-1)
            if ntrials is not None and len(fx) == 1:
                fx = np.full(ntrials, fx[0], dtype=np.int32)
            if ntrials is not None and len(fx) != ntrials:
                raise ValueError("fixed: one value, or one per trial")
            ntrials = len(fx)
        if ntrials is None:
            ntrials = 1  # (no list at all: libperc reports it)
        out = (L.ScanItem * max(ntrials, 1))()
        name = "perc_batch_scan_seeded" if seeded else "perc_batch_scan"
        L.check(getattr(L.lib(), name)(self.h, int(kind), int(scan), ntrials, L.ptr(so), L.ptr(bo),
                                       L.ptr(fx), C.cast(out, C.c_void_p)), name)
        return [{k: getattr(out[i], k) for k, _ in L.ScanItem._fields_} for i in range(ntrials)]

    def batch_clusters(self, kind, item_trial, site_orders=None, bond_orders=None, item_nsites=None,
                       item_nbonds=None, nexact=0, site_seeds=None, bond_seeds=None, hist=True, geometry=False,
                       geometry_rows=True):
        """perc_batch_clusters: the cluster table's statistics of many small
        (trial, nsites, nbonds) items in one launch, one workgroup each -- the
        items, orders and counts of batch_cond.  Returns (records, hist): a
        structured array (CLUSTER_DTYPE: nclusters, nlone, nspan, span_root,
        span_size, maxcs, s1, s2, span_s1, span_s2) and the (nitems, nexact +
        32) int32 histogram rows -- hist[i, s - 1] clusters of size s <= nexact,
        hist[i, nexact + floor(log2 s)] every cluster (hist=False: no rows
        are formed, None).  site_seeds / bond_seeds (one seed per trial) in
        place of the order lists: perc_batch_clusters_seeded, the orders
        shuffled on the device -- the same records.  geometry=True
        (perc_batch_clusters_geom, pbc = 0): returns (records, hist, geom,
        rows) -- records and hist as without it, geom a GEOM_DTYPE array (n1,
        n2, g2, the spanning clusters' span_n1, span_n2, span_g2, the largest
        cluster's big_root, big_n, big_g2, the span_root cluster's root_n,
        root_g2) and rows the (nitems, 96) int64 octave rows (count, sum
        n_c^2, sum G_c per floor(log2 n_c); geometry_rows=False: None)."""
        kind, nexact = int(kind), int(nexact)
        it = np.ascontiguousarray(item_trial, dtype=np.int32).reshape(-1)
        so, bo, ntrials, seeded = self._trial_lists(site_orders, bond_orders, site_seeds, bond_seeds)
        if ntrials is None:
            ntrials = int(it.max()) + 1 if len(it) else 0  # (no list at all: libperc reports it)
        it, ns, nbc = self._item_lists(it, item_nsites, item_nbonds)
        out = np.zeros(max(len(it), 1), dtype=L.CLUSTER_DTYPE)
        hrows = np.zeros((max(len(it), 1), max(nexact, 0) + 32), dtype=np.int32) if hist else None
        if geometry:
            geom = np.zeros(max(len(it), 1), dtype=L.GEOM_DTYPE)
            grows = np.zeros((max(len(it), 1), L.GEOM_ROW), dtype=np.int64) if geometry_rows else None
            name = "perc_batch_clusters_geom_seeded" if seeded else "perc_batch_clusters_geom"
            L.check(getattr(L.lib(), name)(self.h, kind, ntrials, L.ptr(so), L.ptr(bo), len(it), L.ptr(it),
                                           L.ptr(ns), L.ptr(nbc), nexact, L.ptr(out), L.ptr(hrows), L.ptr(geom),
                                           L.ptr(grows)), name)
            return (out[:len(it)], (hrows[:len(it)] if hist else None), geom[:len(it)],
                    (grows[:len(it)] if geometry_rows else None))
        name = "perc_batch_clusters_seeded" if seeded else "perc_batch_clusters"
        L.check(getattr(L.lib(), name)(self.h, kind, ntrials, L.ptr(so), L.ptr(bo), len(it), L.ptr(it),
                                       L.ptr(ns), L.ptr(nbc), nexact, L.ptr(out), L.ptr(hrows)), name)
        return out[:len(it)], (hrows[:len(it)] if hist else None)

    def bondc_realisation(self, order, tbonds, Va=1.0, g0=1.0, tol=1e-8, itmax=2500,
                          device_ptr=None):
        """occupy + label + conductance.  `order` is a host int32 array, or
        pass device_ptr (int address of a device int32 array) instead."""
        r = L.Realisation()
        if device_ptr is not None:
            src, on_dev = C.c_void_p(device_ptr), 1
        else:
            order = np.ascontiguousarray(order, dtype=np.int32)
            src, on_dev = L.ptr(order), 0
        L.check(L.lib().perc_bondc_realisation(self.h, tbonds, src, on_dev, Va, g0, tol, itmax,
                                               C.byref(r)), "perc_bondc_realisation")
        out = {k: getattr(r.label, k) for k, _ in L.LabelInfo._fields_}
        out.update({k: getattr(r.cond, k) for k, _ in L.CondResult._fields_})
        out.update(t_upload_ms=r.t_upload_ms, t_label_ms=r.t_label_ms,
                   t_total_ms=r.t_total_ms)
        return out


# ---------------------------------------------------------------- programs
def dslab_solve_group(ctxs, xport=L.XPORT_RCCL, rule=L.RULE_BOND, cur_rule=L.CUR_FORTRAN, Va=1.0,
                      g0=1.0, leak=LEAK, itol=2, tol=1e-8, itmax=2500, full_x=False):
    """One solve split over the labeled contexts `ctxs` (slab s on ctxs[s]),
    the whole loop inside libperc: perc_dslab_solve_group (RCCL over the
    contexts' devices, or staged through the host)."""
    K = len(ctxs)
    arr = (C.c_void_p * K)(*[c.h for c in ctxs])
    res = L.CondResult()
    L.check(L.lib().perc_dslab_solve_group(K, arr, int(xport), rule, cur_rule, Va, g0, leak, itol,
                                           tol, itmax, int(full_x), C.byref(res)),
            "perc_dslab_solve_group")
    return {k: getattr(res, k) for k, _ in L.CondResult._fields_}


def bondc(lattice=0, m=50, n=50, pbc=0, pb=0.50, seed=626504, Va=1.0, g0=1.0, tol=1e-8,
          itmax=2500, labels=True, ctx=None, device=0):
    """One bond realisation filled to pb, spanning test, conductance
    (Fortran/Square/bondc.f; triangular defaults pb=.35, seed=62703)."""
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        nb = ctx.nb
        order = shuffled_ids(nb, seed)
        tbonds = int(pb * nb)  # bondc.f:191
        ctx.occupy(L.BOND, bond_order=order, nbonds_=tbonds)
        li = ctx.label()
        out = dict(nb=nb, tbonds=tbonds, order=order, nspan=li["nspan"],
                   span_root=li["span_root"], span_sites=li["span_sites"])
        if labels:
            ln = ctx.label_numbers(L.BOND)
            out.update(label=ln["bond_label"], csize=ln["csize"], cln=ln["cln"],
                       maxcn=ln["maxcn"], maxcs=ln["maxcs"], perccln=ln["perccln"],
                       perccls=int(ln["csize"][ln["perccln"]]) if ln["perccln"] else 0)
        c = ctx.conductance(L.RULE_BOND, L.CUR_FORTRAN, Va, g0, LEAK, 2, tol, itmax)
        out.update(gtop=c["gtop"], gbot=c["gbot"], iter=c["iter"], err=c["err"],
                   cond_status=c["status"])
        return out
    finally:
        if own:
            ctx.close()


def site(lattice=0, m=50, n=50, pbc=0, ps=0.60, seed=1080115, conductance=False, Va=1.0,
         g0=1.0, tol=1e-8, itmax=100000, cur_rule=L.CUR_MATLAB, ctx=None, device=0):
    """Site realisation (Fortran/Square/site.f) and, optionally, the
    ConductCalc.m site-rule conductance of its spanning cluster."""
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        t = ctx.t
        order = shuffled_ids(t, seed)
        tsites = int(ps * t)
        ctx.occupy(L.SITE, site_order=order, nsites=tsites)
        li = ctx.label()
        ln = ctx.label_numbers(L.SITE)
        out = dict(order=order, tsites=tsites, site_label=ln["site_label"], csize=ln["csize"],
                   cln=ln["cln"], maxcn=ln["maxcn"], maxcs=ln["maxcs"], perccln=ln["perccln"],
                   nspan=li["nspan"], span_root=li["span_root"])
        if conductance:
            c = ctx.conductance(L.RULE_SITE, cur_rule, Va, g0, LEAK, 2, tol, itmax)
            out.update(gtop=c["gtop"], gbot=c["gbot"], iter=c["iter"], err=c["err"])
        return out
    finally:
        if own:
            ctx.close()


def sitebond(lattice=0, m=50, n=50, pbc=0, ps=0.50, pb=0.50, sseed=143285, bseed=43716,
             conductance=False, Va=1.0, g0=1.0, tol=1e-8, itmax=100000, cur_rule=L.CUR_MATLAB,
             ctx=None, device=0):
    """Mixed site-then-bond realisation (Fortran/Square/sitebond.f) and,
    optionally, the ConductCalc.m mixed-rule conductance."""
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        t, nb = ctx.t, ctx.nb
        sorder = shuffled_ids(t, sseed)   # sitebond.f:129-143
        border = shuffled_ids(nb, bseed)  # sitebond.f:177-189
        ts, tb = int(ps * t), int(pb * nb)
        ctx.occupy(L.SITEBOND, site_order=sorder, nsites=ts, bond_order=border, nbonds_=tb)
        li = ctx.label()
        ln = ctx.label_numbers(L.SITEBOND)
        out = dict(sorder=sorder, border=border, site_label=ln["site_label"],
                   bond_label=ln["bond_label"], csize=ln["csize"], cln=ln["cln"],
                   maxcn=ln["maxcn"], maxcs=ln["maxcs"], perccln=ln["perccln"],
                   nspan=li["nspan"], span_root=li["span_root"])
        if conductance:
            c = ctx.conductance(L.RULE_MIXED, cur_rule, Va, g0, LEAK, 2, tol, itmax)
            out.update(gtop=c["gtop"], gbot=c["gbot"], iter=c["iter"], err=c["err"])
        return out
    finally:
        if own:
            ctx.close()


def bondsite(lattice=0, m=10, n=10, pbc=0, ps=0.50, pb=0.50, sseed=143285, bseed=43716):
    """Mixed bonds-then-sites realisation (Fortran/Square/bondsite.f): bonds
    to pb (seed bseed), each a size-1 cluster, then sites to ps (seed sseed)
    merging their neighbour bonds' clusters; reference numbering by host
    replay (perc_replay_labels, PERC_BONDSITE).  Also the drop-in text of
    bssite.txt / bsbond.txt (bondsite.f:420-430)."""
    t, nb = m * n, nbonds(lattice, m, n, pbc)
    sorder = shuffled_ids(t, sseed)   # bondsite.f:116-127
    border = shuffled_ids(nb, bseed)  # bondsite.f:153-166
    ts, tb = int(ps * t), int(pb * nb)
    r = replay_labels(lattice, m, n, pbc, L.BONDSITE, site_order=sorder, nsites=ts,
                      bond_order=border, nbond=tb)
    b1, b2 = bond_list(lattice, m, n, pbc)
    s_ext = np.zeros(nb + 1, dtype=np.int64)
    s_ext[1:min(t, nb) + 1] = r["site_label"][:min(t, nb)]
    c = r["csize"]
    r["bssite"] = fmt_i10(np.arange(1, nb + 1), s_ext[1:], c[1:nb + 1])
    r["bsbond"] = fmt_i10(b1, b2, r["bond_label"])
    r.update(sorder=sorder, border=border)
    return r


def twister_uniform(seed, n):
    """n draws of rand('twister', seed): MT19937 init_genrand(seed), 53-bit
    genrand_res53 doubles (perc_twister_uniform, host C)."""
    out = np.empty(max(int(n), 1))
    L.check(L.lib().perc_twister_uniform(int(seed) & 0xFFFFFFFF, int(n), out.ctypes.data),
            "perc_twister_uniform")
    return out[:n]


def conductcalc_weights(rule, b1, b2, bond_label, site_label, perccln, seed=1838534):
    """ConductCalc.m condtype 2 (MATLAB/ConductCalc.m:38-47, 94-97, 114-118,
    136-146): the bonds that get -g0 under the rule get -g0*rand instead,
    one rand per such bond in bond-list order from rand('twister', seed).
    MATLAB's 'twister' is MT19937 seeded by init_genrand(seed) with 53-bit
    doubles (genrand_res53) -- the generator numpy.random.RandomState(seed)
    .random_sample implements.  Parity with MATLAB itself is unpinned (no
    MATLAB here).  Returns w (1.0 for the other bonds)."""
    nb = len(b1)
    if rule == L.RULE_BOND:
        mask = bond_label == perccln
    else:
        both = (site_label[b1 - 1] == perccln) & (site_label[b2 - 1] == perccln)
        mask = both if rule == L.RULE_SITE else both & (bond_label == perccln)
    w = np.ones(nb)
    w[mask] = np.random.RandomState(seed).random_sample(int(mask.sum()))
    return w


def pb_grid(lattice, nb):
    """nbarr of bond_cond.f:84-97 (square 0.49.., triangular 0.35.., +5e-3)."""
    pbarr = np.zeros(250)
    pbarr[0] = 0.35 if lattice else 0.49
    npts = 131 if lattice else 103
    for i in range(1, npts):
        pbarr[i] = pbarr[i - 1] + 5.00e-03
    return (pbarr * nb).astype(np.int64).astype(np.int32)  # truncation (H3 repeats kept)


def first_spanning(ctx, order, kind=L.BOND, n=None, on_device=False):
    """Smallest count c such that occupying order[:c] spans (the pc step of
    bond_cond.f:381; bond_perc.f / site_perc.f), 0 if none: perc_first_spanning,
    a bisection with the GPU labeling.  The context is left occupied at c.
    on_device: `order` is the int address of a device int32 array on the
    context's device (kept alive by the caller while the context uses it)."""
    n = (ctx.nb if kind == L.BOND else ctx.t) if n is None else n
    first = C.c_int()
    if on_device:
        src = C.c_void_p(order) if order else None
    else:
        o = np.ascontiguousarray(order[:n], dtype=np.int32)
        src = L.ptr(o)
    L.check(L.lib().perc_first_spanning(ctx.h, kind, src, n, 1 if on_device else 0, C.byref(first)),
            "perc_first_spanning")
    return first.value


def threshold_scan(lattice=0, m=50, n=50, pbc=0, kind=L.BOND, master=58302, numtrials=10,
                   ctx=None, device=0, replay=False, batch=0, device_shuffle=False):
    """bond_perc / site_perc (Fortran/Square/bond_perc.f, site_perc.f): per
    trial ii, seed tseed(ii) = int(rand(0)*1e6)+1, the reference shuffle,
    then the first occupation count that spans; the record is (tseed,
    fraction = REAL*4 count/N, largest cluster size, spanning cluster size)
    at that step (the whole order if nothing spans), sizes on the GPU
    (perc_cluster_sizes; replay=True: by the host label replay, which also
    gives the reference label number perccln).  batch > 0 (on a lattice
    scan_supported accepts, without replay): the orders of `batch` trials at
    a time shuffled on the host, one perc_batch_scan call per group -- the
    same records.  device_shuffle=True (with batch > 0, on such a lattice,
    ignored otherwise): the group's orders shuffled on the device from the
    seeds (perc_batch_scan_seeded), no shuffled_ids call -- the same records."""
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        N = ctx.nb if kind == L.BOND else ctx.t
        seeds = trial_seeds(master, max(numtrials, 1), scale=1000000)
        out = []
        if batch > 0 and not replay and scan_supported(ctx.lattice, ctx.m, ctx.n, ctx.pbc):
            for i0 in range(0, numtrials, batch):
                sd = seeds[i0:min(i0 + batch, numtrials)]
                if device_shuffle and _device_shuffle_ok(ctx, kind):
                    res = ctx.batch_scan_seeded(kind, **{"bond_seeds" if kind == L.BOND else "site_seeds": sd})
                else:
                    orders = np.stack([shuffled_ids(N, int(s)) for s in sd])
                    res = ctx.batch_scan(kind, **{"bond_orders" if kind == L.BOND else "site_orders": orders})
                for s, r in zip(sd, res):
                    c = r["first"] if r["first"] else N
                    out.append(dict(tseed=int(s), count=c,
                                    f=float(np.float32(np.float32(c) / np.float32(N))),
                                    maxcs=r["maxcs"], perccls=r["span_size"] if r["first"] else 0,
                                    perccln=None))
            return out
        for ii in range(numtrials):
            order = shuffled_ids(N, int(seeds[ii]))
            first = first_spanning(ctx, order, kind, N)
            c = first if first else N
            if replay:  # reference label numbers too (host replay)
                r = ctx.label_numbers(kind)
                maxcs, perccln = r["maxcs"], r["perccln"]
                perccls = int(r["csize"][perccln]) if first and perccln else 0
            else:  # the two sizes the record needs, on the GPU
                maxcs, span = ctx.cluster_sizes()
                perccls, perccln = (span if first else 0), None
            out.append(dict(tseed=int(seeds[ii]), count=c,
                            f=float(np.float32(np.float32(c) / np.float32(N))),
                            maxcs=maxcs, perccls=perccls, perccln=perccln))
        return out
    finally:
        if own:
            ctx.close()


def first_spanning_mixed(ctx, scan, site_order, nsites, bond_order, nbonds, on_device=False):
    """perc_first_spanning_mixed: sites fixed and bonds scanned (scan=BOND,
    sb_perc) or bonds fixed and sites scanned (scan=SITE, bs_perc).
    on_device: site_order and bond_order are the int addresses of device
    int32 arrays on the context's device."""
    first = C.c_int()
    if on_device:
        sp = C.c_void_p(site_order) if site_order else None
        bp = C.c_void_p(bond_order) if bond_order else None
    else:
        so = np.ascontiguousarray(site_order[:max(nsites, 1)], dtype=np.int32)
        bo = np.ascontiguousarray(bond_order[:max(nbonds, 1)], dtype=np.int32)
        sp, bp = L.ptr(so), L.ptr(bo)
    L.check(L.lib().perc_first_spanning_mixed(ctx.h, scan, sp, nsites, bp, nbonds,
                                              1 if on_device else 0, C.byref(first)),
            "perc_first_spanning_mixed")
    return first.value


def bs_perc_replay(lattice, m, n, pbc, site_order, nsites, bond_order, nbond, c0_overflow=True):
    """perc_bs_perc_replay: bs_perc's site scan by host replay (first
    spanning site count); c0_overflow reproduces the reference build
    (hazard H11), False gives the intended site+bond connectivity."""
    so = np.ascontiguousarray(site_order[:max(nsites, 1)], dtype=np.int32)
    bo = np.ascontiguousarray(bond_order[:max(nbond, 1)], dtype=np.int32)
    first = C.c_int()
    L.check(L.lib().perc_bs_perc_replay(lattice, m, n, pbc, L.ptr(so), nsites, L.ptr(bo), nbond,
                                        int(c0_overflow), C.byref(first)), "perc_bs_perc_replay")
    return first.value


def paired_seeds(pseed, k=1000):
    """sseed(jj), bseed(jj) = int(rand(0)*1e7)+1 drawn alternately after
    srand(pseed) (sb_perc.f / bs_perc.f:106-111)."""
    lib = L.lib()
    lib.perc_srand(int(pseed))
    ss, bs = _i32(k), _i32(k)
    for j in range(k):
        ss[j] = int(np.float32(lib.perc_rand(0)) * np.float32(10000000)) + 1
        bs[j] = int(np.float32(lib.perc_rand(0)) * np.float32(10000000)) + 1
    return ss, bs


def mixed_scan(lattice=0, m=50, n=50, pbc=0, scan=L.BOND, master=8811064, points=None,
               iters=100, as_built=True, ctx=None, device=0, batch=0, device_shuffle=False):
    """sb_perc (scan=BOND: sites fixed at ps, bonds added until a mixed
    cluster spans; Square/sb_perc.f) / bs_perc (scan=SITE: bonds fixed at
    pb, sites added; Square/bs_perc.f).  points: the ps (sb) / pb (bs)
    values, default the reference's (square 0.59 + 0.01 i x 42, triangular
    0.50 + 0.01 i x 51) / 0.30 + 0.01 i x 71.  Records (sseed, bseed, ps,
    pb); the scanned fraction is 0 when nothing spans.  sb_perc's first
    spanning bond count is the GPU bisection (perc_first_spanning_mixed);
    bs_perc's is the host replay of the reference as built (as_built, hazard
    H11) or, with as_built=False, the GPU bisection of the intended rule.
    batch > 0 (on a lattice scan_supported accepts; not the as-built bs_perc,
    a host replay): the GPU bisections of `batch` trials at a time in one
    perc_batch_scan call -- the same records.  device_shuffle=True (with
    batch > 0 taking effect, ignored otherwise): both orders of those trials
    shuffled on the device from sseed / bseed (perc_batch_scan_seeded)."""
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        t, nb = ctx.t, ctx.nb
        if points is None:
            if scan == L.BOND:
                points = ([0.59 + 0.01 * i for i in range(42)] if lattice == 0
                          else [0.50 + 0.01 * i for i in range(51)])
            else:
                points = [0.30 + 0.01 * i for i in range(71)]
        pseed = trial_seeds(master, 100)
        out = []
        if (batch > 0 and not (scan == L.SITE and as_built)
                and scan_supported(ctx.lattice, ctx.m, ctx.n, ctx.pbc)):
            for ii, pt in enumerate(points):
                ss, bs = paired_seeds(pseed[ii])
                fx = int(pt * t) if scan == L.BOND else int(pt * nb)  # sb_perc.f:210, bs_perc.f:209
                for j0 in range(0, iters, batch):
                    jr = range(j0, min(j0 + batch, iters))
                    if device_shuffle and _device_shuffle_ok(ctx, L.SITEBOND):
                        res = ctx.batch_scan_seeded(L.SITEBOND, site_seeds=ss[jr.start:jr.stop],
                                                    bond_seeds=bs[jr.start:jr.stop], scan=scan, fixed=fx)
                    else:
                        so = np.stack([shuffled_ids(t, int(ss[jj])) for jj in jr])
                        bo = np.stack([shuffled_ids(nb, int(bs[jj])) for jj in jr])
                        res = ctx.batch_scan(L.SITEBOND, site_orders=so, bond_orders=bo, scan=scan, fixed=fx)
                    for jj, r in zip(jr, res):
                        first = r["first"]
                        if scan == L.BOND:
                            ps = float(np.float32(fx) / np.float32(t))
                            pb = float(np.float32(first) / np.float32(nb)) if first else 0.0
                        else:
                            pb = float(np.float32(fx) / np.float32(nb))
                            ps = float(np.float32(first) / np.float32(t)) if first else 0.0
                        out.append(dict(sseed=int(ss[jj]), bseed=int(bs[jj]), ps=ps, pb=pb, first=first))
            return out
        for ii, pt in enumerate(points):
            ss, bs = paired_seeds(pseed[ii])
            for jj in range(iters):
                so = shuffled_ids(t, int(ss[jj]))
                bo = shuffled_ids(nb, int(bs[jj]))
                if scan == L.BOND:
                    ts = int(pt * t)  # sb_perc.f:210 (truncation)
                    first = first_spanning_mixed(ctx, L.BOND, so, ts, bo, nb)
                    ps = float(np.float32(ts) / np.float32(t))
                    pb = float(np.float32(first) / np.float32(nb)) if first else 0.0
                else:
                    tb = int(pt * nb)  # bs_perc.f:209
                    if as_built:
                        first = bs_perc_replay(lattice, m, n, pbc, so, t, bo, tb, True)
                    else:
                        first = first_spanning_mixed(ctx, L.SITE, so, t, bo, tb)
                    pb = float(np.float32(tb) / np.float32(nb))
                    ps = float(np.float32(first) / np.float32(t)) if first else 0.0
                out.append(dict(sseed=int(ss[jj]), bseed=int(bs[jj]), ps=ps, pb=pb, first=first))
        return out
    finally:
        if own:
            ctx.close()


def fmt_mixed_rows(rows):
    """sb_perc.txt / bs_perc.txt records: (i10,",",i10,",",f12.9,",",f12.9)."""
    return "".join("%10d,%10d,%12.9f,%12.9f\n" % (r["sseed"], r["bseed"], r["ps"], r["pb"])
                   for r in rows)


def fmt_perc_rows(rows):
    """bond_perc.txt / site_perc.txt records: (i10,",",f12.9,",",i10,",",i10)."""
    return "".join("%10d,%12.9f,%10d,%10d\n" % (r["tseed"], r["f"], r["maxcs"], r["perccls"])
                   for r in rows)


def bond_cond_grid(lattice=0, m=10, n=10, pbc=0, master=58302, numtrials=1, Va=1.0, g0=1.0,
                   tol=1e-8, itmax=2500, trials=None, with_labels=True, ctx=None, device=0):
    """bond_cond (Fortran/Square/bond_cond.f:123-498): per trial ii, seed
    tseed(ii), conductance of the lowest-label spanning cluster at each
    grid point nbarr(jj) until the sweep ends (or stalls on a repeated
    nbarr value, hazard H3), pc = first spanning fraction, and the final
    lowest spanning label."""
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        nb = ctx.nb
        seeds = trial_seeds(master, 1000)
        nbarr = pb_grid(lattice, nb)
        out = []
        for ii in (trials if trials is not None else range(numtrials)):
            order = shuffled_ids(nb, int(seeds[ii]))
            rows = []
            jj = 0
            for bf in nbarr:
                if bf <= 0 or jj >= len(nbarr) or bf != nbarr[jj]:
                    break
                if rows and bf <= rows[-1]["bf"]:
                    break  # H3: repeated nbarr value stalls the sweep
                ctx.occupy(L.BOND, bond_order=order, nbonds_=int(bf))
                li = ctx.label()
                c = ctx.conductance(L.RULE_BOND, L.CUR_FORTRAN, Va, g0, LEAK, 2, tol, itmax)
                pbv = float(np.float32(np.float32(bf) / np.float32(nb)))
                rows.append(dict(bf=int(bf), pb=pbv, gbot=c["gbot"], gtop=c["gtop"],
                                 iter=c["iter"], spanning=li["nspan"] > 0))
                jj += 1
            bfc = first_spanning(ctx, order)
            pc = float(np.float32(np.float32(bfc) / np.float32(nb))) if bfc else 0.0
            tr = dict(ii=ii + 1, seed=int(seeds[ii]), rows=rows, pc=pc, bf_c=bfc)
            if with_labels:
                ctx.occupy(L.BOND, bond_order=order, nbonds_=nb)
                tr["perccln"] = ctx.label_numbers(L.BOND)["perccln"] if bfc else 0
            out.append(tr)
        return out
    finally:
        if own:
            ctx.close()


def cond_curve(lattice=0, m=50, n=50, pbc=0, kind=L.SITE, grid=(0.6, 0.7, 0.8, 0.9, 1.0), master=58302,
               numtrials=1, batch=256, cur_rule=None, Va=1.0, g0=1.0, tol=1e-8, itmax=2500, ctx=None,
               device=0, device_shuffle=False, large=False, condtype=1, wseed=1838534):
    """The mean conductance curve of site or mixed percolation over trials:
    G(ps) (kind SITE, site.f + ConductCalc.m's site rule; grid a list of ps) or
    G(ps, pb) (kind SITEBOND, sitebond.f + the mixed rule; grid a list of
    (ps, pb)).  Trial ii draws its orders once -- shuffled_ids(t, tseed(ii))
    with trial_seeds(master) for SITE; shuffled_ids(t, sseed(ii)) and
    shuffled_ids(nb, bseed(ii)) with paired_seeds(master), the alternate draw
    of sb_perc.f / mixed_scan, for SITEBOND -- and every grid point occupies
    the first int(ps * t) sites and int(pb * nb) bonds of them (site.f /
    sitebond.f's truncation).  batch > 0 on a lattice batch_cond_supported
    accepts: the (trial, point) items of about `batch` at a time (whole
    trials) through Context.batch_cond; batch=0, or another lattice: each item
    through occupy / label / conductance.  device_shuffle=True (where the batch
    path runs, ignored otherwise): the group's orders shuffled on the device
    from the seeds (perc_batch_cond_seeded), the same results bit for bit.
    large=True: the context's set_batch_large flag set for the call (restored
    after it) and batch_large_supported in place of batch_cond_supported, so
    the batch path runs up to 128 x 128.
    condtype=2 (ConductCalc.m's random conductances): item (trial index ii,
    point j) draws its bond weights with seed (wseed + ii * npts + j) mod 2^32
    -- batched (where batch_weighted_supported accepts the lattice) through
    batch_cond's item_wseed, else set_conductcalc_weights after label() and
    set_bond_weights(None) after the solve; the orders come from the host
    (device_shuffle is ignored), large=True is a ValueError.
    cur_rule=None: CUR_MATLAB, the
    reference's pairing.  The dot order is the context's (ctx).  Returns
    (trials, stats): per trial dict(ii, seed | sseed, bseed, rows) with one row
    per grid point (ps, [pb,] nsites, [nbonds,] gbot, gtop, iter, spanning),
    and the (npts, 5) statistics {count, sum Gtop, sum Gtop^2, count spanning,
    sum iter} accumulated by perc_stats_accumulate in ascending (trial, point)
    order -- the same sums in the same order either way, in the shape
    Ensemble.bond_cond returns."""
    if kind not in (L.SITE, L.SITEBOND):
        raise ValueError("cond_curve: kind SITE or SITEBOND (bond: Ensemble.bond_cond)")
    if numtrials < 0:
        raise ValueError("numtrials < 0")
    if condtype not in (1, 2):
        raise ValueError("cond_curve: condtype 1 or 2")
    if condtype == 2 and large:
        raise ValueError("cond_curve: condtype 2 has its own batch kernel (no large=True)")
    mixed = kind == L.SITEBOND
    rule = KIND_RULE[kind]
    if cur_rule is None:
        cur_rule = natural_cur_rule(kind)
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    was_large = ctx.batch_large()
    try:
        if large:
            ctx.set_batch_large(True)
        t, nb = ctx.t, ctx.nb
        pts = [(float(p[0]), float(p[1])) if mixed else (float(p), None) for p in grid]
        npts = len(pts)
        cnt_s = np.array([int(ps * t) for ps, _ in pts], np.int32)
        cnt_b = np.array([int(pb * nb) for _, pb in pts], np.int32) if mixed else None
        if mixed:
            ss, bs = paired_seeds(master, max(numtrials, 1))
        else:
            ss, bs = trial_seeds(master, max(numtrials, 1)), None
        supported = batch_large_supported if ctx.batch_large() else batch_cond_supported
        if condtype == 2:
            supported = batch_weighted_supported
        batched = batch > 0 and npts > 0 and supported(kind, ctx.lattice, ctx.m, ctx.n, ctx.pbc)
        group = max(1, batch // max(npts, 1)) if batched else 1
        seeded = batched and device_shuffle and condtype == 1 and _device_shuffle_ok(ctx, kind)
        stats = np.zeros(npts * 5)
        acc = L.lib().perc_stats_accumulate
        out = []
        for i0 in range(0, numtrials, group):
            tr = range(i0, min(i0 + group, numtrials))
            if seeded:
                so = bo = None
                src = dict(site_seeds=ss[tr.start:tr.stop], bond_seeds=bs[tr.start:tr.stop] if mixed else None)
            else:
                so = np.stack([shuffled_ids(t, int(ss[ii])) for ii in tr])
                bo = np.stack([shuffled_ids(nb, int(bs[ii])) for ii in tr]) if mixed else None
                src = dict(site_orders=so, bond_orders=bo)
            if batched:
                it = np.repeat(np.arange(len(tr), dtype=np.int32), npts)
                if condtype == 2:
                    src["item_wseed"] = [(wseed + ii * npts + j) & 0xFFFFFFFF for ii in tr for j in range(npts)]
                res = ctx.batch_cond(kind, it, **src,
                                     item_nsites=np.tile(cnt_s, len(tr)),
                                     item_nbonds=np.tile(cnt_b, len(tr)) if mixed else None,
                                     cur_rule=cur_rule, Va=Va, g0=g0, leak=LEAK, itol=2, tol=tol,
                                     itmax=itmax)
            else:
                res = []
                for k in range(len(tr)):
                    for j in range(npts):
                        if mixed:
                            ctx.occupy(kind, site_order=so[k], nsites=int(cnt_s[j]), bond_order=bo[k],
                                       nbonds_=int(cnt_b[j]))
                        else:
                            ctx.occupy(kind, site_order=so[k], nsites=int(cnt_s[j]))
                        li = ctx.label()
                        if condtype == 2:
                            ctx.set_conductcalc_weights(rule, (wseed + tr[k] * npts + j) & 0xFFFFFFFF)
                        c = ctx.conductance(rule, cur_rule, Va, g0, LEAK, 2, tol, itmax)
                        if condtype == 2:
                            ctx.set_bond_weights(None)
                        res.append(dict(gtop=c["gtop"], gbot=c["gbot"], iter=c["iter"], nspan=li["nspan"]))
            for k, ii in enumerate(tr):
                rows = []
                for j, (ps, pb) in enumerate(pts):
                    r = res[k * npts + j]
                    row = dict(ps=ps, nsites=int(cnt_s[j]))
                    if mixed:
                        row.update(pb=pb, nbonds=int(cnt_b[j]))
                    row.update(gbot=r["gbot"], gtop=r["gtop"], iter=r["iter"], spanning=r["nspan"] > 0)
                    rows.append(row)
                    acc(stats, j, r["gtop"], int(r["nspan"] > 0), int(r["iter"]))
                trial = dict(ii=ii + 1, rows=rows)
                if mixed:
                    trial.update(sseed=int(ss[ii]), bseed=int(bs[ii]))
                else:
                    trial.update(seed=int(ss[ii]))
                out.append(trial)
        return out, stats.reshape(npts, 5)
    finally:
        if own:
            ctx.close()
        elif large:
            ctx.set_batch_large(was_large)


def current_curve(lattice=0, m=50, n=50, pbc=0, kind=L.BOND, grid=(0.5, 0.6, 0.7, 0.8, 0.9), master=58302,
                  numtrials=1, cur_rule=None, Va=1.0, g0=1.0, tol=1e-8, itmax=2500, cut=1e-6, batch=True,
                  device_shuffle=False, ctx=None, device=0):
    """Where the current flows as a function of p over trials: the backbone
    fraction, the current moments and the current histogram of bond (grid a
    list of pb), site (ps) or mixed (a list of (ps, pb)) percolation.  Trials
    and counts are cond_curve's: trial ii draws shuffled_ids with
    trial_seeds(master) (BOND: the bond order; SITE: the site order) or
    paired_seeds(master) (SITEBOND), a grid point occupies the first
    int(ps * t) sites and int(pb * nb) bonds.  batch=True on a lattice
    batch_currents_supported accepts: all items of the call through
    Context.batch_cond(currents=True) (device_shuffle=True: from the seeds);
    batch=False, or another lattice: each item through occupy / label /
    conductance(vint=True), conducting_bonds and current_stats_host.  Returns
    (rows, records): records[ii][j] the item's dict (gtop, gbot, iter, nspan
    and the current record's keys); rows[j], over the trials of point j that
    span once or more (count `nspan`, accumulated in trial order), the means
    G of gtop, backbone of nabove / nbonds, m2, m4, m6 of s_q / I^q and imax
    of imax / I with I = gtop * Va, and the pooled hist (int64)."""
    kind = int(kind)
    if kind not in (L.BOND, L.SITE, L.SITEBOND):
        raise ValueError("current_curve: kind BOND, SITE or SITEBOND")
    if numtrials < 0:
        raise ValueError("numtrials < 0")
    mixed = kind == L.SITEBOND
    need_s, need_b = kind != L.BOND, kind != L.SITE
    rule = KIND_RULE[kind]
    if cur_rule is None:
        cur_rule = natural_cur_rule(kind)
    own = ctx is None
    ctx = ctx or Context(lattice, m, n, pbc, device)
    try:
        t, nb = ctx.t, ctx.nb
        pts = [(float(p[0]), float(p[1])) if mixed else ((float(p), None) if need_s else (None, float(p)))
               for p in grid]
        npts = len(pts)
        cnt_s = np.array([int(ps * t) for ps, _ in pts], np.int32) if need_s else None
        cnt_b = np.array([int(pb * nb) for _, pb in pts], np.int32) if need_b else None
        if mixed:
            ss, bs = paired_seeds(master, max(numtrials, 1))
        elif need_s:
            ss, bs = trial_seeds(master, max(numtrials, 1)), None
        else:
            ss, bs = None, trial_seeds(master, max(numtrials, 1))
        batched = bool(batch) and npts > 0 and numtrials > 0 and batch_currents_supported(
            kind, ctx.lattice, ctx.m, ctx.n, ctx.pbc)
        seeded = batched and device_shuffle and _device_shuffle_ok(ctx, kind)
        keys = ("gtop", "gbot", "iter", "nspan")
        if batched:
            if seeded:
                src = dict(site_seeds=ss[:numtrials] if need_s else None,
                           bond_seeds=bs[:numtrials] if need_b else None)
            else:
                src = dict(site_orders=np.stack([shuffled_ids(t, int(ss[ii])) for ii in range(numtrials)])
                           if need_s else None,
                           bond_orders=np.stack([shuffled_ids(nb, int(bs[ii])) for ii in range(numtrials)])
                           if need_b else None)
            res = ctx.batch_cond(kind, np.repeat(np.arange(numtrials, dtype=np.int32), npts), **src,
                                 item_nsites=np.tile(cnt_s, numtrials) if need_s else None,
                                 item_nbonds=np.tile(cnt_b, numtrials) if need_b else None, cur_rule=cur_rule,
                                 Va=Va, g0=g0, leak=LEAK, itol=2, tol=tol, itmax=itmax, currents=True, cut=cut)
            res = [{k: r[k] for k in keys + L.CURRENTS_KEYS} for r in res]
        else:
            b1, b2 = bond_list(ctx.lattice, ctx.m, ctx.n, ctx.pbc)
            res = []
            for ii in range(numtrials):
                so = shuffled_ids(t, int(ss[ii])) if need_s else None
                bo = shuffled_ids(nb, int(bs[ii])) if need_b else None
                for j in range(npts):
                    ctx.occupy(kind, site_order=so, nsites=int(cnt_s[j]) if need_s else 0, bond_order=bo,
                               nbonds_=int(cnt_b[j]) if need_b else 0)
                    li = ctx.label(canon=True)
                    c = ctx.conductance(rule, cur_rule, Va, g0, LEAK, 2, tol, itmax, vint=True)
                    socc, bocc = ctx.occupancy()
                    mask = conducting_bonds(kind, b1, b2, socc, bocc, li["canon"], li["span_root"])
                    if c["status"] != 0:
                        mask[:] = 0
                    r = dict(gtop=c["gtop"], gbot=c["gbot"], iter=c["iter"], nspan=li["nspan"])
                    r.update(current_stats_host(ctx.lattice, ctx.m, ctx.n, ctx.pbc, mask, c["vint"], Va, g0, cut))
                    res.append(r)
        records = [res[ii * npts:(ii + 1) * npts] for ii in range(numtrials)]
        rows = []
        for j, (ps, pb) in enumerate(pts):
            acc = dict(nspan=0, G=0.0, backbone=0.0, m2=0.0, m4=0.0, m6=0.0, imax=0.0)
            hist = np.zeros(64, dtype=np.int64)
            for ii in range(numtrials):
                r = records[ii][j]
                if r["nspan"] < 1 or r["nbonds"] < 1:
                    continue
                cur = r["gtop"] * Va
                i2 = cur * cur
                acc["nspan"] += 1
                acc["G"] += r["gtop"]
                acc["backbone"] += r["nabove"] / r["nbonds"]
                acc["m2"] += r["s2"] / i2
                acc["m4"] += r["s4"] / (i2 * i2)
                acc["m6"] += r["s6"] / (i2 * i2 * i2)
                acc["imax"] += r["imax"] / cur
                hist += r["hist"]
            k = acc["nspan"]
            row = {q: (v / k if k and q != "nspan" else v) for q, v in acc.items()}
            if need_s:
                row["ps"] = ps
            if need_b:
                row["pb"] = pb
            row["hist"] = hist
            rows.append(row)
        return rows, records
    finally:
        if own:
            ctx.close()


def cluster_curve(lattice=0, m=50, n=50, pbc=0, kind=L.BOND, grid=(0.3, 0.4, 0.5, 0.6, 0.7), master=58302,
                  numtrials=1, batch=256, nexact=64, device_shuffle=False, ctx=None, device=0):
    """Cluster statistics as a function of p over trials: the cluster-size
    distribution n_s(p), the moments behind the mean cluster size S(p), the
    spanning clusters' share P_inf(p) and the clusters per site, for bond
    (grid a list of pb), site (a list of ps) or mixed percolation (a list of
    (ps, pb)).  Seeds and orders are cond_curve's: trial ii draws
    shuffled_ids(nb, tseed(ii)) (BOND) or shuffled_ids(t, tseed(ii)) (SITE)
    with trial_seeds(master), both lists with paired_seeds(master) for
    SITEBOND; a grid point occupies the first int(ps * t) sites / int(pb * nb)
    bonds.  batch > 0 on a lattice batch_clusters_supported accepts: about
    `batch` (trial, point) items at a time (whole trials) through
    Context.batch_clusters, with device_shuffle=True the orders shuffled on
    the device from the seeds; batch=0, or another lattice: each item through
    cluster_stats_host, no device at all (ctx is not used).  The same numbers
    either way.  Returns (trials, stats, hist): per trial dict(ii, seed |
    sseed, bseed, rows) with one row per grid point (p, counts and the record's
    fields); stats (npts, 8) int64 {count, sum nclusters, count spanning, sum
    span_size, sum s1, sum s2, sum span_s1, sum span_s2}; hist (npts, nexact +
    32) int64, the items' histogram rows summed over the trials."""
    return _cluster_curve("cluster_curve", False, lattice, m, n, pbc, kind, grid, master, numtrials, batch, nexact,
                          device_shuffle, ctx, device)[:3]


GEOM_SUMS = ("n1", "n2", "g2", "span_n1", "span_n2", "span_g2", "big_n", "big_g2")


def _cluster_curve(who, geometry, lattice, m, n, pbc, kind, grid, master, numtrials, batch, nexact, device_shuffle,
                   ctx, device):
    """cluster_curve and, geometry=True, correlation_curve: (trials, stats,
    hist, gsums, grows) -- the last two None without geometry"""
    if kind not in (L.BOND, L.SITE, L.SITEBOND):
        raise ValueError("%s: kind BOND, SITE or SITEBOND" % who)
    if numtrials < 0:
        raise ValueError("numtrials < 0")
    if ctx is not None:
        lattice, m, n, pbc = ctx.lattice, ctx.m, ctx.n, ctx.pbc
    if geometry and pbc != 0:
        raise ValueError("%s: pbc = 0 only" % who)
    mixed = kind == L.SITEBOND
    need_s, need_b = kind != L.BOND, kind != L.SITE
    t, nb = m * n, nbonds(lattice, m, n, pbc)
    pts = [(float(p[0]), float(p[1])) if mixed else ((float(p), None) if need_s else (None, float(p)))
           for p in grid]
    npts = len(pts)
    cnt_s = np.array([int(ps * t) for ps, _ in pts], np.int32) if need_s else None
    cnt_b = np.array([int(pb * nb) for _, pb in pts], np.int32) if need_b else None
    if mixed:
        ss, bs = paired_seeds(master, max(numtrials, 1))
    elif need_s:
        ss, bs = trial_seeds(master, max(numtrials, 1)), None
    else:
        ss, bs = None, trial_seeds(master, max(numtrials, 1))
    supported = batch_geometry_supported if geometry else batch_clusters_supported
    batched = batch > 0 and npts > 0 and numtrials > 0 and supported(lattice, m, n, pbc, nexact)
    own = batched and ctx is None
    if own:
        ctx = Context(lattice, m, n, pbc, device)
    try:
        group = max(1, batch // max(npts, 1)) if batched else 1
        seeded = batched and device_shuffle and _device_shuffle_ok(ctx, kind)
        stats = np.zeros((npts, 8), dtype=np.int64)
        hist = np.zeros((npts, nexact + 32), dtype=np.int64)
        gsums = np.zeros((npts, 1 + len(GEOM_SUMS) + 1), dtype=np.int64) if geometry else None
        grows = np.zeros((npts, L.GEOM_ROW), dtype=np.int64) if geometry else None
        geom = rrows = None
        out = []
        for i0 in range(0, numtrials, group):
            tr = range(i0, min(i0 + group, numtrials))
            so = bo = None
            if not seeded:
                so = np.stack([shuffled_ids(t, int(ss[ii])) for ii in tr]) if need_s else None
                bo = np.stack([shuffled_ids(nb, int(bs[ii])) for ii in tr]) if need_b else None
            if batched:
                if seeded:
                    src = dict(site_seeds=ss[tr.start:tr.stop] if need_s else None,
                               bond_seeds=bs[tr.start:tr.stop] if need_b else None)
                else:
                    src = dict(site_orders=so, bond_orders=bo)
                got = ctx.batch_clusters(kind, np.repeat(np.arange(len(tr), dtype=np.int32), npts), **src,
                                         item_nsites=np.tile(cnt_s, len(tr)) if need_s else None,
                                         item_nbonds=np.tile(cnt_b, len(tr)) if need_b else None,
                                         nexact=nexact, geometry=geometry)
                recs, rows = got[:2]
                if geometry:
                    geom, rrows = got[2:]
            else:
                recs = np.zeros(len(tr) * npts, dtype=L.CLUSTER_DTYPE)
                rows = np.zeros((len(tr) * npts, nexact + 32), dtype=np.int32)
                if geometry:
                    geom = np.zeros(len(tr) * npts, dtype=L.GEOM_DTYPE)
                    rrows = np.zeros((len(tr) * npts, L.GEOM_ROW), dtype=np.int64)
                for k in range(len(tr)):
                    for j in range(npts):
                        item = (lattice, m, n, pbc, kind, so[k] if need_s else None, int(cnt_s[j]) if need_s else 0,
                                bo[k] if need_b else None, int(cnt_b[j]) if need_b else 0, nexact)
                        recs[k * npts + j], rows[k * npts + j] = cluster_stats_host(*item)
                        if geometry:
                            geom[k * npts + j], rrows[k * npts + j] = cluster_geometry_host(*item)
            for k, ii in enumerate(tr):
                trows = []
                for j, (ps, pb) in enumerate(pts):
                    r = recs[k * npts + j]
                    row = {}
                    if need_s:
                        row.update(ps=ps, nsites=int(cnt_s[j]))
                    if need_b:
                        row.update(pb=pb, nbonds=int(cnt_b[j]))
                    row.update({f: int(r[f]) for f in L.CLUSTER_DTYPE.names})
                    trows.append(row)
                    stats[j] += (1, r["nclusters"], int(r["nspan"] > 0), r["span_size"], r["s1"], r["s2"],
                                 r["span_s1"], r["span_s2"])
                    hist[j] += rows[k * npts + j]
                    if geometry:
                        q = geom[k * npts + j]
                        row.update({f: int(q[f]) for f in L.GEOM_DTYPE.names if f != "pad"})
                        gsums[j] += (1,) + tuple(int(q[f]) for f in GEOM_SUMS) + (int(q["big_n"]) ** 2,)
                        grows[j] += rrows[k * npts + j]
                trial = dict(ii=ii + 1, rows=trows)
                if mixed:
                    trial.update(sseed=int(ss[ii]), bseed=int(bs[ii]))
                else:
                    trial.update(seed=int((ss if need_s else bs)[ii]))
                out.append(trial)
        return out, stats, hist, gsums, grows
    finally:
        if own:
            ctx.close()


def correlation_curve(lattice=0, m=50, n=50, pbc=0, kind=L.BOND, grid=(0.3, 0.4, 0.5, 0.6, 0.7), master=58302,
                      numtrials=1, batch=256, nexact=64, device_shuffle=False, ctx=None, device=0):
    """The clusters' geometry as a function of p over trials: the correlation
    length xi(p), the largest cluster's radius of gyration and R_s^2 per octave
    of the cluster size (the fractal dimension's data), beside cluster_curve's
    statistics -- cluster_curve's arguments, seeds, orders and batching, the
    items through Context.batch_clusters(geometry=True) or, batch=0 or a
    lattice batch_geometry_supported refuses, through cluster_stats_host and
    cluster_geometry_host with no device; the same integers either way.
    pbc = 0 only (ValueError otherwise).  Returns a dict: trials (cluster_curve's,
    each row with the geometry record's fields too), stats and hist
    (cluster_curve's), sums (npts, 10) int64 {count, then the trials' sums of
    n1, n2, g2, span_n1, span_n2, span_g2, big_n, big_g2, big_n^2}, rows (npts,
    96) int64 the items' octave rows summed, unit (1 square, 4 triangular), and
    the derived floats xi (npts) = sqrt(2 (g2 - span_g2) / (unit (n2 -
    span_n2))), big_r2 (npts) = sum big_g2 / (unit sum big_n^2) and rs2 (npts,
    32) = rows[64 + b] / (unit rows[32 + b]); nan where a denominator is 0."""
    trials, stats, hist, sums, rows = _cluster_curve("correlation_curve", True, lattice, m, n, pbc, kind, grid, master,
                                                     numtrials, batch, nexact, device_shuffle, ctx, device)
    unit = 4 if (ctx.lattice if ctx is not None else lattice) == L.TRIANGULAR else 1

    def ratio(num, den):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.full(num.shape, np.nan), where=den != 0)

    xi = np.sqrt(ratio(2.0 * (sums[:, 3] - sums[:, 6]), unit * (sums[:, 2] - sums[:, 5])))
    return dict(trials=trials, stats=stats, hist=hist, sums=sums, rows=rows, unit=unit, xi=xi,
                big_r2=ratio(sums[:, 8], unit * sums[:, 9]), rs2=ratio(rows[:, 64:], unit * rows[:, 32:64]))


# ---------------------------------------------------------------- file output
def fmt_i10(*cols):
    """Records of (i10,",",i10,...) -- the reference's formatted writes."""
    n = len(cols[0])
    f = ",".join(["%10d"] * len(cols)) + "\n"
    return "".join(f % tuple(int(c[i]) for c in cols) for i in range(n))


# ---------------------------------------------------------------- multi-GPU ensemble
class Ensemble:
    """perc_ensemble: one context + host thread per device of this node,
    trials striped ii -> device (ii-1) mod ndev, one RCCL all-reduce of the
    per-grid-point statistics (include/perc.h; Square/bond_cond.f:123-498)."""

    def __init__(self, lattice, m, n, pbc=0, ndev=1, devices=None, workers=1, batch=0, large=False):
        self.lattice, self.m, self.n, self.pbc = lattice, m, n, pbc
        self.nb = nbonds(lattice, m, n, pbc)
        h = C.c_void_p()
        dv = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        L.check(L.lib().perc_ensemble_create(ndev, L.ptr(dv), lattice, m, n, pbc, C.byref(h)),
                "perc_ensemble_create")
        self.h = h
        self.ndev = L.lib().perc_ensemble_ndev(h)
        self.workers = 1
        if workers != 1:
            self.set_workers(workers)
        self.batch = 0
        self.large = False
        if large:
            self.set_batch_large(True)
        if batch:
            self.set_batch(batch)

    def set_batch(self, items):
        """about `items` (trial, grid point) realisations per launch of the
        batch kernel in bond_cond (perc_ensemble_set_batch; 0: the per-trial
        loop).  self.batch is what is in force: 0 on a lattice the batch
        kernel does not support (batch_supported; batch_large_supported
        after set_batch_large)."""
        L.check(L.lib().perc_ensemble_set_batch(self.h, int(items)), "perc_ensemble_set_batch")
        self.batch = L.lib().perc_ensemble_batch(self.h)

    def set_batch_large(self, enable=True):
        """perc_ensemble_set_batch_large: the batch path on the large kernel
        on every device's context, so set_batch holds up to 128 x 128"""
        L.check(L.lib().perc_ensemble_set_batch_large(self.h, int(bool(enable))),
                "perc_ensemble_set_batch_large")
        self.large = bool(enable)
        self.batch = L.lib().perc_ensemble_batch(self.h)

    def set_workers(self, workers):
        """contexts (host threads, streams) per device (perc_ensemble_set_workers)"""
        L.check(L.lib().perc_ensemble_set_workers(self.h, workers), "perc_ensemble_set_workers")
        self.workers = L.lib().perc_ensemble_workers(self.h)

    def set_dot_order(self, order):
        """perc_set_dot_order on every device's context (one worker per device)"""
        for d in range(self.ndev):
            L.check(L.lib().perc_set_dot_order(C.c_void_p(L.lib().perc_ensemble_ctx(self.h, d)), order),
                    "perc_set_dot_order")

    def close(self):
        if self.h:
            L.lib().perc_ensemble_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def allreduce(self, per_device):
        """per_device: (ndev, k) array; returns the sum over devices (RCCL)."""
        a = np.ascontiguousarray(per_device, dtype=np.float64).copy()
        k = a.shape[1]
        L.check(L.lib().perc_ensemble_allreduce(self.h, a.reshape(-1), k),
                "perc_ensemble_allreduce")
        return a

    def bond_cond(self, master=58302, numtrials=1, Va=1.0, g0=1.0, tol=1e-8, itmax=2500):
        """The bond_cond trial loop over the devices; same records as
        bond_cond_grid, plus the all-reduced statistics (npts, 5)."""
        if numtrials < 0:
            raise ValueError("numtrials < 0")
        # tseed(1..1000) as bond_cond.f:65-70, extended with the same stream past 1000
        # trials (perc_ensemble_bond_cond reads tseed[0..numtrials-1])
        seeds = trial_seeds(master, max(1000, numtrials))
        nbarr = pb_grid(self.lattice, self.nb)
        npts = len(nbarr)
        nrows, bfc, pl = _i32(numtrials), _i32(numtrials), _i32(numtrials)
        gbot, gtop = np.zeros(numtrials * npts), np.zeros(numtrials * npts)
        iters = _i32(numtrials * npts)
        stats = np.zeros(npts * 5)
        L.check(L.lib().perc_ensemble_bond_cond(self.h, numtrials, seeds, npts, nbarr, Va, g0,
                                                tol, itmax, nrows, gbot, gtop, iters, bfc, pl,
                                                stats.ctypes.data_as(C.c_void_p)),
                "perc_ensemble_bond_cond")
        out = []
        for t in range(numtrials):
            rows = []
            for j in range(nrows[t]):
                o = t * npts + j
                bf = int(nbarr[j])
                rows.append(dict(bf=bf, pb=float(np.float32(np.float32(bf) / np.float32(self.nb))),
                                 gbot=float(gbot[o]), gtop=float(gtop[o]), iter=int(iters[o])))
            b = int(bfc[t])
            out.append(dict(ii=t + 1, seed=int(seeds[t]), rows=rows, bf_c=b, perccln=int(pl[t]),
                            pc=float(np.float32(np.float32(b) / np.float32(self.nb))) if b else 0.0))
        return out, stats.reshape(npts, 5)


def ensemble_trials(ntrials, ndev, dev):
    """1-based trials device `dev` of `ndev` runs (perc_ensemble_trials)."""
    cnt = L.lib().perc_ensemble_trials(ntrials, ndev, dev, None)
    out = _i32(max(cnt, 0))
    L.lib().perc_ensemble_trials(ntrials, ndev, dev, L.ptr(out))
    return out
