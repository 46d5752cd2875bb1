/*
 * perc.h -- libperc C-ABI: MI355X-native cluster labeling + Kirchhoff
 * conductance for the IsaiahSteinke/Percolation Fortran drivers.
 *
 * Plain C types only (int32 indices, fp64 values, caller-owned host arrays).
 * Every entry returns an int status (PERC_OK == 0) where the reference would
 * `pause` (Fortran/Square/bondc.f:737,777,891,906).  One context per device
 * and host thread; no hidden globals except the gfortran-compatible RNG
 * stream (perc_srand/perc_rand), which is process-global exactly like
 * libgfortran's rand/srand.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   nearestn          Fortran/Square/bondc.f:617-715, Triangular/bondc.f:619-804
 *   bond list         Fortran/Square/bondc.f:137-154
 *   rand / srand      GNU Fortran runtime; call sites Square/bondc.f:162,167
 *   labeling loops    Square/bondc.f:194-393, Square/site.f:167-289,
 *                     Square/sitebond.f:187-400
 *   spanning test     Square/bondc.f:413-456, Square/site.f:309-344,
 *                     Square/sitebond.f:423-458
 *   assembly + solve  Square/bondc.f:465-595 (bond); MATLAB/ConductCalc.m:
 *                     88-196 (site / mixed weight rules)
 *   NR sparse layer   sprsin/linbcg/atimes/asolve/snrm/dsprsax/dsprstx,
 *                     Square/bondc.f:723-917 (symbols below, F77 ABI)
 */
#ifndef PERC_H
#define PERC_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define PERC_OK 0
#define PERC_EINVAL (-1)     /* bad argument                                  */
#define PERC_ENOMEM (-2)     /* device or host allocation failed              */
#define PERC_EHIP (-3)       /* HIP runtime error                             */
#define PERC_ENMAX (-4)      /* 'nmax too small in sprsin'  (bondc.f:737)     */
#define PERC_EITOL (-5)      /* 'illegal itol in linbcg'    (bondc.f:777)     */
#define PERC_EMISMATCH (-6)  /* 'mismatched vector and matrix' (bondc.f:891)  */
#define PERC_EREPLAY (-7)    /* label replay impossible (H7: odd-m triangular) */
#define PERC_ENODEV (-8)     /* no HIP device                                  */
#define PERC_ESTATE (-9)     /* call order violated (e.g. solve before label)  */

/* lattice kinds */
#define PERC_SQUARE 0
#define PERC_TRIANGULAR 1
/* occupancy kinds */
#define PERC_BOND 0
#define PERC_SITE 1
#define PERC_SITEBOND 2
#define PERC_BONDSITE 3  /* bonds first, then sites (Square/bondsite.f); perc_replay_labels only */
/* conductance weight rules (which bonds get g0; all others get `leak`) */
#define PERC_RULE_BOND 0     /* bond label == perccln         (bondc.f:483) */
#define PERC_RULE_SITE 1     /* both end sites in perccln     (ConductCalc.m:90) */
#define PERC_RULE_MIXED 2    /* bond and both sites in perccln (ConductCalc.m:136) */
/* terminal-current rules */
#define PERC_CUR_FORTRAN 0   /* sprsin(G,1e-10) + dsprsax, ascending sums (bondc.f:576-592) */
#define PERC_CUR_MATLAB 1    /* full G*V, Itop summed from site t down (ConductCalc.m:188-196) */

typedef struct perc_ctx perc_ctx;

/* ---- RNG: GNU Fortran rand/srand (Park-Miller 16807, 2^31-1) ----------- */
void perc_srand(int seed);
float perc_rand(int i);
/* tseed(1..k) = int(rand(0)*1e7)+1 after srand(master) (bond_cond.f:65-70) */
void perc_trial_seeds(int master, int k, int *tseed);
/* same with int(rand(0)*scale)+1: the threshold scans use scale 1e6
   (Square/bond_perc.f:70-74, Square/site_perc.f:71-75) */
void perc_trial_seeds_scaled(int master, int k, int scale, int *tseed);

/* ---- host-side lattice helpers --------------------------------------- */
int perc_nbonds(int lattice, int m, int n, int pbc);
/* nn[0..5] of site rn (1-based), 0 = none; returns scn */
int perc_nearestn(int lattice, int m, int n, int pbc, int rn, int *nn);
/* bond list b1[k] < b2[k], k = 0..nb-1 in reference order; returns nb */
int perc_bond_list(int lattice, int m, int n, int pbc, int *b1, int *b2);
/* REAL*4 Fisher-Yates of a 1-based id permutation, H2-exact: order has N+1
   slots; on entry order[k] = k+1 (k<N) and order[N] = 0; uses the global
   RNG stream from the current seed (Square/bondc.f:166-174). */
void perc_shuffle(int N, int *order);

/* ---- context --------------------------------------------------------- */
int perc_ctx_create(int device, int lattice, int m, int n, int pbc, perc_ctx **out);
int perc_ctx_destroy(perc_ctx *h);
/* last HIP error string for diagnostics (never NULL) */
const char *perc_last_error(void);
/* One HIP runtime per process: the number of distinct libamdhip64 objects
   mapped in the process (dl_iterate_phdr), their paths ';'-separated into
   buf (cap bytes, may be NULL), the copy libperc's own calls bind to
   (dladdr of hipGetDeviceCount) first.  Two copies -- e.g. /opt/rocm's,
   loaded with libperc, and a framework's bundled one loaded later -- share
   one device through two runtimes and corrupt the heap at process exit;
   perc_ctx_create refuses to run then (PERC_ESTATE, the paths in
   perc_last_error). */
int perc_hip_runtimes(char *buf, int cap);

/* ---- occupancy + labeling -------------------------------------------- */
/* Occupy the first `count` entries of `order` (1-based bond ids for
   PERC_BOND, site ids for PERC_SITE; 0 = H2 sentinel, skipped).  For
   PERC_SITEBOND both lists are given.  Host arrays, copied to the device. */
int perc_occupy(perc_ctx *h, int kind, int nsites, const int *site_order,
                int nbonds, const int *bond_order);

/* Same, with the order lists already resident in device memory (device
   pointers on the context's device); used when inputs live in HBM. */
int perc_occupy_device(perc_ctx *h, int kind, int nsites, const int *d_site_order,
                       int nbonds, const int *d_bond_order);

typedef struct {
  int nclusters;      /* connected components with >= 1 occupied element     */
  int nspan;          /* spanning components                                  */
  int span_root;      /* canonical id (min site) of the chosen spanning one, 0 */
  int span_sites;     /* sites in the chosen spanning component               */
  int replayed;       /* 1 if the host label replay decided the lowest label  */
  int perccln;        /* reference label of the chosen component if known     */
} perc_label_info;

/* Occupation drawn on the device, with no order array (the metric
   ensemble's inputs without a host draw or an upload): element id (1-based)
   gets the key (hash32(seed, id) << 32) | id and the nsites / nbonds
   smallest keys are occupied (a radix select, 8 passes of one key byte) --
   the first nsites / nbonds of the permutation "ids in ascending key
   order", a uniform random permutation up to the order of equal 32-bit
   hashes.  Bonds use the key stream of mix64(seed ^ 0x5DEECE66D).  A host
   replay (perc_label_numbers, several spanning clusters) regenerates the
   order on the host; perc_random_order gives it to a caller. */
int perc_occupy_random(perc_ctx *h, int kind, int nsites, int nbonds, unsigned long long seed);
int perc_random_order(long long n, int count, unsigned long long seed, int kind, int *order_out);

/* The occupancy in device memory, copied out (either output may be NULL):
   site_occ[t] (site ids 1..t), bond_occ[nb] (bond ids 1..nb), 0 / 1 each. */
int perc_occupancy(perc_ctx *h, unsigned char *site_occ, unsigned char *bond_occ);

/* GPU connected components of the occupancy + spanning detection.  When
   more than one component spans, the reference's lowest-label rule is
   resolved by the host replay (hazard H4).  canon_out (optional, host,
   t ints) receives the canonical component id (min site id, 0 = empty site)
   per site. */
int perc_label(perc_ctx *h, perc_label_info *info, int *canon_out);

/* Reference label numbers (history-dependent, Square/bondc.f:275-364) by
   O(N alpha) host replay of the last occupancy.  Any output may be NULL.
   bond_label[nb], site_label[t], csize[cap] (cap >= nb+2 bond, t+2 site,
   t+nb+2 mixed), stats[4] = {cln, maxcn, maxcs, perccln}. */
int perc_label_numbers(perc_ctx *h, int *bond_label, int *site_label,
                       int *csize, int cap, int *stats);

/* Cluster sizes of the labeled occupancy on the GPU (bond or site kind):
   *maxcs = the largest cluster's size and *span_size = the size of the
   spanning cluster perc_label chose (0 if none), in bonds for PERC_BOND
   (c(label) of Square/bond_perc.f:296-322) and sites for PERC_SITE
   (site_perc.f).  These are the maxcs / perccls columns of bond_perc.txt /
   site_perc.txt: the same numbers as perc_label_numbers' stats[2] and
   csize[perccln] (clusters only grow, so the running maximum is the final
   largest size), without the host replay. */
int perc_cluster_sizes(perc_ctx *h, int *maxcs, int *span_size);

/* Percolation threshold of one order (Square/bond_perc.f:204-366,
   Square/site_perc.f:150-256, Square/bond_cond.f:381 pc): *first = the
   smallest count c such that occupying order[0..c) (bond ids for PERC_BOND,
   site ids for PERC_SITE) has a spanning cluster, 0 if even all n do not.
   Bisection over c with the GPU labeling (spanning is monotone in c); the
   order is uploaded once (or is a device array when on_device != 0).  The
   context is left occupied at c (or n) and labeled, so perc_label_numbers
   gives the reference's maxcs / spanning-cluster size at that step. */
int perc_first_spanning(perc_ctx *h, int kind, const int *order, int n, int on_device,
                        int *first);

/* Mixed threshold scans (Square/sb_perc.f:104-372, Square/bs_perc.f:104-
   395): one kind fixed, the other scanned.  scan = PERC_BOND: sites
   site_order[0..nsites) occupied, *first = smallest c <= nbonds such that
   bonds bond_order[0..c) make a spanning mixed cluster (bonds connect sites
   whose ends are both occupied; spanning on bottom/top-row sites);
   scan = PERC_SITE: bonds bond_order[0..nbonds) fixed, sites scanned.  0 if
   nothing spans.  GPU labeling in a bisection; the context is left
   unoccupied. */
int perc_first_spanning_mixed(perc_ctx *h, int scan, const int *site_order, int nsites,
                              const int *bond_order, int nbonds, int on_device, int *first);

/* bs_perc's scan (Square/bs_perc.f:236-395) by O(N alpha) host replay:
   bonds bond_order[0..nbond) fixed, sites added in site_order; *first = the
   site count at which a cluster spans (0 if none).  c0_overflow != 0
   reproduces the flang-built reference, whose out-of-bounds read of c(0)
   exceeds every cluster size (hazard H11: a site whose first neighbour
   bond is unoccupied leaves the lattice together with every cluster it
   touches); c0_overflow == 0 is the intended site+bond connectivity. */
int perc_bs_perc_replay(int lattice, int m, int n, int pbc, const int *site_order, int nsites,
                        const int *bond_order, int nbond, int c0_overflow, int *first);

/* Same numbering without a context or device: host-only O(N alpha) replay
   of an explicit occupancy (used by the drivers' text output and tests).
   kind PERC_BONDSITE replays Square/bondsite.f:182-354 (bonds first, each a
   size-1 cluster, then sites merging their neighbour bonds' clusters; sizes
   count bonds and sites; spanning: lowest label of size >= 2n-1 holding a
   bottom- and a top-row site, bondsite.f:364-415).  csize needs
   cap >= t + nb + 2; stats = {cln, maxcn, maxcs, perccln}. */
int perc_replay_labels(int lattice, int m, int n, int pbc, int kind, int nsites,
                       const int *site_order, int nbonds, const int *bond_order,
                       int *bond_label, int *site_label, int *csize, int cap,
                       int *stats);
/* bondc.f's per-bond trace (bondocc.txt, Square/bondc.f:194-376): for the
   first nbond entries of bond_order (1-based ids, 0 = the spill slot),
   trace[3i] = 0 when the bond found no occupied neighbour bond and opened
   cluster trace[3i+1], 1 when it joined the largest neighbouring cluster
   trace[3i+1]; trace[3i+2] = that cluster's size after the step (host
   replay; the Fortran bondc driver writes bondocc.txt from it with
   trace = 1). */
int perc_replay_bond_trace(int lattice, int m, int n, int pbc, int nbond, const int *bond_order,
                           int *trace);
/* site.f's per-site trace (siteocc.txt, Square/site.f:167-272,
   Triangular/site.f): for the first nsite entries of site_order (1-based
   ids), PERC_SITE_TRACE ints each: [0] the site, [1..6] nearestn (scn
   used), [7] the neighbour with the largest cluster, [8] that cluster's
   number, [9] its size, [10] k = clusters absorbed, [11 + 2j] the size
   added and [12 + 2j] the largest cluster's size after (j < k), [21] the
   cluster the site joined, [22] its size after the step (host replay; the
   Fortran site driver writes siteocc.txt from it with trace = 1).
   PERC_EREPLAY for an id outside 1..m*n. */
#define PERC_SITE_TRACE 24
int perc_replay_site_trace(int lattice, int m, int n, int pbc, int nsite, const int *site_order,
                           int *trace);
/* The mixed programs' debug logs (sbdebug.txt, Square/sitebond.f:184-465;
   bsdebug.txt, Square/bondsite.f:178-418): the second phase's steps as an
   int stream, one record per order entry (host replay, kind PERC_SITEBOND
   or PERC_BONDSITE, the other arguments as perc_replay_labels).
   PERC_SITEBOND, per bond of bond_order[0..nbonds):
     {0, cln}                      both end sites empty: a new cluster
     {1, a, lcn, size}             only site a occupied, bond joins its cluster
     {2, b, lcn, size}             only site b occupied
     {3, a, la, ca, b, lb, cb, size}     both in one cluster
     {4|5, a, la, ca, b, lb, cb, ns, ns sites, nk, nk bond ids, lcn, size,
      oldcn}                       different clusters: 4 when a's is larger,
                                   5 otherwise; the sites and bonds (1-based
                                   list ids) relabelled oldcn -> lcn in index
                                   order; cluster oldcn is then empty
     {6}                           the shuffle's spill slot (0, 0)
   PERC_BONDSITE, per site of site_order[0..nsites):
     {0, cln}                      no occupied neighbour bond: a new cluster
     {1, k, k x (size added, largest cluster after), lcn, size}
   *len receives the stream length; trace may be NULL to size it, otherwise
   PERC_EINVAL when cap < *len. */
int perc_replay_mixed_trace(int lattice, int m, int n, int pbc, int kind, int nsites,
                            const int *site_order, int nbonds, const int *bond_order, int *trace,
                            long long cap, long long *len);

/* ---- conductance ----------------------------------------------------- */
typedef struct {
  double gtop, gbot;  /* Itop/Va, |Ibot|/Va                                  */
  double err;         /* final linbcg err                                    */
  int iter;           /* linbcg iterations                                   */
  int status;         /* 0 ok, 1 = no spanning cluster (G = 0)               */
  double t_assemble_ms, t_solve_ms, t_currents_ms;
} perc_cond_result;

/* Assemble the interior Kirchhoff system of the chosen spanning component
   (CSR, diagonal first), solve it with the fused Jacobi-PCG that follows
   linbcg's operation order and stopping rule (itol 1 or 2), and compute
   the terminal currents.  itol 3 / 4 (NR's step-size estimate in the L2 /
   max norm, bondc.f:816-832; the reference calls only itol 2) run a plain
   CSR PCG with per-iteration host folds; PERC_EITOL outside 1..4.
   vint_out (optional, host, t-2m doubles). */
int perc_conductance(perc_ctx *h, int rule, int cur_rule, double Va, double g0,
                     double leak, int itol, double tol, int itmax,
                     perc_cond_result *res, double *vint_out);

/* Matrix access for parity tests / roofline runs: copy the assembled
   interior CSR (0-based: rowptr[N+1], col[nnz], val[nnz], diag[N], rhs[N]).
   Pass NULL to skip an array; *nnz_out receives nnz. */
int perc_get_system(perc_ctx *h, int *rowptr, int *col, double *val,
                    double *diag, double *rhs, int *n_out, int *nnz_out);
/* y = A x on the assembled system (dsprsax order), host in / host out */
int perc_spmv_host(perc_ctx *h, const double *x, double *y);
/* Roofline probe: `reps` back-to-back launches of one solver kernel on the
   assembled system; returns mean kernel ms (HIP events on the context
   stream).  which: 0 = SpMV (dsprsax), 1 = CG SpMV + q.p dot, 2 = CG
   residual update (B), 3 = CG x/p update (P), 4 = STREAM copy 512 MB ->
   512 MB (16-B accesses, past the 256 MB Infinity Cache; the achievable-HBM
   reference), 5 = one whole CG iteration (every kernel of it, in order),
   6 = the resident solve's synchronisation floor: per iteration, the two
   block sums + grid all-gathers of k_cg_res on dummy values, nothing else
   (only on a context whose system takes the resident solver; else
   PERC_EHIP).  (Round 4 dropped the probes that lost their A/Bs: the
   16-B-entry CSR SpMV and the L = 8192 march geometries / load policies,
   profiles/r4_3_*.)  Clobbers solver vectors. */
int perc_bench_kernel(perc_ctx *h, int which, int reps, double *ms);
/* Self-test of the solver's table division (z = r/d from y = RN(1/d) and
   one Markstein correction, bitwise IEEE division when it holds) on the
   default device: n random (a, d) pairs; out3[0] = mismatches against `/`,
   out3[1..2] = bit patterns of the first mismatching a and d. */
int perc_selftest_division(long long n, unsigned long long seed, unsigned long long *out3);

/* Live kernel timing: when enabled, the CG launches of every 64th
   iteration (PERC_TIME_EVERY=n: every n-th) inside perc_conductance are
   bracketed by HIP events on the context stream (a timed launch opens a
   dispatch gap of several us: every 8th cost ~1 % of an L = 4096 solve,
   every launch ~10 %); the accumulated device time of the sampled launches
   that did work is returned (ms) with their count.  stats[0..5] = {spmv_ms, spmv_launches, resid_ms (B),
   resid_launches, xp_ms (P), xp_launches}; reset clears the accumulators. */
int perc_set_kernel_timing(perc_ctx *h, int enable);
int perc_kernel_stats(perc_ctx *h, double *stats, int reset);
/* Sizes of the assembled system: out[0] = N (rows), out[1] = nnz (off-diagonal) */
int perc_system_size(perc_ctx *h, long long *out);

/* Operator format of the solver.  The Kirchhoff matrix of a lattice has two
   distinct off-diagonal values (-g0 inside the spanning component, -leak
   elsewhere, bondc.f:482-538) on a fixed stencil, so besides the CSR copy
   the assembly writes a 16-bit code per row (bit j = "in" for the j-th
   sorted neighbour slot, slot count, row form) and the SpMV/CG kernels
   rebuild each row -- values, diagonal and summation order -- from that
   code: bitwise the same numbers as the CSR path from 2 of its 76 bytes.
   PERC_FMT_AUTO (default) uses the stencil operator whenever every stencil
   bond exists; the NR symbols (sprsin_/linbcg_) always use CSR.
   PERC_FMT_STENCIL fuses the p update into the SpMV: the register-march
   kernel when m is a multiple of 128, else the LDS-tiled one (m even). */
#define PERC_FMT_AUTO 0
#define PERC_FMT_CSR 1
#define PERC_FMT_STENCIL 2        /* stencil, p update fused into the SpMV  */
#define PERC_FMT_STENCIL_SPLIT 3  /* stencil, separate p-update and SpMV kernels */
#define PERC_FMT_STENCIL_TILED 4  /* stencil, fused, always the LDS-tiled kernel */
int perc_set_matrix_format(perc_ctx *h, int fmt);
/* Interior voltages.  linbcg never reads x inside its iteration and the
   terminal currents read it only on the interior rows next to the
   electrodes (Square/bondc.f:554-592), so perc_conductance keeps x on those
   2m rows only (bitwise the same values there) unless vint_out is given or
   this option is on -- then every row is updated every iteration, as
   linbcg does.  Default off. */
int perc_set_full_voltages(perc_ctx *h, int enable);

/* Row-slab decomposition of the CG solve (replaces
   one linbcg loop, Square/bondc.f:780-836): the interior rows split into
   nslab contiguous slabs with private r, p, q, x and one ghost row of r and
   p towards each neighbour; per iteration each slab runs the march P+S and
   the streaming B kernels on its rows, the q.p and z.r / r.r partials are
   combined in slab order, and the slabs' edge rows of r are copied into
   the neighbours' ghost rows.  Per-row arithmetic is the single-slab
   solve's; only the dot-product association differs.  Needs the register-
   march format (m a multiple of 128, PERC_FMT_STENCIL); a solve with
   nslab > 1 in another format fails with PERC_EHIP.  Default 1. */
int perc_set_slabs(perc_ctx *h, int nslab);

/* Distributed row slabs: one process per GPU solves slab s of K of the
   system assembled by perc_assemble (every process labels and assembles
   the whole lattice; the solve is split).  The per-slab kernels and the
   slab-order combine are perc_set_slabs's, so K processes reproduce its
   K-slab numbers bitwise.  The caller moves data between processes
   (percolation_amd/dslab.py: torch.distributed, RCCL on the context's
   stream or gloo through the host), through device buffers it owns:
     part_out  4 doubles   this slab's partials after a step (send);
     part_all  4K doubles  every slab's part_out in slab order (receive);
     edge_lo / edge_hi     m doubles: r of the slab's first / last row
                           (send to slab s-1 / s+1; NULL at s = 0 / K-1);
     ghost_lo / ghost_hi   m doubles: slab s-1's last / s+1's first row
                           (receive).
   Protocol: perc_dslab_begin (prologue; publishes part_out and the edges;
   the PS / B steps' kernels write their partials into part_out themselves)
   -> all-gather part_out into part_all, exchange edges into ghosts ->
   step COMBINE_INIT, GHOSTS; then per iteration: PS, all-gather,
   COMBINE_PS, B, all-gather, COMBINE_B, exchange edges, GHOSTS; poll
   perc_dslab_status every few iterations (the steps are no-ops once the
   stop test fired: every process takes the same decision).  perc_dslab_end
   puts this slab's x rows (the electrode rows unless full_x) into the
   context's x; perc_x_row / perc_currents then give Gtop / Gbot on the
   process that holds both electrode rows. */
typedef struct perc_dslab_bufs {
  double *part_out, *part_all, *edge_lo, *edge_hi, *ghost_lo, *ghost_hi;
} perc_dslab_bufs;
#define PERC_DSLAB_COMBINE_INIT 0
#define PERC_DSLAB_PS 1
#define PERC_DSLAB_COMBINE_PS 2
#define PERC_DSLAB_B 3
#define PERC_DSLAB_COMBINE_B 4
#define PERC_DSLAB_GHOSTS 5
int perc_dslab_begin(perc_ctx *h, int K, int s, int itol, double tol, int itmax, int full_x,
                     const perc_dslab_bufs *bufs);
int perc_dslab_step(perc_ctx *h, int op);
int perc_dslab_status(perc_ctx *h, int *iter, double *err, int *done);
int perc_dslab_end(perc_ctx *h);
/* The whole split solve from one host process, no caller code inside the
   loop: K labeled contexts (the same lattice and occupancy, context s on
   its own device for RCCL) solve row slab s each, one host thread per
   context issuing its slab's loop onto the context's stream.  xport
   PERC_XPORT_RCCL: ncclCommInitAll over the contexts' devices, the
   partials all-gathered and the r halo swapped by ncclAllGather /
   ncclSend / ncclRecv on the streams (no host round trip inside the loop);
   PERC_XPORT_HOST: the same exchanges staged through host memory (any
   devices, several contexts on one GPU included).  The numbers are
   perc_set_slabs(K)'s in one context bitwise.  Assembles every context
   (perc_assemble), solves, and returns Gtop / Gbot from slab 0 in *res
   (status 1: nothing spans).  Replaces the linbcg call of
   Fortran/Square/bondc.f:545 for a lattice split over GPUs.
   K = 1 runs the one-slab kernel epilogues (no combine, no collective: the
   same arithmetic) unless xport has PERC_XPORT_EXCHANGE set, which keeps
   the combines and the (one-rank) collectives -- the exchange machinery's
   own cost, measured by tools/dslab_bench.py.  RCCL communicators are made
   once per device list and kept for the process (one group call at a time
   per device list). */
#define PERC_XPORT_RCCL 0
#define PERC_XPORT_HOST 1
#define PERC_XPORT_EXCHANGE 4
int perc_dslab_solve_group(int K, perc_ctx **ctxs, int xport, int rule, int cur_rule, double Va,
                           double g0, double leak, int itol, double tol, int itmax, int full_x,
                           perc_cond_result *res);
/* One process per GPU (torchrun / MPI): rank 0 makes an RCCL unique id
   (PERC_DSLAB_ID_BYTES bytes), the launcher ships it to every rank, each
   rank binds its labeled context to slab s of K with perc_dslab_comm_init,
   then perc_dslab_solve runs the whole loop of perc_dslab_solve_group for
   its slab (assembly, all-gathers and halos over RCCL on the context's
   stream, the top electrode row to rank 0, rank 0's Gtop / Gbot broadcast
   to every rank).  The ranks check that they all found the same spanning
   state before the loop.  The communicator lives until perc_dslab_comm_free
   or perc_ctx_destroy.  Same numbers as perc_dslab_solve_group over K
   contexts. */
#define PERC_DSLAB_ID_BYTES 128
int perc_dslab_unique_id(void *id, int nbytes);
int perc_dslab_comm_init(perc_ctx *h, int K, int s, const void *id, int nbytes);
int perc_dslab_comm_free(perc_ctx *h);
int perc_dslab_solve(perc_ctx *h, int rule, int cur_rule, double Va, double g0, double leak,
                     int itol, double tol, int itmax, int full_x, perc_cond_result *res);
/* assembly only (perc_conductance's first half): the Kirchhoff system of
   the lowest spanning cluster; PERC_ESTATE before perc_label, status 1 in
   *spanning = 0 when nothing spans */
int perc_assemble(perc_ctx *h, int rule, double g0, double leak, double Va, int *spanning);
/* copy row `row` of the interior voltages between the context and a device
   buffer of m doubles (to_ctx = 1: into the context) */
int perc_x_row(perc_ctx *h, int row, double *dev_buf, int to_ctx);
/* terminal currents of the context's x (perc_conductance's last step) */
int perc_currents(perc_ctx *h, int rule, int cur_rule, double Va, double g0, double leak,
                  perc_cond_result *res);
/* the HIP stream the context enqueues on (hipStream_t), e.g. for a caller's
   collectives on the same stream */
void *perc_stream(perc_ctx *h);

/* Band height (lattice rows per wave) of the register-march kernel; 0 (default)
   picks the tallest of 32, 16, .. 2 rows that still gives >= 4096 waves.
   A tuning / test knob: results are the same up to the association of the
   q.p dot. */
int perc_set_march_rows(perc_ctx *h, int rows);

/* Register-march loop structure (PERC_FMT_STENCIL with m a multiple of
   128).  Per-row arithmetic is the same in every mode (bitwise the same
   values); only the association of the dot products differs.  The mode is
   read when the system is assembled; default PERC_MARCH_DEFAULT.
   PERC_MARCH_QFREE: the P+S kernel does not store q; the B kernel (r -= ak
   q, z.r, r.r) marches too and rebuilds q = A p(k) from p(k), so an
   iteration moves 52 instead of 60 bytes per row (strip-major at L = 4096:
   0.164 vs 0.178 ms per iteration; row-major at L = 8192: 0.721 vs 0.737).
   PERC_MARCH_ALT: neighbouring bands walk in opposite directions, so the
   halo rows they share are read at the same moment (cache hits).
   PERC_SOLVE_RESIDENT: the one-workgroup solve of small systems and the
   resident cooperative solve where they apply.
   PERC_MARCH_STRIPS (with QFREE): r, p and the row codes strip-major for the
   solve (each 128-column strip contiguous), so every wave walks one
   contiguous stream; x stays row-major.  Used while one vector fits the
   256 MB Infinity Cache (L <= 4096).
   PERC_MARCH_SLOTS: one workgroup per CU and round, the bands sized by the
   round a wave runs in (the first round on a CU streams fastest), so every
   wave finishes at about the same time (past the Infinity Cache: the
   row-major P kernel's one round of bands).
   PERC_MARCH_TAG (strip-major march): the end-of-kernel reductions publish
   tagged {value, tag} granules the readers poll for, instead of draining
   stores before each ticket; bitwise the same totals.
   PERC_MARCH_NIBBLE (strip-major march, square lattice): the row codes as
   one 4-bit slot mask per site (two sites per byte), count and form from
   the column -- 0.5 instead of 2 bytes of code per element in each kernel
   (52N -> 49N bytes per iteration); bitwise the same codes (checked per
   row when packed).
   Row slabs (perc_set_slabs) and the literal dot order always run the
   row-major q-storing march.  (Round 4 removed the variants that lost their
   A/Bs: workgroup row-march 4, deferred reductions 32, persistent march
   256, the strip-major march past the Infinity Cache 1024; those bits are
   rejected.  Round 6 re-measured the deferred reductions as an opt-in
   variant, 0.1515-0.1527 against 0.1511 ms per iteration with the
   collectors, and they were removed again.) */
#define PERC_MARCH_QFREE 1
#define PERC_MARCH_ALT 2
#define PERC_SOLVE_RESIDENT 8
#define PERC_MARCH_STRIPS 16
#define PERC_MARCH_SLOTS 64
#define PERC_MARCH_TAG 128
#define PERC_MARCH_NIBBLE 512
#define PERC_MARCH_DEFAULT                                                                      \
  (PERC_MARCH_QFREE | PERC_MARCH_ALT | PERC_SOLVE_RESIDENT | PERC_MARCH_STRIPS | PERC_MARCH_SLOTS | \
   PERC_MARCH_TAG | PERC_MARCH_NIBBLE)
int perc_set_march_mode(perc_ctx *h, int mode);
/* Per-round band weights of the slot-weighted bands (PERC_MARCH_SLOTS):
   which = 0 the strip-major P kernel, 1 its B kernel; n = 0 restores both
   defaults (100:76:48:40, 100:78:55:50).  which = 2 was the row-major P past
   the Infinity Cache, which runs on B's 8-row bands since round 4: it is
   still accepted (valid weights return PERC_OK) and changes nothing.  A
   tuning / test knob: the rows stay a partition of the lattice whatever the
   weights. */
int perc_set_band_weights(perc_ctx *h, int which, int n, const int *w);

/* Association of linbcg's three dot products (Square/bondc.f:785-787 bknum,
   :803-805 akden, :872-875 snrm).  PERC_DOT_FAST (default): deterministic
   wave / workgroup trees inside the fused kernels.  PERC_DOT_LITERAL: each
   sum folded term after term in ascending j on one wave of the GPU, exactly
   as the reference loops do -- with every other operation already the
   reference's, the iterates, iter, err history and voltages are then
   bitwise the reference solver's.  One dependent fp64 add per term: a
   verification mode (single slab).  It runs the production kernels of the
   fast order -- the q-free strip-major / row-major march (k_cg_march P, B)
   and the resident solve (k_cg_res), the same code objects -- which store
   each row's dot terms (the reference's IEEE products) for the folds; other
   formats fold from their stored q, p, r.  perc_last_solve says what ran.
   The NR drop-in linbcg_ uses PERC_DOT_LITERAL by default
   (perc_nr_set_dot_order). */
#define PERC_DOT_FAST 0
#define PERC_DOT_LITERAL 1
/* PERC_DOT_LITERAL_HOST: the literal order with the three serial sums formed
   by the host CPU from the terms the q-free march kernels stored (the same
   IEEE adds in the same ascending-j order, so bitwise PERC_DOT_LITERAL; the
   CPU's dependent fp64 add is ~4x shorter than a GPU wave's, which makes the
   config-size verification runs fit one GPU session).  Runs the launched
   march (not the resident solve); formats without it fold on the GPU. */
#define PERC_DOT_LITERAL_HOST 2
int perc_set_dot_order(perc_ctx *h, int order);
/* What the last solve of the context actually ran: out4[0] = kernel family
   (0 other launched kernels: LDS tiles, split stencil, CSR; PERC_RAN_MARCH,
   PERC_RAN_RESIDENT, PERC_RAN_SMALL), out4[1] = PERC_RAN_* flag bits,
   out4[2] = iterations, out4[3] = iterations in which the march skipped dead
   bands (PERC_RAN_FRONT).  PERC_ESTATE before any solve. */
#define PERC_RAN_MARCH 1
#define PERC_RAN_SLABS 2      /* row slabs (perc_set_slabs) */
#define PERC_RAN_RESIDENT 3
#define PERC_RAN_SMALL 4
#define PERC_RAN_LITERAL 1    /* literal dot order */
#define PERC_RAN_LIT_TERMS 2  /* ... folding the terms the solve kernels stored */
#define PERC_RAN_QFREE 4      /* q-free march (P + B rebuild q) */
#define PERC_RAN_STRIPS 8     /* strip-major layout */
#define PERC_RAN_NIBBLE 16    /* 4-bit row codes */
#define PERC_RAN_TAG 32       /* tagged-granule reductions */
#define PERC_RAN_HOST_FOLD 64 /* PERC_DOT_LITERAL_HOST: the sums folded by the host */
#define PERC_RAN_XCD_GROUPED 128 /* resident solve: XCD-grouped reductions (else the flat all-gather) */
/* (bit 256 of out4[1] is retired -- it marked the deferred reductions -- and is not to be reused) */
#define PERC_RAN_OPEN 512     /* strip-major nibble march: the open-lattice kernels (open-square path alone) */
/* the march skipped the bands the Krylov front had not reached (x0 = 0, one
   slab, the launched q-free march; PERC_MARCH_FRONT=0 in the environment
   turns it off); out4[3] counts the iterations that ran with such a band */
#define PERC_RAN_FRONT 1024
int perc_last_solve(perc_ctx *h, int *out4);
/* err of every iteration of the last solve (linbcg's per-iteration
   `write (*,*) iter, err`, bondc.f:834): min(cap, iterations) values into
   out, entry k - 1 = err of iteration k; returns the iteration count (>= 0)
   or a negative status.  itol 3 / 4: EVERY iteration has its entry, also
   those where linbcg takes `goto 100` (bondc.f:822-831) and prints nothing;
   there the entry is the err linbcg set before the jump, znrm / bnrm -- so
   the history has more entries than the reference's log, which holds only
   the tested iterations.  itol 1 / 2: entry for entry the reference's log. */
int perc_err_history(perc_ctx *h, double *out, int cap);
/* Random bond conductances (MATLAB/ConductCalc.m condtype 2, :38-47 and
   :94-97): the bonds of the spanning cluster get G = -g0 * w[id] instead of
   -g0 (w[id] = the MATLAB rand drawn for that bond; the draw order is the
   caller's, see api.conductcalc_weights).  w = NULL restores fixed
   conductances.  n = the lattice's bond count.  With weights the solver
   runs the CSR operator (the stencil code encodes two values only). */
int perc_set_bond_weights(perc_ctx *h, const double *w, long long n);
/* ConductCalc.m condtype 2 from C / Fortran (MATLAB/ConductCalc.m:38-47,
   94-97, 114-118, 136-146): after perc_label, every bond the assembly gives
   -g0 under `rule` (the spanning cluster's) gets -g0*rand, one
   rand('twister', seed) draw per such bond in bond-list order; the others
   keep their value (perc_set_bond_weights with those multipliers; no
   spanning cluster: fixed conductances).  perc_twister_uniform: n draws of
   that generator (MT19937 init_genrand(seed), 53-bit genrand_res53
   doubles).  MATLAB parity itself is unpinned (no MATLAB here). */
int perc_set_conductcalc_weights(perc_ctx *h, int rule, unsigned int seed);
int perc_twister_uniform(unsigned int seed, long long n, double *out);
/* Solver loop of the assembled system: out5[0] = 0 (no march kernel: LDS
   tiles, split or CSR), 1 (per-wave march k_cg_march), 3 (resident
   persistent solve k_cg_res), 4 (one-workgroup solve of a small system,
   k_cg_small: N <= 8192 under PERC_FMT_AUTO with PERC_SOLVE_RESIDENT set);
   out5[1] = bit 0: q-free B, bit 1: strip-major solve layout, bit 3:
   slot-weighted bands (PERC_MARCH_SLOTS; past the Infinity Cache the
   row-major P kernel's one round of bands), bit 4: tagged-granule
   reductions, bit 5: nibble row codes (the last solve); out5[2] = alternating directions, out5[3] = band height,
   out5[4] = strip width (columns). */
int perc_march_info(perc_ctx *h, int *out5);

/* format the solver kernels use on the assembled system: PERC_FMT_CSR,
   PERC_FMT_STENCIL (register-march fused kernel), PERC_FMT_STENCIL_TILED
   (LDS-tiled fused kernel) or PERC_FMT_STENCIL_SPLIT */
int perc_matrix_format(perc_ctx *h);

/* ---- one hot-path realisation (bench / ensemble) ---------------------- */
typedef struct {
  perc_label_info label;
  perc_cond_result cond;
  double t_upload_ms, t_label_ms, t_total_ms;
} perc_realisation;
/* occupy + label + conductance for PERC_BOND with the bondc rules;
   bond_order is a host array, or a device array when on_device != 0 */
int perc_bondc_realisation(perc_ctx *h, int tbonds, const int *bond_order,
                           int on_device, double Va, double g0, double tol,
                           int itmax, perc_realisation *out);

/* ---- batch of small bond realisations (one workgroup each) ------------ *
 * The reference's bond_cond ensemble (Fortran/Square/bond_cond.f:123-498)
 * is ~10^5 independent Kirchhoff solves on lattices of 10 x 10 .. 50 x 50.
 * perc_batch_bondc runs many of them in one launch: item i is the bond
 * realisation "the first item_count[i] entries of trial item_trial[i]'s
 * order" (orders: ntrials rows of nb + 1 entries as perc_shuffle leaves
 * them; the spill slot 0 takes a position and is no bond), and one
 * workgroup takes it from occupancy through labeling, the spanning test,
 * assembly and the linbcg loop to the terminal currents in LDS
 * (PERC_BOND, PERC_RULE_BOND, PERC_CUR_FORTRAN; itol 1 or 2).  solve = 0
 * stops after the spanning test (labels only).  The dot order is the
 * context's (perc_set_dot_order; PERC_DOT_LITERAL_HOST runs as
 * PERC_DOT_LITERAL): literal results are bitwise perc_conductance's under
 * PERC_DOT_LITERAL, fast ones use the workgroup's own fixed tree (the same
 * for an item wherever it stands in the batch).  When several clusters span
 * (nspan > 1) the reference's lowest-label rule needs the host replay:
 * the item comes back with fallback = 1, filled by perc_occupy /
 * perc_label / perc_conductance on the context.  The context's single-
 * realisation state (occupancy, labeling, assembled system) is therefore
 * what the last fallback item left; without one it is unchanged.
 * PERC_EINVAL: itol 3 / 4, a lattice perc_batch_supported refuses (text in
 * perc_last_error), item_trial outside 0..ntrials-1, item_count outside
 * 0..nb+1. */
typedef struct {
  double gtop, gbot, err;
  int iter, status;                         /* as perc_cond_result */
  int nclusters, nspan, span_root, span_sites;
  int fallback;                             /* 1: several clusters span; run through the single path */
} perc_batch_item;
/* host-only: 1 when the batch kernel can run this lattice: n >= 3, the
   interior system has (n-2)*m <= 8192 rows and the stencil operator exists
   (every interior row one of the stencil forms, every stencil bond present) */
int perc_batch_supported(int lattice, int m, int n, int pbc);
int perc_batch_bondc(perc_ctx *h, int ntrials, const int *orders /* ntrials x (nb+1) */,
                     int nitems, const int *item_trial, const int *item_count, int solve,
                     double Va, double g0, double leak, int itol, double tol, int itmax,
                     perc_batch_item *out);

/* ---- the same for site and mixed conductance --------------------------- *
 * site.f / sitebond.f with ConductCalc.m's site rule (:88-109) and mixed
 * rule (:134-160) on the reference's 10 x 10 .. 50 x 50 lattices: the other
 * two (kind, rule) pairs through the same one-workgroup kernel.
 *   kind PERC_BOND,     rule PERC_RULE_BOND   bond id occupied iff its position
 *                       in the trial's bond order < item_nbonds[i]; a bond
 *                       connects iff it is occupied (perc_batch_bondc's items)
 *   kind PERC_SITE,     rule PERC_RULE_SITE   site occupied iff its position in
 *                       the trial's site order < item_nsites[i]; a bond
 *                       connects iff both end sites are occupied
 *   kind PERC_SITEBOND, rule PERC_RULE_MIXED  both lists; a bond connects iff it
 *                       and both end sites are occupied
 * Item i is the first item_nsites[i] sites and item_nbonds[i] bonds of trial
 * item_trial[i]'s orders (site_orders: ntrials rows of t + 1 entries,
 * bond_orders: ntrials rows of nb + 1, as perc_shuffle leaves them; the spill
 * slot 0 takes a position and is no element; a count of t + 1 / nb + 1 is
 * the whole order).  The list the kind does not read may be NULL.  Labels
 * are perc_label's: an isolated occupied site of the site and mixed kinds is
 * a cluster of its own in nclusters.  cur_rule PERC_CUR_FORTRAN or
 * PERC_CUR_MATLAB, as perc_conductance.  solve, the dot order (literal
 * results are bitwise perc_conductance's under PERC_DOT_LITERAL), itol 1 or
 * 2 and the out record are perc_batch_bondc's; with kind PERC_BOND and
 * PERC_CUR_FORTRAN the results are perc_batch_bondc's own.  When several
 * clusters span (nspan > 1) the item comes back with fallback = 1, filled by
 * perc_occupy(kind, ..) / perc_label / perc_conductance(rule, cur_rule, ..)
 * on the context, the spill slot dropped where a count covers a whole order.
 * The context's single-realisation state (occupancy, labeling, assembled
 * system) is therefore what the last fallback item left; without one it is
 * unchanged.  nitems == 0 is PERC_OK.  PERC_EINVAL (text in
 * perc_last_error): a (kind, rule) pair outside the table, a cur_rule other
 * than the two, itol 3 / 4, a lattice perc_batch_cond_supported refuses for
 * the kind, a missing order list or count list the kind reads, item_trial
 * outside 0..ntrials-1, item_nsites outside 0..t+1, item_nbonds outside
 * 0..nb+1, ntrials or nitems below 0. */
/* host-only: 1 when the batch kernel can run this kind on this lattice:
   perc_batch_supported for PERC_BOND; for PERC_SITE / PERC_SITEBOND the same
   checks with the kind's own LDS layout (one more byte per site) */
int perc_batch_cond_supported(int kind, int lattice, int m, int n, int pbc);
int perc_batch_cond(perc_ctx *h, int kind, int rule, int cur_rule, int ntrials,
                    const int *site_orders /* ntrials x (t+1), NULL for PERC_BOND */,
                    const int *bond_orders /* ntrials x (nb+1), NULL for PERC_SITE */,
                    int nitems, const int *item_trial,
                    const int *item_nsites /* NULL for PERC_BOND */,
                    const int *item_nbonds /* NULL for PERC_SITE */,
                    int solve, double Va, double g0, double leak, int itol,
                    double tol, int itmax, perc_batch_item *out);

/* ---- batch conductance up to 128 x 128 (opt-in) ----------------------- *
 * perc_batch_bondc / perc_batch_cond stop at 8192 interior rows (about
 * 90 x 90): their kernel keeps p, q and the row codes of the one-workgroup
 * solve in LDS.  A second kernel, k_batch_cond_large, keeps p alone there --
 * 1024 threads, at most 16 rows each, a thread's row codes and r in its
 * registers, q never in LDS (held in registers between the two passes in
 * the fast order, rebuilt from p, bitwise the q of q.p, in the literal one),
 * x on the 2m rows the currents read -- and so takes every lattice of at most
 * 16384 sites (128 x 128, 64 x 256), the same stages and the same results:
 * under PERC_DOT_LITERAL bitwise perc_conductance's, under PERC_DOT_FAST
 * k_batch_cond's tree over 16 rows per thread.  While the flag of
 * perc_set_batch_large is set on a context, perc_batch_bondc,
 * perc_batch_cond and perc_batch_cond_seeded run that kernel on every
 * lattice perc_batch_large_supported accepts for the kind and answer
 * PERC_EINVAL (the text names perc_batch_large_supported) on any other;
 * argument rules, chunking, the fallback replay and the item records are
 * unchanged.  While it is clear (the default) nothing changes.  On a lattice
 * both kernels take, the default one is the faster. */
/* host-only: 1 when the large batch kernel can run this kind on this
   lattice: m, n >= 3, even m on the triangular lattice, m*n <= 16384, every
   interior row a stencil form with every stencil bond present, and the
   kind's LDS arena within a workgroup's 160 KB.  Accepts every lattice
   perc_batch_cond_supported accepts. */
int perc_batch_large_supported(int kind, int lattice, int m, int n, int pbc);
/* enable != 0: the context's batch calls run the large kernel; 0: the
   default kernel again */
int perc_set_batch_large(perc_ctx *h, int enable);
/* the flag: 1 or 0 (PERC_EINVAL for a NULL context) */
int perc_batch_large(perc_ctx *h);

/* ---- batch conductance with per-bond weights (ConductCalc condtype 2) -- *
 * The reference's second way to the conductance gives every bond of the
 * spanning cluster G = -g0 * rand (MATLAB/ConductCalc.m:33-47, 94-97,
 * 114-118, 136-146).  A disorder average over such conductances is an
 * ensemble of small lattices, and perc_batch_cond's two kernels cannot run
 * it: they rebuild every row from a two-value code.  A third one-workgroup
 * kernel, k_batch_cond_w, keeps the rows' slot values themselves in LDS (one
 * array of N doubles per slot, beside p; r, q, the diagonal and the form of
 * a thread's at most 4 rows in its registers; 256 / 512 / 1024 threads) and
 * multiplies by them in dsprsax's order -- the diagonal, then the used slots
 * in slot order -- with z = r / d a plain division by the stored diagonal:
 * the CSR operator perc_conductance runs under perc_set_bond_weights.  Under
 * PERC_DOT_LITERAL the results are bitwise that single path's, under
 * PERC_DOT_FAST the workgroup's own fixed tree (the same for an item
 * wherever it stands in the call).  perc_batch_cond_weighted is
 * perc_batch_cond with the weights; exactly one of the two inputs is given:
 *   explicit     weights = nwsets rows of nb doubles, w[id-1] for bond id of
 *                the bond list; item i uses row item_wset[i].  As
 *                perc_set_bond_weights(row) before perc_conductance.
 *   ConductCalc  item i draws rand('twister', item_wseed[i]), one draw per
 *                bond the rule gives -g0, in bond-list order, 1.0 for the
 *                others (k_twister_stream generates the draws on the device,
 *                the kernel places them by an exclusive count over the
 *                sites).  As perc_set_conductcalc_weights(h, rule,
 *                item_wseed[i]) after perc_label.
 * The argument rules, chunking (the weight rows add 8 nb bytes per item to
 * the 64 MB bound), item records, dot-order handling (PERC_DOT_LITERAL_HOST
 * runs as literal), solve = 0 and "nitems == 0 is PERC_OK" are
 * perc_batch_cond's.  The call does not read the perc_set_batch_large flag:
 * it has its own kernel.  An item several clusters span (fallback = 1) goes
 * through the single path with its weights set on the context after
 * perc_label -- perc_set_bond_weights(row) or
 * perc_set_conductcalc_weights(rule, seed) -- and cleared with
 * perc_set_bond_weights(h, NULL, 0) after it: a fallback item clears any
 * weights the caller had set on the context, and leaves the context
 * unweighted.  PERC_EINVAL (text in perc_last_error), before any device
 * call: perc_batch_cond's cases; both weight inputs or neither; weights
 * without item_wset or the reverse; nwsets < 1 in explicit mode; item_wset[i]
 * outside 0..nwsets-1; a lattice perc_batch_weighted_supported refuses (the
 * text names it). */
/* host-only: 1 when the weighted batch kernel can run this kind on this
   lattice: m, n >= 3, even m on the triangular lattice, at most 4096 interior
   rows (4 per thread), every interior row a stencil form with every stencil
   bond present, and the kernel's LDS arena (p, the slot values, the electrode
   rows' values) within a workgroup's 160 KB: every square and triangular
   lattice of 10 x 10 .. 50 x 50, open or periodic.  Accepts no lattice
   perc_batch_large_supported refuses. */
int perc_batch_weighted_supported(int kind, int lattice, int m, int n, int pbc);
int perc_batch_cond_weighted(perc_ctx *h, int kind, int rule, int cur_rule, int ntrials,
                             const int *site_orders /* ntrials x (t+1), NULL for PERC_BOND */,
                             const int *bond_orders /* ntrials x (nb+1), NULL for PERC_SITE */,
                             int nitems, const int *item_trial,
                             const int *item_nsites /* NULL for PERC_BOND */,
                             const int *item_nbonds /* NULL for PERC_SITE */,
                             int nwsets, const double *weights /* nwsets x nb, or NULL */,
                             const int *item_wset /* nitems, with weights */,
                             const unsigned int *item_wseed /* nitems, or NULL */,
                             int solve, double Va, double g0, double leak, int itol,
                             double tol, int itmax, perc_batch_item *out);
/* the device generator on its own: n genrand_res53 doubles per seed, bit for
   bit perc_twister_uniform(seed, n); out = nseeds rows of n (host).
   PERC_EINVAL: n < 0 or nseeds < 0. */
int perc_batch_twister(perc_ctx *h, int nseeds, const unsigned int *seeds, long long n,
                       double *out);

/* ---- batch of small threshold scans (one workgroup each) -------------- *
 * The reference's threshold programs (Fortran/Square/bond_perc.f:204-366,
 * site_perc.f:150-256, sb_perc.f:104-372, bs_perc.f:104-395) are ensembles
 * of 10 .. 10^5 trials on lattices of 10 x 10 .. 50 x 50, each "fill one
 * order until a cluster spans".  perc_batch_scan runs many trials in one
 * launch: one workgroup takes trial i from its rank arrays (an element is
 * occupied at count c iff its position in the order < c; the spill slot 0
 * takes a position and is no element) through the whole bisection of
 * perc_first_spanning / perc_first_spanning_mixed -- label at N, then
 * lo = 0, hi = N, mid = lo + (hi - lo) / 2 until hi - lo == 1 -- with the
 * union-find labeling and the spanning rule of perc_batch_bondc in LDS, no
 * host round trip and no second launch, then labels once more at the first
 * spanning count (at N when nothing spans) for the cluster sizes of
 * perc_cluster_sizes.
 *   kind PERC_BOND   bonds scanned; sizes in bonds (bond_perc.txt's columns)
 *   kind PERC_SITE   sites scanned; a bond connects two occupied sites;
 *                    sizes in sites (site_perc.txt's columns)
 *   kind PERC_SITEBOND, scan PERC_BOND (sb_perc): the first fixed[i] entries
 *                    of trial i's site order occupied, bonds scanned; a bond
 *                    connects when it and both end sites are occupied
 *   kind PERC_SITEBOND, scan PERC_SITE (bs_perc's intended rule, hazard H11):
 *                    the first fixed[i] bonds occupied, sites scanned
 * out[i].first = the first spanning count (0: nothing spans, as
 * perc_first_spanning), maxcs / span_size = perc_cluster_sizes' numbers at
 * that count (at N when nothing spans, span_size 0 then; both 0 for
 * PERC_SITEBOND), nspan = the number of spanning clusters there (1 at a
 * first spanning count: the element just added lies in one cluster).
 * kind PERC_BOND / PERC_SITE: scan is ignored, fixed and the other kind's
 * orders may be NULL.  site_orders: ntrials rows of t + 1 entries,
 * bond_orders: ntrials rows of nb + 1, as perc_shuffle leaves them; the
 * scanned prefix ranges over the first N entries (N = nb or t), as
 * perc_first_spanning(order, N).  The call chunks itself so that one
 * launch's rank arrays stay under 64 MB of device memory, and leaves the
 * context's single-realisation state (occupancy, labeling, assembled system)
 * untouched.  ntrials == 0 is PERC_OK.  PERC_EINVAL (text in
 * perc_last_error): a lattice perc_scan_supported refuses, a bad kind or
 * scan, a missing order list, fixed[i] outside 0..t (scan PERC_BOND) /
 * 0..nb (scan PERC_SITE), ntrials < 0. */
typedef struct { int first, maxcs, span_size, nspan; } perc_scan_item;
/* host-only: 1 when the scan kernel can run this lattice: m, n >= 3 and
   m*n <= 16384 sites (128 x 128; the workgroup's LDS arena).  The kernel's
   own limits only: perc_ctx_create's rules (even m on the triangular
   lattice, H7) stand beside it. */
int perc_scan_supported(int lattice, int m, int n, int pbc);
int perc_batch_scan(perc_ctx *h, int kind, int scan, int ntrials,
                    const int *site_orders /* ntrials x (t+1) */,
                    const int *bond_orders /* ntrials x (nb+1) */,
                    const int *fixed, perc_scan_item *out);

/* ---- occupation orders shuffled on the device (one wave per trial) ---- *
 * The batch entry points above take whole orders from the host: one serial
 * perc_shuffle_seeded per trial, the orders' inverse permutations, 4 bytes
 * per element per trial uploaded.  perc_batch_shuffle runs the same shuffle
 * -- srand(seed) on a stream local to the trial, then the REAL*4
 * Fisher-Yates of bondc.f:162-174 with the spill slot (hazard H2), the
 * generator's recurrence and the REAL*4 mapping operation for operation --
 * for ntrials trials at once, one wave each, the order in LDS as N + 1
 * entries of 16 bits, and leaves the inverse permutations in the context's
 * batch rank buffers, where perc_batch_cond's and perc_batch_scan's kernels
 * read them: rank[trial * N + id - 1] = position of id.  The orders are the
 * host's bit for bit (seed 0 is 123459876; a negative seed wraps as unsigned
 * 64 bit in the first update, as in perc_shuffle_seeded).
 *   list PERC_BOND: N = nb, the bond ranks; PERC_SITE: N = t, the site ranks.
 * orders_out (ntrials rows of N + 1, as perc_shuffle_seeded leaves them) and
 * ranks_out (ntrials rows of N) may each be NULL.  perc_batch_scan_seeded
 * and perc_batch_cond_seeded are perc_batch_scan and perc_batch_cond with
 * seed lists (one seed per trial) in place of the order lists: the same
 * argument rules, the same chunking, the same results item for item; an item
 * of perc_batch_cond_seeded that falls back to the single path (fallback =
 * 1) gets its trial's order(s) from perc_shuffle_seeded on the host.
 * ntrials == 0 is PERC_OK.  PERC_EINVAL (text in perc_last_error), before
 * any device call: a list perc_shuffle_device_supported refuses, a missing
 * seed list that the kind reads, ntrials < 0, a bad list, kind or scan.
 * One serial wave per trial loses to the host while few trials share a
 * call: measured at 50 x 50, the seeded scan runs at 0.8-0.9
 * of the order-taking one's rate at 1..8 trials per call, draws level at 16
 * and wins from there (1.2 x at 32, 3-4 x at 256, 7-13 x at 1000).  Nothing
 * takes this path unless asked. */
/* host-only: 1 when the shuffle kernel can take a list of N ids: N >= 1,
   N + 1 <= 65535 (ids and the target N + 1 in 16 bits) and the LDS arena --
   2 (N + 1) bytes for the order, 256 for the swap targets of 64 steps --
   within a workgroup's 160 KB.  Every list of a lattice perc_scan_supported
   or perc_batch_cond_supported accepts passes (the longest: the 48896 bonds
   of the triangular 128 x 128 pbc lattice). */
int perc_shuffle_device_supported(int N);
int perc_batch_shuffle(perc_ctx *h, int list, int ntrials, const int *seeds,
                       int *orders_out /* ntrials x (N+1), or NULL */,
                       int *ranks_out /* ntrials x N, or NULL */);
/* the same kernel on a list of N ids that is no list of the context's
   lattice (any N perc_shuffle_device_supported accepts): the outputs only,
   the context's batch rank buffers stay as they are */
int perc_batch_shuffle_n(perc_ctx *h, int N, int ntrials, const int *seeds,
                         int *orders_out, int *ranks_out);
int perc_batch_scan_seeded(perc_ctx *h, int kind, int scan, int ntrials,
                           const int *site_seeds /* ntrials */,
                           const int *bond_seeds /* ntrials */,
                           const int *fixed, perc_scan_item *out);
int perc_batch_cond_seeded(perc_ctx *h, int kind, int rule, int cur_rule, int ntrials,
                           const int *site_seeds /* ntrials, NULL for PERC_BOND */,
                           const int *bond_seeds /* ntrials, NULL for PERC_SITE */,
                           int nitems, const int *item_trial,
                           const int *item_nsites /* NULL for PERC_BOND */,
                           const int *item_nbonds /* NULL for PERC_SITE */,
                           int solve, double Va, double g0, double leak, int itol,
                           double tol, int itmax, perc_batch_item *out);

/* ---- batch of cluster tables (one workgroup per item) ----------------- *
 * Every reference program writes its cluster table c(label): cln, maxcn,
 * maxcs and the size of every cluster.  perc_batch_clusters forms that table's
 * statistics for many (trial, nsites, nbonds) items in one launch -- the
 * items, orders, counts and NULL rules of perc_batch_cond (a count of t + 1 /
 * nb + 1 is the whole order; the spill slot takes a position and is no
 * element) -- with the labeling and the spanning rule of perc_batch_scan.
 * The clusters are the programs' non-empty c(label) entries; the phantom
 * label the spill slot opens (hazard H2) is none and is never counted:
 *   PERC_BOND      a connected set of occupied bonds (a site with no occupied
 *                  bond is in none); size = its bonds
 *   PERC_SITE      a connected set of occupied sites over the lattice's
 *                  bonds, an isolated occupied site too; size = its sites
 *   PERC_SITEBOND  a component of occupied sites linked by occupied bonds
 *                  whose end sites are both occupied; size = its sites plus
 *                  every occupied bond with at least one end site in it
 *                  (sitebond.f's count)
 *   PERC_SITEBOND, lone bond: an occupied bond with both end sites empty;
 *                  size 1, it never spans
 * The sizes do not depend on the order of occupation.  Several clusters may
 * span; there is no fallback item: the record sums over all of them.
 * Histogram row i (nexact + 32 ints): hist[s - 1] = clusters of size s for
 * 1 <= s <= nexact, hist[nexact + floor(log2 s)] for every cluster (the octave
 * part is complete on its own).  hist may be NULL.  The call chunks itself so
 * that one launch's rank arrays and its histogram rows each stay under 64 MB
 * of device memory, and leaves the context's single-realisation state
 * untouched.  nitems == 0 is PERC_OK.  PERC_EINVAL (text in perc_last_error),
 * before any device call: a lattice / nexact perc_batch_clusters_supported
 * refuses, a bad kind, ntrials or nitems < 0, a missing list that the kind
 * reads, item_trial outside 0..ntrials-1, a count outside 0..t+1 / 0..nb+1;
 * the seeded form: a list perc_shuffle_device_supported refuses. */
typedef struct {
  int nclusters;   /* clusters counted, lone bonds included */
  int nlone;       /* mixed kind: lone bonds; else 0 (perc_label's nclusters = nclusters - nlone) */
  int nspan;       /* spanning clusters */
  int span_root;   /* smallest spanning root (min site id), 0 if none */
  int span_size;   /* size of that cluster, 0 if none */
  int maxcs;       /* largest size, 0 if no cluster */
  long long s1, s2;            /* sum of s, sum of s^2 over all clusters */
  long long span_s1, span_s2;  /* the same over the spanning clusters only */
} perc_cluster_item;
/* host-only: 1 when the cluster kernel can run this lattice with this exact
   range: what perc_scan_supported accepts (m, n >= 3, m*n <= 16384 sites) and
   0 <= nexact <= 1024 (the histogram row beside the scan's arena in the
   workgroup's 160 KB of LDS). */
int perc_batch_clusters_supported(int lattice, int m, int n, int pbc, int nexact);
int perc_batch_clusters(perc_ctx *h, int kind, int ntrials,
                        const int *site_orders /* ntrials x (t+1), NULL for PERC_BOND */,
                        const int *bond_orders /* ntrials x (nb+1), NULL for PERC_SITE */,
                        int nitems, const int *item_trial,
                        const int *item_nsites /* NULL for PERC_BOND */,
                        const int *item_nbonds /* NULL for PERC_SITE */,
                        int nexact, perc_cluster_item *out,
                        int *hist /* nitems x (nexact+32), or NULL */);
/* the same with seed lists (one seed per trial) in place of the order lists,
   the orders shuffled on the device into the batch rank buffers
   (perc_batch_shuffle): the same records item for item */
int perc_batch_clusters_seeded(perc_ctx *h, int kind, int ntrials,
                               const int *site_seeds /* ntrials, NULL for PERC_BOND */,
                               const int *bond_seeds /* ntrials, NULL for PERC_SITE */,
                               int nitems, const int *item_trial, const int *item_nsites,
                               const int *item_nbonds, int nexact, perc_cluster_item *out,
                               int *hist);

/* ---- batch cluster geometry (the same kernel, one more record) -------- *
 * perc_batch_clusters_geom is perc_batch_clusters that also returns the
 * clusters' radii of gyration and the sums behind the correlation length,
 * all of it in integers.
 * Member sites of a cluster: its occupied sites (PERC_SITE, PERC_SITEBOND);
 * the end sites of its bonds (PERC_BOND).  A mixed-kind lone bond has no
 * member site and does not enter.  n_c = the number of member sites (the
 * cluster's `size` for the site kind only).
 * Integer squared distance d2(i, j) of the sites at (row r, column c),
 * 0-based, row-major from the bottom row:
 *   PERC_SQUARE      d2 = dc^2 + dr^2                              unit = 1
 *   PERC_TRIANGULAR  d2 = 3 dc^2 + dY^2, Y = 2 r - (c & 1)         unit = 4
 * (odd 0-based columns sit half a spacing lower; 4 x the squared distance:
 * every bond of an even-m open lattice has d2 = 4).  The positions are (r, c)
 * whatever the bonds are, so the definition holds for every m.
 * Per cluster, G_c = sum over member pairs i < j of d2(i, j)
 *                  = n_c sum_i |r_i|^2 - |sum_i r_i|^2
 * (on the triangular lattice the second term is 3 (sum c)^2 + (sum Y)^2); it
 * does not depend on the origin; R_c^2 = G_c / (unit n_c^2).
 *   xi^2 = 2 (g2 - span_g2) / (unit (n2 - span_n2))
 *   the largest cluster's R^2 = big_g2 / (unit big_n^2)
 * rows (optional, 3 x 32 long long per item): for the octave b =
 * floor(log2 n_c), rows[b] = the number of clusters, rows[32 + b] = sum n_c^2,
 * rows[64 + b] = sum G_c -- R_s^2(s) and with it the fractal dimension.
 * An item with no cluster has an all-zero record and all-zero rows.
 * pbc = 0 only (with the left/right wrap the radius has no single meaning).
 * Everything else -- items, orders, counts, chunking, errors -- is
 * perc_batch_clusters'; out and hist are bit for bit what that call gives. */
typedef struct {
  int n1;          /* sum of n_c over all clusters */
  int span_n1;     /* ... over the spanning clusters (k_span_top's rule, as in perc_cluster_item) */
  int big_root;    /* root (min site id) of the cluster with the most member sites (tie: smallest root), 0 if none */
  int big_n;       /* its n_c */
  int root_n;      /* n_c of the cluster perc_cluster_item's span_root names, 0 if none */
  int pad;
  long long n2, g2;            /* sum of n_c^2, sum of G_c over all clusters */
  long long span_n2, span_g2;  /* the same over the spanning clusters */
  long long big_g2;            /* G_c of the largest cluster */
  long long root_g2;           /* G_c of the span_root cluster, 0 if none */
} perc_cluster_geom;
/* host-only: perc_batch_clusters_supported with pbc == 0 */
int perc_batch_geometry_supported(int lattice, int m, int n, int pbc, int nexact);
int perc_batch_clusters_geom(perc_ctx *h, int kind, int ntrials,
                             const int *site_orders, const int *bond_orders,
                             int nitems, const int *item_trial, const int *item_nsites,
                             const int *item_nbonds, int nexact, perc_cluster_item *out,
                             int *hist /* nitems x (nexact+32), or NULL */,
                             perc_cluster_geom *geom,
                             long long *rows /* nitems x 96, or NULL */);
int perc_batch_clusters_geom_seeded(perc_ctx *h, int kind, int ntrials,
                                    const int *site_seeds, const int *bond_seeds,
                                    int nitems, const int *item_trial, const int *item_nsites,
                                    const int *item_nbonds, int nexact, perc_cluster_item *out,
                                    int *hist, perc_cluster_geom *geom, long long *rows);

/* ---- batch current distributions (one workgroup per item) ------------- *
 * perc_batch_cond returns Gtop and Gbot and drops the voltages between them.
 * perc_batch_cond_currents is perc_batch_cond (it always solves) that also
 * says where the current flows: per item one perc_batch_currents record and,
 * where vint_out is given, the interior voltages -- what a user of the
 * reference's ConductCalc otherwise forms with a loop of their own over the
 * bond list, one realisation at a time.
 * Definition.  V: 0 on the bottom row, Va on the top row, the interior
 * solution x elsewhere (row i of the system is site i + m + 1).  A bond is
 * conducting when the kind's rule gives it g0 (occupied as the kind asks, and
 * in the chosen spanning cluster).  Counted, each once: the conducting bonds
 * with at least one interior end site (a bond inside an electrode row has
 * zero drop by construction).  Per bond i_b = g0 * (V[b2] - V[b1]), one
 * subtraction and one multiplication; only |i_b| is used.
 * nbonds, nabove, imax and hist are exact functions of the voltages' bits.
 * The four sums have no literal reference order: on the device each thread
 * sums its rows in row order with slots ascending and the workgroup's fixed
 * tree combines them -- deterministic and independent of the item's place in
 * the launch under both dot orders; perc_current_stats_host sums in bond-id
 * order.  The two agree to rounding ((nbonds + 8) ulp relative), not bitwise.
 * cut: the backbone at cut is the bonds with |i| >= cut * imax.  A dangling
 * end of the spanning cluster carries no current, but the solve leaves it the
 * residual's noise: about 1e-9 of imax at tol = 1e-8, about 1e-12 at a tight
 * tol.  cut must sit above that noise -- the caller's choice of tol decides
 * how small a cut still separates the backbone.
 * The default kernel only (k_batch_cond, at most 8192 interior rows): the
 * large kernel keeps x on 2m rows and the weighted one has other bond values,
 * so neither has this form, and the calls do not read the
 * perc_set_batch_large flag.  out is filled exactly as perc_batch_cond fills
 * it.  An item no cluster spans has an all-zero record and zero voltages.  An
 * item several clusters span (fallback = 1) runs through perc_occupy /
 * perc_label / perc_conductance on the context and perc_current_stats_host,
 * and leaves the context as perc_batch_cond does.  The call chunks itself as
 * perc_batch_cond, with 8 N more bytes per item against the 64 MB bound when
 * vint_out is given.  PERC_EINVAL (text in perc_last_error), before any
 * device call: perc_batch_cond's cases, cur == NULL, cut outside [0, 1] or
 * NaN, a lattice perc_batch_currents_supported refuses for the kind. */
typedef struct {
  int nbonds;              /* conducting bonds counted                       */
  int nabove;              /* of them, |i| >= cut * imax  (the backbone at cut) */
  double imax;             /* max |i|                                        */
  double s1, s2, s4, s6;   /* sum |i|, i^2, i^4, i^6  (i2 = i*i, i4 = i2*i2, i6 = i4*i2) */
  int hist[64];            /* octaves: bin = clamp(ilogb(g0*Va) - ilogb(|i|), 0, 63); |i| == 0 -> 63 */
} perc_batch_currents;
/* host-only: exactly perc_batch_cond_supported */
int perc_batch_currents_supported(int kind, int lattice, int m, int n, int pbc);
int perc_batch_cond_currents(perc_ctx *h, int kind, int rule, int cur_rule, int ntrials,
                             const int *site_orders /* ntrials x (t+1), NULL for PERC_BOND */,
                             const int *bond_orders /* ntrials x (nb+1), NULL for PERC_SITE */,
                             int nitems, const int *item_trial,
                             const int *item_nsites /* NULL for PERC_BOND */,
                             const int *item_nbonds /* NULL for PERC_SITE */,
                             double Va, double g0, double leak, int itol, double tol, int itmax,
                             perc_batch_item *out, double cut, perc_batch_currents *cur /* nitems */,
                             double *vint_out /* nitems x N, or NULL */);
/* the same with seed lists (one seed per trial), the orders shuffled on the
   device: the same records item for item */
int perc_batch_cond_currents_seeded(perc_ctx *h, int kind, int rule, int cur_rule, int ntrials,
                                    const int *site_seeds /* ntrials, NULL for PERC_BOND */,
                                    const int *bond_seeds /* ntrials, NULL for PERC_SITE */,
                                    int nitems, const int *item_trial, const int *item_nsites,
                                    const int *item_nbonds, double Va, double g0, double leak,
                                    int itol, double tol, int itmax, perc_batch_item *out,
                                    double cut, perc_batch_currents *cur, double *vint_out);
/* The record of one realisation on the host (no device): the bond list in id
   order, conducting[id - 1] != 0 the conducting bonds, vint the t - 2m
   interior voltages, the sums in bond-id order.  PERC_EINVAL: a bad lattice,
   m or n < 1, a NULL array, cut outside [0, 1] or NaN. */
int perc_current_stats_host(int lattice, int m, int n, int pbc,
                            const unsigned char *conducting /* nb, by bond id */,
                            const double *vint, double Va, double g0, double cut,
                            perc_batch_currents *out);

/* ---- ensemble statistics (bond_cond, config 4) ----------------------- */
/* Accumulate stats for one pb point: {count, sum G, sum G^2, count spanning,
   sum iter} into acc[5*point..]. */
void perc_stats_accumulate(double *acc, int point, double g, int spanning, int iter);

/* ---- multi-GPU ensemble (one process, one host thread per device) ----- *
 * Replaces the reference's serial trial loop (Fortran/Square/bond_cond.f:
 * 62-70 seeds, :123-498 trials, rows written at :481-482).  Trial ii
 * (1-based) runs on device (ii-1) mod ndev; each device has its own
 * perc_ctx and host thread; per-trial results land in the caller's arrays
 * at index ii-1 (ii order whatever device ran them).  The only collective
 * is one RCCL all-reduce (sum, fp64) over a communicator ncclCommInitAll
 * builds across the devices. */
typedef struct perc_ensemble perc_ensemble;
/* devices == NULL: devices 0..ndev-1 */
int perc_ensemble_create(int ndev, const int *devices, int lattice, int m, int n, int pbc,
                         perc_ensemble **out);
int perc_ensemble_destroy(perc_ensemble *e);
int perc_ensemble_ndev(perc_ensemble *e);
/* W (1..64) contexts, host threads and streams per device for the trial
   loops (default 1): trial ii runs on device (ii-1) mod ndev and there on
   worker ((ii-1) / ndev) mod W; per-trial results are the same, the
   per-device statistics are summed over the workers in worker order before
   the all-reduce.  For small lattices, whose trials leave a device mostly
   idle.  perc_ensemble_workers returns W. */
int perc_ensemble_set_workers(perc_ensemble *e, int workers);
int perc_ensemble_workers(perc_ensemble *e);
/* Batch path of perc_ensemble_bond_cond (default 0: the per-trial loop):
   with items > 0 and a lattice perc_batch_supported accepts, each device's
   trials run in groups of about `items` (trial, grid point) realisations --
   the orders shuffled on the host (perc_shuffle_seeded), one
   perc_batch_bondc launch per group for the conductances, bf_c by one
   scan launch over the group's trials (one workgroup bisects each, as
   perc_batch_scan), perccln by perc_replay_labels -- with the per-trial loop's stop
   rules, outputs and statistics (accumulated in ascending trial order; the
   workers setting is not used).  Gtop / Gbot differ from the per-trial
   loop's only by the association of the fast dot order's sums (bitwise the
   same under PERC_DOT_LITERAL).  On an unsupported lattice the setting is
   ignored and perc_ensemble_batch returns 0, else it returns items. */
int perc_ensemble_set_batch(perc_ensemble *e, int items);
int perc_ensemble_batch(perc_ensemble *e);
/* perc_set_batch_large on every device's context (enable != 0: the batch
   path runs the large kernel); while set, perc_ensemble_batch goes by
   perc_batch_large_supported(PERC_BOND, ..) instead of perc_batch_supported,
   so the setting of perc_ensemble_set_batch holds up to 128 x 128 */
int perc_ensemble_set_batch_large(perc_ensemble *e, int enable);
/* device dev's own context (e.g. for single-trial calls); NULL if out of range */
perc_ctx *perc_ensemble_ctx(perc_ensemble *e, int dev);
/* the trials device `dev` of `ndev` runs, 1-based, ascending (ii_out may be
   NULL); returns their count.  Host-only. */
int perc_ensemble_trials(int ntrials, int ndev, int dev, int *ii_out);
/* stats holds ndev slices of k doubles (device d's at stats[d*k]); on return
   every slice holds the element-wise sum over the devices (ncclAllReduce). */
int perc_ensemble_allreduce(perc_ensemble *e, double *stats, int k);
/* bond_cond over the devices: trial ii shuffles with tseed[ii-1] (tseed must
   hold at least ntrials seeds; the reference's tseed(1000) caps numtrials at
   1000, bond_cond.f:62-70, callers extend the stream past it) (REAL*4
   Fisher-Yates, bondc.f:162-174), computes the lowest-label conductance at
   grid points nbarr[0..) until a value <= 0, a repeat (hazard H3) or npts;
   outputs, per trial t = ii-1: nrows[t] rows at [t*npts + j] of gbot, gtop,
   iters; bf_c[t] = first spanning bond count (0: none), perccln[t] = lowest
   spanning label with every bond occupied (bond_cond.f:381, 486-496).
   stats (npts*5, may be NULL) = the all-reduced {count, sum Gtop,
   sum Gtop^2, count spanning, sum iter} per grid point. */
int perc_ensemble_bond_cond(perc_ensemble *e, int ntrials, const int *tseed, int npts,
                            const int *nbarr, double Va, double g0, double tol, int itmax,
                            int *nrows, double *gbot, double *gtop, int *iters, int *bf_c,
                            int *perccln, double *stats);
/* REAL*4 Fisher-Yates of ids 1..N after srand(seed) on a stream local to the
   call (thread-safe; same sequence as perc_srand + perc_shuffle): order has
   N+1 slots, order[N] = 0 (hazard H2). */
void perc_shuffle_seeded(int seed, int N, int *order);

/* ---- Numerical-Recipes-compatible layer (F77 ABI, by reference) ------- *
 * Same names and argument meaning as the routines embedded in the
 * reference (Square/bondc.f:723-917).  linbcg_/atimes_/asolve_ read the
 * matrix from COMMON /mat/ sa(NMAX), ija(NMAX) (symbol mat_, NMAX=20000 as
 * in the reference) unless perc_nr_bind() points them at other storage.
 * linbcg_ runs the HIP PCG on device 0.  Errors that `pause` in the
 * reference are reported through perc_nr_status().  Malformed storage is
 * PERC_EMISMATCH before any device call: ija(1) != n+2, a column outside
 * 1..n, descending row pointers, and on the bound paths ija(n+1)-1 > nmax
 * (perc_nr_bind's nmax; nmax <= 0 there means NMAX). */
void sprsin_(double *a, int *n, int *np, double *thresh, int *nmax, double *sa, int *ija);
void dsprsax_(double *sa, int *ija, double *x, double *b, int *n);
void dsprstx_(double *sa, int *ija, double *x, double *b, int *n);
void atimes_(int *n, double *x, double *r, int *itrnsp);
void asolve_(int *n, double *b, double *x, int *itrnsp);
double snrm_(int *n, double *sx, int *itol);
void linbcg_(int *n, double *b, double *x, int *itol, double *tol, int *itmax,
             int *iter, double *err);
void perc_nr_bind(double *sa, int *ija, int nmax);
int perc_nr_status(void);
int perc_nr_status_(void);  /* F77 spelling: `integer perc_nr_status` */
/* association of linbcg_'s dot products (PERC_DOT_LITERAL by default: the
   NR drop-in reproduces the reference solver bitwise; PERC_DOT_FAST: the
   wave-tree sums of perc_conductance) */
int perc_nr_set_dot_order(int order);
/* perc_last_solve of linbcg_'s own context (PERC_ESTATE before its first solve) */
int perc_nr_last_solve(int *out4);
/* call nearestn(rn) (Square/bondc.f:617-715, Triangular/bondc.f:619-804):
   the neighbours of site rn into the caller's blank COMMON m, n, t, pbc,
   nn(10), scn (symbol __BLNK__; scn 4 square, 6 triangular), zeros where a
   neighbour is missing; perc_nr_status() = PERC_ESTATE without one. */
void nearestn_(const int *rn);

#ifdef __cplusplus
}
#endif
#endif /* PERC_H */
