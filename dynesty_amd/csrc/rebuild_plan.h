// Internal: what a rebuild launches and where its scratch lies (rebuild.hip), as plain host arithmetic.
//
// rebuild_plan() decides every size of one rebuild -- the scalars of RebuildArgs, the LDS of each kernel, the grid of
// each launch, the chunks that keep workgroups meeting at spin waits resident together -- from the shape, what the
// device can hold (RebuildCaps) and the diagnostic switches; rebuild_layout() places the scratch arrays.  Neither
// touches the device or the environment, so a host program holds them to their invariants
// (tests/test_rebuild_plan_cpu.py).  Plain C++17: no HIP include.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/dynhip.h"

#ifdef __HIPCC__
#define DH_PLAN_HD __host__ __device__
#else
#define DH_PLAN_HD
#endif

namespace dh_plan {

constexpr int kThreads = 256;
constexpr int kBarStride = 16;  // ints between part-barrier counters (one per 64-byte line)
// k_ell_wave: the largest node one wavefront builds
constexpr int kWaveCap = 128;
// what a kernel may ask of a CU's 160 KB of LDS
constexpr size_t kLdsLimit = 159 * 1024;
// separate Jacobi buffers only while two workgroups still fit one CU's 160 KB
constexpr size_t kLdsSeparate = 79 * 1024;

// The common layout (carve) without the Jacobi work buffers (16-byte multiple); they follow at this offset when
// everything fits kLdsSeparate, else they overlay the point tile.
DH_PLAN_HD inline size_t rebuild_lds_base_bytes(int D, int TP) {
  const int LD = D | 1;
  const size_t dbl = (size_t)TP * LD + 4 * (size_t)D * LD + 7 * (size_t)D + 2 + kThreads + 128;
  return (dbl * 8 + (320 + (size_t)D + 8) * 4 + 15) & ~(size_t)15;
}

DH_PLAN_HD inline size_t rebuild_lds_bytes(int D, int TP = kThreads) {
  const size_t base = rebuild_lds_base_bytes(D, TP);
  const int P = (D + 1) & ~1;
  const size_t jb = 4 * (size_t)P * (P | 1) * 8;
  return base + jb > kLdsSeparate ? base : base + jb;  // else the Jacobi buffers overlay the tile
}

// k_split's own, smaller layout (carve_split): the resident tile of tps points and what the k-means touches (scale,
// centroids, sums, the partial-sum scratch, the integer scratch) -- 31 KB at D = 25, tps = 128, so that five workgroups
// share a CU.  (With the common layout's 77 KB two did, and a level of the 64-run bench rebuild has 512-1 000 busy
// parts: every level took two rounds of workgroups, 135 us instead of the 65-70 us it takes alone.)
DH_PLAN_HD inline size_t split_lds_bytes(int D, int TP) {
  const int LD = D | 1;
  return ((((size_t)TP * LD + 5 * (size_t)D + 2 + kThreads + 128) * 8 + (320 + (size_t)D + 8) * 4) + 15) & ~(size_t)15;
}

// k_ell_wave's layout (carve_wave): a tile of kWaveCap points and four D x D matrices
DH_PLAN_HD inline size_t wave_lds_bytes(int D) {
  const int LD = D | 1;
  return ((((size_t)kWaveCap * LD + 4 * (size_t)D * LD + 2 * (size_t)D + 64) * 8) + 15) & ~(size_t)15;
}

// What the device and the context contribute.  The occupancies are workgroups per CU as the runtime reports them for
// k_root_parts and k_tree with the common layout and for k_split with its own (occ_tree: asked only where there is a
// tail); a query that fails counts as 1.
struct RebuildCaps {
  int num_cu;
  int occ_root, occ_split, occ_tree;
  int split_resident_pct;  // DH_SPLIT_RESIDENT_PCT, through the context: the share of the chip a chunk of k_split may claim
  int coop_launch;         // DH_COOP_LAUNCH, through the context: k_root_parts goes through the cooperative launch
};

// The diagnostic environment switches, read by the caller on every call (the sixth, DH_SPLIT_RESIDENT_PCT, is read
// when the context is created and arrives with the caps).
struct RebuildSwitches {
  int fast = 1;        // DH_REBUILD_FAST: 0 = eigh on every node
  int deep = 1;        // DH_DEEP: 0 = every level by level kernels and no work-queue tail
  int deep_from = -1;  // DH_DEEP_FROM=f: the tail takes over at level f
  int root_parts = 1;  // DH_ROOT_PARTS: 0 = the single-workgroup root for every run
  int wave_ell = 1;    // DH_WAVE_ELL: 0 = no one-wavefront nodes
};

// One (k_split, k_ell_wave, k_ell) step of the level pipeline.
struct RebuildLevel {
  int gp;          // k_split: parts per run -- grid nchunk x cr x gp
  int cr, nchunk;  // k_split: runs per co-resident chunk, chunks
  int ge;          // children a run can have at this level
  int ge_l, gw_l;  // workgroups per run of k_ell (eigen-free forms) and of k_ell_wave
  int g_ell;       // k_ell's workgroups per run as launched: ge_l, or ge in the slow form
  int wave;        // k_ell_wave runs in front of k_ell
  int top, tp;     // k_ell stages tiles of tp = 512 points (top) or 256
  size_t lds_ell;
};

// levels = 2 lv + 8 with 2^lv >= n / 2d + 1: lv <= 16 for the n <= 65 536 of MultiEllipsoid.update
constexpr int kMaxLevels = 2 * 16 + 8;

struct RebuildPlan {
  int runs, n, d, mode, max_ells;
  size_t node_bytes;
  RebuildSwitches sw;
  // scalars of RebuildArgs
  int max_nodes, reslist_cap, maxw, levels, tps, maxp, fast, tree_from, tq_cap, kp_cap, fin_extra_off, fin_res_lds;
  size_t rootbuf_stride;
  double prefactor;
  int nlev;       // levels built by level kernels
  int tail;       // whatever is deeper goes to k_tree
  int wave_from;  // first level whose small nodes k_ell_wave takes (nlev: none)
  size_t lds, lds_split, lds_wave, lds_top, lds_fin;  // common layout | k_split | k_ell_wave | k_ell's 512-point tile (0: none) | k_finish
  // from the caps
  int cap_root, cap_split_level, cap_tree, cap_split;  // co-resident workgroups; cap_split: of the parts of ONE node
  int rp, root_chunk;                                  // k_root_parts: parts per run, runs per launch
  int g_tree;                                          // k_tree's grid
  int g_out;                                           // k_out_eig: workgroups per run
  RebuildLevel level[kMaxLevels];
};

inline bool rebuild_shape_ok(int n, int d, int mode, int max_ells) {
  return n >= 1 && d >= 1 && max_ells >= 1 && (mode == 0 || mode == 1);
}

constexpr size_t kPlanErrLen = 256;

// Step 1: the argument checks of the narrow path and everything that needs no caps -- the occupancy queries behind
// the caps need lds, lds_split and tail.  DH_OK, or DH_ERR_ARG with the text in err.
inline int rebuild_plan_sizes(int runs, int n, int d, int mode, int max_ells, const RebuildSwitches& sw, size_t node_bytes,
                              RebuildPlan& p, char* err) {
  if (!rebuild_shape_ok(n, d, mode, max_ells)) {
    snprintf(err, kPlanErrLen, "rebuild: bad arguments (n=%d d=%d mode=%d)", n, d, mode);
    return DH_ERR_ARG;
  }
  p.lds = rebuild_lds_bytes(d);
  if (p.lds > kLdsLimit) {
    snprintf(err, kPlanErrLen, "rebuild: d=%d is beyond the narrow path", d);
    return DH_ERR_ARG;
  }
  if ((long long)n * d >= (1ll << 31)) {  // (rows are addressed by 32-bit element offsets: stage_tile)
    snprintf(err, kPlanErrLen, "rebuild: n x d = %lld elements per run exceeds 2^31", (long long)n * d);
    return DH_ERR_ARG;
  }
  // the parts of one node meet at a device-scope barrier, so they must all be resident at the
  // same time: 256 parts (65 536 points per run) fit the 256 CUs with room to spare
  if (mode == 0 && n > 256 * kThreads) {
    snprintf(err, kPlanErrLen, "rebuild: MultiEllipsoid.update supports at most %d points per run (n = %d)", 256 * kThreads, n);
    return DH_ERR_ARG;
  }
  p.runs = runs;
  p.n = n;
  p.d = d;
  p.mode = mode;
  p.max_ells = max_ells;
  p.node_bytes = node_bytes;
  p.sw = sw;
  // every split creates two children of >= 2d points each: <= n/d nodes + root
  p.max_nodes = mode == 1 ? 1 : (n / d + 3);
  p.prefactor = d * log(2.0) + d * lgamma(1.5) - lgamma(d / 2.0 + 1.0);
  p.reslist_cap = p.max_nodes * 24 + 64;
  p.maxw = n / (4 * d) + 1;
  // depth: a balanced tree needs log2(n / 2d) levels; unbalanced splits need more.  The level kernels are launched
  // for lv levels, the work-queue form (k_tree) takes whatever is deeper.
  int lv = 4;
  while ((1 << lv) < n / (2 * d) + 1) ++lv;
  p.levels = mode == 1 ? 0 : (2 * lv + 8);
  // 128 points per k-means part: five k_split workgroups per CU (see split_lds_bytes) -- or 256 where five 256-point
  // tiles fit a CU's LDS as well (D <= 13): half the parts to meet at the device-scope barrier.  Measured (round 5, 64
  // sets, tools/r5_tps.sh): eggbox 2-D 4.48 -> 4.10 ms, two blobs 5-D 0.720 -> 0.704; at D = 25 256-point parts lose
  // (1.26 -> 1.40 ms: two workgroups per CU).
  p.tps = split_lds_bytes(d, 256) * 5 <= kLdsLimit ? 256 : 128;
  p.maxp = n / p.tps + p.maxw + 1;
  // eigen-free tree nodes (MultiEllipsoid.update only: Ellipsoid.update's single node IS the output)
  p.fast = mode == 0 && sw.fast != 0 ? 1 : 0;
  // The tree is built by the level pipeline (k_split / k_ell per level) for a balanced tree's depth (lv levels: an
  // idle level pair costs 10 us, and the bench trees use lv = 6 exactly);
  // whatever is deeper -- unbalanced splits -- is handed to persistent workers on a work queue (k_tree: the same
  // node routines, any depth, any node size; in the common case it finds its queue empty and leaves).
  // (The WHOLE tree by the work-queue form, DH_DEEP_FROM=0, gives the same bits but was measured slower in round 3:
  // 64 C2 runs 1.44 against 1.29 ms -- it loses the level pipeline's five k_split workgroups per CU.)
  // DH_DEEP=0: every level by level kernels and no tail, as does the diagnostic slow mode; DH_DEEP_FROM=f: the tail
  // takes over at level f.
  // (one level pair fewer -- a balanced tree's last split level is the one with n >> L >= 4 d: five pairs for the
  // bench's 2000 x 25 live sets instead of six -- was measured in round 5 and is SLOWER: 1.411 against 1.382 ms per
  // 64-run rebuild, eggbox 5.02 against 4.51: real trees are not balanced, and what is deeper than the level kernels
  // goes to the work-queue tail, which costs more than an almost idle level pair)
  p.nlev = p.levels;
  if (p.fast && sw.deep != 0) p.nlev = p.levels < lv ? p.levels : lv;
  if (p.fast && sw.deep_from >= 0 && sw.deep_from < p.levels) p.nlev = sw.deep_from;
  p.tail = p.fast && p.nlev < p.levels;
  p.tree_from = p.tail ? p.nlev : p.levels + 1;
  p.tq_cap = 0;
  p.kp_cap = 0;
  if (p.tail) {
    // partial-sum slots of the multi-part nodes the queue form may meet: a depth has at most n / tps + (nodes) parts
    p.kp_cap = p.levels * (n / p.tps + 1) + 8;
    // items: one ellipsoid per node, and per split node ceil(count / tps) parts
    p.tq_cap = runs * (2 * p.max_nodes + p.levels * (n / p.tps + 1) + 8);
  }
  p.lds_split = split_lds_bytes(d, p.tps);
  // k_finish: tree (and result list) in LDS when they fit behind the standard layout
  p.lds_fin = p.lds;
  p.fin_extra_off = 0;
  p.fin_res_lds = 0;
  const size_t off = (p.lds + 15) & ~(size_t)15;
  const size_t nb_nodes = (size_t)p.max_nodes * node_bytes, nb_res = (size_t)p.reslist_cap * 4;
  if (off + nb_nodes <= kLdsLimit) {
    p.fin_extra_off = (int)off;
    p.lds_fin = off + nb_nodes;
    if (p.lds_fin + nb_res <= kLdsLimit) {
      p.fin_res_lds = 1;
      p.lds_fin += nb_res;
    }
  }
  // k_ell's top levels: a tile of 512 points, if it fits (D <= 29)
  p.lds_top = rebuild_lds_bytes(d, 2 * kThreads);
  if (p.lds_top > kLdsLimit || mode != 0) p.lds_top = 0;
  // small nodes by one wavefront each (k_ell_wave), from the level where the average child fits -- where eight such
  // nodes (128-point tile, four D x D matrices) share a CU's LDS: D <= 13.  Measured (round 5, 64 sets): eggbox 2-D
  // 6.54 -> 4.67 ms, two blobs 5-D 0.91 -> 0.75, 3-D blob 0.71 -> 0.62; above D = 13 the forms tried lost (1.29 -> 1.41
  // ms at D = 25).  DH_WAVE_ELL=0: off.
  p.wave_from = p.nlev;
  p.lds_wave = wave_lds_bytes(d);
  if (p.fast && sw.wave_ell != 0 && p.lds_wave * 8 <= kLdsLimit) {
    p.wave_from = 0;
    while (p.wave_from < p.nlev && (n >> (p.wave_from + 1)) > 2 * kWaveCap) ++p.wave_from;
  }
  p.g_out = max_ells < 8 ? max_ells : 8;
  return DH_OK;
}

// Step 2: the grids, from what can be resident.
// Co-residency.  Workgroups that meet at a spin barrier -- the parts of the root, the parts of one
// k-means node -- must be on the chip together.  How many workgroups of a kernel fit is asked of the
// runtime (occupancy API x CU count), not assumed.  The whole grid of k_root_parts must fit (every part
// waits for part 0's solve); for k_split a CHUNK of runs must (round 5: cr runs x the level's parts per run, sized
// to this capacity; inside a chunk the workgroups are ordered part-major so that every run starts at once): chunks
// have consecutive workgroup ids and the dispatcher hands out workgroups in id order, so the lowest unfinished
// chunk is always dispatched in full as the workgroups in front of it finish, and those never wait for it.
inline int rebuild_plan_grids(RebuildPlan& p, const RebuildCaps& c, char* err) {
  const int runs = p.runs, n = p.n;
  p.cap_root = c.num_cu * (c.occ_root > 0 ? c.occ_root : 1);
  p.cap_split_level = c.num_cu * (c.occ_split > 0 ? c.occ_split : 1);  // (k_split's own: what its chunks are sized to)
  p.cap_split = p.cap_split_level;
  p.cap_tree = 0;
  if (p.tail) {
    p.cap_tree = c.num_cu * (c.occ_tree > 0 ? c.occ_tree : 1);
    if (p.cap_tree < p.cap_split) p.cap_split = p.cap_tree;  // the parts of a node may be k_tree workgroups
  }
  // parts of the root: cooperative only while all parts of all runs are resident with room to spare
  // (a part idles at a barrier while part 0 runs the eigensolver, so on a full chip it only costs slots)
  // The parts of a run meet at spin waits, so what is launched together must be resident together: when all runs x
  // parts do not fit, the root goes in chunks of runs that do (round 6; before, 128 runs x 8 parts fell back to the
  // single-workgroup root, 447 us against 81 us per 64 runs).
  p.rp = n > 1 ? (n + kThreads - 1) / kThreads : 1;
  if (p.rp > p.cap_root || (c.coop_launch && (long long)runs * p.rp > p.cap_root)) p.rp = 1;
  if (p.sw.root_parts == 0) p.rp = 1;
  p.root_chunk = runs;
  if (p.rp > 1 && (long long)runs * p.rp > p.cap_root) p.root_chunk = p.cap_root / p.rp;
  if (p.mode == 0 && (n + p.tps - 1) / p.tps > p.cap_split) {
    snprintf(err, kPlanErrLen, "rebuild: the %d parts of a %d-point node exceed the %d co-resident workgroups of k_split",
             (n + p.tps - 1) / p.tps, n, p.cap_split);
    return DH_ERR_ARG;
  }
  p.rootbuf_stride = 2 * ((size_t)p.rp * (2 * (size_t)p.d + (size_t)p.d * p.d + 1) + (size_t)p.d * p.d + 8);  // (value, tag) pairs
  // (Leaves built beside the level kernels -- on the side stream, or by a light kernel of their own on the main
  // stream -- were measured no better in round 6: EXPERIMENTS.md.)
  for (int L = 0; L < p.nlev; ++L) {
    RebuildLevel& l = p.level[L];
    // Grids no larger than the level can need (round 5): level L splits at most 2^L nodes of a run -- at most
    // n / tps + 2^L parts -- and creates at most 2^(L + 1) children.  Workgroups are dispatched at a finite rate: the
    // 2 368 / 2 688-workgroup grids of the worst case cost the first levels 60 us each at 64 runs, most of them for
    // workgroups that found nothing to do.
    const long long nodes_L = L < 20 ? (1ll << L) : (1ll << 20);
    // (k_split keeps the worst case gp: a loop over parts in it costs registers it does not have -- 5 spilled VGPRs --
    // and, where the parts are real, serialises two k-means chains)
    l.gp = (int)(p.maxp < (long long)n / p.tps + nodes_L + 1 ? p.maxp : (long long)n / p.tps + nodes_L + 1);
    l.ge = (int)(2ll * p.maxw < 2 * nodes_L ? 2ll * p.maxw : 2 * nodes_L);
    // runs per chunk: cr * gp workgroups resident together, with an eighth of the chip to spare (the side stream's
    // kernels hold slots too; a chunk that does not fit would still finish -- they do not wait for it -- only later)
    // (ONE context per GPU is assumed, as for k_root_parts: a second process -- or a long-lived foreign kernel -- can
    // hold slots this sizing counts on; DH_SPLIT_RESIDENT_PCT lowers the share of the chip a chunk may claim (87 by
    // default, e.g. 40 on a GPU shared by two processes), and the spin limit fails a starved run instead of hanging)
    const int split_room = p.cap_split_level > 0 ? (int)((long long)p.cap_split_level * c.split_resident_pct / 100) : 1;
    l.cr = p.cap_split_level > 0 ? split_room / l.gp : 1;
    l.cr = l.cr < 1 ? 1 : (l.cr > runs ? runs : l.cr);
    l.nchunk = (runs + l.cr - 1) / l.cr;
    l.cr = (runs + l.nchunk - 1) / l.nchunk;  // (chunks of equal size)
    // (round 6) no more k_ell / k_ell_wave workgroups than a few rounds of the chip: a workgroup takes every ge-th child
    // of its run (the kernels' own loops).  The bound above is the worst case; a many-mode tree's deep level (eggbox 2-D,
    // nlive 5 000, 16 runs: 1 065 parts and 1 252 children possible per run, some 200 there) was 20 000 workgroups of
    // which a fifth found work, and the dispatch of the rest half the level's time.
    const int cap_ell = 2 * c.num_cu;  // (k_ell: two workgroups per CU)
    const int want_e = 8 * cap_ell / runs > 1 ? 8 * cap_ell / runs : 1;
    l.ge_l = want_e < l.ge ? want_e : l.ge;
    l.g_ell = p.fast ? l.ge_l : l.ge;
    // (k_ell_wave: 16 384 one-wavefront workgroups; 8 192 / 4 096 / 2 048 measured on the C3 loop: 0.088 / 0.089 / 0.089 s
    // against 0.087 -- its time is its nodes, not its dispatch)
    const int want_w = 16384 / runs > 1 ? 16384 / runs : 1;
    l.gw_l = want_w < l.ge ? want_w : l.ge;
    l.wave = L >= p.wave_from ? 1 : 0;
    // The top levels' children are several 256-point tiles each and few (one workgroup per CU or less): their
    // workgroups stage 512 points at once -- a 1 000-point child is gathered three times instead of seven (covariance
    // pass 2 + Mahalanobis pass 1, the last tile still staged), a 500-point child once instead of three times.  Only
    // while the level's workgroups fill at most HALF the CUs (round 6: at 128 runs level 0's 256 one-per-CU workgroups
    // with the big tile lost to two-per-CU with the small one, 2.09 -> 2.05 ms; the LDS of such a tile allows no second one).
    const int child = L + 1 < 31 ? n >> (L + 1) : 0;  // the average child (DH_DEEP=0 runs level kernels beyond 2^31)
    l.top = p.lds_top > 0 && child > kThreads && 2ll * runs * l.ge <= c.num_cu ? 1 : 0;
    l.lds_ell = l.top ? p.lds_top : p.lds;
    l.tp = l.top ? 2 * kThreads : kThreads;
  }
  // k_tree's persistent workers: as many as can be resident (the parts of a node meet at spin barriers), but
  // no more than the tree can ever keep busy
  const long long want = (long long)runs * (n / p.tps + 2 * p.maxw + 1);
  p.g_tree = p.tail ? (int)(want < p.cap_tree ? (want < 1 ? 1 : want) : p.cap_tree) : 0;
  return DH_OK;
}

inline int rebuild_plan(int runs, int n, int d, int mode, int max_ells, const RebuildCaps& caps, const RebuildSwitches& sw,
                        size_t node_bytes, RebuildPlan& p, char* err) {
  const int rc = rebuild_plan_sizes(runs, n, d, mode, max_ells, sw, node_bytes, p, err);
  return rc ? rc : rebuild_plan_grids(p, caps, err);
}

// ---- the scratch --------------------------------------------------------------------------------------------------
enum RebuildArray {
  kWsPerm, kWsPerm2, kWsLab, kWsNodes, kWsEstore, kWsReslist, kWsCounters, kWsSplitList, kWsEllList, kWsScaleG,
  kWsPtsScaled, kWsPartList, kWsPartBase, kWsKpart, kWsKpartTail, kWsRootbuf, kWsFinLse, kWsFinInt, kWsOutNode,
  kWsOutFast, kWsRootEig, kWsArrays
};

struct RebuildSlot {
  const char* name;
  size_t off, bytes;  // bytes == 0: not wanted -- no room, a null pointer
};

// The zeroed counters, one contiguous block cleared by one memset per rebuild; offsets in ints from its start.
struct RebuildCounters {
  size_t nnodes, nsplit, nell, nparts, kerr, kbar;  // the level pipeline's
  size_t kp_top, tq_ctl, nbar, tq_items;            // k_tree's (with a tail only); tq_items on an 8-byte boundary
  size_t ints;
};

struct RebuildLayout {
  RebuildSlot slot[kWsArrays];
  RebuildCounters cnt;
  size_t total;
};

// THE list of the rebuild's scratch arrays, in the order they lie in the context's buffer (256-byte aligned): element
// size, element count, wanted or not.
inline void rebuild_layout(const RebuildPlan& p, RebuildLayout& l) {
  const size_t R = (size_t)p.runs, n = (size_t)p.n, d = (size_t)p.d, lev = (size_t)p.levels, maxw = (size_t)p.maxw;
  const size_t nodes = (size_t)p.max_nodes, maxp = (size_t)p.maxp;
  const bool multi = p.mode != 1, fast = p.fast != 0, tail = p.tail != 0;
  // the counters: nnodes | nsplit (levels+1) | nell (levels) | nparts (levels+1) | kerr | kbar (levels x maxw) | a spare
  // int per run || kp_top (runs) | tq_ctl (64) | nbar (runs x max_nodes x kBarStride) | tq_items (tq_cap x 2 ints)
  RebuildCounters& c = l.cnt;
  c.nnodes = 0;
  c.nsplit = c.nnodes + R;
  c.nell = c.nsplit + (lev + 1) * R;
  c.nparts = c.nell + lev * R;
  c.kerr = c.nparts + (lev + 1) * R;
  c.kbar = c.kerr + R;
  c.ints = c.kbar + lev * R * maxw * kBarStride + R;
  c.kp_top = c.tq_ctl = c.nbar = c.tq_items = 0;
  if (tail) {
    c.kp_top = c.ints;
    c.tq_ctl = c.kp_top + R;
    c.nbar = c.tq_ctl + 64;
    c.tq_items = (c.nbar + R * nodes * kBarStride + 1) & ~(size_t)1;  // 8-byte items (the block itself is 256-aligned)
    c.ints = c.nbar + R * nodes * kBarStride + 2 * (size_t)p.tq_cap + 2;
  }
  const size_t NS = d + 3 * d * d + d + d * (d | 1);  // a node's record in estore
  size_t off = 0;
  auto put = [&](RebuildArray id, const char* name, size_t elem, size_t count, bool wanted = true) {
    const size_t bytes = wanted ? elem * count : 0;
    l.slot[id] = {name, off, bytes};
    off += (bytes + 255) & ~(size_t)255;
  };
  put(kWsPerm, "perm", 4, R * n);
  put(kWsPerm2, "perm2", 4, R * n);
  put(kWsLab, "lab", 1, R * n);
  put(kWsNodes, "nodes", p.node_bytes, R * nodes);
  put(kWsEstore, "estore", 8, R * nodes * NS);
  put(kWsReslist, "reslist", 4, R * (size_t)p.reslist_cap);
  put(kWsCounters, "counters", 4, c.ints);
  put(kWsSplitList, "split_list", 4, 2 * R * maxw);
  put(kWsEllList, "ell_list", 4, (lev > 0 ? lev : 1) * R * 2 * maxw);
  put(kWsScaleG, "scale_g", 8, R * d);
  put(kWsPtsScaled, "pts_scaled", 8, R * n * d, multi);
  put(kWsPartList, "part_list", 4, 2 * R * maxp * 2);
  put(kWsPartBase, "part_base", 4, 2 * R * maxw);
  put(kWsKpart, "kpart", 16, 2 * R * maxp * (2 * d + 2), multi);                           // (value, tag) pairs
  put(kWsKpartTail, "kpart_tail", 16, 2 * R * (size_t)p.kp_cap * (2 * d + 2), tail);  // the queue form's own
  put(kWsRootbuf, "rootbuf", 8, R * p.rootbuf_stride);
  put(kWsFinLse, "fin_lse", 8, R * nodes);
  put(kWsFinInt, "fin_int", 4, R * nodes * 2);
  put(kWsOutNode, "out_node", 4, R * (size_t)p.max_ells, fast);
  put(kWsOutFast, "out_fast", 4, R * (size_t)p.max_ells, fast);
  put(kWsRootEig, "root_eig", 8, R * (2 * d * d + d + 2), fast);
  l.total = off;
}

}  // namespace dh_plan
