// Internal: what the combiner's entry points launch and where their scratch lies (merge.hip, merge_marginals.hip,
// merge_errors.hip), as plain host arithmetic.
//
// The constants the sizes depend on, the launch arithmetic as functions of the shape alone, and one layout per scratch
// user: THE list of that user's arrays -- element type, element count, wanted or not --, written once and walked twice
// by a Carver (carve.h), first without a base for the total, then with the block for the addresses (arena_carve of ctx.h,
// device_carve of merge_dev.h).  Nothing here touches the device, so a host program holds it to its invariants
// (tests/test_merge_plan_cpu.py).  Plain C++17: no HIP include.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "carve.h"

namespace dh_merge {

constexpr int kT = 256;
constexpr int kItems = 8;              // consecutive points per thread of a scan
constexpr int kChunk = kT * kItems;    // points per workgroup of a scan
constexpr int kLiveTile = 1024;        // live keys staged in LDS per step of the rank sort
constexpr long long kMomChunk = 2048;  // points per workgroup of the moment sums (at least)
constexpr size_t kScanElem = 16;       // the widest element of a scan's chunk aggregates (LsePair, Pair2L)

constexpr int kMT = 1024;         // threads per workgroup of the passes over the rows
constexpr int kSelTile = 78;      // 256-bin histograms of u64 per workgroup: 156 KB + their states of the CU's 160 KB
constexpr int kHistBins = 16384;  // 64-bit histogram bins per workgroup: 128 KB
constexpr int kMaxCols = 512;     // requested columns per call (the staging tables of the passes)
constexpr int kDigits = 12;       // 8 digits of the value's 64-bit image, 4 of the 32-bit point index

constexpr int kRealTile = 4;         // realizations a workgroup carries through its chunk
constexpr int kRealLaunch = 64;      // realizations per set of launches: the scratch is chunks x 64 x (6 + D) doubles
constexpr int kRealMax = 65536;      // realizations per call
constexpr int kSeg = kChunk / kT;    // a chunk's mean sums: kSeg segments of kT points, summed in segment order
constexpr int kColTile = kT / kSeg;  // columns per step of the mean sums
constexpr int kPart = 5;             // per (realization, chunk): max ln w, max ln w without logrwt, sum w, sum w^2, sum of H's terms
constexpr int kBootMax = 65536;      // bootstraps per call

// ---- launch arithmetic ----------------------------------------------------------------------------------------------

inline unsigned blocks_for(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

// the moment sums: chunks of *chunk points, at most 1024 of them
inline int moment_chunks(long long M, size_t cols, long long* chunk) {
  long long n = (M + kMomChunk - 1) / kMomChunk;
  const long long cap = (long long)(((size_t)8 << 20) / (cols ? cols : 1));  // at most 64 MB of partial sums
  if (n > 1024) n = 1024;
  if (n > cap) n = cap;
  if (n < 1) n = 1;
  *chunk = (M + n - 1) / n;
  return (int)((M + *chunk - 1) / *chunk);
}

// rows per workgroup: at least 256, at most 2048 workgroups
inline long long rows_per_group(long long M, unsigned* groups) {
  long long rows = (M + 2047) / 2048;
  if (rows < 256) rows = 256;
  *groups = (unsigned)((M + rows - 1) / rows);
  return rows;
}

// the quantile's tile over the requested columns: cpt columns (cpt * nq <= kSelTile selections) per step
struct QuantTile {
  int cpt;
  size_t lds_digit, lds_succ;  // mq_pass<false, .> (256 bins per selection) and mq_pass<true, .> (one)
  bool combine;                // 64 / columns lanes of a wavefront share a column
};
inline QuantTile quantile_tile(int nq, int ncol) {
  QuantTile t;
  t.cpt = kSelTile / nq;
  const int tile_cols = t.cpt < ncol ? t.cpt : ncol, tile_sel = tile_cols * nq;
  t.lds_digit = (size_t)tile_sel * (256 * 8 + 16) + (size_t)tile_cols * 4;
  t.lds_succ = (size_t)tile_sel * (8 + 16) + (size_t)tile_cols * 4;
  t.combine = tile_cols < 16;
  return t;
}

// the histograms: tables of nb bins per tile of the workgroup's LDS, and that LDS for n tables
inline int hist_per(size_t nb) {
  const int per = (int)((size_t)kHistBins / nb);
  return per > 1024 ? 1024 : per;  // (rows x tables of a tile are walked with a 32-bit index)
}
inline size_t hist_lds(int per, int n, size_t nb) { return (size_t)(per < n ? per : n) * nb * 8; }

// me_integrate: the scans' 2 kT Trip; with means kRealTile x kChunk weights and kSeg x kRealTile x kColTile partial sums
inline size_t integrate_lds(bool want_mean) {
  return (size_t)(2 * kT * 3 + (want_mean ? kRealTile * kChunk + kSeg * kRealTile * kColTile : 0)) * 8;
}

// realizations a set of launches carries: the batch's scratch is sized for that many
inline size_t real_tile(int nreal) { return (size_t)(nreal < kRealLaunch ? nreal : kRealLaunch); }

// expanded positions the bootstrap's buffer is carved for: before the first M' is known, and for an M' beyond that
inline size_t boot_cap_first(size_t M) { return M + M / 4 + kChunk; }
inline size_t boot_cap_regrown(size_t Mx) { return Mx + Mx / 4 + kChunk; }

// ---- layouts --------------------------------------------------------------------------------------------------------

// the walk over a layout (carve.h)
using dh_carve::Carver;
using dh_carve::Slot;

typedef unsigned long long u64;

// the merged run: dh_merged's pointer block (ctx.h), M points in merged order
struct MergedArrays {
  double *logl = nullptr, *logvol = nullptr, *logwt = nullptr, *logz = nullptr, *logzerr = nullptr, *h = nullptr;
  double *w = nullptr, *cw = nullptr, *u = nullptr, *v = nullptr;
  double* mom = nullptr;  // [sum w, sum w^2, ESS, sum w v_0 .. sum w v_{D-1}]
  int *run = nullptr, *seq = nullptr, *id = nullptr, *it = nullptr, *nc = nullptr, *n = nullptr, *fin = nullptr;
};
inline void carve_merged(Carver& c, MergedArrays& m, size_t M, size_t D, bool pt) {
  c(m.logl, "logl", M);
  c(m.logvol, "logvol", M);
  c(m.logwt, "logwt", M);
  c(m.logz, "logz", M);
  c(m.logzerr, "logzerr", M);
  c(m.h, "h", M);
  c(m.w, "w", M);
  c(m.cw, "cw", M);
  c(m.u, "u", M * D);
  c(m.v, "v", M * D);
  c(m.mom, "mom", 3 + D);
  c(m.run, "run", M);
  c(m.seq, "seq", M);
  c(m.n, "n", M);
  c(m.fin, "fin", M);
  c(m.id, "id", M, pt);
  c(m.it, "it", M, pt);
  c(m.nc, "nc", M, pt);
}

// the merge's scratch, freed when the merge returns
struct MergeScratch {
  long long *off, *nit, *src_row;
  double *seq_l, *key_b, *step, *logdvol, *eval_l, *mom_part, *last, *summ;
  int *seq_run, *org_a, *org_b, *live_slot, *flags;
  u64* ncall;
  char* part;  // a scan's chunk aggregates
};
inline void carve_scratch(Carver& c, MergeScratch& s, size_t M, size_t R, size_t N, size_t D) {
  long long chunk;
  const size_t nchunk = (size_t)moment_chunks((long long)M, D + 2, &chunk);
  c(s.off, "off", R + 1);
  c(s.nit, "nit", R);
  c(s.src_row, "src_row", M);
  c(s.seq_l, "seq_l", M);
  c(s.key_b, "key_b", M);
  c(s.step, "step", M);
  c(s.logdvol, "logdvol", M);
  c(s.eval_l, "eval_l", M);
  c(s.mom_part, "mom_part", nchunk * (D + 2));
  c(s.last, "last", 1);
  c(s.summ, "summ", 8);
  c(s.seq_run, "seq_run", M);
  c(s.org_a, "org_a", M);
  c(s.org_b, "org_b", M);
  c(s.live_slot, "live_slot", R * N);
  c(s.flags, "flags", 4);
  c(s.ncall, "ncall", 1);
  c(s.part, "part", (blocks_for(M, kChunk) + 1) * kScanElem);
}

// the inputs of dh_merge_runs, staged from the host: rows of S dead points per run (at least one)
struct MergeStage {
  double *dead_logl, *live_logl, *dead_u, *live_u;
  int *dead_id, *dead_it, *dead_nc, *live_it;  // with id / it / nc only
};
inline void carve_stage(Carver& c, MergeStage& s, size_t R, size_t N, size_t D, size_t S, bool pt) {
  c(s.dead_logl, "dead_logl", R * S);
  c(s.live_logl, "live_logl", R * N);
  c(s.dead_u, "dead_u", R * S * D);
  c(s.live_u, "live_u", R * N * D);
  c(s.dead_id, "dead_id", R * S, pt);
  c(s.dead_it, "dead_it", R * S, pt);
  c(s.dead_nc, "dead_nc", R * S, pt);
  c(s.live_it, "live_it", R * N, pt);
}

// the covariance: the chunks' sums and their total
struct CovBuf {
  double *part, *cov;
};
inline void carve_cov(Carver& c, CovBuf& b, size_t M, size_t D) {
  long long chunk;
  c(b.part, "part", (size_t)moment_chunks((long long)M, D * D, &chunk) * D * D);
  c(b.cov, "cov", D * D);
}

// dh_merged_gather: n rows out, their indices in where the caller names them
struct GatherBuf {
  long long* idx;
  double* out;
};
inline void carve_gather(Carver& c, GatherBuf& b, size_t n, size_t D, bool given) {
  c(b.idx, "idx", n, given);
  c(b.out, "out", n * D);
}

// the histograms: n tables of nbx (x nby) bins over ncol = n (1-D) or 2 n (pairs) columns
struct HistBuf {
  int* cols;
  double *xe, *ye;  // n sets of nbx + 1 (nby + 1) edges; ye with pairs only
  u64* table;
  double* out;
};
inline void carve_hist(Carver& c, HistBuf& b, bool two, size_t n, size_t nbx, size_t nby) {
  const size_t total = n * (two ? nbx * nby : nbx);
  c(b.cols, "cols", two ? 2 * n : n);
  c(b.xe, "xe", n * (nbx + 1));
  c(b.ye, "ye", n * (nby + 1), two);
  c(b.table, "table", total);
  c(b.out, "out", total);
}

// the quantiles: S = ncol x nq selections.  table | total | cmax | last | flags lie next to each other and are
// cleared by one memset of zero_bytes from `table`; the kernels initialise the rest themselves.
struct QuantBuf {
  double* q;
  int* cols;
  u64 *table, *total, *cmax;  // S x 256 bins; the sum of all W; per column slot
  unsigned* last;             // per column slot
  int* flags;
  size_t zero_bytes;
  u64 *cmin, *pk, *cb, *wk, *ti, *succ;
  double* frac;
  unsigned* pi;
  int* mode;
  double* out;
};
inline void carve_quantile(Carver& c, QuantBuf& b, size_t nq, size_t ncol) {
  const size_t S = ncol * nq;
  c(b.q, "q", nq);
  c(b.cols, "cols", ncol);
  const size_t zero = c.off;
  c(b.table, "table", S * 256);
  c(b.total, "total", 1);
  c(b.cmax, "cmax", ncol);
  c(b.last, "last", ncol);
  c(b.flags, "flags", 4);
  b.zero_bytes = c.off - zero;
  c(b.cmin, "cmin", ncol);
  c(b.pk, "pk", S);
  c(b.cb, "cb", S);
  c(b.wk, "wk", S);
  c(b.ti, "ti", S);
  c(b.succ, "succ", S);
  c(b.frac, "frac", S);
  c(b.pi, "pi", S);
  c(b.mode, "mode", S);
  c(b.out, "out", S);
}

// a batch of realizations: per point lae (and logrwt), per (realization of a launch set, chunk) the sums, per
// realization of the call its row [logz, h, ess, mean.. | kld]
struct RealBuf {
  double *lae, *rwt, *sums, *part, *mpart, *out, *kpart;
};
inline void carve_real(Carver& c, RealBuf& b, size_t M, size_t D, int nreal, bool rwt, bool want_mean, bool kld) {
  const size_t cells = real_tile(nreal) * blocks_for(M, kChunk);
  c(b.lae, "lae", M);
  c(b.rwt, "rwt", M, rwt);
  c(b.sums, "sums", cells);
  c(b.part, "part", cells * kPart);
  c(b.mpart, "mpart", cells * D, want_mean);
  c(b.out, "out", (size_t)nreal * (3 + D));
  c(b.kpart, "kpart", cells, kld);
}

// the per-point fields of one realization or bootstrap over n points
struct FieldArrays {
  double *step, *logvol, *logwt, *logz, *kld;
};
inline void carve_field_arrays(Carver& c, FieldArrays& f, size_t n, bool kld, bool wanted = true) {
  c(f.step, "step", n, wanted);
  c(f.logvol, "logvol", n, wanted);
  c(f.logwt, "logwt", n, wanted);
  c(f.logz, "logz", n, wanted);
  c(f.kld, "kld", n, wanted && kld);
}
struct FieldBuf {
  double *lae, *rwt;
  FieldArrays f;
  char* part;
};
inline void carve_fields(Carver& c, FieldBuf& b, size_t M, bool rwt, bool kld) {
  c(b.lae, "lae", M);
  c(b.rwt, "rwt", M, rwt);
  carve_field_arrays(c, b.f, M, kld);
  c(b.part, "part", (blocks_for(M, kChunk) + 1) * kScanElem);
}

// one bootstrap call, carved for `cap` expanded positions of a merged run of M points and S strands; `fields`: the
// per-point form (dh_merged_bootstrap_run), else the batch form with one row of integrals
struct BootBuf {
  size_t cap;
  int *mult, *off, *E, *src, *n;
  long long* tot;
  char* part;
  double* lae;
  double *sums, *partr, *mpart, *out, *kpart;  // batch
  FieldArrays f;                               // per-point fields
  long long* wide;
};
inline void carve_boot(Carver& c, BootBuf& b, size_t M, size_t S, size_t D, size_t cap, bool fields, bool want_mean) {
  const size_t nbx = blocks_for(cap, kChunk);
  b.cap = cap;
  c(b.mult, "mult", S);
  c(b.off, "off", M);
  c(b.E, "E", M);
  c(b.tot, "tot", 8);
  c(b.part, "part", (blocks_for(M > cap ? M : cap, kChunk) + 1) * kScanElem);
  c(b.src, "src", cap);
  c(b.n, "n", cap);
  c(b.lae, "lae", cap);
  c(b.sums, "sums", nbx, !fields);
  c(b.partr, "partr", nbx * kPart, !fields);
  c(b.mpart, "mpart", nbx * D, !fields && want_mean);
  c(b.out, "out", 3 + D, !fields);
  c(b.kpart, "kpart", nbx, !fields);
  carve_field_arrays(c, b.f, cap, true, fields);
  c(b.wide, "wide", cap, fields);
}

// the tie structure of the merged run (an allocation of its own) and the scratch of the scan that builds it
struct TieArrays {
  int *tie_idx, *tie_ep;  // [M + 1]; at most one per strand
};
inline void carve_ties(Carver& c, TieArrays& t, size_t M, size_t S) {
  c(t.tie_idx, "tie_idx", M + 1);
  c(t.tie_ep, "tie_ep", S);
}
struct TieScratch {
  char* part;
};
inline void carve_tie_scratch(Carver& c, TieScratch& t, size_t M) { c(t.part, "part", (blocks_for(M, kChunk) + 1) * kScanElem); }

// ---- the fold of dynamic batches (merge_fold.hip): a base run of M points, W new points in R strands of N live points --

// static LDS of the fold's kernels: the rank sort's tile of keys, a scan's two rows of aggregates
inline size_t fold_rank_lds() { return (size_t)kLiveTile * 8; }
inline size_t fold_scan_lds() { return (size_t)2 * kT * kScanElem; }

// the batch index of every point of a run that holds batches: an allocation of its own beside the merged block
struct BatchArrays {
  int* batch = nullptr;
};
inline void carve_batch(Carver& c, BatchArrays& b, size_t T) { c(b.batch, "batch", T); }

// the fold's scratch, freed when the fold returns (T = M + W points)
struct FoldScratch {
  long long *off, *nit, *n_row;
  double *seq_l, *key_b, *ustage, *vstage, *eval_l, *step, *vterm, *logdvol, *mom_part, *last, *summ;
  int *seq_run, *org_a, *org_b, *live_slot, *n_run, *n_seq, *n_fin, *n_id, *n_it, *n_nc;  // the W new points, in their order
  int *src, *finnew, *gstart, *shift, *idmax, *flags;
  u64* ncall;
  char* part;
};
inline void carve_fold_scratch(Carver& c, FoldScratch& s, size_t M, size_t W, size_t R, size_t N, size_t D, bool pt) {
  const size_t T = M + W;
  long long chunk;
  const size_t nchunk = (size_t)moment_chunks((long long)T, D + 2, &chunk);
  c(s.off, "off", R + 1);
  c(s.nit, "nit", R);
  c(s.n_row, "n_row", W);
  c(s.seq_l, "seq_l", W);
  c(s.key_b, "key_b", W);
  c(s.ustage, "ustage", W * D);
  c(s.vstage, "vstage", W * D);
  c(s.eval_l, "eval_l", W);
  c(s.step, "step", T);
  c(s.vterm, "vterm", T);
  c(s.logdvol, "logdvol", T);
  c(s.mom_part, "mom_part", nchunk * (D + 2));
  c(s.last, "last", 1);
  c(s.summ, "summ", 8);
  c(s.seq_run, "seq_run", W);
  c(s.org_a, "org_a", W);
  c(s.org_b, "org_b", W);
  c(s.live_slot, "live_slot", R * N);
  c(s.n_run, "n_run", W);
  c(s.n_seq, "n_seq", W);
  c(s.n_fin, "n_fin", W);
  c(s.n_id, "n_id", W, pt);
  c(s.n_it, "n_it", W, pt);
  c(s.n_nc, "n_nc", W, pt);
  c(s.src, "src", T);
  c(s.finnew, "finnew", T);
  c(s.gstart, "gstart", T);
  c(s.shift, "shift", R);
  c(s.idmax, "idmax", 1);
  c(s.flags, "flags", 4);
  c(s.ncall, "ncall", 1);
  c(s.part, "part", (blocks_for(T, kChunk) + 1) * kScanElem);
}

// the strands of dh_merged_fold, staged from the host: dh_merge_runs' shapes with strands for runs
inline void carve_fold_stage(Carver& c, MergeStage& s, size_t R, size_t N, size_t D, size_t S, bool pt) {
  carve_stage(c, s, R, N, D, S, pt);
}

// dh_merged_gather_rows: n rows of one row field out, their indices in
inline void carve_gather_rows(Carver& c, GatherBuf& b, size_t n, size_t D) { carve_gather(c, b, n, D, true); }

// the weight function: zweight and weight of every point, the maximum's bits, the bounds
struct WeightBuf {
  char* part;
  double *tot, *zw, *wt;
  u64* wmax;
  int* idx;
};
inline void carve_weights(Carver& c, WeightBuf& w, size_t M) {
  c(w.part, "part", (blocks_for(M, kChunk) + 1) * kScanElem);
  c(w.tot, "tot", 1);
  c(w.wmax, "wmax", 1);
  c(w.idx, "idx", 2);
  c(w.zw, "zw", M);
  c(w.wt, "wt", M);
}

// ---- the seeds of a dynamic batch chosen on the device (merge_seed.hip) --------------------
// Per strand the k = nlive_new largest keys logvol_i + Gumbel(seed, strand, i) over the points above logl_min: a radix
// select on the keys' order-preserving 64-bit image, 8 bits per pass from the top, the keys made again in every pass.

constexpr int kSeedStrandsMax = 65536;  // strands per call
constexpr int kSeedNliveMax = 65535;    // the resident loop's limit on nlive_new
constexpr int kSeedPairs = 4;           // Philox blocks (two neighbouring points each) per thread of a pass
constexpr int kSeedChunk = kT * kSeedPairs * 2;  // points per workgroup of a pass
constexpr int kSeedTile = 8;            // strands a workgroup carries through its chunk
constexpr int kSeedBins = 256;          // bins of a pass: 8 bits of the image
constexpr int kSeedPasses = 8;          // at most: the image has 64 bits
constexpr int kSeedCap = 2048;          // a threshold bin of at most this many keys is not narrowed further
constexpr int kSeedRankTile = 1024;     // (image, index) pairs staged in LDS per step of the final rank sort
constexpr int kSeedInfo = 12;           // info_out: prior, lo, count, n_pos, logl_min, vol_idx, start[5], passes
constexpr double kSeedLogMin = -708.0;  // a point has positive weight iff logvol - max(logvol) >= this

enum SeedVerdict : int {
  SV_OK = 0,
  SV_NO_RUN = 1,   // no merged run in the context
  SV_STRANDS = 2,  // strands < 1 or > kSeedStrandsMax
  SV_NLIVE = 3,    // nlive_new < 1 or > kSeedNliveMax
  SV_LOGL_MIN = 4, // logl_min is NaN
  SV_INFO = 5,     // info_out is NULL
  SV_FIRST = 6,    // first < 0 or first + strands beyond 2^62 (the subsequences 2^63 + 2^62 + s stay below 2^64)
};
inline const char* seed_verdict_text(int v) {
  switch (v) {
    case SV_OK: return "ok";
    case SV_NO_RUN: return "no merged run in this context";
    case SV_STRANDS: return "strands must be 1 ... 65536";
    case SV_NLIVE: return "nlive_new must be 1 ... 65535";
    case SV_LOGL_MIN: return "logl_min is NaN";
    case SV_INFO: return "info_out is required";
    case SV_FIRST: return "first must be 0 ... 2^62 - strands";
  }
  return "?";
}
// The first reason to refuse the request, in the order above (decided before the device is touched).
inline int seed_check(bool have_run, long long first, int strands, int nlive_new, double logl_min, bool have_info) {
  if (!have_run) return SV_NO_RUN;
  if (strands < 1 || strands > kSeedStrandsMax) return SV_STRANDS;
  if (nlive_new < 1 || nlive_new > kSeedNliveMax) return SV_NLIVE;
  if (logl_min != logl_min) return SV_LOGL_MIN;
  if (!have_info) return SV_INFO;
  if (first < 0 || first > (1ll << 62) - strands) return SV_FIRST;
  return SV_OK;
}

// The launch of a pass over the subset [lo, M): whole Philox blocks (block b serves points 2 b and 2 b + 1) from the
// one that holds lo, kSeedPairs per thread; a workgroup carries kSeedTile strands through its chunk.
struct SeedGrid {
  long long pair0, npairs;
  unsigned chunks, tiles;
};
inline SeedGrid seed_grid(long long lo, long long M, int strands) {
  SeedGrid g;
  g.pair0 = lo >> 1;
  g.npairs = ((M + 1) >> 1) - g.pair0;
  g.chunks = blocks_for((size_t)g.npairs, (size_t)kT * kSeedPairs);
  g.tiles = blocks_for((size_t)strands, kSeedTile);
  return g;
}
// (image, index) pairs a strand's collect pass can emit: everything above the threshold bin (fewer than k) and that
// bin (at most kSeedCap, or exactly what is still needed), never more than the points of positive weight
inline size_t seed_ecap(int k, long long n_pos) {
  const long long e = (long long)k + kSeedCap;
  return (size_t)(e < n_pos ? e : n_pos);
}
inline size_t seed_pass_lds() { return (size_t)2 * kSeedBins * 4; }
inline size_t seed_rank_lds() { return (size_t)kSeedRankTile * (8 + 4); }

// a strand's state between the passes
struct SeedState {
  u64 prefix;  // the image's bits decided so far
  int need;    // keys still to take from the threshold bin
  int shift;   // where the next pass's digit starts (56 in the first pass, -8 when all 64 bits are decided)
  int active;  // 0: the threshold bin is small enough (or exact)
  unsigned pop;  // the threshold bin's population
};

// the head of a call: what the bounds, the maximum and the count leave for the host
struct SeedHead {
  double* info;  // kSeedInfo
  long long* li; // lo, count
  u64 *maxbits, *npos;
  int *flags, *nactive;
};
inline void carve_seed_head(Carver& c, SeedHead& h) {
  c(h.info, "info", kSeedInfo);
  c(h.li, "li", 2);
  c(h.maxbits, "maxbits", 1);
  c(h.npos, "npos", 1);
  c(h.flags, "flags", 4);
  c(h.nactive, "nactive", 1);
}
// the select's scratch: S strands, k seeds each, ecap pairs per strand
struct SeedSelBuf {
  unsigned *bins, *cnt;
  SeedState* st;
  u64* pimg;
  int* pidx;
  long long* idx;
  double* key;
};
inline void carve_seed_select(Carver& c, SeedSelBuf& b, size_t S, size_t k, size_t ecap) {
  c(b.bins, "bins", S * kSeedBins);
  c(b.cnt, "cnt", S);
  c(b.st, "st", S);
  c(b.pimg, "pimg", S * ecap);
  c(b.pidx, "pidx", S * ecap);
  c(b.idx, "idx", S * k);
  c(b.key, "key", S * k);
}
// the gathered rows: the chosen points' unit-cube rows and ln L, strand after strand in draw order
struct SeedStage {
  double *u = nullptr, *logl = nullptr;
};
inline void carve_seed_stage(Carver& c, SeedStage& s, size_t S, size_t k, size_t D) {
  c(s.u, "u", S * k * D);
  c(s.logl, "logl", S * k);
}

}  // namespace dh_merge
