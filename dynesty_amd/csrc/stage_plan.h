// Internal: where the host-pointer entry points outside the combiner stage their arrays in the context's arena
// (walk.hip, walk2.hip, friends.hip, rebuild.hip, boot.hip, bound.hip, dh_ns_consume of ns.hip), as plain host
// arithmetic.
//
// One layout per entry point: a struct of its staged device pointers and THE list of those arrays -- element type,
// element count, wanted or not --, in the order the call has always taken them, walked twice by a Carver (carve.h;
// arena_carve of ctx.h).  An array that is not wanted takes no room and is a null pointer.  A workspace whose size
// another unit owns enters as a byte count, a record whose type another unit owns as its size.  Nothing here touches
// the device, so a host program holds it to its invariants (tests/test_stage_plan_cpu.py).  Plain C++17: no HIP include.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "carve.h"

namespace dh_stage {

using dh_carve::Carver;

// ---- walk.hip -------------------------------------------------------------------------------------------------------

// dh_rwalk_propose: k walkers, m frames of ncdim x ncdim
struct RwalkProposeBuf {
  double *u0, *axes;
  int32_t* axes_idx;
  int8_t* bc;
  uint64_t* rng;
  double* u;
  int32_t* inside;
  uint64_t* rng_out;
};
inline void carve_rwalk_propose(Carver& c, RwalkProposeBuf& b, size_t k, size_t ndim, size_t ncdim, size_t m, bool idx,
                                bool bc) {
  c(b.u0, "u0", k * ndim);
  c(b.axes, "axes", m * ncdim * ncdim);
  c(b.axes_idx, "axes_idx", k, idx);
  c(b.bc, "bc", ndim, bc);
  c(b.rng, "rng", k * 4);
  c(b.u, "u", k * ndim);
  c(b.inside, "inside", k);
  c(b.rng_out, "rng_out", k * 4);
}

// dh_rwalk_batch / dh_rwalk_batch_philox: the generator states travel with PCG64 streams only
struct RwalkBatchBuf {
  double *u0, *axes;
  int32_t* axes_idx;
  int8_t* bc;
  uint64_t* rng;
  double *u, *v, *logl;
  int32_t *naccept, *nreject;
  uint64_t* rng_out;
};
inline void carve_rwalk_batch(Carver& c, RwalkBatchBuf& b, size_t k, size_t ndim, size_t ncdim, size_t m, bool idx,
                              bool bc, bool philox) {
  c(b.u0, "u0", k * ndim);
  c(b.axes, "axes", m * ncdim * ncdim);
  c(b.axes_idx, "axes_idx", k, idx);
  c(b.bc, "bc", ndim, bc);
  c(b.rng, "rng", k * 4, !philox);
  c(b.u, "u", k * ndim);
  c(b.v, "v", k * ndim);
  c(b.logl, "logl", k);
  c(b.naccept, "naccept", k);
  c(b.nreject, "nreject", k);
  c(b.rng_out, "rng_out", k * 4, !philox);
}

// dh_problem_eval
struct EvalBuf {
  double *u, *v, *logl;
};
inline void carve_eval(Carver& c, EvalBuf& b, size_t k, size_t ndim) {
  c(b.u, "u", k * ndim);
  c(b.v, "v", k * ndim);
  c(b.logl, "logl", k);
}

// dh_seed_children: n_words entropy words in, k states of 4 words out
struct SeedChildrenBuf {
  uint32_t* entropy;
  uint64_t* states;
};
inline void carve_seed_children(Carver& c, SeedChildrenBuf& b, size_t k, size_t n_words) {
  c(b.entropy, "entropy", n_words);
  c(b.states, "states", k * 4);
}

// dh_rng_stream: one more than asked of each kind, so that neither array is empty
struct RngStreamBuf {
  uint64_t* state;
  double *normals, *unifs;
  uint64_t* state_out;
};
inline void carve_rng_stream(Carver& c, RngStreamBuf& b, size_t n_normal, size_t n_unif) {
  c(b.state, "state", 4);
  c(b.normals, "normals", n_normal + 1);
  c(b.unifs, "unifs", n_unif + 1);
  c(b.state_out, "state_out", 4);
}

// ---- walk2.hip ------------------------------------------------------------------------------------------------------

// dh_slice_batch / dh_slice_batch_philox: m frames of ndim x ndim
struct SliceBatchBuf {
  double *u0, *axes;
  int32_t* axes_idx;
  uint64_t* rng;
  double *u, *v, *logl;
  int32_t *ncalls, *nexpand, *ncontract, *flags;
  uint64_t* rng_out;
};
inline void carve_slice_batch(Carver& c, SliceBatchBuf& b, size_t k, size_t ndim, size_t m, bool idx, bool philox) {
  c(b.u0, "u0", k * ndim);
  c(b.axes, "axes", m * ndim * ndim);
  c(b.axes_idx, "axes_idx", k, idx);
  c(b.rng, "rng", k * 4, !philox);
  c(b.u, "u", k * ndim);
  c(b.v, "v", k * ndim);
  c(b.logl, "logl", k);
  c(b.ncalls, "ncalls", k);
  c(b.nexpand, "nexpand", k);
  c(b.ncontract, "ncontract", k);
  c(b.flags, "flags", k);
  c(b.rng_out, "rng_out", k * 4);
}

// dh_unif_batch / dh_unif_batch_philox: m ellipsoids (0: the unit cube; ams and cumprob from two on)
struct UnifBatchBuf {
  double *ctrs, *axes, *ams, *cumprob;
  int8_t* bc;
  uint64_t* rng;
  double *u, *v, *logl;
  int32_t *ncalls, *flags;
  uint64_t* rng_out;
};
inline void carve_unif_batch(Carver& c, UnifBatchBuf& b, size_t k, size_t ndim, size_t ncdim, size_t m, bool bc,
                             bool philox) {
  c(b.ctrs, "ctrs", m * ncdim, m > 0);
  c(b.axes, "axes", m * ncdim * ncdim, m > 0);
  c(b.ams, "ams", m * ncdim * ncdim, m > 1);
  c(b.cumprob, "cumprob", m, m > 1);
  c(b.bc, "bc", ndim, bc);
  c(b.rng, "rng", k * 4, !philox);
  c(b.u, "u", k * ndim);
  c(b.v, "v", k * ndim);
  c(b.logl, "logl", k);
  c(b.ncalls, "ncalls", k);
  c(b.flags, "flags", k);
  c(b.rng_out, "rng_out", k * 4);
}

// dh_unif_friends_batch: n centres and their whitened copies, one shape
struct UnifFriendsBuf {
  double *ctrs, *axes, *axes_inv, *ct;
  int8_t* bc;
  uint64_t* rng;
  double *u, *v, *logl;
  int32_t *ncalls, *flags;
  uint64_t *rng_out, *rng32, *rng32_out;
};
inline void carve_unif_friends(Carver& c, UnifFriendsBuf& b, size_t k, size_t ndim, size_t n, bool bc, bool rng32,
                               bool rng32_out) {
  c(b.ctrs, "ctrs", n * ndim);
  c(b.axes, "axes", ndim * ndim);
  c(b.axes_inv, "axes_inv", ndim * ndim);
  c(b.ct, "ct", n * ndim);
  c(b.bc, "bc", ndim, bc);
  c(b.rng, "rng", k * 4);
  c(b.u, "u", k * ndim);
  c(b.v, "v", k * ndim);
  c(b.logl, "logl", k);
  c(b.ncalls, "ncalls", k);
  c(b.flags, "flags", k);
  c(b.rng_out, "rng_out", k * 4);
  c(b.rng32, "rng32", k * 2, rng32);
  c(b.rng32_out, "rng32_out", k * 2, rng32_out);
}

// dh_bound_draw: nsamp draws from m ellipsoids of dimension d
struct BoundDrawBuf {
  uint64_t* state;
  double *ctrs, *axes, *ams, *cumprob, *x;
  int32_t *idx, *q, *status;
  uint64_t* state_out;
  double* work;
};
inline void carve_bound_draw(Carver& c, BoundDrawBuf& b, size_t nsamp, size_t d, size_t m) {
  c(b.state, "state", 4);
  c(b.ctrs, "ctrs", m * d);
  c(b.axes, "axes", m * d * d);
  c(b.ams, "ams", m * d * d, m > 1);
  c(b.cumprob, "cumprob", m, m > 1);
  c(b.x, "x", nsamp * d);
  c(b.idx, "idx", nsamp);
  c(b.q, "q", nsamp);
  c(b.status, "status", 1);
  c(b.state_out, "state_out", 4);
  c(b.work, "work", 2 * d);
}

// dh_slice_feed: kind 0 directions from m frames, kind 1 permutations, kind 2 the lookahead alone
struct SliceFeedBuf {
  double* axes;
  int32_t* axes_idx;
  uint64_t* st6;
  int32_t* consumed;
  double* dirs;
  int32_t* perm;
  double* look;
};
inline void carve_slice_feed(Carver& c, SliceFeedBuf& b, size_t k, size_t ndim, int kind, size_t m, size_t nlook,
                             bool idx, bool consumed) {
  c(b.axes, "axes", m * ndim * ndim, kind == 0);
  c(b.axes_idx, "axes_idx", k, kind == 0 && idx);
  c(b.st6, "st6", k * 6);
  c(b.consumed, "consumed", k, consumed);
  c(b.dirs, "dirs", k * ndim, kind == 0);
  c(b.perm, "perm", k * ndim, kind == 1);
  c(b.look, "look", k * nlook, nlook > 0);
}

// ---- friends.hip ----------------------------------------------------------------------------------------------------

inline size_t friends_words(size_t n) { return (n + 63) / 64; }  // 64-bit words of a row of the adjacency
inline size_t friends_reps(size_t nboot) { return nboot > 0 ? nboot : 1; }

// dh_friends_update: n points of dimension d; mv holds the cluster means, then the recentred points
struct FriendsUpdateBuf {
  double *x, *y, *mv, *prev;
  unsigned long long* bits;
  int *label, *nc;
  double *mean, *cov, *am, *axes, *axes_inv, *info;
  int* status;
  unsigned char* mask;
  double *nn, *r;
};
inline void carve_friends_update(Carver& c, FriendsUpdateBuf& b, size_t n, size_t d, size_t nboot, bool am_prev) {
  c(b.x, "x", n * d);
  c(b.y, "y", n * d);
  c(b.mv, "mv", n * d);
  c(b.prev, "prev", d * d, am_prev);
  c(b.bits, "bits", n * friends_words(n));
  c(b.label, "label", n);
  c(b.nc, "nc", 2);
  c(b.mean, "mean", d);
  c(b.cov, "cov", d * d);
  c(b.am, "am", d * d);
  c(b.axes, "axes", d * d);
  c(b.axes_inv, "axes_inv", d * d);
  c(b.info, "info", 4);
  c(b.status, "status", 2);
  c(b.mask, "mask", nboot * n, nboot > 0);
  c(b.nn, "nn", friends_reps(nboot) * n);
  c(b.r, "r", 1);
}

// dh_friends_update_batch: R runs; ws of friends_batch_ws_bytes (friends.hip)
struct FriendsBatchBuf {
  double *x, *prev;
  unsigned char* mask;
  int* active;
  double *cov, *am, *axes, *axes_inv, *logvol, *rmax;
  int *nclusters, *status;
  char* ws;
};
inline void carve_friends_batch(Carver& c, FriendsBatchBuf& b, size_t R, size_t n, size_t d, size_t nboot,
                                size_t ws_bytes, bool am_prev, bool active) {
  c(b.x, "x", R * n * d);
  c(b.prev, "prev", R * d * d, am_prev);
  c(b.mask, "mask", R * nboot * n, nboot > 0);
  c(b.active, "active", R, active);
  c(b.cov, "cov", R * d * d);
  c(b.am, "am", R * d * d);
  c(b.axes, "axes", R * d * d);
  c(b.axes_inv, "axes_inv", R * d * d);
  c(b.logvol, "logvol", R);
  c(b.rmax, "rmax", R);
  c(b.nclusters, "nclusters", R);
  c(b.status, "status", R);
  c(b.ws, "ws", ws_bytes);
}

// dh_friends_within: m candidates against n centres
struct FriendsWithinBuf {
  double *ctrs, *x, *axes_inv, *ct, *xt;
  int* counts;
  unsigned long long* bits;
};
inline void carve_friends_within(Carver& c, FriendsWithinBuf& b, size_t n, size_t d, size_t m, bool bits) {
  c(b.ctrs, "ctrs", n * d);
  c(b.x, "x", m * d);
  c(b.axes_inv, "axes_inv", d * d);
  c(b.ct, "ct", n * d);
  c(b.xt, "xt", m * d);
  c(b.counts, "counts", m);
  c(b.bits, "bits", m * friends_words(n), bits);
}

// dh_friends_draw: nsamp draws from n centres; the states are 6 words
struct FriendsDrawBuf {
  uint64_t* state;
  double *ctrs, *axes, *axes_inv, *ct, *x;
  int32_t* q;
  uint64_t* state_out;
};
inline void carve_friends_draw(Carver& c, FriendsDrawBuf& b, size_t nsamp, size_t n, size_t d) {
  c(b.state, "state", 6);
  c(b.ctrs, "ctrs", n * d);
  c(b.axes, "axes", d * d);
  c(b.axes_inv, "axes_inv", d * d);
  c(b.ct, "ct", n * d);
  c(b.x, "x", nsamp * d);
  c(b.q, "q", nsamp);
  c(b.state_out, "state_out", 6);
}

// ---- rebuild.hip ----------------------------------------------------------------------------------------------------

// dh_rebuild: n points, room for max_ells ellipsoids
struct RebuildBuf {
  double* pts;
  int32_t *nells, *status, *nnodes;
  double *ctrs, *covs, *ams, *axes, *axlens, *logvols;
  int32_t* leaf_of_point;
};
inline void carve_rebuild(Carver& c, RebuildBuf& b, size_t n, size_t d, size_t max_ells, bool leaf) {
  c(b.pts, "pts", n * d);
  c(b.nells, "nells", 1);
  c(b.status, "status", 1);
  c(b.nnodes, "nnodes", 1);
  c(b.ctrs, "ctrs", max_ells * d);
  c(b.covs, "covs", max_ells * d * d);
  c(b.ams, "ams", max_ells * d * d);
  c(b.axes, "axes", max_ells * d * d);
  c(b.axlens, "axlens", max_ells * d);
  c(b.logvols, "logvols", max_ells);
  c(b.leaf_of_point, "leaf_of_point", n, leaf);
}

// dh_ell_from_cov: m covariances
struct EllFromCovBuf {
  double *covs, *axes, *ams, *axlens, *logvols;
  int* status;
};
inline void carve_ell_from_cov(Carver& c, EllFromCovBuf& b, size_t m, size_t d) {
  c(b.covs, "covs", m * d * d);
  c(b.axes, "axes", m * d * d);
  c(b.ams, "ams", m * d * d);
  c(b.axlens, "axlens", m * d);
  c(b.logvols, "logvols", m);
  c(b.status, "status", m);
}

// dh_improve_covar_mat: the input padded to rows of d | 1
struct ImproveCovBuf {
  double *padded, *covs, *ams, *axes;
  int* good;
};
inline void carve_improve_cov(Carver& c, ImproveCovBuf& b, size_t m, size_t d) {
  c(b.padded, "padded", m * d * (d | 1));
  c(b.covs, "covs", m * d * d);
  c(b.ams, "ams", m * d * d);
  c(b.axes, "axes", m * d * d);
  c(b.good, "good", m);
}

// dh_scale_to_logvol: m ellipsoids scaled in place
struct ScaleLogvolBuf {
  double *covs, *ams, *axes, *axlens, *logvols, *targets;
};
inline void carve_scale_logvol(Carver& c, ScaleLogvolBuf& b, size_t m, size_t d) {
  c(b.covs, "covs", m * d * d);
  c(b.ams, "ams", m * d * d);
  c(b.axes, "axes", m * d * d);
  c(b.axlens, "axlens", m * d);
  c(b.logvols, "logvols", m);
  c(b.targets, "targets", m);
}

// dh_enlarge_runs: runs bounds of max_ells slots each, scaled in place; the run mask and the per-run shift are optional
struct EnlargeRunsBuf {
  double *covs, *ams, *axes, *axlens, *logvols;
  int32_t *nells, *active;
  double* run_shift;
};
inline void carve_enlarge_runs(Carver& c, EnlargeRunsBuf& b, size_t runs, size_t max_ells, size_t d, bool active,
                               bool run_shift) {
  const size_t m = runs * max_ells;
  c(b.covs, "covs", m * d * d);
  c(b.ams, "ams", m * d * d);
  c(b.axes, "axes", m * d * d);
  c(b.axlens, "axlens", m * d);
  c(b.logvols, "logvols", m);
  c(b.nells, "nells", runs);
  c(b.active, "active", runs, active);
  c(b.run_shift, "run_shift", runs, run_shift);
}

// ---- boot.hip -------------------------------------------------------------------------------------------------------

// dh_bootstrap_expand: ws of bootstrap_ws_bytes (boot.hip)
struct BootExpandBuf {
  double* pts;
  uint64_t* ent;
  char* ws;
  double *shift, *expand;
  int* bstatus;
};
inline void carve_boot_expand(Carver& c, BootExpandBuf& b, size_t runs, size_t n, size_t d, size_t ws_bytes) {
  c(b.pts, "pts", runs * n * d);
  c(b.ent, "ent", runs * 4);
  c(b.ws, "ws", ws_bytes);
  c(b.shift, "shift", runs);
  c(b.expand, "expand", runs);
  c(b.bstatus, "bstatus", runs);
}

// ---- bound.hip ------------------------------------------------------------------------------------------------------

// dh_contains: k candidates against m ellipsoids; the mask is one bit per candidate and ellipsoid
struct ContainsBuf {
  double *x, *ctrs, *ams;
  int32_t* count;
  uint64_t* mask;
  double* quad;
};
inline void carve_contains(Carver& c, ContainsBuf& b, size_t k, size_t d, size_t m, bool mask, bool quad) {
  c(b.x, "x", k * d);
  c(b.ctrs, "ctrs", m * d);
  c(b.ams, "ams", m * d * d);
  c(b.count, "count", k);
  c(b.mask, "mask", (k + 63) / 64 * m, mask);
  c(b.quad, "quad", k * m, quad);
}

// dh_contains_runs: runs queues of wpr candidates, each against its own run's max_ells slots; flag and first go up and
// come back
struct ContainsRunsBuf {
  double *x, *ctrs, *ams;
  int32_t *nells, *run_mode, *bstatus, *flag, *first;
};
inline void carve_contains_runs(Carver& c, ContainsRunsBuf& b, size_t runs, size_t wpr, size_t d, size_t max_ells,
                                bool nells, bool run_mode, bool bstatus, bool first) {
  c(b.x, "x", runs * wpr * d);
  c(b.ctrs, "ctrs", runs * max_ells * d);
  c(b.ams, "ams", runs * max_ells * d * d);
  c(b.nells, "nells", runs, nells);
  c(b.run_mode, "run_mode", runs, run_mode);
  c(b.bstatus, "bstatus", runs, bstatus);
  c(b.flag, "flag", runs);
  c(b.first, "first", runs, first);
}

// ---- ns.hip ---------------------------------------------------------------------------------------------------------

// dh_ns_consume: R runs of N live points and a queue of K; run_bytes = sizeof(NsRun); the per-point arrays come together
struct NsConsumeBuf {
  char* st;
  double *live_logl, *dead_logl, *r_logl;
  int *r_a, *trace_slot, *trace_src, *trace_n, *ndone, *bstatus;
  int *live_it, *dead_id, *dead_it, *dead_nc;
};
constexpr size_t kNsDoneInts = 16;  // the counters cleared ahead of the launch
inline void carve_ns_consume(Carver& c, NsConsumeBuf& b, size_t R, size_t N, size_t K, size_t run_bytes, bool pt) {
  c(b.st, "st", R * run_bytes);
  c(b.live_logl, "live_logl", R * N);
  c(b.dead_logl, "dead_logl", R * K);
  c(b.r_logl, "r_logl", R * K);
  c(b.r_a, "r_a", R * K);
  c(b.trace_slot, "trace_slot", R * K);
  c(b.trace_src, "trace_src", R * K);
  c(b.trace_n, "trace_n", R * 2);
  c(b.ndone, "ndone", kNsDoneInts);
  c(b.bstatus, "bstatus", R);
  c(b.live_it, "live_it", R * N, pt);
  c(b.dead_id, "dead_id", R * K, pt);
  c(b.dead_it, "dead_it", R * K, pt);
  c(b.dead_nc, "dead_nc", R * K, pt);
}

}  // namespace dh_stage
