// dh_ns_batch, what is decided before the device is touched: which requests the entry point refuses, and the sizes of
// the seeding phase (fills, staging arrays).  Plain C++17 on the host: ns.hip includes it, and so does a stand-alone
// program that the tests build with the sanitizers (tests/host/ns_batch_plan_dump.cpp).
//
// A dynamic batch is R strands of nlive_new live points, each started inside (logl_min, logl_max] of a finished run
// from nlive_new of that run's points (the seeds).  Refused here, all with DH_ERR_ARG: the Philox samplers (a strand's
// fills are not the ensemble's, so their offsets would not be reproducible), the friends bounds, a kept batch
// (dh_ns_keep), a non-finite logl_min (a batch from the prior is an ordinary dh_ns_ensemble with logl_max), a seed at or
// below logl_min, nlive_new below the loop's own 4 or beyond its 16-bit slots, and logl_max <= logl_min.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace dh_nsb {

enum Verdict : int {
  V_OK = 0,
  V_SHAPE = 1,      // runs / ndim / queue_size < 1, or a required array missing
  V_NLIVE = 2,      // nlive_new < kMinNlive or > kMaxNlive
  V_SAMPLER = 3,    // not one of rwalk 0, rslice 1, slice 2, unif 6 (the Philox codes 3, 4, 5, 7 among them)
  V_BOUND = 4,      // not single 0 / multi 1 (the friends bounds 2, 3 among them)
  V_KEEP = 5,       // dh_ns_keep is armed
  V_LOGL_MIN = 6,   // logl_min is not finite
  V_LOGL_MAX = 7,   // logl_max <= logl_min (or NaN)
  V_SEED = 8,       // a seed's ln L is not above logl_min
  V_START = 9,      // a start row that is not finite, or a scale <= 0
};

constexpr int kMinNlive = 4;      // the loop's own limits (ns_plan): at least four live points,
constexpr int kMaxNlive = 65535;  // and live slots travel as 16-bit indices

struct Request {
  int runs, nlive_new, ndim, queue_size, sampler, bound, keep;
  double logl_min, logl_max;  // logl_max = +inf: none
  const double* seed_u;       // runs x nlive_new x ndim
  const double* seed_logl;    // runs x nlive_new
  const double* start;        // runs x 6: logvol, logz, h, logzvar, last dead ln L, scale
};

struct Sizes {
  int seed_fills;        // ceil(nlive_new / queue_size): the seed fills; they fill the staging set unless a slice fails
  size_t stage_points;   // runs x nlive_new: rows of the staging live set (u and v: x ndim doubles each)
  size_t stage_bytes;    // the staging arrays and the per-run seeding counters together (each array 256-byte aligned)
};

inline const char* verdict_text(int v) {
  switch (v) {
    case V_OK: return "ok";
    case V_SHAPE: return "runs, ndim, queue_size >= 1 and seed_u, seed_logl, start are required";
    case V_NLIVE: return "nlive_new must be 4 ... 65535 (the resident loop's own limits)";
    case V_SAMPLER: return "sampler must be 0 rwalk, 1 rslice, 2 slice or 6 unif (PCG64 streams; no Philox strands)";
    case V_BOUND: return "bound must be 0 single or 1 multi (no friends bounds)";
    case V_KEEP: return "a batch ensemble cannot be kept (dh_ns_keep)";
    case V_LOGL_MIN: return "logl_min must be finite (a batch from the prior is dh_ns_ensemble with logl_max)";
    case V_LOGL_MAX: return "logl_max must be above logl_min";
    case V_SEED: return "every seed's ln L must be above logl_min";
    case V_START: return "start rows must be finite with a scale > 0";
  }
  return "?";
}

// The first reason to refuse the request, in the order above; *where: the flat index of the offending seed / start
// value (V_SEED, V_START), -1 otherwise.
inline int check(const Request& q, long long* where = nullptr) {
  if (where) *where = -1;
  if (q.runs < 1 || q.ndim < 1 || q.queue_size < 1 || !q.seed_u || !q.seed_logl || !q.start) return V_SHAPE;
  if (q.nlive_new < kMinNlive || q.nlive_new > kMaxNlive) return V_NLIVE;
  if (q.sampler != 0 && q.sampler != 1 && q.sampler != 2 && q.sampler != 6) return V_SAMPLER;
  if (q.bound != 0 && q.bound != 1) return V_BOUND;
  if (q.keep) return V_KEEP;
  if (!std::isfinite(q.logl_min)) return V_LOGL_MIN;
  if (!(q.logl_max > q.logl_min)) return V_LOGL_MAX;
  const size_t n = (size_t)q.runs * (size_t)q.nlive_new;
  for (size_t i = 0; i < n; ++i)
    if (!(q.seed_logl[i] > q.logl_min)) {  // (NaN included)
      if (where) *where = (long long)i;
      return V_SEED;
    }
  for (size_t i = 0; i < (size_t)q.runs * 6; ++i) {
    const double x = q.start[i];
    // logz of a base that has integrated nothing yet is the loop's own -1e300: finite
    if (!std::isfinite(x) || (i % 6 == 5 && !(x > 0.0))) {
      if (where) *where = (long long)i;
      return V_START;
    }
  }
  return V_OK;
}

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

inline Sizes sizes(int runs, int nlive_new, int ndim, int queue_size) {
  Sizes s;
  s.seed_fills = (nlive_new + queue_size - 1) / queue_size;
  s.stage_points = (size_t)runs * (size_t)nlive_new;
  const size_t R = (size_t)runs, P = s.stage_points, D = (size_t)ndim;
  s.stage_bytes = 2 * pad256(P * D * 8)      // u, v
                  + pad256(P * 8)            // ln L
                  + pad256(P * 4)            // nc
                  + pad256(R * 4)            // rows filled
                  + 2 * pad256(R * 8)        // calls of the rejected entries since the last row; calls of the phase
                  + pad256(R * 32)           // the generator at the hand-over
                  + pad256(R * 6 * 8);       // the start rows
  return s;
}

}  // namespace dh_nsb
