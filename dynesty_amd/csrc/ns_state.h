// The resident loop's state between two calls (ns.hip: dh_ns_continue, dh_ns_state_export / _import): the stop rule
// a continuation evaluates before its first fill, and the format of a saved ensemble.  Plain C++17, host and device:
// the kernel (ns_resume) and the entry points use it, tests/host/ns_state_dump.cpp includes it alone.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#define DH_NS_HD __host__ __device__
#else
#define DH_NS_HD
#endif

namespace dh_ns_state {

// ---- the stop rule: the reference's tests at the top of the loop (sampler.py:1071-1100) on a run's state ---------
// What a run holds after its last death: ln X, ln Z, the largest ln L ever inserted (the live set's maximum), the
// worst live ln L, the last dead point's ln L, the loop counter (deaths so far) and the calls (initial points included).
struct StopState {
  double logvol, logz, lmax, loglstar, dead_prev;
  long long it, ncall;
};
// run_nested's criteria; maxiter / maxcall < 0: none, logl_max = +inf: none.  maxiter and maxcall are TOTALS of the run.
struct StopRule {
  double dlogz, logl_max;
  long long maxiter, maxcall;
};

// np.logaddexp(0, v), term for term as ns_consume's stop scan evaluates it (so that a continuation with unchanged
// criteria finds every stopped run stopped)
DH_NS_HD inline double logaddexp0(double v) {
  if (v == 0.0) return 0.6931471805599453;
  const double d = 0.0 - v;
  if (d > 0) return 0.0 + log1p(exp(-d));
  if (d <= 0) return v + log1p(exp(d));
  return 0.0 + v;
}
DH_NS_HD inline double delta_logz(const StopState& s) { return logaddexp0(s.lmax + s.logvol - s.logz); }

enum : int { STOP_DLOGZ = 1, STOP_LOGL_MAX = 2, STOP_MAXITER = 4, STOP_MAXCALL = 8, STOP_PLATEAU = 16 };
// the tests that hold, as a mask (0: the run goes on).  The comparisons are the reference's: all strict but the
// plateau's, which is np.ptp(live_logl) == 0 -- the worst live value has reached the largest.
DH_NS_HD inline int stop_mask(const StopState& s, const StopRule& c) {
  int m = 0;
  if (delta_logz(s) < c.dlogz) m |= STOP_DLOGZ;
  if (s.dead_prev > c.logl_max) m |= STOP_LOGL_MAX;
  if (c.maxiter >= 0 && s.it > c.maxiter) m |= STOP_MAXITER;
  if (c.maxcall >= 0 && s.ncall > c.maxcall) m |= STOP_MAXCALL;
  if (s.loglstar >= s.lmax) m |= STOP_PLATEAU;
  return m;
}

// ---- the image of a kept ensemble ---------------------------------------------------------------------------------
//   Header | plan (plan_bytes: the first call's arguments and resolved plan values, opaque here)
//          | rows (runs x int64: dead points of each run) | the state arrays in the order of ns_arrays, every array
//            padded to 8 bytes; the dead-point arrays hold rows[r] rows per run, so the size does not depend on the capacity
constexpr uint64_t kMagic = 0x31305453534e4844ull;  // "DHNSST01", little endian

struct Header {
  uint64_t magic;
  uint32_t version;      // DH_VERSION of the library that wrote the image
  uint32_t sizeof_run;   // sizeof(NsRun)
  uint32_t header_bytes; // sizeof(Header)
  uint32_t plan_bytes;
  int32_t runs, nlive, ndim, queue_size;
  int64_t cap;           // dead-point capacity per run when saved
  int64_t fill;          // the ensemble's fill counter
  int32_t cube_phase;    // the host still launches the unit-cube kernel
  int32_t n_words;       // entropy words
  int32_t have_bc;       // boundary flags were installed
  int32_t row_bytes;     // bytes one dead point takes over all dead-point arrays
  uint64_t fixed_bytes;  // the arrays that do not grow with the run, padded
  uint64_t total_bytes;  // the whole image
};

DH_NS_HD inline uint64_t pad8(uint64_t n) { return (n + 7) & ~(uint64_t)7; }

// bytes of one run's share of a dead-point array of `elem` bytes per row, as the image stores it
DH_NS_HD inline uint64_t rows_bytes(int64_t rows, uint64_t elem) { return pad8((uint64_t)rows * elem); }

// The image's size as a function of the header's plan values and the runs' row counts.  n_dead / elems: the
// dead-point arrays present and their bytes per row (their sum is row_bytes up to padding).
inline uint64_t image_bytes(const Header& h, const int64_t* rows, int n_dead, const uint32_t* elems) {
  uint64_t n = (uint64_t)h.header_bytes + pad8(h.plan_bytes) + (uint64_t)h.runs * 8 + h.fixed_bytes;
  for (int k = 0; k < n_dead; ++k)
    for (int r = 0; r < h.runs; ++r) n += rows_bytes(rows[r], elems[k]);
  return n;
}

enum : int {
  IMG_OK = 0,
  IMG_SHORT_HEADER,  // fewer bytes than a header
  IMG_MAGIC,
  IMG_VERSION,
  IMG_RUN_SIZE,      // sizeof(NsRun) differs
  IMG_PLAN_SIZE,
  IMG_SHAPE,         // a shape field out of range
  IMG_TRUNCATED,     // fewer bytes than the header promises
  IMG_ROWS,          // a run's row count below zero or above the saved capacity
  IMG_CAPACITY,      // max_iter below a run's rows
  IMG_NDIM           // the problem's ndim differs
};

inline const char* reject_text(int code) {
  switch (code) {
    case IMG_OK: return "ok";
    case IMG_SHORT_HEADER: return "buffer shorter than the header";
    case IMG_MAGIC: return "bad magic";
    case IMG_VERSION: return "written by another library version";
    case IMG_RUN_SIZE: return "sizeof(NsRun) differs";
    case IMG_PLAN_SIZE: return "the plan's size differs";
    case IMG_SHAPE: return "a shape field is out of range";
    case IMG_TRUNCATED: return "truncated buffer";
    case IMG_ROWS: return "a run's row count exceeds the saved capacity";
    case IMG_CAPACITY: return "max_iter below a run's niter";
    case IMG_NDIM: return "the problem's ndim differs";
  }
  return "?";
}

// Everything that can be said about an image without the device: buf / bytes as given by the caller; version,
// sizeof_run, plan_bytes: the reading library's; ndim: the problem's; max_iter: 0 = as saved.  On IMG_OK *out is the
// header, *rows_out points at the row counts inside buf and *cap_out is the capacity the import allocates.
inline int validate(const void* buf, uint64_t bytes, uint32_t version, uint32_t sizeof_run, uint32_t plan_bytes, int ndim,
                    int64_t max_iter, Header* out, const int64_t** rows_out, int64_t* cap_out) {
  if (!buf || bytes < sizeof(Header)) return IMG_SHORT_HEADER;
  Header h;
  memcpy(&h, buf, sizeof h);
  if (h.magic != kMagic) return IMG_MAGIC;
  if (h.version != version) return IMG_VERSION;
  if (h.sizeof_run != sizeof_run) return IMG_RUN_SIZE;
  if (h.header_bytes != sizeof(Header) || h.plan_bytes != plan_bytes) return IMG_PLAN_SIZE;
  if (h.runs < 1 || h.nlive < 1 || h.ndim < 1 || h.queue_size < 1 || h.cap < 1 || h.fill < 0 || h.n_words < 1 ||
      h.row_bytes < 8)
    return IMG_SHAPE;
  const uint64_t head = (uint64_t)h.header_bytes + pad8(h.plan_bytes) + (uint64_t)h.runs * 8;
  if (bytes < head || bytes < h.total_bytes || h.total_bytes < head + h.fixed_bytes) return IMG_TRUNCATED;
  const int64_t* rows = (const int64_t*)((const char*)buf + h.header_bytes + pad8(h.plan_bytes));
  const int64_t cap = max_iter > 0 ? max_iter : h.cap;
  uint64_t least = head + h.fixed_bytes;
  for (int r = 0; r < h.runs; ++r) {
    int64_t n;
    memcpy(&n, rows + r, sizeof n);
    if (n < 0 || n > h.cap) return IMG_ROWS;
    if (n > cap) return IMG_CAPACITY;
    least += (uint64_t)n * 8;  // (every image holds the dead points' ln L)
  }
  if (h.total_bytes < least) return IMG_TRUNCATED;
  if (h.ndim != ndim) return IMG_NDIM;
  if (out) *out = h;
  if (rows_out) *rows_out = rows;
  if (cap_out) *cap_out = cap;
  return IMG_OK;
}

}  // namespace dh_ns_state
