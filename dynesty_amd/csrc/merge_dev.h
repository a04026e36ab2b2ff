// Internal: what the units of the combiner share on the device side (merge.hip, merge_fold.hip, merge_marginals.hip,
// merge_errors.hip): the scan operators and the three-launch scan, np.logaddexp, the small host helpers around a launch,
// and the kernels the merge and the fold both launch (sequences, pairwise rounds, scatter, integrals, summaries).  The
// sizes and the scratch layouts are merge_plan.h's.  Everything here is local to the unit that includes it.
#pragma once
#include <math.h>

#include <vector>

#include "ctx.h"

using namespace dh;
using namespace dh_merge;

namespace {

// ---- scans ----------------------------------------------------------------------------------------------------------

struct SumD {
  typedef double T;
  __device__ static T id() { return 0.0; }
  __device__ static T op(T a, T b) { return a + b; }
};
struct SumI {
  typedef int T;
  __device__ static T id() { return 0; }
  __device__ static T op(T a, T b) { return a + b; }
};
// ln sum exp as (max, sum scaled by exp(-max)) pairs: associative, never underflows against a far later maximum
struct LsePair {
  double m, s;
};
struct Lse {
  typedef LsePair T;
  __device__ static T id() { return T{-INFINITY, 0.0}; }
  __device__ static T op(T a, T b) {
    if (a.s == 0.0) return b;  // the identity (and nothing else: a point's own pair has s = 1) combines exactly
    if (b.s == 0.0 || b.m == -INFINITY) return a;
    if (a.m >= b.m) return T{a.m, a.s + b.s * exp(b.m - a.m)};
    return T{b.m, a.s * exp(a.m - b.m) + b.s};
  }
};
static_assert(sizeof(LsePair) == kScanElem, "the layouts size a scan's chunk aggregates by kScanElem");

// Inclusive scan of the 256 per-thread values of a workgroup (Hillis-Steele in LDS); returns the thread's inclusive
// value, *excl its exclusive one, *total the workgroup's.
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(typename Op::T v, typename Op::T* lds, typename Op::T* excl,
                                                     typename Op::T* total) {
  typedef typename Op::T T;
  const int t = threadIdx.x;
  T* a = lds;
  T* b = lds + kT;
  a[t] = v;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {
    b[t] = t >= d ? Op::op(a[t - d], a[t]) : a[t];
    __syncthreads();
    T* sw = a;
    a = b;
    b = sw;
  }
  const T inc = a[t];
  *excl = t > 0 ? a[t - 1] : Op::id();
  *total = a[kT - 1];
  __syncthreads();
  return inc;
}

// F: struct { typedef Op; __device__ Op::T term(long long k) const; __device__ void put(long long k, Op::T incl, Op::T excl) const; }
template <class F>
__global__ void __launch_bounds__(kT) scan_reduce(F f, long long M, typename F::Op::T* part) {
  typedef typename F::Op Op;
  typedef typename Op::T T;
  __shared__ T lds[2 * kT];
  const long long k0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kItems;
  T acc = Op::id();
  for (int j = 0; j < kItems; ++j)
    if (k0 + j < M) acc = Op::op(acc, f.term(k0 + j));
  T ex, tot;
  block_scan<Op>(acc, lds, &ex, &tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one workgroup: part[b] becomes the combination of the aggregates of the workgroups before b
template <class Op>
__global__ void __launch_bounds__(kT) scan_carry(typename Op::T* part, int nblk) {
  typedef typename Op::T T;
  __shared__ T lds[2 * kT];
  T carry = Op::id();
  for (int b0 = 0; b0 < nblk; b0 += kT) {
    const int b = b0 + threadIdx.x;
    const T v = b < nblk ? part[b] : Op::id();
    T ex, tot;
    block_scan<Op>(v, lds, &ex, &tot);
    if (b < nblk) part[b] = Op::op(carry, ex);
    carry = Op::op(carry, tot);
  }
}

template <class F>
__global__ void __launch_bounds__(kT) scan_apply(F f, long long M, const typename F::Op::T* part) {
  typedef typename F::Op Op;
  typedef typename Op::T T;
  __shared__ T lds[2 * kT];
  const long long k0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kItems;
  T x[kItems];
  T acc = Op::id();
  for (int j = 0; j < kItems; ++j) {
    x[j] = k0 + j < M ? f.term(k0 + j) : Op::id();
    acc = Op::op(acc, x[j]);
  }
  T ex, tot;
  block_scan<Op>(acc, lds, &ex, &tot);
  T run = Op::op(part[blockIdx.x], ex);
  for (int j = 0; j < kItems; ++j) {
    const T before = run;
    run = Op::op(run, x[j]);
    if (k0 + j < M) f.put(k0 + j, run, before);
  }
}

__device__ __forceinline__ double logaddexp_np(double x, double y) {  // np.logaddexp
  if (x == y) return x + 0.6931471805599453;
  const double d = x - y;
  if (d > 0) return x + log1p(exp(-d));
  if (d <= 0) return y + log1p(exp(d));
  return x + y;
}

// ---- the counter-based stream of the statistical errors and of the seeds' choice -------------------------------------

// Philox4x32-10 under key `seed`, rocrand's stream model: block `blk` of subsequence `seq`, four words in stream order
__device__ __forceinline__ void philox4x32_10(uint64_t seed, uint64_t seq, uint64_t blk, uint32_t* w) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = (uint32_t)seq, c3 = (uint32_t)(seq >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}
// rocrand's uniform_distribution_double(v1, v2): (0, 1], exact
__device__ __forceinline__ double uniform_double(uint32_t w0, uint32_t w1) {
  const unsigned long long m = (unsigned long long)w0 | ((unsigned long long)(w1 >> 11) << 32);
  return 1.1102230246251565e-16 + (double)m * 1.1102230246251565e-16;
}

template <class F>
bool run_scan(dh_ctx* ctx, const F& f, long long M, void* part) {
  typedef typename F::Op Op;
  const int nblk = (int)blocks_for((size_t)M, kChunk);
  typename Op::T* p = (typename Op::T*)part;
  hipLaunchKernelGGL(scan_reduce<F>, dim3(nblk), dim3(kT), 0, ctx->stream, f, M, p);
  hipLaunchKernelGGL(scan_carry<Op>, dim3(1), dim3(kT), 0, ctx->stream, p, nblk);
  hipLaunchKernelGGL(scan_apply<F>, dim3(nblk), dim3(kT), 0, ctx->stream, f, M, (const typename Op::T*)p);
  return hip_ok(ctx, hipGetLastError(), "merge scan launch");
}

template <class K>
bool lds_limit(dh_ctx* ctx, K kernel, size_t bytes) {
  return hip_ok(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), "LDS size");
}

// An allocation of its own as one layout: the size pass, hipMalloc of that total, the pointer pass.  Null (and the
// layout's pointers null) where the device has no room.
template <class Layout>
size_t layout_bytes(Layout&& layout) {
  Carver size;
  layout(size);
  return size.off;
}
template <class Layout>
char* device_carve(Layout&& layout) {
  char* base = nullptr;
  if (hipMalloc((void**)&base, layout_bytes(layout)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  Carver place{base};
  layout(place);
  return base;
}

inline int need_merged(dh_ctx* ctx) {
  if (!ctx->merged.base) return fail(ctx, DH_ERR_ARG, "no merged run in this context");
  return DH_OK;
}

// ---- sequences ------------------------------------------------------------------------------------------------------

// final live points of run blockIdx.y: rank of slot s = #{t : l_t < l_s or (l_t == l_s and t < s)} (a stable ascending
// sort by counting: N^2 comparisons per run against LDS tiles, no data-dependent addressing)
__global__ void __launch_bounds__(kT) mg_live_rank(int N, const double* __restrict__ live_logl,
                                                   const long long* __restrict__ off, const long long* __restrict__ nit,
                                                   double* __restrict__ seq_l, int* __restrict__ seq_run,
                                                   int* __restrict__ live_slot) {
  __shared__ double tile[kLiveTile];
  const int r = blockIdx.y, s = blockIdx.x * kT + threadIdx.x;
  const double* keys = live_logl + (size_t)r * N;
  const bool mine = s < N;
  const double x = keys[mine ? s : 0];
  int rank = 0;
  for (int t0 = 0; t0 < N; t0 += kLiveTile) {
    const int nt = N - t0 < kLiveTile ? N - t0 : kLiveTile;
    __syncthreads();
    for (int t = threadIdx.x; t < nt; t += kT) tile[t] = keys[t0 + t];
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const double y = tile[t];
      rank += (y < x || (y == x && t0 + t < s)) ? 1 : 0;
    }
  }
  if (!mine) return;
  const long long g = off[r] + nit[r] + rank;  // rank < N always (NaN keys compare false: ranks may collide, never leave)
  seq_l[g] = x;
  seq_run[g] = r;
  live_slot[(size_t)r * N + rank] = s;
}

__global__ void __launch_bounds__(kT) mg_dead_copy(long long stride, const double* __restrict__ dead_logl,
                                                   const long long* __restrict__ off, const long long* __restrict__ nit,
                                                   double* __restrict__ seq_l, int* __restrict__ seq_run) {
  const int r = blockIdx.y;
  const long long i = (long long)blockIdx.x * kT + threadIdx.x;
  if (i >= nit[r]) return;
  seq_l[off[r] + i] = dead_logl[(size_t)r * stride + i];
  seq_run[off[r] + i] = r;
}

// flags[0]: a NaN value; flags[1]: a run's sequence decreases somewhere; org = identity
__global__ void __launch_bounds__(kT) mg_check(long long M, const double* __restrict__ seq_l, const int* __restrict__ seq_run,
                                               const long long* __restrict__ off, int* __restrict__ org, int* flags) {
  const long long g = (long long)blockIdx.x * kT + threadIdx.x;
  if (g >= M) return;
  const double x = seq_l[g];
  org[g] = (int)g;
  if (x != x) flags[0] = 1;
  if (g > off[seq_run[g]] && x < seq_l[g - 1]) flags[1] = 1;
}

// ---- order ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ long long lower_bound_dev(const double* a, long long n, double x) {  // #{a_j < x}
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ long long upper_bound_dev(const double* a, long long n, double x) {  // #{a_j <= x}
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One round: the lists of runs [a, a + wd) and [a + wd, a + 2 wd) (element ranges off[...]) merge into one, the left
// list first among equal values.  Neighbouring threads hold neighbouring values, so their searches share their probes.
__global__ void __launch_bounds__(kT) mg_merge_round(long long M, int R, int wd, const long long* __restrict__ off,
                                                     const double* __restrict__ key_in, const int* __restrict__ org_in,
                                                     double* __restrict__ key_out, int* __restrict__ org_out) {
  const long long p = (long long)blockIdx.x * kT + threadIdx.x;
  if (p >= M) return;
  int lo_r = 0, hi_r = R;  // the run whose element range holds p: off[lo_r] <= p < off[lo_r + 1]
  while (hi_r - lo_r > 1) {
    const int mid = (lo_r + hi_r) >> 1;
    if (off[mid] <= p) lo_r = mid; else hi_r = mid;
  }
  const int a = lo_r / (2 * wd) * (2 * wd);
  const int m_r = a + wd < R ? a + wd : R, e_r = a + 2 * wd < R ? a + 2 * wd : R;
  const long long lo = off[a], mid = off[m_r], hi = off[e_r];
  const double x = key_in[p];
  long long pos;
  if (p < mid)
    pos = p + lower_bound_dev(key_in + mid, hi - mid, x);
  else
    pos = lo + (p - mid) + upper_bound_dev(key_in + lo, mid - lo, x);
  key_out[pos] = x;  // lo <= pos < hi for any input
  org_out[pos] = org_in[p];
}

// ---- scatter --------------------------------------------------------------------------------------------------------

struct MgSrc {
  const double *dead_u, *live_u;
  const int *dead_id, *dead_it, *dead_nc, *live_it;  // null together
  long long stride;
  int N;
};

__global__ void __launch_bounds__(kT) mg_scatter(long long M, MgSrc s, const double* __restrict__ key, const int* __restrict__ org,
                                                 const int* __restrict__ seq_run, const long long* __restrict__ off,
                                                 const long long* __restrict__ nit, const int* __restrict__ live_slot,
                                                 double* __restrict__ logl, int* __restrict__ run, int* __restrict__ seq,
                                                 int* __restrict__ id, int* __restrict__ it, int* __restrict__ nc,
                                                 int* __restrict__ fin, long long* __restrict__ src_row) {
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  long long g = org[k];
  if (g < 0 || g >= M) g = 0;
  const int r = seq_run[g];
  const long long i = g - off[r], nd = nit[r];
  const bool live = i >= nd;
  long long li = i - nd;
  if (li < 0 || li >= s.N) li = 0;  // (only where NaN keys left a position unwritten: the call fails, the reads stay inside)
  int slot = live ? live_slot[(size_t)r * s.N + li] : 0;
  if (slot < 0 || slot >= s.N) slot = 0;
  const long long drow = (long long)r * s.stride + (live ? 0 : i), lrow = (long long)r * s.N + slot;
  logl[k] = key[k];
  run[k] = r;
  seq[k] = (int)i;
  fin[k] = live ? 1 : 0;
  src_row[k] = live ? -1 - lrow : drow;
  if (s.dead_id) {
    // (both loads are issued, the select follows: no load under a condition)
    const int d_id = s.dead_id[drow], d_it = s.dead_it[drow], d_nc = s.dead_nc[drow], l_it = s.live_it[lrow];
    id[k] = live ? slot : d_id;
    it[k] = live ? l_it : d_it;
    nc[k] = live ? 1 : d_nc;
  }
}

__global__ void __launch_bounds__(kT) mg_scatter_rows(size_t total, int D, MgSrc s, const long long* __restrict__ src_row,
                                                      double* __restrict__ u) {
  const size_t e = (size_t)blockIdx.x * kT + threadIdx.x;
  if (e >= total) return;
  const size_t k = e / (size_t)D;
  const int d = (int)(e - k * (size_t)D);
  const long long row = src_row[k];
  const double* from = row >= 0 ? s.dead_u + (size_t)row * D : s.live_u + (size_t)(-1 - row) * D;
  u[e] = from[d];
}

// ---- integrals --------------------------------------------------------------------------------------------------

// ln w by the trapezoid rule and the cumulative ln Z (nested._integrate_full); d ln X of point k is its own step, not
// the difference of two cumulative values
struct FLogz {
  typedef Lse Op;
  const double *logl, *logvol, *step;
  double *logwt, *logdvol, *logz;
  __device__ LsePair term(long long k) const {
    const double v0 = k > 0 ? logvol[k - 1] : 0.0, l0 = k > 0 ? logl[k - 1] : -1.e300;
    // 1 - exp(-step) through expm1: exp(-step) is next to 1, and its rounding would be n ulps of the difference
    const double ldv = v0 + log(-expm1(-step[k])) + (-0.6931471805599453);
    const double lw = logaddexp_np(logl[k], l0) + ldv;
    logdvol[k] = ldv;
    logwt[k] = lw;
    return LsePair{lw, 1.0};
  }
  __device__ void put(long long k, LsePair incl, LsePair) const { logz[k] = incl.m + log(incl.s); }
};
// information: cumsum(w0 l0 + w1 l1) - ln Z exp(ln Z_k - ln Z), everything normalised by the FINAL Z
struct FInfo {
  typedef SumD Op;
  const double *logl, *logdvol, *logz;
  double* h;
  long long M;
  __device__ double term(long long k) const {
    const double lz = logz[M - 1], l1 = logl[k], l0 = k > 0 ? logl[k - 1] : -1.e300, ldv = logdvol[k];
    const double w0 = exp(l0 - lz + ldv), w1 = exp(l1 - lz + ldv);
    return (w0 > 0 ? w0 * l0 : 0.0) + (w1 > 0 ? w1 * l1 : 0.0);
  }
  __device__ void put(long long k, double incl, double) const {
    const double lz = logz[M - 1];
    h[k] = incl - lz * exp(logz[k] - lz);
  }
};
// var[ln Z] = |cumsum dH d ln X|; stored as its square root
struct FVar {
  typedef SumD Op;
  const double *h, *step;
  double* logzerr;
  __device__ double term(long long k) const { return (h[k] - (k > 0 ? h[k - 1] : 0.0)) * step[k]; }
  __device__ void put(long long k, double incl, double) const { logzerr[k] = sqrt(fabs(incl)); }
};
// cumulative sum of f(k); mode 0: exp(logwt - ln Z) (its inclusive scan lands in cw), mode 1: the normalised weights
struct FCum {
  typedef SumD Op;
  const double *logwt, *logz;
  double *w, *cw;
  long long M;
  int mode;
  __device__ double term(long long k) const { return mode == 0 ? exp(logwt[k] - logz[M - 1]) : w[k]; }
  __device__ void put(long long k, double incl, double) const { cw[k] = incl; }
};

// w = exp(logwt - ln Z) / sum (the sum is the last cumulative value of the first pass)
__global__ void __launch_bounds__(kT) mg_weights(long long M, const double* __restrict__ logwt, const double* __restrict__ logz,
                                                 const double* __restrict__ cw, double* __restrict__ w) {
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  w[k] = exp(logwt[k] - logz[M - 1]) / cw[M - 1];
}
// C /= C_M, so that C_M is 1 exactly (utils.resample_equal); `last` is a copy taken before this launch
__global__ void __launch_bounds__(kT) mg_cum_norm(long long M, double* __restrict__ cw, const double* __restrict__ last) {
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  cw[k] = cw[k] / last[0];
}

// ---- summaries --------------------------------------------------------------------------------------------------

// column c < D: sum w v_c; c = D: sum w; c = D + 1: sum w^2 -- over the points of chunk blockIdx.x, in order
__global__ void __launch_bounds__(kT) mg_mom1(long long M, int D, long long chunk, const double* __restrict__ w,
                                              const double* __restrict__ v, double* __restrict__ part) {
  const int c = blockIdx.y * kT + threadIdx.x;
  if (c >= D + 2) return;
  const long long k0 = (long long)blockIdx.x * chunk, k1 = k0 + chunk < M ? k0 + chunk : M;
  double acc = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const double wk = w[k];
    const double x = c < D ? v[(size_t)k * D + c] : c == D ? 1.0 : wk;
    acc = fma(wk, x, acc);
  }
  part[(size_t)blockIdx.x * (D + 2) + c] = acc;
}
// mom = [sum w, sum w^2, ESS, mean_0 ..]: the chunks' sums in chunk order; mean = sum w v / sum w (np.average)
__global__ void __launch_bounds__(kT) mg_mom1_fin(int D, int nchunk, const double* __restrict__ part, double* __restrict__ mom) {
  const int c = blockIdx.x * kT + threadIdx.x;
  if (c >= D + 2) return;
  double acc = 0.0, ws = 0.0;
  for (int b = 0; b < nchunk; ++b) {
    acc += part[(size_t)b * (D + 2) + c];
    ws += part[(size_t)b * (D + 2) + D];
  }
  if (c < D) mom[3 + c] = acc / ws;
  if (c == D) mom[0] = acc;
  if (c == D + 1) {
    mom[1] = acc;
    mom[2] = 1.0 / acc;
  }
}

// integers: order does not matter
__global__ void __launch_bounds__(kT) mg_sum_nc(long long M, const int* __restrict__ nc, unsigned long long* out) {
  __shared__ unsigned long long red[kT];
  unsigned long long acc = 0;
  for (long long k = (long long)blockIdx.x * kT + threadIdx.x; k < M; k += (long long)gridDim.x * kT) acc += (unsigned long long)nc[k];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out, red[0]);
}

__global__ void mg_summary(long long M, const double* logz, const double* logzerr, const double* h, const double* mom,
                           const unsigned long long* ncall, double* out) {
  if (threadIdx.x || blockIdx.x) return;
  out[0] = (double)M;
  out[1] = logz[M - 1];
  out[2] = logzerr[M - 1];
  out[3] = h[M - 1];
  out[4] = mom[2];
  out[5] = (double)ncall[0];
}

// The integrals of a run whose logl, logvol and per-point steps stand, in the order dh_merge_runs has always launched
// them: ln w and ln Z, H, var ln Z, the weights and their cumulative sums, the first moments, the summary (6 doubles
// into `summ`).  Launches only; `ncall` must be zero.  Shared by the merge (merge.hip) and the fold (merge_fold.hip).
struct IntegralScratch {
  double *logdvol, *mom_part, *last, *summ;
  u64* ncall;
  char* part;
};
inline bool run_integrals(dh_ctx* ctx, const MergedArrays& m, long long M, int D, bool pt, const double* step,
                          const IntegralScratch& s) {
  hipStream_t st = ctx->stream;
  long long chunk1;
  const int nchunk1 = moment_chunks(M, (size_t)D + 2, &chunk1);
  const unsigned gM = blocks_for((size_t)M, kT);
  if (!run_scan(ctx, FLogz{m.logl, m.logvol, step, m.logwt, s.logdvol, m.logz}, M, s.part) ||
      !run_scan(ctx, FInfo{m.logl, s.logdvol, m.logz, m.h, M}, M, s.part) ||
      !run_scan(ctx, FVar{m.h, step, m.logzerr}, M, s.part) ||
      !run_scan(ctx, FCum{m.logwt, m.logz, m.w, m.cw, M, 0}, M, s.part))
    return false;
  hipLaunchKernelGGL(mg_weights, dim3(gM), dim3(kT), 0, st, M, m.logwt, m.logz, m.cw, m.w);
  if (!run_scan(ctx, FCum{m.logwt, m.logz, m.w, m.cw, M, 1}, M, s.part) ||
      !hip_ok(ctx, hipMemcpyAsync(s.last, m.cw + (M - 1), 8, hipMemcpyDeviceToDevice, st), "D2D"))
    return false;
  hipLaunchKernelGGL(mg_cum_norm, dim3(gM), dim3(kT), 0, st, M, m.cw, s.last);
  hipLaunchKernelGGL(mg_mom1, dim3(nchunk1, blocks_for((size_t)D + 2, kT)), dim3(kT), 0, st, M, D, chunk1, m.w, m.v, s.mom_part);
  hipLaunchKernelGGL(mg_mom1_fin, dim3(blocks_for((size_t)D + 2, kT)), dim3(kT), 0, st, D, nchunk1, s.mom_part, m.mom);
  if (pt) hipLaunchKernelGGL(mg_sum_nc, dim3(gM < 1024 ? gM : 1024), dim3(kT), 0, st, M, m.nc, s.ncall);
  hipLaunchKernelGGL(mg_summary, dim3(1), dim3(64), 0, st, M, m.logz, m.logzerr, m.h, m.mom, s.ncall, s.summ);
  return hip_ok(ctx, hipGetLastError(), "integrals launch");
}

}  // namespace
