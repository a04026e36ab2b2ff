// The combiner on the device: R static runs of equal nlive merged into ONE run that stays in HBM (DESIGN.md section
// 3.8).  It follows ensemble.merge_static_runs -- the reference's utils.merge_runs for such runs (utils.py:1817-1900,
// 2000-2226), integrals as utils.compute_integrals (utils.py:1411-1467), moments and resampling as utils.py:1081-1187.
//
// Stages, all on the context's stream with no host synchronisation in between:
//   sequences : per run its dead values in death order, then its final live values ascending (ties by slot)
//   order     : ceil(log2 R) rounds of pairwise stable merges by counting (element i of the left list goes to
//               i + #{right < x}, element j of the right list to j + #{left <= x}) = np.argsort(kind="stable")
//   scatter   : scalars, unit-cube rows; parameters through eval_launch_dev (bit-identical to dh_problem_eval)
//   scans     : three launches each (block aggregates, carries, apply): live counts, ln X, ln Z (rescaling
//               log-sum-exp pairs), information, var[ln Z], cumulative weights
//   summaries : sums of w, w^2, w v per chunk and their fixed-order reduction; the covariance on request
#include <math.h>

#include <vector>

#include "ctx.h"

using namespace dh;

namespace {

constexpr int kT = 256;
constexpr int kItems = 8;              // consecutive points per thread of a scan
constexpr int kChunk = kT * kItems;    // points per workgroup of a scan
constexpr int kLiveTile = 1024;        // live keys staged in LDS per step of the rank sort
constexpr long long kMomChunk = 2048;  // points per workgroup of the moment sums (at least)

inline unsigned blocks_for(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

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

// live counts: samples_n = R N - (final live points before k); step[k] = ln((n + 1) / n) = log1p(1 / n)
struct FCount {
  typedef SumI Op;
  const int* fin;
  int* n;
  double* step;
  int total;
  __device__ int term(long long k) const { return fin[k]; }
  __device__ void put(long long k, int, int excl) const {
    const int nl = total - excl;
    n[k] = nl;
    step[k] = log1p(1.0 / (double)nl);  // (log((n + 1) / n) would carry the quotient's rounding at full size: n ulps of the step)
  }
};
// ln X = -cumsum step
struct FVol {
  typedef SumD Op;
  const double* step;
  double* logvol;
  __device__ double term(long long k) const { return step[k]; }
  __device__ void put(long long k, double incl, double) const { logvol[k] = -incl; }
};
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

// ---- summaries ------------------------------------------------------------------------------------------------------

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
// pair p = i D + j: sum w (v_i - mean_i) (v_j - mean_j) over the chunk's points
__global__ void __launch_bounds__(kT) mg_mom2(long long M, int D, long long chunk, const double* __restrict__ w,
                                              const double* __restrict__ v, const double* __restrict__ mom,
                                              double* __restrict__ part) {
  const int p = blockIdx.y * kT + threadIdx.x;
  if (p >= D * D) return;
  const int i = p / D, j = p - i * D;
  const double mi = mom[3 + i], mj = mom[3 + j];
  const long long k0 = (long long)blockIdx.x * chunk, k1 = k0 + chunk < M ? k0 + chunk : M;
  double acc = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const double* row = v + (size_t)k * D;
    acc = fma(w[k] * (row[i] - mi), row[j] - mj, acc);
  }
  part[(size_t)blockIdx.x * D * D + p] = acc;
}
// utils.mean_and_cov: cov = wsum / (wsum^2 - w2sum) * sum
__global__ void __launch_bounds__(kT) mg_mom2_fin(int D, int nchunk, const double* __restrict__ part, const double* __restrict__ mom,
                                                  double* __restrict__ cov) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= D * D) return;
  double acc = 0.0;
  for (int b = 0; b < nchunk; ++b) acc += part[(size_t)b * D * D + p];
  const double ws = mom[0], w2 = mom[1];
  cov[p] = ws / (ws * ws - w2) * acc;
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

// ---- resampling -----------------------------------------------------------------------------------------------------

// idx[i] = #{j : C_j <= (u0 + i) / n_out} (utils.resample_equal's walk as a search; C_M = 1 > every position)
__global__ void __launch_bounds__(kT) mg_resample(long long M, const double* __restrict__ cw, double u0, long long n_out,
                                                  long long* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * kT + threadIdx.x;
  if (i >= n_out) return;
  const double pos = (u0 + (double)i) / (double)n_out;
  long long j = upper_bound_dev(cw, M, pos);
  idx[i] = j < M ? j : M - 1;
}

__global__ void __launch_bounds__(kT) mg_gather(size_t total, int D, long long M, const double* __restrict__ v,
                                                const long long* __restrict__ idx, double* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * kT + threadIdx.x;
  if (e >= total) return;
  const size_t i = e / (size_t)D;
  long long j = idx[i];
  if (j < 0 || j >= M) j = 0;
  out[e] = v[(size_t)j * D + (e - i * (size_t)D)];
}

// ---- host -----------------------------------------------------------------------------------------------------------

struct Carver {
  char* base;
  size_t off = 0;
  template <class T>
  void operator()(T*& p, size_t count, bool wanted = true) {
    p = nullptr;
    if (!wanted) return;
    if (base) p = (T*)(base + off);
    off += (count * sizeof(T) + 255) & ~(size_t)255;
  }
};

struct Scratch {
  long long *off, *nit, *src_row;
  double *seq_l, *key_b, *step, *logdvol, *eval_l, *mom_part, *last, *summ;
  int *seq_run, *org_a, *org_b, *live_slot, *flags;
  unsigned long long* ncall;
  char* part;
};

void carve_merged(Carver& c, dh_merged& m, size_t M, size_t D, bool pt) {
  c(m.logl, M);
  c(m.logvol, M);
  c(m.logwt, M);
  c(m.logz, M);
  c(m.logzerr, M);
  c(m.h, M);
  c(m.w, M);
  c(m.cw, M);
  c(m.u, M * D);
  c(m.v, M * D);
  c(m.mom, 3 + D);
  c(m.run, M);
  c(m.seq, M);
  c(m.n, M);
  c(m.fin, M);
  c(m.id, M, pt);
  c(m.it, M, pt);
  c(m.nc, M, pt);
}

void carve_scratch(Carver& c, Scratch& s, size_t M, size_t R, size_t N, size_t D, size_t nblk, size_t nchunk) {
  c(s.off, R + 1);
  c(s.nit, R);
  c(s.src_row, M);
  c(s.seq_l, M);
  c(s.key_b, M);
  c(s.step, M);
  c(s.logdvol, M);
  c(s.eval_l, M);
  c(s.mom_part, nchunk * (D + 2));
  c(s.last, 1);
  c(s.summ, 8);
  c(s.seq_run, M);
  c(s.org_a, M);
  c(s.org_b, M);
  c(s.live_slot, R * N);
  c(s.flags, 4);
  c(s.ncall, 1);
  c(s.part, (nblk + 1) * sizeof(LsePair));
}

int moment_chunks(long long M, size_t cols, long long* chunk) {
  long long n = (M + kMomChunk - 1) / kMomChunk;
  const long long cap = (long long)(((size_t)8 << 20) / (cols ? cols : 1));  // at most 64 MB of partial sums
  if (n > 1024) n = 1024;
  if (n > cap) n = cap;
  if (n < 1) n = 1;
  *chunk = (M + n - 1) / n;
  return (int)((M + *chunk - 1) / *chunk);
}

// The merge proper, from device arrays.  `niter` is a host array.
int merge_core(dh_ctx* ctx, int problem, int R, int N, int D, long long stride, const long long* niter,
               const double* dead_logl, const double* live_logl, const double* dead_u, const double* live_u,
               const int* dead_id, const int* dead_it, const int* dead_nc, const int* live_it, double* summary_out) {
  hipStream_t st = ctx->stream;
  std::vector<long long> off((size_t)R + 1, 0), nit((size_t)R);
  long long maxnit = 0;
  for (int r = 0; r < R; ++r) {
    if (niter[r] < 0 || niter[r] > stride) return fail(ctx, DH_ERR_ARG, "merge: niter[%d] = %lld outside [0, %lld]", r, niter[r], stride);
    nit[(size_t)r] = niter[r];
    off[(size_t)r + 1] = off[(size_t)r] + niter[r] + N;
    if (niter[r] > maxnit) maxnit = niter[r];
  }
  const long long M = off[(size_t)R];
  if (M >= (1ll << 31) - kChunk || (long long)R * N >= (1ll << 31))
    return fail(ctx, DH_ERR_ARG, "merge: %lld points (positions travel as 32-bit indices)", M);
  if ((unsigned long long)M * (unsigned long long)D >= (1ull << 32))  // mg_scatter_rows: one thread per element of a row array
    return fail(ctx, DH_ERR_ARG, "merge: %lld points of %d coordinates (a row array is limited to 2^32 elements)", M, D);
  const bool pt = dead_id != nullptr;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(st);
  merged_free(ctx);  // the next merge replaces the merged run
  dh_merged m;
  Scratch s;
  const size_t nblk = blocks_for((size_t)M, kChunk);
  long long chunk1;
  const int nchunk1 = moment_chunks(M, (size_t)D + 2, &chunk1);
  Carver sz{nullptr};
  carve_merged(sz, m, (size_t)M, (size_t)D, pt);
  Carver ssz{nullptr};
  carve_scratch(ssz, s, (size_t)M, (size_t)R, (size_t)N, (size_t)D, nblk, (size_t)nchunk1);
  char *mbase = nullptr, *sbase = nullptr;
  if (hipMalloc((void**)&mbase, sz.off) != hipSuccess || hipMalloc((void**)&sbase, ssz.off) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(mbase);
    return fail(ctx, DH_ERR_NOMEM, "merge: %zu + %zu bytes of device memory", sz.off, ssz.off);
  }
  Carver cm{mbase};
  carve_merged(cm, m, (size_t)M, (size_t)D, pt);
  Carver cs{sbase};
  carve_scratch(cs, s, (size_t)M, (size_t)R, (size_t)N, (size_t)D, nblk, (size_t)nchunk1);
  m.base = mbase;
  m.M = M;
  m.ndim = D;
  m.runs = R;
  m.nlive = N;
  m.have_pt = pt;
  auto done = [&](int rc) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(sbase);
    if (rc != DH_OK) {
      (void)hipFree(mbase);
    } else {
      m.idx = nullptr;
      m.tie_idx = m.tie_ep = nullptr;
      m.tie_n = -1;
      ctx->merged = m;
    }
    return rc;
  };
  if (!hip_ok(ctx, hipMemcpyAsync(s.off, off.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, st), "H2D") ||
      !hip_ok(ctx, hipMemcpyAsync(s.nit, nit.data(), (size_t)R * 8, hipMemcpyHostToDevice, st), "H2D") ||
      !hip_ok(ctx, hipMemsetAsync(s.live_slot, 0, (size_t)R * N * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.org_a, 0, (size_t)M * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.org_b, 0, (size_t)M * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.seq_run, 0, (size_t)M * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.flags, 0, 16, st), "memset") || !hip_ok(ctx, hipMemsetAsync(s.ncall, 0, 8, st), "memset"))
    return done(DH_ERR_HIP);
  // sequences
  hipLaunchKernelGGL(mg_live_rank, dim3(blocks_for((size_t)N, kT), R), dim3(kT), 0, st, N, live_logl, s.off, s.nit, s.seq_l,
                     s.seq_run, s.live_slot);
  if (maxnit > 0)
    hipLaunchKernelGGL(mg_dead_copy, dim3(blocks_for((size_t)maxnit, kT), R), dim3(kT), 0, st, stride, dead_logl, s.off, s.nit,
                       s.seq_l, s.seq_run);
  const unsigned gM = blocks_for((size_t)M, kT);
  hipLaunchKernelGGL(mg_check, dim3(gM), dim3(kT), 0, st, M, s.seq_l, s.seq_run, s.off, s.org_a, s.flags);
  // order: pairwise rounds, ping-pong between (seq_l, org_a) and (key_b, org_b)
  double *kin = s.seq_l, *kout = s.key_b;
  int *oin = s.org_a, *oout = s.org_b;
  for (int wd = 1; wd < R; wd *= 2) {
    hipLaunchKernelGGL(mg_merge_round, dim3(gM), dim3(kT), 0, st, M, R, wd, s.off, kin, oin, kout, oout);
    double* kt = kin;
    kin = kout;
    kout = kt;
    int* ot = oin;
    oin = oout;
    oout = ot;
  }
  // (the sequences' run index is read by position g: it lives in seq_run, which no round writes)
  MgSrc src{dead_u, live_u, dead_id, dead_it, dead_nc, live_it, stride, N};
  hipLaunchKernelGGL(mg_scatter, dim3(gM), dim3(kT), 0, st, M, src, kin, oin, s.seq_run, s.off, s.nit, s.live_slot, m.logl, m.run,
                     m.seq, m.id, m.it, m.nc, m.fin, s.src_row);
  hipLaunchKernelGGL(mg_scatter_rows, dim3(blocks_for((size_t)M * D, kT)), dim3(kT), 0, st, (size_t)M * D, D, src, s.src_row, m.u);
  if (!hip_ok(ctx, hipGetLastError(), "merge launch")) return done(DH_ERR_HIP);
  int rc = eval_launch_dev(ctx, problem, (int)M, m.u, m.v, s.eval_l);
  if (rc) return done(rc);
  // scans
  if (!run_scan(ctx, FCount{m.fin, m.n, s.step, R * N}, M, s.part) || !run_scan(ctx, FVol{s.step, m.logvol}, M, s.part) ||
      !run_scan(ctx, FLogz{m.logl, m.logvol, s.step, m.logwt, s.logdvol, m.logz}, M, s.part) ||
      !run_scan(ctx, FInfo{m.logl, s.logdvol, m.logz, m.h, M}, M, s.part) ||
      !run_scan(ctx, FVar{m.h, s.step, m.logzerr}, M, s.part) ||
      !run_scan(ctx, FCum{m.logwt, m.logz, m.w, m.cw, M, 0}, M, s.part))
    return done(DH_ERR_HIP);
  hipLaunchKernelGGL(mg_weights, dim3(gM), dim3(kT), 0, st, M, m.logwt, m.logz, m.cw, m.w);
  if (!run_scan(ctx, FCum{m.logwt, m.logz, m.w, m.cw, M, 1}, M, s.part) ||
      !hip_ok(ctx, hipMemcpyAsync(s.last, m.cw + (M - 1), 8, hipMemcpyDeviceToDevice, st), "D2D"))
    return done(DH_ERR_HIP);
  hipLaunchKernelGGL(mg_cum_norm, dim3(gM), dim3(kT), 0, st, M, m.cw, s.last);
  // summaries
  hipLaunchKernelGGL(mg_mom1, dim3(nchunk1, blocks_for((size_t)D + 2, kT)), dim3(kT), 0, st, M, D, chunk1, m.w, m.v, s.mom_part);
  hipLaunchKernelGGL(mg_mom1_fin, dim3(blocks_for((size_t)D + 2, kT)), dim3(kT), 0, st, D, nchunk1, s.mom_part, m.mom);
  if (pt) hipLaunchKernelGGL(mg_sum_nc, dim3(gM < 1024 ? gM : 1024), dim3(kT), 0, st, M, m.nc, s.ncall);
  hipLaunchKernelGGL(mg_summary, dim3(1), dim3(64), 0, st, M, m.logz, m.logzerr, m.h, m.mom, s.ncall, s.summ);
  double summ[6];
  int flags[4];
  if (!hip_ok(ctx, hipGetLastError(), "merge launch") ||
      !hip_ok(ctx, hipMemcpyAsync(summ, s.summ, sizeof summ, hipMemcpyDeviceToHost, st), "D2H") ||
      !hip_ok(ctx, hipMemcpyAsync(flags, s.flags, sizeof flags, hipMemcpyDeviceToHost, st), "D2H") ||
      !hip_ok(ctx, hipStreamSynchronize(st), "merge sync"))
    return done(DH_ERR_HIP);
  if (flags[0]) return done(fail(ctx, DH_ERR_VALUE, "merge: a log-likelihood is NaN"));
  // (DH_ERR_VALUE, not _ARG: the data are at fault, and the earlier merged run is gone by now -- DH_ERR_ARG from a merge
  // call always means that nothing was touched)
  if (flags[1]) return done(fail(ctx, DH_ERR_VALUE, "merge: a run's dead log-likelihoods decrease (or exceed its final live points')"));
  if (summary_out)
    for (int i = 0; i < 6; ++i) summary_out[i] = summ[i];
  return done(DH_OK);
}

int need_merged(dh_ctx* ctx) {
  if (!ctx->merged.base) return fail(ctx, DH_ERR_ARG, "no merged run in this context");
  return DH_OK;
}

}  // namespace

void dh::kept_free(dh_ctx* ctx) {
  if (ctx->kept.base) (void)hipFree(ctx->kept.base);
  ctx->kept = dh_kept();
}

void dh::merged_free(dh_ctx* ctx) {
  if (ctx->merged.base) (void)hipFree(ctx->merged.base);
  if (ctx->merged.idx) (void)hipFree(ctx->merged.idx);
  if (ctx->merged.tie_idx) (void)hipFree(ctx->merged.tie_idx);  // (tie_ep lies in the same allocation)
  ctx->merged = dh_merged();
}

extern "C" {

int dh_merge_runs(dh_ctx* ctx, int problem, int runs, int nlive, int ndim, int64_t stride, const int64_t* niter,
                  const double* dead_logl, const double* live_logl, const double* dead_u, const double* live_u,
                  const int32_t* dead_id, const int32_t* dead_it, const int32_t* dead_nc, const int32_t* live_it,
                  double* summary_out) {
  DH_CHECK_CTX(ctx);
  ProblemDev pd;
  if (!get_problem(ctx, problem, &pd)) return DH_ERR_ARG;
  if (pd.ndim != ndim) return fail(ctx, DH_ERR_ARG, "merge_runs: problem ndim %d != %d", pd.ndim, ndim);
  const int npt = !!dead_id + !!dead_it + !!dead_nc + !!live_it;
  if (runs < 1 || nlive < 1 || ndim < 1 || ndim > 512 || stride < 0 || !niter || !live_logl || !live_u ||
      (stride > 0 && (!dead_logl || !dead_u)) || (npt != 0 && npt != 4))
    return fail(ctx, DH_ERR_ARG, "merge_runs: bad arguments (runs %d, nlive %d, ndim %d, stride %lld; id / it / nc / live it come together)",
                runs, nlive, ndim, (long long)stride);
  const size_t R = (size_t)runs, N = (size_t)nlive, D = (size_t)ndim, S = (size_t)stride, S1 = S ? S : 1;
  arena_reset(ctx);
  int rc = arena_reserve(ctx, (R * S1 + R * N) * (8 + 8 * D + 12) + 16 * 256);
  if (rc) return rc;
  const double* d_dl = arena_up(ctx, S ? dead_logl : nullptr, R * S1);
  const double* d_ll = arena_up(ctx, live_logl, R * N);
  const double* d_du = arena_up(ctx, S ? dead_u : nullptr, R * S1 * D);
  const double* d_lu = arena_up(ctx, live_u, R * N * D);
  if (!d_dl || !d_ll || !d_du || !d_lu) return DH_ERR_NOMEM;
  const int *d_id = nullptr, *d_it = nullptr, *d_nc = nullptr, *d_li = nullptr;
  if (npt) {
    d_id = arena_up(ctx, S ? dead_id : nullptr, R * S1);
    d_it = arena_up(ctx, S ? dead_it : nullptr, R * S1);
    d_nc = arena_up(ctx, S ? dead_nc : nullptr, R * S1);
    d_li = arena_up(ctx, live_it, R * N);
    if (!d_id || !d_it || !d_nc || !d_li) return DH_ERR_NOMEM;
  }
  std::vector<long long> nit(niter, niter + runs);
  return merge_core(ctx, problem, runs, nlive, ndim, (long long)S1, nit.data(), d_dl, d_ll, d_du, d_lu, d_id, d_it, d_nc, d_li,
                    summary_out);
}

int dh_merge_kept(dh_ctx* ctx, int problem, const int64_t* niter, double* summary_out) {
  DH_CHECK_CTX(ctx);
  const dh_kept& k = ctx->kept;
  if (!k.base) return fail(ctx, DH_ERR_ARG, "merge_kept: no kept ensemble (dh_ns_keep before dh_ns_ensemble)");
  ProblemDev pd;
  if (!get_problem(ctx, problem, &pd)) return DH_ERR_ARG;
  if (problem != k.problem || pd.ndim != k.ndim)
    return fail(ctx, DH_ERR_ARG, "merge_kept: problem %d (ndim %d) is not the kept ensemble's (%d, ndim %d)", problem, pd.ndim,
                k.problem, k.ndim);
  std::vector<long long> nit(k.niter);
  if (niter)
    for (int r = 0; r < k.runs; ++r) nit[(size_t)r] = niter[r];
  return merge_core(ctx, problem, k.runs, k.nlive, k.ndim, k.cap, nit.data(), k.dead_logl, k.live_logl, k.dead_u, k.live_u,
                    k.dead_id, k.dead_it, k.dead_nc, k.live_it, summary_out);
}

int dh_merged_fetch(dh_ctx* ctx, int field, int64_t first, int64_t count, void* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (first < 0 || count < 0 || first + count > m.M || (count && !out))
    return fail(ctx, DH_ERR_ARG, "merged_fetch: [%lld, %lld) of %lld points", (long long)first, (long long)(first + count), m.M);
  const void* src = nullptr;
  size_t width = 8;
  switch (field) {
    case DH_MERGED_LOGL: src = m.logl; break;
    case DH_MERGED_LOGVOL: src = m.logvol; break;
    case DH_MERGED_LOGWT: src = m.logwt; break;
    case DH_MERGED_LOGZ: src = m.logz; break;
    case DH_MERGED_LOGZERR: src = m.logzerr; break;
    case DH_MERGED_INFORMATION: src = m.h; break;
    case DH_MERGED_WEIGHT: src = m.w; break;
    case DH_MERGED_SAMPLES_U: src = m.u; width = 8 * (size_t)m.ndim; break;
    case DH_MERGED_SAMPLES: src = m.v; width = 8 * (size_t)m.ndim; break;
    case DH_MERGED_RUN: src = m.run; width = 4; break;
    case DH_MERGED_SEQ: src = m.seq; width = 4; break;
    case DH_MERGED_SAMPLES_N: src = m.n; width = 4; break;
    case DH_MERGED_FINAL: src = m.fin; width = 4; break;
    case DH_MERGED_ID: src = m.id; width = 4; break;
    case DH_MERGED_IT: src = m.it; width = 4; break;
    case DH_MERGED_NCALL: src = m.nc; width = 4; break;
    default: return fail(ctx, DH_ERR_ARG, "merged_fetch: field %d", field);
  }
  if (!src) return fail(ctx, DH_ERR_ARG, "merged_fetch: field %d was not given to the merge", field);
  if (!count) return DH_OK;
  if (!hip_ok(ctx, hipMemcpyAsync(out, (const char*)src + (size_t)first * width, (size_t)count * width, hipMemcpyDeviceToHost,
                                  ctx->stream), "D2H merged field"))
    return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_merged_moments(dh_ctx* ctx, double* mean, double* cov) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  const size_t D = (size_t)m.ndim;
  hipStream_t st = ctx->stream;
  if (mean && !hip_ok(ctx, hipMemcpyAsync(mean, m.mom + 3, D * 8, hipMemcpyDeviceToHost, st), "D2H mean")) return DH_ERR_HIP;
  if (!cov) return dh_sync(ctx);
  long long chunk;
  const int nchunk = moment_chunks(m.M, D * D, &chunk);
  double* ws = nullptr;
  (void)hipSetDevice(ctx->device);
  if (hipMalloc((void**)&ws, ((size_t)nchunk + 1) * D * D * 8) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, DH_ERR_NOMEM, "merged_moments: workspace");
  }
  double* d_cov = ws + (size_t)nchunk * D * D;
  hipLaunchKernelGGL(mg_mom2, dim3(nchunk, blocks_for(D * D, kT)), dim3(kT), 0, st, m.M, m.ndim, chunk, m.w, m.v, m.mom, ws);
  hipLaunchKernelGGL(mg_mom2_fin, dim3(blocks_for(D * D, kT)), dim3(kT), 0, st, m.ndim, nchunk, ws, m.mom, d_cov);
  int rc = DH_OK;
  if (!hip_ok(ctx, hipGetLastError(), "moments launch") ||
      !hip_ok(ctx, hipMemcpyAsync(cov, d_cov, D * D * 8, hipMemcpyDeviceToHost, st), "D2H cov"))
    rc = DH_ERR_HIP;
  const int rs = dh_sync(ctx);
  (void)hipFree(ws);
  return rc ? rc : rs;
}

int dh_merged_resample(dh_ctx* ctx, double u0, int64_t n_out, int64_t* idx_out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  dh_merged& m = ctx->merged;
  if (!(u0 >= 0.0 && u0 < 1.0) || n_out < 1 || n_out >= (1ll << 32))  // one thread per output
    return fail(ctx, DH_ERR_ARG, "merged_resample: u0 %g, n_out %lld", u0, (long long)n_out);
  if (n_out > m.idx_cap) {
    (void)hipStreamSynchronize(ctx->stream);
    if (m.idx) (void)hipFree(m.idx);
    m.idx = nullptr;
    m.idx_cap = m.idx_n = 0;
    (void)hipSetDevice(ctx->device);
    if (hipMalloc((void**)&m.idx, (size_t)n_out * 8) != hipSuccess) {
      (void)hipGetLastError();
      m.idx = nullptr;
      return fail(ctx, DH_ERR_NOMEM, "merged_resample: %lld indices", (long long)n_out);
    }
    m.idx_cap = n_out;
  }
  hipLaunchKernelGGL(mg_resample, dim3(blocks_for((size_t)n_out, kT)), dim3(kT), 0, ctx->stream, m.M, m.cw, u0, (long long)n_out, m.idx);
  if (!hip_ok(ctx, hipGetLastError(), "resample launch")) return DH_ERR_HIP;
  m.idx_n = n_out;
  if (idx_out &&
      !hip_ok(ctx, hipMemcpyAsync(idx_out, m.idx, (size_t)n_out * 8, hipMemcpyDeviceToHost, ctx->stream), "D2H idx"))
    return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_merged_gather(dh_ctx* ctx, int64_t n, const int64_t* idx_or_null, double* out_v) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (n < 1 || !out_v || (unsigned long long)n * (unsigned long long)m.ndim >= (1ull << 32))
    return fail(ctx, DH_ERR_ARG, "merged_gather: n %lld (at most 2^32 elements per call)", (long long)n);
  const size_t D = (size_t)m.ndim;
  arena_reset(ctx);
  int rc = arena_reserve(ctx, (size_t)n * (8 * D + 8) + 1024);
  if (rc) return rc;
  const long long* d_idx = m.idx;
  if (idx_or_null) {
    for (int64_t i = 0; i < n; ++i)
      if (idx_or_null[i] < 0 || idx_or_null[i] >= m.M)
        return fail(ctx, DH_ERR_ARG, "merged_gather: index %lld at %lld outside [0, %lld)", (long long)idx_or_null[i], (long long)i, m.M);
    d_idx = (const long long*)arena_up(ctx, (const long long*)idx_or_null, (size_t)n);
    if (!d_idx) return DH_ERR_NOMEM;
  } else if (!m.idx || n > m.idx_n) {
    return fail(ctx, DH_ERR_ARG, "merged_gather: %lld rows asked, the last resample left %lld indices", (long long)n, m.idx_n);
  }
  double* d_out = (double*)arena_get(ctx, (size_t)n * D * 8);
  if (!d_out) return DH_ERR_NOMEM;
  hipLaunchKernelGGL(mg_gather, dim3(blocks_for((size_t)n * D, kT)), dim3(kT), 0, ctx->stream, (size_t)n * D, m.ndim, m.M, m.v, d_idx, d_out);
  if (!hip_ok(ctx, hipGetLastError(), "gather launch") || !down(ctx, out_v, d_out, (size_t)n * D)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_merged_release(dh_ctx* ctx) {
  DH_CHECK_CTX(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  merged_free(ctx);
  return DH_OK;
}

}  // extern "C"

// ---- marginals of the merged run: weighted quantiles, 1-D and 2-D weighted histograms -------
//
// Every sum of weights is a sum of the integers W_i = llrint(w_i 2^62): exact and independent of order, so LDS and
// global 64-bit integer atomics keep the results bitwise reproducible.  A workgroup owns a range of rows and walks
// (row, requested column) pairs in row-major order -- with all columns asked for that is the rows' own layout, read
// coalesced -- and tiles over the requested columns when their tables outgrow its LDS.
namespace {

typedef unsigned long long u64;

constexpr int kMT = 1024;             // threads per workgroup of the passes over the rows
constexpr int kSelTile = 78;          // 256-bin histograms of u64 per workgroup: 156 KB + their states of the CU's 160 KB
constexpr int kHistBins = 16384;      // 64-bit histogram bins per workgroup: 128 KB
constexpr int kMaxCols = 512;         // requested columns per call (the staging tables of the passes)
constexpr int kDigits = 12;           // 8 digits of the value's 64-bit image, 4 of the 32-bit point index
constexpr double kTwo62 = 4611686018427387904.0;

__device__ __forceinline__ u64 weight_int(double w) { return (u64)__double2ll_rn(w * kTwo62); }
// order-preserving image of a double (-0 and +0 are one value, as for a comparison sort)
__device__ __forceinline__ u64 key_of(double x) {
  if (x == 0.0) x = 0.0;
  const u64 b = (u64)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double value_of(u64 k) {
  const u64 b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}

// One (column, q) selection.  The order of a column is (value, point index) ascending = np.argsort(kind="stable");
// the selection walks the digits of that 96-bit image, most significant first.
struct QSel {
  u64 *pk, *cb, *wk, *ti, *succ;  // prefix of the value's image; C before the prefix' range; the last bin; floor(T); successor
  double* frac;                   // T - floor(T)
  unsigned* pi;                   // prefix of the point index
  int* mode;                      // 0: select; 1: the column minimum (q = 0); 2: the maximum (q = 1, T >= Norm)
};

struct QArgs {
  long long M;
  int D, ncol, nq, cpt;  // cpt: columns per tile (cpt * nq <= kSelTile)
  long long rows;        // rows per workgroup
  const double *w, *v, *q;
  const int* cols;
  QSel s;
  u64 *cmin, *cmax, *total, *table;  // per column slot; sum of all W; nsel x 256 bins
  unsigned* last;                    // per column slot: the largest index among the points at the maximum
  int* flags;
  double* out;
};

// minimum and maximum image per requested column, and the sum of all W
__global__ void __launch_bounds__(kMT) mq_minmax(QArgs a) {
  __shared__ u64 mn[kMaxCols], mx[kMaxCols], tot;
  for (int i = threadIdx.x; i < a.ncol; i += kMT) {
    mn[i] = ~0ull;
    mx[i] = 0;
  }
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * a.rows, r1 = r0 + a.rows < a.M ? r0 + a.rows : a.M;
  const unsigned n = (unsigned)(r1 - r0) * (unsigned)a.ncol;
  u64 acc = 0;
  for (unsigned p = threadIdx.x; p < n; p += kMT) {
    const unsigned lr = p / (unsigned)a.ncol, lc = p - lr * (unsigned)a.ncol;
    const u64 key = key_of(a.v[(size_t)(r0 + lr) * a.D + a.cols[lc]]);
    // (the plain reads may be stale; the extremes only move one way, so a stale value costs an atomic, never loses one)
    if (key < mn[lc]) atomicMin(&mn[lc], key);
    if (key > mx[lc]) atomicMax(&mx[lc], key);
    if (lc == 0) acc += weight_int(a.w[r0 + lr]);
  }
  if (acc) atomicAdd(&tot, acc);
  __syncthreads();
  for (int i = threadIdx.x; i < a.ncol; i += kMT) {
    atomicMin(&a.cmin[i], mn[i]);
    atomicMax(&a.cmax[i], mx[i]);
  }
  if (threadIdx.x == 0 && tot) atomicAdd(a.total, tot);
}

// the last point of the stable order: the largest index among the points at the column's maximum
__global__ void __launch_bounds__(kMT) mq_last(QArgs a) {
  const long long r0 = (long long)blockIdx.x * a.rows, r1 = r0 + a.rows < a.M ? r0 + a.rows : a.M;
  const unsigned n = (unsigned)(r1 - r0) * (unsigned)a.ncol;
  for (unsigned p = threadIdx.x; p < n; p += kMT) {
    const unsigned lr = p / (unsigned)a.ncol, lc = p - lr * (unsigned)a.ncol;
    const u64 key = key_of(a.v[(size_t)(r0 + lr) * a.D + a.cols[lc]]);
    if (key == a.cmax[lc]) atomicMax(&a.last[lc], (unsigned)(r0 + lr));
  }
}

// Norm = sum W - W_last (the reference's cumsum(sw)[:-1]); T = q Norm.  Norm = 0 fails the call for a q inside (0, 1) only
__global__ void __launch_bounds__(kT) mq_init(QArgs a) {
  const int s = blockIdx.x * kT + threadIdx.x;
  if (s >= a.ncol * a.nq) return;
  const int slot = s / a.nq;
  const double q = a.q[s - slot * a.nq];
  const u64 norm = a.total[0] - weight_int(a.w[a.last[slot]]);
  if (norm == 0 && q != 0.0 && q != 1.0) a.flags[0] = 1;  // (the extremes do not depend on Norm)
  const double nd = (double)norm, t = q * nd;
  int mode = 0;
  if (q == 0.0) mode = 1;
  else if (q == 1.0 || t >= nd) mode = 2;
  // t < fl(Norm) puts floor(t) below Norm itself, whichever way fl rounded: the selection always finds its point
  const u64 ti = mode ? 0 : (u64)t;
  a.s.pk[s] = 0;
  a.s.pi[s] = 0;
  a.s.cb[s] = 0;
  a.s.wk[s] = 1;
  a.s.ti[s] = ti;
  a.s.frac[s] = mode ? 0.0 : t - (double)ti;
  a.s.succ[s] = ~0ull;
  a.s.mode[s] = mode;
}

// W added to bin `id` of the workgroup's histograms.  kCombine: the lanes of a wavefront that share a bin (the top
// digits of a column hardly vary, and with few columns many lanes hold the same one) are summed in registers first,
// for the four most common bins of the instruction; whatever is left goes to the LDS atomic on its own.
template <bool kCombine>
__device__ __forceinline__ void bin_add(u64* hist, bool on, unsigned id, u64 W) {
  if (kCombine) {
    u64 todo = __ballot(on);
    for (int r = 0; r < 4 && todo; ++r) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned id0 = (unsigned)__shfl((int)id, leader);
      const bool same = on && id == id0;
      u64 sum = same ? W : 0;
      for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[id0], sum);
      todo &= ~__ballot(same);
      on = on && !same;
    }
  }
  if (on) atomicAdd(&hist[id], W);
}

// kSucc = false: digit `pass` of every selection: the W of the points under its prefix, per value of the next digit.
// kSucc = true: the image of the point after the selected one: the smallest image above it, or its own where a point
// of the same value follows it in index order.
template <bool kSucc, bool kCombine>
__global__ void __launch_bounds__(kMT) mq_pass(QArgs a, int pass) {
  extern __shared__ u64 lds[];
  const long long r0 = (long long)blockIdx.x * a.rows, r1 = r0 + a.rows < a.M ? r0 + a.rows : a.M;
  const int nbin = kSucc ? 1 : 256;
  for (int c0 = 0; c0 < a.ncol; c0 += a.cpt) {
    const int nc = a.ncol - c0 < a.cpt ? a.ncol - c0 : a.cpt, ns = nc * a.nq, s0 = c0 * a.nq;
    u64* hist = lds;             // ns x nbin
    u64* spk = lds + ns * nbin;  // ns
    unsigned* spi = (unsigned*)(spk + ns);
    int* son = (int*)(spi + ns);
    int* scol = son + ns;  // nc
    for (int i = threadIdx.x; i < ns * nbin; i += kMT) hist[i] = kSucc ? ~0ull : 0ull;
    for (int i = threadIdx.x; i < ns; i += kMT) {
      spk[i] = a.s.pk[s0 + i];
      spi[i] = a.s.pi[s0 + i];
      son[i] = a.s.mode[s0 + i] == 0;
    }
    for (int i = threadIdx.x; i < nc; i += kMT) scol[i] = a.cols[c0 + i];
    __syncthreads();
    const unsigned n = (unsigned)(r1 - r0) * (unsigned)nc;
    for (unsigned p0 = 0; p0 < n; p0 += kMT) {  // (whole wavefronts stay in the loop: bin_add talks across lanes)
      const unsigned p = p0 + threadIdx.x;
      const bool in = p < n;
      const unsigned lr = in ? p / (unsigned)nc : 0, lc = in ? p - lr * (unsigned)nc : 0;
      const unsigned idx = (unsigned)(r0 + lr);
      const u64 W = weight_int(a.w[idx]);
      const u64 key = key_of(a.v[(size_t)idx * a.D + scol[lc]]);
      for (int qi = 0; qi < a.nq; ++qi) {
        const int s = lc * a.nq + qi;
        const u64 pk = spk[s];
        const unsigned pi = spi[s];
        if (kSucc) {
          if (in && son[s] && (key > pk || (key == pk && idx > pi)) && key < hist[s]) atomicMin(&hist[s], key);
        } else {
          bool on = in && son[s] && W != 0;
          unsigned digit;
          if (pass < 8) {
            const int sh = 64 - 8 * pass;  // bits of the image fixed so far, from the top
            on = on && (pass == 0 || (key >> sh) == (pk >> sh));
            digit = (unsigned)(key >> (sh - 8)) & 255u;
          } else {
            const int sh = 32 - 8 * (pass - 8);
            on = on && key == pk && (pass == 8 || (idx >> sh) == (pi >> sh));
            digit = (idx >> (sh - 8)) & 255u;
          }
          bin_add<kCombine>(hist, on, (unsigned)s * 256u + digit, W);
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ns * nbin; i += kMT) {
      const u64 h = hist[i];
      if (kSucc) {
        if (h != ~0ull) atomicMin(&a.s.succ[s0 + i], h);
      } else if (h) {
        atomicAdd(&a.table[(size_t)s0 * 256 + i], h);
      }
    }
    __syncthreads();
  }
}

// one wavefront per selection: the bin whose range of cumulative weight [C, C + h) holds floor(T) fixes the next digit
// (empty bins have empty ranges and are never chosen); the table is left zeroed for the next pass
__global__ void __launch_bounds__(64) mq_pick(QArgs a, int pass) {
  const int s = blockIdx.x, lane = threadIdx.x;
  u64* bins = a.table + (size_t)s * 256 + 4 * lane;
  u64 h[4], sum = 0;
  for (int j = 0; j < 4; ++j) {
    h[j] = bins[j];
    bins[j] = 0;
    sum += h[j];
  }
  if (a.s.mode[s] != 0) return;  // (uniform over the wavefront)
  u64 inc = sum;
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  u64 lo = a.s.cb[s] + (inc - sum);
  const u64 t = a.s.ti[s];
  for (int j = 0; j < 4; ++j) {
    if (lo <= t && t - lo < h[j]) {
      const unsigned digit = 4u * lane + j;
      if (pass < 8) a.s.pk[s] |= (u64)digit << (56 - 8 * pass);
      else a.s.pi[s] |= digit << (24 - 8 * (pass - 8));
      a.s.cb[s] = lo;
      a.s.wk[s] = h[j];
    }
    lo += h[j];
  }
}

// x_(k) + (T - C_k) / W_(k) (x_(k+1) - x_(k)): np.interp inside its bracket
__global__ void __launch_bounds__(kT) mq_finish(QArgs a) {
  const int s = blockIdx.x * kT + threadIdx.x;
  if (s >= a.ncol * a.nq) return;
  const int slot = s / a.nq, mode = a.s.mode[s];
  double r;
  if (mode == 1) {
    r = value_of(a.cmin[slot]);
  } else if (mode == 2) {
    r = value_of(a.cmax[slot]);
  } else {
    const double x = value_of(a.s.pk[s]);
    const u64 sk = a.s.succ[s];
    const double nx = sk == ~0ull ? x : value_of(sk);
    const double t = ((double)(a.s.ti[s] - a.s.cb[s]) + a.s.frac[s]) / (double)a.s.wk[s];
    r = x + t * (nx - x);
  }
  a.out[s] = r;
}

// the bin of x: the largest i with e[i] <= x; x == e[nb] belongs to the last bin; -1 outside [e[0], e[nb]]
__device__ __forceinline__ int edge_bin(const double* __restrict__ e, int nb, double x) {
  if (!(x >= e[0]) || !(x <= e[nb])) return -1;
  int lo = 0, hi = nb;  // e[lo] <= x throughout
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (e[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo == nb ? nb - 1 : lo;
}

struct HArgs {
  long long M, rows;
  int D, n, per, nbx, nby, weighted;  // n: columns (1-D, nby = 0) or pairs; per: tables per tile of the workgroup's LDS
  const double *w, *v, *xe, *ye;
  const int* cols;  // n columns, or n pairs
  u64* table;       // n x nbx (x nby)
};

template <bool k2D>
__global__ void __launch_bounds__(kMT) mh_hist(HArgs a) {
  extern __shared__ u64 lds[];
  const long long r0 = (long long)blockIdx.x * a.rows, r1 = r0 + a.rows < a.M ? r0 + a.rows : a.M;
  const int nb = k2D ? a.nbx * a.nby : a.nbx;
  for (int c0 = 0; c0 < a.n; c0 += a.per) {
    const int nc = a.n - c0 < a.per ? a.n - c0 : a.per;
    for (int i = threadIdx.x; i < nc * nb; i += kMT) lds[i] = 0;
    __syncthreads();
    const unsigned n = (unsigned)(r1 - r0) * (unsigned)nc;
    for (unsigned p = threadIdx.x; p < n; p += kMT) {
      const unsigned lr = p / (unsigned)nc, lc = p - lr * (unsigned)nc;
      const size_t row = (size_t)(r0 + lr);
      const int c = c0 + (int)lc;
      int bin;
      if (k2D) {
        const int bx = edge_bin(a.xe + (size_t)c * (a.nbx + 1), a.nbx, a.v[row * a.D + a.cols[2 * c]]);
        const int by = edge_bin(a.ye + (size_t)c * (a.nby + 1), a.nby, a.v[row * a.D + a.cols[2 * c + 1]]);
        bin = bx < 0 || by < 0 ? -1 : bx * a.nby + by;
      } else {
        bin = edge_bin(a.xe + (size_t)c * (a.nbx + 1), a.nbx, a.v[row * a.D + a.cols[c]]);
      }
      const u64 W = a.weighted ? weight_int(a.w[row]) : 1ull;
      if (bin >= 0 && W) atomicAdd(&lds[lc * (unsigned)nb + (unsigned)bin], W);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nc * nb; i += kMT)
      if (lds[i]) atomicAdd(&a.table[(size_t)c0 * nb + i], lds[i]);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kT) mh_finish(size_t n, int weighted, const u64* __restrict__ table, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  out[i] = weighted ? ldexp((double)table[i], -62) : (double)table[i];
}

// rows per workgroup: at least 256, at most 2048 workgroups
long long rows_per_group(long long M, unsigned* groups) {
  long long rows = (M + 2047) / 2048;
  if (rows < 256) rows = 256;
  *groups = (unsigned)((M + rows - 1) / rows);
  return rows;
}

template <class K>
bool lds_limit(dh_ctx* ctx, K kernel, size_t bytes) {
  return hip_ok(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), "LDS size");
}

int check_edges(dh_ctx* ctx, const char* what, const double* e, size_t sets, int nb) {
  for (size_t s = 0; s < sets; ++s)
    for (int i = 0; i <= nb; ++i) {
      const double x = e[s * ((size_t)nb + 1) + i];
      if (!(x - x == 0.0) || (i > 0 && x < e[s * ((size_t)nb + 1) + i - 1]))
        return fail(ctx, DH_ERR_ARG, "%s: edge %d of set %zu is not finite or decreases", what, i, s);
    }
  return DH_OK;
}

int run_hist(dh_ctx* ctx, const char* what, bool two, int n, const int32_t* cols, int nbx, int nby, const double* xe,
             const double* ye, int weighted, double* out) {
  const dh_merged& m = ctx->merged;
  const size_t nb = two ? (size_t)nbx * nby : (size_t)nbx, total = (size_t)n * nb;
  const size_t ncol = two ? 2 * (size_t)n : (size_t)n;
  arena_reset(ctx);
  int rc = arena_reserve(ctx, total * 16 + ((size_t)n * ((size_t)nbx + nby + 2)) * 8 + ncol * 4 + 8 * 256);
  if (rc) return rc;
  HArgs a;
  a.M = m.M;
  a.D = m.ndim;
  a.n = n;
  a.nbx = nbx;
  a.nby = two ? nby : 0;
  a.weighted = weighted ? 1 : 0;
  a.per = (int)((size_t)kHistBins / nb);
  if (a.per > 1024) a.per = 1024;  // (rows x tables of a tile are walked with a 32-bit index)
  a.w = m.w;
  a.v = m.v;
  a.cols = arena_up(ctx, (const int*)cols, ncol);
  a.xe = arena_up(ctx, xe, (size_t)n * ((size_t)nbx + 1));
  a.ye = two ? arena_up(ctx, ye, (size_t)n * ((size_t)nby + 1)) : nullptr;
  a.table = (u64*)arena_get(ctx, total * 8);
  double* d_out = (double*)arena_get(ctx, total * 8);
  if (!a.cols || !a.xe || (two && !a.ye) || !a.table || !d_out) return DH_ERR_NOMEM;
  unsigned groups;
  a.rows = rows_per_group(m.M, &groups);
  hipStream_t st = ctx->stream;
  const size_t lds = (size_t)(a.per < n ? a.per : n) * nb * 8;
  if (!hip_ok(ctx, hipMemsetAsync(a.table, 0, total * 8, st), "memset")) return DH_ERR_HIP;
  if (two) {
    if (!lds_limit(ctx, mh_hist<true>, lds)) return DH_ERR_HIP;
    hipLaunchKernelGGL(mh_hist<true>, dim3(groups), dim3(kMT), lds, st, a);
  } else {
    if (!lds_limit(ctx, mh_hist<false>, lds)) return DH_ERR_HIP;
    hipLaunchKernelGGL(mh_hist<false>, dim3(groups), dim3(kMT), lds, st, a);
  }
  hipLaunchKernelGGL(mh_finish, dim3(blocks_for(total, kT)), dim3(kT), 0, st, total, a.weighted, a.table, d_out);
  if (!hip_ok(ctx, hipGetLastError(), what) || !down(ctx, out, d_out, total)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

}  // namespace

extern "C" {

int dh_merged_quantile(dh_ctx* ctx, int nq, const double* q, int ncol, const int32_t* cols_or_null, double* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (nq < 1 || nq > 16 || !q || !out || ncol < 1 || ncol > kMaxCols || (!cols_or_null && ncol != m.ndim))
    return fail(ctx, DH_ERR_ARG, "merged_quantile: nq %d (1 to 16), ncol %d (1 to %d; ndim without a column list)", nq, ncol, kMaxCols);
  for (int i = 0; i < nq; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(ctx, DH_ERR_ARG, "merged_quantile: q[%d] = %g outside [0, 1]", i, q[i]);
  std::vector<int> cols((size_t)ncol);
  for (int i = 0; i < ncol; ++i) {
    cols[(size_t)i] = cols_or_null ? cols_or_null[i] : i;
    if (cols[(size_t)i] < 0 || cols[(size_t)i] >= m.ndim)
      return fail(ctx, DH_ERR_ARG, "merged_quantile: column %d outside [0, %d)", cols[(size_t)i], m.ndim);
  }
  const size_t S = (size_t)ncol * nq;
  arena_reset(ctx);
  int rc = arena_reserve(ctx, S * (256 * 8 + 64) + (size_t)ncol * 32 + 32 * 256);
  if (rc) return rc;
  QArgs a;
  a.M = m.M;
  a.D = m.ndim;
  a.ncol = ncol;
  a.nq = nq;
  a.cpt = kSelTile / nq;
  a.w = m.w;
  a.v = m.v;
  a.q = arena_up(ctx, q, (size_t)nq);
  a.cols = arena_up(ctx, cols.data(), (size_t)ncol);
  // one zeroed block: table, total, cmax, last, flags; then what the kernels initialise themselves
  const size_t zero_bytes = S * 256 * 8 + 8 + (size_t)ncol * 8 + ((size_t)ncol + 1) * 4 + 16;
  char* z = (char*)arena_get(ctx, zero_bytes);
  a.cmin = (u64*)arena_get(ctx, (size_t)ncol * 8);
  a.s.pk = (u64*)arena_get(ctx, S * 8);
  a.s.cb = (u64*)arena_get(ctx, S * 8);
  a.s.wk = (u64*)arena_get(ctx, S * 8);
  a.s.ti = (u64*)arena_get(ctx, S * 8);
  a.s.succ = (u64*)arena_get(ctx, S * 8);
  a.s.frac = (double*)arena_get(ctx, S * 8);
  a.s.pi = (unsigned*)arena_get(ctx, S * 4);
  a.s.mode = (int*)arena_get(ctx, S * 4);
  a.out = (double*)arena_get(ctx, S * 8);
  if (!a.q || !a.cols || !z || !a.cmin || !a.s.pk || !a.s.cb || !a.s.wk || !a.s.ti || !a.s.succ || !a.s.frac || !a.s.pi ||
      !a.s.mode || !a.out)
    return DH_ERR_NOMEM;
  a.table = (u64*)z;
  a.total = a.table + S * 256;
  a.cmax = a.total + 1;
  a.last = (unsigned*)(a.cmax + ncol);
  a.flags = (int*)(a.last + ncol + (ncol & 1));
  unsigned groups;
  a.rows = rows_per_group(m.M, &groups);
  hipStream_t st = ctx->stream;
  const int tile_cols = a.cpt < ncol ? a.cpt : ncol, tile_sel = tile_cols * nq;
  const size_t lds_digit = (size_t)tile_sel * (256 * 8 + 16) + (size_t)tile_cols * 4;
  const size_t lds_succ = (size_t)tile_sel * (8 + 16) + (size_t)tile_cols * 4;
  const bool combine = tile_cols < 16;  // 64 / columns lanes of a wavefront share a column
  if (!hip_ok(ctx, hipMemsetAsync(z, 0, zero_bytes, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(a.cmin, 0xff, (size_t)ncol * 8, st), "memset") ||
      !lds_limit(ctx, mq_pass<false, false>, lds_digit) || !lds_limit(ctx, mq_pass<false, true>, lds_digit))
    return DH_ERR_HIP;
  hipLaunchKernelGGL(mq_minmax, dim3(groups), dim3(kMT), 0, st, a);
  hipLaunchKernelGGL(mq_last, dim3(groups), dim3(kMT), 0, st, a);
  hipLaunchKernelGGL(mq_init, dim3(blocks_for(S, kT)), dim3(kT), 0, st, a);
  for (int pass = 0; pass < kDigits; ++pass) {
    if (combine)
      hipLaunchKernelGGL((mq_pass<false, true>), dim3(groups), dim3(kMT), lds_digit, st, a, pass);
    else
      hipLaunchKernelGGL((mq_pass<false, false>), dim3(groups), dim3(kMT), lds_digit, st, a, pass);
    hipLaunchKernelGGL(mq_pick, dim3((unsigned)S), dim3(64), 0, st, a, pass);
  }
  hipLaunchKernelGGL((mq_pass<true, false>), dim3(groups), dim3(kMT), lds_succ, st, a, kDigits);
  hipLaunchKernelGGL(mq_finish, dim3(blocks_for(S, kT)), dim3(kT), 0, st, a);
  int flags[4] = {0, 0, 0, 0};
  if (!hip_ok(ctx, hipGetLastError(), "quantile launch") || !down(ctx, out, a.out, S) ||
      !hip_ok(ctx, hipMemcpyAsync(flags, a.flags, sizeof flags, hipMemcpyDeviceToHost, st), "D2H"))
    return DH_ERR_HIP;
  rc = dh_sync(ctx);
  if (rc) return rc;
  if (flags[0]) return fail(ctx, DH_ERR_VALUE, "merged_quantile: all weight of a column sits on its last point (the reference divides by zero)");
  return DH_OK;
}

int dh_merged_hist1d(dh_ctx* ctx, int ncol, const int32_t* cols_or_null, int nbins, const double* edges, int weighted,
                     double* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (ncol < 1 || ncol > kMaxCols || nbins < 1 || nbins > 4096 || !edges || !out || (!cols_or_null && ncol != m.ndim))
    return fail(ctx, DH_ERR_ARG, "merged_hist1d: ncol %d (1 to %d; ndim without a column list), nbins %d (1 to 4096)", ncol, kMaxCols, nbins);
  std::vector<int> cols((size_t)ncol);
  for (int i = 0; i < ncol; ++i) {
    cols[(size_t)i] = cols_or_null ? cols_or_null[i] : i;
    if (cols[(size_t)i] < 0 || cols[(size_t)i] >= m.ndim)
      return fail(ctx, DH_ERR_ARG, "merged_hist1d: column %d outside [0, %d)", cols[(size_t)i], m.ndim);
  }
  if (check_edges(ctx, "merged_hist1d", edges, (size_t)ncol, nbins)) return DH_ERR_ARG;
  return run_hist(ctx, "hist1d launch", false, ncol, cols.data(), nbins, 0, edges, nullptr, weighted, out);
}

int dh_merged_hist2d(dh_ctx* ctx, int npair, const int32_t* pairs, int nbx, int nby, const double* xedges,
                     const double* yedges, int weighted, double* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (npair < 1 || npair > 65536 || !pairs || nbx < 1 || nby < 1 || (long long)nbx * nby > kHistBins || !xedges || !yedges || !out)
    return fail(ctx, DH_ERR_ARG, "merged_hist2d: npair %d (1 to 65536), %d x %d bins (at most %d per pair)", npair, nbx, nby, kHistBins);
  for (int i = 0; i < 2 * npair; ++i)
    if (pairs[i] < 0 || pairs[i] >= m.ndim)
      return fail(ctx, DH_ERR_ARG, "merged_hist2d: column %d outside [0, %d)", pairs[i], m.ndim);
  if (check_edges(ctx, "merged_hist2d (x)", xedges, (size_t)npair, nbx) || check_edges(ctx, "merged_hist2d (y)", yedges, (size_t)npair, nby))
    return DH_ERR_ARG;
  return run_hist(ctx, "hist2d launch", true, npair, pairs, nbx, nby, xedges, yedges, weighted, out);
}

}  // extern "C"

// ---- statistical errors of the merged run: volume-jitter realizations and reweighting -----
//
// Realization r (a global index) of the prior-volume sequence: point k shrinks the volume by t_k = u_k^(1 / n_k), its
// step is s_k = log(u_k) / n_k, with u_k = uniform_double of words 2k and 2k + 1 of subsequence r of the Philox4x32-10
// stream keyed by `seed` (utils.jitter_run, utils.py:1317-1408; tests/philox_ref.py restates the words).  jitter = 0
// takes the merged run's own expected step -log1p(1 / n_k) (with logrwt: utils.reweight_run, utils.py:1663-1708).
// The integrals are utils.compute_integrals' (utils.py:1411-1467) in the arithmetic of the scans above.
//
// A batch never holds a (realization x point) array: the words are a function of (seed, r, k), so each pass makes its
// steps again.  me_step_sums: per-chunk sums of the steps; me_step_carry: their exclusive scan over the chunks;
// me_integrate: ln X, ln w and the chunk's sums of w, w^2, the information's terms and w v, each scaled by the chunk's
// own largest term; me_finish: the chunks' sums in chunk order, rescaled to the largest chunk.  A workgroup loads its
// chunk's n, ln L, logaddexp(l_k, l_{k-1}) and logrwt once and carries kRealTile realizations through it.  Every
// reduction has a fixed order and a realization's numbers depend on (seed, r) alone: it comes out bit-identical alone,
// in any batch, at any position.
namespace {

constexpr int kRealTile = 4;         // realizations a workgroup carries through its chunk
constexpr int kRealLaunch = 64;      // realizations per set of launches: the scratch is chunks x 64 x (6 + D) doubles
constexpr int kRealMax = 65536;      // realizations per call
constexpr int kSeg = kChunk / kT;    // a chunk's mean sums: kSeg segments of kT points, summed in segment order
constexpr int kColTile = kT / kSeg;  // columns per step of the mean sums
constexpr int kMeanLoads = 16;       // rows of v a thread of the mean sums has in flight
constexpr int kFinLoads = 8;         // chunks a thread of me_finish has in flight
constexpr int kPart = 5;             // per (realization, chunk): max ln w, max ln w without logrwt, sum w, sum w^2, sum of H's terms
constexpr double kLnHalf = -0.6931471805599453;

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
__device__ __forceinline__ double expected_step(int n) { return -log1p(1.0 / (double)n); }

// the steps of the points k0 .. k0 + kItems - 1 (k0 a multiple of kItems: whole Philox blocks)
__device__ __forceinline__ void real_steps(int jitter, uint64_t seed, uint64_t seq, long long k0, const int* n, double* s) {
  if (jitter) {
#pragma unroll
    for (int j = 0; j < kItems; j += 2) {
      uint32_t w[4];
      philox4x32_10(seed, seq, (uint64_t)(k0 + j) >> 1, w);
      s[j] = log(uniform_double(w[0], w[1])) / (double)n[j];
      s[j + 1] = log(uniform_double(w[2], w[3])) / (double)n[j + 1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kItems; ++j) s[j] = expected_step(n[j]);
  }
}
// one point's step (the per-point fields of one realization)
__device__ __forceinline__ double real_step(int jitter, uint64_t seed, uint64_t seq, long long k, int n) {
  if (!jitter) return expected_step(n);
  uint32_t w[4];
  philox4x32_10(seed, seq, (uint64_t)k >> 1, w);
  const bool odd = k & 1;
  return log(uniform_double(odd ? w[2] : w[0], odd ? w[3] : w[1])) / (double)n;
}

struct Pair2 {
  double a, b;
};
struct Max2 {
  typedef Pair2 T;
  __device__ static T id() { return T{-INFINITY, -INFINITY}; }
  __device__ static T op(T x, T y) { return T{fmax(x.a, y.a), fmax(x.b, y.b)}; }
};
struct Trip {
  double a, b, c;
};
struct Sum3 {
  typedef Trip T;
  __device__ static T id() { return T{0.0, 0.0, 0.0}; }
  __device__ static T op(T x, T y) { return T{x.a + y.a, x.b + y.b, x.c + y.c}; }
};

struct RArgs {
  long long M, first;  // points; global index of this launch set's realization 0
  int D, nblk, nreal, jitter, want_mean;
  uint64_t seed;
  const double *logl, *lae, *rwt, *v;  // rwt: null without logrwt
  const int* n;
  const int* map;  // me_integrate<true> (the strand bootstrap): point k reads logl and v at map[k]; n and lae are per k
  double *sums, *part, *mpart, *out;  // [nreal][nblk], [nreal][nblk][kPart], [nreal][nblk][D], [nreal][3 + D]
  // the divergence (me_integrate<., true>, me_finish<true>): the merged run's own ln w (read through map) and its last
  // cumulative ln Z; the chunks' sums of w (ln w - LOGWT) [nreal][nblk].  The result takes the row's first mean slot.
  const double *lwt0 = nullptr, *lz0 = nullptr;
  double* kpart = nullptr;
};

__global__ void __launch_bounds__(kT) me_lae(long long M, const double* __restrict__ logl, double* __restrict__ lae) {
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  lae[k] = logaddexp_np(logl[k], k > 0 ? logl[k - 1] : -1.e300);
}

// a thread's kItems live counts; past the end the last point's (a clamped load: the step is masked where it is used)
__device__ __forceinline__ void load_counts(const RArgs& a, long long k0, int* n) {
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const long long k = k0 + j < a.M ? k0 + j : a.M - 1;
    n[j] = a.n[k];
  }
}

__global__ void __launch_bounds__(kT) me_step_sums(RArgs a) {
  __shared__ double lds[2 * kT];
  const long long k0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kItems;
  int n[kItems];
  load_counts(a, k0, n);
  const int b0 = blockIdx.y * kRealTile, nb = a.nreal - b0 < kRealTile ? a.nreal - b0 : kRealTile;
  for (int b = 0; b < nb; ++b) {
    double s[kItems];
    real_steps(a.jitter, a.seed, (uint64_t)(a.first + b0 + b), k0, n, s);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) acc += k0 + j < a.M ? s[j] : 0.0;
    double ex, tot;
    block_scan<SumD>(acc, lds, &ex, &tot);
    if (threadIdx.x == 0) a.sums[(size_t)(b0 + b) * a.nblk + blockIdx.x] = tot;
  }
}

// workgroup b: sums[b][c] becomes the sum of the chunks before c (scan_carry's order)
__global__ void __launch_bounds__(kT) me_step_carry(RArgs a) {
  __shared__ double lds[2 * kT];
  double* part = a.sums + (size_t)blockIdx.x * a.nblk;
  double carry = 0.0;
  for (int c0 = 0; c0 < a.nblk; c0 += kT) {
    const int c = c0 + threadIdx.x;
    const double v = c < a.nblk ? part[c] : 0.0;
    double ex, tot;
    block_scan<SumD>(v, lds, &ex, &tot);
    if (c < a.nblk) part[c] = carry + ex;
    carry = carry + tot;
  }
}

// dynamic LDS: the scans' 2 kT Trip; with means kRealTile x kChunk weights and kSeg x kRealTile x kColTile partial sums
// kMap: logl and the rows of v are read through a.map (the unmapped instantiation is the code it was before the map)
// kKld: beside sum w the chunk's sum of w e, e = ln w - LOGWT_src, rescaled as sum w is: me_finish<true> turns the two into
// the divergence from the merged run without any pass knowing ln Z (the instantiations without it keep their code)
template <bool kMap, bool kKld>
__global__ void __launch_bounds__(kT) me_integrate(RArgs a) {
  extern __shared__ double dyn[];
  double* wl = dyn + 2 * kT * 3;
  double* mp = wl + kRealTile * kChunk;
  const int t = threadIdx.x;
  const long long kb = (long long)blockIdx.x * kChunk, k0 = kb + (long long)t * kItems;
  int n[kItems];
  double l[kItems + 1], lae[kItems], rw[kItems];
  load_counts(a, k0, n);
  {
    const long long km = k0 > 0 ? (k0 - 1 < a.M ? k0 - 1 : a.M - 1) : 0;
    const double lm = a.logl[kMap ? (long long)a.map[km] : km];
    l[0] = k0 > 0 ? lm : -1.e300;
  }
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const long long k = k0 + j < a.M ? k0 + j : a.M - 1;
    l[j + 1] = a.logl[kMap ? (long long)a.map[k] : k];
    lae[j] = a.lae[k];
    rw[j] = 0.0;
  }
  double lq[kKld ? kItems : 1];
  if constexpr (kKld) {
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const long long k = k0 + j < a.M ? k0 + j : a.M - 1;
      lq[j] = a.lwt0[kMap ? (long long)a.map[k] : k];
    }
  }
  if (a.rwt) {
#pragma unroll
    for (int j = 0; j < kItems; ++j) rw[j] = a.rwt[k0 + j < a.M ? k0 + j : a.M - 1];
  }
  const int b0 = blockIdx.y * kRealTile, nb = a.nreal - b0 < kRealTile ? a.nreal - b0 : kRealTile;
  for (int b = 0; b < nb; ++b) {
    double s[kItems];
    real_steps(a.jitter, a.seed, (uint64_t)(a.first + b0 + b), k0, n, s);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      s[j] = k0 + j < a.M ? s[j] : 0.0;  // (a step of 0 is a weight of 0: the points past the end add nothing)
      acc += s[j];
    }
    double ex, tot;
    block_scan<SumD>(acc, dyn, &ex, &tot);
    double run = a.sums[(size_t)(b0 + b) * a.nblk + blockIdx.x] + ex;  // ln X of the point before k0
    double ldv[kItems], lw[kItems];
    Pair2 mx = Max2::id();
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      ldv[j] = run + log(-expm1(s[j])) + kLnHalf;  // ln (X_{k-1} - X_k) / 2; s = 0: -inf
      run = run + s[j];
      const double lh = lae[j] + ldv[j];
      lw[j] = lh + rw[j];
      mx = Max2::op(mx, Pair2{lw[j], lh});
    }
    Pair2 mex, mtot;
    block_scan<Max2>(mx, (Pair2*)dyn, &mex, &mtot);
    const double mref = mtot.a == -INFINITY ? 0.0 : mtot.a, href = mtot.b == -INFINITY ? 0.0 : mtot.b;
    Trip sum = Sum3::id();
    double sume = 0.0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const double w = exp(lw[j] - mref);
      if constexpr (kKld) sume += w > 0 ? w * (lw[j] - lq[j]) : 0.0;  // (w = 0: nothing, also where e is inf - inf)
      const double w0 = exp(l[j] - href + ldv[j]), w1 = exp(l[j + 1] - href + ldv[j]);
      sum.a += w;
      sum.b = fma(w, w, sum.b);
      sum.c += (w0 > 0 ? w0 * l[j] : 0.0) + (w1 > 0 ? w1 * l[j + 1] : 0.0);
      if (a.want_mean) wl[b * kChunk + t * kItems + j] = w;
    }
    Trip sex, stot;
    block_scan<Sum3>(sum, (Trip*)dyn, &sex, &stot);
    if (t == 0) {
      double* p = a.part + ((size_t)(b0 + b) * a.nblk + blockIdx.x) * kPart;
      p[0] = mtot.a;
      p[1] = mtot.b;
      p[2] = stot.a;
      p[3] = stot.b;
      p[4] = stot.c;
    }
    if constexpr (kKld) {  // (a scan of its own: one of four doubles in place of Sum3's measured slower)
      double eex, etot;
      block_scan<SumD>(sume, dyn, &eex, &etot);
      if (t == 0) a.kpart[(size_t)(b0 + b) * a.nblk + blockIdx.x] = etot;
    }
  }
  if (!a.want_mean) return;
  __syncthreads();
  // sum w v_c of the chunk: thread (segment, column) adds its kT points in order for the tile's realizations (one load
  // of v serves them all), then the segments are added in order
  const int seg = t / kColTile, cc = t % kColTile;
  for (int c0 = 0; c0 < a.D; c0 += kColTile) {
    const int c = c0 + cc < a.D ? c0 + cc : a.D - 1;
    double acc[kRealTile];
#pragma unroll
    for (int b = 0; b < kRealTile; ++b) acc[b] = 0.0;
    for (int i0 = 0; i0 < kT; i0 += kMeanLoads) {  // (kMeanLoads rows in flight: the sums keep their order)
      double x[kMeanLoads];
#pragma unroll
      for (int i = 0; i < kMeanLoads; ++i) {
        const int p = seg * kT + i0 + i;
        const long long k = kb + p < a.M ? kb + p : a.M - 1;
        x[i] = a.v[(size_t)(kMap ? (long long)a.map[k] : k) * a.D + c];
      }
#pragma unroll
      for (int i = 0; i < kMeanLoads; ++i) {
#pragma unroll
        for (int b = 0; b < kRealTile; ++b) acc[b] = fma(wl[b * kChunk + seg * kT + i0 + i], x[i], acc[b]);
      }
    }
#pragma unroll
    for (int b = 0; b < kRealTile; ++b) mp[(seg * kRealTile + b) * kColTile + cc] = acc[b];
    __syncthreads();
    if (t < kRealTile * kColTile) {
      const int b = t / kColTile;
      double tot = 0.0;
      for (int g = 0; g < kSeg; ++g) tot += mp[(g * kRealTile + b) * kColTile + cc];
      if (b < nb && c0 + cc < a.D) a.mpart[((size_t)(b0 + b) * a.nblk + blockIdx.x) * a.D + c0 + cc] = tot;
    }
    __syncthreads();
  }
}

// workgroup b: out[b] = {ln Z, H, ESS, mean_0 ..}: the chunks' sums in chunk order, each rescaled to the largest chunk
// kKld (never with means): out[b][3] = (sum w' e) / (sum w') - (ln Z - LOGZ_{M-1}), the sum of kpart scaled as sum w' is
template <bool kKld>
__global__ void __launch_bounds__(kT) me_finish(RArgs a) {
  __shared__ Pair2 lds[2 * kT];
  __shared__ double res[3];
  const int t = threadIdx.x;
  const double* part = a.part + (size_t)blockIdx.x * a.nblk * kPart;
  Pair2 mx = Max2::id();
  for (int c = t; c < a.nblk; c += kT) mx = Max2::op(mx, Pair2{part[(size_t)c * kPart], part[(size_t)c * kPart + 1]});
  Pair2 mex, mtot;
  block_scan<Max2>(mx, lds, &mex, &mtot);
  const double ms = mtot.a, hs = mtot.b;
  const int nq = kKld ? 4 : 3 + (a.want_mean ? a.D : 0);
  double* out = a.out + (size_t)blockIdx.x * (3 + a.D);
  for (int q0 = 0; q0 < nq; q0 += kT) {
    const int q = q0 + t;
    double acc = 0.0;
    if (q < nq) {
      const double* mcol = a.want_mean ? a.mpart + (size_t)blockIdx.x * a.nblk * a.D + (q >= 3 ? q - 3 : 0) : nullptr;
      const int mi = q == 2 ? 1 : 0;
      const double top = q == 2 ? hs : ms;
      const double* xs = q < 3 ? part + 2 + q : mcol;  // the chunks' sums of this quantity, xd apart
      size_t xd = q < 3 ? kPart : (size_t)a.D;
      if constexpr (kKld) {
        if (q == 3) {
          xs = a.kpart + (size_t)blockIdx.x * a.nblk;
          xd = 1;
        }
      }
      for (int c0 = 0; c0 < a.nblk; c0 += kFinLoads) {  // (kFinLoads chunks in flight, added in chunk order)
        double m[kFinLoads], x[kFinLoads];
#pragma unroll
        for (int i = 0; i < kFinLoads; ++i) {
          const size_t c = (size_t)(c0 + i < a.nblk ? c0 + i : a.nblk - 1);
          m[i] = part[c * kPart + mi];
          x[i] = xs[c * xd];
        }
#pragma unroll
        for (int i = 0; i < kFinLoads; ++i) {
          const double sc = m[i] == -INFINITY || c0 + i >= a.nblk ? 0.0 : exp(q == 1 ? 2.0 * (m[i] - top) : m[i] - top);
          if constexpr (kKld)
            acc = sc > 0 ? fma(sc, x[i], acc) : acc;  // (a chunk scaled to 0 adds nothing, also where its sum is inf)
          else
            acc = fma(sc, x[i], acc);
        }
      }
    }
    if (q < 3) res[q] = acc;
    __syncthreads();
    const double lz = ms + log(res[0]);
    if (q == 0) out[0] = lz;
    if (q == 1) out[2] = res[0] * res[0] / res[1];
    if (q == 2) out[1] = exp(hs - lz) * res[2] - lz;
    if constexpr (kKld) {
      if (q == 3) out[3] = acc / res[0] - (lz - a.lz0[0]);
    } else {
      if (q >= 3 && q < nq) out[q] = acc / res[0];
    }
  }
}

// the per-point fields of one realization through the scans above
struct FRealVol {
  typedef SumD Op;
  const int* n;
  double *step, *logvol;
  uint64_t seed, seq;
  int jitter;
  __device__ double term(long long k) const {
    const double s = real_step(jitter, seed, seq, k, n[k]);
    step[k] = s;
    return s;
  }
  __device__ void put(long long k, double incl, double) const { logvol[k] = incl; }
};
struct FRealLogz {
  typedef Lse Op;
  const double *lae, *rwt, *logvol, *step;
  double *logwt, *logz;
  __device__ LsePair term(long long k) const {
    const double v0 = k > 0 ? logvol[k - 1] : 0.0, s = step[k];
    const double lh = lae[k] + (v0 + log(-expm1(s)) + kLnHalf);
    const double lw = lh + (rwt ? rwt[k] : 0.0);
    logwt[k] = lw;
    return LsePair{lw, 1.0};
  }
  __device__ void put(long long k, LsePair incl, LsePair) const { logz[k] = incl.m + log(incl.s); }
};

// the cumulative divergence of one realization from the merged run, after FRealLogz: term p =
// exp(lw_p - Z) ((lw_p - LOGWT_src(p)) - (Z - LOGZ_{M-1})), Z the last cumulative ln Z the scan before wrote
struct FRealKld {
  typedef SumD Op;
  const double *logwt, *logz, *lwt0, *lz0;
  const int* map;  // null: src(p) = p
  double* kld;
  long long M;
  __device__ double term(long long k) const {
    const double lz = logz[M - 1], lw = logwt[k];
    const double p = exp(lw - lz);
    return p > 0 ? p * ((lw - lwt0[map ? (long long)map[k] : k]) - (lz - lz0[0])) : 0.0;
  }
  __device__ void put(long long k, double incl, double) const { kld[k] = incl; }
};

// logrwt: NaN and +inf are refused (-inf is a weight of 0)
int check_logrwt(dh_ctx* ctx, const char* what, const double* rwt, long long M) {
  if (!rwt) return DH_OK;
  for (long long k = 0; k < M; ++k)
    if (!(rwt[k] < INFINITY)) return fail(ctx, DH_ERR_VALUE, "%s: logrwt[%lld] = %g (NaN and +inf are not weights)", what, k, rwt[k]);
  return DH_OK;
}

// dh_merged_realize after its argument checks; kld (or null): the realizations' divergence from the merged run too
// (dh_merged_kld), through the instantiation of me_integrate that sums it
int realize_core(dh_ctx* ctx, uint64_t seed, int64_t first, int nreal, int jitter, const double* logrwt_or_null, int want_mean,
                 double* logz, double* h, double* ess, double* mean, double* kld) {
  const dh_merged& m = ctx->merged;
  int rc;
  const size_t M = (size_t)m.M, D = (size_t)m.ndim, nblk = blocks_for(M, kChunk);
  const size_t tile = (size_t)(nreal < kRealLaunch ? nreal : kRealLaunch), W = 3 + D;
  arena_reset(ctx);
  rc = arena_reserve(ctx, (M * 2 + tile * nblk * (1 + kPart + (want_mean ? D : 0) + (kld ? 1 : 0)) +
                           (size_t)nreal * W) * 8 + 18 * 256);
  if (rc) return rc;
  RArgs a;
  a.M = m.M;
  a.D = m.ndim;
  a.nblk = (int)nblk;
  a.jitter = jitter;
  a.want_mean = want_mean ? 1 : 0;
  a.seed = seed;
  a.logl = m.logl;
  a.v = m.v;
  a.n = m.n;
  a.map = nullptr;
  double* lae = (double*)arena_get(ctx, M * 8);
  a.rwt = logrwt_or_null ? arena_up(ctx, logrwt_or_null, M) : nullptr;
  a.sums = (double*)arena_get(ctx, tile * nblk * 8);
  a.part = (double*)arena_get(ctx, tile * nblk * kPart * 8);
  a.mpart = want_mean ? (double*)arena_get(ctx, tile * nblk * D * 8) : nullptr;
  double* d_out = (double*)arena_get(ctx, (size_t)nreal * W * 8);
  if (!lae || (logrwt_or_null && !a.rwt) || !a.sums || !a.part || (want_mean && !a.mpart) || !d_out) return DH_ERR_NOMEM;
  if (kld) {
    a.kpart = (double*)arena_get(ctx, tile * nblk * 8);
    if (!a.kpart) return DH_ERR_NOMEM;
    a.lwt0 = m.logwt;
    a.lz0 = m.logz + (M - 1);
  }
  a.lae = lae;
  hipStream_t st = ctx->stream;
  const size_t lds = (size_t)(2 * kT * 3 + (want_mean ? kRealTile * kChunk + kSeg * kRealTile * kColTile : 0)) * 8;
  if (!(kld ? lds_limit(ctx, me_integrate<false, true>, lds) : lds_limit(ctx, me_integrate<false, false>, lds))) return DH_ERR_HIP;
  hipLaunchKernelGGL(me_lae, dim3(blocks_for(M, kT)), dim3(kT), 0, st, m.M, m.logl, lae);
  for (int r0 = 0; r0 < nreal; r0 += kRealLaunch) {
    a.nreal = nreal - r0 < kRealLaunch ? nreal - r0 : kRealLaunch;
    a.first = (long long)first + r0;
    a.out = d_out + (size_t)r0 * W;
    const dim3 grid((unsigned)nblk, blocks_for((size_t)a.nreal, kRealTile));
    hipLaunchKernelGGL(me_step_sums, grid, dim3(kT), 0, st, a);
    hipLaunchKernelGGL(me_step_carry, dim3(a.nreal), dim3(kT), 0, st, a);
    if (kld) {
      hipLaunchKernelGGL((me_integrate<false, true>), grid, dim3(kT), lds, st, a);
      hipLaunchKernelGGL(me_finish<true>, dim3(a.nreal), dim3(kT), 0, st, a);
    } else {
      hipLaunchKernelGGL((me_integrate<false, false>), grid, dim3(kT), lds, st, a);
      hipLaunchKernelGGL(me_finish<false>, dim3(a.nreal), dim3(kT), 0, st, a);
    }
  }
  if (!hip_ok(ctx, hipGetLastError(), "realize launch")) return DH_ERR_HIP;
  std::vector<double> host((size_t)nreal * W);
  if (!down(ctx, host.data(), (const double*)d_out, host.size())) return DH_ERR_HIP;
  rc = dh_sync(ctx);
  if (rc) return rc;
  for (size_t b = 0; b < (size_t)nreal; ++b) {
    logz[b] = host[b * W];
    if (h) h[b] = host[b * W + 1];
    if (ess) ess[b] = host[b * W + 2];
    if (mean)
      for (size_t c = 0; c < D; ++c) mean[b * D + c] = host[b * W + 3 + c];
    if (kld) kld[b] = host[b * W + 3];
  }
  return DH_OK;
}

}  // namespace

extern "C" {

int dh_merged_realize(dh_ctx* ctx, uint64_t seed, int64_t first, int nreal, int jitter, const double* logrwt_or_null,
                      int want_mean, double* logz, double* h, double* ess, double* mean) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (nreal < 1 || nreal > kRealMax || (jitter != 0 && jitter != 1) || (!jitter && nreal != 1) || first < 0 ||
      first > INT64_MAX - nreal || !logz || (!!want_mean != !!mean))
    return fail(ctx, DH_ERR_ARG,
                "merged_realize: nreal %d (1 to %d; 1 with jitter = 0), jitter %d (0 or 1), first %lld (>= 0), logz, and "
                "want_mean with mean", nreal, kRealMax, jitter, (long long)first);
  const int rc = check_logrwt(ctx, "merged_realize", logrwt_or_null, m.M);
  if (rc) return rc;
  return realize_core(ctx, seed, first, nreal, jitter, logrwt_or_null, want_mean, logz, h, ess, mean, nullptr);
}

int dh_merged_realization(dh_ctx* ctx, uint64_t seed, int64_t real, int jitter, const double* logrwt_or_null, int field,
                          int64_t first, int64_t count, double* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (real < 0 || (jitter != 0 && jitter != 1) ||
      (field != DH_MERGED_LOGVOL && field != DH_MERGED_LOGWT && field != DH_MERGED_LOGZ && field != DH_MERGED_KLD) ||
      (field == DH_MERGED_KLD && logrwt_or_null))
    return fail(ctx, DH_ERR_ARG, "merged_realization: real %lld (>= 0), jitter %d (0 or 1), field %d (LOGVOL, LOGWT, LOGZ, or "
                "KLD without logrwt)", (long long)real, jitter, field);
  if (first < 0 || count < 0 || first > m.M || count > m.M - first || (count && !out))
    return fail(ctx, DH_ERR_ARG, "merged_realization: [%lld, %lld + %lld) of %lld points", (long long)first, (long long)first,
                (long long)count, m.M);
  int rc = check_logrwt(ctx, "merged_realization", logrwt_or_null, m.M);
  if (rc) return rc;
  if (!count) return DH_OK;
  const size_t M = (size_t)m.M, nblk = blocks_for(M, kChunk);
  arena_reset(ctx);
  rc = arena_reserve(ctx, M * 7 * 8 + (nblk + 1) * sizeof(LsePair) + 18 * 256);
  if (rc) return rc;
  double* lae = (double*)arena_get(ctx, M * 8);
  const double* rwt = logrwt_or_null ? arena_up(ctx, logrwt_or_null, M) : nullptr;
  double* step = (double*)arena_get(ctx, M * 8);
  double* logvol = (double*)arena_get(ctx, M * 8);
  double* logwt = (double*)arena_get(ctx, M * 8);
  double* logz = (double*)arena_get(ctx, M * 8);
  void* part = arena_get(ctx, (nblk + 1) * sizeof(LsePair));
  double* kld = field == DH_MERGED_KLD ? (double*)arena_get(ctx, M * 8) : logz;
  if (!lae || (logrwt_or_null && !rwt) || !step || !logvol || !logwt || !logz || !part || !kld) return DH_ERR_NOMEM;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(me_lae, dim3(blocks_for(M, kT)), dim3(kT), 0, st, m.M, m.logl, lae);
  if (!run_scan(ctx, FRealVol{m.n, step, logvol, seed, (uint64_t)real, jitter}, m.M, part)) return DH_ERR_HIP;
  if (field != DH_MERGED_LOGVOL &&
      !run_scan(ctx, FRealLogz{lae, rwt, logvol, step, logwt, logz}, m.M, part))
    return DH_ERR_HIP;
  if (field == DH_MERGED_KLD &&
      !run_scan(ctx, FRealKld{logwt, logz, m.logwt, m.logz + (M - 1), nullptr, kld, m.M}, m.M, part))
    return DH_ERR_HIP;
  const double* src = field == DH_MERGED_LOGVOL ? logvol : field == DH_MERGED_LOGWT ? logwt : field == DH_MERGED_KLD ? kld : logz;
  if (!down(ctx, out, src + first, (size_t)count)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

}  // extern "C"

// ---- the strand bootstrap of the merged run (utils.resample_run, utils.py:1495-1660) ---------
//
// A strand is a (run, live slot) pair, its key run * nlive + slot.  Bootstrap b draws S = runs * nlive strands from
// subsequence 2^63 + b of the stream (mb_draw: an integer histogram, exact in any order), one scan over the merged
// points of (m_k, final ? m_k : 0) gives every point's offset in the resampled run, the exclusive sum E of the final
// points' multiplicities and the totals M' and T, and mb_expand, a thread per expanded position, finds its merged point
// by a search of the offsets and its live count by the reference's rule: T - E (- the copy's index for a final point)
// where the point is alone at its ln L, and in a group of equal ln L, g positions long,
//   n'(i) = T - E(behind the group) + sum over the group's final points with m > 0 of int((g - 1 - i) / (g / m)) + 1
// (float64, as written).  The group's final points are read from a list built once per merged run (FTie).  The
// integrals are section 3.8.2's kernels over (n', lae', logl[src], v[src]) with realization index b.
namespace {

constexpr int kBootMax = 65536;  // bootstraps per call

struct Pair2L {
  long long a, b;
};
struct SumL2 {
  typedef Pair2L T;
  __device__ static T id() { return T{0, 0}; }
  __device__ static T op(T x, T y) { return T{x.a + y.a, x.b + y.b}; }
};

__device__ __forceinline__ bool tied_point(const double* logl, long long M, long long k) {
  const double l = logl[k];
  return (k > 0 && logl[k - 1] == l) || (k + 1 < M && logl[k + 1] == l);
}

// the final points that share their ln L with a neighbour: tie_ep in merged order, tie_idx[k] = how many lie before k
struct FTie {
  typedef SumI Op;
  const double* logl;
  const int* fin;
  int *tie_idx, *tie_ep;
  long long M;
  __device__ int term(long long k) const { return fin[k] && tied_point(logl, M, k) ? 1 : 0; }
  __device__ void put(long long k, int incl, int excl) const {
    tie_idx[k] = excl;
    if (incl != excl) tie_ep[excl] = (int)k;
    if (k == M - 1) tie_idx[M] = incl;
  }
};

__global__ void __launch_bounds__(kT) mb_draw(int S, uint64_t seed, uint64_t seq, int* __restrict__ mult) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= S) return;
  uint32_t w[4];
  philox4x32_10(seed, seq, (uint64_t)j >> 1, w);  // draw j: words 2j and 2j + 1
  const bool odd = j & 1;
  const unsigned long long x = (unsigned long long)(odd ? w[2] : w[0]) | ((unsigned long long)(odd ? w[3] : w[1]) << 32);
  atomicAdd(&mult[__umul64hi(x, (unsigned long long)S)], 1);  // the high 64 bits of x S: in [0, S)
}

// offsets, E and the totals {M', T, a slot outside [0, nlive) was seen}
struct FBoot {
  typedef SumL2 Op;
  const int *run, *id, *fin, *mult;
  int N;
  long long M;
  int *off, *E;
  long long* tot;
  __device__ Pair2L term(long long k) const {
    const int s = id[k];
    if (s < 0 || s >= N) {
      tot[2] = 1;
      return Pair2L{0, 0};
    }
    const long long m = mult[(long long)run[k] * N + s];
    return Pair2L{m, fin[k] ? m : 0};
  }
  __device__ void put(long long k, Pair2L incl, Pair2L excl) const {
    off[k] = (int)excl.a;  // (meaningful below 2^31: the call stops at the totals otherwise)
    E[k] = (int)excl.b;
    if (k == M - 1) {
      tot[0] = incl.a;
      tot[1] = incl.b;
    }
  }
};

struct XArgs {
  long long M, Mx, T;  // merged points, expanded positions, sum of the multiplicities
  int N;
  const double* logl;
  const int *run, *id, *fin, *mult, *off, *E, *tie_idx, *tie_ep;
  int *src, *n;
};

// first k in [0, M) with logl[k] >= l (upper = false) or > l (upper = true)
__device__ __forceinline__ long long bound_logl(const double* logl, long long M, double l, bool upper) {
  long long lo = 0, hi = M;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (upper ? logl[mid] <= l : logl[mid] < l)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kT) mb_expand(XArgs a) {
  const long long p = (long long)blockIdx.x * kT + threadIdx.x;
  if (p >= a.Mx) return;
  long long lo = 0, hi = a.M;  // the last k with off[k] <= p (points never drawn share their successor's offset)
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a.off[mid] <= p)
      lo = mid + 1;
    else
      hi = mid;
  }
  const long long k = lo - 1;
  long long n;
  if (!tied_point(a.logl, a.M, k)) {
    n = a.T - a.E[k] - (a.fin[k] ? p - a.off[k] : 0);
  } else {
    const double l = a.logl[k];
    const long long ga = bound_logl(a.logl, a.M, l, false), gb = bound_logl(a.logl, a.M, l, true);
    const long long p0 = a.off[ga], g = (gb < a.M ? a.off[gb] : a.Mx) - p0, i = p - p0;
    n = a.T - (gb < a.M ? a.E[gb] : a.T);
    const int e1 = a.tie_idx[gb];
    for (int e = a.tie_idx[ga]; e < e1; ++e) {
      const int kk = a.tie_ep[e];
      const int m = a.mult[(long long)a.run[kk] * a.N + a.id[kk]];
      if (m > 0) n += (long long)((double)(g - 1 - i) / ((double)g / (double)m)) + 1;
    }
  }
  a.src[p] = (int)k;
  a.n[p] = (int)n;
}

__global__ void __launch_bounds__(kT) mb_lae(long long Mx, const double* __restrict__ logl, const int* __restrict__ src,
                                             double* __restrict__ lae) {
  const long long p = (long long)blockIdx.x * kT + threadIdx.x;
  if (p >= Mx) return;
  lae[p] = logaddexp_np(logl[src[p]], p > 0 ? logl[src[p - 1]] : -1.e300);
}

__global__ void __launch_bounds__(kT) mb_widen(long long n, const int* __restrict__ in, long long* __restrict__ out) {
  const long long p = (long long)blockIdx.x * kT + threadIdx.x;
  if (p < n) out[p] = in[p];
}

// the arena of one bootstrap call, carved for `cap` expanded positions
struct BootBuf {
  size_t cap = 0;
  int *mult = nullptr, *off = nullptr, *E = nullptr, *src = nullptr, *n = nullptr;
  long long* tot = nullptr;
  void* part = nullptr;
  double *lae = nullptr, *sums = nullptr, *partr = nullptr, *mpart = nullptr, *out = nullptr;  // batch
  double *step = nullptr, *logvol = nullptr, *logwt = nullptr, *logz = nullptr;                // per-point fields
  double *kpart = nullptr, *kld = nullptr;  // the divergence: the chunks' sums (batch); per point (fields)
  long long* wide = nullptr;
};

int boot_carve(dh_ctx* ctx, BootBuf& b, size_t cap, bool fields, bool want_mean) {
  const dh_merged& m = ctx->merged;
  const size_t M = (size_t)m.M, S = (size_t)m.runs * m.nlive, D = (size_t)m.ndim;
  const size_t nblk = blocks_for(M > cap ? M : cap, kChunk), nbx = blocks_for(cap, kChunk);
  const size_t bytes = S * 4 + M * 8 + 64 + (nblk + 1) * sizeof(LsePair) + cap * 16 +
                       (fields ? cap * 48 : (nbx * (2 + kPart + (want_mean ? D : 0)) + 4 + D) * 8) + 27 * 256;
  arena_reset(ctx);
  const int rc = arena_reserve(ctx, bytes);
  if (rc) return rc;
  b = BootBuf();
  b.cap = cap;
  b.mult = (int*)arena_get(ctx, S * 4);
  b.off = (int*)arena_get(ctx, M * 4);
  b.E = (int*)arena_get(ctx, M * 4);
  b.tot = (long long*)arena_get(ctx, 64);
  b.part = arena_get(ctx, (nblk + 1) * sizeof(LsePair));
  b.src = (int*)arena_get(ctx, cap * 4);
  b.n = (int*)arena_get(ctx, cap * 4);
  b.lae = (double*)arena_get(ctx, cap * 8);
  bool ok = b.mult && b.off && b.E && b.tot && b.part && b.src && b.n && b.lae;
  if (fields) {
    b.step = (double*)arena_get(ctx, cap * 8);
    b.logvol = (double*)arena_get(ctx, cap * 8);
    b.logwt = (double*)arena_get(ctx, cap * 8);
    b.logz = (double*)arena_get(ctx, cap * 8);
    b.wide = (long long*)arena_get(ctx, cap * 8);
    b.kld = (double*)arena_get(ctx, cap * 8);
    ok = ok && b.step && b.logvol && b.logwt && b.logz && b.wide && b.kld;
  } else {
    b.sums = (double*)arena_get(ctx, nbx * 8);
    b.partr = (double*)arena_get(ctx, nbx * kPart * 8);
    b.mpart = want_mean ? (double*)arena_get(ctx, nbx * D * 8) : nullptr;
    b.out = (double*)arena_get(ctx, (3 + D) * 8);
    b.kpart = (double*)arena_get(ctx, nbx * 8);
    ok = ok && b.sums && b.partr && (!want_mean || b.mpart) && b.out && b.kpart;
  }
  return ok ? DH_OK : DH_ERR_NOMEM;
}

// the tie structure of the merged run, built by the first bootstrap call on it
int boot_ties(dh_ctx* ctx) {
  dh_merged& m = ctx->merged;
  if (m.tie_n >= 0) return DH_OK;
  const size_t M = (size_t)m.M, S = (size_t)m.runs * m.nlive;
  arena_reset(ctx);
  int rc = arena_reserve(ctx, (blocks_for(M, kChunk) + 1) * sizeof(LsePair) + 1024);
  if (rc) return rc;
  void* part = arena_get(ctx, (blocks_for(M, kChunk) + 1) * sizeof(LsePair));
  if (!part) return DH_ERR_NOMEM;
  int* buf = nullptr;
  (void)hipSetDevice(ctx->device);
  if (hipMalloc((void**)&buf, (M + 1 + S) * 4) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, DH_ERR_NOMEM, "merged_bootstrap: %zu bytes for the tie structure", (M + 1 + S) * 4);
  }
  int tn = 0;
  if (!run_scan(ctx, FTie{m.logl, m.fin, buf, buf + M + 1, m.M}, m.M, part) ||
      !hip_ok(ctx, hipMemcpyAsync(&tn, buf + M, 4, hipMemcpyDeviceToHost, ctx->stream), "D2H ties"))
    rc = DH_ERR_HIP;
  const int rs = dh_sync(ctx);
  if (rc || rs) {
    (void)hipFree(buf);
    return rc ? rc : rs;
  }
  m.tie_idx = buf;
  m.tie_ep = buf + M + 1;
  m.tie_n = tn;
  return DH_OK;
}

int boot_need(dh_ctx* ctx, const char* what, int jitter, const int32_t* mult, int nboot) {
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (!m.have_pt) return fail(ctx, DH_ERR_ARG, "%s: the merge was not given id / it / nc (the strands' slots)", what);
  if (jitter != 0 && jitter != 1) return fail(ctx, DH_ERR_ARG, "%s: jitter %d (0 or 1)", what, jitter);
  if (mult) {
    if (nboot != 1) return fail(ctx, DH_ERR_ARG, "%s: given multiplicities are one bootstrap (nboot %d)", what, nboot);
    const long long S = (long long)m.runs * m.nlive;
    for (long long u = 0; u < S; ++u)
      if (mult[u] < 0) return fail(ctx, DH_ERR_ARG, "%s: mult[%lld] = %d is negative", what, u, mult[u]);
  }
  return DH_OK;
}

// Multiplicities, offsets and totals of bootstrap `boot`, then src and n' (growing the arena where M' exceeds the carve).
// *Mx: M'.  Returns with the stream drained up to the scan.
int boot_expand(dh_ctx* ctx, BootBuf& b, const char* what, uint64_t seed, long long boot, const int32_t* mult, bool fields,
                bool want_mean, long long* Mx) {
  const dh_merged& m = ctx->merged;
  const size_t S = (size_t)m.runs * m.nlive;
  hipStream_t st = ctx->stream;
  if (mult) {
    if (!hip_ok(ctx, hipMemcpyAsync(b.mult, mult, S * 4, hipMemcpyHostToDevice, st), "H2D mult")) return DH_ERR_HIP;
  } else {
    if (!hip_ok(ctx, hipMemsetAsync(b.mult, 0, S * 4, st), "memset")) return DH_ERR_HIP;
    hipLaunchKernelGGL(mb_draw, dim3(blocks_for(S, kT)), dim3(kT), 0, st, (int)S, seed, ((uint64_t)1 << 63) + (uint64_t)boot, b.mult);
  }
  long long tot[3];
  if (!hip_ok(ctx, hipMemsetAsync(b.tot, 0, 24, st), "memset") ||
      !run_scan(ctx, FBoot{m.run, m.id, m.fin, b.mult, m.nlive, m.M, b.off, b.E, b.tot}, m.M, b.part) ||
      !hip_ok(ctx, hipMemcpyAsync(tot, b.tot, 24, hipMemcpyDeviceToHost, st), "D2H totals"))
    return DH_ERR_HIP;
  int rc = dh_sync(ctx);
  if (rc) return rc;
  if (tot[2]) return fail(ctx, DH_ERR_ARG, "%s: a point's slot lies outside [0, %d): these ids do not name strands", what, m.nlive);
  if (tot[0] < 1 || tot[0] >= (1ll << 31))
    return fail(ctx, DH_ERR_ARG, "%s: the resampled run has %lld points (1 to 2^31 - 1)", what, tot[0]);
  *Mx = tot[0];
  if ((size_t)tot[0] > b.cap) {  // the arena grows: the multiplicities travel through the host, the scan runs again
    std::vector<int32_t> keep(S);
    if (!mult) {
      if (!down(ctx, keep.data(), (const int32_t*)b.mult, S)) return DH_ERR_HIP;
      rc = dh_sync(ctx);
      if (rc) return rc;
    }
    rc = boot_carve(ctx, b, (size_t)tot[0] + (size_t)tot[0] / 4 + kChunk, fields, want_mean);
    if (rc) return rc;
    if (!hip_ok(ctx, hipMemcpyAsync(b.mult, mult ? mult : keep.data(), S * 4, hipMemcpyHostToDevice, st), "H2D mult") ||
        !hip_ok(ctx, hipMemsetAsync(b.tot, 0, 24, st), "memset") ||
        !run_scan(ctx, FBoot{m.run, m.id, m.fin, b.mult, m.nlive, m.M, b.off, b.E, b.tot}, m.M, b.part))
      return DH_ERR_HIP;
    rc = dh_sync(ctx);  // (`keep` leaves scope)
    if (rc) return rc;
  }
  XArgs x{m.M, tot[0], tot[1], m.nlive, m.logl, m.run, m.id, m.fin, b.mult, b.off, b.E, m.tie_idx, m.tie_ep, b.src, b.n};
  const unsigned gx = blocks_for((size_t)tot[0], kT);
  hipLaunchKernelGGL(mb_expand, dim3(gx), dim3(kT), 0, st, x);
  hipLaunchKernelGGL(mb_lae, dim3(gx), dim3(kT), 0, st, tot[0], m.logl, (const int*)b.src, b.lae);
  return hip_ok(ctx, hipGetLastError(), "bootstrap launch") ? DH_OK : DH_ERR_HIP;
}

// dh_merged_bootstrap after its argument checks; kld (or null): the bootstraps' divergence from the merged run too
// (dh_merged_kld; logz may then be null)
int bootstrap_core(dh_ctx* ctx, const char* what, uint64_t seed, int64_t first, int nboot, int jitter, const int32_t* mult_or_null,
                   int want_mean, double* logz, double* h, double* ess, double* mean, int64_t* npoints, double* kld) {
  int rc = boot_ties(ctx);
  if (rc) return rc;
  const dh_merged& m = ctx->merged;
  const size_t M = (size_t)m.M, D = (size_t)m.ndim, W = 3 + D;
  BootBuf b;
  rc = boot_carve(ctx, b, M + M / 4 + kChunk, false, want_mean != 0);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  const size_t lds = (size_t)(2 * kT * 3 + (want_mean ? kRealTile * kChunk + kSeg * kRealTile * kColTile : 0)) * 8;
  if (!(kld ? lds_limit(ctx, me_integrate<true, true>, lds) : lds_limit(ctx, me_integrate<true, false>, lds))) return DH_ERR_HIP;
  std::vector<double> host((size_t)nboot * W);
  for (int i = 0; i < nboot; ++i) {
    long long Mx = 0;
    rc = boot_expand(ctx, b, what, seed, (long long)first + i, mult_or_null, false, want_mean != 0, &Mx);
    if (rc) return rc;
    if (npoints) npoints[i] = Mx;
    RArgs a;
    a.M = Mx;
    a.first = (long long)first + i;
    a.D = m.ndim;
    a.nblk = (int)blocks_for((size_t)Mx, kChunk);
    a.nreal = 1;
    a.jitter = jitter;
    a.want_mean = want_mean ? 1 : 0;
    a.seed = seed;
    a.logl = m.logl;
    a.lae = b.lae;
    a.rwt = nullptr;
    a.v = m.v;
    a.n = b.n;
    a.map = b.src;
    a.sums = b.sums;
    a.part = b.partr;
    a.mpart = b.mpart;
    a.out = b.out;
    const dim3 grid((unsigned)a.nblk, 1);
    hipLaunchKernelGGL(me_step_sums, grid, dim3(kT), 0, st, a);
    hipLaunchKernelGGL(me_step_carry, dim3(1), dim3(kT), 0, st, a);
    if (kld) {
      a.lwt0 = m.logwt;
      a.lz0 = m.logz + (M - 1);
      a.kpart = b.kpart;
      hipLaunchKernelGGL((me_integrate<true, true>), grid, dim3(kT), lds, st, a);
      hipLaunchKernelGGL(me_finish<true>, dim3(1), dim3(kT), 0, st, a);
    } else {
      hipLaunchKernelGGL((me_integrate<true, false>), grid, dim3(kT), lds, st, a);
      hipLaunchKernelGGL(me_finish<false>, dim3(1), dim3(kT), 0, st, a);
    }
    // (the row leaves before the next bootstrap's totals are waited for: one synchronisation per bootstrap)
    if (!hip_ok(ctx, hipGetLastError(), "bootstrap launch") || !down(ctx, host.data() + (size_t)i * W, (const double*)b.out, W))
      return DH_ERR_HIP;
  }
  rc = dh_sync(ctx);
  if (rc) return rc;
  for (size_t i = 0; i < (size_t)nboot; ++i) {
    if (logz) logz[i] = host[i * W];
    if (h) h[i] = host[i * W + 1];
    if (ess) ess[i] = host[i * W + 2];
    if (mean)
      for (size_t c = 0; c < D; ++c) mean[i * D + c] = host[i * W + 3 + c];
    if (kld) kld[i] = host[i * W + 3];
  }
  return DH_OK;
}

}  // namespace

extern "C" {

int dh_merged_bootstrap(dh_ctx* ctx, uint64_t seed, int64_t first, int nboot, int jitter, const int32_t* mult_or_null,
                        int want_mean, double* logz, double* h, double* ess, double* mean, int64_t* npoints) {
  DH_CHECK_CTX(ctx);
  const int rc = boot_need(ctx, "merged_bootstrap", jitter, mult_or_null, nboot);
  if (rc) return rc;
  if (nboot < 1 || nboot > kBootMax || first < 0 || first > INT64_MAX - nboot || !logz || (!!want_mean != !!mean))
    return fail(ctx, DH_ERR_ARG, "merged_bootstrap: nboot %d (1 to %d), first %lld (>= 0), logz, and want_mean with mean", nboot,
                kBootMax, (long long)first);
  return bootstrap_core(ctx, "merged_bootstrap", seed, first, nboot, jitter, mult_or_null, want_mean, logz, h, ess, mean, npoints,
                        nullptr);
}

// The divergence of realizations or bootstraps from the merged run (utils.kld_error,
// utils.py:1932-1997): the batch form of the two calls above with one more chunk sum.
int dh_merged_kld(dh_ctx* ctx, uint64_t seed, int64_t first, int n, int mode, const int32_t* mult_or_null, double* kld,
                  double* logz_or_null, int64_t* npoints_or_null) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  if (mode != DH_KLD_JITTER && mode != DH_KLD_RESAMPLE && mode != DH_KLD_SIMULATE)
    return fail(ctx, DH_ERR_ARG, "merged_kld: mode %d (JITTER, RESAMPLE or SIMULATE)", mode);
  if (mode != DH_KLD_JITTER) {
    const int rc = boot_need(ctx, "merged_kld", mode == DH_KLD_SIMULATE, mult_or_null, n);
    if (rc) return rc;
  }
  const int cap = mode == DH_KLD_JITTER ? kRealMax : kBootMax;
  if (n < 1 || n > cap || first < 0 || first > INT64_MAX - n || !kld || (mode == DH_KLD_JITTER && mult_or_null))
    return fail(ctx, DH_ERR_ARG, "merged_kld: n %d (1 to %d), first %lld (>= 0), kld, and mult with a bootstrap mode only", n, cap,
                (long long)first);
  if (mode == DH_KLD_JITTER) {
    std::vector<double> lz(logz_or_null ? 0 : (size_t)n);
    const int rc = realize_core(ctx, seed, first, n, 1, nullptr, 0, logz_or_null ? logz_or_null : lz.data(), nullptr, nullptr,
                                nullptr, kld);
    if (rc) return rc;
    if (npoints_or_null)
      for (int i = 0; i < n; ++i) npoints_or_null[i] = ctx->merged.M;
    return DH_OK;
  }
  return bootstrap_core(ctx, "merged_kld", seed, first, n, mode == DH_KLD_SIMULATE, mult_or_null, 0, logz_or_null, nullptr, nullptr,
                        nullptr, npoints_or_null, kld);
}

int dh_merged_bootstrap_run(dh_ctx* ctx, uint64_t seed, int64_t boot, int jitter, const int32_t* mult_or_null, int field,
                            int64_t first, int64_t count, void* out, int64_t* npoints) {
  DH_CHECK_CTX(ctx);
  int rc = boot_need(ctx, "merged_bootstrap_run", jitter, mult_or_null, 1);
  if (rc) return rc;
  if (boot < 0 || first < 0 || count < 0 || (count && !out) ||
      (field != DH_MERGED_LOGVOL && field != DH_MERGED_LOGWT && field != DH_MERGED_LOGZ && field != DH_MERGED_SAMPLES_N &&
       field != DH_MERGED_SRC && field != DH_MERGED_KLD))
    return fail(ctx, DH_ERR_ARG, "merged_bootstrap_run: boot %lld (>= 0), field %d (LOGVOL, LOGWT, LOGZ, KLD, SAMPLES_N or SRC), "
                "first %lld, count %lld", (long long)boot, field, (long long)first, (long long)count);
  rc = boot_ties(ctx);
  if (rc) return rc;
  const dh_merged& m = ctx->merged;
  const size_t M = (size_t)m.M;
  BootBuf b;
  rc = boot_carve(ctx, b, M + M / 4 + kChunk, true, false);
  if (rc) return rc;
  long long Mx = 0;
  rc = boot_expand(ctx, b, "merged_bootstrap_run", seed, (long long)boot, mult_or_null, true, false, &Mx);
  if (rc) return rc;
  if (first > Mx || count > Mx - first) {
    (void)dh_sync(ctx);
    return fail(ctx, DH_ERR_ARG, "merged_bootstrap_run: [%lld, %lld + %lld) of %lld points", (long long)first, (long long)first,
                (long long)count, Mx);
  }
  if (npoints) *npoints = Mx;
  if (!count) return dh_sync(ctx);
  hipStream_t st = ctx->stream;
  const size_t f = (size_t)first, c = (size_t)count;
  bool ok = true;
  if (field == DH_MERGED_SAMPLES_N) {
    ok = down(ctx, (int*)out, (const int*)b.n + f, c);
  } else if (field == DH_MERGED_SRC) {
    hipLaunchKernelGGL(mb_widen, dim3(blocks_for((size_t)Mx, kT)), dim3(kT), 0, st, Mx, (const int*)b.src, b.wide);
    ok = hip_ok(ctx, hipGetLastError(), "bootstrap launch") && down(ctx, (long long*)out, (const long long*)b.wide + f, c);
  } else {
    if (!run_scan(ctx, FRealVol{b.n, b.step, b.logvol, seed, (uint64_t)boot, jitter}, Mx, b.part)) return DH_ERR_HIP;
    if (field != DH_MERGED_LOGVOL && !run_scan(ctx, FRealLogz{b.lae, nullptr, b.logvol, b.step, b.logwt, b.logz}, Mx, b.part))
      return DH_ERR_HIP;
    if (field == DH_MERGED_KLD &&
        !run_scan(ctx, FRealKld{b.logwt, b.logz, m.logwt, m.logz + (M - 1), b.src, b.kld, Mx}, Mx, b.part))
      return DH_ERR_HIP;
    const double* src = field == DH_MERGED_LOGVOL ? b.logvol : field == DH_MERGED_LOGWT ? b.logwt : field == DH_MERGED_KLD ? b.kld : b.logz;
    ok = down(ctx, (double*)out, src + f, c);
  }
  if (!ok) return DH_ERR_HIP;
  return dh_sync(ctx);
}

}  // extern "C"

// ---- the weight function of the merged run (dynamicsampler.py:48-170) -------------------------
//
// zweight: with Ztot = logaddexp(LOGZ_{M-1}, LOGL_{M-1} + LOGVOL_{M-1}) the remaining evidence of point k over its live
// count, lzw_k = Ztot + log(-expm1(LOGZ_k - Ztot)) - log(n_k), normalised by one fixed-order log-sum-exp (the scans'
// Lse pairs: a workgroup's chunk, then the chunks in scan_carry's order); 1 / M where the cumulative ln Z never moved.
// weight = (1 - pfrac) zweight + pfrac pweight, pweight the WEIGHT field; its maximum and the first and last point above
// maxfrac x maximum through integer atomics (a non-negative double orders as its bits do): exact in any order.
namespace {

struct FZw {
  typedef Lse Op;
  const double *logz, *logl, *logvol;
  const int* n;
  long long M;
  __device__ double lzw(long long k) const {
    const double ztot = logaddexp_np(logz[M - 1], logl[M - 1] + logvol[M - 1]);
    return ztot + log(-expm1(logz[k] - ztot)) - log((double)n[k]);
  }
  __device__ LsePair term(long long k) const { return LsePair{lzw(k), 1.0}; }
  __device__ void put(long long, LsePair, LsePair) const {}
};

// one workgroup: tot[0] = ln sum exp of the chunks' pairs, combined as scan_carry combines them
__global__ void __launch_bounds__(kT) mw_lse_total(const LsePair* __restrict__ part, int nblk, double* __restrict__ tot) {
  __shared__ LsePair lds[2 * kT];
  LsePair carry = Lse::id();
  for (int b0 = 0; b0 < nblk; b0 += kT) {
    const int b = b0 + threadIdx.x;
    const LsePair v = b < nblk ? part[b] : Lse::id();
    LsePair ex, t;
    block_scan<Lse>(v, lds, &ex, &t);
    carry = Lse::op(carry, t);
  }
  if (threadIdx.x == 0) tot[0] = carry.m + log(carry.s);
}

// zw, wt (either may be null) and the maximum of wt as bits in wmax[0] (zeroed before the launch)
__global__ void __launch_bounds__(kT) mw_weight(FZw f, double pfrac, const double* __restrict__ pw, const double* __restrict__ tot,
                                                double* __restrict__ zw, double* __restrict__ wt, unsigned long long* wmax) {
  __shared__ unsigned long long lds[kT];
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  unsigned long long bits = 0;
  if (k < f.M) {
    const double z = f.logz[0] == f.logz[f.M - 1] ? 1.0 / (double)f.M : exp(f.lzw(k) - tot[0]);
    const double w = __dadd_rn(__dmul_rn(1.0 - pfrac, z), __dmul_rn(pfrac, pw[k]));  // (as written: no contraction)
    if (zw) zw[k] = z;
    if (wt) wt[k] = w;
    bits = w > 0 ? (unsigned long long)__double_as_longlong(w) : 0;  // (NaN and 0 are no maximum)
  }
  lds[threadIdx.x] = bits;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if (threadIdx.x < d && lds[threadIdx.x + d] > lds[threadIdx.x]) lds[threadIdx.x] = lds[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0 && lds[0]) atomicMax(wmax, lds[0]);
}

// idx[0] / idx[1]: the first / last k with wt[k] > maxfrac max (set to M / -1 before the launch)
__global__ void __launch_bounds__(kT) mw_bounds(long long M, double maxfrac, const double* __restrict__ wt,
                                                const unsigned long long* __restrict__ wmax, int* idx) {
  __shared__ int lo[kT], hi[kT];
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  const double thr = __dmul_rn(maxfrac, __longlong_as_double((long long)wmax[0]));
  const bool on = k < M && wt[k] > thr;
  lo[threadIdx.x] = on ? (int)k : 0x7fffffff;
  hi[threadIdx.x] = on ? (int)k : -1;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if (threadIdx.x < d) {
      lo[threadIdx.x] = min(lo[threadIdx.x], lo[threadIdx.x + d]);
      hi[threadIdx.x] = max(hi[threadIdx.x], hi[threadIdx.x + d]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && hi[0] >= 0) {
    atomicMin(&idx[0], lo[0]);
    atomicMax(&idx[1], hi[0]);
  }
}

struct WBuf {
  double *tot = nullptr, *zw = nullptr, *wt = nullptr;
  unsigned long long* wmax = nullptr;
  int* idx = nullptr;
};

// zweight and weight of every point into the arena, the maximum's bits in wmax
int weights_enqueue(dh_ctx* ctx, double pfrac, WBuf& w) {
  const dh_merged& m = ctx->merged;
  const size_t M = (size_t)m.M, nblk = blocks_for(M, kChunk);
  arena_reset(ctx);
  const int rc = arena_reserve(ctx, M * 16 + (nblk + 1) * sizeof(LsePair) + 8 * 256);
  if (rc) return rc;
  LsePair* part = (LsePair*)arena_get(ctx, (nblk + 1) * sizeof(LsePair));
  w.tot = (double*)arena_get(ctx, 8);
  w.wmax = (unsigned long long*)arena_get(ctx, 8);
  w.idx = (int*)arena_get(ctx, 8);
  w.zw = (double*)arena_get(ctx, M * 8);
  w.wt = (double*)arena_get(ctx, M * 8);
  if (!part || !w.tot || !w.wmax || !w.idx || !w.zw || !w.wt) return DH_ERR_NOMEM;
  hipStream_t st = ctx->stream;
  const FZw f{m.logz, m.logl, m.logvol, m.n, m.M};
  if (!hip_ok(ctx, hipMemsetAsync(w.wmax, 0, 8, st), "memset")) return DH_ERR_HIP;
  hipLaunchKernelGGL(scan_reduce<FZw>, dim3((unsigned)nblk), dim3(kT), 0, st, f, m.M, part);
  hipLaunchKernelGGL(mw_lse_total, dim3(1), dim3(kT), 0, st, (const LsePair*)part, (int)nblk, w.tot);
  hipLaunchKernelGGL(mw_weight, dim3(blocks_for(M, kT)), dim3(kT), 0, st, f, pfrac, (const double*)m.w, (const double*)w.tot, w.zw,
                     w.wt, w.wmax);
  return hip_ok(ctx, hipGetLastError(), "weights launch") ? DH_OK : DH_ERR_HIP;
}

}  // namespace

extern "C" {

int dh_merged_weight_function(dh_ctx* ctx, double pfrac, double maxfrac, int64_t pad, double* logl_bounds, int64_t* idx) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  if (!(pfrac >= 0.0 && pfrac <= 1.0) || !(maxfrac >= 0.0 && maxfrac <= 1.0) || pad < 0 || !logl_bounds)
    return fail(ctx, DH_ERR_ARG, "merged_weight_function: pfrac %g and maxfrac %g in [0, 1], pad %lld >= 0, logl_bounds", pfrac,
                maxfrac, (long long)pad);
  const dh_merged& m = ctx->merged;
  WBuf w;
  int rc = weights_enqueue(ctx, pfrac, w);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  const int init[2] = {0x7fffffff, -1};
  int got[2] = {0, 0};
  if (!hip_ok(ctx, hipMemcpyAsync(w.idx, init, 8, hipMemcpyHostToDevice, st), "H2D")) return DH_ERR_HIP;
  hipLaunchKernelGGL(mw_bounds, dim3(blocks_for((size_t)m.M, kT)), dim3(kT), 0, st, m.M, maxfrac, (const double*)w.wt,
                     (const unsigned long long*)w.wmax, w.idx);
  if (!hip_ok(ctx, hipGetLastError(), "weights launch") || !down(ctx, got, (const int*)w.idx, 2)) return DH_ERR_HIP;
  rc = dh_sync(ctx);
  if (rc) return rc;
  if (got[1] < 0) return fail(ctx, DH_ERR_VALUE, "merged_weight_function: no weight above %g x the largest", maxfrac);
  if (idx) {
    idx[0] = got[0];
    idx[1] = got[1];
  }
  // the padding and overflow rules of dynamicsampler.py:147-166, as written
  const long long ns = m.M;
  long long b0 = (long long)got[0] - pad, b1 = (long long)got[1] + pad;
  if (b1 > ns - 1) {
    b0 = b0 - (b1 - (ns - 1));
    b1 = ns - 1;
  }
  const long long at0 = b0 <= 0 ? -1 : b0, at1 = b0 <= 0 ? (b1 - b0 < ns - 1 ? b1 - b0 : ns - 1) : b1;
  double l0 = -INFINITY, l1 = INFINITY;
  if (at0 >= 0 && !down(ctx, &l0, (const double*)m.logl + at0, 1)) return DH_ERR_HIP;
  if (b1 != ns - 1 && !down(ctx, &l1, (const double*)m.logl + at1, 1)) return DH_ERR_HIP;
  rc = dh_sync(ctx);
  if (rc) return rc;
  logl_bounds[0] = l0;
  logl_bounds[1] = l1;
  return DH_OK;
}

int dh_merged_weights(dh_ctx* ctx, double pfrac, int which, int64_t first, int64_t count, double* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (!(pfrac >= 0.0 && pfrac <= 1.0) || (which != DH_WEIGHT_P && which != DH_WEIGHT_Z && which != DH_WEIGHT_BOTH) || first < 0 ||
      count < 0 || first > m.M || count > m.M - first || (count && !out))
    return fail(ctx, DH_ERR_ARG, "merged_weights: pfrac %g in [0, 1], which %d (P, Z or BOTH), [%lld, %lld + %lld) of %lld points",
                pfrac, which, (long long)first, (long long)first, (long long)count, m.M);
  if (!count) return DH_OK;
  const double* src = m.w;
  if (which != DH_WEIGHT_P) {
    WBuf w;
    const int rc = weights_enqueue(ctx, pfrac, w);
    if (rc) return rc;
    src = which == DH_WEIGHT_Z ? w.zw : w.wt;
  }
  if (!down(ctx, out, src + first, (size_t)count)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

}  // extern "C"
