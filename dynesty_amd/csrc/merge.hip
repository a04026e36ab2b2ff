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
//
// This unit is the combiner proper with fetch, moments, resample, gather and release; the marginals of the merged run
// are merge_marginals.hip, its statistical errors merge_errors.hip.  The scans are merge_dev.h's, the sizes and the
// scratch layouts merge_plan.h's.
#include "merge_dev.h"

namespace {

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

// ---- scans (the operators and the three launches: merge_dev.h) ------------------------------------------------------

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
  MergeScratch s;
  long long chunk1;
  const int nchunk1 = moment_chunks(M, (size_t)D + 2, &chunk1);
  auto lay_m = [&](Carver& c) { carve_merged(c, m, (size_t)M, (size_t)D, pt); };
  auto lay_s = [&](Carver& c) { carve_scratch(c, s, (size_t)M, (size_t)R, (size_t)N, (size_t)D); };
  char* mbase = device_carve(lay_m);
  char* sbase = mbase ? device_carve(lay_s) : nullptr;
  if (!sbase) {
    (void)hipFree(mbase);
    return fail(ctx, DH_ERR_NOMEM, "merge: %zu + %zu bytes of device memory", layout_bytes(lay_m), layout_bytes(lay_s));
  }
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
  MergeStage g;
  const int rc = arena_carve(ctx, [&](Carver& c) { carve_stage(c, g, R, N, D, S1, npt != 0); });
  if (rc) return rc;
  // (a run without dead points still has its row of one: nothing is copied into it.  A copy that fails returns what
  // the staging always has)
  if (!arena_fill(ctx, g.dead_logl, S ? dead_logl : nullptr, R * S1) || !arena_fill(ctx, g.live_logl, live_logl, R * N) ||
      !arena_fill(ctx, g.dead_u, S ? dead_u : nullptr, R * S1 * D) || !arena_fill(ctx, g.live_u, live_u, R * N * D) ||
      (npt && (!arena_fill(ctx, g.dead_id, S ? (const int*)dead_id : nullptr, R * S1) ||
               !arena_fill(ctx, g.dead_it, S ? (const int*)dead_it : nullptr, R * S1) ||
               !arena_fill(ctx, g.dead_nc, S ? (const int*)dead_nc : nullptr, R * S1) ||
               !arena_fill(ctx, g.live_it, (const int*)live_it, R * N))))
    return DH_ERR_NOMEM;
  std::vector<long long> nit(niter, niter + runs);
  return merge_core(ctx, problem, runs, nlive, ndim, (long long)S1, nit.data(), g.dead_logl, g.live_logl, g.dead_u, g.live_u,
                    g.dead_id, g.dead_it, g.dead_nc, g.live_it, summary_out);
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
  CovBuf b;
  (void)hipSetDevice(ctx->device);
  char* ws = device_carve([&](Carver& c) { carve_cov(c, b, (size_t)m.M, D); });
  if (!ws) return fail(ctx, DH_ERR_NOMEM, "merged_moments: workspace");
  hipLaunchKernelGGL(mg_mom2, dim3(nchunk, blocks_for(D * D, kT)), dim3(kT), 0, st, m.M, m.ndim, chunk, m.w, m.v, m.mom, b.part);
  hipLaunchKernelGGL(mg_mom2_fin, dim3(blocks_for(D * D, kT)), dim3(kT), 0, st, m.ndim, nchunk, b.part, m.mom, b.cov);
  int rc = DH_OK;
  if (!hip_ok(ctx, hipGetLastError(), "moments launch") ||
      !hip_ok(ctx, hipMemcpyAsync(cov, b.cov, D * D * 8, hipMemcpyDeviceToHost, st), "D2H cov"))
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
    if (!device_carve([&](Carver& c) { c(m.idx, "idx", (size_t)n_out); }))
      return fail(ctx, DH_ERR_NOMEM, "merged_resample: %lld indices", (long long)n_out);
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
  GatherBuf b;
  const int rc = arena_carve(ctx, [&](Carver& c) { carve_gather(c, b, (size_t)n, D, idx_or_null != nullptr); });
  if (rc) return rc;
  const long long* d_idx = m.idx;
  if (idx_or_null) {
    for (int64_t i = 0; i < n; ++i)
      if (idx_or_null[i] < 0 || idx_or_null[i] >= m.M)
        return fail(ctx, DH_ERR_ARG, "merged_gather: index %lld at %lld outside [0, %lld)", (long long)idx_or_null[i], (long long)i, m.M);
    if (!arena_fill(ctx, b.idx, (const long long*)idx_or_null, (size_t)n)) return DH_ERR_NOMEM;
    d_idx = b.idx;
  } else if (!m.idx || n > m.idx_n) {
    return fail(ctx, DH_ERR_ARG, "merged_gather: %lld rows asked, the last resample left %lld indices", (long long)n, m.idx_n);
  }
  hipLaunchKernelGGL(mg_gather, dim3(blocks_for((size_t)n * D, kT)), dim3(kT), 0, ctx->stream, (size_t)n * D, m.ndim, m.M, m.v, d_idx, b.out);
  if (!hip_ok(ctx, hipGetLastError(), "gather launch") || !down(ctx, out_v, (const double*)b.out, (size_t)n * D)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_merged_release(dh_ctx* ctx) {
  DH_CHECK_CTX(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  merged_free(ctx);
  return DH_OK;
}

}  // extern "C"
