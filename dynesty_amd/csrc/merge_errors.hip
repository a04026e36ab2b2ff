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
#include "merge_dev.h"

namespace {

constexpr int kMeanLoads = 16;  // rows of v a thread of the mean sums has in flight
constexpr int kFinLoads = 8;    // chunks a thread of me_finish has in flight
constexpr double kLnHalf = -0.6931471805599453;

// (philox4x32_10 and uniform_double: merge_dev.h, shared with the seeds' choice)
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

// What a set of integrals takes from the merged run itself.  The caller adds the points (M, nblk, n, lae, map) and the
// scratch; kld: the divergence from the merged run is summed too.
RArgs merged_rargs(const dh_merged& m, uint64_t seed, int jitter, int want_mean, bool kld) {
  RArgs a{};
  a.D = m.ndim;
  a.jitter = jitter;
  a.want_mean = want_mean ? 1 : 0;
  a.seed = seed;
  a.logl = m.logl;
  a.v = m.v;
  if (kld) {
    a.lwt0 = m.logwt;
    a.lz0 = m.logz + (m.M - 1);
  }
  return a;
}

template <bool kMap, bool kKld>
bool integrals_launch(dh_ctx* ctx, RArgs a, long long first, int rows) {
  const size_t lds = integrate_lds(a.want_mean != 0), W = 3 + (size_t)a.D;
  if (!lds_limit(ctx, me_integrate<kMap, kKld>, lds)) return false;
  double* out = a.out;
  for (int r0 = 0; r0 < rows; r0 += kRealLaunch) {
    a.nreal = rows - r0 < kRealLaunch ? rows - r0 : kRealLaunch;
    a.first = first + r0;
    a.out = out + (size_t)r0 * W;
    const dim3 grid((unsigned)a.nblk, blocks_for((size_t)a.nreal, kRealTile));
    hipLaunchKernelGGL(me_step_sums, grid, dim3(kT), 0, ctx->stream, a);
    hipLaunchKernelGGL(me_step_carry, dim3(a.nreal), dim3(kT), 0, ctx->stream, a);
    hipLaunchKernelGGL((me_integrate<kMap, kKld>), grid, dim3(kT), lds, ctx->stream, a);
    hipLaunchKernelGGL(me_finish<kKld>, dim3(a.nreal), dim3(kT), 0, ctx->stream, a);
  }
  return true;
}

// The integrals of `rows` realizations, global indices `first` on, over the points `a` describes: their rows
// [logz, h, ess, mean.. | kld] land at a.out, kRealLaunch of them per set of launches (the scratch of `a` holds that
// many).  map: logl and v are read through a.map (a bootstrap); kld: the divergence takes the first mean slot.
bool integrals_enqueue(dh_ctx* ctx, const RArgs& a, long long first, int rows, bool map, bool kld) {
  if (map) return kld ? integrals_launch<true, true>(ctx, a, first, rows) : integrals_launch<true, false>(ctx, a, first, rows);
  return kld ? integrals_launch<false, true>(ctx, a, first, rows) : integrals_launch<false, false>(ctx, a, first, rows);
}

// n rows [logz, h, ess, mean.. | kld] into the caller's arrays (each may be null)
void unpack_rows(const std::vector<double>& host, size_t n, size_t D, double* logz, double* h, double* ess, double* mean,
                 double* kld) {
  const size_t W = 3 + D;
  for (size_t b = 0; b < n; ++b) {
    if (logz) logz[b] = host[b * W];
    if (h) h[b] = host[b * W + 1];
    if (ess) ess[b] = host[b * W + 2];
    if (mean)
      for (size_t c = 0; c < D; ++c) mean[b * D + c] = host[b * W + 3 + c];
    if (kld) kld[b] = host[b * W + 3];
  }
}

// The per-point fields of one realization (map null) or bootstrap over n points with live counts `counts`: the scans
// FRealVol -> FRealLogz -> FRealKld as far as `field` needs them.  The device array of the field, or null (error set).
const double* fields_enqueue(dh_ctx* ctx, int field, long long n, const int* counts, const double* lae, const double* rwt,
                             const int* map, uint64_t seed, uint64_t seq, int jitter, const FieldArrays& f, void* part) {
  const dh_merged& m = ctx->merged;
  if (!run_scan(ctx, FRealVol{counts, f.step, f.logvol, seed, seq, jitter}, n, part)) return nullptr;
  if (field != DH_MERGED_LOGVOL && !run_scan(ctx, FRealLogz{lae, rwt, f.logvol, f.step, f.logwt, f.logz}, n, part)) return nullptr;
  if (field == DH_MERGED_KLD &&
      !run_scan(ctx, FRealKld{f.logwt, f.logz, m.logwt, m.logz + (m.M - 1), map, f.kld, n}, n, part))
    return nullptr;
  return field == DH_MERGED_LOGVOL ? f.logvol : field == DH_MERGED_LOGWT ? f.logwt : field == DH_MERGED_KLD ? f.kld : f.logz;
}

// dh_merged_realize after its argument checks; kld (or null): the realizations' divergence from the merged run too
// (dh_merged_kld), through the instantiation of me_integrate that sums it
int realize_core(dh_ctx* ctx, uint64_t seed, int64_t first, int nreal, int jitter, const double* logrwt_or_null, int want_mean,
                 double* logz, double* h, double* ess, double* mean, double* kld) {
  const dh_merged& m = ctx->merged;
  const size_t M = (size_t)m.M, D = (size_t)m.ndim;
  RealBuf b;
  int rc = arena_carve(ctx, [&](Carver& c) {
    carve_real(c, b, M, D, nreal, logrwt_or_null != nullptr, want_mean != 0, kld != nullptr);
  });
  if (rc) return rc;
  if (!arena_fill(ctx, b.rwt, logrwt_or_null, M)) return DH_ERR_NOMEM;  // (what the staging always has returned)
  RArgs a = merged_rargs(m, seed, jitter, want_mean, kld != nullptr);
  a.M = m.M;
  a.nblk = (int)blocks_for(M, kChunk);
  a.n = m.n;
  a.lae = b.lae;
  a.rwt = b.rwt;
  a.sums = b.sums;
  a.part = b.part;
  a.mpart = b.mpart;
  a.kpart = b.kpart;
  a.out = b.out;
  hipLaunchKernelGGL(me_lae, dim3(blocks_for(M, kT)), dim3(kT), 0, ctx->stream, m.M, m.logl, b.lae);
  if (!integrals_enqueue(ctx, a, (long long)first, nreal, false, kld != nullptr) ||
      !hip_ok(ctx, hipGetLastError(), "realize launch"))
    return DH_ERR_HIP;
  std::vector<double> host((size_t)nreal * (3 + D));
  if (!down(ctx, host.data(), (const double*)b.out, host.size())) return DH_ERR_HIP;
  rc = dh_sync(ctx);
  if (rc) return rc;
  unpack_rows(host, (size_t)nreal, D, logz, h, ess, mean, kld);
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
  const size_t M = (size_t)m.M;
  FieldBuf b;
  rc = arena_carve(ctx, [&](Carver& c) { carve_fields(c, b, M, logrwt_or_null != nullptr, field == DH_MERGED_KLD); });
  if (rc) return rc;
  if (!arena_fill(ctx, b.rwt, logrwt_or_null, M)) return DH_ERR_NOMEM;  // (what the staging always has returned)
  hipLaunchKernelGGL(me_lae, dim3(blocks_for(M, kT)), dim3(kT), 0, ctx->stream, m.M, m.logl, b.lae);
  const double* src = fields_enqueue(ctx, field, m.M, m.n, b.lae, b.rwt, nullptr, seed, (uint64_t)real, jitter, b.f, b.part);
  if (!src) return DH_ERR_HIP;
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

struct Pair2L {
  long long a, b;
};
static_assert(sizeof(Pair2L) == kScanElem, "the layouts size a scan's chunk aggregates by kScanElem");
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

// the arena of one bootstrap call, carved for `cap` expanded positions (merge_plan.h: BootBuf)
int boot_carve(dh_ctx* ctx, BootBuf& b, size_t cap, bool fields, bool want_mean) {
  const dh_merged& m = ctx->merged;
  return arena_carve(ctx, [&](Carver& c) {
    carve_boot(c, b, (size_t)m.M, (size_t)m.runs * m.nlive, (size_t)m.ndim, cap, fields, want_mean);
  });
}

// the tie structure of the merged run, built by the first bootstrap call on it
int boot_ties(dh_ctx* ctx) {
  dh_merged& m = ctx->merged;
  if (m.tie_n >= 0) return DH_OK;
  const size_t M = (size_t)m.M, S = (size_t)m.runs * m.nlive;
  TieScratch ts;
  int rc = arena_carve(ctx, [&](Carver& c) { carve_tie_scratch(c, ts, M); });
  if (rc) return rc;
  TieArrays t;
  auto lay = [&](Carver& c) { carve_ties(c, t, M, S); };
  (void)hipSetDevice(ctx->device);
  char* buf = device_carve(lay);
  if (!buf) return fail(ctx, DH_ERR_NOMEM, "merged_bootstrap: %zu bytes for the tie structure", layout_bytes(lay));
  int tn = 0;
  if (!run_scan(ctx, FTie{m.logl, m.fin, t.tie_idx, t.tie_ep, m.M}, m.M, ts.part) ||
      !hip_ok(ctx, hipMemcpyAsync(&tn, t.tie_idx + M, 4, hipMemcpyDeviceToHost, ctx->stream), "D2H ties"))
    rc = DH_ERR_HIP;
  const int rs = dh_sync(ctx);
  if (rc || rs) {
    (void)hipFree(buf);
    return rc ? rc : rs;
  }
  m.tie_idx = t.tie_idx;  // (the allocation's first array: merged_free gives it back through this pointer)
  m.tie_ep = t.tie_ep;
  m.tie_n = tn;
  return DH_OK;
}

int boot_need(dh_ctx* ctx, const char* what, int jitter, const int32_t* mult, int nboot) {
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (!m.have_pt) return fail(ctx, DH_ERR_ARG, "%s: the merge was not given id / it / nc (the strands' slots)", what);
  if (m.nbatch > 0)  // (ensemble.MergedRun's refusal: strands are read off a live count that only falls)
    return fail(ctx, DH_ERR_ARG, "%s: the strand bootstrap is not defined for a run that carries dynamic batches", what);
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
    rc = boot_carve(ctx, b, boot_cap_regrown((size_t)tot[0]), fields, want_mean);
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
  const size_t D = (size_t)m.ndim, W = 3 + D;
  BootBuf b;
  rc = boot_carve(ctx, b, boot_cap_first((size_t)m.M), false, want_mean != 0);
  if (rc) return rc;
  std::vector<double> host((size_t)nboot * W);
  for (int i = 0; i < nboot; ++i) {
    long long Mx = 0;
    rc = boot_expand(ctx, b, what, seed, (long long)first + i, mult_or_null, false, want_mean != 0, &Mx);
    if (rc) return rc;
    if (npoints) npoints[i] = Mx;
    RArgs a = merged_rargs(m, seed, jitter, want_mean, kld != nullptr);
    a.M = Mx;
    a.nblk = (int)blocks_for((size_t)Mx, kChunk);
    a.n = b.n;
    a.lae = b.lae;
    a.map = b.src;
    a.sums = b.sums;
    a.part = b.partr;
    a.mpart = b.mpart;
    a.kpart = kld ? b.kpart : nullptr;
    a.out = b.out;
    // (the row leaves before the next bootstrap's totals are waited for: one synchronisation per bootstrap)
    if (!integrals_enqueue(ctx, a, (long long)first + i, 1, true, kld != nullptr) ||
        !hip_ok(ctx, hipGetLastError(), "bootstrap launch") || !down(ctx, host.data() + (size_t)i * W, (const double*)b.out, W))
      return DH_ERR_HIP;
  }
  rc = dh_sync(ctx);
  if (rc) return rc;
  unpack_rows(host, (size_t)nboot, D, logz, h, ess, mean, kld);
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
  BootBuf b;
  rc = boot_carve(ctx, b, boot_cap_first((size_t)m.M), true, false);
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
    const double* src = fields_enqueue(ctx, field, Mx, b.n, b.lae, nullptr, b.src, seed, (uint64_t)boot, jitter, b.f, b.part);
    if (!src) return DH_ERR_HIP;
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

// zweight and weight of every point into the arena, the maximum's bits in wmax
int weights_enqueue(dh_ctx* ctx, double pfrac, WeightBuf& w) {
  const dh_merged& m = ctx->merged;
  const size_t M = (size_t)m.M, nblk = blocks_for(M, kChunk);
  const int rc = arena_carve(ctx, [&](Carver& c) { carve_weights(c, w, M); });
  if (rc) return rc;
  LsePair* part = (LsePair*)w.part;
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
  WeightBuf w;
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
    WeightBuf w;
    const int rc = weights_enqueue(ctx, pfrac, w);
    if (rc) return rc;
    src = which == DH_WEIGHT_Z ? w.zw : w.wt;
  }
  if (!down(ctx, out, src + first, (size_t)count)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

}  // extern "C"
