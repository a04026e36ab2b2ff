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
// This unit is the combiner proper with fetch, moments, resample, gather and release; the fold of dynamic batches into
// the merged run is merge_fold.hip, the marginals of the merged run are merge_marginals.hip, its statistical errors
// merge_errors.hip.  The scans and the kernels shared with the fold are merge_dev.h's, the sizes and the scratch
// layouts merge_plan.h's.
#include <string.h>

#include "merge_dev.h"

namespace {

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

// ---- summaries (the first moments and the summary: merge_dev.h) ------------------------------------------------------

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
      !run_integrals(ctx, m, M, D, pt, s.step, IntegralScratch{s.logdvol, s.mom_part, s.last, s.summ, s.ncall, s.part}))
    return done(DH_ERR_HIP);
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
  if (ctx->merged.batch) (void)hipFree(ctx->merged.batch);
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
    case DH_MERGED_BATCH:
      if (!m.batch) {  // a run that holds no batch: every point is of batch 0
        if (count) memset(out, 0, (size_t)count * 4);
        return DH_OK;
      }
      src = m.batch;
      width = 4;
      break;
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

int dh_merged_gather_rows(dh_ctx* ctx, int field, int64_t n, const int64_t* idx, double* out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& m = ctx->merged;
  if (field != DH_MERGED_SAMPLES_U && field != DH_MERGED_SAMPLES)
    return fail(ctx, DH_ERR_ARG, "merged_gather_rows: field %d (SAMPLES_U or SAMPLES)", field);
  if (n < 1 || !idx || !out || (unsigned long long)n * (unsigned long long)m.ndim >= (1ull << 32))
    return fail(ctx, DH_ERR_ARG, "merged_gather_rows: n %lld with idx and out (at most 2^32 elements per call)", (long long)n);
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= m.M)
      return fail(ctx, DH_ERR_ARG, "merged_gather_rows: index %lld at %lld outside [0, %lld)", (long long)idx[i], (long long)i, m.M);
  const size_t D = (size_t)m.ndim;
  GatherBuf b;
  const int rc = arena_carve(ctx, [&](Carver& c) { carve_gather_rows(c, b, (size_t)n, D); });
  if (rc) return rc;
  if (!arena_fill(ctx, b.idx, (const long long*)idx, (size_t)n)) return DH_ERR_NOMEM;
  hipLaunchKernelGGL(mg_gather, dim3(blocks_for((size_t)n * D, kT)), dim3(kT), 0, ctx->stream, (size_t)n * D, m.ndim, m.M,
                     field == DH_MERGED_SAMPLES_U ? m.u : m.v, b.idx, b.out);
  if (!hip_ok(ctx, hipGetLastError(), "gather launch") || !down(ctx, out, (const double*)b.out, (size_t)n * D)) return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_merged_release(dh_ctx* ctx) {
  DH_CHECK_CTX(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  merged_free(ctx);
  return DH_OK;
}

}  // extern "C"
