// The fold on the device: the strands of one dynamic batch folded into the context's merged run, which stays in HBM
// (DESIGN.md section 3.8.5).  It follows dynamic.merge_strands -- the reference's combine_runs
// (dynamicsampler.py:1467-1609) applied strand after strand, in one pass: the result equals dynamic.merge_batch folded
// over the strands in strand order.
//
// Stages, all on the context's stream with no host synchronisation in between (M base points, W new points, T = M + W):
//   sequences : per strand its dead values in death order, then its final live values ascending (the merge's kernels)
//   order     : the merge's pairwise rounds among the strands, then ONE two-list round against the base, which is
//               sorted already: base point i goes to i + #{new < x}, new point j to j + #{base <= x}
//   scatter   : the W new points' bookkeeping (the merge's mg_scatter), then every field of the T points by a select
//               between the base's value and the new point's; ids renumbered and shifted, batch indices
//   rows      : the new points' unit-cube rows staged, their parameters through eval_launch_dev (W rows only); one
//               thread per element moves u and v of all T points
//   counts    : samples_n = n_base[base points before k] + (ln L > logl_min ? R N - final new points before k : 0)
//   volumes   : combine_runs' plateau rule as one scan: a group of p equal ln L enters as ONE term at its last point,
//               its members take ln X + log1p(-(j + 1) / (n + 1)) off the group's exclusive value
//   integrals : merge_dev.h's run_integrals over the whole run, every point with its own step
// The fold is built in a block of its own and swapped in on success: any failure leaves the base run as it was.
#include "merge_dev.h"

namespace {

// the largest id of the base (renumbered: run * nlive + id where the base is a merge of several static runs)
__global__ void __launch_bounds__(kT) mf_idmax(long long M, const int* __restrict__ id, const int* __restrict__ run, int nlive,
                                               int renumber, int* out) {
  __shared__ int red[kT];
  int acc = 0;
  for (long long k = (long long)blockIdx.x * kT + threadIdx.x; k < M; k += (long long)gridDim.x * kT) {
    const int v = renumber ? run[k] * nlive + id[k] : id[k];
    acc = v > acc ? v : acc;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] = red[threadIdx.x + d] > red[threadIdx.x] ? red[threadIdx.x + d] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(out, red[0]);
}

// The round against the base: src[pos] = the base index, or M + the new point's index in the strands' merged order.
// flags[2]: a new point at or below logl_min.
__global__ void __launch_bounds__(kT) mf_place(long long M, long long W, const double* __restrict__ base_l,
                                               const double* __restrict__ new_l, double logl_min, int* __restrict__ src,
                                               double* __restrict__ logl, int* flags) {
  const long long p = (long long)blockIdx.x * kT + threadIdx.x;
  if (p >= M + W) return;
  const bool isnew = p >= M;
  const double x = isnew ? new_l[p - M] : base_l[p];
  long long pos;
  if (!isnew) {
    pos = p + lower_bound_dev(new_l, W, x);
  } else {
    pos = (p - M) + upper_bound_dev(base_l, M, x);
    if (!(x > logl_min)) flags[2] = 1;
  }
  src[pos] = (int)p;  // 0 <= pos < M + W for any input
  logl[pos] = x;
}

struct FoldPoint {  // one side's per-point fields (the base's arrays, or the W new points')
  const int *run, *seq, *fin, *id, *it, *nc;  // id / it / nc null together
};

// Every integer field of point k: a select between the base's value and the new point's (both loads are issued, the
// select follows).  n[k] receives the BASE's share of the live count, finnew[k] whether k is a new final live point.
__global__ void __launch_bounds__(kT) mf_scatter(long long M, long long W, const int* __restrict__ src, FoldPoint b, FoldPoint w,
                                                 const int* __restrict__ base_n, const int* __restrict__ base_batch,
                                                 const int* __restrict__ shift, const int* __restrict__ idmax, int renumber,
                                                 int nlive, int batch0, int* __restrict__ run, int* __restrict__ seq,
                                                 int* __restrict__ id, int* __restrict__ it, int* __restrict__ nc,
                                                 int* __restrict__ fin, int* __restrict__ n, int* __restrict__ batch,
                                                 int* __restrict__ finnew) {
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= M + W) return;
  long long s = src[k];
  if (s < 0 || s >= M + W) s = 0;
  const bool isnew = s >= M;
  const long long bi = isnew ? 0 : s, j = isnew ? s - M : 0;
  // the base points before k: the base's head, whose live count the point carries (0 past the base's end)
  long long head = isnew ? k - j : s;
  const bool past = head >= M;
  if (head < 0 || past) head = M - 1;
  const int r = w.run[j];  // the strand
  const int b_run = b.run[bi], b_seq = b.seq[bi], b_fin = b.fin[bi], w_seq = w.seq[j], w_fin = w.fin[j], head_n = base_n[head];
  const int b_bat = base_batch ? base_batch[bi] : 0;
  run[k] = 0;
  seq[k] = isnew ? w_seq : b_seq;
  fin[k] = isnew ? w_fin : b_fin;
  n[k] = past ? 0 : head_n;
  batch[k] = isnew ? batch0 + 1 + r : b_bat;
  finnew[k] = isnew ? w_fin : 0;
  if (b.id) {
    const int b_id = b.id[bi], b_it = b.it[bi], b_nc = b.nc[bi], w_id = w.id[j], w_it = w.it[j], w_nc = w.nc[j];
    const int sh = shift[r] + idmax[0] + 1;
    id[k] = isnew ? w_id + sh : renumber ? b_run * nlive + b_id : b_id;
    it[k] = isnew ? w_it : b_it;
    nc[k] = isnew ? w_nc : b_nc;
  }
}

// u and v of all T points, one thread per element: the source row is chosen, then read (no load under a condition)
__global__ void __launch_bounds__(kT) mf_rows(size_t total, int D, long long M, long long T, const int* __restrict__ src,
                                              const double* __restrict__ base_u, const double* __restrict__ base_v,
                                              const double* __restrict__ new_u, const double* __restrict__ new_v,
                                              double* __restrict__ u, double* __restrict__ v) {
  const size_t e = (size_t)blockIdx.x * kT + threadIdx.x;
  if (e >= total) return;
  const size_t k = e / (size_t)D;
  const int d = (int)(e - k * (size_t)D);
  long long s = src[k];
  if (s < 0 || s >= T) s = 0;
  const bool isnew = s >= M;
  const size_t row = (size_t)(isnew ? s - M : s) * D + d;
  const double* fu = isnew ? new_u : base_u;
  const double* fv = isnew ? new_v : base_v;
  u[e] = fu[row];
  v[e] = fv[row];
}

// live counts: samples_n = the base's share (already in n) + the strands' where ln L lies above logl_min (strictly)
struct FFoldCount {
  typedef SumI Op;
  const int* finnew;
  const double* logl;
  int* n;
  int total;
  double logl_min;
  __device__ int term(long long k) const { return finnew[k]; }
  __device__ void put(long long k, int, int excl) const { n[k] = n[k] + (logl[k] > logl_min ? total - excl : 0); }
};

// The groups of equal ln L: gstart[k] = -1 for a point on its own, else the index where its group starts.  step[k]: the
// point's own step ln X_{k-1} - ln X_k -- log1p(1 / n), or log1p(1 / (n_i - j)) for member j of a group entered at
// live count n_i (the difference of the closed form's neighbours).  vterm[k]: what the volume scan adds at k -- the own
// step of a single point, the group's whole -log1p(-p / (n_i + 1)) at its last point, 0 at its other members.
// flags[3]: a group of p >= n_i + 1 points, which leaves no positive volume.
__global__ void __launch_bounds__(kT) mf_groups(long long T, const double* __restrict__ logl, const int* __restrict__ n,
                                                int* __restrict__ gstart, double* __restrict__ step, double* __restrict__ vterm,
                                                int* flags) {
  const long long k = (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= T) return;
  const double x = logl[k];
  const bool tied = (k > 0 && logl[k - 1] == x) || (k + 1 < T && logl[k + 1] == x);
  if (!tied) {
    const double st = log1p(1.0 / (double)n[k]);
    gstart[k] = -1;
    step[k] = st;
    vterm[k] = st;
    return;
  }
  const long long g0 = lower_bound_dev(logl, T, x), g1 = upper_bound_dev(logl, T, x);
  const long long p = g1 - g0, j = k - g0;
  const int ni = n[g0 < T ? g0 : T - 1];
  if (p >= (long long)ni + 1) flags[3] = 1;
  gstart[k] = (int)g0;
  step[k] = log1p(1.0 / (double)(ni - j));
  vterm[k] = k == g1 - 1 ? -log1p(-(double)p / ((double)ni + 1.0)) : 0.0;
}

// ln X: minus the cumulative sum for a single point; inside a group the value before the group plus the closed form
struct FFoldVol {
  typedef SumD Op;
  const double* vterm;
  const int *gstart, *n;
  double* logvol;
  __device__ double term(long long k) const { return vterm[k]; }
  __device__ void put(long long k, double incl, double excl) const {
    const int g0 = gstart[k];
    // (the members before the group's last add 0: every member's exclusive value is the sum up to the group's start)
    logvol[k] = g0 < 0 ? -incl : -excl + log1p(-(double)(k - g0 + 1) / ((double)n[g0] + 1.0));
  }
};

}  // namespace

extern "C" {

int dh_merged_fold(dh_ctx* ctx, int problem, int strands, int nlive_new, int64_t stride, const int64_t* niter,
                   const double* dead_logl, const double* live_logl, const double* dead_u, const double* live_u,
                   const int32_t* dead_id, const int32_t* dead_it, const int32_t* dead_nc, const int32_t* live_it,
                   double logl_min, double logl_max, double* summary_out) {
  DH_CHECK_CTX(ctx);
  if (need_merged(ctx)) return DH_ERR_ARG;
  const dh_merged& base = ctx->merged;
  ProblemDev pd;
  if (!get_problem(ctx, problem, &pd)) return DH_ERR_ARG;
  if (pd.ndim != base.ndim) return fail(ctx, DH_ERR_ARG, "merged_fold: problem ndim %d != the merged run's %d", pd.ndim, base.ndim);
  const int npt = !!dead_id + !!dead_it + !!dead_nc + !!live_it;
  if (strands < 1 || nlive_new < 1 || stride < 0 || !niter || !live_logl || !live_u || (stride > 0 && (!dead_logl || !dead_u)) ||
      (npt != 0 && npt != 4))
    return fail(ctx, DH_ERR_ARG, "merged_fold: bad arguments (strands %d, nlive_new %d, stride %lld; id / it / nc / live it come together)",
                strands, nlive_new, (long long)stride);
  if (!(logl_min > -INFINITY && logl_min < INFINITY) || !(logl_max > logl_min))
    return fail(ctx, DH_ERR_ARG, "merged_fold: bounds (%g, %g): logl_min finite and logl_max above it", logl_min, logl_max);
  const bool pt = npt != 0;
  if (pt != base.have_pt)
    return fail(ctx, DH_ERR_ARG, "merged_fold: id / it / nc on one side only (the merged run %s them)", base.have_pt ? "has" : "lacks");
  const int R = strands, N = nlive_new, D = base.ndim;
  const long long M = base.M;
  long long W = 0, maxnit = 0;
  std::vector<long long> off((size_t)R + 1, 0), nit((size_t)R);
  for (int r = 0; r < R; ++r) {
    if (niter[r] < 0 || niter[r] > stride) return fail(ctx, DH_ERR_ARG, "merged_fold: niter[%d] = %lld outside [0, %lld]", r, (long long)niter[r], (long long)stride);
    nit[(size_t)r] = niter[r];
    W += niter[r] + N;
    off[(size_t)r + 1] = W;
    if (niter[r] > maxnit) maxnit = niter[r];
    if (W >= (1ll << 31)) break;
  }
  const long long T = M + W;
  if (T >= (1ll << 31) - kChunk || (long long)R * N >= (1ll << 31))
    return fail(ctx, DH_ERR_ARG, "merged_fold: %lld + %lld points (positions travel as 32-bit indices)", M, W);
  if ((unsigned long long)T * (unsigned long long)D >= (1ull << 32))  // mf_rows: one thread per element of a row array
    return fail(ctx, DH_ERR_ARG, "merged_fold: %lld points of %d coordinates (a row array is limited to 2^32 elements)", T, D);
  // ids: strand s is shifted by (the largest id so far) + 1 = max(base id) + 1 + sum over the strands before it of
  // (their largest id + 1); the strands' part is known here, the base's maximum is found on the device
  const size_t S = (size_t)stride, S1 = S ? S : 1;
  std::vector<int> shift((size_t)R, 0);
  if (pt) {
    long long acc = 0;
    for (int r = 0; r < R; ++r) {
      shift[(size_t)r] = (int)acc;
      int mx = N - 1;  // (the final live points carry their slots)
      for (long long i = 0; i < niter[r]; ++i) {
        const int v = dead_id[(size_t)r * S + (size_t)i];
        if (v < 0) return fail(ctx, DH_ERR_ARG, "merged_fold: dead_id[%d, %lld] = %d is negative", r, i, v);
        if (v > mx) mx = v;
      }
      acc += (long long)mx + 1;
      if (acc >= (1ll << 30)) return fail(ctx, DH_ERR_ARG, "merged_fold: the strands' ids exceed 2^30");
    }
  }
  const size_t Rz = (size_t)R, Nz = (size_t)N, Dz = (size_t)D;
  MergeStage g;
  int rc = arena_carve(ctx, [&](Carver& c) { carve_fold_stage(c, g, Rz, Nz, Dz, S1, pt); });
  if (rc) return rc;
  if (!arena_fill(ctx, g.dead_logl, S ? dead_logl : nullptr, Rz * S1) || !arena_fill(ctx, g.live_logl, live_logl, Rz * Nz) ||
      !arena_fill(ctx, g.dead_u, S ? dead_u : nullptr, Rz * S1 * Dz) || !arena_fill(ctx, g.live_u, live_u, Rz * Nz * Dz) ||
      (pt && (!arena_fill(ctx, g.dead_id, S ? (const int*)dead_id : nullptr, Rz * S1) ||
              !arena_fill(ctx, g.dead_it, S ? (const int*)dead_it : nullptr, Rz * S1) ||
              !arena_fill(ctx, g.dead_nc, S ? (const int*)dead_nc : nullptr, Rz * S1) ||
              !arena_fill(ctx, g.live_it, (const int*)live_it, Rz * Nz))))
    return DH_ERR_NOMEM;
  hipStream_t st = ctx->stream;
  (void)hipSetDevice(ctx->device);
  // the new block, the batch column and the scratch: allocated before anything is launched, the base is only read
  dh_merged m;
  BatchArrays ba;
  FoldScratch s;
  auto lay_m = [&](Carver& c) { carve_merged(c, m, (size_t)T, Dz, pt); };
  auto lay_b = [&](Carver& c) { carve_batch(c, ba, (size_t)T); };
  auto lay_s = [&](Carver& c) { carve_fold_scratch(c, s, (size_t)M, (size_t)W, Rz, Nz, Dz, pt); };
  char* mbase = device_carve(lay_m);
  char* bbase = mbase ? device_carve(lay_b) : nullptr;
  char* sbase = bbase ? device_carve(lay_s) : nullptr;
  if (!sbase) {
    (void)hipFree(mbase);
    (void)hipFree(bbase);
    return fail(ctx, DH_ERR_NOMEM, "merged_fold: %zu + %zu + %zu bytes of device memory beside the merged run", layout_bytes(lay_m),
                layout_bytes(lay_b), layout_bytes(lay_s));
  }
  auto done = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(sbase);
    if (code != DH_OK) {
      (void)hipFree(mbase);
      (void)hipFree(bbase);
    }
    return code;
  };
  const int renumber = base.nbatch == 0 && base.runs > 1;
  if (!hip_ok(ctx, hipMemcpyAsync(s.off, off.data(), (Rz + 1) * 8, hipMemcpyHostToDevice, st), "H2D") ||
      !hip_ok(ctx, hipMemcpyAsync(s.nit, nit.data(), Rz * 8, hipMemcpyHostToDevice, st), "H2D") ||
      !hip_ok(ctx, hipMemcpyAsync(s.shift, shift.data(), Rz * 4, hipMemcpyHostToDevice, st), "H2D") ||
      !hip_ok(ctx, hipMemsetAsync(s.live_slot, 0, Rz * Nz * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.org_a, 0, (size_t)W * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.org_b, 0, (size_t)W * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.seq_run, 0, (size_t)W * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.src, 0, (size_t)T * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.idmax, 0, 4, st), "memset") || !hip_ok(ctx, hipMemsetAsync(s.flags, 0, 16, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(s.ncall, 0, 8, st), "memset"))
    return done(DH_ERR_HIP);
  // sequences and order of the strands among themselves
  const unsigned gW = blocks_for((size_t)W, kT), gT = blocks_for((size_t)T, kT), gM = blocks_for((size_t)M, kT);
  hipLaunchKernelGGL(mg_live_rank, dim3(blocks_for(Nz, kT), R), dim3(kT), 0, st, N, g.live_logl, s.off, s.nit, s.seq_l, s.seq_run,
                     s.live_slot);
  if (maxnit > 0)
    hipLaunchKernelGGL(mg_dead_copy, dim3(blocks_for((size_t)maxnit, kT), R), dim3(kT), 0, st, (long long)S1, g.dead_logl, s.off,
                       s.nit, s.seq_l, s.seq_run);
  hipLaunchKernelGGL(mg_check, dim3(gW), dim3(kT), 0, st, W, s.seq_l, s.seq_run, s.off, s.org_a, s.flags);
  double *kin = s.seq_l, *kout = s.key_b;
  int *oin = s.org_a, *oout = s.org_b;
  for (int wd = 1; wd < R; wd *= 2) {
    hipLaunchKernelGGL(mg_merge_round, dim3(gW), dim3(kT), 0, st, W, R, wd, s.off, kin, oin, kout, oout);
    double* kt = kin;
    kin = kout;
    kout = kt;
    int* ot = oin;
    oin = oout;
    oout = ot;
  }
  // the new points' bookkeeping in their merged order (kout serves as the scatter's copy of the keys), their rows
  MgSrc src{g.dead_u, g.live_u, g.dead_id, g.dead_it, g.dead_nc, g.live_it, (long long)S1, N};
  hipLaunchKernelGGL(mg_scatter, dim3(gW), dim3(kT), 0, st, W, src, kin, oin, s.seq_run, s.off, s.nit, s.live_slot, kout, s.n_run,
                     s.n_seq, s.n_id, s.n_it, s.n_nc, s.n_fin, s.n_row);
  hipLaunchKernelGGL(mg_scatter_rows, dim3(blocks_for((size_t)W * Dz, kT)), dim3(kT), 0, st, (size_t)W * Dz, D, src, s.n_row, s.ustage);
  if (!hip_ok(ctx, hipGetLastError(), "fold launch")) return done(DH_ERR_HIP);
  rc = eval_launch_dev(ctx, problem, (int)W, s.ustage, s.vstage, s.eval_l);
  if (rc) return done(rc);
  // the round against the base, then every field
  if (pt) hipLaunchKernelGGL(mf_idmax, dim3(gM < 1024 ? gM : 1024), dim3(kT), 0, st, M, base.id, base.run, base.nlive, renumber, s.idmax);
  hipLaunchKernelGGL(mf_place, dim3(gT), dim3(kT), 0, st, M, W, base.logl, kin, logl_min, s.src, m.logl, s.flags);
  FoldPoint fb{base.run, base.seq, base.fin, base.id, base.it, base.nc}, fw{s.n_run, s.n_seq, s.n_fin, s.n_id, s.n_it, s.n_nc};
  hipLaunchKernelGGL(mf_scatter, dim3(gT), dim3(kT), 0, st, M, W, s.src, fb, fw, base.n, base.batch, s.shift, s.idmax, renumber,
                     base.nlive, base.nbatch, m.run, m.seq, m.id, m.it, m.nc, m.fin, m.n, ba.batch, s.finnew);
  hipLaunchKernelGGL(mf_rows, dim3(blocks_for((size_t)T * Dz, kT)), dim3(kT), 0, st, (size_t)T * Dz, D, M, T, s.src, base.u, base.v,
                     s.ustage, s.vstage, m.u, m.v);
  if (!hip_ok(ctx, hipGetLastError(), "fold launch")) return done(DH_ERR_HIP);
  // counts, volumes, integrals
  if (!run_scan(ctx, FFoldCount{s.finnew, m.logl, m.n, R * N, logl_min}, T, s.part)) return done(DH_ERR_HIP);
  hipLaunchKernelGGL(mf_groups, dim3(gT), dim3(kT), 0, st, T, m.logl, m.n, s.gstart, s.step, s.vterm, s.flags);
  if (!run_scan(ctx, FFoldVol{s.vterm, s.gstart, m.n, m.logvol}, T, s.part) ||
      !run_integrals(ctx, m, T, D, pt, s.step, IntegralScratch{s.logdvol, s.mom_part, s.last, s.summ, s.ncall, s.part}))
    return done(DH_ERR_HIP);
  double summ[6];
  int flags[4];
  if (!hip_ok(ctx, hipMemcpyAsync(summ, s.summ, sizeof summ, hipMemcpyDeviceToHost, st), "D2H") ||
      !hip_ok(ctx, hipMemcpyAsync(flags, s.flags, sizeof flags, hipMemcpyDeviceToHost, st), "D2H") ||
      !hip_ok(ctx, hipStreamSynchronize(st), "fold sync"))
    return done(DH_ERR_HIP);
  if (flags[0]) return done(fail(ctx, DH_ERR_VALUE, "merged_fold: a log-likelihood is NaN"));
  if (flags[1]) return done(fail(ctx, DH_ERR_VALUE, "merged_fold: a strand's dead log-likelihoods decrease (or exceed its final live points')"));
  if (flags[2]) return done(fail(ctx, DH_ERR_VALUE, "merged_fold: a strand point lies at or below logl_min = %.17g", logl_min));
  if (flags[3])
    return done(fail(ctx, DH_ERR_VALUE, "merged_fold: a plateau of equal log-likelihoods is longer than the live count where it "
                                        "starts: no positive volume is left (combine_runs fails there too)"));
  // success: the fold replaces the base (with its resampled indices and its tie structure)
  m.base = mbase;
  m.M = T;
  m.ndim = D;
  m.runs = 1;
  m.nlive = base.nlive;
  m.have_pt = pt;
  m.nbatch = base.nbatch + R;
  m.batch = ba.batch;
  (void)done(DH_OK);
  merged_free(ctx);
  ctx->merged = m;
  if (summary_out)
    for (int i = 0; i < 6; ++i) summary_out[i] = summ[i];
  return DH_OK;
}

}  // extern "C"
