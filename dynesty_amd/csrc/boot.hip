// Bootstrap expansion factor of a bound, device-resident and batched over runs x replicas
// (reference bounding.py:381-400 Ellipsoid.update / 688-703 MultiEllipsoid.update with bootstrap > 0,
// _bootstrap_points :1593-1616, _ellipsoid_bootstrap_expand :1619-1648).
//
//   boot_mask_kernel    one workgroup per (run, replica): n indices drawn with replacement from the replica's own
//                       PCG64 stream, the in-sample points compacted (in index order, as points[sel_in]) into the
//                       replica's slot of a ragged batch
//   rebuild_launch_full the (Multi)Ellipsoid construction of all runs x replicas point sets in one launch sequence
//                       (the ragged form the host-driven bootstrap of dynesty_amd/bootstrap.py uses)
//   boot_expand_kernel  the left-out points against the replica's ellipsoids: max over points of the min over
//                       ellipsoids of the squared normalised distance, max over replicas by atomicMax
//   boot_finish_kernel  expand = max(1, sqrt(.)); what the volume scaling needs: ndim * ln(expand), 0 if <= 1
//
// Streams: replica b of a run draws from PCG64 seeded (ent[0], ent[1] + b), increment words (ent[2], ent[3] + 2 b),
// where ent = four 64-bit words the caller drew from the run's own generator for this rebuild (the resident loop:
// ns_prepare).  oracle/nested_ref.py boot_generator restates it.
#include "ctx.h"
#include "rng_pcg64.h"
#include "stage_plan.h"

using namespace dh;

namespace {

constexpr int kBT = 256;

struct BootArgs {
  const double* pts;  // runs x n x d
  int runs, n, d, B, max_ells, multi;
  const uint64_t* ent;  // runs x 4
  const int* active;    // runs or null
  double* bpts;         // (runs B) x n x d   in-sample points, first n_arr rows
  unsigned char* sel;   // (runs B) x n       1 = in the sample
  int* n_arr;           // runs B
  int* act;             // runs B
  // the replicas' bounds
  int* nells;
  int* status;
  double* ctrs;
  double* ams;
  unsigned long long* ex2;  // runs: bits of the largest squared distance (>= 0: the bits order like the values)
  double* run_shift;        // runs
  double* expand;           // runs or null
  int* bstatus;             // runs or null: a replica whose construction failed fails the run's bound
};

__global__ void __launch_bounds__(kBT) boot_mask_kernel(BootArgs a) {
  extern __shared__ int lds_i[];
  int* sel = lds_i;          // n
  int* pos = lds_i + a.n;    // n
  __shared__ int part[kBT];
  const int b = blockIdx.x, run = blockIdx.y, t = threadIdx.x, n = a.n, d = a.d;
  const size_t rb = (size_t)run * a.B + b;
  if (a.active && !a.active[run]) {
    if (t == 0) {
      a.n_arr[rb] = 0;
      a.act[rb] = 0;
    }
    return;
  }
  for (int i = t; i < n; i += kBT) sel[i] = 0;
  __syncthreads();
  if (t == 0) {
    // idxs = rstate.integers(npoints, size=npoints); sel_in[unique(idxs)] = True
    Pcg64 g;
    const uint64_t* e = a.ent + (size_t)run * 4;
    U128 is = {e[0], e[1] + (uint64_t)b};
    U128 iq = {e[2], e[3] + 2ull * (uint64_t)b};
    g.seed(is, iq);
    for (int i = 0; i < n; ++i) sel[(int)g.bounded_lemire32((uint32_t)(n - 1))] = 1;  // Generator.integers(n)
  }
  __syncthreads();
  // n_in, then the reference's two repairs (both decided on the count BEFORE either is applied)
  const int per = (n + kBT - 1) / kBT, i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
  int c = 0;
  for (int i = i0; i < i1; ++i) c += sel[i];
  part[t] = c;
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int q = 0; q < kBT; ++q) tot += part[q];
    if (tot < 2 && n >= 2) sel[0] = sel[1] = 1;
    if (tot > n - 1) sel[0] = 0;
  }
  __syncthreads();
  c = 0;
  for (int i = i0; i < i1; ++i) c += sel[i];
  part[t] = c;
  __syncthreads();
  if (t == 0) {
    int run_sum = 0;
    for (int q = 0; q < kBT; ++q) {
      const int v = part[q];
      part[q] = run_sum;
      run_sum += v;
    }
    a.n_arr[rb] = run_sum;
    a.act[rb] = 1;
  }
  __syncthreads();
  int p = part[t];
  for (int i = i0; i < i1; ++i) {
    pos[i] = p;
    p += sel[i];
  }
  __syncthreads();
  if (a.bpts) {  // (null: the masks alone, for the friends bounds' radius)
    const double* src = a.pts + (size_t)run * n * d;
    double* dst = a.bpts + rb * n * d;
    for (int e = t; e < n * d; e += kBT) {
      const int i = e / d, j = e - i * d;
      if (sel[i]) dst[(size_t)pos[i] * d + j] = src[e];
    }
  }
  unsigned char* sg = a.sel + rb * n;
  for (int i = t; i < n; i += kBT) sg[i] = (unsigned char)sel[i];
}

__global__ void __launch_bounds__(kBT) boot_expand_kernel(BootArgs a) {
  __shared__ double red[kBT];
  const int b = blockIdx.x, run = blockIdx.y, t = threadIdx.x, n = a.n, d = a.d;
  const size_t rb = (size_t)run * a.B + b;
  if (!a.act[rb]) return;
  const int st = a.status[rb];
  if (st != DH_OK) {
    if (t == 0 && a.bstatus) atomicExch(&a.bstatus[run], st);
    return;
  }
  const int m = a.multi ? a.nells[rb] : 1;
  const double* src = a.pts + (size_t)run * n * d;
  const unsigned char* sg = a.sel + rb * n;
  double worst = 0.0;
  for (int i = t; i < n; i += kBT) {
    if (sg[i]) continue;
    const double* x = src + (size_t)i * d;
    double best = INFINITY;
    for (int e = 0; e < m; ++e) {
      const double* c = a.ctrs + (rb * a.max_ells + e) * d;
      const double* A = a.ams + (rb * a.max_ells + e) * (size_t)d * d;
      double q = 0.0;
      for (int r = 0; r < d; ++r) {
        double s = 0.0;
        for (int k = 0; k < d; ++k) s = fma(A[(size_t)r * d + k], x[k] - c[k], s);
        q = fma(x[r] - c[r], s, q);
      }
      best = fmin(best, q);
    }
    worst = fmax(worst, best);
  }
  red[t] = worst;
  __syncthreads();
  for (int s = kBT / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = fmax(red[t], red[t + s]);
    __syncthreads();
  }
  if (t == 0 && red[0] > 0.0) atomicMax(&a.ex2[run], (unsigned long long)__double_as_longlong(red[0]));
}

__global__ void boot_finish_kernel(BootArgs a) {
  const int run = blockIdx.x * blockDim.x + threadIdx.x;
  if (run >= a.runs) return;
  double ex = 1.0, shift = 0.0;
  if (!a.active || a.active[run]) {
    const double q = __longlong_as_double((long long)a.ex2[run]);
    ex = fmax(1.0, sqrt(q));
    if (ex > 1.0) shift = (double)a.d * log(ex);
  }
  a.run_shift[run] = shift;
  if (a.expand) a.expand[run] = ex;
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t dh::bootstrap_ws_bytes(int runs, int n, int d, int max_ells, int B) {
  const size_t rb = (size_t)runs * B, dd = (size_t)d * d;
  return al256(rb * n * d * 8) + al256(rb * n) + 4 * al256(rb * 4) + 2 * al256(rb * max_ells * d * 8) +
         3 * al256(rb * max_ells * dd * 8) + al256(rb * max_ells * 8) + al256((size_t)runs * 8) + 4096;
}

int dh::bootstrap_expand_launch(dh_ctx* ctx, int runs, const double* pts, int n, int d, int multi, int max_ells, int B,
                                const uint64_t* ent, const int* active, void* ws, double* run_shift, double* expand,
                                int* bstatus) {
  DH_CHECK_CTX(ctx);
  if (runs < 1 || B < 1 || n < 2 || d < 1 || max_ells < 1 || !pts || !ent || !ws || !run_shift)
    return fail(ctx, DH_ERR_ARG, "bootstrap: bad arguments");
  const size_t rb = (size_t)runs * B, dd = (size_t)d * d;
  char* p = (char*)ws;
  auto take = [&](size_t bytes) {
    char* o = p;
    p += al256(bytes);
    return o;
  };
  BootArgs a{};
  a.pts = pts;
  a.runs = runs;
  a.n = n;
  a.d = d;
  a.B = B;
  a.max_ells = max_ells;
  a.multi = multi ? 1 : 0;
  a.ent = ent;
  a.active = active;
  a.bpts = (double*)take(rb * n * d * 8);
  a.sel = (unsigned char*)take(rb * n);
  a.n_arr = (int*)take(rb * 4);
  a.act = (int*)take(rb * 4);
  a.nells = (int*)take(rb * 4);
  a.status = (int*)take(rb * 4);
  a.ctrs = (double*)take(rb * max_ells * d * 8);
  double* axl = (double*)take(rb * max_ells * d * 8);
  double* covs = (double*)take(rb * max_ells * dd * 8);
  a.ams = (double*)take(rb * max_ells * dd * 8);
  double* axes = (double*)take(rb * max_ells * dd * 8);
  double* lv = (double*)take(rb * max_ells * 8);
  a.ex2 = (unsigned long long*)take((size_t)runs * 8);
  a.run_shift = run_shift;
  a.expand = expand;
  a.bstatus = bstatus;
  const size_t lds = (size_t)n * 8;
  if (lds > 60 * 1024) return fail(ctx, DH_ERR_ARG, "bootstrap: n=%d points per run is more than the mask kernel holds", n);
  if (!hip_ok(ctx, hipMemsetAsync(a.ex2, 0, (size_t)runs * 8, ctx->stream), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(a.status, 0, rb * 4, ctx->stream), "memset"))
    return DH_ERR_HIP;
  hipLaunchKernelGGL(boot_mask_kernel, dim3(B, runs), dim3(kBT), lds, ctx->stream, a);
  if (!hip_ok(ctx, hipGetLastError(), "bootstrap mask launch")) return DH_ERR_HIP;
  const int rc = rebuild_launch_full(ctx, (int)rb, a.bpts, n, d, multi ? 0 : 1, max_ells, a.nells, a.status, a.ctrs, covs,
                                     a.ams, axes, axl, lv, nullptr, nullptr, a.act, a.n_arr);
  if (rc) return rc;
  hipLaunchKernelGGL(boot_expand_kernel, dim3(B, runs), dim3(kBT), 0, ctx->stream, a);
  hipLaunchKernelGGL(boot_finish_kernel, dim3((runs + 63) / 64), dim3(64), 0, ctx->stream, a);
  return hip_ok(ctx, hipGetLastError(), "bootstrap launch") ? DH_OK : DH_ERR_HIP;
}

int dh::boot_masks_launch(dh_ctx* ctx, int runs, int n, int B, const uint64_t* ent, const int* active,
                          unsigned char* sel, int* scratch) {
  if (runs < 1 || B < 1 || n < 2 || !ent || !sel || !scratch) return fail(ctx, DH_ERR_ARG, "bootstrap masks: bad arguments");
  const size_t lds = (size_t)n * 8;
  if (lds > 60 * 1024) return fail(ctx, DH_ERR_ARG, "bootstrap: n=%d points per run is more than the mask kernel holds", n);
  BootArgs a{};
  a.runs = runs;
  a.n = n;
  a.B = B;
  a.ent = ent;
  a.active = active;
  a.bpts = nullptr;
  a.sel = sel;
  a.n_arr = scratch;
  a.act = scratch + (size_t)runs * B;
  hipLaunchKernelGGL(boot_mask_kernel, dim3(B, runs), dim3(kBT), lds, ctx->stream, a);
  return hip_ok(ctx, hipGetLastError(), "bootstrap mask launch") ? DH_OK : DH_ERR_HIP;
}

extern "C" {

// see include/dynhip.h
int dh_bootstrap_expand(dh_ctx* ctx, int runs, const double* pts, int n, int d, int multi, int bootstrap,
                        const uint64_t* ent, double* expand, int32_t* n_in) {
  DH_CHECK_CTX(ctx);
  if (runs < 1 || bootstrap < 1 || n < 2 || d < 1 || !pts || !ent || !expand)
    return dh::fail(ctx, DH_ERR_ARG, "bootstrap_expand: bad arguments");
  const int me = multi ? (n / (2 * d) > 0 ? n / (2 * d) : 1) : 1;
  dh_stage::BootExpandBuf b;
  int rc = dh::arena_carve(ctx, [&](dh_stage::Carver& c) {
    dh_stage::carve_boot_expand(c, b, (size_t)runs, (size_t)n, (size_t)d,
                                dh::bootstrap_ws_bytes(runs, n, d, me, bootstrap));
  });
  if (rc) return rc;
  if (!dh::arena_fill(ctx, b.pts, pts, (size_t)runs * n * d) || !dh::arena_fill(ctx, b.ent, ent, (size_t)runs * 4))
    return DH_ERR_NOMEM;
  if (!dh::hip_ok(ctx, hipMemsetAsync(b.bstatus, 0, (size_t)runs * 4, ctx->stream), "memset")) return DH_ERR_HIP;
  rc = dh::bootstrap_expand_launch(ctx, runs, b.pts, n, d, multi, me, bootstrap, b.ent, nullptr, b.ws, b.shift, b.expand,
                                   b.bstatus);
  if (rc) return rc;
  std::vector<int> bs(runs);
  if (!dh::down(ctx, expand, b.expand, (size_t)runs) || !dh::down(ctx, bs.data(), b.bstatus, (size_t)runs)) return DH_ERR_HIP;
  // (the replicas' sample sizes sit right behind the points and the masks in the workspace: see bootstrap_expand_launch)
  if (n_in && !dh::down(ctx, n_in, (const int32_t*)((char*)b.ws + al256((size_t)runs * bootstrap * n * d * 8) +
                                                     al256((size_t)runs * bootstrap * n)),
                        (size_t)runs * bootstrap))
    return DH_ERR_HIP;
  if ((rc = dh_sync(ctx))) return rc;
  for (int r = 0; r < runs; ++r)
    if (bs[r] != DH_OK) return dh::fail(ctx, bs[r], "bootstrap_expand: a replica of run %d could not be bounded", r);
  return DH_OK;
}

}  // extern "C"
