// libdynhip.so: context, memory, events, problem registry (C ABI, see
// include/dynhip.h).  Kernels live in walk.hip / bound.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>

#include <cmath>

#include "ctx.h"
#include "npy_ziggurat_tables.h"
#include "rng_pcg64.h"

static std::string g_err;

namespace dh {

int fail(dh_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx)
    ctx->err = buf;
  else
    g_err = buf;
  return code;
}

bool hip_ok(dh_ctx* ctx, hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  fail(ctx, DH_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return false;
}

void arena_reset(dh_ctx* ctx) { ctx->arena_top = 0; }

int arena_reserve(dh_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->arena_cap) return DH_OK;
  // growing invalidates earlier arena pointers: only legal right after reset
  if (ctx->arena_top != 0) return fail(ctx, DH_ERR_NOMEM, "arena grow while in use");
  if (!hip_ok(ctx, hipStreamSynchronize(ctx->stream), "sync before arena grow")) return DH_ERR_HIP;
  if (ctx->arena) (void)hipFree(ctx->arena);
  ctx->arena = nullptr;
  ctx->arena_cap = 0;
  size_t cap = bytes + bytes / 2 + (1u << 20);
  if (!hip_ok(ctx, hipMalloc((void**)&ctx->arena, cap), "hipMalloc(arena)")) return DH_ERR_NOMEM;
  ctx->arena_cap = cap;
  return DH_OK;
}

void* arena_get(dh_ctx* ctx, size_t bytes) {
  size_t top = (ctx->arena_top + 255) & ~(size_t)255;
  if (top + bytes > ctx->arena_cap) {
    fail(ctx, DH_ERR_NOMEM, "arena overflow (%zu + %zu > %zu): reserve first", top, bytes,
         ctx->arena_cap);
    return nullptr;
  }
  ctx->arena_top = top + bytes;
  return ctx->arena + top;
}

bool get_problem(dh_ctx* ctx, int handle, ProblemDev* out) {
  if (handle < 0 || handle >= (int)ctx->problems.size() || !ctx->problems[handle].live) {
    fail(ctx, DH_ERR_ARG, "bad problem handle %d", handle);
    return false;
  }
  const dh_problem_rec& r = ctx->problems[handle];
  // every launcher takes its problem from here: an id the evaluators do not know never reaches a kernel
  if (!problem_ids_known(r.like_id, r.prior_id)) {
    fail(ctx, DH_ERR_ARG, "problem %d: likelihood id %d / prior id %d unknown to the evaluators", handle, r.like_id,
         r.prior_id);
    return false;
  }
  out->like_id = r.like_id;
  out->prior_id = r.prior_id;
  out->ndim = r.ndim;
  out->like_par = r.like_par;
  out->prior_par = r.prior_par;
  out->prec_t = r.prec_t;
  return true;
}

}  // namespace dh

using namespace dh;

extern "C" {

int dh_version(void) { return DH_VERSION; }

int dh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

dh_ctx* dh_create(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    fail(nullptr, DH_ERR_HIP, "no HIP device visible (%s); libdynhip has no CPU fallback",
         e == hipSuccess ? "count=0" : hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= n) {
    fail(nullptr, DH_ERR_ARG, "device %d out of range (have %d)", device, n);
    return nullptr;
  }
  dh_ctx* ctx = new dh_ctx();
  ctx->device = device;
  if (const char* e = getenv("DH_COOP_LAUNCH")) ctx->coop_launch = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("DH_SPLIT_RESIDENT_PCT")) ctx->split_resident_pct = atoi(e) >= 1 && atoi(e) <= 100 ? atoi(e) : 87;
  if (const char* e = getenv("DH_RWALK_FORM")) ctx->rwalk_form = atoi(e) == 1 ? 1 : atoi(e) == 2 ? 2 : 0;
  if (const char* e = getenv("DH_RWALK_ITEMS")) ctx->rwalk_items = atoi(e) != 0;
  if (const char* e = getenv("DH_RWALK_ITEMS_MB")) ctx->items_budget = (size_t)(atol(e) > 0 ? atol(e) : 1024) << 20;
  if (const char* e = getenv("DH_CUBE_FORM")) ctx->cube_form = atoi(e) == 1 ? 1 : atoi(e) == 2 ? 2 : 0;
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) ctx->num_cu = cu;
  }
  if (!hip_ok(ctx, hipSetDevice(device), "hipSetDevice") ||
      !hip_ok(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking), "hipStreamCreate") ||
      !hip_ok(ctx, hipMalloc((void**)&ctx->zig, (3 * 256 + 128) * sizeof(uint64_t)), "hipMalloc(zig)")) {
    g_err = ctx->err;
    delete ctx;
    return nullptr;
  }
  (void)hipMemcpy(ctx->zig, dh_zig_ki_host, 2048, hipMemcpyHostToDevice);
  (void)hipMemcpy(ctx->zig + 256, dh_zig_wi_bits_host, 2048, hipMemcpyHostToDevice);
  (void)hipMemcpy(ctx->zig + 512, dh_zig_fi_bits_host, 2048, hipMemcpyHostToDevice);
  {
    // PCG64 jump constants G_k = 1 + mult + ... + mult^(k-1) (mod 2^128), k = 1..64, as (hi, lo) pairs: the state k
    // steps ahead is S_0 + G_k (S_1 - S_0) (walkq.hip: one stream drawn by the 64 lanes of a wavefront)
    uint64_t jt[128];
    dh::U128 G = {0ull, 0ull};
    const dh::U128 m = {DH_PCG_MULT_HI, DH_PCG_MULT_LO}, one = {0ull, 1ull};
    for (int k = 0; k < 64; ++k) {
      G = dh::add128(dh::mul128(G, m), one);
      jt[2 * k] = G.hi;
      jt[2 * k + 1] = G.lo;
    }
    (void)hipMemcpy(ctx->zig + 768, jt, sizeof(jt), hipMemcpyHostToDevice);
  }
  if (arena_reserve(ctx, 8u << 20) != DH_OK) {
    g_err = ctx->err;
    dh_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void dh_destroy(dh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& p : ctx->problems) {
    if (p.like_par) (void)hipFree(p.like_par);
    if (p.prior_par) (void)hipFree(p.prior_par);
    if (p.prec_t) (void)hipFree(p.prec_t);
  }
  kept_free(ctx);
  merged_free(ctx);
  if (ctx->zig) (void)hipFree(ctx->zig);
  if (ctx->items) (void)hipFree(ctx->items);
  if (ctx->arena) (void)hipFree(ctx->arena);
  if (ctx->axes_t) (void)hipFree(ctx->axes_t);
  if (ctx->rebuild_ws) (void)hipFree(ctx->rebuild_ws);
  if (ctx->side_stream) {
    (void)hipStreamSynchronize(ctx->side_stream);
    (void)hipStreamDestroy(ctx->side_stream);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* dh_last_error(dh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int dh_sync(dh_ctx* ctx) {
  DH_CHECK_CTX(ctx);
  return hip_ok(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize") ? DH_OK : DH_ERR_HIP;
}

void* dh_stream(dh_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

void* dh_malloc(dh_ctx* ctx, uint64_t bytes) {
  if (!ctx) return nullptr;
  void* p = nullptr;
  (void)hipSetDevice(ctx->device);
  if (!hip_ok(ctx, hipMalloc(&p, bytes ? bytes : 8), "hipMalloc")) return nullptr;
  return p;
}

int dh_free(dh_ctx* ctx, void* dptr) {
  DH_CHECK_CTX(ctx);
  if (!dptr) return DH_OK;
  (void)hipStreamSynchronize(ctx->stream);
  return hip_ok(ctx, hipFree(dptr), "hipFree") ? DH_OK : DH_ERR_HIP;
}

int dh_memcpy_h2d(dh_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  DH_CHECK_CTX(ctx);
  if (!hip_ok(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "H2D"))
    return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_memcpy_d2h(dh_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  DH_CHECK_CTX(ctx);
  if (!hip_ok(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), "D2H"))
    return DH_ERR_HIP;
  return dh_sync(ctx);
}

int dh_memset(dh_ctx* ctx, void* dst, int value, uint64_t bytes) {
  DH_CHECK_CTX(ctx);
  return hip_ok(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream), "memset") ? DH_OK : DH_ERR_HIP;
}

void* dh_event_create(dh_ctx* ctx) {
  if (!ctx) return nullptr;
  hipEvent_t ev;
  if (!hip_ok(ctx, hipEventCreate(&ev), "hipEventCreate")) return nullptr;
  return (void*)ev;
}

int dh_event_destroy(dh_ctx* ctx, void* ev) {
  DH_CHECK_CTX(ctx);
  return hip_ok(ctx, hipEventDestroy((hipEvent_t)ev), "hipEventDestroy") ? DH_OK : DH_ERR_HIP;
}

int dh_event_record(dh_ctx* ctx, void* ev) {
  DH_CHECK_CTX(ctx);
  return hip_ok(ctx, hipEventRecord((hipEvent_t)ev, ctx->stream), "hipEventRecord") ? DH_OK
                                                                                    : DH_ERR_HIP;
}

int dh_event_elapsed_ms(dh_ctx* ctx, void* ev0, void* ev1, double* ms) {
  DH_CHECK_CTX(ctx);
  if (!hip_ok(ctx, hipEventSynchronize((hipEvent_t)ev1), "hipEventSynchronize")) return DH_ERR_HIP;
  float f = 0.f;
  if (!hip_ok(ctx, hipEventElapsedTime(&f, (hipEvent_t)ev0, (hipEvent_t)ev1), "hipEventElapsedTime"))
    return DH_ERR_HIP;
  *ms = (double)f;
  return DH_OK;
}

// The store step of both entry points (the arguments are checked): what is kept, in which bits.
// Matrices (GAUSS_PREC's P, a mixture's P_m): v^T P v only sees the symmetric part of P, and the evaluators read
// different triangles of it (upper, lower, all of it), so every copy holds (P + P^T) / 2.  (a + a) / 2 == a: a
// symmetric P is stored as given.
// The lane kernels' copies (ndim <= 32), zero padded to their N: GAUSS_PREC's transposed matrix for the column-sweep
// mat-vec (of the symmetrised P: its transpose is itself, bit for bit); a mixture's [mu_m (N), P_m (N x N)] per
// component (loglike_mix_lds).  mix_m: the number of components, 0 for every other likelihood.
static int problem_store(dh_ctx* ctx, int ndim, int like_id, const double* like_par, int n_like_par, int prior_id,
                         const double* prior_par, int n_prior_par, int mix_m) {
  const size_t nn = (size_t)ndim * ndim, blk_len = 1 + ndim + nn;
  std::vector<double> lp(like_par, like_par + n_like_par);
  const int nmat = like_id == DH_LIKE_GAUSS_MIX ? mix_m : like_id == DH_LIKE_GAUSS_PREC ? 1 : 0;
  for (int m = 0; m < nmat; ++m) {
    const size_t base = like_id == DH_LIKE_GAUSS_MIX ? 1 + (size_t)m * blk_len + 1 + ndim : 1;
    for (int i = 0; i < ndim; ++i)
      for (int j = 0; j < ndim; ++j) {
        const size_t ij = base + (size_t)i * ndim + j, ji = base + (size_t)j * ndim + i;
        lp[ij] = 0.5 * (like_par[ij] + like_par[ji]);
      }
  }
  const bool want_t = nmat > 0 && ndim <= kMaxRegDim;
  const int N = want_t ? pad_dim(ndim) : 0;
  std::vector<double> pt((size_t)(like_id == DH_LIKE_GAUSS_MIX ? mix_m * (N + N * N) : N * N), 0.0);
  if (want_t && like_id == DH_LIKE_GAUSS_PREC)
    for (int i = 0; i < ndim; ++i)
      for (int j = 0; j < ndim; ++j) pt[(size_t)j * N + i] = lp[1 + (size_t)i * ndim + j];
  if (want_t && like_id == DH_LIKE_GAUSS_MIX)
    for (int m = 0; m < mix_m; ++m) {
      const double* blk = lp.data() + 1 + (size_t)m * blk_len + 1;  // mu_m, then P_m
      double* out = pt.data() + (size_t)m * (N + N * N);
      for (int i = 0; i < ndim; ++i) {
        out[i] = blk[i];
        for (int j = 0; j < ndim; ++j) out[N + (size_t)i * N + j] = blk[ndim + (size_t)i * ndim + j];
      }
    }
  dh_problem_rec r;
  r.live = true;
  r.ndim = ndim;
  r.like_id = like_id;
  r.prior_id = prior_id;
  r.n_like = n_like_par;
  r.n_prior = n_prior_par;
  r.mix_m = mix_m;
  (void)hipSetDevice(ctx->device);
  // an error below gives back what was allocated so far (hipFree(nullptr) does nothing)
  auto give_up = [&r](int code) {
    (void)hipFree(r.like_par);
    (void)hipFree(r.prior_par);
    (void)hipFree(r.prec_t);
    return code;
  };
  if (!hip_ok(ctx, hipMalloc((void**)&r.like_par, sizeof(double) * (n_like_par + 1)), "hipMalloc") ||
      !hip_ok(ctx, hipMalloc((void**)&r.prior_par, sizeof(double) * (n_prior_par + 2)), "hipMalloc") ||
      (want_t && !hip_ok(ctx, hipMalloc((void**)&r.prec_t, sizeof(double) * pt.size()), "hipMalloc")))
    return give_up(DH_ERR_NOMEM);
  if (!hip_ok(ctx, hipMemcpy(r.like_par, lp.data(), sizeof(double) * n_like_par, hipMemcpyHostToDevice), "H2D like_par") ||
      (n_prior_par && !hip_ok(ctx, hipMemcpy(r.prior_par, prior_par, sizeof(double) * n_prior_par, hipMemcpyHostToDevice),
                              "H2D prior_par")) ||
      (want_t && !hip_ok(ctx, hipMemcpy(r.prec_t, pt.data(), sizeof(double) * pt.size(), hipMemcpyHostToDevice), "H2D prec_t")))
    return give_up(DH_ERR_HIP);
  for (size_t i = 0; i < ctx->problems.size(); ++i)
    if (!ctx->problems[i].live) {
      ctx->problems[i] = r;
      return (int)i;
    }
  ctx->problems.push_back(r);
  return (int)ctx->problems.size() - 1;
}

int dh_problem_create(dh_ctx* ctx, int ndim, int like_id, const double* like_par, int n_like_par,
                      int prior_id, const double* prior_par, int n_prior_par) {
  DH_CHECK_CTX(ctx);
  if (ndim < 1) return fail(ctx, DH_ERR_ARG, "ndim=%d", ndim);
  int need_like = like_id == DH_LIKE_GAUSS_PREC ? 1 + ndim * ndim : 1;
  if (like_id < 0 || like_id > DH_LIKE_EGGBOX || n_like_par < need_like)
    return fail(ctx, DH_ERR_ARG, "likelihood id %d needs %d parameters, got %d", like_id, need_like,
                n_like_par);
  int need_prior = prior_id == DH_PRIOR_IDENTITY ? 0 : 2;
  if (prior_id < 0 || prior_id > DH_PRIOR_NORMAL || n_prior_par < need_prior)
    return fail(ctx, DH_ERR_ARG, "prior id %d needs %d parameters, got %d", prior_id, need_prior,
                n_prior_par);
  if (!like_par || (n_prior_par > 0 && !prior_par))
    return fail(ctx, DH_ERR_ARG, "problem_create: null pointer");
  return problem_store(ctx, ndim, like_id, like_par, n_like_par, prior_id, prior_par, n_prior_par, 0);
}

// Every id 0..3 in any pairing.  A pair of the ids 0..2 IS dh_problem_create's (the same checks, the same stored
// bits); a pair with DH_LIKE_GAUSS_MIX or DH_PRIOR_TABLE is checked here and stored by the same problem_store.
// The parameters of an older id paired with a new one are checked as dh_problem_create checks them (at least the
// count it needs, finite here besides): AFFINE's a and NORMAL's sigma are not required to be positive.
int dh_problem_create_ex(dh_ctx* ctx, int ndim, int like_id, const double* like_par, int n_like_par, int prior_id,
                         const double* prior_par, int n_prior_par) {
  DH_CHECK_CTX(ctx);
  if (like_id != DH_LIKE_GAUSS_MIX && prior_id != DH_PRIOR_TABLE)
    return dh_problem_create(ctx, ndim, like_id, like_par, n_like_par, prior_id, prior_par, n_prior_par);
  if (ndim < 1) return fail(ctx, DH_ERR_ARG, "ndim=%d", ndim);
  if (like_id < 0 || like_id > DH_LIKE_GAUSS_MIX) return fail(ctx, DH_ERR_ARG, "likelihood id %d", like_id);
  if (prior_id < 0 || prior_id > DH_PRIOR_TABLE) return fail(ctx, DH_ERR_ARG, "prior id %d", prior_id);
  if (!like_par || n_like_par < 1 || (n_prior_par > 0 && !prior_par) || n_prior_par < 0)
    return fail(ctx, DH_ERR_ARG, "problem_create_ex: null pointer or no likelihood parameter");
  const long long nn = (long long)ndim * ndim;
  int M = 0;
  if (like_id == DH_LIKE_GAUSS_MIX) {
    const double m = like_par[0];
    if (!(m >= 1.0 && m <= (double)DH_MIX_MAX) || m != (double)(int)m)
      return fail(ctx, DH_ERR_ARG, "Gaussian mixture: M = %g components, need an integer in 1..%d", m, DH_MIX_MAX);
    M = (int)m;
    const long long need = 1 + M * (1 + (long long)ndim + nn);
    if ((long long)n_like_par != need)
      return fail(ctx, DH_ERR_ARG, "Gaussian mixture of %d components in %d dimensions has %lld parameters, got %d", M,
                  ndim, need, n_like_par);
  } else {
    const long long need = like_id == DH_LIKE_GAUSS_PREC ? 1 + nn : 1;
    if ((long long)n_like_par < need)
      return fail(ctx, DH_ERR_ARG, "likelihood id %d needs %lld parameters, got %d", like_id, need, n_like_par);
  }
  if (prior_id == DH_PRIOR_TABLE) {
    if ((long long)n_prior_par != 3ll * ndim)
      return fail(ctx, DH_ERR_ARG, "prior table of %d coordinates has %d parameters, got %d", ndim, 3 * ndim, n_prior_par);
  } else if (n_prior_par < (prior_id == DH_PRIOR_IDENTITY ? 0 : 2)) {
    return fail(ctx, DH_ERR_ARG, "prior id %d needs 2 parameters, got %d", prior_id, n_prior_par);
  }
  for (int i = 0; i < n_like_par; ++i)
    if (!std::isfinite(like_par[i])) return fail(ctx, DH_ERR_ARG, "likelihood parameter %d is not finite", i);
  for (int i = 0; i < n_prior_par; ++i)
    if (!std::isfinite(prior_par[i])) return fail(ctx, DH_ERR_ARG, "prior parameter %d is not finite", i);
  if (prior_id == DH_PRIOR_TABLE)
    for (int i = 0; i < ndim; ++i) {
      const double kind = prior_par[3 * i], p1 = prior_par[3 * i + 2];
      if (kind != (double)DH_TABLE_UNIFORM && kind != (double)DH_TABLE_NORMAL && kind != (double)DH_TABLE_LOGUNIFORM)
        return fail(ctx, DH_ERR_ARG, "prior table row %d: kind %g (0 uniform, 1 normal, 2 log-uniform)", i, kind);
      if (kind != (double)DH_TABLE_LOGUNIFORM && !(p1 > 0.0))
        return fail(ctx, DH_ERR_ARG, "prior table row %d: width / sigma %g is not positive", i, p1);
    }
  if (like_id == DH_LIKE_GAUSS_MIX)
    for (int m = 0; m < M; ++m)
      for (int i = 0; i < ndim; ++i)
        if (!(like_par[1 + (size_t)m * (1 + ndim + nn) + 1 + ndim + (size_t)i * ndim + i] > 0.0))
          return fail(ctx, DH_ERR_ARG, "Gaussian mixture: component %d has a non-positive diagonal entry (%d)", m, i);
  return problem_store(ctx, ndim, like_id, like_par, n_like_par, prior_id, prior_par, n_prior_par, M);
}

int dh_problem_destroy(dh_ctx* ctx, int problem) {
  DH_CHECK_CTX(ctx);
  ProblemDev p;
  if (!get_problem(ctx, problem, &p)) return DH_ERR_ARG;
  (void)hipStreamSynchronize(ctx->stream);
  dh_problem_rec& r = ctx->problems[problem];
  (void)hipFree(r.like_par);
  (void)hipFree(r.prior_par);
  if (r.prec_t) (void)hipFree(r.prec_t);
  r = dh_problem_rec();
  return DH_OK;
}

}  // extern "C"
