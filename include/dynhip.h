/* dynhip.h -- C ABI of libdynhip.so, the MI355X (gfx950) implementation of
 * dynesty's bounding + proposal hot path.
 *
 * The reference (joshspeagle/dynesty 3.0.0) is pure Python and has no FFI of
 * its own; the entry points below are what a ctypes binding for this path
 * binds to.  Each one names the reference function(s) it replaces
 * (file:line relative to /root/reference/py/dynesty/).  INTEGRATION.md shows
 * the reference-side stubs; dynesty_amd/_lib.py is the binding used here.
 *
 * Conventions
 *   - plain C types only; all matrices are C-contiguous row-major float64.
 *   - every function returns DH_OK (0) or a negative DH_ERR_* code; the
 *     message is available from dh_last_error(ctx).  The Python shim maps the
 *     codes back to the exception types the reference raises.
 *   - host-pointer entry points copy in, launch on the context's stream, copy
 *     out and synchronise before returning; the library never keeps a host
 *     pointer.  `*_dev` entry points take device pointers (from dh_malloc),
 *     only enqueue work on the context's stream and do NOT synchronise.
 *   - a dh_ctx is bound to one device and one stream; calls on one context are
 *     serialised.  No global state: fork/spawn-safe until the first dh_create.
 *   - RNG: one numpy-compatible PCG64 stream per walker, 4 x uint64 words
 *     {state_hi, state_lo, inc_hi, inc_lo} (numpy PCG64().state['state']).
 */
#ifndef DYNHIP_H
#define DYNHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_VERSION 100

#define DH_OK 0
#define DH_ERR_VALUE (-1)   /* ValueError: single point / singular covariance (bounding.py:1405-1407, 220-224) */
#define DH_ERR_CONTAIN (-2) /* RuntimeError: failed to contain all the points (bounding.py:1451-1453) */
#define DH_ERR_REGION (-3)  /* RuntimeError: Rejecting invalid MultiEllipsoid region (bounding.py:683-685) */
#define DH_ERR_SLICE (-4)   /* RuntimeError: slice sampler failed, x == 0 (internal_samplers.py:1188-1199) */
#define DH_ERR_HIP (-5)     /* HIP runtime failure */
#define DH_ERR_ARG (-6)     /* bad argument (unsupported dimension, null pointer, bad handle) */
#define DH_ERR_QZERO (-7)   /* RuntimeError: Ellipsoid check failed q=0 (bounding.py:565-572) */
#define DH_ERR_NOMEM (-8)

/* likelihood / prior ids -- twins of dynesty_amd/problems.py */
#define DH_LIKE_GAUSS_IID 0  /* -0.5 sum v^2 + c                par = [c]        */
#define DH_LIKE_GAUSS_PREC 1 /* -0.5 v^T P v + c                par = [c, P]     */
/* (P need not be symmetric: v^T P v only sees (P + P^T) / 2, and that is what dh_problem_create stores -- every
 * evaluator, whichever triangle of the matrix it reads, computes the full quadratic form.  A symmetric P is stored bit
 * for bit as given.) */
#define DH_LIKE_EGGBOX 2     /* (2 + prod cos((2 tmax v - tmax)/2))^5  par = [tmax] */
#define DH_PRIOR_IDENTITY 0  /* v = u                                            */
#define DH_PRIOR_AFFINE 1    /* v = a (2u - 1) + b              par = [a, b]     */
#define DH_PRIOR_NORMAL 2    /* v = mu + sigma ndtri(u)         par = [mu, sigma]*/
/* The two ids below are created through dh_problem_create_ex only (dh_problem_create refuses them).
 * DH_LIKE_GAUSS_MIX: logl = a* + log(sum_m exp(a_m - a*)), a* = max_m a_m,
 *                    a_m = c_m - (v - mu_m)^T P_m (v - mu_m) / 2;  M = 1 gives a_0 itself (no exp, no log)
 *   par = [M, then per component m: c_m, mu_m (ndim), P_m (ndim x ndim, row-major)],  1 <= M <= DH_MIX_MAX;
 *   c_m = ln w_m + ln det P_m / 2 - (ndim / 2) ln 2 pi for a normalised mixture.  Every P_m is stored symmetrised.
 * DH_PRIOR_TABLE: one row [kind, p0, p1] per coordinate, par = ndim rows
 *   DH_TABLE_UNIFORM     v = fma(u, p1, p0)        p0 = lo,     p1 = hi - lo     (p1 > 0)
 *   DH_TABLE_NORMAL      v = p0 + p1 ndtri(u)      p0 = mu,     p1 = sigma       (p1 > 0)
 *   DH_TABLE_LOGUNIFORM  v = exp(fma(u, p1, p0))   p0 = ln lo,  p1 = ln(hi / lo) */
#define DH_LIKE_GAUSS_MIX 3
#define DH_PRIOR_TABLE 3
#define DH_MIX_MAX 8
#define DH_TABLE_UNIFORM 0
#define DH_TABLE_NORMAL 1
#define DH_TABLE_LOGUNIFORM 2

/* per-dimension boundary flags (reference kwargs periodic / reflective,
 * utils.py:950-976 get_nonbounded) */
#define DH_BC_HARD 0
#define DH_BC_PERIODIC 1
#define DH_BC_REFLECT 2

typedef struct dh_ctx dh_ctx;

/* ---- context ----------------------------------------------------------- */
int dh_version(void);
int dh_device_count(void);
/* NULL on failure (no HIP device / bad ordinal): the message is in
 * dh_last_error(NULL).  There is no CPU fallback. */
dh_ctx* dh_create(int device);
void dh_destroy(dh_ctx* ctx);
const char* dh_last_error(dh_ctx* ctx);
int dh_sync(dh_ctx* ctx);
/* the hipStream_t every launch of this context goes to */
void* dh_stream(dh_ctx* ctx);

/* ---- device memory + events (for resident data and on-stream timing) --- */
void* dh_malloc(dh_ctx* ctx, uint64_t bytes);
int dh_free(dh_ctx* ctx, void* dptr);
int dh_memcpy_h2d(dh_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);
int dh_memcpy_d2h(dh_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);
int dh_memset(dh_ctx* ctx, void* dst_dev, int value, uint64_t bytes);
void* dh_event_create(dh_ctx* ctx);
int dh_event_destroy(dh_ctx* ctx, void* ev);
int dh_event_record(dh_ctx* ctx, void* ev);                     /* on dh_stream(ctx) */
int dh_event_elapsed_ms(dh_ctx* ctx, void* ev0, void* ev1, double* ms); /* syncs ev1 */

/* ---- problems: device twins of the user's loglikelihood/prior_transform --
 * callbacks (internal_samplers.py:957-958; dynesty.py:529-557).  Returns a
 * handle >= 0 or a DH_ERR_* code. */
int dh_problem_create(dh_ctx* ctx, int ndim, int like_id, const double* like_par,
                      int n_like_par, int prior_id, const double* prior_par,
                      int n_prior_par);
/* Every id 0..3 in any pairing.  A pair of the ids 0..2 goes to dh_problem_create unchanged (same checks, same
 * stored bits).  With DH_LIKE_GAUSS_MIX or DH_PRIOR_TABLE it answers DH_ERR_ARG (message in dh_last_error) for: M
 * outside 1..DH_MIX_MAX or not an integer; n_like_par != 1 + M (1 + ndim + ndim^2); n_prior_par != 3 ndim; a table
 * kind outside 0..2; a parameter that is not finite; p1 <= 0 in a uniform or normal row; a diagonal entry <= 0 of a
 * P_m.  The parameters of an older id paired with a new one are held to dh_problem_create's rules (at least the count
 * that id needs; DH_PRIOR_AFFINE's a and DH_PRIOR_NORMAL's sigma are not required to be positive), plus finiteness. */
int dh_problem_create_ex(dh_ctx* ctx, int ndim, int like_id, const double* like_par,
                         int n_like_par, int prior_id, const double* prior_par,
                         int n_prior_par);
int dh_problem_destroy(dh_ctx* ctx, int problem);
/* logl/v for k points: the batched form of loglikelihood(prior_transform(u)) */
int dh_problem_eval(dh_ctx* ctx, int problem, int k, const double* u, double* v,
                    double* logl);

/* ---- RNG ---------------------------------------------------------------- */
/* numpy: [PCG64(c).state for c in SeedSequence(entropy).spawn(first+k)[first:]]
 * (utils.py:1002-1009 get_seed_sequence + :993-999 get_random_generator).
 * entropy_words = the entropy ints coerced to little-endian uint32 words. */
int dh_seed_children(dh_ctx* ctx, const uint32_t* entropy_words, int n_words,
                     uint32_t first_child, int k, uint64_t* states /* k*4 */);
/* test hook: from one state draw n_normal standard_normal() then n_unif
 * random(); returns the advanced state. */
int dh_rng_stream(dh_ctx* ctx, const uint64_t* state4, int n_normal, int n_unif,
                  double* normals, double* unifs, uint64_t* state4_out);

/* ---- membership ---------------------------------------------------------
 * MultiEllipsoid.contains/within/overlap (bounding.py:502-523) and
 * Ellipsoid.contains (bounding.py:286-305) for k points against m ellipsoids.
 *   mode 0: (x-c)^T A (x-c) < 1          (MultiEllipsoid, strict)
 *   mode 1: sqrt((x-c)^T A (x-c)) <= 1   (Ellipsoid)
 * count[i]  = number of ellipsoids containing x_i
 * mask      = bit matrix, word (a * ceil(k/64) + i/64), bit i%64 set iff x_i is
 *             inside ellipsoid a  (one 64-lane ballot per word); may be NULL
 * quad      = k*m quadratic forms (row i = point i); may be NULL */
int dh_contains(dh_ctx* ctx, const double* x, int k, int d, const double* ctrs,
                const double* ams, int m, int mode, int32_t* count,
                uint64_t* mask, double* quad);
/* diagnostic: the resident loop's membership test of its start points
 * (Sampler.propose_live, sampler.py:484-489) as one launch of its own.  runs
 * queues of wpr candidates (x: runs*wpr x d); candidate w of run r is tested
 * against the first nells[r] of that run's max_ells ellipsoids (ctrs
 * runs*max_ells*d, ams runs*max_ells*d*d; nells NULL: the first one only).
 *   strict 1: inside iff some (x-c)^T A (x-c) < 1;  strict 0: sqrt(..) <= 1
 * A run is served when run_mode[r] == my_mode (run_mode NULL: always) and
 * bstatus[r] == 0 (bstatus NULL: always).  flag and first (runs each; first may
 * be NULL) are IN/OUT: a served run with a candidate outside gets flag[r] |= 1
 * and first[r] = min(first[r], lowest queue index outside); everything else
 * comes back as it was sent.  DH_ERR_ARG: a NULL required pointer, runs / wpr /
 * d / max_ells < 1, d > 512, an nells[r] outside 0..max_ells. */
int dh_contains_runs(dh_ctx* ctx, const double* x, int runs, int wpr, int d,
                     const double* ctrs, const double* ams, const int32_t* nells,
                     int max_ells, int strict, const int32_t* run_mode, int my_mode,
                     const int32_t* bstatus, int32_t* flag, int32_t* first);

/* ---- rebuild -------------------------------------------------------------
 * mode 0: MultiEllipsoid.update(points) without bootstrap (bounding.py:632-686)
 *         = bounding_ellipsoid (:1387-1461) + _bounding_ellipsoids (:1464-1563,
 *         incl. scipy kmeans2 k=2 iter=10) + improve_covar_mat (:1311-1384)
 *         + the all-points-covered check (:683-685).
 * mode 1: Ellipsoid.update(points) without bootstrap (bounding.py:345-375).
 * Outputs for the nells ellipsoids, in the reference's list order (left subtree
 * first): ctrs nells*d, covs/ams/axes nells*d*d (axes: column i = axis i, sorted
 * by ascending eigenvalue, sign fixed so the largest component is positive),
 * axlens nells*d, logvols nells; leaf_of_point[n] = index of the ellipsoid whose
 * cluster owns each point (may be NULL); nnodes = visited tree nodes (may be
 * NULL).  Errors: DH_ERR_VALUE / DH_ERR_CONTAIN / DH_ERR_REGION as the
 * reference raises; DH_ERR_NOMEM if more than max_ells ellipsoids result.
 * Dimensions: d <= 44 runs the LDS-resident kernel pipeline (rebuild.hip);
 * 44 < d <= 512 the wide path (wide.hip: multi-workgroup covariance /
 * eigensolver / Mahalanobis maximum; mode 0 as a host recursion over device node
 * work).  The batched / ragged forms below take any d <= 512 too; above 44 their
 * sets go through the wide constructions one after the other. */
int dh_rebuild(dh_ctx* ctx, const double* pts, int n, int d, int mode, int max_ells,
               int32_t* nells, double* ctrs, double* covs, double* ams, double* axes,
               double* axlens, double* logvols, int32_t* leaf_of_point,
               int32_t* nnodes);
/* `runs` independent live sets (pts: runs*n*d) in one launch, one workgroup per
 * run; outputs strided by max_ells per run; status[run] holds the per-run
 * DH_ERR code (the call itself only fails on launch errors). */
int dh_rebuild_batch_dev(dh_ctx* ctx, int runs, const double* pts, int n, int d,
                         int mode, int max_ells, int32_t* nells, int32_t* status,
                         double* ctrs, double* covs, double* ams, double* axes,
                         double* axlens, double* logvols, int32_t* leaf_of_point,
                         int32_t* nnodes);

/* Ragged batch: run r bounds the first n_arr[r] (<= n_max) rows of its
 * n_max x d block -- the B bootstrap replicas of _ellipsoid_bootstrap_expand
 * (bounding.py:1619-1648) in one launch. */
int dh_rebuild_ragged_dev(dh_ctx* ctx, int runs, const double* pts, int n_max,
                          const int32_t* n_arr, int d, int mode, int max_ells,
                          int32_t* nells, int32_t* status, double* ctrs, double* covs,
                          double* ams, double* axes, double* axlens, double* logvols);

/* Ellipsoid.__init__(ctr, cov) (bounding.py:201-240) for m covariance matrices:
 * eigen-decomposition -> axes (ascending, sign-canonical), axlens, am, logvol.
 * DH_ERR_VALUE if an eigenvalue is not positive/finite. */
int dh_ell_from_cov(dh_ctx* ctx, int m, int d, const double* covs, double* axes,
                    double* axlens, double* ams, double* logvols);
/* Ellipsoid.scale_to_logvol (bounding.py:242-276) applied in place to m
 * ellipsoids with per-ellipsoid targets (MultiEllipsoid.scale_to_logvol,
 * bounding.py:478-495, supplies logvol_ells + shift). */
int dh_scale_to_logvol(dh_ctx* ctx, int m, int d, double* covs, double* ams,
                       double* axes, double* axlens, double* logvols,
                       const double* targets);

/* improve_covar_mat (bounding.py:1311-1384; exercised by the reference's tests/test_ellipsoid.py:242-255
 * test_bounds): for each of m symmetric d x d matrices the 100-trial regularisation loop of the rebuild
 * kernels -- eigenvalue floor at 10 * max / 1e12 when the condition number exceeds 1e12, blend towards
 * the identity when the eigenvalues are not finite / not positive, identity after 100 failures.
 * Outputs: good[e] = 1 iff the input needed no change (the reference's `good_mat`), the returned
 * covariance, its inverse and the axes (eigenvectors * sqrt(eigenvalues), ascending, sign-canonical).
 * d <= 44. */
int dh_improve_covar_mat(dh_ctx* ctx, int m, int d, const double* covs_in, int32_t* good,
                         double* covs, double* ams, double* axes);

/* Sampler.update_bound's enlargement (sampler.py:506-508):
 * bound.scale_to_logvol(bound.logvol + log(enlarge)) for `runs` bounds laid out
 * as by dh_rebuild_batch_dev (max_ells slots per run, nells[run] live): every
 * live ellipsoid's target is its own logvol + log_enlarge (bounding.py:485-490). */
int dh_enlarge_batch_dev(dh_ctx* ctx, int runs, int max_ells, const int32_t* nells,
                         int d, double* covs, double* ams, double* axes,
                         double* axlens, double* logvols, double log_enlarge);
/* diagnostic: the resident loop's enlarge launch as one launch of its own, on
 * host arrays laid out as above (updated in place).  Slot s of run r is scaled
 * to logvols + run_shift[r] + log_enlarge when s < nells[r] and active[r] != 0
 * (active NULL: every run; run_shift NULL: no per-run shift).  With run_shift
 * given, a run whose run_shift[r] == 0 is left alone when log_enlarge == 0 (a
 * bootstrap expansion factor of 1).  Everything else comes back as it was sent.
 * DH_ERR_ARG: a NULL required pointer, runs / max_ells / d < 1, d > 512, an
 * nells[r] outside 0..max_ells.  dh_scale_to_logvol refuses d > 512 too. */
int dh_enlarge_runs(dh_ctx* ctx, int runs, int max_ells, const int32_t* nells, int d,
                    double* covs, double* ams, double* axes, double* axlens,
                    double* logvols, double log_enlarge, const int32_t* active,
                    const double* run_shift);

/* ---- proposals ----------------------------------------------------------
 * RWalkSampler.sample over a batch of k walkers = generic_random_walk +
 * propose_ball_point + randsphere (internal_samplers.py:866-1035,
 * bounding.py:1288-1297), prior/likelihood evaluated in-kernel.
 *   u0        k*ndim   start points (copies of live points)
 *   axes      m*ncdim*ncdim proposal frames, column i = axis i
 *   axes_idx  k        frame per walker (NULL: all use frame 0)
 *   bc        ndim     DH_BC_* flags or NULL (all hard)
 *   rng       k*4      PCG64 states in
 *   outputs   u,v k*ndim; logl k; naccept,nreject k; rng_out k*4 (may be NULL)
 * ncalls == walks for every walker (internal_samplers.py:925-944). */
int dh_rwalk_batch(dh_ctx* ctx, int problem, int k, int ndim, int ncdim,
                   const double* u0, const double* axes, int m,
                   const int32_t* axes_idx, double scale, double loglstar,
                   int walks, const int8_t* bc, const uint64_t* rng, double* u,
                   double* v, double* logl, int32_t* naccept, int32_t* nreject,
                   uint64_t* rng_out);
int dh_rwalk_batch_dev(dh_ctx* ctx, int problem, int k, int ndim, int ncdim,
                       const double* u0, const double* axes, int m,
                       const int32_t* axes_idx, double scale, double loglstar,
                       int walks, const int8_t* bc, const uint64_t* rng,
                       double* u, double* v, double* logl, int32_t* naccept,
                       int32_t* nreject, uint64_t* rng_out);

/* Kernel form of the fused rwalk entry points (dh_rwalk_batch[_dev], dh_rwalk_batch_philox[_dev], the
 * rwalk stage of dh_ns_ensemble).  Two kernels implement generic_random_walk
 * (internal_samplers.py:866-986) on the same generator streams: one walker per lane (any ndim <= 32, any
 * options), and one walker on four lanes of a wavefront with the frame product / Gaussian quadratic form
 * on the fp64 matrix cores (built for ndim == ncdim in 2..32; periodic / reflective coordinates and every
 * fused prior included).  Accept / reject counts and generator end states of the two are identical,
 * coordinates agree to rounding (~1e-15: sums over a vector are taken in a different order).
 *   form 0 (default)  four lanes per walker wherever built: decided by the problem alone (its dimension, and
 *                     ndim == ncdim), never by the launch size or the device, so that a run's results do
 *                     not depend on how an ensemble is sharded
 *   form 1            one walker per lane always
 *   form 2            same as 0 (kept for callers of the round-3 interface)
 * The environment variable DH_RWALK_FORM sets the initial value.  DH_RWALK_ITEMS=0 keeps the PCG64 generator of
 * the four-lane form inside the walk kernel instead of a generator pass ahead of it (same streams, same results);
 * DH_RWALK_ITEMS_MB bounds that pass's buffer (default 1024: larger launches go in chunks of walkers). */
int dh_set_rwalk_form(dh_ctx* ctx, int form);

/* The four-lane form's PCG64 generator as a pass of its own ahead of the walk (on = 1, default: every walker's
 * walks x (ndim normals + 1 uniform) items written to a context buffer by one wavefront per walker, read back by
 * the walk kernel) or inside the walk kernel (on = 0).  Same streams, bit-identical results either way.
 * budget_bytes > 0 bounds the buffer (default 2^30): a launch whose streams need more runs in chunks of walkers;
 * 0 leaves the bound as it is.  (RWalkSampler.sample draws them in internal_samplers.py:1007-1021.) */
int dh_set_rwalk_items(dh_ctx* ctx, int on, long long budget_bytes);

/* Throughput mode of RWalkSampler.sample: the same walk (generic_random_walk, propose_ball_point,
 * randsphere; internal_samplers.py:866-1035, bounding.py:1288-1297) drawing from hiprand's Philox4x32-10
 * device generator instead of NumPy-compatible PCG64 streams: walker i uses subsequence sequence0 + i of
 * `seed`, starting `offset` draws in, so no generator state is read or written.  Normals are hiprand's
 * fp32 Box-Muller pairs widened to fp64 (the step direction is resolved to 6e-8; the proposal stays
 * exactly symmetric), uniforms hiprand_uniform_double.  Everything else -- frame product, wrap / reflect,
 * unitcheck, prior transform, log-likelihood, accept rule, counters -- is the parity kernel's code.
 * NOT stream-compatible with the reference: validated statistically (tests/test_gpu_philox.py: the
 * reference's KS tests of tests/test_ellipsoid.py on device output, chain statistics against the parity
 * mode).  Any ndim <= 512 (above 32 the wave-per-walker kernel).  A caller advances `offset` by at least walks * (ndim + 8) per launch (or changes
 * `seed`) to get fresh draws. */
int dh_rwalk_batch_philox(dh_ctx* ctx, int problem, int k, int ndim, int ncdim, const double* u0,
                          const double* axes, int m, const int32_t* axes_idx, double scale,
                          double loglstar, int walks, const int8_t* bc, uint64_t seed,
                          uint64_t sequence0, uint64_t offset, double* u, double* v, double* logl,
                          int32_t* naccept, int32_t* nreject);
int dh_rwalk_batch_philox_dev(dh_ctx* ctx, int problem, int k, int ndim, int ncdim, const double* u0,
                              const double* axes, int m, const int32_t* axes_idx, double scale,
                              double loglstar, int walks, const int8_t* bc, uint64_t seed,
                              uint64_t sequence0, uint64_t offset, double* u, double* v, double* logl,
                              int32_t* naccept, int32_t* nreject);

/* Lock-step form for an arbitrary host likelihood: ONE propose_ball_point
 * (internal_samplers.py:989-1035) per walker -- draws, frame mat-vec,
 * wrap/reflect, unitcheck -- returning the proposals, their in-cube flags and the
 * advanced streams; the caller evaluates prior_transform/loglikelihood on the
 * host, applies the accept rule (internal_samplers.py:946-968) and calls again. */
int dh_rwalk_propose(dh_ctx* ctx, int k, int ndim, int ncdim, const double* u0,
                     const double* axes, int m, const int32_t* axes_idx, double scale,
                     const int8_t* bc, const uint64_t* rng, double* u_prop,
                     int32_t* inside, uint64_t* rng_out);

/* Slice sampling in lock step with a HOST likelihood.  generic_slice_step
 * (internal_samplers.py:1076-1206) evaluates F(x) = loglikelihood(prior_transform(u + x d)) at
 * every stepping-out / shrinking move; with an arbitrary Python likelihood the host runs that
 * state machine and this call supplies what each walker's random stream produces:
 *   kind 0  rslice: drhat = standard_normal(ndim) / |.|, dirs = axes . drhat * scale (:818-823)
 *   kind 1  slice : perm = the shuffled axis order of one sweep (:667-669)
 *   kind 2  nothing (advance / refill / commit only)
 * followed by a LOOKAHEAD of the next `nlook` Generator.random() values (rand0, doubling
 * draws, shrink draws) that is NOT committed to the stream.
 *   state6    k x 6 in/out: PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger; on
 *             entry the stream is first advanced by consumed[i] draws (the part of the previous
 *             lookahead the host used; NULL = 0), on return it stands after the direction /
 *             shuffle draws and before the lookahead.
 *   axes      m x ndim x ndim (kind 0), axes_idx k or NULL
 *   dirs      k x ndim (kind 0); perm k x ndim (kind 1); look k x nlook */
int dh_slice_feed(dh_ctx* ctx, int k, int ndim, int kind, const double* axes, int m,
                  const int32_t* axes_idx, double scale, uint64_t* state6,
                  const int32_t* consumed, int nlook, double* dirs, int32_t* perm,
                  double* look);

/* RSliceSampler.sample (mode 0, internal_samplers.py:745-855) / SliceSampler.sample
 * (mode 1, :593-709) over k walkers; generic_slice_step + Neal's doubling
 * (:1038-1206) run as a per-lane state machine.  ncdim == ndim (dynesty.py:507-509).
 *   doubling   kwargs['slice_doubling'] on entry
 *   outputs    u,v k*ndim; logl, ncalls, nexpand, ncontract k;
 *              flags k: bit0 expansion_warning_set, bit1 x == 0 failure
 * The host-pointer form returns DH_ERR_SLICE if any walker failed. */
int dh_slice_batch(dh_ctx* ctx, int problem, int k, int ndim, int mode,
                   const double* u0, const double* axes, int m,
                   const int32_t* axes_idx, double scale, double loglstar,
                   int slices, int doubling, const uint64_t* rng, double* u,
                   double* v, double* logl, int32_t* ncalls, int32_t* nexpand,
                   int32_t* ncontract, int32_t* flags, uint64_t* rng_out);
int dh_slice_batch_dev(dh_ctx* ctx, int problem, int k, int ndim, int mode,
                       const double* u0, const double* axes, int m,
                       const int32_t* axes_idx, double scale, double loglstar,
                       int slices, int doubling, const uint64_t* rng, double* u,
                       double* v, double* logl, int32_t* ncalls, int32_t* nexpand,
                       int32_t* ncontract, int32_t* flags, uint64_t* rng_out);

/* Throughput mode of the slice samplers (see dh_rwalk_batch_philox): the same kernels drawing from
 * hiprand's Philox4x32-10 generator -- directions (internal_samplers.py:820) from fp32 Box-Muller normals
 * widened to fp64, the axis shuffle (:673) by masked rejection on 32-bit draws, rand0 / doubling coin /
 * shrink uniforms (:1099, 1151, 1173) from 53-bit doubles in [0, 1) -- walker i on subsequence
 * sequence0 + i of `seed`, `offset` draws in.  Consumption depends on the data: advance `offset` by more
 * than a walker can draw in one call (2^24 is what dh_ns_ensemble uses).  Any ndim <= 512 (above 32, and
 * at dimensions without a register instantiation, the wave-per-walker kernels of the wide path). */
int dh_slice_batch_philox(dh_ctx* ctx, int problem, int k, int ndim, int mode, const double* u0,
                          const double* axes, int m, const int32_t* axes_idx, double scale,
                          double loglstar, int slices, int doubling, uint64_t seed, uint64_t sequence0,
                          uint64_t offset, double* u, double* v, double* logl, int32_t* ncalls,
                          int32_t* nexpand, int32_t* ncontract, int32_t* flags);
int dh_slice_batch_philox_dev(dh_ctx* ctx, int problem, int k, int ndim, int mode, const double* u0,
                              const double* axes, int m, const int32_t* axes_idx, double scale,
                              double loglstar, int slices, int doubling, uint64_t seed, uint64_t sequence0,
                              uint64_t offset, double* u, double* v, double* logl, int32_t* ncalls,
                              int32_t* nexpand, int32_t* ncontract, int32_t* flags);

/* UniformBoundSampler.sample (internal_samplers.py:243-340) with the bound's
 * sample() inlined: m == 1 Ellipsoid.sample (bounding.py:307-319), m > 1
 * MultiEllipsoid.sample incl. the 1/q overlap rejection (bounding.py:525-590),
 * m == 0 UnitCubeSampler.sample (internal_samplers.py:364-441).
 *   ctrs m*ncdim, axes/ams m*ncdim*ncdim, cumprob m = cumsum(exp(logvol_ells -
 *   logvol)) (rand_choice, bounding.py:1300-1308); bc: DH_BC_* per dim or NULL
 *   max_tries: per-walker guard (<= 0: 2^32 tries, then DH_ERR with "exceeded max_tries"); ncalls = likelihood calls. */
int dh_unif_batch(dh_ctx* ctx, int problem, int k, int ndim, int ncdim, int m,
                  const double* ctrs, const double* axes, const double* ams,
                  const double* cumprob, double loglstar, const int8_t* bc,
                  const uint64_t* rng, int64_t max_tries, double* u, double* v,
                  double* logl, int32_t* ncalls, uint64_t* rng_out);
int dh_unif_batch_dev(dh_ctx* ctx, int problem, int k, int ndim, int ncdim, int m,
                      const double* ctrs, const double* axes, const double* ams,
                      const double* cumprob, double loglstar, const int8_t* bc,
                      const uint64_t* rng, int64_t max_tries, double* u, double* v,
                      double* logl, int32_t* ncalls, int32_t* flags,
                      uint64_t* rng_out);

/* Throughput mode of UniformBoundSampler.sample / UnitCubeSampler.sample (m = 0: north_star's "hiprand for the
 * unit-cube draws"): ellipsoid choice, randsphere (bounding.py:1288-1297, 543-590), the 1/q test and the
 * unit-cube uniforms (internal_samplers.py:428) from hiprand's Philox4x32-10 generator, keyed as in
 * dh_rwalk_batch_philox.  Consumption depends on the data: advance `offset` generously between calls. */
int dh_unif_batch_philox(dh_ctx* ctx, int problem, int k, int ndim, int ncdim, int m, const double* ctrs,
                         const double* axes, const double* ams, const double* cumprob, double loglstar,
                         const int8_t* bc, uint64_t seed, uint64_t sequence0, uint64_t offset,
                         int64_t max_tries, double* u, double* v, double* logl, int32_t* ncalls);
int dh_unif_batch_philox_dev(dh_ctx* ctx, int problem, int k, int ndim, int ncdim, int m, const double* ctrs,
                             const double* axes, const double* ams, const double* cumprob, double loglstar,
                             const int8_t* bc, uint64_t seed, uint64_t sequence0, uint64_t offset,
                             int64_t max_tries, double* u, double* v, double* logl, int32_t* ncalls,
                             int32_t* flags);

/* Bound.sample / samples from ONE generator: Ellipsoid.sample(s)
 * (bounding.py:307-334) for m == 1, MultiEllipsoid.sample(s)
 * (bounding.py:525-606) for m > 1 (return_q != 0: no internal 1/q rejection).
 * xs nsamp*d, idxs/qs nsamp, state4_out = the generator after the draws. */
int dh_bound_draw(dh_ctx* ctx, const uint64_t* state4, int nsamp, int d, int m,
                  const double* ctrs, const double* axes, const double* ams,
                  const double* cumprob, int return_q, double* xs, int32_t* idxs,
                  int32_t* qs, uint64_t* state4_out);

/* One queue consumption of the static run loop for `runs` independent runs -- the iteration loop of
 * Sampler.sample over ONE queue fill (sampler.py:1070-1185) with _new_point's queue rule
 * (sampler.py:741-776): while the dlogz criterion has not fired, the worst live point dies and is replaced
 * by the next queue entry whose logl beats it (entries that do not are discarded, their calls still
 * charged); every death takes the volume step ln((N+1)/N) (inside a likelihood plateau: the plateau's step) and one step of progress_integration
 * (utils.py:1470-1492).  This is the `ns_consume` stage of dh_ns_ensemble as an operator of its own
 * (used to hold it to the oracle's restatement of the reference loop; a host-driven loop can use it too).
 *   live_logl  runs x nlive   in/out, slot order
 *   q_logl     runs x K       the queue's log-likelihoods in queue order; q_ncalls their call counts
 *   state      runs x 8       in/out: logvol, logz, h, logzvar, loglstar of the last dead point
 *                             (-1e300 before the first), it, ncall, [out only] the current worst logl
 *   dead_logl / dead_slot / dead_src   runs x K: this call's deaths in order (logl, slot, queue index of
 *                             the replacement); ndead[r] of them are valid; stopped[r] = dlogz fired
 *   live_it / dead_it / dead_nc  optional (NULL together): the per-point bookkeeping of saved_run
 *                             (sampler.py:1107, 1141, 1165-1182).  live_it runs x nlive in/out = iteration at
 *                             which the point living in each slot was proposed (0 = initial point; the
 *                             reference counts iterations from 1); dead_it runs x K = that value for every
 *                             dead point ('it'); dead_nc runs x K = likelihood calls spent on its replacement
 *                             ('nc': every queue entry popped since the previous death); dead_slot is 'id'.
 *   plateau    optional, runs x 2 in/out: the likelihood-plateau mode of the reference (sampler.py:1112-1127,
 *                             1190-1193) carried between calls -- deaths still to be taken with the plateau's
 *                             constant volume step (0 = off) and the logarithm of that step's volume; NULL:
 *                             the call starts outside plateau mode and the state is not handed back
 * Equal log-likelihoods die lowest slot first, as in the reference (np.argmin, sampler.py:1107), and when the
 * worst point shares its value with others the deaths take the reference's plateau volume steps. */
int dh_ns_consume(dh_ctx* ctx, int runs, int nlive, int queue_size, double dlogz, double* live_logl,
                  const double* q_logl, const int32_t* q_ncalls, double* state, double* dead_logl,
                  int32_t* dead_slot, int32_t* dead_src, int32_t* ndead, int32_t* stopped, int32_t* live_it,
                  int32_t* dead_it, int32_t* dead_nc, double* plateau);

/* ---- device-resident ensemble of static nested-sampling runs (BASELINE config
 * C5): the loop of Sampler.sample (sampler.py:932-1212) with a
 * proposal queue of `queue_size` rwalk / rslice / slice walkers per run
 * (sampler.py:676-778; tune / tune_slice once per fill),
 * unit-cube start, MultiEllipsoid (bound_multi=1) or Ellipsoid bound rebuilt
 * every walks*nlive calls and enlarged by `enlarge`, RWalkSampler.tune, evidence
 * integration (utils.py:1470-1492) and the final live points -- all on the
 * device for `runs` independent runs at once.  Dimensions: any ndim <= 512 (above 32 the walkers are the
 * wave-per-walker kernels, above 44 the bound is the multi-workgroup Ellipsoid.update: BASELINE config C4 -- or,
 * bound_multi=1, the wide MultiEllipsoid.update, whose recursion the host drives: such a run synchronises the
 * stream on its rebuild fills); sample='unif' ndim <= 32.  Sizes: nlive <= 65535 (slots travel as 16-bit indices),
 * queue_size <= 2048.  The queue consumption keeps a run's keys, their sorted order and the queue in LDS while
 * 12 nlive + 2 P + 52 queue_size bytes <= 150 KB (P = nlive rounded up to a power of two) and nlive <= 8192; beyond
 * that it selects the queue_size + 1 smallest live points from the keys in global memory first -- the only ones a fill
 * can touch -- and works on those (same deaths, same evidence).  DH_ERR_ARG otherwise.  Run r seeds from
 * SeedSequence(entropy) children keyed on first_run + r (independent of how the
 * ensemble is sharded).  records: runs x 8 doubles {logz, logzerr, niter, ncall,
 * h, nbound, status (0 ok, 1 max_fills hit, -1 failed), eff%}.
 * dead_logl_out (optional): runs x max_iter dead-point log-likelihoods;
 * live_logl_out (optional): runs x nlive log-likelihoods of the final live points
 * (together they are what utils.merge_runs needs to combine the ensemble);
 * dead_u_out (optional): runs x max_iter x ndim unit-cube coordinates of the dead
 * points in death order (only the first niter rows of a run are written);
 * live_u_out (optional): runs x nlive x ndim final live points (slot order, matching
 * live_logl_out) -- the posterior samples of the runs.
 * dead_id_out / dead_it_out / dead_nc_out (optional, NULL together with live_it_out): runs x max_iter
 * int32 = the reference's per-point 'id' (live slot), 'it' (iteration at which the point was proposed,
 * counted from 1; 0 = initial point) and 'nc' (likelihood calls spent on the point's replacement) of every
 * dead point (sampler.py:1165-1182) -- what utils.merge_runs carries through as samples_id / samples_it /
 * ncall; live_it_out: runs x nlive = 'it' of the final live points (slot order; their id is the slot,
 * their nc is 1 by the reference's convention, sampler.py:880-886).
 * rebuild_sync = 0 keeps the reference's schedule per run (rebuild when ncall has
 * advanced by update_interval, sampler.py:625-674); rebuild_sync = 1 lets every run
 * that already has a bound rebuild whenever ANY run of the ensemble is due (its
 * rebuild comes early, never late): a rebuild is a latency-bound tree construction
 * that costs about the same for one run or the whole ensemble.
 * sampler 6 (PCG64) / 7 (Philox): the uniform sampler inside the run's bound (UniformBoundSampler.sample,
 * internal_samplers.py:243-340; rand_choice over the ellipsoids, randsphere, 1/q acceptance), ndim <= 32; the
 * bound is rebuilt every nlive calls (its update_bound_interval_ratio is the base class's 1,
 * internal_samplers.py:88-94), `walks` is ignored, a walker whose draw no ellipsoid holds fails its run as the
 * reference's RuntimeError does.  bootstrap = B > 1: every rebuild is followed by the bootstrap expansion of
 * bounding.py:381-400 / 688-703 -- B resampled replicas per run (bounding.py:1593-1648), all rebuilt in one ragged
 * batch, the bound scaled by max(1, largest normalised distance of a left-out point)^ndim; the reference's default
 * for sample='unif' is (enlarge 1, bootstrap 5), dynesty.py:169-200.  (Above ndim = 44 the replicas are built one
 * by one by the wide constructions, with the host between them.)  0: none.
 * rebuild_every = n: bounds are built only every n-th queue fill; a run that becomes due in between idles (proposes
 * and consumes nothing) until then.  Runs are independent, so a run's own sequence -- and with PCG64 streams its
 * result, bit for bit -- is that of the reference schedule (n = 1).  Once n reaches the number of fills a run needs
 * to spend its update interval every run is due by the next rebuild fill: the ensemble rebuilds together, one
 * latency chain per interval instead of one per fill (64 C2 runs: 0.335 s at n = 1, 0.20 s at n >= 4).  0: chosen
 * from (sampler, nlive, queue_size) alone: ceil(nlive / K) for rwalk, ceil(1.3 nlive / (4.4 K)) for the slice
 * samplers, ceil(1.3 nlive / (1.7 K)) for unif; at most 16.
 * bound (the bound code): 0 single ellipsoid, 1 multi-ellipsoid (MultiEllipsoid), 2 RadFriends ('balls'), 3 SupFriends
 * ('cubes').  Codes 2 / 3 need sampler 6 (unif, PCG64 streams) and ndim <= 32; any other value or combination is
 * DH_ERR_ARG.  With a friends bound every rebuild is RadFriends.update / SupFriends.update of the runs that are due
 * (bounding.py:876-957, 1141-1222: clusters cut in the run's previous metric -- the identity before its first update --,
 * the covariance, its square root, the radius from leave-one-out or from the B bootstrap replicas of the resident
 * protocol), batched over the runs on the device (dh_friends_update_batch's kernels), then scale_to_logvol(logvol +
 * ln enlarge) where enlarge != 1; a failed update (non-finite or singular covariance, zero radius) fails its run.  The
 * shapes sit on the run's live points of the fill (prepare_sampler: bound.ctrs = live_u).  nbound counts the updates.
 * An rwalk walker that accepted no step returns its start point with that live point's own stored ln L (an exact tie, as
 * the reference's re-evaluation gives: internal_samplers.py:970-975, sampler.py:1107-1119).
 * max_fills (0: 10^6) bounds the fills the ENSEMBLE is taken through, idle ones included: a fill in which a run
 * waits for its rebuild counts for that run as well, so with rebuild_every > 1 a run reaches status 1 after fewer of
 * its own fills than max_fills (n_fills_out is the same count). */
int dh_ns_ensemble(dh_ctx* ctx, int problem, int runs, int nlive, int ndim,
                   int queue_size, int sampler /* 0 rwalk, 1 rslice, 2 slice; + 3: unit-cube phase and proposals from hiprand Philox streams; 6 / 7 unif */,
                   int walks /* or slices */, int bound /* 0 single, 1 multi, 2 balls, 3 cubes */,
                   int rebuild_sync /* 1: all runs rebuild together, see below */, double dlogz,
                   double enlarge, int64_t max_fills, int64_t max_iter,
                   const uint32_t* entropy_words, int n_words, uint32_t first_run,
                   double* records, double* dead_logl_out, double* live_logl_out,
                   double* dead_u_out, double* live_u_out, int64_t* n_fills_out, int32_t* dead_id_out,
                   int32_t* dead_it_out, int32_t* dead_nc_out, int32_t* live_it_out, int bootstrap,
                   int rebuild_every /* bounds are built every n-th fill, runs due in between wait; 0: chosen from the shape */);

/* Options of the resident run loop that the reference takes in NestedSampler(...) / run_nested(...) and that
 * dh_ns_ensemble otherwise fixes at the reference's defaults.  Set before a dh_ns_ensemble call, they
 * apply to that call alone (see below); value NaN restores the default.
 *   DH_NS_OPT_UPDATE_INTERVAL   calls between bound updates (dynesty.py:213-234 `update_interval` as a number of calls;
 *                               a caller holding the ratio form multiplies by nlive); default: the sampler's ratio
 *                               (1 unif, walks rwalk, slices rslice, slices * ndim slice) * nlive
 *   DH_NS_OPT_FIRST_MIN_NCALL   first_update['min_ncall'] (sampler.py:625-674), default 2 nlive
 *   DH_NS_OPT_FIRST_MIN_EFF     first_update['min_eff'] in per cent, default 10
 *   DH_NS_OPT_MAXITER           run_nested(maxiter): the loop stops once its counter exceeds it, i.e. after maxiter + 1
 *                               deaths (sampler.py:1076-1083); default none
 *   DH_NS_OPT_MAXCALL           run_nested(maxcall): stops once the likelihood calls (initial points included)
 *                               exceed it; default none
 *   DH_NS_OPT_LOGL_MAX          run_nested(logl_max): stops once the last dead point's ln L exceeds it; default +inf
 *   DH_NS_OPT_ADD_LIVE          run_nested(add_live): 0 = the record is the dead points' running evidence, the
 *                               final live points stay out (sampler.py:1319-1341); default 1
 *   DH_NS_OPT_FORCED_EXACT      1 (the default since round 5) = the reference's protocol: Sampler.propose_live's forced
 *                               bound update (sampler.py:484-489) belongs to the fill that finds a start point outside
 *                               the bound -- the queue entries up to and including the first one outside keep their
 *                               axes from the old bound, the later ones take theirs from the new one -- and the regular
 *                               bound is built as the reference builds it, without the point that the previous fill's
 *                               last queue entry brought in (update_bound_if_needed runs before that replacement:
 *                               sampler.py:771-772, 1176-1185).  Scheduling: the forced update is built together with
 *                               the regular updates of the next fill that builds bounds (one masked rebuild sequence
 *                               for both); until then the flagged run keeps its queue and sits the fills out, which
 *                               leaves its own sequence of events unchanged (runs are independent).
 *                               0 = the late form: the run is flagged, walks this fill from the old bound and rebuilds
 *                               before its next fill; the regular bound includes the newest point (9-20 % fewer bound
 *                               updates than the reference; a few per cent faster).  The uniform sampler has no start
 *                               points: the option does not apply.
 * A run ended by maxiter / maxcall / logl_max ends normally (status 0), as the reference's does.
 * Options (and dh_ns_set_boundary's flags) apply to the NEXT dh_ns_ensemble call only: that call takes them and the
 * context forgets them, however the call ends. */
enum {
  DH_NS_OPT_UPDATE_INTERVAL = 0,
  DH_NS_OPT_FIRST_MIN_NCALL = 1,
  DH_NS_OPT_FIRST_MIN_EFF = 2,
  DH_NS_OPT_MAXITER = 3,
  DH_NS_OPT_MAXCALL = 4,
  DH_NS_OPT_LOGL_MAX = 5,
  DH_NS_OPT_ADD_LIVE = 6,
  DH_NS_OPT_FORCED_EXACT = 7,
  DH_NS_OPT_COUNT = 8
};
int dh_ns_set_option(dh_ctx* ctx, int key, double value);

/* NestedSampler(periodic=, reflective=) for the resident loop (dynesty.py:126-142: the lists only reach the internal
 * sampler): bc = ndim DH_BC_* flags, or NULL / ndim <= 0 for none.  Taken by the next dh_ns_ensemble call (one-shot, like the options; a rejected call leaves installed flags as they were);
 * dh_ns_ensemble refuses a flag array whose length is not its ndim.  rwalk wraps / reflects the flagged coordinates and
 * tests them against (-0.5, 1.5) (internal_samplers.py:1023-1032), the uniform sampler only widens its unitcheck
 * (:301-314); the slice samplers ignore the flags, as the reference's do (its `nonperiodic` kwarg is never set). */
int dh_ns_set_boundary(dh_ctx* ctx, int ndim, const int8_t* bc);

/* The bootstrap expansion factor on its own (host pointers; what the resident loop runs after a rebuild):
 * for each of `runs` point sets (runs x n x d) the max over `bootstrap` replicas of max(1, largest normalised
 * distance of a left-out point to the replica's Ellipsoid (multi = 0) / nearest of its MultiEllipsoid's ellipsoids
 * (multi = 1)) -- _ellipsoid_bootstrap_expand, bounding.py:1619-1648.  Replica b of run r resamples with the
 * PCG64 stream seeded (ent[4r], ent[4r+1] + b) with increment words (ent[4r+2], ent[4r+3] + 2b)
 * (oracle/nested_ref.py boot_generator).  expand: runs doubles; n_in (optional): runs x bootstrap sample sizes
 * (distinct points drawn, after _bootstrap_points' repairs). */
int dh_bootstrap_expand(dh_ctx* ctx, int runs, const double* pts, int n, int d, int multi, int bootstrap,
                        const uint64_t* ent, double* expand, int32_t* n_in);

/* ---- RadFriends / SupFriends (bounding.py:734-1263, 1651-1702) ----------------
 * kind: 0 = 'balls' (RadFriends, Euclidean norm), 1 = 'cubes' (SupFriends, max norm).
 * All matrices are d x d row-major host arrays; axes = sqrtm(cov) and axes_inv = pinvh(axes)
 * are symmetric, am = pinvh(cov).
 *
 * dh_friends_update = RadFriends.update / SupFriends.update (bounding.py:876-957, 1141-1222):
 * covariance of the points after re-centring every single-linkage cluster (cut at Mahalanobis
 * distance 1 in the PREVIOUS metric am_prev, evaluated with the arithmetic of scipy's pdist so
 * that the knife-edge pair -- the radius puts the loneliest point exactly at distance 1 -- falls
 * the reference's way; NULL = use_clustering=False), its symmetric square root and pseudo-inverses, the points in
 * the whitened frame, and the radius / half-side = max nearest-neighbour distance: leave-one-out
 * (nboot = 0) or, per bootstrap replica b, from the left-out points to the resampled ones
 * (in_mask[b*n + i] != 0 iff point i was resampled; the index bookkeeping of
 * _bootstrap_points, bounding.py:1593-1616, stays on the host).  Outputs are already scaled by
 * the radius (cov r^2, am / r^2, axes r, axes_inv / r); logvol = ln volume of ONE shape.
 * 2 <= n, 1 <= d <= 64; with clustering (am_prev != NULL) d <= 63: the adjacency tile of the pairwise distances,
 * (d^2 + 260 d) * 8 bytes, must fit the 160 KB of LDS of a workgroup -- d = 64 with a metric is DH_ERR_ARG, with
 * am_prev = NULL it works.  The same limits hold for dh_friends_update_batch.
 * DH_ERR_VALUE: non-finite or singular covariance, or zero radius (the reference divides by 0); the contents of
 * the output arrays are then unspecified (the unscaled intermediates may have been written).  The batched call
 * below leaves a failed run's outputs untouched. */
int dh_friends_update(dh_ctx* ctx, const double* pts, int n, int d, int kind,
                      const double* am_prev, int nboot, const uint8_t* in_mask,
                      double* cov, double* am, double* axes, double* axes_inv,
                      double* logvol, double* rmax, int32_t* nclusters);

/* RadFriends.within / overlap / contains for m candidate points (bounding.py:777-793,
 * 1043-1064): counts[c] = number of balls / cubes containing x_c; bits (optional,
 * m x ceil(n/64) words) = which ones (bit j of word j/64). */
/* dh_friends_update over `runs` point sets at once (the resident loop's rebuild): pts runs x n x d; am_prev
 * (runs x d x d, NULL: no clustering); in_mask runs x nboot x n; active (runs int32, NULL: all) -- an inactive run's
 * outputs are left as they are.  Outputs per run: cov / am / axes / axes_inv (runs x d x d), logvol, rmax,
 * nclusters (optional) and status (DH_OK, or DH_ERR_VALUE where dh_friends_update fails; a failed run's other
 * outputs are left as they are).  Every stage is one launch over all runs with no host synchronisation between them;
 * per run the results are bit-identical to dh_friends_update's, logvol agrees to 1e-14 (the device's log / lgamma).
 * The call itself returns DH_OK unless its arguments or the device fail. */
int dh_friends_update_batch(dh_ctx* ctx, int runs, const double* pts, int n, int d, int kind,
                            const double* am_prev, int nboot, const uint8_t* in_mask, const int32_t* active,
                            double* cov, double* am, double* axes, double* axes_inv, double* logvol,
                            double* rmax, int32_t* nclusters, int32_t* status);

int dh_friends_within(dh_ctx* ctx, const double* ctrs, int n, int d, int kind,
                      const double* axes_inv, const double* x, int m, int32_t* counts,
                      uint64_t* bits);

/* RadFriends.sample(s) / SupFriends.sample(s) from ONE generator (bounding.py:795-847,
 * 1066-1117), same draw order as the reference (balls: d normals + 1 uniform; cubes: d uniforms;
 * then integers(n) on the buffered 32-bit stream when n > 1; then 1 uniform iff q > 1 and not
 * return_q).  state6 = {state hi, state lo, inc hi, inc lo, has_uint32, uinteger}. */
int dh_friends_draw(dh_ctx* ctx, const uint64_t* state6, int nsamp, const double* ctrs, int n,
                    int d, int kind, const double* axes, const double* axes_inv, int return_q,
                    double* xs, int32_t* qs, uint64_t* state6_out);

/* UniformBoundSampler.sample over a queue of k walkers with a RadFriends / SupFriends bound
 * (internal_samplers.py:243-340 with bounding.py:795-831 / 1066-1101 as bound.samples(1)):
 * per try one draw from the union of shapes (1/q rule, brute-force overlap over the n centres),
 * unitcheck, prior transform and likelihood of the device problem, until logl > loglstar.
 * Same arguments and outputs as dh_unif_batch; ncdim == ndim (the reference's friends bounds
 * need it too: their centres are the full live points).
 * problem = -1 (also accepted by dh_unif_batch) selects the lock-step form for an arbitrary
 * host likelihood: every walker returns the next candidate of its stream that lies in the bound
 * and passes unitcheck (u, rng_out; v / logl / ncalls may be NULL) and the caller evaluates it.
 * rng32 / rng32_out (optional, k x 2 {has_uint32, uinteger}) carry NumPy's buffered 32-bit half,
 * which integers(n) consumes, from one lock-step round to the next. */
int dh_unif_friends_batch(dh_ctx* ctx, int problem, int k, int ndim, int kind, const double* ctrs,
                          int n, const double* axes, const double* axes_inv, double loglstar,
                          const int8_t* bc, const uint64_t* rng, int64_t max_tries, double* u,
                          double* v, double* logl, int32_t* ncalls, uint64_t* rng_out,
                          const uint64_t* rng32, uint64_t* rng32_out);

/* ---- the combiner on the device (csrc/merge*.hip) ---------------------------------------
 * dh_ns_keep(ctx, 1): the NEXT dh_ns_ensemble call (one-shot, like the options) stores the samples and the per-point
 * id / it / nc on the device whether or not their host pointers are given, downloads only what the host pointers ask
 * for, and leaves its allocation with the context as "the kept ensemble" (one per context).  A later keep,
 * dh_ns_release or dh_destroy frees it.  Without the switch dh_ns_ensemble is unchanged. */
int dh_ns_keep(dh_ctx* ctx, int on);
int dh_ns_release(dh_ctx* ctx);

/* ---- a kept ensemble taken further, saved and restored (csrc/ns.hip, csrc/ns_state.h) ----
 * dh_ns_continue re-enters the loop of the ensemble that dh_ns_keep + dh_ns_ensemble (or dh_ns_state_import) left on
 * the device, as calling run_nested again does in the reference (sampler.py:1038-1066).  The allocation, the plan, the
 * streams and the ENSEMBLE's fill counter are the first call's.  Records and outputs are those of dh_ns_ensemble, over
 * the whole run; the host buffers are runs x max_iter of the FIRST call: the dead-point capacity is chosen once, for the
 * whole run (dh_ns_state_import can give a saved ensemble more).  The ensemble stays kept, and dh_merge_kept merges the
 * continued runs.  max_fills (0: 10^6) bounds the fills of THIS call; n_fills_out counts them.
 * Stop rules.  dlogz (the argument) and the one-shot options DH_NS_OPT_MAXITER / MAXCALL / LOGL_MAX / ADD_LIVE are taken
 *   anew by each call (not set: none / add_live 1).  maxiter and maxcall are TOTALS of the run -- iterations and calls
 *   since the run began, exactly as in the first call.  The reference's repeated run_nested counts them per call: a
 *   deliberate difference; a caller who wants a per-call budget adds the records' niter / ncall.  Everything else is
 *   fixed by the first call: sampler, bound, walks, enlarge, bootstrap, rebuild_every, the update interval, first_update,
 *   forced_exact, the boundary flags and the resolved values of the environment switches.  Setting
 *   DH_NS_OPT_UPDATE_INTERVAL / FIRST_MIN_NCALL / FIRST_MIN_EFF / FORCED_EXACT or dh_ns_set_boundary before
 *   dh_ns_continue is DH_ERR_ARG, as is a context without a kept ensemble.  As for every call, the context forgets the
 *   options however the call ends; an argument error leaves the kept ensemble as it was.
 * Which runs go on.  Before the first fill the reference's top-of-loop tests (sampler.py:1071-1100: delta ln Z from
 *   lmax, ln X, ln Z below dlogz; the last dead point above logl_max; it > maxiter; ncall > maxcall; the plateau stop)
 *   are evaluated on every run's state.  A run for which one holds is done (status 0) with no new death; the others go
 *   on in the mode they had (unit-cube phase or bound); a failed run (status -1) stays failed, its record as it was; a
 *   run that max_fills stopped (status 1) simply goes on.  Continuing with unchanged criteria is therefore a no-op that
 *   returns the same records and zero fills.
 * The unspent queue.  A stop rule that ends a run inside a fill leaves queue entries behind the stopping one; the
 *   reference keeps them and pops them first when the run goes on.  So does the continuation: the fill's proposals stay
 *   on the device, the state the fill found is put back, and the fill is consumed again -- whole, under the new criteria,
 *   ahead of the call's first regular fill, without a second tuning step and without counting as a fill.  rest_out
 *   (optional, runs) reports how many entries behind its stop each run took over this way (0: none, or not stopped
 *   inside a fill).
 * What is exact.  PCG64 streams: a run's result depends on its own seed and its own sequence of events only, so any
 *   chain of calls that ends under criteria C gives, run for run and bit for bit, what ONE dh_ns_ensemble call under C
 *   gives (records, dead ln L / u / id / it / nc, final live ln L / u / it) -- whether the earlier calls were ended by
 *   max_fills, maxiter, maxcall, logl_max or a looser dlogz (criteria that stop a run later than C would are the
 *   caller's to avoid: a dead point does not come back), with or without an export / import in between, with
 *   rebuild_sync = 0.  Philox streams: offsets are keyed on the ENSEMBLE's fill index.  Calls cut by max_fills are
 *   bit-exact (all runs stop at the same fill boundary); after a criterion stop a run resumes at a later ensemble fill
 *   than it would have reached uninterrupted, and its result is then a different, equally valid draw: deterministic, not
 *   equal. */
int dh_ns_continue(dh_ctx* ctx, double dlogz, int64_t max_fills, double* records, double* dead_logl_out,
                   double* live_logl_out, double* dead_u_out, double* live_u_out, int64_t* n_fills_out,
                   int32_t* dead_id_out, int32_t* dead_it_out, int32_t* dead_nc_out, int32_t* live_it_out,
                   int32_t* rest_out /* optional, runs: unspent queue entries each run took over */);

/* ---- a dynamic batch: strands started inside a finished run (csrc/ns.hip, csrc/ns_batch_plan.h) ----
 * dh_ns_batch runs `runs` strands of nlive_new live points each inside the ln L range (logl_min, logl_max] of a
 * finished run: the reference's _configure_batch_sampler + sample_batch (dynamicsampler.py:300-622, 1228-1465).  The
 * arguments, the one-shot options (logl_max comes through DH_NS_OPT_LOGL_MAX), the boundary flags, the records and the
 * outputs are those of dh_ns_ensemble with nlive = nlive_new (rebuild_sync is 0), plus:
 *   seed_u (runs x nlive_new x ndim), seed_logl (runs x nlive_new): every strand's seeds, points of the finished run
 *     with ln L > logl_min, as stored: they are not evaluated again (the reference copies them);
 *   logl_min: finite; start (runs x 6): logvol, logz, h, logzvar and ln L of the finished run's row at logl_min -- where
 *     the strand's volume and running evidence go on from -- and the sampler's scale the strand starts with;
 *   start_u_out / start_logl_out / start_nc_out (optional, runs x nlive_new (x ndim)): the live set the sampling phase
 *     begins with, in the order the points were accepted, and the calls spent on each; seed_ncall_out (runs, required):
 *     the likelihood calls of the seeding phase; seed_rng_out (optional, runs x 4): the strand's generator at the
 *     hand-over.
 * Phase S (seeding).  The seeds are the strand's live set; its bound is built on them once (nbound = 1, masked rebuild,
 *   bootstrap expansion, enlarge); ceil(nlive_new / queue_size) fills of the ordinary selection / walk stages at the
 *   fixed threshold logl_min, start points drawn among the seeds, fill a staging set in queue order (nc of a point: its
 *   entry's calls and the rejected entries' before it); every call is charged; the scale is tuned once per fill.  The
 *   staging set then replaces the seeds (it = 0 for every point) and the loop of dh_ns_ensemble goes on from there, its
 *   counters at 0: niter counts the strand's own deaths, ncall = seed calls + the calls of the sampling phase.  The
 *   record's logz / logzerr / h are the RUNNING values continued from the start row: they steer the dlogz stop as in the
 *   reference's batch sampler and are not results -- the combined run's integrals are recomputed by whoever merges.
 * Streams.  Strand r has the streams dh_ns_ensemble gives run first_run + r (generator: child 0x80000000 + first_run +
 *   r of the entropy): an ensemble of strands equals its shards, bit for bit.
 * Departures from the reference: (a) the bound is not rebuilt during seeding (the seeds do not change); (b) the last seed
 *   fill's unused queue entries are dropped, their calls counted (the reference pops them for the first deaths); (c) a
 *   strand always starts in bound mode (the reference stays on the unit cube while logl_min is below the base run's
 *   first bound update); (d) the starting scale is the caller's (the reference takes the saved scale of the lowest
 *   point above logl_min).
 * DH_ERR_ARG, decided before the device is touched, the context left usable: the Philox samplers (3, 4, 5, 7), the
 *   friends bounds (2, 3), an armed dh_ns_keep, a non-finite logl_min (a batch from the prior is dh_ns_ensemble with
 *   logl_max), a seed with seed_logl <= logl_min, nlive_new below 4 or above 65535 (the loop's own limits), logl_max <=
 *   logl_min, a non-finite start row or a scale <= 0, and whatever dh_ns_ensemble refuses for the same shape.
 * The seed fills are exactly ceil(nlive_new / queue_size), enqueued without a look at the device, and run without the
 *   start points' membership test (the start points are the seeds the bound was built on).  An entry is lost only to a
 *   failed slice; a strand whose staging set is not full after the seed fills ends with status -1. */
int dh_ns_batch(dh_ctx* ctx, int problem, int runs, int nlive_new, int ndim, int queue_size,
                int sampler /* 0 rwalk, 1 rslice, 2 slice, 6 unif */, int walks /* or slices */,
                int bound /* 0 single, 1 multi */, double dlogz, double enlarge, int64_t max_fills, int64_t max_iter,
                const uint32_t* entropy_words, int n_words, uint32_t first_run, const double* seed_u,
                const double* seed_logl, double logl_min, const double* start, double* records,
                double* dead_logl_out, double* live_logl_out, double* dead_u_out, double* live_u_out,
                int64_t* n_fills_out, int32_t* dead_id_out, int32_t* dead_it_out, int32_t* dead_nc_out,
                int32_t* live_it_out, int bootstrap, int rebuild_every, double* start_u_out, double* start_logl_out,
                int32_t* start_nc_out, int64_t* seed_ncall_out, uint64_t* seed_rng_out);

/* The kept ensemble as one host buffer and back.  The image holds a header (magic, DH_VERSION, sizeof of the per-run
 * state, the shapes, the fill counter, whether the unit-cube phase is still on), every argument and resolved plan value
 * of the first call, and the state arrays; the five dead-point arrays (ln L, u, id, it, nc) by each run's first niter
 * rows only, so the size depends on what the runs produced, not on max_iter.  Workspaces that every fill rewrites are
 * left out.  An image is read by the library version that wrote it.
 * dh_ns_state_size: the bytes dh_ns_state_export will write now.  dh_ns_state_export: DH_ERR_ARG if `bytes` is less.
 * dh_ns_state_import rebuilds the plan from the image (not from the environment), allocates, copies, and installs the
 * result as the context's kept ensemble (an earlier one is freed), ready for dh_ns_continue / dh_merge_kept.
 * max_iter = 0: the saved capacity; larger values give the runs more room (rows are `capacity` apart: only strides
 * change).  DH_ERR_ARG, with the context left as it was: bad magic or version, another sizeof of the per-run state, a
 * truncated buffer, a row count above the capacity, max_iter below a run's niter, a problem whose ndim differs.  That
 * the problem is otherwise the one the ensemble was run on is the caller's responsibility, as is the integrity of the
 * image's body. */
int dh_ns_state_size(dh_ctx* ctx, uint64_t* bytes);
int dh_ns_state_export(dh_ctx* ctx, void* buf, uint64_t bytes);
int dh_ns_state_import(dh_ctx* ctx, int problem, const void* buf, uint64_t bytes,
                       int64_t max_iter /* 0: as saved; else >= every run's niter */);

/* Per-point fields of the merged run (dh_merged_fetch).  LOGL .. WEIGHT: one double per point; SAMPLES_U / SAMPLES:
 * ndim doubles per point; RUN .. NCALL and BATCH: one int32 per point (ID / IT / NCALL only where the merge was given
 * them). */
enum {
  DH_MERGED_LOGL = 0,
  DH_MERGED_LOGVOL = 1,
  DH_MERGED_LOGWT = 2,
  DH_MERGED_LOGZ = 3,
  DH_MERGED_LOGZERR = 4,
  DH_MERGED_INFORMATION = 5,
  DH_MERGED_WEIGHT = 6,    /* exp(logwt - ln Z) / sum */
  DH_MERGED_SAMPLES_U = 7,
  DH_MERGED_SAMPLES = 8,
  DH_MERGED_RUN = 9,       /* run the point came from */
  DH_MERGED_SEQ = 10,      /* its index in that run's own sequence (dead points, then final live points ascending) */
  DH_MERGED_SAMPLES_N = 11,
  DH_MERGED_FINAL = 12,    /* 1: a final live point */
  DH_MERGED_ID = 13,
  DH_MERGED_IT = 14,
  DH_MERGED_NCALL = 15
};
/* Not a field of the merged run (dh_merged_fetch refuses it): for dh_merged_bootstrap_run, the merged-run index of
 * every point of a resampled run, int64. */
#define DH_MERGED_SRC 16
/* Nor is this one: for dh_merged_realization and dh_merged_bootstrap_run, the cumulative Kullback-Leibler divergence of
 * one realization or bootstrap from the merged run (utils.kld_error, utils.py:1932-1997), a double per point. */
#define DH_MERGED_KLD 17
/* A field of the merged run again (dh_merged_fetch): the dynamic batch the point came in with, int32 -- 0 for the base
 * run, b for the b-th strand folded in by dh_merged_fold (samples_batch of dynamicsampler.py:1467-1609); 0 everywhere
 * on a run that holds no batch. */
#define DH_MERGED_BATCH 18

/* `runs` static runs of equal nlive merged into one run that stays on the device -- ensemble.merge_static_runs, i.e.
 * the reference's utils.merge_runs for such runs.  Host pointers: niter (runs), dead_logl / dead_id / dead_it / dead_nc
 * (runs x stride, the first niter[r] of a row are read), dead_u (runs x stride x ndim), live_logl / live_it
 * (runs x nlive, slot order), live_u (runs x nlive x ndim).  dead_id, dead_it, dead_nc and live_it may be NULL
 * together.  The merged order is the stable order of the concatenated sequences (exact, ties included); parameters
 * are dh_problem_eval's of the same rows, bit for bit.  summary_out: 6 doubles {M, ln Z, its error, H, ESS,
 * sum ncall}.  The merged run (one per context) is replaced by the next merge.
 * DH_ERR_ARG: shapes and sizes (M < 2^31 points, M x ndim < 2^32 elements); nothing was touched, an earlier merged
 * run is still there.  Every other error leaves the context without a merged run: DH_ERR_VALUE: a NaN
 * log-likelihood, or a run whose sequence decreases; DH_ERR_NOMEM. */
int dh_merge_runs(dh_ctx* ctx, int problem, int runs, int nlive, int ndim, int64_t stride, const int64_t* niter,
                  const double* dead_logl, const double* live_logl, const double* dead_u, const double* live_u,
                  const int32_t* dead_id, const int32_t* dead_it, const int32_t* dead_nc, const int32_t* live_it,
                  double* summary_out);
/* The same from the kept ensemble, with no upload.  niter: NULL = the kept records'.  DH_ERR_ARG: no kept ensemble,
 * or `problem` is not the one it ran. */
int dh_merge_kept(dh_ctx* ctx, int problem, const int64_t* niter, double* summary_out);
/* `count` points of one field from point `first` on, to the host. */
int dh_merged_fetch(dh_ctx* ctx, int field, int64_t first, int64_t count, void* out);
/* utils.mean_and_cov of (samples, weights): mean ndim, cov ndim x ndim (either may be NULL). */
int dh_merged_moments(dh_ctx* ctx, double* mean, double* cov);
/* Systematic resampling (utils.resample_equal before its shuffle): idx[i] = #{j : C_j <= (u0 + i) / n_out} over the
 * normalised cumulative weights.  idx_out (n_out int64) may be NULL: the indices stay on the device.  n_out < 2^32. */
int dh_merged_resample(dh_ctx* ctx, double u0, int64_t n_out, int64_t* idx_out);
/* Parameter rows of n points: out_v n x ndim (n x ndim < 2^32 per call).  idx NULL = the first n indices of the last
 * dh_merged_resample. */
int dh_merged_gather(dh_ctx* ctx, int64_t n, const int64_t* idx_or_null, double* out_v);
/* Rows of the n points idx of one row field, DH_MERGED_SAMPLES_U or DH_MERGED_SAMPLES: out n x ndim (n x ndim < 2^32 per
 * call).  The seeds of a dynamic batch -- the unit-cube rows of the points _configure_batch_sampler chose
 * (dynamicsampler.py:457-533) -- come to the host this way, without the column.  DH_ERR_ARG: no merged run, another
 * field, n < 1, idx or out NULL, an index outside [0, M). */
int dh_merged_gather_rows(dh_ctx* ctx, int field, int64_t n, const int64_t* idx, double* out);
int dh_merged_release(dh_ctx* ctx);

/* ---- dynamic batches folded into the merged run ------------------------------------------
 * The strands of one batch folded into the context's merged run -- the reference's combine_runs
 * (dynamicsampler.py:1467-1609) applied strand after strand, in strand order, with the same bounds; here in one pass.
 * The strand arguments have the shapes and meaning of dh_merge_runs' run arguments: per strand niter[r] dead points in
 * death order and nlive_new final live points in slot order (host pointers; id / it / nc / live it together, and only
 * where the merged run has them).  The result replaces the merged run and stays on the device:
 *   order    the stable order of (base, strand 0, .., strand R-1): on equal ln L the base point first, then the strands
 *            by index, then a strand's own order (:1517-1552)
 *   n        the base's live count at its next point (0 past its end) plus, where ln L > logl_min (strictly), the
 *            strands': strands x nlive_new less their final live points before the position (:1528-1545)
 *   id       strand s shifted by (the largest id so far) + 1; a base that is a merge of several static runs is first
 *            renumbered id <- run x nlive + id, run <- 0; new points get run 0, seq their index in the strand's own
 *            sequence, final 1 for a final live point, batch = (batches before) + 1 + s
 *   ln X     combine_runs' plateau rule (:1554-1583): an ordinary point steps by log1p(1 / n); p >= 2 equal ln L
 *            entered at volume X with live count n take ln X + log1p(-(j + 1) / (n + 1)), j = 0 .. p - 1
 *   ln w, ln Z, H, var ln Z, the weights, the moments, the summary: recomputed over the whole run as by dh_merge_runs,
 *            every point with its own step ln X_{k-1} - ln X_k
 *   rows     the base's u and v rows move bit for bit; a new point's v is dh_problem_eval of its u, bit for bit
 * summary_out: 6 doubles as dh_merge_runs'.  The fold is built beside the base run and swapped in on success, so EVERY
 * error leaves the merged run as it was:
 * DH_ERR_ARG: no merged run, a problem of another ndim, strands < 1, nlive_new < 1, logl_min not finite (a batch from
 * the prior passes -DBL_MAX), logl_max <= logl_min, id / it / nc on one side only, M + W >= 2^31 points or
 * (M + W) x ndim >= 2^32 elements.  DH_ERR_VALUE: a NaN, a strand's sequence that decreases, a strand point with
 * ln L <= logl_min, a plateau of p >= n + 1 points (no positive volume is left; the reference's log fails there).
 * DH_ERR_NOMEM.  After a fold dh_merged_bootstrap, dh_merged_bootstrap_run and the DH_KLD_RESAMPLE / DH_KLD_SIMULATE
 * modes of dh_merged_kld answer DH_ERR_ARG: the strand bootstrap is not defined for a run that carries dynamic batches. */
int dh_merged_fold(dh_ctx* ctx, int problem, int strands, int nlive_new, int64_t stride, const int64_t* niter,
                   const double* dead_logl, const double* live_logl, const double* dead_u, const double* live_u,
                   const int32_t* dead_id, const int32_t* dead_it, const int32_t* dead_nc, const int32_t* live_it,
                   double logl_min, double logl_max, double* summary_out);

/* ---- the seeds of a dynamic batch, chosen where the merged run lives (csrc/merge_seed.hip) --
 * dh_merged_batch_seed chooses the start points of `strands` strands of one batch in one call: the reference's
 * _configure_batch_sampler (dynamicsampler.py:394-416 the subset, :457-533 the weighted choice without replacement,
 * :606-610 vol_idx), dynamic.batch_seed on the host.  The choice is the reference's successive sampling, order of the
 * draws included, written as a pure function (Plackett-Luce: the nlive_new largest of logvol_i + Gumbel noise):
 *   words   strand s of the call is the global strand first + s and uses subsequence 2^63 + 2^62 + first + s of the
 *           Philox4x32-10 stream keyed by `seed` (volume realizations stay below 2^63, bootstraps are 2^63 + b); point
 *           i -- its index in the merged run -- takes words 2 i and 2 i + 1; u = 2^-53 + m 2^-53 in (0, 1] as for the
 *           realizations
 *   key     logvol_i - log(-log u); u = 1 gives +inf, a legal key that is always chosen
 *   order   descending key, equal keys by smaller i; the strand's seeds are the first nlive_new points, in that order
 *   subset  lo = #{logl <= logl_min}; lo = 0: from the prior, no choice is made; fewer than nlive_new points above
 *           logl_min: the boundary moves down to the last nlive_new points and logl_min becomes logl[lo' - 1], or -inf
 *           at lo' = 0 (the seeds stand, the strand is a prior strand); vol_idx = argmin |logl - logl_min| + 1, first
 *           occurrence; the start row is (logvol, logz, information, logzerr^2, logl) at vol_idx - 1
 * idx_out / key_out (optional, strands x nlive_new): the chosen indices into the merged run in draw order, their keys.
 * u_out (optional, strands x nlive_new x ndim) / logl_out (optional, strands x nlive_new): the chosen points' unit-cube
 * rows and ln L, gathered on the device and brought down in one piece -- what dh_ns_batch takes as seed_u and
 * seed_logl; the logl and logvol columns never cross.
 * info_out (required, 12 doubles): prior (0 / 1), lo, count (points of the subset), n_pos (those of positive weight),
 * logl_min (effective), vol_idx, start[5] (NaN for a prior batch), the select's histogram passes.  n_pos < nlive_new
 * (dynamic.batch_seed's ValueError) and prior = 1 with lo = 0 and n_pos = 0 are answers in info_out, not errors: no
 * choice is returned.
 * Departures from dynamic.batch_seed: (a) the stream is Philox, not the Generator's; the law is the same, the indices
 * are not; (b) a point has positive weight iff logvol_i - max(logvol over the subset) >= -708, a threshold on exp's
 * argument where the host tests exp(..) / sum > 0 (the two libraries' exp may differ at the denormal edge); (c) more
 * than 2048 exactly equal keys at a strand's threshold -- every one u = 1 -- are DH_ERR_VALUE.
 * Not built: a staging block that would keep the chosen rows on the device for dh_ns_batch.
 * Errors, all leaving the merged run as it was: DH_ERR_ARG: no merged run, strands < 1 or > 65536, nlive_new < 1 or
 * > 65535, NaN logl_min, info_out NULL, first < 0, strands x nlive_new x ndim >= 2^32.  DH_ERR_VALUE: no point above
 * logl_min (the reference's RuntimeError).  DH_ERR_NOMEM. */
int dh_merged_batch_seed(dh_ctx* ctx, uint64_t seed, int64_t first, int strands, int nlive_new, double logl_min,
                         int64_t* idx_out_or_null, double* key_out_or_null, double* u_out_or_null, double* logl_out_or_null,
                         double* info_out);

/* ---- marginals of the merged run --------------------------------------------------------
 * All three work on the merged run's parameter rows (the SAMPLES field) and normalised weights (the WEIGHT field)
 * where they live; only the results come to the host.  Every sum of weights is a sum of the integers
 * W_i = llrint(w_i 2^62): exact and independent of order, so the results are bitwise reproducible.  cols_or_null:
 * ncol column indices (repeats allowed, at most 512), or NULL with ncol = ndim for all columns in order.
 * DH_ERR_ARG (the merged run stays in place): no merged run, a column outside [0, ndim), a size cap, and what each
 * call names below.
 *
 * Weighted quantiles -- utils.quantile(x, q, weights) (utils.py:1190-1234), which plotting._make_subplots's spans
 * are too (plotting.py:80-93).  The order of a column is (value, point index) ascending = np.argsort(kind="stable");
 * C_k = the sum of W over its first k points, Norm = C_{M-1} (the reference's cumsum(sw)[:-1]).  q = 0: the column
 * minimum; q = 1 or q Norm >= Norm: the maximum (np.interp's ends); otherwise with T = q Norm and k the largest with
 * C_k <= T: x_(k) + (T - C_k) / W_(k) (x_(k+1) - x_(k)).  out: ncol x nq.  DH_ERR_ARG: nq outside [1, 16], a q
 * outside [0, 1] or NaN.  DH_ERR_VALUE: Norm = 0 for a column and a q inside (0, 1) (the reference divides by zero;
 * q = 0 and q = 1, the extremes, do not depend on Norm and are returned for such a column too). */
int dh_merged_quantile(dh_ctx* ctx, int nq, const double* q, int ncol, const int32_t* cols_or_null, double* out);
/* 1-D weighted histograms -- np.histogram(x, bins, weights=weights) as plotting.py:1356 calls it.  edges: per column
 * nbins + 1 non-decreasing finite values.  A point falls in bin i = the largest i with edges[i] <= x;
 * x == edges[nbins] belongs to the last bin; points outside are dropped (np.histogram's membership, bin for bin).
 * out (ncol x nbins): the bins' sums of W scaled by 2^-62, or with weighted = 0 the counts.  DH_ERR_ARG: nbins outside
 * [1, 4096], decreasing or non-finite edges. */
int dh_merged_hist1d(dh_ctx* ctx, int ncol, const int32_t* cols_or_null, int nbins, const double* edges, int weighted,
                     double* out);
/* 2-D weighted histograms -- np.histogram2d(x, y, bins, weights=weights) as plotting.py:2159-2294 calls it.  pairs:
 * npair x 2 columns (x, y); xedges npair x (nbx + 1), yedges npair x (nby + 1); the membership rule of
 * dh_merged_hist1d per axis, a point counts where both axes are inside.  out: npair x nbx x nby.  DH_ERR_ARG:
 * nbx x nby above 16384 (one pair's table of 64-bit sums in a workgroup's LDS), npair outside [1, 65536], decreasing
 * or non-finite edges. */
int dh_merged_hist2d(dh_ctx* ctx, int npair, const int32_t* pairs, int nbx, int nby, const double* xedges,
                     const double* yedges, int weighted, double* out);

/* ---- statistical errors of the merged run ------------------------------------------------
 * Realizations of the prior-volume sequence -- utils.jitter_run (utils.py:1317-1408) -- and reweighting --
 * utils.reweight_run (utils.py:1663-1708) -- where the merged run lives.  Realization r >= 0 is a global index: point
 * k's volume shrinks by t_k = u_k^(1 / n_k), n_k the SAMPLES_N field and u_k = uniform_double(w_2k, w_2k+1) in (0, 1]
 * of the words of subsequence r of the Philox4x32-10 stream keyed by `seed` (rocrand's stream model and transform).
 * For a merged run, whose live count never drops by more than 1 per point, that is the distribution of the
 * reference's exact form and of approx=True alike; the stream is not NumPy's.  A realization is a function of
 * (seed, r) alone: bit-identical alone, in a batch of any size, at any position.  jitter = 0 takes the expected
 * volumes instead, the merged run's own steps -log1p(1 / n_k).  logrwt_or_null: M values on the host added to ln w
 * (ln of the new over the old target); -inf is a weight of 0.  The integrals are utils.compute_integrals'
 * (utils.py:1411-1467), every sum in a fixed order.
 * DH_ERR_ARG (nothing was touched): no merged run, jitter outside {0, 1}, and what each call names below.
 * DH_ERR_VALUE: a NaN or +inf in logrwt.  The merged run stays in place after either.
 *
 * Realizations first .. first + nreal - 1 at once.  logz: nreal values of ln Z; h (or NULL): the information
 * sum(w0 l0 + w1 l1) - ln Z (the two trapezoid halves, WITHOUT logrwt, as the reference); ess (or NULL):
 * (sum w)^2 / sum w^2; mean (want_mean = 1: nreal x ndim, else NULL with want_mean = 0): sum w v / sum w.
 * DH_ERR_ARG: nreal outside [1, 65536], nreal != 1 with jitter = 0, first < 0, logz NULL, want_mean or mean without
 * the other. */
int dh_merged_realize(dh_ctx* ctx, uint64_t seed, int64_t first, int nreal, int jitter, const double* logrwt_or_null,
                      int want_mean, double* logz, double* h, double* ess, double* mean);
/* `count` points from point `first` on of one per-point field of realization `real`: DH_MERGED_LOGVOL (ln X),
 * DH_MERGED_LOGWT or DH_MERGED_LOGZ (cumulative).  The last LOGZ equals dh_merged_realize's ln Z of that realization
 * to rounding (the same terms, summed as the merge's own scan sums them).  DH_ERR_ARG: real < 0, another field, a
 * slice outside [0, M). */
int dh_merged_realization(dh_ctx* ctx, uint64_t seed, int64_t real, int jitter, const double* logrwt_or_null, int field,
                          int64_t first, int64_t count, double* out);

/* The strand bootstrap of the merged run (the reference's utils.resample_run, and with
 * jitter = 1 its jitter_run after it).  A strand is a (run, live slot) pair, its key run * nlive + slot, S = runs *
 * nlive of them.  Bootstrap b >= 0 draws S strands from subsequence 2^63 + b of the Philox4x32-10 stream keyed by
 * `seed`: draw j takes words 2j and 2j + 1, the strand is the high 64 bits of (w0 | w1 << 32) S.  The resampled run is
 * every merged point repeated as often as its strand was drawn, in merged order, M' points; its live counts follow the
 * reference's rule (ties included), its integrals are dh_merged_realize's over the expanded sequence with realization
 * index b (jitter = 0: the expected volumes).  Results of bootstraps first .. first + nboot - 1: logz, h, ess, npoints
 * (M') of nboot each (h, ess, npoints may be NULL), mean [nboot][ndim] with want_mean.  A bootstrap's numbers depend on
 * (seed, b) alone.  mult_or_null: S host values >= 0 in strand-key order that replace the drawn multiplicities
 * (nboot = 1; their sum need not be S).
 * DH_ERR_ARG (the merged run stays): no merged run, a merge without id / it / nc, a run that holds dynamic batches
 * (dh_merged_fold: strands are read off a live count that only falls), nboot outside [1, 65536], first < 0,
 * jitter not 0 or 1, mult with nboot != 1 or a negative entry, M' = 0 or M' >= 2^31, want_mean without mean or the
 * reverse, no logz. */
int dh_merged_bootstrap(dh_ctx* ctx, uint64_t seed, int64_t first, int nboot, int jitter, const int32_t* mult_or_null,
                        int want_mean, double* logz, double* h, double* ess, double* mean, int64_t* npoints);
/* `count` points from point `first` on of one per-point field of bootstrap `boot`: DH_MERGED_LOGVOL, DH_MERGED_LOGWT,
 * DH_MERGED_LOGZ (cumulative) as doubles, DH_MERGED_SAMPLES_N as int32, DH_MERGED_SRC as int64.  npoints (may be NULL)
 * receives M', also with count = 0: the way to size a fetch.  DH_ERR_ARG as above, another field, a slice outside
 * [0, M'). */
int dh_merged_bootstrap_run(dh_ctx* ctx, uint64_t seed, int64_t boot, int jitter, const int32_t* mult_or_null, int field,
                            int64_t first, int64_t count, void* out, int64_t* npoints);

/* ---- divergence, weight function -----------------------------------------------------------
 * utils.kld_error (utils.py:1932-1997) in batches: the Kullback-Leibler divergence from the merged run to realizations
 * (DH_KLD_JITTER: realization r of dh_merged_realize under the same stream, no logrwt) or strand bootstraps
 * (DH_KLD_RESAMPLE: bootstrap b of dh_merged_bootstrap with jitter = 0; DH_KLD_SIMULATE: with jitter = 1) first ..
 * first + n - 1.  With lq_k = LOGWT_k - LOGZ_{M-1}, per-point ln w_p of the realization, Z = ln sum exp ln w_p and
 * src(p) the merged index of position p (the identity for JITTER):
 *   kld = sum_p exp(ln w_p - Z) ((ln w_p - Z) - lq_src(p)).
 * A position of weight 0 adds 0 (the reference's 0 x inf is NaN there); a positive weight where lq is -inf makes the
 * result +inf; the bootstrap modes may be negative, as the reference's are (lq[src] is not normalised over the resampled
 * run).  kld: n values; logz_or_null: their ln Z (bit for bit dh_merged_realize's / dh_merged_bootstrap's);
 * npoints_or_null: the realizations' lengths (M for JITTER).  mult_or_null: as dh_merged_bootstrap (bootstrap modes,
 * n = 1).  A result depends on (seed, index) alone: bit-identical alone, in any batch, at any position.
 * DH_ERR_ARG (the merged run stays): no merged run, another mode, n outside [1, 65536], first < 0, kld NULL, mult with
 * JITTER, and what dh_merged_bootstrap refuses for the bootstrap modes.
 * The cumulative form is the field DH_MERGED_KLD of dh_merged_realization (without logrwt) and
 * dh_merged_bootstrap_run; its last value equals this call's to rounding. */
enum { DH_KLD_JITTER = 0, DH_KLD_RESAMPLE = 1, DH_KLD_SIMULATE = 2 };
int dh_merged_kld(dh_ctx* ctx, uint64_t seed, int64_t first, int n, int mode, const int32_t* mult_or_null, double* kld,
                  double* logz_or_null, int64_t* npoints_or_null);
/* dynamicsampler.weight_function (dynamicsampler.py:48-170) of the merged run.  zweight_k = exp(lzw_k - ln sum exp lzw),
 * lzw_k = Ztot + log(-expm1(LOGZ_k - Ztot)) - log(n_k), Ztot = logaddexp(LOGZ_{M-1}, LOGL_{M-1} + LOGVOL_{M-1}): the
 * reference's ln(exp(Ztot) - exp(logz_k)) without its cancellation; 1 / M where LOGZ_0 == LOGZ_{M-1} (its
 * np.ptp(logz) == 0 branch).  pweight is the WEIGHT field, weight = (1 - pfrac) zweight + pfrac pweight.  idx (or NULL):
 * the first and last point with weight > maxfrac x max(weight); logl_bounds: (logl_min, logl_max) after the padding and
 * overflow rules of lines 147-166 (+-inf at the ends).  Only these four numbers leave the device.
 * DH_ERR_ARG (the merged run stays): no merged run, pfrac or maxfrac outside [0, 1] or NaN, pad < 0, logl_bounds NULL.
 * DH_ERR_VALUE: no weight lies above maxfrac x the largest (maxfrac = 1; the reference fails there too). */
int dh_merged_weight_function(dh_ctx* ctx, double pfrac, double maxfrac, int64_t pad, double* logl_bounds, int64_t* idx);
/* `count` points from point `first` on of pweight (DH_WEIGHT_P), zweight (DH_WEIGHT_Z) or weight (DH_WEIGHT_BOTH) above.
 * DH_ERR_ARG: no merged run, pfrac outside [0, 1], another `which`, a slice outside [0, M). */
enum { DH_WEIGHT_P = 0, DH_WEIGHT_Z = 1, DH_WEIGHT_BOTH = 2 };
int dh_merged_weights(dh_ctx* ctx, double pfrac, int which, int64_t first, int64_t count, double* out);

#ifdef __cplusplus
}
#endif
#endif /* DYNHIP_H */
