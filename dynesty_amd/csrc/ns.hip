// Device-resident ensemble of static nested-sampling runs (SURVEY.md section 8f-1,
// BASELINE config C5).  The run loop of the reference (sampler.py:932-1212:
// pop the worst live point, replace it by a proposal that beats it, integrate
// ln Z; :676-778 queue semantics; :625-674 bound-update policy) is executed on
// the GPU for `runs` independent runs at once; the host only enqueues a fixed
// kernel sequence per queue fill and polls a done-counter every few fills.
//
//   per fill:  ns_prepare  (policy: switch unit cube -> bound, schedule rebuilds)
//              rebuild pipeline + enlarge        (only runs that asked for it)
//              ns_select   (K start points, proposal frames, walker RNG streams)
//              unit-cube / rwalk walk kernels    (all runs x K walkers, one launch each)
//              ns_gather   (the walkers' start coordinates)
//              ns_consume  (queue consumption per run: slots sorted once, deaths walk that
//                           order; dead-point record, evidence integration, tuning)
//   at the end: ns_finish  (append the final live points, write the record; reads the state, changes nothing)
//   dh_ns_continue (a kept ensemble taken further): ns_resume (which runs go on; a fill that a stop rule cut
//              short is put back) and one ns_consume replay of those fills, then the fills as above
//   dh_ns_batch (strands of a dynamic batch, started inside a finished run): ns_batch_init, the bound on the seeds,
//              seed fills of ns_seed_prepare / ns_select / ns_gather / walk / ns_seed_consume, ns_batch_start (the
//              hand-over), then the fills as above
//
// All state (live points, dead points, integrals, RNG) stays in HBM; with
// 288 GB there is room for the full dead-point history of thousands of runs.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include <cmath>

#include "ctx.h"
#include "ns_batch_plan.h"
#include "ns_sort.h"
#include "ns_state.h"
#include "rng_pcg64.h"
#include "stage_plan.h"

using namespace dh;


namespace {

constexpr int kT = 256;
// Phase B of ns_consume sums a fill's weights relative to M, the largest of them: a ln Z_e more than this far below M
// is lost to it (exp underflows at -745; the margin keeps every term that matters to H_e in the normal range)
constexpr double kNsUnder = 600.0;
enum : int { MODE_CUBE = 0, MODE_BOUND = 1, MODE_DONE = 2, MODE_FAILED = 3, MODE_WAIT = 4 /* run_mode only: sits this fill out */ };

struct NsRun {
  double logvol, logz, h, lmax, scale, loglstar, dead_prev;
  long long it, ncall, ncall_last_update;
  int mode, need_rebuild, nbound, nfill;
  int acc, rej, doubling, due;  // due: a bound update the run is waiting for (see ns_prepare: rebuild_fill)
  double logzvar;
  uint64_t rng[4];
  long long nc_carry;  // calls of the entries popped after the last death: charged to the NEXT death (sampler.py:1141)
  // likelihood plateau (sampler.py:1112-1127, 1190-1193): deaths still to be taken with the plateau's volume
  // step (0 = not in plateau mode), ln of that step's volume, and the two sums that make var[ln Z] exact
  // although the dead points' d ln X is then no longer constant (see ns_finish)
  int pcount, sampler_failed;  // (sampler_failed: a uniform-sampler walker gave up, see ns_consume)
  // forced_exact: a start point of the run's CURRENT queue (selected, kept) lies outside its bound and the forced
  // update waits for the next fill that builds bounds; the run proposes and consumes nothing until then
  // qstop (kept ensembles, dh_ns_continue): > 0 = a stop rule ended the run inside a fill after this many of the
  // queue's entries, and what the fill found before it is saved (NsArgs::sv_*); -1 = ns_resume has put that state back
  // and the fill is consumed again, whole, under the call's criteria; 0 otherwise
  int fpend, qstop;
  double plogdvol, var_a, var_b;
};

struct NsArgs {
  int runs, nlive, ndim, K, walks, bound_multi, max_ells;
  int sampler;  // 0 rwalk, 1 rslice, 2 slice, 3 unif ; `walks` holds the slice count for 1, 2 (unused for 3)
  int bootstrap;  // replicas of the bootstrap expansion per rebuild (0: none)
  long long cap;  // dead-point capacity per run
  double dlogz, enlarge_log, facc, first_eff;
  long long first_ncall, update_interval;
  // run_nested's other stopping rules (sampler.py:1070-1093; dh_ns_set_option): maxiter / maxcall < 0 = none,
  // logl_max = +inf = none; add_live = 0: the record is the dead points' running evidence (no final live points)
  long long maxiter = -1, maxcall = -1;
  double logl_max = INFINITY;
  int add_live = 1;
  int store_samples;
  long long* prof;   // optional (DH_NS_PROF=1): cycle counters of ns_consume's phases, run 0
  int rebuild_sync;  // 1: all bound-mode runs rebuild whenever any run is due (see ns_prepare)
  int rebuild_fill;  // 1: this fill builds bounds; 0: a run that is due waits (idle) for the next fill that does
  int serial_walk;   // diagnostic (DH_NS_SERIAL=1): ns_consume walks every queue with the one-wavefront routine
  // (round 6) the slot order of every run's live points for THIS fill, sorted by the generator pass's presort workgroups
  // beside the walk (dh_ctx::PresortReq); presorted = 1: ns_consume reads it instead of sorting
  const unsigned short* presort;
  int presort_stride, presorted;
  NsRun* st;
  double* live_u;
  double* live_v;
  double* live_logl;
  double* dead_logl;
  double* dead_u;      // optional
  // queue
  double* q_u0;
  int* q_frame;
  uint64_t* q_rng;
  uint64_t* q_rng_out;
  double* r_u;
  double* r_v;
  double* r_logl;
  int* r_a;  // naccept | ncalls (unit cube, slice)
  int* r_b;  // nreject | flags (unit cube) | nexpand (slice)
  int* r_c;  // ncontract (slice)
  int* r_d;  // flags (slice)
  int* run_doubling;
  // per-run walk parameters
  double* run_loglstar;
  double* run_scale;
  int* run_mode;
  int* rebuild_mask;
  int* force;  // runs: set by the start-point membership check of the previous fill (forced rebuild, sampler.py:484-489)
  // DH_NS_OPT_FORCED_EXACT: the forced update inside the fill that found the start point
  int forced_exact;
  int* force_first;   // runs: queue index of the first start point outside the bound (INT_MAX: none)
  // (forced_exact) update_bound_if_needed runs when the queue's last entry has been POPPED, before its point replaces the
  // worst one (sampler.py:771-772, 1176-1185): when that entry made the fill's last death, the slot's previous content
  // is kept here and stands in the live set while the next regular bound is built (ns_swap_undo)
  double* undo_u;     // runs x ndim
  int* undo_slot;     // runs: the slot, or -1
  uint64_t* sel_ent;  // runs x 4: the words ns_select seeded this fill's walker selections from
  // (forced_exact) what this fill does to the run's bound: 0 nothing, 1 regular update (built before the queue is
  // selected), 2 forced update (built after: the queue found a start point outside); the runs a selection /
  // membership pass serves (MODE_BOUND / MODE_WAIT per run); which pass ns_select / ns_gather are in
  int* fx_kind;
  int* pass_mode;
  int fx_pass;  // 0: not forced_exact; 1: before the fill's rebuild (every run but the regular updates'); 2: after (those)
  int* ndone;
  // bound (rebuild outputs)
  int* nells;
  int* bstatus;
  double* b_ctrs;
  double* b_covs;
  double* b_ams;
  double* b_axes;
  double* b_axl;
  double* b_lv;
  double* b_cum;        // unif sampler: rand_choice weights of the run's ellipsoids, cumulated (bounding.py:726-731)
  uint64_t* boot_ent;   // runs x 4: the words a rebuilding run drew for its bootstrap replicas
  double* run_shift;    // runs: ndim * ln(bootstrap expansion factor) of the rebuild just done
  // results
  double* records;  // runs x 8: logz, logzerr, niter, ncall, h, nbound, status, eff
  double* fin_ws;   // runs x fin_stride: ns_finish's per-point terms (3 nlive) and, for large live sets, the sorted values
  size_t fin_stride;
  // dh_ns_consume (one queue consumption as an operator of its own): death list of THIS call
  int dead_rel;     // 1: dead_logl rows are K wide and hold this call's deaths from index 0
  int* trace_slot;  // runs x K or null: slot of every death
  int* trace_src;   // runs x K or null: queue index of its replacement
  int* trace_n;     // runs x 2 or null: number of deaths kept, stopped flag
  // per-point bookkeeping of the reference's saved_run (sampler.py:1165-1182), all optional (null together):
  int* live_it;  // runs x N   in/out: iteration at which the point living in the slot was proposed (0 = initial)
  int* dead_id;  // like dead_logl: slot of the dead point                        ('id')
  int* dead_it;  //                 iteration at which it had been proposed        ('it')
  int* dead_nc;  //                 likelihood calls spent to replace it           ('nc')
  // Kept ensembles (dh_ns_keep; null together otherwise): what the fill in which a stop rule ended a run found before
  // it -- the run's state and the previous content of the slots the fill replaced -- so that dh_ns_continue can take
  // the whole fill again under other criteria (ns_resume puts it back, `replay` consumes the same r_* rows)
  NsRun* sv_st;      // runs
  double* sv_u;      // runs x K x ndim
  double* sv_v;      // runs x K x ndim
  double* sv_logl;   // runs x K
  int* sv_slot;      // runs x K
  int* sv_it;        // runs x K   (live_it of the slot)
  int* sv_n;         // runs: slots saved
  int* rest;         // runs: queue entries the continuation took over (ns_resume)
  int replay;        // 1: ns_consume serves the runs with qstop == -1 only; no tuning, no fill count
};

// dh_ns_batch: the seeding phase's own arrays (the kernels ns_batch_init, ns_seed_prepare, ns_seed_consume and
// ns_batch_start take them beside NsArgs, whose layout -- part of a saved image's plan -- stays as it is)
struct NsSeed {
  double* u;         // runs x N x D  the staging live set, in the order its points were accepted
  double* v;         // runs x N x D
  double* logl;      // runs x N
  int* nc;           // runs x N      calls of a staged point: its entry's and the rejected entries' before it
  int* n;            // runs          rows staged
  long long* rej;    // runs          calls of the rejected entries since the last staged row
  long long* ncall;  // runs          the calls the phase spent (written at the hand-over)
  uint64_t* rng;     // runs x 4      the run's generator at the hand-over
  double* start;     // runs x 6      logvol, logz, h, logzvar, last dead ln L, scale: where the strand joins the base run
  double logl_min;
};

__device__ __forceinline__ double logaddexp_dev(double x, double y) {
  if (x == y) return x + 0.6931471805599453;
  const double d = x - y;
  if (d > 0) return x + log1p(exp(-d));
  if (d <= 0) return y + log1p(exp(d));
  return x + y;
}

// progress_integration (utils.py:1470-1492), one dead point.  ns_consume's phase B does not run it (see there) except
// for var[ln Z] of a fill with a plateau death whose ln Z_e is out of its linear sums' reach (kNsUnder).
__device__ __forceinline__ void integrate_step(double& logz, double& h, double& logzvar, double lprev,
                                               double lnew, double logvol, double dlv) {
  const double logdvol = logvol + log(0.5 * expm1(dlv));
  const double logwt = logaddexp_dev(lnew, lprev) + logdvol;
  const double logz_new = logaddexp_dev(logz, logwt);
  const double t0 = exp(lprev - logz_new + logdvol), t1 = exp(lnew - logz_new + logdvol);
  const double lzterm = (t0 > 0.0 ? t0 * lprev : 0.0) + (t1 > 0.0 ? t1 * lnew : 0.0);
  const double w = exp(logz - logz_new);
  const double h_new = lzterm + (w > 0.0 ? w * (h + logz) : 0.0) - logz_new;
  logzvar += (h_new - h) * dlv;  // logzvar_new = logzvar + dh * dlogvol
  h = h_new;
  logz = logz_new;
}

// ---- init: RNG, uniform live points --------------------------------------
__global__ void __launch_bounds__(kT)
    ns_init(NsArgs a, const uint32_t* __restrict__ entropy, int nwords, uint32_t first_run) {
  const int run = blockIdx.x, t = threadIdx.x;
  const int N = a.nlive, D = a.ndim;
  // every live point gets its own stream: child (first_run + run) * N + i of the entropy
  for (int i = t; i < N; i += kT) {
    Pcg64 g;
    seed_from_child(g, entropy, nwords, (uint32_t)((first_run + run) * (uint32_t)N + i));
    double* u = a.live_u + ((size_t)run * N + i) * D;
    for (int j = 0; j < D; ++j) u[j] = g.next_double();
  }
  if (t == 0) {
    NsRun r;
    r.logvol = 0.0;
    r.logz = -1e300;
    r.h = 0.0;
    r.lmax = -1e300;
    r.scale = 1.0;
    r.loglstar = -1e300;
    r.dead_prev = -1e300;
    r.it = 0;
    r.ncall = N;
    r.ncall_last_update = 0;
    r.mode = MODE_CUBE;
    r.need_rebuild = 0;
    r.nbound = 0;
    r.nfill = 0;
    r.acc = r.rej = r.doubling = r.due = 0;
    r.fpend = r.qstop = 0;
    r.logzvar = 0.0;
    r.nc_carry = 0;
    r.pcount = r.sampler_failed = 0;
    r.plogdvol = r.var_a = r.var_b = 0.0;
    Pcg64 g;
    seed_from_child(g, entropy, nwords, 0x80000000u + first_run + (uint32_t)run);
    g.store(r.rng);
    a.st[run] = r;
  }
}

// ---- wave-level minimum helpers (the queue walk of ns_consume) --------------------------------------
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  // butterflies inside each row of 16 lanes, then row_bcast15 / row_bcast31: lane 63 holds the minimum
#define DH_DPP_MIN(ctrl, rmask) \
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rmask, 0xF, false))
  DH_DPP_MIN(0xB1, 0xF);   // quad_perm [1,0,3,2]
  DH_DPP_MIN(0x4E, 0xF);   // quad_perm [2,3,0,1]
  DH_DPP_MIN(0x141, 0xF);  // row_half_mirror
  DH_DPP_MIN(0x140, 0xF);  // row_mirror
  DH_DPP_MIN(0x142, 0xA);  // row_bcast:15 -> rows 1, 3
  DH_DPP_MIN(0x143, 0xC);  // row_bcast:31 -> rows 2, 3
#undef DH_DPP_MIN
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// lane holding the smallest of the wave's 64 keys (lowest lane on ties) and that key
__device__ __forceinline__ int wave_argmin(double key, double* kmin) {
  unsigned long long bits = (unsigned long long)__double_as_longlong(key);
  bits = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);  // order-preserving image
  const unsigned hi = (unsigned)(bits >> 32), lo = (unsigned)bits;
  const unsigned mh = wave_min_u32(hi);
  const unsigned ml = wave_min_u32(hi == mh ? lo : 0xFFFFFFFFu);
  const unsigned long long win = __ballot(hi == mh && lo == ml);
  const int l = __ffsll((long long)win) - 1;
  const int klo = __builtin_amdgcn_readlane((int)(unsigned)__double_as_longlong(key), l);
  const int khi = __builtin_amdgcn_readlane((int)(unsigned)(__double_as_longlong(key) >> 32), l);
  *kmin = __longlong_as_double(((long long)khi << 32) | (unsigned)klo);
  return l;
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ---- after the initial evaluation: the worst and the best live log-likelihood of every run ------------
__global__ void __launch_bounds__(kT) ns_start(NsArgs a) {
  const int run = blockIdx.x, t = threadIdx.x, N = a.nlive;
  __shared__ double rmax[kT], rmin[kT];
  double mx = -1e300, mn = INFINITY;
  for (int i = t; i < N; i += kT) {
    const double k = a.live_logl[(size_t)run * N + i];
    mx = fmax(mx, k);
    mn = fmin(mn, k);
  }
  rmax[t] = mx;
  rmin[t] = mn;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (t < s) {
      rmax[t] = fmax(rmax[t], rmax[t + s]);
      rmin[t] = fmin(rmin[t], rmin[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) {
    a.st[run].lmax = rmax[0];
    a.st[run].loglstar = rmin[0];
  }
}

// ---- friends bounds: every run's metric starts as the identity (RadFriends(ndim), cov=None) -----------------
__global__ void __launch_bounds__(256) ns_fr_eye(double* am, int runs, int d) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, dd = (size_t)d * d;
  if (e >= (size_t)runs * dd) return;
  const size_t k = e % dd;
  am[e] = (k / d == k % d) ? 1.0 : 0.0;
}

// ---- policy (sampler.py:625-674 update_bound_if_needed) ------------------------
// One workgroup looks at all runs.  With rebuild_sync the runs of the ensemble rebuild
// TOGETHER: as soon as any run is due, every run that already samples from a bound joins
// (its rebuild comes early, never late).  A rebuild is a latency-bound tree construction
// that costs about the same for 1 or 64 runs; with rwalk every run spends exactly
// K * walks calls per fill, so after the first joint rebuild all runs are due in the same
// fill and the ensemble pays one rebuild per update interval instead of one per fill.
__global__ void __launch_bounds__(kT) ns_prepare(NsArgs a) {
  const int t = threadIdx.x;
  int any = 0;
  for (int run = t; run < a.runs; run += kT) {
    NsRun& r = a.st[run];
    int want = 0;
    if (r.fpend) {
      // its queue is selected and waits for the forced update: nothing is decided for it (ns_force_prepare takes it in
      // the next fill that builds bounds)
    } else if (r.mode == MODE_CUBE || r.mode == MODE_BOUND) {
      if (r.mode == MODE_BOUND && a.bstatus[run] != DH_OK) {
        r.mode = MODE_FAILED;
        atomicAdd(a.ndone, 1);
      } else {
        const double eff = 100.0 * (double)(r.it > 0 ? r.it : 1) / (double)r.ncall;
        if (r.mode == MODE_CUBE) {
          want = (r.ncall >= a.first_ncall && eff < a.first_eff) ? 1 : 0;
        } else if (r.ncall >= r.ncall_last_update + a.update_interval || (a.force && a.force[run])) {
          // (force: a start point of the last fill lay outside the bound, sampler.py:484-489)
          want = 1;
        }
        if (r.due) want = 1;
      }
    }
    // The rebuild is a latency chain that costs about the same for one run or sixty-four, so the loop builds bounds
    // only every rebuild_every-th fill: a run that becomes due in between WAITS -- it proposes nothing and consumes
    // nothing until then.  Runs are independent, so idling changes nothing in a run's own sequence (rebuild on the
    // same live set, then walk with the same generator state): results are those of the reference schedule.
    if (want && !a.rebuild_fill) {
      r.due = 1;
      want = 0;
    }
    r.need_rebuild = want;
    any |= want;
  }
  any = __syncthreads_or(any);
  for (int run = t; run < a.runs; run += kT) {
    NsRun& r = a.st[run];
    int need = r.need_rebuild;
    if (a.rebuild_sync && any && a.rebuild_fill && r.mode == MODE_BOUND && !r.fpend) need = 1;
    if (need) {
      if (r.mode == MODE_CUBE) r.mode = MODE_BOUND;
      r.due = 0;
      r.ncall_last_update = r.ncall;
      r.nbound += 1;
      if (a.bootstrap > 0) {  // get_seed_sequence(rstate, bootstrap) (utils.py:1002-1009): one draw per rebuild
        Pcg64 g;
        g.load(r.rng);
        for (int i = 0; i < 4; ++i) a.boot_ent[(size_t)run * 4 + i] = g.next64();
        g.store(r.rng);
      }
    }
    r.need_rebuild = need;
    // (a finished run keeps the flag of its last fill: a continuation's first ns_prepare reads it, dh_ns_continue)
    if (a.force && r.mode != MODE_DONE) a.force[run] = 0;
    a.rebuild_mask[run] = need;
    a.run_mode[run] = (r.due || (r.fpend && !a.rebuild_fill)) ? MODE_WAIT : r.mode;
    if (a.fx_kind) a.fx_kind[run] = need ? 1 : 0;
    a.run_loglstar[run] = r.loglstar;
    a.run_scale[run] = r.scale;
    a.run_doubling[run] = r.doubling;
  }
  // runs still in the unit-cube phase (the host stops launching that phase's kernel once there are none:
  // a run never returns to it)
  int ncube = 0;
  for (int run = t; run < a.runs; run += kT) ncube += a.st[run].mode == MODE_CUBE ? 1 : 0;
  ncube = __syncthreads_count(ncube > 0) ? 1 : 0;
  if (t == 0) a.ndone[1] = ncube;
}

// ---- queue fill: start points, frames, walker streams ---------------------------
constexpr int kMaxCum = 4096;  // ellipsoids per run the frame choice can weigh (32 KB of LDS)
__global__ void __launch_bounds__(kT) ns_select(NsArgs a) {
  __shared__ uint64_t ent[4];
  __shared__ double cum[kMaxCum];  // rand_choice weights of ALL ellipsoids of the run (bounding.py:726-731)
  __shared__ int Msh;
  __shared__ double mxs;
  const int run = blockIdx.x, t = threadIdx.x;
  const int N = a.nlive, K = a.K;
  NsRun& r = a.st[run];
  const int mode = r.mode;
  if (mode != MODE_CUBE && mode != MODE_BOUND) return;
  if (a.run_mode[run] == MODE_WAIT) return;  // waiting for its bound: the run proposes nothing this fill
  if (a.fx_pass == 1 && (a.fx_kind[run] == 1 || r.fpend)) return;  // selects after its rebuild / keeps its queue
  if (a.fx_pass == 2 && a.fx_kind[run] != 1) return;
  if (mode == MODE_BOUND && a.bstatus[run] != DH_OK) return;  // ns_prepare fails the run next fill
  int M = 1;
  if (t == 0) {
    Pcg64 g;
    g.load(r.rng);
    for (int i = 0; i < 4; ++i) ent[i] = g.next64();
    g.store(r.rng);
    if (a.sel_ent)
      for (int i = 0; i < 4; ++i) a.sel_ent[(size_t)run * 4 + i] = ent[i];
    if (mode == MODE_BOUND && a.bound_multi) {
      M = a.nells[run];
      if (M > kMaxCum) M = kMaxCum;  // unreachable: dh_ns_ensemble refuses max_ells > kMaxCum
      double mx = -INFINITY;
      for (int e = 0; e < M; ++e) mx = fmax(mx, a.b_lv[(size_t)run * a.max_ells + e]);
      mxs = mx;
    }
    Msh = M;
  }
  __syncthreads();
  M = Msh;
  if (M > 1) {
    // cumsum(exp(logvol_ells - logsumexp)): the exponentials on all threads, the running sum by one
    for (int e = t; e < M; e += kT) cum[e] = exp(a.b_lv[(size_t)run * a.max_ells + e] - mxs);
    __syncthreads();
    if (t == 0) {
      double c = 0.0;
      for (int e = 0; e < M; ++e) {
        c += cum[e];
        cum[e] = c;
      }
      const double inv = 1.0 / c;
      for (int e = 0; e < M; ++e) cum[e] *= inv;
    }
    __syncthreads();
    if (a.sampler == 3)
      for (int e = t; e < M; e += kT) a.b_cum[(size_t)run * a.max_ells + e] = cum[e];
  }
  const double loglstar = r.loglstar;
  for (int w = t; w < K; w += kT) {
    Pcg64 g;
    U128 is = {ent[0], ent[1] + (uint64_t)w};
    U128 iq = {ent[2], ent[3] + 2ull * (uint64_t)w};
    g.seed(is, iq);
    const size_t q = (size_t)run * K + w;
    int frame = 0;
    if (mode == MODE_BOUND && a.sampler != 3) {  // (the uniform sampler starts nowhere: internal_samplers.py:214-242)
      // a live point with logl > loglstar, uniformly (sampler.py:469-474)
      int i;
      int guard = 0;
      do {
        i = (int)g.interval((uint64_t)(N - 1));
      } while (!(a.live_logl[(size_t)run * N + i] > loglstar) && ++guard < 100000);
      a.r_d[q] = i;  // the chosen live point: ns_gather copies its coordinates (r_d is free until the walkers run)
      if (M > 1) {
        // min(searchsorted(cum, xr), M - 1): first index with cum[i] >= xr
        const double xr = g.next_double();
        int lo = 0, hi = M - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cum[mid] < xr) lo = mid + 1; else hi = mid;
        }
        frame = lo;
      }
    }
    a.q_frame[q] = run * a.max_ells + frame;
    g.store(a.q_rng + q * 4);
  }
}

// start points of the walkers: q_u0[q] = live_u[run, r_d[q]], one thread per coordinate over the whole ensemble (a
// thread per walker inside ns_select was a serial copy of D strided doubles: 0.23 ms per fill at D = 200)
__global__ void __launch_bounds__(256) ns_gather(NsArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int D = a.ndim, K = a.K, N = a.nlive;
  if (e >= (size_t)a.runs * K * D) return;
  const size_t q = e / D;
  const int j = (int)(e - q * D), run = (int)(q / K);
  if (a.st[run].mode != MODE_BOUND || a.bstatus[run] != DH_OK) return;
  if (a.run_mode[run] == MODE_WAIT) return;
  if (a.fx_pass == 1 && a.fx_kind[run] == 1) return;
  if (a.fx_pass == 2 && a.fx_kind[run] != 1) return;
  a.q_u0[e] = a.live_u[((size_t)run * N + a.r_d[q]) * D + j];
}

// ---- the forced update inside the fill (DH_NS_OPT_FORCED_EXACT; sampler.py:484-489) ----------------------------
// Sampler._fill_queue proposes the K start points one after the other; the first one that lies outside the bound
// rebuilds it at once (update_bound_if_needed(force=True): all live points, nbound + 1, the call counter of the last
// update reset), AFTER its own axes were drawn from the old bound (propose_live: get_random_axes stands before the
// membership test).  The later entries draw their axes from the new bound, which holds every live point, so there is
// at most one forced update per fill.  Here: the membership kernel has left force[run] and force_first[run];
// ns_force_prepare turns the flags into the rebuild mask and does the run's bookkeeping, ns_shadow_axes keeps the old
// frames of the masked runs in the second half of the axes array, the masked rebuild runs, and ns_reselect points the
// entries up to force_first at the kept frames and redraws the frames of the later ones from the new volumes (same
// variates: the selection generator of entry w is a function of the fill's four words and w).
// (forced_exact) the live set as the reference's regular bound update sees it: without the point that the previous
// fill's last queue entry brought in (see NsArgs::undo_u); launched before and after the masked rebuild (a swap)
__global__ void __launch_bounds__(64) ns_swap_undo(NsArgs a) {
  const int run = blockIdx.x;
  if (!a.rebuild_mask[run] || a.fx_kind[run] != 1) return;  // (a forced update sees the live set as it is)
  const int s = a.undo_slot[run];
  if (s < 0) return;
  for (int x = threadIdx.x; x < a.ndim; x += 64) {
    double* p = a.live_u + ((size_t)run * a.nlive + s) * a.ndim + x;
    double* q = a.undo_u + (size_t)run * a.ndim + x;
    const double tmp = *p;
    *p = *q;
    *q = tmp;
  }
}

// the runs a selection / membership pass serves -> pass_mode
__global__ void __launch_bounds__(kT) ns_pass_mask(NsArgs a, int pass) {
  for (int run = threadIdx.x; run < a.runs; run += kT) {
    const NsRun& r = a.st[run];
    const bool walking = r.mode == MODE_BOUND && a.run_mode[run] == MODE_BOUND && a.bstatus[run] == DH_OK;
    const int kd = a.fx_kind[run];
    a.pass_mode[run] = (walking && (pass == 1 ? kd != 1 : kd != 0)) ? MODE_BOUND : MODE_WAIT;
  }
}

// After the first membership pass.  A flagged run's forced update is built with this fill's bounds if the fill builds
// bounds; otherwise the run keeps its queue (start points, frames, streams, the selection words) and sits the fills
// out until one does -- runs are independent, so idling changes nothing in the run's own sequence (the same live set,
// the same generator state, the same queue: ns_prepare / ns_select leave a pending run alone), and the ensemble pays
// one rebuild chain per rebuild fill, as without forced updates.
__global__ void __launch_bounds__(kT) ns_force_prepare(NsArgs a) {
  for (int run = threadIdx.x; run < a.runs; run += kT) {
    NsRun& r = a.st[run];
    const int f = (a.force[run] && a.pass_mode[run] == MODE_BOUND) ? 1 : 0;
    if (f && a.rebuild_fill) {
      r.due = 0;
      r.fpend = 0;
      // update_bound_if_needed(-inf, force=True) records self.ncall (sampler.py:631-632, 674): the sampler's counter,
      // which at a refill does not yet hold the calls of the entries popped since the last death (they are still in
      // _new_point's ncall_accum, sampler.py:739-747) -- the carry
      r.ncall_last_update = r.ncall - r.nc_carry;
      r.nbound += 1;
      if (a.bootstrap > 0) {
        Pcg64 g;
        g.load(r.rng);
        for (int i = 0; i < 4; ++i) a.boot_ent[(size_t)run * 4 + i] = g.next64();
        g.store(r.rng);
      }
      a.fx_kind[run] = 2;
      a.rebuild_mask[run] = 1;
    } else if (f) {
      r.fpend = 1;
      a.run_mode[run] = MODE_WAIT;
      a.force_first[run] = 0x7fffffff;  // (found again, from the same queue and bound, in the fill that rebuilds)
    } else {
      if (a.pass_mode[run] == MODE_BOUND) {
        a.force_first[run] = 0x7fffffff;
        r.fpend = 0;  // (a pending run is flagged again by construction)
      }
    }
    a.force[run] = 0;  // (the membership test after the rebuild sets it again: update failed / a new pending run)
  }
}

__global__ void __launch_bounds__(256) ns_shadow_axes(NsArgs a) {
  const int run = blockIdx.x;
  if (!a.rebuild_mask[run] || a.fx_kind[run] != 2) return;
  const size_t dd = (size_t)a.ndim * a.ndim, n = (size_t)(a.bound_multi ? a.nells[run] : 1) * dd;
  const double* src = a.b_axes + (size_t)run * a.max_ells * dd;
  double* dst = a.b_axes + ((size_t)a.runs + run) * a.max_ells * dd;
  for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < n; i += (size_t)gridDim.y * 256) dst[i] = src[i];
}

__global__ void __launch_bounds__(kT) ns_reselect(NsArgs a) {
  __shared__ double cum[kMaxCum];
  __shared__ double mxs;
  const int run = blockIdx.x, t = threadIdx.x;
  if (!a.rebuild_mask[run]) return;
  const int N = a.nlive, K = a.K;
  NsRun& r = a.st[run];
  if (a.fx_kind[run] == 1) {
    // a regular update whose fresh queue has a start point outside the fresh bound (the point the bound was built
    // without, sampler.py:771-772): a forced update of its own, taken in the next fill that builds bounds
    if (t == 0 && a.force[run] && a.bstatus[run] == DH_OK) {
      r.fpend = 1;
      a.run_mode[run] = MODE_WAIT;
      a.force[run] = 0;
    }
    return;
  }
  if (a.force[run] || a.bstatus[run] != DH_OK) {
    // RuntimeError('Update of the ellipsoid failed') (sampler.py:489), or the rebuild itself failed: the run proposes
    // nothing; ns_prepare ends it at the next fill
    if (t == 0) {
      if (a.bstatus[run] == DH_OK) a.bstatus[run] = DH_ERR_CONTAIN;
      a.run_mode[run] = MODE_WAIT;
      a.force_first[run] = 0x7fffffff;
    }
    return;
  }
  int M = a.bound_multi ? a.nells[run] : 1;
  if (M > kMaxCum) M = kMaxCum;
  if (M > 1) {
    if (t == 0) {
      double mx = -INFINITY;
      for (int e = 0; e < M; ++e) mx = fmax(mx, a.b_lv[(size_t)run * a.max_ells + e]);
      mxs = mx;
    }
    __syncthreads();
    for (int e = t; e < M; e += kT) cum[e] = exp(a.b_lv[(size_t)run * a.max_ells + e] - mxs);
    __syncthreads();
    if (t == 0) {
      double c = 0.0;
      for (int e = 0; e < M; ++e) {
        c += cum[e];
        cum[e] = c;
      }
      const double inv = 1.0 / c;
      for (int e = 0; e < M; ++e) cum[e] *= inv;
    }
    __syncthreads();
  }
  const int jstar = a.force_first[run];
  const double loglstar = r.loglstar;
  const uint64_t* ent = a.sel_ent + (size_t)run * 4;
  for (int w = t; w < K; w += kT) {
    const size_t q = (size_t)run * K + w;
    if (w <= jstar) {
      a.q_frame[q] += a.runs * a.max_ells;  // its axes were drawn from the old bound
      continue;
    }
    int frame = 0;
    if (M > 1) {
      Pcg64 g;
      U128 is = {ent[0], ent[1] + (uint64_t)w};
      U128 iq = {ent[2], ent[3] + 2ull * (uint64_t)w};
      g.seed(is, iq);
      int i, guard = 0;
      do {
        i = (int)g.interval((uint64_t)(N - 1));
      } while (!(a.live_logl[(size_t)run * N + i] > loglstar) && ++guard < 100000);
      const double xr = g.next_double();
      int lo = 0, hi = M - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] < xr) lo = mid + 1; else hi = mid;
      }
      frame = lo;
    }
    a.q_frame[q] = run * a.max_ells + frame;
  }
  __syncthreads();
  if (t == 0) a.force_first[run] = 0x7fffffff;
}

// ---- consume the queue (sampler.py:732-778 + 1105-1185), one workgroup per run ----
// Only the walk over the queue is inherently serial (which proposal kills which live point
// depends on every earlier one): consume_sorted, one wavefront.  Everything transcendental -- the evidence integration of progress_integration
// (utils.py:1470-1492) and the dlogz stopping rule, ~10 exp/log per dead point -- is a
// prefix scan over the deaths of the fill and runs on all lanes afterwards:
//   ln Z_e   = logaddexp-scan of the trapezoid weights,
//   lmax_e   = running maximum of the inserted log-likelihoods,
//   stop     = first e with ln(1 + exp(lmax_e + lnX_e - lnZ_e)) < dlogz,
//   H_E      = e^{-lnZ_E} [ G_0 + sum_{e<=E} dX_e (L e^L terms) ] - lnZ_E   (G = e^{lnZ}(H + lnZ) is additive),
//   var lnZ += dlnX (H_E - H_0)                         (the per-step sum telescopes: dlnX is constant).
// If the stop index falls inside the fill, the walk is replayed up to it (once per run).
#define NS_PROF(i)                                              \
  do {                                                          \
    if (a.prof && run == 0 && t == 0) {                          \
      const long long now_ = clock64();                          \
      a.prof[i] += now_ - pt_;                                   \
      pt_ = now_;                                                \
    }                                                            \
  } while (0)

constexpr int kEPTMax = 8;  // deaths per lane in the scan phases: K <= kEPTMax * kT
// (round 6) ns_consume and its parallel walk are compiled for kEPT = 1, 2, 4, 8 deaths per lane and launched for the
// smallest that holds the queue: with one form for all, a queue of 512 carried eight-element register arrays and
// eight-trip loops of which two trips did anything.

// LDS of ns_consume: keys and slot sources by slot, the sorted slot order (padded to a power of two), the queue's
// arrays and the buffer of low replacements
__host__ __device__ inline size_t ns_consume_lds_full(int N, int K) {
  size_t P = 1;
  while (P < (size_t)N) P <<= 1;
  if (P < 256) P = 256;  // (the slot order is sorted 256 entries at a time at least)
  return (size_t)N * 12 + (size_t)K * 52 + P * 2 + 64;
}
// Large live sets (round 4).  A fill makes at most K deaths, so only the K + 1 smallest live points by
// (log-likelihood, slot) can take part in it: at least one of them outlives the fill and stands before every other
// point, which therefore is never the worst.  Where the whole set does not fit the arrays above (nlive > 32 kT, the
// register sort's reach, or more than 150 KB), ns_consume first SELECTS those K + 1 from the keys in global memory
// (radix select on the order-preserving integer image of the key, ties at the threshold by lowest slot), compacts
// them in slot order -- so that "lowest slot first" among equal values is "lowest compact index first" -- and
// runs the same consumption on that subset; the slots of the death list and of the replacements are translated back
// when they are stored.  Same deaths, same replacements, same evidence as the full arrays would give
// (tests/test_gpu_ns_consume.py holds the two paths to each other and to the oracle).
// (round 6) ... and where the register sort of all slots costs more than the selection: at C3 (nlive 5 000, K = 1 024)
// the sort of 8 192 padded slots was 144 k of the kernel's 230 k cycles per fill; selected first, 1 025 of them are
// sorted.  Taken from nlive > 4 096 (the sort's 16 and 32 elements per lane) when the queue is a quarter of the live
// set or less.
__host__ __device__ inline bool ns_consume_compact(int N, int K) {
  return K + 1 < N && (N > 32 * kT || ns_consume_lds_full(N, K) > (size_t)150 * 1024 || (N > 4096 && 4 * (K + 1) <= N + 4));
}
__host__ __device__ inline bool ns_finish_big(int N) {  // ns_finish: keys by slot, keys in order, sorted slots in LDS?
  size_t P = 1;
  while (P < (size_t)N) P <<= 1;
  return N > 32 * kT || (size_t)N * 16 + (P > 256 ? P : 256) * 2 + 64 > (size_t)150 * 1024;
}
__host__ __device__ inline size_t ns_fin_stride(int N) {  // doubles of ns_finish's workspace per run
  size_t P = 1;
  while (P < (size_t)N) P <<= 1;
  return 3 * (size_t)N + (ns_finish_big(N) ? P : 0);
}
__host__ __device__ inline size_t ns_select_scratch(int N) {  // histogram, two lane masks per 64 slots, their prefixes
  const size_t nm = ((size_t)N + 63) / 64;
  return 256 * 4 + nm * 16 + nm * 8 + 64;
}
__host__ __device__ inline size_t ns_consume_lds(int N, int K) {
  if (!ns_consume_compact(N, K)) return ns_consume_lds_full(N, K);
  const size_t NC = (size_t)K + 1;
  size_t P = 1;
  while (P < NC) P <<= 1;
  if (P < 256) P = 256;
  size_t q = (size_t)K * 52, sc = ns_select_scratch(N);
  if (q < sc) q = sc;  // (the selection's scratch lies where the queue's arrays come afterwards)
  q = (q + 15) & ~(size_t)15;
  return NC * 12 + q + P * 2 + NC * 2 + 64 + 16;
}

// The serial part of the queue consumption (sampler.py:741-776), run by wave 0: stale test, death record,
// replacement.  The live points are NOT kept in a priority queue: the run's slots are sorted once per fill by
// (log-likelihood, slot) -- `sidx` -- and the worst live point is then either the next unconsumed entry of that order
// or the smallest of the replacements made during this fill.  Of those only the ones that stand before the original at
// sorted position K (value theta; by value, then by slot: a replacement that equals theta in a lower slot does) can
// ever become the worst point within K deaths (K + 1 originals stand before any other), so they are
// the only ones kept, unsorted, in a buffer B whose minimum is re-scanned by the wave when it is consumed.  A step is
// a few LDS words instead of two sift levels of a 64-ary heap (1 950 cycles).  Ties die lowest slot first, as the
// reference's np.argmin picks them (sampler.py:1107).  Returns the number of deaths (wave-uniform); *newmin = the
// worst live log-likelihood after the walk.
struct WorstKey {
  double key;
  int slot;
};
__device__ __forceinline__ bool key_before(double ka, int sa, double kb, int sb) { return ka < kb || (ka == kb && sa < sb); }

__device__ __forceinline__ int consume_sorted(const double* skey, const unsigned short* sidx, int* src, const double* ql,
                                              double* dcur, int* dj, int* dslot, int* dsrc, double* bkey, int* bslot,
                                              int* bsrc, int N, int K, long long room, int limit, int* jcap,
                                              double* newmin, int lane) {
  int ndead = 0, ptr = 0, nb = 0, bpos = -1;
  *jcap = -1;
  // (theta with its slot: a replacement that EQUALS theta in a lower slot stands before that original too)
  const double theta = K < N ? skey[sidx[K]] : INFINITY;
  const int theta_slot = K < N ? (int)sidx[K] : 0x7fffffff;
  // The queue and the sorted order are walked through registers: every lane holds one of the next 64 entries, the
  // current one comes by readlane (the index is wave-uniform) -- no LDS round trip on the serial chain.
  auto lane_d = [](double v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)__double_as_longlong(v), l);
    const int hi = __builtin_amdgcn_readlane((int)(unsigned)(__double_as_longlong(v) >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  };
  int pb = 0;  // sorted positions pb .. pb + 63 are in the lanes
  int my_slot = pb + lane < N ? (int)sidx[pb + lane] : 0x7fffffff;
  double my_key = pb + lane < N ? skey[my_slot] : INFINITY;
  int sslot = __builtin_amdgcn_readlane(my_slot, 0);
  double skeyp = lane_d(my_key, 0), bmin = INFINITY;
  int bminslot = 0x7fffffff;
  double my_q = 0.0;
  for (int j = 0; j < K; ++j) {
    if ((j & 63) == 0) my_q = j + lane < K ? ql[j + lane] : 0.0;
    const bool from_b = nb > 0 && key_before(bmin, bminslot, skeyp, sslot);
    const double worst = from_b ? bmin : skeyp;
    const double lj = lane_d(my_q, j & 63);
    if (!(lj > worst)) continue;  // stale proposal (sampler.py:774-776)
    if (ndead >= room) {          // dead-point store exhausted
      *jcap = j;
      break;
    }
    int s, from;
    if (from_b) {
      s = bminslot;
      from = bsrc[bpos];
      // remove B[bpos] (the last entry takes its place) and find the new minimum with the whole wave
      --nb;
      wave_lds_fence();
      if (lane == 0 && bpos != nb) {
        bkey[bpos] = bkey[nb];
        bslot[bpos] = bslot[nb];
        bsrc[bpos] = bsrc[nb];
      }
      wave_lds_fence();
      double mk = INFINITY;
      int ms = 0x7fffffff, mp = -1;
      for (int q = lane; q < nb; q += 64) {
        const double kq = bkey[q];
        const int sq = bslot[q];
        if (key_before(kq, sq, mk, ms)) {
          mk = kq;
          ms = sq;
          mp = q;
        }
      }
      double kmin;
      (void)wave_argmin(mk, &kmin);
      // among the lanes holding kmin the lowest slot wins
      const unsigned cand = (nb > 0 && mk == kmin) ? (unsigned)ms : 0xFFFFFFFFu;
      const unsigned smin = wave_min_u32(cand);
      const unsigned long long win = __ballot(cand == smin && mp >= 0);
      const int wl = win ? __ffsll((long long)win) - 1 : 0;
      bpos = __builtin_amdgcn_readlane(mp, wl);
      bmin = nb > 0 ? kmin : INFINITY;
      bminslot = nb > 0 ? (int)smin : 0x7fffffff;
    } else {
      s = sslot;
      from = -1;
      ++ptr;
      if (ptr - pb == 64) {  // next 64 positions of the sorted order
        pb = ptr;
        my_slot = pb + lane < N ? (int)sidx[pb + lane] : 0x7fffffff;
        my_key = pb + lane < N ? skey[my_slot] : INFINITY;
      }
      sslot = __builtin_amdgcn_readlane(my_slot, ptr - pb);
      skeyp = lane_d(my_key, ptr - pb);
    }
    if (lane == 0) {
      dcur[ndead] = worst;
      dj[ndead] = j;
      dslot[ndead] = s;
      dsrc[ndead] = from;
      src[s] = j;
      if (key_before(lj, s, theta, theta_slot)) {  // may become the worst point again within this fill
        bkey[nb] = lj;
        bslot[nb] = s;
        bsrc[nb] = j;
      }
    }
    if (key_before(lj, s, theta, theta_slot)) {
      if (nb == 0 || key_before(lj, s, bmin, bminslot)) {
        bmin = lj;
        bminslot = s;
        bpos = nb;
      }
      ++nb;
    }
    ++ndead;
    if (ndead == limit) break;
  }
  wave_lds_fence();
  *newmin = (nb > 0 && key_before(bmin, bminslot, skeyp, sslot)) ? bmin : skeyp;
  return ndead;
}

// (sort_slots: ns_sort.h)
using dh_sort::key_before_nb;
using dh_sort::sort_slots;

// The same walk without the serial chain, by the whole workgroup.  Let U_j = the run's live values at the start of
// the fill plus the proposals accepted before entry j, dead or alive; c_j = the deaths before j.  Entry j is
// accepted iff q_j beats the worst live value, i.e. iff more than c_j values of U_j are below q_j:
//     R_j = #{originals < q_j} + #{accepted i < j : q_i < q_j} > c_j .
// The worst value never decreases, so a stale entry i < j (q_i <= the worst at its time) lies below every LATER
// accepted q_j: for an accepted j all j - c_j stale entries before it count into #{i < j : q_i < q_j}, and for a
// stale j at most that many do.  Hence
//     entry j is accepted  <=>  #{originals < q_j} + #{i < j : q_i < q_j}  >  j ,
// a rank that does not depend on what happened to the entries before it.  Proposals accepted after death e are
// strictly above its value, so death e is the e-th smallest of originals + all accepted proposals: a merge of the
// sorted originals with the (few) accepted values low enough to die within this fill; a proposal inherits the slot
// of the death that let it in (chains of such inheritances are followed until none is open).  Equal values are
// ordered by slot in the reference (np.argmin, sampler.py:1107), and the slot of a proposal is only known after the
// deaths below it: whenever an accepted value that could die in this fill equals an original or another such value
// (rwalk handing back its start point), and when the dead-point store runs out, this routine changes nothing and
// returns 0 -- the serial walk takes the fill.  All threads call it; cj = K ints of scratch (c_j of every entry);
// sh = 4 shared ints; on success *ndead_out / *newmin as consume_sorted.
template <int kEPT>
__device__ int consume_parallel(const double* skey, const unsigned short* sidx, int* src, const double* ql, double* dcur,
                                int* dj, int* dslot, int* dsrc, double* bkey, int* bqs, int* cj, int N, int K,
                                long long room, int* sh, int* ndead_out, double* newmin, long long* prof) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  long long pt_ = prof ? clock64() : 0;
#define CP_PROF(i)                         \
  do {                                     \
    if (prof && t == 0) {                  \
      const long long now_ = clock64();    \
      prof[i] += now_ - pt_;               \
      pt_ = now_;                          \
    }                                      \
  } while (0)
  __shared__ int wcnt[kEPT][kT / 64];
  int* rA = dsrc;                  // #{originals < q_j}   (dsrc is written last)
  int* posB = (int*)dcur;          // death index of the r-th lowest accepted value   (dcur likewise)
  int* bq = posB + K;              // its queue entry
  double qv[kEPT];
#pragma unroll
  for (int u = 0; u < kEPT; ++u) {
    const int j = t + u * kT;
    qv[u] = j < K ? ql[j] : -INFINITY;
    if (j < K) {
      int lo = 0, hi = N;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (skey[sidx[mid]] < qv[u]) lo = mid + 1; else hi = mid;
      }
      rA[j] = lo;
    }
  }
  CP_PROF(11);
  if (t == 0) sh[0] = sh[1] = sh[2] = sh[3] = 0;  // [0] low accepted values, [1] tie, [2] undecided entries, [3] give up
  __syncthreads();
  // #{i < j : q_i < q_j} is needed only where the originals alone do not decide (rA[j] <= j: a quarter of a late
  // fill): those entries are listed, and every one is counted by four lanes (a quarter of i < j each)
  const int nu = (K + kT - 1) / kT;
  int* needl = posB;  // (scratch until the merge)
  int* lcnt = bq;
  for (int u = 0; u < nu; ++u) {
    const int j = t + u * kT;
    const bool need = j < K && rA[j] <= j;
    const unsigned long long b = __ballot(need);
    if (j < K) cj[j] = 1;  // accepted unless found otherwise below
    if (b) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&sh[2], __popcll(b));
      base = __builtin_amdgcn_readfirstlane(base);
      if (need) {
        const int x = base + __popcll(b & ((1ull << lane) - 1ull));
        needl[x] = j;
        lcnt[x] = 0;
      }
    }
  }
  __syncthreads();
  const int nn = sh[2];
  for (int w = t; w < 4 * nn; w += kT) {
    const int x = w >> 2, part = w & 3, j = needl[x];
    const double q = ql[j];
    int c = 0, i = (j * part) >> 2;
    const int i1 = (j * (part + 1)) >> 2;
    for (; i + 8 <= i1; i += 8) {  // (eight loads in flight: the loop is LDS latency otherwise)
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = ql[i + k];
#pragma unroll
      for (int k = 0; k < 8; ++k) c += v[k] < q ? 1 : 0;
    }
    for (; i < i1; ++i) c += ql[i] < q ? 1 : 0;
    if (c) atomicAdd(&lcnt[x], c);
  }
  __syncthreads();
  for (int x = t; x < nn; x += kT) {
    const int j = needl[x];
    cj[j] = rA[j] + lcnt[x] > j ? 1 : 0;
  }
  __syncthreads();
  CP_PROF(12);
  bool acc[kEPT];
  int pre[kEPT];
#pragma unroll
  for (int u = 0; u < kEPT; ++u) {
    const int j = t + u * kT;
    acc[u] = u < nu && j < K && cj[j] != 0;
    pre[u] = 0;
    if (u < nu) {
      const unsigned long long b = __ballot(acc[u]);
      pre[u] = __popcll(b & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[u][wv] = __popcll(b);
    }
  }
  __syncthreads();
  int ndead = 0;
  {
    int run_sum = 0;
    for (int uu = 0; uu < nu; ++uu)
      for (int w = 0; w < kT / 64; ++w) {
        const int c = wcnt[uu][w];
#pragma unroll
        for (int u = 0; u < kEPT; ++u)
          if (uu == u && w == wv) pre[u] += run_sum;
        run_sum += c;
      }
    ndead = run_sum;
  }
  if ((long long)ndead > room) return 0;  // (uniform)
#pragma unroll
  for (int u = 0; u < kEPT; ++u) {
    const int j = t + u * kT;
    if (u < nu) {
      const bool low = acc[u] && rA[j] <= ndead;  // may die within this fill (or be the worst point left)
      const unsigned long long b = __ballot(low);
      int base = 0;
      if (b) {
        if (lane == 0) base = atomicAdd(&sh[0], __popcll(b));
        base = __builtin_amdgcn_readfirstlane(base);
      }
      if (j < K) {
        cj[j] = pre[u];
        if (acc[u]) dj[pre[u]] = j;
        if (low) {
          const int x = base + __popcll(b & ((1ull << lane) - 1ull));
          bkey[x] = qv[u];
          bq[x] = j;
          if (rA[j] < N && skey[sidx[rA[j]]] == qv[u]) sh[1] = 1;  // ties with an original: slot order decides (below)
        }
      }
    }
  }
  __syncthreads();
  const int nB = sh[0];
  CP_PROF(13);
  // rank among the low accepted values (counted: there are few)
  int myr[kEPT], myq[kEPT];
  for (int u = 0; u < kEPT; ++u) {
    const int x = t + u * kT;
    myr[u] = -1;
    if (x < nB) {
      const double v = bkey[x];
      int r = 0, eq = 0;
      for (int y = 0; y < nB; ++y) {
        const double w = bkey[y];
        r += (w < v || (w == v && y < x)) ? 1 : 0;  // equal values: a provisional order, settled by slot below
        eq += w == v ? 1 : 0;
      }
      if (eq > 1) sh[1] = 1;
      if (eq > 8) sh[3] = 1;  // (a plateau of proposals: left to the serial walk)
      myr[u] = r;
      myq[u] = bq[x];
    }
  }
  __syncthreads();
  if (sh[3]) return 0;
  const bool tied = sh[1] != 0;  // an accepted value that could die now equals an original or another such value
  for (int u = 0; u < kEPT; ++u)
    if (myr[u] >= 0) {
      posB[myr[u]] = rA[myq[u]] + myr[u];
      bq[myr[u]] = myq[u];  // (ranks are a permutation; every old bq entry sits in a register by now)
      bqs[myr[u]] = myq[u];  // ... and once more where the death list will not overwrite it
    }
  __syncthreads();
  CP_PROF(14);
  // death e = the element of rank e in the merge; e == ndead: the worst point left
  double dval[kEPT + 1];
  int dsl[kEPT + 1], dsr[kEPT + 1];
  for (int u = 0; u <= kEPT; ++u) {
    const int e = u < kEPT ? t + u * kT : (t == 0 ? ndead : ndead + 1);  // (thread 0: also the worst point left)
    dsl[u] = dsr[u] = -1;
    dval[u] = INFINITY;
    if (e <= ndead) {
      int lo = 0, hi = nB;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (posB[mid] < e) lo = mid + 1; else hi = mid;
      }
      if (lo < nB && posB[lo] == e) {
        dsr[u] = bq[lo];
        dval[u] = ql[dsr[u]];
      } else if (e - lo < N) {
        dsl[u] = sidx[e - lo];
        dval[u] = skey[dsl[u]];
      }
    }
  }
  __syncthreads();
  for (int u = 0; u < kEPT; ++u) {
    const int e = t + u * kT;
    if (e < ndead) {
      dcur[e] = dval[u];
      dsrc[e] = dsr[u];
      dslot[e] = dsl[u];
    }
  }
  if (t == 0) {
    *newmin = dval[kEPT];
    *ndead_out = ndead;
  }
  __syncthreads();
  CP_PROF(15);
  // Equal values die lowest slot first (np.argmin, sampler.py:1107), and a proposal's slot is that of the death that
  // let it in -- a death of a strictly lower value.  The merge above put equal values in a provisional order; the
  // positions of a group of equal values that holds a proposal are marked (-2) and settled -- group by group, from the
  // lowest value up, as their members' slots become known -- by selecting the (e - group start)-th smallest slot of
  // the group: its originals (already in slot order) and its proposals (at most 8).
  auto val_of = [&](int r) { return ql[bqs[r]]; };
  if (tied) {
    for (int e = t; e < ndead; e += kT) {
      const double v = dcur[e];
      int lo = 0, hi = nB;  // proposals of value v: [rl, rh)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (val_of(mid) < v) lo = mid + 1; else hi = mid;
      }
      const int rl = lo;
      hi = nB;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (val_of(mid) <= v) lo = mid + 1; else hi = mid;
      }
      const int rh = lo;
      if (rh > rl) {
        const bool orig_too = dsrc[e] < 0 || (e + 1 < ndead && dcur[e + 1] == v && dsrc[e + 1] < 0) ||
                              (e > 0 && dcur[e - 1] == v && dsrc[e - 1] < 0);
        // (an original of the same value sits, in the provisional order, right behind the group's proposals; one
        // that is not among the deaths still counts: test the sorted originals)
        int pl = 0, ph = N;
        while (pl < ph) {
          const int mid = (pl + ph) >> 1;
          if (skey[sidx[mid]] < v) pl = mid + 1; else ph = mid;
        }
        const bool has_orig = orig_too || (pl < N && skey[sidx[pl]] == v);
        if (rh - rl > 1 || has_orig) dslot[e] = -2;
      }
    }
    __syncthreads();
  }
  for (;;) {
    int open = 0;
    for (int e = t; e < ndead; e += kT) {
      const int s0 = ((volatile int*)dslot)[e];
      if (s0 == -1) {  // a proposal alone at its value: the slot of the death that let it in
        const int sl = ((volatile int*)dslot)[cj[dsrc[e]]];
        if (sl >= 0)
          ((volatile int*)dslot)[e] = sl;
        else
          open = 1;
      } else if (s0 == -2) {
        const double v = dcur[e];
        int lo = 0, hi = nB;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (val_of(mid) < v) lo = mid + 1; else hi = mid;
        }
        const int rl = lo;
        hi = nB;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (val_of(mid) <= v) lo = mid + 1; else hi = mid;
        }
        const int rh = lo, gi = rh - rl;
        int pl = 0, ph = N;
        while (pl < ph) {
          const int mid = (pl + ph) >> 1;
          if (skey[sidx[mid]] < v) pl = mid + 1; else ph = mid;
        }
        int pu = pl, pe = N;
        while (pu < pe) {
          const int mid = (pu + pe) >> 1;
          if (skey[sidx[mid]] <= v) pu = mid + 1; else pe = mid;
        }
        // the proposals' slots (all must be known)
        int sr[8];
        bool known = true;
        for (int q = 0; q < 8; ++q) {
          sr[q] = 0x7fffffff;
          if (q < gi) {
            sr[q] = ((volatile int*)dslot)[cj[bqs[rl + q]]];
            known = known && sr[q] >= 0;
          }
        }
        if (!known) {
          open = 1;
        } else {
          const int m = e - (pl + rl);  // rank inside the group
          int chosen = -1, below = 0;
          for (int q = 0; q < 8; ++q)
            if (q < gi) {
              int rk = 0;
              {  // originals of the group with a smaller slot (they are in slot order)
                int a0 = pl, a1 = pu;
                while (a0 < a1) {
                  const int mid = (a0 + a1) >> 1;
                  if ((int)sidx[mid] < sr[q]) a0 = mid + 1; else a1 = mid;
                }
                rk = a0 - pl;
              }
              for (int q2 = 0; q2 < 8; ++q2) rk += (q2 < gi && sr[q2] < sr[q]) ? 1 : 0;
              if (rk == m) chosen = q;
              below += rk < m ? 1 : 0;
            }
          if (chosen >= 0) {
            dsrc[e] = bqs[rl + chosen];
            ((volatile int*)dslot)[e] = sr[chosen];
          } else {
            dsrc[e] = -1;
            ((volatile int*)dslot)[e] = (int)sidx[pl + m - below];
          }
        }
      }
    }
    if (!__syncthreads_or(open)) break;
  }
  for (int j = t; j < K; j += kT)
    if (cj[j] < ndead && dj[cj[j]] == j) atomicMax(&src[dslot[cj[j]]], j);
  __syncthreads();
  CP_PROF(7);
  return 1;
}

// Kept ensembles: a stop rule ended the run inside this fill.  What the fill found is put aside before ns_consume
// changes it -- the run's state and what the slots the fill replaces (src[s] >= 0; compact slots translated by cslot)
// hold now -- so that a continuation can take the fill again from its beginning (ns_resume).  All threads call it.
// (the arrays one by one: a reference to NsArgs would put the whole argument block on the caller's stack)
__device__ __attribute__((noinline)) void ns_save_fill(NsRun* sv_st, const NsRun* st, int* sv_slot, double* sv_logl,
                                                       int* sv_it, const int* live_it, double* sv_u, double* sv_v,
                                                       const double* live_u, const double* live_v, int* sv_n, int N,
                                                       int D, int K, int run, const int* src, const double* skey,
                                                       const unsigned short* cslot, int NC, int* list, int* count) {
  const int t = threadIdx.x;
  if (t == 0) {
    sv_st[run] = st[run];
    *count = 0;
  }
  __syncthreads();
  for (int s = t; s < NC; s += kT)
    if (src[s] >= 0) {
      const int c = atomicAdd(count, 1), rs = cslot ? (int)cslot[s] : s;  // at most K slots change
      const size_t o = (size_t)run * K + c;
      list[c] = rs;
      sv_slot[o] = rs;
      sv_logl[o] = skey[s];
      sv_it[o] = live_it ? live_it[(size_t)run * N + rs] : 0;
    }
  __syncthreads();
  const int nsv = *count;
  for (int x = t; x < nsv * D; x += kT) {
    const int c = x / D, j = x - c * D;
    const size_t from = ((size_t)run * N + list[c]) * D + j, to = ((size_t)run * K + c) * D + j;
    sv_u[to] = live_u[from];
    sv_v[to] = live_v[from];
  }
  if (t == 0) sv_n[run] = nsv;
  __syncthreads();
}

template <int kEPT>
__global__ void __launch_bounds__(kT) ns_consume(NsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int run = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int N = a.nlive, D = a.ndim, K = a.K;
  NsRun& r = a.st[run];
  const int mode = r.mode;
  if (mode != MODE_CUBE && mode != MODE_BOUND) return;
  if (a.replay) {
    if (r.qstop != -1) return;  // (dh_ns_continue: only the runs whose last fill ns_resume has put back)
  } else {
    if (a.run_mode && a.run_mode[run] == MODE_WAIT) return;
    if (mode == MODE_BOUND && a.bstatus[run] != DH_OK) return;
  }
  long long pt_ = a.prof ? clock64() : 0;
  // NC = the slots the consumption works on: all of them, or the K + 1 smallest in slot order (ns_consume_compact)
  const bool compact = ns_consume_compact(N, K);
  const int NC = compact ? K + 1 : N;
  int P = 1;
  while (P < NC) P <<= 1;
  size_t qbytes = (size_t)K * 52;
  if (compact) {
    const size_t sc = ns_select_scratch(N);
    if (qbytes < sc) qbytes = sc;
    qbytes = (qbytes + 15) & ~(size_t)15;
  }
  double* skey = (double*)smem;     // NC  live log-likelihoods by (compact) slot
  double* ql = skey + NC;           // K   proposal logl
  double* dcur = ql + K;            // K   death list: logl of the dead point
  double* bkey = dcur + K;          // K   low replacements of this fill (see consume_sorted)
  int* qc = (int*)(bkey + K);       // K   calls
  int* dj = qc + K;                 // K   death list: queue index of the replacement
  int* dslot = dj + K;              // K               slot
  int* dsrc = dslot + K;            // K               content source at death
  int* qborn = dsrc + K;            // K   (per-point bookkeeping only) death index at which entry j went live
  int* bslot = qborn + K;           // K
  int* bsrc = bslot + K;            // K
  int* src = (int*)((unsigned char*)ql + qbytes);      // NC  queue index now living in the slot, -1 = original
  unsigned short* sidx = (unsigned short*)(src + NC);  // P   slots in ascending (logl, slot) order; 0xFFFF = padding
  unsigned short* cslot = sidx + (P > kT ? P : kT);    // NC  (compact) the live slot behind a compact index
  __shared__ int misc[8];
  __shared__ double wred[2][4];
  __shared__ double bcast[4];
  __shared__ long long lred[4];
  __shared__ int sel_i[4];
  __shared__ unsigned long long sel_u[2];
  double sel_v = INFINITY;  // compact: the threshold value (the (K + 1)-th smallest key) ...
  int sel_extra = 0;        // ... and how many live points OUTSIDE the subset carry it
  if (!compact) {
    // (round 6: eight keys of a thread in flight -- one load, one LDS store at a time the 2 000 keys of a C2 run were
    // eight cold round trips in a row, 11 k cycles of every fill)
    const double* keys = a.live_logl + (size_t)run * N;
    for (int i0 = t; i0 < N; i0 += 8 * kT) {
      double kv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) kv[q] = keys[i0 + q * kT < N ? i0 + q * kT : 0];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (i0 + q * kT < N) {
          skey[i0 + q * kT] = kv[q];
          src[i0 + q * kT] = -1;
        }
    }
  } else {
    const double* keys = a.live_logl + (size_t)run * N;
    int* hist = (int*)ql;                                            // 256
    const int nm = (N + 63) >> 6;
    unsigned long long* lmask = (unsigned long long*)(hist + 256);   // nm: lanes below the threshold
    unsigned long long* tmask = lmask + nm;                          // nm: lanes at the threshold
    int* pless = (int*)(tmask + nm);                                 // nm: exclusive prefixes of the two counts
    int* ptie = pless + nm;
    // the order-preserving image of a key (-0 folded into +0, as the double comparison has it)
    auto ord = [](double x) -> unsigned long long {
      const unsigned long long b = (unsigned long long)__double_as_longlong(x + 0.0);
      return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    };
    unsigned long long prefix = 0, mask = 0;
    int want = K + 1;  // rank (1-based) of the threshold among the keys that share the prefix
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[t] = 0;
      __syncthreads();
      // (eight independent loads in flight per thread: one at a time a pass is N / kT global round trips)
      for (int i0 = t; i0 < N; i0 += 8 * kT) {
        double kv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) kv[q] = i0 + q * kT < N ? keys[i0 + q * kT] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned long long o = ord(kv[q]);
          if (i0 + q * kT < N && (o & mask) == prefix) atomicAdd(&hist[(int)((o >> shift) & 255ull)], 1);
        }
      }
      __syncthreads();
      if (wv == 0) {
        // first digit whose cumulative count reaches `want`: a wave scan over four bins per lane (one thread walking
        // the 256 bins was 256 dependent LDS reads per pass)
        const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int sum4 = h0 + h1 + h2 + h3;
        int incl = sum4;
        for (int off = 1; off < 64; off <<= 1) {
          const int y = __shfl_up(incl, off);
          if (lane >= off) incl += y;
        }
        const unsigned long long reach = __ballot(incl >= want);
        const int hitl = reach ? (int)__ffsll((long long)reach) - 1 : 63;
        if (lane == hitl) {
          int cum = incl - sum4, d = 4 * lane;
          const int hh[4] = {h0, h1, h2, h3};
          int q = 0;
          while (q < 3 && cum + hh[q] < want) cum += hh[q++];
          d += q;
          sel_i[0] = d;
          sel_i[1] = want - cum;
          sel_i[2] = hh[q];
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)sel_i[0] << shift;
      mask |= 255ull << shift;
      want = sel_i[1];
      __syncthreads();
    }
    // `want` of the keys equal to the threshold belong to the subset: the lowest slots
    const int need = want, eq_total = sel_i[2];
    sel_extra = eq_total - need;
    for (int m0 = wv; m0 < nm; m0 += 4 * (kT / 64)) {
      double kv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = (m0 + q * (kT / 64)) * 64 + lane;
        kv[q] = i < N ? keys[i] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mi = m0 + q * (kT / 64), i = mi * 64 + lane;
        const unsigned long long o = ord(kv[q]);
        const unsigned long long lm = __ballot(i < N && o < prefix), tm = __ballot(i < N && o == prefix);
        if (lane == 0 && mi < nm) {
          lmask[mi] = lm;
          tmask[mi] = tm;
        }
      }
    }
    __syncthreads();
    if (wv == 0) {  // exclusive prefixes of the per-mask counts, one wavefront
      int bl = 0, bt = 0;
      for (int m0 = 0; m0 < nm; m0 += 64) {
        const int mi = m0 + lane;
        const int cl = mi < nm ? __popcll(lmask[mi]) : 0, ct = mi < nm ? __popcll(tmask[mi]) : 0;
        int sl = cl, st = ct;
        for (int off = 1; off < 64; off <<= 1) {
          const int yl = __shfl_up(sl, off), yt = __shfl_up(st, off);
          if (lane >= off) {
            sl += yl;
            st += yt;
          }
        }
        if (mi < nm) {
          pless[mi] = bl + sl - cl;
          ptie[mi] = bt + st - ct;
        }
        bl += __shfl(sl, 63);
        bt += __shfl(st, 63);
      }
    }
    __syncthreads();
    for (int mi = wv; mi < nm; mi += kT / 64) {
      const int i = mi * 64 + lane;
      const unsigned long long lm = lmask[mi], tm = tmask[mi], below = (1ull << lane) - 1ull;
      const int tb = ptie[mi] + __popcll(tm & below);
      const bool take = ((lm >> lane) & 1ull) || (((tm >> lane) & 1ull) && tb < need);
      if (take) {
        const int pos = pless[mi] + __popcll(lm & below) + (tb < need ? tb : need);
        skey[pos] = keys[i];
        cslot[pos] = (unsigned short)i;
        src[pos] = -1;
      }
      if (((tm >> lane) & 1ull) && tb == 0) sel_u[0] = (unsigned long long)__double_as_longlong(keys[i]);
    }
    __syncthreads();
    sel_v = __longlong_as_double((long long)sel_u[0]);
    __syncthreads();  // (the scratch is the queue's from here on)
  }
  auto real_slot = [&](int sl) -> int { return compact ? (int)cslot[sl] : sl; };
  __syncthreads();
  NS_PROF(16);
  if (a.presorted && !compact) {
    const int nsidx = P > kT ? P : kT;
    const unsigned short* pre = a.presort + (size_t)run * a.presort_stride;
    for (int i0 = t; i0 < nsidx; i0 += 8 * kT) {
      unsigned short sv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) sv[q] = pre[i0 + q * kT < nsidx ? i0 + q * kT : 0];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (i0 + q * kT < nsidx) sidx[i0 + q * kT] = sv[q];
    }
    __syncthreads();
  } else {
    const int nsidx = P > kT ? P : kT;
    switch (nsidx / kT) {
      case 1: sort_slots<1>(skey, sidx, NC, nsidx); break;
      case 2: sort_slots<2>(skey, sidx, NC, nsidx); break;
      case 4: sort_slots<4>(skey, sidx, NC, nsidx); break;
      case 8: sort_slots<8>(skey, sidx, NC, nsidx); break;
      case 16: sort_slots<16>(skey, sidx, NC, nsidx); break;
      default: sort_slots<32>(skey, sidx, NC, nsidx); break;
    }
  }
  NS_PROF(17);
  int acc = 0, rej = 0;
  for (int j = t; j < K; j += kT) {
    const size_t q = (size_t)run * K + j;
    ql[j] = a.r_logl[q];
    if (mode == MODE_CUBE) {
      qc[j] = a.r_a[q];
    } else if (a.sampler == 3) {
      qc[j] = a.r_a[q];
      if (a.r_b[q] & 3) ql[j] = -INFINITY;  // no ellipsoid held the draw / the try limit: never accepted, the run fails below
      if (a.r_b[q] & 3) atomicOr(&r.sampler_failed, 1);
    } else if (a.sampler == 0) {
      qc[j] = a.walks;
      acc += a.r_a[q];
      rej += a.r_b[q];
      // No step accepted: the walker hands back its start point, a LIVE point, and the reference's re-evaluation of it
      // (internal_samplers.py:970-975) gives that point's own ln L again, bit for bit -- an exact tie, which dies
      // lowest slot first and opens the plateau mode (sampler.py:1107-1119).  Two kernels evaluating the same point
      // can differ in the last bit (summation order), so the live point's stored value is taken.
      if (a.r_a[q] == 0) ql[j] = a.live_logl[(size_t)run * N + a.r_d[q]];
    } else {
      qc[j] = a.r_a[q];
      acc += a.r_b[q];                      // n_expand
      rej += a.r_c[q];                      // n_contract
      if (a.r_d[q] & 1) atomicOr(&r.doubling, 1);  // expansion_warning_set -> slice_doubling
      if (a.r_d[q] & 2) ql[j] = -INFINITY;         // failed slice: never accepted
    }
  }
  // block sums of accept / reject for the scale tuning
  __shared__ int racc[kT], rrej[kT];
  racc[t] = acc;
  rrej[t] = rej;
  if (t == 0) misc[3] = 0x7fffffff;  // first stop index
  __syncthreads();
  for (int sft = kT / 2; sft > 0; sft >>= 1) {
    if (t < sft) {
      racc[t] += racc[t + sft];
      rrej[t] += rrej[t + sft];
    }
    __syncthreads();
  }
  const long long it0 = r.it, carry0 = r.nc_carry, ncall0 = r.ncall;
  const double logvol0 = r.logvol, logz0 = r.logz, h0 = r.h, lmax0 = r.lmax, dead_prev0 = r.dead_prev;
  const double dlv = log(((double)N + 1.0) / (double)N);
  const double ldv_c = log(0.5 * expm1(dlv));  // ln(dX_e / X_e) of the trapezoid rule
  NS_PROF(0);
  // ---- phase A: the walk over the queue (wave 0) ----
  const long long room = a.dead_rel ? (long long)K + 1 : a.cap - it0;
  int walked = 0;
  if (!a.serial_walk) {
    walked = consume_parallel<kEPT>(skey, sidx, src, ql, dcur, dj, dslot, dsrc, bkey, bslot, qborn, NC, K, room, &misc[4],
                              &misc[0], &bcast[2], run == 0 ? a.prof : nullptr);
    if (walked && t == 0) misc[1] = -1;
    if (a.prof && run == 0 && t == 0 && !walked) atomicAdd((unsigned long long*)&a.prof[10], 1ull);
  }
  if (!walked && t < 64) {
    int jcap;
    double nm;
    const int nd = consume_sorted(skey, sidx, src, ql, dcur, dj, dslot, dsrc, bkey, bslot, bsrc, NC, K, room, K + 1,
                                  &jcap, &nm, t);
    if (t == 0) {
      misc[0] = nd;
      misc[1] = jcap;
      bcast[2] = nm;
    }
  }
  __syncthreads();
  const int ndead = misc[0], jcap = misc[1];
  NS_PROF(1);
  // ---- likelihood plateaus (sampler.py:1112-1127, 1190-1193) ----
  // When the worst live point shares its log-likelihood with others -- rwalk hands back its start point when no
  // step was accepted: about one queue fill in seven of a C2 run meets such a pair -- the reference takes the
  // next `multiplicity` deaths with a constant VOLUME step X_s / (N + 1) instead of the constant ln X step.
  // Equal values die consecutively, so the plateaus of a fill are its runs of equal death values (and what an
  // earlier fill left open); the j-th death of a plateau shrinks ln X by ln((N + 2 - j) / (N + 1 - j)) whatever
  // X_s was.  Every death's own step is therefore known without walking the fill; a sum scan of the steps gives
  // ln X, and the scans below take both per death (has_tie) instead of the closed form of the constant step.
  __shared__ int pl_int[4];
  __shared__ double pl_dbl[2];
  __shared__ double sred[3][4];
  int has_tie = r.pcount > 0 ? 1 : 0;
  for (int e = t; e < ndead; e += kT)
    if ((e + 1 < ndead && dcur[e + 1] == dcur[e]) || (e + 1 == ndead && bcast[2] == dcur[e])) has_tie = 1;
  has_tie = __syncthreads_or(has_tie);
  if (a.prof && t == 0 && has_tie) atomicAdd((unsigned long long*)&a.prof[8 + (r.pcount > 0 ? 1 : 0)], 1ull);
  int ntail_tot = 0;
  if (has_tie) {
    // live points left after this fill's deaths that share the last death's value (a plateau that goes on)
    int ntail = 0;
    if (ndead > 0 && bcast[2] == dcur[ndead - 1]) {
      const double x = dcur[ndead - 1];
      for (int sl = t; sl < NC; sl += kT) ntail += (src[sl] >= 0 ? ql[src[sl]] : skey[sl]) == x ? 1 : 0;
      // (compact: no death value exceeds the threshold, and the points left out are not below it)
      if (t == 0 && x == sel_v) ntail += sel_extra;
    }
    if (t == 0) {
      pl_int[2] = 0;
      pl_int[3] = 0;
    }
    __syncthreads();
    if (ntail) atomicAdd(&pl_int[2], ntail);
    __syncthreads();
    ntail_tot = pl_int[2];
  }
  const int pc_in = r.pcount;                      // deaths an open plateau still has to take
  const int pc0 = pc_in < ndead ? pc_in : ndead;   // ... of which this fill holds the first pc0
  const double rho0 = pc_in > 0 ? exp(r.plogdvol - logvol0) : 0.0;
  // position j (1-based) of death e >= pc0 in its run of equal values and the run's multiplicity m at its start
  auto run_info = [&](int e, int& j, int& m) {
    const double x = dcur[e];
    int sst = e, fin = e;
    while (sst > pc0 && dcur[sst - 1] == x) --sst;
    while (fin + 1 < ndead && dcur[fin + 1] == x) ++fin;
    m = fin - sst + 1 + ((fin == ndead - 1 && bcast[2] == x) ? ntail_tot : 0);
    j = e - sst + 1;
  };
  auto step_of = [&](int e) -> double {  // -d ln X of death e
    if (e < pc0) return -log1p(-rho0 / (1.0 - (double)e * rho0));
    int j, m;
    run_info(e, j, m);
    return m > 1 ? -log1p(-1.0 / ((double)N + 2.0 - (double)j)) : dlv;
  };
  // sum over the workgroup's per-thread totals: returns this thread's exclusive prefix (threads own contiguous deaths)
  auto excl_sum = [&](double v, double* scratch4) -> double {
    double sc = v;
    for (int off = 1; off < 64; off <<= 1) {
      const double y = __shfl_up(sc, off);
      if (lane >= off) sc += y;
    }
    double ex = __shfl_up(sc, 1);
    if (lane == 0) ex = 0.0;
    __syncthreads();
    if (lane == 63) scratch4[wv] = sc;
    __syncthreads();
    double pre = 0.0;
    for (int w2 = 0; w2 < wv; ++w2) pre += scratch4[w2];
    return pre + ex;
  };
  NS_PROF(18);
  // ---- phase B: integration + stopping rule as prefix scans over the deaths ----
  const int EPT = (K + kT - 1) / kT;
  double lw[kEPT], nl[kEPT], cd[kEPT], lvv[kEPT];
  {
    double run_cd = 0.0;
#pragma unroll
    for (int i = 0; i < kEPT; ++i) {
      const int e = t * EPT + i;
      cd[i] = dlv;
      lvv[i] = logvol0 - (double)(e + 1) * dlv;
      if (has_tie && i < EPT && e < ndead) {
        cd[i] = step_of(e);
        run_cd += cd[i];
        lvv[i] = run_cd;
      }
    }
    if (has_tie) {
      const double ex = excl_sum(run_cd, sred[0]);
#pragma unroll
      for (int i = 0; i < kEPT; ++i) lvv[i] = logvol0 - (ex + lvv[i]);
    }
  }
  // ln Z after every death = ln(Z_0 + prefix sum of the weights): the weights are summed in the LINEAR domain, relative
  // to M = the largest of them and of ln Z_0 (one exp and one log per death; a logaddexp scan -- an exp and a log1p
  // for every element AND every scan step -- was the largest part of this phase: 41 k of its 67 k cycles at C2).  The
  // recurrence's rounding differs from the serial chain's in the last bits only (tested to 1e-10 absolute).
  double mloc = logz0;
#pragma unroll
  for (int i = 0; i < kEPT; ++i) {
    lw[i] = -INFINITY;
    nl[i] = -INFINITY;
    const int e = t * EPT + i;
    if (i < EPT && e < ndead) {
      const double lnew = dcur[e], lprev = e ? dcur[e - 1] : dead_prev0;
      const double logvol_e = lvv[i];
      lw[i] = logaddexp_dev(lnew, lprev) + logvol_e + (has_tie ? log(0.5 * expm1(cd[i])) : ldv_c);
      nl[i] = ql[dj[e]];
      mloc = fmax(mloc, lw[i]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) mloc = fmax(mloc, __shfl_xor(mloc, off));
  if (lane == 0) wred[0][wv] = mloc;
  __syncthreads();
  const double M = fmax(fmax(wred[0][0], wred[0][1]), fmax(wred[0][2], wred[0][3]));
  __syncthreads();
  double tz = 0.0, tm = -INFINITY;
#pragma unroll
  for (int i = 0; i < kEPT; ++i)
    if (i < EPT) {
      tz += lw[i] > -INFINITY ? exp(lw[i] - M) : 0.0;  // running (inclusive) values of this lane's segment
      tm = fmax(tm, nl[i]);
      lw[i] = tz;
      nl[i] = tm;
    }
  // inclusive scan of the lane totals across the wave, then across the 4 waves
  double sz = tz, sm = tm;
  for (int off = 1; off < 64; off <<= 1) {
    const double yz = __shfl_up(sz, off), ym = __shfl_up(sm, off);
    if (lane >= off) {
      sz += yz;
      sm = fmax(ym, sm);
    }
  }
  if (lane == 63) {
    wred[0][wv] = sz;
    wred[1][wv] = sm;
  }
  double ez = __shfl_up(sz, 1), em = __shfl_up(sm, 1);  // exclusive prefix inside the wave
  if (lane == 0) {
    ez = 0.0;
    em = -INFINITY;
  }
  __syncthreads();
  const double z0 = logz0 > -INFINITY ? exp(logz0 - M) : 0.0;
  double sbefore = z0, pm = lmax0;  // everything before this lane's segment
  for (int w2 = 0; w2 < wv; ++w2) {
    sbefore += wred[0][w2];
    pm = fmax(pm, wred[1][w2]);
  }
  sbefore += ez;
  pm = fmax(pm, em);
  const double pz = M + log(sbefore);  // ln Z before this lane's segment
  NS_PROF(19);
  int mystop = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < kEPT; ++i) {
    const int e = t * EPT + i;
    if (i < EPT && e < ndead) {
      lw[i] = M + log(sbefore + lw[i]);  // ln Z after death e
      nl[i] = fmax(pm, nl[i]);           // lmax after death e
      const double dz = logaddexp_dev(0.0, nl[i] + lvv[i] - lw[i]);
      // the reference tests at the top of the NEXT iteration, with the state this death leaves behind:
      // delta ln Z < dlogz, the last dead point above logl_max, its loop counter it = it0 + e + 1 > maxiter,
      // the calls spent so far > maxcall (sampler.py:1070-1093)
      bool stop = dz < a.dlogz || dcur[e] > a.logl_max || (a.maxiter >= 0 && it0 + e + 1 > a.maxiter);
      if (a.maxcall >= 0 && !stop) {  // (rarely asked for: a plain sum over the entries popped up to this death)
        long long cum = ncall0;
        for (int j = 0; j <= dj[e]; ++j) cum += qc[j];
        stop = cum > a.maxcall;
      }
      if (stop && e < mystop) mystop = e;
    }
  }
  if (mystop != 0x7fffffff) atomicMin(&misc[3], mystop);
  __syncthreads();
  const int estop = misc[3];
  const bool stopped = estop != 0x7fffffff;
  const int nkeep = stopped ? estop + 1 : ndead;
  const int E = nkeep - 1;
#pragma unroll
  for (int i = 0; i < kEPT; ++i)
    if (i < EPT && t * EPT + i == E) {
      bcast[0] = lw[i];
      bcast[1] = nl[i];
      bcast[3] = lvv[i];
      // the plateau mode after death E: what its plateau still has to take
      int pcn = 0;
      double plogn = 0.0;
      if (has_tie) {
        if (E < pc_in) {
          pcn = pc_in - nkeep;
          plogn = r.plogdvol;
        } else {
          int j, m;
          run_info(E, j, m);
          if (m > j) {
            pcn = m - j;
            // ln of the plateau's volume step: ln X at its start (ln X now minus the j steps taken) - ln(N + 1)
            plogn = lvv[i] - log1p(-(double)j / ((double)N + 1.0)) - log((double)N + 1.0);
          }
        }
      }
      pl_int[0] = pcn;
      pl_dbl[0] = plogn;
    }
  __syncthreads();
  const double logz_E = E >= 0 ? bcast[0] : logz0, lmax_E = E >= 0 ? bcast[1] : lmax0;
  NS_PROF(20);
  // information: sum of the L e^L dX terms relative to e^{lnZ_E}
  double hs = 0.0;
  double tt[kEPT];
  long long calls = 0;
  const int jlast = stopped ? dj[E] : (jcap >= 0 ? jcap : K - 1);
#pragma unroll
  for (int i = 0; i < kEPT; ++i) {
    const int e = t * EPT + i;
    tt[i] = 0.0;
    if (i < EPT && e <= E) {
      const double lnew = dcur[e], lprev = e ? dcur[e - 1] : dead_prev0;
      const double ldv = lvv[i] + (has_tie ? log(0.5 * expm1(cd[i])) : ldv_c);
      const double t0 = exp(lprev - logz_E + ldv), t1 = exp(lnew - logz_E + ldv);
      tt[i] = (t0 > 0.0 ? t0 * lprev : 0.0) + (t1 > 0.0 ? t1 * lnew : 0.0);
      hs += tt[i];
    }
  }
  // plateau deaths: their d ln X differs from the constant step, so their share of var[ln Z] = sum dH dlnX does not
  // telescope -- each needs its own dH = H_e - H_{e-1}, from the prefix sums of the terms above:
  //   H_e = e^{lnZ_E - lnZ_e} (w0 (H_0 + lnZ_0) + P_e) - lnZ_e,   P_e = sum_{k <= e} terms_k
  // -- and the two sums ns_finish needs for the same purpose (relative to Z_E): A += terms_e delta_e, B += (dZ_e / Z_E) delta_e
  double corr = 0.0, va_add = 0.0, vb_add = 0.0;
  if (has_tie) {
    const double ex = excl_sum(hs, sred[1]);
    const double w0 = exp(logz0 - logz_E);
    const double g0 = w0 > 0.0 ? w0 * (h0 + logz0) : 0.0;
    double pbefore = ex, lzbefore = pz;
    int under = 0;
#pragma unroll
    for (int i = 0; i < kEPT; ++i) {
      const int e = t * EPT + i;
      if (i < EPT && e <= E) {
        const double delta = cd[i] - dlv;
        if (delta != 0.0) {
          if (lw[i] < M - kNsUnder || (e > 0 && lzbefore < M - kNsUnder)) under = 1;
          const double hprev = e == 0 ? h0 : exp(logz_E - lzbefore) * (g0 + pbefore) - lzbefore;
          const double he = exp(logz_E - lw[i]) * (g0 + pbefore + tt[i]) - lw[i];
          corr += (he - hprev) * delta;
          va_add += tt[i] * delta;
          vb_add += (exp(lw[i] - logz_E) - exp(lzbefore - logz_E)) * delta;
        }
        pbefore += tt[i];
        lzbefore = lw[i];
      }
    }
    // A plateau far below the values the same fill goes on to (a penalty floor outside the likelihood's support, with
    // the first points of the support behind it): relative to M its deaths' weights are 0, ln Z_e = -inf and P_e = 0,
    // and H_e above is inf * 0 + inf.  ln Z_E and H_E do not feel it (those deaths' share of them is below rounding),
    // only the correction does: such a fill takes its var[ln Z] from the recurrence itself, death by death.
    if (__syncthreads_or(under)) {
      corr = 0.0;
      if (t == 0) {
        double sz = logz0, sh = h0, sv = 0.0, slv = logvol0, lprev = dead_prev0;
        int jrun = 0, mrun = 0;
        for (int e = 0; e <= E; ++e) {
          double st;
          if (e < pc0) {
            st = -log1p(-rho0 / (1.0 - (double)e * rho0));
          } else {
            if (e == pc0 || dcur[e] != dcur[e - 1]) {
              run_info(e, jrun, mrun);
            } else {
              ++jrun;
            }
            st = mrun > 1 ? -log1p(-1.0 / ((double)N + 2.0 - (double)jrun)) : dlv;
          }
          slv -= st;
          integrate_step(sz, sh, sv, lprev, dcur[e], slv, st);
          lprev = dcur[e];
        }
        pl_dbl[1] = sv;
        pl_int[3] = 1;
      }
    }
  }
  NS_PROF(21);
  for (int j = t; j <= jlast; j += kT) calls += qc[j];
  for (int off = 32; off > 0; off >>= 1) {
    hs += __shfl_xor(hs, off);
    calls += __shfl_xor(calls, off);
    corr += __shfl_xor(corr, off);
    va_add += __shfl_xor(va_add, off);
    vb_add += __shfl_xor(vb_add, off);
  }
  __syncthreads();  // (sred[1] / wred were read above)
  if (lane == 0) {
    wred[0][wv] = hs;
    lred[wv] = calls;
    sred[0][wv] = corr;
    sred[1][wv] = va_add;
    sred[2][wv] = vb_add;
  }
  NS_PROF(2);
  // ---- replay the walk up to the stop index (once per run): the sorted order is untouched ----
  if (nkeep < ndead) {
    __syncthreads();
    for (int i = t; i < NC; i += kT) src[i] = -1;
    __syncthreads();
    if (t < 64) {
      int jc;
      double nm;
      consume_sorted(skey, sidx, src, ql, dcur, dj, dslot, dsrc, bkey, bslot, bsrc, NC, K,
                     a.dead_rel ? (long long)K + 1 : a.cap - it0, nkeep, &jc, &nm, t);
      if (t == 0) bcast[2] = nm;
    }
  }
  __syncthreads();
  // (kept ensembles, once per run and call: behind a call of its own, so that the fills that do not stop carry
  // nothing of it in their registers)
  if (stopped && a.sv_st)
    ns_save_fill(a.sv_st, a.st, a.sv_slot, a.sv_logl, a.sv_it, a.live_it, a.sv_u, a.sv_v, a.live_u, a.live_v, a.sv_n, N, D, K,
                 run, src, skey, compact ? cslot : nullptr, NC, bslot, &misc[5]);
  if (t == 0) {
    const double hsum = wred[0][0] + wred[0][1] + wred[0][2] + wred[0][3];
    r.ncall += lred[0] + lred[1] + lred[2] + lred[3];
    if (nkeep > 0) {
      const double w = exp(logz0 - logz_E);
      const double h_E = hsum + (w > 0.0 ? w * (h0 + logz0) : 0.0) - logz_E;
      const double logzvar0 = r.logzvar;
      r.logzvar += (h_E - h0) * dlv;
      r.h = h_E;
      r.logz = logz_E;
      r.lmax = lmax_E;
      r.dead_prev = dcur[E];
      r.logvol = has_tie ? bcast[3] : logvol0 - (double)nkeep * dlv;
      r.it = it0 + nkeep;
      if (has_tie || r.var_a != 0.0 || r.var_b != 0.0) {
        // (the plateau sums are kept relative to the running Z)
        r.logzvar += sred[0][0] + sred[0][1] + sred[0][2] + sred[0][3];
        r.var_a = (w > 0.0 ? r.var_a * w : 0.0) + (sred[1][0] + sred[1][1] + sred[1][2] + sred[1][3]);
        r.var_b = (w > 0.0 ? r.var_b * w : 0.0) + (sred[2][0] + sred[2][1] + sred[2][2] + sred[2][3]);
      }
      if (has_tie && pl_int[3]) r.logzvar = logzvar0 + pl_dbl[1];  // (the recurrence's own sum, see kNsUnder)
      if (has_tie) {
        r.pcount = pl_int[0];
        r.plogdvol = pl_dbl[0];
      }
    }
    r.loglstar = bcast[2];
    r.nfill += a.replay ? 0 : 1;
    r.qstop = stopped ? dj[E] + 1 : 0;
    {
      // entries popped after the last kept death found no worse point to replace any more in this fill: the
      // reference goes on popping from the refilled queue within the same iteration, so their calls belong
      // to the next death's 'nc'
      long long c = nkeep > 0 ? 0 : carry0;
      for (int j = nkeep > 0 ? dj[E] + 1 : 0; j <= jlast; ++j) c += qc[j];
      r.nc_carry = c;
    }
    if (mode == MODE_BOUND && a.sampler != 3 && !a.replay) {  // (a fill taken again was tuned from when it stopped)
      const int ta = racc[0], tr = rrej[0];
      if (a.sampler == 0) {
        // RWalkSampler.tune (internal_samplers.py:460-493), once per queue fill
        if (ta + tr > 0) r.scale *= exp(((double)ta / (double)(ta + tr) - a.facc) / (double)D / a.facc);
      } else {
        // tune_slice (internal_samplers.py:1209-1239)
        const double ne = ta > 1 ? (double)ta : 1.0, nt = (double)tr;
        double mult = ne * 2.0 / (ne + nt);
        mult = fmin(fmax(mult, 0.5), 2.0);
        r.scale *= mult;
      }
    }
    int done = stopped ? 1 : ((jcap >= 0 || atomicOr(&r.sampler_failed, 0)) ? 2 : 0);
    // The plateau mode's companion stop (sampler.py:1095-1100: np.ptp(live_logl) == 0 -> "we have reached the plateau
    // in the likelihood", the run ends normally): lmax is the largest value ever inserted and the point that carries
    // it is alive until it is the worst, so the live set has no spread exactly when its worst value has reached
    // lmax.  No proposal can beat such a threshold: without this stop the run would idle to max_fills (and the
    // uniform samplers retry 2^32 times per walker).  (The reference tests before every death, here once per fill.)
    if (!done && bcast[2] >= r.lmax) done = 1;
    if (done) {
      r.mode = done == 1 ? MODE_DONE : MODE_FAILED;
      atomicAdd(a.ndone, 1);
    }
  }
  NS_PROF(3);
  // dead-point log-likelihoods, in death order
  const size_t dbase = a.dead_rel ? (size_t)run * K : (size_t)run * a.cap + it0;
  for (int e = t; e < nkeep; e += kT) a.dead_logl[dbase + e] = dcur[e];
  if (a.trace_slot)
    for (int e = t; e < nkeep; e += kT) {
      a.trace_slot[(size_t)run * K + e] = real_slot(dslot[e]);
      a.trace_src[(size_t)run * K + e] = dj[e];
    }
  if (a.trace_n && t == 0) {
    a.trace_n[run * 2] = nkeep;
    a.trace_n[run * 2 + 1] = stopped ? 1 : 0;
  }
  if (a.dead_id) {
    for (int e = t; e < nkeep; e += kT) qborn[dj[e]] = e;
    __syncthreads();
    for (int e = t; e < nkeep; e += kT) {
      long long nc = e ? 0 : carry0;
      for (int j = e ? dj[e - 1] + 1 : 0; j <= dj[e]; ++j) nc += qc[j];
      const int sj = dsrc[e];
      a.dead_nc[dbase + e] = (int)nc;
      a.dead_id[dbase + e] = real_slot(dslot[e]);
      // self.it starts at 1 (sampler.py:396): the replacement of death index i (0-based) is born at i + 1
      a.dead_it[dbase + e] = sj < 0 ? a.live_it[(size_t)run * N + real_slot(dslot[e])] : (int)(it0 + qborn[sj] + 1);
    }
    __syncthreads();
    for (int sl = t; sl < NC; sl += kT)
      if (src[sl] >= 0) a.live_it[(size_t)run * N + real_slot(sl)] = (int)(it0 + qborn[src[sl]] + 1);
  }
  // dead-point coordinates (optional), in death order
  if (a.store_samples) {
    double* to = a.dead_u + ((size_t)run * a.cap + it0) * D;
    for (int x = t; x < nkeep * D; x += kT) {
      const int e = x / D, j = x - e * D;
      const int s = real_slot(dslot[e]), sj = dsrc[e];
      to[x] = sj < 0 ? a.live_u[((size_t)run * N + s) * D + j] : a.r_u[((size_t)run * K + sj) * D + j];
    }
  }
  if (a.undo_slot) {
    const int E1 = nkeep - 1;
    if (nkeep > 0 && dj[E1] == K - 1) {
      const int s = real_slot(dslot[E1]), sj = dsrc[E1];
      for (int x = t; x < D; x += kT)
        a.undo_u[(size_t)run * D + x] = sj < 0 ? a.live_u[((size_t)run * N + s) * D + x] : a.r_u[((size_t)run * K + sj) * D + x];
      if (t == 0) a.undo_slot[run] = s;
    } else if (t == 0) {
      a.undo_slot[run] = -1;
    }
  }
  __syncthreads();
  NS_PROF(4);
  // apply the surviving replacements to the live set: the replaced slots are listed first (dslot / dj are free by
  // now), then their rows are copied element-parallel (one thread per slot copying 2 D strided doubles was 1 ms of
  // the 1.7 ms this kernel took per fill at D = 200)
  if (t == 0) misc[4] = 0;
  __syncthreads();
  for (int s = t; s < NC; s += kT) {
    const int sj = src[s];
    if (sj >= 0) {
      a.live_logl[(size_t)run * N + real_slot(s)] = ql[sj];
      const int c = atomicAdd(&misc[4], 1);  // at most K slots change
      dslot[c] = real_slot(s);
      dj[c] = sj;
    }
  }
  __syncthreads();
  {
    const int nrep = misc[4];
    double* lu = a.live_u + (size_t)run * N * D;
    double* lv = a.live_v + (size_t)run * N * D;
    const double* ru = a.r_u + (size_t)run * K * D;
    const double* rv = a.r_v + (size_t)run * K * D;
    // (sixteen elements per thread in flight -- one at a time the loop ran at one global round trip per element, with
    // eight it was still five dependent trips per C2 fill: 20 k of the kernel's 108 k cycles)
    const int tot = nrep * D;
    constexpr int LS = 16;
    for (int e0 = t; e0 < tot; e0 += LS * kT) {
      size_t to[LS];
      double xu[LS], xv[LS];
#pragma unroll
      for (int q = 0; q < LS; ++q) {
        const int e = e0 + q * kT;
        const int ec = e < tot ? e : 0;
        const int c = ec / D, j = ec - c * D;
        to[q] = (size_t)dslot[c] * D + j;
        const size_t from = (size_t)dj[c] * D + j;
        xu[q] = ru[from];
        xv[q] = rv[from];
      }
#pragma unroll
      for (int q = 0; q < LS; ++q)
        if (e0 + q * kT < tot) {
          lu[to[q]] = xu[q];
          lv[to[q]] = xv[q];
        }
    }
  }
  NS_PROF(5);
}

// ---- final live points (sampler.py:780-930) + record -----------------------------
// exclusive prefix of one value per thread over the workgroup (threads in order), and the total; OP = logaddexp or +
template <bool LOGADD>
__device__ __forceinline__ double block_excl_scan(double v, double ident, double* wtot /* 4 shared */, double* total) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double sc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const double y = __shfl_up(sc, off);
    if (lane >= off) sc = LOGADD ? logaddexp_dev(y, sc) : y + sc;
  }
  double ex = __shfl_up(sc, 1);
  if (lane == 0) ex = ident;
  __syncthreads();
  if (lane == 63) wtot[wv] = sc;
  __syncthreads();
  double pre = ident, tot = ident;
  for (int w2 = 0; w2 < kT / 64; ++w2) {
    if (w2 < wv) pre = LOGADD ? logaddexp_dev(pre, wtot[w2]) : pre + wtot[w2];
    tot = LOGADD ? logaddexp_dev(tot, wtot[w2]) : tot + wtot[w2];
  }
  *total = tot;
  return LOGADD ? logaddexp_dev(pre, ex) : pre + ex;
}

__global__ void __launch_bounds__(kT) ns_finish(NsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int run = blockIdx.x, t = threadIdx.x, N = a.nlive;
  if (!a.add_live) {
    // run_nested(add_live=False): the results are the loop's running integrals (progress_integration's values after
    // the last death), the live points stay out (sampler.py:1319-1341)
    if (t == 0) {
      const NsRun& r = a.st[run];
      double* rec = a.records + (size_t)run * 8;
      rec[0] = r.logz;
      rec[1] = sqrt(fabs(r.logzvar));
      rec[2] = (double)r.it;
      rec[3] = (double)r.ncall;
      rec[4] = r.h;
      rec[5] = (double)r.nbound;
      rec[6] = (double)(r.mode == MODE_DONE ? 0 : (r.mode == MODE_FAILED ? -1 : 1));
      rec[7] = 100.0 * (double)r.it / (double)r.ncall;
    }
    return;
  }
  // the final live log-likelihoods, ascending: the slots sorted by (value, slot) with the register network of
  // ns_consume, then the values in that order (the integration below does not care which slot a value came from).
  // Live sets beyond the sort's reach or the LDS (ns_finish_big): the values alone, by a bitonic network in global
  // memory behind the per-point terms (once per run; padded with +inf to a power of two).
  int P = 1;
  while (P < N) P <<= 1;
  const int nsidx = P > kT ? P : kT;
  double* sorted;
  if (ns_finish_big(N)) {
    sorted = a.fin_ws + (size_t)run * a.fin_stride + 3 * (size_t)N;
    for (int i = t; i < P; i += kT) sorted[i] = i < N ? a.live_logl[(size_t)run * N + i] + 0.0 : INFINITY;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
      for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
        for (int x = t; x < P / 2; x += kT) {
          const int lo = 2 * x - (x & (j2 - 1)), hi = lo + j2;  // the pair (lo, lo ^ j2) with lo's bit j2 clear
          const double va = sorted[lo], vb = sorted[hi];
          const bool up = (lo & k2) == 0;
          if ((va > vb) == up) {
            sorted[lo] = vb;
            sorted[hi] = va;
          }
        }
        __syncthreads();
      }
  } else {
    double* skey = (double*)smem;                                // N   by slot
    sorted = skey + N;                                           // N   ascending
    unsigned short* sidx = (unsigned short*)(sorted + N);        // max(P, kT)
    for (int i = t; i < N; i += kT) skey[i] = a.live_logl[(size_t)run * N + i];
    __syncthreads();
    switch (nsidx / kT) {
      case 1: sort_slots<1>(skey, sidx, N, nsidx); break;
      case 2: sort_slots<2>(skey, sidx, N, nsidx); break;
      case 4: sort_slots<4>(skey, sidx, N, nsidx); break;
      case 8: sort_slots<8>(skey, sidx, N, nsidx); break;
      case 16: sort_slots<16>(skey, sidx, N, nsidx); break;
      default: sort_slots<32>(skey, sidx, N, nsidx); break;
    }
    for (int i = t; i < N; i += kT) sorted[i] = skey[sidx[i]];
    __syncthreads();
  }
  // The final live points, lowest first (sampler.py:780-930).  What Results reports is
  // compute_integrals over the whole run (sampler.py:1342-1348, utils.py:1411-1467): ln Z the
  // accumulated logaddexp, and the partial informations H_i normalised by the FINAL Z,
  //   H_i = (1/Z_f) sum_{k<=i} [L ln L]-terms - (Z_i / Z_f) ln Z_f,   var ln Z = |sum_i (H_i - H_{i-1}) dlnX_i|.
  // With G = e^{lnZ}(H + lnZ) (additive) the state after the dead points gives
  // H_n = e^{lnZ_n - lnZ_f} (H^run_n + lnZ_n - lnZ_f); over the dead points dlnX is constant, so their
  // share of the variance sum telescopes to dlnX * H_n.
  // Every thread owns a contiguous stretch of the points; the two running quantities -- ln Z_i (logaddexp) and the sum
  // of the L e^L terms -- are prefix scans over the stretches' totals, after which a thread walks its own stretch
  // (one thread walking all N points in the reference's order was 1.4 of this kernel's 6.5 ms at N = 5 000; the
  // results agree to 1e-13).
  __shared__ double wtot[kT / 64];
  NsRun& r = a.st[run];
  const double lv0 = r.logvol, dead_prev = r.dead_prev;
  double* W = a.fin_ws + (size_t)run * a.fin_stride;  // trapezoid ln-weights
  double* DL = W + N;                          // -d ln X
  double* T = DL + N;                          // ln dX, then the L e^L terms
  // a plateau still being worked off keeps its volume steps for its remaining points, the rest of the final
  // points share what is left (sampler.py:813-830)
  const int pc = r.pcount < N ? r.pcount : N;
  const double pstep = pc > 0 ? exp(r.plogdvol - lv0) : 0.0;
  auto lv_at = [&](int i) {  // ln X after the i-th final point (1-based; 0: before the first)
    if (pc == 0) return i > 0 ? lv0 + log(1.0 - (double)i / ((double)N + 1.0)) : lv0;
    if (i <= pc) return lv0 + log1p(-(double)i * pstep);
    return lv0 + log1p(-(double)pc * pstep) + log1p(-(double)(i - pc) / ((double)(N - pc) + 1.0));
  };
  const int per = (N + kT - 1) / kT, c0 = t * per < N ? t * per : N, c1 = c0 + per < N ? c0 + per : N;
  double zc = -INFINITY;  // ln of the stretch's summed weights
  for (int i = c0 + 1; i <= c1; ++i) {
    const double cur = sorted[i - 1], prev = i > 1 ? sorted[i - 2] : dead_prev;
    const double lv = lv_at(i);
    const double lvprev = lv_at(i - 1);
    const double dl = lvprev - lv;
    const double logdvol = lv + log(0.5 * expm1(dl));
    const double w = logaddexp_dev(cur, prev) + logdvol;
    W[i - 1] = w;
    DL[i - 1] = dl;
    T[i - 1] = logdvol;
    zc = logaddexp_dev(zc, w);
  }
  double ztot;
  double zpre = block_excl_scan<true>(zc, -INFINITY, wtot, &ztot);
  const double logz_f = logaddexp_dev(r.logz, ztot);
  zpre = logaddexp_dev(r.logz, zpre);  // ln Z before this thread's stretch
  double hc = 0.0;
  for (int i = c0 + 1; i <= c1; ++i) {
    const double cur = sorted[i - 1], prev = i > 1 ? sorted[i - 2] : dead_prev;
    const double logdvol = T[i - 1];
    const double t0 = exp(prev - logz_f + logdvol), t1 = exp(cur - logz_f + logdvol);
    const double tt = (t1 > 0.0 ? t1 * cur : 0.0) + (t0 > 0.0 ? t0 * prev : 0.0);
    T[i - 1] = tt;
    hc += tt;
  }
  double htot;
  const double hpre = block_excl_scan<false>(hc, 0.0, wtot, &htot);
  const double dlv = log(((double)N + 1.0) / (double)N);
  const double wn = exp(r.logz - logz_f);
  const double hpart0 = r.it > 0 && wn > 0.0 ? wn * (r.h + r.logz) : 0.0;  // (1/Z_f) sum of the L ln L terms so far
  // H before this thread's stretch (for the first stretch: H_n)
  double logz = zpre, hpart = hpart0 + hpre;
  double hcur = hpart - (c0 == 0 ? (r.it > 0 ? wn * logz_f : 0.0) : logz_f * exp(logz - logz_f));
  double var = 0.0;
  for (int i = c0; i < c1; ++i) {
    logz = logaddexp_dev(logz, W[i]);
    hpart += T[i];
    const double hi = hpart - logz_f * exp(logz - logz_f);
    var += (hi - hcur) * DL[i];
    hcur = hi;
  }
  __shared__ double fin_h;
  if (c1 == N && c0 < N) fin_h = hcur;  // the thread that owns the last point
  double vtot;
  (void)block_excl_scan<false>(var, 0.0, wtot, &vtot);
  __syncthreads();
  if (t == 0) {
    // the dead points' share of sum_i (H_i - H_{i-1}) dlnX_i: it telescopes for the constant step, and the
    // plateau deaths' departures from it were summed on the way (ns_consume: var_a, var_b, relative to Z_n)
    const double h_n = hpart0 - (r.it > 0 ? wn * logz_f : 0.0);
    const double logzvar = h_n * dlv + (wn > 0.0 ? wn * (r.var_a - logz_f * r.var_b) : 0.0) + vtot;
    double* rec = a.records + (size_t)run * 8;
    rec[0] = logz_f;
    rec[1] = sqrt(fabs(logzvar));
    rec[2] = (double)r.it;
    rec[3] = (double)r.ncall;
    rec[4] = N > 0 ? fin_h : h_n;
    rec[5] = (double)r.nbound;
    rec[6] = (double)(r.mode == MODE_DONE ? 0 : (r.mode == MODE_FAILED ? -1 : 1));  // 1: hit maxfills
    rec[7] = 100.0 * (double)r.it / (double)r.ncall;
  }
}

// ---- dh_ns_continue: which runs of a kept ensemble go on, one workgroup per run ------------------------------------
// The reference's tests at the top of the loop (sampler.py:1071-1100, ns_state.h) on the state the last call left,
// under THIS call's criteria.  A run for which one holds is MODE_DONE (again) with nothing new; a failed run stays
// failed; a run that max_fills stopped simply goes on.  A run that a stop rule ended inside a fill gets back what
// that fill found -- its state (NsArgs::sv_st; the scale tuned from that fill, the fill count and the sampler's
// flags stay) and the previous content of the slots the fill replaced -- and is marked for ns_consume's replay,
// which takes the fill's r_* rows again, whole: the entries behind the stop are not lost (the reference keeps its
// queue), and the fill's evidence sums are those of the uninterrupted run to the last bit, which the sums of two
// partial consumptions would not be.  ndone[0] / ndone[1] are counted anew.
__global__ void __launch_bounds__(kT) ns_resume(NsArgs a) {
  const int run = blockIdx.x, t = threadIdx.x, N = a.nlive, D = a.ndim, K = a.K;
  NsRun& r = a.st[run];
  __shared__ int back;
  if (t == 0) {
    int rest = 0, put_back = 0;
    if (r.mode != MODE_FAILED) {
      const dh_ns_state::StopState s = {r.logvol, r.logz, r.lmax, r.loglstar, r.dead_prev, r.it, r.ncall};
      const dh_ns_state::StopRule c = {a.dlogz, a.logl_max, a.maxiter, a.maxcall};
      if (dh_ns_state::stop_mask(s, c)) {
        if (r.mode != MODE_DONE) r.qstop = 0;
        r.mode = MODE_DONE;
      } else if (r.mode == MODE_DONE) {
        if (r.qstop > 0 && a.sv_st) {
          NsRun b = a.sv_st[run];
          rest = K - r.qstop;
          b.scale = r.scale;
          b.nfill = r.nfill;
          b.doubling = r.doubling;
          b.sampler_failed = r.sampler_failed;
          b.qstop = -1;
          r = b;
          put_back = 1;
        } else {
          r.mode = r.nbound > 0 ? MODE_BOUND : MODE_CUBE;
          r.qstop = 0;
        }
      }
    }
    a.rest[run] = rest;
    back = put_back;
    if (r.mode == MODE_DONE || r.mode == MODE_FAILED) atomicAdd(a.ndone, 1);
    if (r.mode == MODE_CUBE) atomicOr(a.ndone + 1, 1);
  }
  __syncthreads();
  if (!back) return;
  // (the counts and slots come from ns_consume -- or from an imported image: nothing outside the run's rows is written)
  int n = a.sv_n[run];
  n = n < 0 ? 0 : n > K ? K : n;
  for (int c = t; c < n; c += kT) {
    const size_t o = (size_t)run * K + c;
    if (a.sv_slot[o] < 0 || a.sv_slot[o] >= N) continue;
    const size_t sl = (size_t)run * N + a.sv_slot[o];
    a.live_logl[sl] = a.sv_logl[o];
    if (a.live_it) a.live_it[sl] = a.sv_it[o];
  }
  for (int x = t; x < n * D; x += kT) {
    const int c = x / D, j = x - c * D, slot = a.sv_slot[(size_t)run * K + c];
    if (slot < 0 || slot >= N) continue;
    const size_t from = ((size_t)run * K + c) * D + j, to = ((size_t)run * N + slot) * D + j;
    a.live_u[to] = a.sv_u[from];
    a.live_v[to] = a.sv_v[from];
  }
}

// ---- dh_ns_batch: the seeding phase of a dynamic batch and the hand-over into the loop ------------------------------
// _configure_batch_sampler (dynamicsampler.py:300-622) for R strands at once.  A strand's live set is first the
// nlive_new points chosen from the base run (the seeds, all above logl_min); its bound is built on them, once; then
// nlive_new new points are proposed at the FIXED threshold logl_min from start points among the seeds -- the ordinary
// ns_select / ns_gather / walk stages -- and collected in a staging set (ns_seed_consume), which replaces the seeds
// when it is full (ns_batch_start).  From there on the strand is an ordinary run of the loop whose volume and evidence
// go on from the base run's row at logl_min.  Where this departs from the reference:
//  (a) the bound is not rebuilt during seeding (the reference's update policy would fire on the calls spent): the seed
//      points do not change, so a second bound on them would be the first again but for its bootstrap draw;
//  (b) the last seed fill's unused queue entries are dropped, their calls counted (the reference keeps them in the
//      queue for the first deaths);
//  (c) a strand always starts in bound mode (the reference stays on the unit cube while logl_min is below the base
//      run's first bound update, sampler.py:650-653);
//  (d) the scale the strand starts with is the caller's (start row, column 5): the merged run keeps no per-point scale
//      (the reference takes saved_scale[subset0[0]]).

// the strands' states from the start rows, their generators (child 0x80000000 + first_run + run, as ns_init), and the
// bookkeeping of the one bound update: nbound = 1 at call count 0, its bootstrap words drawn as ns_prepare draws them
__global__ void __launch_bounds__(kT)
    ns_batch_init(NsArgs a, NsSeed sd, const uint32_t* __restrict__ entropy, int nwords, uint32_t first_run) {
  for (int run = threadIdx.x; run < a.runs; run += kT) {
    const double* s = sd.start + (size_t)run * 6;
    NsRun r;
    r.logvol = s[0];
    r.logz = s[1];
    r.h = s[2];
    r.logzvar = s[3];
    r.dead_prev = s[4];
    r.scale = s[5];
    r.lmax = -1e300;
    r.loglstar = sd.logl_min;
    r.it = 0;
    r.ncall = 0;
    r.ncall_last_update = 0;
    r.mode = MODE_BOUND;
    r.need_rebuild = 1;
    r.nbound = 1;
    r.nfill = 0;
    r.acc = r.rej = r.doubling = r.due = 0;
    r.fpend = r.qstop = 0;
    r.nc_carry = 0;
    r.pcount = r.sampler_failed = 0;
    r.plogdvol = r.var_a = r.var_b = 0.0;
    Pcg64 g;
    seed_from_child(g, entropy, nwords, 0x80000000u + first_run + (uint32_t)run);
    if (a.bootstrap > 0)
      for (int i = 0; i < 4; ++i) a.boot_ent[(size_t)run * 4 + i] = g.next64();
    g.store(r.rng);
    a.st[run] = r;
    a.rebuild_mask[run] = 1;
    a.run_mode[run] = MODE_BOUND;
    sd.n[run] = 0;
    sd.rej[run] = 0;
    sd.ncall[run] = 0;
  }
}

// before every seed fill: which strands still collect points (the others sit the fill out), the walkers' per-run
// parameters at the fixed threshold; a strand whose bound could not be built fails, as in ns_prepare.
__global__ void __launch_bounds__(kT) ns_seed_prepare(NsArgs a, NsSeed sd) {
  for (int run = threadIdx.x; run < a.runs; run += kT) {
    NsRun& r = a.st[run];
    if (r.mode == MODE_BOUND && a.bstatus[run] != DH_OK) {
      r.mode = MODE_FAILED;
      atomicAdd(a.ndone, 1);
    }
    const int seeding = (r.mode == MODE_BOUND && sd.n[run] < a.nlive) ? 1 : 0;
    r.need_rebuild = 0;
    a.rebuild_mask[run] = 0;
    a.run_mode[run] = seeding ? MODE_BOUND : MODE_WAIT;
    a.run_loglstar[run] = sd.logl_min;
    a.run_scale[run] = r.scale;
    a.run_doubling[run] = r.doubling;
  }
}

// One seed fill's queue, one workgroup per strand: in queue order every entry above logl_min joins the staging set
// (u, v, ln L, nc = its calls and those of the rejected entries before it) until the set holds nlive_new points; all
// of the fill's calls are charged to the strand, and the sampler's scale is tuned as ns_consume tunes it for a fill.
// No live point is replaced.  Which entry gets which row is a serial pass of one thread over the queue's values in LDS
// (K <= 2048 reads, once per seed fill, nlive_new / K fills per batch: an entry is rejected only when its slice
// failed); the rows' coordinates are then copied by all threads, sixteen elements of a thread in flight.
__global__ void __launch_bounds__(kT) ns_seed_consume(NsArgs a, NsSeed sd) {
  constexpr int kQ = kEPTMax * kT;
  __shared__ double ql[kQ];
  __shared__ int qc[kQ];
  __shared__ int tj[kQ];   // queue index of the c-th entry this fill stages
  __shared__ int tnc[kQ];  // ... and its nc
  __shared__ int racc[kT], rrej[kT];
  __shared__ int ntake_s, n0_s;
  const int run = blockIdx.x, t = threadIdx.x;
  const int N = a.nlive, D = a.ndim, K = a.K;
  NsRun& r = a.st[run];
  if (r.mode != MODE_BOUND || a.run_mode[run] != MODE_BOUND) return;
  int acc = 0, rej = 0, bad = 0, dbl = 0;
  for (int j = t; j < K; j += kT) {
    const size_t q = (size_t)run * K + j;
    // (every load unconditional, from a clamped offset where the index is data: selects below)
    const double rl = a.r_logl[q];
    const int ra = a.r_a[q], rb = a.r_b[q], rc = a.r_c[q], rd = a.r_d[q];
    const double own = a.live_logl[(size_t)run * N + ((unsigned)rd < (unsigned)N ? rd : 0)];
    double l = rl;
    int c = ra;
    if (a.sampler == 3) {
      if (rb & 3) l = -INFINITY;  // no ellipsoid held the draw / the try limit: the strand fails below
      bad |= rb & 3;
    } else if (a.sampler == 0) {
      c = a.walks;
      acc += ra;
      rej += rb;
      if (ra == 0) l = own;  // no step accepted: the start point (a seed) with its own stored ln L, as in ns_consume
    } else {
      acc += rb;  // n_expand
      rej += rc;  // n_contract
      dbl |= rd & 1;
      if (rd & 2) l = -INFINITY;  // failed slice: never accepted
    }
    ql[j] = l;
    qc[j] = c;
  }
  racc[t] = acc;
  rrej[t] = rej;
  bad = __syncthreads_or(bad);
  dbl = __syncthreads_or(dbl);
  for (int sft = kT / 2; sft > 0; sft >>= 1) {
    if (t < sft) {
      racc[t] += racc[t + sft];
      rrej[t] += rrej[t + sft];
    }
    __syncthreads();
  }
  // (the rows staged so far are read by the ONE thread that also stores the new count, and reach the others through
  // LDS behind the barrier below: a wave that read the global count itself could read it after that store)
  if (t == 0) {
    long long pend = sd.rej[run], calls = 0;
    const int first = sd.n[run];
    int n = first;
    for (int j = 0; j < K; ++j) {
      const int c = qc[j];
      calls += c;
      if (n < N && ql[j] > sd.logl_min) {
        tj[n - first] = j;
        tnc[n - first] = (int)(pend + c);
        pend = 0;
        ++n;
      } else {
        pend += c;  // (behind the last row: dropped with the fill, departure (b))
      }
    }
    ntake_s = n - first;
    n0_s = first;
    sd.n[run] = n;
    sd.rej[run] = pend;
    r.ncall += calls;
    if (dbl) r.doubling = 1;
    if (a.sampler != 3) {
      const int ta = racc[0], tr = rrej[0];
      if (a.sampler == 0) {
        // RWalkSampler.tune (internal_samplers.py:460-493), once per queue fill
        if (ta + tr > 0) r.scale *= exp(((double)ta / (double)(ta + tr) - a.facc) / (double)D / a.facc);
      } else {
        // tune_slice (internal_samplers.py:1209-1239)
        const double ne = ta > 1 ? (double)ta : 1.0, nt = (double)tr;
        double mult = ne * 2.0 / (ne + nt);
        mult = fmin(fmax(mult, 0.5), 2.0);
        r.scale *= mult;
      }
    }
    if (bad) {  // a uniform-sampler walker gave up: the reference's RuntimeError
      r.sampler_failed = 1;
      r.mode = MODE_FAILED;
      atomicAdd(a.ndone, 1);
    }
  }
  __syncthreads();
  const int ntake = ntake_s, n0 = n0_s;
  for (int c = t; c < ntake; c += kT) {
    sd.logl[(size_t)run * N + n0 + c] = ql[tj[c]];
    sd.nc[(size_t)run * N + n0 + c] = tnc[c];
  }
  double* su = sd.u + ((size_t)run * N + n0) * D;
  double* sv = sd.v + ((size_t)run * N + n0) * D;
  const double* ru = a.r_u + (size_t)run * K * D;
  const double* rv = a.r_v + (size_t)run * K * D;
  const int tot = ntake * D;
  constexpr int LS = 16;
  for (int e0 = t; e0 < tot; e0 += LS * kT) {
    double xu[LS], xv[LS];
#pragma unroll
    for (int q = 0; q < LS; ++q) {
      const int e = e0 + q * kT;
      const int ec = e < tot ? e : 0;
      const int c = ec / D, j = ec - c * D;
      const size_t from = (size_t)tj[c] * D + j;
      xu[q] = ru[from];
      xv[q] = rv[from];
    }
#pragma unroll
    for (int q = 0; q < LS; ++q)
      if (e0 + q * kT < tot) {
        su[e0 + q * kT] = xu[q];
        sv[e0 + q * kT] = xv[q];
      }
  }
}

// The hand-over, one workgroup per strand: the staging set becomes the live set (every point proposed at iteration 0),
// lmax / loglstar are its largest / smallest ln L as ns_start takes them, the loop's counters start at 0 and the
// volume, the evidence sums and the last dead ln L are the start row's (ns_batch_init put them there; seeding does not
// touch them).  A strand whose staging set is not full after the seed fills has failed.
__global__ void __launch_bounds__(kT) ns_batch_start(NsArgs a, NsSeed sd) {
  const int run = blockIdx.x, t = threadIdx.x, N = a.nlive, D = a.ndim;
  NsRun& r = a.st[run];
  __shared__ double rmax[kT], rmin[kT];
  if (r.mode != MODE_BOUND) return;
  if (sd.n[run] < N) {
    if (t == 0) {
      r.mode = MODE_FAILED;
      atomicAdd(a.ndone, 1);
      sd.ncall[run] = r.ncall;
    }
    return;
  }
  double mx = -1e300, mn = INFINITY;
  for (int i = t; i < N; i += kT) {
    const double k = sd.logl[(size_t)run * N + i];
    a.live_logl[(size_t)run * N + i] = k;
    if (a.live_it) a.live_it[(size_t)run * N + i] = 0;
    mx = fmax(mx, k);
    mn = fmin(mn, k);
  }
  rmax[t] = mx;
  rmin[t] = mn;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (t < s) {
      rmax[t] = fmax(rmax[t], rmax[t + s]);
      rmin[t] = fmin(rmin[t], rmin[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) {
    r.lmax = rmax[0];
    r.loglstar = rmin[0];
    r.it = 0;
    r.nc_carry = 0;
    sd.ncall[run] = r.ncall;
    for (int i = 0; i < 4; ++i) sd.rng[(size_t)run * 4 + i] = r.rng[i];
  }
  // (the rows of a strand are contiguous: sixteen elements of a thread in flight, as in ns_consume's live store)
  const double* su = sd.u + (size_t)run * N * D;
  const double* sv = sd.v + (size_t)run * N * D;
  double* lu = a.live_u + (size_t)run * N * D;
  double* lv = a.live_v + (size_t)run * N * D;
  const size_t tot = (size_t)N * D;
  constexpr int LS = 16;
  for (size_t e0 = t; e0 < tot; e0 += (size_t)LS * kT) {
    double xu[LS], xv[LS];
#pragma unroll
    for (int q = 0; q < LS; ++q) {
      const size_t e = e0 + (size_t)q * kT;
      const size_t ec = e < tot ? e : 0;
      xu[q] = su[ec];
      xv[q] = sv[ec];
    }
#pragma unroll
    for (int q = 0; q < LS; ++q)
      if (e0 + (size_t)q * kT < tot) {
        lu[e0 + (size_t)q * kT] = xu[q];
        lv[e0 + (size_t)q * kT] = xv[q];
      }
  }
}

}  // namespace

namespace {
// the instance of ns_consume for a queue of K entries (kEPT = 1, 2, 4 or 8 deaths per lane)
typedef void (*NsConsumeFn)(NsArgs);
inline NsConsumeFn ns_consume_for(int K) {
  const int ept = (K + kT - 1) / kT;
  return ept <= 1 ? ns_consume<1> : ept <= 2 ? ns_consume<2> : ept <= 4 ? ns_consume<4> : ns_consume<8>;
}

constexpr size_t kNsLdsMax = 150 * 1024;  // dynamic LDS a workgroup of ns_consume / ns_start / ns_finish may ask for

inline int ns_serial_walk() { return env_int("DH_NS_SERIAL", 0) != 0 ? 1 : 0; }

// the attribute is per device (and the call is cheap): set it on every call, on this context's device
bool ns_set_lds(dh_ctx* ctx, int K, size_t lds_max, bool finish) {
  const hipFuncAttribute at = hipFuncAttributeMaxDynamicSharedMemorySize;
  return hip_ok(ctx, hipFuncSetAttribute((const void*)ns_consume_for(K), at, (int)lds_max), "hipFuncSetAttribute(ns_consume)") &&
         hip_ok(ctx, hipFuncSetAttribute((const void*)ns_start, at, (int)lds_max), "hipFuncSetAttribute(ns_start)") &&
         (!finish || hip_ok(ctx, hipFuncSetAttribute((const void*)ns_finish, at, (int)lds_max), "hipFuncSetAttribute(ns_finish)"));
}

// ---- dh_ns_ensemble, host side: plan (arguments, options, environment) -> layout (one allocation) -> stages ----

// Everything a call decides before it touches the device.
struct NsPlan {
  NsArgs a;  // the scalar part; the arrays come from ns_arrays
  int problem;
  bool philox;  // proposals (and the unit-cube phase) from Philox streams
  int fr_kind;  // friends.hip KIND_BALLS / KIND_CUBES, -1: ellipsoids
  int fr_reps;  // bootstrap replicas of the friends update
  int every;    // bounds are built every `every`-th fill
  bool enlarged, force_check, presort_ok, want_pt, want_prof;
  size_t lds_cons, lds_fin;
  int64_t fills_cap;
  int n_frames;
  dh::PhiloxKey key;  // seed and first subsequence of the call (ns_philox_key)
  // (set by dh_ns_ensemble, not by ns_plan) the ensemble is kept: the arrays of NsArgs::sv_st exist; the entropy
  // words' count and whether boundary flags were installed -- with them ns_arrays is a function of the plan alone
  bool keep;
  int n_words;
  bool have_bc;
};

// the arrays of the state allocation that no kernel takes through NsArgs
struct NsAux {
  uint32_t* ent;     // the caller's entropy words
  int8_t* bc;        // periodic / reflective coordinates (dh_ns_set_boundary), null: all hard
  char* boot_ws;     // bootstrap_expand_launch
  unsigned short* presort;
  // friends bounds: the shapes' axes_inv (the metric am, cov, axes and ln V sit in b_ams, b_covs, b_axes, b_lv), the
  // live sets in each shape's whitened frame, the batched update's workspace, bootstrap masks and their scratch
  double *fai, *fct;
  char* fr_ws;
  unsigned char* fr_mask;
  int* fr_scratch;
  double* frr;
  int* fnc;
  // dh_ns_batch: the seeding phase's arrays (set `batch` before ns_arrays to have them carved)
  bool batch = false;
  NsSeed seed{};
};

int ns_plan(dh_ctx* ctx, const double* opt, size_t n_bc, int problem, int runs, int nlive, int ndim, int queue_size,
            int sampler, int walks, int bound, int rebuild_sync, double dlogz, double enlarge, int64_t max_fills,
            int64_t max_iter, const uint32_t* entropy_words, int n_words, uint32_t first_run, const double* records,
            bool store_samples, int n_pt_out, int bootstrap, int rebuild_every, NsPlan* plan) {
  NsPlan& p = *plan;
  p.want_pt = n_pt_out > 0;
  if (p.want_pt && n_pt_out != 4)
    return fail(ctx, DH_ERR_ARG, "ns_ensemble: the per-point outputs (id, it, nc, live it) come together");
  ProblemDev pd;
  if (!get_problem(ctx, problem, &pd)) return DH_ERR_ARG;
  if (pd.ndim != ndim) return fail(ctx, DH_ERR_ARG, "problem ndim %d != %d", pd.ndim, ndim);
  p.problem = problem;
  // sampler 3 / 4 / 5 = rwalk / rslice / slice with the unit-cube phase and the proposals drawn from hiprand
  // Philox streams (throughput RNG mode); start points and frames keep their PCG64 streams
  // sampler 6 / 7 = the uniform sampler inside the bound (UniformBoundSampler) from PCG64 / Philox streams
  p.philox = (sampler >= 3 && sampler <= 5) || sampler == 7;
  // bound: 0 single ellipsoid, 1 multi-ellipsoid, 2 RadFriends (balls), 3 SupFriends (cubes); the friends bounds with
  // the uniform sampler from PCG64 streams (sampler 6) at ndim <= 32 only
  if (bound < 0 || bound > 3) return fail(ctx, DH_ERR_ARG, "ns_ensemble: bound code %d (0 single, 1 multi, 2 balls, 3 cubes)", bound);
  if (bound >= 2 && (sampler != 6 || ndim > kMaxRegDim))
    return fail(ctx, DH_ERR_ARG, "ns_ensemble: bound code %d (balls / cubes) needs sampler 6 (unif, PCG64) and ndim <= %d "
                                 "(sampler %d, ndim %d)", bound, kMaxRegDim, sampler, ndim);
  const int bound_multi = bound == 1 ? 1 : 0;
  p.fr_kind = bound >= 2 ? bound - 2 : -1;
  p.fr_reps = bootstrap > 0 ? bootstrap : 0;
  if (sampler >= 6 && sampler <= 7)
    sampler = 3;  // internal code of `unif`
  else if (p.philox)
    sampler -= 3;
  else if (sampler > 2)
    sampler = -1;
  if (runs < 1 || nlive < 4 || queue_size < 1 || walks < 1 || sampler < 0 || sampler > 3 || !entropy_words ||
      n_words < 1 || !records || bootstrap < 0 || bootstrap == 1)
    return fail(ctx, DH_ERR_ARG, "ns_ensemble: bad arguments");
  // Above the register-resident dimensions (and for slice samplers at dimensions without an instantiation) the
  // walker launches go to the wave-per-walker kernels of wide.hip, which take the same per-run arrays; above
  // d = 44 the bound is the multi-workgroup Ellipsoid.update with the run mask, or -- bound='multi' -- the wide
  // MultiEllipsoid.update: a host recursion over device node work, so a rebuild fill there synchronises the stream
  // and reads the run mask back (the loop is no longer launch-ahead on those fills; the tree is a handful of nodes).
  const int N = nlive, D = ndim, K = queue_size, R = runs;
  // the register sort of the live slots is built for at most 32 keys per thread (sort_slots<32>); the LDS bound of
  // ns_finish below is tighter today, this one is the sort's own
  if (N > 65535) return fail(ctx, DH_ERR_ARG, "ns_ensemble: nlive %d > 65535 (slots travel as 16-bit indices)", N);
  if (n_bc && (int)n_bc != ndim)
    return fail(ctx, DH_ERR_ARG, "ns_ensemble: %d boundary flags for ndim %d", (int)n_bc, ndim);
  const int me = bound_multi ? (N / (2 * D) > 0 ? N / (2 * D) : 1) : 1;
  NsArgs& a = p.a;
  a = NsArgs{};
  a.runs = R;
  a.nlive = N;
  a.ndim = D;
  a.K = K;
  a.walks = walks;
  a.sampler = sampler;
  a.bound_multi = bound_multi;
  a.max_ells = me;
  a.cap = max_iter > 0 ? max_iter : 400000;
  a.dlogz = dlogz;
  a.enlarge_log = log(enlarge);
  a.facc = fmin(1.0, fmax(1.0 / (double)(walks > 2 ? walks : 2), 0.5));
  a.first_eff = 10.0;
  a.first_ncall = 2ll * N;
  // update_bound_interval_ratio (internal_samplers.py:495-502, 581-588, 737-744) * nlive
  // (UniformBoundSampler keeps the base class's ratio 1, internal_samplers.py:88-94)
  a.update_interval = (long long)(sampler == 3 ? 1 : sampler == 2 ? walks * D : walks) * N;
  // the sampler's / run_nested's options a caller has set (dh_ns_set_option; NaN = the reference's default)
  if (!std::isnan(opt[DH_NS_OPT_UPDATE_INTERVAL])) {
    // update_interval as dynesty takes it (dynesty.py:213-234): a float is a multiple of nlive, an int a number of calls
    const double v = opt[DH_NS_OPT_UPDATE_INTERVAL];
    // (a value below one call is one call: the reference's max(min(round(...), maxsize), 1), dynesty.py:646-649)
    a.update_interval = v >= 1.0 ? (long long)llround(v) : 1;
  }
  if (!std::isnan(opt[DH_NS_OPT_FIRST_MIN_NCALL])) a.first_ncall = (long long)llround(opt[DH_NS_OPT_FIRST_MIN_NCALL]);
  if (!std::isnan(opt[DH_NS_OPT_FIRST_MIN_EFF])) a.first_eff = opt[DH_NS_OPT_FIRST_MIN_EFF];
  if (!std::isnan(opt[DH_NS_OPT_MAXITER])) a.maxiter = (long long)llround(opt[DH_NS_OPT_MAXITER]);
  if (!std::isnan(opt[DH_NS_OPT_MAXCALL])) a.maxcall = (long long)llround(opt[DH_NS_OPT_MAXCALL]);
  if (!std::isnan(opt[DH_NS_OPT_LOGL_MAX])) a.logl_max = opt[DH_NS_OPT_LOGL_MAX];
  if (!std::isnan(opt[DH_NS_OPT_ADD_LIVE])) a.add_live = opt[DH_NS_OPT_ADD_LIVE] != 0.0 ? 1 : 0;
  // default (round 5): the reference's protocol; 0 = the late form (opt-in fast mode)
  // (the uniform sampler has no start points, hence no forced update: for it the option is the ordering of the
  // regular update alone)
  a.forced_exact = 1;
  if (!std::isnan(opt[DH_NS_OPT_FORCED_EXACT])) a.forced_exact = opt[DH_NS_OPT_FORCED_EXACT] != 0.0 ? 1 : 0;
  if (a.maxcall >= 0 && a.maxcall < N)
    return fail(ctx, DH_ERR_ARG, "ns_ensemble: maxcall %lld below the %d calls of the initial live points", a.maxcall, N);
  a.bootstrap = bootstrap;
  a.store_samples = store_samples ? 1 : 0;
  a.rebuild_sync = rebuild_sync ? 1 : 0;
  a.serial_walk = ns_serial_walk();
  a.fin_stride = ns_fin_stride(N);
  a.presort_stride = 2048;
  p.enlarged = enlarge != 1.0;
  // Bounds are built every rebuild_every-th fill (runs that become due in between wait, see ns_prepare); 0 = chosen
  // here.  Once the period reaches the number of fills a run needs to spend its update interval, EVERY run is due (and
  // waiting) by the next rebuild fill: the ensemble rebuilds together and walks together, one latency chain per
  // interval instead of one per fill, with each run's own sequence untouched.  Longer periods only add idle fills
  // (a fill in which every run waits costs its launches, ~75 us), shorter ones lose the synchrony -- measured flat
  // from the interval upwards (64 C2 runs: 0.335 s at 1, 0.246 at 2, 0.29 at 3, 0.20 at 4 ... 12).  The interval in
  // fills is nlive / K for rwalk (every walker spends `walks` calls), about nlive / (4.4 K) for the slice samplers
  // (4.4 evaluations per slice step measured) and nlive / (1.7 K) for the uniform sampler; rounded up generously.
  // The choice is a function of the arguments only -- never of timings -- so a run's global fill indices, and with
  // them its Philox offsets, are reproducible.
  p.every = env_int("DH_NS_REBUILD_EVERY", rebuild_every);
  if (p.every <= 0) {
    const double I = sampler == 0 ? (double)N / K : 1.3 * (double)N / ((sampler == 3 ? 1.7 : 4.4) * K);
    p.every = (int)ceil(I - 1e-9);
  }
  if (p.every < 1) p.every = 1;
  if (p.every > 16) p.every = 16;
  p.want_prof = env_int("DH_NS_PROF", 0) != 0;
  p.force_check = env_int("DH_NS_FORCE", 1) != 0;  // diagnostic: 0 = no forced rebuilds
  if (K > kEPTMax * kT) return fail(ctx, DH_ERR_ARG, "ns_ensemble: queue_size %d > %d", K, kEPTMax * kT);
  p.lds_fin = 64;  // ns_finish: the keys by slot, the keys in order, the sorted slots (large sets: global memory)
  if (!ns_finish_big(N)) {
    size_t Pf = 1;
    while (Pf < (size_t)N) Pf <<= 1;
    p.lds_fin += (size_t)N * 16 + (Pf > 256 ? Pf : 256) * 2;
  }
  p.lds_cons = ns_consume_lds(N, K);
  if ((p.lds_cons > p.lds_fin ? p.lds_cons : p.lds_fin) > kNsLdsMax)
    return fail(ctx, DH_ERR_ARG, "ns_ensemble: nlive/queue too large for LDS");
  if (me > kMaxCum) return fail(ctx, DH_ERR_ARG, "ns_ensemble: nlive/(2 ndim) = %d ellipsoids > %d", me, kMaxCum);
  p.fills_cap = max_fills > 0 ? max_fills : 1000000;
  p.n_frames = R * me * (a.forced_exact ? 2 : 1);
  // the slot order ns_consume needs can be sorted in front of the generator pass's grid (beside the walk) where the
  // whole live set is sorted (not the compact form) and fits the generator's LDS
  p.presort_ok = sampler == 0 && N <= 2048 && !ns_consume_compact(N, K) && env_int("DH_NS_PRESORT", 1) != 0;
  // Philox keys: seed from the entropy words, subsequence = global walker slot (first_run + run) * K + w (independent
  // of the sharding)
  p.key.seed = ((unsigned long long)entropy_words[0] << 32) ^ (n_words > 1 ? entropy_words[1] : 0u) ^ 0x9E3779B97F4A7C15ull;
  p.key.seq0 = (unsigned long long)first_run * (unsigned long long)K;
  p.key.offset = 0;
  return DH_OK;
}

// The key of one stage's Philox streams in one fill.  Every stage has a seed of its own, so that the stages' offset
// schemes cannot meet.  Stages whose consumption depends on the data (unit cube, slice samplers, uniform sampler) get
// 2^24 draws per walker and fill.  rwalk consumes a fixed number of 32-bit draws per walker and fill: per step
// hiprand_normal4 x ceil(D / 4) and one hiprand_uniform_double (2 draws; padded to 4 so that a fill's block stays
// 4-aligned).
enum NsStage { STAGE_CUBE, STAGE_RWALK, STAGE_SLICE, STAGE_UNIF };
dh::PhiloxKey ns_philox_key(const NsPlan& p, NsStage stage, int64_t fill) {
  dh::PhiloxKey key = p.key;
  if (stage == STAGE_RWALK) {
    key.offset = (unsigned long long)fill * (unsigned long long)p.a.walks * (unsigned long long)(4 * ((p.a.ndim + 3) / 4) + 4);
    return key;
  }
  key.seed ^= stage == STAGE_CUBE ? 0x5BD1E995C0BEull : 0x27D4EB2F511CEull;
  if (stage == STAGE_UNIF) key.seed ^= 0x3C6EF372FE94F82Bull;
  key.offset = (unsigned long long)fill << 24;
  return key;
}

// Walks the list of state arrays: without a base it adds up their sizes (256-byte aligned), with one it hands out the
// pointers and enqueues the initial fills.  An array that is not wanted takes no room and stays null.
struct NsEntry {  // one array of the allocation: where it starts and its bytes
  size_t off, bytes;
};
struct NsCarver {
  dh_ctx* ctx;
  char* base;
  size_t off = 0;
  bool ok = true;
  std::vector<NsEntry>* list = nullptr;  // optional: the arrays handed out, in order (dh_ns_state_export / _import)
  bool fills = true;                     // false: pointers only, the arrays are in use (a kept ensemble's own base)
  template <class T>
  void operator()(T*& p, size_t count, bool wanted = true, int fill = -1) {
    p = nullptr;
    if (!wanted) return;
    const size_t bytes = count * sizeof(T);
    if (base) {
      p = (T*)(base + off);
      if (fill >= 0 && ok && fills) ok = hip_ok(ctx, hipMemsetAsync(base + off, fill, bytes, ctx->stream), "memset");
    }
    if (list && bytes) list->push_back({off, bytes});
    off += (bytes + 255) & ~(size_t)255;
  }
};

// THE list of the ensemble's device arrays: element type (the pointer's), element count, wanted or not, initial fill
void ns_arrays(NsCarver& c, const NsPlan& p, NsArgs& a, NsAux& x, int n_words, bool have_bc) {
  const size_t R = (size_t)a.runs, N = (size_t)a.nlive, D = (size_t)a.ndim, K = (size_t)a.K, me = (size_t)a.max_ells;
  const size_t cap = (size_t)a.cap, dd = D * D;
  const bool fx = a.forced_exact != 0, fr = p.fr_kind >= 0, frb = fr && p.fr_reps > 0;
  c(a.st, R);
  c(a.live_u, R * N * D);
  c(a.live_v, R * N * D);
  c(a.live_logl, R * N);
  c(a.dead_logl, R * cap);
  c(a.dead_u, R * cap * D, a.store_samples != 0);
  c(a.q_u0, R * K * D);
  c(a.q_frame, R * K);
  c(a.q_rng, R * K * 4);
  c(a.q_rng_out, R * K * 4);
  c(a.r_u, R * K * D);
  c(a.r_v, R * K * D);
  c(a.r_logl, R * K);
  c(a.r_a, R * K);
  c(a.r_b, R * K);
  c(a.r_c, R * K);
  c(a.r_d, R * K);
  c(a.run_doubling, R);
  c(a.run_loglstar, R);
  c(a.run_scale, R);
  c(a.run_mode, R);
  c(a.rebuild_mask, R);
  c(a.force, R, true, 0);
  c(a.ndone, 16, true, 0);
  c(a.nells, R, true, 0);
  c(a.bstatus, R, true, 0);
  c(a.b_ctrs, R * me * D);
  c(a.b_covs, R * me * dd);
  c(a.b_ams, R * me * dd);
  c(a.b_axes, R * me * dd * (fx ? 2 : 1));  // (forced_exact: and the frames a forced update keeps, ns_shadow_axes)
  c(a.b_axl, R * me * D);
  c(a.b_lv, R * me);
  c(a.records, R * 8);
  c(x.ent, (size_t)n_words);
  c(a.fin_ws, R * a.fin_stride);
  c(a.b_cum, R * me);
  c(a.boot_ent, R * 4);
  c(a.run_shift, R);
  c(a.force_first, R, true, 0x7f);
  c(a.sel_ent, R * 4, fx);
  c(x.bc, D + 8, have_bc);
  c(a.undo_u, R * D, fx);
  c(a.undo_slot, R, fx, 0xff);
  c(a.fx_kind, R, fx, 0);
  c(a.pass_mode, R, fx, 0);
  c(x.boot_ws, a.bootstrap > 0 ? bootstrap_ws_bytes(a.runs, a.nlive, a.ndim, a.max_ells, a.bootstrap) : 0, a.bootstrap > 0);
  c(a.live_it, R * N, p.want_pt, 0);
  c(a.dead_id, R * cap, p.want_pt);
  c(a.dead_it, R * cap, p.want_pt);
  c(a.dead_nc, R * cap, p.want_pt);
  c(x.presort, R * 2048);
  c(x.fai, R * dd, fr);
  c(x.fct, R * N * D, fr);
  c(x.fr_ws, fr ? friends_batch_ws_bytes(a.runs, a.nlive, a.ndim, p.fr_reps) : 0, fr);
  c(x.fr_mask, R * p.fr_reps * N, frb);
  c(x.fr_scratch, R * p.fr_reps * 2, frb);
  c(x.frr, R);
  c(x.fnc, R);
  c(a.prof, 32, p.want_prof, 0);
  c(a.sv_st, R, p.keep);
  c(a.sv_u, R * K * D, p.keep);
  c(a.sv_v, R * K * D, p.keep);
  c(a.sv_logl, R * K, p.keep);
  c(a.sv_slot, R * K, p.keep);
  c(a.sv_it, R * K, p.keep);
  c(a.sv_n, R, p.keep, 0);
  c(a.rest, R, p.keep, 0);
  // the seeding phase of a dynamic batch (dh_ns_batch): never part of a saved image (ns_entry_kind)
  c(x.seed.u, R * N * D, x.batch);
  c(x.seed.v, R * N * D, x.batch);
  c(x.seed.logl, R * N, x.batch);
  c(x.seed.nc, R * N, x.batch);
  c(x.seed.n, R, x.batch, 0);
  c(x.seed.rej, R, x.batch, 0);
  c(x.seed.ncall, R, x.batch, 0);
  c(x.seed.rng, R * 4, x.batch, 0);
  c(x.seed.start, R * 6, x.batch);
  a.presort = x.presort;
}

// bound.update of the runs in rebuild_mask (+ bootstrap expansion, + enlarge): sampler.py:492-508
int build_bounds(dh_ctx* ctx, const NsPlan& p, const NsArgs& a, const NsAux& x) {
  const int R = a.runs, N = a.nlive, D = a.ndim, me = a.max_ells;
  if (p.fr_kind >= 0) {
    // RadFriends.update / SupFriends.update of the masked runs in one launch sequence (friends.hip), clustering in
    // each run's previous metric; the bootstrap replicas' in-sample masks from the words ns_prepare drew
    int rc = DH_OK;
    if (p.fr_reps) rc = boot_masks_launch(ctx, R, N, p.fr_reps, a.boot_ent, a.rebuild_mask, x.fr_mask, x.fr_scratch);
    if (rc) return rc;
    return friends_update_launch(ctx, R, a.live_u, N, D, p.fr_kind, a.b_ams, p.fr_reps, x.fr_mask, a.rebuild_mask,
                                 p.enlarged ? a.enlarge_log : 0.0, x.fr_ws, a.b_covs, a.b_ams, a.b_axes, x.fai, a.b_lv,
                                 x.frr, x.fnc, a.bstatus, a.run_mode);
  }
  int rc = rebuild_launch_masked(ctx, R, a.live_u, N, D, a.bound_multi ? 0 : 1, me, a.nells, a.bstatus, a.b_ctrs,
                                 a.b_covs, a.b_ams, a.b_axes, a.b_axl, a.b_lv, a.rebuild_mask);
  if (rc) return rc;
  if (a.bootstrap > 0) {
    // bound.update(points, bootstrap=B): the expansion factor from B resampled replicas per rebuilding run,
    // then scale_to_logvol(logvol + ndim ln(expand)) where it exceeds 1 (bounding.py:381-400, 688-703)
    rc = bootstrap_expand_launch(ctx, R, a.live_u, N, D, a.bound_multi, me, a.bootstrap, a.boot_ent, a.rebuild_mask,
                                 x.boot_ws, a.run_shift, nullptr, a.bstatus);
    if (rc) return rc;
    rc = enlarge_launch_masked(ctx, R, me, a.nells, D, a.b_covs, a.b_ams, a.b_axes, a.b_axl, a.b_lv, 0.0,
                               a.rebuild_mask, a.run_shift);
    if (rc) return rc;
  }
  if (p.enlarged)  // sampler.py:506-508
    rc = enlarge_launch_masked(ctx, R, me, a.nells, D, a.b_covs, a.b_ams, a.b_axes, a.b_axl, a.b_lv, a.enlarge_log,
                               a.rebuild_mask);
  return rc;
}

// ns_select, the start points' coordinates (ns_gather) and their membership test against the bounds of the runs that
// `modes` marks MODE_BOUND; pass: NsArgs::fx_pass, 0 outside the forced-exact protocol.  The uniform sampler starts
// nowhere: selection only.  (Above the register-resident dimensions the test takes one wavefront per start point.)
int select_and_test(dh_ctx* ctx, const NsPlan& p, NsArgs& a, int pass, const int* modes, int* first) {
  const int R = a.runs, K = a.K, D = a.ndim;
  hipStream_t s = ctx->stream;
  a.fx_pass = pass;
  hipLaunchKernelGGL(ns_select, dim3(R), dim3(kT), 0, s, a);
  if (a.sampler == 3) return DH_OK;
  hipLaunchKernelGGL(ns_gather, dim3((unsigned)(((size_t)R * K * D + 255) / 256)), dim3(256), 0, s, a);
  if (!p.force_check) return DH_OK;
  if (pass) hipLaunchKernelGGL(ns_pass_mask, dim3(1), dim3(kT), 0, s, a, pass);
  return contains_runs_launch(ctx, a.q_u0, R * K, D, K, a.b_ctrs, a.b_ams, a.bound_multi ? a.nells : nullptr, a.max_ells,
                              a.bound_multi ? 1 : 0, modes, MODE_BOUND, a.bstatus, a.force, first);
}

// The late form of the forced update (DH_NS_OPT_FORCED_EXACT = 0, the opt-in fast one).  Sampler.propose_live rebuilds
// the bound at once when a start point lies outside it (sampler.py:484-489: a point accepted since the last update,
// beyond the enlarged ellipsoids).  Here the run is flagged and rebuilds before its NEXT fill: the walkers of this fill
// are already chosen, and a queue of K proposals is as stale in the reference.
int bounds_late(dh_ctx* ctx, const NsPlan& p, NsArgs& a, const NsAux& x) {
  if (a.rebuild_fill) {
    const int rc = build_bounds(ctx, p, a, x);
    if (rc) return rc;
  }
  return select_and_test(ctx, p, a, 0, a.run_mode, nullptr);
}

// The reference's protocol (DH_NS_OPT_FORCED_EXACT, the default of the Python layer since round 5), with ONE
// rebuild chain per fill that builds bounds.  Pass 1: every run but those of this fill's regular updates
// selects its queue (a pending run keeps the one it has) and the membership test finds the first start point
// outside (force_first).  ns_force_prepare: a flagged run takes its forced update with this fill's bounds, or
// -- in a fill that builds none -- keeps its queue and waits for one that does (its own sequence is unchanged).
// Then the masked rebuild of the regular AND the forced updates together (the regular ones see the live set
// without the newest point: ns_swap_undo; the forced ones as it is, their old frames kept: ns_shadow_axes),
// pass 2 (the regular updates' runs select from their new bounds; the membership test is the reference's check
// that a forced update worked, and flags a regular update's run whose newest point lies outside its new
// bound: pending), and ns_reselect (entries behind the first one outside redraw their frames from the new
// volumes with the same variates).
int bounds_exact(dh_ctx* ctx, const NsPlan& p, NsArgs& a, const NsAux& x) {
  const int R = a.runs;
  hipStream_t s = ctx->stream;
  const bool starts = a.sampler != 3;  // (the uniform sampler starts nowhere: no membership test, no forced update)
  int rc = select_and_test(ctx, p, a, 1, a.pass_mode, a.force_first);
  if (rc) return rc;
  if (p.force_check && starts) hipLaunchKernelGGL(ns_force_prepare, dim3(1), dim3(kT), 0, s, a);
  if (a.rebuild_fill) {
    if (starts) hipLaunchKernelGGL(ns_shadow_axes, dim3(R, 16), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ns_swap_undo, dim3(R), dim3(64), 0, s, a);
    rc = build_bounds(ctx, p, a, x);
    if (rc) return rc;
    hipLaunchKernelGGL(ns_swap_undo, dim3(R), dim3(64), 0, s, a);
    rc = select_and_test(ctx, p, a, 2, a.pass_mode, nullptr);
    if (rc) return rc;
    if (starts) hipLaunchKernelGGL(ns_reselect, dim3(R), dim3(kT), 0, s, a);
  }
  a.fx_pass = 0;
  return DH_OK;
}

// The walkers of one fill: the unit-cube proposals of the runs without a bound yet, then the sampler's launch for the
// runs with one.  Leaves a.presorted set where the rwalk generator pass sorted the slots for this fill's ns_consume.
int walk_stage(dh_ctx* ctx, const NsPlan& p, NsArgs& a, const NsAux& x, int64_t fill, bool cube_phase) {
  const int R = a.runs, N = a.nlive, D = a.ndim, K = a.K, me = a.max_ells;
  int rc = DH_OK;
  if (cube_phase) {
    const dh::PhiloxKey key = ns_philox_key(p, STAGE_CUBE, fill);
    rc = unif_launch_runs(ctx, p.problem, R * K, D, D, 0, nullptr, nullptr, nullptr, nullptr, 0.0, nullptr, a.q_rng, 0,
                          a.r_u, a.r_v, a.r_logl, a.r_a, a.r_b, a.q_rng_out, a.run_loglstar, a.run_mode, K, MODE_CUBE,
                          p.philox ? &key : nullptr);
    if (rc) return rc;
  }
  if (a.sampler == 3) {
    // UniformBoundSampler.sample (internal_samplers.py:243-340): draws from the run's bound until one beats
    // the run's threshold; r_a = calls, r_b = flags
    if (p.fr_kind >= 0) {
      // the shapes sit on the runs' CURRENT live points (prepare_sampler: bound.ctrs = live_u every fill,
      // internal_samplers.py:232-233): each walking run's live set in its whitened frame, one launch
      rc = friends_whiten_runs_launch(ctx, R, a.live_u, x.fai, N, D, x.fct, a.run_mode, MODE_BOUND);
      if (rc) return rc;
      return unif_friends_launch_runs(ctx, p.problem, R * K, D, p.fr_kind, N, a.live_u, x.fct, a.b_axes, x.fai, x.bc,
                                      a.q_rng, a.r_u, a.r_v, a.r_logl, a.r_a, a.r_b, a.q_rng_out, a.run_loglstar,
                                      a.run_mode, K, MODE_BOUND);
    }
    const dh::PhiloxKey key = ns_philox_key(p, STAGE_UNIF, fill);
    return unif_launch_runs(ctx, p.problem, R * K, D, D, R * me, a.b_ctrs, a.b_axes, a.b_ams, a.b_cum, 0.0, x.bc, a.q_rng,
                            0, a.r_u, a.r_v, a.r_logl, a.r_a, a.r_b, a.q_rng_out, a.run_loglstar, a.run_mode, K,
                            MODE_BOUND, p.philox ? &key : nullptr, a.bound_multi ? a.nells : nullptr, me);
  }
  if (a.sampler == 0) {
    const dh::PhiloxKey key = ns_philox_key(p, STAGE_RWALK, fill);
    if (p.presort_ok) {
      ctx->presort.keys = a.live_logl;
      ctx->presort.out = x.presort;
      ctx->presort.n = N;
      ctx->presort.runs = R;
      ctx->presort.stride = a.presort_stride;
      ctx->presort.done = 0;
    }
    rc = rwalk_launch_runs(ctx, p.problem, R * K, D, D, a.q_u0, a.b_axes, p.n_frames, a.q_frame, 1.0, 0.0, a.walks, x.bc,
                           a.q_rng, a.r_u, a.r_v, a.r_logl, a.r_a, a.r_b, a.q_rng_out, a.run_loglstar, a.run_scale,
                           a.run_mode, K, MODE_BOUND, p.philox ? &key : nullptr);
    a.presorted = p.presort_ok && ctx->presort.done ? 1 : 0;
    ctx->presort = dh_ctx::PresortReq();
    return rc;
  }
  const dh::PhiloxKey key = ns_philox_key(p, STAGE_SLICE, fill);
  return slice_launch_runs(ctx, p.problem, R * K, D, a.sampler - 1, a.q_u0, a.b_axes, p.n_frames, a.q_frame, 1.0, 0.0,
                           a.walks, 0, a.q_rng, a.r_u, a.r_v, a.r_logl, a.r_a, a.r_b, a.r_c, a.r_d, a.q_rng_out,
                           a.run_loglstar, a.run_scale, a.run_mode, a.run_doubling, K, MODE_BOUND,
                           p.philox ? &key : nullptr);
}

// the read-back: records, final live points, and of the dead points' arrays what each run wrote
bool download(dh_ctx* ctx, const NsArgs& a, double* records, double* dead_logl, double* live_logl, double* dead_u,
              double* live_u, int32_t* dead_id, int32_t* dead_it, int32_t* dead_nc, int32_t* live_it) {
  const size_t R = (size_t)a.runs, N = (size_t)a.nlive, D = (size_t)a.ndim;
  hipStream_t s = ctx->stream;
  // `count` elements from element `at` on, where the caller wants the array
  auto get = [&](auto* host, const auto* dev, size_t at, size_t count, const char* what) {
    static_assert(sizeof *host == sizeof *dev, "element sizes");
    return !host || hip_ok(ctx, hipMemcpyAsync(host + at, dev + at, count * sizeof *host, hipMemcpyDeviceToHost, s), what);
  };
  if (!get(records, a.records, 0, R * 8, "D2H records") || !get(live_logl, a.live_logl, 0, R * N, "D2H live") ||
      !get(live_u, a.live_u, 0, R * N * D, "D2H live u") || !get(live_it, a.live_it, 0, R * N, "D2H live it"))
    return false;
  if (!dead_u && !dead_id && !dead_logl) return true;
  // only the niter rows each run produced (the caller's runs x max_iter (x ndim) buffers may be
  // far larger than what is touched here: 64 runs x 400 000 would be 300 MB of pageable copies)
  if (!hip_ok(ctx, hipStreamSynchronize(s), "sync")) return false;
  for (size_t r = 0; r < R; ++r) {
    long long nit = (long long)records[r * 8 + 2];
    if (nit > a.cap) nit = a.cap;
    if (nit <= 0) continue;
    const size_t o = r * (size_t)a.cap, n = (size_t)nit;
    if (!get(dead_logl, a.dead_logl, o, n, "D2H dead") || !get(dead_u, a.dead_u, o * D, n * D, "D2H dead u") ||
        !get(dead_id, a.dead_id, o, n, "D2H id") || !get(dead_it, a.dead_it, o, n, "D2H it") ||
        !get(dead_nc, a.dead_nc, o, n, "D2H nc"))
      return false;
  }
  return true;
}

// dh_ns_keep: a kept ensemble stores the samples and all four per-point arrays whether or not the caller downloads them
int ns_point_outputs(bool keep, int given) { return keep && given == 0 ? 4 : given; }

// the context takes over the call's allocation as "the kept ensemble" (merge.hip reads it through dh_kept)
void ns_keep_arrays(dh_ctx* ctx, const NsArgs& a, int problem, char* base, const double* records) {
  dh_kept& k = ctx->kept;
  k.base = base;
  k.problem = problem;
  k.runs = a.runs;
  k.nlive = a.nlive;
  k.ndim = a.ndim;
  k.cap = a.cap;
  k.dead_logl = a.dead_logl;
  k.live_logl = a.live_logl;
  k.dead_u = a.dead_u;
  k.live_u = a.live_u;
  k.dead_id = a.dead_id;
  k.dead_it = a.dead_it;
  k.dead_nc = a.dead_nc;
  k.live_it = a.live_it;
  k.niter.resize((size_t)a.runs);
  for (int r = 0; r < a.runs; ++r) {
    long long nit = (long long)records[(size_t)r * 8 + 2];
    k.niter[(size_t)r] = nit < 0 ? 0 : nit > a.cap ? a.cap : nit;
  }
}

// What a kept ensemble needs to be taken further (dh_ns_continue) or saved (dh_ns_state_export): the first call's plan,
// its arguments with the carved pointers, and the two things the host keeps between fills.  Owned by dh_kept::loop.
struct NsLoop {
  NsPlan p;
  NsArgs a;
  NsAux x;
  int64_t fill;     // the ENSEMBLE's fill counter: rebuild fills and Philox offsets are keyed on it
  bool cube_phase;
};

void ns_keep_loop(dh_ctx* ctx, const NsPlan& p, const NsArgs& a, const NsAux& x, int64_t fill, bool cube_phase) {
  ctx->kept.loop = std::shared_ptr<void>(new NsLoop{p, a, x, fill, cube_phase}, [](void* q) { delete (NsLoop*)q; });
}
NsLoop* ns_kept_loop(dh_ctx* ctx) { return ctx->kept.base ? (NsLoop*)ctx->kept.loop.get() : nullptr; }

// The fills from *fill up to fill_end, or until every run is over: the done-counter is read every eighth fill.
// h_state: [runs done, any run still in the unit-cube phase], as the caller knows them on entry.
int ns_fill_loop(dh_ctx* ctx, const NsPlan& p, NsArgs& a, const NsAux& x, int64_t* fill_io, int64_t fill_end,
                 int* h_state, bool* cube_io) {
  const int R = a.runs, K = a.K;
  hipStream_t s = ctx->stream;
  int64_t fill = *fill_io;
  bool cube_phase = *cube_io;
  int rc = DH_OK;
  while (fill < fill_end && h_state[0] < R) {
    for (int burst = 0; burst < 8 && fill < fill_end; ++burst, ++fill) {
      a.rebuild_fill = fill % p.every == 0 ? 1 : 0;
      hipLaunchKernelGGL(ns_prepare, dim3(1), dim3(kT), 0, s, a);
      rc = a.forced_exact ? bounds_exact(ctx, p, a, x) : bounds_late(ctx, p, a, x);
      if (!rc) rc = walk_stage(ctx, p, a, x, fill, cube_phase);
      if (rc) return rc;
      hipLaunchKernelGGL(ns_consume_for(K), dim3(R), dim3(kT), p.lds_cons, s, a);
      a.presorted = 0;
    }
    if (!hip_ok(ctx, hipMemcpyAsync(h_state, a.ndone, 8, hipMemcpyDeviceToHost, s), "D2H ndone") ||
        !hip_ok(ctx, hipStreamSynchronize(s), "sync"))
      return DH_ERR_HIP;
    if (!h_state[1]) cube_phase = false;  // (as of the last ns_prepare: every run has its first bound)
  }
  *fill_io = fill;
  *cube_io = cube_phase;
  return DH_OK;
}

void ns_prof_print(dh_ctx* ctx, const long long* prof, long long fills) {
  long long h[32];
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipMemcpy(h, prof, sizeof h, hipMemcpyDeviceToHost);
  fprintf(stderr, "ns_consume cycles (run 0, %lld fills): load+sort %lld | walk %lld | scan %lld | replay+state %lld | dead %lld | live store %lld ; fills integrated serially (all runs): %lld new plateau + %lld carried ; queues of run 0 left to the serial walk: %lld ; parallel walk: ranks %lld | counts %lld | scan+pick %lld | low ranks %lld | merge %lld | slots %lld\n",
          fills, h[0], h[1], h[2], h[3], h[4], h[5], h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15], h[7]);
  fprintf(stderr, "  load+sort = live keys %lld | sort %lld | queue + sums %lld ; scan = ties %lld | weights + ln Z scan %lld | stop %lld | information %lld | rest %lld\n", h[16], h[17], h[0], h[18], h[19], h[20], h[21], h[2]);
}
}  // namespace

extern "C" {

// see include/dynhip.h
int dh_ns_consume(dh_ctx* ctx, int runs, int nlive, int queue_size, double dlogz, double* live_logl,
                  const double* q_logl, const int32_t* q_ncalls, double* state, double* dead_logl,
                  int32_t* dead_slot, int32_t* dead_src, int32_t* ndead, int32_t* stopped, int32_t* live_it,
                  int32_t* dead_it, int32_t* dead_nc, double* plateau) {
  DH_CHECK_CTX(ctx);
  const bool want_pt = live_it || dead_it || dead_nc;
  if (want_pt && !(live_it && dead_it && dead_nc))
    return fail(ctx, DH_ERR_ARG, "ns_consume: live_it, dead_it and dead_nc come together");
  if (runs < 1 || nlive < 4 || queue_size < 1 || !live_logl || !q_logl || !q_ncalls || !state || !dead_logl ||
      !dead_slot || !dead_src || !ndead || !stopped)
    return fail(ctx, DH_ERR_ARG, "ns_consume: bad arguments");
  const int R = runs, N = nlive, K = queue_size;
  if (K > kEPTMax * kT) return fail(ctx, DH_ERR_ARG, "ns_consume: queue_size %d > %d", K, kEPTMax * kT);
  // slots travel as 16-bit indices; beyond the register sort's 32 keys per thread (or the LDS) the consumption works on
  // the K + 1 smallest live points (ns_consume_compact)
  if (N > 65535) return fail(ctx, DH_ERR_ARG, "ns_consume: nlive %d > 65535", N);
  const size_t lds_max = ns_consume_lds(N, K);
  if (lds_max > kNsLdsMax) return fail(ctx, DH_ERR_ARG, "ns_consume: nlive/queue too large for LDS");
  NsArgs a{};
  a.serial_walk = ns_serial_walk();
  a.runs = R;
  a.nlive = N;
  a.ndim = 0;  // log-likelihoods only: no coordinates travel
  a.K = K;
  a.walks = 1;
  a.cap = K;
  a.dlogz = dlogz;
  a.dead_rel = 1;
  dh_stage::NsConsumeBuf b;
  int rc = arena_carve(ctx, [&](dh_stage::Carver& c) {
    dh_stage::carve_ns_consume(c, b, (size_t)R, (size_t)N, (size_t)K, sizeof(NsRun), want_pt);
  });
  if (rc) return rc;
  std::vector<NsRun> st((size_t)R);
  for (int r = 0; r < R; ++r) {
    NsRun& x = st[(size_t)r];
    memset(&x, 0, sizeof x);
    const double* sv = state + (size_t)r * 8;
    x.logvol = sv[0];
    x.logz = sv[1];
    x.h = sv[2];
    x.logzvar = sv[3];
    x.dead_prev = sv[4];
    x.it = (long long)sv[5];
    x.ncall = (long long)sv[6];
    x.mode = MODE_CUBE;  // the queue's ncalls come from q_ncalls; no sampler tuning
    x.scale = 1.0;
    if (plateau) {  // plateau mode carried from the previous call (sampler.py:1112-1127)
      x.pcount = (int)plateau[(size_t)r * 2];
      x.plogdvol = plateau[(size_t)r * 2 + 1];
    }
  }
  a.st = (NsRun*)b.st;
  a.live_logl = b.live_logl;
  a.dead_logl = b.dead_logl;
  a.r_logl = b.r_logl;
  a.r_a = b.r_a;
  a.trace_slot = b.trace_slot;
  a.trace_src = b.trace_src;
  a.trace_n = b.trace_n;
  a.ndone = b.ndone;
  a.bstatus = b.bstatus;
  a.live_it = b.live_it;
  a.dead_id = b.dead_id;
  a.dead_it = b.dead_it;
  a.dead_nc = b.dead_nc;
  if (!arena_fill(ctx, a.st, st.data(), (size_t)R) || !arena_fill(ctx, b.live_logl, live_logl, (size_t)R * N) ||
      !arena_fill(ctx, b.r_logl, q_logl, (size_t)R * K) || !arena_fill(ctx, b.r_a, q_ncalls, (size_t)R * K) ||
      (want_pt && !arena_fill(ctx, b.live_it, live_it, (size_t)R * N)))
    return DH_ERR_NOMEM;
  hipStream_t s = ctx->stream;
  if (!hip_ok(ctx, hipMemsetAsync(a.ndone, 0, dh_stage::kNsDoneInts * 4, s), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(a.bstatus, 0, (size_t)R * 4, s), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(a.trace_n, 0, (size_t)R * 8, s), "memset"))
    return DH_ERR_HIP;
  if (!ns_set_lds(ctx, K, lds_max, false)) return DH_ERR_HIP;
  hipLaunchKernelGGL(ns_start, dim3(R), dim3(kT), 0, s, a);  // loglstar = min, lmax = max of live_logl
  hipLaunchKernelGGL(ns_consume_for(K), dim3(R), dim3(kT), lds_max, s, a);
  if (!hip_ok(ctx, hipGetLastError(), "ns_consume launch")) return DH_ERR_HIP;
  std::vector<int> tn((size_t)R * 2);
  if (!down(ctx, st.data(), a.st, (size_t)R) || !down(ctx, live_logl, a.live_logl, (size_t)R * N) ||
      !down(ctx, dead_logl, a.dead_logl, (size_t)R * K) || !down(ctx, (int*)dead_slot, a.trace_slot, (size_t)R * K) ||
      !down(ctx, (int*)dead_src, a.trace_src, (size_t)R * K) || !down(ctx, tn.data(), a.trace_n, (size_t)R * 2))
    return DH_ERR_HIP;
  if (want_pt && (!down(ctx, (int*)live_it, a.live_it, (size_t)R * N) || !down(ctx, (int*)dead_it, a.dead_it, (size_t)R * K) ||
                  !down(ctx, (int*)dead_nc, a.dead_nc, (size_t)R * K)))
    return DH_ERR_HIP;
  if ((rc = dh_sync(ctx))) return rc;
  for (int r = 0; r < R; ++r) {
    const NsRun& x = st[(size_t)r];
    double* sv = state + (size_t)r * 8;
    sv[0] = x.logvol;
    sv[1] = x.logz;
    sv[2] = x.h;
    sv[3] = x.logzvar;
    sv[4] = x.dead_prev;
    sv[5] = (double)x.it;
    sv[6] = (double)x.ncall;
    sv[7] = x.loglstar;  // the current worst live point
    if (plateau) {
      plateau[(size_t)r * 2] = (double)x.pcount;
      plateau[(size_t)r * 2 + 1] = x.plogdvol;
    }
    ndead[r] = tn[(size_t)r * 2];
    stopped[r] = tn[(size_t)r * 2 + 1];
  }
  return DH_OK;
}

int dh_ns_set_option(dh_ctx* ctx, int key, double value) {
  DH_CHECK_CTX(ctx);
  if (key < 0 || key >= DH_NS_OPT_COUNT) return fail(ctx, DH_ERR_ARG, "ns option %d", key);
  ctx->ns_opt[key] = value;
  return DH_OK;
}

int dh_ns_keep(dh_ctx* ctx, int on) {
  DH_CHECK_CTX(ctx);
  ctx->ns_keep = on ? 1 : 0;
  return DH_OK;
}

int dh_ns_release(dh_ctx* ctx) {
  DH_CHECK_CTX(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  kept_free(ctx);
  return DH_OK;
}

int dh_ns_set_boundary(dh_ctx* ctx, int ndim, const int8_t* bc) {
  DH_CHECK_CTX(ctx);
  // validate first: a rejected call leaves the installed flags as they were
  if (bc && ndim > 0) {
    for (int i = 0; i < ndim; ++i)
      if (bc[i] != DH_BC_HARD && bc[i] != DH_BC_PERIODIC && bc[i] != DH_BC_REFLECT)
        return fail(ctx, DH_ERR_ARG, "ns boundary flag %d of dimension %d", (int)bc[i], i);
    ctx->ns_bc.assign(bc, bc + ndim);
  } else {
    ctx->ns_bc.clear();
  }
  return DH_OK;
}

int dh_ns_ensemble(dh_ctx* ctx, int problem, int runs, int nlive, int ndim, int queue_size, int sampler,
                   int walks, int bound, int rebuild_sync, double dlogz, double enlarge, int64_t max_fills,
                   int64_t max_iter,
                   const uint32_t* entropy_words, int n_words, uint32_t first_run, double* records,
                   double* dead_logl_out, double* live_logl_out, double* dead_u_out, double* live_u_out,
                   int64_t* n_fills_out, int32_t* dead_id_out, int32_t* dead_it_out, int32_t* dead_nc_out,
                   int32_t* live_it_out, int bootstrap, int rebuild_every) {
  DH_CHECK_CTX(ctx);
  // Options and boundary flags are one-shot: this call takes them and the context forgets them, whichever way the call
  // ends, so that nothing set for one ensemble (maxiter, add_live = 0, forced_exact, periodic coordinates) can leak
  // into a later one whose caller set nothing.
  struct NsOneShot {
    dh_ctx* c;
    double opt[DH_NS_OPT_COUNT];
    std::vector<int8_t> bc;
    int keep;
    explicit NsOneShot(dh_ctx* cc) : c(cc), keep(cc->ns_keep) {
      c->ns_keep = 0;
      for (int i = 0; i < DH_NS_OPT_COUNT; ++i) {
        opt[i] = c->ns_opt[i];
        c->ns_opt[i] = __builtin_nan("");
      }
      bc.swap(c->ns_bc);
    }
  } shot(ctx);
  NsPlan p;
  int rc = ns_plan(ctx, shot.opt, shot.bc.size(), problem, runs, nlive, ndim, queue_size, sampler, walks, bound,
                   rebuild_sync, dlogz, enlarge, max_fills, max_iter, entropy_words, n_words, first_run, records,
                   dead_u_out != nullptr || shot.keep, ns_point_outputs(shot.keep != 0, !!dead_id_out + !!dead_it_out + !!dead_nc_out + !!live_it_out),
                   bootstrap, rebuild_every, &p);
  if (rc) return rc;
  p.keep = shot.keep != 0;
  p.n_words = n_words;
  p.have_bc = !shot.bc.empty();
  if (shot.keep) kept_free(ctx);  // a later keep replaces the earlier one (before this call's allocation)
  NsArgs a = p.a;
  NsAux x;
  const int R = a.runs, N = a.nlive, D = a.ndim, K = a.K;
  // ---- one allocation for all state ----
  NsCarver sizes{ctx, nullptr};
  ns_arrays(sizes, p, a, x, n_words, !shot.bc.empty());
  char* base = nullptr;
  (void)hipSetDevice(ctx->device);
  if (!hip_ok(ctx, hipMalloc((void**)&base, sizes.off), "hipMalloc(ns state)")) return DH_ERR_NOMEM;
  hipStream_t s = ctx->stream;
  int64_t kept_fill = 0;
  bool kept_cube = true;
  auto cleanup = [&](int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    if (shot.keep && rc == DH_OK) {
      ns_keep_arrays(ctx, a, problem, base, records);
      ns_keep_loop(ctx, p, a, x, kept_fill, kept_cube);
      return rc;
    }
    (void)hipFree(base);
    return rc;
  };
  NsCarver carve{ctx, base};
  ns_arrays(carve, p, a, x, n_words, !shot.bc.empty());
  if (!carve.ok ||
      (x.bc && !hip_ok(ctx, hipMemcpyAsync(x.bc, shot.bc.data(), (size_t)D, hipMemcpyHostToDevice, s), "H2D bc")) ||
      !hip_ok(ctx, hipMemcpyAsync(x.ent, entropy_words, (size_t)n_words * 4, hipMemcpyHostToDevice, s), "H2D"))
    return cleanup(DH_ERR_HIP);
  hipLaunchKernelGGL(ns_init, dim3(R), dim3(kT), 0, s, a, x.ent, n_words, first_run);
  // (friends) the metric before the first update: RadFriends(ndim) / SupFriends(ndim) with cov=None, the identity
  if (p.fr_kind >= 0)
    hipLaunchKernelGGL(ns_fr_eye, dim3((unsigned)(((size_t)R * D * D + 255) / 256)), dim3(256), 0, s, a.b_ams, R, D);
  rc = eval_launch_dev(ctx, problem, R * N, a.live_u, a.live_v, a.live_logl);
  if (rc) return cleanup(rc);
  if (!ns_set_lds(ctx, K, p.lds_cons > p.lds_fin ? p.lds_cons : p.lds_fin, true)) return cleanup(DH_ERR_HIP);
  hipLaunchKernelGGL(ns_start, dim3(R), dim3(kT), 0, s, a);
  if (!hip_ok(ctx, hipGetLastError(), "ns_start launch")) return cleanup(DH_ERR_HIP);
  int64_t fill = 0;
  int h_state[2] = {0, 1};  // [runs done, any run still in the unit-cube phase]
  bool cube_phase = true;
  rc = ns_fill_loop(ctx, p, a, x, &fill, p.fills_cap, h_state, &cube_phase);
  if (rc) return cleanup(rc);
  kept_fill = fill;
  kept_cube = cube_phase;
  hipLaunchKernelGGL(ns_finish, dim3(R), dim3(kT), p.lds_fin, s, a);
  if (!hip_ok(ctx, hipGetLastError(), "ns launch") ||
      !download(ctx, a, records, dead_logl_out, live_logl_out, dead_u_out, live_u_out, dead_id_out, dead_it_out,
                dead_nc_out, live_it_out))
    return cleanup(DH_ERR_HIP);
  if (n_fills_out) *n_fills_out = fill;
  if (a.prof) ns_prof_print(ctx, a.prof, (long long)fill);
  return cleanup(DH_OK);
}

// see include/dynhip.h and the kernels' header comment (ns_batch_init ... ns_batch_start)
int dh_ns_batch(dh_ctx* ctx, int problem, int runs, int nlive_new, int ndim, int queue_size, int sampler, int walks,
                int bound, double dlogz, double enlarge, int64_t max_fills, int64_t max_iter,
                const uint32_t* entropy_words, int n_words, uint32_t first_run, const double* seed_u,
                const double* seed_logl, double logl_min, const double* start, double* records,
                double* dead_logl_out, double* live_logl_out, double* dead_u_out, double* live_u_out,
                int64_t* n_fills_out, int32_t* dead_id_out, int32_t* dead_it_out, int32_t* dead_nc_out,
                int32_t* live_it_out, int bootstrap, int rebuild_every, double* start_u_out, double* start_logl_out,
                int32_t* start_nc_out, int64_t* seed_ncall_out, uint64_t* seed_rng_out) {
  DH_CHECK_CTX(ctx);
  // one-shot options, boundary flags and the keep switch, as for dh_ns_ensemble: taken and forgotten however this ends
  double opt[DH_NS_OPT_COUNT];
  for (int i = 0; i < DH_NS_OPT_COUNT; ++i) {
    opt[i] = ctx->ns_opt[i];
    ctx->ns_opt[i] = __builtin_nan("");
  }
  std::vector<int8_t> bc;
  bc.swap(ctx->ns_bc);
  const int keep = ctx->ns_keep;
  ctx->ns_keep = 0;
  // ---- plan: everything that can be refused is refused before the device is touched ----
  namespace nb = dh_nsb;
  const nb::Request req = {runs,     nlive_new, ndim,   queue_size, sampler,
                           bound,    keep,      logl_min, std::isnan(opt[DH_NS_OPT_LOGL_MAX]) ? INFINITY : opt[DH_NS_OPT_LOGL_MAX],
                           seed_u,   seed_logl, start};
  long long where = -1;
  const int verdict = nb::check(req, &where);
  if (verdict != nb::V_OK) return fail(ctx, DH_ERR_ARG, "ns_batch: %s (index %lld)", nb::verdict_text(verdict), where);
  if (!seed_ncall_out) return fail(ctx, DH_ERR_ARG, "ns_batch: seed_ncall_out is required");
  NsPlan p;
  int rc = ns_plan(ctx, opt, bc.size(), problem, runs, nlive_new, ndim, queue_size, sampler, walks, bound, 0, dlogz,
                   enlarge, max_fills, max_iter, entropy_words, n_words, first_run, records, dead_u_out != nullptr,
                   !!dead_id_out + !!dead_it_out + !!dead_nc_out + !!live_it_out, bootstrap, rebuild_every, &p);
  if (rc) return rc;
  p.keep = false;
  p.n_words = n_words;
  p.have_bc = !bc.empty();
  const nb::Sizes sz = nb::sizes(runs, nlive_new, ndim, queue_size);
  NsArgs a = p.a;
  NsAux x;
  x.batch = true;
  const int R = a.runs, N = a.nlive, D = a.ndim, K = a.K;
  NsCarver sizes{ctx, nullptr};
  ns_arrays(sizes, p, a, x, n_words, p.have_bc);
  {
    // the plan's size of the seeding arrays is what the layout carves for them
    NsAux plain;
    NsArgs a0 = p.a;
    NsCarver without{ctx, nullptr};
    ns_arrays(without, p, a0, plain, n_words, p.have_bc);
    if (sizes.off - without.off != sz.stage_bytes)
      return fail(ctx, DH_ERR_ARG, "ns_batch: the plan sizes the seeding arrays at %zu bytes, the layout at %zu",
                  sz.stage_bytes, sizes.off - without.off);
  }
  char* base = nullptr;
  (void)hipSetDevice(ctx->device);
  if (!hip_ok(ctx, hipMalloc((void**)&base, sizes.off), "hipMalloc(ns batch state)")) return DH_ERR_NOMEM;
  hipStream_t s = ctx->stream;
  auto cleanup = [&](int code) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(base);
    return code;
  };
  NsCarver carve{ctx, base};
  ns_arrays(carve, p, a, x, n_words, p.have_bc);
  NsSeed sd = x.seed;
  sd.logl_min = logl_min;
  const size_t RN = (size_t)R * N;
  // the seeds are the strands' live sets: stored values, not evaluated again (their v is never read: the seeds leave
  // before any of them can die)
  if (!carve.ok ||
      (x.bc && !hip_ok(ctx, hipMemcpyAsync(x.bc, bc.data(), (size_t)D, hipMemcpyHostToDevice, s), "H2D bc")) ||
      !hip_ok(ctx, hipMemcpyAsync(x.ent, entropy_words, (size_t)n_words * 4, hipMemcpyHostToDevice, s), "H2D") ||
      !hip_ok(ctx, hipMemcpyAsync(a.live_u, seed_u, RN * D * 8, hipMemcpyHostToDevice, s), "H2D seed u") ||
      !hip_ok(ctx, hipMemcpyAsync(a.live_logl, seed_logl, RN * 8, hipMemcpyHostToDevice, s), "H2D seed logl") ||
      !hip_ok(ctx, hipMemcpyAsync(sd.start, start, (size_t)R * 6 * 8, hipMemcpyHostToDevice, s), "H2D start") ||
      !hip_ok(ctx, hipMemsetAsync(a.live_v, 0, RN * D * 8, s), "memset"))
    return cleanup(DH_ERR_HIP);
  if (!ns_set_lds(ctx, K, p.lds_cons > p.lds_fin ? p.lds_cons : p.lds_fin, true)) return cleanup(DH_ERR_HIP);
  // ---- phase S: the bound on the seeds, once; then the seed fills at the fixed threshold ----
  hipLaunchKernelGGL(ns_batch_init, dim3(1), dim3(kT), 0, s, a, sd, x.ent, n_words, first_run);
  rc = build_bounds(ctx, p, a, x);
  if (rc) return cleanup(rc);
  // Exactly ceil(nlive_new / K) fills, enqueued without a look at the device.  No membership test of the start points:
  // they are seeds, and the bound was built on the seeds (and only ever enlarged), so every one lies inside it and
  // the forced update the test exists for cannot be due.  An entry is lost only to a failed slice; a strand whose
  // staging set is short after these fills fails (ns_batch_start).
  for (int f = 0; f < sz.seed_fills; ++f) {
    hipLaunchKernelGGL(ns_seed_prepare, dim3(1), dim3(kT), 0, s, a, sd);
    a.fx_pass = 0;
    hipLaunchKernelGGL(ns_select, dim3(R), dim3(kT), 0, s, a);
    if (a.sampler != 3)
      hipLaunchKernelGGL(ns_gather, dim3((unsigned)(((size_t)R * K * D + 255) / 256)), dim3(256), 0, s, a);
    rc = walk_stage(ctx, p, a, x, f, false);
    if (rc) return cleanup(rc);
    // (rwalk: walk_stage lets the generator pass presort the live ln L beside the walk, as in every fill of the loop;
    // here the order is the seeds' and nothing consumes it -- a few workgroups of wasted work per seed fill, kept
    // rather than giving walk_stage a second form)
    a.presorted = 0;
    hipLaunchKernelGGL(ns_seed_consume, dim3(R), dim3(kT), 0, s, a, sd);
  }
  hipLaunchKernelGGL(ns_batch_start, dim3(R), dim3(kT), 0, s, a, sd);
  if (!hip_ok(ctx, hipGetLastError(), "ns_batch_start launch")) return cleanup(DH_ERR_HIP);
  // ---- from here the loop dh_ns_ensemble runs: its fills count from 0 ----
  int64_t fill = 0;
  int l_state[2] = {0, 0};
  bool cube_phase = false;
  rc = ns_fill_loop(ctx, p, a, x, &fill, p.fills_cap, l_state, &cube_phase);
  if (rc) return cleanup(rc);
  hipLaunchKernelGGL(ns_finish, dim3(R), dim3(kT), p.lds_fin, s, a);
  if (!hip_ok(ctx, hipGetLastError(), "ns launch") ||
      !download(ctx, a, records, dead_logl_out, live_logl_out, dead_u_out, live_u_out, dead_id_out, dead_it_out,
                dead_nc_out, live_it_out))
    return cleanup(DH_ERR_HIP);
  static_assert(sizeof(long long) == sizeof(int64_t), "seed_ncall");
  if (!down(ctx, (long long*)seed_ncall_out, sd.ncall, (size_t)R) ||
      (start_u_out && !down(ctx, start_u_out, sd.u, RN * D)) ||
      (start_logl_out && !down(ctx, start_logl_out, sd.logl, RN)) ||
      (start_nc_out && !down(ctx, (int*)start_nc_out, sd.nc, RN)) ||
      (seed_rng_out && !down(ctx, seed_rng_out, sd.rng, (size_t)R * 4)))
    return cleanup(DH_ERR_HIP);
  if (n_fills_out) *n_fills_out = fill;
  return cleanup(DH_OK);
}

}  // extern "C"

// ---- a kept ensemble between two calls: dh_ns_continue, dh_ns_state_size / _export / _import (ns_state.h) ----------
namespace {
namespace nst = dh_ns_state;

enum { ENT_FIXED, ENT_DEAD, ENT_SKIP };
// How the image treats the array at `ptr`: the dead-point arrays by rows (*elem bytes each); not at all the workspaces
// that a fill or ns_finish writes before it reads them; everything else whole.
int ns_entry_kind(const NsArgs& a, const NsAux& x, const void* ptr, size_t* elem) {
  *elem = 0;
  if (ptr == a.dead_logl) return *elem = 8, ENT_DEAD;
  if (ptr == a.dead_u) return *elem = 8 * (size_t)a.ndim, ENT_DEAD;
  if (ptr == a.dead_id || ptr == a.dead_it || ptr == a.dead_nc) return *elem = 4, ENT_DEAD;
  if (ptr == a.fin_ws || ptr == x.boot_ws || ptr == x.fr_ws || ptr == x.presort || ptr == a.prof || ptr == x.fr_mask ||
      ptr == x.fr_scratch || ptr == a.records || ptr == x.seed.u || ptr == x.seed.v || ptr == x.seed.logl ||
      ptr == x.seed.nc || ptr == x.seed.n || ptr == x.seed.rej || ptr == x.seed.ncall || ptr == x.seed.rng ||
      ptr == x.seed.start)
    return ENT_SKIP;
  return ENT_FIXED;
}

// the arrays of plan p at capacity scalars.cap, carved from `base` (null: the total size alone); fresh: a new
// allocation, which takes the arrays' initial fills
struct NsLayout {
  NsArgs a;
  NsAux x;
  std::vector<NsEntry> list;
  std::vector<int> kind;
  std::vector<size_t> elem;
  size_t bytes = 0, fixed_bytes = 0, row_bytes = 0;
  bool ok = true;
};
void ns_layout(dh_ctx* ctx, const NsPlan& p, const NsArgs& scalars, char* base, bool fresh, NsLayout* out) {
  out->a = scalars;
  out->list.clear();
  NsCarver c{ctx, base};
  c.list = &out->list;
  c.fills = fresh;  // (an ensemble in use keeps what its arrays hold)
  ns_arrays(c, p, out->a, out->x, p.n_words, p.have_bc);
  out->bytes = c.off;
  out->ok = c.ok;
  out->kind.clear();
  out->elem.clear();
  out->fixed_bytes = out->row_bytes = 0;
  if (!base) return;  // (sizes alone: without pointers no array can be told from another)
  for (const NsEntry& e : out->list) {
    size_t el;
    const int k = ns_entry_kind(out->a, out->x, base + e.off, &el);
    out->kind.push_back(k);
    out->elem.push_back(el);
    if (k == ENT_FIXED) out->fixed_bytes += nst::pad8(e.bytes);
    if (k == ENT_DEAD) out->row_bytes += el;
  }
}

// the header and the rows of the kept ensemble as it stands (reads the runs' states back)
int ns_image_header(dh_ctx* ctx, NsLoop* L, const NsLayout& lay, nst::Header* h, std::vector<int64_t>* rows) {
  const NsArgs& a = L->a;
  std::vector<NsRun> stv((size_t)a.runs);
  if (!down(ctx, stv.data(), a.st, (size_t)a.runs) || !hip_ok(ctx, hipStreamSynchronize(ctx->stream), "sync"))
    return DH_ERR_HIP;
  rows->resize((size_t)a.runs);
  for (int r = 0; r < a.runs; ++r) {
    const long long it = stv[(size_t)r].it;
    (*rows)[(size_t)r] = it < 0 ? 0 : it > a.cap ? a.cap : it;
  }
  memset(h, 0, sizeof *h);
  h->magic = nst::kMagic;
  h->version = DH_VERSION;
  h->sizeof_run = sizeof(NsRun);
  h->header_bytes = sizeof(nst::Header);
  h->plan_bytes = sizeof(NsPlan);
  h->runs = a.runs;
  h->nlive = a.nlive;
  h->ndim = a.ndim;
  h->queue_size = a.K;
  h->cap = a.cap;
  h->fill = L->fill;
  h->cube_phase = L->cube_phase ? 1 : 0;
  h->n_words = L->p.n_words;
  h->have_bc = L->p.have_bc ? 1 : 0;
  h->row_bytes = (int32_t)lay.row_bytes;
  h->fixed_bytes = lay.fixed_bytes;
  std::vector<uint32_t> elems;
  for (size_t i = 0; i < lay.list.size(); ++i)
    if (lay.kind[i] == ENT_DEAD) elems.push_back((uint32_t)lay.elem[i]);
  h->total_bytes = nst::image_bytes(*h, rows->data(), (int)elems.size(), elems.data());
  return DH_OK;
}

// the plan as the image carries it: the call's scalars, no pointers
NsPlan ns_plan_image(const NsLoop& L) {
  NsPlan p = L.p;
  p.a = L.a;
  NsAux x;
  NsCarver none{nullptr, nullptr};
  ns_arrays(none, p, p.a, x, p.n_words, p.have_bc);  // (a carver without a base nulls every pointer)
  p.a.prof = nullptr;
  p.a.presort = nullptr;
  return p;
}
}  // namespace

extern "C" {

int dh_ns_continue(dh_ctx* ctx, double dlogz, int64_t max_fills, double* records, double* dead_logl_out,
                   double* live_logl_out, double* dead_u_out, double* live_u_out, int64_t* n_fills_out,
                   int32_t* dead_id_out, int32_t* dead_it_out, int32_t* dead_nc_out, int32_t* live_it_out,
                   int32_t* rest_out) {
  DH_CHECK_CTX(ctx);
  // one-shot, as for dh_ns_ensemble: the context forgets the options however this call ends
  double opt[DH_NS_OPT_COUNT];
  for (int i = 0; i < DH_NS_OPT_COUNT; ++i) {
    opt[i] = ctx->ns_opt[i];
    ctx->ns_opt[i] = __builtin_nan("");
  }
  const bool had_bc = !ctx->ns_bc.empty();
  ctx->ns_bc.clear();
  ctx->ns_keep = 0;  // (the ensemble stays kept; the switch is not left armed for a later dh_ns_ensemble)
  NsLoop* L = ns_kept_loop(ctx);
  if (!L) return fail(ctx, DH_ERR_ARG, "ns_continue: the context holds no kept ensemble (dh_ns_keep + dh_ns_ensemble)");
  if (!records) return fail(ctx, DH_ERR_ARG, "ns_continue: records is required");
  if (had_bc || !std::isnan(opt[DH_NS_OPT_UPDATE_INTERVAL]) || !std::isnan(opt[DH_NS_OPT_FIRST_MIN_NCALL]) ||
      !std::isnan(opt[DH_NS_OPT_FIRST_MIN_EFF]) || !std::isnan(opt[DH_NS_OPT_FORCED_EXACT]))
    return fail(ctx, DH_ERR_ARG, "ns_continue: the update interval, first_update, forced_exact and the boundary flags "
                                 "are fixed by the ensemble's first call");
  const NsPlan& p = L->p;
  NsArgs a = L->a;
  const NsAux& x = L->x;
  const int R = a.runs, K = a.K;
  a.dlogz = dlogz;
  a.maxiter = a.maxcall = -1;
  a.logl_max = INFINITY;
  a.add_live = 1;
  if (!std::isnan(opt[DH_NS_OPT_MAXITER])) a.maxiter = (long long)llround(opt[DH_NS_OPT_MAXITER]);
  if (!std::isnan(opt[DH_NS_OPT_MAXCALL])) a.maxcall = (long long)llround(opt[DH_NS_OPT_MAXCALL]);
  if (!std::isnan(opt[DH_NS_OPT_LOGL_MAX])) a.logl_max = opt[DH_NS_OPT_LOGL_MAX];
  if (!std::isnan(opt[DH_NS_OPT_ADD_LIVE])) a.add_live = opt[DH_NS_OPT_ADD_LIVE] != 0.0 ? 1 : 0;
  if (a.maxcall >= 0 && a.maxcall < a.nlive)
    return fail(ctx, DH_ERR_ARG, "ns_continue: maxcall %lld below the %d calls of the initial live points", a.maxcall, a.nlive);
  a.presorted = 0;
  a.fx_pass = 0;
  (void)hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  if (!ns_set_lds(ctx, K, p.lds_cons > p.lds_fin ? p.lds_cons : p.lds_fin, true)) return DH_ERR_HIP;
  // which runs go on (ns_resume), then the fills that a stop rule cut short, once more and whole: ahead of the
  // first ns_prepare, which must see the call count the uninterrupted run had at that fill's end
  if (!hip_ok(ctx, hipMemsetAsync(a.ndone, 0, 64, s), "memset")) return DH_ERR_HIP;
  hipLaunchKernelGGL(ns_resume, dim3(R), dim3(kT), 0, s, a);
  a.replay = 1;
  hipLaunchKernelGGL(ns_consume_for(K), dim3(R), dim3(kT), p.lds_cons, s, a);
  a.replay = 0;
  int h_state[2] = {0, 1};
  std::vector<int> rest((size_t)R);
  if (!hip_ok(ctx, hipGetLastError(), "ns_resume launch") || !down(ctx, h_state, a.ndone, 2) ||
      !down(ctx, rest.data(), a.rest, (size_t)R) || !hip_ok(ctx, hipStreamSynchronize(s), "sync"))
    return DH_ERR_HIP;
  const int64_t fill0 = L->fill;
  int64_t fill = fill0;
  bool cube_phase = h_state[1] != 0;
  const int64_t budget = max_fills > 0 ? max_fills : 1000000;
  int rc = ns_fill_loop(ctx, p, a, x, &fill, fill0 + budget, h_state, &cube_phase);
  // whatever happens below, the fills are spent: the ensemble's counter moves with them
  L->fill = fill;
  L->cube_phase = cube_phase;
  L->a = a;
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  hipLaunchKernelGGL(ns_finish, dim3(R), dim3(kT), p.lds_fin, s, a);
  if (!hip_ok(ctx, hipGetLastError(), "ns launch") ||
      !download(ctx, a, records, dead_logl_out, live_logl_out, dead_u_out, live_u_out, dead_id_out, dead_it_out,
                dead_nc_out, live_it_out) ||
      !hip_ok(ctx, hipStreamSynchronize(s), "sync"))
    return DH_ERR_HIP;
  for (int r = 0; r < R; ++r) {
    long long nit = (long long)records[(size_t)r * 8 + 2];
    ctx->kept.niter[(size_t)r] = nit < 0 ? 0 : nit > a.cap ? a.cap : nit;
    if (rest_out) rest_out[r] = rest[(size_t)r];
  }
  if (n_fills_out) *n_fills_out = fill - fill0;
  return DH_OK;
}

int dh_ns_state_size(dh_ctx* ctx, uint64_t* bytes) {
  DH_CHECK_CTX(ctx);
  NsLoop* L = ns_kept_loop(ctx);
  if (!L || !bytes) return fail(ctx, DH_ERR_ARG, "ns_state_size: no kept ensemble");
  NsLayout lay;
  ns_layout(ctx, L->p, L->a, ctx->kept.base, false, &lay);  // (the pointers it hands out are the ensemble's own: nothing is written)
  nst::Header h;
  std::vector<int64_t> rows;
  const int rc = ns_image_header(ctx, L, lay, &h, &rows);
  if (rc) return rc;
  *bytes = h.total_bytes;
  return DH_OK;
}

int dh_ns_state_export(dh_ctx* ctx, void* buf, uint64_t bytes) {
  DH_CHECK_CTX(ctx);
  NsLoop* L = ns_kept_loop(ctx);
  if (!L || !buf) return fail(ctx, DH_ERR_ARG, "ns_state_export: no kept ensemble");
  NsLayout lay;
  ns_layout(ctx, L->p, L->a, ctx->kept.base, false, &lay);
  nst::Header h;
  std::vector<int64_t> rows;
  int rc = ns_image_header(ctx, L, lay, &h, &rows);
  if (rc) return rc;
  if (bytes < h.total_bytes)
    return fail(ctx, DH_ERR_ARG, "ns_state_export: %llu bytes given, the image takes %llu", (unsigned long long)bytes,
                (unsigned long long)h.total_bytes);
  char* out = (char*)buf;
  memset(out, 0, (size_t)h.total_bytes);
  size_t at = 0;
  memcpy(out, &h, sizeof h);
  at += sizeof h;
  const NsPlan pi = ns_plan_image(*L);
  memcpy(out + at, &pi, sizeof pi);
  at += (size_t)nst::pad8(sizeof pi);
  memcpy(out + at, rows.data(), rows.size() * 8);
  at += rows.size() * 8;
  const size_t cap = (size_t)L->a.cap;
  hipStream_t s = ctx->stream;
  for (size_t i = 0; i < lay.list.size(); ++i) {
    const char* dev = ctx->kept.base + lay.list[i].off;
    if (lay.kind[i] == ENT_FIXED) {
      if (!hip_ok(ctx, hipMemcpyAsync(out + at, dev, lay.list[i].bytes, hipMemcpyDeviceToHost, s), "D2H state")) return DH_ERR_HIP;
      at += (size_t)nst::pad8(lay.list[i].bytes);
    } else if (lay.kind[i] == ENT_DEAD) {
      const size_t el = lay.elem[i];
      for (size_t r = 0; r < rows.size(); ++r) {
        const size_t n = (size_t)rows[r] * el;
        if (n && !hip_ok(ctx, hipMemcpyAsync(out + at, dev + r * cap * el, n, hipMemcpyDeviceToHost, s), "D2H rows")) return DH_ERR_HIP;
        at += (size_t)nst::pad8(n);
      }
    }
  }
  if (!hip_ok(ctx, hipStreamSynchronize(s), "sync")) return DH_ERR_HIP;
  if (at != h.total_bytes) return fail(ctx, DH_ERR_ARG, "ns_state_export: wrote %zu of %llu bytes", at, (unsigned long long)h.total_bytes);
  return DH_OK;
}

int dh_ns_state_import(dh_ctx* ctx, int problem, const void* buf, uint64_t bytes, int64_t max_iter) {
  DH_CHECK_CTX(ctx);
  ProblemDev pd;
  if (!get_problem(ctx, problem, &pd)) return DH_ERR_ARG;
  if (max_iter < 0) return fail(ctx, DH_ERR_ARG, "ns_state_import: max_iter %lld", (long long)max_iter);
  nst::Header h;
  const int64_t* rows_p = nullptr;
  int64_t cap = 0;
  const int why = nst::validate(buf, bytes, DH_VERSION, sizeof(NsRun), sizeof(NsPlan), pd.ndim, max_iter, &h, &rows_p, &cap);
  if (why != nst::IMG_OK) return fail(ctx, DH_ERR_ARG, "ns_state_import: %s", nst::reject_text(why));
  const char* in = (const char*)buf;
  NsPlan p;
  memcpy((void*)&p, in + h.header_bytes, sizeof p);
  std::vector<int64_t> rows((size_t)h.runs);
  memcpy(rows.data(), rows_p, rows.size() * 8);
  // the plan must be the header's, and the image exactly as long as its arrays say: all of it is known before the
  // device or the context's kept ensemble is touched
  if (p.a.runs != h.runs || p.a.nlive != h.nlive || p.a.ndim != h.ndim || p.a.K != h.queue_size || p.a.cap != h.cap ||
      p.n_words != h.n_words || (p.have_bc ? 1 : 0) != h.have_bc || !p.keep || p.a.runs < 1 || p.a.nlive < 4 ||
      p.a.K > kEPTMax * kT || p.a.max_ells < 1 || p.lds_cons > kNsLdsMax || p.lds_fin > kNsLdsMax || p.every < 1)
    return fail(ctx, DH_ERR_ARG, "ns_state_import: the plan does not belong to the header");
  p.problem = problem;
  p.a.cap = cap;
  NsLayout sizes;
  ns_layout(ctx, p, p.a, nullptr, false, &sizes);
  // (with a null base no kind can be told from the pointers: the sizes alone here, the kinds after the carving)
  char* base = nullptr;
  (void)hipSetDevice(ctx->device);
  if (!hip_ok(ctx, hipMalloc((void**)&base, sizes.bytes), "hipMalloc(ns state)")) return DH_ERR_NOMEM;
  NsLayout lay;
  ns_layout(ctx, p, p.a, base, true, &lay);
  hipStream_t s = ctx->stream;
  auto give_up = [&](int rc) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(base);
    return rc;
  };
  if (!lay.ok) return give_up(DH_ERR_HIP);
  std::vector<uint32_t> elems;
  for (size_t i = 0; i < lay.list.size(); ++i)
    if (lay.kind[i] == ENT_DEAD) elems.push_back((uint32_t)lay.elem[i]);
  if (lay.fixed_bytes != h.fixed_bytes || (size_t)h.row_bytes != lay.row_bytes ||
      nst::image_bytes(h, rows.data(), (int)elems.size(), elems.data()) != h.total_bytes)
    return give_up(fail(ctx, DH_ERR_ARG, "ns_state_import: the image's arrays are not those of its plan"));
  size_t at = (size_t)h.header_bytes + (size_t)nst::pad8(h.plan_bytes) + rows.size() * 8;
  for (size_t i = 0; i < lay.list.size(); ++i) {
    char* dev = base + lay.list[i].off;
    if (lay.kind[i] == ENT_FIXED) {
      if (!hip_ok(ctx, hipMemcpyAsync(dev, in + at, lay.list[i].bytes, hipMemcpyHostToDevice, s), "H2D state")) return give_up(DH_ERR_HIP);
      at += (size_t)nst::pad8(lay.list[i].bytes);
    } else if (lay.kind[i] == ENT_DEAD) {
      const size_t el = lay.elem[i];
      for (size_t r = 0; r < rows.size(); ++r) {
        const size_t n = (size_t)rows[r] * el;
        if (n && !hip_ok(ctx, hipMemcpyAsync(dev + r * (size_t)cap * el, in + at, n, hipMemcpyHostToDevice, s), "H2D rows"))
          return give_up(DH_ERR_HIP);
        at += (size_t)nst::pad8(n);
      }
    }
  }
  if (!hip_ok(ctx, hipStreamSynchronize(s), "sync")) return give_up(DH_ERR_HIP);
  // installed: the context's earlier kept ensemble goes, as with a later keep
  kept_free(ctx);
  std::vector<double> rec((size_t)h.runs * 8, 0.0);
  for (int r = 0; r < h.runs; ++r) rec[(size_t)r * 8 + 2] = (double)rows[(size_t)r];
  ns_keep_arrays(ctx, lay.a, problem, base, rec.data());
  p.a = lay.a;
  ns_keep_loop(ctx, p, lay.a, lay.x, h.fill, h.cube_phase != 0);
  return DH_OK;
}

}  // extern "C"
