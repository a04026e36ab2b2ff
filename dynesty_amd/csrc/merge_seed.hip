// The seeds of a dynamic batch chosen on the device, from the merged run where it lives.
// The reference draws nlive_new indices without replacement, each draw proportional to the remaining exp(logvol_i)
// (_configure_batch_sampler, dynamicsampler.py:457-533: successive sampling).  The same law, order of the draws
// included, is "the nlive_new largest of logvol_i + G_i, G_i i.i.d. standard Gumbel, in descending order"
// (Plackett-Luce), a pure function of (seed, strand, point):
//   words   strand s (global index first + s) uses subsequence 2^63 + 2^62 + s of the Philox4x32-10 stream keyed by
//           `seed`; point i -- its index in the merged run -- takes words 2 i and 2 i + 1: block b serves points 2 b, 2 b + 1
//   key     logvol_i - log(-log u), u = uniform_double of the two words in (0, 1]; u = 1 is +inf, always chosen
//   order   descending key, equal keys by smaller i; a strand's seeds are the first nlive_new points of that order
// The subset, the moved boundary, vol_idx and the start row follow dynamic.batch_seed; a point can be chosen iff
// logvol_i - max(logvol over the subset) >= -708.
//
// Stages (S strands, k = nlive_new, the subset [lo, M) of the merged run):
//   ms_bounds   one thread: lo, the moved boundary, vol_idx (NumPy's first-occurrence argmin), the start row
//   ms_max, ms_npos   the exact maximum of logvol over the subset (integer atomicMax on the order-preserving image) and
//               the number of points of positive weight (integer atomicAdd)
//   ms_pass<false>   a histogram pass: every key of the subset made again, the 8 bits below the strand's decided prefix
//               counted in an LDS histogram per (workgroup, strand), added to the strand's 256 global bins
//   ms_decide   one thread per strand: the bin in which the k-th largest key lies; the strand is done when that bin
//               holds at most kSeedCap keys (or exactly what is still needed, or all 64 bits are decided)
//   ms_pass<true>    the collect pass: every key at or above the threshold bin as an (image, index) pair, to
//               atomically claimed slots of the strand's list
//   ms_rank     the strand's pairs ranked by (key descending, index ascending) by counting against LDS tiles; the
//               first k ranks are the output, whatever order the collect wrote in
//   ms_stage    on request: the chosen points' unit-cube rows and ln L gathered into one block, which comes to the host
//               with the indices (the logl and logvol columns never do)
// All counts are integers, so the output is bitwise reproducible from call to call; a strand's seeds depend on
// (seed, first + s) alone.
#include "merge_dev.h"

namespace {

constexpr u64 kSign = 0x8000000000000000ull;

// the order-preserving image of a double (NaN never arrives here) and back
__device__ __forceinline__ u64 key_image(double x) {
  const u64 b = (u64)__double_as_longlong(x);
  return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double image_key(u64 m) {
  return __longlong_as_double((long long)((m & kSign) ? (m ^ kSign) : ~m));
}
__device__ __forceinline__ double seed_key(double logvol, uint32_t w0, uint32_t w1) {
  return logvol - log(-log(uniform_double(w0, w1)));
}

// info: prior, lo, count, n_pos (filled in by the host), logl_min (effective), vol_idx, start[5]; li: lo, count;
// flags[0]: no point above logl_min; flags[1]: every point lies above it -- no choice is made
__global__ void ms_bounds(long long M, int k, double logl_min, const double* __restrict__ logl, const double* __restrict__ logvol,
                          const double* __restrict__ logz, const double* __restrict__ h, const double* __restrict__ logzerr,
                          double* info, long long* li, int* flags) {
  if (threadIdx.x || blockIdx.x) return;
  long long lo = upper_bound_dev(logl, M, logl_min), count = M - lo;
  double eff = logl_min;
  int prior = 0;
  if (lo == 0) {
    prior = 1;
    flags[1] = 1;
  } else if (count == 0) {
    flags[0] = 1;
  } else if (count < k) {  // the boundary moves down to collect k points
    lo = M < k ? 0 : M - k;
    count = M - lo;
    eff = lo > 0 ? logl[lo - 1] : -INFINITY;
    if (lo == 0) prior = 1;
  }
  long long vol_idx = 0;
  if (eff != -INFINITY) {
    // argmin |logl - eff|, first occurrence: the nearest neighbours on either side give the smallest distance; the
    // rounded distance does not increase towards eff, so its first occurrence is found by bisection below
    const long long j = lower_bound_dev(logl, M, eff);
    double dmin = INFINITY;
    if (j < M) dmin = fabs(logl[j] - eff);
    if (j > 0) {
      const double d = fabs(logl[j - 1] - eff);
      if (d <= dmin) dmin = d;
    }
    long long a = 0, b = j;  // first i in [0, j) with |logl_i - eff| <= dmin, else j
    while (a < b) {
      const long long mid = (a + b) >> 1;
      if (fabs(logl[mid] - eff) <= dmin) b = mid; else a = mid + 1;
    }
    vol_idx = a + 1;
  }
  info[0] = (double)prior;
  info[1] = (double)lo;
  info[2] = (double)count;
  info[3] = 0.0;
  info[4] = eff;
  info[5] = (double)vol_idx;
  const bool row = !prior && !flags[0] && vol_idx >= 1 && vol_idx <= M;
  const long long r = row ? vol_idx - 1 : 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double e = logzerr[r];
  info[6] = row ? logvol[r] : nan;
  info[7] = row ? logz[r] : nan;
  info[8] = row ? h[r] : nan;
  info[9] = row ? e * e : nan;
  info[10] = row ? logl[r] : nan;
  info[11] = 0.0;
  li[0] = lo;
  li[1] = count;
}

// the largest logvol of the subset, as its image (0 = none; NaN values are passed over)
__global__ void __launch_bounds__(kT) ms_max(long long lo, long long M, const double* __restrict__ logvol, u64* out) {
  __shared__ u64 red[kT];
  u64 acc = 0;
  for (long long i = lo + (long long)blockIdx.x * kT + threadIdx.x; i < M; i += (long long)gridDim.x * kT) {
    const double x = logvol[i];
    const u64 m = x == x ? key_image(x) : 0;
    acc = m > acc ? m : acc;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] = red[threadIdx.x + d] > red[threadIdx.x] ? red[threadIdx.x + d] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(out, red[0]);
}

// the points of positive weight
__global__ void __launch_bounds__(kT) ms_npos(long long lo, long long M, const double* __restrict__ logvol,
                                              const u64* __restrict__ maxbits, u64* out) {
  __shared__ u64 red[kT];
  const double mx = image_key(maxbits[0]);
  u64 acc = 0;
  for (long long i = lo + (long long)blockIdx.x * kT + threadIdx.x; i < M; i += (long long)gridDim.x * kT)
    acc += (logvol[i] - mx >= kSeedLogMin) ? 1 : 0;
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int d = kT / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out, red[0]);
}

__global__ void __launch_bounds__(kT) ms_init(int S, int k, SeedState* st) {
  const int s = blockIdx.x * kT + threadIdx.x;
  if (s >= S) return;
  st[s] = SeedState{0, k, 56, 1, 0};
}

struct SeedArgs {
  const double* logvol;
  const u64* maxbits;
  long long M, lo, pair0;
  uint64_t seed, seq0;  // strand s of the call: subsequence seq0 + s
  int strands;
};

// One pass over the subset for the strands of tile blockIdx.y: the thread's kSeedPairs Philox blocks (two neighbouring
// points each; logvol is loaded once, at clamped indices, and masked afterwards -- no load under a condition), every
// key made again.  COLLECT = false: the digit at q.shift of the keys whose higher bits equal the strand's prefix is
// counted, in one of two LDS histograms taken in turn (a thread flushes and clears its own bin after the barrier; the
// next strand counts into the other table, so one barrier per strand is enough).  COLLECT = true: the keys at or above
// the threshold bin go to claimed slots of the strand's pair list; flags[1]: a slot beyond the list's capacity.
template <bool COLLECT>
__global__ void __launch_bounds__(kT) ms_pass(SeedArgs a, const SeedState* __restrict__ st, unsigned* __restrict__ bins,
                                              unsigned* __restrict__ cnt, u64* __restrict__ pimg, int* __restrict__ pidx,
                                              long long ecap, int* flags) {
  __shared__ unsigned hist[2][kSeedBins];
  const int t = threadIdx.x;
  const double mx = image_key(a.maxbits[0]);
  const long long pb0 = a.pair0 + (long long)blockIdx.x * (kT * kSeedPairs) + t;
  double lv[2 * kSeedPairs];
  bool ok[2 * kSeedPairs];
#pragma unroll
  for (int j = 0; j < kSeedPairs; ++j) {
    const long long i0 = 2 * (pb0 + (long long)j * kT), i1 = i0 + 1;
    const long long c0 = i0 < a.M ? i0 : a.M - 1, c1 = i1 < a.M ? i1 : a.M - 1;
    const double x0 = a.logvol[c0], x1 = a.logvol[c1];
    lv[2 * j] = x0;
    lv[2 * j + 1] = x1;
    ok[2 * j] = i0 >= a.lo && i0 < a.M && x0 - mx >= kSeedLogMin;
    ok[2 * j + 1] = i1 >= a.lo && i1 < a.M && x1 - mx >= kSeedLogMin;
  }
  if (!COLLECT) {
    hist[0][t] = 0;
    hist[1][t] = 0;
    __syncthreads();
  }
  const int s0 = blockIdx.y * kSeedTile, s1 = s0 + kSeedTile < a.strands ? s0 + kSeedTile : a.strands;
  int turn = 0;
  for (int s = s0; s < s1; ++s) {
    const SeedState q = st[s];  // (the same for the whole workgroup)
    if (!COLLECT && !q.active) continue;
    unsigned* hcur = hist[turn & 1];
    ++turn;
    const int up = q.shift + 8;  // the decided bits lie above this position (64 in the first pass: none yet)
#pragma unroll
    for (int j = 0; j < kSeedPairs; ++j) {
      const long long pb = pb0 + (long long)j * kT;
      uint32_t w[4];
      philox4x32_10(a.seed, a.seq0 + (uint64_t)s, (uint64_t)pb, w);
      const u64 m0 = key_image(seed_key(lv[2 * j], w[0], w[1])), m1 = key_image(seed_key(lv[2 * j + 1], w[2], w[3]));
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const u64 m = e ? m1 : m0;
        const bool valid = ok[2 * j + e];
        if (!COLLECT) {
          const bool in = valid && (up >= 64 || (m >> up) == q.prefix);
          if (in) atomicAdd(&hcur[(unsigned)(m >> q.shift) & (kSeedBins - 1)], 1u);
        } else {
          if (valid && (m >> up) >= q.prefix) {
            const unsigned slot = atomicAdd(&cnt[s], 1u);
            if ((long long)slot < ecap) {
              pimg[(size_t)s * (size_t)ecap + slot] = m;
              pidx[(size_t)s * (size_t)ecap + slot] = (int)(2 * pb + e);
            } else {
              flags[1] = 1;
            }
          }
        }
      }
    }
    if (!COLLECT) {
      __syncthreads();
      const unsigned g = hcur[t];
      hcur[t] = 0;
      if (g) atomicAdd(&bins[(size_t)s * kSeedBins + t], g);
    }
  }
}

// The bin of the k-th largest key of every active strand, from the top; the bins are cleared for the next pass.
// flags[0]: fewer keys than needed (never, given n_pos >= k); flags[2]: all 64 bits decided and more than kSeedCap
// keys are exactly equal at the threshold.
__global__ void __launch_bounds__(kT) ms_decide(int S, SeedState* st, unsigned* bins, int* nactive, int* flags) {
  const int s = blockIdx.x * kT + threadIdx.x;
  if (s >= S) return;
  SeedState q = st[s];
  if (!q.active) return;
  unsigned acc = 0, pop = 0;
  int b = -1;
  for (int d = kSeedBins - 1; d >= 0; --d) {
    const unsigned c = bins[(size_t)s * kSeedBins + d];
    bins[(size_t)s * kSeedBins + d] = 0;
    if (b < 0) {
      if (acc + c >= (unsigned)q.need) {
        b = d;
        pop = c;
      } else {
        acc += c;
      }
    }
  }
  if (b < 0) {
    flags[0] = 1;
    q.active = 0;
  } else {
    q.need -= (int)acc;
    q.prefix = (q.prefix << 8) | (u64)b;
    q.shift -= 8;
    q.pop = pop;
    const bool done = pop <= (unsigned)kSeedCap || pop == (unsigned)q.need || q.shift < 0;
    if (done && pop > (unsigned)kSeedCap && pop != (unsigned)q.need) flags[2] = 1;
    q.active = done ? 0 : 1;
    if (!done) atomicAdd(nactive, 1);
  }
  st[s] = q;
}

// Strand blockIdx.x: the rank of each of its E collected pairs in (key descending, index ascending) by counting against
// LDS tiles; ranks below k are the output.  The pairs are distinct, so are the ranks.  flags[3]: fewer than k pairs.
__global__ void __launch_bounds__(kT) ms_rank(int k, long long ecap, const unsigned* __restrict__ cnt, const u64* __restrict__ pimg,
                                              const int* __restrict__ pidx, long long* __restrict__ idx_out,
                                              double* __restrict__ key_out, int* flags) {
  __shared__ u64 tm[kSeedRankTile];
  __shared__ int ti[kSeedRankTile];
  const int s = blockIdx.x;
  long long E = cnt[s];
  if (E > ecap) E = ecap;
  if (E < k && blockIdx.y == 0 && threadIdx.x == 0) flags[3] = 1;
  if ((long long)blockIdx.y * kT >= E) return;  // (the whole workgroup)
  const u64* im = pimg + (size_t)s * (size_t)ecap;
  const int* ix = pidx + (size_t)s * (size_t)ecap;
  const long long e = (long long)blockIdx.y * kT + threadIdx.x;
  const bool mine = e < E;
  const u64 m = im[mine ? e : 0];
  const int i = ix[mine ? e : 0];
  long long rank = 0;
  for (long long t0 = 0; t0 < E; t0 += kSeedRankTile) {
    const int nt = E - t0 < kSeedRankTile ? (int)(E - t0) : kSeedRankTile;
    __syncthreads();
    for (int t = threadIdx.x; t < nt; t += kT) {
      tm[t] = im[t0 + t];
      ti[t] = ix[t0 + t];
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) rank += (tm[t] > m || (tm[t] == m && ti[t] < i)) ? 1 : 0;
  }
  if (mine && rank < k) {
    idx_out[(size_t)s * k + rank] = i;
    key_out[(size_t)s * k + rank] = image_key(m);
  }
}

// the chosen points' unit-cube rows (one thread per element) and ln L (the threads of column 0)
__global__ void __launch_bounds__(kT) ms_stage(size_t total, int D, long long M, const long long* __restrict__ idx,
                                               const double* __restrict__ u, const double* __restrict__ logl,
                                               double* __restrict__ out_u, double* __restrict__ out_l) {
  const size_t e = (size_t)blockIdx.x * kT + threadIdx.x;
  if (e >= total) return;
  const size_t p = e / (size_t)D;
  const int d = (int)(e - p * (size_t)D);
  long long row = idx[p];
  if (row < 0 || row >= M) row = 0;
  out_u[e] = u[(size_t)row * D + d];
  if (d == 0) out_l[p] = logl[row];
}

}  // namespace

extern "C" {

int dh_merged_batch_seed(dh_ctx* ctx, uint64_t seed, int64_t first, int strands, int nlive_new, double logl_min,
                         int64_t* idx_out, double* key_out, double* u_out, double* logl_out, double* info_out) {
  DH_CHECK_CTX(ctx);
  // ---- plan: refused before the device is touched ----
  const int verdict = seed_check(ctx->merged.base != nullptr, (long long)first, strands, nlive_new, logl_min, info_out != nullptr);
  if (verdict != SV_OK) return fail(ctx, DH_ERR_ARG, "merged_batch_seed: %s", seed_verdict_text(verdict));
  const dh_merged& m = ctx->merged;
  const long long M = m.M;
  const int S = strands, k = nlive_new, D = m.ndim;
  if ((unsigned long long)S * (unsigned long long)k * (unsigned long long)D >= (1ull << 32))
    return fail(ctx, DH_ERR_ARG, "merged_batch_seed: %d strands x %d seeds x %d coordinates (a row array is limited to 2^32 elements)", S, k, D);
  hipStream_t st = ctx->stream;
  (void)hipSetDevice(ctx->device);
  SeedHead hd;
  auto lay_h = [&](Carver& c) { carve_seed_head(c, hd); };
  const size_t hbytes = layout_bytes(lay_h);  // (before the carve: a size pass nulls the layout's pointers)
  char* hbase = device_carve(lay_h);
  if (!hbase) return fail(ctx, DH_ERR_NOMEM, "merged_batch_seed: %zu bytes of device memory", hbytes);
  char *sbase = nullptr, *gbase = nullptr;  // the select's scratch; the gathered rows
  auto done = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(hbase);
    (void)hipFree(sbase);
    (void)hipFree(gbase);
    return code;
  };
  double info[kSeedInfo];
  long long li[2];
  int flags[4];
  if (!hip_ok(ctx, hipMemsetAsync(hbase, 0, hbytes, st), "memset")) return done(DH_ERR_HIP);
  hipLaunchKernelGGL(ms_bounds, dim3(1), dim3(64), 0, st, M, k, logl_min, m.logl, m.logvol, m.logz, m.h, m.logzerr, hd.info, hd.li,
                     hd.flags);
  if (!hip_ok(ctx, hipGetLastError(), "seed bounds launch") || !down(ctx, info, hd.info, (size_t)kSeedInfo) ||
      !down(ctx, li, hd.li, (size_t)2) || !down(ctx, flags, hd.flags, (size_t)4) ||
      !hip_ok(ctx, hipStreamSynchronize(st), "seed bounds sync"))
    return done(DH_ERR_HIP);
  if (flags[0])
    return done(fail(ctx, DH_ERR_VALUE, "merged_batch_seed: could not find live points in the required logl interval: no point above "
                                        "logl_min = %.17g", logl_min));
  auto answer = [&]() {
    for (int i = 0; i < kSeedInfo; ++i) info_out[i] = info[i];
  };
  if (flags[1]) {  // from the prior: no choice is made
    answer();
    return done(DH_OK);
  }
  const long long lo = li[0], count = li[1];
  if (lo < 0 || count < 1 || lo + count != M) return done(fail(ctx, DH_ERR_HIP, "merged_batch_seed: subset [%lld, +%lld) of %lld", lo, count, M));
  // ---- the maximum of logvol over the subset and the points of positive weight ----
  const unsigned gsub = blocks_for((size_t)count, kT) < 1024 ? blocks_for((size_t)count, kT) : 1024;
  hipLaunchKernelGGL(ms_max, dim3(gsub), dim3(kT), 0, st, lo, M, m.logvol, hd.maxbits);
  hipLaunchKernelGGL(ms_npos, dim3(gsub), dim3(kT), 0, st, lo, M, m.logvol, hd.maxbits, hd.npos);
  u64 npos = 0;
  if (!hip_ok(ctx, hipGetLastError(), "seed count launch") || !down(ctx, &npos, hd.npos, (size_t)1) ||
      !hip_ok(ctx, hipStreamSynchronize(st), "seed count sync"))
    return done(DH_ERR_HIP);
  info[3] = (double)npos;
  if (npos < (u64)k) {  // batch_seed's ValueError: an answer, not an error
    answer();
    return done(DH_OK);
  }
  // ---- the select ----
  const size_t ecap = seed_ecap(k, (long long)npos);
  SeedSelBuf b;
  SeedStage g;
  auto lay_s = [&](Carver& c) { carve_seed_select(c, b, (size_t)S, (size_t)k, ecap); };
  auto lay_g = [&](Carver& c) { carve_seed_stage(c, g, (size_t)S, (size_t)k, (size_t)D); };
  const bool rows = u_out || logl_out;  // the chosen rows are gathered on the device and come down in one piece
  sbase = device_carve(lay_s);
  if (sbase && rows) gbase = device_carve(lay_g);
  if (!sbase || (rows && !gbase))
    return done(fail(ctx, DH_ERR_NOMEM, "merged_batch_seed: %zu + %zu bytes of device memory beside the merged run", layout_bytes(lay_s),
                     rows ? layout_bytes(lay_g) : (size_t)0));
  const SeedGrid gr = seed_grid(lo, M, S);
  const SeedArgs a{m.logvol, hd.maxbits, M, lo, gr.pair0, seed, (3ull << 62) + (uint64_t)first, S};
  if (!hip_ok(ctx, hipMemsetAsync(b.bins, 0, (size_t)S * kSeedBins * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(b.cnt, 0, (size_t)S * 4, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(b.idx, 0xff, (size_t)S * k * 8, st), "memset") ||
      !hip_ok(ctx, hipMemsetAsync(b.key, 0, (size_t)S * k * 8, st), "memset"))
    return done(DH_ERR_HIP);
  const unsigned gS = blocks_for((size_t)S, kT);
  hipLaunchKernelGGL(ms_init, dim3(gS), dim3(kT), 0, st, S, k, b.st);
  int passes = 0;
  for (; passes < kSeedPasses;) {
    int nactive = 0;
    if (!hip_ok(ctx, hipMemsetAsync(hd.nactive, 0, 4, st), "memset")) return done(DH_ERR_HIP);
    hipLaunchKernelGGL(ms_pass<false>, dim3(gr.chunks, gr.tiles), dim3(kT), 0, st, a, b.st, b.bins, b.cnt, b.pimg, b.pidx,
                       (long long)ecap, hd.flags);
    hipLaunchKernelGGL(ms_decide, dim3(gS), dim3(kT), 0, st, S, b.st, b.bins, hd.nactive, hd.flags);
    ++passes;
    if (!hip_ok(ctx, hipGetLastError(), "seed pass launch") || !down(ctx, &nactive, hd.nactive, (size_t)1) ||
        !down(ctx, flags, hd.flags, (size_t)4) || !hip_ok(ctx, hipStreamSynchronize(st), "seed pass sync"))
      return done(DH_ERR_HIP);
    if (flags[0]) return done(fail(ctx, DH_ERR_HIP, "merged_batch_seed: a strand's histogram holds fewer keys than needed"));
    if (flags[2])
      return done(fail(ctx, DH_ERR_VALUE, "merged_batch_seed: more than %d exactly equal keys at a strand's threshold", kSeedCap));
    if (nactive == 0) break;
  }
  hipLaunchKernelGGL(ms_pass<true>, dim3(gr.chunks, gr.tiles), dim3(kT), 0, st, a, b.st, b.bins, b.cnt, b.pimg, b.pidx, (long long)ecap,
                     hd.flags);
  hipLaunchKernelGGL(ms_rank, dim3(S, blocks_for(ecap, kT)), dim3(kT), 0, st, k, (long long)ecap, b.cnt, b.pimg, b.pidx, b.idx, b.key,
                     hd.flags);
  if (rows)
    hipLaunchKernelGGL(ms_stage, dim3(blocks_for((size_t)S * k * D, kT)), dim3(kT), 0, st, (size_t)S * k * D, D, M, b.idx, m.u, m.logl,
                       g.u, g.logl);
  static_assert(sizeof(long long) == sizeof(int64_t), "idx_out");
  if (!hip_ok(ctx, hipGetLastError(), "seed collect launch") || !down(ctx, flags, hd.flags, (size_t)4) ||
      !down(ctx, (long long*)idx_out, b.idx, (size_t)S * k) || !down(ctx, key_out, b.key, (size_t)S * k) ||
      (rows && (!down(ctx, u_out, (const double*)g.u, (size_t)S * k * D) || !down(ctx, logl_out, (const double*)g.logl, (size_t)S * k))) ||
      !hip_ok(ctx, hipStreamSynchronize(st), "seed collect sync"))
    return done(DH_ERR_HIP);
  if (flags[1] || flags[3])
    return done(fail(ctx, DH_ERR_HIP, "merged_batch_seed: the collect pass and the histograms disagree (%s)",
                     flags[1] ? "more pairs than counted" : "fewer pairs than needed"));
  info[11] = (double)passes;
  answer();
  return done(DH_OK);
}

}  // extern "C"
