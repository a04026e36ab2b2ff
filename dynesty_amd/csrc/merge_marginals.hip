// ---- marginals of the merged run: weighted quantiles, 1-D and 2-D weighted histograms -------
//
// Every sum of weights is a sum of the integers W_i = llrint(w_i 2^62): exact and independent of order, so LDS and
// global 64-bit integer atomics keep the results bitwise reproducible.  A workgroup owns a range of rows and walks
// (row, requested column) pairs in row-major order -- with all columns asked for that is the rows' own layout, read
// coalesced -- and tiles over the requested columns when their tables outgrow its LDS.
#include "merge_dev.h"

namespace {

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
// the requested columns of a quantile or 1-D histogram call (all of them without a list), each inside [0, ndim)
int check_cols(dh_ctx* ctx, const char* what, int ncol, const int32_t* cols_or_null, int ndim, std::vector<int>& cols) {
  cols.resize((size_t)ncol);
  for (int i = 0; i < ncol; ++i) {
    cols[(size_t)i] = cols_or_null ? cols_or_null[i] : i;
    if (cols[(size_t)i] < 0 || cols[(size_t)i] >= ndim)
      return fail(ctx, DH_ERR_ARG, "%s: column %d outside [0, %d)", what, cols[(size_t)i], ndim);
  }
  return DH_OK;
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
  HistBuf b;
  const int rc = arena_carve(ctx, [&](Carver& c) { carve_hist(c, b, two, (size_t)n, (size_t)nbx, (size_t)nby); });
  if (rc) return rc;
  HArgs a;
  a.M = m.M;
  a.D = m.ndim;
  a.n = n;
  a.nbx = nbx;
  a.nby = two ? nby : 0;
  a.weighted = weighted ? 1 : 0;
  a.per = hist_per(nb);
  a.w = m.w;
  a.v = m.v;
  if (!arena_fill(ctx, b.cols, (const int*)cols, ncol) || !arena_fill(ctx, b.xe, xe, (size_t)n * ((size_t)nbx + 1)) ||
      (two && !arena_fill(ctx, b.ye, ye, (size_t)n * ((size_t)nby + 1))))
    return DH_ERR_NOMEM;  // (what the staging always has returned)
  a.cols = b.cols;
  a.xe = b.xe;
  a.ye = b.ye;
  a.table = b.table;
  double* d_out = b.out;
  unsigned groups;
  a.rows = rows_per_group(m.M, &groups);
  hipStream_t st = ctx->stream;
  const size_t lds = hist_lds(a.per, n, nb);
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
  std::vector<int> cols;
  if (check_cols(ctx, "merged_quantile", ncol, cols_or_null, m.ndim, cols)) return DH_ERR_ARG;
  const size_t S = (size_t)ncol * nq;
  QuantBuf b;
  int rc = arena_carve(ctx, [&](Carver& c) { carve_quantile(c, b, (size_t)nq, (size_t)ncol); });
  if (rc) return rc;
  const QuantTile tile = quantile_tile(nq, ncol);
  QArgs a;
  a.M = m.M;
  a.D = m.ndim;
  a.ncol = ncol;
  a.nq = nq;
  a.cpt = tile.cpt;
  a.w = m.w;
  a.v = m.v;
  if (!arena_fill(ctx, b.q, q, (size_t)nq) || !arena_fill(ctx, b.cols, (const int*)cols.data(), (size_t)ncol))
    return DH_ERR_NOMEM;  // (what the staging always has returned)
  a.q = b.q;
  a.cols = b.cols;
  a.table = b.table;
  a.total = b.total;
  a.cmax = b.cmax;
  a.last = b.last;
  a.flags = b.flags;
  a.cmin = b.cmin;
  a.s = QSel{b.pk, b.cb, b.wk, b.ti, b.succ, b.frac, b.pi, b.mode};
  a.out = b.out;
  unsigned groups;
  a.rows = rows_per_group(m.M, &groups);
  hipStream_t st = ctx->stream;
  const size_t lds_digit = tile.lds_digit, lds_succ = tile.lds_succ;
  const bool combine = tile.combine;
  // one memset clears table, total, cmax, last and flags; the kernels initialise the rest themselves
  if (!hip_ok(ctx, hipMemsetAsync(b.table, 0, b.zero_bytes, st), "memset") ||
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
  std::vector<int> cols;
  if (check_cols(ctx, "merged_hist1d", ncol, cols_or_null, m.ndim, cols)) return DH_ERR_ARG;
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
