// Internal: what the units of the combiner share on the device side (merge.hip, merge_marginals.hip, merge_errors.hip):
// the scan operators and the three-launch scan, np.logaddexp, and the small host helpers around a launch.  The sizes
// and the scratch layouts are merge_plan.h's.  Everything here is local to the unit that includes it.
#pragma once
#include <math.h>

#include <vector>

#include "ctx.h"

using namespace dh;
using namespace dh_merge;

namespace {

// ---- scans ----------------------------------------------------------------------------------------------------------

struct SumD {
  typedef double T;
  __device__ static T id() { return 0.0; }
  __device__ static T op(T a, T b) { return a + b; }
};
struct SumI {
  typedef int T;
  __device__ static T id() { return 0; }
  __device__ static T op(T a, T b) { return a + b; }
};
// ln sum exp as (max, sum scaled by exp(-max)) pairs: associative, never underflows against a far later maximum
struct LsePair {
  double m, s;
};
struct Lse {
  typedef LsePair T;
  __device__ static T id() { return T{-INFINITY, 0.0}; }
  __device__ static T op(T a, T b) {
    if (a.s == 0.0) return b;  // the identity (and nothing else: a point's own pair has s = 1) combines exactly
    if (b.s == 0.0 || b.m == -INFINITY) return a;
    if (a.m >= b.m) return T{a.m, a.s + b.s * exp(b.m - a.m)};
    return T{b.m, a.s * exp(a.m - b.m) + b.s};
  }
};
static_assert(sizeof(LsePair) == kScanElem, "the layouts size a scan's chunk aggregates by kScanElem");

// Inclusive scan of the 256 per-thread values of a workgroup (Hillis-Steele in LDS); returns the thread's inclusive
// value, *excl its exclusive one, *total the workgroup's.
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(typename Op::T v, typename Op::T* lds, typename Op::T* excl,
                                                     typename Op::T* total) {
  typedef typename Op::T T;
  const int t = threadIdx.x;
  T* a = lds;
  T* b = lds + kT;
  a[t] = v;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {
    b[t] = t >= d ? Op::op(a[t - d], a[t]) : a[t];
    __syncthreads();
    T* sw = a;
    a = b;
    b = sw;
  }
  const T inc = a[t];
  *excl = t > 0 ? a[t - 1] : Op::id();
  *total = a[kT - 1];
  __syncthreads();
  return inc;
}

// F: struct { typedef Op; __device__ Op::T term(long long k) const; __device__ void put(long long k, Op::T incl, Op::T excl) const; }
template <class F>
__global__ void __launch_bounds__(kT) scan_reduce(F f, long long M, typename F::Op::T* part) {
  typedef typename F::Op Op;
  typedef typename Op::T T;
  __shared__ T lds[2 * kT];
  const long long k0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kItems;
  T acc = Op::id();
  for (int j = 0; j < kItems; ++j)
    if (k0 + j < M) acc = Op::op(acc, f.term(k0 + j));
  T ex, tot;
  block_scan<Op>(acc, lds, &ex, &tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one workgroup: part[b] becomes the combination of the aggregates of the workgroups before b
template <class Op>
__global__ void __launch_bounds__(kT) scan_carry(typename Op::T* part, int nblk) {
  typedef typename Op::T T;
  __shared__ T lds[2 * kT];
  T carry = Op::id();
  for (int b0 = 0; b0 < nblk; b0 += kT) {
    const int b = b0 + threadIdx.x;
    const T v = b < nblk ? part[b] : Op::id();
    T ex, tot;
    block_scan<Op>(v, lds, &ex, &tot);
    if (b < nblk) part[b] = Op::op(carry, ex);
    carry = Op::op(carry, tot);
  }
}

template <class F>
__global__ void __launch_bounds__(kT) scan_apply(F f, long long M, const typename F::Op::T* part) {
  typedef typename F::Op Op;
  typedef typename Op::T T;
  __shared__ T lds[2 * kT];
  const long long k0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kItems;
  T x[kItems];
  T acc = Op::id();
  for (int j = 0; j < kItems; ++j) {
    x[j] = k0 + j < M ? f.term(k0 + j) : Op::id();
    acc = Op::op(acc, x[j]);
  }
  T ex, tot;
  block_scan<Op>(acc, lds, &ex, &tot);
  T run = Op::op(part[blockIdx.x], ex);
  for (int j = 0; j < kItems; ++j) {
    const T before = run;
    run = Op::op(run, x[j]);
    if (k0 + j < M) f.put(k0 + j, run, before);
  }
}

__device__ __forceinline__ double logaddexp_np(double x, double y) {  // np.logaddexp
  if (x == y) return x + 0.6931471805599453;
  const double d = x - y;
  if (d > 0) return x + log1p(exp(-d));
  if (d <= 0) return y + log1p(exp(d));
  return x + y;
}

template <class F>
bool run_scan(dh_ctx* ctx, const F& f, long long M, void* part) {
  typedef typename F::Op Op;
  const int nblk = (int)blocks_for((size_t)M, kChunk);
  typename Op::T* p = (typename Op::T*)part;
  hipLaunchKernelGGL(scan_reduce<F>, dim3(nblk), dim3(kT), 0, ctx->stream, f, M, p);
  hipLaunchKernelGGL(scan_carry<Op>, dim3(1), dim3(kT), 0, ctx->stream, p, nblk);
  hipLaunchKernelGGL(scan_apply<F>, dim3(nblk), dim3(kT), 0, ctx->stream, f, M, (const typename Op::T*)p);
  return hip_ok(ctx, hipGetLastError(), "merge scan launch");
}

template <class K>
bool lds_limit(dh_ctx* ctx, K kernel, size_t bytes) {
  return hip_ok(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), "LDS size");
}

// An allocation of its own as one layout: the size pass, hipMalloc of that total, the pointer pass.  Null (and the
// layout's pointers null) where the device has no room.
template <class Layout>
size_t layout_bytes(Layout&& layout) {
  Carver size;
  layout(size);
  return size.off;
}
template <class Layout>
char* device_carve(Layout&& layout) {
  char* base = nullptr;
  if (hipMalloc((void**)&base, layout_bytes(layout)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  Carver place{base};
  layout(place);
  return base;
}

inline int need_merged(dh_ctx* ctx) {
  if (!ctx->merged.base) return fail(ctx, DH_ERR_ARG, "no merged run in this context");
  return DH_OK;
}

}  // namespace
