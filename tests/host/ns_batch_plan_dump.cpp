// Prints what ns_batch_plan.h decides, for tests/test_ns_batch_plan_cpu.py.
// stdin, one request per line:
//   check runs nlive_new ndim queue_size sampler bound keep logl_min logl_max have_arrays seed_lo n_bad_seed bad_value
//         start_kind
//         every seed's ln L is seed_lo + 0.001 i (i = flat index) except that seed number n_bad_seed (-1: none) is
//         bad_value; have_arrays = 0 passes null arrays; start_kind: 0 a good row, 1 a NaN logvol in the last run,
//         2 a scale of 0 in the last run, 3 logz = -1e300 (good: the loop's own "nothing integrated yet")
//         -> {"verdict": v, "where": w, "text": "..."}
//   sizes runs nlive_new ndim queue_size
//         -> {"seed_fills": f, "stage_points": p, "stage_bytes": b}
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ns_batch_plan.h"

using namespace dh_nsb;

static double num() {
  char w[64];
  if (scanf("%63s", w) != 1) exit(2);
  if (!strcmp(w, "inf")) return INFINITY;
  if (!strcmp(w, "-inf")) return -INFINITY;
  if (!strcmp(w, "nan")) return NAN;
  return strtod(w, nullptr);
}
static long long whole() {
  long long v;
  if (scanf("%lld", &v) != 1) exit(2);
  return v;
}

int main() {
  char word[32];
  while (scanf("%31s", word) == 1) {
    if (!strcmp(word, "check")) {
      Request q;
      q.runs = (int)whole();
      q.nlive_new = (int)whole();
      q.ndim = (int)whole();
      q.queue_size = (int)whole();
      q.sampler = (int)whole();
      q.bound = (int)whole();
      q.keep = (int)whole();
      q.logl_min = num();
      q.logl_max = num();
      const int have = (int)whole();
      const double seed_lo = num();
      const long long nbad = whole();
      const double bad = num();
      const int start_kind = (int)whole();
      // (the arrays exist at the size the request names only where that size is sane: check() must not read them
      // before it has refused a request with runs < 1 or nlive_new out of range)
      const bool sane = q.runs >= 1 && q.ndim >= 1 && q.nlive_new >= kMinNlive && q.nlive_new <= kMaxNlive;
      const size_t n = sane ? (size_t)q.runs * (size_t)q.nlive_new : 1;
      std::vector<double> logl(n), u(sane ? n * (size_t)q.ndim : 1, 0.5), start(sane ? (size_t)q.runs * 6 : 6);
      for (size_t i = 0; i < n; ++i) logl[i] = seed_lo + 0.001 * (double)i;
      if (nbad >= 0 && (size_t)nbad < n) logl[(size_t)nbad] = bad;
      for (size_t r = 0; r * 6 < start.size(); ++r) {
        double* s = &start[r * 6];
        s[0] = -3.0;
        s[1] = start_kind == 3 ? -1e300 : -12.0;
        s[2] = 0.5;
        s[3] = 0.01;
        s[4] = q.logl_min;
        s[5] = 1.0;
      }
      if (start_kind == 1) start[start.size() - 6] = NAN;
      if (start_kind == 2) start[start.size() - 1] = 0.0;
      if (!std::isfinite(q.logl_min))
        for (size_t r = 0; r * 6 < start.size(); ++r) start[r * 6 + 4] = -5.0;
      q.seed_u = have ? u.data() : nullptr;
      q.seed_logl = have ? logl.data() : nullptr;
      q.start = have ? start.data() : nullptr;
      long long where = -7;
      const int v = check(q, &where);
      printf("{\"verdict\": %d, \"where\": %lld, \"text\": \"%s\"}\n", v, where, verdict_text(v));
    } else if (!strcmp(word, "sizes")) {
      const int runs = (int)whole(), nlive = (int)whole(), ndim = (int)whole(), K = (int)whole();
      const Sizes s = sizes(runs, nlive, ndim, K);
      printf("{\"seed_fills\": %d, \"stage_points\": %zu, \"stage_bytes\": %zu}\n", s.seed_fills, s.stage_points,
             s.stage_bytes);
    } else {
      return 3;
    }
  }
  return 0;
}
