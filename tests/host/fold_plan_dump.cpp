// Prints what merge_plan.h decides for the fold of dynamic batches (merge_fold.hip), for tests/test_fold_plan_cpu.py.
// stdin, one request per line: a word and its integers
//   batch T | fold_scratch M W R N D pt | fold_stage R N D S pt | gather_rows n D | merged M D pt | lds
// stdout, one JSON line per request: a layout as {"total": bytes of the size pass, "end": bytes of the pointer pass,
// "slots": [[name, offset, bytes, null], ..]}, or the static LDS sizes of the fold's kernels.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "merge_plan.h"

using namespace dh_merge;

// walks a layout as the library does -- without a base, then with one -- and prints the second walk
template <class Layout>
static void dump(Layout&& layout) {
  static Slot log[64];
  Carver size;
  layout(size);
  Carver place;
  place.base = (char*)(uintptr_t)(1 << 20);  // never dereferenced
  place.log = log;
  layout(place);
  printf("{\"total\": %zu, \"end\": %zu, \"slots\": [", size.off, place.off);
  for (int i = 0; i < place.nlog; ++i)
    printf("%s[\"%s\", %zu, %zu, %s]", i ? ", " : "", log[i].name, log[i].off, log[i].bytes, log[i].null ? "true" : "false");
  printf("]}\n");
}

int main() {
  char word[32];
  long long v[8];
  while (scanf("%31s", word) == 1) {
    const char* kinds[] = {"batch", "fold_scratch", "fold_stage", "gather_rows", "merged", "lds"};
    const int nargs[] = {1, 6, 5, 2, 3, 0};
    int kind = -1;
    for (int i = 0; i < 6; ++i)
      if (!strcmp(word, kinds[i])) kind = i;
    if (kind < 0) return 2;
    for (int i = 0; i < nargs[kind]; ++i)
      if (scanf("%lld", &v[i]) != 1) return 2;
    const size_t a = (size_t)v[0], b = (size_t)v[1], c = (size_t)v[2], d = (size_t)v[3], e = (size_t)v[4];
    switch (kind) {
      case 0: { BatchArrays s; dump([&](Carver& k) { carve_batch(k, s, a); }); break; }
      case 1: { FoldScratch s; dump([&](Carver& k) { carve_fold_scratch(k, s, a, b, c, d, e, v[5] != 0); }); break; }
      case 2: { MergeStage s; dump([&](Carver& k) { carve_fold_stage(k, s, a, b, c, d, v[4] != 0); }); break; }
      case 3: { GatherBuf s; dump([&](Carver& k) { carve_gather_rows(k, s, a, b); }); break; }
      case 4: { MergedArrays s; dump([&](Carver& k) { carve_merged(k, s, a, b, v[2] != 0); }); break; }
      default: printf("{\"rank\": %zu, \"scan\": %zu}\n", fold_rank_lds(), fold_scan_lds());
    }
  }
  return 0;
}
