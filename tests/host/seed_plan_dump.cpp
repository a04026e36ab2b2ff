// Prints what merge_plan.h decides for the seeds' choice (merge_seed.hip), for tests/test_seed_plan_cpu.py.
// stdin, one request per line: a word and its numbers
//   check have_run first strands nlive_new logl_min have_info | grid lo M strands | ecap k n_pos |
//   head | select S k ecap | stage S k D | lds
// stdout, one JSON line per request: a verdict with its text, the launch of a pass, a capacity, a layout as
// {"total": bytes of the size pass, "end": bytes of the pointer pass, "slots": [[name, offset, bytes, null], ..]}, or the
// static LDS sizes of the select's kernels.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "merge_plan.h"

using namespace dh_merge;

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
  char word[32], num[64];
  long long v[8];
  while (scanf("%31s", word) == 1) {
    if (!strcmp(word, "check")) {
      long long have, first, strands, k, info;
      if (scanf("%lld %lld %lld %lld %63s %lld", &have, &first, &strands, &k, num, &info) != 6) return 2;
      const int verdict = seed_check(have != 0, first, (int)strands, (int)k, strtod(num, nullptr), info != 0);
      printf("{\"verdict\": %d, \"text\": \"%s\"}\n", verdict, seed_verdict_text(verdict));
      continue;
    }
    const char* kinds[] = {"grid", "ecap", "head", "select", "stage", "lds"};
    const int nargs[] = {3, 2, 0, 3, 3, 0};
    int kind = -1;
    for (int i = 0; i < 6; ++i)
      if (!strcmp(word, kinds[i])) kind = i;
    if (kind < 0) return 2;
    for (int i = 0; i < nargs[kind]; ++i)
      if (scanf("%lld", &v[i]) != 1) return 2;
    const size_t a = (size_t)v[0], b = (size_t)v[1], c = (size_t)v[2];
    switch (kind) {
      case 0: {
        const SeedGrid g = seed_grid(v[0], v[1], (int)v[2]);
        printf("{\"pair0\": %lld, \"npairs\": %lld, \"chunks\": %u, \"tiles\": %u, \"pairs_per_chunk\": %d, \"tile\": %d}\n", g.pair0,
               g.npairs, g.chunks, g.tiles, kT * kSeedPairs, kSeedTile);
        break;
      }
      case 1: printf("{\"ecap\": %zu, \"cap\": %d}\n", seed_ecap((int)v[0], v[1]), kSeedCap); break;
      case 2: { SeedHead s; dump([&](Carver& k) { carve_seed_head(k, s); }); break; }
      case 3: { SeedSelBuf s; dump([&](Carver& k) { carve_seed_select(k, s, a, b, c); }); break; }
      case 4: { SeedStage s; dump([&](Carver& k) { carve_seed_stage(k, s, a, b, c); }); break; }
      default: printf("{\"pass\": %zu, \"rank\": %zu, \"state\": %zu}\n", seed_pass_lds(), seed_rank_lds(), sizeof(SeedState));
    }
  }
  return 0;
}
