// Prints the layouts of stage_plan.h, for tests/test_stage_plan_cpu.py.
// stdin, one request per line: a word and its integers
//   propose k ndim ncdim m idx bc | rwalk k ndim ncdim m idx bc philox | eval k ndim | seed k n_words | stream nn nu |
//   slice k ndim m idx philox | unif k ndim ncdim m bc philox | unif_friends k ndim n bc rng32 rng32_out |
//   bound_draw nsamp d m | slice_feed k ndim kind m nlook idx consumed | friends_update n d nboot prev |
//   friends_batch R n d nboot ws_bytes prev active | friends_within n d m bits | friends_draw nsamp n d |
//   rebuild n d max_ells leaf | ell_from_cov m d | improve_cov m d | scale_logvol m d | boot_expand runs n d ws_bytes |
//   contains k d m mask quad | ns_consume R N K run_bytes pt |
//   contains_runs runs wpr d max_ells nells run_mode bstatus first | enlarge_runs runs max_ells d active run_shift
// stdout, one JSON line per request: {"total": bytes of the size pass, "end": bytes of the pointer pass,
// "slots": [[name, offset, bytes, null], ..]}
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "stage_plan.h"

using namespace dh_stage;
using dh_carve::Slot;

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
  const char* kinds[] = {"propose",       "rwalk",          "eval",         "seed",    "stream",      "slice",       "unif",
                         "unif_friends",  "bound_draw",     "slice_feed",   "friends_update", "friends_batch",
                         "friends_within", "friends_draw",  "rebuild",      "ell_from_cov", "improve_cov", "scale_logvol",
                         "boot_expand",   "contains",       "ns_consume",   "contains_runs",
                         "enlarge_runs"};
  const int nargs[] = {6, 7, 2, 2, 2, 5, 6, 6, 3, 7, 4, 7, 4, 3, 4, 2, 2, 2, 4, 5, 5, 8, 5};
  const int nkinds = (int)(sizeof nargs / sizeof nargs[0]);
  while (scanf("%31s", word) == 1) {
    int kind = -1;
    for (int i = 0; i < nkinds; ++i)
      if (!strcmp(word, kinds[i])) kind = i;
    if (kind < 0) return 2;
    for (int i = 0; i < nargs[kind]; ++i)
      if (scanf("%lld", &v[i]) != 1) return 2;
    const size_t a = (size_t)v[0], b = (size_t)v[1], c = (size_t)v[2], d = (size_t)v[3], e = (size_t)v[4];
    switch (kind) {
      case 0: { RwalkProposeBuf s; dump([&](Carver& k) { carve_rwalk_propose(k, s, a, b, c, d, v[4] != 0, v[5] != 0); }); break; }
      case 1: { RwalkBatchBuf s; dump([&](Carver& k) { carve_rwalk_batch(k, s, a, b, c, d, v[4] != 0, v[5] != 0, v[6] != 0); }); break; }
      case 2: { EvalBuf s; dump([&](Carver& k) { carve_eval(k, s, a, b); }); break; }
      case 3: { SeedChildrenBuf s; dump([&](Carver& k) { carve_seed_children(k, s, a, b); }); break; }
      case 4: { RngStreamBuf s; dump([&](Carver& k) { carve_rng_stream(k, s, a, b); }); break; }
      case 5: { SliceBatchBuf s; dump([&](Carver& k) { carve_slice_batch(k, s, a, b, c, v[3] != 0, v[4] != 0); }); break; }
      case 6: { UnifBatchBuf s; dump([&](Carver& k) { carve_unif_batch(k, s, a, b, c, d, v[4] != 0, v[5] != 0); }); break; }
      case 7: { UnifFriendsBuf s; dump([&](Carver& k) { carve_unif_friends(k, s, a, b, c, v[3] != 0, v[4] != 0, v[5] != 0); }); break; }
      case 8: { BoundDrawBuf s; dump([&](Carver& k) { carve_bound_draw(k, s, a, b, c); }); break; }
      case 9: { SliceFeedBuf s; dump([&](Carver& k) { carve_slice_feed(k, s, a, b, (int)v[2], d, e, v[5] != 0, v[6] != 0); }); break; }
      case 10: { FriendsUpdateBuf s; dump([&](Carver& k) { carve_friends_update(k, s, a, b, c, v[3] != 0); }); break; }
      case 11: { FriendsBatchBuf s; dump([&](Carver& k) { carve_friends_batch(k, s, a, b, c, d, e, v[5] != 0, v[6] != 0); }); break; }
      case 12: { FriendsWithinBuf s; dump([&](Carver& k) { carve_friends_within(k, s, a, b, c, v[3] != 0); }); break; }
      case 13: { FriendsDrawBuf s; dump([&](Carver& k) { carve_friends_draw(k, s, a, b, c); }); break; }
      case 14: { RebuildBuf s; dump([&](Carver& k) { carve_rebuild(k, s, a, b, c, v[3] != 0); }); break; }
      case 15: { EllFromCovBuf s; dump([&](Carver& k) { carve_ell_from_cov(k, s, a, b); }); break; }
      case 16: { ImproveCovBuf s; dump([&](Carver& k) { carve_improve_cov(k, s, a, b); }); break; }
      case 17: { ScaleLogvolBuf s; dump([&](Carver& k) { carve_scale_logvol(k, s, a, b); }); break; }
      case 18: { BootExpandBuf s; dump([&](Carver& k) { carve_boot_expand(k, s, a, b, c, d); }); break; }
      case 19: { ContainsBuf s; dump([&](Carver& k) { carve_contains(k, s, a, b, c, v[3] != 0, v[4] != 0); }); break; }
      case 21: { ContainsRunsBuf s; dump([&](Carver& k) { carve_contains_runs(k, s, a, b, c, d, v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0); }); break; }
      case 22: { EnlargeRunsBuf s; dump([&](Carver& k) { carve_enlarge_runs(k, s, a, b, c, v[3] != 0, v[4] != 0); }); break; }
      default: { NsConsumeBuf s; dump([&](Carver& k) { carve_ns_consume(k, s, a, b, c, d, v[4] != 0); }); break; }
    }
  }
  return 0;
}
