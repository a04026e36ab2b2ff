// Prints what merge_plan.h decides, for tests/test_merge_plan_cpu.py.
// stdin, one request per line: a word and its integers
//   merged M D pt | scratch M R N D | stage R N D S pt | cov M D | gather n D given | hist two n nbx nby |
//   quantile nq ncol | real M D nreal rwt mean kld | fields M rwt kld | boot M S D cap fields mean | ties M S |
//   tie_scratch M | weights M | arith M D nreal nq ncol n nb
// stdout, one JSON line per request: a layout as {"total": bytes of the size pass, "end": bytes of the pointer pass,
// "slots": [[name, offset, bytes, null], ..]} (the quantile's with "zero": [offset, bytes] of its cleared block), or
// the launch arithmetic of the shape.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "merge_plan.h"

using namespace dh_merge;

// walks a layout as the library does -- without a base, then with one -- and prints the second walk
template <class Layout>
static void dump(Layout&& layout, const char* extra = "") {
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
  printf("]%s}\n", extra);
}

int main() {
  char word[32];
  long long v[8];
  while (scanf("%31s", word) == 1) {
    const char* kinds[] = {"merged", "scratch", "stage", "cov", "gather", "hist", "quantile", "real", "fields", "boot", "ties",
                           "tie_scratch", "weights", "arith"};
    const int nargs[] = {3, 4, 5, 2, 3, 4, 2, 6, 3, 6, 2, 1, 1, 7};
    int kind = -1;
    for (int i = 0; i < 14; ++i)
      if (!strcmp(word, kinds[i])) kind = i;
    if (kind < 0) return 2;
    for (int i = 0; i < nargs[kind]; ++i)
      if (scanf("%lld", &v[i]) != 1) return 2;
    const size_t a = (size_t)v[0], b = (size_t)v[1], c = (size_t)v[2], d = (size_t)v[3];
    switch (kind) {
      case 0: { MergedArrays m; dump([&](Carver& k) { carve_merged(k, m, a, b, v[2] != 0); }); break; }
      case 1: { MergeScratch s; dump([&](Carver& k) { carve_scratch(k, s, a, b, c, d); }); break; }
      case 2: { MergeStage s; dump([&](Carver& k) { carve_stage(k, s, a, b, c, d, v[4] != 0); }); break; }
      case 3: { CovBuf s; dump([&](Carver& k) { carve_cov(k, s, a, b); }); break; }
      case 4: { GatherBuf s; dump([&](Carver& k) { carve_gather(k, s, a, b, v[2] != 0); }); break; }
      case 5: { HistBuf s; dump([&](Carver& k) { carve_hist(k, s, v[0] != 0, b, c, d); }); break; }
      case 6: {
        QuantBuf s;
        Carver base;
        base.base = (char*)(uintptr_t)(1 << 20);
        carve_quantile(base, s, a, b);
        char extra[96];
        snprintf(extra, sizeof extra, ", \"zero\": [%zu, %zu]", (size_t)((char*)s.table - base.base), s.zero_bytes);
        dump([&](Carver& k) { carve_quantile(k, s, a, b); }, extra);
        break;
      }
      case 7: { RealBuf s; dump([&](Carver& k) { carve_real(k, s, a, b, (int)v[2], v[3] != 0, v[4] != 0, v[5] != 0); }); break; }
      case 8: { FieldBuf s; dump([&](Carver& k) { carve_fields(k, s, a, v[1] != 0, v[2] != 0); }); break; }
      case 9: { BootBuf s; dump([&](Carver& k) { carve_boot(k, s, a, b, c, d, v[4] != 0, v[5] != 0); }); break; }
      case 10: { TieArrays s; dump([&](Carver& k) { carve_ties(k, s, a, b); }); break; }
      case 11: { TieScratch s; dump([&](Carver& k) { carve_tie_scratch(k, s, a); }); break; }
      case 12: { WeightBuf s; dump([&](Carver& k) { carve_weights(k, s, a); }); break; }
      default: {
        const long long M = v[0];
        const size_t D = (size_t)v[1];
        const int nreal = (int)v[2], nq = (int)v[3], ncol = (int)v[4], n = (int)v[5];
        const size_t nb = (size_t)v[6];
        long long chunk1, chunk2;
        unsigned groups;
        const int nchunk1 = moment_chunks(M, D + 2, &chunk1), nchunk2 = moment_chunks(M, D * D, &chunk2);
        const long long rows = rows_per_group(M, &groups);
        const QuantTile t = quantile_tile(nq, ncol);
        const int per = hist_per(nb);
        printf("{\"nchunk1\": %d, \"chunk1\": %lld, \"nchunk2\": %d, \"chunk2\": %lld, \"rows\": %lld, \"groups\": %u, \"cpt\": %d, "
               "\"lds_digit\": %zu, \"lds_succ\": %zu, \"combine\": %d, \"per\": %d, \"lds_hist\": %zu, \"lds_int\": %zu, "
               "\"lds_int_mean\": %zu, \"tile\": %zu, \"cap_first\": %zu, \"cap_regrown\": %zu, \"nblk\": %u}\n",
               nchunk1, chunk1, nchunk2, chunk2, rows, groups, t.cpt, t.lds_digit, t.lds_succ, t.combine ? 1 : 0, per,
               hist_lds(per, n, nb), integrate_lds(false), integrate_lds(true), real_tile(nreal), boot_cap_first((size_t)M),
               boot_cap_regrown((size_t)M), blocks_for((size_t)M, kChunk));
      }
    }
  }
  return 0;
}
