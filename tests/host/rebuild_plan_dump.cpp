// Prints what rebuild_plan.h decides, for tests/test_rebuild_plan_cpu.py.
// stdin, one shape per line:
//   runs n d mode max_ells node_bytes | num_cu occ_root occ_split occ_tree split_resident_pct coop_launch |
//   fast deep deep_from root_parts wave_ell                                              (17 integers, no bars)
// stdout, one JSON line per shape: {"rc": code, "err": text} or the plan and the scratch layout.
#include <stdio.h>

#include "rebuild_plan.h"

using namespace dh_plan;

int main() {
  static RebuildPlan p;
  static RebuildLayout l;
  RebuildCaps c;
  RebuildSwitches sw;
  int runs, n, d, mode, max_ells, node_bytes;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &runs, &n, &d, &mode, &max_ells, &node_bytes, &c.num_cu,
               &c.occ_root, &c.occ_split, &c.occ_tree, &c.split_resident_pct, &c.coop_launch, &sw.fast, &sw.deep,
               &sw.deep_from, &sw.root_parts, &sw.wave_ell) == 17) {
    char err[kPlanErrLen] = "";
    const int rc = rebuild_plan(runs, n, d, mode, max_ells, c, sw, (size_t)node_bytes, p, err);
    if (rc) {
      printf("{\"rc\": %d, \"err\": \"%s\"}\n", rc, err);
      continue;
    }
    rebuild_layout(p, l);
    printf("{\"rc\": 0, \"max_nodes\": %d, \"reslist_cap\": %d, \"maxw\": %d, \"levels\": %d, \"tps\": %d, \"maxp\": %d, \"fast\": %d, "
           "\"tree_from\": %d, \"tq_cap\": %d, \"kp_cap\": %d, \"fin_extra_off\": %d, \"fin_res_lds\": %d, \"rootbuf_stride\": %zu, "
           "\"prefactor\": %.17g, \"nlev\": %d, \"tail\": %d, \"wave_from\": %d, \"lds\": %zu, \"lds_split\": %zu, \"lds_wave\": %zu, "
           "\"lds_top\": %zu, \"lds_fin\": %zu, \"cap_root\": %d, \"cap_split_level\": %d, \"cap_tree\": %d, \"cap_split\": %d, "
           "\"rp\": %d, \"root_chunk\": %d, \"g_tree\": %d, \"g_out\": %d, \"level\": [",
           p.max_nodes, p.reslist_cap, p.maxw, p.levels, p.tps, p.maxp, p.fast, p.tree_from, p.tq_cap, p.kp_cap, p.fin_extra_off,
           p.fin_res_lds, p.rootbuf_stride, p.prefactor, p.nlev, p.tail, p.wave_from, p.lds, p.lds_split, p.lds_wave, p.lds_top,
           p.lds_fin, p.cap_root, p.cap_split_level, p.cap_tree, p.cap_split, p.rp, p.root_chunk, p.g_tree, p.g_out);
    for (int L = 0; L < p.nlev; ++L) {
      const RebuildLevel& v = p.level[L];
      printf("%s{\"gp\": %d, \"cr\": %d, \"nchunk\": %d, \"ge\": %d, \"ge_l\": %d, \"gw_l\": %d, \"g_ell\": %d, \"wave\": %d, \"top\": %d, "
             "\"tp\": %d, \"lds_ell\": %zu}",
             L ? ", " : "", v.gp, v.cr, v.nchunk, v.ge, v.ge_l, v.gw_l, v.g_ell, v.wave, v.top, v.tp, v.lds_ell);
    }
    printf("], \"slots\": [");
    for (int i = 0; i < kWsArrays; ++i)
      printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", l.slot[i].name, l.slot[i].off, l.slot[i].bytes);
    const RebuildCounters& k = l.cnt;
    printf("], \"total\": %zu, \"counters\": {\"nnodes\": %zu, \"nsplit\": %zu, \"nell\": %zu, \"nparts\": %zu, \"kerr\": %zu, \"kbar\": %zu, "
           "\"kp_top\": %zu, \"tq_ctl\": %zu, \"nbar\": %zu, \"tq_items\": %zu, \"ints\": %zu}}\n",
           l.total, k.nnodes, k.nsplit, k.nell, k.nparts, k.kerr, k.kbar, k.kp_top, k.tq_ctl, k.nbar, k.tq_items, k.ints);
  }
  return 0;
}
