// Host driver of tests/test_mg_slab_plan_cpu.py: mg_slab_plan (csrc/mg_slab_plan.h) is pure C++, so the whole shape of a slab multigrid solve
// can be walked without a card.  Reads one query per line from stdin
//     nx ny world gather_cells                 (gather_cells 0: no knob, the limit is kGatherCells)
// and prints, tab separated: the flat plan record (status, levels, g, tail_first, rows of level 0 per rank, ranks, then nx ny rows per
// level), a '|', the collectives one iteration issues at two sweeps (exchanges, all-reduces, all-gathers), a '|', the message (- if none).
#include <stdio.h>

#include "../differentiable-piso_amd/csrc/mg_slab_plan.h"

int main() {
  int nx, ny, world, knob;
  while (scanf("%d %d %d %d", &nx, &ny, &world, &knob) == 4) {
    const piso::MgSlabPlan p = piso::mg_slab_plan(nx, ny, world, knob);
    int rec[piso::kMgSlabPlanHead + 3 * piso::kPlanMaxLevels];
    const int n = piso::mg_slab_plan_record(p, rec, (int)(sizeof(rec) / sizeof(rec[0])));
    for (int i = 0; i < n; ++i) printf("%d\t", rec[i]);
    if (p.status == 0) {
      const piso::MgSlabCollectives c = piso::mg_slab_collectives(p, 2);
      printf("|\t%d\t%d\t%d\t", c.exchanges, c.allreduces, c.allgathers);
    } else {
      printf("|\t0\t0\t0\t");
    }
    printf("|\t%s\n", p.msg[0] ? p.msg : "-");
  }
  return 0;
}
