// Host driver of tests/test_conv_any_cpu.py: conv_plan (csrc/conv_dispatch.h) for the queries of piso_conv2d_forward_any / piso_conv2d_wgrad_any
// (the run-time-shaped family), walked without a card.  Reads one query per line from stdin
//     any entry H W cin cout ks pad_y pad_x wrap_y wrap_x leaky conv_lds null_ptr operands_off16 result_off16 workspace_bytes
// (workspace_bytes -1: exactly enough for the entry asked, -2: one byte less; any 0: the same query to the *_ex entries) and prints, tab separated:
// status, message (- if none), the 15 fields of the dispatch record the plan would leave, then ex, pad_y, pad_x, wrap_h, wrap_w, groups,
// item_groups, reduce_grid.  A line "inst entry ks cin cout" prints conv_instantiated; "elems ks cin cout" conv_weight_elems_any;
// "ws ks cin cout Ho" conv_wgrad_any_workspace_bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../differentiable-piso_amd/csrc/conv_dispatch.h"

int main() {
  char word[16];
  while (scanf("%15s", word) == 1) {
    if (!strcmp(word, "inst")) {
      int entry, ks, cin, cout;
      if (scanf("%d %d %d %d", &entry, &ks, &cin, &cout) != 4) return 1;
      printf("%d\n", piso::conv_instantiated(entry, ks, cin, cout));
      continue;
    }
    if (!strcmp(word, "elems")) {
      int ks, cin, cout;
      if (scanf("%d %d %d", &ks, &cin, &cout) != 3) return 1;
      printf("%zu\n", piso::conv_weight_elems_any(ks, cin, cout));
      continue;
    }
    if (!strcmp(word, "ws")) {
      int ks, cin, cout, Ho;
      if (scanf("%d %d %d %d", &ks, &cin, &cout, &Ho) != 4) return 1;
      printf("%zu\n", piso::conv_wgrad_any_workspace_bytes(ks, cin, cout, Ho));
      continue;
    }
    int any = atoi(word), entry, H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, leaky, conv_lds, null_ptr, off_op, off_res;
    long long ws;
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld", &entry, &H, &W, &cin, &cout, &ks, &pad_y, &pad_x, &wrap_y, &wrap_x, &leaky, &conv_lds, &null_ptr,
              &off_op, &off_res, &ws) != 16)
      return 1;
    const size_t enough = any ? piso::conv_wgrad_any_workspace_bytes(ks, cin, cout, H + 2 * pad_y - ks + 1) : piso::conv_wgrad_workspace_bytes(ks, cin, cout);
    piso::ConvQuery q{entry, H, W, cin, cout, ks, pad_y, leaky, conv_lds, null_ptr != 0, off_op != 0, off_res != 0,
                      ws == -1 ? enough : ws == -2 ? enough - 1 : (size_t)ws, true, pad_x, wrap_y, wrap_x, any != 0};
    const piso::ConvPlan p = piso::conv_plan(q);
    int r[piso::kConvRecordFields];
    piso::conv_record(p, r);
    printf("%d\t%s", p.status, p.msg ? p.msg : "-");
    for (int v : r) printf("\t%d", v);
    printf("\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", (int)p.ex, p.gx.pad_y, p.gx.pad_x, p.gx.wrap_h, p.gx.wrap_w, p.groups, p.item_groups, p.reduce_grid);
  }
  return 0;
}
