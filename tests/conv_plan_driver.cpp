// Host driver of tests/test_gpu_conv_dispatch.py::test_conv_plan_on_the_host: conv_plan (csrc/conv_dispatch.h) is pure C++, so the whole kernel
// choice of the closure convolutions can be walked without a card.  Reads one query per line from stdin
//     entry H W cin cout ks pad leaky conv_lds null_ptr operands_off16 result_off16 workspace_bytes      (workspace_bytes -1: exactly enough)
// and prints, tab separated: status, message (- if none), the 15 fields of the dispatch record the plan would leave.
#include <stdio.h>

#include "../differentiable-piso_amd/csrc/conv_dispatch.h"

int main() {
  int entry, H, W, cin, cout, ks, pad, leaky, conv_lds, null_ptr, off_op, off_res;
  long long ws;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %lld", &entry, &H, &W, &cin, &cout, &ks, &pad, &leaky, &conv_lds, &null_ptr, &off_op, &off_res, &ws) == 13) {
    piso::ConvQuery q{entry, H, W, cin, cout, ks, pad, leaky, conv_lds, null_ptr != 0, off_op != 0, off_res != 0,
                      ws < 0 ? piso::conv_wgrad_workspace_bytes(ks, cin, cout) : (size_t)ws};
    const piso::ConvPlan p = piso::conv_plan(q);
    int r[piso::kConvRecordFields];
    piso::conv_record(p, r);
    printf("%d\t%s", p.status, p.msg ? p.msg : "-");
    for (int v : r) printf("\t%d", v);
    printf("\n");
  }
  return 0;
}
