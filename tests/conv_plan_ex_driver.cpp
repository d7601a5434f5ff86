// Host driver of tests/test_conv_wrap_cpu.py: conv_plan (csrc/conv_dispatch.h) for the queries of piso_conv2d_forward_ex / piso_conv2d_wgrad_ex
// (padding per axis, wrap-around per axis), walked without a card.  Reads one query per line from stdin
//     entry H W cin cout ks pad_y pad_x wrap_y wrap_x leaky conv_lds null_ptr operands_off16 result_off16 workspace_bytes   (-1: exactly enough)
// and prints, tab separated: status, message (- if none), the 15 fields of the dispatch record the plan would leave, then the geometry the
// kernels would be handed: ex, pad_y, pad_x, wrap_h, wrap_w (the extent on a wrapped axis, 0 otherwise).
#include <stdio.h>

#include "../differentiable-piso_amd/csrc/conv_dispatch.h"

int main() {
  int entry, H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, leaky, conv_lds, null_ptr, off_op, off_res;
  long long ws;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld", &entry, &H, &W, &cin, &cout, &ks, &pad_y, &pad_x, &wrap_y, &wrap_x, &leaky, &conv_lds,
               &null_ptr, &off_op, &off_res, &ws) == 16) {
    piso::ConvQuery q{entry, H, W, cin, cout, ks, pad_y, leaky, conv_lds, null_ptr != 0, off_op != 0, off_res != 0,
                      ws < 0 ? piso::conv_wgrad_workspace_bytes(ks, cin, cout) : (size_t)ws, true, pad_x, wrap_y, wrap_x};
    const piso::ConvPlan p = piso::conv_plan(q);
    int r[piso::kConvRecordFields];
    piso::conv_record(p, r);
    printf("%d\t%s", p.status, p.msg ? p.msg : "-");
    for (int v : r) printf("\t%d", v);
    printf("\t%d\t%d\t%d\t%d\t%d\n", (int)p.ex, p.gx.pad_y, p.gx.pad_x, p.gx.wrap_h, p.gx.wrap_w);
  }
  return 0;
}
