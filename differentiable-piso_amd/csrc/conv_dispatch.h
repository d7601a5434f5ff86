// Host side of the closure convolutions' kernel choice (conv.hip): the geometry a kernel is handed, WHICH instances exist (kConvFwd, kConvWg,
// the PACK4 and 64 -> 64 rows, conv_fwd_has_lds: the one statement of it - the planner asks at run time, conv_launch at compile time) and the
// plan of a call (conv_plan: pure, no HIP calls - every refusal of both entry points, the family, every launch dimension, the bands, the
// reducer, i.e. the whole dispatch record).  Plain C++: a host compiler can include this file and walk every plan without a card.
// Beside the instances: the run-time-shaped family of conv_any.hip (ConvQuery::any, conv_plan_any - its own rules: odd kernel sizes up to 9, up to 256
// channels, no alignment rule; the same record with the families CF_FWD_ANY / CF_WG_ANY), reached only through the *_any entries, and
// conv_instantiated: which shapes the instance tables serve, asked of conv_plan itself.
#pragma once
#include <stddef.h>

#include <type_traits>
#include <utility>

#include "../../include/piso_hip.h"

namespace piso {

constexpr int kConvBlock = 256;   // threads of a workgroup (piso_common.h: kBlock; conv.hip holds the two equal)

struct ConvGeom {
  int H, W;          // input rows / columns
  int Ho, Wo;        // output rows / columns
  int pad;           // zero padding on every side
  int cin, cout;     // true channel counts of `in` / `out` (the weight tensor is [KS][KS][CINP][COUTP], zero padded)
};
inline ConvGeom conv_geom(int H, int W, int cin, int cout, int ks, int pad) {
  return ConvGeom{H, W, H + 2 * pad - ks + 1, W + 2 * pad - ks + 1, pad, cin, cout};
}

// The general geometry of piso_conv2d_forward_ex / piso_conv2d_wgrad_ex (the *_ex_kernel instances): padding per axis, and per axis
//     out[y][x][co] = sum over (ky, kx, ci) of in[Y][X][ci] w[ky][kx][ci][co],  Y = y + ky - pad_y, X = x + kx - pad_x
// where a coordinate outside the image contributes nothing on a zero-padded axis and is taken modulo the extent on a WRAPPED one.
struct ConvGeomEx {
  int H, W;
  int Ho, Wo;
  int pad_y, pad_x;
  int wrap_h, wrap_w;  // what a coordinate that left the image is moved by: H / W on a wrapped axis, 0 on a zero-padded one
  int cin, cout;
};
constexpr int kConvGeometryFields = 4;   // piso_conv_last_geometry: pad_y, pad_x, wrap_y, wrap_x

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }
constexpr int ceil_div(int v, int m) { return (v + m - 1) / m; }
constexpr int padded_cin(int cin) { return cin <= 4 ? 4 : round_up(cin, 16); }
// row bands = partial sums per weight: what the second stage has to add (and re-read).  256: one output row per band at config 4's
// size - with bands of two rows the 9 x 126 waves of the 64 -> 64 layer left SIMDs with two waves next to SIMDs with one
constexpr int kWgradMaxBlocks = 256;
inline size_t conv_weight_elems(int ks, int cin, int cout) { return (size_t)ks * ks * padded_cin(cin) * round_up(cout, 16); }
inline size_t conv_wgrad_workspace_bytes(int ks, int cin, int cout) {
  return (size_t)kWgradMaxBlocks * ks * ks * round_up(cin, 16) * round_up(cout, 16) * sizeof(float);
}

// ---- the run-time-shaped family (conv_any.hip: conv_forward_any_kernel<NT, LEAKY>, conv_wgrad_any_kernel<NT>; piso_conv2d_forward_any /
// piso_conv2d_wgrad_any): any odd kernel size up to kConvAnyMaxKs, any channel counts up to kConvAnyMaxChannels.  Output channels are served in
// GROUPS of up to 4 tiles of 16 - the groups are balanced: cout 80 is 5 tiles = 2 groups of NT 3 (the last one partly beyond COUTP, guarded).
constexpr int kConvAnyMaxKs = 9, kConvAnyMaxChannels = 256;
constexpr int kWgradAnyMaxBlocks = 64;   // row bands of conv_wgrad_any_kernel: the workspace of a wide layer stays small (5 x 5, 128 -> 128: 105 MB)
constexpr int conv_any_groups(int cout) { return ceil_div(ceil_div(cout, 16), 4); }
constexpr int conv_any_nt(int cout) { return ceil_div(ceil_div(cout, 16), conv_any_groups(cout)); }
constexpr int conv_any_rows_per_block(int Ho) { return Ho < 1 ? 1 : ceil_div(Ho, kWgradAnyMaxBlocks); }
constexpr int conv_any_nblocks(int Ho) { return Ho < 1 ? 1 : ceil_div(Ho, conv_any_rows_per_block(Ho)); }
// weights of piso_conv2d_forward_any: [ks][ks][CINP4][COUTP], CINP4 = round_up(cin, 4), COUTP = round_up(cout, 16), zero filled
inline size_t conv_weight_elems_any(int ks, int cin, int cout) { return (size_t)ks * ks * round_up(cin, 4) * round_up(cout, 16); }
// partials of piso_conv2d_wgrad_any: [band][ks][ks][CINP16][COUTP], band < conv_any_nblocks(Ho)
inline size_t conv_wgrad_any_workspace_bytes(int ks, int cin, int cout, int Ho) {
  return (size_t)conv_any_nblocks(Ho) * ks * ks * round_up(cin, 16) * round_up(cout, 16) * sizeof(float);
}

// ---- the instances.  A shape is the record's (KS, C, NT, IPW): C = CINP forward (input channels rounded up to 4 or to 16), MTI = CINP16 / 16
// for the weight gradient; NT output-channel tiles of 16; IPW items per wave (weight gradient: enough waves to fill the chip, few enough
// registers for the 4 x 4-pixel prefetch).  Forward: the layers of the closure and of its input-gradient pass (channel roles swapped).
struct ConvShape { int KS, C, NT, IPW; };
inline constexpr ConvShape kConvFwd[] = {{7, 4, 1, 0},  {7, 16, 1, 0}, {5, 16, 1, 0}, {5, 16, 2, 0}, {5, 32, 1, 0}, {3, 32, 4, 0},
                                  {3, 64, 2, 0}, {3, 64, 4, 0}, {1, 64, 4, 0}, {1, 64, 1, 0}, {1, 4, 4, 0}};
inline constexpr ConvShape kConvWg[] = {{7, 1, 1, 3}, {5, 1, 1, 2}, {5, 1, 2, 2}, {3, 2, 4, 1}, {3, 4, 4, 1}, {1, 4, 4, 1}, {1, 4, 1, 1}};
inline constexpr ConvShape kConvWgPack4 = {7, 1, 1, 1};   // conv_wgrad_kernel<.., PACK4>: the first layer
inline constexpr ConvShape kConvWg64 = {3, 4, 4, 1};      // conv_wgrad64[_lds]_kernel<KS>: workgroups of KS waves, one per tap column; grid y = KS tap rows
// conv_with_shape<table>(ks, c, nt, f) calls f(std::integral_constant<size_t, i>) for THE row i of the table with these (KS, C, NT); false - and no call -
// if there is none
template <const auto& T, typename F, size_t... I>
inline bool conv_with_shape_(int ks, int c, int nt, F&& f, std::index_sequence<I...>) {
  return (... || (T[I].KS == ks && T[I].C == c && T[I].NT == nt && (f(std::integral_constant<size_t, I>{}), true)));
}
template <const auto& T, typename F>
inline bool conv_with_shape(int ks, int c, int nt, F&& f) {
  return conv_with_shape_<T>(ks, c, nt, f, std::make_index_sequence<sizeof(T) / sizeof(T[0])>{});
}
// forward: a form with the operands staged through LDS exists (tap columns share the staged pixels; channels in blocks of 16)
constexpr bool conv_fwd_has_lds(int ks, int cinp) { return cinp >= 16 && ks >= 3; }
// forward, CINP >= 16: every operand is a 16-byte load (both forms)
constexpr bool conv_fwd_loads16(int cinp) { return cinp >= 16; }
// (measured: 304 us against 329 us for the generic kernel at 250 x 876; the 1 x 1 layer has a single tap, i.e. one busy wave per workgroup
// there, and stays on the generic kernel: 130 us against 219 us)
constexpr bool conv_wg_is_64(int ks, int cin, int cout) { return ks == kConvWg64.KS && cin == 64 && cout == 64; }
constexpr bool conv_wg_is_pack4(int ks, int cin, int nt) { return ks == kConvWgPack4.KS && cin <= 4 && nt == kConvWgPack4.NT; }
// weight gradient: the channel counts whose 16-byte forms exist - the staged generic kernel, both 64 -> 64 kernels load `in` and `grad_out`
// that way.  Option conv_lds decides whether a staged form RUNS, never what a call must satisfy: the alignment rule asks this, not the family
constexpr bool conv_wg_loads16(int cin, int cout) { return cin % 4 == 0 && cout % 4 == 0; }
// ... and the 4-wide reducer reads the partials and writes dw with 16-byte accesses
constexpr int conv_wg_reducer(int cout) { return cout % 4 == 0 ? 4 : 1; }

// ---- the plan: everything an entry point decides before it launches
enum { CE_FORWARD = 1, CE_WGRAD = 2 };
enum { CF_FWD_DIRECT = 0, CF_FWD_LDS, CF_WG_GENERIC, CF_WG_GENERIC_LDS, CF_WG_PACK4, CF_WG_64, CF_WG_64_LDS, CF_FWD_ANY, CF_WG_ANY };
struct ConvQuery {
  int entry;                         // CE_FORWARD (piso_conv2d_forward) | CE_WGRAD (piso_conv2d_wgrad)
  int H, W, cin, cout, ks, pad;
  int leaky;                         // forward: leaky_out as passed
  int conv_lds;                      // option value (-1: not set)
  bool null_ptr;                     // one of the entry's pointers is NULL
  bool operands_off16, result_off16; // not 16-byte aligned: `in` or the second operand (w_laid_out / grad_out); wgrad: dw or workspace
  size_t workspace_bytes;            // wgrad
  // the *_ex entries: `pad` is pad_y, and
  bool ex = false;
  int pad_x = 0;
  int wrap_y = 0, wrap_x = 0;        // != 0: the axis is periodic
  // the *_any entries (always with the fields of `ex`): the run-time-shaped family, whatever the instance tables hold
  bool any = false;
};
constexpr int kConvRecordFields = 15;
struct ConvPlan {
  int status = PISO_OK;              // != PISO_OK: the call is refused with `msg`, nothing else of the plan is to be used
  const char* msg = nullptr;
  ConvGeom g;                        // (a *_ex plan: Ho, Wo, cin, cout as launched; pad = pad_y)
  bool ex = false;                   // the *_ex_kernel twins run, with
  ConvGeomEx gx;
  // the dispatch record (include/piso_hip.h: piso_conv_last_dispatch; with g.Ho, g.Wo) = the launch of the main kernel: grid (grid_x, grid_y), block
  int entry, KS, C, NT, IPW, family, leaky, grid_x, grid_y, block, rows_per_block, nblocks, reducer;
  int reduce_grid;                   // gridDim.x of the reducer
  // family CF_FWD_ANY / CF_WG_ANY: groups of NT output-channel tiles.  grid_y: forward - the groups;  wgrad - item_groups x groups, item_groups
  // workgroups of four waves over the work items (tap, 16-channel tile of ci), one item per wave: blockIdx.y = group * item_groups + item group
  int groups = 1, item_groups = 1;
};
inline void conv_record(const ConvPlan& p, int (&r)[kConvRecordFields]) {
  const int v[kConvRecordFields] = {p.entry, p.KS, p.C, p.NT, p.IPW, p.family, p.leaky, p.grid_x, p.grid_y, p.block, p.rows_per_block, p.nblocks, p.reducer,
                                    p.g.Ho, p.g.Wo};
  for (int i = 0; i < kConvRecordFields; ++i) r[i] = v[i];
}

// the plan of a *_any call: its own rules (no instance table, no alignment rule), the same record
inline ConvPlan conv_plan_any(const ConvQuery& q) {
  ConvPlan p{};
  const bool fwd = q.entry == CE_FORWARD;
  const auto refuse = [&p, fwd](const char* f, const char* w) { p.status = PISO_ERR_INVALID_ARG; p.msg = fwd ? f : w; return p; };
  const int cin = q.cin, cout = q.cout, ks = q.ks;
  p.g = conv_geom(q.H, q.W, cin, cout, ks, q.pad);
  p.g.Wo = q.W + 2 * q.pad_x - ks + 1;
  p.ex = true;
  p.gx = ConvGeomEx{q.H, q.W, p.g.Ho, p.g.Wo, q.pad, q.pad_x, q.wrap_y ? q.H : 0, q.wrap_x ? q.W : 0, cin, cout};
  if (q.null_ptr) return refuse("piso_conv2d_forward_any: invalid argument (a pointer is NULL)", "piso_conv2d_wgrad_any: invalid argument (a pointer is NULL)");
  if (ks < 1 || ks > kConvAnyMaxKs || ks % 2 == 0)
    return refuse("piso_conv2d_forward_any: invalid argument (kernel size: odd, 1 .. 9)", "piso_conv2d_wgrad_any: invalid argument (kernel size: odd, 1 .. 9)");
  if (cin < 1 || cin > kConvAnyMaxChannels || cout < 1 || cout > kConvAnyMaxChannels)
    return refuse("piso_conv2d_forward_any: invalid argument (channels: 1 .. 256 in, 1 .. 256 out)", "piso_conv2d_wgrad_any: invalid argument (channels: 1 .. 256 in, 1 .. 256 out)");
  if (q.H < 1 || q.W < 1 || q.pad < 0 || q.pad_x < 0 || p.g.Ho < 1 || p.g.Wo < 1)
    return refuse("piso_conv2d_forward_any: invalid argument (the output needs at least one row and one column: H + 2 pad_y - ks + 1 >= 1, W + 2 pad_x - ks + 1 >= 1)",
                  "piso_conv2d_wgrad_any: invalid argument (the output needs at least one row and one column: H + 2 pad_y - ks + 1 >= 1, W + 2 pad_x - ks + 1 >= 1)");
  if (!fwd && q.workspace_bytes < conv_wgrad_any_workspace_bytes(ks, cin, cout, p.g.Ho))
    return refuse("", "piso_conv2d_wgrad_any: invalid argument (workspace_bytes is below piso_conv2d_wgrad_any_workspace_bytes(ks, cin, cout, Ho))");
  if ((q.wrap_y && q.pad != ks / 2) || (q.wrap_x && q.pad_x != ks / 2))
    return refuse("piso_conv2d_forward_any: invalid argument (a wrapped axis must have pad == ks / 2: it keeps its extent, and the adjoint is again such a convolution)",
                  "piso_conv2d_wgrad_any: invalid argument (a wrapped axis must have pad == ks / 2: it keeps its extent, and the adjoint is again such a convolution)");
  if ((q.wrap_y && q.H < q.pad) || (q.wrap_x && q.W < q.pad_x))
    return refuse("piso_conv2d_forward_any: invalid argument (a wrapped axis must have an extent >= its pad: an index wraps at most once)",
                  "piso_conv2d_wgrad_any: invalid argument (a wrapped axis must have an extent >= its pad: an index wraps at most once)");
  p.entry = q.entry; p.KS = ks; p.block = kConvBlock;
  p.groups = conv_any_groups(cout); p.NT = conv_any_nt(cout);
  if (fwd) {
    p.C = round_up(cin, 4);
    p.family = CF_FWD_ANY;
    p.leaky = q.leaky != 0;
    p.grid_x = ceil_div(ceil_div(p.g.Wo, 64) * p.g.Ho, kConvBlock / 64);
    p.grid_y = p.groups;
    return p;
  }
  p.C = ceil_div(cin, 16);
  p.IPW = 1; p.family = CF_WG_ANY;
  p.item_groups = ceil_div(ks * ks * p.C, kConvBlock / 64);
  p.grid_y = p.item_groups * p.groups;
  p.rows_per_block = conv_any_rows_per_block(p.g.Ho);
  p.grid_x = p.nblocks = conv_any_nblocks(p.g.Ho);
  // (the 4-wide reducer needs `dw` and `workspace` 16-byte aligned; the scalar one adds the same bands in the same order: no alignment rule)
  p.reducer = q.result_off16 ? 1 : conv_wg_reducer(cout);
  const int n = ks * ks * cin * cout;
  p.reduce_grid = p.reducer == 4 ? ceil_div(n / 4, 64) : ceil_div(n, 64);
  return p;
}

inline ConvPlan conv_plan(const ConvQuery& q) {
  if (q.any) return conv_plan_any(q);
  ConvPlan p{};
  const auto refuse = [&p](const char* msg) { p.status = PISO_ERR_INVALID_ARG; p.msg = msg; return p; };
  p.g = conv_geom(q.H, q.W, q.cin, q.cout, q.ks, q.pad);
  p.ex = q.ex;
  if (q.ex) {
    p.g.Wo = q.W + 2 * q.pad_x - q.ks + 1;
    p.gx = ConvGeomEx{q.H, q.W, p.g.Ho, p.g.Wo, q.pad, q.pad_x, q.wrap_y ? q.H : 0, q.wrap_x ? q.W : 0, q.cin, q.cout};
  }
  const ConvGeom& g = p.g;
  const int cin = q.cin, cout = q.cout, ks = q.ks;
  // the two rules of a wrapped axis (after the entry's own argument checks, below)
  const auto wrap_refusal = [&q]() -> const char* {
    const bool fwd = q.entry == CE_FORWARD;
    if (!q.ex) return nullptr;
    if ((q.wrap_y && q.pad != q.ks / 2) || (q.wrap_x && q.pad_x != q.ks / 2))
      return fwd ? "piso_conv2d_forward_ex: invalid argument (a wrapped axis must have pad == ks / 2: it keeps its extent, and the adjoint is again such a convolution)"
                 : "piso_conv2d_wgrad_ex: invalid argument (a wrapped axis must have pad == ks / 2: it keeps its extent, and the adjoint is again such a convolution)";
    if ((q.wrap_y && q.H < q.pad) || (q.wrap_x && q.W < q.pad_x))
      return fwd ? "piso_conv2d_forward_ex: invalid argument (a wrapped axis must have an extent >= its pad: an index wraps at most once)"
                 : "piso_conv2d_wgrad_ex: invalid argument (a wrapped axis must have an extent >= its pad: an index wraps at most once)";
    return nullptr;
  };
  const bool sizes_ok = g.Ho >= 1 && g.Wo >= 1 && cin >= 1 && cout >= 1 && cout <= 64 && cin <= 64;
  const bool lds = q.conv_lds != 0;                          // (option conv_lds 0: the direct kernels)
  p.entry = q.entry; p.KS = ks; p.NT = round_up(cout, 16) / 16; p.grid_y = 1; p.block = kConvBlock;
  if (q.entry == CE_FORWARD) {
    if (q.null_ptr || !sizes_ok || (cin > 4 && cin % 16 != 0))
      return refuse("piso_conv2d_forward: invalid argument (channels: 1..4 or a multiple of 16 up to 64 in, 1..64 out; kernel size 1 | 3 | 5 | 7)");
    p.C = padded_cin(cin);
    if (conv_fwd_loads16(p.C) && q.operands_off16)
      return refuse("piso_conv2d_forward: invalid argument (with more than 4 input channels `in` and `w_laid_out` must be 16-byte aligned)");
    if (!conv_with_shape<kConvFwd>(ks, p.C, p.NT, [](auto) {})) return refuse("piso_conv2d_forward: this (kernel size, channels) combination is not instantiated");
    if (const char* why = wrap_refusal()) return refuse(why);
    p.family = lds && conv_fwd_has_lds(ks, p.C) ? CF_FWD_LDS : CF_FWD_DIRECT;
    p.leaky = q.leaky != 0;
    p.grid_x = ceil_div(ceil_div(g.Wo, 64) * g.Ho, kConvBlock / 64);       // a wave owns a tile of 64 pixels of one output row
    return p;
  }
  if (q.null_ptr || !sizes_ok || q.workspace_bytes < conv_wgrad_workspace_bytes(ks, cin, cout)) return refuse("piso_conv2d_wgrad: invalid argument");
  if (const char* why = wrap_refusal()) return refuse(why);
  p.C = round_up(cin, 16) / 16;
  p.reducer = conv_wg_reducer(cout);
  if ((p.reducer == 4 && q.result_off16) || (conv_wg_loads16(cin, cout) && q.operands_off16))
    return refuse("piso_conv2d_wgrad: invalid argument (cout % 4 == 0: `dw` and `workspace` must be 16-byte aligned; cin % 4 == 0 as well: `in` and `grad_out` too)");
  // grid y: the work items of a band - (tap, 16-channel tile of ci); PACK4: (ky, group of 4 kx) - over workgroups of four waves x IPW items
  if (conv_wg_is_64(ks, cin, cout)) {
    p.IPW = kConvWg64.IPW; p.family = lds ? CF_WG_64_LDS : CF_WG_64;
    p.grid_y = ks; p.block = 64 * ks;
  } else if (conv_wg_is_pack4(ks, cin, p.NT)) {
    p.IPW = kConvWgPack4.IPW; p.family = CF_WG_PACK4;
    p.grid_y = ceil_div(ks * ceil_div(ks, 4), 4 * p.IPW);
  } else if (conv_with_shape<kConvWg>(ks, p.C, p.NT, [&p](auto i) { p.IPW = kConvWg[i].IPW; })) {
    p.family = lds && conv_wg_loads16(cin, cout) ? CF_WG_GENERIC_LDS : CF_WG_GENERIC;
    p.grid_y = ceil_div(ks * ks * p.C, 4 * p.IPW);
  } else {
    return refuse("piso_conv2d_wgrad: this (kernel size, channels) combination is not instantiated");
  }
  p.rows_per_block = ceil_div(g.Ho, kWgradMaxBlocks);
  p.grid_x = p.nblocks = ceil_div(g.Ho, p.rows_per_block);
  const int n = ks * ks * cin * cout;                        // the reducers: 64 weights (scalar) or 64 x 4 (4-wide) per workgroup
  p.reduce_grid = p.reducer == 4 ? ceil_div(n / 4, 64) : ceil_div(n, 64);
  return p;
}

// piso_conv2d_instantiated: do the fixed tables serve (entry, ks, cin, cout)?  The answer of conv_plan itself, for a call of the old entry that
// nothing else could refuse: the smallest image, aligned pointers, enough workspace
inline int conv_instantiated(int entry, int ks, int cin, int cout) {
  if ((entry != CE_FORWARD && entry != CE_WGRAD) || ks < 1 || cin < 1 || cout < 1 || cin > 64 || cout > 64) return 0;
  const ConvQuery q{entry, ks, ks, cin, cout, ks, 0, 0, -1, false, false, false, conv_wgrad_workspace_bytes(ks, cin, cout)};
  return conv_plan(q).status == PISO_OK ? 1 : 0;
}

}  // namespace piso
