// The run-time-shaped family of the closure convolutions (gfx950 MFMA, exact fp32: v_mfma_f32_16x16x4_f32): kernel size and channel counts
// are kernel ARGUMENTS, so any odd kernel size up to 9 and any channel counts up to 256 run on the matrix cores - the shapes the tuned, fixed
// instances of conv.hip (conv_dispatch.h: kConvFwd, kConvWg, ...) do not hold.  Reached through piso_conv2d_forward_any / piso_conv2d_wgrad_any
// only; a translation unit of its own, so that no kernel of conv.hip is compiled next to these.
//   conv_forward_any_kernel<NT, LEAKY>   the tiling of conv_forward_kernel: a wave owns 64 consecutive pixels of one output row (four M tiles),
//                  a workgroup four such tiles; blockIdx.y is a GROUP of NT <= 4 tiles of 16 output channels (cout > 64: more groups, not more
//                  registers).  One K step = 4 input channels of one tap, K order (tap row, tap column, block of 4 channels); weights
//                  [ks][ks][CINP4][COUTP].  Every operand is a guarded 4-byte load: no alignment rule.
//   conv_wgrad_any_kernel<NT>            the structure of conv_wgrad_kernel with one work item (tap, 16-channel tile of ci) per wave; row bands
//                  write the partials [band][ks][ks][CINP16][COUTP] that the two reducers of conv.hip add in a fixed order.
// The geometry is the general one (ConvGeomEx: padding per axis, wrap-around per axis).  What a call is refused for, and every launch dimension:
// conv_dispatch.h (conv_plan_any).
#include "piso_common.h"
#include "conv_any.h"

namespace piso {

static_assert(kConvBlock == kBlock, "conv_dispatch.h plans workgroups of kBlock threads");

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kLeakySlopeAny = 0.2f;

// a coordinate that left a wrapped axis re-enters on the other side (conv_plan: pad <= extent there - one conditional add or subtract); `wrap`
// is 0 on a zero-padded axis: the coordinate stays as it is and fails the bounds test that follows
__device__ __forceinline__ int wrapped_any(int v, int extent, int wrap) {
  v += v < 0 ? wrap : 0;
  return v - (v >= extent ? wrap : 0);
}

template <int NT, bool LEAKY_OUT>
__global__ __launch_bounds__(kBlock) void conv_forward_any_kernel(ConvGeomEx g, const float* __restrict__ in, const float* __restrict__ w,
                                                                   float* __restrict__ out, int ks, int cinp4, int coutp) {
  constexpr int MT = 4;                                     // 4 x 16 = 64 pixels per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (g.Wo + 16 * MT - 1) / (16 * MT);
  const int tile = blockIdx.x * (kBlock / 64) + wave;
  if (tile >= tiles_x * g.Ho) return;
  const int y = tile / tiles_x, x0 = (tile - y * tiles_x) * 16 * MT;
  const int ai = lane & 15, ak = lane >> 4;                 // A: pixel in tile, channel of the K step;  B: channel = ak, co = ai
  const int co0 = blockIdx.y * 16 * NT;                     // this group's first output channel
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nblk = cinp4 >> 2, nseq = ks * nblk;            // K steps of a tap row: (tap column, block of 4 channels)
  for (int ky = 0; ky < ks; ++ky) {
    const int yy = wrapped_any(y + ky - g.pad_y, g.H, g.wrap_h);
    if (yy < 0 || yy >= g.H) continue;                       // (wave-uniform: a whole tap row of zero padding; a wrapped row is never outside)
    const float* inrow = in + (size_t)yy * g.W * g.cin;
    const float* wrow = w + (size_t)ky * ks * cinp4 * coutp + co0 + ai;
    int kxn = 0, blkn = 0;                                   // the K step the next load_ab fetches
    auto load_ab = [&](float (&a)[MT], float (&b)[NT]) __attribute__((always_inline)) {
      const int c = 4 * blkn + ak;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int xx = wrapped_any(x0 + 16 * m + ai + kxn - g.pad_x, g.W, g.wrap_w);
        a[m] = (xx >= 0 && xx < g.W && c < g.cin) ? inrow[(size_t)xx * g.cin + c] : 0.f;
      }
#pragma unroll
      for (int n = 0; n < NT; ++n)                           // (a tile beyond COUTP - the last group of a balanced split - reads as zero)
        b[n] = (co0 + 16 * n < coutp) ? wrow[((size_t)kxn * cinp4 + c) * coutp + 16 * n] : 0.f;
      if (++blkn == nblk) { blkn = 0; ++kxn; }
    };
    // software pipeline: the operands of step s + 1 are loaded before the MT NT MFMAs of step s are issued
    float a0[MT], b0[NT], a1[MT], b1[NT];
    load_ab(a0, b0);
    for (int s = 0; s < nseq; s += 2) {
      if (s + 1 < nseq) load_ab(a1, b1);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[m], b0[n], acc[m][n], 0, 0, 0);
      if (s + 1 < nseq) {
        if (s + 2 < nseq) load_ab(a0, b0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[m], b1[n], acc[m][n], 0, 0, 0);
      }
    }
  }
  // C/D layout: column (co) = lane & 15, row (pixel) = (lane >> 4) * 4 + register
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int co = co0 + 16 * n + ai;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = x0 + 16 * m + ak * 4 + r;
        if (x < g.Wo && co < g.cout) {
          float v = acc[m][n][r];
          if (LEAKY_OUT) v = v > 0.f ? v : kLeakySlopeAny * v;
          out[((size_t)y * g.Wo + x) * g.cout + co] = v;
        }
      }
    }
}

// Weight gradient.  blockIdx.y = group * item_groups + item group: wave w of the workgroup owns the work item 4 (item group) + w = (tap, 16-channel
// tile of ci) x the NT tiles of co of its group, and reduces the output rows of band blockIdx.x into part[band][ks][ks][CINP16][COUTP].  The K loop
// (pixels) is unrolled 4 x 4 pixels with every operand load issued before the first MFMA, as in conv_wgrad_kernel.
template <int NT>
__global__ __launch_bounds__(kBlock) void conv_wgrad_any_kernel(ConvGeomEx g, const float* __restrict__ in, const float* __restrict__ gout,
                                                                 float* __restrict__ part, int rows_per_block, int ks, int mti, int item_groups, int coutp) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = lane & 15, ak = lane >> 4;                 // A: ci = ai, pixel-in-step = ak;  B: pixel-in-step = ak, co = ai
  const int grp = blockIdx.y / item_groups, item = (blockIdx.y - grp * item_groups) * (kBlock / 64) + wave;
  const int taps = ks * ks, cinp16 = 16 * mti;
  if (item >= taps * mti) return;
  const int tap = item / mti, mt = item - tap * mti;
  const int ky = tap / ks, kx = tap - ky * ks;
  const int ci = 16 * mt + ai, co0 = grp * 16 * NT;
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int y_begin = blockIdx.x * rows_per_block, y_end = min(y_begin + rows_per_block, g.Ho);
  for (int y = y_begin; y < y_end; ++y) {
    const int yy = wrapped_any(y + ky - g.pad_y, g.H, g.wrap_h);
    if (yy < 0 || yy >= g.H) continue;                       // (wave-uniform; zero padding only: a wrapped row is never outside)
    const float* inrow = in + (size_t)yy * g.W * g.cin + ci;
    const float* grow = gout + (size_t)y * g.Wo * g.cout + co0 + ai;
    for (int x0 = 0; x0 < g.Wo; x0 += 4 * U) {
      float a[U], b[U][NT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int x = x0 + 4 * u + ak;
        const int xx = wrapped_any(x + kx - g.pad_x, g.W, g.wrap_w);
        // (a pixel whose tap leaves the image is no term of this wave's weights: neither operand is read - 0 x NaN would be NaN)
        const bool term = x < g.Wo && xx >= 0 && xx < g.W;
#pragma unroll
        for (int n = 0; n < NT; ++n) b[u][n] = (term && co0 + 16 * n + ai < g.cout) ? grow[(size_t)x * g.cout + 16 * n] : 0.f;
        a[u] = (term && ci < g.cin) ? inrow[(size_t)xx * g.cin] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u][n], acc[n], 0, 0, 0);
    }
  }
  float* mine = part + (size_t)blockIdx.x * taps * cinp16 * coutp;
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ak * 4 + r, co = co0 + 16 * n + ai;   // row of the tile = (lane >> 4) * 4 + r, column (co) = lane & 15
      if (co < coutp) mine[((size_t)tap * cinp16 + 16 * mt + row) * coutp + co] = acc[n][r];
    }
}

template <int NT>
static void launch_nt(const ConvPlan& p, const float* in, const float* b, float* out, hipStream_t stream) {
  const dim3 grid(p.grid_x, p.grid_y);
  const int coutp = round_up(p.gx.cout, 16);
  if (p.family == CF_FWD_ANY) {
    if (p.leaky) conv_forward_any_kernel<NT, true><<<grid, p.block, 0, stream>>>(p.gx, in, b, out, p.KS, p.C, coutp);
    else conv_forward_any_kernel<NT, false><<<grid, p.block, 0, stream>>>(p.gx, in, b, out, p.KS, p.C, coutp);
  } else {
    conv_wgrad_any_kernel<NT><<<grid, p.block, 0, stream>>>(p.gx, in, b, out, p.rows_per_block, p.KS, p.C, p.item_groups, coutp);
  }
}

int conv_any_launch(const ConvPlan& p, const float* in, const float* b, float* out, hipStream_t stream) {
  if ((p.family != CF_FWD_ANY && p.family != CF_WG_ANY) || p.NT < 1 || p.NT > 4) {
    set_error_msg("conv_any_launch: not a plan of the run-time-shaped family");
    return PISO_ERR_INVALID_ARG;
  }
  switch (p.NT) {
    case 1: launch_nt<1>(p, in, b, out, stream); break;
    case 2: launch_nt<2>(p, in, b, out, stream); break;
    case 3: launch_nt<3>(p, in, b, out, stream); break;
    default: launch_nt<4>(p, in, b, out, stream); break;
  }
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

}  // namespace piso
