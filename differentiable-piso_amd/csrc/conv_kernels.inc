// The kernels of the closure convolutions (conv.hip includes this text twice), written once for two geometries:
//   CONV_GEOM ConvGeom    one zero padding on every side: the *_kernel instances of piso_conv2d_forward / piso_conv2d_wgrad
//   CONV_GEOM ConvGeomEx  padding per axis and wrap-around per axis: the *_ex_kernel instances of piso_conv2d_forward_ex / piso_conv2d_wgrad_ex
// conv.hip defines, per inclusion: CONV_GEOM, CONV_KERNEL(name) (the kernel's symbol), CONV_PAD_Y / CONV_PAD_X (the padding of `g`) and
// CONV_ROW(yy) / CONV_COL(xx): the source row / column of a tap.  Each family forms and tests yy / xx in ONE place; a coordinate that is still
// outside the image after CONV_ROW / CONV_COL contributes nothing (zero padding, or a pixel only outputs beyond the row's end would read).
// (Text inclusion, not a template over the geometry: the first geometry's device code is then the compiler's output for the very same tokens
// as before the second existed - a body templated on the geometry type compiled to other instructions.)

// KS: kernel size; CINP: input channels rounded up to 4 (<= 4 channels) or to 16; NT: output-channel tiles of 16 (COUTP = 16 NT).
// CINP >= 16: the K dimension of a block of 16 channels is PERMUTED so that every operand is one 16-byte load: K-step j of the
// block takes channel 4 (lane >> 4) + j from lane group lane >> 4 - a lane loads the float4 of its pixel's channels
// [4 (lane >> 4), +4) once and feeds component j to step j; the host lays the weights out to match:
//     w[tap][block][lane >> 4][co][j] = W[tap][16 block + 4 (lane >> 4) + j][co]          (piso_conv2d_weight_layout)
template <int KS, int CINP, int NT, bool LEAKY_OUT>
__global__ __launch_bounds__(kBlock) void CONV_KERNEL(conv_forward)(CONV_GEOM g, const float* __restrict__ in, const float* __restrict__ w,
                                                               float* __restrict__ out) {
  constexpr int MT = 4;                                     // 4 x 16 = 64 pixels per wave
  constexpr int COUTP = 16 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (g.Wo + 16 * MT - 1) / (16 * MT);
  const int tile = blockIdx.x * (kBlock / 64) + wave;
  if (tile >= tiles_x * g.Ho) return;
  const int y = tile / tiles_x, x0 = (tile - y * tiles_x) * 16 * MT;
  const int ai = lane & 15, ak = lane >> 4;                 // A: pixel in tile, channel group;  B: channel group = ak, co = ai
  f32x4 acc[MT][NT];
  zero_tiles(acc);
  if constexpr (CINP >= 16) {
    // Software pipeline over the K-blocks (tap row, block of 16 channels, tap column): the operands of block s + 1 are loaded while
    // the 16 MT NT / 4 MFMAs of block s run - issued and consumed in the same block the loop ran at the latency of one L2 round
    // trip per block (forward 3 x 3, 64 -> 64: 264 us at 256 x 896, 40 % of the fp32 MFMA peak).
    constexpr int CB = CINP / 16, NSEQ = KS * CB;
    auto load_ab = [&](int yy, int sidx, f32x4 (&a)[MT], f32x4 (&b)[NT], int ky) __attribute__((always_inline)) {
      const int cb = sidx / KS, kx = sidx - cb * KS;         // (block of 16 channels outside, tap column inside: the staged kernel's K order)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int xx = CONV_COL(x0 + 16 * m + ai + kx - CONV_PAD_X);
        a[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (xx >= 0 && xx < g.W) a[m] = *reinterpret_cast<const f32x4*>(in + ((size_t)yy * g.W + xx) * g.cin + 16 * cb + 4 * ak);
      }
#pragma unroll
      for (int n = 0; n < NT; ++n)
        b[n] = *reinterpret_cast<const f32x4*>(w + ((((size_t)(ky * KS + kx) * CB + cb) * 4 + ak) * COUTP + 16 * n + ai) * 4);
    };
    for (int ky = 0; ky < KS; ++ky) {
      const int yy = CONV_ROW(y + ky - CONV_PAD_Y);
      if (yy < 0 || yy >= g.H) continue;                     // (wave-uniform: a whole tap row of zero padding; a wrapped row is never outside)
      f32x4 a0[MT], b0[NT], a1[MT], b1[NT];
      load_ab(yy, 0, a0, b0, ky);
#pragma unroll
      for (int sq = 0; sq < NSEQ; sq += 2) {
        if (sq + 1 < NSEQ) load_ab(yy, sq + 1, a1, b1, ky);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[m][j], b0[n][j], acc[m][n], 0, 0, 0);
        if (sq + 1 < NSEQ) {
          if (sq + 2 < NSEQ) load_ab(yy, sq + 2, a0, b0, ky);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
              for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[m][j], b1[n][j], acc[m][n], 0, 0, 0);
        }
      }
    }
  } else {
  for (int ky = 0; ky < KS; ++ky) {
    const int yy = CONV_ROW(y + ky - CONV_PAD_Y);
    if (yy < 0 || yy >= g.H) continue;                       // (wave-uniform: a whole tap row of zero padding; a wrapped row is never outside)
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) {
      {
        static_assert(CINP == 4, "up to 4 input channels: one K-step per tap");
        float a[MT], b[NT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int xx = CONV_COL(x0 + 16 * m + ai + kx - CONV_PAD_X);
          a[m] = (xx >= 0 && xx < g.W && ak < g.cin) ? in[((size_t)yy * g.W + xx) * g.cin + ak] : 0.f;
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) b[n] = w[((size_t)(ky * KS + kx) * 4 + ak) * COUTP + 16 * n + ai];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
      }
    }
  }
  }
  // C/D layout: column (co) = lane & 15, row (pixel) = (lane >> 4) * 4 + register
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int co = 16 * n + ai;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = x0 + 16 * m + ak * 4 + r;
        if (x < g.Wo && co < g.cout) {
          float v = acc[m][n][r];
          if (LEAKY_OUT) v = v > 0.f ? v : kLeakySlope * v;
          out[((size_t)y * g.Wo + x) * g.cout + co] = v;
        }
      }
    }
}

// The same convolution with its operands STAGED THROUGH LDS (CINP >= 16, KS >= 3).  The kernel above reads, per K-block of a wave,
// 4 KB of A and NT KB of B from L2 for 16 MT NT MFMAs: at config 4's size that is ~10 TB/s of L2 traffic chip-wide - the 64 -> 64
// layers ran at 53 % of the fp32 MFMA peak, bound by it.  Here the four waves of a workgroup (four consecutive tiles of 64 pixels,
// possibly of two output rows) walk the same stages = (tap row ky, block of 16 input channels) in lock step:
//   * B of the stage - the weights of all KS tap columns, KS NT KB - is loaded ONCE per workgroup and shared by the four waves;
//   * A of the stage - the 64 + KS - 1 input pixels a wave's tile touches over the KS tap columns, 16 channels - is loaded ONCE per
//     wave; the tap columns read it at pixel offsets 0 .. KS - 1 (a lane's 16-byte reads cover a contiguous KB: conflict-free).
// L2 traffic per stage and wave: (64 + KS - 1) 64 B + KS NT KB / 4 instead of KS (4 + NT) KB (3 x 3, 64 -> 64: 7.2 instead of 24 KB).
// Double-buffered: the next stage's operands travel from L2 into registers while the MFMAs of this stage run, are written to the
// other LDS buffer behind them, one barrier per stage.  Same K order per output as the kernel above (tap row, block of 16 channels, tap
// column, channel): the same bits - tests/test_gpu_conv_dispatch.py compares them.
template <int KS, int CINP, int NT, bool LEAKY_OUT>
__global__ __launch_bounds__(kBlock) void CONV_KERNEL(conv_forward_lds)(CONV_GEOM g, const float* __restrict__ in, const float* __restrict__ w,
                                                                   float* __restrict__ out) {
  static_assert(CINP >= 16 && KS >= 3, "tap columns share the staged pixels; channels in blocks of 16");
  constexpr int MT = 4, COUTP = 16 * NT, CB = CINP / 16;
  constexpr int P = 16 * MT + KS - 1;                       // pixels of a wave's A segment
  constexpr int NA = (P * 4 + 63) / 64;                     // 16-byte loads per lane for it
  constexpr int BV = KS * NT * 64;                          // 16-byte words of a stage's B
  constexpr int NB = (BV + kBlock - 1) / kBlock;            // ... per thread
  __shared__ f32x4 As[2][kBlock / 64][P * 4];
  __shared__ f32x4 Bs[2][BV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (g.Wo + 16 * MT - 1) / (16 * MT);
  const int tile = blockIdx.x * (kBlock / 64) + wave;
  const bool active = tile < tiles_x * g.Ho;                // (a wave without a tile still helps with B and takes part in the barriers)
  const int y = active ? tile / tiles_x : 0, x0 = active ? (tile - y * tiles_x) * 16 * MT : 0;
  const int ai = lane & 15, ak = lane >> 4;
  f32x4 acc[MT][NT];
  zero_tiles(acc);
  // every wave walks ALL tap rows (the weights of a stage are the same for every output row); a tap row outside the image - zero
  // padding above / below - contributes nothing: its pixels are staged as zeros (wave-uniform: no loads are issued)
  constexpr int nstages = KS * CB;
  f32x4 ra[NA], rb[NB];
  auto fetch = [&](int s) __attribute__((always_inline)) {        // stage s: global -> registers
    const int ky = s / CB, cb = s - (s / CB) * CB;
    const int yy = CONV_ROW(y + ky - CONV_PAD_Y);
    const bool row_ok = active && yy >= 0 && yy < g.H;
#pragma unroll
    for (int t = 0; t < NA; ++t) {
      const int i = lane + 64 * t, px = i >> 2, grp = i & 3;
      const int xx = CONV_COL(x0 + px - CONV_PAD_X);
      ra[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (row_ok && i < P * 4 && xx >= 0 && xx < g.W) ra[t] = *reinterpret_cast<const f32x4*>(in + ((size_t)yy * g.W + xx) * g.cin + 16 * cb + 4 * grp);
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int i = threadIdx.x + kBlock * t;                // [kx][ak][COUTP] 16-byte words: NT x 64 per tap column
      const int kx = i / (NT * 64), r = i - kx * (NT * 64);
      rb[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (i < BV) rb[t] = *reinterpret_cast<const f32x4*>(w + ((((size_t)(ky * KS + kx) * CB + cb) * 4) * COUTP + r) * 4);
    }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {      // registers -> LDS
#pragma unroll
    for (int t = 0; t < NA; ++t) { const int i = lane + 64 * t; if (i < P * 4) As[buf][wave][i] = ra[t]; }
#pragma unroll
    for (int t = 0; t < NB; ++t) { const int i = threadIdx.x + kBlock * t; if (i < BV) Bs[buf][i] = rb[t]; }
  };
  fetch(0); stash(0);
  __syncthreads();
  for (int s = 0; s < nstages; ++s) {
    const int buf = s & 1;
    if (s + 1 < nstages) fetch(s + 1);
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) {
      f32x4 a[MT], b[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m] = As[buf][wave][(16 * m + ai + kx) * 4 + ak];
#pragma unroll
      for (int n = 0; n < NT; ++n) b[n] = Bs[buf][(kx * 4 + ak) * COUTP + 16 * n + ai];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][j], b[n][j], acc[m][n], 0, 0, 0);
    }
    if (s + 1 < nstages) stash(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int co = 16 * n + ai;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = x0 + 16 * m + ak * 4 + r;
        if (active && x < g.Wo && co < g.cout) {
          float v = acc[m][n][r];
          if (LEAKY_OUT) v = v > 0.f ? v : kLeakySlope * v;
          out[((size_t)y * g.Wo + x) * g.cout + co] = v;
        }
      }
    }
}

// Weight gradient.  A work item is one (tap, 16-channel tile of ci); wave w of workgroup (band, group) owns the items
// [(4 group + w) IPW, +IPW) x all NT tiles of co and reduces the output rows of its band into part[band][KS][KS][CINP16][COUTP].
// The K loop (pixels) is unrolled 4 x 4 pixels with every operand load issued before the first MFMA: the loop is latency
// bound otherwise (one global round trip per 4 pixels).  CINP16: input channels rounded up to 16.
// PACK4 (cin <= 4, the first layer): the 16 rows of an M tile are 4 consecutive kx taps x 4 channels - one contiguous 64-byte
// segment of NHWC per pixel - instead of 16 channels of which 12 would be padding; an item is then (ky, group of 4 kx).
template <int KS, int MTI, int NT, int IPW, bool PACK4 = false>
__global__ __launch_bounds__(kBlock) void CONV_KERNEL(conv_wgrad)(CONV_GEOM g, const float* __restrict__ in, const float* __restrict__ gout,
                                                             float* __restrict__ part, int rows_per_block) {
  constexpr int TAPS = KS * KS, KXG = (KS + 3) / 4, ITEMS = PACK4 ? KS * KXG : TAPS * MTI, U = 4;
  constexpr int CINP16 = 16 * MTI, COUTP = 16 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = lane & 15, ak = lane >> 4;                 // A: ci = ai, pixel-in-step = ak;  B: pixel-in-step = ak, co = ai
  const int item0 = (blockIdx.y * 4 + wave) * IPW;
  if (item0 >= ITEMS) return;
  f32x4 acc[IPW][NT];
  zero_tiles(acc);
  int ky[IPW], kx[IPW], ci[IPW];
#pragma unroll
  for (int t = 0; t < IPW; ++t) {
    const int item = item0 + t < ITEMS ? item0 + t : ITEMS - 1;     // (a duplicate of the last item: computed, never stored)
    if (PACK4) {
      ky[t] = item / KXG;
      kx[t] = 4 * (item - ky[t] * KXG) + (ai >> 2);                  // this lane's tap of the group; >= KS: padding
      ci[t] = (kx[t] < KS) ? (ai & 3) : g.cin;                       // (channel >= cin reads as zero)
    } else {
      const int tap = item / MTI;
      ky[t] = tap / KS; kx[t] = tap - ky[t] * KS;
      ci[t] = 16 * (item - tap * MTI) + ai;
    }
  }
  const int y_begin = blockIdx.x * rows_per_block, y_end = min(y_begin + rows_per_block, g.Ho);
  for (int y = y_begin; y < y_end; ++y) {
    for (int x0 = 0; x0 < g.Wo; x0 += 4 * U) {
      float a[U][IPW], b[U][NT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int x = x0 + 4 * u + ak;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int co = 16 * n + ai;
          b[u][n] = (x < g.Wo && co < g.cout) ? gout[((size_t)y * g.Wo + x) * g.cout + co] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < IPW; ++t) {
          const int yy = CONV_ROW(y + ky[t] - CONV_PAD_Y), xx = CONV_COL(x + kx[t] - CONV_PAD_X);
          a[u][t] = (x < g.Wo && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W && ci[t] < g.cin) ? in[((size_t)yy * g.W + xx) * g.cin + ci[t]] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < IPW; ++t)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t], b[u][n], acc[t][n], 0, 0, 0);
    }
  }
  float* mine = part + (size_t)blockIdx.x * TAPS * CINP16 * COUTP;
#pragma unroll
  for (int t = 0; t < IPW; ++t) {
    const int item = item0 + t;
    if (item >= ITEMS) break;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ak * 4 + r, co = 16 * n + ai;                  // row of the tile = (lane >> 4) * 4 + r, column (co) = lane & 15
        if (PACK4) {
          const int kyi = item / KXG, kxi = 4 * (item - kyi * KXG) + (row >> 2);
          if (kxi < KS) mine[((size_t)(kyi * KS + kxi) * CINP16 + (row & 3)) * COUTP + co] = acc[t][n][r];
        } else {
          const int tap = item / MTI, m = item - tap * MTI;
          mine[((size_t)tap * CINP16 + 16 * m + row) * COUTP + co] = acc[t][n][r];
        }
      }
  }
}

// The generic weight gradient with its operands staged through LDS (cin, cout multiples of 4).  The kernel above issues one 4-byte
// load with its own bounds checks per operand element - U (IPW + NT) load instructions and ~8 VALU instructions each per 4 U IPW NT
// MFMAs: the address arithmetic costs as much as the matrix cores.  Here the four waves of a workgroup - the items (tap, 16-channel
// tile of ci) of one group - share a staged chunk of 32 output pixels: gout[32][COUTP] and in[KS rows][32 + KS - 1][CINP16], zero where
// the image ends, loaded with 16-byte accesses once per workgroup, double-buffered, one barrier per chunk.  The inner loop reads
// LDS at addresses that need no checks.  Same pixel order per weight: the same bits.
template <int KS, int MTI, int NT, int IPW>
__global__ __launch_bounds__(kBlock) void CONV_KERNEL(conv_wgrad_lds)(CONV_GEOM g, const float* __restrict__ in, const float* __restrict__ gout,
                                                                 float* __restrict__ part, int rows_per_block) {
  constexpr int TAPS = KS * KS, ITEMS = TAPS * MTI, CH = 32, PA = CH + KS - 1;
  constexpr int CINP16 = 16 * MTI, COUTP = 16 * NT;
  constexpr int GV = CH * COUTP / 4, IV = KS * PA * CINP16 / 4;            // 16-byte words of a staged chunk
  constexpr int NG = (GV + kBlock - 1) / kBlock, NI = (IV + kBlock - 1) / kBlock;
  __shared__ f32x4 Gs[2][GV], Is[2][IV + 1];                // (Is[.][IV]: a word of zeros, never overwritten - see `live` below)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = lane & 15, ak = lane >> 4;
  const int item0 = (blockIdx.y * 4 + wave) * IPW;
  if (threadIdx.x < 2) Is[threadIdx.x][IV] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 acc[IPW][NT];
  zero_tiles(acc);
  int aoff[IPW];                                            // float offset of (ky, kx, ci tile) inside a staged `in` chunk, + my ci
#pragma unroll
  for (int t = 0; t < IPW; ++t) {
    const int item = item0 + t < ITEMS ? item0 + t : ITEMS - 1;     // (a duplicate of the last item: computed, never stored)
    const int tap = item / MTI, ky = tap / KS, kx = tap - ky * KS;
    aoff[t] = (ky * PA + kx) * CINP16 + 16 * (item - tap * MTI) + ai;
  }
  const int y_begin = blockIdx.x * rows_per_block, y_end = min(y_begin + rows_per_block, g.Ho);
  const int chunks_x = (g.Wo + CH - 1) / CH, nsteps = (y_end - y_begin) * chunks_x;
  f32x4 rg[NG], ri[NI];
  auto fetch = [&](int s) __attribute__((always_inline)) {
    const int y = y_begin + s / chunks_x, x0 = (s - (s / chunks_x) * chunks_x) * CH;
#pragma unroll
    for (int t = 0; t < NG; ++t) {
      const int i = threadIdx.x + kBlock * t, px = i / (COUTP / 4), c4 = (i - px * (COUTP / 4)) * 4, x = x0 + px;
      rg[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (i < GV && x < g.Wo && c4 < g.cout) rg[t] = *reinterpret_cast<const f32x4*>(gout + ((size_t)y * g.Wo + x) * g.cout + c4);
    }
#pragma unroll
    for (int t = 0; t < NI; ++t) {
      const int i = threadIdx.x + kBlock * t;
      const int c4 = (i % (CINP16 / 4)) * 4, rest = i / (CINP16 / 4), px = rest % PA, ky = rest / PA;
      const int yy = CONV_ROW(y + ky - CONV_PAD_Y), xx = CONV_COL(x0 + px - CONV_PAD_X);
      ri[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // (a pixel of `in` beyond the output row's last pixel + KS - 1 is only ever paired with output pixels that do not exist: the inner
      // loop masks those, the chunk's own bound suffices here)
      if (i < IV && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W && c4 < g.cin) ri[t] = *reinterpret_cast<const f32x4*>(in + ((size_t)yy * g.W + xx) * g.cin + c4);
    }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < NG; ++t) { const int i = threadIdx.x + kBlock * t; if (i < GV) Gs[buf][i] = rg[t]; }
#pragma unroll
    for (int t = 0; t < NI; ++t) { const int i = threadIdx.x + kBlock * t; if (i < IV) Is[buf][i] = ri[t]; }
  };
  if (nsteps > 0) { fetch(0); stash(0); }
  __syncthreads();
  const bool working = item0 < ITEMS;                       // (a wave without items still loads its share and takes part in the barriers)
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) fetch(s + 1);
    if (working) {
      const float* gs = reinterpret_cast<const float*>(Gs[buf]);
      const float* is = reinterpret_cast<const float*>(Is[buf]);
      const int live = g.Wo - (s - (s / chunks_x) * chunks_x) * CH;      // output pixels of this chunk that exist
#pragma unroll
      for (int q = 0; q < CH / 16; ++q) {
        float a[4][IPW], b[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int px = 16 * q + 4 * u + ak;
#pragma unroll
          for (int n = 0; n < NT; ++n) b[u][n] = gs[px * COUTP + 16 * n + ai];
          // (beyond the row's last output pixel gout is staged as zero, but the pixel of `in` a tap pairs with it may be a real one: it takes
          // no part in this weight's sum, so it must not reach the MFMA - 0 x NaN is NaN.  The direct kernel's `x < g.Wo` says the same;
          // here the ADDRESS is switched to the word of zeros: one select per operand, no second copy of it in registers)
#pragma unroll
          for (int t = 0; t < IPW; ++t) a[u][t] = is[px < live ? px * CINP16 + aoff[t] : 4 * IV];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int t = 0; t < IPW; ++t)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t], b[u][n], acc[t][n], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) stash(buf ^ 1);
    __syncthreads();
  }
  if (!working) return;
  float* mine = part + (size_t)blockIdx.x * TAPS * CINP16 * COUTP;
#pragma unroll
  for (int t = 0; t < IPW; ++t) {
    const int item = item0 + t;
    if (item >= ITEMS) break;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ak * 4 + r, co = 16 * n + ai;
        const int tap = item / MTI, m = item - tap * MTI;
        mine[((size_t)tap * CINP16 + 16 * m + row) * COUTP + co] = acc[t][n][r];
      }
  }
}

// Weight gradient of the 64 -> 64 channel layers: M and N are PERMUTED (tile m, row i <-> channel 4 i + m; tile n, column j <->
// channel 4 j + n) so that a lane's operand for all four tiles is ONE float4 of its pixel (channels [4 (lane & 15), +4)):
// one 16-byte load of `in`, one of `gout` per 4 pixels and 16 MFMAs.  A wave owns one tap and all 4 x 4 tiles.
template <int KS>
__global__ __launch_bounds__(kBlock) void CONV_KERNEL(conv_wgrad64)(CONV_GEOM g, const float* __restrict__ in, const float* __restrict__ gout,
                                                               float* __restrict__ part, int rows_per_block) {
  constexpr int TAPS = KS * KS, U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = lane & 15, ak = lane >> 4;
  const int tap = blockIdx.y * 3 + wave;                   // (workgroups of three waves: the nine taps of a 3 x 3 kernel fill three of them)
  if (tap >= TAPS) return;
  const int ky = tap / KS, kx = tap - ky * KS;
  f32x4 acc[4][4];
  zero_tiles(acc);
  const int y_begin = blockIdx.x * rows_per_block, y_end = min(y_begin + rows_per_block, g.Ho);
  for (int y = y_begin; y < y_end; ++y) {
    const int yy = CONV_ROW(y + ky - CONV_PAD_Y);
    if (yy < 0 || yy >= g.H) continue;                       // (zero padding only: a wrapped row is never outside)
    for (int x0 = 0; x0 < g.Wo; x0 += 4 * U) {
      f32x4 a[U], b[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int x = x0 + 4 * u + ak, xx = CONV_COL(x + kx - CONV_PAD_X);
        a[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        b[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (x < g.Wo) {
          b[u] = *reinterpret_cast<const f32x4*>(gout + ((size_t)y * g.Wo + x) * 64 + 4 * ai);
          if (xx >= 0 && xx < g.W) a[u] = *reinterpret_cast<const f32x4*>(in + ((size_t)yy * g.W + xx) * 64 + 4 * ai);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][m], b[u][n], acc[m][n], 0, 0, 0);
    }
  }
  float* mine = part + ((size_t)blockIdx.x * TAPS + tap) * 64 * 64;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) mine[(size_t)(4 * (ak * 4 + r) + m) * 64 + 4 * ai + n] = acc[m][n][r];
}

// The same with the operands staged through LDS: the three waves of a workgroup are the three tap COLUMNS of one tap row - they read the
// same row of `gout` and the same row of `in`, shifted by one pixel each.  Chunks of 32 output pixels: gout[32][64] and in[34][64]
// are loaded once per workgroup (L2 traffic / 3), double-buffered, one barrier per chunk (32 pixels: 32 MFMAs per wave).  Same pixel order
// per weight as the kernel above: the same bits.
template <int KS>
__global__ __launch_bounds__(64 * KS) void CONV_KERNEL(conv_wgrad64_lds)(CONV_GEOM g, const float* __restrict__ in, const float* __restrict__ gout,
                                                                    float* __restrict__ part, int rows_per_block) {
  constexpr int TAPS = KS * KS, CH = 32, PA = CH + KS - 1, NTH = 64 * KS;   // (chunks of 32 pixels: 33 KB of LDS, four workgroups = 12 waves per CU)
  constexpr int NLB = (CH * 16 + NTH - 1) / NTH, NLA = (PA * 16 + NTH - 1) / NTH;       // 16-byte loads per thread: gout chunk, in chunk
  __shared__ f32x4 Gs[2][CH * 16], Is[2][PA * 16 + 1];      // [pixel][16 groups of 4 channels]; Is[.][PA * 16]: zeros, never overwritten
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = lane & 15, ak = lane >> 4;
  const int ky = blockIdx.y, kx = wave;                      // (one workgroup = one tap row, one wave per tap column)
  if (threadIdx.x < 2) Is[threadIdx.x][PA * 16] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int tap = ky * KS + kx;
  f32x4 acc[4][4];
  zero_tiles(acc);
  const int y_begin = blockIdx.x * rows_per_block, y_end = min(y_begin + rows_per_block, g.Ho);
  const int chunks_x = (g.Wo + CH - 1) / CH;
  f32x4 rg[NLB], ri[NLA];
  auto fetch = [&](int y, int c) __attribute__((always_inline)) {
    const int yy = CONV_ROW(y + ky - CONV_PAD_Y), x0 = c * CH;
    const bool row_ok = yy >= 0 && yy < g.H;
#pragma unroll
    for (int t = 0; t < NLB; ++t) {
      const int i = threadIdx.x + NTH * t, px = i >> 4, grp = i & 15, x = x0 + px;
      rg[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (i < CH * 16 && x < g.Wo) rg[t] = *reinterpret_cast<const f32x4*>(gout + ((size_t)y * g.Wo + x) * 64 + 4 * grp);
    }
#pragma unroll
    for (int t = 0; t < NLA; ++t) {
      const int i = threadIdx.x + NTH * t, px = i >> 4, grp = i & 15, xx = CONV_COL(x0 + px - CONV_PAD_X);
      ri[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (row_ok && i < PA * 16 && xx >= 0 && xx < g.W) ri[t] = *reinterpret_cast<const f32x4*>(in + ((size_t)yy * g.W + xx) * 64 + 4 * grp);
    }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < NLB; ++t) { const int i = threadIdx.x + NTH * t; if (i < CH * 16) Gs[buf][i] = rg[t]; }
#pragma unroll
    for (int t = 0; t < NLA; ++t) { const int i = threadIdx.x + NTH * t; if (i < PA * 16) Is[buf][i] = ri[t]; }
  };
  const int nsteps = (y_end - y_begin) * chunks_x;
  if (nsteps > 0) { fetch(y_begin, 0); stash(0); }
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) { const int yn = y_begin + (s + 1) / chunks_x, cn = (s + 1) - ((s + 1) / chunks_x) * chunks_x; fetch(yn, cn); }
    // (a tap row outside the image was staged as zeros: its products vanish; same as the `continue` of the direct kernel)
    const int live = g.Wo - (s - (s / chunks_x) * chunks_x) * CH;        // output pixels of this chunk that exist
#pragma unroll
    for (int q = 0; q < CH / 16; ++q) {                     // 16 pixels = 4 x (4 pixels, one per lane group ak)
      f32x4 a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int px = 16 * q + 4 * u + ak;
        b[u] = Gs[buf][px * 16 + ai];
        // (a pixel of `in` paired with an output pixel beyond the row's end takes no part in the sum: 0 x NaN is NaN; as `x < g.Wo` above.
        // The address is switched to the word of zeros)
        a[u] = Is[buf][px < live ? (px + kx) * 16 + ai : PA * 16];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][m], b[u][n], acc[m][n], 0, 0, 0);
    }
    if (s + 1 < nsteps) stash(buf ^ 1);
    __syncthreads();
  }
  float* mine = part + ((size_t)blockIdx.x * TAPS + tap) * 64 * 64;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) mine[(size_t)(4 * (ak * 4 + r) + m) * 64 + 4 * ai + n] = acc[m][n][r];
}

