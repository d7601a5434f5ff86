// The epilogue of a closure layer, one pass per direction behind whichever convolution kernel the layer's shape is routed to (conv.hip,
// conv_any.hip: untouched): bias, skip connection and activation on NHWC [pixels][channels] float32.
//   forward    y = act((z + bias[c]) + skip), fp32, in that order; bias / skip may be NULL, y may be z (in place).  One grid-stride pass.
//   backward   gpre = g * act'(y) from the saved OUTPUT (leaky ReLU and ReLU keep the sign of the pre-activation where it matters) and, in the
//              same pass, dbias[c] = sum over pixels of gpre[p][c]: a workgroup owns one BAND of pixels_per_band pixels, thread (row, col) walks
//              the band's pixels row, row + rows, ... of its column, the rows of a column are added on chip (wave butterflies where the columns
//              are a power of two <= 64, then LDS across the four waves; an LDS tree otherwise) and the band's sums are STORED to
//              ws[band][channels].  A second small kernel adds the bands (band r, r + 64, ... per thread, then the same fixed on-chip order).
//              No atomics: the order of every sum is a function of (pixels, channels, access form) alone - never of the launch, the card's
//              CU count or the run.  The skip cotangent is gpre itself: no kernel, no copy.
// Access form: 16 bytes per lane where channels % 4 == 0 and every pointer is 16-byte aligned; otherwise 4 bytes per lane with no alignment rule
// (the element-wise results are the same bits in both; a bias sum may differ in its last bits between the two, each is reproducible).
// The banding (epilogue_plan) depends on (pixels, channels) only.
#include "piso_common.h"

namespace piso {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kEpiSlope = 0.2f;                           // the slope of conv.hip's kLeakySlope
constexpr int kEpiBandFloats = 4096;                        // a band holds at least this many elements ...
constexpr int kEpiMaxBands = 1024;                          // ... and there are at most this many bands
constexpr int kEpiReduceCols = 4;                           // the band reducer: 4 channels x 64 band rows per workgroup

struct EpiPlan {
  int bands, pixels_per_band, bands_bound;                  // bands_bound >= bands, monotone in pixels: what the workspace is sized for
};
static inline EpiPlan epilogue_plan(int pixels, int channels) {
  const long long base = (kEpiBandFloats + channels - 1) / channels;
  const long long cap = ((long long)pixels + kEpiMaxBands - 1) / kEpiMaxBands;
  const long long ppb = base > cap ? base : cap;
  const long long bound = ((long long)pixels + base - 1) / base;
  EpiPlan p;
  p.pixels_per_band = (int)ppb;
  p.bands = (int)(((long long)pixels + ppb - 1) / ppb);
  p.bands_bound = (int)(bound < kEpiMaxBands ? bound : kEpiMaxBands);
  return p;
}

template <int V> struct EpiVec;
template <> struct EpiVec<1> { typedef float T; };
template <> struct EpiVec<4> { typedef f32x4 T; };

template <int ACT>
__device__ __forceinline__ float epi_act(float v) {
  if (ACT == 1) return v > 0.f ? v : kEpiSlope * v;
  if (ACT == 2) return v > 0.f ? v : 0.f;
  return v;
}
template <int ACT>
__device__ __forceinline__ float epi_act_grad(float g, float y) {
  if (ACT == 1) return y > 0.f ? g : kEpiSlope * g;
  if (ACT == 2) return y > 0.f ? g : 0.f;
  return g;
}
__device__ __forceinline__ float epi_lane(float v, int) { return v; }
__device__ __forceinline__ float epi_lane(const f32x4& v, int q) { return v[q]; }
__device__ __forceinline__ void epi_set(float& v, int, float s) { v = s; }
__device__ __forceinline__ void epi_set(f32x4& v, int q, float s) { v[q] = s; }
__device__ __forceinline__ float epi_shfl_xor(float v, int off) { return __shfl_xor(v, off, kWave); }
__device__ __forceinline__ f32x4 epi_shfl_xor(const f32x4& v, int off) {
  f32x4 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = __shfl_xor(v[q], off, kWave);
  return r;
}

// n elements of V floats, element i of column i % cols (cols = channels / V).  z and y are not __restrict__: y may be z.
template <int V, int ACT>
__global__ __launch_bounds__(kBlock) void conv_epilogue_forward_kernel(const float* z, const float* __restrict__ bias, const float* __restrict__ skip, float* y,
                                                                      size_t n, int cols) {
  typedef typename EpiVec<V>::T VT;
  const size_t stride = (size_t)gridDim.x * kBlock;
  const int step = (int)(stride % (size_t)cols);
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  int col = (int)(i % (size_t)cols);
  for (; i < n; i += stride) {
    VT v = reinterpret_cast<const VT*>(z)[i];
    if (bias) {
      const VT b = reinterpret_cast<const VT*>(bias)[col];
#pragma unroll
      for (int q = 0; q < V; ++q) epi_set(v, q, epi_lane(v, q) + epi_lane(b, q));
    }
    if (skip) {
      const VT s = reinterpret_cast<const VT*>(skip)[i];
#pragma unroll
      for (int q = 0; q < V; ++q) epi_set(v, q, epi_lane(v, q) + epi_lane(s, q));
    }
#pragma unroll
    for (int q = 0; q < V; ++q) epi_set(v, q, epi_act<ACT>(epi_lane(v, q)));
    reinterpret_cast<VT*>(y)[i] = v;
    col += step;
    col -= col >= cols ? cols : 0;
  }
}

// The rows of a column, added on chip; the result is valid in the threads of row 0 (threadIdx.x < cols).  Thread t = row * cols + col holds `acc`;
// threads beyond rows * cols hold nothing.  sm: kBlock elements.
template <typename VT>
__device__ __forceinline__ VT epi_sum_rows(VT acc, int cols, int rows, VT* sm) {
  const int t = threadIdx.x;
  if (cols <= kWave && (cols & (cols - 1)) == 0) {           // (kBlock % cols == 0: every thread has a row)
    for (int off = kWave / 2; off >= cols; off >>= 1) acc += epi_shfl_xor(acc, off);
    const int lane = t & (kWave - 1), wave = t >> 6;
    if (lane < cols) sm[wave * cols + lane] = acc;
    __syncthreads();
    if (t < cols) acc = (sm[t] + sm[cols + t]) + (sm[2 * cols + t] + sm[3 * cols + t]);
    return acc;
  }
  const int row = t / cols;
  if (row < rows) sm[t] = acc;
  __syncthreads();
  int half = 1;
  while (half < rows) half <<= 1;
  for (half >>= 1; half > 0; half >>= 1) {
    if (row < half && row + half < rows) sm[t] += sm[t + half * cols];
    __syncthreads();
  }
  return sm[t < cols ? t : 0];
}

// blockIdx.x: the band [band * ppb, min(pixels, (band + 1) * ppb)).  WRITE: gpre is stored (ACT != 0); SUM: the band's column sums go to ws[band][channels].
template <int V, int ACT, bool WRITE, bool SUM>
__global__ __launch_bounds__(kBlock) void conv_epilogue_backward_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ gpre,
                                                                       float* __restrict__ ws, int pixels, int cols, int ppb) {
  typedef typename EpiVec<V>::T VT;
  __shared__ VT sm[kBlock];
  const int rows = kBlock / cols;
  const int t = threadIdx.x, row = t / cols, col = t - row * cols;
  const long long p0 = (long long)blockIdx.x * ppb;
  const long long p1 = p0 + ppb < pixels ? p0 + ppb : pixels;
  VT acc;
#pragma unroll
  for (int q = 0; q < V; ++q) epi_set(acc, q, 0.f);
  if (row < rows) {
#pragma unroll 2
    for (long long p = p0 + row; p < p1; p += rows) {
      const size_t e = (size_t)p * cols + col;
      VT r = reinterpret_cast<const VT*>(g)[e];
      if (ACT != 0) {
        const VT o = reinterpret_cast<const VT*>(y)[e];
#pragma unroll
        for (int q = 0; q < V; ++q) epi_set(r, q, epi_act_grad<ACT>(epi_lane(r, q), epi_lane(o, q)));
      }
      if (WRITE) reinterpret_cast<VT*>(gpre)[e] = r;
      if (SUM) acc += r;
    }
  }
  if (SUM) {
    acc = epi_sum_rows<VT>(acc, cols, rows, sm);
    if (t < cols) reinterpret_cast<VT*>(ws)[(size_t)blockIdx.x * cols + t] = acc;
  }
}

// dbias[c] = the bands of ws[bands][channels] added: blockIdx.x owns 4 channels, thread (row, col) adds bands row, row + 64, ... in index order, the 64
// rows are added by four butterflies in the wave and across the four waves in LDS (many short chains of loads, not a few long ones).
__global__ __launch_bounds__(kBlock) void conv_epilogue_bias_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dbias, int bands, int channels) {
  __shared__ float sm[kBlock];
  const int t = threadIdx.x, row = t / kEpiReduceCols, c = blockIdx.x * kEpiReduceCols + (t & (kEpiReduceCols - 1));
  float acc = 0.f;
  if (c < channels)
#pragma unroll 4
    for (int b = row; b < bands; b += kBlock / kEpiReduceCols) acc += ws[(size_t)b * channels + c];
  acc = epi_sum_rows<float>(acc, kEpiReduceCols, kBlock / kEpiReduceCols, sm);
  if (t < kEpiReduceCols && c < channels) dbias[c] = acc;
}

static inline bool epi_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}
static int epi_refuse(const char* msg) {
  set_error_msg(msg);
  return PISO_ERR_INVALID_ARG;
}

template <int V>
static void launch_forward(const float* z, const float* bias, const float* skip, float* y, size_t n, int cols, int act, hipStream_t stream) {
  const int grid = grid_for((long long)n, kBlock * 2, 4096);
  if (act == 1) conv_epilogue_forward_kernel<V, 1><<<grid, kBlock, 0, stream>>>(z, bias, skip, y, n, cols);
  else if (act == 2) conv_epilogue_forward_kernel<V, 2><<<grid, kBlock, 0, stream>>>(z, bias, skip, y, n, cols);
  else conv_epilogue_forward_kernel<V, 0><<<grid, kBlock, 0, stream>>>(z, bias, skip, y, n, cols);
}

template <int V, bool SUM>
static void launch_backward(const float* g, const float* y, float* gpre, float* ws, int pixels, int cols, int act, const EpiPlan& p, hipStream_t stream) {
  if (act == 1) conv_epilogue_backward_kernel<V, 1, true, SUM><<<p.bands, kBlock, 0, stream>>>(g, y, gpre, ws, pixels, cols, p.pixels_per_band);
  else if (act == 2) conv_epilogue_backward_kernel<V, 2, true, SUM><<<p.bands, kBlock, 0, stream>>>(g, y, gpre, ws, pixels, cols, p.pixels_per_band);
  else conv_epilogue_backward_kernel<V, 0, false, SUM><<<p.bands, kBlock, 0, stream>>>(g, y, gpre, ws, pixels, cols, p.pixels_per_band);
}
}  // namespace piso

using namespace piso;

extern "C" {
int piso_conv_epilogue_plan(int pixels, int channels, int* bands, int* pixels_per_band) {
  if (pixels < 1) return epi_refuse("piso_conv_epilogue_plan: pixels: at least 1");
  if (channels < 1 || channels > 256) return epi_refuse("piso_conv_epilogue_plan: channels: 1 .. 256");
  const EpiPlan p = epilogue_plan(pixels, channels);
  if (bands) *bands = p.bands;
  if (pixels_per_band) *pixels_per_band = p.pixels_per_band;
  return PISO_OK;
}

size_t piso_conv_epilogue_workspace_bytes(int pixels, int channels) {
  if (pixels < 1 || channels < 1 || channels > 256) return 0;
  return (size_t)epilogue_plan(pixels, channels).bands_bound * channels * sizeof(float);
}

int piso_conv_epilogue_forward(const float* z, const float* bias, const float* skip, float* y, int pixels, int channels, int act, piso_stream_t stream_) {
  if (!z || !y) return epi_refuse("piso_conv_epilogue_forward: z or y is NULL");
  if (channels < 1 || channels > 256) return epi_refuse("piso_conv_epilogue_forward: channels: 1 .. 256");
  if (pixels < 1) return epi_refuse("piso_conv_epilogue_forward: pixels: at least 1");
  if (act < 0 || act > 2) return epi_refuse("piso_conv_epilogue_forward: act: 0 none, 1 leaky ReLU, 2 ReLU");
  if (skip && skip == y) return epi_refuse("piso_conv_epilogue_forward: skip must not alias y");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const size_t n = (size_t)pixels * channels;
  if (channels % 4 == 0 && epi_aligned16(z, bias, skip, y)) launch_forward<4>(z, bias, skip, y, n / 4, channels / 4, act, stream);
  else launch_forward<1>(z, bias, skip, y, n, channels, act, stream);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int piso_conv_epilogue_backward(const float* g, const float* y, float* gpre, float* dbias, int pixels, int channels, int act, float* ws, size_t ws_elems,
                                piso_stream_t stream_) {
  if (!g) return epi_refuse("piso_conv_epilogue_backward: g is NULL");
  if (channels < 1 || channels > 256) return epi_refuse("piso_conv_epilogue_backward: channels: 1 .. 256");
  if (pixels < 1) return epi_refuse("piso_conv_epilogue_backward: pixels: at least 1");
  if (act < 0 || act > 2) return epi_refuse("piso_conv_epilogue_backward: act: 0 none, 1 leaky ReLU, 2 ReLU");
  if (act != 0 && (!y || !gpre)) return epi_refuse("piso_conv_epilogue_backward: y or gpre is NULL with act != 0");
  const EpiPlan p = epilogue_plan(pixels, channels);
  if (dbias && (!ws || ws_elems < (size_t)p.bands * channels))
    return epi_refuse("piso_conv_epilogue_backward: ws too small: piso_conv_epilogue_workspace_bytes(pixels, channels) / 4 elements with dbias given");
  if (act == 0 && !dbias) return PISO_OK;                    // gpre is g: nothing to compute, nothing written
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool wide = channels % 4 == 0 && epi_aligned16(g, act ? y : nullptr, act ? gpre : nullptr, dbias ? ws : nullptr);
  if (wide) {
    if (dbias) launch_backward<4, true>(g, y, gpre, ws, pixels, channels / 4, act, p, stream);
    else launch_backward<4, false>(g, y, gpre, ws, pixels, channels / 4, act, p, stream);
  } else {
    if (dbias) launch_backward<1, true>(g, y, gpre, ws, pixels, channels, act, p, stream);
    else launch_backward<1, false>(g, y, gpre, ws, pixels, channels, act, p, stream);
  }
  if (dbias) conv_epilogue_bias_reduce_kernel<<<(channels + kEpiReduceCols - 1) / kEpiReduceCols, kBlock, 0, stream>>>(ws, dbias, p.bands, channels);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
}  // extern "C"
