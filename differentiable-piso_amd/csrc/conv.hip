// Convolutions of the CNN turbulence closure on the matrix cores (gfx950 MFMA, exact fp32: v_mfma_f32_16x16x4_f32).
//
// The closure of the reference (diffpiso/networks.py:3-73) is a 7-layer fully convolutional network, 4 -> 16 -> 16 -> 32 -> 64 -> 64
// -> 64 -> 2 channels, kernels 7,5,5,3,3,1,1, stride 1, no bias, leaky ReLU (0.2) after all but the last layer, NHWC tensors,
// HWIO weights, 'SAME' or 'VALID' padding (tf.nn.conv2d = cross-correlation).  Every layer is an implicit GEMM
//     out[pixel][co] = sum over (ky, kx, ci) in[pixel + (ky, kx) - pad][ci] * w[ky][kx][ci][co]
// with M = pixels, N = co, K = taps * ci.  One wavefront owns 64 consecutive pixels of one output row x all output channels
// (up to 4 x 4 tiles of 16 x 16 accumulators = 64 VGPRs); per K-step of 4 input channels of one tap it loads the A fragments
// (lane l: pixel l & 15, channel l >> 4 - 16-byte channel groups of NHWC, served by L1 / L2: a tap re-reads the row band its
// neighbours just touched) and the B fragments (lane l: channel l >> 4, output channel l & 15 - the weights of a layer are at
// most 147 KB and stay in L2) and issues MT x NT MFMAs.  fp32 MFMA is an exact fmaf chain, so results agree with a plain fp32
// convolution to summation order.
//   conv_forward   out = [leaky](conv(in, w)): the forward pass AND the input gradient (the caller passes the gradient of the
//                  layer's pre-activation output as `in` and the flipped, transposed weights; pad' = k - 1 - pad)
//   conv_wgrad     dW[ky][kx][ci][co] = sum over pixels in[pixel + (ky, kx) - pad][ci] * g[pixel][co]: M = ci,
//                  N = co, K = pixels; every workgroup reduces a band of rows into its own partial, a second kernel adds the
//                  partials in a fixed order (deterministic, no atomics)
//
// Which instance a call runs, with what launch shape, and what it refuses: conv_dispatch.h (conv_plan, the instance table).  Here: the kernels (their text:
// conv_kernels.inc, compiled for the two geometries), and conv_launch - the only host code that names one.  Shapes without a fixed instance:
// the run-time-shaped family of conv_any.hip (piso_conv2d_forward_any / piso_conv2d_wgrad_any; conv_any.h: its launcher) - the entries, the
// thread-local record and the reducers of its weight gradient are here.
#include "piso_common.h"
#include "options.h"
#include "conv_dispatch.h"
#include "conv_any.h"

namespace piso {

static_assert(kConvBlock == kBlock, "conv_dispatch.h plans workgroups of kBlock threads");

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kLeakySlope = 0.2f;

template <int A, int B>
__device__ __forceinline__ void zero_tiles(f32x4 (&acc)[A][B]) {
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int b = 0; b < B; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// ---- the kernels: conv_kernels.inc, once per geometry
#define CONV_GEOM ConvGeom
#define CONV_KERNEL(name) name##_kernel
#define CONV_PAD_Y g.pad
#define CONV_PAD_X g.pad
#define CONV_ROW(yy) yy
#define CONV_COL(xx) xx
#include "conv_kernels.inc"
#undef CONV_GEOM
#undef CONV_KERNEL
#undef CONV_PAD_Y
#undef CONV_PAD_X
#undef CONV_ROW
#undef CONV_COL

// The general geometry.  On a wrapped axis a coordinate that left the image re-enters on the other side: conv_plan guarantees pad <= extent
// there, so ONE conditional add or subtract of the extent brings every coordinate a stored output reads into [0, extent) - no division.  `wrap`
// is the extent on a wrapped axis and 0 on a zero-padded one, where the coordinate stays as it is and fails the bounds test that follows.
__device__ __forceinline__ int wrapped(int v, int extent, int wrap) {
  v += v < 0 ? wrap : 0;
  return v - (v >= extent ? wrap : 0);
}
#define CONV_GEOM ConvGeomEx
#define CONV_KERNEL(name) name##_ex_kernel
#define CONV_PAD_Y g.pad_y
#define CONV_PAD_X g.pad_x
#define CONV_ROW(yy) wrapped(yy, g.H, g.wrap_h)
#define CONV_COL(xx) wrapped(xx, g.W, g.wrap_w)
#include "conv_kernels.inc"
#undef CONV_GEOM
#undef CONV_KERNEL
#undef CONV_PAD_Y
#undef CONV_PAD_X
#undef CONV_ROW
#undef CONV_COL

// dW[tap][ci][co] (true sizes) = sum of the band partials in a fixed order: a workgroup owns 64 weights, its 4 waves add the
// bands b = wave, wave + 4, ... and the four wave sums are added in wave order
__global__ __launch_bounds__(kBlock) void conv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int nblocks, int taps,
                                                                    int cinp16, int coutp, int cin, int cout) {
  __shared__ float sm[kBlock];
  const int n = taps * cin * cout;
  const int k = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
  float s = 0.f;
  if (k < n) {
    const int co = k % cout, ci = (k / cout) % cin, tap = k / (cout * cin);
    const size_t src = ((size_t)tap * cinp16 + ci) * coutp + co, stride = (size_t)taps * cinp16 * coutp;
    for (int b = wave; b < nblocks; b += 4) s += part[b * stride + src];
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (wave == 0 && k < n) dw[k] = ((sm[threadIdx.x] + sm[64 + threadIdx.x]) + sm[128 + threadIdx.x]) + sm[192 + threadIdx.x];
}

// The same for cout % 4 == 0 (every layer but the last): a lane owns FOUR consecutive output channels of one (tap, ci) - 16-byte
// loads, four independent sums per lane, eight bands in flight per wave; a workgroup owns 256 weights.  Same summation order per
// weight as the scalar kernel (bands b = wave, wave + 4, ... inside a wave, then the four waves in order).
__global__ __launch_bounds__(kBlock) void conv_wgrad_reduce4_kernel(const float* __restrict__ part, float* __restrict__ dw, int nblocks, int taps,
                                                                     int cinp16, int coutp, int cin, int cout) {
  __shared__ f32x4 sm[kBlock];
  const int n4 = taps * cin * (cout >> 2);
  const int k4 = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (k4 < n4) {
    const int cq = cout >> 2;
    const int co = (k4 % cq) * 4, ci = (k4 / cq) % cin, tap = k4 / (cq * cin);
    const size_t src = ((size_t)tap * cinp16 + ci) * coutp + co, stride = (size_t)taps * cinp16 * coutp;
    int b = wave;
    for (; b + 28 < nblocks; b += 32) {                      // eight bands of this wave at once: the loads are independent, the sums ordered
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(part + (size_t)(b + 4 * u) * stride + src);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < nblocks; b += 4) s += *reinterpret_cast<const f32x4*>(part + (size_t)b * stride + src);
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (wave == 0 && k4 < n4) *reinterpret_cast<f32x4*>(dw + (size_t)k4 * 4) = ((sm[threadIdx.x] + sm[64 + threadIdx.x]) + sm[128 + threadIdx.x]) + sm[192 + threadIdx.x];
}

// which kernel instance the calling thread's last convolution ran (piso_conv_last_dispatch; fields: include/piso_hip.h): the plan that was launched
static thread_local int tl_conv_dispatch[kConvRecordFields];
static thread_local int tl_conv_dispatch_n = 0;
// ... and its geometry (piso_conv_last_geometry): pad_y, pad_x, wrap_y, wrap_x after a *_ex entry, no fields after an old one
static thread_local int tl_conv_geometry[kConvGeometryFields];
static thread_local int tl_conv_geometry_n = 0;
static void record(const ConvPlan& p) {
  conv_record(p, tl_conv_dispatch);
  tl_conv_dispatch_n = kConvRecordFields;
  tl_conv_geometry_n = p.ex ? kConvGeometryFields : 0;
  if (p.ex) { const int v[kConvGeometryFields] = {p.gx.pad_y, p.gx.pad_x, p.gx.wrap_h != 0, p.gx.wrap_w != 0}; for (int i = 0; i < kConvGeometryFields; ++i) tl_conv_geometry[i] = v[i]; }
}

// The only host code that names a convolution kernel: the instance is the plan's (KS, C, NT, family), every launch dimension the plan's; EX: the
// *_ex_kernel twin with the plan's general geometry.  b: w_laid_out (forward) / grad_out (weight gradient); out: `out` / dw
template <bool EX>
static int conv_launch_as(const ConvPlan& p, const float* in, const float* b, float* out, float* part, hipStream_t stream) {
  const auto& g = [&p]() -> const auto& { if constexpr (EX) return p.gx; else return p.g; }();
  const dim3 grid(p.grid_x, p.grid_y);
  const int block = p.block, rows = p.rows_per_block;
  if (p.entry == CE_FORWARD) {
    conv_with_shape<kConvFwd>(p.KS, p.C, p.NT, [&](auto i) {
      constexpr ConvShape s = kConvFwd[decltype(i)::value];
      if constexpr (conv_fwd_has_lds(s.KS, s.C)) {
        if (p.family == CF_FWD_LDS) {
          if constexpr (EX) {
            if (p.leaky) conv_forward_lds_ex_kernel<s.KS, s.C, s.NT, true><<<grid, block, 0, stream>>>(g, in, b, out);
            else conv_forward_lds_ex_kernel<s.KS, s.C, s.NT, false><<<grid, block, 0, stream>>>(g, in, b, out);
          } else {
            if (p.leaky) conv_forward_lds_kernel<s.KS, s.C, s.NT, true><<<grid, block, 0, stream>>>(g, in, b, out);
            else conv_forward_lds_kernel<s.KS, s.C, s.NT, false><<<grid, block, 0, stream>>>(g, in, b, out);
          }
          return;
        }
      }
      if constexpr (EX) {
        if (p.leaky) conv_forward_ex_kernel<s.KS, s.C, s.NT, true><<<grid, block, 0, stream>>>(g, in, b, out);
        else conv_forward_ex_kernel<s.KS, s.C, s.NT, false><<<grid, block, 0, stream>>>(g, in, b, out);
      } else {
        if (p.leaky) conv_forward_kernel<s.KS, s.C, s.NT, true><<<grid, block, 0, stream>>>(g, in, b, out);
        else conv_forward_kernel<s.KS, s.C, s.NT, false><<<grid, block, 0, stream>>>(g, in, b, out);
      }
    });
    PISO_LAUNCH_CHECK();
    return PISO_OK;
  }
  constexpr ConvShape p4 = kConvWgPack4;
  if constexpr (EX) {
    if (p.family == CF_WG_64_LDS) conv_wgrad64_lds_ex_kernel<kConvWg64.KS><<<grid, block, 0, stream>>>(g, in, b, part, rows);
    else if (p.family == CF_WG_64) conv_wgrad64_ex_kernel<kConvWg64.KS><<<grid, block, 0, stream>>>(g, in, b, part, rows);
    else if (p.family == CF_WG_PACK4) conv_wgrad_ex_kernel<p4.KS, p4.C, p4.NT, p4.IPW, true><<<grid, block, 0, stream>>>(g, in, b, part, rows);
    else
      conv_with_shape<kConvWg>(p.KS, p.C, p.NT, [&](auto i) {
        constexpr ConvShape s = kConvWg[decltype(i)::value];
        if (p.family == CF_WG_GENERIC_LDS) conv_wgrad_lds_ex_kernel<s.KS, s.C, s.NT, s.IPW><<<grid, block, 0, stream>>>(g, in, b, part, rows);
        else conv_wgrad_ex_kernel<s.KS, s.C, s.NT, s.IPW><<<grid, block, 0, stream>>>(g, in, b, part, rows);
      });
  } else {
    if (p.family == CF_WG_64_LDS) conv_wgrad64_lds_kernel<kConvWg64.KS><<<grid, block, 0, stream>>>(g, in, b, part, rows);
    else if (p.family == CF_WG_64) conv_wgrad64_kernel<kConvWg64.KS><<<grid, block, 0, stream>>>(g, in, b, part, rows);
    else if (p.family == CF_WG_PACK4) conv_wgrad_kernel<p4.KS, p4.C, p4.NT, p4.IPW, true><<<grid, block, 0, stream>>>(g, in, b, part, rows);
    else
      conv_with_shape<kConvWg>(p.KS, p.C, p.NT, [&](auto i) {
        constexpr ConvShape s = kConvWg[decltype(i)::value];
        if (p.family == CF_WG_GENERIC_LDS) conv_wgrad_lds_kernel<s.KS, s.C, s.NT, s.IPW><<<grid, block, 0, stream>>>(g, in, b, part, rows);
        else conv_wgrad_kernel<s.KS, s.C, s.NT, s.IPW><<<grid, block, 0, stream>>>(g, in, b, part, rows);
      });
  }
  PISO_LAUNCH_CHECK();
  const int taps = p.KS * p.KS, cinp16 = 16 * p.C, coutp = 16 * p.NT;
  if (p.reducer == 4) conv_wgrad_reduce4_kernel<<<p.reduce_grid, kBlock, 0, stream>>>(part, out, p.nblocks, taps, cinp16, coutp, g.cin, g.cout);
  else conv_wgrad_reduce_kernel<<<p.reduce_grid, kBlock, 0, stream>>>(part, out, p.nblocks, taps, cinp16, coutp, g.cin, g.cout);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
// the run-time-shaped family: its main kernel (conv_any.hip), then - weight gradient - the reducers above on [band][ks][ks][CINP16][COUTP]
static int conv_launch_any(const ConvPlan& p, const float* in, const float* b, float* out, float* part, hipStream_t stream) {
  const int st = conv_any_launch(p, in, b, p.entry == CE_FORWARD ? out : part, stream);
  if (st != PISO_OK || p.entry == CE_FORWARD) return st;
  const int taps = p.KS * p.KS, cinp16 = 16 * p.C, coutp = round_up(p.gx.cout, 16);
  if (p.reducer == 4) conv_wgrad_reduce4_kernel<<<p.reduce_grid, kBlock, 0, stream>>>(part, out, p.nblocks, taps, cinp16, coutp, p.gx.cin, p.gx.cout);
  else conv_wgrad_reduce_kernel<<<p.reduce_grid, kBlock, 0, stream>>>(part, out, p.nblocks, taps, cinp16, coutp, p.gx.cin, p.gx.cout);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
static int conv_launch(const ConvPlan& p, const float* in, const float* b, float* out, float* part, hipStream_t stream) {
  if (p.family == CF_FWD_ANY || p.family == CF_WG_ANY) return conv_launch_any(p, in, b, out, part, stream);
  return p.ex ? conv_launch_as<true>(p, in, b, out, part, stream) : conv_launch_as<false>(p, in, b, out, part, stream);
}

// one call: plan it, refuse it or launch it, record what ran (a refused or failed call leaves the record untouched)
static int conv_run(const ConvQuery& q, const float* in, const float* b, float* out, void* workspace, piso_stream_t stream) {
  const ConvPlan p = conv_plan(q);
  if (p.status != PISO_OK) { set_error_msg(p.msg); return p.status; }
  const int st = conv_launch(p, in, b, out, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
  if (st == PISO_OK) record(p);
  return st;
}

// g' = g * leaky'(pre-activation) from the layer's saved OUTPUT (a leaky ReLU with a positive slope keeps the sign): the gradient of
// the pre-activation that both the input gradient and the weight gradient consume.  One pass (torch: a multiply and a where).
__global__ __launch_bounds__(kBlock) void leaky_backward_kernel(const float* __restrict__ g, const float* __restrict__ out, float* __restrict__ gp, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (size_t)gridDim.x * kBlock) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i], ov = reinterpret_cast<const f32x4*>(out)[i];
    f32x4 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = ov[q] > 0.f ? gv[q] : kLeakySlope * gv[q];
    reinterpret_cast<f32x4*>(gp)[i] = r;
  }
}
__global__ __launch_bounds__(kBlock) void leaky_backward_tail_kernel(const float* __restrict__ g, const float* __restrict__ out, float* __restrict__ gp, size_t begin, size_t n) {
  const size_t i = begin + (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) gp[i] = out[i] > 0.f ? g[i] : kLeakySlope * g[i];
}

static inline bool misaligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) != 0; }
}  // namespace piso

using namespace piso;

extern "C" {
int piso_conv_last_dispatch(int* out, int capacity) {
  const int n = tl_conv_dispatch_n < capacity ? tl_conv_dispatch_n : capacity;
  for (int i = 0; i < n; ++i) out[i] = tl_conv_dispatch[i];
  return tl_conv_dispatch_n;
}

int piso_conv_last_geometry(int* out, int capacity) {
  const int n = tl_conv_geometry_n < capacity ? tl_conv_geometry_n : capacity;
  for (int i = 0; i < n; ++i) out[i] = tl_conv_geometry[i];
  return tl_conv_geometry_n;
}

int piso_leaky_relu_backward(const float* grad_out, const float* out, float* grad_pre, size_t n, piso_stream_t stream_) {
  using namespace piso;
  if (!grad_out || !out || !grad_pre) { set_error_msg("piso_leaky_relu_backward: invalid argument"); return PISO_ERR_INVALID_ARG; }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool aligned = ((reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad_pre)) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  if (n4 > 0) leaky_backward_kernel<<<grid_for((long long)n4, kBlock * 2, 4096), kBlock, 0, stream>>>(grad_out, out, grad_pre, n4);
  if (n4 * 4 < n) leaky_backward_tail_kernel<<<(int)((n - n4 * 4 + kBlock - 1) / kBlock), kBlock, 0, stream>>>(grad_out, out, grad_pre, n4 * 4, n);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

// Weight layout expected by piso_conv2d_forward (zero filled beyond the true channel counts), COUTP = round_up(cout, 16):
//   cin <= 4 : [ks][ks][4][COUTP]                                 (HWIO, channels padded to 4)
//   cin  > 4 : [ks][ks][CINP / 16][4][COUTP][4], CINP = round_up(cin, 16): element [tap][blk][q][co][j] = W[tap][16 blk + 4 q + j][co]
size_t piso_conv2d_weight_elems(int ks, int cin, int cout) { return conv_weight_elems(ks, cin, cout); }

size_t piso_conv2d_wgrad_workspace_bytes(int ks, int cin, int cout) { return conv_wgrad_workspace_bytes(ks, cin, cout); }

int piso_conv2d_forward(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad, int leaky_out,
                        piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  const ConvQuery q{CE_FORWARD, H, W, cin, cout, ks, pad, leaky_out, opt(OPT_CONV_LDS), !in || !w_laid_out || !out, misaligned16(in, w_laid_out), false, 0};
  return conv_run(q, in, w_laid_out, out, nullptr, stream);
}

int piso_conv2d_wgrad(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad, void* workspace,
                      size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;                              // (the call works on a snapshot of the knobs, options.h)
  const ConvQuery q{CE_WGRAD, H, W, cin, cout, ks, pad, 0, opt(OPT_CONV_LDS), !in || !grad_out || !dw || !workspace, misaligned16(in, grad_out),
                    misaligned16(dw, workspace), workspace_bytes};
  return conv_run(q, in, grad_out, dw, workspace, stream);
}

int piso_conv2d_forward_ex(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,
                           int wrap_y, int wrap_x, int leaky_out, piso_stream_t stream) {
  const piso::OptScope knobs;
  const ConvQuery q{CE_FORWARD, H, W, cin, cout, ks, pad_y, leaky_out, opt(OPT_CONV_LDS), !in || !w_laid_out || !out, misaligned16(in, w_laid_out), false, 0,
                    true, pad_x, wrap_y, wrap_x};
  return conv_run(q, in, w_laid_out, out, nullptr, stream);
}

int piso_conv2d_wgrad_ex(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x, int wrap_y,
                         int wrap_x, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;
  const ConvQuery q{CE_WGRAD, H, W, cin, cout, ks, pad_y, 0, opt(OPT_CONV_LDS), !in || !grad_out || !dw || !workspace, misaligned16(in, grad_out),
                    misaligned16(dw, workspace), workspace_bytes, true, pad_x, wrap_y, wrap_x};
  return conv_run(q, in, grad_out, dw, workspace, stream);
}

// The run-time-shaped family (conv_any.hip), whatever the instance tables hold.  Weight layout of piso_conv2d_forward_any:
//   [ks][ks][CINP4][COUTP], CINP4 = round_up(cin, 4), COUTP = round_up(cout, 16): element [ky][kx][ci][co] = W[ky][kx][ci][co], zero beyond
size_t piso_conv2d_weight_elems_any(int ks, int cin, int cout) { return conv_weight_elems_any(ks, cin, cout); }

size_t piso_conv2d_wgrad_any_workspace_bytes(int ks, int cin, int cout, int Ho) { return conv_wgrad_any_workspace_bytes(ks, cin, cout, Ho); }

int piso_conv2d_instantiated(int entry, int ks, int cin, int cout) { return conv_instantiated(entry, ks, cin, cout); }

int piso_conv2d_forward_any(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,
                            int wrap_y, int wrap_x, int leaky_out, piso_stream_t stream) {
  const piso::OptScope knobs;
  const ConvQuery q{CE_FORWARD, H, W, cin, cout, ks, pad_y, leaky_out, opt(OPT_CONV_LDS), !in || !w_laid_out || !out, misaligned16(in, w_laid_out), false, 0,
                    true, pad_x, wrap_y, wrap_x, true};
  return conv_run(q, in, w_laid_out, out, nullptr, stream);
}

int piso_conv2d_wgrad_any(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x, int wrap_y,
                          int wrap_x, void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  const piso::OptScope knobs;
  const ConvQuery q{CE_WGRAD, H, W, cin, cout, ks, pad_y, 0, opt(OPT_CONV_LDS), !in || !grad_out || !dw || !workspace, misaligned16(in, grad_out),
                    misaligned16(dw, workspace), workspace_bytes, true, pad_x, wrap_y, wrap_x, true};
  return conv_run(q, in, grad_out, dw, workspace, stream);
}

}  // extern "C"
