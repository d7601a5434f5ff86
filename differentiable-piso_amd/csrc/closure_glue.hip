// Coupling of the CNN closure to the PISO step on the flat "u-first" face layout: what diffpiso/closure.py does with torch ops
// (network_input = velocity.at_centers() [+ centered_gradient(pressure)], centered_to_staggered) as four launches, forward and
// reverse mode, whole grid and one rank's y-slab.
//   piso_closure_input           faces, pressure cells -> NHWC network input [rows][nx][2 | 4]
//                                ch 0 = 0.5 (v[j + 1][i] + v[j][i]), ch 1 = 0.5 (u[j][i + 1] + u[j][i]),
//                                ch 2 = (P[j + 1][i] - P[j - 1][i]) r, ch 3 = (P[j][i + 1] - P[j][i - 1]) r, P = the pressure padded by one cell
//                                with the pad mode of each side, r = (float)(1.0 / two_dx): the reciprocal of the DOUBLE, rounded to float32 once
//                                on the host.  closure.centered_gradient writes "/ (2 dx)", and torch's device kernel for a float32 tensor divided
//                                by a host scalar multiplies by exactly this number - these are the bits network_input has on the GPU (a true
//                                division differs in the last bit of 7 % of the elements, 1.0f / (float)two_dx for some cell sizes)
//   piso_closure_input_adjoint   cotangent of that tensor -> cotangents of the faces and of the pressure cells
//   piso_closure_force           NHWC network output [rows][nx][2] -> forcing faces: v[j][i] = 0.5 (C0[j][i] + C0[j - 1][i]),
//                                u[j][i] = 0.5 (C1[j][i] + C1[j][i - 1]), C = the output padded by one cell: edge value, or the other side
//                                of a wrapped axis
//   piso_closure_force_adjoint   cotangent of the faces -> cotangent of the NHWC output
//   piso_closure_halo_add        dst[k] += src[k]: the rows a reverse wide-halo exchange delivered, added into their owner's edge rows
// Like glue.hip: one thread per OUTPUT element gathering its inputs (the adjoints too: no atomics), float32, products and quotients in
// the order the torch ops have them (-ffp-contract=off), x fastest.
// Slab twins: faces and cells are the rank's stored rows (RowMap, piso_common.h); an NHWC buffer holds the whole-grid rows
// [row_begin - ext_lo, row_end + ext_hi) around the ring of ny rows ("extended rows": the halo the network's receptive field needs, 0 on
// a side that ends at a border of the domain).  Every boundary rule is decided on the whole grid's (i, j); only "where does row j live"
// differs.  A launch writes the OWNED rows of its outputs (v rows incl. the duplicate row v[ny] on the slab that owns it).
#include "piso_common.h"

namespace piso {

enum { CPAD_ZERO = 0, CPAD_EDGE = 1, CPAD_WRAP = 2 };       // 'constant', 'boundary', 'periodic' (glue.hip: PAD_*)

// where the rows of an NHWC buffer live: the whole grid (on = 0), or rows [j0 - lo, j1 + hi) of the ring
struct ExtRows {
  int on, ny, j0, nyl, lo, hi;
  __host__ __device__ int rows() const { return on ? nyl + lo + hi : ny; }
  __device__ __forceinline__ int row(int j) const {
    if (!on) return j;
    int d = j - j0;
    if (d < -lo) d += ny; else if (d >= nyl + hi) d -= ny;
    return lo + d;
  }
  // is row j of the whole grid held at all?  (host-side checks of what a launch will read)
  __host__ bool holds(int j) const {
    if (!on) return j >= 0 && j < ny;
    int d = j - j0;
    if (d < -lo) d += ny; else if (d >= nyl + hi) d -= ny;
    return d >= -lo && d < nyl + hi;
  }
};

struct ClosureGeom {
  int nx, ny, ch;
  int px_lo, px_hi, py_lo, py_hi;        // pressure pad mode per side
  int wrap_x, wrap_y;                    // centre -> face resampling: wrapped axes
  float inv_two_dx;                      // (float)(1.0 / two_dx) (see the header of this file)
};

// index of the padded line's element m (-1 .. n) in the unpadded line of n cells, or -1 for a zero
__device__ __forceinline__ int padded_cell(int m, int n, int lo_mode, int hi_mode) {
  if (m < 0) return lo_mode == CPAD_ZERO ? -1 : (lo_mode == CPAD_EDGE ? 0 : n - 1);
  if (m >= n) return hi_mode == CPAD_ZERO ? -1 : (hi_mode == CPAD_EDGE ? n - 1 : 0);
  return m;
}

// ---- network input: one thread per (cell, channel)
__global__ __launch_bounds__(kBlock) void closure_input_kernel(ClosureGeom g, const float* __restrict__ faces, const float* __restrict__ p,
                                                                float* __restrict__ nn_in, CellWin cw, RowMap M, ExtRows X) {
  const int nx = g.nx, ny = g.ny, ch = g.ch;
  const long long n = (long long)cw.n * ch;
  for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long long)gridDim.x * kBlock) {
    const int c = cw.lo + (int)(t / ch), k = (int)(t % ch);
    const int j = c / nx, i = c - j * nx;
    float r;
    if (k == 0) r = 0.5f * (faces[M.v(j + 1, i)] + faces[M.v(j, i)]);
    else if (k == 1) r = 0.5f * (faces[M.u(j, i + 1)] + faces[M.u(j, i)]);
    else if (k == 2) {
      const int a = padded_cell(j + 1, ny, g.py_lo, g.py_hi), b = padded_cell(j - 1, ny, g.py_lo, g.py_hi);
      r = ((a < 0 ? 0.0f : p[M.c(a, i)]) - (b < 0 ? 0.0f : p[M.c(b, i)])) * g.inv_two_dx;
    } else {
      const int a = padded_cell(i + 1, nx, g.px_lo, g.px_hi), b = padded_cell(i - 1, nx, g.px_lo, g.px_hi);
      r = ((a < 0 ? 0.0f : p[M.c(j, a)]) - (b < 0 ? 0.0f : p[M.c(j, b)])) * g.inv_two_dx;
    }
    nn_in[((size_t)X.row(j) * nx + i) * ch + k] = r;
  }
}

// ---- its adjoint w.r.t. the faces: d v[j][i] = 0.5 g0[j][i] + 0.5 g0[j - 1][i], d u[j][i] = 0.5 g1[j][i] + 0.5 g1[j][i - 1] (terms that exist)
__global__ __launch_bounds__(kBlock) void closure_input_adjoint_faces_kernel(ClosureGeom g, const float* __restrict__ d_in, float* __restrict__ d_faces,
                                                                              FaceWin fw, RowMap M, ExtRows X) {
  const int nx = g.nx, ny = g.ny, ch = g.ch, n_u = (nx + 1) * ny;
  for (int w = blockIdx.x * kBlock + threadIdx.x; w < fw.count(); w += gridDim.x * kBlock) {
    const int f = fw.map(w);
    float s = 0.0f;
    if (f < n_u) {
      const int j = f / (nx + 1), i = f - j * (nx + 1);
      const size_t row = (size_t)X.row(j) * nx;
      if (i < nx) s = 0.5f * d_in[(row + i) * ch + 1];
      if (i > 0) s = s + 0.5f * d_in[(row + i - 1) * ch + 1];
      d_faces[M.u(j, i)] = s;
    } else {
      const int q = f - n_u, j = q / nx, i = q - j * nx;
      if (j < ny) s = 0.5f * d_in[((size_t)X.row(j) * nx + i) * ch];
      if (j > 0) s = s + 0.5f * d_in[((size_t)X.row(j - 1) * nx + i) * ch];
      d_faces[M.v(j, i)] = s;
    }
  }
}

// the gather of one axis of the central-difference adjoint: cell m of a line of n cells receives + t(m - 1) (it is the upper sample of cell
// m - 1), - t(m + 1) (the lower sample of cell m + 1) and, through the padding, - t(0) (lower sample of cell 0: the edge value is cell 0, the
// wrap value cell n - 1) and + t(n - 1) (upper sample of cell n - 1: edge value cell n - 1, wrap value cell 0); t(k) = g[k] (1 / two_dx), the reciprocal as in the forward kernel (autograd divides the cotangent by the same host scalar)
template <typename F>
__device__ __forceinline__ float gradient_adjoint_axis(F t, int m, int n, int lo_mode, int hi_mode) {
  float s = 0.0f;
  if (m > 0) s = t(m - 1);
  if (m < n - 1) s = s - t(m + 1);
  if (lo_mode == CPAD_EDGE && m == 0) s = s - t(0);
  if (lo_mode == CPAD_WRAP && m == n - 1) s = s - t(0);
  if (hi_mode == CPAD_EDGE && m == n - 1) s = s + t(n - 1);
  if (hi_mode == CPAD_WRAP && m == 0) s = s + t(n - 1);
  return s;
}
__global__ __launch_bounds__(kBlock) void closure_input_adjoint_pressure_kernel(ClosureGeom g, const float* __restrict__ d_in, float* __restrict__ d_p,
                                                                                 CellWin cw, RowMap M, ExtRows X) {
  const int nx = g.nx, ny = g.ny;
  for (int c = cw.lo + blockIdx.x * kBlock + threadIdx.x; c < cw.lo + cw.n; c += gridDim.x * kBlock) {
    const int j = c / nx, i = c - j * nx;
    const float sy = gradient_adjoint_axis([&](int k) { return d_in[((size_t)X.row(k) * nx + i) * 4 + 2] * g.inv_two_dx; }, j, ny, g.py_lo, g.py_hi);
    const size_t row = (size_t)X.row(j) * nx;
    const float sx = gradient_adjoint_axis([&](int k) { return d_in[(row + k) * 4 + 3] * g.inv_two_dx; }, i, nx, g.px_lo, g.px_hi);
    d_p[M.c(j, i)] = sy + sx;
  }
}

// ---- centre -> face resampling of the network output
__global__ __launch_bounds__(kBlock) void closure_force_kernel(ClosureGeom g, const float* __restrict__ nn_out, float* __restrict__ faces, FaceWin fw,
                                                                RowMap M, ExtRows X) {
  const int nx = g.nx, ny = g.ny, n_u = (nx + 1) * ny;
  const int mx = g.wrap_x ? CPAD_WRAP : CPAD_EDGE, my = g.wrap_y ? CPAD_WRAP : CPAD_EDGE;
  for (int w = blockIdx.x * kBlock + threadIdx.x; w < fw.count(); w += gridDim.x * kBlock) {
    const int f = fw.map(w);
    if (f < n_u) {
      const int j = f / (nx + 1), i = f - j * (nx + 1);
      const size_t row = (size_t)X.row(j) * nx;
      const int a = padded_cell(i, nx, mx, mx), b = padded_cell(i - 1, nx, mx, mx);
      faces[M.u(j, i)] = 0.5f * (nn_out[(row + a) * 2 + 1] + nn_out[(row + b) * 2 + 1]);
    } else {
      const int q = f - n_u, j = q / nx, i = q - j * nx;
      const int a = padded_cell(j, ny, my, my), b = padded_cell(j - 1, ny, my, my);
      faces[M.v(j, i)] = 0.5f * (nn_out[((size_t)X.row(a) * nx + i) * 2] + nn_out[((size_t)X.row(b) * nx + i) * 2]);
    }
  }
}

// its adjoint along one axis: cell m of n receives 0.5 d[m] (upper sample of face m) + 0.5 d[m + 1] (lower sample of face m + 1) and through the
// padding 0.5 d[0] (lower sample of face 0: edge -> cell 0, wrap -> cell n - 1) and 0.5 d[n] (upper sample of face n: edge -> cell n - 1, wrap -> cell 0)
template <typename F>
__device__ __forceinline__ float force_adjoint_axis(F d, int m, int n, int wrapped) {
  float s = 0.5f * d(m) + 0.5f * d(m + 1);
  if (m == (wrapped ? n - 1 : 0)) s = s + 0.5f * d(0);
  if (m == (wrapped ? 0 : n - 1)) s = s + 0.5f * d(n);
  return s;
}
__global__ __launch_bounds__(kBlock) void closure_force_adjoint_kernel(ClosureGeom g, const float* __restrict__ d_faces, float* __restrict__ d_out,
                                                                        CellWin cw, RowMap M, ExtRows X) {
  const int nx = g.nx, ny = g.ny;
  const long long n = (long long)cw.n * 2;
  for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long long)gridDim.x * kBlock) {
    const int c = cw.lo + (int)(t >> 1), k = (int)(t & 1);
    const int j = c / nx, i = c - j * nx;
    const float s = k == 0 ? force_adjoint_axis([&](int m) { return d_faces[M.v(m, i)]; }, j, ny, g.wrap_y)
                           : force_adjoint_axis([&](int m) { return d_faces[M.u(j, m)]; }, i, nx, g.wrap_x);
    d_out[((size_t)X.row(j) * nx + i) * 2 + k] = s;
  }
}

__global__ __launch_bounds__(kBlock) void closure_halo_add_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock) dst[k] = dst[k] + src[k];
}

static int closure_grid(long long n) { return grid_for(n, kBlock * 2, 2048); }

}  // namespace piso

using namespace piso;

namespace {

// what a launch may assume: a legal slab, extended rows that fit the ring, and every NHWC row it will read
int closure_rows(const char* who, const piso_slab_t* slab, int ny, int ext_lo, int ext_hi, ExtRows& X) {
  X = ExtRows{0, ny, 0, ny, 0, 0};
  if (!slab_ok(slab, ny)) { set_error_msg("closure coupling: invalid slab (rows must lie inside the grid, at least 4, at most ny - 6)"); return PISO_ERR_INVALID_ARG; }
  if (!slab) return PISO_OK;
  const int nyl = slab->row_end - slab->row_begin;
  if (ext_lo < 0 || ext_hi < 0 || ext_lo > ny || ext_hi > ny) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: extended rows (%d below, %d above) must lie between 0 and ny = %d", who, ext_lo, ext_hi, ny);
    set_error_msg(msg);
    return PISO_ERR_INVALID_ARG;
  }
  X = ExtRows{1, ny, slab->row_begin, nyl, ext_lo, ext_hi};
  return PISO_OK;
}
int missing_row(const char* who, int j) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: the launch reads NHWC row %d, which the extended rows do not hold", who, j);
  set_error_msg(msg);
  return PISO_ERR_INVALID_ARG;
}

int closure_geom(ClosureGeom& g, int nx, int ny, int channels, const int* pad_modes, int wrap_x, int wrap_y, double two_dx) {
  g.nx = nx; g.ny = ny; g.ch = channels; g.wrap_x = wrap_x ? 1 : 0; g.wrap_y = wrap_y ? 1 : 0; g.inv_two_dx = static_cast<float>(1.0 / two_dx);
  g.px_lo = g.px_hi = g.py_lo = g.py_hi = CPAD_EDGE;
  if (nx < 2 || ny < 2 || (channels != 2 && channels != 4)) return PISO_ERR_INVALID_ARG;
  if (channels == 4) {
    if (!pad_modes || !(two_dx > 0.0)) return PISO_ERR_INVALID_ARG;
    for (int q = 0; q < 4; ++q) if (pad_modes[q] < 0 || pad_modes[q] > 2) return PISO_ERR_INVALID_ARG;
    if ((pad_modes[0] == CPAD_WRAP) != (pad_modes[1] == CPAD_WRAP) || (pad_modes[2] == CPAD_WRAP) != (pad_modes[3] == CPAD_WRAP)) return PISO_ERR_INVALID_ARG;
    g.px_lo = pad_modes[0]; g.px_hi = pad_modes[1]; g.py_lo = pad_modes[2]; g.py_hi = pad_modes[3];
  }
  return PISO_OK;
}

int closure_input_impl(const float* faces, const float* pressure, float* nn_in, int nx, int ny, int channels, const int* pad_modes, double two_dx,
                       piso_stream_t stream_, const piso_slab_t* slab, int ext_lo, int ext_hi) {
  ClosureGeom g;
  if (closure_geom(g, nx, ny, channels, pad_modes, 0, 0, two_dx) != PISO_OK || !faces || !nn_in || (channels == 4 && !pressure)) {
    set_error_msg("piso_closure_input: invalid argument (2 or 4 channels; 4: pressure, pad modes 0 .. 2 with both sides of a periodic axis periodic, two_dx > 0)");
    return PISO_ERR_INVALID_ARG;
  }
  ExtRows X;
  PISO_TRY(closure_rows("piso_closure_input", slab, ny, ext_lo, ext_hi, X));
  const RowMap M = make_row_map(slab, nx, ny);
  const CellWin cw = cell_window(M);
  closure_input_kernel<<<closure_grid((long long)cw.n * channels), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(g, faces, pressure, nn_in, cw, M, X);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int closure_input_adjoint_impl(const float* d_nn_in, float* d_faces, float* d_pressure, int nx, int ny, int channels, const int* pad_modes, double two_dx,
                               piso_stream_t stream_, const piso_slab_t* slab, int ext_lo, int ext_hi) {
  ClosureGeom g;
  if (closure_geom(g, nx, ny, channels, pad_modes, 0, 0, two_dx) != PISO_OK || !d_nn_in || !d_faces || (channels == 4 && !d_pressure)) {
    set_error_msg("piso_closure_input_adjoint: invalid argument (2 or 4 channels; 4: d_pressure, pad modes 0 .. 2 with both sides of a periodic axis periodic, two_dx > 0)");
    return PISO_ERR_INVALID_ARG;
  }
  ExtRows X;
  PISO_TRY(closure_rows("piso_closure_input_adjoint", slab, ny, ext_lo, ext_hi, X));
  const RowMap M = make_row_map(slab, nx, ny);
  // the face gather reads rows j0 - 1 .. j1 - 1, the pressure gather the rows either side of the owned ones (around the ring on a periodic axis)
  if (M.j0 > 0 && !X.holds(M.j0 - 1)) return missing_row("piso_closure_input_adjoint", M.j0 - 1);
  if (channels == 4) {
    const int wrap = g.py_lo == CPAD_WRAP;
    if ((M.j0 > 0 || wrap) && !X.holds((M.j0 - 1 + ny) % ny)) return missing_row("piso_closure_input_adjoint", (M.j0 - 1 + ny) % ny);
    if ((M.j1 < ny || wrap) && !X.holds(M.j1 % ny)) return missing_row("piso_closure_input_adjoint", M.j1 % ny);
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const FaceWin fw = face_window(M);
  const CellWin cw = cell_window(M);
  closure_input_adjoint_faces_kernel<<<closure_grid(fw.count()), kBlock, 0, stream>>>(g, d_nn_in, d_faces, fw, M, X);
  if (channels == 4) closure_input_adjoint_pressure_kernel<<<closure_grid(cw.n), kBlock, 0, stream>>>(g, d_nn_in, d_pressure, cw, M, X);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int closure_force_impl(const float* nn_out, float* faces, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream_, const piso_slab_t* slab,
                       int ext_lo, int ext_hi) {
  ClosureGeom g;
  if (closure_geom(g, nx, ny, 2, nullptr, wrap_x, wrap_y, 1.0) != PISO_OK || !nn_out || !faces) {
    set_error_msg("piso_closure_force: invalid argument");
    return PISO_ERR_INVALID_ARG;
  }
  ExtRows X;
  PISO_TRY(closure_rows("piso_closure_force", slab, ny, ext_lo, ext_hi, X));
  const RowMap M = make_row_map(slab, nx, ny);
  // face row j0 reads cell row j0 - 1 (the wrap row ny - 1 on the first slab of a wrapped axis), the duplicate face row v[ny] cell row 0
  if ((M.j0 > 0 || g.wrap_y) && !X.holds((M.j0 - 1 + ny) % ny)) return missing_row("piso_closure_force", (M.j0 - 1 + ny) % ny);
  if (M.last && g.wrap_y && !X.holds(0)) return missing_row("piso_closure_force", 0);
  const FaceWin fw = face_window(M);
  closure_force_kernel<<<closure_grid(fw.count()), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(g, nn_out, faces, fw, M, X);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int closure_force_adjoint_impl(const float* d_faces, float* d_nn_out, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream_,
                               const piso_slab_t* slab, int ext_lo, int ext_hi) {
  ClosureGeom g;
  if (closure_geom(g, nx, ny, 2, nullptr, wrap_x, wrap_y, 1.0) != PISO_OK || !d_faces || !d_nn_out) {
    set_error_msg("piso_closure_force_adjoint: invalid argument");
    return PISO_ERR_INVALID_ARG;
  }
  ExtRows X;
  PISO_TRY(closure_rows("piso_closure_force_adjoint", slab, ny, ext_lo, ext_hi, X));
  const RowMap M = make_row_map(slab, nx, ny);      // (reads the stored face rows only; writes the owned NHWC rows, which every ExtRows holds)
  const CellWin cw = cell_window(M);
  closure_force_adjoint_kernel<<<closure_grid((long long)cw.n * 2), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(g, d_faces, d_nn_out, cw, M, X);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

}  // namespace

extern "C" {

int piso_closure_input(const float* faces, const float* pressure, float* nn_in, int nx, int ny, int channels, const int* pad_modes, double two_dx,
                       piso_stream_t stream) {
  return closure_input_impl(faces, pressure, nn_in, nx, ny, channels, pad_modes, two_dx, stream, nullptr, 0, 0);
}
int piso_closure_input_slab(const float* faces, const float* pressure, float* nn_in, int nx, int ny, int channels, const int* pad_modes, double two_dx,
                            piso_stream_t stream, const piso_slab_t* slab, int ext_lo, int ext_hi) {
  if (!slab) { set_error_msg("piso_closure_input_slab: NULL slab"); return PISO_ERR_INVALID_ARG; }
  return closure_input_impl(faces, pressure, nn_in, nx, ny, channels, pad_modes, two_dx, stream, slab, ext_lo, ext_hi);
}
int piso_closure_input_adjoint(const float* d_nn_in, float* d_faces, float* d_pressure, int nx, int ny, int channels, const int* pad_modes, double two_dx,
                               piso_stream_t stream) {
  return closure_input_adjoint_impl(d_nn_in, d_faces, d_pressure, nx, ny, channels, pad_modes, two_dx, stream, nullptr, 0, 0);
}
int piso_closure_input_adjoint_slab(const float* d_nn_in, float* d_faces, float* d_pressure, int nx, int ny, int channels, const int* pad_modes,
                                    double two_dx, piso_stream_t stream, const piso_slab_t* slab, int ext_lo, int ext_hi) {
  if (!slab) { set_error_msg("piso_closure_input_adjoint_slab: NULL slab"); return PISO_ERR_INVALID_ARG; }
  return closure_input_adjoint_impl(d_nn_in, d_faces, d_pressure, nx, ny, channels, pad_modes, two_dx, stream, slab, ext_lo, ext_hi);
}
int piso_closure_force(const float* nn_out, float* faces, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream) {
  return closure_force_impl(nn_out, faces, nx, ny, wrap_x, wrap_y, stream, nullptr, 0, 0);
}
int piso_closure_force_slab(const float* nn_out, float* faces, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream, const piso_slab_t* slab,
                            int ext_lo, int ext_hi) {
  if (!slab) { set_error_msg("piso_closure_force_slab: NULL slab"); return PISO_ERR_INVALID_ARG; }
  return closure_force_impl(nn_out, faces, nx, ny, wrap_x, wrap_y, stream, slab, ext_lo, ext_hi);
}
int piso_closure_force_adjoint(const float* d_faces, float* d_nn_out, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream) {
  return closure_force_adjoint_impl(d_faces, d_nn_out, nx, ny, wrap_x, wrap_y, stream, nullptr, 0, 0);
}
int piso_closure_force_adjoint_slab(const float* d_faces, float* d_nn_out, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream,
                                    const piso_slab_t* slab, int ext_lo, int ext_hi) {
  if (!slab) { set_error_msg("piso_closure_force_adjoint_slab: NULL slab"); return PISO_ERR_INVALID_ARG; }
  return closure_force_adjoint_impl(d_faces, d_nn_out, nx, ny, wrap_x, wrap_y, stream, slab, ext_lo, ext_hi);
}
int piso_closure_halo_add(float* dst, const float* src, size_t n, piso_stream_t stream) {
  if (!dst || !src) { set_error_msg("piso_closure_halo_add: invalid argument"); return PISO_ERR_INVALID_ARG; }
  if (n == 0) return PISO_OK;
  closure_halo_add_kernel<<<closure_grid((long long)n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(dst, src, n);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

}  // extern "C"
