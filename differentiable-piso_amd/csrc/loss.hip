// Fused training losses on the flat "u-first" face layout (u [ny][nx+1] followed by v [ny+1][nx]): the crop-window L2 loss and the
// strain-rate L1 loss of diffpiso/losses.py (the reference's losses.py:6-35, :66-95), value and gradient.
//
// Like every kernel of the step there is ONE per-element body per loss, instantiated for the whole grid and for one rank's rows of a
// grid cut into y-slabs (piso_*_slab): index rules - the crop window, the corner set of the off-diagonal strain entry, which entries
// read a face - are decided on whole-grid (i, j), only "where does row j live" goes through the rank's RowMap (piso_common.h).
//   value     two launches.  Every thread adds its elements' float64 terms, a block publishes ONE partial, one workgroup re-adds the
//             partials in a fixed order (reduce_partials): the double on the device is the same bits on every run.  A slab launch adds
//             the elements the rank owns (L2: its faces; strain: the entries of its cell rows) - the ranks' values add up to the grid's.
//   gradient  one launch, one thread per OWNED face, gathering: a face adds what the at most six strain entries that read it send back,
//             so nothing is scattered and no halo row is written.  The upstream scalar is read from the device.
// Both launches of the strain loss read rows j - 1 .. j + 1 of prediction and target: on slabs the caller fills the halo rows first.
// Arithmetic on the fields is float32 in the order of the torch losses (each strain entry for prediction and target on its own, then
// subtracted; -ffp-contract=off); only the sum is float64.  Bandwidth-trivial: x fastest, coalesced, no LDS beyond the block sum.
#include "piso_common.h"

namespace piso {

struct LossWin {                      // crop window on staggered-tensor indices: a face (j, i) counts iff y0 <= j < y1 and x0 <= i < x1
  int y0, y1, x0, x1;
  __device__ __forceinline__ bool has(int j, int i) const { return j >= y0 && j < y1 && i >= x0 && i < x1; }
};

// ---- L2: pred - target of a face inside the window, 0 outside.  f: whole-grid u-first index of a face that exists.
__device__ __forceinline__ float l2_diff(const float* __restrict__ pred, const float* __restrict__ tgt, int f, int nx, int ny, const LossWin& win,
                                         const RowMap& M, int* at) {
  const int n_u = (nx + 1) * ny;
  int j, i, k;
  if (f < n_u) { j = f / (nx + 1); i = f - j * (nx + 1); k = M.u(j, i); }
  else { const int q = f - n_u; j = q / nx; i = q - j * nx; k = M.v(j, i); }
  *at = k;
  return win.has(j, i) ? pred[k] - tgt[k] : 0.0f;
}

__global__ __launch_bounds__(kBlock) void loss_l2_value_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int nx, int ny,
                                                                LossWin win, FaceWin fw, RowMap M, double* __restrict__ part) {
  __shared__ double smem[4];
  double s[1] = {0.0};
  for (int w = blockIdx.x * kBlock + threadIdx.x; w < fw.count(); w += gridDim.x * kBlock) {
    int k;
    const double d = l2_diff(pred, tgt, fw.map(w), nx, ny, win, M, &k);
    s[0] += d * d;
  }
  block_sum<double, 1>(s, smem);
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(kBlock) void loss_l2_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int nx, int ny,
                                                               LossWin win, float factor, const float* __restrict__ upstream,
                                                               float* __restrict__ d_pred, FaceWin fw, RowMap M) {
  const float up = upstream[0];
  for (int w = blockIdx.x * kBlock + threadIdx.x; w < fw.count(); w += gridDim.x * kBlock) {
    int k;
    const float d = l2_diff(pred, tgt, fw.map(w), nx, ny, win, M, &k);
    d_pred[k] = (factor * d) * up;
  }
}

// ---- strain rate: the three kinds of entries (diffpiso/losses.py: _strain_parts), each for ONE field
struct StrainGeom {
  int nx, ny;
  float dx, dy;
};
// d v / d y at cell (j, i), 0 <= j < ny, 0 <= i < nx
__device__ __forceinline__ float strain_yy(const float* __restrict__ f, const StrainGeom& g, const RowMap& M, int j, int i) {
  return (f[M.v(j + 1, i)] - f[M.v(j, i)]) / g.dy;
}
// d u / d x at cell (j, i)
__device__ __forceinline__ float strain_xx(const float* __restrict__ f, const StrainGeom& g, const RowMap& M, int j, int i) {
  return (f[M.u(j, i + 1)] - f[M.u(j, i)]) / g.dx;
}
// the off-diagonal entry at the interior grid corner (j, i), 1 <= j <= ny - 1, 1 <= i <= nx - 1
__device__ __forceinline__ float strain_off(const float* __restrict__ f, const StrainGeom& g, const RowMap& M, int j, int i) {
  return ((f[M.v(j, i)] - f[M.v(j, i - 1)]) / g.dx + (f[M.u(j, i)] - f[M.u(j - 1, i)]) / g.dy) / 2.0f;
}
__device__ __forceinline__ bool strain_corner(const StrainGeom& g, int j, int i) { return j >= 1 && j <= g.ny - 1 && i >= 1 && i <= g.nx - 1; }
__device__ __forceinline__ float sgn(float x) { return static_cast<float>((x > 0.0f) - (x < 0.0f)); }      // sign(0) = 0

#define PISO_STRAIN_DELTA(kind, j, i) (strain_##kind(pred, g, M, (j), (i)) - strain_##kind(tgt, g, M, (j), (i)))

// value: the entries of the rank's cell rows - the two diagonal entries of cell (j, i) and the corner (j, i), which counts twice
__global__ __launch_bounds__(kBlock) void loss_strain_value_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, StrainGeom g,
                                                                    CellWin cw, RowMap M, double* __restrict__ part) {
  __shared__ double smem[4];
  double s[1] = {0.0};
  for (int c = cw.lo + blockIdx.x * kBlock + threadIdx.x; c < cw.lo + cw.n; c += gridDim.x * kBlock) {
    const int j = c / g.nx, i = c - j * g.nx;
    double t = static_cast<double>(fabsf(PISO_STRAIN_DELTA(yy, j, i)));
    if (strain_corner(g, j, i)) t += 2.0 * static_cast<double>(fabsf(PISO_STRAIN_DELTA(off, j, i)));
    t += static_cast<double>(fabsf(PISO_STRAIN_DELTA(xx, j, i)));
    s[0] += t;
  }
  block_sum<double, 1>(s, smem);
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

// gradient of one face: sign(entry(pred) - entry(target)) times the stencil weight over the entries that read the face.
// wx = factor / dx, wy = factor / dy; the corner entry counts twice, so its weights 1/2 / h become 1 / h.
__global__ __launch_bounds__(kBlock) void loss_strain_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, StrainGeom g,
                                                                   float wx, float wy, const float* __restrict__ upstream,
                                                                   float* __restrict__ d_pred, FaceWin fw, RowMap M) {
  const int nx = g.nx, ny = g.ny, n_u = (nx + 1) * ny;
  const float up = upstream[0];
  for (int w = blockIdx.x * kBlock + threadIdx.x; w < fw.count(); w += gridDim.x * kBlock) {
    const int f = fw.map(w);
    float s = 0.0f;
    if (f < n_u) {                                            // u face (j, i), 0 <= i <= nx
      const int j = f / (nx + 1), i = f - j * (nx + 1);
      if (i < nx) s -= sgn(PISO_STRAIN_DELTA(xx, j, i)) * wx;
      if (i >= 1) s += sgn(PISO_STRAIN_DELTA(xx, j, i - 1)) * wx;
      if (strain_corner(g, j, i)) s += sgn(PISO_STRAIN_DELTA(off, j, i)) * wy;
      if (strain_corner(g, j + 1, i)) s -= sgn(PISO_STRAIN_DELTA(off, j + 1, i)) * wy;
      d_pred[M.u(j, i)] = s * up;
    } else {                                                  // v face (j, i), 0 <= j <= ny
      const int q = f - n_u, j = q / nx, i = q - j * nx;
      if (j < ny) s -= sgn(PISO_STRAIN_DELTA(yy, j, i)) * wy;
      if (j >= 1) s += sgn(PISO_STRAIN_DELTA(yy, j - 1, i)) * wy;
      if (strain_corner(g, j, i)) s += sgn(PISO_STRAIN_DELTA(off, j, i)) * wx;
      if (strain_corner(g, j, i + 1)) s -= sgn(PISO_STRAIN_DELTA(off, j, i + 1)) * wx;
      d_pred[M.v(j, i)] = s * up;
    }
  }
}
#undef PISO_STRAIN_DELTA

// the second launch of a value: ONE workgroup adds the `count` partials in a fixed order and scales
__global__ __launch_bounds__(kBlock) void loss_finish_kernel(const double* __restrict__ part, int count, double scale, double* __restrict__ out) {
  __shared__ double smem[4];
  double s[1];
  reduce_partials<double, 1>(part, count, s, smem);
  if (threadIdx.x == 0) out[0] = scale * s[0];
}

static int loss_grid(long long n) { return grid_for(n, kBlock * 2, kMaxPartials); }

}  // namespace piso

using namespace piso;

namespace {

#define PISO_SLAB_CHECK(what)                                                                                     \
  if (!slab_ok(slab, ny)) { set_error_msg(what ": invalid slab (rows must lie inside the grid, at least 4, at most ny - 6)"); return PISO_ERR_INVALID_ARG; }

// the window clipped to the staggered tensor [ny + 1][nx + 1] (the faces that exist are the launch's own index space)
bool make_window(int nx, int ny, int y0, int y1, int x0, int x1, LossWin* w) {
  if (y0 < 0 || x0 < 0 || y1 > ny + 1 || x1 > nx + 1) return false;
  w->y0 = y0; w->y1 = y1 > y0 ? y1 : y0; w->x0 = x0; w->x1 = x1 > x0 ? x1 : x0;
  return true;
}

int l2_value_impl(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, double factor, double* value,
                  void* workspace, size_t workspace_bytes, piso_stream_t stream_, const piso_slab_t* slab) {
  LossWin win;
  if (!pred || !target || !value || !workspace || nx < 1 || ny < 1 || workspace_bytes < piso_loss_workspace_bytes() ||
      !make_window(nx, ny, y0, y1, x0, x1, &win)) {
    set_error_msg("piso_loss_l2: invalid argument (window inside [0, ny + 1] x [0, nx + 1], workspace of piso_loss_workspace_bytes())");
    return PISO_ERR_INVALID_ARG;
  }
  PISO_SLAB_CHECK("piso_loss_l2");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const RowMap M = make_row_map(slab, nx, ny);
  const FaceWin fw = face_window(M);
  const int grid = loss_grid(fw.count());
  double* part = static_cast<double*>(workspace);
  loss_l2_value_kernel<<<grid, kBlock, 0, stream>>>(pred, target, nx, ny, win, fw, M, part);
  loss_finish_kernel<<<1, kBlock, 0, stream>>>(part, grid, factor / 2, value);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int l2_grad_impl(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, float factor, const float* upstream,
                 float* d_pred, piso_stream_t stream_, const piso_slab_t* slab) {
  LossWin win;
  if (!pred || !target || !upstream || !d_pred || nx < 1 || ny < 1 || !make_window(nx, ny, y0, y1, x0, x1, &win)) {
    set_error_msg("piso_loss_l2_grad: invalid argument (window inside [0, ny + 1] x [0, nx + 1])");
    return PISO_ERR_INVALID_ARG;
  }
  PISO_SLAB_CHECK("piso_loss_l2_grad");
  const RowMap M = make_row_map(slab, nx, ny);
  const FaceWin fw = face_window(M);
  loss_l2_grad_kernel<<<loss_grid(fw.count()), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(pred, target, nx, ny, win, factor, upstream, d_pred,
                                                                                                  fw, M);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int strain_value_impl(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, double* value, void* workspace,
                      size_t workspace_bytes, piso_stream_t stream_, const piso_slab_t* slab) {
  if (!pred || !target || !value || !workspace || nx < 2 || ny < 2 || !(dx > 0.0f) || !(dy > 0.0f) ||
      workspace_bytes < piso_loss_workspace_bytes()) {
    set_error_msg("piso_loss_strain: invalid argument (nx, ny >= 2, dx, dy > 0, workspace of piso_loss_workspace_bytes())");
    return PISO_ERR_INVALID_ARG;
  }
  PISO_SLAB_CHECK("piso_loss_strain");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const RowMap M = make_row_map(slab, nx, ny);
  const CellWin cw = cell_window(M);
  const int grid = loss_grid(cw.n);
  double* part = static_cast<double*>(workspace);
  loss_strain_value_kernel<<<grid, kBlock, 0, stream>>>(pred, target, StrainGeom{nx, ny, dx, dy}, cw, M, part);
  loss_finish_kernel<<<1, kBlock, 0, stream>>>(part, grid, factor, value);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int strain_grad_impl(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, const float* upstream,
                     float* d_pred, piso_stream_t stream_, const piso_slab_t* slab) {
  if (!pred || !target || !upstream || !d_pred || nx < 2 || ny < 2 || !(dx > 0.0f) || !(dy > 0.0f)) {
    set_error_msg("piso_loss_strain_grad: invalid argument (nx, ny >= 2, dx, dy > 0)");
    return PISO_ERR_INVALID_ARG;
  }
  PISO_SLAB_CHECK("piso_loss_strain_grad");
  const RowMap M = make_row_map(slab, nx, ny);
  const FaceWin fw = face_window(M);
  const float wx = static_cast<float>(factor / static_cast<double>(dx)), wy = static_cast<float>(factor / static_cast<double>(dy));
  loss_strain_grad_kernel<<<loss_grid(fw.count()), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(pred, target, StrainGeom{nx, ny, dx, dy}, wx, wy,
                                                                                                      upstream, d_pred, fw, M);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}
#undef PISO_SLAB_CHECK

}  // namespace

extern "C" {

size_t piso_loss_workspace_bytes(void) { return static_cast<size_t>(kMaxPartials) * sizeof(double); }

int piso_loss_l2(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, double factor, double* value,
                 void* workspace, size_t workspace_bytes, piso_stream_t stream) {
  return l2_value_impl(pred, target, nx, ny, y0, y1, x0, x1, factor, value, workspace, workspace_bytes, stream, nullptr);
}
int piso_loss_l2_slab(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, double factor, double* value,
                      void* workspace, size_t workspace_bytes, piso_stream_t stream, const piso_slab_t* slab) {
  return l2_value_impl(pred, target, nx, ny, y0, y1, x0, x1, factor, value, workspace, workspace_bytes, stream, slab);
}
int piso_loss_l2_grad(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, float factor,
                      const float* upstream, float* d_pred, piso_stream_t stream) {
  return l2_grad_impl(pred, target, nx, ny, y0, y1, x0, x1, factor, upstream, d_pred, stream, nullptr);
}
int piso_loss_l2_grad_slab(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, float factor,
                           const float* upstream, float* d_pred, piso_stream_t stream, const piso_slab_t* slab) {
  return l2_grad_impl(pred, target, nx, ny, y0, y1, x0, x1, factor, upstream, d_pred, stream, slab);
}
int piso_loss_strain(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, double* value, void* workspace,
                     size_t workspace_bytes, piso_stream_t stream) {
  return strain_value_impl(pred, target, nx, ny, dx, dy, factor, value, workspace, workspace_bytes, stream, nullptr);
}
int piso_loss_strain_slab(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, double* value,
                          void* workspace, size_t workspace_bytes, piso_stream_t stream, const piso_slab_t* slab) {
  return strain_value_impl(pred, target, nx, ny, dx, dy, factor, value, workspace, workspace_bytes, stream, slab);
}
int piso_loss_strain_grad(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, const float* upstream,
                          float* d_pred, piso_stream_t stream) {
  return strain_grad_impl(pred, target, nx, ny, dx, dy, factor, upstream, d_pred, stream, nullptr);
}
int piso_loss_strain_grad_slab(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, const float* upstream,
                               float* d_pred, piso_stream_t stream, const piso_slab_t* slab) {
  return strain_grad_impl(pred, target, nx, ny, dx, dy, factor, upstream, d_pred, stream, slab);
}

}  // extern "C"
