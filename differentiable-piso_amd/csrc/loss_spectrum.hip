// Fused spectral-energy loss (diffpiso/losses.py: spectral_energy_loss(..., fused=True); the reference's losses.py:38-64 over
// evaluation_tools.py:157-186) around the rocFFT transform that stays in torch.fft.  Whole-grid kernels, no atomics:
//   centre + crop   flat u-first face vector -> two float32 planes [2][h][w] (plane 0: v at the cell centres, plane 1: u - the channel
//                   order of StaggeredGrid.at_centers()), the crop [y0, y1) x [x0, x1) on CELL indices; 0.5f * (a + b) like the torch op.
//                   Adjoint: one thread per face GATHERS 0.5 * g from the at most two cropped cells that read it; zero elsewhere.
//   shell sums      the interleaved complex64 transform of the planes -> E[cutoff] in float64.  Which cells belong to shell k is a table
//                   built once per crop shape on the host (losses.spectrum_plan): perm[offsets[k] : offsets[k + 1]] lists the UNSHIFTED
//                   FFT indices of shell k in ascending order.  One workgroup per shell walks its list strided by thread and ends in the
//                   fixed-order block sum: the same bits on every run, where index_add adds with float atomics.
//                   Adjoint: a pure map over the coefficients through shell[q] - nothing is scattered.
//   distance        one workgroup: E_pred, E_gt -> the loss term and d term / d E_pred, both float64.
// |c|^2 of a float32 pair is formed in float64 (exact products); -ffp-contract=off like loss.hip.
#include "piso_common.h"

namespace piso {

struct CropWin {                      // the crop on cell indices: cell (j, i) counts iff y0 <= j < y1 and x0 <= i < x1; h = y1 - y0, w = x1 - x0
  int y0, y1, x0, x1, h, w;
  __device__ __forceinline__ bool has(int j, int i) const { return j >= y0 && j < y1 && i >= x0 && i < x1; }
  __device__ __forceinline__ int at(int j, int i) const { return (j - y0) * w + (i - x0); }
};

__global__ __launch_bounds__(kBlock) void centre_crop_kernel(const float* __restrict__ faces, int nx, int ny, CropWin win,
                                                              float* __restrict__ planes) {
  const int n_u = (nx + 1) * ny, hw = win.h * win.w;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < 2 * hw; t += gridDim.x * kBlock) {
    const int comp = t >= hw, r = t - comp * hw;
    const int jj = r / win.w, j = win.y0 + jj, i = win.x0 + (r - jj * win.w);
    planes[t] = comp ? 0.5f * (faces[j * (nx + 1) + i + 1] + faces[j * (nx + 1) + i])
                     : 0.5f * (faces[n_u + (j + 1) * nx + i] + faces[n_u + j * nx + i]);
  }
}

__global__ __launch_bounds__(kBlock) void centre_crop_adjoint_kernel(const float* __restrict__ d_planes, int nx, int ny, CropWin win,
                                                                      float* __restrict__ d_faces) {
  const int n_u = (nx + 1) * ny, n = n_u + nx * (ny + 1), hw = win.h * win.w;
  for (int f = blockIdx.x * kBlock + threadIdx.x; f < n; f += gridDim.x * kBlock) {
    float s = 0.0f;
    if (f < n_u) {                                            // u face (j, i): read by the cells (j, i - 1) and (j, i)
      const int j = f / (nx + 1), i = f - j * (nx + 1);
      if (win.has(j, i - 1)) s += 0.5f * d_planes[hw + win.at(j, i - 1)];
      if (win.has(j, i)) s += 0.5f * d_planes[hw + win.at(j, i)];
    } else {                                                  // v face (j, i): read by the cells (j - 1, i) and (j, i)
      const int q = f - n_u, j = q / nx, i = q - j * nx;
      if (win.has(j - 1, i)) s += 0.5f * d_planes[win.at(j - 1, i)];
      if (win.has(j, i)) s += 0.5f * d_planes[win.at(j, i)];
    }
    d_faces[f] = s;
  }
}

// spec: [2][hw] complex64 as (re, im) float pairs.  Block k = shell k.
__global__ __launch_bounds__(kBlock) void spectrum_shells_kernel(const float2* __restrict__ spec, const int* __restrict__ perm,
                                                                  const int* __restrict__ offsets, int hw, double scale,
                                                                  double* __restrict__ energy) {
  __shared__ double smem[4];
  const int k = blockIdx.x, end = offsets[k + 1];
  double s[1] = {0.0};
  for (int t = offsets[k] + threadIdx.x; t < end; t += kBlock) {
    const int q = perm[t];
    if (static_cast<unsigned>(q) >= static_cast<unsigned>(hw)) continue;     // (a table that is not this crop's must not read out of bounds)
    const float2 a = spec[q], b = spec[hw + q];
    const double ar = a.x, ai = a.y, br = b.x, bi = b.y;
    s[0] += (ar * ar + ai * ai) + (br * br + bi * bi);
  }
  block_sum<double, 1>(s, smem);
  if (threadIdx.x == 0) energy[k] = scale * s[0];
}

// d_spec[c][q] = upstream * 2 * scale * d_energy[shell[q]] * spec[c][q]; 0 where the shell lies at or beyond the cutoff
__global__ __launch_bounds__(kBlock) void spectrum_shells_adjoint_kernel(const float2* __restrict__ spec, const int* __restrict__ shell,
                                                                          const double* __restrict__ d_energy, const float* __restrict__ upstream,
                                                                          int hw, int cutoff, double scale2, float2* __restrict__ d_spec) {
  const double up = upstream ? static_cast<double>(upstream[0]) * scale2 : scale2;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < 2 * hw; t += gridDim.x * kBlock) {
    const int q = t >= hw ? t - hw : t, k = shell[q];
    float2 out = make_float2(0.0f, 0.0f);
    if (static_cast<unsigned>(k) < static_cast<unsigned>(cutoff)) {
      const double c = up * d_energy[k];
      const float2 z = spec[t];
      out.x = static_cast<float>(c * static_cast<double>(z.x));
      out.y = static_cast<float>(c * static_cast<double>(z.y));
    }
    d_spec[t] = out;
  }
}

// one workgroup.  first: the first shell that counts (log form: 1 + start_wavenumber; absolute form: 1)
__global__ __launch_bounds__(kBlock) void spectrum_distance_kernel(const double* __restrict__ e_pred, const double* __restrict__ e_gt, int cutoff,
                                                                    int first, int log_distance, double factor, double* __restrict__ value,
                                                                    double* __restrict__ d_e_pred) {
  __shared__ double smem[4];
  double s[1] = {0.0};
  for (int k = first + threadIdx.x; k < cutoff; k += kBlock) {
    if (log_distance) {
      const double t = log(e_gt[k] / e_pred[k]);
      s[0] += t * t;
    } else {
      s[0] += fabs(e_gt[k] - e_pred[k]);
    }
  }
  block_sum<double, 1>(s, smem);
  const double total = s[0], root = sqrt(total);
  if (threadIdx.x == 0) value[0] = log_distance ? factor * root : factor * total;
  for (int k = threadIdx.x; k < cutoff; k += kBlock) {
    double d = 0.0;
    if (k >= first) {
      if (log_distance) {
        // d sqrt(S) / d e_k = -log(g_k / e_k) / (sqrt(S) e_k); S == 0 (identical spectra): 0, where sqrt'(0) would give NaN
        if (total != 0.0) d = -factor * log(e_gt[k] / e_pred[k]) / (root * e_pred[k]);
      } else {
        const double diff = e_gt[k] - e_pred[k];
        d = -factor * static_cast<double>((diff > 0.0) - (diff < 0.0));
      }
    }
    d_e_pred[k] = d;
  }
}

static int spectrum_grid(long long n) { return grid_for(n, kBlock * 2, kMaxPartials); }

}  // namespace piso

using namespace piso;

namespace {

constexpr long long kMaxCropCells = 1LL << 28;                // 4 h w float indices stay below 2^31

bool make_crop(int nx, int ny, int y0, int y1, int x0, int x1, CropWin* w) {
  if (nx < 1 || ny < 1 || y0 < 0 || x0 < 0 || y1 > ny || x1 > nx || y1 - y0 < 1 || x1 - x0 < 1) return false;
  if (static_cast<long long>(nx + 1) * (ny + 1) > kMaxCropCells) return false;
  *w = CropWin{y0, y1, x0, x1, y1 - y0, x1 - x0};
  return true;
}

bool crop_shape_ok(int h, int w, int cutoff) {
  return h >= 1 && w >= 1 && static_cast<long long>(h) * w <= kMaxCropCells && cutoff >= 0 && cutoff <= (h < w ? h : w) / 2;
}

}  // namespace

extern "C" {

int piso_loss_centre_crop(const float* faces, int nx, int ny, int y0, int y1, int x0, int x1, float* planes, piso_stream_t stream) {
  CropWin win;
  if (!faces || !planes || !make_crop(nx, ny, y0, y1, x0, x1, &win)) {
    set_error_msg("piso_loss_centre_crop: invalid argument (non-null pointers, nx, ny >= 1, a crop 0 <= y0 < y1 <= ny, 0 <= x0 < x1 <= nx on cell indices)");
    return PISO_ERR_INVALID_ARG;
  }
  centre_crop_kernel<<<spectrum_grid(2LL * win.h * win.w), kBlock, 0, static_cast<hipStream_t>(stream)>>>(faces, nx, ny, win, planes);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int piso_loss_centre_crop_adjoint(const float* d_planes, int nx, int ny, int y0, int y1, int x0, int x1, float* d_faces, piso_stream_t stream) {
  CropWin win;
  if (!d_planes || !d_faces || !make_crop(nx, ny, y0, y1, x0, x1, &win)) {
    set_error_msg("piso_loss_centre_crop_adjoint: invalid argument (non-null pointers, nx, ny >= 1, a crop 0 <= y0 < y1 <= ny, 0 <= x0 < x1 <= nx on cell indices)");
    return PISO_ERR_INVALID_ARG;
  }
  const long long n = static_cast<long long>(nx + 1) * ny + static_cast<long long>(nx) * (ny + 1);
  centre_crop_adjoint_kernel<<<spectrum_grid(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(d_planes, nx, ny, win, d_faces);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int piso_loss_spectrum_shells(const float* spec, const int* perm, const int* offsets, int h, int w, int cutoff, double* energy,
                              piso_stream_t stream) {
  if (!spec || !perm || !offsets || !energy || !crop_shape_ok(h, w, cutoff)) {
    set_error_msg("piso_loss_spectrum_shells: invalid argument (non-null pointers, h, w >= 1, 0 <= cutoff <= min(h, w) / 2)");
    return PISO_ERR_INVALID_ARG;
  }
  if (cutoff == 0) return PISO_OK;                            // (a crop one cell wide has no shell below its cutoff)
  const double cells = static_cast<double>(h) * static_cast<double>(w);
  spectrum_shells_kernel<<<cutoff, kBlock, 0, static_cast<hipStream_t>(stream)>>>(reinterpret_cast<const float2*>(spec), perm, offsets, h * w,
                                                                                 0.5 / (cells * cells), energy);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int piso_loss_spectrum_shells_adjoint(const float* spec, const int* shell, const double* d_energy, const float* upstream, int h, int w, int cutoff,
                                      float* d_spec, piso_stream_t stream) {
  if (!spec || !shell || !d_energy || !d_spec || !crop_shape_ok(h, w, cutoff)) {
    set_error_msg("piso_loss_spectrum_shells_adjoint: invalid argument (non-null pointers - upstream alone may be NULL -, h, w >= 1, "
                  "0 <= cutoff <= min(h, w) / 2)");
    return PISO_ERR_INVALID_ARG;
  }
  const double cells = static_cast<double>(h) * static_cast<double>(w);
  spectrum_shells_adjoint_kernel<<<spectrum_grid(2LL * h * w), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float2*>(spec), shell, d_energy, upstream, h * w, cutoff, 2.0 * (0.5 / (cells * cells)), reinterpret_cast<float2*>(d_spec));
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

int piso_loss_spectrum_distance(const double* e_pred, const double* e_gt, int cutoff, int start_wavenumber, int log_distance, double factor,
                                double* value, double* d_e_pred, piso_stream_t stream) {
  if (!e_pred || !e_gt || !value || !d_e_pred || cutoff < 0 || start_wavenumber < 0 || start_wavenumber > (1 << 30)) {
    set_error_msg("piso_loss_spectrum_distance: invalid argument (non-null pointers, cutoff >= 0, start_wavenumber >= 0)");
    return PISO_ERR_INVALID_ARG;
  }
  const int first = log_distance ? 1 + start_wavenumber : 1;
  spectrum_distance_kernel<<<1, kBlock, 0, static_cast<hipStream_t>(stream)>>>(e_pred, e_gt, cutoff, first, log_distance ? 1 : 0, factor, value,
                                                                             d_e_pred);
  PISO_LAUNCH_CHECK();
  return PISO_OK;
}

}  // extern "C"
