/*
 * piso_hip.h -- C ABI of libpiso_hip.so, the MI355X (gfx950) native library behind the differentiable-PISO hot path.
 *
 * Drop-in boundary: each entry point replaces one native launcher of tum-pbs/differentiable-piso (the functions the
 * reference's TensorFlow OpKernel shells call after unpacking their tensors).  Differences from the reference launchers,
 * all deliberate:
 *   - every array argument is a DEVICE pointer owned by the caller; small scalars (sizes, tolerances, flags) are passed
 *     BY VALUE instead of as device arrays that the launcher copies back to the host;
 *   - an explicit HIP stream (hipStream_t passed as void*; NULL = the null stream);
 *   - scratch memory is a caller-provided workspace (query *_workspace_bytes first); nothing is hipMalloc'ed per call;
 *   - an int status is returned (PISO_OK == 0) instead of exit(1)/assert(0);
 *   - outputs are separate arrays (no input buffer is overwritten in place).
 * Numerical failure handling mirrors the reference: non-convergence of BiCGStab yields a zero solution after one restart,
 * NaN input sets warning[0] = 1; the pressure CG reports its iteration count.
 *
 * Layout conventions (identical to the reference):
 *   nx, ny          cell resolution; x is the fastest index everywhere
 *   u faces         [ny][nx+1]     v faces [ny+1][nx]      "u-first" flat vector = u followed by v
 *   padded u        [ny+2][nx+3]   padded v [ny+3][nx+2]   (custom_padded, diffpiso/piso_helpers.py:35-55)
 *   cell masks      [ny+2][nx+2]   (one ghost ring)        pressure / divergence [ny][nx]
 *   pressure matrix [ny*nx][5]     row = (-y, -x, diag, +x, +y)
 *   A0 (face coefficient of the pressure matrix) flat "v-first": v faces followed by u faces
 */
#ifndef PISO_HIP_H
#define PISO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PISO_OK 0
#define PISO_ERR_INVALID_ARG 1       /* bad size / NULL pointer / workspace too small */
#define PISO_ERR_HIP 2               /* a HIP runtime call failed (piso_last_error_string() has the text) */
#define PISO_ERR_UNSUPPORTED_PATTERN 3 /* CSR input is not a 5-point staggered-grid matrix */
#define PISO_ERR_NO_DEVICE 4
#define PISO_ERR_NEEDS_HOST 5        /* piso_cg_solve_async_*: this grid is solved with the host in the loop, call piso_cg_solve_* */

typedef void* piso_stream_t;

/* One rank's part of a grid cut into y-slabs (the slab-decomposed STEP; no counterpart in the reference).  The *_slab
 * twin of an entry point takes the same arguments as the entry point itself - nx, ny and every index rule are the WHOLE grid's -
 * plus this struct; its arrays hold the rank's rows only (LOCAL storage; round 5 - there is no process-wide row window any more):
 *   cell arrays, u faces   the ring rows [row_begin - 2, row_end + 2) (mod ny_global), row_end - row_begin + 4 of them
 *   v faces                the ring rows [row_begin - 3, row_end + 3) of the ring v[0] .. v[ny - 1], v[ny] (the duplicate row),
 *                          row_end - row_begin + 6 of them; flat face vectors: the stored u rows followed by the stored v rows
 *                          (v-first vectors: v then u)
 *   padded cell masks      rows [row_begin, row_begin + (row_end - row_begin) + 3) of the [ny + 2] padded rows (no ring)
 *   padded velocities      padded u rows [row_begin, row_end + 2), then padded v rows [row_begin, row_end + 3): the STORAGE.
 *                          piso_pad_velocity_slab fills padded u rows [row_begin, row_end + 1 + owns_last_face_row) and padded v rows
 *                          [row_begin, row_end + 2 + owns_last_face_row) - all the assembly of the owned face rows reads - and leaves the
 *                          remaining stored row of each component (every slab but the last has one) untouched
 *   CSR                    the rows of the stored face rows (u rows, then v rows) in stored order; row pointers
 *                          [stored u rows (nx + 1) + 1][stored v rows nx + 1] are offsets into the stored value / column arrays of
 *                          each component; column indices keep the whole grid's numbering (component-local row numbers)
 *   pressure matrix, CG    the owned rows only ([row_end - row_begin][nx][5]; what piso_cg_solve_slab_* takes)
 * A launch writes the OWNED rows (cells / u rows [row_begin, row_end), v rows [row_begin, row_end + owns_last_face_row)) and reads
 * the stored rows around them, which the caller fills with piso_comm_exchange (element segments of the stored arrays).
 * Constraints: 0 <= row_begin, row_end <= ny_global, 4 <= row_end - row_begin <= ny_global - 6, and owns_last_face_row only with
 * row_end == ny_global (a slab below the last one would write v[row_end], which its upper neighbour owns); anything else:
 * PISO_ERR_INVALID_ARG.  row_end == ny_global WITHOUT owns_last_face_row is accepted: that launch leaves v[ny] to its caller (no
 * entry point then writes it; the stored arrays are the same either way). */
typedef struct piso_slab {
  int ny_global;              /* cell rows of the whole grid (must equal the entry point's ny) */
  int row_begin, row_end;     /* owned cell rows */
  int owns_last_face_row;     /* the last slab also owns the duplicate face row v[ny] */
} piso_slab_t;

/* Library / build information. */
const char* piso_version(void);
const char* piso_last_error_string(void);
/* Number of visible HIP devices (0 if none; never initialises a context). */
int piso_device_count(void);
/* Tuning / test knobs (no counterpart in the reference).  NONE of them changes what is computed: a knob picks between implementations
 * that return bitwise the same result (which kernel instance runs, how operands are staged, launch shapes) or switches a check / a
 * measurement aid on and off.  Each knob `name` takes its default ONCE, at library load, from the environment variable
 * PISO_<NAME IN UPPER CASE>; -1 = not set (automatic).  The store is process-wide and atomic; every entry point that reads knobs copies
 * ALL of them when it is entered and works on that snapshot, so a piso_set_option() from another thread (a test flipping a knob while an
 * autograd backward thread is inside a solve) never changes a decision in the middle of a call.  The list, with what each one selects,
 * is differentiable-piso_amd/csrc/options.h; the ones callers outside the tests use:
 *   cg_persist (0 forbid / 1 force the persistent CG kernel; default by grid size), cg_persist_r (2|4|16 rows per region),
 *   cg_segment (iterations per persistent launch), cg_verify (0: skip the true-residual check of persistent solves),
 *   slab_force (1: a communicator of ONE rank still runs the slab code paths - a ring with itself),
 *   bicg_fold / bicg_sweep_lds / bicg_fuse_p (0: the un-fused forms of the BiCGStab stages), conv_lds (0: closure convolutions read
 *   their operands straight from L2). */
int piso_set_option(const char* name, int value);
int piso_get_option(const char* name, int* value_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Advection-diffusion matrix assembly.
 * Replaces CentralDifferenceMatrixCsrKernelLauncher (CUDAsrc/central_difference_csr_op.cc:33-36,
 * CUDAsrc/central_difference_csr_op.cu.cc:543-664; kernels :148-453, :472-505).
 *   vel_pad      [(ny+2)(nx+3) + (ny+3)(nx+2)] padded u then padded v
 *   csr_val/col  [nnz_u + nnz_v]; csr_rowptr [n_u+1 + n_v+1] (two 0-based segments); diag [n_u + n_v] (the "A" array)
 *   dirichlet    [n_u + n_v] bytes (u first); active [(ny+2)(nx+2)]; no_slip [(ny+2)(nx+2)] bytes or NULL
 *   viscosity    1 value, or n_u+n_v values when viscosity_is_field != 0
 *   cell_area_x/y = area of the x-/y-normal face (dy, dx); spacing_x/y = (dx, dy); beta = dx*dy/dt
 * nnz_u/nnz_v follow diffpiso/piso_tf.py:102-106; piso_csr_nnz() returns them.
 * ------------------------------------------------------------------------------------------------------------- */
void piso_csr_nnz(int nx, int ny, int periodic_x, int periodic_y, int* nnz_u, int* nnz_v);

int piso_assemble_csr(const float* vel_pad, float* csr_val, int* csr_col, int* csr_rowptr, float* diag,
                      const uint8_t* dirichlet, const float* active, const float* viscosity, int viscosity_is_field,
                      int nx, int ny, int periodic_x, int periodic_y, float cell_area_x, float cell_area_y,
                      float spacing_x, float spacing_y, const uint8_t* no_slip, float beta, piso_stream_t stream);
/* one rank's rows (piso_slab_t).  pattern_only != 0: column indices and row pointers of ALL stored rows (owned and halo: the pattern is
 * geometry), no values - called once per set-up; pattern_only == 0: values, columns, row pointers and diag of the OWNED rows. */
int piso_assemble_csr_slab(const float* vel_pad, float* csr_val, int* csr_col, int* csr_rowptr, float* diag,
                           const uint8_t* dirichlet, const float* active, const float* viscosity, int viscosity_is_field,
                           int nx, int ny, int periodic_x, int periodic_y, float cell_area_x, float cell_area_y,
                           float spacing_x, float spacing_y, const uint8_t* no_slip, float beta, piso_stream_t stream,
                           const piso_slab_t* slab, int pattern_only);
/* sizes of a rank's stored arrays (piso_slab_t): out8 = {stored u rows, stored v rows, stored u faces, stored v faces, stored CSR
 * entries of the u matrix, of the v matrix, stored mask rows, elements of the stored padded velocities} */
int piso_slab_sizes(const piso_slab_t* slab, int nx, int ny, int periodic_x, int periodic_y, int* out8);

/* ---------------------------------------------------------------------------------------------------------------
 * ILU(0)-preconditioned BiCGStab on the u and v matrices (both components advance in the same launches).
 * Replaces MultiBicgstabIluLinearSolveLauncher (CUDAsrc/multi_bicgstab_ilu_linear_solve_op.cc:50-58,
 * .cu.cc:455-531 float / :912-988 double; per-component algorithm :85-453 / :540-910).
 *   csr_*      the concatenated two-matrix CSR produced by piso_assemble_csr (values possibly negated by the caller)
 *   rhs, x0    [n_u + n_v];  x_out [n_u + n_v]
 *   tol        absolute ||r||_2 tolerance; max_it per restart; transpose: bit 0 = solve with A^T (adjoint), bit 1 = the system matrix
 *              is -csr_val (the reference hands the op `-matrix_values`, piso_tf.py:41: the sign is applied where the values are read);
 *              any other bit set: PISO_ERR_INVALID_ARG (a caller meaning "non-zero = transpose" with 2 or -1 must not get another system)
 *   band_rows  rows of faces per preconditioner block: < 0  = one block (global structured ILU0),
 *              0 = automatic (8 rows from ny = 2048 on, 4 from 1024, 2 from 256, 8 below), > 0 = that many.  See DESIGN.md "structured block ILU0".
 *   warning    device byte, set to 1 on NaN input (never cleared);  iterations_out: host int[2] or NULL
 * Scope limits: 4 <= nx <= 8191, ny >= 4; the CSR must be the 5-point staggered-grid pattern piso_assemble_csr produces
 * (any other matrix: PISO_ERR_UNSUPPORTED_PATTERN) -- this is not a general CSR solver.
 * ------------------------------------------------------------------------------------------------------------- */
size_t piso_bicgstab_workspace_bytes(int nx, int ny, int elem_size);

int piso_multi_bicgstab_ilu_f32(const float* csr_val, const int* csr_rowptr, const int* csr_col, const float* rhs,
                                const float* x0, float* x_out, int nx, int ny, float tol, int max_it, int transpose,
                                int band_rows, uint8_t* warning, int* iterations_out, void* workspace,
                                size_t workspace_bytes, piso_stream_t stream);
int piso_multi_bicgstab_ilu_f64(const double* csr_val, const int* csr_rowptr, const int* csr_col, const double* rhs,
                                const double* x0, double* x_out, int nx, int ny, float tol, int max_it, int transpose,
                                int band_rows, uint8_t* warning, int* iterations_out, void* workspace,
                                size_t workspace_bytes, piso_stream_t stream);
/* Which kernel instances the calling thread's last piso_multi_bicgstab_ilu_* solve (one GPU or slab: they share the driver) ran:
 * out[0 .. min(return value, capacity)); returns the number of fields (0: this thread has not solved, or its last call was refused
 * before it chose).  Read-only: the record is written on the host while the solve is set up - the last three fields when it returns -
 * and changes nothing that is computed.  Fields, in this order:
 *    0 sizeof(T)        8 / 4
 *    1 E                row elements per thread of bi_factor / bi_sweep: the smallest of 1, 2, 3, 4, 5, 8, 9, 16, 32 with nx + 1 <= 256 E
 *    2 sweep_lds        1: the sweeps that stage rows through LDS ran (bi_sweep<.., LDS = true>: float E = 5, 8, 9, 16, double E = 5, 8, 9; option
 *                       bicg_sweep_lds 0: never)
 *    3 factor_lds       1: likewise the factorisation (bi_factor<.., LDS = true>, the same instances)
 *    4 R                band height in face rows after the automatic choice and the clamp to ny + 1
 *    5 bands_u          bands (= workgroups of a sweep) of the u component this rank works on: ceil(ny / R) on one GPU
 *    6 bands_v          ... of the v component: ceil((ny + 1) / R) - a last band of one row when R divides ny
 *    7 blocks           workgroups per component of the vector kernels (a multiple of 8, at most 1 024; slab: interior + edge blocks)
 *    8 fold             1: the scalar stages are folded into the kernels that consume them (one GPU; option bicg_fold 0: never)
 *    9 fuse_p           1: the direction update runs inside the forward sweep (option bicg_fuse_p 0: never)
 *   10 transpose_flags  the call's `transpose` argument: bit 0 A^T, bit 1 negated values
 *   11 slab             1: the rows are split over the ranks of a communicator (or option slab_force)
 *   12 look0            iterations before the host first fetches the scalar record: 1 below 32 768 rows in all, else 2 (then 2, 2, 4, 8, 16 ...)
 *   13 passes           1, or 2 when a component ended above 100 tol (or at NaN), was zeroed and run again from x = 0
 *   14 host_looks       device-to-host fetches of the scalar record over both passes
 *   15 failed_mask      bit c: component c was above 100 tol after the second pass as well and was returned as zeros */
int piso_bicgstab_last_dispatch(int* out, int capacity);

/* y = A x (transpose == 0) or A^T x on the concatenated two-matrix CSR; the H-operator product of the second corrector
 * (diffpiso/piso_helpers.py:209-223 uses tf.gather/segment_sum for it). */
int piso_csr_matvec_f32(const float* csr_val, const int* csr_rowptr, const int* csr_col, const float* x, float* y,
                        int nx, int ny, int transpose, piso_stream_t stream);
int piso_csr_matvec_f32_slab(const float* csr_val, const int* csr_rowptr, const int* csr_col, const float* x, float* y,
                             int nx, int ny, int periodic_x, int periodic_y, int transpose, piso_stream_t stream, const piso_slab_t* slab);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused stencil glue of the step on the flat "u-first" face layout, forward and reverse mode (csrc/glue.hip).  Replaces the
 * TensorFlow / PhiFlow-math ops of diffpiso/piso_tf.py:36-73 and diffpiso/piso_helpers.py:35-55 (custom_padded), :169-172
 * (arrange_rhs_term_tf), :226-274 (finite_volume_gradient_tensor, circular_padded_gradient), :277-310
 * (finite_volume_divergence) and :223 (the H combination).  The reverse-mode entries implement the reference's custom
 * gradients, including their deviations from the exact transpose.
 *   pad_modes   int[4] = pressure extrapolation (x_lo, x_hi, y_lo, y_hi): 0 'constant' (zero), 1 'boundary' (edge), 2 'periodic'
 *   accessible  [(ny+2)(nx+2)] padded cell mask of the gradient (piso_helpers.py:255-265) or NULL (no mask)
 *   a_flat      [n_u+n_v] the "A" array of piso_assemble_csr;  dirichlet [n_u+n_v] bytes or NULL;  hx, hy = (dx, dy)
 * piso_face_forward, by mode (G = masked finite-volume pressure gradient on the faces):
 *   0 RHS    out0 = dirichlet ? -in2 : in0 * beta - G(p) [+ in1 * dxdy]     in0 velocity, in1 forcing or NULL, in2 Dirichlet values
 *   1 CORR1  out0 = in0 - (G(p) / (beta - A)) / dxdy ; out1 = out0 - in0     in0 = u*
 *   2 FINAL  out0 = in0 + (in1 - G(p) / dxdy) / (beta - A)                   in0 = u**, in1 = H
 * piso_face_backward: d_in* and d_p from d_out0 [, d_out1]; NULL d_in1 / d_in2 are skipped.
 * ------------------------------------------------------------------------------------------------------------- */
int piso_pad_velocity(const float* vel_flat, float* vel_pad, int nx, int ny, int periodic_x, int periodic_y, piso_stream_t stream);
int piso_a0_vfirst(const float* a_flat, float* a0_vfirst, int nx, int ny, float beta, float dx_factor, piso_stream_t stream);
int piso_face_forward(int mode, int nx, int ny, const int* pad_modes, float dxdy, float hx, float hy, float beta, const float* p,
                      const float* accessible, const float* a_flat, const float* in0, const float* in1, const float* in2,
                      const uint8_t* dirichlet, float* out0, float* out1, piso_stream_t stream);
int piso_face_backward(int mode, int nx, int ny, const int* pad_modes, float dxdy, float hx, float hy, float beta,
                       const float* accessible, const float* a_flat, const uint8_t* dirichlet, const float* d_out0,
                       const float* d_out1, float* d_in0, float* d_in1, float* d_in2, float* d_p, piso_stream_t stream);
int piso_divergence(const float* faces, float* div, int nx, int ny, float dxdy, float hx, float hy, piso_stream_t stream);
int piso_divergence_adjoint(const float* d_div, float* d_faces, int nx, int ny, int periodic_x, int periodic_y, float dxdy, float hx,
                            float hy, piso_stream_t stream);
/* h = m_delta - (A - beta) delta ; h_over_bma = h / (beta - A)   (piso_helpers.py:223, piso_tf.py:66) and its reverse mode:
 * d_m_delta = d_h + d_h_over_bma / (beta - A) ; d_delta = -(A - beta) d_m_delta   (d_h may be NULL) */
int piso_h_contribution(const float* m_delta, const float* delta, const float* a_flat, float beta, float* h, float* h_over_bma, int nx,
                        int ny, piso_stream_t stream);
int piso_h_contribution_adjoint(const float* d_h, const float* d_h_over_bma, const float* a_flat, float beta, float* d_m_delta,
                                float* d_delta, int nx, int ny, piso_stream_t stream);
/* the same on one rank's rows (piso_slab_t: what the arrays hold, which rows a launch writes) */
int piso_pad_velocity_slab(const float* vel_flat, float* vel_pad, int nx, int ny, int periodic_x, int periodic_y, piso_stream_t stream,
                           const piso_slab_t* slab);
int piso_a0_vfirst_slab(const float* a_flat, float* a0_vfirst, int nx, int ny, float beta, float dx_factor, piso_stream_t stream,
                        const piso_slab_t* slab);
int piso_face_forward_slab(int mode, int nx, int ny, const int* pad_modes, float dxdy, float hx, float hy, float beta, const float* p,
                           const float* accessible, const float* a_flat, const float* in0, const float* in1, const float* in2,
                           const uint8_t* dirichlet, float* out0, float* out1, piso_stream_t stream, const piso_slab_t* slab);
int piso_face_backward_slab(int mode, int nx, int ny, const int* pad_modes, float dxdy, float hx, float hy, float beta,
                            const float* accessible, const float* a_flat, const uint8_t* dirichlet, const float* d_out0,
                            const float* d_out1, float* d_in0, float* d_in1, float* d_in2, float* d_p, piso_stream_t stream,
                            const piso_slab_t* slab);
int piso_divergence_slab(const float* faces, float* div, int nx, int ny, float dxdy, float hx, float hy, piso_stream_t stream,
                         const piso_slab_t* slab);
int piso_divergence_adjoint_slab(const float* d_div, float* d_faces, int nx, int ny, int periodic_x, int periodic_y, float dxdy, float hx,
                                 float hy, piso_stream_t stream, const piso_slab_t* slab);
int piso_h_contribution_slab(const float* m_delta, const float* delta, const float* a_flat, float beta, float* h, float* h_over_bma,
                             int nx, int ny, piso_stream_t stream, const piso_slab_t* slab);
int piso_h_contribution_adjoint_slab(const float* d_h, const float* d_h_over_bma, const float* a_flat, float beta, float* d_m_delta,
                                     float* d_delta, int nx, int ny, piso_stream_t stream, const piso_slab_t* slab);

/* ---------------------------------------------------------------------------------------------------------------
 * Coupling of the CNN closure to the step (csrc/closure_glue.hip): what diffpiso/closure.py does with torch ops - network_input
 * (velocity.at_centers() [+ centered_gradient(pressure)]) and centered_to_staggered - forward and reverse mode.  float32, one thread per
 * OUTPUT element gathering its inputs (the adjoints as well: no atomics).
 *   faces      flat u-first face vector          pressure   cells [ny][nx]
 *   nn_in      NHWC [rows][nx][channels], channels 2 (v, u at the centres) or 4 (+ d/dy, d/dx of the pressure: central differences of the
 *              pressure padded by one cell with pad_modes = {x lower, x upper, y lower, y upper}, 0 zeros | 1 edge value | 2 periodic -
 *              both sides of a periodic axis periodic -, times (float)(1.0 / two_dx), the reciprocal of the double rounded to float32
 *              once: what torch's device kernel makes of centered_gradient's "/ (2 dx)", bit for bit; channels 2: pressure, pad_modes,
 *              two_dx are not read)
 *   nn_out     NHWC [rows][nx][2] -> faces: the mean of the two cells of a face; at a border the edge cell twice, on a wrapped axis
 *              (wrap_x / wrap_y) the cell across the seam, the duplicate face as well
 * The *_adjoint entries take the cotangent of the forward entry's output and write the cotangents of its inputs (d_pressure may be NULL
 * with 2 channels).
 * Slab twins: faces / cells are the rank's stored rows (piso_slab_t); an NHWC buffer holds the whole-grid rows
 * [row_begin - ext_lo, row_end + ext_hi) around the ring of ny rows (the halo rows of the network's receptive field plus the row the
 * resampling reads across the cut; 0 on a side that ends at a border, where the network's own zero padding acts).  A launch writes the
 * OWNED rows of its outputs and reads the rows around them, which the caller fills (piso_comm_exchange); a launch that would read an NHWC
 * row the extended rows do not hold is refused with PISO_ERR_INVALID_ARG.  Boundary rules are decided on the whole grid's (i, j).
 * piso_closure_halo_add: dst[k] += src[k], k < n - rows a reverse exchange delivered, added into their owner's edge rows. */
int piso_closure_input(const float* faces, const float* pressure, float* nn_in, int nx, int ny, int channels, const int* pad_modes,
                       double two_dx, piso_stream_t stream);
int piso_closure_input_adjoint(const float* d_nn_in, float* d_faces, float* d_pressure, int nx, int ny, int channels, const int* pad_modes,
                               double two_dx, piso_stream_t stream);
int piso_closure_force(const float* nn_out, float* faces, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream);
int piso_closure_force_adjoint(const float* d_faces, float* d_nn_out, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream);
int piso_closure_input_slab(const float* faces, const float* pressure, float* nn_in, int nx, int ny, int channels, const int* pad_modes,
                            double two_dx, piso_stream_t stream, const piso_slab_t* slab, int ext_lo, int ext_hi);
int piso_closure_input_adjoint_slab(const float* d_nn_in, float* d_faces, float* d_pressure, int nx, int ny, int channels,
                                    const int* pad_modes, double two_dx, piso_stream_t stream, const piso_slab_t* slab, int ext_lo,
                                    int ext_hi);
int piso_closure_force_slab(const float* nn_out, float* faces, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream,
                            const piso_slab_t* slab, int ext_lo, int ext_hi);
int piso_closure_force_adjoint_slab(const float* d_faces, float* d_nn_out, int nx, int ny, int wrap_x, int wrap_y, piso_stream_t stream,
                                    const piso_slab_t* slab, int ext_lo, int ext_hi);
int piso_closure_halo_add(float* dst, const float* src, size_t n, piso_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Pressure matrix.  Replaces LaplaceMatrixKernelLauncher (CUDAsrc/pressure_solve_op.cc:78-84,
 * CUDAsrc/laplace_op.cu.cc:79-239).
 * ------------------------------------------------------------------------------------------------------------- */
int piso_laplace_matrix_f64(int nx, int ny, const float* active, const float* fluid, const float* a0_vfirst,
                            double* laplace, piso_stream_t stream);
int piso_laplace_matrix_f32(int nx, int ny, const float* active, const float* fluid, const float* a0_vfirst,
                            float* laplace, piso_stream_t stream);
/* one rank's OWNED rows: laplace [(row_end - row_begin) nx][5], masks and a0_vfirst as piso_slab_t stores them */
int piso_laplace_matrix_f64_slab(int nx, int ny, const float* active, const float* fluid, const float* a0_vfirst,
                                 double* laplace, piso_stream_t stream, const piso_slab_t* slab);
int piso_laplace_matrix_f32_slab(int nx, int ny, const float* active, const float* fluid, const float* a0_vfirst,
                                 float* laplace, piso_stream_t stream, const piso_slab_t* slab);

/* ---------------------------------------------------------------------------------------------------------------
 * Pressure CG.  Replaces LaunchPressureKernel (CUDAsrc/pressure_solve_op.cc:48-76,
 * CUDAsrc/pressure_solve_op.cu.cc:140-418 double / :420-696 float): plain CG on (L + c 1 1^T) x = b from x0 = 0,
 * c = 0.1*mean|diag L| if rank_deficient, p/r re-initialised every residual_reset iterations, max-norm stop tested
 * every 5th iteration with the reference's flag semantics.
 *   laplace [N][5], divergence [N], x_out [N]; iterations_out: host int* (also the reference's `iterations` output)
 * The call returns when the solve has finished (the host must see the convergence flag, as in the reference).
 * Grids whose rows are a multiple of 128 cells (fp64; 256 for fp32) and that fit the chip run the iterations inside
 * persistent launches (csrc/cg_persist1.h); a grid-wide exchange that times out fails the call with
 * PISO_ERR_HIP.  Tuning / test knobs: piso_set_option() above.
 * ------------------------------------------------------------------------------------------------------------- */
size_t piso_cg_workspace_bytes(int nx, int ny, int elem_size);

int piso_cg_solve_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                      double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                      int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_cg_solve_f32(int nx, int ny, int periodic_x, int periodic_y, const float* laplace, const float* divergence,
                      float* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                      int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);

/* The same solve WITHOUT a host round trip, where the library can run it in one launch (today: grids of at most 4 608 cells,
 * csrc/cg_tiny.h - the lid-driven cavity of lid_driven_cavity_2d.py): the call returns as soon as the kernel is queued and the
 * iteration count (the reference's `iterations` output tensor, pressure_solve_op.cc:60-76) is written to DEVICE memory.
 * Any other grid: PISO_ERR_NEEDS_HOST and nothing has been queued - call piso_cg_solve_*. */
int piso_cg_solve_async_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                            double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                            int* iterations_dev, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_cg_solve_async_f32(int nx, int ny, int periodic_x, int periodic_y, const float* laplace, const float* divergence,
                            float* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                            int* iterations_dev, void* workspace, size_t workspace_bytes, piso_stream_t stream);

/* Fixed-work variant for bandwidth measurements: runs exactly `iterations` CG iterations (no convergence test),
 * optionally timing the kernels with HIP events on `stream`; kernel_ms_out (NULL to skip): host float[2] = average ms per
 * launch of K1 (fused p-update + stencil + dots) and K2 (x/r update + dots), or, when the iterations ran inside persistent
 * launches, {average ms per ITERATION, 0}. */
int piso_cg_fixed_iterations_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace,
                                 const double* divergence, double* x_out, int rank_deficient, int iterations,
                                 float* kernel_ms_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);

/* Sampling of K1 / K2 launch durations with HIP events on the launch stream (every `stride`-th iteration); used by
 * bench.py for roofline.achieved.  ms_sum / count: host arrays of FOUR entries: [0] K1 launches, [1] K2 launches,
 * [2] persistent segments (ms_sum[2] = total duration of all segment launches, count[2] = CG ITERATIONS executed inside
 * them), [3] count[3] = number of segment launches (ms_sum[3] unused). */
void piso_cg_profile_enable(int enable, int stride);
void piso_cg_profile_read(double* ms_sum, long long* count);
/* Solves (since load) that were restarted on the two-kernel path because a grid-wide exchange of the persistent kernel timed
 * out (workgroups not co-resident: CU mask, another process on the GPU).  0 on a dedicated GPU. */
int piso_cg_persist_fallbacks(void);
/* With option "cg_xcd_map" = 1: the XCD (0-7) that every workgroup of the calling thread's last solve's LAST chip-wide persistent launch
 * ran on, out[0 .. min(return value, capacity)); returns the number of workgroups (0: the solve ran no such launch).  The exchange adds
 * an XCD's records in workgroup order, so two solves of the same input are bit-for-bit equal whenever the hardware dealt the workgroups
 * to the XCDs the same way - which it does on an otherwise idle GPU; the reproducibility tests check exactly that precondition. */
int piso_cg_last_xcd_map(int* out, int capacity);
/* Solves of grids of at most 4 608 cells run inside ONE workgroup, one launch for the whole solve (csrc/cg_tiny.h: the lid-driven
 * cavity of BASELINE.json's config 1); same iteration and control flow as the chip-wide paths.  Option "cg_tiny": 0 = never. */
long long piso_cg_tiny_solves(void);
/* Which kernel instance the calling thread's last piso_cg_solve_* / piso_cg_solve_async_* / piso_cg_fixed_iterations_* was dispatched
 * to: out[0 .. min(return value, capacity)); returns the number of fields (0: this thread has not solved, or its last call was refused
 * before it chose).  Read-only: the record is written on the host while the solve is set up and changes nothing that is computed.
 * Fields, in this order (a field that does not apply to the path is 0):
 *    0 path           0 cg_tiny, 1 cg_tiny_cols (one workgroup, cg_tiny.h), 2 the two-kernel iteration cg_k1 + cg_k2 only,
 *                     3 persistent segments (cg_persist1) with the two-kernel pair for iteration 0 and every reset iteration
 *    1 sizeof(T)      state type: 8 / 4
 *    2 sizeof(CT)     type the off-diagonals are stored in: 4 when every one of them is exactly a float, else sizeof(T)
 *    3 V              cells per lane of cg_k1 / cg_k2: 16 / sizeof(T) (rows a multiple of it, b and x 16-byte aligned) or 1
 *    4 RECON          1: the diagonal is rebuilt from the off-diagonals instead of read
 *    5 symmetric      1: the matrix passed the bit-for-bit symmetry check (and option cg_no_sym is off)
 *    6 rows_per_wave  rows every wave of cg_k1 walks per tile (2 .. 16; option cg_rpw)
 *    7 k1_grid        workgroups of cg_k1 (at most 1 024, option cg_maxblocks; rounded down to a multiple of 8 from 8 on)
 *    8 k1_tiles       tiles of cg_k1 (column strips x groups of 4 * rows_per_wave rows): more than k1_grid -> some blocks walk several
 *    9 R             persistent kernel: rows per region (2 / 4 / 16)
 *   10 NQ             ... regions per working wave (1 / 2)
 *   11 waves          ... working waves per workgroup (8, or 4: "half" workgroups, option cg_persist_half)
 *   12 launch_grid    ... workgroups launched (XCD-local: 8 x the workgroups that work)
 *   13 padded         1: a wall-bounded grid embedded in a larger one the persistent kernel can tile (option cg_pad)
 *   14 xcd_local      1: the persistent solve runs on the workgroups of one XCD (option cg_xcd_local)
 *   15 fell_back      1: the solve was restarted on the two-kernel path (exchange timed out / verification failed); path is then 2
 *   16 tiny_per_x     cg_tiny_cols: 1 the periodic-x instance, 0 the wall-bounded one
 *   17 k2_grid        workgroups of cg_k2
 *   18 segments       persistent launches the solve made (0 with path 3: it ended before the first segment) */
int piso_cg_last_dispatch(int* out, int capacity);
/* Every fp64 solve that ran iterations inside the persistent kernel is VERIFIED before it returns: the recurrence residual r must
 * equal b - (L x + c sum x) for the returned x to 1e-5 max|b| (one extra stencil pass).  The persistent kernel publishes perimeter
 * rows without release / acquire fences; a value read before it was visible would break exactly this identity.  A failed check
 * restarts the solve on the two-kernel iteration and is counted here (and in piso_cg_persist_fallbacks).  Option "cg_verify": 0
 * skips the check, 2 treats every check as failed (test knob). */
void piso_cg_verify_stats(long long* runs_out, int* failures_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Multigrid-preconditioned CG for the pressure system (csrc/mg.hip; fp64; opt-in - the reference has no such solver, and
 * piso_cg_solve_* stays what every default path calls).  Solves the system piso_cg_solve_f64 solves, (L + c 1 1^T) x = b with
 * c = 0.1 mean|diag L| when rank_deficient, from x0 = 0, and stops when max|r| < accuracy on the recurred residual, tested on the
 * device after EVERY iteration; the true residual is recomputed every residual_reset iterations.  Preconditioner: one V(sweeps,
 * sweeps) cycle of damped Jacobi on a hierarchy of 2 x 2 aggregates, A_c = 1/2 P^T A P, rebuilt from `laplace` in every call.
 * A cell with a zero diagonal is absent (x = 0 there).  Iteration counts are tens where plain CG needs thousands, independent of the
 * polling cadence, and a solve is reproducible bit for bit.  NaN input never counts as converged: max_iterations, NaN in x.
 * Refused with PISO_ERR_UNSUPPORTED_PATTERN: a non-zero border entry in a non-periodic direction, a zero-diagonal row with entries,
 * rank_deficient = 1 on a matrix whose rows do not sum to zero.  nx, ny >= 4; workspace too small: PISO_ERR_INVALID_ARG.
 * Precondition (not checked): the cells with a non-zero diagonal are connected through their couplings.  With a pocket of fluid enclosed
 * by solid cells the solve does not converge: it returns max_iterations and a finite x (the plain CG does not solve that system either).
 * Options: "mg_tail" 0 runs the coarse levels as launches of their own instead of inside one workgroup (same result),
 * "mg_check_every" sets the iterations queued between two host looks (default 4; same result and count). */
size_t piso_mg_workspace_bytes(int nx, int ny);
int piso_mg_pcg_solve_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                          double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                          int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* test / measurement entries.  z_out = M^-1 r_in: one cycle, an approximation of L^-1 r_in (symmetric, negative definite on the
 * present cells).  piso_mg_level_f64 copies the operator of `level` out as [nx_out * ny_out][5] (laplace_level_out NULL: sizes only;
 * level 0 is `laplace` with couplings into absent cells dropped). */
int piso_mg_vcycle_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out,
                       int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_level_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out, int* ny_out,
                      double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* The float32 cycle (csrc/mg_f32.h; opt-in): the same PCG in float64 - x, r, p, q, the level-0 operator of q = L p and of the residual
 * recomputation, alpha, beta, every sum, the stopping rule, the constant mode - around a V-cycle whose hierarchy and vectors are stored and
 * computed in float32.  Level 0 is fl32 of the fp64 set-up's arrays, level l + 1 is fl32(1/2 P^T A_l P) accumulated in double from the
 * float32 entries of level l and rounded once, the Jacobi weight is fl32(0.8 / (double)diag32); the cycle reads fl32(r) and returns a
 * float32 z, which the direction kernel widens; the (r, z) partials are accumulated in double from the double r and the float z.  r is
 * not scaled: a residual beyond float32's range turns Inf / NaN in the cycle and never counts as converged, and an accuracy below about
 * 1e-30 is outside this mode.  Iteration counts are those of the fp64 cycle or a few more.  The entries take the arguments
 * of their fp64 namesakes, refuse what they refuse with the same status (the pattern checks run on the double matrix), want a workspace
 * of piso_mg_workspace_bytes_cycle(nx, ny, 4) bytes (cycle_elem_size 8: piso_mg_workspace_bytes; anything else: 0) and are bitwise
 * reproducible.  piso_mg_vcycle_c32_f64 casts r_in and widens z_out; piso_mg_level_c32_f64 returns the float32 entries widened.
 * Option "mg_f32_vec" 0 runs the one-cell-per-thread kernels on every level instead of the four-cell kernels (levels with nx % 4 == 0
 * above the tail): the same z bit for bit, a solve equal to round-off (the (r, z) partials are grouped by other threads). */
size_t piso_mg_workspace_bytes_cycle(int nx, int ny, int cycle_elem_size);
int piso_mg_pcg_solve_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                              double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset,
                              int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_vcycle_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out,
                           int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_level_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out, int* ny_out,
                          double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* A PREPARED hierarchy (csrc/mg_prepared.h): set-up once, any number of solves of the same matrix.  piso_mg_prepare_* runs the set-up of
 * piso_mg_pcg_solve_* into `hierarchy`, a buffer of piso_mg_hierarchy_bytes(nx, ny, cycle_elem_size) bytes the caller owns and keeps (the
 * five coefficient arrays and the Jacobi weights of every level - for the float32 cycle the fp64 level 0 and the float32 levels - and the
 * sums the constant mode needs), makes the one host look with the three PISO_ERR_UNSUPPORTED_PATTERN refusals, and on success seals the
 * buffer with a device-side header (nx, ny, the periodic flags, the cycle's element size, rank_deficient), written last: a refused or failed
 * prepare leaves no valid header.  piso_mg_pcg_solve_prepared_* / piso_mg_vcycle_prepared_* take the arguments of piso_mg_pcg_solve_* /
 * piso_mg_vcycle_* with (hierarchy, hierarchy_bytes) in place of `laplace` and a scratch workspace of piso_mg_solve_workspace_bytes(nx, ny,
 * cycle_elem_size) bytes (every call may use another one; prepare takes one too), make no host look before the first iteration and return
 * x, the count and the piso_mg_last_dispatch record of the ordinary call bit for bit.  Their first kernel compares the header with the
 * call's arguments; a mismatch ends the solve on the device and is reported at the first regular look: PISO_ERR_INVALID_ARG, "not a
 * hierarchy prepared for this grid" (a cycle runs on a hierarchy prepared with either rank_deficient).  Buffers below the two sizes are
 * refused on the host.  Both size functions return 0 where piso_mg_workspace_bytes_cycle does.  The caller must not change the matrix's
 * hierarchy behind the library's back: the buffer is only read by a solve, so solves on it may follow each other on one stream. */
size_t piso_mg_hierarchy_bytes(int nx, int ny, int cycle_elem_size);
size_t piso_mg_solve_workspace_bytes(int nx, int ny, int cycle_elem_size);
int piso_mg_prepare_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int rank_deficient, void* hierarchy,
                        size_t hierarchy_bytes, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_prepared_f64(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,
                                   const double* divergence, double* x_out, float accuracy, int max_iterations, int rank_deficient,
                                   int residual_reset, int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes,
                                   piso_stream_t stream);
int piso_mg_vcycle_prepared_f64(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes, const double* r_in,
                                double* z_out, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_prepare_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int rank_deficient, void* hierarchy,
                            size_t hierarchy_bytes, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_prepared_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,
                                       const double* divergence, double* x_out, float accuracy, int max_iterations, int rank_deficient,
                                       int residual_reset, int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes,
                                       piso_stream_t stream);
int piso_mg_vcycle_prepared_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,
                                    const double* r_in, double* z_out, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* The same solver on y-slabs (csrc/mg_slab.h, csrc/mg_slab_plan.h): every rank owns ny_local = ny / world contiguous rows and passes its
 * rows of laplace / divergence / x, otherwise the arguments of piso_mg_pcg_solve_f64.  Levels 0 .. g - 1 are sharded (a rank's rows
 * plus one halo row below and above), level g - the first of at most 8192 cells, or of at most "mg_slab_gather_cells" cells where that
 * option is positive and smaller - and everything coarser is replicated: the ranks' rows of level g are all-gathered and every rank
 * runs the coarse levels itself.  Refused with PISO_ERR_INVALID_ARG before any launch: ny_local not divisible by 2^g, no level within
 * the limit (the message states the rule and names the plain solver), a workspace below piso_mg_slab_workspace_bytes(nx, ny_local,
 * world, 1).  Halo rows, sums and gathers go through the communicator's collectives (either transport); every sum is formed from
 * per-rank fixed-order partials, so every rank takes the same decisions, reports the same count and the same status.  Against the
 * one-GPU solver the hierarchy and a cycle are bit for bit the same, a solve differs by the grouping of its dot products only.
 * The *_emulated entries run `slabs` virtual ranks on one device over the full arrays (their rows are copied, no communicator): the test
 * harness of every cut; their workspace is piso_mg_slab_workspace_bytes(nx, ny / slabs, slabs, slabs).
 * piso_mg_level_slab_f64: a rank's rows of a sharded level, or the whole replicated level, as [nx_out * rows_out][5].
 * piso_mg_slab_plan: the pure plan as a flat int record {status (0 accepted), levels, g, tail_first, rows per rank of level 0, ranks,
 * then nx, ny, rows held per rank for every level}; gather_cells <= 0: the option / 8192; returns the number of fields (6 when refused,
 * with the reason in piso_last_error_string). */
size_t piso_mg_slab_workspace_bytes(int nx, int ny_local, int world, int local_ranks);
int piso_mg_slab_plan(int nx, int ny, int world, int gather_cells, int* out, int capacity);
int piso_mg_pcg_solve_slab_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local,
                               const double* divergence_local, double* x_out_local, float accuracy, int max_iterations, int rank_deficient,
                               int residual_reset, int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_vcycle_slab_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, const double* r_local,
                            double* z_local, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_level_slab_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, int level, int* nx_out,
                           int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_slab_emulated_f64(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                                        double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,
                                        int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_vcycle_slab_emulated_f64(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in, double* z_out,
                                     int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_level_slab_emulated_f64(int slabs, int rank, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level, int* nx_out,
                                    int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* The float32 cycle on y-slabs (csrc/mg_slab_f32.h): the _c32_f64 twins of the six slab entries take the arguments of their _f64 namesakes and
 * run the float32 cycle of piso_mg_*_c32_f64 on the same plan - the outer iteration stays fp64 and sharded, the sharded levels hold the
 * rank's float rows with halo rows, the rank's float rows of level g are all-gathered and levels g .. coarsest run replicated in
 * float32.  The collectives per iteration are the fp64 plan's in number; the halo rows and the gather carry half the bytes.  Against the
 * one-GPU float32 cycle the hierarchy and a cycle are bit for bit the same.  One more refusal (PISO_ERR_INVALID_ARG): a plan with g = 0 -
 * the whole grid within the gather limit, the cycle replicated altogether - has nothing to gain from float32 and wants the _f64 entries.
 * piso_mg_slab_workspace_bytes_cycle: the workspace for cycle_elem_size 4 or 8 (8: piso_mg_slab_workspace_bytes; anything else, a refused
 * plan, or g = 0 with 4: 0). */
size_t piso_mg_slab_workspace_bytes_cycle(int nx, int ny_local, int world, int local_ranks, int cycle_elem_size);
int piso_mg_pcg_solve_slab_c32_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local,
                                   const double* divergence_local, double* x_out_local, float accuracy, int max_iterations, int rank_deficient,
                                   int residual_reset, int sweeps, int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_vcycle_slab_c32_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, const double* r_local,
                                double* z_local, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_level_slab_c32_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local, int level, int* nx_out,
                               int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_slab_emulated_c32_f64(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence,
                                            double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,
                                            int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_vcycle_slab_emulated_c32_f64(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* r_in,
                                         double* z_out, int sweeps, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_level_slab_emulated_c32_f64(int slabs, int rank, int nx, int ny, int periodic_x, int periodic_y, const double* laplace, int level,
                                        int* nx_out, int* rows_out, double* laplace_level_out, void* workspace, size_t workspace_bytes,
                                        piso_stream_t stream);
/* Starting from a GUESS (csrc/mg_guess.h; opt-in, one GPU).  The four *_guess_* entries take the arguments of their namesakes plus
 * `x0` after `divergence`: nx * ny doubles, the same pointer as x_out or disjoint from it.  x0 NULL is the namesake's call.  Otherwise, with
 * b' the right-hand side the iteration sees (zero on absent cells, its mean over the present cells removed where rank_deficient) and x0~ =
 * x0 on the present cells, 0 elsewhere (x0 is not read for its values on absent cells), the device forms r_g = b' - L x0~ and ACCEPTS the
 * guess iff max|r_g| < max|b'| (strict; false for a NaN or Inf in r_g and for x0 = 0): the solve then starts from x = x0~, r = r_g, and is
 * done with 0 iterations where max|r_g| < accuracy already.  A REJECTED guess starts from x = 0, r = b': the namesake's x, count and
 * piso_mg_last_dispatch record bit for bit (a solve without an accepted guess always runs at least one iteration).  The guard is there
 * because the previous time step's solution is a worse start than zero in a start-up transient - its residual then exceeds the right-hand
 * side.  The iteration, its stopping rule and the constant mode are untouched (the end of a rank-deficient solve replaces
 * the mean of x, so the mean of x0 is immaterial); workspace sizes are those of the namesakes; the cost is two more small launches.
 * Adjoint solves and the slab entries take no guess.
 * piso_mg_last_guess: what the calling thread's last piso_mg_pcg_solve* call (slab entries included) did with its guess - 0 none given, 1
 * accepted, 2 rejected; reset to 0 when such a call begins and filled when its solve returns, so a refused or failed call reports 0. */
int piso_mg_pcg_solve_guess_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence, const double* x0,
                                double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,
                                int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_guess_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const double* laplace, const double* divergence, const double* x0,
                                    double* x_out, float accuracy, int max_iterations, int rank_deficient, int residual_reset, int sweeps,
                                    int* iterations_out, void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_prepared_guess_f64(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,
                                         const double* divergence, const double* x0, double* x_out, float accuracy, int max_iterations,
                                         int rank_deficient, int residual_reset, int sweeps, int* iterations_out, void* workspace,
                                         size_t workspace_bytes, piso_stream_t stream);
int piso_mg_pcg_solve_prepared_guess_c32_f64(int nx, int ny, int periodic_x, int periodic_y, const void* hierarchy, size_t hierarchy_bytes,
                                             const double* divergence, const double* x0, double* x_out, float accuracy, int max_iterations,
                                             int rank_deficient, int residual_reset, int sweeps, int* iterations_out, void* workspace,
                                             size_t workspace_bytes, piso_stream_t stream);
int piso_mg_last_guess(void);
/* What the calling thread's last multigrid solve / cycle ran (fp64, float32 cycle or slab); returns the number of fields (8):
 *    0 levels         levels of the hierarchy
 *    1 tail_first     first level that ran inside the one-workgroup tail kernel (-1: none)
 *    2 sweeps
 *    3 iterations     0 after piso_mg_vcycle_f64
 *    4 cycles         V-cycles that contributed to the result
 *    5 residual_recomputations
 *    6 cycle_elem     bytes of a value of the cycle: 8, or 4 after a piso_mg_*_c32_f64 entry
 *    7 vec_mask       bit l set where level l ran the four-cell float32 kernels (0 for the fp64 paths) */
int piso_mg_last_dispatch(int* out, int capacity);

/* ---------------------------------------------------------------------------------------------------------------
 * Convolutions of the CNN turbulence closure on the matrix cores (csrc/conv.hip; exact fp32 MFMA).  Replaces the
 * tf.nn.conv2d / tf.nn.leaky_relu calls of diffpiso/networks.py:3-57 (NHWC activations, batch 1, stride 1, no bias, kernel
 * sizes and channel counts of the closure: 7x7 4->16, 5x5 16->16, 5x5 16->32, 3x3 32->64, 3x3 64->64, 1x1 64->64, 1x1 64->2 and
 * the transposed shapes of the input-gradient pass; every other odd kernel size up to 9 and channel count up to 256: the *_any entries below).
 *   in [H][W][cin], out [Ho][Wo][cout] with Ho = H + 2 pad - ks + 1; leaky_out != 0: leaky ReLU (slope 0.2) on the output.
 *   w_laid_out: the HWIO weights in the kernel's operand layout, zero filled beyond the true channel counts
 *   (piso_conv2d_weight_elems floats, COUTP = round_up(cout, 16)):
 *     cin <= 4: [ks][ks][4][COUTP];   cin > 4 (a multiple of 16): [ks][ks][cin/16][4][COUTP][4] with
 *     element [tap][blk][q][co][j] = W[tap][16 blk + 4 q + j][co]   (every MFMA operand is then one 16-byte load).
 * Input gradient = piso_conv2d_forward(grad of the pre-activation output, flipped + transposed weights, pad = ks - 1 - pad).
 * piso_conv2d_wgrad: dw [ks][ks][cin][cout] (HWIO, true sizes) = sum over pixels of in (x) grad_out (pre-activation);
 * deterministic two-stage reduction through the caller's workspace.
 * Alignment (checked, PISO_ERR_INVALID_ARG): forward with cin > 4: `in` and `w_laid_out` 16-byte aligned;  wgrad with cout % 4 == 0:
 * `dw` and `workspace`, with cin % 4 == 0 as well: `in` and `grad_out` too (the kernels use 16-byte accesses there).
 * Non-finite values stay where the definition puts them: an output (a weight gradient) is NaN exactly if a term of ITS sum is.
 * ------------------------------------------------------------------------------------------------------------- */
size_t piso_conv2d_weight_elems(int ks, int cin, int cout);
size_t piso_conv2d_wgrad_workspace_bytes(int ks, int cin, int cout);
int piso_conv2d_forward(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad,
                        int leaky_out, piso_stream_t stream);
int piso_conv2d_wgrad(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad,
                      void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* grad_pre = grad_out * leaky_relu'(pre-activation) (slope 0.2), from the layer's saved output (same sign as the pre-activation). */
int piso_leaky_relu_backward(const float* grad_out, const float* out, float* grad_pre, size_t n, piso_stream_t stream);
/* Which kernel instance the calling thread's last piso_conv2d_forward / piso_conv2d_wgrad ran: out[0 .. min(return value, capacity));
 * returns the number of fields (0: this thread has not run a convolution).  Read-only: the record is written on the host after the
 * launches of a call succeeded and changes nothing that is computed; a refused call (PISO_ERR_INVALID_ARG) leaves it as it was.
 * Fields, in this order:
 *    0 entry           1 piso_conv2d_forward, 2 piso_conv2d_wgrad
 *    1 KS              kernel size of the instance
 *    2 C               forward: CINP, the input channels of the instance (4 for cin <= 4, else cin);  wgrad: MTI, tiles of 16 input channels
 *    3 NT              tiles of 16 output channels
 *    4 IPW             wgrad: work items (tap, tile of input channels) per wave (the 64 -> 64 kernels: 1, one tap);  forward: 0
 *    5 family          forward: 0 conv_forward_kernel (operands from L2), 1 conv_forward_lds_kernel;  wgrad: 2 conv_wgrad_kernel, 3
 *                      conv_wgrad_lds_kernel (cin % 4 == 0 and cout % 4 == 0), 4 conv_wgrad_kernel PACK4 (7 x 7, cin <= 4, cout <= 16), 5
 *                      conv_wgrad64_kernel (3 x 3, 64 -> 64), 6 conv_wgrad64_lds_kernel.  Option conv_lds 0: never 1, 3 or 6
 *    6 leaky           forward: 1 the instance applies the leaky ReLU;  wgrad: 0
 *    7 grid_x          forward: workgroups of four 64-pixel tiles, ceil(ceil(Wo / 64) Ho / 4);  wgrad: nblocks
 *    8 grid_y          wgrad: groups of waves over the work items (the 64 -> 64 kernels: 3, one per tap row);  forward: 1
 *    9 block           threads per workgroup: 256 (the 64 -> 64 wgrad kernels: 192)
 *   10 rows_per_block  wgrad: output rows per row band, ceil(Ho / 256);  forward: 0
 *   11 nblocks         wgrad: row bands = partial sums per weight, ceil(Ho / rows_per_block) <= 256;  forward: 0
 *   12 reducer         wgrad: 4 conv_wgrad_reduce4_kernel (cout % 4 == 0), 1 conv_wgrad_reduce_kernel;  forward: 0
 *   13 Ho              output rows (wgrad: rows of grad_out)
 *   14 Wo              output columns */
int piso_conv_last_dispatch(int* out, int capacity);

/* The same convolutions with a GENERAL GEOMETRY: padding per axis (pad_y, pad_x) and wrap-around per axis (wrap_y, wrap_x != 0: the axis is
 * periodic) - the closure on a periodic domain sees cell n - 1 and cell 0 as the neighbours they are.  Definition:
 *     out[y][x][co] = sum over (ky, kx, ci) of in[Y][X][ci] w[ky][kx][ci][co],   Y = y + ky - pad_y,  X = x + kx - pad_x
 *   on an axis that is not wrapped a coordinate outside the image contributes nothing (zero padding, as above); on a wrapped axis it is taken
 *   modulo the extent.  Output extents as above: Ho = H + 2 pad_y - ks + 1, Wo = W + 2 pad_x - ks + 1.
 *   piso_conv2d_wgrad_ex: dw[ky][kx][ci][co] = sum over output pixels (y, x) of in[Y][X][ci] grad_out[y][x][co], Y and X as above.
 * Two rules for a wrapped axis (checked, PISO_ERR_INVALID_ARG, the message states the rule):
 *   - its pad is ks / 2: the axis keeps its extent, and the adjoint is again such a convolution - the input gradient is
 *     piso_conv2d_forward_ex(grad of the pre-activation output, flipped + transposed weights, pad' = ks - 1 - pad per axis, the same wrap);
 *   - its extent is at least its pad: an index wraps at most once (one conditional add or subtract in the kernels, no division).
 * Weight layout, alignment rules, workspace size, the refusals and the treatment of non-finite values are those of the entries above; the kernel
 * instance is chosen by the same rules (option conv_lds included) and piso_conv_last_dispatch reports it with the same 15 fields (entry 1 for
 * piso_conv2d_forward_ex, 2 for piso_conv2d_wgrad_ex: the *_ex_kernel twin of the instance named there).  The order of the terms of every sum
 * is the instance's: with wrap (0, 0) and pad_y == pad_x the results are those of the entries above bit for bit, and with both axes wrapped
 * every output pixel adds the same sequence of terms (the result of a circularly shifted input is the shifted result, bit for bit). */
int piso_conv2d_forward_ex(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,
                           int wrap_y, int wrap_x, int leaky_out, piso_stream_t stream);
int piso_conv2d_wgrad_ex(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,
                         int wrap_y, int wrap_x, void* workspace, size_t workspace_bytes, piso_stream_t stream);
/* The geometry of the calling thread's last convolution, written with the dispatch record: out[0 .. min(return value, capacity)) = pad_y,
 * pad_x, wrap_y (0 | 1), wrap_x (0 | 1); returns the number of fields: 4 after piso_conv2d_forward_ex / piso_conv2d_wgrad_ex, 0 after
 * piso_conv2d_forward / piso_conv2d_wgrad (their one `pad` is an argument of the call) or before any convolution. */
int piso_conv_last_geometry(int* out, int capacity);

/* ANY channel counts and odd kernel sizes: a second kernel family (csrc/conv_any.hip) whose kernel size and channel counts are run-time values, for
 * the shapes the tuned instances above do not hold (they refuse 5 .. 15 input channels, more than 64 channels, 9 x 9, 5 x 5 on 64 -> 64, ...).
 * Definition, geometry (pad per axis, wrap per axis), the two rules of a wrapped axis and the treatment of non-finite values: those of the *_ex
 * entries above.  Accepted: ks odd, 1 .. 9;  1 <= cin, cout <= 256;  Ho, Wo >= 1.  NO alignment rule: every access of the main kernels is 4 bytes
 * (the 4-wide reducer runs only where cout % 4 == 0 AND `dw` and `workspace` are 16-byte aligned; the scalar one adds the same bands in the same
 * order).  Everything else is PISO_ERR_INVALID_ARG before any launch, with a message that starts with the entry's name.
 * These entries ALWAYS run the new family, also for a shape that has a fixed instance (that holds one family to the other in the tests); which
 * shapes the fixed tables serve: piso_conv2d_instantiated(entry, ks, cin, cout) - entry 1 forward, 2 weight gradient; 1 where piso_conv2d_forward /
 * piso_conv2d_wgrad have an instance for the shape, 0 otherwise.  Pure host code: it asks the plan the old entries ask.
 *   w_laid_out of piso_conv2d_forward_any (piso_conv2d_weight_elems_any floats): [ks][ks][CINP4][COUTP], CINP4 = round_up(cin, 4), COUTP =
 *     round_up(cout, 16):  element ((ky ks + kx) CINP4 + ci) COUTP + co = W[ky][kx][ci][co], zero where ci >= cin or co >= cout
 *     (the cin <= 4 layout above with more channel rows).  K order of every output's sum: tap row, tap column, input channel.
 *   workspace of piso_conv2d_wgrad_any: piso_conv2d_wgrad_any_workspace_bytes(ks, cin, cout, Ho) bytes, Ho = H + 2 pad_y - ks + 1: at most 64 row
 *     bands of partials [band][ks][ks][round_up(cin, 16)][COUTP], added in a fixed order (deterministic, no atomics).
 * piso_conv_last_dispatch reports these calls with the same 15 fields: entry 1 / 2, and
 *    2 C               forward: CINP4;  wgrad: tiles of 16 input channels, ceil(cin / 16)
 *    3 NT              tiles of 16 output channels PER GROUP: the ceil(cout / 16) tiles are split evenly over groups = ceil(tiles / 4) groups
 *    4 IPW             wgrad: 1;  forward: 0
 *    5 family          7 conv_forward_any_kernel<NT, leaky>, 8 conv_wgrad_any_kernel<NT>
 *    8 grid_y          forward: the groups;  wgrad: ceil(ks ks C / 4) x groups - workgroups of four waves over the work items (tap, tile of 16
 *                      input channels), one item per wave, times the groups
 *   10 rows_per_block  wgrad: ceil(Ho / 64)
 *   11 nblocks         wgrad: ceil(Ho / rows_per_block) <= 64
 *   12 reducer         wgrad: 4 if cout % 4 == 0 and `dw`, `workspace` are 16-byte aligned, else 1
 * the other fields as above.  piso_conv_last_geometry: always 4 fields.  A refused call leaves both records untouched. */
size_t piso_conv2d_weight_elems_any(int ks, int cin, int cout);
size_t piso_conv2d_wgrad_any_workspace_bytes(int ks, int cin, int cout, int Ho);
int piso_conv2d_instantiated(int entry, int ks, int cin, int cout);
int piso_conv2d_forward_any(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,
                            int wrap_y, int wrap_x, int leaky_out, piso_stream_t stream);
int piso_conv2d_wgrad_any(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,
                          int wrap_y, int wrap_x, void* workspace, size_t workspace_bytes, piso_stream_t stream);

/* The EPILOGUE of a closure layer (csrc/conv_epilogue.hip): bias, skip connection and activation, one pass per direction behind whichever
 * convolution entry above served the layer (called with leaky_out = 0).  Layout: NHWC [pixels][channels] float32, pixels = Ho Wo, bias [channels].
 * act: 0 none, 1 leaky ReLU (slope 0.2: v > 0 ? v : 0.2f v), 2 ReLU (v > 0 ? v : 0).
 *   piso_conv_epilogue_forward:  y[p][c] = act((z[p][c] + bias[c]) + skip[p][c]), fp32, in that order.  bias and skip may each be NULL; y may be z
 *     (in place); skip must not be y.
 *   piso_conv_epilogue_backward: gpre[p][c] = g[p][c] act'(y[p][c]) from the saved OUTPUT y (leaky: y > 0 ? g : 0.2f g; ReLU: y > 0 ? g : 0).  act == 0:
 *     gpre IS g - y and gpre may be NULL and nothing is written to gpre.  dbias non-NULL: dbias[c] = sum over pixels of gpre[p][c], in the same pass
 *     (g is read once).  The cotangent of skip is gpre itself: no kernel and no copy.
 *   Summation order of dbias (deterministic, no atomics): the pixels are cut into `bands` bands of `pixels_per_band` consecutive pixels
 *     (piso_conv_epilogue_plan: pixels_per_band = max(ceil(4096 / channels), ceil(pixels / 1024)), bands = ceil(pixels / pixels_per_band) - a function
 *     of (pixels, channels) alone, never of the card or the launch).  A workgroup adds one band: thread (row, column) the pixels row, row + rows, ...
 *     of its band in index order (rows = 256 / columns; columns = channels, or channels / 4 in the 16-byte form), then the rows of a column in a
 *     fixed tree, and stores ws[band][channels].  A second kernel adds the bands of a channel: band r, r + 64, ... per thread in index order,
 *     then the 64 partial sums in a fixed tree.  The same call gives the same bits on every run and card.
 *   workspace: piso_conv_epilogue_workspace_bytes(pixels, channels) = min(ceil(pixels / ceil(4096 / channels)), 1024) x channels x 4 bytes - bands x
 *     channels x 4 up to 1024 bands, its upper bound beyond (monotone in pixels); ws_elems counts floats.  Needed with dbias only.
 *   Access form: 16 bytes per lane where channels % 4 == 0 and every pointer given is 16-byte aligned, else guarded 4-byte accesses with NO
 *     alignment rule; y and gpre are the same bits in both (a dbias may differ in its last bits between the two forms).
 * Refused with PISO_ERR_INVALID_ARG before any launch, the message naming the rule, and nothing written: z / y / g NULL; channels outside 1 .. 256;
 * pixels < 1; act outside 0 .. 2; y or gpre NULL with act != 0; ws NULL or ws_elems < bands x channels with dbias given; skip == y. */
int piso_conv_epilogue_plan(int pixels, int channels, int* bands, int* pixels_per_band);
size_t piso_conv_epilogue_workspace_bytes(int pixels, int channels);
int piso_conv_epilogue_forward(const float* z, const float* bias, const float* skip, float* y, int pixels, int channels, int act, piso_stream_t stream);
int piso_conv_epilogue_backward(const float* g, const float* y, float* gpre, float* dbias, int pixels, int channels, int act, float* ws, size_t ws_elems,
                                piso_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Slab-decomposed pressure CG (no counterpart in the reference, which is single-GPU).
 * The grid is cut along y into `world` slabs of ny_local rows, one rank (process) per GPU.  Two transports:
 *
 *  PEER (piso_comm_peer_create / _connect, or piso_comm_peer_create_fd / _connect_fd; the GPUs of one node, world <= 8): every rank
 *  owns a peer-mapped MAILBOX (uncached device memory exported with hipIpcGetMemHandle - or as a POSIX file descriptor of a
 *  virtual-memory allocation - and mapped by all ranks).  Step 1 creates the mailbox and returns its 64-byte
 *  handle; the caller distributes the handles of all ranks by any means (torch.distributed all_gather, MPI, a pipe); step 2 maps
 *  them.  Reductions and halo rows are written by kernels straight into the consumers' mailboxes (tagged words / release-acquire
 *  at system scope), never through the host.  The NORMAL iterations run inside the persistent kernel: the slab's r, p, x stay on
 *  chip, the z' rows at the slab edges and the per-GPU totals cross xGMI from inside the kernel, one extra hop per iteration;
 *  resets, the first iteration and slab shapes the kernel cannot tile (row length not a multiple of 128, ...) run the two-kernel
 *  iteration with mailbox collectives between the kernels.  A wait on a peer that gives up (peer gone) fails the call, it never
 *  hangs; a failed persistent segment makes ALL ranks restart the solve on the two-kernel iteration (piso_comm_stats counts it).
 *  row_capacity = longest grid row (cells) the communicator will carry.  x_out_global must be NULL (gather the slabs yourself).
 *
 *  RCCL (piso_comm_unique_id / piso_comm_create): per iteration K1, a 3-double all-reduce, K2, a 3-double all-reduce and a
 *  one-row halo exchange of the residual -- stream-ordered RCCL calls, no host sync, two-kernel iteration only.  The same
 *  communicator carries the slab BiCGStab and the halo messages of the sharded step (below).  librccl is
 *  dlopen'ed on first use; the 128-byte unique id is created on one rank and distributed by the caller.
 *
 *   laplace_local [ny_local*nx][5], divergence_local / x_out_local [ny_local*nx]: this rank's rows;
 *   x_out_global  [world*ny_local*nx] or NULL (RCCL transport): every rank receives the full solution (all-gather).
 * piso_cg_solve_slab_emulated_f64 runs `slabs` virtual ranks on ONE device in lock-step with an in-process loopback: same
 * kernels, same halo / partial-sum logic; it exists to test the multi-rank index logic of the two-kernel iteration on one GPU.
 * piso_comm_stats: out6 = {transport (1 RCCL, 2 peer), CG iterations executed inside persistent slab segments, solves restarted
 * on the two-kernel iteration, persistent launches, slab solves verified against the true residual b - A^ x after persistent
 * segments (every one is; the check needs the neighbours' edge rows of x and covers what crossed xGMI), checks that failed on
 * some rank (all ranks then restart together)}.
 * ------------------------------------------------------------------------------------------------------------- */
int piso_comm_peer_create(int rank, int world, int row_capacity, void** comm_out, void* ipc_handle64_out);
int piso_comm_peer_connect(void* comm, const void* ipc_handles64_all_ranks);
/* The same mailboxes for nodes that refuse hipIpc handles across ranks: exportable virtual-memory allocations (hipMemCreate, uncached
 * type) shared as POSIX file descriptors.  Step 1 creates and maps the rank's mailbox and returns a file descriptor; the caller hands a
 * copy to every other rank (a Unix socket with SCM_RIGHTS; diffpiso/distributed.py) and closes its own; step 2 takes the descriptors
 * received from the other ranks (fds_all_ranks[r] for r != rank), imports and maps them.  Everything else is the peer transport above. */
int piso_comm_peer_create_fd(int rank, int world, int row_capacity, void** comm_out, int* fd_out);
int piso_comm_peer_connect_fd(void* comm, const int* fds_all_ranks);
/* Mailbox ping-pong: `iters` round trips of one tagged 8-byte word between ranks a (initiator) and b; a == b: a rank's own mailbox.
 * Called by EVERY rank with the same arguments (others return at once); us_per_round_trip_out is written on rank a. */
int piso_comm_pingpong(void* comm, int a, int b, int iters, float* us_per_round_trip_out, piso_stream_t stream);
int piso_comm_stats(void* comm, long long* out6);
/* The slab-decomposed STEP (new design): the *_slab twins of piso_assemble_csr, piso_pad_velocity, piso_a0_vfirst,
 * piso_face_forward / _backward, piso_divergence(_adjoint), piso_h_contribution(_adjoint), piso_laplace_matrix_* and piso_csr_matvec_f32
 * (declared next to their entry points; piso_slab_t above says what the arrays hold) work on one rank's rows.
 * piso_comm_exchange fills halo rows: msgs28 = 4 x {count <= 3, off[3], len[3]} element segments of `vec` {sent to the upper
 * neighbour, sent to the lower, received from the lower, received from the upper} (ring neighbours); dtype 0 float, 1 double,
 * 2 int32; a no-op on one rank.  Peer transport: one launch, the elements cross xGMI as 8-byte words written into the consumer's
 * mailbox.  RCCL transport: grouped ncclSend / ncclRecv of the segments on the stream, straight from / into `vec`.
 * piso_comm_check: has a wait on a peer given up (agreed over the ranks; peer transport - RCCL has no bounded waits)? */
int piso_comm_exchange(void* comm, void* vec, int dtype, const int* msgs28, piso_stream_t stream);
int piso_comm_check(void* comm, piso_stream_t stream);
/* All-gather of `count` doubles per rank, in rank order: dst holds count * world doubles on every rank (queued on the stream).  Peer
 * transport: a host-launched mailbox kernel, count * world <= 8192 (more: PISO_ERR_INVALID_ARG); one rank copies, unless the option
 * "slab_force" sends the chunk through its own mailbox.  The bits arrive unchanged (NaN payloads, -0.0, infinities). */
int piso_comm_allgather_f64(void* comm, const void* src, void* dst, int count, piso_stream_t stream);
/* ... and of `count` floats per rank (the float rows of the float32 multigrid cycle): peer transport count * world <= 8192, a float is
 * one tagged word of the gather area; RCCL: ncclFloat.  The bits arrive unchanged. */
int piso_comm_allgather_f32(void* comm, const void* src, void* dst, int count, piso_stream_t stream);
/* Slab-decomposed ILU(0)-BiCGStab (either transport): same arguments as piso_multi_bicgstab_ilu_*, all arrays FULL on every rank
 * (the assembly is cheap and replicated); the rank works on the face rows of its ny / world cell rows, which must be whole
 * preconditioner bands (ny / world a multiple of the band height: then the banded ILU(0) is the single-GPU one and the iterates
 * agree to summation order).  Per iteration: the five dot products are all-reduced INSIDE the one-block scalar kernels (tagged
 * words through the mailboxes), the inputs of the two SpMVs receive their neighbours' edge rows (u[j], v[j], v[j+1] downwards,
 * u[j], v[j] upwards, ring).  x_out is valid on the owned rows only.  The communicator's row_capacity must be >= 3 nx + 1.
 * RCCL transport (where the environment refuses hipIpc): every scalar stage is two launches around an 8-double ncclAllReduce, the
 * edge rows travel by grouped ncclSend / ncclRecv on the side stream - stream-ordered, no host sync, same arithmetic. */
int piso_multi_bicgstab_ilu_slab_f32(void* comm, const float* csr_val, const int* csr_rowptr, const int* csr_col, const float* rhs,
                                     const float* x0, float* x_out, int nx, int ny, float tol, int max_it, int transpose,
                                     int band_rows, uint8_t* warning, int* iterations_out, void* workspace, size_t workspace_bytes,
                                     piso_stream_t stream);
int piso_multi_bicgstab_ilu_slab_f64(void* comm, const double* csr_val, const int* csr_rowptr, const int* csr_col, const double* rhs,
                                     const double* x0, double* x_out, int nx, int ny, float tol, int max_it, int transpose,
                                     int band_rows, uint8_t* warning, int* iterations_out, void* workspace, size_t workspace_bytes,
                                     piso_stream_t stream);
/* The same solver on LOCAL storage (the slab-decomposed step, round 5): csr_*, rhs, x0, x_out and the workspace hold the rank's stored
 * rows only (piso_slab_t; the caller fills the halo rows of csr_val with piso_comm_exchange - the transposed solve gathers from them);
 * nx, ny, periodic_* are the whole grid's.  x_out is written on the owned rows. */
size_t piso_bicgstab_slab_workspace_bytes(int nx, int ny, int elem_size, const piso_slab_t* slab);
int piso_multi_bicgstab_ilu_slab_local_f32(void* comm, const float* csr_val, const int* csr_rowptr, const int* csr_col, const float* rhs,
                                           const float* x0, float* x_out, int nx, int ny, int periodic_x, int periodic_y, float tol, int max_it,
                                           int transpose, int band_rows, uint8_t* warning, int* iterations_out, void* workspace,
                                           size_t workspace_bytes, piso_stream_t stream, const piso_slab_t* slab);
int piso_multi_bicgstab_ilu_slab_local_f64(void* comm, const double* csr_val, const int* csr_rowptr, const int* csr_col, const double* rhs,
                                           const double* x0, double* x_out, int nx, int ny, int periodic_x, int periodic_y, float tol, int max_it,
                                           int transpose, int band_rows, uint8_t* warning, int* iterations_out, void* workspace,
                                           size_t workspace_bytes, piso_stream_t stream, const piso_slab_t* slab);
int piso_comm_unique_id(void* id128);
int piso_comm_create(const void* id128, int rank, int world, void** comm_out);
int piso_comm_destroy(void* comm);
size_t piso_cg_slab_workspace_bytes(int nx, int ny_local, int local_ranks);
int piso_cg_solve_slab_f64(void* comm, int nx, int ny_local, int periodic_x, int periodic_y, const double* laplace_local,
                           const double* divergence_local, double* x_out_local, double* x_out_global, float accuracy,
                           int max_iterations, int rank_deficient, int residual_reset, int* iterations_out, void* workspace,
                           size_t workspace_bytes, piso_stream_t stream);
int piso_cg_solve_slab_emulated_f64(int slabs, int nx, int ny, int periodic_x, int periodic_y, const double* laplace,
                                    const double* divergence, double* x_out, float accuracy, int max_iterations,
                                    int rank_deficient, int residual_reset, int* iterations_out, void* workspace,
                                    size_t workspace_bytes, piso_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training losses on flat u-first face vectors (csrc/loss.hip; the reference computes them as TensorFlow graph ops,
 * diffpiso/losses.py:6-35 and :66-95).  pred / target: the `.flat` vector of a step's result - the whole grid's, or for the *_slab
 * twins the rank's stored rows (piso_slab_t).  Fields are read as float32 and every term is formed in float32 in the order of the
 * reference's ops; only the sum is float64.
 *
 * Value entries: two launches - float64 per-block partials into `workspace` (piso_loss_workspace_bytes()), then ONE workgroup re-adds
 *   them in index order into value[0] (a device double; the same bits on every run of the same launch).  A slab launch adds what the rank
 *   OWNS, so the ranks' values add up to the whole grid's: L2 - its owned faces (the duplicate row v[ny] belongs to the slab with
 *   owns_last_face_row); strain - the entries of its owned cell rows (corner (j, i) belongs to cell row j).
 * Gradient entries (*_grad): d_pred[face] = upstream[0] * d value / d pred[face] as float32, one thread per owned face, GATHERING - a
 *   launch writes the owned faces and nothing else (the caller zeroes the halo rows of d_pred once).  upstream: ONE float on the device.
 *
 * piso_loss_l2:  factor / 2 * sum (pred - target)^2 over the crop window.  The window lives on the indices of the staggered tensor
 *   [ny + 1][nx + 1][2] the torch loss slices: a u face (j, i), 0 <= j < ny, 0 <= i <= nx, and a v face (j, i), 0 <= j <= ny, 0 <= i < nx,
 *   count iff y0 <= j < y1 and x0 <= i < x1 (0 <= y0, y1 <= ny + 1, 0 <= x0, x1 <= nx + 1; y1 <= y0 or x1 <= x0: empty).  The tensor's
 *   padded last row of u and last column of v are not faces and contribute nothing.  Gradient: factor * (pred - target) inside, 0 outside.
 *
 * piso_loss_strain:  factor * (sum |D yy| + 2 sum |D off| + sum |D xx|), D e = e(pred) - e(target), the unpadded strain entries
 *     yy  at cells (j, i), 0 <= j < ny, 0 <= i < nx:        (v[j+1][i] - v[j][i]) / dy
 *     xx  at the same cells:                                 (u[j][i+1] - u[j][i]) / dx
 *     off at the INTERIOR grid corners (j, i), 1 <= j <= ny - 1, 1 <= i <= nx - 1 (corner (j, i) = the lower left corner of cell (j, i)):
 *                                                            ((v[j][i] - v[j][i-1]) / dx + (u[j][i] - u[j-1][i]) / dy) / 2
 *   The corner set has no entry on the border of the domain: row 0 and column 0 are not corners, and neither are row ny / column nx.
 *   off counts twice - the reference sums the four parts [yy, off, off, xx].  Gradient of a face: the sum of sign(D e) * (d e / d face)
 *   over the at most six entries that read it, sign(0) = 0.  Both launches read rows j - 1 .. j + 1 around an owned row j of pred AND
 *   target: on slabs the caller fills their halo rows (one row either side suffices; the stored 2 (u) / 3 (v) rows hold it).
 * nx, ny >= 1 (strain: >= 2, dx, dy > 0); anything else, or an illegal slab: PISO_ERR_INVALID_ARG before any launch.
 * ------------------------------------------------------------------------------------------------------------- */
size_t piso_loss_workspace_bytes(void);
int piso_loss_l2(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, double factor, double* value,
                 void* workspace, size_t workspace_bytes, piso_stream_t stream);
int piso_loss_l2_slab(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, double factor, double* value,
                      void* workspace, size_t workspace_bytes, piso_stream_t stream, const piso_slab_t* slab);
int piso_loss_l2_grad(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, float factor,
                      const float* upstream, float* d_pred, piso_stream_t stream);
int piso_loss_l2_grad_slab(const float* pred, const float* target, int nx, int ny, int y0, int y1, int x0, int x1, float factor,
                           const float* upstream, float* d_pred, piso_stream_t stream, const piso_slab_t* slab);
int piso_loss_strain(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, double* value, void* workspace,
                     size_t workspace_bytes, piso_stream_t stream);
int piso_loss_strain_slab(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, double* value,
                          void* workspace, size_t workspace_bytes, piso_stream_t stream, const piso_slab_t* slab);
int piso_loss_strain_grad(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, const float* upstream,
                          float* d_pred, piso_stream_t stream);
int piso_loss_strain_grad_slab(const float* pred, const float* target, int nx, int ny, float dx, float dy, double factor, const float* upstream,
                               float* d_pred, piso_stream_t stream, const piso_slab_t* slab);

/* ---------------------------------------------------------------------------------------------------------------
 * Spectral-energy loss around the transform (csrc/loss_spectrum.hip; the reference's losses.py:38-64 over evaluation_tools.py:157-186).
 * The FFT itself is the caller's (rocFFT); these are the passes either side of it.  Whole-grid kernels, no atomics, no workspace: every
 * output is the same bits on every run of the same launch.
 *
 * piso_loss_centre_crop:  flat u-first face vector -> planes [2][h][w] float32, the crop of the field at the cell centres.  The crop lives
 *   on CELL indices: cell (j, i) counts iff y0 <= j < y1 and x0 <= i < x1 (0 <= y0 < y1 <= ny, 0 <= x0 < x1 <= nx); h = y1 - y0, w = x1 - x0.
 *   plane 0 (v at the centres): 0.5f * (v[j+1][i] + v[j][i]);  plane 1 (u at the centres): 0.5f * (u[j][i+1] + u[j][i]).
 * piso_loss_centre_crop_adjoint:  d_planes [2][h][w] -> d_faces (the WHOLE flat vector is written): one thread per face gathers
 *   0.5f * d_planes of the at most two cropped cells that read the face; 0 for a face no cropped cell reads.
 *
 * piso_loss_spectrum_shells:  spec = the complex64 transform of the planes, [2][h][w] interleaved (re, im) floats, UNSHIFTED.
 *   energy[k] = 0.5 / (h w)^2 * sum over the coefficients q of shell k of (|spec[0][q]|^2 + |spec[1][q]|^2), 0 <= k < cutoff, float64.
 *   The shells come as a table: perm[offsets[k]] .. perm[offsets[k + 1] - 1] are the flat indices q = q0 * w + q1 of shell k (int32, offsets
 *   has cutoff + 1 entries, entries of perm outside [0, h w) are skipped).  One workgroup per shell, strided by thread, fixed-order block sum.
 * piso_loss_spectrum_shells_adjoint:  d_spec[c][q] = upstream[0] * 2 * 0.5 / (h w)^2 * d_energy[shell[q]] * spec[c][q] for both floats of the
 *   pair - the cotangent of the REAL view of the transform -, 0 where shell[q] is not in [0, cutoff).  shell: int32 [h w], the shell of
 *   every unshifted coefficient.  upstream: ONE float on the device, or NULL for 1.
 *
 * piso_loss_spectrum_distance:  one workgroup; value[0] and d_e_pred[k] = d value / d e_pred[k] (all cutoff entries are written), float64.
 *     log_distance != 0:  factor * sqrt(sum over k >= 1 + start_wavenumber of log(e_gt[k] / e_pred[k])^2)
 *     log_distance == 0:  factor * sum over k >= 1 of |e_gt[k] - e_pred[k]|  (start_wavenumber is ignored, as in the reference)
 *   An empty range (cutoff <= 1 + start_wavenumber) gives 0.  A sum of exactly 0 in the log form (identical spectra) gives value 0 and
 *   gradient 0.  A zero or non-finite energy inside the range of the log form gives a non-finite value (log of 0, of infinity or of 0 / 0).
 * NULL pointers (upstream excepted), h or w below 1, a crop outside the grid, cutoff outside [0, min(h, w) / 2], a negative
 * start_wavenumber: PISO_ERR_INVALID_ARG before any launch.
 * ------------------------------------------------------------------------------------------------------------- */
int piso_loss_centre_crop(const float* faces, int nx, int ny, int y0, int y1, int x0, int x1, float* planes, piso_stream_t stream);
int piso_loss_centre_crop_adjoint(const float* d_planes, int nx, int ny, int y0, int y1, int x0, int x1, float* d_faces, piso_stream_t stream);
int piso_loss_spectrum_shells(const float* spec, const int* perm, const int* offsets, int h, int w, int cutoff, double* energy,
                              piso_stream_t stream);
int piso_loss_spectrum_shells_adjoint(const float* spec, const int* shell, const double* d_energy, const float* upstream, int h, int w, int cutoff,
                                      float* d_spec, piso_stream_t stream);
int piso_loss_spectrum_distance(const double* e_pred, const double* e_gt, int cutoff, int start_wavenumber, int log_distance, double factor,
                                double* value, double* d_e_pred, piso_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PISO_HIP_H */
