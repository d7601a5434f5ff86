"""ctypes binding of libpiso_hip.so -- the hand-written gfx950 kernels behind the C ABI of include/piso_hip.h.

Mirrors the reference's `tf.load_op_library(...)` blocks (diffpiso/piso_tf.py:3-8, diffpiso/linear_solver.py:6-12,
diffpiso/piso_cuda_pressure_solver.py:4-8): importing the package FAILS if the native library is missing -- there is no
CPU or PyTorch fallback for the solver path.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PISO_HIP_LIB: load another BUILD of the same library (A/B timing of kernel variants, scripts/sweep_*.sh) instead of
# overwriting the product library in place.  It is not a fallback: the file must exist and export the same C ABI.
LIB_PATH = os.environ.get("PISO_HIP_LIB") or os.path.join(_HERE, "libpiso_hip.so")

if not os.path.isfile(LIB_PATH):
    raise ImportError('HIP binaries not found at %s. Run "python differentiable-piso_amd/build_native.py" '
                      '(or __graft_entry__.build()) to compile them' % LIB_PATH)

lib = C.CDLL(LIB_PATH)

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_ip = C.POINTER(C.c_int)

lib.piso_version.restype = C.c_char_p
lib.piso_last_error_string.restype = C.c_char_p
lib.piso_device_count.restype = _i
lib.piso_set_option.argtypes = [C.c_char_p, _i]
lib.piso_set_option.restype = _i
lib.piso_get_option.argtypes = [C.c_char_p, _ip]
lib.piso_get_option.restype = _i
lib.piso_cg_persist_fallbacks.restype = _i
lib.piso_cg_last_xcd_map.argtypes = [_ip, _i]
lib.piso_cg_last_xcd_map.restype = _i
lib.piso_cg_tiny_solves.restype = C.c_longlong
lib.piso_cg_last_dispatch.argtypes = [_ip, _i]
lib.piso_cg_last_dispatch.restype = _i
lib.piso_bicgstab_last_dispatch.argtypes = [_ip, _i]
lib.piso_bicgstab_last_dispatch.restype = _i
lib.piso_conv_last_dispatch.argtypes = [_ip, _i]
lib.piso_conv_last_dispatch.restype = _i
lib.piso_cg_verify_stats.argtypes = [C.POINTER(C.c_longlong), _ip]
lib.piso_cg_verify_stats.restype = None
lib.piso_csr_nnz.argtypes = [_i, _i, _i, _i, _ip, _ip]
lib.piso_csr_nnz.restype = None
lib.piso_assemble_csr.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _vp, _f, _vp]
lib.piso_assemble_csr.restype = _i
for _n in ("piso_laplace_matrix_f64", "piso_laplace_matrix_f32"):
    getattr(lib, _n).argtypes = [_i, _i, _vp, _vp, _vp, _vp, _vp]
    getattr(lib, _n).restype = _i
lib.piso_cg_workspace_bytes.argtypes = [_i, _i, _i]
lib.piso_cg_workspace_bytes.restype = _sz
for _n in ("piso_cg_solve_f64", "piso_cg_solve_f32"):
    getattr(lib, _n).argtypes = [_i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _i, _ip, _vp, _sz, _vp]
    getattr(lib, _n).restype = _i
for _n in ("piso_cg_solve_async_f64", "piso_cg_solve_async_f32"):
    getattr(lib, _n).argtypes = [_i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _i, _vp, _vp, _sz, _vp]
    getattr(lib, _n).restype = _i
ERR_NEEDS_HOST = 5      # include/piso_hip.h: PISO_ERR_NEEDS_HOST
ERR_UNSUPPORTED_PATTERN = 3
lib.piso_mg_workspace_bytes.argtypes = [_i, _i]
lib.piso_mg_workspace_bytes.restype = _sz
lib.piso_mg_pcg_solve_f64.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _i, _i, _ip, _vp, _sz, _vp]
lib.piso_mg_pcg_solve_f64.restype = _i
lib.piso_mg_vcycle_f64.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]
lib.piso_mg_vcycle_f64.restype = _i
lib.piso_mg_level_f64.argtypes = [_i, _i, _i, _i, _vp, _i, _ip, _ip, _vp, _vp, _sz, _vp]
lib.piso_mg_level_f64.restype = _i
lib.piso_mg_workspace_bytes_cycle.argtypes = [_i, _i, _i]
lib.piso_mg_workspace_bytes_cycle.restype = _sz
lib.piso_mg_pcg_solve_c32_f64.argtypes = lib.piso_mg_pcg_solve_f64.argtypes
lib.piso_mg_pcg_solve_c32_f64.restype = _i
lib.piso_mg_vcycle_c32_f64.argtypes = lib.piso_mg_vcycle_f64.argtypes
lib.piso_mg_vcycle_c32_f64.restype = _i
lib.piso_mg_level_c32_f64.argtypes = lib.piso_mg_level_f64.argtypes
lib.piso_mg_level_c32_f64.restype = _i
for _s in ("_f64", "_c32_f64"):            # (x0 after the divergence; NULL: the namesake's call)
    getattr(lib, "piso_mg_pcg_solve_guess" + _s).argtypes = [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _ip, _vp, _sz, _vp]
    getattr(lib, "piso_mg_pcg_solve_guess" + _s).restype = _i
    getattr(lib, "piso_mg_pcg_solve_prepared_guess" + _s).argtypes = [_i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _f, _i, _i, _i, _i, _ip, _vp, _sz, _vp]
    getattr(lib, "piso_mg_pcg_solve_prepared_guess" + _s).restype = _i
lib.piso_mg_last_guess.argtypes = []
lib.piso_mg_last_guess.restype = _i
lib.piso_mg_hierarchy_bytes.argtypes = [_i, _i, _i]
lib.piso_mg_hierarchy_bytes.restype = _sz
lib.piso_mg_solve_workspace_bytes.argtypes = [_i, _i, _i]
lib.piso_mg_solve_workspace_bytes.restype = _sz
for _s in ("_f64", "_c32_f64"):
    getattr(lib, "piso_mg_prepare" + _s).argtypes = [_i, _i, _i, _i, _vp, _i, _vp, _sz, _vp, _sz, _vp]
    getattr(lib, "piso_mg_prepare" + _s).restype = _i
    getattr(lib, "piso_mg_pcg_solve_prepared" + _s).argtypes = [_i, _i, _i, _i, _vp, _sz, _vp, _vp, _f, _i, _i, _i, _i, _ip, _vp, _sz, _vp]
    getattr(lib, "piso_mg_pcg_solve_prepared" + _s).restype = _i
    getattr(lib, "piso_mg_vcycle_prepared" + _s).argtypes = [_i, _i, _i, _i, _vp, _sz, _vp, _vp, _i, _vp, _sz, _vp]
    getattr(lib, "piso_mg_vcycle_prepared" + _s).restype = _i
lib.piso_mg_slab_workspace_bytes.argtypes = [_i, _i, _i, _i]
lib.piso_mg_slab_workspace_bytes.restype = _sz
lib.piso_mg_slab_plan.argtypes = [_i, _i, _i, _i, _ip, _i]
lib.piso_mg_slab_plan.restype = _i
lib.piso_mg_pcg_solve_slab_f64.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _i, _i, _ip, _vp, _sz, _vp]
lib.piso_mg_pcg_solve_slab_f64.restype = _i
lib.piso_mg_vcycle_slab_f64.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]
lib.piso_mg_vcycle_slab_f64.restype = _i
lib.piso_mg_level_slab_f64.argtypes = [_vp, _i, _i, _i, _i, _vp, _i, _ip, _ip, _vp, _vp, _sz, _vp]
lib.piso_mg_level_slab_f64.restype = _i
lib.piso_mg_pcg_solve_slab_emulated_f64.argtypes = [_i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _i, _i, _ip, _vp, _sz, _vp]
lib.piso_mg_pcg_solve_slab_emulated_f64.restype = _i
lib.piso_mg_vcycle_slab_emulated_f64.argtypes = [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]
lib.piso_mg_vcycle_slab_emulated_f64.restype = _i
lib.piso_mg_level_slab_emulated_f64.argtypes = [_i, _i, _i, _i, _i, _i, _vp, _i, _ip, _ip, _vp, _vp, _sz, _vp]
lib.piso_mg_level_slab_emulated_f64.restype = _i
lib.piso_mg_slab_workspace_bytes_cycle.argtypes = [_i, _i, _i, _i, _i]
lib.piso_mg_slab_workspace_bytes_cycle.restype = _sz
for _n in ("pcg_solve_slab", "vcycle_slab", "level_slab", "pcg_solve_slab_emulated", "vcycle_slab_emulated", "level_slab_emulated"):
    getattr(lib, "piso_mg_%s_c32_f64" % _n).argtypes = getattr(lib, "piso_mg_%s_f64" % _n).argtypes
    getattr(lib, "piso_mg_%s_c32_f64" % _n).restype = _i
lib.piso_mg_last_dispatch.argtypes = [_ip, _i]
lib.piso_mg_last_dispatch.restype = _i
lib.piso_cg_fixed_iterations_f64.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp, _i, _i, C.POINTER(C.c_float), _vp, _sz, _vp]
lib.piso_cg_fixed_iterations_f64.restype = _i
lib.piso_cg_profile_enable.argtypes = [_i, _i]
lib.piso_cg_profile_enable.restype = None
lib.piso_cg_profile_read.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
lib.piso_cg_profile_read.restype = None
lib.piso_bicgstab_workspace_bytes.argtypes = [_i, _i, _i]
lib.piso_bicgstab_workspace_bytes.restype = _sz
for _n in ("piso_multi_bicgstab_ilu_f32", "piso_multi_bicgstab_ilu_f64"):
    getattr(lib, _n).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _i, _i, _vp, _ip, _vp, _sz, _vp]
    getattr(lib, _n).restype = _i
for _n in ("piso_multi_bicgstab_ilu_slab_f32", "piso_multi_bicgstab_ilu_slab_f64"):
    getattr(lib, _n).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _i, _i, _vp, _ip, _vp, _sz, _vp]
    getattr(lib, _n).restype = _i
lib.piso_csr_matvec_f32.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]
lib.piso_csr_matvec_f32.restype = _i


lib.piso_pad_velocity.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp]
lib.piso_pad_velocity.restype = _i
lib.piso_a0_vfirst.argtypes = [_vp, _vp, _i, _i, _f, _f, _vp]
lib.piso_a0_vfirst.restype = _i
lib.piso_face_forward.argtypes = [_i, _i, _i, _ip, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
lib.piso_face_forward.restype = _i
lib.piso_face_backward.argtypes = [_i, _i, _i, _ip, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
lib.piso_face_backward.restype = _i
lib.piso_divergence.argtypes = [_vp, _vp, _i, _i, _f, _f, _f, _vp]
lib.piso_divergence.restype = _i
lib.piso_divergence_adjoint.argtypes = [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp]
lib.piso_divergence_adjoint.restype = _i
lib.piso_h_contribution.argtypes = [_vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp]
lib.piso_h_contribution.restype = _i
lib.piso_h_contribution_adjoint.argtypes = [_vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp]
lib.piso_h_contribution_adjoint.restype = _i

lib.piso_conv2d_weight_elems.argtypes = [_i, _i, _i]
lib.piso_conv2d_weight_elems.restype = _sz
lib.piso_conv2d_wgrad_workspace_bytes.argtypes = [_i, _i, _i]
lib.piso_conv2d_wgrad_workspace_bytes.restype = _sz
lib.piso_conv2d_forward.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]
lib.piso_conv2d_forward.restype = _i
lib.piso_conv2d_wgrad.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]
lib.piso_conv2d_wgrad.restype = _i
lib.piso_conv2d_forward_ex.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]
lib.piso_conv2d_forward_ex.restype = _i
lib.piso_conv2d_wgrad_ex.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]
lib.piso_conv2d_wgrad_ex.restype = _i
lib.piso_conv2d_weight_elems_any.argtypes = [_i, _i, _i]
lib.piso_conv2d_weight_elems_any.restype = _sz
lib.piso_conv2d_wgrad_any_workspace_bytes.argtypes = [_i, _i, _i, _i]
lib.piso_conv2d_wgrad_any_workspace_bytes.restype = _sz
lib.piso_conv2d_instantiated.argtypes = [_i, _i, _i, _i]
lib.piso_conv2d_instantiated.restype = _i
lib.piso_conv2d_forward_any.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]
lib.piso_conv2d_forward_any.restype = _i
lib.piso_conv2d_wgrad_any.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]
lib.piso_conv2d_wgrad_any.restype = _i
lib.piso_conv_epilogue_plan.argtypes = [_i, _i, _ip, _ip]
lib.piso_conv_epilogue_plan.restype = _i
lib.piso_conv_epilogue_workspace_bytes.argtypes = [_i, _i]
lib.piso_conv_epilogue_workspace_bytes.restype = _sz
lib.piso_conv_epilogue_forward.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]
lib.piso_conv_epilogue_forward.restype = _i
lib.piso_conv_epilogue_backward.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]
lib.piso_conv_epilogue_backward.restype = _i
lib.piso_conv_last_geometry.argtypes = [_ip, _i]
lib.piso_conv_last_geometry.restype = _i
lib.piso_leaky_relu_backward.argtypes = [_vp, _vp, _vp, _sz, _vp]
lib.piso_leaky_relu_backward.restype = _i

lib.piso_comm_unique_id.argtypes = [_vp]
lib.piso_comm_unique_id.restype = _i
lib.piso_comm_create.argtypes = [_vp, _i, _i, C.POINTER(_vp)]
lib.piso_comm_create.restype = _i
lib.piso_comm_destroy.argtypes = [_vp]
lib.piso_comm_destroy.restype = _i
lib.piso_comm_peer_create.argtypes = [_i, _i, _i, C.POINTER(_vp), _vp]
lib.piso_comm_peer_create.restype = _i
lib.piso_comm_peer_connect.argtypes = [_vp, _vp]
lib.piso_comm_peer_connect.restype = _i
lib.piso_comm_peer_create_fd.argtypes = [_i, _i, _i, C.POINTER(_vp), _ip]
lib.piso_comm_peer_create_fd.restype = _i
lib.piso_comm_peer_connect_fd.argtypes = [_vp, _ip]
lib.piso_comm_peer_connect_fd.restype = _i
lib.piso_comm_pingpong.argtypes = [_vp, _i, _i, _i, C.POINTER(C.c_float), _vp]
lib.piso_comm_pingpong.restype = _i
lib.piso_comm_stats.argtypes = [_vp, C.POINTER(C.c_longlong)]
lib.piso_comm_stats.restype = _i


class Slab(C.Structure):
    """include/piso_hip.h: piso_slab_t - one rank's rows of a grid cut into y-slabs (the *_slab entry points; local storage)."""
    _fields_ = [("ny_global", _i), ("row_begin", _i), ("row_end", _i), ("owns_last_face_row", _i)]


_sp = C.POINTER(Slab)
lib.piso_slab_sizes.argtypes = [_sp, _i, _i, _i, _i, _ip]
lib.piso_slab_sizes.restype = _i
lib.piso_assemble_csr_slab.argtypes = lib.piso_assemble_csr.argtypes + [_sp, _i]
lib.piso_assemble_csr_slab.restype = _i
for _n in ("piso_laplace_matrix_f64", "piso_laplace_matrix_f32", "piso_pad_velocity", "piso_a0_vfirst", "piso_face_forward", "piso_face_backward",
           "piso_divergence", "piso_divergence_adjoint", "piso_h_contribution", "piso_h_contribution_adjoint"):
    getattr(lib, _n + "_slab").argtypes = getattr(lib, _n).argtypes + [_sp]
    getattr(lib, _n + "_slab").restype = _i
lib.piso_closure_input.argtypes = [_vp, _vp, _vp, _i, _i, _i, _ip, C.c_double, _vp]
lib.piso_closure_input_adjoint.argtypes = [_vp, _vp, _vp, _i, _i, _i, _ip, C.c_double, _vp]
lib.piso_closure_force.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp]
lib.piso_closure_force_adjoint.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp]
for _n in ("piso_closure_input", "piso_closure_input_adjoint", "piso_closure_force", "piso_closure_force_adjoint"):
    getattr(lib, _n).restype = _i
    getattr(lib, _n + "_slab").argtypes = getattr(lib, _n).argtypes + [_sp, _i, _i]        # (slab, ext_lo, ext_hi)
    getattr(lib, _n + "_slab").restype = _i
lib.piso_closure_halo_add.argtypes = [_vp, _vp, _sz, _vp]
lib.piso_closure_halo_add.restype = _i
_d = C.c_double
lib.piso_loss_workspace_bytes.argtypes = []
lib.piso_loss_workspace_bytes.restype = _sz
lib.piso_loss_l2.argtypes = [_vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _sz, _vp]          # (pred, target, nx, ny, y0, y1, x0, x1, factor, value, ws, bytes, stream)
lib.piso_loss_l2_grad.argtypes = [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]          # (..., factor, upstream, d_pred, stream)
lib.piso_loss_strain.argtypes = [_vp, _vp, _i, _i, _f, _f, _d, _vp, _vp, _sz, _vp]              # (pred, target, nx, ny, dx, dy, factor, value, ws, bytes, stream)
lib.piso_loss_strain_grad.argtypes = [_vp, _vp, _i, _i, _f, _f, _d, _vp, _vp, _vp]              # (..., factor, upstream, d_pred, stream)
for _n in ("piso_loss_l2", "piso_loss_l2_grad", "piso_loss_strain", "piso_loss_strain_grad"):
    getattr(lib, _n).restype = _i
    getattr(lib, _n + "_slab").argtypes = getattr(lib, _n).argtypes + [_sp]
    getattr(lib, _n + "_slab").restype = _i
lib.piso_loss_centre_crop.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]                    # (faces, nx, ny, y0, y1, x0, x1, planes, stream)
lib.piso_loss_centre_crop_adjoint.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]            # (d_planes, ..., d_faces, stream)
lib.piso_loss_spectrum_shells.argtypes = [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]                  # (spec, perm, offsets, h, w, cutoff, energy, stream)
lib.piso_loss_spectrum_shells_adjoint.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]     # (spec, shell, d_energy, upstream, h, w, cutoff, d_spec, stream)
lib.piso_loss_spectrum_distance.argtypes = [_vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp]            # (e_pred, e_gt, cutoff, start, log, factor, value, d_e_pred, stream)
for _n in ("piso_loss_centre_crop", "piso_loss_centre_crop_adjoint", "piso_loss_spectrum_shells", "piso_loss_spectrum_shells_adjoint",
           "piso_loss_spectrum_distance"):
    getattr(lib, _n).restype = _i
lib.piso_csr_matvec_f32_slab.argtypes =[_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sp]
lib.piso_csr_matvec_f32_slab.restype = _i
lib.piso_bicgstab_slab_workspace_bytes.argtypes = [_i, _i, _i, _sp]
lib.piso_bicgstab_slab_workspace_bytes.restype = _sz
for _n in ("piso_multi_bicgstab_ilu_slab_local_f32", "piso_multi_bicgstab_ilu_slab_local_f64"):
    getattr(lib, _n).argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, _i, _vp, _ip, _vp, _sz, _vp, _sp]
    getattr(lib, _n).restype = _i
lib.piso_comm_exchange.argtypes = [_vp, _vp, _i, _ip, _vp]
lib.piso_comm_exchange.restype = _i
lib.piso_comm_allgather_f64.argtypes = [_vp, _vp, _vp, _i, _vp]
lib.piso_comm_allgather_f64.restype = _i
lib.piso_comm_allgather_f32.argtypes = lib.piso_comm_allgather_f64.argtypes
lib.piso_comm_allgather_f32.restype = _i
lib.piso_comm_check.argtypes = [_vp, _vp]
lib.piso_comm_check.restype = _i
lib.piso_cg_slab_workspace_bytes.argtypes = [_i, _i, _i]
lib.piso_cg_slab_workspace_bytes.restype = _sz
lib.piso_cg_solve_slab_f64.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _ip, _vp, _sz, _vp]
lib.piso_cg_solve_slab_f64.restype = _i
lib.piso_cg_solve_slab_emulated_f64.argtypes = [_i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _i, _ip, _vp, _sz, _vp]
lib.piso_cg_solve_slab_emulated_f64.restype = _i


class PisoNativeError(RuntimeError):
    pass


def set_option(name, value):
    """Tuning / test knob of the library (include/piso_hip.h: piso_set_option); -1 = automatic."""
    if lib.piso_set_option(name.encode(), int(value)) != 0:
        raise PisoNativeError("unknown libpiso_hip option %r" % name)


def get_option(name):
    v = C.c_int(0)
    if lib.piso_get_option(name.encode(), C.byref(v)) != 0:
        raise PisoNativeError("unknown libpiso_hip option %r" % name)
    return v.value


def cg_verify_stats():
    """(solves whose result was checked against the true residual, checks that failed) -- include/piso_hip.h."""
    runs, fails = C.c_longlong(0), C.c_int(0)
    lib.piso_cg_verify_stats(C.byref(runs), C.byref(fails))
    return int(runs.value), int(fails.value)


def check(status, what):
    if status != 0:
        raise PisoNativeError("%s failed with status %d: %s" % (what, status, lib.piso_last_error_string().decode()))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise PisoNativeError("libpiso_hip needs device tensors; got a %s tensor (no CPU fallback exists)" % t.device)
    if not t.is_contiguous():
        raise PisoNativeError("non-contiguous tensor passed to libpiso_hip")
    if t.device.index != torch._C._cuda_getDevice():
        # the kernels are launched on the CURRENT device's stream: a tensor of another GPU would be a wild pointer there
        raise PisoNativeError("tensor lives on %s but the current HIP device is cuda:%d (wrap the call in "
                              "`with torch.cuda.device(t.device)`)" % (t.device, torch.cuda.current_device()))
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    # (torch.cuda.current_stream() builds a Stream object and walks os.environ on the way: ~35 us per call, 15 calls per step)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


_workspaces = {}


def workspace(nbytes, device, tag):
    """Cached byte workspace per (device, tag); grown on demand. The library never allocates device memory itself."""
    key = (str(device), tag)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def cg_last_xcd_map():
    """The XCD of every workgroup of this thread's last chip-wide persistent CG launch (option cg_xcd_map = 1), as a tuple; () if none."""
    buf = (C.c_int * 256)()
    n = lib.piso_cg_last_xcd_map(buf, 256)
    return tuple(buf[i] for i in range(min(n, 256)))


def _last_dispatch(fn, name, fields):
    """The record a piso_*_last_dispatch function of the library keeps for the calling thread, as a dict over `fields`; {} if it has none."""
    buf = (C.c_int * 32)()
    n = fn(buf, 32)
    if n != 0 and n != len(fields):
        raise PisoNativeError("%s returned %d fields, this binding knows %d" % (name, n, len(fields)))
    return {k: buf[i] for i, k in enumerate(fields[:n])}


DISPATCH_FIELDS = ("path", "sizeof_T", "sizeof_CT", "V", "RECON", "symmetric", "rows_per_wave", "k1_grid", "k1_tiles", "R", "NQ", "waves",
                   "launch_grid", "padded", "xcd_local", "fell_back", "tiny_per_x", "k2_grid", "segments")


def cg_last_dispatch():
    """Which kernel instance this thread's last pressure CG solve was dispatched to (include/piso_hip.h: piso_cg_last_dispatch),
    as a dict; {} if the thread has not solved."""
    return _last_dispatch(lib.piso_cg_last_dispatch, "piso_cg_last_dispatch", DISPATCH_FIELDS)


BICGSTAB_DISPATCH_FIELDS = ("sizeof_T", "E", "sweep_lds", "factor_lds", "R", "bands_u", "bands_v", "blocks", "fold", "fuse_p", "transpose_flags",
                            "slab", "look0", "passes", "host_looks", "failed_mask")


def bicgstab_last_dispatch():
    """Which kernel instances this thread's last ILU(0)-BiCGStab solve ran (include/piso_hip.h: piso_bicgstab_last_dispatch), as a dict;
    {} if the thread has not solved or its last call was refused."""
    return _last_dispatch(lib.piso_bicgstab_last_dispatch, "piso_bicgstab_last_dispatch", BICGSTAB_DISPATCH_FIELDS)


CONV_DISPATCH_FIELDS = ("entry", "KS", "C", "NT", "IPW", "family", "leaky", "grid_x", "grid_y", "block", "rows_per_block", "nblocks", "reducer",
                        "Ho", "Wo")


def conv_last_dispatch():
    """Which kernel instance this thread's last piso_conv2d_forward / piso_conv2d_wgrad (or their *_ex / *_any forms) ran (include/piso_hip.h:
    piso_conv_last_dispatch), as a dict; {} if the thread has not run a convolution."""
    return _last_dispatch(lib.piso_conv_last_dispatch, "piso_conv_last_dispatch", CONV_DISPATCH_FIELDS)


def conv2d_instantiated(entry, ks, cin, cout):
    """Do the fixed instance tables serve (entry 1 forward | 2 weight gradient, ks, cin, cout)?  (include/piso_hip.h: piso_conv2d_instantiated;
    pure host code.)  False: the shape runs the run-time-shaped family of the *_any entries."""
    return bool(lib.piso_conv2d_instantiated(int(entry), int(ks), int(cin), int(cout)))


def conv_epilogue_plan(pixels, channels):
    """(bands, pixels_per_band) of the bias sum of piso_conv_epilogue_backward (include/piso_hip.h: piso_conv_epilogue_plan; pure host code)."""
    bands, ppb = C.c_int(0), C.c_int(0)
    check(lib.piso_conv_epilogue_plan(int(pixels), int(channels), C.byref(bands), C.byref(ppb)), "piso_conv_epilogue_plan")
    return bands.value, ppb.value


CONV_GEOMETRY_FIELDS = ("pad_y", "pad_x", "wrap_y", "wrap_x")


def conv_last_geometry():
    """The geometry of this thread's last convolution (include/piso_hip.h: piso_conv_last_geometry) as a dict; {} after piso_conv2d_forward /
    piso_conv2d_wgrad (one pad, no wrap: the call's own argument) or before any convolution."""
    return _last_dispatch(lib.piso_conv_last_geometry, "piso_conv_last_geometry", CONV_GEOMETRY_FIELDS)


MG_DISPATCH_FIELDS = ("levels", "tail_first", "sweeps", "iterations", "cycles", "residual_recomputations", "cycle_elem", "vec_mask")


def mg_slab_plan(nx, ny, world, gather_cells=0):
    """The pure plan of a slab multigrid solve (csrc/mg_slab_plan.h) as a dict: levels [(nx, ny)], g (first replicated level), tail_first,
    rows (held per rank and level).  gather_cells 0: the option mg_slab_gather_cells / 8192.  A refused shape raises PisoNativeError."""
    buf = (C.c_int * 64)()
    n = lib.piso_mg_slab_plan(int(nx), int(ny), int(world), int(gather_cells), buf, 64)
    if buf[0] != 0:
        raise PisoNativeError("piso_mg_slab_plan refused %d x %d on %d ranks: %s" % (nx, ny, world, lib.piso_last_error_string().decode()))
    lv = [(buf[6 + 3 * l], buf[7 + 3 * l]) for l in range(buf[1])]
    assert n == 6 + 3 * buf[1]
    return {"levels": lv, "g": buf[2], "tail_first": buf[3], "nyl": buf[4], "world": buf[5], "rows": [buf[8 + 3 * l] for l in range(buf[1])]}


def mg_last_dispatch():
    """What this thread's last multigrid solve / cycle ran (include/piso_hip.h: piso_mg_last_dispatch), as a dict; {} if none."""
    return _last_dispatch(lib.piso_mg_last_dispatch, "piso_mg_last_dispatch", MG_DISPATCH_FIELDS)


def mg_last_guess():
    """What this thread's last multigrid solve did with its guess (include/piso_hip.h: piso_mg_last_guess): 0 none given, 1 accepted, 2 rejected."""
    return int(lib.piso_mg_last_guess())
