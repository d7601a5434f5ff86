"""Solver classes of the PISO step, backed by libpiso_hip.so (hand-written gfx950 kernels behind a C ABI).

Same class surface as the reference (diffpiso/linear_solver.py, diffpiso/piso_cuda_pressure_solver.py):
  LinearSolver                              base type                               (linear_solver.py:15-30)
  LinearSolverScipy                         host-side direct solve, cross-check only   (linear_solver.py:33-57)
  LinearSolverCudaMultiBicgstabILU          u+v ILU(0)-BiCGStab, adjoint = A^T solve  (linear_solver.py:113-178)
  PisoPressureSolverCudaCustom              A0-weighted 5-diagonal CG, adjoint = same solve (piso_cuda_pressure_solver.py:36-114)
The adjoint linear solves are `torch.autograd.Function` nodes (the reference uses tf.custom_gradient).
There is NO CPU / PyTorch fallback: tensors must live on the GPU and the native library must be present.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .grids import StaggeredGrid, as_tensor
from .stencils import flatten_staggered_data


class LinearSolver(object):
    """diffpiso/linear_solver.py:15-30."""

    def __init__(self, name, supported_devices, supports_guess, supports_batch, solver_type, input_format):
        self.name = name
        self.supported_devices = supported_devices
        self.supports_guess = supports_guess
        self.supports_batch = supports_batch
        self.solver_type = solver_type
        self.input_format = input_format

    def solve(self, *args):
        raise NotImplementedError(self.__class__)

    def __repr__(self):
        return self.name


def _scalar(v):
    if isinstance(v, torch.Tensor):
        return float(v.item())
    return float(v)


class _ScipySolveFn(torch.autograd.Function):
    """solve_call of LinearSolverScipy (diffpiso/linear_solver.py:45-54): direct sparse solve on the host, gradient w.r.t. the
    right-hand side = solve with the transposed matrix."""

    @staticmethod
    def _solve(mv, ci, rp, rhs, transpose):
        import scipy.sparse
        import scipy.sparse.linalg
        m = scipy.sparse.csr_matrix((mv.detach().cpu().numpy(), ci.detach().cpu().numpy(), rp.detach().cpu().numpy()))
        if transpose:
            m = m.transpose()
        x = scipy.sparse.linalg.spsolve(m.tocsr(), rhs.detach().cpu().numpy().reshape(-1))
        return torch.as_tensor(np.asarray(x, dtype=np.float32), device=rhs.device)

    @staticmethod
    def forward(ctx, rhs, mv, ci, rp, transpose):
        ctx.save_for_backward(mv, ci, rp)
        ctx.transpose = transpose
        return _ScipySolveFn._solve(mv, ci, rp, rhs, transpose)

    @staticmethod
    def backward(ctx, ds):
        mv, ci, rp = ctx.saved_tensors
        return _ScipySolveFn._solve(mv, ci, rp, ds, not ctx.transpose), None, None, None, None


class LinearSolverScipy(LinearSolver):
    """diffpiso/linear_solver.py:33-57: scipy.sparse.linalg.spsolve on ONE CSR matrix, on the host (the reference's manual
    cross-check for the CUDA solvers; it wraps it in tf.py_function).  It is a CPU solver by design, exactly as in the
    reference -- `piso_step` never selects it by itself and the HIP solvers never fall back to it."""

    def __init__(self):
        LinearSolver.__init__(self, "Scipy Solver for sparse matrix", supported_devices="CPU", supports_guess=False,
                              supports_batch=False, solver_type="-", input_format="csr")

    def solve(self, matrix_values, row_ptr, col_indices, rhs, transpose=False):
        return _ScipySolveFn.apply(rhs.reshape(-1), matrix_values.reshape(-1), col_indices.reshape(-1), row_ptr.reshape(-1),
                                   bool(transpose))


def multi_bicgstab_ilu_native(values, row_ptr, col_indices, rhs, x0, nx, ny, tol, max_it, transpose, band_rows, warn, slab_comm=None, negate=False):
    """One call of piso_multi_bicgstab_ilu_{f32,f64}. Returns (x, iterations[2]); sets warn[0] in place on NaN input.
    slab_comm (distributed.SlabCommunicator, either transport, more than one rank): the solve is cut into y-slabs over the ranks
    (every rank passes the full arrays and works on its rows; dot products are all-reduced inside the scalar kernels, the edge
    rows of the SpMV inputs travel through the mailboxes) and every rank returns the full solution.
    negate: the system matrix is -values (the sign is applied where the kernel reads the values: no pass over the array for it)."""
    if slab_comm is not None and slab_comm.world > 1:
        from .distributed import multi_bicgstab_ilu_slab, multi_bicgstab_ilu_slab_local
        if slab_comm.sharded:                # slab-decomposed STEP: every array holds the rank's stored rows (sharding.py)
            return multi_bicgstab_ilu_slab_local(slab_comm, values, row_ptr, col_indices, rhs, x0, nx, ny, tol, max_it, transpose, band_rows, warn,
                                                 negate=negate)
        return multi_bicgstab_ilu_slab(slab_comm, values, row_ptr, col_indices, rhs, x0, nx, ny, tol, max_it, transpose, band_rows, warn, negate=negate)
    dt = values.dtype
    assert dt in (torch.float32, torch.float64)
    values, rhs, x0 = values.contiguous(), rhs.to(dt).contiguous(), x0.to(dt).contiguous()
    row_ptr, col_indices = row_ptr.contiguous(), col_indices.contiguous()
    x = torch.empty_like(rhs)
    elem = 8 if dt == torch.float64 else 4
    nbytes = N.lib.piso_bicgstab_workspace_bytes(nx, ny, elem)
    ws = N.workspace(nbytes, rhs.device, "bicgstab")
    its = (C.c_int * 2)()
    fn = N.lib.piso_multi_bicgstab_ilu_f64 if dt == torch.float64 else N.lib.piso_multi_bicgstab_ilu_f32
    st = fn(N.ptr(values), N.ptr(row_ptr), N.ptr(col_indices), N.ptr(rhs), N.ptr(x0), N.ptr(x), nx, ny, C.c_float(tol),
            int(max_it), (1 if transpose else 0) | (2 if negate else 0), int(band_rows), N.ptr(warn), its, N.ptr(ws), C.c_size_t(ws.numel()),
            N.stream_ptr())
    N.check(st, "piso_multi_bicgstab_ilu")
    return x, (its[0], its[1])


class _LinearSolveFn(torch.autograd.Function):
    """solve_call of diffpiso/linear_solver.py:163-175: gradient only w.r.t. the right-hand side, obtained by solving with
    the transposed matrix (same initial guess), multiplied by (1 - warn)."""

    @staticmethod
    def forward(ctx, rhs, values, row_ptr, col_indices, x0, solver, nx, ny, transpose, warn, negate=False):
        tol = _scalar(solver.accuracy)
        x, its = multi_bicgstab_ilu_native(values, row_ptr, col_indices, rhs, x0, nx, ny, tol, solver.max_iterations,
                                           transpose, solver.band_rows, warn, solver.slab_comm, negate=negate)
        solver.last_iterations = its
        solver.stats["solves"] += 1
        solver.stats["iterations"] += max(its)
        # the reference's backward op receives the SAME warn buffer the forward op aliased and mutated
        # (linear_solver.py:165-173, multi_bicgstab_ilu_linear_solve_op.cc:136-140): a forward warning zeroes the gradient
        ctx.save_for_backward(values, row_ptr, col_indices, x0, warn.clone())
        ctx.meta = (solver, nx, ny, transpose, negate)
        return x.to(torch.float32), warn.to(torch.float32)

    @staticmethod
    def backward(ctx, ds, dw):
        values, row_ptr, col_indices, x0, warn_fwd = ctx.saved_tensors
        solver, nx, ny, transpose, negate = ctx.meta
        warn_b = warn_fwd.clone()
        tol = _scalar(solver.accuracy)
        df, its = multi_bicgstab_ilu_native(values, row_ptr, col_indices, ds.to(values.dtype), x0, nx, ny, tol,
                                            solver.max_iterations, not transpose, solver.band_rows, warn_b, solver.slab_comm, negate=negate)
        solver.last_adjoint_iterations = its
        solver.stats["adjoint_solves"] += 1
        solver.stats["adjoint_iterations"] += max(its)
        df = df.to(torch.float32) * (1.0 - warn_b.to(torch.float32)[0])
        return df, None, None, None, None, None, None, None, None, None, None


class LinearSolverCudaMultiBicgstabILU(LinearSolver):
    """diffpiso/linear_solver.py:113-178.  `accuracy` may be a float or a 0-d/1-element tensor (the reference accepts a
    placeholder, lid_driven_cavity_2d.py:12-13) and may be re-assigned between steps.
    band_rows: preconditioner block height of the MI355X engine (0 = automatic, < 0 = one block); not in the reference."""

    def __init__(self, accuracy=1e-5, max_iterations=2000, cast_to_double=False, band_rows=0):
        LinearSolver.__init__(self, "HIP dual iLU-preconditioned BiCGStab solve", supported_devices=("GPU",),
                              supports_guess=True, supports_batch=False, solver_type="iterative", input_format="csr")
        self.max_iterations = max_iterations
        self.cast_to_double = cast_to_double
        self.accuracy = accuracy
        self.band_rows = band_rows
        self.slab_comm = None        # distributed.SlabCommunicator: cut every solve into y-slabs over the ranks
        self.last_iterations = None
        self.last_adjoint_iterations = None
        self.stats = dict(solves=0, iterations=0, adjoint_solves=0, adjoint_iterations=0)   # cumulative (max over u, v per solve)

    def solve(self, matrix_values, row_ptr, col_indices, rhs, staggered_shape, initial_guess=None, offset=0,
              transpose=False, unrolling_step=0, warn=None, negate=False):
        """negate (not in the reference): the system matrix is -matrix_values.  The reference's step passes `-matrix_values`
        (piso_tf.py:41) - a pass over the whole value array per step; `piso_step` here passes the values and this flag instead."""
        dt = torch.float64 if self.cast_to_double else torch.float32
        values = matrix_values.reshape(-1).to(dt)
        flat_rhs = rhs.reshape(-1)
        ny, nx = int(staggered_shape[1]) - 1, int(staggered_shape[2]) - 1
        n_tot = (nx + 1) * ny + nx * (ny + 1)
        if initial_guess is None:
            flat_x = torch.zeros(n_tot, dtype=dt, device=flat_rhs.device)
        else:
            flat_x = initial_guess.reshape(-1).detach().to(dt)
        if warn is None:
            warn = torch.zeros(1, dtype=torch.uint8, device=flat_rhs.device)
        elif warn.dtype != torch.uint8:
            warn = (warn != 0).to(torch.uint8)
        sol, w = _LinearSolveFn.apply(flat_rhs, values.detach(), row_ptr.reshape(-1), col_indices.reshape(-1), flat_x, self,
                                      nx, ny, bool(transpose), warn, bool(negate))
        return [sol, w]


LinearSolverHipMultiBicgstabILU = LinearSolverCudaMultiBicgstabILU


class _SingleSolveFn(torch.autograd.Function):
    """solve_call of diffpiso/linear_solver.py:95-107: gradient w.r.t. the right-hand side by the transposed solve."""

    @staticmethod
    def forward(ctx, rhs_pair, values, row_ptr, col_indices, x0, solver, nx, ny, transpose):
        warn = torch.zeros(1, dtype=torch.uint8, device=rhs_pair.device)
        x, its = multi_bicgstab_ilu_native(values, row_ptr, col_indices, rhs_pair, x0, nx, ny, _scalar(solver.accuracy),
                                           solver.max_iterations, transpose, 0, warn)
        solver.last_iterations = its
        solver.last_warn = warn                              # (device byte: NaN input; `solve` looks at it)
        ctx.save_for_backward(values, row_ptr, col_indices, x0)
        ctx.meta = (solver, nx, ny, transpose)
        return x

    @staticmethod
    def backward(ctx, ds):
        values, row_ptr, col_indices, x0 = ctx.saved_tensors
        solver, nx, ny, transpose = ctx.meta
        warn = torch.zeros(1, dtype=torch.uint8, device=ds.device)
        df, _ = multi_bicgstab_ilu_native(values, row_ptr, col_indices, ds.contiguous(), x0, nx, ny, _scalar(solver.accuracy),
                                          solver.max_iterations, not transpose, 0, warn)
        return df, None, None, None, None, None, None, None, None


class LinearSolverCudaBicgstabILU(LinearSolver):
    """diffpiso/linear_solver.py:60-110: the single-matrix ILU(0)-BiCGStab (superseded in the reference by the pair solver; none
    of its scripts constructs it).  The HIP engine solves the two advection matrices of a staggered grid together and takes its
    structure from the grid, so the ONE matrix must be the u or the v matrix of a grid that is named: `staggered_shape`
    ([1, ny+1, nx+1, 2]), `component` ('u' | 'v') and `bool_periodic` ((y, x)) are additional keyword arguments of `solve`.  The
    other component is filled in with a diffusion matrix of the same grid and a zero right-hand side (it converges at once)."""

    _patterns = {}       # (nx, ny, per_x, per_y, device) -> (stand-in pair values, row pointers, columns, nnz): geometry only, built once

    def __init__(self, accuracy=1e-5, max_iterations=2000, raise_on_nan=True):
        LinearSolver.__init__(self, "HIP iLU-preconditioned BiCGStab solve", supported_devices=("GPU",), supports_guess=True,
                              supports_batch=False, solver_type="iterative", input_format="csr")
        self.accuracy = accuracy
        self.max_iterations = max_iterations
        self.last_iterations = None
        self.last_warn = None           # the pair solver's warning byte of the last solve (1: NaN in the matrix / right-hand side / guess)
        self.raise_on_nan = raise_on_nan

    @classmethod
    def _pattern(cls, nx, ny, per_x, per_y, dev):
        """The pair's pattern and a well-posed stand-in for the other component (diffusion + identity on a resting fluid), cached per
        grid: it depends on (nx, ny, periodicity) only, and checking a caller's pattern against it costs two host synchronisations."""
        from .piso import assemble_from_padded
        key = (nx, ny, per_x, per_y, str(dev))
        hit = cls._patterns.get(key)
        if hit is None:
            n_u, n_v = (nx + 1) * ny, nx * (ny + 1)
            pad = torch.zeros((ny + 2) * (nx + 3) + (ny + 3) * (nx + 2), dtype=torch.float32, device=dev)
            val, rp, col, _, nnz = assemble_from_padded(pad, nx, ny, (1.0, 1.0), per_x, per_y, torch.zeros(n_u + n_v, dtype=torch.uint8, device=dev),
                                                        torch.ones((ny + 2) * (nx + 2), dtype=torch.float32, device=dev), 1.0, None, 1.0)
            if len(cls._patterns) > 8:
                cls._patterns.clear()
            hit = cls._patterns[key] = (-val, rp, col, (int(nnz[0]), int(nnz[1])), set())      # (piso_step hands the solver -matrix_values, piso_tf.py:41)
        return hit

    def solve(self, matrix_values, row_ptr, col_indices, rhs, initial_guess=None, offset=0, transpose=False,
              staggered_shape=None, component=None, bool_periodic=(False, False)):
        if staggered_shape is None or component not in ("u", "v"):
            raise NotImplementedError("LinearSolverCudaBicgstabILU.solve: the MI355X engine takes the matrix structure from the staggered grid - "
                                      "pass staggered_shape=[1, ny+1, nx+1, 2], component='u'|'v' (and bool_periodic), or use "
                                      "LinearSolverCudaMultiBicgstabILU, which is what the reference's scripts use")
        ny, nx = int(staggered_shape[1]) - 1, int(staggered_shape[2]) - 1
        n_u, n_v = (nx + 1) * ny, nx * (ny + 1)
        dev = rhs.device
        per_y, per_x = bool(bool_periodic[0]), bool(bool_periodic[1])
        val, rp, col, (nnz_u, nnz_v), checked = self._pattern(nx, ny, per_x, per_y, dev)
        lo, hi, r0, rows = (0, nnz_u, 0, n_u) if component == "u" else (nnz_u, nnz_u + nnz_v, n_u + 1, n_v)
        mv = matrix_values.reshape(-1).to(torch.float32)
        if mv.numel() != hi - lo or int(row_ptr.numel()) != rows + 1 or int(col_indices.numel()) != hi - lo:
            raise ValueError("LinearSolverCudaBicgstabILU: the matrix is not the %s matrix of a %d x %d staggered grid (%d values, expected %d)"
                             % (component, nx, ny, mv.numel(), hi - lo))
        # (a caller's pattern arrays are compared with the grid's ONCE per pair of tensors: the comparison synchronises the host)
        pat_key = (component, row_ptr.data_ptr(), col_indices.data_ptr(), int(row_ptr._version), int(col_indices._version))
        if pat_key not in checked:
            if not (torch.equal(row_ptr.reshape(-1).to(torch.int32), rp[r0:r0 + rows + 1]) and torch.equal(col_indices.reshape(-1).to(torch.int32), col[lo:hi])):
                raise ValueError("LinearSolverCudaBicgstabILU: row pointers / column indices are not the 5-point pattern of the grid")
            if len(checked) > 16:
                checked.clear()
            checked.add(pat_key)
        val = val.clone()
        val[lo:hi] = mv
        flat_rhs = rhs.reshape(-1).to(torch.float32)
        off = 0 if component == "u" else n_u
        x0 = torch.zeros(n_u + n_v, dtype=torch.float32, device=dev)
        if initial_guess is not None:
            x0[off:off + rows] = initial_guess.reshape(-1).detach().to(torch.float32)
        embed = torch.zeros(n_u + n_v, dtype=torch.float32, device=dev)
        pair_rhs = embed.index_put((torch.arange(off, off + rows, device=dev),), flat_rhs)          # (differentiable w.r.t. rhs)
        sol = _SingleSolveFn.apply(pair_rhs, val, rp, col, x0, self, nx, ny, bool(transpose))
        if self.raise_on_nan and int(self.last_warn.item()) != 0:
            # (the pair solver's failure handling is the reference's - NaN input: warning byte, zero solution; this class has no `warn`
            # output to hand it to, so it says so instead of returning zeros silently)
            raise N.PisoNativeError("LinearSolverCudaBicgstabILU: NaN in the matrix, the right-hand side or the initial guess (the solver's warning byte is set)")
        return sol[off:off + rows]


def mat_vec_mul_csr(matrix_values, row_pointers, column_indices, staggered_field, staggered_shape):
    """diffpiso/linear_solver.py:181-196: [M_u u, M_v v] of the two advection matrices (CSR pair as `advection_matrix_cuda` returns
    it) as a staggered tensor - the HIP gather / segment-sum product (`piso_csr_matvec_f32`)."""
    from .grids import StaggeredGrid
    from .piso import _CsrMatVec
    from .stencils import flatten_staggered_data, stagger_flattened_data
    ny, nx = int(staggered_shape[1]) - 1, int(staggered_shape[2]) - 1
    field = staggered_field if isinstance(staggered_field, StaggeredGrid) else StaggeredGrid(staggered_field)
    flat = flatten_staggered_data(field, coord_flip=True)
    prod = _CsrMatVec.apply(flat, matrix_values.reshape(-1).to(torch.float32), row_pointers.reshape(-1), column_indices.reshape(-1), nx, ny)
    return stagger_flattened_data(prod, tuple(int(v) for v in staggered_shape), coord_flip=True)


def print_residual(matrix_values, row_pointers, column_indices, staggered_field, staggered_shape, rhs):
    """diffpiso/linear_solver.py:198-206: prints sum |M x - rhs| and returns the residual (flat, in the reference's default
    flatten order)."""
    from .grids import StaggeredGrid
    from .stencils import flatten_staggered_data
    prod = mat_vec_mul_csr(matrix_values, row_pointers, column_indices, staggered_field, staggered_shape)
    residual = flatten_staggered_data(StaggeredGrid(prod)) - rhs.reshape(-1)
    print("linsolve residual", float(residual.abs().sum()))
    return residual


# ------------------------------------------------------------------------------------------------------------------
class PoissonSolver(object):
    """PhiFlow/phi/physics/pressuresolver/solver_api.py:10-38 (attribute holder)."""

    def __init__(self, name, supported_devices, supports_guess, supports_loop_counter, supports_continuous_masks):
        self.name = name
        self.supported_devices = supported_devices
        self.supports_guess = supports_guess
        self.supports_loop_counter = supports_loop_counter
        self.supports_continuous_masks = supports_continuous_masks

    def __repr__(self):
        return self.name


def laplace_matrix_native(nx, ny, active, accessible, a0_vfirst, dtype, sharding=None):
    """[ny nx][5] pressure matrix; sharding (the slab-decomposed step): masks and a0 hold the rank's stored rows, the matrix its
    OWNED rows [nyl nx][5] - what the slab CG takes."""
    if sharding is None:
        L = torch.empty(nx * ny * 5, dtype=dtype, device=a0_vfirst.device)
        fn = N.lib.piso_laplace_matrix_f64 if dtype == torch.float64 else N.lib.piso_laplace_matrix_f32
        N.check(fn(nx, ny, N.ptr(active), N.ptr(accessible), N.ptr(a0_vfirst.contiguous()), N.ptr(L), N.stream_ptr()),
                "piso_laplace_matrix")
        return L
    L = torch.empty(nx * sharding.nyl * 5, dtype=dtype, device=a0_vfirst.device)
    fn = N.lib.piso_laplace_matrix_f64_slab if dtype == torch.float64 else N.lib.piso_laplace_matrix_f32_slab
    N.check(fn(nx, ny, N.ptr(active), N.ptr(accessible), N.ptr(a0_vfirst.contiguous()), N.ptr(L), N.stream_ptr(), sharding.slab_ptr),
            "piso_laplace_matrix_slab")
    return L


class DeferredInt(object):
    """An iteration count that still lives on the device (asynchronous solves, piso_cg_solve_async_*): behaves like an int and
    reads its value - ONE synchronising copy - the first time somebody looks at it.  Sums of such counts (solver.stats) stay
    deferred, so a training loop that never looks never waits."""
    __slots__ = ("_base", "_pending")

    def __init__(self, base=0, pending=()):
        self._base, self._pending = int(base), list(pending)

    def device_tensor(self):
        """The count as an int32 device tensor [1] (the reference's `iterations` output) without a host round trip."""
        if len(self._pending) == 1 and self._base == 0:
            return self._pending[0]
        dev = self._pending[0].device if self._pending else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        return torch.tensor([int(self)], dtype=torch.int32, device=dev)

    def __int__(self):
        if self._pending:
            self._base += int(torch.stack([t.reshape(()) for t in self._pending]).sum().item())
            self._pending = []
        return self._base

    __index__ = __int__

    def __add__(self, other):
        if isinstance(other, DeferredInt):
            out = DeferredInt(self._base + other._base, self._pending + other._pending)
        else:
            out = DeferredInt(self._base + int(other), self._pending)
        if len(out._pending) > 64:          # (a long run that never looks: fold the pending counts on the device, still no wait)
            out._pending = [torch.stack([t.reshape(()) for t in out._pending]).sum().to(torch.int64)]
        return out

    __radd__ = __add__

    def __float__(self): return float(int(self))
    def __bool__(self): return int(self) != 0
    def __hash__(self): return hash(int(self))
    def __repr__(self): return repr(int(self))
    def __str__(self): return str(int(self))
    def __format__(self, spec): return format(int(self), spec)
    def __eq__(self, o): return int(self) == o
    def __ne__(self, o): return int(self) != o
    def __lt__(self, o): return int(self) < o
    def __le__(self, o): return int(self) <= o
    def __gt__(self, o): return int(self) > o
    def __ge__(self, o): return int(self) >= o
    def __sub__(self, o): return int(self) - o
    def __rsub__(self, o): return o - int(self)
    def __mul__(self, o): return int(self) * o
    __rmul__ = __mul__
    def __mod__(self, o): return int(self) % o
    def __truediv__(self, o): return int(self) / o
    def __rtruediv__(self, o): return o / int(self)
    def __floordiv__(self, o): return int(self) // o
    def __neg__(self): return -int(self)
    def __abs__(self): return abs(int(self))


class _Stats(dict):
    """Cumulative solver counters.  Counts of asynchronous solves are added as DeferredInt (no host wait); whatever LEAVES the
    solver through the mapping interface - solver.stats["iterations"], dict(solver.stats), .items() - is a plain int (so that
    json.dumps, numpy and torch see numbers), at the price of the one synchronising read that looking costs."""

    def add(self, key, value):
        dict.__setitem__(self, key, dict.__getitem__(self, key) + value)

    @staticmethod
    def _plain(v):
        return int(v) if isinstance(v, DeferredInt) else v

    def __getitem__(self, key):
        return self._plain(dict.__getitem__(self, key))

    def get(self, key, default=None):
        return self._plain(dict.get(self, key, default))

    def items(self):
        return [(k, self._plain(v)) for k, v in dict.items(self)]

    def values(self):
        return [self._plain(v) for v in dict.values(self)]

    def copy(self):
        return dict(self.items())

    def keys(self):
        return dict.keys(self)

    def __iter__(self):
        return dict.__iter__(self)


class _PlainCount(object):
    """Descriptor of `last_iterations` / `last_adjoint_iterations`: stored as handed in (possibly a DeferredInt), read as int."""

    def __init__(self, name):
        self.name = "_" + name

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        v = getattr(obj, self.name, None)
        if isinstance(v, DeferredInt):
            v = int(v)
            setattr(obj, self.name, v)
        return v

    def __set__(self, obj, value):
        setattr(obj, self.name, value)


_ASYNC_MAX_CELLS = 4608          # csrc/cg_tiny.h: kTinyMaxCells (the library answers PISO_ERR_NEEDS_HOST for anything it cannot run in one launch)


def cg_solve_native(nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset):
    """-> (x, iterations).  Grids the library solves in ONE launch (tiny grids: the lid-driven cavity) are queued without waiting
    for the result; `iterations` is then a DeferredInt."""
    dt = L.dtype
    div = div.reshape(-1).to(dt).contiguous()
    x = torch.empty_like(div)
    elem = 8 if dt == torch.float64 else 4
    ws = N.workspace(N.lib.piso_cg_workspace_bytes(nx, ny, elem), div.device, "cg")
    if nx * ny <= _ASYNC_MAX_CELLS:
        it_dev = torch.empty(1, dtype=torch.int32, device=div.device)
        fn = N.lib.piso_cg_solve_async_f64 if dt == torch.float64 else N.lib.piso_cg_solve_async_f32
        st = fn(nx, ny, int(per_x), int(per_y), N.ptr(L), N.ptr(div), N.ptr(x), C.c_float(accuracy), int(max_iterations),
                int(bool(rank_deficient)), int(residual_reset), N.ptr(it_dev), N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr())
        if st == 0:
            return x, DeferredInt(0, [it_dev])
        if st != N.ERR_NEEDS_HOST:
            N.check(st, "piso_cg_solve_async")
    it = C.c_int(0)
    fn = N.lib.piso_cg_solve_f64 if dt == torch.float64 else N.lib.piso_cg_solve_f32
    st = fn(nx, ny, int(per_x), int(per_y), N.ptr(L), N.ptr(div), N.ptr(x), C.c_float(accuracy), int(max_iterations),
            int(bool(rank_deficient)), int(residual_reset), C.byref(it), N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr())
    N.check(st, "piso_cg_solve")
    return x, it.value


class _PressureSolveFn(torch.autograd.Function):
    """psolve of diffpiso/piso_cuda_pressure_solver.py:90-109: gradient only w.r.t. the divergence = the same CG solve
    applied to the incoming gradient (the operator is symmetric)."""

    @staticmethod
    def forward(ctx, divergence, L, solver, nx, ny, per_x, per_y, rank_deficient, guess=None):
        # (`guess`: only a solver that asks for one is handed one - PisoPressureSolverMultigrid(use_guess=True); never differentiated)
        if guess is None:
            x, it = solver._cg(nx, ny, per_x, per_y, L, divergence, _scalar(solver.accuracy), solver.max_iterations,
                               rank_deficient, solver.residual_reset)
        else:
            x, it = solver._cg(nx, ny, per_x, per_y, L, divergence, _scalar(solver.accuracy), solver.max_iterations,
                               rank_deficient, solver.residual_reset, x0=guess)
        solver.last_iterations = it
        solver.stats.add("solves", 1)
        solver.stats.add("iterations", it)
        ctx.save_for_backward(L)
        ctx.meta = (solver, nx, ny, per_x, per_y, rank_deficient, divergence.shape)
        iterations = it.device_tensor() if isinstance(it, DeferredInt) else torch.tensor([it], dtype=torch.int32, device=divergence.device)
        return x.reshape(divergence.shape).to(torch.float32), iterations

    @staticmethod
    def backward(ctx, dp, di):
        (L,) = ctx.saved_tensors
        solver, nx, ny, per_x, per_y, rank_deficient, shape = ctx.meta
        g, it = solver._cg(nx, ny, per_x, per_y, L, dp.reshape(-1), _scalar(solver.accuracy), solver.max_iterations,
                           rank_deficient, solver.residual_reset)
        solver.last_adjoint_iterations = it
        solver.stats.add("adjoint_solves", 1)
        solver.stats.add("adjoint_iterations", it)
        return g.reshape(shape).to(torch.float32), None, None, None, None, None, None, None, None


class PisoPressureSolverCudaCustom(PoissonSolver):
    """diffpiso/piso_cuda_pressure_solver.py:36-114."""
    last_iterations = _PlainCount("last_iterations")                   # (int on read; a tiny grid's asynchronous solve hands in a DeferredInt)
    last_adjoint_iterations = _PlainCount("last_adjoint_iterations")

    def __init__(self, dx, accuracy=1e-5, max_iterations=2000, residual_reset=10, randomized_restarts=0,
                 cast_to_double=True):
        PoissonSolver.__init__(self, "HIP Conjugate Gradient", supported_devices=("GPU",), supports_loop_counter=False,
                               supports_guess=True, supports_continuous_masks=False)
        self.accuracy = accuracy
        self.max_iterations = max_iterations
        self.dx = dx
        self.scaling_field = None
        self.solve_count = 0.001
        self.laplace_rank_deficient = None
        self.residual_reset = residual_reset
        assert randomized_restarts >= 0
        if randomized_restarts != 0:
            raise NotImplementedError("randomized_restarts > 0 is never used by the reference's scripts "
                                      "(combined_training_integrated.py:487) and is not implemented")
        self.randomized_restarts = randomized_restarts
        self.cast_to_double = cast_to_double
        self.last_iterations = None
        self.last_adjoint_iterations = None
        self.slab_comm = None        # distributed.SlabCommunicator: decompose the CG into y-slabs over the ranks (fp64 only)
        self.stats = _Stats(solves=0, iterations=0, adjoint_solves=0, adjoint_iterations=0)   # cumulative; callers may reset

    def _cg(self, nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset):
        if self.slab_comm is not None and self.slab_comm.sharded and L.dtype != torch.float64:
            # (L and div of a sharded step are valid on this rank's rows only: the one-GPU kernel on the whole grid would read garbage)
            raise N.PisoNativeError("the slab-decomposed pressure CG is fp64 only: a sharded step needs cast_to_double=True")
        if self.slab_comm is not None and self.slab_comm.world > 1 and L.dtype == torch.float64:
            from .distributed import cg_solve_slab, cg_solve_slab_local
            if self.slab_comm.sharded:       # slab-decomposed STEP: L holds the rank's owned rows, div its stored rows; the result stays there
                sh = self.slab_comm.step_sharding
                d_loc = sh.owned_cells(div.reshape(-1).to(torch.float64)).reshape(-1).contiguous()
                x_loc, it = cg_solve_slab_local(self.slab_comm, nx, sh.nyl, per_x, per_y, L, d_loc, accuracy, max_iterations, rank_deficient,
                                                residual_reset, gather=False)
                x = torch.zeros(sh.n_cells, dtype=x_loc.dtype, device=x_loc.device)
                sh.owned_cells(x).copy_(x_loc.view(sh.nyl, nx))
                return x, it
            return cg_solve_slab(self.slab_comm, nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient,
                                 residual_reset)
        return cg_solve_native(nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset)

    def _laplace(self, nx, ny, active, accessible, a0, dt, sharding):
        """The pressure matrix of one solve_flat call (PisoPressureSolverMultigrid may hand back the previous call's)."""
        return laplace_matrix_native(nx, ny, active, accessible, a0, dt, sharding)

    def solve(self, scaling_field, divergence, guess, enable_backprop, simulation_physics, offset=0, unrolling_step=0):
        # `guess` is ignored exactly like in the reference (init_with_zeros=True, piso_cuda_pressure_solver.py:95)
        scaling_field = scaling_field if isinstance(scaling_field, StaggeredGrid) else StaggeredGrid(scaling_field)
        a0 = flatten_staggered_data(scaling_field, coord_flip=False).detach().to(torch.float32)   # v first (:70)
        return self.solve_flat(a0, divergence, simulation_physics, unrolling_step=unrolling_step)

    def _guess_for_solve(self, guess, divergence):
        return None                                          # (init_with_zeros=True; PisoPressureSolverMultigrid(use_guess=True) overrides)

    def solve_flat(self, a0_vfirst, divergence, simulation_physics, unrolling_step=0, guess=None):
        """`solve` with the face coefficients already in the op's layout (flat, v faces first, :70); used by the fused step."""
        guess = self._guess_for_solve(guess, divergence)
        dt = torch.float64 if self.cast_to_double else torch.float32
        sharding = getattr(simulation_physics, "sharding", None)
        ny, nx = (int(divergence.shape[1]), int(divergence.shape[2])) if sharding is None else (sharding.ny, sharding.nx)
        dev = divergence.device
        a0 = a0_vfirst
        if self.laplace_rank_deficient is None:                                     # :84-87
            # (looked at once per solver, on the host: the whole-grid masks of a sharded simulation never go to the device as a whole)
            a, c = (as_tensor(m, dtype=torch.float32, device="cpu") for m in (simulation_physics.accessible_mask, simulation_physics.active_mask))
            prod = a * c + (1 - a) * (1 - c)
            prod = torch.prod(prod[0, 0, 1:-1, 0]) * torch.prod(prod[0, -1, 1:-1, 0]) * \
                torch.prod(prod[0, 1:-1, 0, 0]) * torch.prod(prod[0, 1:-1, -1, 0])
            self.laplace_rank_deficient = bool(prod.item() != 0)
        rank_def = self.laplace_rank_deficient
        if isinstance(rank_def, torch.Tensor):
            rank_def = bool(rank_def.reshape(-1)[0].item())
        if (sharding is not None) != bool(self.slab_comm is not None and self.slab_comm.sharded):
            raise ValueError("pressure solve: the simulation's `sharding` and this solver's slab communicator disagree")
        if sharding is None:
            active = simulation_physics.active_mask_tensor(dev).reshape(-1).contiguous()
            accessible = simulation_physics.accessible_mask_tensor(dev).reshape(-1).contiguous()
        else:
            loc = sharding.sim_tensors(simulation_physics, dev)
            active, accessible = loc["active"], loc["accessible"]
        L = self._laplace(nx, ny, active, accessible, a0, dt, sharding)
        per_y, per_x = [bool(b) for b in simulation_physics.bool_periodic]          # given (y, x), flipped for the op (:95)
        if guess is None:
            pressure, iteration = _PressureSolveFn.apply(divergence, L, self, nx, ny, per_x, per_y, rank_def)
        else:
            pressure, iteration = _PressureSolveFn.apply(divergence, L, self, nx, ny, per_x, per_y, rank_def, guess)
        self.solve_count = self.solve_count + .001
        return pressure, iteration, L


PisoPressureSolverHip = PisoPressureSolverCudaCustom


def _mg_cycle_elem(cycle_dtype):
    """8 / 4 for the two precisions of the multigrid cycle; anything else is refused."""
    if cycle_dtype == torch.float64:
        return 8
    if cycle_dtype == torch.float32:
        return 4
    raise ValueError("cycle_dtype must be torch.float64 or torch.float32 (got %r)" % (cycle_dtype,))


def mg_entry(stem, cycle_dtype):
    """The C entry piso_mg_<stem>_f64 / piso_mg_<stem>_c32_f64 for the precision of the cycle (one-GPU, prepared and slab entries alike)."""
    return getattr(N.lib, "piso_mg_%s%s" % (stem, "_f64" if _mg_cycle_elem(cycle_dtype) == 8 else "_c32_f64"))


def mg_workspace(nx, ny, device, cycle_dtype=torch.float64):
    nbytes = N.lib.piso_mg_workspace_bytes_cycle(nx, ny, _mg_cycle_elem(cycle_dtype))
    if nbytes == 0:
        raise N.PisoNativeError("the multigrid pressure solver needs at least 4 cells in each dimension (got %d x %d); "
                                "use PisoPressureSolverCudaCustom" % (ny, nx))
    return N.workspace(nbytes, device, "mg")


def _mg_guess(x0, div):
    """The guess of a multigrid solve as the library takes it - detached, float64, flat - or the refusal of one that does not fit `div`
    (before any launch)."""
    if not isinstance(x0, torch.Tensor):
        raise TypeError("a multigrid guess must be a tensor (got %s)" % type(x0).__name__)
    if not x0.is_floating_point():
        raise TypeError("a multigrid guess must be a floating-point tensor (got %s)" % x0.dtype)
    if x0.numel() != div.numel():
        raise ValueError("a multigrid guess must have the solution's %d cells (got %d)" % (div.numel(), x0.numel()))
    if x0.device != div.device:
        raise ValueError("a multigrid guess must live on the right-hand side's device %s (got %s)" % (div.device, x0.device))
    return x0.detach().reshape(-1).to(torch.float64).contiguous()


def _mg_x_out(x_out, div):
    if x_out is None:
        return torch.empty_like(div)
    if x_out.dtype != torch.float64 or x_out.numel() != div.numel() or x_out.device != div.device or not x_out.is_contiguous():
        raise ValueError("x_out must be a contiguous float64 tensor of the solution's %d cells on %s" % (div.numel(), div.device))
    return x_out


def mg_solve_native(nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset, sweeps=2, cycle_dtype=torch.float64,
                    x0=None, x_out=None):
    """-> (x, iterations): multigrid-preconditioned CG on the system cg_solve_native solves (csrc/mg.hip; fp64).  cycle_dtype=torch.float32:
    the same fp64 iteration around a float32 V-cycle (csrc/mg_f32.h).  x0: a guess the solve starts from where its residual is below the
    right-hand side, else from zero (csrc/mg_guess.h; N.mg_last_guess() says which); x_out: where the result goes (x0 itself is allowed)."""
    if L.dtype != torch.float64:
        raise N.PisoNativeError("the multigrid pressure solver is fp64 only; use the plain CG (cg_solve_native) for float32")
    solve, solve_guess = mg_entry("pcg_solve", cycle_dtype), mg_entry("pcg_solve_guess", cycle_dtype)
    div = div.reshape(-1).to(torch.float64).contiguous()
    guess = None if x0 is None else (x0 if x0 is x_out else _mg_guess(x0, div))
    x = _mg_x_out(x_out, div)
    ws = mg_workspace(nx, ny, div.device, cycle_dtype)
    it = C.c_int(0)
    head = (nx, ny, int(per_x), int(per_y), N.ptr(L), N.ptr(div))
    tail = (N.ptr(x), C.c_float(accuracy), int(max_iterations), int(bool(rank_deficient)), int(residual_reset), int(sweeps), C.byref(it), N.ptr(ws),
            C.c_size_t(ws.numel()), N.stream_ptr())
    if guess is None:
        st = solve(*(head + tail))
    else:
        st = solve_guess(*(head + (N.ptr(guess),) + tail))
    N.check(st, "piso_mg_pcg_solve")
    return x, it.value


def mg_vcycle_native(nx, ny, per_x, per_y, L, r, sweeps=2, cycle_dtype=torch.float64):
    """z = M^-1 r: one V-cycle of the multigrid preconditioner (tests, measurements); float64 in and out in either precision of the cycle."""
    fn = mg_entry("vcycle", cycle_dtype)
    r = r.reshape(-1).to(torch.float64).contiguous()
    z = torch.empty_like(r)
    ws = mg_workspace(nx, ny, r.device, cycle_dtype)
    N.check(fn(nx, ny, int(per_x), int(per_y), N.ptr(L), N.ptr(r), N.ptr(z), int(sweeps), N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr()),
            "piso_mg_vcycle")
    return z


def mg_level_native(nx, ny, per_x, per_y, L, level, cycle_dtype=torch.float64):
    """-> (A_level [nyl * nxl, 5], nxl, nyl), or None past the coarsest level (tests); the float32 cycle's entries come widened to float64."""
    fn = mg_entry("level", cycle_dtype)
    ws = mg_workspace(nx, ny, L.device, cycle_dtype)
    nxl, nyl = C.c_int(0), C.c_int(0)
    if fn(nx, ny, int(per_x), int(per_y), N.ptr(L), int(level), C.byref(nxl), C.byref(nyl), None, N.ptr(ws), C.c_size_t(ws.numel()),
          N.stream_ptr()) != 0:
        return None
    out = torch.empty((nxl.value * nyl.value, 5), dtype=torch.float64, device=L.device)
    N.check(fn(nx, ny, int(per_x), int(per_y), N.ptr(L), int(level), C.byref(nxl), C.byref(nyl), N.ptr(out), N.ptr(ws), C.c_size_t(ws.numel()),
               N.stream_ptr()), "piso_mg_level")
    return out, nxl.value, nyl.value


class MgHierarchy(object):
    """A multigrid hierarchy built once and solved on any number of times (csrc/mg_prepared.h).  Owns `buf`, a byte tensor of its own of
    piso_mg_hierarchy_bytes - never the shared N.workspace(..., "mg"), which any other solver instance may overwrite: everything that depends
    on the matrix only (the fp64 level 0 and, for cycle_dtype=torch.float32, the float32 levels too).  After prepare(L) it keeps a tensor
    that shares L's storage alive, so that the recorded pointer cannot be handed to another tensor while the record is compared, and records
    `key` = (data_ptr, _version, nx, ny, per_x, per_y, rank_deficient, cycle_dtype, device).  What the key cannot see is a matrix overwritten
    through a raw pointer (a kernel of the library writing into L, a ctypes call): neither the pointer nor the version changes then."""

    def __init__(self, nx, ny, per_x, per_y, rank_deficient, cycle_dtype=torch.float64, device=None):
        self.elem = _mg_cycle_elem(cycle_dtype)
        self.nx, self.ny, self.per_x, self.per_y = int(nx), int(ny), bool(per_x), bool(per_y)
        self.rank_deficient, self.cycle_dtype = bool(rank_deficient), cycle_dtype
        nbytes = N.lib.piso_mg_hierarchy_bytes(self.nx, self.ny, self.elem)
        if nbytes == 0:
            raise N.PisoNativeError("the multigrid pressure solver needs at least 4 cells in each dimension (got %d x %d); "
                                    "use PisoPressureSolverCudaCustom" % (ny, nx))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.buf[:256].zero_()                      # (memory the allocator hands back may still hold the header of a hierarchy that was freed)
        self.matrix = None
        self.key = None

    def scratch(self):
        return N.workspace(N.lib.piso_mg_solve_workspace_bytes(self.nx, self.ny, self.elem), self.device, "mg_solve")

    def prepare(self, L):
        """Builds the hierarchy of L [N][5] into the buffer; the library's three refusals leave it without a valid header."""
        if L.dtype != torch.float64:
            raise N.PisoNativeError("the multigrid pressure solver is fp64 only; use the plain CG (cg_solve_native) for float32")
        self.matrix, self.key = None, None
        ws = self.scratch()
        fn = mg_entry("prepare", self.cycle_dtype)
        N.check(fn(self.nx, self.ny, int(self.per_x), int(self.per_y), N.ptr(L), int(self.rank_deficient), N.ptr(self.buf), C.c_size_t(self.buf.numel()),
                   N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr()), "piso_mg_prepare")
        self.matrix = L.detach()
        self.key = self.key_of(L, self.nx, self.ny, self.per_x, self.per_y, self.rank_deficient, self.cycle_dtype)
        return self

    @staticmethod
    def key_of(L, nx, ny, per_x, per_y, rank_deficient, cycle_dtype):
        return (L.data_ptr(), L._version, int(nx), int(ny), bool(per_x), bool(per_y), bool(rank_deficient), cycle_dtype, L.device)


def mg_prepare_native(nx, ny, per_x, per_y, L, rank_deficient, cycle_dtype=torch.float64):
    """-> MgHierarchy of L, ready for mg_solve_prepared_native / mg_vcycle_prepared_native."""
    return MgHierarchy(nx, ny, per_x, per_y, rank_deficient, cycle_dtype, L.device).prepare(L)


def mg_solve_prepared_native(h, div, accuracy, max_iterations, residual_reset, sweeps=2):
    """-> (x, iterations) of mg_solve_native on the matrix `h` was prepared from, bit for bit, without the set-up and its host look."""
    return mg_solve_prepared_guess_native(h, div, None, accuracy, max_iterations, residual_reset, sweeps)


def mg_solve_prepared_guess_native(h, div, x0, accuracy, max_iterations, residual_reset, sweeps=2, x_out=None):
    """mg_solve_prepared_native from the guess `x0` (None: no guess), x and count of mg_solve_native(..., x0=x0) bit for bit; x_out as there."""
    div = div.reshape(-1).to(torch.float64).contiguous()
    guess = None if x0 is None else (x0 if x0 is x_out else _mg_guess(x0, div))
    x = _mg_x_out(x_out, div)
    ws = h.scratch()
    it = C.c_int(0)
    head = (h.nx, h.ny, int(h.per_x), int(h.per_y), N.ptr(h.buf), C.c_size_t(h.buf.numel()), N.ptr(div))
    tail = (N.ptr(x), C.c_float(accuracy), int(max_iterations), int(h.rank_deficient), int(residual_reset), int(sweeps), C.byref(it), N.ptr(ws),
            C.c_size_t(ws.numel()), N.stream_ptr())
    if guess is None:
        st = mg_entry("pcg_solve_prepared", h.cycle_dtype)(*(head + tail))
    else:
        st = mg_entry("pcg_solve_prepared_guess", h.cycle_dtype)(*(head + (N.ptr(guess),) + tail))
    N.check(st, "piso_mg_pcg_solve_prepared")
    return x, it.value


def mg_vcycle_prepared_native(h, r, sweeps=2):
    """z = M^-1 r of mg_vcycle_native on a prepared hierarchy, bit for bit."""
    r = r.reshape(-1).to(torch.float64).contiguous()
    z = torch.empty_like(r)
    ws = h.scratch()
    fn = mg_entry("vcycle_prepared", h.cycle_dtype)
    N.check(fn(h.nx, h.ny, int(h.per_x), int(h.per_y), N.ptr(h.buf), C.c_size_t(h.buf.numel()), N.ptr(r), N.ptr(z), int(sweeps), N.ptr(ws),
               C.c_size_t(ws.numel()), N.stream_ptr()), "piso_mg_vcycle_prepared")
    return z


class PisoPressureSolverMultigrid(PisoPressureSolverCudaCustom):
    """Opt-in pressure solver: CG preconditioned by one multigrid V-cycle per iteration (csrc/mg.hip).  The reference has no such
    solver.  It solves the system PisoPressureSolverCudaCustom solves, to the same stopping rule (max|r| < accuracy), in tens of
    iterations where plain CG needs thousands, so converged solves (tight `accuracy`, adjoints included) become affordable on large
    grids; the two solvers agree to the tolerance they are run at, not bit for bit, and `max_iterations` counts multigrid
    iterations here (a few dozen suffice).  Measured faster than the plain solver from 256 x 256 cells up (3x at 256^2, 25 - 77x at
    2048^2; DESIGN.md 3.7 has the table); not measured on smaller grids, where the plain solver's one-workgroup kernels have no
    launch or host round trip per iteration and are the better choice.  fp64 only: cast_to_double=False is refused.
    cycle_dtype=torch.float32 (opt-in) keeps that fp64 iteration - x, r, p, q, the operator, every sum, the stopping rule - and runs the
    V-cycle, hierarchy included, in float32 (csrc/mg_f32.h): the same counts or a few more iterations (DESIGN.md 3.7 has both tables), r is
    not scaled, so a residual beyond float32's range never converges and tolerances below ~1e-30 are outside that mode.  It runs on y-slabs
    too (csrc/mg_slab_f32.h: the sharded levels and the gathered rows of level g are float32, so the halo rows and the gather carry half the
    bytes in the same number of collectives; the outer iteration stays fp64 and sharded) - except where the plan replicates the whole cycle
    (g = 0: the whole grid within the gather limit of 8192 cells), which has nothing to gain from float32 and is refused with a message
    naming cycle_dtype=torch.float64.
    With a distributed.SlabCommunicator of more than one rank in `slab_comm` the solve is cut into y-slabs like the plain solver's (csrc/mg_slab.h:
    fine levels sharded with halo rows, the levels of at most 8192 cells replicated; ny / ranks must be divisible by 2^g, g the first replicated
    level, else the call is refused and names the plain solver); with `.sharded` L holds the rank's rows and the result stays on them.  Anything
    else in `slab_comm` is refused.
    The fluid cells must be CONNECTED: a pocket of fluid enclosed by solid cells is not detected, and the solve then runs to `max_iterations`
    without converging (as the plain solver does).  Grids whose hierarchy stops after 0 or 1 coarsenings (a dimension below 8 or 16 cells
    next to a long one) are preconditioned poorly: ~200 iterations instead of tens.
    reuse_hierarchy=True (opt-in, one GPU) separates set-up from solve: the solver keeps ONE MgHierarchy, the last one built, and solves on it
    whenever the incoming matrix is the tensor it was built from (same storage pointer and version, grid, periodic flags, rank_deficient,
    cycle_dtype, device), and solve_flat keeps the last (a0, masks, nx, ny) -> L the same way, so the two correctors of a step and their
    adjoints share one matrix tensor, one hierarchy and one host look where the default builds four.  Results are those of the default bit
    for bit.  The one thing the key cannot see is a matrix (or a0) overwritten through a raw pointer, outside torch's version counter: call
    drop_hierarchy() after that.  The cache holds memory until it is dropped or replaced: the matrix [N][5] fp64 and a0, the fp64 level 0
    (48 bytes a cell) and the coarser levels (fp64 cycle: 16 more) or, in float32 mode, the float32 levels (32 more).  `stats` counts
    hierarchy_builds, hierarchy_reuses and laplace_builds in either mode.  Refused (naming reuse_hierarchy=False) with a slab communicator
    in use: sharded hierarchies are not kept.
    use_guess=True (opt-in, one GPU) starts a forward solve from the guess it is handed instead of from zero (csrc/mg_guess.h): `solve(...,
    guess, ...)` and `solve_flat(..., guess=...)` pass it on - detached and cast to float64, so no gradient flows through it; a tensor of
    another size or device is refused before any launch - piso_step hands corrector 1 and 2 the `pressure_inc1` / `pressure_inc2` it
    receives, and run_piso_steps / unroll_piso_steps hand step n's increments to step n + 1.  The device keeps a guess only where
    max|b' - L x0| < max|b'| (b' the right-hand side the iteration sees): in a start-up transient the previous increment is a worse start
    than zero, and such a guess, like one holding a NaN, becomes the solve from zero, bit for bit.  A settled flow saves 1 - 2 of its 3 - 6
    iterations a solve (DESIGN.md 3.7 has the tables and what two more launches cost a small grid).  With a guess the result agrees with the
    default's to the tolerance the solve is run at, not bit for bit.  `stats` of a solver built with the option counts guesses_accepted and
    guesses_rejected.  The adjoint solve always starts from zero (the previous adjoint is no better a start).  Works with reuse_hierarchy
    and both cycle_dtypes; refused (naming use_guess=False) with a slab communicator in use.  Off, `guess` is ignored as the plain solver
    ignores it.
    Forward and adjoint solves, `last_iterations`, `stats` and SimulationParameters(pressure_solver=...) work as with the plain
    solver."""

    def __init__(self, dx, accuracy=1e-5, max_iterations=2000, residual_reset=10, randomized_restarts=0, cast_to_double=True,
                 smoothing_sweeps=2, cycle_dtype=torch.float64, reuse_hierarchy=False, use_guess=False):
        if not cast_to_double:
            raise ValueError("PisoPressureSolverMultigrid is fp64 only (cast_to_double=True); use PisoPressureSolverCudaCustom for float32")
        if not 1 <= int(smoothing_sweeps) <= 8:
            raise ValueError("smoothing_sweeps must be 1 .. 8")
        _mg_cycle_elem(cycle_dtype)
        PisoPressureSolverCudaCustom.__init__(self, dx, accuracy=accuracy, max_iterations=max_iterations, residual_reset=residual_reset,
                                              randomized_restarts=randomized_restarts, cast_to_double=True)
        self.name = "HIP multigrid-preconditioned Conjugate Gradient"
        self.smoothing_sweeps = int(smoothing_sweeps)
        self.cycle_dtype = cycle_dtype
        self.reuse_hierarchy = bool(reuse_hierarchy)
        self.use_guess = bool(use_guess)
        self._hierarchy = None           # the last MgHierarchy built (reuse_hierarchy)
        self._laplace_cache = None       # (key, the tensors the key points at, L) of the last solve_flat (reuse_hierarchy)
        for k in ("hierarchy_builds", "hierarchy_reuses", "laplace_builds") + (("guesses_accepted", "guesses_rejected") if self.use_guess else ()):
            dict.__setitem__(self.stats, k, 0)

    def drop_hierarchy(self):
        """Forgets the kept hierarchy and matrix (and frees their memory): the next solve builds both."""
        self._hierarchy = None
        self._laplace_cache = None

    def _laplace(self, nx, ny, active, accessible, a0, dt, sharding):
        if not self.reuse_hierarchy or sharding is not None:
            self.stats.add("laplace_builds", 1)
            return laplace_matrix_native(nx, ny, active, accessible, a0, dt, sharding)
        key = (a0.data_ptr(), a0._version, active.data_ptr(), active._version, accessible.data_ptr(), accessible._version, nx, ny, dt, a0.device)
        if self._laplace_cache is None or self._laplace_cache[0] != key:
            self._laplace_cache = None
            L = laplace_matrix_native(nx, ny, active, accessible, a0, dt, sharding)
            self.stats.add("laplace_builds", 1)
            self._laplace_cache = (key, (a0, active, accessible), L)      # (the tensors stay alive: their pointers cannot be handed out again)
        return self._laplace_cache[2]

    def solve(self, scaling_field, divergence, guess, enable_backprop, simulation_physics, offset=0, unrolling_step=0):
        # (use_guess off: `guess` is ignored like the plain solver's)
        scaling_field = scaling_field if isinstance(scaling_field, StaggeredGrid) else StaggeredGrid(scaling_field)
        a0 = flatten_staggered_data(scaling_field, coord_flip=False).detach().to(torch.float32)
        guess = getattr(guess, "data", guess) if self.use_guess else None       # (a CenteredGrid or its tensor)
        return self.solve_flat(a0, divergence, simulation_physics, unrolling_step=unrolling_step, guess=guess)

    def _slabs_in_use(self):
        # (option slab_force: a communicator of ONE rank still runs the slab solve - a ring of one, tests)
        return self.slab_comm is not None and (getattr(self.slab_comm, "world", 1) > 1 or getattr(self.slab_comm, "sharded", False) or
                                               N.get_option("slab_force") > 0)

    def _guess_for_solve(self, guess, divergence):
        if not self.use_guess or guess is None:
            return None
        if self._slabs_in_use():             # (before the guess is looked at: a sharded step's fields have the rank's cells only)
            self._refuse_guess_on_slabs()
        return _mg_guess(guess, divergence)                  # (detached, float64; a wrong size or device is refused here, before any launch)

    def _refuse_guess_on_slabs(self):
        raise N.PisoNativeError("PisoPressureSolverMultigrid: a guess is taken on one GPU only; a solve cut into y-slabs needs use_guess=False")

    def _cg(self, nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset, x0=None):
        from .distributed import SlabCommunicator, mg_solve_slab, mg_solve_slab_local
        if self.slab_comm is not None and not isinstance(self.slab_comm, SlabCommunicator):
            raise N.PisoNativeError("PisoPressureSolverMultigrid cuts a solve into y-slabs over a distributed.SlabCommunicator only; anything else "
                                    "in slab_comm is refused (one GPU: leave it None; other decompositions need PisoPressureSolverCudaCustom)")
        if not self.cast_to_double or L.dtype != torch.float64:
            raise N.PisoNativeError("PisoPressureSolverMultigrid is fp64 only; use PisoPressureSolverCudaCustom for float32")
        # (option slab_force: a communicator of ONE rank still runs the slab solve - a ring of one, tests)
        if self.slab_comm is not None and (self.slab_comm.world > 1 or N.get_option("slab_force") > 0):
            if self.use_guess:               # (before the communicator is touched)
                self._refuse_guess_on_slabs()
            if self.reuse_hierarchy:
                raise N.PisoNativeError("PisoPressureSolverMultigrid: a hierarchy is kept on one GPU only; a solve cut into y-slabs needs "
                                        "reuse_hierarchy=False")
            # (the plan is asked on the host, before the communicator is touched: g = 0 replicates the whole cycle, where float32 gains nothing)
            ny_all = self.slab_comm.step_sharding.nyl * self.slab_comm.world if self.slab_comm.sharded else ny
            if self.cycle_dtype != torch.float64 and N.mg_slab_plan(nx, ny_all, self.slab_comm.world)["g"] == 0:
                raise N.PisoNativeError("PisoPressureSolverMultigrid: the float32 cycle runs on one GPU only; a solve cut into y-slabs needs "
                                        "cycle_dtype=torch.float64")
            if self.slab_comm.sharded:       # slab-decomposed STEP: L holds the rank's owned rows, div its stored rows; the result stays there
                sh = self.slab_comm.step_sharding
                d_loc = sh.owned_cells(div.reshape(-1).to(torch.float64)).reshape(-1).contiguous()
                x_loc, it = mg_solve_slab_local(self.slab_comm, nx, sh.nyl, per_x, per_y, L, d_loc, accuracy, max_iterations, rank_deficient,
                                                residual_reset, self.smoothing_sweeps, cycle_dtype=self.cycle_dtype)
                x = torch.zeros(sh.n_cells, dtype=x_loc.dtype, device=x_loc.device)
                sh.owned_cells(x).copy_(x_loc.view(sh.nyl, nx))
                return x, it
            return mg_solve_slab(self.slab_comm, nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset,
                                 self.smoothing_sweeps, cycle_dtype=self.cycle_dtype)
        if not self.use_guess:
            x0 = None
        if not self.reuse_hierarchy:
            self.stats.add("hierarchy_builds", 1)
            out = mg_solve_native(nx, ny, per_x, per_y, L, div, accuracy, max_iterations, rank_deficient, residual_reset, self.smoothing_sweeps,
                                  self.cycle_dtype, x0=x0)
            return self._count_guess(x0, out)
        h = self._hierarchy
        if h is None or h.key != MgHierarchy.key_of(L, nx, ny, per_x, per_y, rank_deficient, self.cycle_dtype):
            self._hierarchy = None           # (freed before its successor is allocated; a refused prepare leaves none)
            h = self._hierarchy = mg_prepare_native(nx, ny, per_x, per_y, L, rank_deficient, self.cycle_dtype)
            self.stats.add("hierarchy_builds", 1)
        else:
            self.stats.add("hierarchy_reuses", 1)
        return self._count_guess(x0, mg_solve_prepared_guess_native(h, div, x0, accuracy, max_iterations, residual_reset, self.smoothing_sweeps))

    def _count_guess(self, x0, out):
        if x0 is not None:
            for k in ("guesses_accepted", "guesses_rejected"):       # (use_guess switched on after construction)
                dict.setdefault(self.stats, k, 0)
            self.stats.add("guesses_accepted" if N.mg_last_guess() == 1 else "guesses_rejected", 1)
        return out

    @staticmethod
    def last_dispatch():
        """levels, tail_first, sweeps, iterations, cycles, residual_recomputations, cycle_elem, vec_mask of this thread's last multigrid solve."""
        return N.mg_last_dispatch()
