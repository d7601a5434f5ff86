"""The slab-decomposed STEP (new design, the reference is single-GPU) -- host side.  Round 5: LOCAL storage.

`distributed.py` cuts the two linear solvers into y-slabs; this module cuts everything else of `piso_step`: matrix assembly, the
stencil glue (forward and reverse mode), the Laplacian and the CSR product work on the face / cell rows of the rank's slab
(the `*_slab` entry points of libpiso_hip.so, include/piso_hip.h: piso_slab_t) and nothing is all-gathered.  A rank STORES its own
rows plus the rows either side that its gathers read, and nothing else - every tensor of a sharded step has 1 / ranks of the grid's
size (plus the halo rows), the library's workspaces included:

  cells, u faces   the ring rows [j0 - 2, j1 + 2)   (mod ny)                                     nyl + 4 rows
  v faces          the ring rows [j0 - 3, j1 + 3)   of the ring v[0] .. v[ny - 1], v[ny]        nyl + 6 rows
                   (the duplicate row v[ny] is a row of its own between v[ny - 1] and v[0]: the padded v of the last slab reads
                   v[0] and v[1], the first slab's lower halo is v[ny - 2], v[ny - 1], v[ny])
  flat face vectors = the stored u rows followed by the stored v rows ("v-first": v, then u)

The index arithmetic inside the kernels stays the whole grid's (boundary rules, seams, the reference's adjoint quirks are decided on
global (i, j)); only "where does row j live" goes through the rank's row map.  Every kernel of the step is "one thread per OUTPUT
element, gathering its inputs": in reverse mode the incoming cotangents are halo-filled before the adjoint kernel gathers from them,
so a halo exchange never needs an adjoint of its own.

Fields of a sharded simulation are `SlabStaggered` / `SlabCentered` (this module): what `piso_step` / `unroll_piso_steps` take and
return instead of StaggeredGrid / CenteredGrid when `simulation_physics.sharding` is set.  `StepSharding.scatter_*` cut a whole-grid
array (host or device) into the rank's stored rows, `owned_*` pick the rows a rank owns out of a stored array.

The CNN closure runs on the slabs as well (`make_slab_forcing_fn`, at the end of this module): its NHWC buffers hold the rank's rows plus
E = R + 1 halo rows either side (`ClosureHalo`; R = the network's reduced_buffer_width), filled by one wide exchange per step and direction.
"""
import ctypes as C
import zlib

import numpy as np
import torch

from . import _native as N
from .grids import AABox, as_tensor

HALO = 2      # u / cell rows either side: the widest stencil of the step (the periodic divergence adjoint's dc[n-2]; v: 3, see above)


def _msg(segments):
    """One message: up to three (offset, length) element segments -> 7 ints {count, off[3], len[3]}."""
    segments = [(int(o), int(n)) for o, n in segments if n > 0]
    assert len(segments) <= 3
    off = [o for o, _ in segments] + [0] * (3 - len(segments))
    ln = [n for _, n in segments] + [0] * (3 - len(segments))
    return [len(segments)] + off + ln


class StepSharding(object):
    """Row map + halo messages of one rank for an nx x ny grid cut into `comm.world` y-slabs (local storage)."""

    def __init__(self, comm, nx, ny):
        world, rank = comm.world, comm.rank
        nyl = ny // max(world, 1)
        if world < 2 or ny % world != 0 or nyl < 2 * HALO or nyl + 6 > ny:
            raise ValueError("slab-decomposed step: at least two ranks, ny (%d) divisible by the ranks (%d), at least %d rows per slab"
                             % (ny, world, 2 * HALO))
        self.comm, self.nx, self.ny, self.world, self.rank = comm, int(nx), int(ny), world, rank
        self.j0, self.j1, self.last = rank * nyl, (rank + 1) * nyl, rank == world - 1
        self.nyl = nyl
        self.slab = N.Slab(int(ny), int(self.j0), int(self.j1), 1 if self.last else 0)
        self.slab_ptr = C.pointer(self.slab)
        # stored rows (csrc/piso_common.h: RowMap)
        self.cb, self.cr = (self.j0 - 2) % ny, nyl + 4
        self.vb, self.vr = (self.j0 - 3) % (ny + 1), nyl + 6
        self.mb, self.mr = self.j0, nyl + 3
        self.n_u, self.n_v = self.cr * (nx + 1), self.vr * nx
        self.n_faces, self.n_cells = self.n_u + self.n_v, self.cr * nx
        self.n_pad = (nyl + 2) * (nx + 3) + (nyl + 3) * (nx + 2)
        w = HALO
        lower, upper = (rank - 1) % world, (rank + 1) % world
        jl1 = lower * nyl + nyl                      # end row of the ring-lower slab
        ju0 = upper * nyl                            # first row of the ring-upper slab
        lower_last = 1 if lower == world - 1 else 0
        mine_last = 1 if self.last else 0
        # (row interval) per message for u rows, v rows and cell rows - whole-grid row numbers; the rows of an interval follow each
        # other around the ring, so they are neighbours in the stored arrays as well
        self._rows = dict(
            to_upper=dict(u=(self.j1 - w, self.j1), v=(self.j1 - w, self.j1 + mine_last), c=(self.j1 - w, self.j1)),
            to_lower=dict(u=(self.j0, self.j0 + w), v=(self.j0, self.j0 + w), c=(self.j0, self.j0 + w)),
            from_lower=dict(u=(jl1 - w, jl1), v=(jl1 - w, jl1 + lower_last), c=(jl1 - w, jl1)),
            from_upper=dict(u=(ju0, ju0 + w), v=(ju0, ju0 + w), c=(ju0, ju0 + w)))
        nxu = nx + 1
        self._order = ("to_upper", "to_lower", "from_lower", "from_upper")

        def pack(fn):
            flat = []
            for key in self._order:
                flat += _msg(fn(self._rows[key]))
            return (C.c_int * 28)(*flat)
        self.msgs_faces = pack(lambda r: [(self.urow(r["u"][0]) * nxu, (r["u"][1] - r["u"][0]) * nxu),
                                          (self.n_u + self.vrow(r["v"][0]) * nx, (r["v"][1] - r["v"][0]) * nx)])
        self.msgs_faces_vfirst = pack(lambda r: [(self.vrow(r["v"][0]) * nx, (r["v"][1] - r["v"][0]) * nx),
                                                 (self.n_v + self.urow(r["u"][0]) * nxu, (r["u"][1] - r["u"][0]) * nxu)])
        self.msgs_cells = pack(lambda r: [(self.urow(r["c"][0]) * nx, (r["c"][1] - r["c"][0]) * nx)])
        self.msgs_csr = None                         # needs the row pointers: set by `set_pattern`
        self.pattern = None                          # (col_indices, row_pointers) of the STORED rows: geometry only, built once
        self.nnz = None                              # stored CSR entries (u matrix, v matrix)
        self.exchanges = 0
        self._sim_cache = {}
        self._scatter_cache = {}
        self._patterns = {}                          # (per_x, per_y) -> (pattern, msgs_csr, nnz)
        self._closure_halos = {}                     # (R, channels, periodic_y) -> ClosureHalo
        self.periodic_xy = (False, False)            # (x, y) periodicity of the velocity: set by the step (the CSR numbering needs it)
        comm.sharded = True
        comm.step_sharding = self                    # the solvers reach the row map through their communicator

    # ------------------------------------------------------------------------------------------------ the row map
    def urow(self, j):
        """Stored row of whole-grid u / cell row j."""
        return (int(j) - self.cb) % self.ny

    def vrow(self, j):
        return (int(j) - self.vb) % (self.ny + 1)

    def sizes(self, per_x, per_y):
        out = (C.c_int * 8)()
        N.check(N.lib.piso_slab_sizes(self.slab_ptr, self.nx, self.ny, int(per_x), int(per_y), out), "piso_slab_sizes")
        assert (out[0], out[1], out[2], out[3]) == (self.cr, self.vr, self.n_u, self.n_v) and out[7] == self.n_pad
        return dict(nnz_u=int(out[4]), nnz_v=int(out[5]), mask_rows=int(out[6]))

    # ------------------------------------------------------------------------------------------------ pattern of the two matrices
    def pattern_for(self, per_x, per_y):
        """The cached (col, rowptr, msgs_csr, (nnz_u, nnz_v)) of this periodicity, or None.  The stored nnz and the segments of the value
        array depend on (per_x, per_y): one entry per periodicity the sharding has been stepped with - never a pattern of another one."""
        hit = self._patterns.get((bool(per_x), bool(per_y)))
        if hit is not None:
            self.pattern, self.msgs_csr, self.nnz = hit[0], hit[1], hit[2]
        return hit

    def set_pattern(self, col_indices, row_pointers, nnz_u, per_xy=None, nnz=None):
        """col / rowptr of the STORED rows (one pattern-only assembly per periodicity: they depend on the geometry only) and, from the
        row pointers, the segments of the stored value array that hold a block of face rows."""
        nx = self.nx
        nxu = nx + 1
        rp = row_pointers.cpu().numpy().astype(np.int64)
        rp_u, rp_v = rp[:self.n_u + 1], rp[self.n_u + 1:]

        def segs(r):
            (ua, ub), (va, vb) = r["u"], r["v"]
            la, lb = self.urow(ua) * nxu, self.urow(ua) * nxu + (ub - ua) * nxu
            ma, mb = self.vrow(va) * nx, self.vrow(va) * nx + (vb - va) * nx
            return [(rp_u[la], rp_u[lb] - rp_u[la]), (nnz_u + rp_v[ma], rp_v[mb] - rp_v[ma])]
        flat = []
        for key in self._order:
            flat += _msg(segs(self._rows[key]))
        self.msgs_csr = (C.c_int * 28)(*flat)
        self.pattern = (col_indices, row_pointers)
        if nnz is not None:
            self.nnz = tuple(nnz)
        if per_xy is not None:
            self._patterns[(bool(per_xy[0]), bool(per_xy[1]))] = (self.pattern, self.msgs_csr, self.nnz)

    # ------------------------------------------------------------------------------------------------ halo exchanges (in place)
    def _exchange(self, t, msgs):
        if not t.is_contiguous():
            raise N.PisoNativeError("halo exchange of a non-contiguous tensor")
        code = {torch.float32: 0, torch.float64: 1, torch.int32: 2}[t.dtype]
        N.check(N.lib.piso_comm_exchange(self.comm.handle, N.ptr(t), code, msgs, N.stream_ptr()), "piso_comm_exchange")
        self.exchanges += 1
        return t

    def halo_faces(self, t):
        """Flat u-first face vector (stored rows): two rows below / above the slab (incl. the duplicate row v[ny] across the seam)."""
        assert t.numel() == self.n_faces
        return self._exchange(t, self.msgs_faces)

    def halo_faces_vfirst(self, t):
        assert t.numel() == self.n_faces
        return self._exchange(t, self.msgs_faces_vfirst)

    def halo_cells(self, t):
        assert t.numel() == self.n_cells
        return self._exchange(t, self.msgs_cells)

    def halo_csr_values(self, t):
        return self._exchange(t, self.msgs_csr)

    # ------------------------------------------------------------------------------------------------ whole grid <-> stored rows
    def _row_index(self, base, rows, period, device):
        return ((torch.arange(rows, device=device) + base) % period)

    def scatter_staggered(self, tensor, dtype=torch.float32, device=None):
        """Whole-grid staggered tensor [1, ny + 1, nx + 1, 2] (numpy / host / device) -> this rank's flat u-first face vector."""
        t = torch.as_tensor(tensor) if not isinstance(tensor, torch.Tensor) else tensor
        dev = device if device is not None else self.comm.device
        ny, nx = self.ny, self.nx
        u = t[0, :ny, :, 1].index_select(0, self._row_index(self.cb, self.cr, ny, t.device))
        v = t[0, :, :nx, 0].index_select(0, self._row_index(self.vb, self.vr, ny + 1, t.device))
        return torch.cat([u.reshape(-1), v.reshape(-1)]).to(device=dev, dtype=dtype).contiguous()

    def scatter_faces(self, flat, dtype=None, device=None):
        """Whole-grid flat u-first face vector -> stored rows."""
        t = torch.as_tensor(flat) if not isinstance(flat, torch.Tensor) else flat
        dev = device if device is not None else self.comm.device
        ny, nx = self.ny, self.nx
        n_u = (nx + 1) * ny
        u = t[:n_u].reshape(ny, nx + 1).index_select(0, self._row_index(self.cb, self.cr, ny, t.device))
        v = t[n_u:].reshape(ny + 1, nx).index_select(0, self._row_index(self.vb, self.vr, ny + 1, t.device))
        out = torch.cat([u.reshape(-1), v.reshape(-1)])
        return out.to(device=dev, dtype=dtype if dtype is not None else out.dtype).contiguous()

    def scatter_cells(self, tensor, dtype=torch.float32, device=None):
        """Whole-grid cell array [1, ny, nx, 1] (or [ny, nx]) -> [1, stored rows, nx, 1]."""
        t = torch.as_tensor(tensor) if not isinstance(tensor, torch.Tensor) else tensor
        dev = device if device is not None else self.comm.device
        t = t.reshape(self.ny, self.nx)
        c = t.index_select(0, self._row_index(self.cb, self.cr, self.ny, t.device))
        return c.to(device=dev, dtype=dtype).reshape(1, self.cr, self.nx, 1).contiguous()

    def scatter_mask(self, tensor, dtype=torch.float32, device=None):
        """Whole-grid padded cell mask [1, ny + 2, nx + 2, 1] (any shape with (ny + 2)(nx + 2) elements) -> the stored mask rows, flat."""
        t = torch.as_tensor(tensor) if not isinstance(tensor, torch.Tensor) else tensor
        dev = device if device is not None else self.comm.device
        t = t.reshape(self.ny + 2, self.nx + 2)
        hi = min(self.mb + self.mr, self.ny + 2)
        out = torch.zeros((self.mr, self.nx + 2), dtype=t.dtype, device=t.device)
        out[:hi - self.mb] = t[self.mb:hi]
        return out.to(device=dev, dtype=dtype).reshape(-1).contiguous()

    def owned_faces(self, flat):
        """(u rows [nyl, nx + 1], v rows [nyl + last, nx]) this rank owns, as views of a stored flat face vector."""
        nx, nyl = self.nx, self.nyl
        u = flat[:self.n_u].view(self.cr, nx + 1)[2:2 + nyl]
        v = flat[self.n_u:].view(self.vr, nx)[3:3 + nyl + (1 if self.last else 0)]
        return u, v

    def owned_cells(self, cells):
        return cells.reshape(self.cr, self.nx)[2:2 + self.nyl]

    def owned_sum_of_squares(self, flat):
        u, v = self.owned_faces(flat)
        return (u ** 2).sum() + (v ** 2).sum()

    # ------------------------------------------------------------------------------------------------ the simulation's constants, stored rows only
    def sim_tensors(self, sim, device):
        """active / accessible masks, Dirichlet mask, no-slip mask of `sim` cut to this rank's stored rows.  Cached per sim OBJECT (the
        entry holds the object: an id() reused after a collection cannot hit) and per content stamp of its four arrays: replaced arrays and
        in-place edits of arrays up to 1 MB (tensors: of any size) cut them again; larger numpy masks are constants of the sim object,
        as they are on the one-GPU path (SimulationParameters._cached keys its device copies by the array's identity)."""
        key = (id(sim), str(device))
        stamp = tuple(_stamp(a, big="identity") for a in (sim.active_mask, sim.accessible_mask, sim.dirichlet_mask, sim.no_slip_mask))
        hit = self._sim_cache.get(key)
        if hit is not None and hit[0] is sim and hit[1] == stamp:
            return hit[2]
        if len(self._sim_cache) > 8:
            self._sim_cache.clear()
        c = dict(active=self.scatter_mask(_host(sim.active_mask), torch.float32, device),
                 accessible=self.scatter_mask(_host(sim.accessible_mask), torch.float32, device),
                 dmask=self.scatter_staggered(_host(sim.dirichlet_mask).astype(np.float32), torch.float32, device).ne(0).to(torch.uint8).contiguous(),
                 no_slip=None)
        if sim.no_slip_mask is not None:
            # (as SimulationParameters.no_slip_flat reads it on one GPU: the first (ny + 2)(nx + 2) elements of an array that may be larger -
            # spatialMixingLayer_setup hands over one of the staggered tensor's shape)
            ns, need = _host(sim.no_slip_mask).astype(np.float32).reshape(-1), (self.ny + 2) * (self.nx + 2)
            if ns.size < need:
                raise ValueError("no_slip_mask must cover the padded cell grid (Ny+2)*(Nx+2)")
            c["no_slip"] = self.scatter_mask(ns[:need], torch.float32, device).ne(0).to(torch.uint8).contiguous()
        self._sim_cache[key] = (sim, stamp, c)
        return c

    def _cached(self, kind, obj, cut):
        """`cut(obj)` once per object AND content: identity + checksum for numpy arrays, identity + tensor._version for tensors (an
        array updated in place - a dirichlet_update_fn that returns the same array, a viscosity field edited between steps - is cut
        again; the one-GPU path re-uploads in exactly these cases, grids.device_constant).  Numpy arrays above 1 MB are not cached."""
        key = (kind, id(obj))
        stamp = _stamp(obj)
        if stamp is None:                              # a numpy array above 1 MB: cut every time (the one-GPU path uploads it every time)
            return cut(obj)
        hit = self._scatter_cache.get(key)
        if hit is None or hit[0] is not obj or hit[1] != stamp:
            if len(self._scatter_cache) > 32:
                self._scatter_cache.clear()
            hit = (obj, stamp, cut(obj))
            self._scatter_cache[key] = hit
        return hit[2]

    def cached_scatter_staggered(self, tensor):
        """scatter_staggered of a constant of the simulation (Dirichlet values)."""
        return self._cached("st", tensor, lambda t: self.scatter_staggered(_host(t).astype(np.float32)))

    def cached_scatter_faces(self, flat):
        return self._cached("fl", flat, lambda f: self.scatter_faces(torch.as_tensor(_host(f).reshape(-1)), dtype=torch.float32))

    # ------------------------------------------------------------------------------------------------ fields
    def staggered_grid(self, flat, box, extrapolation):
        return SlabStaggered(flat, self, box, extrapolation)

    def centered_grid(self, data, box, extrapolation):
        return SlabCentered(data, self, box, extrapolation)

    # ------------------------------------------------------------------------------------------------ the CNN closure on slabs
    def closure_halo(self, R, channels, periodic_y=False):
        """The wide halo of an NHWC buffer of the closure (ClosureHalo): R = the network's reduced_buffer_width."""
        key = (int(R), int(channels), bool(periodic_y))
        hit = self._closure_halos.get(key)
        if hit is None:
            hit = self._closure_halos[key] = ClosureHalo(self, *key)
        return hit

    def allreduce_gradients(self, params):
        """Sum `.grad` of the parameters over the ranks, in place: a rank's weight gradients of a sharded closure are the part that belongs to
        its owned outputs.  Through torch.distributed (host tensors for gloo, like mg_solve_slab(gather=True))."""
        import torch.distributed as dist
        from .distributed import _comm_device
        grads = [p.grad for p in params if p.grad is not None]
        if not grads or self.world < 2:
            return
        flat = torch.cat([g.reshape(-1) for g in grads])
        moved = flat.to(_comm_device(flat.device))
        dist.all_reduce(moved, op=dist.ReduceOp.SUM)
        flat = moved.to(flat.device)
        at = 0
        for g in grads:
            g.copy_(flat[at:at + g.numel()].view_as(g))
            at += g.numel()

    def check(self):
        """Raise if a wait on a peer gave up since the last check (agreed over the ranks; synchronises the stream)."""
        N.check(N.lib.piso_comm_check(self.comm.handle, N.stream_ptr()), "piso_comm_check")

    def close(self):
        self.comm.sharded = False
        self.comm.step_sharding = None


def _stamp(x, big=None):
    """What changes when the CONTENT of a cached input changes: tensor._version for tensors (bumped by every in-place op), an adler32
    checksum for numpy arrays up to 1 MB (the bound of grids.device_constant; ~1 ms per MB).  Above that: None ("do not cache"), or with
    big="identity" the array's address and shape (constants of a simulation object)."""
    if x is None:
        return ("none",)
    if isinstance(x, torch.Tensor):
        return ("v", x._version, tuple(x.shape), x.data_ptr())
    a = np.asarray(x)
    if a.nbytes > (1 << 20):
        return ("i", a.__array_interface__["data"][0], a.shape, str(a.dtype)) if big == "identity" else None
    return ("c", zlib.adler32(a if a.flags.c_contiguous else np.ascontiguousarray(a)), a.shape, str(a.dtype))


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


class SlabStaggered(object):
    """A staggered field of a slab-decomposed simulation: the rank's stored face rows as ONE flat u-first vector.  Quacks like the
    StaggeredGrid that `piso_step` / `unroll_piso_steps` take and return; `resolution`, `dx` and `box` are the WHOLE grid's."""

    def __init__(self, flat, sharding, box=None, extrapolation=None):
        if flat.numel() != sharding.n_faces:
            raise ValueError("SlabStaggered: %d elements, the rank stores %d" % (flat.numel(), sharding.n_faces))
        self.flat, self.sharding, self.extrapolation = flat.reshape(-1), sharding, extrapolation
        self.box = AABox.to_box(box, resolution_hint=[sharding.ny, sharding.nx]) if box is not None else None

    @property
    def resolution(self):
        return np.array([self.sharding.ny, self.sharding.nx])

    @property
    def dx(self):
        return self.box.size / self.resolution

    @property
    def device(self):
        return self.flat.device

    def staggered_tensor(self):
        return self.flat

    def rewrap(self, flat):
        return SlabStaggered(flat, self.sharding, self.box, self.extrapolation)


class SlabCentered(object):
    """A cell field of a slab-decomposed simulation: [1, stored rows, nx, 1]."""

    def __init__(self, data, sharding, box=None, extrapolation=None):
        if data.numel() != sharding.n_cells:
            raise ValueError("SlabCentered: %d elements, the rank stores %d" % (data.numel(), sharding.n_cells))
        self.data, self.sharding, self.extrapolation = data.reshape(1, sharding.cr, sharding.nx, 1), sharding, extrapolation
        self.box = AABox.to_box(box, resolution_hint=[sharding.ny, sharding.nx]) if box is not None else None

    @property
    def resolution(self):
        return np.array([self.sharding.ny, self.sharding.nx])

    @property
    def dx(self):
        return self.box.size / self.resolution

    def rewrap(self, data):
        return SlabCentered(data, self.sharding, self.box, self.extrapolation)

    def __add__(self, other):
        return self.rewrap(self.data + (other.data if isinstance(other, SlabCentered) else other))


# ---------------------------------------------------------------------------------------------------- the CNN closure on slabs
_PAD_MODE = {"constant": 0, "boundary": 1, "periodic": 2}


class ClosureHalo(object):
    """The wide halo of one NHWC buffer [rows][nx][channels] of the closure on a rank's slab.

    R = the network's reduced_buffer_width (the sum of k // 2 over its layers), E = R + 1: the extra row is the one the centre -> face
    resampling reads across the cut.  The buffer's EXTENDED ROWS are the whole-grid rows [j0 - lo, j1 + hi): lo / hi = E on a side with a
    ring neighbour (the seam of a periodic y axis included), 0 on a side that ends at a border of the domain - there the network's own SAME
    zero padding has to act, layer by layer.  Behind the extended rows the buffer carries 2 E SCRATCH rows: [A: E rows that arrive from the
    lower neighbour][B: E rows that arrive from the upper neighbour].
    Three exchanges, each a list of message tables in the 7-int format of piso_comm_exchange, chunked by whole rows so that no message is
    longer than the communicator's row_capacity (elements):
      forward   every rank's E edge rows -> its ring neighbours' halo rows
      reverse   every rank's halo rows (a cotangent's partial sums) -> their owner's scratch rows; `reverse_add` then adds A into the owner's
                first and B into its last E rows (piso_closure_halo_add)
      narrow    forward with one row (the adjoint of the network input gathers from one row either side)
    The exchange is always a ring with messages of full length (what piso_comm_exchange's other users send): where a side has no halo rows
    the rows that arrive land in the scratch rows and nobody reads them, and what is sent from there is not added by its receiver."""

    def __init__(self, sharding, R, channels, periodic_y=False):
        sh = self.sharding = sharding
        self.R, self.E, self.channels, self.periodic_y = int(R), int(R) + 1, int(channels), bool(periodic_y)
        E = self.E
        if R < 0 or channels < 1:
            raise ValueError("closure halo: R >= 0 and at least one channel")
        if sh.nyl < E:
            raise ValueError("closure on slabs: a slab needs at least E = R + 1 = %d rows (the network reads R = %d rows beyond a cut and the "
                             "resampling one more; with fewer a halo would span two neighbours), ny = %d on %d ranks gives %d"
                             % (E, R, sh.ny, sh.world, sh.nyl))
        self.lo = E if (sh.rank > 0 or self.periodic_y) else 0
        self.hi = E if (sh.rank < sh.world - 1 or self.periodic_y) else 0
        self.rows = sh.nyl + self.lo + self.hi
        self.L = L = sh.nx * self.channels                     # elements of one row
        self.numel = (self.rows + 2 * E) * L
        cap = int(getattr(sh.comm, "row_capacity", 8192))
        if L > cap:
            raise ValueError("closure on slabs: one NHWC row (nx %d x %d channels = %d elements) is longer than the communicator's row_capacity "
                             "(%d): the halo is chunked by whole rows" % (sh.nx, self.channels, L, cap))
        self.rows_per_message = cap // L
        self.tables_forward = self._tables(E, False)
        self.tables_reverse = self._tables(E, True)
        self.tables_narrow = self._tables(1, False)

    def _tables(self, w, reverse):
        lo, hi, nyl, rows, E, L = self.lo, self.hi, self.sharding.nyl, self.rows, self.E, self.L
        a_row, b_row = rows, rows + E                          # scratch A (from the lower neighbour), scratch B (from the upper)
        if not reverse:
            first = dict(to_upper=lo + nyl - w, to_lower=lo, from_lower=lo - w if lo else a_row, from_upper=lo + nyl if hi else b_row)
        else:
            first = dict(to_upper=lo + nyl if hi else b_row, to_lower=0 if lo else a_row, from_lower=a_row, from_upper=b_row)
        out = []
        for a in range(0, w, self.rows_per_message):
            n = min(w, a + self.rows_per_message) - a
            flat = []
            for key in ("to_upper", "to_lower", "from_lower", "from_upper"):
                flat += _msg([((first[key] + a) * L, n * L)])
            out.append((C.c_int * 28)(*flat))
        return out

    # ---- buffers
    def alloc(self, device, zero=False):
        return (torch.zeros if zero else torch.empty)(self.numel, dtype=torch.float32, device=device)

    def extended(self, buf):
        """The extended rows of a buffer as the NHWC tensor the network takes: [1, rows, nx, channels] (a view)."""
        return buf[:self.rows * self.L].view(1, self.rows, self.sharding.nx, self.channels)

    def _run(self, buf, tables):
        if buf.numel() != self.numel or buf.dtype != torch.float32:
            raise N.PisoNativeError("closure halo: the buffer holds %d float32 elements, the exchange needs %d" % (buf.numel(), self.numel))
        for t in tables:
            self.sharding._exchange(buf, t)
        return buf

    def forward(self, buf):
        return self._run(buf, self.tables_forward)

    def narrow(self, buf):
        return self._run(buf, self.tables_narrow)

    def reverse_add(self, buf):
        """Halo rows back to their owners, added into the owners' edge rows.  The halo rows themselves keep their (now stale) partial sums."""
        self._run(buf, self.tables_reverse)
        return self.add_received(buf)

    def add_received(self, buf):
        """The second half of `reverse_add`: scratch A into the first E owned rows, scratch B into the last E (sides with a neighbour)."""
        lo, hi, nyl, rows, E, L = self.lo, self.hi, self.sharding.nyl, self.rows, self.E, self.L
        for have, dst_row, src_row in ((lo, lo, rows), (hi, lo + nyl - E, rows + E)):
            if have:
                N.check(N.lib.piso_closure_halo_add(N.ptr(buf[dst_row * L:(dst_row + E) * L]), N.ptr(buf[src_row * L:(src_row + E) * L]),
                                                    C.c_size_t(E * L), N.stream_ptr()), "piso_closure_halo_add")
        return buf


class _SlabCoupling(object):
    """What the two autograd functions of a sharded closure share: the sharding, the halos of the network's input and output, the pressure's
    pad modes and 2 dx."""

    def __init__(self, sharding, halo_in, halo_out, pad_modes, two_dx, wrap):
        self.sh, self.halo_in, self.halo_out, self.wrap = sharding, halo_in, halo_out, wrap
        self.pad_modes = (C.c_int * 4)(*pad_modes)
        self.two_dx = C.c_double(float(two_dx))


class _SlabClosureInput(torch.autograd.Function):
    """Stored face rows, stored pressure rows -> the network input on the rank's extended rows (piso_closure_input_slab + the wide halo).
    Reverse: the cotangent that arrives holds, on every extended row, the part of d nn_in that belongs to THIS rank's owned outputs; the
    reverse exchange + add completes the owned rows, a one-row halo fill follows, piso_closure_input_adjoint_slab gathers."""

    @staticmethod
    def forward(ctx, faces, pressure, cp):
        sh, H = cp.sh, cp.halo_in
        sh.halo_faces(faces.detach())                          # (centre row j1 - 1 reads face row v[j1]; in place, as the step itself does next)
        if pressure is not None:
            sh.halo_cells(pressure.detach())
        buf = H.alloc(faces.device)
        N.check(N.lib.piso_closure_input_slab(N.ptr(faces), N.ptr(pressure), N.ptr(buf), sh.nx, sh.ny, H.channels, cp.pad_modes, cp.two_dx,
                                              N.stream_ptr(), sh.slab_ptr, H.lo, H.hi), "piso_closure_input_slab")
        H.forward(buf)
        ctx.cp, ctx.p_shape = cp, None if pressure is None else pressure.shape
        return H.extended(buf)

    @staticmethod
    def backward(ctx, g):
        cp = ctx.cp
        sh, H = cp.sh, cp.halo_in
        buf = H.alloc(g.device)
        H.extended(buf).copy_(g)
        H.reverse_add(buf)
        H.narrow(buf)
        d_faces = torch.zeros(sh.n_faces, dtype=torch.float32, device=g.device)
        d_p = torch.zeros(sh.n_cells, dtype=torch.float32, device=g.device) if H.channels == 4 else None
        N.check(N.lib.piso_closure_input_adjoint_slab(N.ptr(buf), N.ptr(d_faces), N.ptr(d_p), sh.nx, sh.ny, H.channels, cp.pad_modes, cp.two_dx,
                                                      N.stream_ptr(), sh.slab_ptr, H.lo, H.hi), "piso_closure_input_adjoint_slab")
        return d_faces, None if d_p is None or ctx.p_shape is None else d_p.view(ctx.p_shape), None


class _SlabClosureForce(torch.autograd.Function):
    """The network output on the extended rows -> the forcing on the rank's owned face rows (piso_closure_force_slab).  Reverse: the
    cotangent of the faces is halo-filled (halo_faces), the gather-form adjoint then completes d nn_out on the OWNED rows - every other
    extended row stays exactly zero, so that what the convolution backward makes of it is the part of d nn_in, and of the weight gradients,
    that belongs to this rank's owned outputs."""

    @staticmethod
    def forward(ctx, nn_out, cp):
        sh, H = cp.sh, cp.halo_out
        nn_out = nn_out.contiguous()
        if tuple(nn_out.shape) != (1, H.rows, sh.nx, 2):
            raise ValueError("closure on slabs: the network returned %s for the extended rows %s" % (tuple(nn_out.shape), (1, H.rows, sh.nx, 2)))
        faces = torch.zeros(sh.n_faces, dtype=torch.float32, device=nn_out.device)
        N.check(N.lib.piso_closure_force_slab(N.ptr(nn_out), N.ptr(faces), sh.nx, sh.ny, int(cp.wrap[1]), int(cp.wrap[0]), N.stream_ptr(),
                                              sh.slab_ptr, H.lo, H.hi), "piso_closure_force_slab")
        ctx.cp = cp
        return faces

    @staticmethod
    def backward(ctx, g):
        cp = ctx.cp
        sh, H = cp.sh, cp.halo_out
        g = sh.halo_faces(g.contiguous().clone())
        d_out = torch.zeros((1, H.rows, sh.nx, 2), dtype=torch.float32, device=g.device)
        N.check(N.lib.piso_closure_force_adjoint_slab(N.ptr(g), N.ptr(d_out), sh.nx, sh.ny, int(cp.wrap[1]), int(cp.wrap[0]), N.stream_ptr(),
                                                      sh.slab_ptr, H.lo, H.hi), "piso_closure_force_adjoint_slab")
        return d_out, None


class _WrappedOnSlabs(object):
    """The network as a wrapper sees it on slabs: called without `wrap`, it runs with the slab path's (False, wrap_x) - the ring halo is the
    y wrap."""

    def __init__(self, network, wrap):
        self.network, self.wrap = network, wrap

    def __call__(self, fields, wrap=None):
        return self.network(fields, wrap=self.wrap if wrap is None else wrap)

    def __getattr__(self, name):
        return getattr(self.network, name)


def check_slab_network(network):
    """What a network must be to run on y-slabs; raises ValueError naming the rule.  -> its reduced_buffer_width."""
    R = getattr(network, "reduced_buffer_width", None)
    if R is None or isinstance(R, (list, tuple)):
        raise ValueError("closure on slabs: the network must state its `reduced_buffer_width` (the sum of k // 2 over its layers, an int): it is "
                         "the width of the halo its receptive field needs")
    if getattr(network, "padding", "SAME") != "SAME":
        raise ValueError("closure on slabs: padding must be 'SAME' (got %r): a VALID network shrinks the rows of every slab" % (network.padding,))
    bw = getattr(network, "buffer_width", None)
    if bw is not None and any(int(b) != 0 for b in bw[0]):
        raise ValueError("closure on slabs: the y entries of buffer_width must be 0 (got %s): a crop of the whole grid's first and last rows is not "
                         "a crop of every slab's; x entries are local and stay allowed" % (list(bw[0]),))
    return int(R)


def make_slab_forcing_fn(network, sharding, pressure_included=True, wrap=None, wrapper=None):
    """closure.make_forcing_fn for a slab-decomposed simulation: forcing_fn(i, velocity, pressure) takes SlabStaggered / SlabCentered fields
    and returns the SlabStaggered forcing of the rank's rows.
      1. piso_closure_input_slab writes the owned rows of the network input, 2. the wide halo exchange (ClosureHalo, E = R + 1 rows) fills
      the halo rows, 3. the network runs on the extended rows as network(x, wrap=(False, wrap_x)), 4. piso_closure_force_slab reads the
      owned rows and one row either side of its output.
    Why 3. is right: a SAME convolution of kernel size k lets the zero padding of an ARTIFICIAL end (a cut) into k // 2 rows per layer.
    After all layers the wrong values have advanced R = sum k // 2 rows: rows [0, R) and [rows - R, rows) of the output, which are halo rows;
    row R (the one the resampling reads across the cut) and every owned row saw whole-grid data only - with one wavefront per 64 pixels of
    an output row and a K loop that does not depend on the image height (csrc/conv.hip) bit for bit what the whole grid computes.  At a
    border of the domain there is no halo (lo / hi = 0) and the padding is the network's own.
    Reverse mode runs the same count backwards: d nn_out is non-zero on the owned rows only, so the gradient w.r.t. the output of layer l
    is non-zero within sum_{m > l} k_m // 2 rows of the owned ones - and the saved activations of layer l are valid within
    1 + sum_{m > l} k_m // 2 rows: every product of the input and weight gradients pairs a non-zero cotangent with a valid activation
    (garbage activations are finite - sums of whole-grid data and zeros - and meet exact zeros).  Each rank ends with the part of d nn_in
    that belongs to its owned outputs, on owned + R rows; the reverse exchange adds the parts across the cuts (one more rounding than on
    one GPU).  Weight gradients: the part that belongs to the rank's owned outputs - StepSharding.allreduce_gradients sums them.
    A network with biases, skip connections or another activation (FullyConvNetwork(bias=, skips=, activation=)) changes none of this: the
    epilogue of a layer is element-wise, a skip adds no receptive field and the halo width is the same R.  The bias gradient of a rank is
    the sum over its extended rows of the layer's pre-activation cotangent, which is exactly zero wherever the saved activations are
    invalid (above) - the part of the rank's owned outputs; allreduce_gradients over weights and biases gives the whole gradient.
    wrap = (wrap_y, wrap_x) of the resampling (None: edges replicated).  wrap_y must equal the network's: on a y-periodic domain the ring
    halo IS the wrap of both.  wrapper(network, nn_in_ext): the network it is handed runs with (False, wrap_x) unless told otherwise.
    Refused before any launch: VALID padding, a y buffer_width, a network without reduced_buffer_width, slabs thinner than E rows."""
    from .closure import _wrap2
    from .grids import axis_extrapolation
    R = check_slab_network(network)
    wrap = _wrap2(wrap)
    net_wrap = _wrap2(getattr(network, "wrap", None))
    if net_wrap[0] != wrap[0]:
        raise ValueError("closure on slabs: the network (wrap_y %s) and the centre -> face resampling (wrap_y %s) must wrap y together: the ring "
                         "halo is the wrap of both" % (net_wrap[0], wrap[0]))
    channels = 4 if pressure_included else 2
    halo_in = sharding.closure_halo(R, channels, wrap[0])
    halo_out = sharding.closure_halo(R, 2, wrap[0])
    slab_wrap = (False, net_wrap[1])

    def forcing(i, velocity, pressure):
        if not (hasattr(velocity, "rewrap") and velocity.sharding is sharding):
            raise ValueError("closure on slabs: the forcing function of a sharded closure takes the SlabStaggered / SlabCentered fields of its sharding")
        modes, two_dx = (1, 1, 1, 1), 1.0
        if pressure_included:
            assert np.allclose(pressure.dx, np.mean(pressure.dx)), "Only cubic cells supported."
            ext = axis_extrapolation(pressure.extrapolation, 2)
            modes = []
            for axis in (1, 0):                                # (x lower, x upper, y lower, y upper)
                e = ext[axis]
                lo_mode, hi_mode = (e, e) if isinstance(e, str) else e
                modes += [_PAD_MODE[lo_mode], _PAD_MODE[hi_mode]]
            two_dx = 2 * float(np.mean(pressure.dx))
        cp = _SlabCoupling(sharding, halo_in, halo_out, modes, two_dx, wrap)
        nn_in = _SlabClosureInput.apply(velocity.flat, pressure.data if pressure_included else None, cp)
        if wrapper is not None:
            nn_out = wrapper(_WrappedOnSlabs(network, slab_wrap), nn_in)
        else:
            nn_out = network(nn_in, wrap=slab_wrap)
        return velocity.rewrap(_SlabClosureForce.apply(nn_out, cp))
    return forcing
