"""Training losses of the reference (diffpiso/losses.py): same names, argument meaning and return convention
(`(loss + contribution, contribution)` when sum_steps, per-step lists otherwise).  `fields` / `velocity_fields` are lists
(batch) of lists (steps) of StaggeredGrid as returned by the unrolled PISO steps; `ground_truths[i]` is a staggered tensor
sequence [1, T, Ny+1, Nx+1, 2].

Slab fields (sharding.SlabStaggered, what a step of a slab-decomposed simulation returns): every loss keeps its signature and its return
convention and returns the RANK'S PART - the parts add up over the ranks to the one-GPU value (the caller all-reduces, training.py).
`ground_truths[i]` stays the whole-grid sequence on every rank; a step's frame is cut with `scatter_staggered`.
  L2, strain   the fused kernels of csrc/loss.hip on the rank's stored rows (`piso_loss_*_slab`); the strain loss fills the prediction's
               halo rows first (one `halo_faces`), its gather-form adjoint needs no exchange
  multistep    torch ops on the `owned_faces` views, cropped with the window's intersection with the owned rows
  spectral     every rank gathers the whole face field (`gather_face_rows`), evaluates the unchanged loss on it and contributes
               value / world; costs ONE whole-grid field per step, transiently (no rocFFT on slabs)
Whole-grid fields take the torch paths below unchanged; `L2_field_loss(..., fused=True)` / `strain_rate_loss(..., fused=True)` opt into the
whole-grid instantiation of the same kernels (device tensors only - there is no CPU form of them).
`spectral_energy_loss(..., fused=True)` replaces the torch expression around the transform by the kernels of csrc/loss_spectrum.hip: centre +
crop -> torch.fft.fft2 (rocFFT) -> shell sums through the tables of `spectrum_plan` (built once per crop shape, the bins of EK_spectrum_2D_tf
by construction) -> distance.  Fixed-order float64 sums instead of index_add_'s float atomics, no host read, gather-form adjoints.  On slab
fields the gathered whole field takes that path on every rank (value / world as before).  `training_dict["fused_losses"] = True` passes
fused=True to every loss of a training_run (training.py)."""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .evaluation_tools import EK_spectrum_2D_tf
from .grids import StaggeredGrid
from .les import forward_gradient
from .sharding import SlabStaggered


def _step_range(step_range):
    return step_range if isinstance(step_range, list) else [0, step_range]


# ---------------------------------------------------------------------------------------------------- fused kernels (csrc/loss.hip)
def loss_window(buffer_width, sponge_start, ny, nx):
    """(y0, y1, x0, x1): the crop of L2_field_loss on the indices of the staggered tensor [ny + 1][nx + 1], exactly the two slices it
    takes (`None`: the whole tensor; sponge_start 0: the tensor's width), resolved like Python resolves a slice and never inverted."""
    rows, cols = int(ny) + 1, int(nx) + 1
    if buffer_width is None:
        return 0, rows, 0, cols
    if sponge_start == 0:
        sponge_start = cols
    y0, y1, _ = slice(int(buffer_width[0][0]), rows - int(buffer_width[0][1])).indices(rows)
    x0, x1, _ = slice(int(buffer_width[1][0]), int(sponge_start) - int(buffer_width[1][1])).indices(cols)
    return y0, max(y1, y0), x0, max(x1, x0)


def _loss_entry(name, slab_ptr):
    """The whole-grid entry point, or its *_slab twin with the rank's piso_slab_t appended."""
    if slab_ptr is None:
        return getattr(N.lib, name), ()
    return getattr(N.lib, name + "_slab"), (slab_ptr,)


def _loss_workspace(device):
    return N.workspace(N.lib.piso_loss_workspace_bytes(), device, "loss")


def fused_l2_value(pred, target, nx, ny, window, factor, slab_ptr=None):
    """piso_loss_l2(_slab): factor / 2 * sum (pred - target)^2 over the window's (owned) faces -> one float64 on the device."""
    fn, tail = _loss_entry("piso_loss_l2", slab_ptr)
    out = torch.empty(1, dtype=torch.float64, device=pred.device)
    ws = _loss_workspace(pred.device)
    N.check(fn(N.ptr(pred), N.ptr(target), int(nx), int(ny), *[int(w) for w in window], C.c_double(float(factor)), N.ptr(out), N.ptr(ws),
               C.c_size_t(ws.numel()), N.stream_ptr(), *tail), "piso_loss_l2")
    return out


def fused_l2_grad(pred, target, nx, ny, window, factor, upstream, slab_ptr=None):
    """piso_loss_l2_grad(_slab): upstream * factor * (pred - target) inside the window on the owned faces, zero everywhere else."""
    fn, tail = _loss_entry("piso_loss_l2_grad", slab_ptr)
    out = torch.zeros_like(pred)
    N.check(fn(N.ptr(pred), N.ptr(target), int(nx), int(ny), *[int(w) for w in window], C.c_float(np.float32(factor)), N.ptr(upstream), N.ptr(out),
               N.stream_ptr(), *tail), "piso_loss_l2_grad")
    return out


def fused_strain_value(pred, target, nx, ny, dx_yx, factor, slab_ptr=None):
    """piso_loss_strain(_slab): factor * L1 distance of the unpadded strain entries (of the owned cell rows) -> one float64 on the device."""
    fn, tail = _loss_entry("piso_loss_strain", slab_ptr)
    out = torch.empty(1, dtype=torch.float64, device=pred.device)
    ws = _loss_workspace(pred.device)
    N.check(fn(N.ptr(pred), N.ptr(target), int(nx), int(ny), C.c_float(np.float32(dx_yx[1])), C.c_float(np.float32(dx_yx[0])),
               C.c_double(float(factor)), N.ptr(out), N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr(), *tail), "piso_loss_strain")
    return out


def fused_strain_grad(pred, target, nx, ny, dx_yx, factor, upstream, slab_ptr=None):
    fn, tail = _loss_entry("piso_loss_strain_grad", slab_ptr)
    out = torch.zeros_like(pred)
    N.check(fn(N.ptr(pred), N.ptr(target), int(nx), int(ny), C.c_float(np.float32(dx_yx[1])), C.c_float(np.float32(dx_yx[0])),
               C.c_double(float(factor)), N.ptr(upstream), N.ptr(out), N.stream_ptr(), *tail), "piso_loss_strain_grad")
    return out


class _FusedL2(torch.autograd.Function):
    """cfg = (nx, ny, window, factor, slab_ptr): the value as a float32 scalar; reverse mode is the gradient kernel (no host read)."""

    @staticmethod
    def forward(ctx, pred, target, cfg):
        ctx.cfg = cfg
        ctx.save_for_backward(pred, target)
        return fused_l2_value(pred, target, *cfg)[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        nx, ny, window, factor, slab_ptr = ctx.cfg
        return fused_l2_grad(pred, target, nx, ny, window, factor, g.to(torch.float32).reshape(1).contiguous(), slab_ptr), None, None


class _FusedStrain(torch.autograd.Function):
    """cfg = (nx, ny, dx_yx, factor, slab_ptr).  On slabs the caller has filled the halo rows of `pred` (the saved tensor keeps them)."""

    @staticmethod
    def forward(ctx, pred, target, cfg):
        ctx.cfg = cfg
        ctx.save_for_backward(pred, target)
        return fused_strain_value(pred, target, *cfg)[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        nx, ny, dx_yx, factor, slab_ptr = ctx.cfg
        return fused_strain_grad(pred, target, nx, ny, dx_yx, factor, g.to(torch.float32).reshape(1).contiguous(), slab_ptr), None, None


def _flat_pair(field, truth_frame):
    """(prediction, target, nx, ny, slab_ptr, sharding) as flat u-first face vectors: the rank's stored rows for a SlabStaggered (the target
    cut out of the replicated frame, halo rows included), the whole grid's otherwise."""
    from .fused import flat_faces
    ny, nx = (int(r) for r in field.resolution)
    if isinstance(field, SlabStaggered):
        sh = field.sharding
        pred = field.flat.contiguous()
        return pred, sh.scatter_staggered(truth_frame, device=pred.device), nx, ny, sh.slab_ptr, sh
    pred = flat_faces(field).to(torch.float32).contiguous()
    target = flat_faces(StaggeredGrid(truth_frame)).to(device=pred.device, dtype=torch.float32).contiguous()
    return pred, target, nx, ny, None, None


def _fused_l2(field, truth_frame, buffer_width, sponge_start, factor):
    pred, target, nx, ny, slab_ptr, _ = _flat_pair(field, truth_frame)
    return _FusedL2.apply(pred, target, (nx, ny, loss_window(buffer_width, sponge_start, ny, nx), float(factor), slab_ptr))


def _fused_strain(field, truth_frame, factor):
    pred, target, nx, ny, slab_ptr, sh = _flat_pair(field, truth_frame)
    if sh is not None:
        sh.halo_faces(pred.detach())                         # both launches read one row either side of the owned rows (in place, like the step)
    return _FusedStrain.apply(pred, target, (nx, ny, tuple(float(d) for d in field.dx), float(factor), slab_ptr))


# ---------------------------------------------------------------------------------------- fused spectral loss (csrc/loss_spectrum.hip)
def spectrum_window(buffer_width, sponge_start, ny, nx):
    """(y0, y1, x0, x1): the crop of spectral_energy_loss on CELL indices [ny][nx], exactly the two slices it takes of the centred field
    (sponge_start 0: the field's width), resolved like Python resolves a slice and never inverted."""
    rows, cols = int(ny), int(nx)
    if sponge_start == 0:
        sponge_start = cols
    y0, y1, _ = slice(int(buffer_width[0][0]), rows - int(buffer_width[0][1])).indices(rows)
    x0, x1, _ = slice(int(buffer_width[1][0]), int(sponge_start) - int(buffer_width[1][1])).indices(cols)
    return y0, max(y1, y0), x0, max(x1, x0)


class SpectrumPlan(object):
    """The wavenumber shells of an h x w crop, as tables on `device` (all int32):
      shell    [h * w] on the UNSHIFTED FFT index q = q0 * w + q1: the shell EK_spectrum_2D_tf adds that coefficient to - its `wvn` read
               at p = (q - n // 2) mod n per axis, tf_fftshift's quadrant swap without the copies
      perm     the q with shell[q] < cutoff, sorted by (shell, q)
      offsets  [cutoff + 1]: shell k is perm[offsets[k] : offsets[k + 1]]
    cutoff = min(h, w) // 2."""

    def __init__(self, h, w, device):
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError("spectrum plan: a crop of %d x %d cells" % (h, w))
        # the float32 expression of EK_spectrum_2D_tf, evaluated on the host: the arguments of sqrt are exact multiples of 1/4, a radius of
        # exactly k + 1/2 is the root of an exact square (exact on every IEEE sqrt, then rounded to even by torch.round like there), and
        # every other radius is further from k + 1/2 than any sqrt's error - so these are the device's bins, with no device-to-host copy
        ii = (torch.arange(h, dtype=torch.float32) - h / 2) ** 2
        jj = (torch.arange(w, dtype=torch.float32) - w / 2) ** 2
        wvn = torch.round(torch.sqrt(ii[:, None] + jj[None, :])).to(torch.int64)
        p0 = (torch.arange(h) - h // 2) % h
        p1 = (torch.arange(w) - w // 2) % w
        shell = wvn[p0][:, p1].reshape(-1)
        self.h, self.w, self.cutoff = h, w, min(h, w) // 2
        order = torch.sort(shell, stable=True).indices        # (shell, q): q ascends inside a shell because the sort is stable
        below = int((shell < self.cutoff).sum())
        counts = torch.bincount(shell[shell < self.cutoff], minlength=self.cutoff)[:self.cutoff]
        offsets = torch.zeros(self.cutoff + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(counts, 0)
        self.shell = shell.to(torch.int32).to(device)
        self.perm = order[:below].to(torch.int32).to(device)
        self.offsets = offsets.to(torch.int32).to(device)


_spectrum_plans = {}
_SPECTRUM_PLANS_MAX = 16


def spectrum_plan(h, w, device="cpu"):
    """The cached SpectrumPlan of an h x w crop on `device` (at most 16 are kept, the oldest goes first)."""
    key = (int(h), int(w), str(torch.device(device)))
    plan = _spectrum_plans.pop(key, None)
    if plan is None:
        plan = SpectrumPlan(h, w, device)
        while len(_spectrum_plans) >= _SPECTRUM_PLANS_MAX:
            _spectrum_plans.pop(next(iter(_spectrum_plans)))
    _spectrum_plans[key] = plan                                # (re-inserted: the dict's order is the order of last use)
    return plan


def _table_ptr(t):
    """Device pointer of a table that may be empty (a crop one cell wide has no shell below its cutoff): the entries refuse NULL, and an
    empty tensor has no address - one spare element stands in, which nothing reads."""
    return N.ptr(t if t.numel() else t.new_zeros(1))


def fused_centre_crop(flat, nx, ny, window):
    """piso_loss_centre_crop: flat u-first face vector -> [2, h, w] float32, the crop of at_centers() (plane 0: v, plane 1: u)."""
    y0, y1, x0, x1 = (int(v) for v in window)
    out = torch.empty((2, max(y1 - y0, 0), max(x1 - x0, 0)), dtype=torch.float32, device=flat.device)
    N.check(N.lib.piso_loss_centre_crop(N.ptr(flat), int(nx), int(ny), y0, y1, x0, x1, N.ptr(out), N.stream_ptr()), "piso_loss_centre_crop")
    return out


def fused_centre_crop_adjoint(d_planes, nx, ny, window):
    """piso_loss_centre_crop_adjoint: the cotangent of the planes -> the cotangent of the whole flat face vector (gathering)."""
    out = torch.empty((int(nx) + 1) * int(ny) + int(nx) * (int(ny) + 1), dtype=torch.float32, device=d_planes.device)
    N.check(N.lib.piso_loss_centre_crop_adjoint(N.ptr(d_planes), int(nx), int(ny), *[int(v) for v in window], N.ptr(out), N.stream_ptr()),
            "piso_loss_centre_crop_adjoint")
    return out


def fused_shell_sums(spec_real, plan):
    """piso_loss_spectrum_shells: torch.view_as_real(fft2(planes)) [2, h, w, 2] -> E[cutoff] float64, the first `cutoff` entries of
    EK_spectrum_2D_tf, summed in a fixed order."""
    store = torch.empty(max(plan.cutoff, 1), dtype=torch.float64, device=spec_real.device)
    N.check(N.lib.piso_loss_spectrum_shells(N.ptr(spec_real), _table_ptr(plan.perm), N.ptr(plan.offsets), plan.h, plan.w, plan.cutoff, N.ptr(store),
                                            N.stream_ptr()), "piso_loss_spectrum_shells")
    return store[:plan.cutoff]


def fused_shell_sums_adjoint(spec_real, plan, d_energy, upstream=None):
    """piso_loss_spectrum_shells_adjoint: (upstream *) d E -> the cotangent of the real view of the transform, a pure map."""
    out = torch.empty_like(spec_real)
    N.check(N.lib.piso_loss_spectrum_shells_adjoint(N.ptr(spec_real), N.ptr(plan.shell), _table_ptr(d_energy), N.ptr(upstream), plan.h, plan.w,
                                                    plan.cutoff, N.ptr(out), N.stream_ptr()), "piso_loss_spectrum_shells_adjoint")
    return out


def fused_spectrum_distance(e_pred, e_gt, cutoff, start_wavenumber, log_distance, factor):
    """piso_loss_spectrum_distance -> (value [1], d value / d e_pred [cutoff]), float64 on the device."""
    out = torch.empty(1 + max(int(cutoff), 1), dtype=torch.float64, device=e_pred.device)
    N.check(N.lib.piso_loss_spectrum_distance(_table_ptr(e_pred), _table_ptr(e_gt), int(cutoff), int(start_wavenumber), 1 if log_distance else 0,
                                              C.c_double(float(factor)), N.ptr(out), N.ptr(out[1:]), N.stream_ptr()),
            "piso_loss_spectrum_distance")
    return out[:1], out[1:1 + int(cutoff)]


class _CentreCrop(torch.autograd.Function):
    """cfg = (nx, ny, window): the flat face vector -> the cropped planes at the cell centres; reverse mode is the gathering adjoint."""

    @staticmethod
    def forward(ctx, flat, cfg):
        ctx.cfg = cfg
        return fused_centre_crop(flat, *cfg)

    @staticmethod
    def backward(ctx, g):
        return fused_centre_crop_adjoint(g.to(torch.float32).contiguous(), *ctx.cfg), None


class _SpectrumDistance(torch.autograd.Function):
    """The real view of the prediction's transform, the ground truth's shell energies -> the loss term as a float32 scalar (shell sums +
    distance, two launches).  cfg = (start_wavenumber, log_distance, factor).  Reverse mode is ONE map over the coefficients: the distance
    launch has left d value / d E on the device, the upstream scalar is read there too."""

    @staticmethod
    def forward(ctx, spec_real, e_gt, plan, cfg):
        e = fused_shell_sums(spec_real, plan)
        value, d_e = fused_spectrum_distance(e, e_gt, plan.cutoff, *cfg)
        ctx.plan = plan
        ctx.save_for_backward(spec_real, d_e)
        return value[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        spec_real, d_e = ctx.saved_tensors
        return fused_shell_sums_adjoint(spec_real, ctx.plan, d_e, g.to(torch.float32).reshape(1).contiguous()), None, None, None


def _fused_spectral(field, truth_frame, buffer_width, sponge_start, log_distance, start_wavenumber, factor):
    """One step's term of spectral_energy_loss(fused=True) on a whole-grid field: centre + crop -> torch.fft.fft2 (rocFFT) -> shell sums ->
    distance; the ground-truth frame through the same kernels without a graph."""
    from .fused import flat_faces
    ny, nx = (int(r) for r in field.resolution)
    pred = flat_faces(field).to(torch.float32).contiguous()
    if not pred.is_cuda:
        raise N.PisoNativeError("spectral_energy_loss(fused=True) needs device tensors; got a %s field (there is no CPU form of the fused "
                                "losses)" % pred.device)
    target = flat_faces(StaggeredGrid(truth_frame)).to(device=pred.device, dtype=torch.float32).contiguous()
    window = spectrum_window(buffer_width, sponge_start, ny, nx)
    plan = spectrum_plan(window[1] - window[0], window[3] - window[2], pred.device)
    with torch.no_grad():
        e_gt = fused_shell_sums(torch.view_as_real(torch.fft.fft2(fused_centre_crop(target, nx, ny, window))).contiguous(), plan)
    spec = torch.view_as_real(torch.fft.fft2(_CentreCrop.apply(pred, (nx, ny, window)))).contiguous()
    return _SpectrumDistance.apply(spec, e_gt, plan, (int(start_wavenumber), bool(log_distance), float(factor)))


class _GatherFaces(torch.autograd.Function):
    """The rank's stored rows -> the whole grid's flat face vector on every rank (distributed.gather_face_rows).  Every rank then evaluates
    the SAME function of the replicated field and contributes value / world: the cotangent that arrives is 1 / world of the whole gradient,
    so the rank's own rows of it are taken `world` times - and nothing has to be summed over the ranks."""

    @staticmethod
    def forward(ctx, flat, sh):
        from .distributed import face_rows_of_rank, gather_face_rows
        nx, ny = sh.nx, sh.ny
        (u0, u1), (v0, v1) = face_rows_of_rank(sh.rank, sh.world, nx, ny)
        u, v = sh.owned_faces(flat)
        whole = torch.zeros((nx + 1) * ny + nx * (ny + 1), dtype=flat.dtype, device=flat.device)
        whole[u0:u1] = u.reshape(-1)
        whole[v0:v1] = v.reshape(-1)
        ctx.sh, ctx.ranges = sh, ((u0, u1), (v0, v1))
        return gather_face_rows(sh.comm, whole, nx, ny)

    @staticmethod
    def backward(ctx, g):
        sh, ((u0, u1), (v0, v1)) = ctx.sh, ctx.ranges
        d = torch.zeros(sh.n_faces, dtype=g.dtype, device=g.device)
        u, v = sh.owned_faces(d)
        u.copy_(g[u0:u1].view_as(u) * sh.world)
        v.copy_(g[v0:v1].view_as(v) * sh.world)
        return d, None


def _gathered_grid(field):
    """A SlabStaggered as the whole grid's StaggeredGrid, replicated on every rank (one whole-grid field, alive while its loss term is)."""
    sh = field.sharding
    whole = _GatherFaces.apply(field.flat, sh)
    n_u = (sh.nx + 1) * sh.ny
    return StaggeredGrid([whole[n_u:].view(1, sh.ny + 1, sh.nx, 1), whole[:n_u].view(1, sh.ny, sh.nx + 1, 1)], field.box,
                         extrapolation=field.extrapolation)


def _owned_crop(rows, row_slice, first, count):
    """Local row slice of an owned-rows view: the whole-grid `row_slice` of a component of `rows` rows, cut to the owned rows
    [first, first + count)."""
    a, b, _ = row_slice.indices(rows)
    lo, hi = max(a, first), min(b, first + count)
    return slice(lo - first, max(hi, lo) - first)


def _l2(t):                                                   # tf.nn.l2_loss
    return (t ** 2).sum() / 2


def _sum(xs):
    xs = list(xs)
    return torch.stack([torch.as_tensor(x) for x in xs]).sum() if xs else torch.zeros(())


def L2_field_loss(loss, fields, ground_truths, step_range, buffer_width, loss_factor, sponge_start, box=None, sum_steps=True,
                  loss_influence_range=None, **kwargs):
    """losses.py:6-35."""
    step_range = _step_range(step_range)
    if not isinstance(loss_factor, list):
        loss_factor = [loss_factor for _ in range(step_range[1])]
    contrib = [[] for _ in range(step_range[1] - step_range[0])]
    for i in range(len(fields)):
        for s in range(step_range[0], step_range[1]):
            if isinstance(fields[i][s], SlabStaggered) or kwargs.get("fused", False):
                contrib[s - step_range[0]].append(_fused_l2(fields[i][s], ground_truths[i][:, s, ...], buffer_width, sponge_start, loss_factor[s]))
                continue
            data = fields[i][s].staggered_tensor()
            target = StaggeredGrid(ground_truths[i][:, s, ...]).staggered_tensor().to(data.device)
            if buffer_width is not None:
                if sponge_start == 0:
                    sponge_start = data.shape[2]
                ys = slice(buffer_width[0][0], int(data.shape[1]) - buffer_width[0][1])
                xs = slice(buffer_width[1][0], int(sponge_start) - buffer_width[1][1])
                contrib[s - step_range[0]].append(loss_factor[s] * _l2(data[:, ys, xs, :] - target[:, ys, xs, :]))
            else:
                contrib[s - step_range[0]].append(loss_factor[s] * _l2(data - target))
    if sum_steps:
        total = _sum(c for row in contrib for c in row)
        return loss + total, total
    per_step = [_sum(row) for row in contrib]
    r = loss_influence_range
    groups = [_sum(per_step[i * r:min((i + 1) * r, len(per_step))]) for i in range((len(per_step) - 1) // r + 1)]
    return [loss[i] + groups[i // r] for i in range(step_range[1] - step_range[0])], groups


def spectral_energy_loss(loss, velocity_fields, ground_truths, step_range, buffer_width=[[0, 0], [0, 0]], loss_factor=1,
                         sponge_start=0, log_distance=True, start_wavenumber=0, sum_steps=True, loss_influence_range=None,
                         **kwargs):
    """losses.py:38-64: distance between the shell-summed energy spectra of prediction and ground truth (first batch entry).

    fused=True (device tensors only): the kernels of csrc/loss_spectrum.hip either side of torch.fft.fft2 - centre + crop, shell sums in
    float64 over tables cached per crop shape (`spectrum_plan`), the distance - instead of the torch expression: no atomics (the same bits
    on every run, where index_add_ is non-deterministic on the GPU), no host read, a float32 scalar per step.  Same shells, same
    meaning of every argument and the same return shapes.  One deliberate difference: identical spectra in the log form (a sum of exactly
    0) give value 0 and gradient 0, where the torch path's sqrt'(0) returns NaN gradients.  A shell of zero or non-finite energy inside the
    log form's range still gives a non-finite value."""
    step_range = _step_range(step_range)
    if not isinstance(loss_factor, list):
        loss_factor = [loss_factor for _ in range(step_range[1])]
    contrib = []
    for s in range(step_range[0], step_range[1]):
        vel, share = velocity_fields[0][s], None
        if isinstance(vel, SlabStaggered):                   # the replicated whole field; this rank's part is value / world
            vel, share = _gathered_grid(vel), 1.0 / vel.sharding.world
        if kwargs.get("fused", False):
            contrib.append(_fused_spectral(vel, ground_truths[0][:, s, ...], buffer_width, sponge_start, log_distance, start_wavenumber,
                                           loss_factor[s]))
            if share is not None:
                contrib[-1] = contrib[-1] * share
            continue
        central = vel.at_centers().data
        if sponge_start == 0:
            sponge_start = central.shape[2]
        ys = slice(buffer_width[0][0], int(central.shape[1]) - buffer_width[0][1])
        xs = slice(buffer_width[1][0], int(sponge_start) - buffer_width[1][1])
        e = EK_spectrum_2D_tf(central[:, ys, xs, :][0])
        gt = StaggeredGrid(ground_truths[0][:, s, ...]).at_centers().data.to(central.device)
        g = EK_spectrum_2D_tf(gt[:, ys, xs, :][0])
        if log_distance:
            d = torch.log(g[:e.shape[0]] / e) ** 2
            contrib.append(torch.sqrt(d[1 + start_wavenumber:].sum()) * loss_factor[s])
        else:
            contrib.append((g[:e.shape[0]] - e).abs()[1:].sum() * loss_factor[s])
        if share is not None:
            contrib[-1] = contrib[-1] * share
    if sum_steps:
        total = _sum(contrib)
        return loss + total, total
    r = loss_influence_range
    return [loss[i] + _sum(contrib[i:min(i + r, len(contrib))]) for i in range(step_range[1] - step_range[0])], contrib


def _strain_parts(grid):
    g = [forward_gradient(grid.data[i].data, grid.dx) for i in range(2)]
    off = (g[0][:, 1:-1, 0:-1, 1] + g[1][:, 0:-1, 1:-1, 0]) / 2
    return [g[0][:, :-1, :, 0], off, off, g[1][:, :, :-1, 1]]


def strain_rate_loss(loss, velocity_fields, ground_truths, step_range, buffer_width, loss_factor=1, sponge_start=0, box=None,
                     sum_steps=True, loss_influence_range=None, **kwargs):
    """losses.py:66-95: L1 distance of the (unpadded) strain-rate entries."""
    step_range = _step_range(step_range)
    if not isinstance(loss_factor, list):
        loss_factor = [loss_factor for _ in range(step_range[1])]
    contrib = []
    for s in range(step_range[0], step_range[1]):
        vel = velocity_fields[0][s]
        if isinstance(vel, SlabStaggered) or kwargs.get("fused", False):
            contrib.append(_fused_strain(vel, ground_truths[0][:, s, ...], loss_factor[s]))
            continue
        gt = StaggeredGrid(ground_truths[0][:, s, ...].to(vel.staggered_tensor().device), vel.box)
        a, b = _strain_parts(vel), _strain_parts(gt)
        contrib.append(sum((a[i] - b[i]).abs().sum() for i in range(4)) * loss_factor[s])
    if sum_steps:
        total = _sum(contrib)
        return loss + total, total
    r = loss_influence_range
    return [loss[i] + _sum(contrib[i:min(i + r, len(contrib))]) for i in range(step_range[1] - step_range[0])], contrib


def multistep_averaging_loss(loss, velocity_fields, ground_truths, step_range, buffer_width, loss_factor=1, sponge_start=0,
                             box=None, sum_steps=True, loss_influence_range=None, **kwargs):
    """losses.py:97-148: L1 distance between moving time averages (window loss_influence_range) of prediction and truth."""
    step_range = _step_range(step_range)
    n = step_range[1] - step_range[0]
    du, dv, du_gt, dv_gt = [], [], [], []
    for s in range(step_range[0], step_range[1]):
        if isinstance(velocity_fields[0][s], SlabStaggered):
            # pointwise in space: the owned rows of prediction and truth, cropped with the window's intersection with the owned rows
            sh = velocity_fields[0][s].sharding
            u, v = sh.owned_faces(velocity_fields[0][s].flat)
            last = 1 if sh.last else 0
            gt = StaggeredGrid(ground_truths[0][:, s, ...].to(u.device))
            ru = _owned_crop(sh.ny, slice(buffer_width[0][0], sh.ny - buffer_width[0][1]), sh.j0, sh.nyl)
            rv = _owned_crop(sh.ny + 1, slice(buffer_width[0][0], sh.ny + 1 - buffer_width[0][1]), sh.j0, sh.nyl + last)
            cu = slice(buffer_width[1][0], sh.nx + 1 - buffer_width[1][1])
            cv = slice(buffer_width[1][0], sh.nx - buffer_width[1][1])
            du.append(u[ru, cu][None]); dv.append(v[rv, cv][None])
            du_gt.append(gt.data[1].data[0, sh.j0:sh.j1, :, 0][ru, cu][None])
            dv_gt.append(gt.data[0].data[0, sh.j0:sh.j1 + last, :, 0][rv, cv][None])
            continue
        u, v = velocity_fields[0][s].data[1].data, velocity_fields[0][s].data[0].data
        su = (slice(None), slice(buffer_width[0][0], int(u.shape[1]) - buffer_width[0][1]),
              slice(buffer_width[1][0], int(u.shape[2]) - buffer_width[1][1]), 0)
        sv = (slice(None), slice(buffer_width[0][0], int(v.shape[1]) - buffer_width[0][1]),
              slice(buffer_width[1][0], int(v.shape[2]) - buffer_width[1][1]), 0)
        gt = StaggeredGrid(ground_truths[0][:, s, ...].to(u.device))
        du.append(u[su]); dv.append(v[sv]); du_gt.append(gt.data[1].data[su]); dv_gt.append(gt.data[0].data[sv])
    if loss_influence_range is None:
        loss_influence_range = n
    r = loss_influence_range
    du, dv, du_gt, dv_gt = (torch.cat(x, dim=0) for x in (du, dv, du_gt, dv_gt))
    avg = lambda d: [d[i:i + r].mean(dim=0) for i in range(n - r + 1)]
    au, av, au_gt, av_gt = avg(du), avg(dv), avg(du_gt), avg(dv_gt)
    dist = lambda k: ((au[k] - au_gt[k]).abs().sum() + (av[k] - av_gt[k]).abs().sum()) * loss_factor
    contrib = []
    for i in range(n):
        if i < r // 2:
            contrib.append(dist(0))
        elif i >= r // 2 + n - r:
            contrib.append(dist(-1))
        else:
            contrib.append(dist(i - r // 2))
    if sum_steps:
        total = _sum(contrib)
        return loss + total, total
    return [loss[i] + contrib[i] for i in range(n)], contrib
