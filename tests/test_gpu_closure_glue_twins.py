"""The coupling kernels of the CNN closure (csrc/closure_glue.hip).

(1) The whole-grid entries against the torch functions they restate (closure.network_input, closure.centered_to_staggered), on the four
    set-ups of tests/cases.py (their pressure pad modes), pressure on and off, every wrap combination, grids 12 x 10, 13 x 12, 70 x 33:
    forward bit for bit; adjoints bit for bit against torch autograd on cotangents that make every float32 partial sum exact, and once on
    random cotangents against a float64 autograd evaluation.
(2) The `_slab` twins against the whole-grid entries the way tests/test_gpu_slab_twins.py does it: every legal slab of the 10-, 12- and
    13-row grids, Space.check - written elements bit for bit, everything else and both guard bands still the pre-fill, no written element
    the pre-fill.  NHWC buffers hold the extended rows [row_begin - lo, row_end + hi) (include/piso_hip.h); as INPUTS they carry whole-grid
    data on the owned rows and ONE row either side only - every other row is NaN, so a kernel that reads further shows."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import slab_emulation as E
from tests.cases import make_case
from tests.test_gpu_slab_twins import Inputs, case_modes, finish, slabs_of

pytestmark = pytest.mark.gpu
CASES = ["periodic", "xper_ywall", "cavity", "spatial_ml"]
GRIDS = [(10, 12), (12, 13), (33, 70)]                      # (ny, nx): nx x ny = 12 x 10, 13 x 12, 70 x 33
SMALL = [(10, 5), (12, 5), (13, 4)]
WRAPS = list(itertools.product((False, True), (False, True)))      # (wrap_y, wrap_x)
U32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- layouts of the NHWC buffers
def add_nhwc(L, ext, ring):
    """Adds the kinds nhwc2 / nhwc4 (outputs: the owned rows are written) and nhwc2_in / nhwc4_in (inputs: whole-grid data on the owned rows
    and one row either side, nothing elsewhere) to a layout.  -> (lo, hi)."""
    nx, ny = L.nx, L.ny
    if L.whole:
        rows, lo, hi, n = np.arange(ny), 0, 0, ny
    else:
        lo = ext if (L.row_begin > 0 or ring) else 0
        hi = ext if (L.row_end < ny or ring) else 0
        n = L.rows
        rows = (L.row_begin - lo + np.arange(n + lo + hi)) % ny
    pos = np.arange(rows.size)
    owned = (pos >= lo) & (pos < lo + n)
    near = (pos >= lo - 1) & (pos < lo + n + 1)
    for ch in (2, 4):
        idx = (rows[:, None] * nx * ch + np.arange(nx * ch)[None, :]).astype(np.int64)
        L.idx["nhwc%d" % ch], L.own["nhwc%d" % ch] = idx.ravel(), np.repeat(owned, nx * ch)
        near_idx = idx.copy()
        near_idx[~near] = -1
        L.idx["nhwc%d_in" % ch], L.own["nhwc%d_in" % ch] = near_idx.ravel(), np.repeat(owned, nx * ch)
    return lo, hi


class Ext(object):
    """A Space whose layout knows the NHWC kinds."""

    def __init__(self, layout, ext=0, ring=False):
        self.lo, self.hi = add_nhwc(layout, ext, ring)
        self.S = E.Space(layout)

    def call(self, name, *args):
        from diffpiso import _native as N
        S = self.S
        if S.slab_ptr is None:
            st = getattr(N.lib, name)(*args)
        else:
            st = getattr(N.lib, name + "_slab")(*(args + (S.slab_ptr, self.lo, self.hi)))
        assert st == 0, "%s returned %d: %s" % (name, st, N.lib.piso_last_error_string().decode())


def op_input(X, faces, p, ch, modes, two_dx):
    out = X.S.out("nhwc%d" % ch)
    X.call("piso_closure_input", E.ptr(faces), E.ptr(p), E.ptr(out), X.S.nx, X.S.ny, ch, E.pad_modes_c(modes), C.c_double(two_dx), E._stream())
    return {"nn_in": ("nhwc%d" % ch, out)}


def op_input_adjoint(X, g, ch, modes, two_dx):
    df, dp = X.S.out("faces"), (X.S.out("cells") if ch == 4 else None)
    X.call("piso_closure_input_adjoint", E.ptr(g), E.ptr(df), E.ptr(dp), X.S.nx, X.S.ny, ch, E.pad_modes_c(modes), C.c_double(two_dx), E._stream())
    outs = {"d_faces": ("faces", df)}
    if dp is not None:
        outs["d_p"] = ("cells", dp)
    return outs


def op_force(X, nn_out, wrap):
    out = X.S.out("faces")
    X.call("piso_closure_force", E.ptr(nn_out), E.ptr(out), X.S.nx, X.S.ny, int(wrap[1]), int(wrap[0]), E._stream())
    return {"faces": ("faces", out)}


def op_force_adjoint(X, g, wrap):
    out = X.S.out("nhwc2")
    X.call("piso_closure_force_adjoint", E.ptr(g), E.ptr(out), X.S.nx, X.S.ny, int(wrap[1]), int(wrap[0]), E._stream())
    return {"d_nn_out": ("nhwc2", out)}


# ---------------------------------------------------------------------------------------------------------------- (1) against torch
def torch_fields(c, vel_src, p, two_dx, grad=False):
    """The case's velocity / pressure as the package's fields on the device, the cell size chosen so that 2 dx = two_dx."""
    import diffpiso as dp
    ny, nx = c["ny"], c["nx"]
    dx = two_dx / 2.0
    box = dp.box[0:dx * ny, 0:dx * nx]
    vel_t = vel_src.clone().requires_grad_(grad)
    p_t = p.reshape(1, ny, nx, 1).clone().requires_grad_(grad)
    return vel_t, p_t, dp.StaggeredGrid(vel_t, box), dp.CenteredGrid(p_t, box, extrapolation=c["p_ext"])


def network_input64(c, vel_src, p, two_dx, channels):
    """closure.network_input in float64 (the package's field classes keep float32): the two means of at_centers written out, and
    closure.centered_gradient on a float64 stand-in for the pressure field.  -> (staggered leaf, pressure leaf, network input)."""
    import types
    import diffpiso as dp
    ny, nx = c["ny"], c["nx"]
    vel_t = vel_src.detach().double().clone().requires_grad_(True)
    p_t = p.detach().double().reshape(1, ny, nx, 1).clone().requires_grad_(True)
    v, u = vel_t[:, :, :-1, 0:1], vel_t[:, :-1, :, 1:2]
    nn_in = torch.cat([0.5 * (v[:, 1:] + v[:, :-1]), 0.5 * (u[:, :, 1:] + u[:, :, :-1])], dim=-1)
    if channels == 4:
        field = types.SimpleNamespace(data=p_t, extrapolation=c["p_ext"], dx=np.array([two_dx / 2.0, two_dx / 2.0]))
        nn_in = torch.cat([nn_in, dp.centered_gradient(field)], dim=-1)
    return vel_t, p_t, nn_in


def flat_faces(t):
    """Staggered tensor [1, ny + 1, nx + 1, 2] -> the flat u-first face vector, in the tensor's own dtype (the package's
    flatten_staggered_data goes through StaggeredGrid, which keeps float32: a float64 oracle would be rounded on the way)."""
    return torch.cat([t[0, :-1, :, 1].reshape(-1), t[0, :, :-1, 0].reshape(-1)]).contiguous()


def same_bits(a, b):
    return (E._int_view(a.reshape(-1).contiguous()) == E._int_view(b.reshape(-1).contiguous())).all()


def exact_cotangent(gen, shape):
    """Small integers times a power of two: every float32 sum of up to eight of them, halved or divided by a power of two, is exact."""
    return (torch.randint(-8, 9, shape, generator=gen).float() * 0.125).cuda()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", GRIDS)
def test_whole_grid_kernels_are_the_torch_functions(name, shape):
    """Forward bit for bit; adjoints bit for bit on exact cotangents with 2 dx = 1/2 (a power of two: the quotient of every term is exact, so
    the sums are exact in any order); adjoints on random cotangents and the case's own 2 dx against float64 autograd.
    Bound of the random run: an output is a sum of at most four terms, each 0.5 g (exact) or g x fl(1 / (2 dx)) (the device's form of the one
    division, the reciprocal taken in double: two roundings, relative 2 x 2^-24); three additions of a left-to-right sum add at most 3 x 2^-24 of the sum of the terms'
    magnitudes.  With every term at most G = max|g| max(0.5, 1 / (2 dx)):   |error| <= (2 + 3) 2^-24 x 4 G = 20 x 2^-24 G  per element (the
    float64 evaluation's own error, 2^-53 relative, is far below it)."""
    import diffpiso as dp
    ny, nx = shape
    c = make_case(name, ny, nx, seed=2)
    I = Inputs(nx, ny, 21)
    modes = case_modes(c)
    vel = torch.as_tensor(c["vel"]).cuda()
    p = torch.as_tensor(c["p"]).cuda()
    X = Ext(E.WholeLayout(nx, ny))
    W = X.S
    f_vel, f_p = W.put("faces", flat_faces(vel)), W.put("cells", p.reshape(-1))
    tally = E.Tally()
    gen = torch.Generator().manual_seed(3)
    two_dx_case = 2 * float(np.mean(c["dx_yx"]))
    for ch in (4, 2):
        for two_dx, exact in ((0.5, True), (two_dx_case, False)):
            vel_t, p_t, velocity, pressure = torch_fields(c, vel, p, two_dx, grad=True)
            want = dp.network_input(velocity, pressure, pressure_included=ch == 4)
            o = op_input(X, f_vel, f_p, ch, modes, two_dx)
            tally.launch("input %d ch 2dx %g" % (ch, two_dx), W, o, None)
            tally.add("input %d ch 2dx %g == network_input" % (ch, two_dx), same_bits(o["nn_in"][1].t, want))
            g = exact_cotangent(gen, (1, ny, nx, ch)) if exact else I.randn(ny * nx * ch).reshape(1, ny, nx, ch)
            want.backward(g)
            a = op_input_adjoint(X, W.put("nhwc%d" % ch, g.reshape(-1)), ch, modes, two_dx)
            tally.launch("input adjoint %d ch 2dx %g" % (ch, two_dx), W, a, None)
            got = [a["d_faces"][1].t] + ([a["d_p"][1].t] if ch == 4 else [])
            if exact:
                tally.add("input adjoint %d ch: d faces == autograd" % ch, same_bits(got[0], flat_faces(vel_t.grad)))
                if ch == 4:
                    tally.add("input adjoint: d p == autograd", same_bits(got[1], p_t.grad))
            else:
                v64, p64, nn64 = network_input64(c, vel, p, two_dx, ch)
                nn64.backward(g.double())
                bound = 20 * U32 * float(g.abs().max()) * max(0.5, 1.0 / two_dx)
                errs = [float((got[0].double() - flat_faces(v64.grad)).abs().max())] + ([float((got[1].double() - p64.grad.reshape(-1)).abs().max())] if ch == 4 else [])
                print("%s %dx%d input adjoint %d ch vs float64 autograd: max errors %s, bound %.3e" % (name, nx, ny, ch, errs, bound))
                assert max(errs) <= bound, (errs, bound)
    for wrap in WRAPS:
        nn_out = I.randn(ny * nx * 2).reshape(1, ny, nx, 2).requires_grad_(True)
        want = dp.centered_to_staggered(nn_out, wrap)
        o = op_force(X, W.put("nhwc2", nn_out.detach().reshape(-1)), wrap)
        tally.launch("force wrap %s" % (wrap,), W, o, None)
        tally.add("force wrap %s == centered_to_staggered" % (wrap,), same_bits(o["faces"][1].t, flat_faces(want)))
        g_st = torch.zeros_like(want)
        g_st[:, :, :nx, 0] = exact_cotangent(gen, (1, ny + 1, nx))
        g_st[:, :ny, :, 1] = exact_cotangent(gen, (1, ny, nx + 1))
        want.backward(g_st)
        a = op_force_adjoint(X, W.put("faces", flat_faces(g_st)), wrap)
        tally.launch("force adjoint wrap %s" % (wrap,), W, a, None)
        tally.add("force adjoint wrap %s == autograd" % (wrap,), same_bits(a["d_nn_out"][1].t, nn_out.grad))
        # random cotangent against float64: at most three terms 0.5 d (exact) per output, two additions: 2 x 2^-24 x 3 x 0.5 max|d|
        n64 = nn_out.detach().double().requires_grad_(True)
        gr = torch.zeros_like(want)
        gr[:, :, :nx, 0], gr[:, :ny, :, 1] = I.randn((ny + 1) * nx).reshape(1, ny + 1, nx), I.randn(ny * (nx + 1)).reshape(1, ny, nx + 1)
        dp.centered_to_staggered(n64, wrap).backward(gr.double())
        a = op_force_adjoint(X, W.put("faces", flat_faces(gr)), wrap)
        err, bound = float((a["d_nn_out"][1].t.double() - n64.grad.reshape(-1)).abs().max()), 3 * U32 * float(gr.abs().max())
        print("%s %dx%d force adjoint wrap %s vs float64 autograd: max error %.3e, bound %.3e" % (name, nx, ny, wrap, err, bound))
        assert err <= bound, (wrap, err, bound)
    finish(tally)


# ---------------------------------------------------------------------------------------------------------------- (2) the slab twins
AXIS_MODES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)]
PAD_MODES = [x + y for x in AXIS_MODES for y in AXIS_MODES]


@pytest.mark.parametrize("ext", [1, 3])
@pytest.mark.parametrize("shape", SMALL)
def test_slab_twins_equal_the_whole_grid_kernels(shape, ext):
    """Every legal slab (with and without the duplicate face row), all 25 pad-mode combinations of the pressure, 2 and 4 channels, all four
    wraps, extended rows of ext = 1 (the least the kernels read) and 3 (R = 2)."""
    ny, nx = shape
    I = Inputs(nx, ny, 17)
    w = dict(vel=I.randn(I.nf), p=I.randn(I.nc), g4=I.randn(I.nc * 4), g2=I.randn(I.nc * 2), out=I.randn(I.nc * 2), df=I.randn(I.nf))
    two_dx = 0.37

    def run(X, modes_list, wraps):
        S = X.S
        f = dict(vel=S.put("faces", w["vel"]), p=S.put("cells", w["p"]), g4=S.put("nhwc4_in", w["g4"]), g2=S.put("nhwc2_in", w["g2"]),
                 out=S.put("nhwc2_in", w["out"]), df=S.put("faces", w["df"]))
        o = {}
        for modes in modes_list:
            o["input 4 %s" % (modes,)] = op_input(X, f["vel"], f["p"], 4, modes, two_dx)
            o["input adjoint 4 %s" % (modes,)] = op_input_adjoint(X, f["g4"], 4, modes, two_dx)
        if modes_list:
            o["input 2"] = op_input(X, f["vel"], None, 2, modes_list[0], two_dx)
            o["input adjoint 2"] = op_input_adjoint(X, f["g2"], 2, modes_list[0], two_dx)
        for wrap in wraps:
            o["force %s" % (wrap,)] = op_force(X, f["out"], wrap)
            o["force adjoint %s" % (wrap,)] = op_force_adjoint(X, f["df"], wrap)
        return o
    XW = Ext(E.WholeLayout(nx, ny))
    tally = E.Tally()
    ref = run(XW, PAD_MODES, WRAPS)
    for k, o in ref.items():
        tally.launch("whole grid %s" % k, XW.S, o, None)
    for rb, re, last in slabs_of(ny):
        for ring in (False, True):        # the extended rows depend on whether y is a ring: the pressure's y mode / the resampling's wrap_y
            X = Ext(E.SlabLayout(nx, ny, rb, re, last), ext, ring)
            modes_list = [m for m in PAD_MODES if (m[2] == 2) == ring]
            wraps = [wr for wr in WRAPS if wr[0] == ring]
            for k, o in run(X, modes_list, wraps).items():
                tally.launch("slab [%d, %d) last %d ext %d ring %d: %s" % (rb, re, last, ext, ring, k), X.S, o, ref[k])
    finish(tally)


def test_halo_add_adds_and_touches_nothing_else():
    from diffpiso import _native as N
    I = Inputs(4, 4, 1)
    n = 3 * 257
    W = E.Space(E.WholeLayout(4, 10))
    dst = E.Guarded(E._filled(n + 2 * W.band, torch.float32, "cuda"), W.band, n)
    a, b = I.randn(n), I.randn(n)
    dst.t.copy_(a)
    assert N.lib.piso_closure_halo_add(E.ptr(dst), C_ptr(b), n, E._stream()) == 0
    want = E._filled(n + 2 * W.band, torch.float32, "cuda")
    want[W.band:W.band + n] = a + b
    assert bool(same_bits(dst.buf, want))


def C_ptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr())


def test_slab_twins_refuse_extended_rows_that_miss_a_row_they_read():
    """Before any launch (PISO_ERR_INVALID_ARG, outputs keep their pre-fill): an interior slab without a lower extended row."""
    from diffpiso import _native as N
    ny, nx = 12, 5
    X = Ext(E.SlabLayout(nx, ny, 4, 8, 0), 1, False)
    S = X.S
    I = Inputs(nx, ny, 2)
    out_f, out_c, g = S.out("faces"), S.out("cells"), S.put("nhwc4", I.randn(I.nc * 4))
    modes = E.pad_modes_c((1, 1, 1, 1))
    st = [N.lib.piso_closure_force_slab(E.ptr(S.put("nhwc2", I.randn(I.nc * 2))), E.ptr(out_f), nx, ny, 0, 0, E._stream(), S.slab_ptr, 0, 1),
          N.lib.piso_closure_input_adjoint_slab(E.ptr(g), E.ptr(out_f), E.ptr(out_c), nx, ny, 4, modes, C.c_double(1.0), E._stream(), S.slab_ptr, 0, 1),
          N.lib.piso_closure_input_adjoint_slab(E.ptr(g), E.ptr(out_f), E.ptr(out_c), nx, ny, 4, modes, C.c_double(1.0), E._stream(), S.slab_ptr, 1, 0),
          N.lib.piso_closure_input_slab(E.ptr(S.put("faces", I.randn(I.nf))), None, E.ptr(g), nx, ny, 3, modes, C.c_double(1.0), E._stream(), S.slab_ptr, 1, 1)]
    assert st == [E.INVALID_ARG] * 4, st
    nothing_f = torch.zeros(S.n("faces"), dtype=torch.bool, device="cuda")
    nothing_c = torch.zeros(S.n("cells"), dtype=torch.bool, device="cuda")
    assert bool(S.check("faces", out_f, out_f.t, nothing_f)) and bool(S.check("cells", out_c, out_c.t, nothing_c))
