"""The `*_slab` twins of the loss kernels (csrc/loss.hip) against their whole-grid entry points, on ONE GPU in one process, through a bare
piso_slab_t - no communicator (the pattern of tests/test_gpu_slab_twins.py; the row map is tests/slab_emulation.py's restatement of the
header's text).  For every legal slab of 10-, 12- and 13-row grids, with the halo rows of prediction and target filled from the whole field:
  gradient   the owned faces bit for bit the whole-grid kernel's; every other stored element and the guard bands keep the pre-fill (a launch
             writes the owned faces and nothing else), no owned face is left unwritten; through the Python operator, whose buffer starts
             as zeros, the halo entries of the gradient ARE zero
  value      the values of the slabs of a partition of the grid add up to the whole-grid value to 1e-12 relative - float64 re-association
             only.  Every partition into legal slabs is taken (12 rows: 4 + 4 + 4 and 6 + 6; 13 rows: 6 + 7, 4 + 4 + 5, ... in every order;
             10 rows admit none - a legal slab has 4 <= rows <= ny - 6 = 4 - so there the L2 value of every slab is held to the whole-grid
             kernel on a prediction that equals the target outside the slab's owned faces, and the strain value is covered by 12 and 13)
Both losses, the four windows of tests/test_gpu_loss_kernels.py and the velocity fields of the four boundary set-ups."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import slab_emulation as E
from tests.cases import make_case

pytestmark = pytest.mark.gpu
CASES = ["periodic", "xper_ywall", "cavity", "spatial_ml"]
SHAPES = [(10, 12), (12, 16), (13, 9)]
DX_YX = (0.61, 0.37)
L2_FACTOR, STRAIN_FACTOR = 50.0, 2.0
SUM_RTOL = 1e-12


def windows(ny, nx):
    from diffpiso.losses import loss_window
    return [loss_window(bw, sponge, ny, nx) for bw, sponge in ((None, 0), ([[1, 2], [2, 1]], 0), ([[0, 0], [3, 0]], 7), ([[4, ny - 4], [1, 1]], 0))]


def partitions(ny):
    """Every way to cut ny rows into legal slabs, as lists of (row_begin, row_end)."""
    def cut(at):
        if at == ny:
            yield []
        for rows in range(4, ny - 6 + 1):
            if at + rows <= ny:
                for rest in cut(at + rows):
                    yield [(at, at + rows)] + rest
    return [p for p in cut(0) if p]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    from diffpiso import _native as N
    return N.stream_ptr()


class Scalars(object):
    """The upstream scalar, the workspace and the value slots (a double between two NaN guards each) of one test."""

    def __init__(self):
        from diffpiso import _native as N
        self.up = torch.tensor([0.75], dtype=torch.float32, device="cuda")
        self.ws = torch.empty(int(N.lib.piso_loss_workspace_bytes()), dtype=torch.uint8, device="cuda")
        self.slots = []

    def slot(self):
        s = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        self.slots.append(s)
        return s


def op_l2_grad(S, pred, tgt, window, sc):
    out = S.out("faces")
    S.call("piso_loss_l2_grad", E.ptr(pred), E.ptr(tgt), S.nx, S.ny, *window, E.f32c(L2_FACTOR), _ptr(sc.up), E.ptr(out), _stream())
    return {"d_pred": ("faces", out)}


def op_strain_grad(S, pred, tgt, sc):
    out = S.out("faces")
    S.call("piso_loss_strain_grad", E.ptr(pred), E.ptr(tgt), S.nx, S.ny, E.f32c(DX_YX[1]), E.f32c(DX_YX[0]), C.c_double(STRAIN_FACTOR), _ptr(sc.up),
           E.ptr(out), _stream())
    return {"d_pred": ("faces", out)}


def op_l2_value(S, pred, tgt, window, sc):
    s = sc.slot()
    S.call("piso_loss_l2", E.ptr(pred), E.ptr(tgt), S.nx, S.ny, *window, C.c_double(L2_FACTOR), _ptr(s[1:]), _ptr(sc.ws), C.c_size_t(sc.ws.numel()),
           _stream())
    return s


def op_strain_value(S, pred, tgt, sc):
    s = sc.slot()
    S.call("piso_loss_strain", E.ptr(pred), E.ptr(tgt), S.nx, S.ny, E.f32c(DX_YX[1]), E.f32c(DX_YX[0]), C.c_double(STRAIN_FACTOR), _ptr(s[1:]),
           _ptr(sc.ws), C.c_size_t(sc.ws.numel()), _stream())
    return s


def fields_of(name, ny, nx):
    """Whole-grid prediction (the set-up's velocity) and target (the same, perturbed) as flat u-first vectors on the device."""
    from oracle import piso_ref as R
    c = make_case(name, ny, nx, seed=3)
    pred = torch.as_tensor(R.flatten_staggered(c["vel"], True).astype(np.float32))
    g = torch.Generator().manual_seed(ny * 100 + nx)
    return pred.cuda(), (pred + 0.3 * torch.randn(pred.numel(), generator=g)).cuda()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_twins(name, shape):
    from diffpiso import losses
    ny, nx = shape
    pred, tgt = fields_of(name, ny, nx)
    wins = windows(ny, nx)
    sc = Scalars()
    W = E.Space(E.WholeLayout(nx, ny))
    wp, wt = W.put("faces", pred), W.put("faces", tgt)
    tally = E.Tally()
    ref = {("l2", k): op_l2_grad(W, wp, wt, w, sc) for k, w in enumerate(wins)}
    ref["strain"] = op_strain_grad(W, wp, wt, sc)
    for k, o in ref.items():
        tally.launch("whole grid %s" % (k,), W, o, None)
    whole_values = [op_l2_value(W, wp, wt, w, sc) for w in wins] + [op_strain_value(W, wp, wt, sc)]
    slab_values = {}
    for rb, re, last in E.with_last(ny, E.legal_slabs(ny)):
        S = E.Space(E.SlabLayout(nx, ny, rb, re, last))
        label = "slab [%d, %d) last %d" % (rb, re, last)
        sp, st = S.put("faces", pred), S.put("faces", tgt)        # every stored row from the whole field: the halo rows are filled
        own, idx = S.own("faces"), S.idx("faces")
        for k, w in enumerate(wins):
            tally.launch("%s: l2 gradient, window %s" % (label, w), S, op_l2_grad(S, sp, st, w, sc), ref[("l2", k)])
        tally.launch("%s: strain gradient" % label, S, op_strain_grad(S, sp, st, sc), ref["strain"])
        # the Python operators: zeros outside the owned faces, the whole-grid launch's bits on them
        for what, got, want in (("l2", losses.fused_l2_grad(sp.t, st.t, nx, ny, wins[1], L2_FACTOR, sc.up, S.slab_ptr), ref[("l2", 1)]),
                                ("strain", losses.fused_strain_grad(sp.t, st.t, nx, ny, DX_YX, STRAIN_FACTOR, sc.up, S.slab_ptr), ref["strain"])):
            whole = want["d_pred"][1].t
            tally.add("%s: %s operator, halo entries zero" % (label, what), (got[~own] == 0).all())
            tally.add("%s: %s operator, owned faces" % (label, what), (got[own].view(torch.int32) == whole[idx[own]].view(torch.int32)).all())
        slab_values[(rb, re, last)] = [op_l2_value(S, sp, st, w, sc) for w in wins] + [op_strain_value(S, sp, st, sc)]
        # L2 of one slab = the whole-grid kernel on a prediction that equals the target on every face the slab does not own
        keep = torch.zeros(pred.numel(), dtype=torch.bool, device="cuda")
        keep[idx[own]] = True
        masked = W.put("faces", torch.where(keep, pred, tgt))
        slab_values[(rb, re, last, "masked")] = [op_l2_value(W, masked, wt, w, sc) for w in wins]
    finish_values = []
    whole = [float(s[1]) for s in whole_values]
    assert all(v > 0 for v in whole[:2] + whole[4:]), whole
    for key, vals in slab_values.items():
        if len(key) == 4:
            for k, (a, b) in enumerate(zip(slab_values[key[:3]], vals)):
                a, b = float(a[1]), float(b[1])
                finish_values.append(("slab %s window %d: own L2 value %r, masked whole-grid %r" % (key[:3], k, a, b), abs(a - b), abs(b)))
    parts = partitions(ny)
    assert (ny == 10) == (not parts)
    for p in parts:
        keys = [(rb, re, 1 if re == ny else 0) for rb, re in p]
        for k in range(len(whole)):
            total = sum(float(slab_values[key][k][1]) for key in keys)
            finish_values.append(("partition %s, value %d: %r against %r" % (p, k, total, whole[k]), abs(total - whole[k]), abs(whole[k])))
    worst = 0.0
    for label, err, scale in finish_values:
        assert err <= SUM_RTOL * scale, label
        if scale > 0:
            worst = max(worst, err / (SUM_RTOL * scale))
    for s in sc.slots:
        assert bool(torch.isnan(s[0])) and bool(torch.isnan(s[2])) and not bool(torch.isnan(s[1])), "a value launch wrote beside its double"
    bad = tally.failures()
    assert not bad, "%d launches checked; first failures: %s" % (len(tally), bad)
    print("%s %dx%d: %d gradient launches bit-equal, %d value sums, worst error / 1e-12 = %.3g" % (name, ny, nx, len(tally), len(finish_values), worst))


def test_loss_twins_refuse_an_illegal_slab():
    """Every slab the header refuses returns PISO_ERR_INVALID_ARG before anything is launched: the outputs keep their pre-fill."""
    from diffpiso import _native as N
    ny, nx = 16, 9
    W = E.Space(E.WholeLayout(nx, ny))
    g = torch.Generator().manual_seed(1)
    faces = W.put("faces", torch.randn(W.n("faces"), generator=g).cuda())
    sc = Scalars()
    out = W.out("faces")
    value = sc.slot()
    for label, (nyg, rb, re, last) in E.refused_slabs(ny).items():
        sp = N._sp(E.slab_struct(nyg, rb, re, last))
        got = [N.lib.piso_loss_l2_slab(E.ptr(faces), E.ptr(faces), nx, ny, 0, ny + 1, 0, nx + 1, C.c_double(1.0), _ptr(value[1:]), _ptr(sc.ws),
                                       C.c_size_t(sc.ws.numel()), _stream(), sp),
               N.lib.piso_loss_l2_grad_slab(E.ptr(faces), E.ptr(faces), nx, ny, 0, ny + 1, 0, nx + 1, E.f32c(1.0), _ptr(sc.up), E.ptr(out), _stream(), sp),
               N.lib.piso_loss_strain_slab(E.ptr(faces), E.ptr(faces), nx, ny, E.f32c(1.0), E.f32c(1.0), C.c_double(1.0), _ptr(value[1:]), _ptr(sc.ws),
                                           C.c_size_t(sc.ws.numel()), _stream(), sp),
               N.lib.piso_loss_strain_grad_slab(E.ptr(faces), E.ptr(faces), nx, ny, E.f32c(1.0), E.f32c(1.0), C.c_double(1.0), _ptr(sc.up), E.ptr(out),
                                                _stream(), sp)]
        assert got == [E.INVALID_ARG] * 4, (label, got)
    nothing = torch.zeros(out.t.numel(), dtype=torch.bool, device="cuda")
    assert bool(W.check("faces", out, out.t, nothing)) and bool(torch.isnan(value).all())
