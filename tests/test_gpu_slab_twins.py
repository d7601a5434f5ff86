"""Every `*_slab` entry point of the step against its whole-grid entry point, on ONE GPU in one process - no communicator, no peer
mapping, no subprocess.  For a slab the twin runs on the stored rows of the SAME inputs (tests/slab_emulation.py cuts them out by the
text of include/piso_hip.h, halos populated) and must
  (a) give the whole-grid launch's owned rows bit for bit,
  (b) leave every other stored element of every output, and the guard bands around it, at the pre-fill pattern,
  (c) leave no owned element unwritten.
Slabs: every legal (row_begin, row_end) on the grids with ny = 10, 12, 13 - which takes in the smallest and the largest slab, the first
slab of a non-periodic grid (its lower halo rows wrap to ny - 2, ny - 1 and must not be used), slabs whose v ring crosses the seam
while they own neither end, and the last cell row with and without the duplicate face row - and five picked slabs on the larger grids."""
import itertools

import numpy as np
import pytest
import torch

from tests import slab_emulation as E
from tests.cases import make_case

pytestmark = pytest.mark.gpu
CASES = ["periodic", "xper_ywall", "cavity", "spatial_ml"]
SMALL = [(10, 5), (12, 5), (13, 4)]
LARGE = [(37, 70), (64, 129), (24, 600)]
GEO = dict(hx=0.37, hy=0.61, dxdy=0.37 * 0.61, beta=2.5)        # hx != hy: a kernel that mixes the two up is not bit-equal to itself
AXIS_MODES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)]
PAD_MODES = [x + y for x in AXIS_MODES for y in AXIS_MODES]     # (x_lo, x_hi, y_lo, y_hi): all 25 the kernels accept
_PAD = {"constant": 0, "boundary": 1, "periodic": 2}


def slabs_of(ny):
    return E.with_last(ny, E.legal_slabs(ny) if ny <= 13 else E.picked_slabs(ny))


class Inputs(object):
    """Seeded whole-grid inputs on the device."""

    def __init__(self, nx, ny, seed):
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self.nx, self.ny = nx, ny
        self.nf, self.nc, self.nm = (nx + 1) * ny + nx * (ny + 1), nx * ny, (nx + 2) * (ny + 2)

    def randn(self, n, scale=1.0):
        return (scale * torch.randn(n, generator=self.gen)).cuda()

    def bits(self, n, p=0.3, dtype=torch.uint8):
        return (torch.rand(n, generator=self.gen) < p).to(dtype).cuda()


def case_modes(c):
    out = []
    for axis in (1, 0):
        e = c["p_ext"][axis]
        lo, hi = (e, e) if isinstance(e, str) else e
        out += [_PAD[lo], _PAD[hi]]
    return tuple(out)


def spaces(nx, ny, per_x=0, per_y=0):
    yield from ((rb, re, last, E.Space(E.SlabLayout(nx, ny, rb, re, last, per_x, per_y))) for rb, re, last in slabs_of(ny))


def finish(tally):
    assert len(tally) > 0
    bad = tally.failures()
    assert not bad, "%d launches checked; first failures: %s" % (len(tally), bad)


# ---------------------------------------------------------------------------------------------------------------- glue without a pressure gradient
@pytest.mark.parametrize("shape", SMALL + LARGE)
def test_elementwise_and_divergence_twins(shape):
    """piso_pad_velocity (four periodicities), piso_a0_vfirst, piso_divergence, piso_divergence_adjoint (four periodicities),
    piso_h_contribution and its adjoint with d_h present and NULL."""
    ny, nx = shape
    I = Inputs(nx, ny, 11)
    W = E.Space(E.WholeLayout(nx, ny))
    w = dict(vel=I.randn(I.nf), a=I.randn(I.nf, 0.3), dc=I.randn(I.nc), md=I.randn(I.nf), delta=I.randn(I.nf), dh=I.randn(I.nf), dhb=I.randn(I.nf))
    pers = list(itertools.product((0, 1), (0, 1)))

    def run(S):
        f = {k: S.put("cells" if k == "dc" else "faces", v) for k, v in w.items()}
        outs = {}
        for px, py in pers:
            outs["pad%d%d" % (px, py)] = E.op_pad_velocity(S, f["vel"], px, py)
            outs["diva%d%d" % (px, py)] = E.op_divergence_adjoint(S, f["dc"], px, py, GEO)
        outs["a0"] = E.op_a0_vfirst(S, f["a"], GEO["beta"], 1.7)
        outs["div"] = E.op_divergence(S, f["vel"], GEO)
        outs["h"] = E.op_h_contribution(S, f["md"], f["delta"], f["a"], GEO["beta"])
        outs["hadj"] = E.op_h_contribution_adjoint(S, f["dh"], f["dhb"], f["a"], GEO["beta"])
        outs["hadj_null"] = E.op_h_contribution_adjoint(S, None, f["dhb"], f["a"], GEO["beta"])
        return outs
    tally = E.Tally()
    ref = run(W)
    for k, o in ref.items():
        tally.launch("whole grid %s" % k, W, o, None)
    for rb, re, last, S in spaces(nx, ny):
        for k, o in run(S).items():
            tally.launch("slab [%d, %d) last %d: %s" % (rb, re, last, k), S, o, ref[k])
    finish(tally)


# ---------------------------------------------------------------------------------------------------------------- the face operators
def face_launches(S, f, modes, k):
    """Forward modes 0 - 2 and their reverse mode for one pad-mode combination: with and without forcing, Dirichlet mask and
    accessible mask, with the optional outputs and inputs of the reverse mode present and NULL (k alternates what the single-variant
    modes get)."""
    acc_a, acc_b = (f["acc"], None) if k % 2 == 0 else (None, f["acc"])
    o = {}
    o["fwd0 bare"] = E.op_face_forward(S, 0, modes, GEO, f["p"], None, None, f["in0"], None, None, None)
    o["fwd0 forcing dirichlet mask"] = E.op_face_forward(S, 0, modes, GEO, f["p"], f["acc"], None, f["in0"], f["in1"], f["in2"], f["dmask"])
    o["fwd1"] = E.op_face_forward(S, 1, modes, GEO, f["p"], acc_a, f["a"], f["in0"], None, None, None)
    o["fwd2"] = E.op_face_forward(S, 2, modes, GEO, f["p"], acc_b, f["a"], f["in0"], f["in1"], None, None)
    o["bwd0 all"] = E.op_face_backward(S, 0, modes, GEO, f["acc"], None, f["dmask"], f["d0"], None, True, True)
    o["bwd0 bare"] = E.op_face_backward(S, 0, modes, GEO, None, None, None, f["d0"], None, False, False)
    o["bwd1 d_out1"] = E.op_face_backward(S, 1, modes, GEO, acc_b, f["a"], None, f["d0"], f["d1"], False, False)
    o["bwd1 null"] = E.op_face_backward(S, 1, modes, GEO, acc_a, f["a"], None, f["d0"], None, False, False)
    o["bwd2"] = E.op_face_backward(S, 2, modes, GEO, acc_a, f["a"], None, f["d0"], None, True, False)
    return o


def face_inputs(I):
    return dict(p=("cells", I.randn(I.nc)), acc=("mask", I.bits(I.nm, 0.8, torch.float32)), a=("faces", I.randn(I.nf, 0.3)),
                in0=("faces", I.randn(I.nf)), in1=("faces", I.randn(I.nf)), in2=("faces", I.randn(I.nf)), dmask=("faces", I.bits(I.nf)),
                d0=("faces", I.randn(I.nf)), d1=("faces", I.randn(I.nf)))


@pytest.mark.parametrize("shape", SMALL)
def test_face_operator_twins_over_all_pad_modes(shape):
    ny, nx = shape
    I = Inputs(nx, ny, 5)
    w = face_inputs(I)
    W = E.Space(E.WholeLayout(nx, ny))
    fw = {k: W.put(kind, v) for k, (kind, v) in w.items()}
    tally = E.Tally()
    ref = [face_launches(W, fw, modes, k) for k, modes in enumerate(PAD_MODES)]
    for modes, r in zip(PAD_MODES, ref):
        for k, o in r.items():
            tally.launch("whole grid %s %s" % (modes, k), W, o, None)
    for rb, re, last, S in spaces(nx, ny):
        fs = {k: S.put(kind, v) for k, (kind, v) in w.items()}
        for n, modes in enumerate(PAD_MODES):
            for k, o in face_launches(S, fs, modes, n).items():
                tally.launch("slab [%d, %d) last %d, pad modes %s: %s" % (rb, re, last, modes, k), S, o, ref[n][k])
    finish(tally)


# ---------------------------------------------------------------------------------------------------------------- the four set-ups
def setup_inputs(c, I):
    ny, nx = c["ny"], c["nx"]
    from oracle import piso_ref as R
    dm = torch.as_tensor(R.flatten_staggered(c["dirichlet_mask"], True).astype(np.uint8)).cuda()
    vel = torch.as_tensor(R.flatten_staggered(c["vel"], True)).cuda()
    ns = None if c["no_slip"] is None else torch.as_tensor(np.asarray(c["no_slip"]).astype(np.uint8).ravel()).cuda()
    return dict(vel=("faces", vel), dmask=("faces", dm), active=("mask", torch.as_tensor(c["active"].ravel()).cuda()),
                acc=("mask", torch.as_tensor(c["accessible"].ravel()).cuda()), no_slip=("mask", ns),
                visc=("faces", (1e-2 * (1.0 + torch.rand(I.nf, generator=I.gen))).cuda()), x=("faces", I.randn(I.nf)),
                p=("cells", I.randn(I.nc)), a=("faces", I.randn(I.nf, 0.3)), in0=("faces", I.randn(I.nf)), in1=("faces", I.randn(I.nf)),
                in2=("faces", I.randn(I.nf)), d0=("faces", I.randn(I.nf)), d1=("faces", I.randn(I.nf)))


def setup_launches(S, f, c, visc1, ref=None, faces=True):
    """What one set-up runs on a Space: padding, assembly (scalar and per-face viscosity, with and without the no-slip mask; slab: the
    pattern-only launch as well), both CSR products, A0, both Laplacians and - with the set-up's own pad modes and masks - the face
    operators.  The chain feeds the whole-grid launch's outputs to the twin (ref), cut to its stored rows."""
    per_y, per_x = [int(b) for b in c["periodic_yx"]]
    o = {}
    o["pad"] = E.op_pad_velocity(S, f["vel"], per_x, per_y)
    pad = o["pad"]["vel_pad"][1] if ref is None else S.put("pad", ref["pad"]["vel_pad"][1].t)
    o["assemble scalar"] = E.op_assemble(S, pad, f["dmask"], f["active"], visc1, 0, f["no_slip"], GEO)
    o["assemble field"] = E.op_assemble(S, pad, f["dmask"], f["active"], f["visc"], 1, None, GEO)
    if ref is not None:
        o["assemble pattern"] = E.op_assemble(S, None, None, None, None, 0, None, GEO, pattern_only=1)
    src = (o if ref is None else ref)["assemble scalar"]
    val, col = [S.put("csr", src[k][1].t) for k in ("val", "col")]
    rp = S.row_pointers()
    diag = S.put("faces", src["diag"][1].t)
    o["matvec"] = E.op_matvec(S, val, rp, col, f["x"], 0)
    o["matvec T"] = E.op_matvec(S, val, rp, col, f["x"], 1)
    o["a0"] = E.op_a0_vfirst(S, diag, GEO["beta"], 0.61)
    a0 = S.put("faces_vfirst", (o if ref is None else ref)["a0"]["a0"][1].t)
    o["laplace f32"] = E.op_laplace(S, torch.float32, f["active"], f["acc"], a0)
    o["laplace f64"] = E.op_laplace(S, torch.float64, f["active"], f["acc"], a0)
    if faces:
        modes = case_modes(c)
        o["fwd0"] = E.op_face_forward(S, 0, modes, GEO, f["p"], f["acc"], None, f["in0"], f["in1"], f["in2"], f["dmask"])
        o["fwd1"] = E.op_face_forward(S, 1, modes, GEO, f["p"], f["acc"], f["a"], f["in0"], None, None, None)
        o["fwd2"] = E.op_face_forward(S, 2, modes, GEO, f["p"], f["acc"], f["a"], f["in0"], f["in1"], None, None)
        o["bwd0"] = E.op_face_backward(S, 0, modes, GEO, f["acc"], None, f["dmask"], f["d0"], None, True, True)
        o["bwd1"] = E.op_face_backward(S, 1, modes, GEO, f["acc"], f["a"], None, f["d0"], f["d1"], False, False)
        o["bwd2"] = E.op_face_backward(S, 2, modes, GEO, f["acc"], f["a"], None, f["d0"], None, True, False)
    return o


def check_setup(tally, label, S, o, ref):
    for k, outs in o.items():
        if k == "assemble pattern":
            # columns and row pointers of EVERY stored row, no value and no diagonal
            everything = {kind: torch.ones(S.n(kind), dtype=torch.bool, device=S.device) for kind in ("csr", "csr_rp")}
            nothing = {kind: torch.zeros(S.n(kind), dtype=torch.bool, device=S.device) for kind in ("csr", "faces")}
            src = ref["assemble scalar"]
            flag = (S.check("csr", outs["col"][1], src["col"][1].t, everything["csr"]) & S.check("csr_rp", outs["rowptr"][1], None, everything["csr_rp"])
                    & S.check("csr", outs["val"][1], src["val"][1].t, nothing["csr"]) & S.check("faces", outs["diag"][1], src["diag"][1].t, nothing["faces"]))
            tally.add("%s: %s" % (label, k), flag)
        else:
            tally.launch("%s: %s" % (label, k), S, outs, None if ref is None else ref[k])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", SMALL + LARGE)
def test_set_up_twins(name, shape):
    ny, nx = shape
    c = make_case(name, ny, nx, seed=3)
    per_y, per_x = [int(b) for b in c["periodic_yx"]]
    I = Inputs(nx, ny, 7)
    w = setup_inputs(c, I)
    visc_w = torch.full((1,), 1e-2).cuda()
    W = E.Space(E.WholeLayout(nx, ny, per_x, per_y))
    tally = E.Tally()
    ref = setup_launches(W, {k: W.put(kind, v) for k, (kind, v) in w.items()}, c, E.Guarded(visc_w, 0, 1))
    check_setup(tally, "whole grid", W, ref, None)
    for rb, re, last, S in spaces(nx, ny, per_x, per_y):
        o = setup_launches(S, {k: S.put(kind, v) for k, (kind, v) in w.items()}, c, E.Guarded(visc_w, 0, 1), ref)
        check_setup(tally, "slab [%d, %d) last %d" % (rb, re, last), S, o, ref)
    finish(tally)


def test_largest_slab_of_a_grid_that_reaches_the_launch_caps():
    """1100 x 1030 with the (ny - 6)-row slab: more than 2048 x 512 elements per launch, so the glue kernels' grid is capped and every
    thread's grid-stride loop runs more than once."""
    ny, nx = 1100, 1030
    c = make_case("spatial_ml", ny, nx, seed=1)
    I = Inputs(nx, ny, 9)
    w = setup_inputs(c, I)
    assert (ny - 6) * nx > 2048 * 512
    w.update(dc=("cells", I.randn(I.nc)))
    visc_w = torch.full((1,), 1e-2).cuda()
    W = E.Space(E.WholeLayout(nx, ny))
    S = E.Space(E.SlabLayout(nx, ny, 3, 3 + ny - 6, 0))
    tally = E.Tally()

    def run(X, ref):
        f = {k: X.put(kind, v) for k, (kind, v) in w.items()}
        o = setup_launches(X, f, c, E.Guarded(visc_w, 0, 1), ref)
        o["div"] = E.op_divergence(X, f["vel"], GEO)
        o["diva"] = E.op_divergence_adjoint(X, f["dc"], 0, 1, GEO)
        o["h"] = E.op_h_contribution(X, f["in0"], f["in1"], f["a"], GEO["beta"])
        o["hadj"] = E.op_h_contribution_adjoint(X, f["d0"], f["d1"], f["a"], GEO["beta"])
        return o
    ref = run(W, None)
    check_setup(tally, "whole grid", W, ref, None)
    check_setup(tally, "slab [3, %d)" % (ny - 3), S, run(S, ref), ref)
    finish(tally)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_one_twin_of_each_source_file_refuses_an_illegal_slab():
    """glue.hip (piso_divergence_slab), assembly.hip (piso_assemble_csr_slab), laplace.hip (piso_laplace_matrix_f32_slab) and
    bicgstab.hip (piso_csr_matvec_f32_slab) return PISO_ERR_INVALID_ARG before they launch anything: the outputs keep their pre-fill."""
    from diffpiso import _native as N
    ny, nx = 16, 9
    W = E.Space(E.WholeLayout(nx, ny))
    I = Inputs(nx, ny, 1)
    faces, mask, one = W.put("faces", I.randn(I.nf)), W.put("mask", I.bits(I.nm, 0.8, torch.float32)), W.put("faces", I.randn(I.nf))
    dm = W.put("faces", I.bits(I.nf))
    pad = W.put("pad", I.randn(W.n("pad")))
    outs = dict(cells=W.out("cells"), val=W.out("csr"), col=W.out("csr", torch.int32), rp=W.out("csr_rp", torch.int32), diag=W.out("faces"),
                lap=W.out("laplace"), y=W.out("faces"))
    p, f, s = E.ptr, E.f32c, N.stream_ptr()
    for label, (nyg, rb, re, last) in E.refused_slabs(ny).items():
        slab = E.slab_struct(nyg, rb, re, last)
        sp = N._sp(slab)
        got = [N.lib.piso_divergence_slab(p(faces), p(outs["cells"]), nx, ny, f(1.0), f(1.0), f(1.0), s, sp),
               N.lib.piso_assemble_csr_slab(p(pad), p(outs["val"]), p(outs["col"]), p(outs["rp"]), p(outs["diag"]), p(dm), p(mask), p(one), 0, nx, ny,
                                            0, 0, f(1.0), f(1.0), f(1.0), f(1.0), None, f(1.0), s, sp, 0),
               N.lib.piso_laplace_matrix_f32_slab(nx, ny, p(mask), p(mask), p(faces), p(outs["lap"]), s, sp),
               N.lib.piso_csr_matvec_f32_slab(p(outs["val"]), p(outs["rp"]), p(outs["col"]), p(faces), p(outs["y"]), nx, ny, 0, 0, 0, s, sp)]
        assert got == [E.INVALID_ARG] * 4, (label, got)
    nothing = {k: torch.zeros(g.t.numel(), dtype=torch.bool, device="cuda") for k, g in outs.items()}
    kinds = dict(cells="cells", val="csr", col="csr", rp="csr_rp", diag="faces", lap="laplace", y="faces")
    for k, g in outs.items():
        assert bool(W.check(kinds[k], g, g.t, nothing[k])), k
