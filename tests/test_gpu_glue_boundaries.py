"""The whole-grid face operators and the divergence adjoint (csrc/glue.hip) on every pressure boundary combination the kernels accept -
all 25 `pad_modes`, with and without the accessible mask - against oracle/piso_ref.py evaluated in float64.  The slab tests
(tests/test_gpu_slab_twins.py) compare the twins with THESE kernels; tests/test_gpu_fused.py reaches only the four set-ups' pad modes.

Bounds are a few float32 ulps of the summands (K_ULP * 2^-23 * sum of the magnitudes that enter an element), never a relative error
of the result: a gradient cancels.  The spacings are exact in float32, so the kernel and the float64 reference see the same numbers."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from tests import slab_emulation as E
from tests.test_gpu_slab_twins import PAD_MODES, Inputs, face_inputs

pytestmark = pytest.mark.gpu
SHAPES = [(13, 9), (37, 70)]
G3 = dict(hx=0.375, hy=0.625, dxdy=0.234375, beta=2.5)           # hx != hy, all four exact in float32
EPS, K_ULP = 2.0 ** -23, 4.0
NAMES = {0: "constant", 1: "boundary", 2: "periodic"}


def p_extrapolation(modes):
    """(x_lo, x_hi, y_lo, y_hi) of the kernels -> the oracle's per-axis (y, x) specification."""
    def axis(lo, hi):
        return "periodic" if lo == 2 else (NAMES[lo], NAMES[hi])
    return (axis(modes[2], modes[3]), axis(modes[0], modes[1]))


@contextlib.contextmanager
def float64_oracle():
    """oracle/piso_ref.py casts through its module-level `f32`: with that name bound to float64 the same statements run in float64."""
    from oracle import piso_ref as R
    saved = R.f32
    R.f32 = np.float64
    try:
        yield R
    finally:
        R.f32 = saved


def host(g):
    return g.t.detach().cpu().numpy().astype(np.float64)


def worst(got, want, tol):
    """max of |got - want| / tol (elementwise tol), and where."""
    r = (np.abs(got - want) / tol).reshape(-1)
    k = int(np.argmax(r))
    return float(r[k]), k


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_face_operators_against_the_float64_reference_on_all_pad_modes(shape, masked):
    ny, nx = shape
    n_u = (nx + 1) * ny
    I = Inputs(nx, ny, 21)
    w = face_inputs(I)
    w["zero"] = ("faces", torch.zeros(I.nf, device="cuda"))
    d0 = w["d0"][1]
    w["d0_u"] = ("faces", torch.cat([d0[:n_u], torch.zeros_like(d0[n_u:])]))
    w["d0_v"] = ("faces", torch.cat([torch.zeros_like(d0[:n_u]), d0[n_u:]]))
    W = E.Space(E.WholeLayout(nx, ny))
    f = {k: W.put(kind, v) for k, (kind, v) in w.items()}
    acc = f["acc"] if masked else None
    runs = []
    for modes in PAD_MODES:                                     # every launch first, the host comparisons afterwards
        o = {}
        o["fwd0"] = E.op_face_forward(W, 0, modes, G3, f["p"], acc, None, f["in0"], f["in1"], f["in2"], f["dmask"])
        o["fwd1"] = E.op_face_forward(W, 1, modes, G3, f["p"], acc, f["a"], f["in0"], None, None, None)
        o["fwd2"] = E.op_face_forward(W, 2, modes, G3, f["p"], acc, f["a"], f["in0"], f["in1"], None, None)
        o["bwd0"] = E.op_face_backward(W, 0, modes, G3, acc, None, f["dmask"], f["d0"], None, True, True)
        o["bwd1"] = E.op_face_backward(W, 1, modes, G3, acc, f["a"], None, f["d0"], f["d1"], False, False)
        o["bwd2"] = E.op_face_backward(W, 2, modes, G3, acc, f["a"], None, f["d0"], None, True, False)
        o["minus G"] = E.op_face_forward(W, 0, modes, G3, f["p"], acc, None, f["zero"], None, None, None)      # 0 * beta - G(p)
        o["GT u"] = E.op_face_backward(W, 0, modes, G3, acc, None, None, f["d0_u"], None, False, False)           # d_p = G^T(-d0): x axis alone
        o["GT v"] = E.op_face_backward(W, 0, modes, G3, acc, None, None, f["d0_v"], None, False, False)           # ... y axis alone
        runs.append(o)
    h = {k: v.detach().cpu().numpy().astype(np.float64) for k, (_, v) in w.items()}
    dm = h["dmask"] != 0
    hx, hy, dxdy, beta = G3["hx"], G3["hy"], G3["dxdy"], G3["beta"]
    acc_t = h["acc"].reshape(1, ny + 2, nx + 2, 1) if masked else None
    p2 = h["p"].reshape(ny, nx)
    bmA = beta - h["a"]
    g_mag = 2.0 * np.abs(p2).max() * dxdy / min(hx, hy)          # what enters one face of G(p), in magnitude
    with float64_oracle() as R:
        def st(flat):
            return R.stagger_flattened(flat, nx, ny, True)
        mv, mu = R.gradient_mask(acc_t) if masked else (np.ones((ny + 1, nx)), np.ones((ny, nx + 1)))
        for modes, o in zip(PAD_MODES, runs):
            ext = p_extrapolation(modes)
            G = R.flatten_staggered(R.fv_gradient(p2, ext, (hy, hx), acc_t), True)
            want = R.arrange_rhs(st(h["in0"] * beta - G + h["in1"] * dxdy), st(dm.astype(np.float64)), st(h["in2"]))
            tol = K_ULP * EPS * (np.abs(h["in0"]) * beta + g_mag + np.abs(h["in1"]) * dxdy + np.abs(h["in2"]))
            r, k = worst(host(o["fwd0"]["out0"][1]), want, tol)
            assert r <= 1.0, ("mode 0", modes, r, k)
            want0 = h["in0"] - (G / bmA) / dxdy
            tol0 = K_ULP * EPS * (np.abs(h["in0"]) + g_mag / np.abs(bmA) / dxdy)
            r, k = worst(host(o["fwd1"]["out0"][1]), want0, tol0)
            assert r <= 1.0, ("mode 1 out0", modes, r, k)
            r, k = worst(host(o["fwd1"]["out1"][1]), want0 - h["in0"], tol0 + EPS * np.abs(want0 - h["in0"]))
            assert r <= 1.0, ("mode 1 out1", modes, r, k)
            want2 = h["in0"] + (h["in1"] - G / dxdy) / bmA
            r, k = worst(host(o["fwd2"]["out0"][1]), want2, K_ULP * EPS * (np.abs(h["in0"]) + (np.abs(h["in1"]) + g_mag / dxdy) / np.abs(bmA)))
            assert r <= 1.0, ("mode 2", modes, r, k)
            # d_p: the reference's adjoint of G applied to the weight of G in each update (up to six summands |w| dxdy / h per cell)
            weights = {"bwd0": np.where(dm, 0.0, -h["d0"]), "bwd1": -(((h["d0"] + h["d1"]) / dxdy) / bmA), "bwd2": -((h["d0"] / bmA) / dxdy)}
            for key, wt in weights.items():
                want_p = R.fv_gradient_adjoint(st(wt), ext, (hy, hx), acc_t)
                tol_p = K_ULP * EPS * 6.0 * np.abs(wt).max() * dxdy / min(hx, hy)
                r, k = worst(host(o[key]["d_p"][1]).reshape(ny, nx), want_p, tol_p)
                assert r <= 1.0, (key, "d_p", modes, r, k)
            # axis by axis, from the kernels' own outputs
            mG = host(o["minus G"]["out0"][1])
            r, k = worst(mG, -G, K_ULP * EPS * g_mag)
            assert r <= 1.0, ("G", modes, r, k)
            for axis, key, sl, lo in ((1, "GT u", slice(0, n_u), modes[0]), (0, "GT v", slice(n_u, None), modes[2])):
                dp = host(o[key]["d_p"][1]).reshape(ny, nx)
                cot = h["d0"][sl]
                if lo != 2:
                    # not periodic: the reference's adjoint is the exact transpose, <G p, w> = <p, G^T w> (here: <-G p, w> = <p, G^T(-w)>)
                    lhs, rhs = float(np.sum(mG[sl] * cot)), float(np.sum(p2 * dp))
                    bound = 16 * EPS * (float(np.sum(np.abs(mG[sl] * cot))) + float(np.sum(np.abs(p2 * dp))))
                    assert abs(lhs - rhs) <= bound, ("dot-product identity", key, modes, lhs, rhs, bound)
                else:
                    # periodic: NOT the transpose - d p[c] = W[c] - W[c + 1] for c = 0 .. n - 1 and no wrap term (the duplicate face n feeds
                    # cell n - 1 only, face 0 feeds cell 0 only)
                    if axis == 0:
                        Wf = ((-cot.reshape(ny + 1, nx) * mv) / hy) * dxdy
                        explicit = Wf[:-1, :] - Wf[1:, :]
                    else:
                        Wf = ((-cot.reshape(ny, nx + 1) * mu) / hx) * dxdy
                        explicit = Wf[:, :-1] - Wf[:, 1:]
                    r, k = worst(dp, explicit, K_ULP * EPS * 2.0 * np.abs(Wf).max())
                    assert r <= 1.0, ("periodic adjoint without wrap term", key, modes, r, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_divergence_adjoint_against_the_float64_reference_on_all_periodicities(shape):
    ny, nx = shape
    n_u = (nx + 1) * ny
    I = Inputs(nx, ny, 23)
    dc_t = I.randn(I.nc)
    W = E.Space(E.WholeLayout(nx, ny))
    dc = W.put("cells", dc_t)
    pers = list(itertools.product((0, 1), (0, 1)))
    outs = [E.op_divergence_adjoint(W, dc, px, py, G3)["d_faces"][1] for px, py in pers]
    d2 = dc_t.cpu().numpy().astype(np.float64).reshape(ny, nx)
    hx, hy, dxdy = G3["hx"], G3["hy"], G3["dxdy"]
    tol = K_ULP * EPS * 2.0 * np.abs(d2).max() * dxdy / min(hx, hy)

    def fy(a):
        return (a * dxdy) / hy

    def fx(a):
        return (a * dxdy) / hx
    with float64_oracle() as R:
        for (px, py), g in zip(pers, outs):
            got = host(g)
            want = R.flatten_staggered(R.fv_divergence_adjoint(d2, (bool(py), bool(px)), (hy, hx)), True)
            r, k = worst(got, want, tol)
            assert r <= 1.0, (px, py, r, k)
            u, v = got[:n_u].reshape(ny, nx + 1), got[n_u:].reshape(ny + 1, nx)
            # the reference's deviation from the transpose, stated: a periodic axis feeds face 0 with dc[n - 2] (not dc[n - 1]) and the
            # duplicate face n with dc[0] and dc[n - 1]; a closed axis feeds both end faces with one cell only
            first_v = -fy(d2[0]) + (fy(d2[ny - 2]) if py else 0.0)
            last_v = (-fy(d2[0]) if py else 0.0) + fy(d2[ny - 1])
            first_u = -fx(d2[:, 0]) + (fx(d2[:, nx - 2]) if px else 0.0)
            last_u = (-fx(d2[:, 0]) if px else 0.0) + fx(d2[:, nx - 1])
            for name, a, b in (("v[0]", v[0], first_v), ("v[ny]", v[ny], last_v), ("u[:, 0]", u[:, 0], first_u), ("u[:, nx]", u[:, nx], last_u)):
                assert np.abs(a - b).max() <= tol, (px, py, name)
