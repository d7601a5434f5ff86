"""The multigrid-preconditioned pressure CG (csrc/mg.hip, PisoPressureSolverMultigrid) on the GPU, held to its numpy twin
(tests/mg_reference.py), to the plain CG of the library, to the true residual in float64 on the host, and - at step level - to the
oracle fixtures with the bounds the plain solver is held to there."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import mg_reference as M
from tests.cases import laplace_case, product_setup

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("periodic", "xper_ywall", "cavity", "spatial_ml")
SHAPES = ((33, 70), (64, 256), (130, 129), (64, 64))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _system(name, shape, seed=3):
    ny, nx = shape
    s, L, b = laplace_case(name, ny, nx, seed)
    per_y, per_x = (bool(v) for v in s.periodic_yx)
    return s, np.asarray(L, np.float64).reshape(-1, 5), b, nx, ny, per_x, per_y, bool(s.rank_deficient)


def _matvec(L, nx, ny, per_x, per_y, x, c=0.0):
    return M.matrix(L, nx, ny, per_x, per_y) @ x + c * x.sum()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_level_operators_equal_the_twin(name, shape):
    from diffpiso.solvers import mg_level_native
    s, L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    H = M.Hierarchy(L, nx, ny, per_x, per_y)
    Ld = _dev(L)
    for l in range(len(H.levels)):
        want, nxl, nyl = H.level_rows(l)
        got, gx, gy = mg_level_native(nx, ny, per_x, per_y, Ld, l)
        assert (gx, gy) == (nxl, nyl)
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-13 * np.abs(want).max(), (name, shape, l)
    assert mg_level_native(nx, ny, per_x, per_y, Ld, len(H.levels)) is None


@pytest.mark.parametrize("sweeps", (1, 2, 3))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_one_cycle_equals_the_twin_with_and_without_the_tail(name, shape, sweeps, piso_option):
    import diffpiso._native as N
    from diffpiso.solvers import mg_vcycle_native
    s, L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    H = M.Hierarchy(L, nx, ny, per_x, per_y)
    Ld = _dev(L)
    rng = np.random.default_rng(7)
    a, c = rng.standard_normal(nx * ny), rng.standard_normal(nx * ny)
    za = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(a), sweeps).cpu().numpy()
    d = N.mg_last_dispatch()
    assert d["levels"] == len(H.levels) and d["sweeps"] == sweeps and d["cycles"] == 1 and 0 <= d["tail_first"] < d["levels"]
    zc = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(c), sweeps).cpu().numpy()
    want = H.cycle(a, sweeps)
    assert np.abs(za - want).max() <= 1e-11 * np.abs(want).max()
    assert abs(za @ c - a @ zc) <= 1e-12 * np.linalg.norm(a) * np.linalg.norm(c)
    assert za @ a < 0 and zc @ c < 0
    piso_option("mg_tail", 0)
    zl = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(a), sweeps).cpu().numpy()
    assert N.mg_last_dispatch()["tail_first"] == -1
    assert np.abs(zl - za).max() <= 1e-13 * np.abs(za).max()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_solve_against_twin_plain_cg_and_true_residual(name, shape):
    import diffpiso._native as N
    from diffpiso.solvers import cg_solve_native, mg_solve_native
    s, L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    Ld, bd = _dev(L), _dev(b)
    acc = 1e-10
    x, it = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, acc, 200, rd, 1 << 30)
    x = x.cpu().numpy()
    xt, itt = M.pcg(L, b, nx, ny, per_x, per_y, acc, 200, rd)
    xp, itp = cg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-12, 50000, rd, 1 << 30)
    xp = xp.cpu().numpy()
    print("%s %s: multigrid %d iterations (twin %d), plain CG to 1e-12 %d" % (name, shape, it, itt, int(itp)))
    assert abs(it - itt) <= 1 and it <= 40
    d = N.mg_last_dispatch()
    assert d["iterations"] == it and d["residual_recomputations"] == 0
    c = 0.1 * np.abs(L[:, 2]).mean() if rd else 0.0
    assert np.abs(b - _matvec(L, nx, ny, per_x, per_y, x, c)).max() < acc        # the SAME system, in float64 on the host
    present = L[:, 2] != 0
    dd = (x - xp)[present]
    if rd and not present.all():
        dd = dd - dd.mean()                                     # (solid cells make the shifted system singular along one direction)
    assert np.abs(dd).max() <= 1e-8 * np.abs(xp).max()
    assert np.abs(x - xt).max() <= 1e-8 * np.abs(xt).max()
    assert np.all(x[~present] == 0)


@pytest.mark.parametrize("walls", (False, True))
@pytest.mark.parametrize("shape", ((256, 256), (256, 1024), (1024, 1024), (2048, 2048)))
def test_large_grids_converge_in_tens_of_iterations(shape, walls):
    from diffpiso.solvers import mg_solve_native
    ny, nx = shape
    L, b = cases.pressure_system(nx, ny, walls=walls)
    per = not walls
    x, it = mg_solve_native(nx, ny, per, per, L, b, 1e-10, 200, True, 1 << 30)
    Lh, xh, bh = L.cpu().numpy().reshape(-1, 5), x.cpu().numpy(), b.cpu().numpy()
    c = 0.1 * np.abs(Lh[:, 2]).mean()
    # the system splits into L x = b - mean(b) and c sum(x) = mean(b) (here 0).  The second is held to the round-off of a sum of N
    # terms of size max|x| - at 4 M cells c N eps max|x| is far above 1e-10 for ANY float64 x -, the first to `accuracy` plus the
    # round-off of this host product
    eps = np.finfo(np.float64).eps
    res = np.abs(bh - _matvec(Lh, nx, ny, per, per, xh)).max()
    shift = abs(c * xh.sum())
    print("pressure_system %dx%d walls=%s: %d multigrid iterations to 1e-10, true residual %.2e, c sum(x) %.2e, max|x| %.2e"
          % (ny, nx, walls, it, res, shift, np.abs(xh).max()))
    assert it <= 40
    assert res < 1e-10 + 64 * eps * np.abs(Lh[:, 2]).max() * np.abs(xh).max()
    assert shift <= 4 * c * nx * ny * eps * np.abs(xh).max()


def test_right_hand_side_with_a_mean_matches_the_plain_solver():
    from diffpiso.solvers import cg_solve_native, mg_solve_native
    s, L, b, nx, ny, per_x, per_y, rd = _system("periodic", (64, 96))
    assert rd
    b = b + 0.37
    Ld, bd = _dev(L), _dev(b)
    x, it = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-11, 200, rd, 1 << 30)
    xp, _ = cg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-13, 50000, rd, 1 << 30)
    x, xp = x.cpu().numpy(), xp.cpu().numpy()
    assert abs(xp.mean()) > 1e-5 and abs(x.mean() - xp.mean()) <= 1e-6 * abs(xp.mean())      # mean(b) / (c N)
    assert np.abs(x - xp).max() <= 1e-8 * np.abs(xp).max()


def test_residual_reset_recomputes_the_true_residual():
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native
    s, L, b, nx, ny, per_x, per_y, rd = _system("xper_ywall", (130, 129))
    Ld, bd = _dev(L), _dev(b)
    x0, it0 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-10, 200, rd, 1 << 30)
    x1, it1 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-10, 200, rd, 5)
    xt, itt = M.pcg(L, b, nx, ny, per_x, per_y, 1e-10, 200, rd, residual_reset=5)
    d = N.mg_last_dispatch()
    assert abs(it1 - itt) <= 1 and it0 <= it1 <= it0 + 10
    assert d["residual_recomputations"] == sum(1 for k in range(1, it1) if (k + 1) % 5 == 0) > 0
    assert float((x1 - x0).abs().max()) <= 1e-8 * float(x0.abs().max())


@pytest.mark.parametrize("shape", ((64, 64), (130, 129), (512, 512)))
def test_solves_are_bitwise_reproducible_and_independent_of_the_polling_cadence(shape, piso_option):
    from diffpiso.solvers import mg_solve_native
    s, L, b, nx, ny, per_x, per_y, rd = _system("cavity", shape)
    Ld, bd = _dev(L), _dev(b)
    x0, it0 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-9, 200, rd, 1 << 30)
    x1, it1 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-9, 200, rd, 1 << 30)
    assert it0 == it1 and torch.equal(x0, x1)
    for every in (1, 3, 7):
        piso_option("mg_check_every", every)
        x2, it2 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-9, 200, rd, 1 << 30)
        assert it2 == it0 and torch.equal(x0, x2), every


def test_refusals():
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native
    s, L, b, nx, ny, per_x, per_y, rd = _system("cavity", (32, 48))
    bad = L.copy()
    bad[5, 0] = 0.25                                            # a -y entry in the first row of a wall-bounded grid
    with pytest.raises(N.PisoNativeError, match="border"):
        mg_solve_native(nx, ny, per_x, per_y, _dev(bad), _dev(b), 1e-8, 50, rd, 10)
    x = torch.empty(nx * ny, dtype=torch.float64, device="cuda")
    it = C.c_int(0)
    need = N.lib.piso_mg_workspace_bytes(nx, ny)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    Ld, bd = _dev(bad), _dev(b)
    args = lambda nbytes: (nx, ny, 0, 0, N.ptr(Ld), N.ptr(bd), N.ptr(x), C.c_float(1e-8), 50, 1, 10, 2, C.byref(it), N.ptr(ws),
                           C.c_size_t(nbytes), N.stream_ptr())
    assert N.lib.piso_mg_pcg_solve_f64(*args(need)) == N.ERR_UNSUPPORTED_PATTERN
    assert N.lib.piso_mg_pcg_solve_f64(*args(need - 1)) == 1 and b"workspace" in N.lib.piso_last_error_string()
    # rank_deficient = 1 on an operator that is not singular
    s2, L2, b2, nx2, ny2, px2, py2, rd2 = _system("spatial_ml", (32, 48))
    assert not rd2
    with pytest.raises(N.PisoNativeError, match="sum to zero"):
        mg_solve_native(nx2, ny2, px2, py2, _dev(L2), _dev(b2), 1e-8, 50, True, 10)
    with pytest.raises(N.PisoNativeError, match="fp64"):
        mg_solve_native(nx, ny, per_x, per_y, _dev(L).float(), _dev(b), 1e-8, 50, rd, 10)
    with pytest.raises(ValueError, match="PisoPressureSolverCudaCustom"):
        dp.PisoPressureSolverMultigrid(dx=[], cast_to_double=False)
    ps = dp.PisoPressureSolverMultigrid(dx=[])
    ps.slab_comm = object()
    with pytest.raises(N.PisoNativeError, match="PisoPressureSolverCudaCustom"):
        ps._cg(nx, ny, per_x, per_y, _dev(L), _dev(b), 1e-8, 50, rd, 10)
    with pytest.raises(N.PisoNativeError, match="4 cells"):
        mg_solve_native(3, 40, False, False, _dev(L[:120]), _dev(b[:120]), 1e-8, 50, rd, 10)


def test_nan_never_counts_as_converged():
    from diffpiso.solvers import mg_solve_native
    s, L, b, nx, ny, per_x, per_y, rd = _system("periodic", (64, 64))
    bn = b.copy(); bn[100] = np.nan
    x, it = mg_solve_native(nx, ny, per_x, per_y, _dev(L), _dev(bn), 1e-8, 9, rd, 1 << 30)
    assert it == 9 and bool(torch.isnan(x).any())
    Ln = L.copy(); Ln[200, 3] = np.nan
    x, it = mg_solve_native(nx, ny, per_x, per_y, _dev(Ln), _dev(b), 1e-8, 9, rd, 1 << 30)
    assert it == 9 and bool(torch.isnan(x).any())


# ---- step level: the oracle fixtures, with the bounds test_gpu_golden_configs.py holds the plain solver to ---------------------------
def _multigrid_like(ps):
    import diffpiso as dp
    return dp.PisoPressureSolverMultigrid(dx=[], accuracy=ps.accuracy, max_iterations=200, residual_reset=ps.residual_reset)


_TIGHT = dict(u=1e-5, p=1e-5, du=1e-5, dp=1e-5)


def _bench_fixture(fixture, tols, steps_key):
    import bench
    import diffpiso as dp
    from tests.test_gpu_golden_configs import _check, _load
    d, meta = _load(fixture)
    n, sv = meta["grid"], meta["solver"]
    steps = meta["steps"] if steps_key else 1
    P = bench.build_problem(n, torch.device("cuda"), sv["p_tol"], sv["p_max_it"], sv["p_reset"])
    P["lin"].accuracy, P["lin"].max_iterations = sv["lin_tol"], sv["lin_max_it"]
    ps = _multigrid_like(P["ps"])
    P["sim"].pressure_solver = ps
    assert abs(np.linalg.norm(P["vel"].astype(np.float64)) - float(d["in_vel_norm"])) < 1e-6 * float(d["in_vel_norm"])
    stride = int(d["stride"])
    vel_t = P["vel_t"].clone().requires_grad_(True)
    p_t = P["p_t"].clone().requires_grad_(True)
    ext = dp.Material.extrapolation_mode(P["domain"].boundaries)
    velocity = dp.StaggeredGrid(vel_t, P["domain"].box, extrapolation=ext)
    pressure = dp.CenteredGrid(p_t, P["domain"].box, dp.pressure_extrapolation(P["domain"].boundaries))
    va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, P["dt"], P["sim"], step_count=steps)
    bad = []
    _check("u", vn.staggered_tensor(), d["vel_sub"], float(d["vel_norm"]), stride, tols["u"], bad)
    _check("p", pn.data, d["p_sub"], float(d["p_norm"]), stride, tols["p"], bad)
    if "p_tol_adjoint" in sv:
        ps.accuracy = sv["p_tol_adjoint"]
    (0.5 * (vn.staggered_tensor() ** 2).sum()).backward()
    _check("dL/du_0", vel_t.grad, d["d_vel_sub"], float(d["d_vel_norm"]), stride, tols["du"], bad)
    dx = 2 * np.pi / n
    summands = np.sqrt(2.0) * float(d["dt"]) / dx * float(d["d_vel_norm"])
    _check("dL/dp_0", p_t.grad, d["d_p_sub"], float(d["d_p_norm"]), stride, tols["dp"], bad, scale_norm=max(summands, float(d["d_p_norm"])))
    total = ps.stats["iterations"] + ps.stats["adjoint_iterations"]
    plain = int(np.sum(meta["cg_iterations_fwd"])) + int(np.sum(meta["cg_iterations_adjoint"]))
    print("%s: multigrid pressure iterations fwd %d (%d solves) + adjoint %d (%d solves) = %d; the fixture's plain CG: %d"
          % (fixture, ps.stats["iterations"], ps.stats["solves"], ps.stats["adjoint_iterations"], ps.stats["adjoint_solves"], total, plain))
    assert not bad, bad
    assert ps.stats["solves"] == ps.stats["adjoint_solves"] > 0
    return total, plain


def test_step_512_sixteen_steps_converged_with_the_multigrid_solver():
    total, plain = _bench_fixture("bench512_tight_unroll16.npz", _TIGHT, True)
    assert total * 50 <= plain


def test_step_1024_converged_with_the_multigrid_solver():
    total, plain = _bench_fixture("bench1024_tight_step.npz", _TIGHT, False)
    assert total * 50 <= plain


def test_step_2048_converged_with_the_multigrid_solver():
    """The point of it all: the plain solver's parity bounds at 2048^2 with two orders of magnitude fewer pressure iterations."""
    total, plain = _bench_fixture("bench2048_tight_step.npz", _TIGHT, False)
    assert total * 100 <= plain


def test_config3_walls_512x256_with_the_multigrid_solver():
    import diffpiso as dp
    from tests.test_gpu_golden_configs import _check, _load
    d, meta = _load("cfg3_tml_512x256.npz")
    c = cases.tml_case()
    P = product_setup(c, **meta["solver"])
    ps = _multigrid_like(P["ps"])
    P["sim"].pressure_solver = ps
    stride = int(d["stride"])
    vel_t = P["vel_tensor"].clone().requires_grad_(True)
    velocity = dp.StaggeredGrid(vel_t, P["velocity"].box, extrapolation=P["velocity"].extrapolation)
    p_t = P["pressure"].data.clone().requires_grad_(True)
    pressure = dp.CenteredGrid(p_t, P["pressure"].box, P["pressure"].extrapolation)
    va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, c["dt"], P["sim"], step_count=meta["steps"])
    assert float(sum(w.sum() for w in warn)) == 0
    _check("cfg3 u_4", vn.staggered_tensor(), d["vel_sub"], float(d["vel_norm"]), stride, 1e-5)
    _check("cfg3 p_4", pn.data, d["p_sub"], float(d["p_norm"]), stride, 1e-5)
    (0.5 * (vn.staggered_tensor() ** 2).sum()).backward()
    _check("cfg3 dL/du_0", vel_t.grad, d["d_vel_sub"], float(d["d_vel_norm"]), stride, 1e-5)
    dy, dx = (float(v) for v in c["dx_yx"])
    summands = np.sqrt(2.0) * float(c["dt"]) / min(dx, dy) * float(d["d_vel_norm"])
    _check("cfg3 dL/dp_0", p_t.grad, d["d_p_sub"], float(d["d_p_norm"]), stride, 1e-5, scale_norm=max(summands, float(d["d_p_norm"])))
    print("cfg3: multigrid pressure iterations fwd %d (%d solves), adjoint %d (%d solves); last dispatch %s"
          % (ps.stats["iterations"], ps.stats["solves"], ps.stats["adjoint_iterations"], ps.stats["adjoint_solves"], ps.last_dispatch()))
    assert ps.stats["iterations"] <= 40 * ps.stats["solves"]
