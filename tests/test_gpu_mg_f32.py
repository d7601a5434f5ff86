"""The float32 V-cycle under the fp64 multigrid PCG (csrc/mg_f32.h, cycle_dtype=torch.float32) on the GPU, held to its numpy twin
(tests/mg_reference_f32.py), to the fp64 solver, to the true residual in float64 on the host and - at step level - to the oracle fixtures
with the bounds of the fp64 solver.  The shapes (ny, nx) are chosen for what can go wrong in the four-cell kernels, not for size:
(64, 256) level 0 in quads, level 1 opens the tail; (72, 264) levels 0 and 1 in quads; (71, 264) odd ny under ceil aggregation;
(72, 268) level 0 in quads and level 1 (134 columns) scalar; (33, 70) and (130, 129) no level in quads; (64, 64) the tail at level 0."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import cases
from tests import mg_reference as M
from tests import mg_reference_f32 as M32
from tests.cases import laplace_case, product_setup

pytestmark = pytest.mark.gpu
CASES = ("periodic", "xper_ywall", "cavity", "spatial_ml")
SHAPES = ((64, 256), (72, 264), (71, 264), (72, 268), (33, 70), (130, 129), (64, 64))
F32 = torch.float32
EPS32 = 2.0 ** -23


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")


@functools.lru_cache(maxsize=None)
def _system(name, shape, pattern="none", seed=3):
    """(L, b, nx, ny, per_x, per_y, rank_deficient, float32 twin hierarchy): built once per system and shared, never modified"""
    ny, nx = shape
    s, L, b = laplace_case(name, ny, nx, seed, solids=cases.solid_pattern(pattern, ny, nx) or None)
    per_y, per_x = (bool(v) for v in s.periodic_yx)
    L = np.asarray(L, np.float64).reshape(-1, 5)
    return L, b, nx, ny, per_x, per_y, bool(s.rank_deficient), M32.Hierarchy32(L, nx, ny, per_x, per_y)


def _predicted_mask(nx, ny):
    sizes, tail_first = M.plan(nx, ny)
    return sum(1 << l for l in range(max(tail_first, 0)) if sizes[l][0] % 4 == 0)


def _cycle_checks(name, shape, pattern, sweeps, piso_option, full):
    """2(a) - 2(e) of one cycle on one system; `full` False: (b), (d) and z == 0 on absent cells only"""
    import diffpiso._native as N
    from diffpiso.solvers import mg_vcycle_native
    L, b, nx, ny, per_x, per_y, rd, H = _system(name, shape, pattern)
    Ld = _dev(L)
    rng = np.random.default_rng(7)
    a, c = rng.standard_normal(nx * ny), rng.standard_normal(nx * ny)
    present = L[:, 2] != 0
    za = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(a), sweeps, cycle_dtype=F32).cpu().numpy()
    d = N.mg_last_dispatch()
    assert d["cycle_elem"] == 4 and d["levels"] == len(H.levels) and d["sweeps"] == sweeps and d["cycles"] == 1
    assert d["vec_mask"] == _predicted_mask(nx, ny), (d, M.plan(nx, ny))                                   # (a)
    piso_option("mg_f32_vec", 0)
    zs = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(a), sweeps, cycle_dtype=F32).cpu().numpy()
    assert N.mg_last_dispatch()["vec_mask"] == 0
    assert np.array_equal(zs, za), "four-cell and scalar kernels differ in %d cells" % (zs != za).sum()     # (b)
    piso_option("mg_f32_vec", 1)
    z32, z64 = H.cycle(a, sweeps), H.cycle(a, sweeps, dtype=np.float64)
    d_ref = np.abs(z32 - z64).max()
    differ = int((za != z32).sum())
    print("%s %s %s sweeps %d: GPU and twin differ in %d of %d cells; max|z_gpu - z64| %.3e, d_ref %.3e, max|z| %.3e"
          % (name, shape, pattern, sweeps, differ, za.size, np.abs(za - z64).max(), d_ref, np.abs(z64).max()))
    assert np.abs(za - z64).max() <= 2 * d_ref                                                             # (d)
    assert np.all(za[~present] == 0)
    if not full:
        return
    piso_option("mg_tail", 0)
    zl = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(a), sweeps, cycle_dtype=F32).cpu().numpy()
    assert N.mg_last_dispatch()["tail_first"] == -1
    assert np.array_equal(zl, za)                                                                          # (c)
    piso_option("mg_tail", 1)
    zc = mg_vcycle_native(nx, ny, per_x, per_y, Ld, _dev(c), sweeps, cycle_dtype=F32).cpu().numpy()
    assert abs(za @ c - a @ zc) <= 1e-6 * np.linalg.norm(a) * np.linalg.norm(c)                            # (e)
    assert za @ a < 0 and zc @ c < 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_level_operators_equal_the_float32_twin(name, shape):
    from diffpiso.solvers import mg_level_native
    L, b, nx, ny, per_x, per_y, rd, H = _system(name, shape)
    Ld = _dev(L)
    differ = 0
    for l in range(len(H.levels)):
        want, nxl, nyl = H.level_rows(l)
        got, gx, gy = mg_level_native(nx, ny, per_x, per_y, Ld, l, cycle_dtype=F32)
        got = got.cpu().numpy()
        assert (gx, gy) == (nxl, nyl)
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))              # float32 entries, widened
        differ += int((got != want).sum())
        assert np.abs(got - want).max() <= EPS32 * np.abs(want).max(), (name, shape, l)
    print("%s %s: %d entries of %d levels differ from the twin" % (name, shape, differ, len(H.levels)))
    assert mg_level_native(nx, ny, per_x, per_y, Ld, len(H.levels), cycle_dtype=F32) is None


@pytest.mark.parametrize("sweeps", (1, 2, 3))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_one_cycle_quads_scalar_tail_and_twin(name, shape, sweeps, piso_option):
    _cycle_checks(name, shape, "none", sweeps, piso_option, True)


@pytest.mark.parametrize("pattern,shape", [(p, s) for p in ("cell_eo", "block4", "wall", "seam", "corners") for s in ((72, 264), (33, 70))] +
                         [("random10", (130, 129)), ("random10", (33, 70))])
@pytest.mark.parametrize("name", CASES)
def test_solid_cells_inside_quads(name, pattern, shape, piso_option):
    _cycle_checks(name, shape, pattern, 2, piso_option, False)


@functools.lru_cache(maxsize=None)
def _fp64_solve(name, shape, acc):
    from diffpiso.solvers import mg_solve_native
    L, b, nx, ny, per_x, per_y, rd, H = _system(name, shape)
    x, it = mg_solve_native(nx, ny, per_x, per_y, _dev(L), _dev(b), acc, 300, rd, 1 << 30)
    return x.cpu().numpy(), it


@pytest.mark.parametrize("acc", (1e-10, 1e-5))
@pytest.mark.parametrize("shape", ((72, 264), (130, 129), (64, 256)))
@pytest.mark.parametrize("name", CASES)
def test_solves_against_the_twin_the_fp64_solver_and_the_true_residual(name, shape, acc):
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native
    L, b, nx, ny, per_x, per_y, rd, H = _system(name, shape)
    x, it = mg_solve_native(nx, ny, per_x, per_y, _dev(L), _dev(b), acc, 300, rd, 1 << 30, cycle_dtype=F32)
    d = N.mg_last_dispatch()
    x = x.cpu().numpy()
    xt, itt = M32.pcg_mixed(L, b, nx, ny, per_x, per_y, acc, 300, rd, H=H)
    x64, it64 = _fp64_solve(name, shape, acc)
    first, second, floor = M.residuals(L, b, x, nx, ny, per_x, per_y, rd)
    print("%s %s accuracy %.0e: float32 cycle %d iterations (twin %d, fp64 cycle on the GPU %d); true residual %.2e, second part %.2e (floor %.2e), "
          "|x - x_fp64| / max|x| %.2e" % (name, shape, acc, it, itt, it64, first, second, floor, np.abs(x - x64).max() / np.abs(x64).max()))
    assert abs(it - itt) <= 2
    assert it <= it64 + max(2, math.ceil(0.3 * it64))
    eps = np.finfo(np.float64).eps
    assert first < 2 * acc + 64 * eps * np.abs(L[:, 2]).max() * np.abs(x).max()
    assert second <= floor
    if acc == 1e-10:
        assert np.abs(x - x64).max() <= 1e-8 * np.abs(x64).max()
    assert np.all(x[L[:, 2] == 0] == 0)
    assert d["cycle_elem"] == 4 and d["iterations"] == it and d["vec_mask"] == _predicted_mask(nx, ny)


def test_grid_stride_loop_of_the_four_cell_kernels(piso_option):
    """2048 x 520 = 1 064 960 cells = 266 240 quads: more than the 1024 x 256 threads of a launch, so the stride loop runs twice."""
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native, mg_vcycle_native
    nx, ny = 2048, 520
    L, b = cases.pressure_system(nx, ny)
    za = mg_vcycle_native(nx, ny, True, True, L, b, 2, cycle_dtype=F32)
    assert N.mg_last_dispatch()["vec_mask"] == _predicted_mask(nx, ny) and N.mg_last_dispatch()["vec_mask"] & 1
    piso_option("mg_f32_vec", 0)
    zs = mg_vcycle_native(nx, ny, True, True, L, b, 2, cycle_dtype=F32)
    piso_option("mg_f32_vec", 1)
    assert torch.equal(za, zs)
    x64, it64 = mg_solve_native(nx, ny, True, True, L, b, 1e-10, 200, True, 1 << 30)
    x, it = mg_solve_native(nx, ny, True, True, L, b, 1e-10, 200, True, 1 << 30, cycle_dtype=F32)
    print("2048 x 520: fp64 cycle %d iterations, float32 cycle %d" % (it64, it))
    assert it <= it64 + 2
    assert float((x - x64).abs().max()) <= 1e-8 * float(x64.abs().max())


@pytest.mark.parametrize("shape", ((130, 129), (72, 264)))
def test_solves_are_bitwise_reproducible_and_independent_of_the_polling_cadence(shape, piso_option):
    from diffpiso.solvers import mg_solve_native
    L, b, nx, ny, per_x, per_y, rd, H = _system("cavity", shape)
    Ld, bd = _dev(L), _dev(b)
    x0, it0 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-9, 200, rd, 1 << 30, cycle_dtype=F32)
    x1, it1 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-9, 200, rd, 1 << 30, cycle_dtype=F32)
    assert it0 == it1 and torch.equal(x0, x1)
    for every in (1, 3, 7):
        piso_option("mg_check_every", every)
        x2, it2 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-9, 200, rd, 1 << 30, cycle_dtype=F32)
        assert it2 == it0 and torch.equal(x0, x2), every


def test_residual_reset_recomputes_the_true_residual():
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native
    L, b, nx, ny, per_x, per_y, rd, H = _system("xper_ywall", (130, 129))
    Ld, bd = _dev(L), _dev(b)
    x0, it0 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-10, 200, rd, 1 << 30, cycle_dtype=F32)
    x1, it1 = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-10, 200, rd, 5, cycle_dtype=F32)
    d = N.mg_last_dispatch()
    assert it0 <= it1 <= it0 + 10
    assert d["residual_recomputations"] == sum(1 for k in range(1, it1) if (k + 1) % 5 == 0) > 0
    assert float((x1 - x0).abs().max()) <= 1e-8 * float(x0.abs().max())


def test_nan_never_counts_as_converged():
    from diffpiso.solvers import mg_solve_native
    L, b, nx, ny, per_x, per_y, rd, H = _system("periodic", (64, 256))
    bn = b.copy(); bn[100] = np.nan
    x, it = mg_solve_native(nx, ny, per_x, per_y, _dev(L), _dev(bn), 1e-8, 9, rd, 1 << 30, cycle_dtype=F32)
    assert it == 9 and bool(torch.isnan(x).any())
    Ln = L.copy(); Ln[200, 3] = np.nan
    x, it = mg_solve_native(nx, ny, per_x, per_y, _dev(Ln), _dev(b), 1e-8, 9, rd, 1 << 30, cycle_dtype=F32)
    assert it == 9 and bool(torch.isnan(x).any())


def test_right_hand_side_with_a_mean_matches_the_plain_solver():
    from diffpiso.solvers import cg_solve_native, mg_solve_native
    ny, nx = 64, 96
    s, L, b = laplace_case("periodic", ny, nx, 3)
    assert s.rank_deficient
    b = b + 0.37
    Ld, bd = _dev(np.asarray(L, np.float64).reshape(-1, 5)), _dev(b)
    x, it = mg_solve_native(nx, ny, True, True, Ld, bd, 1e-11, 200, True, 1 << 30, cycle_dtype=F32)
    xp, _ = cg_solve_native(nx, ny, True, True, Ld, bd, 1e-13, 50000, True, 1 << 30)
    x, xp = x.cpu().numpy(), xp.cpu().numpy()
    assert abs(xp.mean()) > 1e-5 and abs(x.mean() - xp.mean()) <= 1e-6 * abs(xp.mean())      # mean(b) / (c N)
    assert np.abs(x - xp).max() <= 1e-8 * np.abs(xp).max()


def test_refusals_of_the_float32_cycle_entries():
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native
    ny, nx = 32, 48
    s, L, b = laplace_case("cavity", ny, nx, 3)
    L = np.asarray(L, np.float64).reshape(-1, 5)
    rd = bool(s.rank_deficient)
    bad = L.copy()
    bad[5, 0] = 0.25                                            # a -y entry in the first row of a wall-bounded grid
    with pytest.raises(N.PisoNativeError, match="border"):
        mg_solve_native(nx, ny, False, False, _dev(bad), _dev(b), 1e-8, 50, rd, 10, cycle_dtype=F32)
    x = torch.empty(nx * ny, dtype=torch.float64, device="cuda")
    it = C.c_int(0)
    need = N.lib.piso_mg_workspace_bytes_cycle(nx, ny, 4)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    Ld, bd = _dev(bad), _dev(b)
    args = lambda nbytes: (nx, ny, 0, 0, N.ptr(Ld), N.ptr(bd), N.ptr(x), C.c_float(1e-8), 50, 1, 10, 2, C.byref(it), N.ptr(ws),
                           C.c_size_t(nbytes), N.stream_ptr())
    assert N.lib.piso_mg_pcg_solve_c32_f64(*args(need)) == N.ERR_UNSUPPORTED_PATTERN
    assert N.lib.piso_mg_pcg_solve_c32_f64(*args(need - 1)) == 1 and b"workspace" in N.lib.piso_last_error_string()
    s2, L2, b2 = laplace_case("spatial_ml", ny, nx, 3)
    assert not s2.rank_deficient
    per_y2, per_x2 = (bool(v) for v in s2.periodic_yx)
    with pytest.raises(N.PisoNativeError, match="sum to zero"):
        mg_solve_native(nx, ny, per_x2, per_y2, _dev(np.asarray(L2, np.float64).reshape(-1, 5)), _dev(b2), 1e-8, 50, True, 10, cycle_dtype=F32)
    with pytest.raises(N.PisoNativeError, match="fp64"):
        mg_solve_native(nx, ny, False, False, _dev(L).float(), _dev(b), 1e-8, 50, rd, 10, cycle_dtype=F32)


# ---- step level: the oracle fixtures, with the bounds test_gpu_mg.py holds the fp64 cycle to ---------------------------------------------------
def _float32_cycle_like(ps):
    import diffpiso as dp
    return dp.PisoPressureSolverMultigrid(dx=[], accuracy=ps.accuracy, max_iterations=200, residual_reset=ps.residual_reset, cycle_dtype=F32)


def test_config3_walls_512x256_with_the_float32_cycle():
    import diffpiso as dp
    from tests.test_gpu_golden_configs import _check, _load
    d, meta = _load("cfg3_tml_512x256.npz")
    c = cases.tml_case()
    P = product_setup(c, **meta["solver"])
    ps = _float32_cycle_like(P["ps"])
    per_solve, solve = [], ps._cg

    def counted(*args):
        x, it = solve(*args)
        per_solve.append(int(it))
        return x, it
    ps._cg = counted
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
    print("cfg3: float32-cycle pressure iterations fwd %d (%d solves), adjoint %d (%d solves); last dispatch %s"
          % (ps.stats["iterations"], ps.stats["solves"], ps.stats["adjoint_iterations"], ps.stats["adjoint_solves"], ps.last_dispatch()))
    print("cfg3: iterations of each solve, forward then adjoint: %s" % per_solve)
    assert len(per_solve) == ps.stats["solves"] + ps.stats["adjoint_solves"] and max(per_solve) <= 40
    assert ps.last_dispatch()["cycle_elem"] == 4


def test_step_1024_converged_with_the_float32_cycle():
    import bench
    import diffpiso as dp
    from tests.test_gpu_golden_configs import _check, _load
    from tests.test_gpu_mg import _TIGHT as tols
    d, meta = _load("bench1024_tight_step.npz")
    n, sv = meta["grid"], meta["solver"]
    P = bench.build_problem(n, torch.device("cuda"), sv["p_tol"], sv["p_max_it"], sv["p_reset"])
    P["lin"].accuracy, P["lin"].max_iterations = sv["lin_tol"], sv["lin_max_it"]
    ps = _float32_cycle_like(P["ps"])
    P["sim"].pressure_solver = ps
    assert abs(np.linalg.norm(P["vel"].astype(np.float64)) - float(d["in_vel_norm"])) < 1e-6 * float(d["in_vel_norm"])
    stride = int(d["stride"])
    vel_t = P["vel_t"].clone().requires_grad_(True)
    p_t = P["p_t"].clone().requires_grad_(True)
    ext = dp.Material.extrapolation_mode(P["domain"].boundaries)
    velocity = dp.StaggeredGrid(vel_t, P["domain"].box, extrapolation=ext)
    pressure = dp.CenteredGrid(p_t, P["domain"].box, dp.pressure_extrapolation(P["domain"].boundaries))
    va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, P["dt"], P["sim"], step_count=1)
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
    print("bench1024_tight_step: float32-cycle pressure iterations fwd %d (%d solves) + adjoint %d (%d solves); last dispatch %s"
          % (ps.stats["iterations"], ps.stats["solves"], ps.stats["adjoint_iterations"], ps.stats["adjoint_solves"], ps.last_dispatch()))
    assert not bad, bad
    assert ps.stats["solves"] == ps.stats["adjoint_solves"] > 0
    assert ps.last_dispatch()["cycle_elem"] == 4
