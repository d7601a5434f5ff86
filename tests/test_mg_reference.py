"""The multigrid-preconditioned pressure CG, checked on the host through its numpy twin (tests/mg_reference.py): the cycle is a
symmetric definite operator, the preconditioned iteration reaches the oracle's answer in tens of iterations where the plain CG of
the oracle needs hundreds.  The GPU tests (test_gpu_mg.py) hold the HIP solver to this twin."""
import numpy as np
import pytest

from oracle import native as O
from tests import mg_reference as M
from tests.cases import laplace_case

CASES = ("periodic", "xper_ywall", "cavity", "spatial_ml")
SHAPES = ((33, 70), (64, 256), (130, 129))


def _apply(nx, ny, per_x, per_y, L, x):
    """L x with the oracle's stencil semantics (the matrices here have no entry the quirk of the reference stencil would move)."""
    return M.matrix(L, nx, ny, per_x, per_y) @ x


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_cycle_is_symmetric_and_definite(name, shape):
    ny, nx = shape
    s, L, _ = laplace_case(name, ny, nx, 5)
    per_y, per_x = s.periodic_yx
    H = M.Hierarchy(L, nx, ny, per_x, per_y)
    present = H.levels[0][1] != 0
    assert len(H.levels) >= 3
    rng = np.random.default_rng(1)
    for _ in range(3):
        a, b = rng.standard_normal(nx * ny), rng.standard_normal(nx * ny)
        za, zb = H.cycle(a), H.cycle(b)
        assert abs(za @ b - a @ zb) <= 1e-12 * np.linalg.norm(a) * np.linalg.norm(b)
        assert np.all(za[~present] == 0)
        assert za @ a < 0 and zb @ b < 0                      # an approximation of L^-1: negative definite on the present cells
    ones = present.astype(np.float64)
    assert H.cycle(ones) @ ones < 0                            # ... constants included


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_coarse_operators_keep_the_five_point_form(name, shape):
    ny, nx = shape
    s, L, _ = laplace_case(name, ny, nx, 6)
    per_y, per_x = s.periodic_yx
    H = M.Hierarchy(L, nx, ny, per_x, per_y)
    assert np.array_equal(H.level_rows(0)[0], np.asarray(L).reshape(-1, 5))
    for l in range(len(H.levels)):
        rows, nxl, nyl = H.level_rows(l)
        A = H.levels[l][0]
        assert abs(M.matrix(rows, nxl, nyl, per_x, per_y) - A).max() <= 1e-13 * abs(A).max()    # nothing outside the five slots
        assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
        assert min(nxl, nyl) >= M.MIN_DIM
        if s.rank_deficient:                                   # constants stay in the null space on every level
            assert np.abs(A @ (A.diagonal() != 0).astype(np.float64)).max() <= 1e-12 * abs(A).max()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_pcg_reaches_the_oracle_solution_in_tens_of_iterations(name, shape):
    ny, nx = shape
    s, L, b = laplace_case(name, ny, nx, 3)
    per_y, per_x = s.periodic_yx
    rd = bool(s.rank_deficient)
    x, it = M.pcg(L, b, nx, ny, per_x, per_y, 1e-9, 200, rd)
    xo, ito = O.cg_solve(nx, ny, per_x, per_y, L, b, 1e-12, 20000, rd, 1 << 30)
    print("%s %dx%d: multigrid PCG %d iterations, plain CG %d" % (name, ny, nx, it, ito))
    assert it <= 40 and ito >= 300
    c = 0.1 * np.abs(L.reshape(-1, 5)[:, 2]).mean() if rd else 0.0
    res = b - (_apply(nx, ny, per_x, per_y, L, x) + c * x.sum())
    assert np.abs(res).max() < 1e-9
    present = L.reshape(-1, 5)[:, 2] != 0
    d = (x - xo)[present]
    if rd:
        d = d - d.mean()
    assert np.abs(d).max() <= 1e-8 * np.abs(xo).max()
    assert np.all(x[~present] == 0)


def test_constant_mode_of_a_right_hand_side_with_a_mean():
    ny, nx = 40, 48
    s, L, b = laplace_case("periodic", ny, nx, 2)
    b = b + 0.37
    x, it = M.pcg(L, b, nx, ny, True, True, 1e-10, 100, True)
    xo, _ = O.cg_solve(nx, ny, True, True, L, b, 1e-13, 20000, True, 1 << 30)
    assert it <= 40
    assert np.abs(x - xo).max() <= 1e-8 * np.abs(xo).max()
    assert abs(x.mean() - xo.mean()) <= 1e-9 * abs(xo.mean())


def test_residual_reset_and_nan():
    ny, nx = 33, 70
    s, L, b = laplace_case("xper_ywall", ny, nx, 4)
    x0, it0 = M.pcg(L, b, nx, ny, True, False, 1e-10, 100, True)
    x1, it1 = M.pcg(L, b, nx, ny, True, False, 1e-10, 100, True, residual_reset=5)
    assert it0 <= it1 <= it0 + 10 and np.abs(x1 - x0).max() <= 1e-8 * np.abs(x0).max()
    bn = b.copy(); bn[7] = np.nan
    xn, itn = M.pcg(L, bn, nx, ny, True, False, 1e-10, 12, True)
    assert itn == 12 and np.isnan(xn).any()


def test_border_entry_in_a_non_periodic_direction_is_refused():
    ny, nx = 16, 16
    s, L, b = laplace_case("cavity", ny, nx, 1)
    L = L.reshape(-1, 5).copy()
    L[3, 0] = 0.25                                             # a -y entry in the first row of a wall-bounded grid
    with pytest.raises(ValueError):
        M.Hierarchy(L, nx, ny, False, False)
