"""Starting the multigrid PCG from a guess (csrc/mg_guess.h), checked without a GPU on its numpy twin (tests/mg_reference_guess.py): a guess
the guard rejects - x0 = 0 among them - is mg_reference.pcg bit for bit, a converged x0 costs no iteration, a NaN or Inf never fails a
solve, and what x0 holds on solid cells or as its mean does not matter.  Plus the C entries and the option's surface."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import mg_reference as M
from tests import mg_reference_f32 as M32
from tests import mg_reference_guess as G
from tests.cases import laplace_case, solid_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, ny, nx, solids): two levels; the whole cycle in the tail, 10 % random solids; a 4 x 4 block on a wall-bounded grid
SYSTEMS = (("periodic", 10, 12, None), ("xper_ywall", 33, 70, "random10"), ("cavity", 33, 70, "block4"), ("spatial_ml", 33, 70, "random10"))
_cache = {}


def _system(name, ny, nx, pattern):
    key = (name, ny, nx, pattern)
    if key not in _cache:
        s, L, b = laplace_case(name, ny, nx, 3, solids=solid_pattern(pattern, ny, nx) if pattern else None)
        per_y, per_x = (bool(v) for v in s.periodic_yx)
        L = np.asarray(L, np.float64).reshape(-1, 5)
        geo = (nx, ny, per_x, per_y)
        _cache[key] = (L, b, geo, bool(s.rank_deficient), M.Hierarchy(L, *geo), L[:, 2] != 0)
    return _cache[key]


@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: "%s-%dx%d-%s" % s)
def test_no_guess_a_zero_guess_and_a_rejected_guess_are_the_plain_solve_bit_for_bit(system):
    L, b, geo, rd, H, present = _system(*system)
    rng = np.random.default_rng(5)
    for acc, max_it, reset in ((1e-8, 200, 1 << 30), (1e-30, 5, 3)):
        want, itw = M.pcg(L, b, *geo, acc, max_it, rd, reset, H=H)
        for x0 in (None, np.zeros(geo[0] * geo[1]), 10 * rng.standard_normal(geo[0] * geo[1])):
            x, it, accepted = G.pcg_guess(L, b, x0, *geo, acc, max_it, rd, reset, H=H)
            assert not accepted and it == itw >= 1 and np.array_equal(x, want)
    # ... and the float32 cycle's twin likewise
    H32 = M32.Hierarchy32(L, *geo)
    want, itw = M32.pcg_mixed(L, b, *geo, 1e-8, 200, rd, H=H32)
    for x0 in (None, np.zeros(geo[0] * geo[1])):
        x, it, accepted = G.pcg_guess_f32(L, b, x0, *geo, 1e-8, 200, rd, H=H32)
        assert not accepted and it == itw and np.array_equal(x, want)


@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: "%s-%dx%d-%s" % s)
def test_a_converged_guess_costs_no_iteration_and_a_near_one_fewer(system):
    L, b, geo, rd, H, present = _system(*system)
    x12, it12 = M.pcg(L, b, *geo, 1e-12, 200, rd, H=H)
    assert it12 < 200
    x, it, accepted = G.pcg_guess(L, b, x12, *geo, 1e-8, 200, rd, H=H)
    assert accepted and it == 0
    assert np.abs(x - x12).max() <= 4 * np.finfo(np.float64).eps * np.abs(x12).max()      # (the constant mode's mean replacement)
    x3, _ = M.pcg(L, b, *geo, 1e-3, 200, rd, H=H)
    _, it0 = M.pcg(L, b, *geo, 1e-8, 200, rd, H=H)
    x, it, accepted = G.pcg_guess(L, b, x3, *geo, 1e-8, 200, rd, H=H)
    assert accepted and 1 <= it < it0
    first, second, floor = M.residuals(L, b, x, *geo, rd)
    assert first < 1e-8 + 64 * np.finfo(np.float64).eps * np.abs(L[:, 2]).max() * np.abs(x).max() and second <= floor
    assert np.all(x[~present] == 0)


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_a_nan_or_inf_in_the_guess_is_a_plain_solve(bad):
    L, b, geo, rd, H, present = _system(*SYSTEMS[1])
    want, itw = M.pcg(L, b, *geo, 1e-8, 200, rd, H=H)
    x0, _ = M.pcg(L, b, *geo, 1e-3, 200, rd, H=H)
    x0[np.nonzero(present)[0][17]] = bad
    x, it, accepted = G.pcg_guess(L, b, x0, *geo, 1e-8, 200, rd, H=H)
    assert not accepted and it == itw and np.array_equal(x, want)


@pytest.mark.parametrize("system", SYSTEMS[1:], ids=lambda s: "%s-%dx%d-%s" % s)
def test_solid_cells_and_the_mean_of_the_guess_do_not_matter(system):
    L, b, geo, rd, H, present = _system(*system)
    assert (~present).sum() >= 16
    clean, _ = M.pcg(L, b, *geo, 1e-3, 200, rd, H=H)
    dirty = clean + (3.7 if rd else 0.0)                       # (an arbitrary mean: immaterial where the operator is rank deficient)
    dirty[~present] = np.random.default_rng(2).standard_normal((~present).sum()) * 1e6
    dirty[np.nonzero(~present)[0][0]] = np.nan
    xc, itc, ac = G.pcg_guess(L, b, clean, *geo, 1e-9, 200, rd, H=H)
    xd, itd, ad = G.pcg_guess(L, b, dirty, *geo, 1e-9, 200, rd, H=H)
    assert ac and ad and abs(itc - itd) <= 1
    slack = 64 * np.finfo(np.float64).eps * np.abs(L[:, 2]).max()
    for x in (xc, xd):
        first, second, floor = M.residuals(L, b, x, *geo, rd)
        assert first < 1e-9 + slack * np.abs(x).max() and second <= floor
        assert np.all(x[~present] == 0)
    if not rd:                                                 # the same guess on the present cells: the same solve bit for bit
        assert itc == itd and np.array_equal(xc, xd)


def test_the_guard_compares_the_guess_residual_with_the_right_hand_side():
    L, b, geo, rd, H, present = _system(*SYSTEMS[0])
    rows = H.level_rows(0)[0]
    bp = np.where(present, b - (b[present].mean() if rd else 0.0), 0.0)
    x3, _ = M.pcg(L, b, *geo, 1e-3, 200, rd, H=H)
    xt, rg, accepted = G.guess_start(rows, present, bp, x3, *geo[:2])
    assert accepted and np.abs(rg).max() < np.abs(bp).max()
    assert np.abs(rg - (bp - M.matrix(L, *geo) @ xt)).max() <= 1e-13 * np.abs(bp).max()     # the stencil order against the CSR product
    assert not G.guess_start(rows, present, bp, np.zeros_like(bp), *geo[:2])[2]             # r_g = b': not strictly below
    assert not G.guess_start(rows, present, bp, -x3, *geo[:2])[2]                           # a residual of about 2 b'


def test_the_entries_are_declared_exported_and_bound():
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso import solvers as S
    with open(os.path.join(ROOT, "include", "piso_hip.h")) as f:
        header = f.read()
    for stem in ("pcg_solve_guess", "pcg_solve_prepared_guess"):
        for sfx in ("_f64", "_c32_f64"):
            name = "piso_mg_%s%s" % (stem, sfx)
            assert hasattr(N.lib, name), name
            decl = re.search(r"\bint %s\(int nx, int ny, int periodic_x, int periodic_y, [^;]*;" % name, header)
            assert decl and "const double* divergence, const double* x0," in re.sub(r"\s+", " ", decl.group(0)), name
        assert getattr(N.lib, "piso_mg_%s_f64" % stem).argtypes == getattr(N.lib, "piso_mg_%s_c32_f64" % stem).argtypes
        # the namesake's arguments plus one pointer
        assert len(getattr(N.lib, "piso_mg_%s_f64" % stem).argtypes) == len(getattr(N.lib, "piso_mg_%s_f64" % stem.replace("_guess", "")).argtypes) + 1
    assert re.search(r"\bint piso_mg_last_guess\(void\);", header) and N.mg_last_guess() in (0, 1, 2)
    assert len(N.MG_DISPATCH_FIELDS) == 8
    p = inspect.signature(dp.PisoPressureSolverMultigrid.__init__).parameters
    assert p["use_guess"].default is False
    assert inspect.signature(S.mg_solve_native).parameters["x0"].default is None
    # (mg_solve_prepared_native keeps the six parameters tests/test_mg_prepared_cpu.py pins: the prepared solve from a guess is a sibling)
    assert tuple(inspect.signature(S.mg_solve_prepared_guess_native).parameters)[:3] == ("h", "div", "x0")
    ps = dp.PisoPressureSolverMultigrid(dx=[])
    assert ps.use_guess is False and "guesses_accepted" not in ps.stats       # (the default's stats are the seven counters they were)
    on = dp.PisoPressureSolverMultigrid(dx=[], use_guess=True)
    assert on.use_guess is True and on.stats["guesses_accepted"] == 0 and on.stats["guesses_rejected"] == 0
    assert "use_guess=False" in dp.PisoPressureSolverMultigrid.__doc__
    # the plain solver takes no guess
    assert dp.PisoPressureSolverCudaCustom(dx=[])._guess_for_solve(object(), None) is None and not hasattr(dp.PisoPressureSolverCudaCustom(dx=[]), "use_guess")


def test_the_refusal_next_to_a_slab_communicator_and_of_a_guess_that_does_not_fit(monkeypatch):
    import torch
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso import distributed as D
    calls = []
    monkeypatch.setattr(D, "mg_solve_slab", lambda *a, **kw: calls.append(a) or ("x", 7))
    comm = object.__new__(D.SlabCommunicator)                  # (no attribute beyond these two exists: touching it raises AttributeError)
    comm.world, comm.sharded = 2, False
    L, div = torch.zeros(64 * 64, 5, dtype=torch.float64), torch.zeros(64 * 64, dtype=torch.float64)
    for dtype in (torch.float64, torch.float32):
        on = dp.PisoPressureSolverMultigrid(dx=[], cycle_dtype=dtype, use_guess=True)
        on.slab_comm = comm
        with pytest.raises(N.PisoNativeError, match="use_guess=False"):
            on._cg(64, 64, True, True, L, div, 1e-8, 10, True, 10, x0=div)
        with pytest.raises(N.PisoNativeError, match="use_guess=False"):       # ... and through solve_flat's first statement, whatever the guess
            on._guess_for_solve(div[:-1], div.reshape(1, 64, 64, 1))
        assert not calls
    on = dp.PisoPressureSolverMultigrid(dx=[], use_guess=True)
    shaped = div.reshape(1, 64, 64, 1)
    g = on._guess_for_solve(shaped.to(torch.float32).requires_grad_(True), shaped)
    assert g.dtype == torch.float64 and g.shape == (64 * 64,) and not g.requires_grad
    with pytest.raises(ValueError, match="4096 cells"):
        on._guess_for_solve(div[:-1], shaped)
    with pytest.raises(TypeError):
        on._guess_for_solve(torch.zeros(64 * 64, dtype=torch.int64), shaped)
    with pytest.raises(ValueError, match="device"):
        on._guess_for_solve(torch.zeros(64 * 64, device="meta"), shaped)
    assert dp.PisoPressureSolverMultigrid(dx=[])._guess_for_solve(div[:-1], shaped) is None      # off: ignored, whatever it is
