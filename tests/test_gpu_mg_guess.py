"""Starting the multigrid PCG from a guess (csrc/mg_guess.h; piso_mg_pcg_solve*_guess_*, PisoPressureSolverMultigrid(use_guess=True)), through
the ordinary and the prepared entries and both precisions of the cycle.  Oracles: the solve without a guess of the same library BIT FOR BIT
wherever the guard rejects the guess (or none is given), the numpy twins tests/mg_reference_guess.py (pcg_guess: fp64 cycle; pcg_guess_f32:
the float32 cycle - tests/mg_reference_f32.py exposes its cycle, so the float32 counts are held to a twin run from the same guess, not to
the fp64-cycle GPU count) wherever it accepts it, and the true residual of mg_reference.residuals.  A result WITH a guess is never compared
with the from-zero result by a tolerance of its own below the step level, where the project's parity bar (1e-5 relative L2) applies.

Grids (nx x ny), the smallest that reach every path: 12 x 10 two levels; 70 x 33 the whole cycle in the tail; 129 x 130 six levels, tail_first
2, odd sizes; 264 x 72 four-cell kernels of the float32 cycle; 520 x 516 several blocks in the partial maxima (268 320 cells > 1024 blocks of
256: the walk takes a second stride) and the prepared test's largest.

The ACCEPTED guess of these tests: the twin's solution at 1e-3 plus 1 % noise measured in the right-hand side - 0.01 max|b'| / max|diag L|
times a standard normal draw on every present cell - so its residual is the 1e-3 solve's plus a few percent of b' on any grid; acceptance
is asserted on the CPU.  (Noise of 1 % of each value of x is rejected by the guard from about 100 x 100 cells on, where max|x| reaches 40 -
160 against max|b'| ~ 4: measured on the twin, residuals of 5 - 25; 10 randn, the rejected guess of these tests, is of that kind.)"""
import numpy as np
import pytest
import torch

from tests import mg_reference as M
from tests import mg_reference_f32 as M32
from tests import mg_reference_guess as G
from tests.cases import laplace_case, make_case, product_setup, solid_pattern

pytestmark = pytest.mark.gpu
BIG = 1 << 30
EPS = np.finfo(np.float64).eps
F64, F32 = torch.float64, torch.float32
DTYPES = (F64, F32)
KINDS = ("ordinary", "prepared")
# (border kind, ny, nx, solids)
SYSTEMS = (("periodic", 10, 12, None), ("cavity", 10, 12, None),
           ("periodic", 33, 70, "random10"), ("xper_ywall", 33, 70, "random10"), ("cavity", 33, 70, "block4"), ("spatial_ml", 33, 70, "random10"),
           ("xper_ywall", 130, 129, "block4"), ("spatial_ml", 130, 129, "random10"),
           ("periodic", 72, 264, None), ("cavity", 72, 264, "block4"),
           ("xper_ywall", 516, 520, None))
SMALL = SYSTEMS[:10]
_sid = lambda s: "%s-%dx%d-%s" % (s[0], s[2], s[1], s[3])
_systems, _hier = {}, {}


class _S(object):
    pass


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _system(name, ny, nx, pattern):
    """The system on the host and the device, its twin hierarchy and the accepted guess, built once and left unchanged."""
    key = (name, ny, nx, pattern)
    if key not in _systems:
        S = _S()
        s, L, b = laplace_case(name, ny, nx, 3, solids=solid_pattern(pattern, ny, nx) if pattern else None)
        per_y, per_x = (bool(v) for v in s.periodic_yx)
        S.L, S.b, S.rd = np.asarray(L, np.float64).reshape(-1, 5), b, bool(s.rank_deficient)
        S.geo = (nx, ny, per_x, per_y)
        S.n = nx * ny
        S.present = S.L[:, 2] != 0
        S.H = M.Hierarchy(S.L, *S.geo)
        S.Ld, S.bd = _dev(S.L), _dev(S.b)
        x3, _ = M.pcg(S.L, S.b, *S.geo, 1e-3, 200, S.rd, H=S.H)
        bp = np.where(S.present, S.b - (S.b[S.present].mean() if S.rd else 0.0), 0.0)
        noise = 0.01 * np.abs(bp).max() / np.abs(S.L[:, 2]).max() * np.random.default_rng(11).standard_normal(S.n)
        S.x0 = x3 + np.where(S.present, noise, 0.0)
        _, rg, accepted = G.guess_start(S.H.level_rows(0)[0], S.present, bp, S.x0, nx, ny)
        assert accepted and np.abs(rg).max() < 0.5 * np.abs(bp).max(), "the guess of these tests must be an accepted one"
        S.x0d = _dev(S.x0)
        S.bad = _dev(10 * np.random.default_rng(12).standard_normal(S.n))
        _systems[key] = S
    return _systems[key]


def _solve(S, kind, dtype, acc, max_it, reset, x0=None, x_out=None, b=None):
    """-> (x, iterations, dispatch record, piso_mg_last_guess) through the ordinary or the prepared entry"""
    import diffpiso._native as N
    from diffpiso.solvers import mg_prepare_native, mg_solve_native, mg_solve_prepared_guess_native
    nx, ny, per_x, per_y = S.geo
    b = S.bd if b is None else b
    if kind == "ordinary":
        x, it = mg_solve_native(nx, ny, per_x, per_y, S.Ld, b, acc, max_it, S.rd, reset, 2, dtype, x0=x0, x_out=x_out)
    else:
        key = (id(S), dtype)
        if key not in _hier:
            _hier[key] = mg_prepare_native(nx, ny, per_x, per_y, S.Ld, S.rd, dtype)
        x, it = mg_solve_prepared_guess_native(_hier[key], b, x0, acc, max_it, reset, 2, x_out=x_out)
    return x, it, N.mg_last_dispatch(), N.mg_last_guess()


def _twin(S, dtype, acc, max_it, reset):
    """(x, iterations, accepted) of the twin from the system's accepted guess, computed once"""
    key = (dtype, acc, max_it, reset)
    if not hasattr(S, "twin"):
        S.twin = {}
    if key not in S.twin:
        if dtype == F64:
            S.twin[key] = G.pcg_guess(S.L, S.b, S.x0, *S.geo, acc, max_it, S.rd, reset, H=S.H)
        else:
            if not hasattr(S, "H32"):
                S.H32 = M32.Hierarchy32(S.L, *S.geo)
            S.twin[key] = G.pcg_guess_f32(S.L, S.b, S.x0, *S.geo, acc, max_it, S.rd, reset, H=S.H32)
    return S.twin[key]


def _slack(S, x):
    return 64 * EPS * np.abs(S.L[:, 2]).max() * np.abs(x).max()


# ---- 1 (and the neutral half of 5): no guess, a zero guess, a rejected guess ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("c64", "c32"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("system", SYSTEMS, ids=_sid)
def test_neutral(system, kind, dtype):
    S = _system(*system)
    for acc, max_it, reset in ((1e-8, 200, 10), (1e-30, 5, 3)):
        want, itw, dw, gw = _solve(S, kind, dtype, acc, max_it, reset)
        assert gw == 0 and itw >= 1 and dw["cycle_elem"] == (8 if dtype == F64 else 4)
        for x0 in (torch.zeros_like(S.bd), S.bad):
            x, it, d, g = _solve(S, kind, dtype, acc, max_it, reset, x0=x0)
            assert g == 2 and it == itw and d == dw, (acc, g, it, itw, d, dw)
            assert torch.equal(x, want), float((x - want).abs().max())


# ---- 2: capped solves against the twin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("system", SMALL, ids=_sid)
def test_capped_solves_from_an_accepted_guess_against_the_twin(system, kind):
    """x after K iterations from the guess against the twin's, bound K 1e-10 max|x_K| (test_gpu_mg_hierarchy.py::_check_capped_solves: the
    cycle is held to 1e-11, an iteration adds two quotients of dot products).  Largest measured fraction of the bound: printed."""
    S = _system(*system)
    worst = 0.0
    for K in (1, 2, 5, 6):
        for reset in (BIG, 3):
            xt, itt, accepted = _twin(S, F64, 1e-30, K, reset)
            x, it, d, g = _solve(S, kind, F64, 1e-30, K, reset, x0=S.x0d)
            x = x.cpu().numpy()
            assert accepted and g == 1 and it == itt == K and d["iterations"] == K and d["cycles"] == K
            assert d["residual_recomputations"] == sum(1 for k in range(1, K) if (k + 1) % reset == 0)
            assert np.all(np.isfinite(x)) and np.all(x[~S.present] == 0)
            ratio = np.abs(x - xt).max() / (K * 1e-10 * np.abs(xt).max())
            worst = max(worst, ratio)
            assert ratio <= 1, (K, reset, ratio)
    print("capped from a guess %s %s: largest max|x - x_twin| = %.2e of the bound" % (_sid(system), kind, worst))


# ---- 3 (and the accepted half of 5): converged solves ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("c64", "c32"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("system", SYSTEMS, ids=_sid)
def test_converged_solves_from_an_accepted_guess(system, kind, dtype):
    S = _system(*system)
    for acc in (1e-5, 1e-10):
        _, itt, accepted = _twin(S, dtype, acc, 200, BIG)
        x, it, d, g = _solve(S, kind, dtype, acc, 200, BIG, x0=S.x0d)
        x = x.cpu().numpy()
        first, second, floor = M.residuals(S.L, S.b, x, *S.geo, S.rd)
        print("%s %s %s accuracy %.0e: %d iterations from the guess (twin %d); true residual %.2e, c sum(x) - mean(b) %.2e (floor %.2e)"
              % (_sid(system), kind, dtype, acc, it, itt, first, second, floor))
        assert accepted and g == 1 and d["iterations"] == it < 200
        assert abs(it - itt) <= 1, (it, itt)
        assert first < acc + _slack(S, x) and second <= floor
        assert np.all(x[~S.present] == 0)


# ---- 4: zero iterations --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("c64", "c32"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("system", (SYSTEMS[3], SYSTEMS[5], SYSTEMS[6], SYSTEMS[8], SYSTEMS[10]), ids=_sid)
def test_a_converged_guess_costs_no_iteration(system, kind, dtype, piso_option):
    S = _system(*system)
    x12, it12, _, _ = _solve(S, kind, dtype, 1e-12, 200, 10)
    assert it12 < 200
    for every in (4, 1):
        piso_option("mg_check_every", every)
        x, it, d, g = _solve(S, kind, dtype, 1e-8, 200, 10, x0=x12)
        assert it == 0 and g == 1 and d["iterations"] == 0 and d["cycles"] == 0 and d["residual_recomputations"] == 0
        pres = _dev(S.present) != 0
        assert float((x - x12)[pres].abs().max()) <= 4 * EPS * float(x12.abs().max())
        assert not bool(x[~pres].any())
    x, it, _, g = _solve(S, kind, dtype, 1e-8, 1, 10, x0=x12)           # (max_iterations 1: the only look is the last one)
    assert it == 0 and g == 1


# ---- 6: x0 may be x_out ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("c64", "c32"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("system", (SYSTEMS[0], SYSTEMS[4], SYSTEMS[7], SYSTEMS[9], SYSTEMS[10]), ids=_sid)
def test_the_guess_may_be_the_output_buffer(system, kind, dtype):
    S = _system(*system)
    for guess, code in ((S.x0d, 1), (S.bad, 2)):
        for acc, max_it in ((1e-9, 200), (1e-30, 3)):
            want, itw, dw, gw = _solve(S, kind, dtype, acc, max_it, 10, x0=guess)
            buf = guess.clone()
            x, it, d, g = _solve(S, kind, dtype, acc, max_it, 10, x0=buf, x_out=buf)
            assert x is buf and gw == g == code and it == itw and d == dw
            assert torch.equal(x, want)
            other = torch.full_like(guess, float("nan"))                  # a disjoint output buffer that held NaN
            x, it, d, g = _solve(S, kind, dtype, acc, max_it, 10, x0=guess, x_out=other)
            assert g == code and it == itw and torch.equal(x, want)


# ---- 7: robustness ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("c64", "c32"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("system", (SYSTEMS[3], SYSTEMS[7], SYSTEMS[9], SYSTEMS[10]), ids=_sid)
def test_reproducible_and_robust(system, kind, dtype, piso_option):
    S = _system(*system)
    zero, itz, dz, _ = _solve(S, kind, dtype, 1e-9, 200, 10)
    want, itw, dw, gw = _solve(S, kind, dtype, 1e-9, 200, 10, x0=S.x0d)
    assert gw == 1
    for every in (1, 4, 4):
        piso_option("mg_check_every", every)
        x, it, d, g = _solve(S, kind, dtype, 1e-9, 200, 10, x0=S.x0d)
        assert g == 1 and it == itw and d == dw and torch.equal(x, want), every
    for bad in (float("nan"), float("inf")):                          # on a present cell: rejected, the from-zero bits
        x0 = S.x0d.clone()
        x0[int(np.nonzero(S.present)[0][S.present.sum() // 2])] = bad
        x, it, d, g = _solve(S, kind, dtype, 1e-9, 200, 10, x0=x0)
        assert g == 2 and it == itz and d == dz and torch.equal(x, zero)
    if (~S.present).any():                                            # garbage on solid cells is not read: the accepted solve's bits
        x0 = S.x0d.clone()
        x0[_dev(~S.present) != 0] = float("nan")
        x, it, d, g = _solve(S, kind, dtype, 1e-9, 200, 10, x0=x0)
        assert g == 1 and it == itw and torch.equal(x, want)
    bn = S.bd.clone()
    bn[int(np.nonzero(S.present)[0][5])] = float("nan")               # a NaN in b still never converges, guess or not
    for x0 in (S.x0d, S.bad):
        x, it, d, g = _solve(S, kind, dtype, 1e-9, 7, 10, x0=x0, b=bn)
        assert it == 7 and g == 2 and bool(torch.isnan(x).any())


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(piso_option):
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso import distributed as D
    from diffpiso.solvers import MgHierarchy, mg_prepare_native, mg_solve_native, mg_solve_prepared_guess_native
    S = _system(*SYSTEMS[2])
    nx, ny, per_x, per_y = S.geo
    h = mg_prepare_native(nx, ny, per_x, per_y, S.Ld, S.rd, F64)
    calls = (lambda x0: mg_solve_native(nx, ny, per_x, per_y, S.Ld, S.bd, 1e-8, 50, S.rd, 10, x0=x0),
             lambda x0: mg_solve_prepared_guess_native(h, S.bd, x0, 1e-8, 50, 10))
    want, itw = calls[0](None)
    for call in calls:
        with pytest.raises(ValueError, match="cells"):
            call(S.x0d[:-1])
        with pytest.raises(TypeError, match="floating"):
            call(torch.zeros(S.n, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="device"):
            call(S.x0d.cpu())
        x, it = call(S.x0d.to(torch.float32).reshape(1, ny, nx, 1))    # another float type and shape: cast
        assert N.mg_last_guess() == 1 and it < itw
    # the solver: refused before any launch, whatever the guess is, and ignored with the option off
    on = dp.PisoPressureSolverMultigrid(dx=[], use_guess=True)
    div = S.bd.reshape(1, ny, nx, 1)
    with pytest.raises(ValueError, match="cells"):
        on._guess_for_solve(S.x0d[:-1], div)
    with pytest.raises(ValueError, match="device"):
        on._guess_for_solve(S.x0d.cpu(), div)
    assert dp.PisoPressureSolverMultigrid(dx=[])._guess_for_solve(S.x0d[:-1], div) is None
    assert on.stats["solves"] == 0 and on.stats["guesses_accepted"] == 0
    # a slab communicator in use: refused before it is touched
    piso_option("slab_force", 1)
    on.slab_comm = object.__new__(D.SlabCommunicator)            # (no attribute beyond these two exists: touching it raises AttributeError)
    on.slab_comm.world, on.slab_comm.sharded = 1, False
    with pytest.raises(N.PisoNativeError, match="use_guess=False"):
        on._cg(nx, ny, per_x, per_y, S.Ld, S.bd, 1e-8, 50, S.rd, 10, x0=S.x0d)
    assert on.stats["hierarchy_builds"] == 0
    piso_option("slab_force", 0)
    # a buffer nobody prepared, and a hierarchy of another grid: the mismatch is reported as before, guess or not
    for dtype in DTYPES:
        with pytest.raises(N.PisoNativeError, match="not a hierarchy prepared for this grid"):
            mg_solve_prepared_guess_native(MgHierarchy(nx, ny, per_x, per_y, S.rd, dtype, "cuda"), S.bd, S.x0d, 1e-8, 50, 10)
        hh = mg_prepare_native(nx, ny, per_x, per_y, S.Ld, S.rd, dtype)
        h2 = MgHierarchy(nx - 4, ny, per_x, per_y, S.rd, dtype, "cuda")
        h2.buf = hh.buf
        with pytest.raises(N.PisoNativeError, match="not a hierarchy prepared for this grid"):
            mg_solve_prepared_guess_native(h2, S.bd[:(nx - 4) * ny], S.x0d[:(nx - 4) * ny], 1e-8, 50, 10)
        x, it = mg_solve_prepared_guess_native(hh, S.bd, S.x0d, 1e-8, 50, 10)      # ... and the hierarchy is none the worse for it
        assert it < itw and N.mg_last_guess() == 1 and bool(torch.isfinite(x).all())


# ---- 9, 10: step level -----------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _solver(p_tol, use_guess, **kw):
    """-> the solver and the list its forward solves append (iterations, piso_mg_last_guess) to"""
    import diffpiso as dp
    import diffpiso._native as N
    ps = dp.PisoPressureSolverMultigrid(dx=[], accuracy=p_tol, max_iterations=200, residual_reset=10, **({"use_guess": True} if use_guess else {}), **kw)
    log, inner = [], ps._cg

    def cg(*a, **k):
        out = inner(*a, **k)
        log.append((int(out[1]), N.mg_last_guess(), "x0" in k))
        return out
    ps._cg = cg
    return ps, log


def _forward(case, P, ps, steps, how):
    import diffpiso as dp
    P["sim"].pressure_solver = ps
    vel, p = P["velocity"], P["pressure"]
    if how == "run_piso_steps":
        td = dict(step_count=steps, loss_influence_range=steps + 1, pressure_included=False, HR_buffer_width=[[0, 0], [0, 0]])
        out = dp.run_piso_steps(vel, p, P["domain"], {}, dict(dt=case["dt"], dt_ratio=1, dx_ratio=1), td, None, None, P["sim"], None, None, None)
        return out[3].staggered_tensor(), out[4].data
    inc1 = dp.CenteredGrid(torch.full_like(p.data, 5e-13), p.box, p.extrapolation)
    inc2 = dp.CenteredGrid(torch.full_like(p.data, 1e-12), p.box, p.extrapolation)
    for i in range(steps):
        out = dp.piso_step(vel, p, inc1, inc2, case["dt"], P["sim"], P["sim"].dirichlet_values, unrolling_step=i, full_output=True)
        vel, p, inc1, inc2 = out[0], out[1], out[2], out[3]
    return vel.staggered_tensor(), p.data


def _step_case(name, ny, nx, p_tol, steps=6):
    """-> per way of stepping: (u, p, per-solve log, stats) without and with guesses"""
    c = make_case(name, ny, nx, seed=0)
    P = product_setup(c, lin_tol=1e-8, p_tol=p_tol)
    out = {}
    for how in ("run_piso_steps", "piso_step"):
        for use_guess in (False, True):
            ps, log = _solver(p_tol, use_guess)
            with torch.no_grad():
                u, p = _forward(c, P, ps, steps, how)
            assert len(log) == 2 * steps and ps.stats["solves"] == 2 * steps
            assert all(given == use_guess for _, _, given in log)
            out[(how, use_guess)] = (u, p, log, dict(ps.stats))
    return out


@pytest.mark.parametrize("p_tol,twin", ((1e-8, (45, 55)), (1e-5, (15, 35))))
def test_steps_of_a_settled_flow_take_fewer_iterations(p_tol, twin):
    """periodic 64 x 64: the previous step's increments are good guesses from step 1 on.  (twin, from the oracle's fields, steps 1 - 5: `twin`)
    The fields are held to the default's at p_tol 1e-8 only: at 1e-5 every solve is only as exact as that tolerance (measured 8.7e-06 for
    u), so there the counts are asserted and the distance is printed."""
    out = _step_case("periodic", 64, 64, p_tol)
    for how in ("run_piso_steps", "piso_step"):
        (u0, p0, log0, st0), (u1, p1, log1, st1) = out[(how, False)], out[(how, True)]
        it0, it1 = [l[0] for l in log0], [l[0] for l in log1]
        print("periodic 64 x 64 p_tol %.0e %s: iterations per solve without %s (steps 1 - 5: %d), with guesses %s (steps 1 - 5: %d; twin %d against %d); "
              "accepted %d rejected %d; u %.2e p %.2e relative L2" % (p_tol, how, it0, sum(it0[2:]), it1, sum(it1[2:]), twin[0], twin[1],
                                                                      st1["guesses_accepted"], st1["guesses_rejected"], _rel(u1, u0), _rel(p1, p0)))
        assert sum(it1[2:]) < sum(it0[2:])
        assert all(b <= a + 1 for a, b in zip(it0, it1))
        assert st1["guesses_accepted"] > 0 and st1["guesses_accepted"] + st1["guesses_rejected"] == 12
        assert "guesses_accepted" not in st0 and all(g == 0 for _, g, _ in log0)
        if p_tol == 1e-8:
            assert _rel(u1, u0) < 1e-5 and _rel(p1, p0) < 1e-5
    # the two ways of stepping hand over the same guesses
    assert [l[:2] for l in out[("run_piso_steps", True)][2]] == [l[:2] for l in out[("piso_step", True)][2]]
    assert torch.equal(out[("run_piso_steps", True)][0], out[("piso_step", True)][0])


def test_a_start_up_transient_rejects_its_guesses():
    """x-periodic walls 128 x 64 (nx x ny): in the first steps the previous increment is a worse start than zero and the guard says so."""
    out = _step_case("xper_ywall", 64, 128, 1e-8)
    for how in ("run_piso_steps", "piso_step"):
        (u0, p0, log0, st0), (u1, p1, log1, st1) = out[(how, False)], out[(how, True)]
        it0, it1 = [l[0] for l in log0], [l[0] for l in log1]
        print("xper_ywall 128 x 64 %s: iterations per solve without %s, with guesses %s, guard %s; u %.2e p %.2e relative L2"
              % (how, it0, it1, [g for _, g, _ in log1], _rel(u1, u0), _rel(p1, p0)))
        assert st1["guesses_rejected"] >= 1
        assert any(g == 2 for _, g, _ in log1[2:6])              # ... of a real guess: steps 1 and 2 start from the increments of steps 0 and 1
        assert sum(it1) <= sum(it0) + 1
        assert all(b <= a + 1 for a, b in zip(it0, it1))
        assert _rel(u1, u0) < 1e-5 and _rel(p1, p0) < 1e-5


@pytest.mark.parametrize("dtype,reuse", ((F64, False), (F32, True)), ids=("c64", "c32-reuse"))
def test_gradients_of_an_unroll_with_guesses(dtype, reuse):
    """dL/du0, dL/dp0 of a 4-step unroll at p_tol 1e-10: the adjoint solves start from zero and take no guess; parity bar 1e-5 relative L2."""
    import diffpiso as dp
    c = make_case("periodic", 64, 64, seed=0)
    P = product_setup(c, lin_tol=1e-8, p_tol=1e-10)
    res = {}
    for use_guess in (False, True):
        ps, log = _solver(1e-10, use_guess, cycle_dtype=dtype, reuse_hierarchy=reuse)
        P["sim"].pressure_solver = ps
        vel_t, p_t = P["vel_tensor"].clone().requires_grad_(True), P["pressure"].data.clone().requires_grad_(True)
        velocity = dp.StaggeredGrid(vel_t, P["velocity"].box, extrapolation=P["velocity"].extrapolation)
        pressure = dp.CenteredGrid(p_t, P["pressure"].box, P["pressure"].extrapolation)
        va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, c["dt"], P["sim"], step_count=4)
        (0.5 * (vn.staggered_tensor() ** 2).sum() + 0.5 * (pn.data ** 2).sum()).backward()
        assert len(log) == 16 and [given for _, _, given in log] == [use_guess] * 8 + [False] * 8       # 8 forward solves, then 8 adjoints
        assert ps.last_dispatch()["cycle_elem"] == (8 if dtype == F64 else 4)
        assert ps.stats["adjoint_solves"] == 8 and ps.stats.get("guesses_accepted", 0) + ps.stats.get("guesses_rejected", 0) == (8 if use_guess else 0)
        res[use_guess] = (vn.staggered_tensor().detach(), pn.data.detach(), vel_t.grad, p_t.grad, dict(ps.stats))
    off, on = res[False], res[True]
    rel = [_rel(a, b) for a, b in zip(on[:4], off[:4])]
    print("4-step unroll at 1e-10 %s reuse %s: u %.2e p %.2e dL/du0 %.2e dL/dp0 %.2e relative L2; forward iterations %d -> %d, adjoint %d -> %d, accepted %d"
          % (dtype, reuse, rel[0], rel[1], rel[2], rel[3], off[4]["iterations"], on[4]["iterations"], off[4]["adjoint_iterations"],
             on[4]["adjoint_iterations"], on[4]["guesses_accepted"]))
    assert all(r < 1e-5 for r in rel) and all(float(t.abs().max()) > 0 for t in on[:4])
    assert on[4]["guesses_accepted"] > 0 and on[4]["iterations"] <= off[4]["iterations"]
    if reuse:
        assert on[4]["hierarchy_reuses"] == off[4]["hierarchy_reuses"] > 0


def test_the_default_ignores_the_increments():
    """Without the option a solver fed non-zero increments through piso_step gives the bits it gives with any others: the default does not
    read them.  (That those bits are the parent commit's is not shown here - no golden of a multigrid step exists; it rests on the unchanged
    launch sequence of a solve without a guess and on the ISA diff of its kernels.)"""
    import diffpiso as dp
    c = make_case("periodic", 64, 64, seed=0)
    P = product_setup(c, lin_tol=1e-8, p_tol=1e-8)
    p = P["pressure"]
    res = []
    for fill in ((5e-13, 1e-12), None):
        ps, log = _solver(1e-8, False)
        P["sim"].pressure_solver = ps
        if fill is None:
            g = torch.Generator(device="cpu"); g.manual_seed(1)
            inc = [dp.CenteredGrid(torch.randn(p.data.shape, generator=g).cuda(), p.box, p.extrapolation) for _ in range(2)]
        else:
            inc = [dp.CenteredGrid(torch.full_like(p.data, v), p.box, p.extrapolation) for v in fill]
        with torch.no_grad():
            out = dp.piso_step(P["velocity"], p, inc[0], inc[1], c["dt"], P["sim"], P["sim"].dirichlet_values, full_output=True)
        assert [l[1:] for l in log] == [(0, False)] * 2 and "guesses_accepted" not in ps.stats
        res.append((out[0].staggered_tensor(), out[1].data, out[2].data, out[3].data, [l[0] for l in log]))
    assert res[0][4] == res[1][4]
    for a, b in zip(res[0][:4], res[1][:4]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
