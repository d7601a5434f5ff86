"""The prepared multigrid hierarchy (csrc/mg_prepared.h, diffpiso.solvers.MgHierarchy, PisoPressureSolverMultigrid(reuse_hierarchy=True)):
build once, solve many times.  Its oracle is the ordinary, unprepared solve of the same library, BIT FOR BIT: every comparison is
torch.equal on x plus equality of the iteration count and of the dispatch record, in both precisions of the cycle."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.cases import laplace_case, make_case, product_setup, solid_pattern

pytestmark = pytest.mark.gpu
CASES = ("periodic", "xper_ywall", "cavity", "spatial_ml")
# (ny, nx), each the smallest of its kind: everything in the tail with odd coarse dimensions; tail only, at its 4096-cell limit; one level above
# the tail with nx % 4 == 0 (the float32 cycle runs in quads); the scalar float32 path; 268 320 cells > kMgGrid * kBlock = 262 144 (the walk of
# mg_rhs_sums takes a second stride)
SHAPES = ((10, 12), (64, 64), (80, 96), (66, 70), (516, 520))
DTYPES = (torch.float64, torch.float32)
BIG = 1 << 30
_systems = {}


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _system(name, shape, seed=3, pattern=None):
    """(L, b) on the device and the call's geometry, built once per case and left unchanged."""
    key = (name, shape, seed, pattern)
    if key not in _systems:
        ny, nx = shape
        s, L, b = laplace_case(name, ny, nx, seed, solids=solid_pattern(pattern, ny, nx) if pattern else None)
        per_y, per_x = (bool(v) for v in s.periodic_yx)
        _systems[key] = (_dev(np.asarray(L, np.float64).reshape(-1, 5)), _dev(b), nx, ny, per_x, per_y, bool(s.rank_deficient))
    return _systems[key]


def _same_solve(h, L, b, geo, acc, max_it, reset, dtype, what):
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native, mg_solve_prepared_native
    nx, ny, per_x, per_y, rd = geo
    x0, it0 = mg_solve_native(nx, ny, per_x, per_y, L, b, acc, max_it, rd, reset, 2, dtype)
    d0 = N.mg_last_dispatch()
    x1, it1 = mg_solve_prepared_native(h, b, acc, max_it, reset, 2)
    d1 = N.mg_last_dispatch()
    assert it0 == it1 and d0 == d1 and d1["cycle_elem"] == (8 if dtype == torch.float64 else 4), (what, it0, it1, d0, d1)
    assert torch.equal(x0, x1), (what, float((x0 - x1).abs().max()))
    return it1


def _sweep(L, b, geo, dtype, piso_option, what):
    """Converged solves at 1e-5 and 1e-10 and capped solves with a recomputation inside, over the polling cadence and the tail."""
    from diffpiso.solvers import mg_prepare_native
    nx, ny, per_x, per_y, rd = geo
    h = mg_prepare_native(nx, ny, per_x, per_y, L, rd, dtype)
    for tail in (1, 0):
        piso_option("mg_tail", tail)
        for every in (1, 4):
            piso_option("mg_check_every", every)
            for acc in (1e-5, 1e-10):
                it = _same_solve(h, L, b, geo, acc, 500, BIG, dtype, (what, tail, every, acc))
                assert it < 500
            for max_it in (1, 2, 5):
                assert _same_solve(h, L, b, geo, 1e-30, max_it, 3, dtype, (what, tail, every, "capped", max_it)) == max_it


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_prepared_equals_unprepared(name, shape, dtype, piso_option):
    L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    assert rd == (name != "spatial_ml")
    _sweep(L, b, (nx, ny, per_x, per_y, rd), dtype, piso_option, (name, shape))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_prepared_equals_unprepared_with_a_solid_block_across_aggregates(name, dtype, piso_option):
    L, b, nx, ny, per_x, per_y, rd = _system(name, (80, 96), pattern="block2_odd")
    assert int((L[:, 2] == 0).sum()) >= 4
    _sweep(L, b, (nx, ny, per_x, per_y, rd), dtype, piso_option, (name, "block2_odd"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("periodic", "xper_ywall"))
def test_prepared_equals_unprepared_with_a_mean_in_the_right_hand_side(name, dtype, piso_option):
    """The only path that reads SC_MEAN_B: the mean mg_rhs_sums / mg_rhs_fin form must have the bits of mg_setup0 / mg_setup_fin's."""
    L, b, nx, ny, per_x, per_y, rd = _system(name, (80, 96))
    assert rd
    for pattern in (None, "block2_odd"):
        Lp, bp = _system(name, (80, 96), pattern=pattern)[:2]
        bm = torch.where(Lp[:, 2] != 0, bp + 0.37, bp)
        _sweep(Lp, bm, (nx, ny, per_x, per_y, rd), dtype, piso_option, (name, pattern, "mean"))
        from diffpiso.solvers import mg_solve_native
        x, _ = mg_solve_native(nx, ny, per_x, per_y, Lp, bm, 1e-10, 200, rd, BIG, 2, dtype)
        assert abs(float(x.sum())) > 1e-3                        # (the constant mode is there)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hierarchy_many_right_hand_sides(dtype):
    import diffpiso as dp
    from diffpiso.solvers import mg_prepare_native, mg_solve_native, mg_solve_prepared_native
    L, b, nx, ny, per_x, per_y, rd = _system("xper_ywall", (80, 96))
    Lo, bo = _system("xper_ywall", (80, 96), seed=5, pattern="block4")[:2]
    other = dp.PisoPressureSolverMultigrid(dx=[], cycle_dtype=dtype)
    h = mg_prepare_native(nx, ny, per_x, per_y, L, rd, dtype)
    rng = np.random.default_rng(17)
    for k in range(3):
        bk = b if k == 0 else _dev(rng.standard_normal(nx * ny))
        # another solver instance solves another matrix of the same size in between: it overwrites the shared "mg" workspace
        xo, _ = other._cg(nx, ny, per_x, per_y, Lo, bo, 1e-8, 200, rd, 10)
        assert bool(torch.isfinite(xo).all())
        x1, it1 = mg_solve_prepared_native(h, bk, 1e-10, 200, 10, 2)
        x0, it0 = mg_solve_native(nx, ny, per_x, per_y, L, bk, 1e-10, 200, rd, 10, 2, dtype)
        assert it0 == it1 < 200 and torch.equal(x0, x1), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sweeps", (1, 2, 3))
@pytest.mark.parametrize("shape", ((64, 64), (80, 96), (66, 70)))
def test_one_cycle_on_a_prepared_hierarchy(shape, sweeps, dtype, piso_option):
    import diffpiso._native as N
    from diffpiso.solvers import mg_prepare_native, mg_vcycle_native, mg_vcycle_prepared_native
    for name in ("periodic", "cavity"):
        L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
        h = mg_prepare_native(nx, ny, per_x, per_y, L, rd, dtype)
        r = _dev(np.random.default_rng(7).standard_normal(nx * ny))
        for tail in (1, 0):
            piso_option("mg_tail", tail)
            z0 = mg_vcycle_native(nx, ny, per_x, per_y, L, r, sweeps, dtype)
            d0 = N.mg_last_dispatch()
            z1 = mg_vcycle_prepared_native(h, r, sweeps)
            assert d0 == N.mg_last_dispatch() and d0["cycles"] == 1 and d0["sweeps"] == sweeps
            assert torch.equal(z0, z1) and float(z1.abs().max()) > 0


def test_the_cache_key():
    import diffpiso as dp
    from diffpiso.solvers import mg_solve_native
    L, b, nx, ny, per_x, per_y, rd = _system("periodic", (64, 64))
    ps = dp.PisoPressureSolverMultigrid(dx=[], reuse_hierarchy=True)
    geo = (nx, ny, per_x, per_y)
    want, itw = mg_solve_native(nx, ny, per_x, per_y, L, b, 1e-9, 200, rd, 10)

    def solve(Lt, rank_deficient=rd, builds=None, reuses=None):
        x, it = ps._cg(*geo, Lt, b, 1e-9, 200, rank_deficient, 10)
        assert (ps.stats["hierarchy_builds"], ps.stats["hierarchy_reuses"]) == (builds, reuses)
        return x, it

    Lc = L.clone()
    for n, (bu, re) in enumerate(((1, 0), (1, 1))):              # the same L twice: 1 build, 1 reuse
        x, it = solve(Lc, builds=bu, reuses=re)
        assert it == itw and torch.equal(x, want)
    Lc.mul_(1.0)                                                 # a version bump
    solve(Lc, builds=2, reuses=1)
    solve(Lc.clone(), builds=3, reuses=1)                        # an equal-valued clone: another storage
    Lk = Lc.clone()
    solve(Lk, builds=4, reuses=1)
    solve(Lk, builds=4, reuses=2)
    ps.cycle_dtype = torch.float32
    x32, it32 = solve(Lk, builds=5, reuses=2)
    w32, i32 = mg_solve_native(nx, ny, per_x, per_y, L, b, 1e-9, 200, rd, 10, 2, torch.float32)
    assert it32 == i32 and torch.equal(x32, w32)
    ps.cycle_dtype = torch.float64
    solve(Lk, builds=6, reuses=2)
    ps2 = dp.PisoPressureSolverMultigrid(dx=[], reuse_hierarchy=True)       # rank_deficient changed: a build (3 iterations: counts only)
    ps2._cg(*geo, Lk, b, 1e-9, 3, True, 10)
    ps2._cg(*geo, Lk, b, 1e-9, 3, True, 10)
    ps2._cg(*geo, Lk, b, 1e-9, 3, False, 10)
    assert (ps2.stats["hierarchy_builds"], ps2.stats["hierarchy_reuses"]) == (2, 1)
    solve(Lk, builds=6, reuses=3)
    ps.drop_hierarchy()
    solve(Lk, builds=7, reuses=3)
    # the matrix dies, a fresh one of the same size takes its place (and, without the tensor the hierarchy keeps, could take its pointer)
    Lo, bo = _system("periodic", (64, 64), seed=5, pattern="block4")[:2]
    wo, io = mg_solve_native(nx, ny, per_x, per_y, Lo, b, 1e-9, 200, rd, 10)
    L1 = L.clone()
    solve(L1, builds=8, reuses=3)
    del L1
    L2 = Lo.clone()
    x, it = ps._cg(*geo, L2, b, 1e-9, 200, rd, 10)
    assert ps.stats["hierarchy_builds"] == 9 and it == io and torch.equal(x, wo)


def _header(h):
    return np.frombuffer(h.buf[:32].cpu().numpy().tobytes(), np.int32)


def test_refusals(piso_option):
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso import distributed as D
    from diffpiso.solvers import MgHierarchy, mg_prepare_native, mg_solve_prepared_native, mg_vcycle_prepared_native
    MAGIC = int.from_bytes(b"MGH1", "little")
    NOT = "not a hierarchy prepared for this grid"
    L, b, nx, ny, per_x, per_y, rd = _system("cavity", (32, 48))
    Lp, bp, _, _, ppx, ppy, prd = _system("periodic", (32, 48))
    Ls = _system("spatial_ml", (32, 48))[0]
    border = L.clone(); border[5, 0] = 0.25                      # a -y entry in the first row of a wall-bounded grid
    zero_diag = Lp.clone(); zero_diag[nx * 7 + 9, 2] = 0.0       # a row without a diagonal that still has entries
    # (good matrix, refused matrix, per_x, per_y, rank_deficient of the good prepare, of the refused one, today's message)
    refused = ((L, border, per_x, per_y, rd, rd, "non-zero border entry in a non-periodic direction"),
               (Lp, zero_diag, ppx, ppy, prd, prd, "a row with a zero diagonal has non-zero entries"),
               (Ls, Ls, False, False, False, True, "rank_deficient = 1 but the rows of the matrix do not sum to zero"))
    for dtype in DTYPES:
        for good, bad, px, py, rd_good, rd_bad, msg in refused:
            h = MgHierarchy(nx, ny, px, py, rd_good, dtype, "cuda").prepare(good)
            assert _header(h)[0] == MAGIC and tuple(_header(h)[1:3]) == (nx, ny) and h.key is not None
            h.rank_deficient = rd_bad
            with pytest.raises(N.PisoNativeError, match=msg):
                h.prepare(bad)
            assert not _header(h).any() and h.key is None and h.matrix is None      # no valid header is left
            with pytest.raises(N.PisoNativeError, match=NOT):
                mg_solve_prepared_native(h, b, 1e-8, 50, 10, 2)
            with pytest.raises(N.PisoNativeError, match=NOT):
                mg_vcycle_prepared_native(h, b, 2)
        with pytest.raises(N.PisoNativeError, match=NOT):         # a buffer nobody prepared
            mg_solve_prepared_native(MgHierarchy(nx, ny, per_x, per_y, rd, dtype, "cuda"), b, 1e-8, 50, 10, 2)
        # a hierarchy of another grid (the buffer is large enough for the call's: nothing is read past it)
        h = mg_prepare_native(nx, ny, per_x, per_y, L, rd, dtype)
        for other in (dict(nx=nx - 4), dict(ny=ny - 2), dict(per_x=not per_x), dict(rank_deficient=not rd)):
            g = dict(nx=nx, ny=ny, per_x=per_x, per_y=per_y, rank_deficient=rd); g.update(other)
            h2 = MgHierarchy(g["nx"], g["ny"], g["per_x"], g["per_y"], g["rank_deficient"], dtype, "cuda")
            assert h2.buf.numel() <= h.buf.numel()
            h2.buf = h.buf
            with pytest.raises(N.PisoNativeError, match=NOT):
                mg_solve_prepared_native(h2, b[:g["nx"] * g["ny"]], 1e-8, 50, 10, 2)
            if "rank_deficient" not in other:
                with pytest.raises(N.PisoNativeError, match=NOT):
                    mg_vcycle_prepared_native(h2, b[:g["nx"] * g["ny"]], 2)
        x, it = mg_solve_prepared_native(h, b, 1e-8, 50, 10, 2)   # ... and is none the worse for it
        assert it < 50 and bool(torch.isfinite(x).all())
    # a float32 hierarchy through the _f64 entry (the float32 buffer is the larger one)
    hf = mg_prepare_native(nx, ny, per_x, per_y, L, rd, torch.float32)
    h64 = MgHierarchy(nx, ny, per_x, per_y, rd, torch.float64, "cuda")
    assert h64.buf.numel() <= hf.buf.numel()
    h64.buf = hf.buf
    with pytest.raises(N.PisoNativeError, match=NOT):
        mg_solve_prepared_native(h64, b, 1e-8, 50, 10, 2)
    with pytest.raises(N.PisoNativeError, match=NOT):
        mg_vcycle_prepared_native(h64, b, 2)
    # buffers one byte short are refused on the host
    x = torch.empty(nx * ny, dtype=torch.float64, device="cuda")
    it = C.c_int(0)
    for sfx, elem in (("_f64", 8), ("_c32_f64", 4)):
        hb, wb = N.lib.piso_mg_hierarchy_bytes(nx, ny, elem), N.lib.piso_mg_solve_workspace_bytes(nx, ny, elem)
        hier = torch.zeros(hb, dtype=torch.uint8, device="cuda")
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        prep = lambda h_, w_: getattr(N.lib, "piso_mg_prepare" + sfx)(nx, ny, 0, 0, N.ptr(L), 0, N.ptr(hier), C.c_size_t(h_), N.ptr(ws), C.c_size_t(w_),
                                                                       N.stream_ptr())
        solve = lambda h_, w_: getattr(N.lib, "piso_mg_pcg_solve_prepared" + sfx)(
            nx, ny, 0, 0, N.ptr(hier), C.c_size_t(h_), N.ptr(b), N.ptr(x), C.c_float(1e-8), 50, 0, 10, 2, C.byref(it), N.ptr(ws), C.c_size_t(w_), N.stream_ptr())
        cyc = lambda h_, w_: getattr(N.lib, "piso_mg_vcycle_prepared" + sfx)(nx, ny, 0, 0, N.ptr(hier), C.c_size_t(h_), N.ptr(b), N.ptr(x), 2, N.ptr(ws),
                                                                              C.c_size_t(w_), N.stream_ptr())
        for fn in (prep, solve, cyc):
            assert fn(hb - 1, wb) == 1 and b"hierarchy buffer too small" in N.lib.piso_last_error_string()
            assert fn(hb, wb - 1) == 1 and b"workspace too small" in N.lib.piso_last_error_string()
        torch.cuda.synchronize()
        assert not hier.any()                                    # nothing was written
        assert prep(hb, wb) == 0 and solve(hb, wb) == 0 and it.value < 50 and cyc(hb, wb) == 0
    # a slab communicator in use: refused before it is touched
    piso_option("slab_force", 1)
    ps = dp.PisoPressureSolverMultigrid(dx=[], reuse_hierarchy=True)
    ps.slab_comm = object.__new__(D.SlabCommunicator)            # (no attribute beyond these two exists: touching it raises AttributeError)
    ps.slab_comm.world, ps.slab_comm.sharded = 1, False
    with pytest.raises(N.PisoNativeError, match="reuse_hierarchy=False"):
        ps._cg(nx, ny, per_x, per_y, L, b, 1e-8, 50, rd, 10)
    assert ps.stats["hierarchy_builds"] == 0


# ---- step level ------------------------------------------------------------------------------------------------------------------------------
def _run(P, vel0, p0, box, v_ext, p_ext, dt, steps, reuse, dtype):
    import diffpiso as dp
    ps = dp.PisoPressureSolverMultigrid(dx=[], accuracy=1e-6, max_iterations=200, residual_reset=10, cycle_dtype=dtype, reuse_hierarchy=reuse)
    P["sim"].pressure_solver = ps
    vel_t, p_t = vel0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
    velocity = dp.StaggeredGrid(vel_t, box, extrapolation=v_ext)
    pressure = dp.CenteredGrid(p_t, box, p_ext)
    va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, dt, P["sim"], step_count=steps)
    (0.5 * (vn.staggered_tensor() ** 2).sum() + 0.5 * (pn.data ** 2).sum()).backward()
    return (vn.staggered_tensor().detach(), pn.data.detach(), vel_t.grad, p_t.grad), ps


def _problems():
    import bench
    import diffpiso as dp
    P = bench.build_problem(64, torch.device("cuda"), 1e-6, 2000, 10)
    ext = dp.Material.extrapolation_mode(P["domain"].boundaries)
    yield "bench64", P, P["vel_t"], P["p_t"], P["domain"].box, ext, dp.pressure_extrapolation(P["domain"].boundaries), P["dt"]
    c = make_case("xper_ywall", 32, 64, seed=2)
    Q = product_setup(c, lin_tol=1e-6, p_tol=1e-6)
    yield "xper_ywall 64 x 32", Q, Q["vel_tensor"], Q["pressure"].data, Q["velocity"].box, Q["velocity"].extrapolation, Q["pressure"].extrapolation, c["dt"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_step_and_an_unroll_with_and_without_reuse(dtype):
    """One step forward and backward, and a 2-step unroll.  A step solves one pressure matrix four times (two correctors, two adjoints) and
    calls solve_flat twice: without the option that is 4 hierarchy builds and 2 matrix builds a step; with it the correctors share the matrix
    tensor (1 matrix build a step) and the backward of step k meets adjoint 2 and adjoint 1 of the same matrix (2 N - 1 hierarchy builds)."""
    for what, P, vel0, p0, box, v_ext, p_ext, dt in _problems():
        for steps, builds_on, builds_off, lap_on, lap_off in ((1, 1, 4, 1, 2), (2, 3, 8, 2, 4)):
            off, ps_off = _run(P, vel0, p0, box, v_ext, p_ext, dt, steps, False, dtype)
            on, ps_on = _run(P, vel0, p0, box, v_ext, p_ext, dt, steps, True, dtype)
            for k, (a, b) in enumerate(zip(off, on)):
                assert torch.equal(a, b) and float(a.abs().max()) > 0, (what, steps, ("u", "p", "dL/du0", "dL/dp0")[k])
            so, sn = dict(ps_off.stats), dict(ps_on.stats)
            print(what, steps, "steps: off", so, "on", sn)
            for k in ("solves", "iterations", "adjoint_solves", "adjoint_iterations"):
                assert so[k] == sn[k] > 0, (what, steps, k)
            assert so["solves"] == so["adjoint_solves"] == 2 * steps
            assert (sn["hierarchy_builds"], sn["hierarchy_reuses"]) == (builds_on, 4 * steps - builds_on), (what, steps)
            assert (so["hierarchy_builds"], so["hierarchy_reuses"]) == (builds_off, 0), (what, steps)
            assert (sn["laplace_builds"], so["laplace_builds"]) == (lap_on, lap_off), (what, steps)
