"""The multigrid-preconditioned pressure CG on y-slabs (csrc/mg_slab.h) in ONE process: V virtual ranks over the loopback link (rows copied
between the ranks' arrays, no mailbox), held to the one-GPU solver (csrc/mg.hip) - the hierarchy and a V-cycle bit for bit (per-cell code on
identical inputs, no sum in either), capped and converged solves to the bounds tests/test_gpu_mg_hierarchy.py uses for two summation
orders - and a ring of one through a real peer communicator, where the wrap rows and the gather travel through the rank's own mailbox.
"Knob" is the option mg_slab_gather_cells, which moves the first replicated level g so that small grids have sharded levels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mg_reference as M
from tests.cases import check_pressure_matrix, laplace_case

pytestmark = pytest.mark.gpu
ACC = 1e-10
BIG = 1 << 30
BORDERS = ("periodic", "cavity", "spatial_ml", "xper_ywall")
# (nx, ny, knob, ranks) -> g; knob 0: none.  The accepted rows of tests/test_mg_slab_plan_cpu.py without the two large ones
ROWS = {(64, 64, 64, 1): 3, (64, 64, 64, 2): 3, (64, 64, 64, 4): 3, (64, 64, 64, 8): 3, (70, 96, 64, 2): 4, (70, 96, 64, 3): 4, (70, 96, 128, 4): 3,
        (64, 64, 0, 1): 0, (64, 64, 0, 2): 0, (64, 64, 0, 4): 0, (64, 64, 0, 8): 0, (512, 256, 0, 2): 2, (512, 256, 0, 4): 2}
SOLID_ROWS = ((64, 64, 64, 4), (70, 96, 64, 2), (70, 96, 64, 3))
SOLIDS = ("block_on_cut", "seam_at_cut", "random10")
CAPS = ((1, BIG), (2, BIG), (5, 3), (6, 3))                     # (K, residual_reset)
SYSTEMS = tuple((row, name, "none") for row in sorted(ROWS) for name in BORDERS) + \
    tuple((row, name, pat) for row in SOLID_ROWS for name in BORDERS for pat in SOLIDS)


def _gid(v):
    if isinstance(v, tuple) and len(v) == 4:
        return "%dx%d-knob%d-%dranks" % v
    return str(v)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _solids(pattern, nx, ny, name):
    """block_on_cut: 4 x 4 blocks straddling the cuts at rows 32 (2 and 4 ranks of 64 rows, 3 ranks of 96) and 48 (2 ranks of 96 rows);
    seam_at_cut: single cells on the x seam in the rows either side of those cuts and in the last row (next to the cut the y wrap crosses);
    random10: 10 % of the cells, the first seed whose pattern check_pressure_matrix accepts (connected, no enclosed fluid cell)."""
    if pattern == "none":
        return []
    if pattern == "block_on_cut":
        return [(j, i) for j0, i0 in ((30, 20), (46, 40)) for j in range(j0, j0 + 4) for i in range(i0, i0 + 4)]
    if pattern == "seam_at_cut":
        return [(31, 0), (32, nx - 1), (47, nx - 1), (48, 0), (ny - 1, 0), (ny - 2, nx - 1)]
    assert pattern == "random10"
    for seed in range(1, 50):
        rng = np.random.default_rng(seed)
        k = np.sort(rng.choice(ny * nx, size=ny * nx // 10, replace=False))
        solids = [(int(c) // nx, int(c) % nx) for c in k]
        s, L, b = laplace_case(name, ny, nx, 3, solids=solids)
        try:
            check_pressure_matrix(L, nx, ny, bool(s.periodic_yx[1]), bool(s.periodic_yx[0]), s.rank_deficient)
        except AssertionError:
            continue
        dead = set(solids)
        if not any((j, i) not in dead and L.reshape(-1, 5)[j * nx + i, 2] == 0 for j in range(ny) for i in range(nx) if name != "cavity" or j < ny - 1):
            return solids
    raise AssertionError("no seed gives a valid random pattern")


@functools.lru_cache(maxsize=None)
def _system(name, nx, ny, pattern="none"):
    solids = _solids(pattern, nx, ny, name)
    s, L, b = laplace_case(name, ny, nx, 3, solids=solids)
    per_y, per_x = (bool(v) for v in s.periodic_yx)
    L = np.ascontiguousarray(np.asarray(L, np.float64).reshape(-1, 5))
    check_pressure_matrix(L, nx, ny, per_x, per_y, s.rank_deficient)
    return dict(L=L, b=np.asarray(b, np.float64).ravel(), nx=nx, ny=ny, per_x=per_x, per_y=per_y, rd=bool(s.rank_deficient), present=L[:, 2] != 0,
                Ld=_dev(L), bd=_dev(b))


def _args(S):
    return S["nx"], S["ny"], S["per_x"], S["per_y"], S["Ld"]


@functools.lru_cache(maxsize=None)
def _native_cycles(name, nx, ny, pattern, sweeps, tail):
    """The whole-grid cycle on the fixed random r: computed once, shared, never changed."""
    import diffpiso._native as N
    from diffpiso.solvers import mg_vcycle_native
    S = _system(name, nx, ny, pattern)
    saved = N.get_option("mg_tail")
    N.set_option("mg_tail", tail)
    try:
        return mg_vcycle_native(*_args(S), _rand(nx * ny), sweeps)
    finally:
        N.set_option("mg_tail", saved)


@functools.lru_cache(maxsize=None)
def _rand(n):
    return _dev(np.random.default_rng(7).standard_normal(n))


@functools.lru_cache(maxsize=None)
def _native_solve(name, nx, ny, pattern, acc, K, reset):
    from diffpiso.solvers import mg_solve_native
    S = _system(name, nx, ny, pattern)
    return mg_solve_native(*_args(S), S["bd"], acc, K, S["rd"], reset)


def _setup(row, name, pattern, piso_option):
    import diffpiso._native as N
    nx, ny, knob, ranks = row
    piso_option("mg_slab_gather_cells", knob if knob else -1)
    plan = N.mg_slab_plan(nx, ny, ranks)
    assert plan["g"] == ROWS[row], plan
    return _system(name, nx, ny, pattern), plan


# ---- hierarchy, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,name,pattern", SYSTEMS, ids=_gid)
def test_hierarchy_bit_for_bit(row, name, pattern, piso_option):
    from diffpiso.distributed import mg_level_slab_emulated
    from diffpiso.solvers import mg_level_native
    S, plan = _setup(row, name, pattern, piso_option)
    nx, ny, knob, ranks = row
    for l, (nxl, nyl) in enumerate(plan["levels"]):
        want, wx, wy = mg_level_native(*_args(S), l)
        assert (wx, wy) == (nxl, nyl)
        for rank in (range(ranks) if l < plan["g"] else (0, ranks - 1)):
            got, gx, rows = mg_level_slab_emulated(ranks, rank, *_args(S), l)
            assert gx == nxl and rows == plan["rows"][l]
            part = want if l >= plan["g"] else want[rank * rows * nxl:(rank + 1) * rows * nxl]
            assert torch.equal(got, part), (l, rank)


# ---- one V-cycle, bit for bit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,name,pattern", SYSTEMS, ids=_gid)
def test_vcycle_bit_for_bit(row, name, pattern, piso_option):
    import diffpiso._native as N
    from diffpiso.distributed import mg_vcycle_slab_emulated
    S, plan = _setup(row, name, pattern, piso_option)
    nx, ny, knob, ranks = row
    r = _rand(nx * ny)
    for tail in (1, 0):
        piso_option("mg_tail", tail)
        for sweeps in (1, 2, 3):
            want = _native_cycles(name, nx, ny, pattern, sweeps, tail)
            got = mg_vcycle_slab_emulated(ranks, *_args(S), r, sweeps)
            d = N.mg_last_dispatch()
            assert (d["levels"], d["tail_first"], d["sweeps"], d["cycles"]) == (len(plan["levels"]), plan["tail_first"] if tail else -1, sweeps, 1)
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got, want), (tail, sweeps, float((got - want).abs().max()))


# ---- capped solves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,name,pattern", SYSTEMS, ids=_gid)
def test_capped_solves(row, name, pattern, piso_option):
    """x after K iterations against the one-GPU solver's x after K.  Bound K 1e-10 max|x_K|, the one tests/test_gpu_mg_hierarchy.py uses for
    two summation orders (the cycle is bit for bit; every iteration adds two quotients of dot products grouped by other rows).  Largest
    measured fraction of the bound: DESIGN.md 3.7."""
    from diffpiso.distributed import mg_solve_slab_emulated
    S, plan = _setup(row, name, pattern, piso_option)
    nx, ny, knob, ranks = row
    worst = 0.0
    for K, reset in CAPS:
        want, itw = _native_solve(name, nx, ny, pattern, 1e-30, K, reset)
        got, it = mg_solve_slab_emulated(ranks, *_args(S), S["bd"], 1e-30, K, S["rd"], reset)
        assert it == itw == K
        assert bool(torch.isfinite(got).all()) and bool((got[torch.tensor(~S["present"], device="cuda")] == 0).all())
        bound = K * 1e-10 * float(want.abs().max())
        ratio = float((got - want).abs().max()) / bound
        worst = max(worst, ratio)
        print("capped %s %s %s K=%d reset=%s: %.2e of the bound" % (_gid(row), name, pattern, K, "none" if reset == BIG else reset, ratio))
        assert ratio <= 1.0, (K, reset, ratio)
    print("capped worst %s %s %s: %.3e" % (_gid(row), name, pattern, worst))


# ---- converged solves, reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,name,pattern", SYSTEMS, ids=_gid)
def test_converged_solve_and_reproducibility(row, name, pattern, piso_option):
    from diffpiso.distributed import mg_solve_slab_emulated
    S, plan = _setup(row, name, pattern, piso_option)
    nx, ny, knob, ranks = row
    want, itw = _native_solve(name, nx, ny, pattern, ACC, 400, BIG)
    assert itw < 400
    x, it = mg_solve_slab_emulated(ranks, *_args(S), S["bd"], ACC, 400, S["rd"], BIG)
    assert abs(it - itw) <= 1, (it, itw)
    xh = x.cpu().numpy()
    first, second, floor = M.residuals(S["L"], S["b"], xh, nx, ny, S["per_x"], S["per_y"], S["rd"])
    slack = 64 * np.finfo(np.float64).eps * np.abs(S["L"][:, 2]).max() * np.abs(xh).max()
    print("solve %s %s %s: %d iterations (one GPU %d); true residual %.2e, c sum(x) - mean(b) %.2e (floor %.2e)" % (_gid(row), name, pattern, it, itw, first, second, floor))
    assert first < ACC + slack and second <= floor
    assert np.all(xh[~S["present"]] == 0)
    x2, it2 = mg_solve_slab_emulated(ranks, *_args(S), S["bd"], ACC, 400, S["rd"], BIG)
    assert it2 == it and torch.equal(x2, x)
    for every in (1, 7):
        piso_option("mg_check_every", every)
        xe, ite = mg_solve_slab_emulated(ranks, *_args(S), S["bd"], ACC, 400, S["rd"], BIG)
        assert ite == it and torch.equal(xe, x), every


# ---- NaN hygiene: a caller workspace of 0xFF bytes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BORDERS)
@pytest.mark.parametrize("row", ((64, 64, 64, 4), (70, 96, 64, 3), (64, 64, 0, 2)), ids=_gid)
def test_workspace_of_nan_bytes(row, name, piso_option):
    """A halo row at a wall that nothing writes would come out of a workspace of NaN bytes as NaN: the results must be the same bits as
    with any other workspace."""
    import diffpiso._native as N
    from diffpiso.distributed import mg_solve_slab_emulated, mg_vcycle_slab_emulated
    S, plan = _setup(row, name, "none", piso_option)
    nx, ny, knob, ranks = row
    nbytes = N.lib.piso_mg_slab_workspace_bytes(nx, ny // ranks, ranks, ranks)
    assert nbytes > 0

    def ws(byte):
        return torch.full((nbytes,), byte, dtype=torch.uint8, device="cuda")
    r = _rand(nx * ny)
    for sweeps in (2, 3):
        z = mg_vcycle_slab_emulated(ranks, *_args(S), r, sweeps, workspace=ws(0xFF))
        assert bool(torch.isfinite(z).all()) and torch.equal(z, _native_cycles(name, nx, ny, "none", sweeps, 1))
    x, it = mg_solve_slab_emulated(ranks, *_args(S), S["bd"], ACC, 400, S["rd"], 3, workspace=ws(0xFF))
    x0, it0 = mg_solve_slab_emulated(ranks, *_args(S), S["bd"], ACC, 400, S["rd"], 3, workspace=ws(0))
    assert it == it0 < 400 and bool(torch.isfinite(x).all()) and torch.equal(x, x0)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(piso_option):
    import diffpiso._native as N
    from diffpiso.distributed import mg_solve_slab_emulated, mg_vcycle_slab_emulated
    piso_option("mg_slab_gather_cells", 64)
    S = _system("periodic", 70, 96)
    with pytest.raises(N.PisoNativeError, match=r"divisible by 2\^g.*24 rows per rank are not divisible by 16.*PisoPressureSolverCudaCustom"):
        mg_solve_slab_emulated(4, *_args(S), S["bd"], 1e-8, 50, S["rd"], 10)
    with pytest.raises(N.PisoNativeError, match="PisoPressureSolverCudaCustom"):
        N.mg_slab_plan(70, 96, 4)
    with pytest.raises(N.PisoNativeError, match="not divisible by 5 ranks"):
        mg_vcycle_slab_emulated(5, *_args(S), S["bd"], 2)
    # a workspace one byte short
    need = N.lib.piso_mg_slab_workspace_bytes(70, 48, 2, 2)
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(N.PisoNativeError, match="workspace too small"):
        mg_solve_slab_emulated(2, *_args(S), S["bd"], 1e-8, 50, S["rd"], 10, workspace=small)
    with pytest.raises(N.PisoNativeError, match="workspace too small"):
        mg_vcycle_slab_emulated(2, *_args(S), S["bd"], 2, workspace=small)
    mg_solve_slab_emulated(2, *_args(S), S["bd"], 1e-8, 50, S["rd"], 10, workspace=torch.empty(need, dtype=torch.uint8, device="cuda"))
    # the pattern refusals of the set-up, with the offending row on a rank other than 0 (4 ranks of 16 rows)
    C4 = _system("cavity", 64, 64)
    bad = C4["L"].copy()
    bad[63 * 64 + 5, 4] = 0.25                                  # a +y entry in the last row of a wall-bounded grid: rank 3
    with pytest.raises(N.PisoNativeError, match="border"):
        mg_solve_slab_emulated(4, 64, 64, C4["per_x"], C4["per_y"], _dev(bad), C4["bd"], 1e-8, 50, C4["rd"], 10)
    P4 = _system("periodic", 64, 64)
    cell = 40 * 64 + 20                                         # rank 2
    zeroed = P4["L"].copy()
    zeroed[cell] = 0                                            # its neighbours still couple into it: their rows no longer sum to zero
    bz = P4["b"].copy()
    bz[cell] = 0
    with pytest.raises(N.PisoNativeError, match="sum to zero"):
        mg_solve_slab_emulated(4, 64, 64, True, True, _dev(zeroed), _dev(bz), 1e-8, 50, True, 10)
    nodiag = P4["L"].copy()
    nodiag[cell, 2] = 0
    with pytest.raises(N.PisoNativeError, match="zero diagonal"):
        mg_solve_slab_emulated(4, 64, 64, True, True, _dev(nodiag), P4["bd"], 1e-8, 50, True, 10)
    with pytest.raises(N.PisoNativeError, match="zero diagonal"):
        mg_vcycle_slab_emulated(4, 64, 64, True, True, _dev(nodiag), P4["bd"], 2)


# ---- a ring of one through a real communicator ----------------------------------------------------------------------------------------------------
@pytest.fixture
def ring_of_one():
    from diffpiso.distributed import SlabCommunicator
    comm = SlabCommunicator(rank=0, world=1, transport="peer")
    yield comm
    comm.close()


@pytest.mark.parametrize("force", (0, 1))
def test_ring_of_one_vcycle_bit_for_bit(ring_of_one, force, piso_option):
    """64 x 64 periodic, knob 64: the wrap rows of every sharded level travel through the rank's own mailbox (force = 1: the rows of level g
    and the error flag as well)."""
    from diffpiso.distributed import mg_solve_slab_local, mg_vcycle_slab_local
    piso_option("mg_slab_gather_cells", 64)
    piso_option("slab_force", force)
    S = _system("periodic", 64, 64)
    r = _rand(64 * 64)
    for sweeps in (1, 2, 3):
        z = mg_vcycle_slab_local(ring_of_one, 64, 64, True, True, S["Ld"], r, sweeps)
        assert torch.equal(z, _native_cycles("periodic", 64, 64, "none", sweeps, 1)), sweeps
    for K, reset in CAPS:
        want, _ = _native_solve("periodic", 64, 64, "none", 1e-30, K, reset)
        got, it = mg_solve_slab_local(ring_of_one, 64, 64, True, True, S["Ld"], S["bd"], 1e-30, K, S["rd"], reset)
        assert it == K and float((got - want).abs().max()) <= K * 1e-10 * float(want.abs().max())
    st = ring_of_one.stats()
    assert st["transport"] == "peer" and st["persistent_fallbacks"] == 0 and st["verification_failures"] == 0


def test_allgather_ring_of_one(ring_of_one, piso_option):
    import diffpiso._native as N
    from diffpiso.distributed import comm_allgather
    piso_option("slab_force", 1)
    bits = torch.tensor([0x7FF8000000000001, 0x7FF0000000000123 - (1 << 63), -(1 << 63), 0x7FF0000000000000, 0x7FF0000000000000 - (1 << 63), 0, 1,
                         0x3FF0000000000000], dtype=torch.int64, device="cuda")        # quiet / signalling NaN payloads, -0.0, +-inf, 0, a denormal, 1.0
    out = comm_allgather(ring_of_one, bits.view(torch.float64))
    assert torch.equal(out.view(torch.int64), bits)
    # the largest payload, and one more
    big = torch.arange(8192, device="cuda", dtype=torch.float64) * 1.25 - 3.0
    assert torch.equal(comm_allgather(ring_of_one, big), big)
    over = torch.zeros(8193, dtype=torch.float64, device="cuda")
    dst = torch.zeros(8193, dtype=torch.float64, device="cuda")
    assert N.lib.piso_comm_allgather_f64(ring_of_one.handle, N.ptr(over), N.ptr(dst), 8193, N.stream_ptr()) == 1
    assert b"8192" in N.lib.piso_last_error_string()
    # three gathers in a row (both halves of the area, then the first again), interleaved with halo messages
    msgs = (C.c_int * 28)(1, 10, 0, 0, 5, 0, 0, 1, 20, 0, 0, 5, 0, 0, 1, 40, 0, 0, 5, 0, 0, 1, 50, 0, 0, 5, 0, 0)
    for k in range(3):
        src = torch.arange(100 + k, device="cuda", dtype=torch.float64) + 1000.0 * k
        v = torch.arange(100, device="cuda", dtype=torch.float64)
        N.check(N.lib.piso_comm_exchange(ring_of_one.handle, N.ptr(v), 1, msgs, N.stream_ptr()), "piso_comm_exchange")
        out = comm_allgather(ring_of_one, src)
        N.check(N.lib.piso_comm_exchange(ring_of_one.handle, N.ptr(v), 1, msgs, N.stream_ptr()), "piso_comm_exchange")
        N.check(N.lib.piso_comm_check(ring_of_one.handle, N.stream_ptr()), "piso_comm_check")
        ref = torch.arange(100, device="cuda", dtype=torch.float64)
        ref[40:45] = ref[10:15]; ref[50:55] = ref[20:25]
        assert torch.equal(out, src) and torch.equal(v, ref), k


def test_solver_object_forward_and_adjoint(ring_of_one, piso_option):
    """PisoPressureSolverMultigrid with the communicator (slab_force: the ring of one runs the slab solve) through _PressureSolveFn, forward and
    adjoint, against the solver without communicator: capped solves of K = 6 iterations (accuracy far below anything a residual reaches),
    held to the capped solves' bound on the float64 results of the two solves - the function hands them on as float32, whose rounding is
    coarser than the bound, so the float32 outputs are only checked to be those results' casts."""
    import diffpiso as dp
    from diffpiso.solvers import _PressureSolveFn
    piso_option("mg_slab_gather_cells", 64)
    piso_option("slab_force", 1)
    S = _system("periodic", 64, 64)
    w = torch.tensor(np.random.default_rng(9).standard_normal((1, 64, 64, 1)), dtype=torch.float32, device="cuda")
    runs = {}
    for tag, comm in (("one", None), ("slab", ring_of_one)):
        ps = dp.PisoPressureSolverMultigrid(dx=[], accuracy=1e-30, max_iterations=6, residual_reset=3)
        ps.slab_comm = comm
        seen, inner = [], ps._cg

        def spy(*a, _inner=inner, _seen=seen):
            x, it = _inner(*a)
            _seen.append((x.clone(), it))
            return x, it
        ps._cg = spy
        div = S["bd"].reshape(1, 64, 64, 1).clone().requires_grad_(True)
        p, it = _PressureSolveFn.apply(div, S["Ld"], ps, 64, 64, True, True, S["rd"])
        (p * w).sum().backward()                               # (dL/dp = w whatever p is: both adjoint solves get the same right-hand side)
        assert ps.last_iterations == int(it) == seen[0][1] and ps.last_adjoint_iterations == seen[1][1]
        assert ps.stats["solves"] == 1 and ps.stats["adjoint_solves"] == 1
        assert torch.equal(p.reshape(-1), seen[0][0].to(torch.float32)) and torch.equal(div.grad.reshape(-1), seen[1][0].to(torch.float32))
        runs[tag] = seen
    for k in (0, 1):
        (xa, ita), (xb, itb) = runs["one"][k], runs["slab"][k]
        assert ita == itb == 6
        assert float((xa - xb).abs().max()) <= 6 * 1e-10 * float(xa.abs().max()), k
    assert dp.PisoPressureSolverMultigrid.last_dispatch()["levels"] == 5
