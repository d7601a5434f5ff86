"""The float32 V-cycle under the fp64 multigrid PCG, checked on the host: its numpy twin (tests/mg_reference_f32.py) against the fp64 twin
(tests/mg_reference.py) - hierarchy, one cycle, iteration counts of the mixed iteration - and the parts of the product that need no GPU
(workspace sizes, the cycle_dtype keyword and its refusals).  test_gpu_mg_f32.py holds the HIP kernels to the float32 twin."""
import numpy as np
import pytest

from tests import mg_reference as M
from tests import mg_reference_f32 as M32
from tests.cases import laplace_case
from tests.test_mg_reference import CASES, SHAPES


def _system(name, shape, seed=3):
    ny, nx = shape
    s, L, b = laplace_case(name, ny, nx, seed)
    per_y, per_x = (bool(v) for v in s.periodic_yx)
    return np.asarray(L, np.float64).reshape(-1, 5), b, nx, ny, per_x, per_y, bool(s.rank_deficient)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_float32_hierarchy_is_the_fp64_hierarchy_rounded_once_per_level(name, shape):
    L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    H, H32 = M.Hierarchy(L, nx, ny, per_x, per_y), M32.Hierarchy32(L, nx, ny, per_x, per_y)
    assert len(H32.levels) == len(H.levels)
    for l in range(len(H.levels)):
        want, nxl, nyl = H.level_rows(l)
        got, gx, gy = H32.level_rows(l)
        assert (gx, gy) == (nxl, nyl)
        # one rounding per level, with margin 2
        assert np.abs(got - want).max() <= (l + 1) * 2.0 ** -23 * np.abs(want).max(), (name, shape, l)
        assert np.array_equal(got[:, 2] != 0, want[:, 2] != 0)
    assert np.array_equal(H32.level_rows(0)[0], L.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_float32_cycle_against_the_fp64_cycle(name, shape):
    L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    H, H32 = M.Hierarchy(L, nx, ny, per_x, per_y), M32.Hierarchy32(L, nx, ny, per_x, per_y)
    rng = np.random.default_rng(7)
    a = rng.standard_normal(nx * ny)
    z, want = H32.cycle(a), H.cycle(a)
    dev = np.abs(z - want).max() / np.abs(want).max()
    print("%s %s: float32 cycle deviates from the fp64 cycle by %.2e max|z|" % (name, shape, dev))
    assert dev < 1e-5                  # a sanity bound against a wrong twin, not a precision claim
    assert z @ a < 0
    # the float64 evaluation on the float32 hierarchy sits between the two
    assert np.abs(H32.cycle(a, dtype=np.float64) - want).max() < 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("shape", ((33, 70), (130, 129)))
@pytest.mark.parametrize("name", CASES)
def test_mixed_iteration_counts_follow_the_fp64_twin(name, shape):
    L, b, nx, ny, per_x, per_y, rd = _system(name, shape)
    H, H32 = M.Hierarchy(L, nx, ny, per_x, per_y), M32.Hierarchy32(L, nx, ny, per_x, per_y)
    for acc, extra in ((1e-5, 1), (1e-10, 3)):
        x64, it64 = M.pcg(L, b, nx, ny, per_x, per_y, acc, 300, rd, H=H)
        x, it = M32.pcg_mixed(L, b, nx, ny, per_x, per_y, acc, 300, rd, H=H32)
        first, second, floor = M.residuals(L, b, x, nx, ny, per_x, per_y, rd)
        print("%-10s %-10s accuracy %.0e: fp64 cycle %3d iterations, float32 cycle %3d; true residual %.2e, |x - x_fp64| / max|x| %.2e"
              % (name, shape, acc, it64, it, first, np.abs(x - x64).max() / np.abs(x64).max()))
        assert it64 <= it <= it64 + extra
        assert first < 2 * acc


def test_workspace_sizes_and_the_cycle_dtype_keyword():
    import torch
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso.distributed import SlabCommunicator
    assert N.lib.piso_mg_workspace_bytes_cycle(64, 64, 8) == N.lib.piso_mg_workspace_bytes(64, 64) > 0
    assert N.lib.piso_mg_workspace_bytes_cycle(64, 64, 4) > 0
    assert N.lib.piso_mg_workspace_bytes_cycle(64, 64, 2) == 0
    assert N.lib.piso_mg_workspace_bytes_cycle(3, 64, 4) == 0
    assert N.MG_DISPATCH_FIELDS[-2:] == ("cycle_elem", "vec_mask") and len(N.MG_DISPATCH_FIELDS) == 8
    saved = N.get_option("mg_f32_vec")                      # the option exists: a set / restore round trip
    try:
        N.set_option("mg_f32_vec", 0)
        assert N.get_option("mg_f32_vec") == 0
    finally:
        N.set_option("mg_f32_vec", saved)
    ps = dp.PisoPressureSolverMultigrid(dx=[], cycle_dtype=torch.float32)
    assert ps.cycle_dtype == torch.float32 and dp.PisoPressureSolverMultigrid(dx=[]).cycle_dtype == torch.float64
    with pytest.raises(ValueError, match="cycle_dtype"):
        dp.PisoPressureSolverMultigrid(dx=[], cycle_dtype=torch.float16)
    with pytest.raises(ValueError, match="PisoPressureSolverCudaCustom"):
        dp.PisoPressureSolverMultigrid(dx=[], cast_to_double=False, cycle_dtype=torch.float32)
    # a communicator that would cut the solve: refused before any launch
    comm = object.__new__(SlabCommunicator)
    comm.world, comm.sharded = 2, False
    ps.slab_comm = comm
    L = torch.zeros(64, 5, dtype=torch.float64)
    with pytest.raises(N.PisoNativeError, match=r"cycle_dtype=torch\.float64"):
        ps._cg(8, 8, True, True, L, torch.zeros(64, dtype=torch.float64), 1e-8, 10, True, 10)
