"""The slab multigrid with the float32 cycle (csrc/mg_slab_f32.h) over real PROCESSES: 2 and 4 ranks share the one GPU, their mailboxes are
mapped across the processes, the float halo rows, the sums and the float rows of level g travel through them (tests/mg_slab_f32_worker.py is
a rank).  What this cannot cover is the xGMI hop itself.  At most FOUR ranks, as everywhere in the suite.  Every process is waited for with a
time limit (240 s the solver cases, 300 s the step); a rank that dies or times out fails the test and nothing is tried again."""
import pytest

from tests.test_gpu_multiproc import run_ranks

pytestmark = pytest.mark.gpu
WORKER = "mg_slab_f32_worker.py"
# (nx, ny, knob, border) -> (g, vec_mask with the tail)
SOLVER_CASES = {(64, 64, 64, "periodic"): (3, 0b111), (64, 64, 64, "cavity"): (3, 0b111), (512, 256, 0, "periodic"): (2, 0b111)}


@pytest.mark.parametrize("world", (2, 4))
@pytest.mark.parametrize("case", sorted(SOLVER_CASES), ids=lambda c: "%dx%d-knob%d-%s" % c)
def test_float32_cycle_on_slabs_over_processes(world, case):
    nx, ny, knob, border = case
    g, mask = SOLVER_CASES[case]
    res = run_ranks(world, nx, ny, False, timeout=240, worker=WORKER, extra=["solver", str(nx), str(ny), str(knob), border])
    assert len(res) == world
    for r in res:
        print(r)
        assert r["ok"], r
        assert r["plan"]["g"] == g and r["plan"]["world"] == world
        assert r["vcycle_equal"] == [True, True, True]          # the rank's rows of the one-GPU float32 cycle, bit for bit
        assert all(d["cycle_elem"] == 4 and d["vec_mask"] == mask for d in r["dispatch"]), r["dispatch"]
        its, itw = r["converged_its"]
        assert itw < 400 and abs(its - itw) <= 1, r["converged_its"]
        assert r["converged_diff"] <= 1e-8
        assert r["allgather_ok"]
        st = r["stats"]
        assert st["transport"] == "peer" and st["persistent_fallbacks"] == 0 and st["verification_failures"] == 0, st
    assert len({r["converged_its"][0] for r in res}) == 1        # every rank took the same decisions


def test_sharded_step_with_the_float32_cycle_matches_one_gpu():
    """Two ranks, ONE 128 x 256 periodic box (g = 1), two unrolled steps forward + reverse sweep, PisoPressureSolverMultigrid(cycle_dtype=
    torch.float32) with converged solves (pressure 1e-10) on the ranks' rows: loss and |dL/du_0| against the same box on one GPU with the same
    solver to 1e-5 relative, every pressure solve's count within one of the one-GPU step's."""
    one = run_ranks(1, 128, 256, False, timeout=300, worker=WORKER, extra=["step", "128", "256", "2"])[0]
    two = run_ranks(2, 128, 256, False, timeout=300, worker=WORKER, extra=["step", "128", "256", "2"])
    print(one, two)
    assert one["ok"], one
    assert one["dispatch"]["cycle_elem"] == 4
    for r in two:
        assert r["ok"], r
        assert r["non_finite"] == [0, 0, 0, 0] and r["warn"] == 0.0
        assert r["dispatch"]["levels"] == one["dispatch"]["levels"] and r["dispatch"]["cycle_elem"] == 4
        assert len(r["pressure_iterations"]) == len(one["pressure_iterations"]) == 8       # 2 steps x 2 corrector solves, forward and adjoint
        assert all(abs(a - b) <= 1 for a, b in zip(r["pressure_iterations"], one["pressure_iterations"])), (r["pressure_iterations"], one["pressure_iterations"])
        assert max(r["pressure_iterations"]) < 200
        assert r["stats"]["verification_failures"] == 0 and r["stats"]["persistent_fallbacks"] == 0
    assert two[0]["pressure_iterations"] == two[1]["pressure_iterations"]
    loss = sum(r["loss"] for r in two)
    grad = sum(r["grad_sq"] for r in two) ** 0.5
    assert abs(loss - one["loss"]) <= 1e-5 * abs(one["loss"]), (loss, one["loss"])
    assert abs(grad - one["grad_sq"] ** 0.5) <= 1e-5 * one["grad_sq"] ** 0.5, (grad, one["grad_sq"] ** 0.5)
