"""One rank of the slab multigrid with the float32 cycle over real PROCESSES that share the one GPU (started by
tests/test_gpu_mg_slab_f32_multiproc.py; tests/mg_slab_worker.py is its fp64 twin):

    python tests/mg_slab_f32_worker.py RANK WORLD PORT solver NX NY KNOB BORDER
    python tests/mg_slab_f32_worker.py RANK WORLD PORT step NX NY STEPS

`solver`: every rank builds the same pressure system (tests/cases.laplace_case), computes the ONE-GPU float32 cycle and solve in its own
process and compares ITS rows of the slab results with cycle_dtype=torch.float32 (peer communicator, mailboxes mapped across the processes)
with them: V-cycles bit for bit, the converged counts and difference, the dispatch record, the communicator's stats, and the all-gather of
floats with a payload per rank.
`step`: the sharded step (tests/sharded_worker.py builds and runs it) on an NX x NY periodic box with
PisoPressureSolverMultigrid(cycle_dtype=torch.float32) and converged solves; WORLD 1 is the same box on one GPU with the same solver."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "differentiable-piso_amd"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
BIG = 1 << 30


def solver_checks(comm, nx, ny, knob, border, out):
    import numpy as np
    import torch
    import diffpiso._native as N
    from diffpiso.distributed import comm_allgather, mg_solve_slab_local, mg_vcycle_slab_local, slab_rows
    from diffpiso.solvers import mg_solve_native, mg_vcycle_native
    from tests.cases import laplace_case
    F32 = torch.float32
    if knob > 0:
        N.set_option("mg_slab_gather_cells", knob)
    s, L, b = laplace_case(border, ny, nx, 3)
    per_y, per_x = (bool(v) for v in s.periodic_yx)
    rd = bool(s.rank_deficient)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")
    Ld, bd = dev(np.asarray(L, np.float64).reshape(-1, 5)), dev(b)
    r = dev(np.random.default_rng(7).standard_normal(nx * ny))
    j0, j1 = slab_rows(comm.rank, comm.world, ny)
    nyl, lo, hi = j1 - j0, j0 * nx, j1 * nx
    L_loc, b_loc, r_loc = Ld[lo:hi].contiguous(), bd[lo:hi].contiguous(), r[lo:hi].contiguous()
    out["plan"] = N.mg_slab_plan(nx, ny, comm.world)
    out["vcycle_equal"], out["dispatch"] = [], []
    for sweeps in (1, 2, 3):
        want = mg_vcycle_native(nx, ny, per_x, per_y, Ld, r, sweeps, cycle_dtype=F32)
        got = mg_vcycle_slab_local(comm, nx, nyl, per_x, per_y, L_loc, r_loc, sweeps, cycle_dtype=F32)
        out["dispatch"].append(N.mg_last_dispatch())
        out["vcycle_equal"].append(bool(torch.equal(got, want[lo:hi])))
    want, itw = mg_solve_native(nx, ny, per_x, per_y, Ld, bd, 1e-10, 400, rd, BIG, cycle_dtype=F32)
    got, it = mg_solve_slab_local(comm, nx, nyl, per_x, per_y, L_loc, b_loc, 1e-10, 400, rd, BIG, cycle_dtype=F32)
    out["converged_its"] = [int(it), int(itw)]
    out["converged_diff"] = float((got - want[lo:hi]).abs().max() / want.abs().max())
    # the all-gather of floats with a payload of its own per rank (a NaN payload and -0.0 among them), three in a row
    ok = True
    for k, count in enumerate((1, 37, 8192 // comm.world)):
        def payload(rank):
            v = torch.arange(count, dtype=F32) * (rank + 1) + 1000.0 * k
            bits = v.view(torch.int32).clone()
            bits[0] = 0x7FC00000 + rank + 1                        # a NaN whose payload names the rank
            if count > 1:
                bits[1] = -(1 << 31)                               # -0.0
            return bits
        got = comm_allgather(comm, payload(comm.rank).view(F32).cuda())
        want = torch.cat([payload(q) for q in range(comm.world)])
        ok = ok and bool(torch.equal(got.view(torch.int32).cpu(), want))
    out["allgather_ok"] = ok
    out["stats"] = comm.stats()


def step_run(comm, world, rank, nx, ny, steps, device, out):
    import torch
    import diffpiso as dp
    import sharded_worker as W
    B = W.build_case("box:%d:%d:%d:1e-10:200:1" % (nx, ny, steps), torch.device("cpu") if world > 1 else device)
    ps = dp.PisoPressureSolverMultigrid(dx=[], accuracy=1e-10, max_iterations=200, residual_reset=1000, cycle_dtype=torch.float32)
    B["ps"] = B["sim"].pressure_solver = ps
    counts, inner = [], ps._cg

    def spy(*a):
        x, it = inner(*a)
        counts.append(int(it))
        return x, it
    ps._cg = spy
    sh = None
    if world > 1:
        from diffpiso.sharding import StepSharding
        ps.slab_comm = comm
        B["lin"].slab_comm = comm
        sh = B["sim"].sharding = StepSharding(comm, nx, ny)
    u, p, du, dp_, loss, warn = W.run_case(B, sh)
    if sh is not None:
        sh.check()
        out["stats"] = comm.stats()
    g2 = float(sh.owned_sum_of_squares(du)) if sh is not None else float((du.double() ** 2).sum())
    out.update(loss=loss, warn=warn, grad_sq=g2, pressure_iterations=counts, non_finite=[int((~torch.isfinite(t)).sum()) for t in (u, p, du, dp_)],
               dispatch=dp.PisoPressureSolverMultigrid.last_dispatch())


def main():
    rank, world, port = (int(v) for v in sys.argv[1:4])
    mode, args = sys.argv[4], sys.argv[5:]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    out = {"rank": rank, "world": world, "ok": False}
    comm = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        if world > 1:
            from diffpiso.distributed import SlabCommunicator
            nx = int(args[0])
            comm = SlabCommunicator(rank=rank, world=world, device=device, transport="peer", row_capacity=26 * nx + 64)
        if mode == "solver":
            solver_checks(comm, int(args[0]), int(args[1]), int(args[2]), args[3], out)
        else:
            step_run(comm, world, rank, int(args[0]), int(args[1]), int(args[2]), device, out)
        out["ok"] = True
    except Exception as e:        # the parent reads the reason
        import traceback
        out["error"] = "%r\n%s" % (e, traceback.format_exc()[-1500:])
    finally:
        print("SLAB_WORKER " + json.dumps(out), flush=True)
        try:
            if comm is not None:
                comm.close()
        except Exception:
            pass
        try:
            if world > 1:
                dist.destroy_process_group()
        except Exception:
            pass


if __name__ == "__main__":
    main()
