"""Multigrid-preconditioned pressure CG - with the fp64 cycle and with the float32 cycle (cycle_dtype=torch.float32) - against the plain
CG: iterations and time per solve at 1e-5 / 1e-10 on periodic and walled systems of four sizes, one whole bench-workload step (forward +
adjoint at the converged 2048^2 fixture's tolerances) with each solver, and a float32-cycle iteration at 2048^2 with the four-cell
kernels against the one-cell kernels (option mg_f32_vec).  Warmed up, medians of interleaved repeats, every timing ends in a device
synchronise.  Every result is one JSON line.  Needs a GPU.

    python scripts/bench_mg.py [--reps 5] [--no-step] [--no-solves] [--no-plain] [--no-vec] [--sizes 256x256,1024x256,...]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-piso_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def solves(sizes, reps, plain=True):
    from diffpiso.solvers import cg_solve_native, mg_solve_native, mg_vcycle_native
    from tests.cases import pressure_system
    rows = []
    for nx, ny in sizes:
        for walls in (False, True):
            L, b = pressure_system(nx, ny, walls=walls)
            per = not walls
            for tol in (1e-5, 1e-10):
                run = {"multigrid": lambda: mg_solve_native(nx, ny, per, per, L, b, tol, 500, True, 1000),
                       "multigrid_f32": lambda: mg_solve_native(nx, ny, per, per, L, b, tol, 500, True, 1000, cycle_dtype=torch.float32)}
                if plain:
                    run["plain"] = lambda: cg_solve_native(nx, ny, per, per, L, b, tol, 200000, True, 1000)
                ms, its = {k: [] for k in run}, {}
                for k in run:
                    run[k]()                                   # warm-up
                for _ in range(reps):                          # interleaved
                    for k in run:
                        t, (x, it) = timed(run[k])
                        ms[k].append(t); its[k] = int(it)
                row = dict(nx=nx, ny=ny, walls=walls, tol=tol, mg_iterations=its["multigrid"], mg_ms=statistics.median(ms["multigrid"]),
                           mg_ms_spread=(min(ms["multigrid"]), max(ms["multigrid"])),
                           mg32_iterations=its["multigrid_f32"], mg32_ms=statistics.median(ms["multigrid_f32"]),
                           mg32_ms_spread=(min(ms["multigrid_f32"]), max(ms["multigrid_f32"])))
                if plain:
                    row.update(plain_iterations=its["plain"], plain_ms=statistics.median(ms["plain"]), plain_ms_spread=(min(ms["plain"]), max(ms["plain"])))
                row["mg_us_per_iteration_incl_setup"] = 1e3 * row["mg_ms"] / max(its["multigrid"], 1)
                row["mg32_us_per_iteration_incl_setup"] = 1e3 * row["mg32_ms"] / max(its["multigrid_f32"], 1)
                row["fp64_ms_over_f32_cycle_ms"] = row["mg_ms"] / row["mg32_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            # one cycle through the test entry (rebuilds the hierarchy in every call: an upper bound on a cycle)
            r = torch.randn_like(b)
            mg_vcycle_native(nx, ny, per, per, L, r)
            t = [timed(lambda: mg_vcycle_native(nx, ny, per, per, L, r))[0] for _ in range(reps)]
            t32 = [timed(lambda: mg_vcycle_native(nx, ny, per, per, L, r, cycle_dtype=torch.float32))[0] for _ in range(reps + 1)][1:]
            print(json.dumps(dict(nx=nx, ny=ny, walls=walls, vcycle_entry_ms_incl_hierarchy_build=statistics.median(t),
                                  vcycle_f32_entry_ms_incl_hierarchy_build=statistics.median(t32))), flush=True)
    return rows


def vec(reps, n=2048):
    """A float32-cycle iteration at n^2 with the four-cell kernels (mg_f32_vec 1) against the one-cell kernels (0): what the 16-byte
    accesses are worth.  Per iteration = (solve of 40 iterations - solve of 8) / 32 at a tolerance no solve reaches: the set-up drops out."""
    import diffpiso._native as N
    from diffpiso.solvers import mg_solve_native
    from tests.cases import pressure_system
    L, b = pressure_system(n, n)
    saved = N.get_option("mg_f32_vec")
    kinds = {"fp64_cycle": (torch.float64, 1), "f32_cycle_vec1": (torch.float32, 1), "f32_cycle_vec0": (torch.float32, 0)}
    ms = {k: {8: [], 40: []} for k in kinds}
    try:
        for rep in range(reps + 1):
            for k, (dt, v) in kinds.items():
                N.set_option("mg_f32_vec", v)
                for its in (8, 40):
                    t, _ = timed(lambda: mg_solve_native(n, n, True, True, L, b, 1e-30, its, True, 1000, cycle_dtype=dt))
                    if rep:
                        ms[k][its].append(t)
    finally:
        N.set_option("mg_f32_vec", saved)
    out = dict(workload="pcg iteration %dx%d periodic" % (n, n))
    for k in kinds:
        out[k + "_us_per_iteration"] = 1e3 * (statistics.median(ms[k][40]) - statistics.median(ms[k][8])) / 32
    print(json.dumps(out), flush=True)


def step(reps):
    """One bench-workload step at 2048^2, forward + adjoint, at the tolerances of tests/golden/bench2048_tight_step.npz."""
    import bench
    import diffpiso as dp
    meta = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "bench2048_tight_step.npz"))["meta"]))
    sv, n = meta["solver"], meta["grid"]
    out = {}
    P = bench.build_problem(n, torch.device("cuda"), sv["p_tol"], sv["p_max_it"], sv["p_reset"])
    P["lin"].accuracy, P["lin"].max_iterations = sv["lin_tol"], sv["lin_max_it"]
    solvers = {"plain": P["ps"], "multigrid": dp.PisoPressureSolverMultigrid(dx=[], accuracy=sv["p_tol"], max_iterations=200, residual_reset=sv["p_reset"]),
               "multigrid_f32": dp.PisoPressureSolverMultigrid(dx=[], accuracy=sv["p_tol"], max_iterations=200, residual_reset=sv["p_reset"],
                                                               cycle_dtype=torch.float32)}

    def one(ps):
        P["sim"].pressure_solver = ps
        ps.accuracy = sv["p_tol"]
        ps.stats.update(solves=0, iterations=0, adjoint_solves=0, adjoint_iterations=0)
        vel_t = P["vel_t"].clone().requires_grad_(True)
        p_t = P["p_t"].clone().requires_grad_(True)
        velocity = dp.StaggeredGrid(vel_t, P["domain"].box, extrapolation=dp.Material.extrapolation_mode(P["domain"].boundaries))
        pressure = dp.CenteredGrid(p_t, P["domain"].box, dp.pressure_extrapolation(P["domain"].boundaries))
        va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, P["dt"], P["sim"], step_count=1)
        ps.accuracy = sv.get("p_tol_adjoint", sv["p_tol"])
        (0.5 * (vn.staggered_tensor() ** 2).sum()).backward()
        return ps.stats["iterations"] + ps.stats["adjoint_iterations"]

    ms = {k: [] for k in solvers}
    for k, ps in solvers.items():
        one(ps)
    for _ in range(reps):
        for k, ps in solvers.items():
            t, its = timed(lambda: one(ps))
            ms[k].append(t); out[k + "_pressure_iterations"] = its
    for k in solvers:
        out[k + "_step_ms"] = statistics.median(ms[k]); out[k + "_step_ms_spread"] = (min(ms[k]), max(ms[k]))
    out.update(workload="bench 2048^2 step fwd + adjoint", p_tol=sv["p_tol"], p_tol_adjoint=sv.get("p_tol_adjoint", sv["p_tol"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--no-plain", action="store_true", help="solves: leave the plain CG out (it takes most of the time)")
    ap.add_argument("--no-vec", action="store_true")
    ap.add_argument("--sizes", default="256x256,1024x256,1024x1024,2048x2048")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mg.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps)), flush=True)
    if not a.no_solves:
        solves([tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")], a.reps, plain=not a.no_plain)
    if not a.no_vec:
        vec(a.reps)
    if not a.no_step:
        step(max(3, a.reps // 2 + 1))
