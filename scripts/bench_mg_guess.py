"""What starting the multigrid pressure solves from the previous step's increments (PisoPressureSolverMultigrid(use_guess=True), csrc/mg_guess.h)
is worth.  Forward-only runs of `--warmup` + `--steps` PISO steps from the workload's initial state (default 5 + 20: the first steps are the
start-up transient, in which the guard rejects the guesses; they are stepped but not timed), with the option off and on, interleaved
repeats, medians and (min - max); every timing ends in a device synchronise.  Workloads: the bench workload (decaying turbulence, doubly
periodic) at 2048^2 and 1024^2 and the config-4 shape 1024 x 256 (spatially evolving mixing layer, open borders), p_tol 1e-5 and 1e-8, both
precisions of the cycle; the momentum solver runs at 1e-5 throughout.  Per row: pressure iterations per step (timed steps), accepted /
rejected guesses (all steps) and ms per step.  Every result is one JSON line; a table follows.  Needs a GPU.

    python scripts/bench_mg_guess.py [--reps 3] [--steps 20] [--warmup 5] [--workloads bench2048,bench1024,cfg4] [--tols 1e-5,1e-8]
                                     [--tree PATH]
--tree PATH measures another checkout of the project (its package and its library) with the option off only: the off path against the
parent commit built from its own sources."""
import argparse
import json
import os
import statistics
import sys
import time

a = argparse.ArgumentParser()
a.add_argument("--reps", type=int, default=3)
a.add_argument("--steps", type=int, default=20)
a.add_argument("--warmup", type=int, default=5)
a.add_argument("--workloads", default="bench2048,bench1024,cfg4")
a.add_argument("--tols", default="1e-5,1e-8")
a.add_argument("--tree", default=None)
ARGS = a.parse_args()

ROOT = os.path.abspath(ARGS.tree) if ARGS.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-piso_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

LIN_TOL = 1e-5


def problem(name):
    """-> (label, sim, velocity, pressure, dt)"""
    import diffpiso as dp
    if name.startswith("bench"):
        import bench
        n = int(name[5:])
        P = bench.build_problem(n, torch.device("cuda"), LIN_TOL, 2000, 10)
        velocity = dp.StaggeredGrid(P["vel_t"], P["domain"].box, extrapolation=dp.Material.extrapolation_mode(P["domain"].boundaries))
        pressure = dp.CenteredGrid(P["p_t"], P["domain"].box, dp.pressure_extrapolation(P["domain"].boundaries))
        return "bench %d^2" % n, P["sim"], velocity, pressure, P["dt"]
    from tests.cases import product_setup, sml_case
    c = sml_case()
    Q = product_setup(c, lin_tol=LIN_TOL, p_tol=LIN_TOL)
    return "config 4 1024 x 256", Q["sim"], Q["velocity"], Q["pressure"], c["dt"]


def run(sim, velocity, pressure, dt, ps, use_guess):
    """-> (ms per timed step, pressure iterations per timed step, stats of all steps)"""
    import diffpiso as dp
    sim.pressure_solver = ps
    for k in ps.stats:
        ps.stats[k] = 0
    inc1 = dp.CenteredGrid(torch.full_like(pressure.data, 5e-13), pressure.box, pressure.extrapolation)
    inc2 = dp.CenteredGrid(torch.full_like(pressure.data, 1e-12), pressure.box, pressure.extrapolation)
    vel, p, carry = velocity, pressure, []
    with torch.no_grad():
        for i in range(ARGS.warmup + ARGS.steps):
            if i == ARGS.warmup:
                torch.cuda.synchronize()
                it0, t0 = ps.stats["iterations"], time.perf_counter()
            if use_guess:
                vel, p, _ = dp.piso_step(vel, p, inc1, inc2, dt, sim, sim.dirichlet_values, unrolling_step=i, increments_out=carry)
                inc1, inc2 = carry
            else:
                vel, p, _ = dp.piso_step(vel, p, inc1, inc2, dt, sim, sim.dirichlet_values, unrolling_step=i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / ARGS.steps
    assert bool(torch.isfinite(p.data).all())
    return ms, (ps.stats["iterations"] - it0) / ARGS.steps, dict(ps.stats)


def main():
    import diffpiso as dp
    if not torch.cuda.is_available():
        sys.exit("bench_mg_guess.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=ARGS.reps, steps=ARGS.steps, warmup=ARGS.warmup, lin_tol=LIN_TOL,
                          tree="another checkout, option off only" if ARGS.tree else "this checkout")), flush=True)
    modes = (False,) if ARGS.tree else (False, True)
    rows = []
    for name in ARGS.workloads.split(","):
        label, sim, velocity, pressure, dt = problem(name)
        for tol in (float(t) for t in ARGS.tols.split(",")):
            for dtype, cyc in ((torch.float64, "fp64"), (torch.float32, "f32")):
                make = lambda g: dp.PisoPressureSolverMultigrid(dx=[], accuracy=tol, max_iterations=200, residual_reset=10, cycle_dtype=dtype,
                                                                **({"use_guess": True} if g else {}))
                ms, its, stats = {g: [] for g in modes}, {}, {}
                run(sim, velocity, pressure, dt, make(False), False)                   # warm-up of the process and the allocator
                for _ in range(ARGS.reps):                                              # interleaved
                    for g in modes:
                        t, its[g], stats[g] = run(sim, velocity, pressure, dt, make(g), g)
                        ms[g].append(t)
                row = dict(workload=label, p_tol=tol, cycle=cyc)
                for g in modes:
                    k = "on" if g else "off"
                    row[k + "_ms_per_step"] = statistics.median(ms[g])
                    row[k + "_spread"] = (min(ms[g]), max(ms[g]))
                    row[k + "_pressure_iterations_per_step"] = its[g]
                if True in modes:
                    row["accepted"], row["rejected"] = stats[True]["guesses_accepted"], stats[True]["guesses_rejected"]
                    off, on = row["off_ms_per_step"], row["on_ms_per_step"]
                    spread = max(max(ms[g]) - min(ms[g]) for g in modes)
                    row.update(gain_ms=off - on, gain_percent=100 * (off - on) / off, within_spread=bool(abs(off - on) <= spread))
                rows.append(row)
                print(json.dumps(row), flush=True)
    print()
    if True in modes:
        print("| workload | p_tol | cycle | iterations / step off -> on | accepted / rejected | ms / step off (min - max) | ms / step on (min - max) | gain |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %.0e | %s | %.2f -> %.2f | %d / %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %+.1f %%%s |"
                  % (r["workload"], r["p_tol"], r["cycle"], r["off_pressure_iterations_per_step"], r["on_pressure_iterations_per_step"], r["accepted"],
                     r["rejected"], r["off_ms_per_step"], r["off_spread"][0], r["off_spread"][1], r["on_ms_per_step"], r["on_spread"][0],
                     r["on_spread"][1], r["gain_percent"], " (within the spread)" if r["within_spread"] else ""))
    else:
        print("| workload | p_tol | cycle | iterations / step | ms / step off (min - max) |")
        print("|---|---|---|---|---|")
        for r in rows:
            print("| %s | %.0e | %s | %.2f | %.2f (%.2f - %.2f) |" % (r["workload"], r["p_tol"], r["cycle"], r["off_pressure_iterations_per_step"],
                                                                     r["off_ms_per_step"], r["off_spread"][0], r["off_spread"][1]))


if __name__ == "__main__":
    main()
