"""What a prepared multigrid hierarchy (csrc/mg_prepared.h, PisoPressureSolverMultigrid(reuse_hierarchy=True)) is worth.
Solve rows - per size, at 1e-5, in both precisions of the cycle: (a) the ordinary solve (set-up and its host look inside), (b) prepare alone,
(c) a solve on the prepared hierarchy; x and the count of (c) are checked against (a) bit for bit.  Step rows: the 2048^2 bench step, forward +
adjoint at the converged fixture's tolerances, and the 512^2 16-step unroll, each with reuse off and on.  Warmed up, medians and (min, max) of
interleaved repeats, every timing ends in a device synchronise.  Every result is one JSON line.  Needs a GPU.

    python scripts/bench_mg_reuse.py [--reps 7] [--no-solves] [--no-step] [--no-unroll] [--sizes 256x256,1024x256w,1024x1024,2048x2048]
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


def med(v):
    return dict(ms=statistics.median(v), spread=(min(v), max(v)))


def solves(sizes, reps, tol=1e-5):
    from diffpiso.solvers import MgHierarchy, mg_solve_native, mg_solve_prepared_native
    from tests.cases import pressure_system
    for nx, ny, walls in sizes:
        L, b = pressure_system(nx, ny, walls=walls)
        per = not walls
        for dtype, label in ((torch.float64, "fp64"), (torch.float32, "f32")):
            h = MgHierarchy(nx, ny, per, per, True, dtype, L.device)
            run = {"a_ordinary": lambda: mg_solve_native(nx, ny, per, per, L, b, tol, 500, True, 1000, cycle_dtype=dtype),
                   "b_prepare": lambda: h.prepare(L),
                   "c_prepared": lambda: mg_solve_prepared_native(h, b, tol, 500, 1000)}
            ms = {k: [] for k in run}
            for k in run:
                run[k]()                                       # warm-up (b before c)
            for _ in range(reps):                              # interleaved
                for k in run:
                    t, out = timed(run[k])
                    ms[k].append(t)
            (xa, ita), (xc, itc) = run["a_ordinary"](), run["c_prepared"]()
            assert int(ita) == int(itc) and torch.equal(xa, xc), "a prepared solve differs from the ordinary one"
            row = dict(nx=nx, ny=ny, walls=walls, tol=tol, cycle=label, iterations=int(ita))
            for k in run:
                row[k] = med(ms[k])
            a, bb, c = (row[k]["ms"] for k in ("a_ordinary", "b_prepare", "c_prepared"))
            spread = max(row[k]["spread"][1] - row[k]["spread"][0] for k in run)
            row.update(gain_ms=a - c, gain_percent=100 * (a - c) / a, b_plus_c_minus_a_ms=bb + c - a, largest_spread_ms=spread,
                       c_within_a=bool(c <= a + spread), within_noise=bool(abs(a - c) <= spread))
            print(json.dumps(row), flush=True)


def _fixture(name):
    return json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", name))["meta"]))


def steps(reps, fixture, step_count, what):
    """`step_count` bench-workload steps, forward + adjoint, at the tolerances of the converged fixture, with reuse off and on."""
    import bench
    import diffpiso as dp
    meta = _fixture(fixture)
    sv, n = meta["solver"], meta["grid"]
    P = bench.build_problem(n, torch.device("cuda"), sv["p_tol"], sv["p_max_it"], sv["p_reset"])
    P["lin"].accuracy, P["lin"].max_iterations = sv["lin_tol"], sv["lin_max_it"]
    make = lambda dtype, reuse: dp.PisoPressureSolverMultigrid(dx=[], accuracy=sv["p_tol"], max_iterations=200, residual_reset=sv["p_reset"], cycle_dtype=dtype,
                                                               reuse_hierarchy=reuse)
    solvers = {"%s_reuse_%s" % (label, "on" if reuse else "off"): make(dtype, reuse)
               for dtype, label in ((torch.float64, "fp64"), (torch.float32, "f32")) for reuse in (False, True)}

    def one(ps):
        P["sim"].pressure_solver = ps
        ps.accuracy = sv["p_tol"]
        for k in ps.stats:
            ps.stats[k] = 0
        vel_t = P["vel_t"].clone().requires_grad_(True)
        p_t = P["p_t"].clone().requires_grad_(True)
        velocity = dp.StaggeredGrid(vel_t, P["domain"].box, extrapolation=dp.Material.extrapolation_mode(P["domain"].boundaries))
        pressure = dp.CenteredGrid(p_t, P["domain"].box, dp.pressure_extrapolation(P["domain"].boundaries))
        va, pa, vn, pn, warn = dp.unroll_piso_steps(velocity, pressure, P["dt"], P["sim"], step_count=step_count)
        ps.accuracy = sv.get("p_tol_adjoint", sv["p_tol"])
        (0.5 * (vn.staggered_tensor() ** 2).sum()).backward()
        return dict(ps.stats), vel_t.grad

    ms, stats, grads = {k: [] for k in solvers}, {}, {}
    for k, ps in solvers.items():
        one(ps)
    for _ in range(reps):
        for k, ps in solvers.items():
            t, (stats[k], grads[k]) = timed(lambda: one(ps))
            ms[k].append(t)
    out = dict(workload=what, p_tol=sv["p_tol"], p_tol_adjoint=sv.get("p_tol_adjoint", sv["p_tol"]))
    for label in ("fp64", "f32"):
        off, on = label + "_reuse_off", label + "_reuse_on"
        assert torch.equal(grads[off], grads[on]), "reuse changes the gradient"
        assert all(stats[off][k] == stats[on][k] for k in ("iterations", "adjoint_iterations"))
        out[off], out[on] = med(ms[off]), med(ms[on])
        spread = max(out[k]["spread"][1] - out[k]["spread"][0] for k in (off, on))
        out[label + "_gain_ms"] = out[off]["ms"] - out[on]["ms"]
        out[label + "_gain_percent"] = 100 * (out[off]["ms"] - out[on]["ms"]) / out[off]["ms"]
        out[label + "_within_noise"] = bool(abs(out[off]["ms"] - out[on]["ms"]) <= spread)
        out[label + "_builds_off_on"] = (stats[off]["hierarchy_builds"], stats[on]["hierarchy_builds"])
        out[label + "_laplace_builds_off_on"] = (stats[off]["laplace_builds"], stats[on]["laplace_builds"])
        out[label + "_pressure_iterations"] = stats[on]["iterations"] + stats[on]["adjoint_iterations"]
    print(json.dumps(out), flush=True)


def parse_sizes(text):
    out = []
    for s in text.split(","):
        walls = s.endswith("w")
        nx, ny = (int(v) for v in s.rstrip("w").split("x"))
        out.append((nx, ny, walls))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-unroll", action="store_true")
    ap.add_argument("--sizes", default="256x256,1024x256w,1024x1024,2048x2048", help="nx x ny, a trailing w: walls in both directions")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mg_reuse.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps)), flush=True)
    if not a.no_solves:
        solves(parse_sizes(a.sizes), a.reps)
    if not a.no_step:
        steps(max(3, a.reps // 2 + 1), "bench2048_tight_step.npz", 1, "bench 2048^2 step fwd + adjoint")
    if not a.no_unroll:
        steps(max(3, a.reps // 2 + 1), "bench512_tight_unroll16.npz", 16, "bench 512^2 16-step unroll fwd + adjoint")
