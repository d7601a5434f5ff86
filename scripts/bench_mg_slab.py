"""The slab multigrid before any link: median ms per solve of (a) the one-GPU multigrid, (b) the slab multigrid through a peer communicator
of ONE rank (halo rows through the rank's own mailbox, the collapse kernels, the gather of level g as a copy), (c) the same slab multigrid
with the float32 cycle (cycle_dtype=torch.float32: float halo rows and gather, the fp64 outer iteration) and (d) the plain slab CG
through the same communicator, at 1e-5 and 1e-10 on 1024 x 256 walls, 1024^2 and 2048^2 (periodic and walls).  (b) / (a) is what the halo
rows, the collectives' kernels and the gather cost on one GPU, (c) / (b) what the float32 cycle is worth on slabs (a plan with g = 0 has no
column (c): the float32 cycle is refused there); the collectives per iteration (from the plan) are what a real node multiplies
by its hop.  Warmed up, medians of interleaved repeats, every timing ends in a device synchronise.  Needs a GPU.

    python scripts/bench_mg_slab.py [--reps 5] [--sizes 1024x256w,1024x1024,1024x1024w,2048x2048,2048x2048w]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-piso_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PLAIN_CAP = 200000


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024x256w,1024x1024,1024x1024w,2048x2048,2048x2048w")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mg_slab.py needs a GPU")
    import diffpiso._native as N
    from diffpiso.distributed import SlabCommunicator, cg_solve_slab, mg_solve_slab_local
    from diffpiso.solvers import mg_solve_native
    from tests.cases import pressure_system
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps)), flush=True)
    comm = SlabCommunicator(rank=0, world=1, transport="peer", row_capacity=8192)
    try:
        for size in a.sizes.split(","):
            walls = size.endswith("w")
            nx, ny = (int(v) for v in size.rstrip("w").split("x"))
            L, b = pressure_system(nx, ny, walls=walls)
            per = not walls
            plan = N.mg_slab_plan(nx, ny, 1)
            # what one iteration issues at two sweeps (csrc/mg_slab_plan.h: mg_slab_collectives)
            g = plan["g"]
            coll = dict(exchanges=0 if g == 0 else 3 * g + (g - 1) + 1, allreduces=2, allgathers=2)
            for tol in (1e-5, 1e-10):
                run = {"mg_one_gpu": lambda: mg_solve_native(nx, ny, per, per, L, b, tol, 500, True, 1000),
                       "mg_slab_ring_of_one": lambda: mg_solve_slab_local(comm, nx, ny, per, per, L.reshape(-1), b, tol, 500, True, 1000),
                       "mg_slab_f32_ring_of_one": lambda: mg_solve_slab_local(comm, nx, ny, per, per, L.reshape(-1), b, tol, 500, True, 1000,
                                                                              cycle_dtype=torch.float32),
                       "plain_slab_ring_of_one": lambda: cg_solve_slab(comm, nx, ny, per, per, L.reshape(-1), b, tol, PLAIN_CAP, True, 1000, gather=False)}
                if g == 0:
                    del run["mg_slab_f32_ring_of_one"]
                ms, its = {k: [] for k in run}, {}
                for k in run:
                    run[k]()                                   # warm-up
                for _ in range(a.reps):                        # interleaved
                    for k in run:
                        t, (x, it) = timed(run[k])
                        ms[k].append(t); its[k] = int(it)
                row = dict(nx=nx, ny=ny, walls=walls, tol=tol, g=g, levels=len(plan["levels"]), collectives_per_iteration=coll, iterations=its,
                           ms={k: statistics.median(v) for k, v in ms.items()}, ms_spread={k: (min(v), max(v)) for k, v in ms.items()},
                           plain_hit_cap=its["plain_slab_ring_of_one"] >= PLAIN_CAP)
                row["slab_over_one_gpu"] = row["ms"]["mg_slab_ring_of_one"] / row["ms"]["mg_one_gpu"]
                if g > 0:
                    row["slab_f32_over_slab_f64"] = row["ms"]["mg_slab_f32_ring_of_one"] / row["ms"]["mg_slab_ring_of_one"]
                row["slab_mg_faster_than_plain_slab"] = row["ms"]["mg_slab_ring_of_one"] < row["ms"]["plain_slab_ring_of_one"]
                print(json.dumps(row), flush=True)
    finally:
        comm.close()


if __name__ == "__main__":
    main()
