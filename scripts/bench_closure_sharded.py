"""What the CNN closure on y-slabs costs on ONE GPU, at config 4's size 1024 x 256 (nx x ny).  It REPORTS; nothing is asserted.
    (a) the four coupling kernels of csrc/closure_glue.hip (whole-grid entries) against the torch ops they restate (closure.network_input,
        closure.centered_to_staggered and their autograd adjoints);
    (b) the network (the reference's seven layers, forward and forward + backward) on the extended rows of one rank, nyl + 2 E rows with
        E = R + 1 = 10, against 1 / N of the whole-grid network, for N = 2, 4, 8: the 2 E rows of redundant convolution work per rank.
NO LINK IS TIMED by any of this: the wide halo exchange (two per step and direction) needs more than one rank and is not part of these numbers.
Warmed up, medians of alternated repeats in one process, every timing ends in a device synchronise.  Every result is one JSON line (also
appended to --out, default profiles/closure_sharded_bench.txt).  Needs a GPU.

    python scripts/bench_closure_sharded.py [--reps 20] [--out FILE]
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

NX, NY = 1024, 256


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternated(cases, reps):
    """{name: fn} -> {name: median ms}, the cases taking turns"""
    for fn in cases.values():
        fn()
        fn()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ms.items()}


def part_a(emit, reps):
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso.stencils import flatten_staggered_data
    lib, s = N.lib, N.stream_ptr()
    gen = torch.Generator().manual_seed(0)
    box = dp.box[0:float(NY), 0:float(NX)]
    vel = torch.randn(1, NY + 1, NX + 1, 2, generator=gen).cuda().requires_grad_(True)
    p = torch.randn(1, NY, NX, 1, generator=gen).cuda().requires_grad_(True)
    p_ext = (("boundary", "boundary"), ("boundary", "constant"))
    modes = (C.c_int * 4)(1, 0, 1, 1)
    faces = flatten_staggered_data(vel.detach(), coord_flip=True).contiguous()
    nn_in = torch.empty(1, NY, NX, 4, device="cuda")
    g_in = torch.randn(1, NY, NX, 4, generator=gen).cuda()
    d_faces, d_p = torch.empty_like(faces), torch.empty(NY * NX, device="cuda")
    nn_out = torch.randn(1, NY, NX, 2, generator=gen).cuda().requires_grad_(True)
    g_faces_st = torch.randn(1, NY + 1, NX + 1, 2, generator=gen).cuda()
    g_faces = flatten_staggered_data(g_faces_st, coord_flip=True).contiguous()
    forcing, d_out = torch.empty_like(faces), torch.empty(1, NY, NX, 2, device="cuda")
    two_dx = C.c_double(2.0)

    def torch_input():
        return dp.network_input(dp.StaggeredGrid(vel, box), dp.CenteredGrid(p, box, extrapolation=p_ext), True)

    def torch_force():
        return dp.centered_to_staggered(nn_out)
    y_in, y_force = torch_input(), torch_force()
    cases = {
        "input kernel": lambda: N.check(lib.piso_closure_input(N.ptr(faces), N.ptr(p.detach()), N.ptr(nn_in), NX, NY, 4, modes, two_dx, s), "input"),
        "input torch": torch_input,
        "input adjoint kernel": lambda: N.check(lib.piso_closure_input_adjoint(N.ptr(g_in), N.ptr(d_faces), N.ptr(d_p), NX, NY, 4, modes, two_dx, s), "input adjoint"),
        "input adjoint torch": lambda: torch.autograd.grad(y_in, (vel, p), g_in, retain_graph=True),
        "force kernel": lambda: N.check(lib.piso_closure_force(N.ptr(nn_out.detach()), N.ptr(forcing), NX, NY, 0, 0, s), "force"),
        "force torch": torch_force,
        "force adjoint kernel": lambda: N.check(lib.piso_closure_force_adjoint(N.ptr(g_faces), N.ptr(d_out), NX, NY, 0, 0, s), "force adjoint"),
        "force adjoint torch": lambda: torch.autograd.grad(y_force, (nn_out,), g_faces_st, retain_graph=True),
    }
    ms = alternated(cases, reps)
    for what in ("input", "input adjoint", "force", "force adjoint"):
        k, t = ms[what + " kernel"], ms[what + " torch"]
        emit({"part": "a", "what": what, "grid": "%dx%d" % (NX, NY), "kernel_ms": round(k, 4), "torch_ops_ms": round(t, 4), "ratio": round(k / t, 3)})


def part_b(emit, reps):
    import diffpiso as dp
    net = dp.FullyConvNetwork(seed=1).cuda()
    E = net.reduced_buffer_width + 1
    gen = torch.Generator().manual_seed(1)

    def passes(rows):
        x = torch.randn(1, rows, NX, 4, generator=gen).cuda().requires_grad_(True)
        g = torch.randn(1, rows, NX, 2, generator=gen).cuda()

        def fwd():
            with torch.no_grad():
                net(x)

        def both():
            net.zero_grad()
            x.grad = None
            net(x).backward(g)
        return fwd, both
    cases = {}
    for tag, rows in [("whole", NY)] + [("N%d" % n, NY // n + 2 * E) for n in (2, 4, 8)]:
        cases[tag + " forward"], cases[tag + " forward+backward"] = passes(rows)
    ms = alternated(cases, reps)
    for n in (2, 4, 8):
        for what in ("forward", "forward+backward"):
            whole, mine = ms["whole " + what], ms["N%d %s" % (n, what)]
            emit({"part": "b", "what": what, "ranks": n, "rows_per_rank": NY // n + 2 * E, "redundant_rows": 2 * E, "rank_ms": round(mine, 4),
                  "whole_grid_ms": round(whole, 4), "whole_over_N_ms": round(whole / n, 4), "ratio_to_whole_over_N": round(mine / (whole / n), 3),
                  "rows_ratio": round((NY // n + 2 * E) / (NY / n), 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closure_sharded_bench.txt"))
    a = ap.parse_args()
    lines = []

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)
    emit({"note": "one GPU; no link is timed: the wide halo exchanges of the sharded closure are not part of these numbers", "device": torch.cuda.get_device_name(0)})
    part_a(emit, a.reps)
    part_b(emit, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
