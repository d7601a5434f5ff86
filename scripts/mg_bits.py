"""What the multigrid pressure solver computes, as one sha256 per result: run once per BUILD of the library (PISO_HIP_LIB, a fresh process
each) and compare the two outputs line for line - a refactoring of csrc/mg*.h must leave every line as it was.  Needs a GPU.

    PISO_HIP_LIB=<build A> python scripts/mg_bits.py > a.txt;  PISO_HIP_LIB=<build B> python scripts/mg_bits.py > b.txt;  cmp a.txt b.txt

Per case and type of the cycle's values: every level operator, one V-cycle's z (tail on / off, four-cell kernels on / off), x and the count
of a capped and of a converged solve, the same from a prepared hierarchy, from an accepted and a rejected guess, and the dispatch record of
each.  Cases are the tables of tests/test_gpu_mg_hierarchy.py (every class of hierarchy, every solid pattern) and tests/test_gpu_mg_slab.py
(emulated slabs of 2 and 4, every g the knob gives, solids on the cuts)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-piso_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diffpiso._native as N  # noqa: E402
from diffpiso import distributed as D, solvers as S  # noqa: E402
from tests import test_gpu_mg_hierarchy as TH, test_gpu_mg_slab as TS  # noqa: E402
from tests.cases import laplace_case, solid_pattern  # noqa: E402

ACC, BIG = 1e-10, 1 << 30
DTYPES = (("f64", torch.float64), ("c32", torch.float32))


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def out(case, what, *vals):
    d = N.mg_last_dispatch()
    print(case, what, *vals, "dispatch=" + ",".join("%s:%s" % kv for kv in sorted(d.items())), flush=True)


def guarded(case, what, fn):
    """A refusal is a result too: its message must be the same in both builds."""
    try:
        return fn()
    except N.PisoNativeError as e:
        print(case, what, "refused:", hashlib.sha256(str(e).encode()).hexdigest()[:24], flush=True)
        return None


def system(name, nx, ny, solids):
    s, L, b = laplace_case(name, ny, nx, 3, solids=solids)
    per_y, per_x = (bool(v) for v in s.periodic_yx)
    return (nx, ny, per_x, per_y, dev(np.asarray(L, np.float64).reshape(-1, 5))), dev(b), bool(s.rank_deficient)


def whole(case, args, b, rd, solves):
    nx, ny = args[0], args[1]
    r = dev(np.random.default_rng(7).standard_normal(nx * ny))
    for tag, dt in DTYPES:
        c = "%s %s" % (case, tag)
        level = 0
        while True:
            lv = S.mg_level_native(*args, level, cycle_dtype=dt)
            if lv is None:
                break
            out(c, "level%d" % level, lv[1], lv[2], sha(lv[0]))
            level += 1
        for tail, vec in ((1, 1), (0, 1), (1, 0)):
            N.set_option("mg_tail", tail)
            N.set_option("mg_f32_vec", vec)
            for sweeps in (1, 2, 3):
                out(c, "vcycle tail%d vec%d nu%d" % (tail, vec, sweeps), sha(S.mg_vcycle_native(*args, r, sweeps, cycle_dtype=dt)))
        N.set_option("mg_tail", -1)
        N.set_option("mg_f32_vec", -1)
        x, it = S.mg_solve_native(*args, b, 1e-30, 6, rd, 3, cycle_dtype=dt)
        out(c, "capped", it, sha(x))
        if not solves:
            continue
        x, it = S.mg_solve_native(*args, b, ACC, 400, rd, 10, cycle_dtype=dt)
        out(c, "converged", it, sha(x))
        h = S.mg_prepare_native(*args, rd, cycle_dtype=dt)
        out(c, "prepared vcycle", sha(S.mg_vcycle_prepared_native(h, r)))
        xp, itp = S.mg_solve_prepared_native(h, b, ACC, 400, 10)
        out(c, "prepared converged", itp, sha(xp))
        for kind, x0 in (("near", x * (1 + 1e-3)), ("far", x * -50.0)):
            xg, itg = S.mg_solve_native(*args, b, ACC, 400, rd, 10, cycle_dtype=dt, x0=x0)
            out(c, "guess %s" % kind, itg, N.mg_last_guess(), sha(xg))
            xg, itg = S.mg_solve_prepared_guess_native(h, b, x0, ACC, 400, 10)
            out(c, "prepared guess %s" % kind, itg, N.mg_last_guess(), sha(xg))


def slabs(case, row, args, b, rd):
    nx, ny, knob, ranks = row
    N.set_option("mg_slab_gather_cells", knob if knob else -1)
    plan = N.mg_slab_plan(nx, ny, ranks)
    r = dev(np.random.default_rng(7).standard_normal(nx * ny))
    for tag, dt in DTYPES:
        c = "%s %s" % (case, tag)
        for level in range(len(plan["levels"])):
            for rank in range(ranks):
                lv = guarded(c, "level%d rank%d" % (level, rank), lambda: D.mg_level_slab_emulated(ranks, rank, *args, level, cycle_dtype=dt))
                if lv is not None:
                    out(c, "level%d rank%d" % (level, rank), lv[1], lv[2], sha(lv[0]))
        for vec in (1, 0):
            N.set_option("mg_f32_vec", vec)
            for sweeps in (1, 2, 3):
                z = guarded(c, "vcycle", lambda: D.mg_vcycle_slab_emulated(ranks, *args, r, sweeps, cycle_dtype=dt))
                if z is not None:
                    out(c, "vcycle vec%d nu%d" % (vec, sweeps), sha(z))
        N.set_option("mg_f32_vec", -1)
        for what, acc, K, reset in (("capped", 1e-30, 6, 3), ("converged", ACC, 400, 10)):
            res = guarded(c, what, lambda: D.mg_solve_slab_emulated(ranks, *args, b, acc, K, rd, reset, cycle_dtype=dt))
            if res is not None:
                out(c, what, res[1], sha(res[0]))
    N.set_option("mg_slab_gather_cells", -1)


def main():
    for (nx, ny), name in TH.HIERARCHY_SYSTEMS:
        args, b, rd = system(name, nx, ny, None)
        whole("whole %dx%d %s" % (nx, ny, name), args, b, rd, True)
    for (ny, nx), name, pattern in TH.SOLID_SYSTEMS:
        args, b, rd = system(name, nx, ny, solid_pattern(pattern, ny, nx))
        whole("solid %dx%d %s %s" % (nx, ny, name, pattern), args, b, rd, pattern in ("block4", "wall"))
    for row, name, pattern in TS.SYSTEMS:
        if row[3] in (2, 4):
            args, b, rd = system(name, row[0], row[1], TS._solids(pattern, row[0], row[1], name))
            slabs("slab %dx%d-knob%d-%dranks %s %s" % (row + (name, pattern)), row, args, b, rd)


if __name__ == "__main__":
    main()
