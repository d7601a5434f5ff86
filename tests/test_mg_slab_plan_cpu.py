"""The plan of the slab multigrid (csrc/mg_slab_plan.h) is pure host code: tests/mg_slab_plan_driver.cpp, built with a host compiler, walks it
without a card.  Level dimensions against the one-GPU plan (tests/mg_reference.plan, the numpy twin's restatement of mg.hip's), the first
replicated level g, the rows a rank holds of every level, the tail, and the refusals with their rule."""
import os
import shutil
import subprocess

import pytest

from tests import mg_reference as M

HERE = os.path.dirname(os.path.abspath(__file__))
GATHER_CELLS = 8192
# (nx, ny, ranks, knob) -> g; knob 0: none
ACCEPTED = {(64, 64, 1, 64): 3, (64, 64, 2, 64): 3, (64, 64, 4, 64): 3, (64, 64, 8, 64): 3,
            (70, 96, 2, 64): 4, (70, 96, 3, 64): 4, (70, 96, 4, 128): 3,
            (64, 64, 1, 0): 0, (64, 64, 2, 0): 0, (64, 64, 4, 0): 0, (64, 64, 8, 0): 0,
            (512, 256, 2, 0): 2, (512, 256, 4, 0): 2,
            (2048, 2048, 8, 0): None, (4096, 4096, 8, 0): None}          # (sizes only: g from the rule below)
REFUSED = {(70, 96, 4, 64): "24 rows per rank are not divisible by 16", (64, 64, 3, 64): "not divisible by 3 ranks", (70, 96, 5, 0): "not divisible by 5 ranks",
           (64, 64, 2, 8): "no level"}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("mg_slab_plan") / "mg_slab_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(HERE, "mg_slab_plan_driver.cpp")], check=True)
    queries = list(ACCEPTED) + list(REFUSED)
    out = subprocess.run([exe], input="".join("%d %d %d %d\n" % q for q in queries), capture_output=True, text=True, check=True, timeout=60).stdout
    res = {}
    for q, line in zip(queries, out.strip("\n").split("\n")):
        rec, coll, msg = line.split("|")
        res[q] = ([int(v) for v in rec.split()], [int(v) for v in coll.split()], msg.strip())
    assert len(res) == len(queries)
    return res


def _expected_g(sizes, limit):
    return next(l for l, (nx, ny) in enumerate(sizes) if nx * ny <= limit)


@pytest.mark.parametrize("q", sorted(ACCEPTED))
def test_accepted_plans(plans, q):
    nx, ny, world, knob = q
    rec, coll, msg = plans[q]
    sizes, tail_first = M.plan(nx, ny)                          # the one-GPU plan
    status, nlev, g, tail, nyl, w = rec[:6]
    assert status == 0 and msg == "-" and (nlev, nyl, w) == (len(sizes), ny // world, world)
    levels = [(rec[6 + 3 * l], rec[7 + 3 * l]) for l in range(nlev)]
    rows = [rec[8 + 3 * l] for l in range(nlev)]
    assert levels == [tuple(s) for s in sizes]
    limit = knob if 0 < knob < GATHER_CELLS else GATHER_CELLS
    assert g == _expected_g(sizes, limit)
    if ACCEPTED[q] is not None:
        assert g == ACCEPTED[q]
    assert nyl % (1 << g) == 0
    assert rows == [nyl >> l if l < g else sizes[l][1] for l in range(nlev)]
    assert all(r >= 1 for r in rows)
    assert sizes[g][1] % world == 0 and sizes[g][0] * sizes[g][1] <= limit          # the gather carries whole rows of every rank
    assert tail == (-1 if tail_first < 0 else max(tail_first, g))
    # two sweeps: per sharded level r before the first sweeps, z before the restriction and before the second post-sweep; e of every sharded
    # coarser level; z before the direction.  (r, z) and (p, q); the residual of level g and the maxima of |r|
    assert coll == ([0, 2, 2] if g == 0 else [3 * g + (g - 1) + 1, 2, 2])


def test_named_rows(plans):
    assert plans[(64, 64, 8, 64)][0][8 + 3 * 3] == 8             # the gather level is whole on every rank ...
    assert plans[(64, 64, 8, 64)][0][8 + 3 * 2] == 2 and (64 // 8) >> 3 == 1       # ... one row per rank goes into it, two rows at the last sharded level
    rec = plans[(512, 256, 4, 0)][0]
    assert (rec[2], rec[3]) == (2, 3)                            # a replicated level that runs as kernels of its own before the tail
    assert plans[(2048, 2048, 8, 0)][0][2] == 5 and plans[(4096, 4096, 8, 0)][0][2] == 6


@pytest.mark.parametrize("q", sorted(REFUSED))
def test_refused_plans(plans, q):
    rec, coll, msg = plans[q]
    assert rec[0] != 0 and len(rec) == 6
    assert REFUSED[q] in msg and "PisoPressureSolverCudaCustom" in msg and "2^g" in msg
