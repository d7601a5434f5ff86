"""What the prepared multigrid hierarchy (csrc/mg_prepared.h) promises without a GPU: the two size entries, the exported and declared C
entries in both precisions of the cycle, the reuse_hierarchy option's surface and its refusal next to a slab communicator, and the host-side
carves of the two buffers and of the ordinary solve's one workspace (csrc/mg_prepared_carve.h) walked by a stand-alone program built with
-fsanitize=address,undefined against arenas without memory."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GRIDS = ((12, 10), (64, 64), (96, 80), (70, 66), (520, 516), (1024, 256), (2048, 2048))      # (nx, ny)
NO_GRIDS = ((3, 40), (40, 3), (0, 0), (-4, 64), (1 << 16, 1 << 15))                          # below 4 cells a dimension, or above 2^30 cells
STEMS = ("prepare", "pcg_solve_prepared", "vcycle_prepared")
# piso_mg_workspace_bytes_cycle(nx, ny, elem) as the library returned it before the ordinary workspace got one carve over the cycle's type
# (two hand-written walks then): every array keeps its offset, so every size stays
WORKSPACE_BYTES = {(12, 10, 4): 74768, (12, 10, 8): 72208, (64, 64, 4): 583440, (64, 64, 8): 549904, (96, 80, 4): 1042960, (96, 80, 8): 979216,
                   (70, 66, 4): 659216, (70, 66, 8): 620560, (520, 516, 4): 34421008, (520, 516, 8): 32276752, (1024, 256, 4): 33611280,
                   (1024, 256, 8): 31513360, (2048, 2048, 4): 536930064, (2048, 2048, 8): 503374864}


def test_size_entries():
    import diffpiso._native as N
    hier, solve, whole = N.lib.piso_mg_hierarchy_bytes, N.lib.piso_mg_solve_workspace_bytes, N.lib.piso_mg_workspace_bytes_cycle
    for nx, ny in GRIDS:
        for elem in (4, 8):
            assert whole(nx, ny, elem) == WORKSPACE_BYTES[nx, ny, elem]
            assert whole(nx, ny, elem) > 0 and hier(nx, ny, elem) > 0 and solve(nx, ny, elem) > 0
            # the two buffers hold what the one workspace of the ordinary solve holds, plus the header and the second copy of the sums
            assert whole(nx, ny, elem) < hier(nx, ny, elem) + solve(nx, ny, elem) <= whole(nx, ny, elem) + 2 * 256
            assert hier(nx, ny, elem) >= 6 * 8 * nx * ny                   # at least the fp64 level 0
        assert N.lib.piso_mg_workspace_bytes(nx, ny) == WORKSPACE_BYTES[nx, ny, 8]
        assert hier(nx, ny, 4) > hier(nx, ny, 8)                           # (the float32 mode keeps the fp64 level 0 AND the float32 levels)
        for elem in (0, 2, 16, -4):
            assert whole(nx, ny, elem) == hier(nx, ny, elem) == solve(nx, ny, elem) == 0
    for nx, ny in NO_GRIDS:
        for elem in (4, 8):
            assert whole(nx, ny, elem) == hier(nx, ny, elem) == solve(nx, ny, elem) == 0


def test_every_entry_is_exported_and_declared_in_both_precisions():
    import diffpiso._native as N
    with open(os.path.join(ROOT, "include", "piso_hip.h")) as f:
        header = f.read()
    for name in ("piso_mg_hierarchy_bytes", "piso_mg_solve_workspace_bytes"):
        assert hasattr(N.lib, name) and re.search(r"\bsize_t %s\(int nx, int ny, int cycle_elem_size\);" % name, header), name
    for stem in STEMS:
        for sfx in ("_f64", "_c32_f64"):
            name = "piso_mg_%s%s" % (stem, sfx)
            assert hasattr(N.lib, name), name
            assert re.search(r"\bint %s\(int nx, int ny, int periodic_x, int periodic_y, " % name, header), name
        assert getattr(N.lib, "piso_mg_%s_f64" % stem).argtypes == getattr(N.lib, "piso_mg_%s_c32_f64" % stem).argtypes
    assert "not a hierarchy prepared for this grid" in re.sub(r"\s+\*\s+|\s+", " ", header)


def test_the_option_and_its_refusal_next_to_a_slab_communicator(monkeypatch):
    import torch
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso import distributed as D
    from diffpiso import solvers as S
    p = inspect.signature(dp.PisoPressureSolverMultigrid.__init__).parameters
    assert p["reuse_hierarchy"].default is False
    for fn, names in ((S.mg_prepare_native, ("nx", "ny", "per_x", "per_y", "L", "rank_deficient", "cycle_dtype")),
                      (S.mg_solve_prepared_native, ("h", "div", "accuracy", "max_iterations", "residual_reset", "sweeps")),
                      (S.mg_vcycle_prepared_native, ("h", "r", "sweeps"))):
        assert tuple(inspect.signature(fn).parameters) == names, fn.__name__
    ps = dp.PisoPressureSolverMultigrid(dx=[])
    assert ps.reuse_hierarchy is False
    assert dict(ps.stats) == dict(solves=0, iterations=0, adjoint_solves=0, adjoint_iterations=0, hierarchy_builds=0, hierarchy_reuses=0, laplace_builds=0)
    ps.drop_hierarchy()
    assert "raw pointer" in dp.PisoPressureSolverMultigrid.__doc__ and "float32 levels" in dp.PisoPressureSolverMultigrid.__doc__
    # a communicator that would cut the solve is never touched (it has no attribute beyond these two), and no solve is attempted
    calls = []
    monkeypatch.setattr(D, "mg_solve_slab", lambda *a, **kw: calls.append(a) or ("x", 7))
    comm = object.__new__(D.SlabCommunicator)
    comm.world, comm.sharded = 2, False
    L, div = torch.zeros(64 * 64, 5, dtype=torch.float64), torch.zeros(64 * 64, dtype=torch.float64)
    for dtype in (torch.float64, torch.float32):
        on = dp.PisoPressureSolverMultigrid(dx=[], cycle_dtype=dtype, reuse_hierarchy=True)
        on.slab_comm = comm
        with pytest.raises(N.PisoNativeError, match="reuse_hierarchy=False"):
            on._cg(64, 64, True, True, L, div, 1e-8, 10, True, 10)
        assert not calls and on.stats["hierarchy_builds"] == 0
    ps.slab_comm = comm                                         # the default is not refused: the slab solve as before
    assert ps._cg(64, 64, True, True, L, div, 1e-8, 10, True, 10) == ("x", 7) and len(calls) == 1


def test_the_carves_walk_clean_under_the_sanitizers(tmp_path):
    import diffpiso._native as N
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mg_prepared_carve_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "mg_prepared_carve_driver.cpp")], check=True)
    queries = [(nx, ny, elem) for nx, ny in GRIDS + NO_GRIDS for elem in (4, 8)] + [(64, 64, 2)]
    run = subprocess.run([exe], input="".join("%d %d %d\n" % q for q in queries), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = run.stdout.strip("\n").split("\n")
    assert len(lines) == len(queries)
    for (nx, ny, elem), line in zip(queries, lines):
        status, hb, sb, why, wb = line.split("\t")
        if (nx, ny) in NO_GRIDS or elem == 2:
            assert (int(status), int(hb), int(sb), int(wb)) == (1, 0, 0, 0), (nx, ny, elem, why)
            continue
        assert int(status) == 0, (nx, ny, elem, why)
        assert int(hb) == N.lib.piso_mg_hierarchy_bytes(nx, ny, elem) and int(sb) == N.lib.piso_mg_solve_workspace_bytes(nx, ny, elem), (nx, ny, elem)
        assert int(wb) == N.lib.piso_mg_workspace_bytes_cycle(nx, ny, elem) == WORKSPACE_BYTES[nx, ny, elem], (nx, ny, elem)
