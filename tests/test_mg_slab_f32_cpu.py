"""What the float32 cycle on y-slabs (csrc/mg_slab_f32.h) promises without a GPU: the workspace-size entry, the exported C entries, the
cycle_dtype keywords, the g = 0 refusal of PisoPressureSolverMultigrid._cg on a faked communicator, and the host-side workspace carve
(csrc/mg_slab_carve.h) walked by a stand-alone program built with -fsanitize=address,undefined against an arena without memory."""
import inspect
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
# (nx, ny, knob, ranks) -> g: the rows of tests/test_gpu_mg_slab_f32.py
ROWS = {(64, 64, 64, 1): 3, (64, 64, 64, 2): 3, (64, 64, 64, 4): 3, (64, 64, 64, 8): 3, (72, 96, 64, 2): 4, (72, 96, 64, 3): 4, (70, 96, 64, 3): 4,
        (512, 256, 0, 2): 2, (512, 256, 0, 4): 2, (2048, 1088, 0, 2): 5}
G0_ROWS = ((64, 64, 0, 2), (64, 64, 0, 4))
ENTRIES = ("pcg_solve_slab", "vcycle_slab", "level_slab", "pcg_solve_slab_emulated", "vcycle_slab_emulated", "level_slab_emulated")


@pytest.fixture
def knob():
    import diffpiso._native as N
    saved = N.get_option("mg_slab_gather_cells")
    yield lambda v: N.set_option("mg_slab_gather_cells", v if v else -1)
    N.set_option("mg_slab_gather_cells", saved)


def test_the_plan_gives_the_stated_g(knob):
    import diffpiso._native as N
    for (nx, ny, k, ranks), g in ROWS.items():
        knob(k)
        assert N.mg_slab_plan(nx, ny, ranks)["g"] == g, (nx, ny, k, ranks)
    for nx, ny, k, ranks in G0_ROWS:
        knob(k)
        assert N.mg_slab_plan(nx, ny, ranks)["g"] == 0


def test_workspace_size_entry_and_exports(knob):
    import diffpiso._native as N
    size = N.lib.piso_mg_slab_workspace_bytes_cycle
    for (nx, ny, k, ranks), g in ROWS.items():
        knob(k)
        for local in (1, ranks):
            old = N.lib.piso_mg_slab_workspace_bytes(nx, ny // ranks, ranks, local)
            assert size(nx, ny // ranks, ranks, local, 8) == old > 0
            assert size(nx, ny // ranks, ranks, local, 4) > 0
            for elem in (0, 2, 16, -4):
                assert size(nx, ny // ranks, ranks, local, elem) == 0
    for nx, ny, k, ranks in G0_ROWS:                            # g = 0: the fp64 cycle has a workspace, the float32 cycle is refused
        knob(k)
        assert size(nx, ny // ranks, ranks, ranks, 8) == N.lib.piso_mg_slab_workspace_bytes(nx, ny // ranks, ranks, ranks) > 0
        assert size(nx, ny // ranks, ranks, ranks, 4) == 0
    knob(64)
    assert size(70, 24, 4, 4, 4) == size(70, 24, 4, 4, 8) == 0    # a refused plan (24 rows per rank, g = 4)
    for stem in ENTRIES:
        assert hasattr(N.lib, "piso_mg_%s_c32_f64" % stem) and hasattr(N.lib, "piso_mg_%s_f64" % stem)
    assert hasattr(N.lib, "piso_comm_allgather_f32")


def test_cycle_dtype_keywords():
    import torch
    from diffpiso import distributed as D
    for fn in (D.mg_solve_slab, D.mg_solve_slab_local, D.mg_solve_slab_emulated, D.mg_vcycle_slab_local, D.mg_vcycle_slab_emulated, D.mg_level_slab_emulated,
               D._mg_slab_workspace):
        p = inspect.signature(fn).parameters
        assert "cycle_dtype" in p and p["cycle_dtype"].default == torch.float64, fn.__name__
    with pytest.raises(ValueError, match="cycle_dtype"):
        D._mg_slab_fn("vcycle_slab", torch.float16)


def test_g0_is_refused_by_the_solver_object_and_nothing_else_is(monkeypatch, knob):
    import torch
    import diffpiso as dp
    import diffpiso._native as N
    from diffpiso import distributed as D
    comm = object.__new__(D.SlabCommunicator)                   # a communicator that would cut the solve, never touched
    comm.world, comm.sharded = 2, False
    calls = []
    monkeypatch.setattr(D, "mg_solve_slab", lambda *a, **kw: calls.append((a, kw)) or ("x", 7))
    ps = dp.PisoPressureSolverMultigrid(dx=[], cycle_dtype=torch.float32)
    ps.slab_comm = comm
    knob(0)
    L = torch.zeros(64 * 64, 5, dtype=torch.float64)
    with pytest.raises(N.PisoNativeError, match=r"the float32 cycle runs on one GPU only; a solve cut into y-slabs needs cycle_dtype=torch\.float64"):
        ps._cg(64, 64, True, True, L, torch.zeros(64 * 64, dtype=torch.float64), 1e-8, 10, True, 10)      # 4096 cells: g = 0
    assert not calls
    knob(64)                                                    # the same grid with three sharded levels: not refused by that rule
    assert ps._cg(64, 64, True, True, L, torch.zeros(64 * 64, dtype=torch.float64), 1e-8, 10, True, 10) == ("x", 7)
    assert len(calls) == 1 and calls[0][1]["cycle_dtype"] == torch.float32 and calls[0][0][0] is comm
    knob(0)                                                     # a natural plan with g > 0
    L2 = torch.zeros(128 * 256, 5, dtype=torch.float64)
    assert ps._cg(128, 256, True, True, L2, torch.zeros(128 * 256, dtype=torch.float64), 1e-8, 10, True, 10) == ("x", 7)
    assert len(calls) == 2
    # the fp64 cycle never asks: g = 0 runs as before
    ps64 = dp.PisoPressureSolverMultigrid(dx=[])
    ps64.slab_comm = comm
    assert ps64._cg(64, 64, True, True, L, torch.zeros(64 * 64, dtype=torch.float64), 1e-8, 10, True, 10) == ("x", 7)
    assert calls[-1][1]["cycle_dtype"] == torch.float64


def test_the_carve_walks_clean_under_the_sanitizers(tmp_path):
    import diffpiso._native as N
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mg_slab_carve_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "mg_slab_carve_driver.cpp")], check=True)
    queries = [(nx, ny, ranks, k, elem) for (nx, ny, k, ranks) in ROWS for elem in (4, 8)] + [(64, 64, 2, 0, 8), (70, 96, 4, 64, 4)]
    run = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % q for q in queries), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = run.stdout.strip("\n").split("\n")
    assert len(lines) == len(queries)
    saved = N.get_option("mg_slab_gather_cells")
    try:
        for (nx, ny, ranks, k, elem), line in zip(queries, lines):
            status, nbytes, rows, why = line.split("\t")
            if (nx, ny, ranks, k) == (70, 96, 4, 64):
                assert int(status) == 1                         # the plan's refusal
                continue
            assert int(status) == 0, (nx, ny, ranks, k, elem, why)
            # the size is the library's: the collective buffer (one 256-byte block up to 2 ranks' worth) plus the rank's share rounded to 256
            N.set_option("mg_slab_gather_cells", k if k else -1)
            share = (int(nbytes) + 255) // 256 * 256
            assert N.lib.piso_mg_slab_workspace_bytes_cycle(nx, ny // ranks, ranks, 1, elem) == 256 + share, (nx, ny, ranks, k, elem)
            if elem == 4:
                quad_rows = sum(9 * (r + (2 if l < N.mg_slab_plan(nx, ny, ranks)["g"] else 0))
                                for l, ((lx, ly), r) in enumerate(zip(N.mg_slab_plan(nx, ny, ranks)["levels"], N.mg_slab_plan(nx, ny, ranks)["rows"])) if lx % 4 == 0)
                assert int(rows) == quad_rows, (nx, ny, ranks, k, rows, quad_rows)
            else:
                assert int(rows) == 0
    finally:
        N.set_option("mg_slab_gather_cells", saved)
