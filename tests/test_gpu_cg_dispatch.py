"""Which kernel instance does a pressure CG solve run, and is every instance the dispatcher can pick right?

One call of piso_cg_solve_* ends in one of about thirty kernel instances, chosen from the grid, the DATA (are the off-diagonals exact
floats, can the diagonal be rebuilt, is the matrix symmetric bit for bit) and the POINTERS (16-byte alignment of b and x) - cg.hip:
cg_solve / GpuLink over cg_driver.h: cg_coefs, cg_with_instance and cg_dispatch.h: persist_plan.  Every row of ROWS below pins one instance class: the solve goes through the C ABI, the dispatch record
(piso_cg_last_dispatch) must EQUAL the row's expectation - written from the dispatch code, not read back from the card - and the result
is compared with the C oracle (never with another GPU path alone).  Run with `-m gpu` on an MI355X (256 CUs, 8 XCDs: the expected
persistent shapes assume them).

Coefficient classes of a row:
  A   the Laplace matrix of the case as assembled: float-exact off-diagonals, symmetric; the diagonal can be rebuilt (RECON) except
      for spatial_ml, whose diagonal carries the faces to the outside (that case is class B of the dispatcher: CT = float, RECON = 0)
  C   L * (1/3) in fp64, b scaled alike: still symmetric, off-diagonals no longer floats -> CT = double, RECON = 0 without a knob
  U   every odd grid row of L (and of b) times 2: the same solution, exact in floating point, float-exact - and NOT symmetric (what a C
      caller's one-sided couplings look like to the set-up check); short fixed-iteration runs only (CG need not converge on it)
  CU  both.
fp32 rows: "A" is assembled in float32 (diagonal rebuildable in float32), "A64" is the float64 matrix rounded to float32 (it is not).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import native as O
from tests.cases import dev, laplace_case, pressure_system

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

CENSUS_KEY = ("path", "sizeof_T", "sizeof_CT", "V", "RECON", "symmetric", "R", "NQ", "waves", "padded", "xcd_local")


def two(T, CT, V, recon, sym=1, **extra):
    """Expected record of a solve that iterates on cg_k1<T, CT, V, RECON> + cg_k2<T, V> only."""
    d = dict(path=2, sizeof_T=T, sizeof_CT=CT, V=V, RECON=recon, symmetric=sym, R=0, NQ=0, waves=0, launch_grid=0, padded=0, xcd_local=0,
             fell_back=0, tiny_per_x=0, segments=0)
    d.update(extra)
    return d


def per(T, CT, recon, sym, R, NQ, waves, launch_grid, padded=0, xcd_local=0, **extra):
    """Expected record of a solve dispatched to cg_persist1<T, CT, R, NQ, RECON, SYMV, ...> (+ the two-kernel pair for iteration 0 / resets)."""
    d = dict(path=3, sizeof_T=T, sizeof_CT=CT, V=16 // T, RECON=recon, symmetric=sym, R=R, NQ=NQ, waves=waves, launch_grid=launch_grid,
             padded=padded, xcd_local=xcd_local, fell_back=0, tiny_per_x=0)
    d.update(extra)
    return d


def tiny(path, T, per_x=0):
    d = dict.fromkeys(("V", "RECON", "symmetric", "rows_per_wave", "k1_grid", "k1_tiles", "R", "NQ", "waves", "launch_grid", "padded", "xcd_local",
                       "fell_back", "k2_grid", "segments"), 0)
    d.update(path=path, sizeof_T=T, sizeof_CT=T, tiny_per_x=per_x)
    return d


def row(id, case, ny, nx, expect, dtype=f64, cls="A", offset=0, knobs=(), checks="TSK"):
    return dict(id=id, case=case, ny=ny, nx=nx, dtype=dtype, cls=cls, offset=offset, knobs=dict(knobs), expect=expect, checks=checks)


P0 = (("cg_persist", 0),)
# checks: T fixed-iteration trajectory (un-shifted), S the rank-1 shift (short runs + converged), K converged un-shifted solve
ROWS = [
    # ---- two-kernel, fp64, V = 2: all four cases above the tiny threshold.  The periodic grids get here with no knob (rows that are not
    # a multiple of 128 cells cannot be tiled and a periodic axis is never padded); the wall-bounded ones would be padded (padded_dims)
    row("k2-periodic-72x130", "periodic", 72, 130, two(8, 4, 2, 1, rows_per_wave=2, k1_tiles=18, k1_grid=16, k2_grid=5)),
    row("k2-xper-72x130", "xper_ywall", 72, 130, two(8, 4, 2, 1, rows_per_wave=2, k1_tiles=18, k1_grid=16)),
    row("k2-cavity-72x130", "cavity", 72, 130, two(8, 4, 2, 1, k1_tiles=18, k1_grid=16), knobs=(("cg_pad", 0),)),
    row("k2-sml-72x130", "spatial_ml", 72, 130, two(8, 4, 2, 0, k1_tiles=18, k1_grid=16), knobs=P0, checks="TK"),
    row("k2-periodic-75x192", "periodic", 75, 192, two(8, 4, 2, 1, k1_tiles=20, k1_grid=16), checks="TS"),       # ny odd, partial last strip
    row("k2-xper-75x192", "xper_ywall", 75, 192, two(8, 4, 2, 1, k1_tiles=20, k1_grid=16), checks="TS"),
    row("k2-periodic-41x320", "periodic", 41, 320, two(8, 4, 2, 1, k1_tiles=18, k1_grid=16), checks="TK"),
    row("k2-cavity-41x320", "cavity", 41, 320, two(8, 4, 2, 1, k1_tiles=18, k1_grid=16), knobs=(("cg_pad", 0),), checks="T"),
    # ---- V = 1 because nx is odd: the wrap partner of a last strip of 3 / 1 cells
    row("v1-periodic-70x131", "periodic", 70, 131, two(8, 4, 1, 1, k1_tiles=27, k1_grid=24)),
    row("v1-xper-70x131", "xper_ywall", 70, 131, two(8, 4, 1, 1, k1_tiles=27, k1_grid=24)),
    row("v1-cavity-70x131", "cavity", 70, 131, two(8, 4, 1, 1, k1_tiles=27, k1_grid=24)),
    row("v1-sml-70x131", "spatial_ml", 70, 131, two(8, 4, 1, 0, k1_tiles=27, k1_grid=24), checks="TK"),
    row("v1-cavity-80x65", "cavity", 80, 65, two(8, 4, 1, 1, k1_tiles=20, k1_grid=16), checks="TK"),
    row("v1-xper-70x129", "xper_ywall", 70, 129, two(8, 4, 1, 1, k1_tiles=27, k1_grid=24), checks="TS"),
    # ---- V = 1 because b and x are only 8-byte aligned (legal through the C ABI)
    row("v1-unaligned-72x130", "periodic", 72, 130, two(8, 4, 1, 1, k1_tiles=27, k1_grid=24), offset=1),
    row("v1-unaligned-xper-72x130", "xper_ywall", 72, 130, two(8, 4, 1, 1, k1_tiles=27, k1_grid=24), offset=1, checks="TS"),
    # ---- fp32 state on the two-kernel path: V = 4, V = 1 by nx, V = 1 by a 4-byte aligned pointer; rebuildable diagonal or not
    row("f32-periodic-64x256", "periodic", 64, 256, two(4, 4, 4, 1, k1_tiles=8, k1_grid=8), dtype=f32, knobs=P0, checks="TK"),
    row("f32-cavity-64x256", "cavity", 64, 256, two(4, 4, 4, 1, k1_tiles=8, k1_grid=8), dtype=f32, knobs=P0, checks="TK"),
    row("f32-periodic-72x132", "periodic", 72, 132, two(4, 4, 4, 1, k1_tiles=9, k1_grid=8), dtype=f32, checks="TK"),
    row("f32-a64-72x132", "xper_ywall", 72, 132, two(4, 4, 4, 0, k1_tiles=9, k1_grid=8), dtype=f32, cls="A64", checks="TK"),
    row("f32-v1-periodic-70x130", "periodic", 70, 130, two(4, 4, 1, 1, k1_tiles=27, k1_grid=24), dtype=f32, checks="TK"),
    row("f32-v1-cavity-70x131", "cavity", 70, 131, two(4, 4, 1, 1, k1_tiles=27, k1_grid=24), dtype=f32, checks="TK"),
    row("f32-v1-a64-70x131", "periodic", 70, 131, two(4, 4, 1, 0, k1_tiles=27, k1_grid=24), dtype=f32, cls="A64", checks="TK"),
    row("f32-v1-unaligned-72x132", "periodic", 72, 132, two(4, 4, 1, 1, k1_tiles=27, k1_grid=24), dtype=f32, offset=1, checks="TK"),
    # ---- off-diagonals that are not floats (CT = T), and unsymmetric systems, with no knob
    row("c-periodic-72x130", "periodic", 72, 130, two(8, 8, 2, 0, k1_tiles=18, k1_grid=16), cls="C"),
    # (a wall-bounded grid is padded BEFORE the coefficients are looked at; the padded persistent instance is for CT = float only, so this
    # one iterates on the two-kernel path over the padded 72 x 256 grid: true_cell() keeps the shift off the padding)
    row("c-cavity-72x130", "cavity", 72, 130, two(8, 8, 2, 0, k1_tiles=18, k1_grid=16, padded=1), cls="C"),
    row("c-v1-periodic-70x131", "periodic", 70, 131, two(8, 8, 1, 0, k1_tiles=27, k1_grid=24), cls="C"),
    row("c-sml-64x256", "spatial_ml", 64, 256, two(8, 8, 2, 0, k1_tiles=16, k1_grid=16), cls="C", knobs=P0, checks="T"),
    row("u-periodic-72x130", "periodic", 72, 130, two(8, 4, 2, 1, sym=0), cls="U", checks="T"),
    row("cu-sml-72x130", "spatial_ml", 72, 130, two(8, 8, 2, 0, sym=0), cls="CU", knobs=P0, checks="T"),
    row("cu-v1-sml-70x131", "spatial_ml", 70, 131, two(8, 8, 1, 0, sym=0), cls="CU", checks="T"),
    # ---- rows per wave 3 / 8 / 16 with ny NOT a multiple of 4 * rpw: clamped last tile row, waves with no rows, odd waves walking downwards
    row("rpw3-periodic-100x192", "periodic", 100, 192, two(8, 4, 2, 1, rows_per_wave=3, k1_tiles=18, k1_grid=16), knobs=(("cg_rpw", 3),), checks="TS"),
    row("rpw8-periodic-67x256", "periodic", 67, 256, two(8, 4, 2, 1, rows_per_wave=8, k1_tiles=6, k1_grid=6), knobs=(("cg_rpw", 8),), checks="TS"),
    row("rpw16-xper-130x128", "xper_ywall", 130, 128, two(8, 4, 2, 1, rows_per_wave=16, k1_tiles=3, k1_grid=3), knobs=(("cg_rpw", 16), ("cg_persist", 0)),
        checks="TS"),
    row("rpw8-v1-cavity-67x131", "cavity", 67, 131, two(8, 4, 1, 1, rows_per_wave=8, k1_tiles=9, k1_grid=8), knobs=(("cg_rpw", 8),), checks="TK"),
    # ---- how tiles (K1) and chunks (K2) are dealt to blocks (xcd_range): fewer than 8 blocks - plain stride; a grid rounded DOWN to a
    # multiple of 8 (18 tiles on 16 blocks: chunks of 3, XCD 6's range empty, XCD 7's inverted); an exact split; many tiles per block
    row("deal-stride-24x130", "periodic", 24, 130, two(8, 4, 2, 1, k1_tiles=6, k1_grid=6, k2_grid=2), knobs=(("cg_tiny", 0),), checks="TS"),
    row("deal-exact-64x256", "periodic", 64, 256, two(8, 4, 2, 1, k1_tiles=16, k1_grid=16, k2_grid=8), knobs=P0, checks="TS"),
    row("deal-cap8-256x512", "periodic", 256, 512, two(8, 4, 2, 1, rows_per_wave=2, k1_tiles=128, k1_grid=8, k2_grid=64),
        knobs=(("cg_maxblocks", 8), ("cg_persist", 0)), checks="T"),
    row("deal-cap8-130x384", "xper_ywall", 130, 384, two(8, 4, 2, 1, rows_per_wave=2, k1_tiles=51, k1_grid=8, k2_grid=24),
        knobs=(("cg_maxblocks", 8), ("cg_persist", 0)), checks="TS"),
    row("deal-cap16-v1-70x131", "periodic", 70, 131, two(8, 4, 1, 1, k1_tiles=27, k1_grid=16), knobs=(("cg_maxblocks", 16),), checks="TS"),
    # ---- persistent kernel: the instances the DATA picks.  CT = double means regions of 2 / 4 rows (persist_instance_exists; a forced 16 has no
    # instance -> two-kernel); an unsymmetric matrix streams all four arrays (SYMV = false), with regions of 2 / 4 / 16 rows
    row("p-c-r2-32x256", "periodic", 32, 256, per(8, 8, 0, 1, 2, 2, 4, 4), cls="C", knobs=(("cg_persist", 1), ("cg_persist_r", 2))),
    row("p-c-r4-32x256", "cavity", 32, 256, per(8, 8, 0, 1, 4, 2, 4, 2), cls="C", knobs=(("cg_persist", 1), ("cg_persist_r", 4)), checks="TK"),
    row("p-c-auto-64x512", "periodic", 64, 512, per(8, 8, 0, 1, 2, 2, 4, 16), cls="C", checks="TK"),
    row("p-c-r16-64x256", "periodic", 64, 256, two(8, 8, 2, 0, k1_tiles=16, k1_grid=16), cls="C", knobs=(("cg_persist", 1), ("cg_persist_r", 16)), checks="T"),
    row("p-cu-r2-32x256", "spatial_ml", 32, 256, per(8, 8, 0, 0, 2, 2, 4, 4), cls="CU", knobs=(("cg_persist", 1), ("cg_persist_r", 2)), checks="T"),
    row("p-cu-r4-32x256", "periodic", 32, 256, per(8, 8, 0, 0, 4, 2, 4, 2), cls="CU", knobs=(("cg_persist", 1), ("cg_persist_r", 4)), checks="T"),
    row("p-u-r2-32x256", "periodic", 32, 256, per(8, 4, 1, 0, 2, 2, 4, 4), cls="U", knobs=(("cg_persist", 1), ("cg_persist_r", 2)), checks="T"),
    row("p-u-r4-32x256", "spatial_ml", 32, 256, per(8, 4, 0, 0, 4, 2, 4, 2), cls="U", knobs=(("cg_persist", 1), ("cg_persist_r", 4)), checks="T"),
    row("p-u-r16-64x256", "periodic", 64, 256, per(8, 4, 1, 0, 16, 1, 8, 1), cls="U", knobs=(("cg_persist", 1), ("cg_persist_r", 16)), checks="T"),
    # ... and the symmetric ones (their arithmetic is test_gpu_kernels.py's subject; here the record is pinned): XCD-local by default
    row("p-r2-32x256", "periodic", 32, 256, per(8, 4, 1, 1, 2, 1, 8, 32, xcd_local=1), knobs=(("cg_persist", 1), ("cg_persist_r", 2)), checks="TS"),
    row("p-r4-32x256", "xper_ywall", 32, 256, per(8, 4, 1, 1, 4, 2, 4, 16, xcd_local=1), knobs=(("cg_persist", 1), ("cg_persist_r", 4)), checks="TS"),
    row("p-r16-64x256", "periodic", 64, 256, per(8, 4, 1, 1, 16, 1, 8, 1), knobs=(("cg_persist", 1), ("cg_persist_r", 16)), checks="TS"),
    row("p-sml-r2-32x256", "spatial_ml", 32, 256, per(8, 4, 0, 1, 2, 1, 8, 4), knobs=(("cg_persist", 1), ("cg_persist_r", 2)), checks="T"),
    row("p-sml-r4-32x256", "spatial_ml", 32, 256, per(8, 4, 0, 1, 4, 2, 4, 2), knobs=(("cg_persist", 1), ("cg_persist_r", 4)), checks="T"),
    row("p-sml-r16-64x256", "spatial_ml", 64, 256, per(8, 4, 0, 1, 16, 1, 8, 1), knobs=(("cg_persist", 1), ("cg_persist_r", 16)), checks="T"),
    row("p-nq2-chipwide-64x512", "periodic", 64, 512, per(8, 4, 1, 1, 2, 2, 8, 8), knobs=(("cg_persist_nq", 0), ("cg_persist_half", 0), ("cg_xcd_local", 0)),
        checks="TS"),
    # ---- padded-grid mode: a wall-bounded 72 x 130 grid embedded in 72 x 256, on one XCD (default) and chip-wide
    row("pad-cavity-72x130", "cavity", 72, 130, per(8, 4, 1, 1, 2, 2, 4, 72, padded=1, xcd_local=1, k1_tiles=18, k1_grid=16)),
    row("pad-chipwide-cavity-72x130", "cavity", 72, 130, per(8, 4, 1, 1, 2, 2, 4, 9, padded=1), knobs=(("cg_xcd_local", 0),), checks="TK"),
    row("pad-r4-cavity-70x130", "cavity", 70, 130, per(8, 4, 1, 1, 4, 2, 4, 5, padded=1), knobs=(("cg_xcd_local", 0), ("cg_persist_r", 4)), checks="TK"),
    # ---- one workgroup (cg_tiny.h): the record only; the arithmetic is test_cg_tiny_single_workgroup_matches_oracle's subject
    row("tiny-cols-65x64", "cavity", 65, 64, tiny(1, 8), checks="T"),
    row("tiny-cols-perx-40x64", "periodic", 40, 64, tiny(1, 8, per_x=1), checks="T"),
    row("tiny-general-33x70", "periodic", 33, 70, tiny(0, 8), checks="T"),
    row("tiny-general-f32-33x70", "periodic", 33, 70, tiny(0, 4), dtype=f32, checks="T"),
]
ROW = {r["id"]: r for r in ROWS}
assert len(ROW) == len(ROWS)

# Every (path, sizeof T, sizeof CT, V, RECON, symmetric, R, NQ, waves, padded, xcd_local) the rows above - and the knob pairs of
# test_persistent_workgroup_knobs - must reach.  A kernel instance added to the dispatcher without a row shows up as a diff here.
#
# cg.hip's instantiations and the row that reaches each:
#   cg_k1<double, float, 2, true>            k2-periodic-72x130 ...        cg_k1<double, float, 2, false>   k2-sml-72x130
#   cg_k1<double, float, 1, true>            v1-periodic-70x131 ...        cg_k1<double, float, 1, false>   v1-sml-70x131
#   cg_k1<double, double, 2, false>          c-periodic-72x130             cg_k1<double, double, 1, false>  c-v1-periodic-70x131
#   cg_k1<float, float, 4, true / false>     f32-periodic-64x256 / f32-a64-72x132
#   cg_k1<float, float, 1, true / false>     f32-v1-periodic-70x130 / f32-v1-a64-70x131
#   cg_persist1<double, float, 2 | 4 | 16, NQ, RECON, SYMV = true>   p-r2 / p-r4 / p-r16 (RECON), p-sml-r2 / -r4 / -r16 (diagonal streamed)
#   cg_persist1<double, float, 2, 1, ...>    p-r2-32x256 (XCD-local), p-sml-r2-32x256 (chip-wide); NQ = 2: p-nq2-chipwide-64x512
#   cg_persist1<double, float, R, NQ, RECON, false>   p-u-r2 / p-u-r4 / p-u-r16 (SYMV = false: all four arrays)
#   cg_persist1<double, double, 2 | 4, 2, false, false>   p-c-r2 / p-c-r4 / p-cu-r2 / p-cu-r4 (a symmetric CT = double system has no
#                                            SYMV instance, and none of 16 rows: persist_instance_exists) -> p-c-r16-64x256 is two-kernel
#   cg_persist1<..., RAGGED>                 pad-cavity-72x130 (LOCAL), pad-chipwide-cavity-72x130, pad-r4-cavity-70x130
#   cg_persist1<..., LOCAL>                  p-r2 / p-r4-32x256, test_persistent_workgroup_knobs
#   cg_persist1<float, ...>                  test_gpu_kernels.py: test_cg_persistent_float32_state_matches_oracle (record asserted there)
#   cg_persist1<..., SLAB = true>            more than one GPU: test_gpu_slab.py / test_gpu_multiproc.py
#   the restart after an exchange gave up    cannot be provoked and must not be; fell_back = 1 is reached through cg_verify = 2
#                                            (test_gpu_fullsize.py)
#   cg_tiny / cg_tiny_cols<per_x>            tiny-general-33x70, tiny-cols-65x64, tiny-cols-perx-40x64
CENSUS = [
    # path T CT V RECON sym  R NQ waves padded local
    (0, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0), (1, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0), (0, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0),
    (2, 8, 4, 2, 1, 1, 0, 0, 0, 0, 0), (2, 8, 4, 2, 0, 1, 0, 0, 0, 0, 0), (2, 8, 4, 1, 1, 1, 0, 0, 0, 0, 0), (2, 8, 4, 1, 0, 1, 0, 0, 0, 0, 0),
    (2, 8, 8, 2, 0, 1, 0, 0, 0, 0, 0), (2, 8, 8, 1, 0, 1, 0, 0, 0, 0, 0), (2, 8, 8, 2, 0, 0, 0, 0, 0, 0, 0), (2, 8, 8, 1, 0, 0, 0, 0, 0, 0, 0),
    (2, 8, 4, 2, 1, 0, 0, 0, 0, 0, 0), (2, 8, 8, 2, 0, 1, 0, 0, 0, 1, 0),
    (2, 4, 4, 4, 1, 1, 0, 0, 0, 0, 0), (2, 4, 4, 4, 0, 1, 0, 0, 0, 0, 0), (2, 4, 4, 1, 1, 1, 0, 0, 0, 0, 0), (2, 4, 4, 1, 0, 1, 0, 0, 0, 0, 0),
    (3, 8, 4, 2, 1, 1, 2, 1, 8, 0, 1), (3, 8, 4, 2, 1, 1, 4, 2, 4, 0, 1), (3, 8, 4, 2, 1, 1, 16, 1, 8, 0, 0), (3, 8, 4, 2, 1, 1, 2, 2, 8, 0, 0),
    (3, 8, 4, 2, 0, 1, 2, 1, 8, 0, 0), (3, 8, 4, 2, 0, 1, 4, 2, 4, 0, 0), (3, 8, 4, 2, 0, 1, 16, 1, 8, 0, 0),
    (3, 8, 4, 2, 1, 0, 2, 2, 4, 0, 0), (3, 8, 4, 2, 0, 0, 4, 2, 4, 0, 0), (3, 8, 4, 2, 1, 0, 16, 1, 8, 0, 0),
    (3, 8, 8, 2, 0, 1, 2, 2, 4, 0, 0), (3, 8, 8, 2, 0, 1, 4, 2, 4, 0, 0), (3, 8, 8, 2, 0, 0, 2, 2, 4, 0, 0), (3, 8, 8, 2, 0, 0, 4, 2, 4, 0, 0),
    (3, 8, 4, 2, 1, 1, 2, 2, 4, 1, 1), (3, 8, 4, 2, 1, 1, 2, 2, 4, 1, 0), (3, 8, 4, 2, 1, 1, 4, 2, 4, 1, 0),
    # the knob pairs of test_persistent_workgroup_knobs: full / half workgroups, one XCD / chip-wide, one / two regions per wave
    (3, 8, 4, 2, 1, 1, 2, 2, 8, 0, 1), (3, 8, 4, 2, 1, 1, 2, 2, 4, 0, 0), (3, 8, 4, 2, 1, 1, 2, 1, 8, 0, 0), (3, 8, 4, 2, 1, 1, 2, 2, 4, 0, 1),
]


def census_key(rec):
    return tuple(rec[k] for k in CENSUS_KEY)


# ------------------------------------------------------------------------------------------------------------------ helpers
def system(r):
    """-> (set-up, L [n, 5] and b on the host in float64 - what the oracle is given)."""
    built = f32 if (r["dtype"] == f32 and r["cls"] == "A") else f64
    s, L, b = laplace_case(r["case"], r["ny"], r["nx"], seed=11, dtype=built)
    L = np.array(L, f64).reshape(r["ny"], r["nx"], 5)
    b = np.array(b, f64).reshape(r["ny"], r["nx"])
    if "U" in r["cls"]:
        L[1::2] *= 2.0
        b[1::2] *= 2.0
    if "C" in r["cls"]:
        L = L * (1.0 / 3.0)
        b = b * (1.0 / 3.0)
    return s, np.ascontiguousarray(L.reshape(-1, 5)), np.ascontiguousarray(b.reshape(-1))


def offset_view(t, offset):
    """A copy of t that starts `offset` ELEMENTS behind a 256-byte aligned address (offset 1: element-aligned only - a valid input)."""
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == offset * t.element_size()
    return v


def solve(s, L_t, b_t, tol, max_it, shift, reset, offset=0):
    """piso_cg_solve_f64 / _f32 through the C ABI -> (x, iterations, dispatch record)."""
    from diffpiso import _native as N
    nx, ny = s.nx, s.ny
    px, py = s.periodic_yx[1], s.periodic_yx[0]
    elem = L_t.element_size()
    b_v = offset_view(b_t, offset)
    x_v = offset_view(torch.full_like(b_t, float("nan")), offset)
    ws = N.workspace(N.lib.piso_cg_workspace_bytes(nx, ny, elem), b_t.device, "cg")
    it = C.c_int(-1)
    fn = N.lib.piso_cg_solve_f64 if elem == 8 else N.lib.piso_cg_solve_f32
    st = fn(nx, ny, int(px), int(py), N.ptr(L_t), N.ptr(b_v), N.ptr(x_v), C.c_float(tol), int(max_it), int(bool(shift)), int(reset),
            C.byref(it), N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr())
    N.check(st, "piso_cg_solve")
    torch.cuda.synchronize()
    return x_v.clone(), it.value, N.cg_last_dispatch()


def assert_record(rec, expect, what):
    got = {k: rec[k] for k in expect}
    assert got == expect, "%s: dispatched to %r, expected %r" % (what, {k: v for k, v in got.items() if v != expect[k]},
                                                                  {k: v for k, v in expect.items() if v != got[k]})


def oracle(s, L, b, tol, max_it, shift, reset, dtype):
    return O.cg_solve(s.nx, s.ny, s.periodic_yx[1], s.periodic_yx[0], L, b, tol, max_it, shift, reset, dtype=dtype)


def true_residual(s, L, b, x, shift):
    """max |b - (L + c 1 1^T) x| in torch fp64 on the host (c: the reference's shift, 0.1 * sum|diag| / cells - cg_kernels.h: cg_init)."""
    ny, nx = s.ny, s.nx
    py, px = s.periodic_yx
    Lt = torch.as_tensor(L, dtype=torch.float64).reshape(ny, nx, 5)
    xt = torch.as_tensor(x, dtype=torch.float64).reshape(ny, nx)

    def nb(dj, di):
        y = torch.roll(xt, shifts=(-dj, -di), dims=(0, 1)).clone()
        if dj == -1 and not py: y[0] = 0
        if dj == 1 and not py: y[-1] = 0
        if di == -1 and not px: y[:, 0] = 0
        if di == 1 and not px: y[:, -1] = 0
        return y
    Ax = Lt[..., 0] * nb(-1, 0) + Lt[..., 1] * nb(0, -1) + Lt[..., 2] * xt + Lt[..., 3] * nb(0, 1) + Lt[..., 4] * nb(1, 0)
    if shift:
        Ax = Ax + Lt[..., 2].abs().sum() * (0.1 / (nx * ny)) * xt.sum()
    return float((torch.as_tensor(b, dtype=torch.float64).reshape(ny, nx) - Ax).abs().max())


def setup_row(r, piso_option):
    for k, v in r["knobs"].items():
        piso_option(k, v)
    s, L, b = system(r)
    tdt = torch.float64 if r["dtype"] == f64 else torch.float32
    return s, L, b, dev(L, tdt), dev(b, tdt)


def ids(checks):
    return [r["id"] for r in ROWS if checks in r["checks"]]


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("rid", ids("T"))
def test_trajectory_matches_oracle(rid, piso_option):
    """Fixed-iteration runs on the un-shifted operator follow the oracle to round-off (1e-9 of max|x| in fp64; the float32 oracle at the
    bars of test_cg_persistent_float32_state_matches_oracle), also across residual resets (reset 10 and 7 with 23 iterations: MODE_RESET,
    the flush before it, and the INIT iteration behind it)."""
    r = ROW[rid]
    s, L, b, L_t, b_t = setup_row(r, piso_option)
    fp64 = r["dtype"] == f64
    general = "U" in r["cls"]                                # unsymmetric: CG is only an algorithm there - short runs
    runs = [(1, 1000), (2, 1000), (3, 1000), (7, 1000), (7, 3)] if general else [(1, 1000), (2, 1000), (3, 1000), (7, 1000), (23, 1000), (23, 10), (23, 7)]
    segments = 0
    for nit, reset in runs:
        x, it, rec = solve(s, L_t, b_t, 1e-30, nit, False, reset, r["offset"])
        assert_record(rec, {k: v for k, v in r["expect"].items() if k != "segments"}, "%s nit %d" % (rid, nit))
        segments += rec["segments"]
        xo, ito = oracle(s, L, b, 1e-30, nit, False, reset, r["dtype"])
        assert it == ito == nit
        bar = 1e-9 if fp64 else 2e-4
        err = np.abs(x.cpu().numpy() - xo).max()
        assert err <= bar * np.abs(xo).max(), (rid, nit, reset, err / np.abs(xo).max())
    assert (segments > 0) == (r["expect"]["path"] == 3), "persistent launches: %d" % segments


@pytest.mark.parametrize("rid", ids("K"))
def test_converged_solve_matches_oracle(rid, piso_option):
    """The converged answer, the iteration count (a 5-step test apart: the dot products are summed in another order), the reference's
    stopping cadence - and the TRUE residual of what came back, so that a wrong oracle and a wrong kernel cannot agree by accident."""
    r = ROW[rid]
    s, L, b, L_t, b_t = setup_row(r, piso_option)
    fp64 = r["dtype"] == f64
    tol, reset = (1e-9, 333) if fp64 else (1e-4, 1000)
    x, it, rec = solve(s, L_t, b_t, tol, 4000, False, reset, r["offset"])
    assert_record(rec, {k: v for k, v in r["expect"].items() if k != "segments"}, rid)
    xo, ito = oracle(s, L, b, tol, 4000, False, reset, r["dtype"])
    assert ito < 4000 and it < 4000
    assert abs(it - ito) <= max(10, (0.08 if fp64 else 0.15) * ito), (it, ito)
    assert it % 5 == 0 and it >= 10 and it % reset != 0
    x = x.cpu().numpy()
    assert np.abs(x - xo).max() <= (1e-6 if fp64 else 2e-3) * np.abs(xo).max()
    scale = 1.0 if fp64 else 30.0                             # (fp32: the recurrence residual drifts from the true one by eps32 * |L| |x|)
    assert true_residual(s, L, b, x, False) <= 10 * tol * scale


@pytest.mark.parametrize("rid", ids("S"))
def test_rank_one_shift_matches_oracle(rid, piso_option):
    """With the rank-1 shift the operator is indefinite and iteration counts are not reproducible between summation orders (see
    test_cg_rank_deficient_shift): the first three iterations at round-off, then the converged answer, its zero mean, the stopping
    cadence and the true residual of the SHIFTED system."""
    r = ROW[rid]
    s, L, b, L_t, b_t = setup_row(r, piso_option)
    assert s.rank_deficient and r["dtype"] == f64
    for nit in (1, 2, 3):
        x, it, rec = solve(s, L_t, b_t, 1e-30, nit, True, 1000, r["offset"])
        assert_record(rec, {k: v for k, v in r["expect"].items() if k != "segments"}, "%s nit %d" % (rid, nit))
        xo, ito = oracle(s, L, b, 1e-30, nit, True, 1000, f64)
        assert np.abs(x.cpu().numpy() - xo).max() <= 1e-9 * np.abs(xo).max(), nit
    tol, reset = 1e-9, 1000
    x, it, rec = solve(s, L_t, b_t, tol, 6000, True, reset, r["offset"])
    xo, ito = oracle(s, L, b, tol, 6000, True, reset, f64)
    assert ito < 6000 and it < 6000 and it % 5 == 0 and it >= 10 and it % reset != 0
    x = x.cpu().numpy()
    assert np.abs(x - xo).max() <= 1e-6 * np.abs(xo).max()
    assert abs(x.mean()) <= 1e-7 * np.abs(x).max()
    assert true_residual(s, L, b, x, True) <= 10 * tol


def test_census_of_kernel_instances():
    """Pure Python, independent of test order and selection: the EXPECTED records of the table (each asserted against the card by its
    own test) and of the knob pairs cover the committed list of instance classes."""
    have = {census_key({**dict.fromkeys(CENSUS_KEY, 0), **r["expect"]}) for r in ROWS}
    have |= {census_key({**dict.fromkeys(CENSUS_KEY, 0), **e}) for _, _, _, _, pairs in KNOB_PAIRS for _, e in pairs}
    missing = [c for c in CENSUS if c not in have]
    assert not missing, missing
    assert len(set(CENSUS)) == len(CENSUS)
    extra = sorted(have - set(CENSUS))
    assert not extra, "instance classes reached by a row but not listed in CENSUS: %r" % extra


# ------------------------------------------------------------------------------------------------------------------ knobs
@pytest.mark.parametrize("rid", ["k2-periodic-72x130", "v1-cavity-70x131", "k2-cavity-72x130"])
def test_coefficient_knobs_are_bitwise_neutral(rid, piso_option):
    """cg_no_compact (off-diagonals kept in double: cg_k1<double, double, V, false>) and cg_no_recon (the diagonal read instead of
    rebuilt) on a float-exact system with a rebuildable diagonal change the instance, not one bit of the result (options.h)."""
    r = ROW[rid]
    s, L, b, L_t, b_t = setup_row(r, piso_option)
    base = r["expect"]
    x0, _, rec = solve(s, L_t, b_t, 1e-30, 23, False, 10)
    assert_record(rec, {k: base[k] for k in ("path", "sizeof_CT", "V", "RECON")}, rid)
    for knob, ct, recon in (("cg_no_compact", 8, 0), ("cg_no_recon", 4, 0)):
        piso_option(knob, 1)
        x1, _, rec = solve(s, L_t, b_t, 1e-30, 23, False, 10)
        piso_option(knob, -1)
        assert_record(rec, dict(path=2, sizeof_CT=ct, V=base["V"], RECON=recon), "%s %s" % (rid, knob))
        assert torch.equal(x0, x1), (knob, float((x0 - x1).abs().max()))
    xo, _ = oracle(s, L, b, 1e-30, 23, False, 10, f64)
    assert np.abs(x0.cpu().numpy() - xo).max() <= 1e-9 * np.abs(xo).max()


@pytest.mark.parametrize("rid", ["k2-periodic-72x130", "v1-periodic-70x131", "f32-periodic-72x132"])
def test_non_temporal_bits_are_bitwise_neutral(rid, piso_option):
    """cg_nt: non-temporal loads / stores of K1 and K2 - how memory is touched, never what is computed."""
    r = ROW[rid]
    s, L, b, L_t, b_t = setup_row(r, piso_option)
    x0, _, rec = solve(s, L_t, b_t, 1e-30, 23, False, 7)
    assert_record(rec, {k: r["expect"][k] for k in ("path", "sizeof_T", "V")}, rid)
    for bits in (1, 2, 4, 8, 15):
        piso_option("cg_nt", bits)
        x1, _, _ = solve(s, L_t, b_t, 1e-30, 23, False, 7)
        assert torch.equal(x0, x1), (bits, float((x0 - x1).abs().max()))
    xo, _ = oracle(s, L, b, 1e-30, 23, False, 7, r["dtype"])
    assert np.abs(x0.cpu().numpy() - xo).max() <= (1e-9 if r["dtype"] == f64 else 2e-4) * np.abs(xo).max()


def test_unaligned_pointers_change_the_instance_not_the_answer(piso_option):
    """The same data through 16-byte and through 8-byte aligned b / x: V = 2 against V = 1 (the strips are cut differently, so the
    partial sums are grouped differently: round-off, not bitwise)."""
    s, L, b, L_t, b_t = setup_row(ROW["k2-periodic-72x130"], piso_option)
    xa, _, ra = solve(s, L_t, b_t, 1e-30, 7, False, 1000, 0)
    xu, _, ru = solve(s, L_t, b_t, 1e-30, 7, False, 1000, 1)
    assert (ra["V"], ru["V"]) == (2, 1) and ra["path"] == ru["path"] == 2
    assert float((xa - xu).abs().max()) <= 1e-12 * float(xa.abs().max())
    # only ONE of the two pointers off the 16-byte grid is enough
    from diffpiso.solvers import cg_solve_native
    from diffpiso import _native as N
    cg_solve_native(s.nx, s.ny, True, True, L_t, offset_view(b_t, 1), 1e-30, 7, False, 1000)
    assert N.cg_last_dispatch()["V"] == 1


def test_scaled_system_has_the_solution_of_the_original(piso_option):
    """Class C is class A times 1/3 on both sides: another kernel instance (double coefficients, diagonal read), the same solution."""
    for a, c in (("k2-periodic-72x130", "c-periodic-72x130"), ("v1-periodic-70x131", "c-v1-periodic-70x131")):
        sa, La, ba, La_t, ba_t = setup_row(ROW[a], piso_option)
        sc, Lc, bc, Lc_t, bc_t = setup_row(ROW[c], piso_option)
        for nit in (2, 7):
            xa, _, ra = solve(sa, La_t, ba_t, 1e-30, nit, False, 1000)
            xc, _, rc = solve(sc, Lc_t, bc_t, 1e-30, nit, False, 1000)
            assert (ra["sizeof_CT"], rc["sizeof_CT"]) == (4, 8) and (ra["RECON"], rc["RECON"]) == (1, 0)
            assert float((xa - xc).abs().max()) <= 1e-9 * float(xa.abs().max())


# (case, ny, nx, what the pair shows, ((knobs, expected record), ...)): the same system under both settings of a knob that picks between
# persistent launch shapes.  The exchange adds the workgroups' records in workgroup order, so a shape with other workgroups groups the dot
# products differently: equal to round-off, NOT bitwise (options.h names these knobs).
KNOB_PAIRS = [
    ("periodic", 256, 256, "cg_persist_half",
     (((("cg_persist_half", 0), ("cg_persist_nq", 0)), per(8, 4, 1, 1, 2, 2, 8, 128, xcd_local=1)),
      ((("cg_persist_half", 1), ("cg_persist_nq", 0)), per(8, 4, 1, 1, 2, 2, 4, 256, xcd_local=1)))),
    ("xper_ywall", 256, 512, "cg_persist_half",
     (((("cg_persist_half", -1), ("cg_persist_nq", 0)), per(8, 4, 1, 1, 2, 2, 8, 256, xcd_local=1)),      # automatic: 32 full workgroups stay on one XCD
      ((("cg_persist_half", 1), ("cg_persist_nq", 0)), per(8, 4, 1, 1, 2, 2, 4, 64)))),
    ("periodic", 64, 512, "cg_xcd_local",
     (((("cg_xcd_local", 1),), per(8, 4, 1, 1, 2, 1, 8, 128, xcd_local=1)),
      ((("cg_xcd_local", 0),), per(8, 4, 1, 1, 2, 1, 8, 16)))),
    ("periodic", 256, 256, "cg_xcd_local",
     (((("cg_xcd_local", 1),), per(8, 4, 1, 1, 2, 1, 8, 256, xcd_local=1)),
      ((("cg_xcd_local", 0),), per(8, 4, 1, 1, 2, 1, 8, 32)))),
    ("cavity", 256, 512, "cg_persist_nq",
     (((("cg_persist_nq", 0), ("cg_xcd_local", 0), ("cg_persist_half", 0)), per(8, 4, 1, 1, 2, 2, 8, 32)),
      ((("cg_persist_nq", 1), ("cg_xcd_local", 0)), per(8, 4, 1, 1, 2, 1, 8, 64)))),
]
BITWISE = {"cg_persist_half": False, "cg_xcd_local": False, "cg_persist_nq": False}


@pytest.mark.parametrize("case,ny,nx,knob,pairs", KNOB_PAIRS, ids=["%s-%dx%d-%s" % p[:4] for p in KNOB_PAIRS])
def test_persistent_workgroup_knobs(case, ny, nx, knob, pairs, piso_option):
    from diffpiso import _native as N
    s, L, b = laplace_case(case, ny, nx, seed=11)
    L_t, b_t = dev(L), dev(b)
    xs = []
    for knobs, expect in pairs:
        for k, v in knobs:
            piso_option(k, v)
        x, it, rec = solve(s, L_t, b_t, 1e-30, 23, False, 10)
        for k, _ in knobs:
            N.set_option(k, -1)
        assert_record(rec, expect, "%s %r" % (knob, knobs))
        assert rec["segments"] > 0
        xs.append(x)
    xo, _ = oracle(s, L, b, 1e-30, 23, False, 10, f64)
    for x in xs:
        assert np.abs(x.cpu().numpy() - xo).max() <= 1e-9 * np.abs(xo).max()
    assert float((xs[0] - xs[1]).abs().max()) <= 1e-12 * float(xs[0].abs().max())
    assert torch.equal(xs[0], xs[1]) == BITWISE[knob], "options.h says which knobs regroup sums: %s does%s" % (knob, " not" if BITWISE[knob] else "")


def test_natural_16_rows_per_wave_and_capped_grid():
    """One row over 2048^2-class grids nothing tiles any more: 2064 x 4096 (129 groups of 16 rows - not a multiple of 8, so no 16-row
    regions; too many regions of 2 / 4 rows) iterates on the two-kernel path with 16 rows per wave and K1's grid at its cap, every block
    walking more than one tile - with no knob set.  12 iterations against the oracle un-shifted, two with the rank-1 shift: at 8.4 M cells
    every shifted iteration multiplies the round-off in the constant mode by c N alpha ~ 1e6 (see test_cg_rank_deficient_shift) and the
    third already has it in alpha through c sum(p)^2 - two summation orders then differ by 1e-6, the oracle's own two included."""
    from diffpiso import _native as N
    from diffpiso.solvers import cg_solve_native
    ny, nx = 2064, 4096
    L_t, b_t = pressure_system(nx, ny, seed=3)
    L, b = L_t.cpu().numpy(), b_t.cpu().numpy()
    for shift, nit in ((False, 12), (True, 2)):
        x, it = cg_solve_native(nx, ny, True, True, L_t, b_t, 1e-30, nit, shift, 1000)
        assert_record(N.cg_last_dispatch(), two(8, 4, 2, 1, rows_per_wave=16, k1_tiles=1056, k1_grid=1024, k2_grid=2048), "2064 x 4096")
        xo, ito = O.cg_solve_omp(nx, ny, True, True, L, b, 1e-30, nit, shift, 1000)
        assert it == ito == nit
        assert float(np.abs(x.cpu().numpy() - xo).max()) <= 1e-9 * float(np.abs(xo).max()), (shift, nit)
