"""Which kernel instances does an ILU(0)-BiCGStab solve run, and is every instance, band geometry and edge the driver can pick right?

One call of piso_multi_bicgstab_ilu_* picks (csrc/bicgstab_dispatch.h: bi_plan, the one place the driver bi_solve of csrc/bicgstab.hip decides in)
  E       row elements per thread of the factorisation and the sweeps, from need = ceil((nx + 1) / 256): 1, 2, 3, 4, 5, 8, 9, 16, 32
  LDS     the LDS-staged forms of bi_sweep / bi_factor instead of the direct ones where they exist (float E = 5, 8, 9, 16; double E = 5, 8, 9) and option
          bicg_sweep_lds is not 0
  R       the band height: band_rows < 0 one band, 0 automatic (ny >= 2048: 8, >= 1024: 4, >= 256: 2, else 8), > 0 as given; clamped to ny + 1
  blocks  ceil(rows of the larger component / 1024) rounded up to 8, at most 1 024
  look0   iterations before the first host look: 1 below 32 768 rows in all, else 2; then 2, 2, 4, 8, 16 ...
BiCGStab converges to the same answer with any reasonable preconditioner, so a sweep that mishandles the last element of a row at one E or a
factorisation that keeps a coupling across a band edge only costs iterations: converged answers cannot see it.  Every row of ROWS therefore
solves through the C ABI, requires the dispatch record (piso_bicgstab_last_dispatch) to EQUAL an expectation written here from the dispatch
code - not read back from the card - and compares EARLY ITERATES and ITERATION COUNTS with the C oracle running the same drop mask.

Checks a row names:
  K  early iterates: x_k for a few k through the public ABI (max_it = k and a tolerance, chosen from the oracle's norm history, that no
     component reaches before k and that ||r_k|| is within 100 times of - otherwise the failure path would zero x)
  T  tolerance ladder: iteration counts per component equal the oracle's at tolerances its stopping decision has a 3 % margin on
  C  converged answer against the oracle WITHOUT drop mask (the reference's ILU(0)) and the true residual b - A x recomputed in numpy fp64
  R  restart path: a component above 100 tol is zeroed and run again alone; twice above: returned as zeros (failed_mask)
The CPU-only tests at the end hold every row's oracle-side premises (counts, margins, non-zero x) and restate the expected record in plain
Python, so the table can be debugged without a card and a row cannot silently stop exercising what it claims.

Regimes: "easy" is the suite's usual cfl 0.5 / viscosity 1e-2 (3 - 6 iterations), "hard" is cfl 6 / viscosity 0.5: the oracle needs 10 - 25
iterations and the off-diagonal part of L and U and the band cuts carry weight.  Tolerances are the usual absolute ones times
max(1, ||rhs|| / 28) - the norm of the right-hand side at 21 x 18 - so that wide grids are asked for the same relative accuracy.

Bars.  fp64: ||x - x_oracle|| <= 1e-9 ||x_oracle||, counts equal.  fp32: two float32 evaluations of the same iterate that add their dot
products and scan their rows in another order are each about as far from the exact iterate as the other; the distance of the float32
ORACLE's iterate from the float64 oracle's is measured on the spot and the card is allowed four times that plus the suite's 2e-5:
||x - x_o64|| <= 2e-5 ||x_o64|| + 4 ||x_o32 - x_o64||.  A wrong coefficient moves an early iterate by 1e-2 or more (see the pull request's
sensitivity runs), far outside either bar.
"""
import functools
import math

import numpy as np
import pytest

from oracle import native as O, piso_ref as R
from tests.cases import dev, make_case, oracle_setup

f32, f64 = np.float32, np.float64
CASES = ("periodic", "xper_ywall", "cavity", "spatial_ml")
REGIME = {"easy": dict(cfl=0.5, viscosity=1e-2), "mid": dict(cfl=2.0, viscosity=0.1), "hard": dict(cfl=6.0, viscosity=0.5)}
E_LADDER = (1, 2, 3, 4, 5, 8, 9, 16, 32)
# (sizeof T, E) that have LDS-staged bi_sweep / bi_factor instances: bi_lds_instance - four (factor: five) staged rows of E * 256 + E * 8 elements in 96 KB
LDS_FORMS = {(4, 5), (4, 8), (4, 9), (4, 16), (8, 5), (8, 8), (8, 9)}
K_DEFAULT = (1, 2, 3, 5, 7)           # 7: past the first doubling of the look cadence (looks after 2, 4, 6 / 1, 3, 5, 7 iterations)


def row(id, case, ny, nx, E, R_, blocks, look0, dtype=f64, band=0, tr=0, regime="hard", checks="KT", knobs=(), ks=K_DEFAULT, seed=7, **special):
    """tr: the ABI's transpose flags (bit 0 A^T, bit 1: the caller passes +val and the kernel negates).  special: rhs_u / x0_u scale the u
    component of the right-hand side / the initial guess (restart rows), tol / max_it fix a restart row's solve."""
    sizeof = 8 if dtype == f64 else 4
    lds_off = dict(knobs).get("bicg_sweep_lds", -1) == 0
    lds = int((sizeof, E) in LDS_FORMS and not lds_off)
    expect = dict(sizeof_T=sizeof, E=E, sweep_lds=lds, factor_lds=lds, R=R_, bands_u=-(-ny // R_), bands_v=-(-(ny + 1) // R_), blocks=blocks,
                  fold=int(dict(knobs).get("bicg_fold", -1) != 0), fuse_p=int(dict(knobs).get("bicg_fuse_p", -1) != 0), transpose_flags=tr, slab=0,
                  look0=look0)
    return dict(id=id, case=case, ny=ny, nx=nx, dtype=dtype, band=band, tr=tr, regime=regime, checks=checks, knobs=dict(knobs), ks=tuple(ks), seed=seed,
                all_ks=special.pop("all_ks", False), special=special, expect=expect)


ROWS = []
# ---- 1. every E, both fits: at each boundary of the `need` ladder the largest nx of one instance and the smallest of the next.  The u rows
# (W = nx + 1) and the v rows (W = nx) sit on opposite sides of "exactly fills the threads", so the full row and the one-element tail are both
# hit.  (nx, E, ny, blocks): blocks = ceil(rows of the LARGER component / 1024) rounded up to 8 (v is the larger one when ny < nx)
for nx, E, ny, blocks in ((255, 1, 24, 8), (256, 2, 23, 8), (511, 2, 16, 16), (512, 3, 17, 16), (767, 3, 12, 16), (768, 4, 13, 16), (1023, 4, 10, 16),
                          (1024, 5, 11, 16), (1279, 5, 9, 16), (1280, 8, 10, 16), (2047, 8, 8, 24), (2048, 9, 9, 24), (2303, 9, 8, 24),
                          (2304, 16, 9, 24), (4095, 16, 8, 40), (4096, 32, 9, 40), (8191, 32, 8, 72)):
    cases = CASES[(nx + E) % 4], CASES[(nx + E + 1) % 4], CASES[(nx + E + 2) % 4]
    neg = 2 if nx in (255, 511, 767, 1023, 1279, 2047, 2303, 4095, 8191) else 0             # bit 1 (negated values) on one nx of every E
    ROWS += [row("e%d-%d-f64" % (E, nx), cases[0], ny, nx, E, 8, blocks, 1 if 2 * nx * ny + nx + ny < 32768 else 2),
             row("e%d-%d-f64-t" % (E, nx), cases[1], ny, nx, E, 8, blocks, 1 if 2 * nx * ny + nx + ny < 32768 else 2, tr=1 | neg),
             row("e%d-%d-f32%s" % (E, nx, "-t" if nx % 2 else ""), cases[2], ny, nx, E, 8, blocks, 1 if 2 * nx * ny + nx + ny < 32768 else 2, dtype=f32,
                 tr=(nx % 2) | neg, ks=(1, 2, 3))]
    if E in (5, 8, 9, 16):                                                                    # the plain kernels where the LDS forms are the default
        ROWS += [row("e%d-%d-f64-nolds" % (E, nx), cases[1], ny, nx, E, 8, blocks, 1 if 2 * nx * ny + nx + ny < 32768 else 2, tr=(nx + 1) % 2,
                     knobs=(("bicg_sweep_lds", 0),), ks=(1, 2, 3)),
                 row("e%d-%d-f32-nolds" % (E, nx), cases[0], ny, nx, E, 8, blocks, 1 if 2 * nx * ny + nx + ny < 32768 else 2, dtype=f32, tr=nx % 2,
                     knobs=(("bicg_sweep_lds", 0),), ks=(1, 2, 3))]
# ---- 3. band geometry: R divides ny (the v component, ny + 1 rows, ends in a band of ONE row) and does not; the clamp; one band; automatic
for ny in (21, 20):
    for i, (band, R_) in enumerate(((1, 1), (2, 2), (3, 3), (4, 4), (7, 7), (ny, ny), (ny + 1, ny + 1), (ny + 50, ny + 1), (-1, ny + 1), (0, 8))):
        ROWS.append(row("band%d-%dx18%s" % (band, ny, "-t" if (i + ny) % 2 else ""), CASES[(i + ny) % 4], ny, 18, 1, R_, 8, 1, band=band, tr=(i + ny) % 2))
for i, (band, R_) in enumerate(((1, 1), (2, 2), (3, 3), (4, 4), (7, 7), (12, 12), (13, 13), (62, 13), (-1, 13), (0, 8))):
    ROWS.append(row("band%d-12x1030%s" % (band, "" if i % 2 else "-t"), CASES[i % 4], 12, 1030, 5, R_, 16, 1, band=band, tr=(i + 1) % 2))
ROWS.append(row("band3-12x1030-f32", "periodic", 12, 1030, 5, 3, 16, 1, band=3, dtype=f32, ks=(1, 2, 3)))
# automatic height on narrow grids: (ny, nx, R, blocks)
for ny, nx, R_, blocks in ((255, 16, 8, 8), (256, 16, 2, 8), (1023, 24, 2, 32), (1024, 24, 4, 32), (2047, 20, 4, 48), (2048, 20, 8, 48)):
    ROWS.append(row("auto-%dx%d" % (ny, nx), "periodic" if ny % 2 else "xper_ywall", ny, nx, 1, R_, blocks, 1 if 2 * nx * ny + nx + ny < 32768 else 2,
                    tr=ny % 2, ks=(1, 2, 3), regime="mid"))
# ---- 4. smallest legal grids: W or H <= 4 makes EVERY row a frame row, and the wrap distances sit next to the near offsets - where
# bi_convert's classification and the exception table could alias
for case in CASES:
    for ny in (4, 5, 6):
        for nx in (4, 5, 6):
            t = (ny + nx + CASES.index(case)) % 2
            ROWS.append(row("small-%s-%dx%d%s" % (case, ny, nx, "-t" if t else ""), case, ny, nx, 1, 2, 8, 1, band=2, tr=t, checks="KTC", ks=(1, 2, 3, 4)))
    ROWS.append(row("small-%s-4x4-f32-t" % case, case, 4, 4, 1, 5, 8, 1, band=-1, tr=1, dtype=f32, checks="KC", ks=(1, 2)))
    ROWS.append(row("small-%s-5x4-neg" % case, case, 5, 4, 1, 3, 8, 1, band=3, tr=2, checks="KC", ks=(1, 2)))
# ---- 5. all four boundary cases at two mid shapes: states the iteration counts on the wall-bounded configurations
# (spatial_ml's hard matrices - variable viscosity, an open boundary - make BiCGStab's residual jump: transposed at 33 x 70 it rises a hundredfold
# in iteration 2, and what follows amplifies round-off to 1e-7 by k = 7; at 40 x 36 the card and the oracle were 2.4e-9 apart after 16 iterations
# and two iterations apart in float32.  No arithmetic reproduces such a trajectory to 1e-9: spatial_ml runs in the mid regime here)
for case in CASES:
    for ny, nx, blocks in ((40, 36, 8), (33, 70, 8)):
        regime = "mid" if case == "spatial_ml" else "hard"
        for tr in (0, 1):
            ROWS.append(row("mid-%s-%dx%d%s" % (case, ny, nx, "-t" if tr else ""), case, ny, nx, 1, 8, blocks, 1, tr=tr, checks="KTC", regime=regime))
            ROWS.append(row("mid-%s-%dx%d-f32%s" % (case, ny, nx, "-t" if tr else ""), case, ny, nx, 1, 8, blocks, 1, tr=tr, dtype=f32, checks="KTC",
                            ks=(1, 2, 3, 4, 5), regime=regime))
# ---- 6. many blocks: more than 1 048 576 face rows per component - the block count clamps at 1 024, blocks walk several chunks and the
# partial-sum records are full - and one grid just below
ROWS += [row("blocks-1024x1040", "periodic", 1024, 1040, 5, 4, 1024, 2, regime="easy", checks="tC"),
         row("blocks-999x1040-t", "periodic", 999, 1040, 5, 2, 1016, 2, regime="easy", checks="tC", tr=1)]
# ---- 7. look cadence: 32 767 and 33 024 rows in all, every max_it around the chunk edges, scalar stages folded or not, p fused or not
for ny, nx, look0, blocks in ((127, 128, 1, 16), (128, 128, 2, 24)):
    for tag, knobs in (("", ()), ("-nofold", (("bicg_fold", 0),)), ("-nofuse", (("bicg_fuse_p", 0),))):
        ROWS.append(row("look-%dx%d%s" % (ny, nx, tag), "periodic", ny, nx, 1, 8, blocks, look0, checks="K", knobs=knobs, ks=(1, 2, 3, 4, 5, 6, 7, 9, 17), all_ks=True))
# ---- 8. restart rows.  x0_u / x0_v: a random initial guess of that size instead of the velocity field; rhs_u = 1e8: u's residual sits eight
# decades above v's, so a tolerance v reaches leaves u above 100 tol in both passes
for dtype, tag in ((f64, "f64"), (f32, "f32")):
    ROWS += [
        # (i) u starts far away and is above 100 tol after its first pass, is zeroed and run again ALONE; v converges in its first pass
        row("restart-one-%s" % tag, "cavity", 21, 18, 1, 4, 8, 1, dtype=dtype, band=4, checks="R", x0_u=1e6, x0_v=1.0, tol=1e-3, max_it=14),
        # (ii) from a far initial guess both fail, from zero both converge
        row("restart-far-%s" % tag, "periodic", 21, 18, 1, 4, 8, 1, dtype=dtype, band=4, tr=1, checks="R", x0_u=1e7, x0_v=1e7, tol=1e-3, max_it=14),
        # (iii) u fails twice and comes back as zeros, v is untouched by it
        row("restart-twice-%s" % tag, "xper_ywall", 21, 18, 1, 4, 8, 1, dtype=dtype, band=4, checks="R", rhs_u=1e8, tol=8e-4, max_it=8),
    ]
ROW = {r["id"]: r for r in ROWS}
assert len(ROW) == len(ROWS)


def ids(check):
    return [r["id"] for r in ROWS if check in r["checks"]]


# ------------------------------------------------------------------------------------------------------------------ the system of a row
@functools.lru_cache(maxsize=4)
def system(rid):
    """-> dict: the CSR arrays as assembled (val: the solver works on -val), rhs, x0 in float64, the tolerance scale."""
    r = ROW[rid]
    c = make_case(r["case"], r["ny"], r["nx"], seed=r["seed"], variable_viscosity=(r["case"] == "spatial_ml"), **REGIME[r["regime"]])
    s = oracle_setup(c)
    beta = float(np.prod(c["dx_yx"])) / c["dt"]
    val, rp, col, _, _ = R.advection_matrix(s, c["vel"], beta)
    rhs = np.random.default_rng(11).standard_normal(s.n_u + s.n_v).astype(f32).astype(f64)
    x0 = R.flatten_staggered(c["vel"], True).astype(f64)
    sp = r["special"]
    rhs[:s.n_u] *= sp.get("rhs_u", 1.0)
    if "x0_u" in sp:
        far = np.random.default_rng(12).standard_normal(s.n_u + s.n_v)
        x0 = np.concatenate([far[:s.n_u] * sp["x0_u"], far[s.n_u:] * sp["x0_v"]])
    scale = max(1.0, float(np.linalg.norm(np.random.default_rng(11).standard_normal(s.n_u + s.n_v))) / 28.0)
    return dict(n_u=s.n_u, n_v=s.n_v, val=val, rp=rp, col=col, rhs=rhs, x0=x0, scale=scale)


def oracle(r, sy, tol, max_it, dtype=None, history=False, mask=True):
    """The C oracle on -val with the row's drop mask (mask False: none - the reference's ILU(0))."""
    dtype = dtype or r["dtype"]
    R_ = r["expect"]["R"]
    return O.multi_bicgstab_ilu((-sy["val"]).astype(dtype), sy["rp"], sy["col"], sy["rhs"].astype(dtype), sy["x0"].astype(dtype), sy["n_u"], sy["n_v"],
                                tol, max_it, bool(r["tr"] & 1), band_rows=R_ if mask else None, grid=(r["nx"], r["ny"]), dtype=dtype, history=history)


def gpu_solve(r, sy, tol, max_it):
    """piso_multi_bicgstab_ilu_f64 / _f32 through the C ABI -> (x, iterations, warning, dispatch record)."""
    import torch
    from diffpiso import _native as N
    from diffpiso.solvers import multi_bicgstab_ilu_native
    tdt = torch.float64 if r["dtype"] == f64 else torch.float32
    negate = bool(r["tr"] & 2)
    warn = torch.zeros(1, dtype=torch.uint8, device="cuda")
    val = sy["val"] if negate else -sy["val"]
    x, its = multi_bicgstab_ilu_native(dev(val, tdt), dev(sy["rp"]), dev(sy["col"]), dev(sy["rhs"], tdt), dev(sy["x0"], tdt), r["nx"], r["ny"], tol, max_it,
                                       bool(r["tr"] & 1), r["band"], warn, negate=negate)
    return x.cpu().numpy(), [int(i) for i in its], int(warn.item()), N.bicgstab_last_dispatch()


# ------------------------------------------------------------------------------------------------------------------ what the oracle says
def f32_below(v):
    """The tolerance travels as a C float: the float32 value the solver will compare with."""
    return float(np.float32(v))


def done_at(h, tol):
    """Iteration (1-based; 0: the initial residual) at which a pass with norm history h set `done`, None if it ran out of iterations."""
    return (len(h) // 2) if (len(h) and h[-1] < tol) else None


def expected_looks(look0, max_it, passes):
    """Host fetches of the scalar record, restated from the driver (csrc/bicgstab.hip BiRun::pass): passes = per pass the iteration at which each component was done (None:
    never).  A chunk of `look` iterations, then a fetch; look: look0, then 2, and doubling up to 16 from iteration 4 on."""
    looks = 0
    for done in passes:
        it, look, all_done = 0, look0, False
        while it < max_it and not all_done:
            chunk = min(max_it - it, look)
            look = 2 if look < 2 else (look * 2 if (it >= 4 and look < 16) else look)
            it += chunk
            looks += 1
            all_done = all(d is not None and d <= it for d in done)
    return looks


@functools.lru_cache(maxsize=None)
def plan_k(rid):
    """Check K: -> [(k, tol, x_k of the oracle, x_k of the float64 oracle, expected host looks)].  From ONE free-running oracle pass (tolerance
    out of reach) the norms h[0] = ||r0||, h[2i - 1] = ||s_i||, h[2i] = ||r_i|| of both components; a tolerance for k must lie below every norm
    tested before ||r_k|| (nobody stops early) and above ||r_k|| / 100 (nobody is zeroed), with a factor sqrt(2) to spare on either side.  BiCGStab's
    residual is not monotone: behind a peak there may be no such tolerance for some k > 1, and that k is left out (all_ks rows: it is an error);
    test_row_premises_hold_in_the_oracle requires k = 1 and at least three iterates of every row."""
    r, sy = ROW[rid], system(rid)
    kmax = max(r["ks"])
    hist = [h[0] for h in oracle(r, sy, 1e-30, kmax, history=True)[3]]
    out = []
    for k in r["ks"]:
        assert all(len(h) == 2 * kmax + 1 for h in hist), "%s: the free-running pass ended early" % rid
        hi = min(float(h[:2 * k].min()) for h in hist)
        lo = max(float(h[2 * k]) for h in hist) / 100.0
        if hi < 2.0 * lo and k > 1 and not r["all_ks"]:
            continue                                             # (a residual peak before k: no tolerance isolates this iterate - the next k will do)
        assert hi >= 2.0 * lo, "%s: no tolerance isolates iterate %d (||r_k|| / 100 = %.3g, smallest norm before = %.3g)" % (rid, k, lo, hi)
        tol = f32_below(math.sqrt(lo * hi))
        xo, wo, ito, ho = oracle(r, sy, tol, k, history=True)
        # the premises, on the oracle's side: exactly k iterations of ONE pass for both components, and an x that is not the failure path's zeros
        assert ito == [k, k] and not wo and all(len(h[1]) == 0 for h in ho), (rid, k, ito)
        assert np.abs(xo[:sy["n_u"]]).max() > 0 and np.abs(xo[sy["n_u"]:]).max() > 0
        x64 = xo if r["dtype"] == f64 else oracle(r, sy, tol, k, dtype=f64)[0]
        looks = expected_looks(r["expect"]["look0"], k, [[done_at(h[0], tol) for h in ho]])
        out.append((k, tol, xo, x64, looks))
    return out


T_LADDER = {f64: (1e-3, 1e-5, 1e-7, 1e-9), f32: (1e-3, 1e-5)}
# Two correct BiCGStab implementations that add their dot products in another order follow each other to round-off for a while and then
# drift: on the card, counts were 1 - 4 apart after 27 - 41 iterations (x 1e-9 .. 3e-7 apart) on rows whose every iterate up to k = 17
# agrees to 1e-9.  Counts are therefore compared where the oracle needs at most T_HORIZON iterations: a rung beyond is moved up until it is not.
T_HORIZON = 16


@functools.lru_cache(maxsize=None)
def plan_t(rid):
    """Check T: -> [(tol, x, x of the float64 oracle, iterations, expected host looks)].  Each rung of the ladder is moved up in steps of 1.17
    until the oracle's stopping decision has a margin: every norm it tested and passed over is 3 % above the tolerance, the one it stopped at 3 %
    below.  ("t" rows: one rung.)"""
    r, sy = ROW[rid], system(rid)
    ladder = T_LADDER[r["dtype"]] if "T" in r["checks"] else (1e-5,)
    out = []
    for base in ladder:
        while max(oracle(r, sy, f32_below(base * sy["scale"]), 200)[2]) > T_HORIZON:
            base *= 3.0
        for attempt in range(16):
            tol = f32_below(base * sy["scale"] * 1.17 ** attempt)
            xo, wo, ito, ho = oracle(r, sy, tol, 200, history=True)
            if all(len(h[1]) == 0 and h[0][-1] <= tol / 1.03 and (len(h[0]) == 1 or h[0][:-1].min() >= tol * 1.03) for h in ho):
                break
        else:
            raise AssertionError("%s: no tolerance near %g with a margin on the oracle's stopping decision" % (rid, base))
        assert not wo and max(ito) < 200 and np.abs(xo).max() > 0
        x64 = xo if r["dtype"] == f64 else oracle(r, sy, tol, 200, dtype=f64)[0]
        looks = expected_looks(r["expect"]["look0"], 200, [[done_at(h[0], tol) for h in ho]])
        if not any(o[3] == ito for o in out):                    # (rungs moved onto the same iterate: once)
            out.append((tol, xo, x64, ito, looks))
    return out


@functools.lru_cache(maxsize=None)
def plan_r(rid):
    """Check R: -> (tol, max_it, x, x of the float64 oracle, iterations, passes, failed_mask, expected host looks), all from the oracle's run."""
    r, sy = ROW[rid], system(rid)
    tol, max_it = f32_below(r["special"]["tol"]), r["special"]["max_it"]
    xo, wo, ito, ho = oracle(r, sy, tol, max_it, history=True)
    assert not wo
    second = [len(h[1]) > 0 for h in ho]
    xs = (xo[:sy["n_u"]], xo[sy["n_u"]:])
    failed = sum(1 << c for c in (0, 1) if second[c] and not (ho[c][1][-1] <= 100 * tol))
    for c in (0, 1):
        assert (np.abs(xs[c]).max() == 0) == bool(failed >> c & 1), "the oracle zeroes exactly what failed twice"
        # margins on every decision of the run: stop / go on at tol, fail / keep at 100 tol
        for h in ho[c]:
            if len(h):
                assert h[:-1].min() >= 1.05 * tol if len(h) > 1 else True
                assert not (tol / 1.05 < h[-1] < tol * 1.05) and not (100 * tol / 1.05 < h[-1] < 100 * tol * 1.05), (rid, c, h[-1], tol)
    passes = [[done_at(h[0], tol) for h in ho]]
    if any(second):
        passes.append([done_at(ho[c][1], tol) if second[c] else 0 for c in (0, 1)])          # (a component that passed is `done` from the start)
    x64 = xo if r["dtype"] == f64 else oracle(r, sy, tol, max_it, dtype=f64)[0]
    return tol, max_it, xo, x64, ito, 1 + int(any(second)), failed, expected_looks(r["expect"]["look0"], max_it, passes)


RESTART_PREMISE = {          # what each restart row must exercise IN THE ORACLE: (passes, failed_mask, components with iterations of two passes)
    "restart-one": (2, 0, [0]), "restart-far": (2, 0, [0, 1]), "restart-twice": (2, 1, [0]),
}


def assert_restart_premise(rid):
    r = ROW[rid]
    tol, max_it, xo, x64, ito, passes, failed, looks = plan_r(rid)
    want = RESTART_PREMISE[rid.rsplit("-", 1)[0]]
    assert (passes, failed) == want[:2], (rid, passes, failed, ito)
    for c in (0, 1):
        assert (ito[c] > max_it) == (c in want[2]), (rid, ito, max_it)
    if rid.startswith("restart-twice"):
        assert ito[0] == 2 * max_it and ito[1] < max_it and np.abs(xo[system(rid)["n_u"]:]).max() > 0


# ------------------------------------------------------------------------------------------------------------------ comparisons
def assert_record(rec, expect, what):
    got = {k: rec.get(k) for k in expect}
    assert got == expect, "%s: recorded %r, expected %r" % (what, {k: v for k, v in got.items() if v != expect[k]},
                                                         {k: v for k, v in expect.items() if v != got[k]})


def assert_close(r, x, xo, x64, what):
    if r["dtype"] == f64:
        err, bar = np.linalg.norm(x - xo), 1e-9 * np.linalg.norm(xo)
    else:
        x = x.astype(f64)
        err, bar = np.linalg.norm(x - x64), 2e-5 * np.linalg.norm(x64) + 4.0 * np.linalg.norm(xo.astype(f64) - x64)
    assert err <= bar, "%s: ||x - x_oracle|| = %.3g, bar %.3g (||x_oracle|| = %.3g)" % (what, err, bar, np.linalg.norm(x64))


def matvec64(sy, x, transpose):
    """(-val) x or (-val)^T x on the concatenated CSR in numpy float64."""
    out = np.zeros(sy["n_u"] + sy["n_v"])
    rp, col, val = sy["rp"], sy["col"], -sy["val"].astype(f64)
    nnz_u = int(rp[sy["n_u"]])
    for r0, n, k0, p in ((0, sy["n_u"], 0, rp[:sy["n_u"] + 1]), (sy["n_u"], sy["n_v"], nnz_u, rp[sy["n_u"] + 1:])):
        rows = np.repeat(np.arange(n), np.diff(p[:n + 1]))
        cols, v = col[k0:k0 + p[n]], val[k0:k0 + p[n]]
        if transpose:
            np.add.at(out, r0 + cols, v * x[r0 + rows])
        else:
            np.add.at(out, r0 + rows, v * x[r0 + cols])
    return out


# ------------------------------------------------------------------------------------------------------------------ the table on the card
@pytest.mark.gpu
@pytest.mark.parametrize("rid", ids("K"))
def test_early_iterates_match_oracle(rid, piso_option):
    r, sy = ROW[rid], system(rid)
    for k_, v in r["knobs"].items():
        piso_option(k_, v)
    for k, tol, xo, x64, looks in plan_k(rid):
        x, its, warn, rec = gpu_solve(r, sy, tol, k)
        assert_record(rec, dict(r["expect"], passes=1, host_looks=looks, failed_mask=0), "%s k %d" % (rid, k))
        assert its == [k, k] and warn == 0, (rid, k, its)
        assert_close(r, x, xo, x64, "%s k %d" % (rid, k))


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ids("T") + ids("t"))
def test_iteration_counts_match_oracle(rid, piso_option):
    r, sy = ROW[rid], system(rid)
    for k_, v in r["knobs"].items():
        piso_option(k_, v)
    for tol, xo, x64, ito, looks in plan_t(rid):
        x, its, warn, rec = gpu_solve(r, sy, tol, 200)
        assert warn == 0
        if r["dtype"] == f64:
            assert its == ito, (rid, tol, its, ito)
            assert_record(rec, dict(r["expect"], passes=1, host_looks=looks, failed_mask=0), "%s tol %g" % (rid, tol))
        else:
            assert max(abs(a - b) for a, b in zip(its, ito)) <= 1, (rid, tol, its, ito)
            assert_record(rec, dict(r["expect"], passes=1, failed_mask=0), "%s tol %g" % (rid, tol))
        assert_close(r, x, xo, x64, "%s tol %g" % (rid, tol))


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ids("C"))
def test_converged_answer_and_true_residual(rid, piso_option):
    """Against the reference's preconditioner (no drop mask) at 1e-11, and b - A x recomputed on the host: a wrong oracle and a wrong kernel
    cannot agree by accident.  The recurrence residual is below tol; the true one may differ from it by the round-off of the updates,
    a few eps ||A|| ||x|| per iteration - 1e-3 tol in float64 at these sizes, and eps32 sqrt(n) ||A||_max ||x|| in float32."""
    r, sy = ROW[rid], system(rid)
    fp64 = r["dtype"] == f64
    tol = f32_below((1e-9 if fp64 else 1e-5) * sy["scale"])
    x, its, warn, rec = gpu_solve(r, sy, tol, 300)
    assert_record(rec, dict(r["expect"], passes=1, failed_mask=0), rid)
    assert warn == 0 and max(its) < 300
    x = x.astype(f64)
    res = np.linalg.norm((sy["rhs"].astype(r["dtype"]).astype(f64) - matvec64(sy, x, r["tr"] & 1))[:sy["n_u"]]), \
        np.linalg.norm((sy["rhs"].astype(r["dtype"]).astype(f64) - matvec64(sy, x, r["tr"] & 1))[sy["n_u"]:])
    slack = 1e-3 * tol if fp64 else 8 * float(np.finfo(f32).eps) * math.sqrt(x.size) * float(np.abs(sy["val"]).max()) * float(np.abs(x).max())
    assert max(res) <= tol + slack, (rid, res, tol, slack)
    xe = oracle(r, sy, 1e-11, 400, dtype=f64, mask=False)[0]
    rel = np.linalg.norm(x - xe) / np.linalg.norm(xe)
    assert rel < (1e-7 if fp64 else 2e-5), (rid, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ids("R"))
def test_restart_path_matches_oracle(rid):
    r, sy = ROW[rid], system(rid)
    assert_restart_premise(rid)
    tol, max_it, xo, x64, ito, passes, failed, looks = plan_r(rid)
    x, its, warn, rec = gpu_solve(r, sy, tol, max_it)
    assert its == ito and warn == 0, (rid, its, ito)                                           # (the counts add up over both passes, as the oracle's)
    assert_record(rec, dict(r["expect"], passes=passes, failed_mask=failed, host_looks=looks), rid)
    n_u = sy["n_u"]
    for c, sl in enumerate((slice(0, n_u), slice(n_u, None))):
        if failed >> c & 1:
            assert not x[sl].any(), "component %d failed twice and must come back as zeros" % c
        else:
            assert np.abs(x[sl]).max() > 0
    assert_close(r, x, xo, x64, rid)


@pytest.mark.gpu
def test_nx_8192_is_refused_before_anything_is_launched():
    """A host-side check: PISO_ERR_INVALID_ARG, x untouched, no dispatch record."""
    import ctypes as C
    import torch
    from diffpiso import _native as N
    nx, ny = 8192, 4
    n = (nx + 1) * ny + nx * (ny + 1)
    val, col = torch.ones(5 * n, dtype=torch.float64, device="cuda"), torch.zeros(5 * n, dtype=torch.int32, device="cuda")
    rp = torch.arange(0, 5 * (n + 2) + 1, 5, dtype=torch.int32, device="cuda")[:n + 2].contiguous()
    rhs = torch.ones(n, dtype=torch.float64, device="cuda")
    x = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    ws = N.workspace(N.lib.piso_bicgstab_workspace_bytes(nx, ny, 8), rhs.device, "bicgstab")
    its = (C.c_int * 2)(-1, -1)
    warn = torch.zeros(1, dtype=torch.uint8, device="cuda")
    st = N.lib.piso_multi_bicgstab_ilu_f64(N.ptr(val), N.ptr(rp), N.ptr(col), N.ptr(rhs), N.ptr(rhs), N.ptr(x), nx, ny, C.c_float(1e-6), 5, 0, 0, N.ptr(warn),
                                           its, N.ptr(ws), C.c_size_t(ws.numel()), N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 1, st                                                                         # PISO_ERR_INVALID_ARG
    assert bool((x == 7.0).all()) and (its[0], its[1]) == (-1, -1) and int(warn.item()) == 0
    assert N.bicgstab_last_dispatch() == {}


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["values", "x0", "rhs"])
@pytest.mark.parametrize("rid", ["mid-cavity-40x36", "e5-1024-f32"])
def test_nan_input_sets_the_warning_as_the_oracle_does(rid, where):
    r = ROW[rid]
    sy = dict(system(rid))
    key = {"values": "val", "x0": "x0", "rhs": "rhs"}[where]
    a = sy[key].astype(f64).copy()
    a[a.size // 3] = np.nan
    sy[key] = a
    tol = f32_below(1e-5 * sy["scale"])
    xo, wo, ito = oracle(r, sy, tol, 5)
    assert wo is True
    x, its, warn, rec = gpu_solve(r, sy, tol, 5)
    assert warn == 1
    clean_x, clean_its, clean_warn, _ = gpu_solve(r, system(rid), tol, 5)
    assert clean_warn == 0


@pytest.mark.gpu
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("rid", [i for i in ROW if i.startswith("e") and i.endswith("-f64")] + [i for i in ROW if i.startswith("small-") and "f32" not in i
                                                                                                 and "neg" not in i and "-t" not in i] + ["blocks-1024x1040"])
def test_csr_matvec_over_the_table_shapes(rid, transpose):
    """piso_csr_matvec_f32 (A x and the gather form of A^T x) at every row width of the E ladder, on the smallest grids (all rows frame rows)
    and past a million rows, against the product in numpy float64: float32 products of five terms, 8 eps32 sum|a x| per row."""
    import torch
    import diffpiso._native as N
    r, sy = ROW[rid], system(rid)
    val = sy["val"].astype(f32)
    x = np.random.default_rng(3).standard_normal(sy["n_u"] + sy["n_v"]).astype(f32)
    y = torch.empty(x.size, device="cuda")
    d_val, d_rp, d_col, d_x = dev(val), dev(sy["rp"]), dev(sy["col"]), dev(x)
    N.check(N.lib.piso_csr_matvec_f32(N.ptr(d_val), N.ptr(d_rp), N.ptr(d_col), N.ptr(d_x), N.ptr(y), r["nx"], r["ny"], transpose, N.stream_ptr()), "matvec")
    want = -matvec64(dict(sy, val=val), x.astype(f64), transpose)
    mag = matvec64(dict(sy, val=-np.abs(val)), np.abs(x).astype(f64), transpose)
    err = np.abs(y.cpu().numpy().astype(f64) - want)
    assert (err <= 8 * float(np.finfo(f32).eps) * mag + 1e-30).all(), (rid, float((err / (mag + 1e-30)).max()))


# ------------------------------------------------------------------------------------------------------------------ without a card
def restated_record(r):
    """The dispatch rules of bi_plan (csrc/bicgstab_dispatch.h) in plain Python, from the row's grid and knobs alone."""
    ny, nx, band = r["ny"], r["nx"], r["band"]
    need = -(-(nx + 1) // 256)
    E = min(e for e in E_LADDER if e >= need)
    R_ = ny + 1 if band < 0 else ((8 if ny >= 2048 else 4 if ny >= 1024 else 2 if ny >= 256 else 8) if band == 0 else band)
    R_ = min(R_, ny + 1)
    gv = -(-max((nx + 1) * ny, nx * (ny + 1)) // 1024)
    gv = max(1, min(1024, (gv + 7) & ~7))
    sizeof = 8 if r["dtype"] == f64 else 4
    lds = int(E >= 5 and 4 * (E * 256 + E * 8) * sizeof <= 96 * 1024 and r["knobs"].get("bicg_sweep_lds", -1) != 0)
    flds = int(lds and 5 * (E * 256 + E * 8) * sizeof <= 96 * 1024)
    return dict(sizeof_T=sizeof, E=E, sweep_lds=lds, factor_lds=flds, R=R_, bands_u=(ny + R_ - 1) // R_, bands_v=(ny + R_) // R_, blocks=gv,
                fold=int(r["knobs"].get("bicg_fold", -1) != 0), fuse_p=int(r["knobs"].get("bicg_fuse_p", -1) != 0), transpose_flags=r["tr"], slab=0,
                look0=1 if (nx + 1) * ny + nx * (ny + 1) < 32768 else 2)


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_row_premises_hold_in_the_oracle(rid):
    """CPU only.  The literal expectation of the row equals the restated dispatch rules, and everything the GPU test of the row takes from the
    oracle exists: tolerances that isolate every k, a ladder with margins, the restart scenario the row is named after."""
    r = ROW[rid]
    assert r["expect"] == restated_record(r)
    if "K" in r["checks"]:
        plan = plan_k(rid)
        got = [p[0] for p in plan]
        assert got[0] == 1 and len(got) >= min(3, len(r["ks"])) and all(p[4] >= 1 for p in plan), (rid, got)
        assert got == list(r["ks"]) or not r["all_ks"]
    if "T" in r["checks"] or "t" in r["checks"]:
        plan = plan_t(rid)
        assert 1 <= len(plan) <= (len(T_LADDER[r["dtype"]]) if "T" in r["checks"] else 1) and all(max(p[3]) <= T_HORIZON for p in plan)
        if r["regime"] == "hard" and r["dtype"] == f64 and "T" in r["checks"]:
            assert max(plan[-1][3]) >= 6, "%s: the hard regime should need iterations: %r" % (rid, plan[-1][3])
    if "R" in r["checks"]:
        assert_restart_premise(rid)
    plan_k.cache_clear(), plan_t.cache_clear(), plan_r.cache_clear()


def test_norm_history_is_the_stopping_test_of_the_plain_oracle():
    """oracle_bicgstab_ilu_hist_* against oracle_bicgstab_ilu_* run on its own: the history of a free pass predicts, for a tolerance just above
    any of its entries, the iteration the plain function stops in and the x it returns - in both precisions, with and without a restart."""
    r, sy = ROW["mid-cavity-40x36"], system("mid-cavity-40x36")
    for dtype in (f64, f32):
        xf, wf, itf, hist = oracle(r, sy, 1e-30, 9, dtype=dtype, history=True)
        assert itf == [18, 18] and not xf.any() and all(len(h[0]) == 19 and len(h[1]) == 19 for h in hist)
        x_plain, w_plain, it_plain = oracle(r, sy, 1e-30, 9, dtype=dtype)
        assert it_plain == itf and np.array_equal(x_plain, xf)
        for c, (lo, hi) in enumerate(((0, sy["n_u"]), (sy["n_u"], sy["n_u"] + sy["n_v"]))):
            h = hist[c][0].astype(f64)
            for j in range(1, len(h)):
                if h[j] >= h[:j].min():
                    continue                                                                   # (only a new minimum can be the first norm below a tolerance)
                tol = f32_below(math.sqrt(h[j] * h[:j].min()))
                if not (h[j] < tol <= h[:j].min()):
                    continue
                x1, _, it1 = oracle(r, sy, tol, 9, dtype=dtype)
                assert it1[c] == (j + 1) // 2, (dtype, c, j, it1)
                x2, _, it2, h2 = oracle(r, sy, tol, 9, dtype=dtype, history=True)
                assert np.array_equal(x1, x2) and it1 == it2 and len(h2[c][0]) == j + 1 and len(h2[c][1]) == 0
                assert np.array_equal(h2[c][0], hist[c][0][:j + 1])


def test_census_of_kernel_instances():
    """Pure Python: the EXPECTED records of the table (each asserted against the card by the row's own test) reach all 2 x 9 instances of the
    plain kernels, all 7 LDS instances, the band heights 1, 2, 4, 8 and ny + 1, and both values of `passes`."""
    have = {(r["expect"]["sizeof_T"], r["expect"]["E"], r["expect"]["sweep_lds"], r["expect"]["factor_lds"]) for r in ROWS}
    plain = {(T, E, 0, 0) for T in (4, 8) for E in E_LADDER}
    lds = {(T, E, 1, 1) for T, E in LDS_FORMS}
    assert not (plain - have), sorted(plain - have)
    assert not (lds - have), sorted(lds - have)
    assert have == plain | lds, sorted(have - plain - lds)
    heights = {r["expect"]["R"] for r in ROWS}
    assert {1, 2, 4, 8} <= heights and any(r["expect"]["R"] == r["ny"] + 1 for r in ROWS)
    assert any(r["expect"]["bands_v"] == r["expect"]["bands_u"] + 1 for r in ROWS) and any(r["expect"]["bands_v"] == r["expect"]["bands_u"] for r in ROWS)
    assert {RESTART_PREMISE[r["id"].rsplit("-", 1)[0]][0] for r in ROWS if "R" in r["checks"]} == {2} and ids("K")      # passes 2 / 1
    assert {r["expect"]["look0"] for r in ROWS} == {1, 2} and {r["tr"] for r in ROWS} == {0, 1, 2, 3}
