"""numpy twin of the multigrid PCG started from a GUESS (csrc/mg_guess.h), written from the definition and not from the kernels; the
hierarchy, the cycle and the iteration are those of tests/mg_reference.py (float32 cycle: tests/mg_reference_f32.py).

With `present` the cells of level 0 with a non-zero diagonal and b' = present (b - mean_b) as in mg_reference.pcg:
  x0~ = present x0 (by selection: a NaN on an absent cell is not read)
  r_g = present (b' - L x0~), L the level-0 operator in the summation order of the kernels' stencil (S, W, C, E, N)
  m_g = max|r_g|, m_b = max|b'|; the guess is ACCEPTED iff m_g < m_b (strict; a NaN or Inf in r_g makes the comparison false)
  accepted   x = x0~, r = r_g; m_g < accuracy: done with 0 iterations
  rejected   x = 0, r = b': mg_reference.pcg bit for bit (which always runs at least one iteration); x0 = None likewise
The iteration is pcg's: k = 0 has beta = 0, the residual is recomputed when (k + 1) % residual_reset == 0, the stopping rule is max|r| <
accuracy after every update, and the end of a rank-deficient solve replaces the mean of x over the present cells - so the mean of x0 is
immaterial (and r_g is mean-free: the columns of L sum to zero)."""
import numpy as np

from tests.mg_reference import Hierarchy


def stencil_apply(rows, v, nx, ny):
    """L v from the level's [N][5] rows, summed S, W, C, E, N with wrap (a wrapped neighbour of a non-periodic axis has a zero coefficient)"""
    v = v.reshape(ny, nx)
    c = rows.reshape(ny, nx, 5)
    t = c[..., 0] * np.roll(v, 1, axis=0)
    t = t + c[..., 1] * np.roll(v, 1, axis=1)
    t = t + c[..., 2] * v
    t = t + c[..., 3] * np.roll(v, -1, axis=1)
    t = t + c[..., 4] * np.roll(v, -1, axis=0)
    return t.ravel()


def guess_start(rows, present, bp, x0, nx, ny):
    """-> (x0~, r_g, accepted) of the definition above; `rows`: level 0 as [N][5], `present` a bool mask, bp = b'"""
    xt = np.where(present, np.asarray(x0, np.float64).ravel(), 0.0)
    with np.errstate(all="ignore"):
        rg = np.where(present, bp - stencil_apply(rows, xt, nx, ny), 0.0)
        accepted = bool(np.all(np.isfinite(rg))) and bool(np.abs(rg).max() < np.abs(bp).max())
    return xt, rg, accepted


def _iterate(cycle, apply0, present, bp, x, r, accuracy, max_iterations, residual_reset, sweeps):
    """the loop of mg_reference.pcg / mg_reference_f32.pcg_mixed from a given (x, r), statement for statement -> (x, iterations)"""
    p = np.zeros_like(bp)
    rz_old, it = 0.0, max_iterations
    for k in range(max_iterations):
        restart = k > 0 and (k + 1) % residual_reset == 0
        if restart:
            r = present * (bp - apply0(x))
        z = cycle(r, sweeps)
        rz = float(r @ z)
        beta = rz / rz_old if (k > 0 and not restart and rz_old != 0) else 0.0
        p = z + beta * p
        q = apply0(p)
        pq = float(p @ q)
        alpha = rz / pq if pq != 0 else 0.0
        x = x + alpha * p
        r = r - alpha * q
        rz_old = rz
        if np.abs(r).max() < accuracy:            # (False for NaN)
            it = k + 1
            break
    return x, it


def _solve(cycle, apply0, rows, present_f, L, b, x0, nx, ny, accuracy, max_iterations, rank_deficient, residual_reset, sweeps):
    npres = present_f.sum()
    b = np.asarray(b, np.float64).ravel()
    mean_b = (b * present_f).sum() / npres if rank_deficient else 0.0
    bp = present_f * (b - mean_b)
    x, r, accepted, it = np.zeros_like(bp), bp.copy(), False, None
    if x0 is not None:
        xt, rg, accepted = guess_start(rows, present_f != 0, bp, x0, nx, ny)
        if accepted:
            x, r = xt, rg
            if np.abs(rg).max() < accuracy:
                it = 0
    if it is None:
        x, it = _iterate(cycle, apply0, present_f, bp, x, r, accuracy, max_iterations, residual_reset, sweeps)
    if rank_deficient:
        c = 0.1 * np.abs(np.asarray(L, np.float64).reshape(-1, 5)[:, 2]).sum() / (nx * ny)
        x = present_f * (x - (x * present_f).sum() / npres + mean_b / (c * npres))
    return x, it, accepted


def pcg_guess(L, b, x0, nx, ny, per_x, per_y, accuracy, max_iterations, rank_deficient, residual_reset=1 << 30, sweeps=2, H=None):
    """-> (x, iterations, accepted): mg_reference.pcg started from x0 where the guard accepts it (x0 None: no guess)."""
    H = H or Hierarchy(L, nx, ny, per_x, per_y)
    A, dinv = H.levels[0][0], H.levels[0][1]
    return _solve(H.cycle, lambda v: A @ v, H.level_rows(0)[0], (dinv != 0).astype(np.float64), L, b, x0, nx, ny, accuracy, max_iterations,
                  rank_deficient, residual_reset, sweeps)


def pcg_guess_f32(L, b, x0, nx, ny, per_x, per_y, accuracy, max_iterations, rank_deficient, residual_reset=1 << 30, sweeps=2, H=None):
    """The same around the float32 cycle (mg_reference_f32.pcg_mixed; fl32(r_g) is what its cycle reads); H: a Hierarchy32."""
    from tests.mg_reference_f32 import Hierarchy32
    H = H or Hierarchy32(L, nx, ny, per_x, per_y)
    rows = np.stack([a.ravel() for a in H.c64], axis=1)
    return _solve(H.cycle, H.apply0, rows, H.present.ravel().astype(np.float64), L, b, x0, nx, ny, accuracy, max_iterations, rank_deficient,
                  residual_reset, sweeps)
