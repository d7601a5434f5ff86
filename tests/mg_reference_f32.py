"""numpy twin of the float32 V-cycle under the fp64 PCG (csrc/mg_f32.h; cycle_dtype=torch.float32), written from the definition and not
from the kernels.  Constants, refusals and the outer iteration are those of tests/mg_reference.py.

  level 0      fl32 of the level-0 arrays of the fp64 set-up (couplings into absent cells dropped)
  level l + 1  fl32(S_GALERKIN P^T A_l P), accumulated in float64 from the float32 entries of level l and rounded once per entry; the
               GUARD rule is evaluated on the float64 accumulations
  dinv         fl32(OMEGA / (float64) diag32), 0 on absent cells
  cycle        input fl32(r); every operation in float32 in the order of the kernels - the stencil sums S, W, C, E, N; a sweep is
               z1 + dinv (r - A z1); the restriction adds the four cells of an aggregate over (dj, di); the prolongation is added before
               the stencil of the first post-sweep - so the GPU and this twin can agree bit for bit
  outer PCG    float64 (pcg_mixed): x, r, p, q, the level-0 operator, every sum; (r, z) from the float64 r and the widened z

The hierarchy is stored as five arrays [ny, nx] per level (S, W, C, E, N), not as scipy matrices.  `Hierarchy32.cycle(r, dtype=np.float64)`
evaluates the same cycle on the same float32 hierarchy in float64: what the rounding of the cycle's arithmetic is measured against."""
import numpy as np

from tests import mg_reference as M

F32 = np.float32


def _shift(a, s):
    """the value of `a` at the neighbour of slot s (S, W, C, E, N) of every cell, with wrap"""
    if s == 2:
        return a
    return np.roll(a, {0: 1, 1: 1, 3: -1, 4: -1}[s], axis=0 if s in (0, 4) else 1)


def _apply(c, v):
    """A v in the summation order of the kernels; the dtype of v decides the arithmetic"""
    t = c[0].astype(v.dtype) * _shift(v, 0)
    for s in range(1, 5):
        t = t + c[s].astype(v.dtype) * _shift(v, s)
    return t


def _pad_even(a):
    ny, nx = a.shape
    return np.pad(a, ((0, ny & 1), (0, nx & 1)))


class Hierarchy32(object):
    def __init__(self, L, nx, ny, per_x, per_y):
        M.matrix(L, nx, ny, per_x, per_y)                              # (refuses a border entry in a non-periodic direction)
        L = np.asarray(L, np.float64).reshape(ny, nx, 5)
        present = L[..., 2] != 0
        if np.any((L[~present] != 0)):
            raise ValueError("a row with a zero diagonal has non-zero entries")
        self.c64 = [np.where(present & _shift(present, s), L[..., s], 0.0) for s in range(5)]     # level 0 of the outer iteration
        self.present = present
        c = [a.astype(F32) for a in self.c64]
        self.levels = []                                               # (c [5] float32, dinv float32, nx, ny)
        while True:
            diag = c[2]
            dinv = np.where(diag != 0, M.OMEGA / np.where(diag != 0, diag, F32(1)).astype(np.float64), 0.0).astype(F32)
            self.levels.append((c, dinv, nx, ny))
            nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
            if nxc < M.MIN_DIM or nyc < M.MIN_DIM or len(self.levels) == M.MAX_LEVELS:
                break
            c, nx, ny = self._coarsen(c, nx, ny), nxc, nyc

    @staticmethod
    def _coarsen(c, nx, ny):
        c64 = [a.astype(np.float64) for a in c]
        pres = c64[2] != 0
        off = [np.where(pres & _shift(pres, s), c64[s], 0.0) for s in range(5)]      # couplings into absent cells count as zero
        nyc, nxc = (ny + 1) // 2, (nx + 1) // 2
        dg, oS, oW, oE, oN, scale = (np.zeros((nyc, nxc)) for _ in range(6))
        for dj in range(2):
            for di in range(2):
                sub = lambda a: _pad_even(a)[dj::2, di::2]
                cc = sub(c64[2])
                s, w, e, n = sub(off[0]), sub(off[1]), sub(off[3]), sub(off[4])
                in_e = (2 * np.arange(nxc) + di + 1 < nx)[None, :] & (di == 0)
                in_n = (2 * np.arange(nyc) + dj + 1 < ny)[:, None] & (dj == 0)
                scale = scale + np.abs(cc)
                dg = dg + cc
                if dj == 1: dg = dg + s
                else: oS = oS + s
                if di == 1: dg = dg + w
                else: oW = oW + w
                dg = dg + np.where(in_e, e, 0.0); oE = oE + np.where(in_e, 0.0, e)
                dg = dg + np.where(in_n, n, 0.0); oN = oN + np.where(in_n, 0.0, n)
        g = M.S_GALERKIN
        dg, oS, oW, oE, oN = dg * g, oS * g, oW * g, oE * g, oN * g
        live = np.abs(dg) > M.GUARD * g * scale
        return [np.where(live, a, 0.0).astype(F32) for a in (oS, oW, dg, oE, oN)]

    def level_rows(self, l):
        """-> ([n, 5] float64 holding the float32 entries, nx, ny)"""
        c, _, nx, ny = self.levels[l]
        return np.stack([a.astype(np.float64).ravel() for a in c], axis=1), nx, ny

    def _sweep(self, c, dinv, r, z):
        return np.where(dinv != 0, z + dinv * (r - _apply(c, z)), 0).astype(r.dtype)

    def _first(self, c, dinv, r, nu):
        z1 = dinv * r
        if nu == 1:
            return z1
        z = z1 + dinv * (r - _apply(c, z1))
        for _ in range(nu - 2):
            z = self._sweep(c, dinv, r, z)
        return z

    def _cycle(self, r, nu, l, dt):
        c, dinv, nx, ny = self.levels[l]
        dinv = dinv.astype(dt)
        if l == len(self.levels) - 1:
            return self._first(c, dinv, r, M.COARSEST_SWEEPS)
        z = self._first(c, dinv, r, nu)
        res = _pad_even(np.where(dinv != 0, r - _apply(c, z), 0).astype(dt))
        rc = np.zeros(((ny + 1) // 2, (nx + 1) // 2), dt)
        for dj in range(2):
            for di in range(2):
                rc = rc + res[dj::2, di::2]
        e = self._cycle(rc, nu, l + 1, dt)
        z = z + np.where(dinv != 0, np.repeat(np.repeat(e, 2, axis=0), 2, axis=1)[:ny, :nx], 0).astype(dt)
        for _ in range(nu):
            z = self._sweep(c, dinv, r, z)
        return z

    def cycle(self, r, sweeps=2, dtype=F32):
        """z = M^-1 fl32(r), flat float64 in and out; dtype: the arithmetic of the cycle (float32: the definition; float64: the same cycle
        on the same float32 hierarchy without the rounding of its operations)."""
        _, _, nx, ny = self.levels[0]
        r32 = np.asarray(r, np.float64).reshape(ny, nx).astype(F32)
        with np.errstate(all="ignore"):
            return self._cycle(r32.astype(dtype), sweeps, 0, dtype).astype(np.float64).ravel()

    def apply0(self, x):
        """L x in float64 on level 0 of the outer iteration"""
        _, _, nx, ny = self.levels[0]
        return _apply(self.c64, np.asarray(x, np.float64).reshape(ny, nx)).ravel()


def pcg_mixed(L, b, nx, ny, per_x, per_y, accuracy, max_iterations, rank_deficient, residual_reset=1 << 30, sweeps=2, H=None):
    """-> (x, iterations): the float64 outer loop of mg_reference.pcg around the float32 cycle."""
    H = H or Hierarchy32(L, nx, ny, per_x, per_y)
    present = H.present.ravel().astype(np.float64)
    npres = present.sum()
    b = np.asarray(b, np.float64).ravel()
    mean_b = (b * present).sum() / npres if rank_deficient else 0.0
    bp = present * (b - mean_b)
    x, r, p = np.zeros_like(bp), bp.copy(), np.zeros_like(bp)
    rz_old, it = 0.0, max_iterations
    for k in range(max_iterations):
        restart = k > 0 and (k + 1) % residual_reset == 0
        if restart:
            r = present * (bp - H.apply0(x))
        z = H.cycle(r, sweeps)
        rz = float(r @ z)
        beta = rz / rz_old if (k > 0 and not restart and rz_old != 0) else 0.0
        p = z + beta * p
        q = H.apply0(p)
        pq = float(p @ q)
        alpha = rz / pq if pq != 0 else 0.0
        x = x + alpha * p
        r = r - alpha * q
        rz_old = rz
        if np.abs(r).max() < accuracy:            # (False for NaN)
            it = k + 1
            break
    if rank_deficient:
        c = 0.1 * np.abs(np.asarray(L, np.float64).reshape(-1, 5)[:, 2]).sum() / (nx * ny)
        x = present * (x - (x * present).sum() / npres + mean_b / (c * npres))
    return x, it
