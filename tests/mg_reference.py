"""numpy / scipy.sparse twin of the multigrid-preconditioned pressure CG (csrc/mg.hip), written from the algorithm's description and
not from the kernels.  It is what the GPU tests hold level operators, one V-cycle and iteration counts to, and it makes the algorithm
checkable on a machine without a GPU.

System: (L + c 1 1^T) x = b, L [N][5] = (-y, -x, diag, +x, +y) with diagonal <= 0, c = 0.1 mean|diag L| when rank_deficient, else 0.
Cells with a zero diagonal are ABSENT: x = 0 there, they join no aggregate.  Hierarchy: 2 x 2 aggregation (ceil), piecewise-constant
P, A_c = S_GALERKIN P^T A P, until a dimension would fall below MIN_DIM.  Cycle: V(nu, nu) damped Jacobi from a zero guess, the
coarsest level gets COARSEST_SWEEPS sweeps.  The cycle approximates L^-1 (negative definite on the present cells).
Constant mode of a rank-deficient system: L 1_present = 0, so the rank-one term only couples the means: the right-hand side is
projected (mean over the present cells removed), CG runs on L alone, and at the end x gets its present-cell mean replaced by
sum(b) / (c n_present^2), which is mean(b) / (c N) on a grid without absent cells."""
import numpy as np
import scipy.sparse as sp

S_GALERKIN = 0.5      # constant transfers under-correct by ~2 on cell-centred grids
OMEGA = 0.8           # Jacobi damping
MIN_DIM = 4           # no level has fewer cells than this in a dimension
COARSEST_SWEEPS = 16  # the coarsest level is "solved" by a FIXED number of sweeps (the cycle stays one linear operator)
GUARD = 1e-10         # a coarse diagonal this small relative to its aggregate's diagonals is round-off: the coarse cell is absent


def matrix(L, nx, ny, per_x, per_y):
    """[N][5] -> CSR, wrap where periodic.  A non-zero border entry in a non-periodic direction is refused (the solver does too)."""
    L = np.asarray(L, np.float64).reshape(ny * nx, 5)
    j, i = np.divmod(np.arange(nx * ny), nx)
    rows, cols, vals = [], [], []
    for s, (dj, di) in enumerate(((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))):
        jj, ii = j + dj, i + di
        out = (jj < 0) | (jj >= ny) | (ii < 0) | (ii >= nx)
        wrap_ok = ((ii < 0) | (ii >= nx)) & bool(per_x) | ((jj < 0) | (jj >= ny)) & bool(per_y)
        if np.any((L[:, s] != 0) & out & ~wrap_ok):
            raise ValueError("non-zero border entry in a non-periodic direction")
        keep = (L[:, s] != 0) & (~out | wrap_ok)
        rows.append(np.nonzero(keep)[0]); cols.append(((jj % ny) * nx + ii % nx)[keep]); vals.append(L[keep, s])
    n = nx * ny
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


def to_rows(A, nx, ny):
    """CSR of a 5-point operator -> [N][5] (only valid while no dimension is < 3 under wrap: MIN_DIM guarantees it)."""
    A = A.tocoo()
    out = np.zeros((nx * ny, 5))
    dj, di = A.col // nx - A.row // nx, A.col % nx - A.row % nx
    dj = np.where(dj > 1, -1, np.where(dj < -1, 1, dj)); di = np.where(di > 1, -1, np.where(di < -1, 1, di))
    slot = np.where(dj == -1, 0, np.where(dj == 1, 4, np.where(di == -1, 1, np.where(di == 1, 3, 2))))
    np.add.at(out, (A.row, slot), A.data)
    return out


class Hierarchy(object):
    def __init__(self, L, nx, ny, per_x, per_y):
        A = matrix(L, nx, ny, per_x, per_y)
        self.levels = []                                   # (A, dinv, nx, ny, P to the next level or None)
        while True:
            d = A.diagonal()
            present = d != 0
            dinv = np.where(present, OMEGA / np.where(present, d, 1.0), 0.0)
            nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
            if nxc < MIN_DIM or nyc < MIN_DIM:
                self.levels.append((A, dinv, nx, ny, None))
                break
            j, i = np.divmod(np.arange(nx * ny), nx)
            P = sp.csr_matrix((present.astype(np.float64), (np.arange(nx * ny), (j // 2) * nxc + i // 2)), shape=(nx * ny, nxc * nyc))
            Ap = sp.diags(present.astype(np.float64)) @ A @ sp.diags(present.astype(np.float64))
            Ac = (S_GALERKIN * (P.T @ Ap @ P)).tocsr()
            scale = S_GALERKIN * (P.T @ np.abs(d))
            dead = np.abs(Ac.diagonal()) <= GUARD * scale       # (exactly cancelled, or absent, aggregates)
            keep = sp.diags((~dead).astype(np.float64))
            Ac = (keep @ Ac).tocsr(); Ac.eliminate_zeros()     # a dead coarse cell's ROW is zero (its column multiplies z = 0)
            self.levels.append((A, dinv, nx, ny, P))
            A, nx, ny = Ac, nxc, nyc

    def level_rows(self, l):
        A, _, nx, ny, _ = self.levels[l]
        return to_rows(A, nx, ny), nx, ny

    def cycle(self, r, sweeps=2, l=0):
        """z = M^-1 r: one V(sweeps, sweeps) cycle from a zero guess."""
        A, dinv, nx, ny, P = self.levels[l]
        z = np.zeros_like(r)
        if P is None:
            for _ in range(COARSEST_SWEEPS):
                z = z + dinv * (r - A @ z)
            return z
        for _ in range(sweeps):
            z = z + dinv * (r - A @ z)
        z = z + P @ self.cycle(P.T @ ((dinv != 0) * (r - A @ z)), sweeps, l + 1)
        for _ in range(sweeps):
            z = z + dinv * (r - A @ z)
        return z


def pcg(L, b, nx, ny, per_x, per_y, accuracy, max_iterations, rank_deficient, residual_reset=1 << 30, sweeps=2, history=None):
    """-> (x, iterations).  Stops when max|r| < accuracy on the recurred residual, tested after every update."""
    H = Hierarchy(L, nx, ny, per_x, per_y)
    A, dinv = H.levels[0][0], H.levels[0][1]
    present = (dinv != 0).astype(np.float64)
    npres = present.sum()
    b = np.asarray(b, np.float64).ravel()
    mean_b = (b * present).sum() / npres if rank_deficient else 0.0
    bp = present * (b - mean_b)
    x, r, p = np.zeros_like(bp), bp.copy(), np.zeros_like(bp)
    rz_old, it = 0.0, max_iterations
    for k in range(max_iterations):
        restart = k > 0 and (k + 1) % residual_reset == 0
        if restart:
            r = present * (bp - A @ x)
        z = H.cycle(r, sweeps)
        rz = float(r @ z)
        beta = rz / rz_old if (k > 0 and not restart and rz_old != 0) else 0.0
        p = z + beta * p
        q = A @ p
        pq = float(p @ q)
        alpha = rz / pq if pq != 0 else 0.0
        x = x + alpha * p
        r = r - alpha * q
        rz_old = rz
        res = np.abs(r).max()
        if history is not None:
            history.append(res)
        if res < accuracy:            # (False for NaN: a NaN never counts as converged)
            it = k + 1
            break
    if rank_deficient:
        c = 0.1 * np.abs(np.asarray(L, np.float64).reshape(-1, 5)[:, 2]).sum() / (nx * ny)
        x = present * (x - (x * present).sum() / npres + mean_b / (c * npres))
    return x, it
