"""numpy / scipy.sparse twin of the multigrid-preconditioned pressure CG (csrc/mg.hip), written from the algorithm's description and
not from the kernels.  It is what the GPU tests hold level operators, one V-cycle and iteration counts to, and it makes the algorithm
checkable on a machine without a GPU.

System: (L + c 1 1^T) x = b, L [N][5] = (-y, -x, diag, +x, +y) with diagonal <= 0, c = 0.1 mean|diag L| when rank_deficient, else 0.
Cells with a zero diagonal are ABSENT: x = 0 there, they join no aggregate, couplings into them are dropped on level 0 (a zero-diagonal row
with entries is refused); the present cells must be connected (cases.check_pressure_matrix).  Hierarchy: 2 x 2 aggregation (ceil), piecewise-constant
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
MAX_LEVELS = 16       # the hierarchy never has more levels than this
TAIL_CELLS = 4096     # a level of at most this many cells may open the one-workgroup tail ...
TAIL_LDS = 6144       # ... if all levels from it down hold at most this many cells together ...
TAIL_MAX_LEVELS = 8   # ... and are at most this many


def plan(nx, ny):
    """-> ([(nx, ny) of every level], tail_first): the shape of the hierarchy and the first level of the one-workgroup tail (-1: no
    level qualifies), from the header comment of csrc/mg.hip and its constants (test_mg_reference.py compares them with the text)."""
    sizes = [(nx, ny)]
    while True:
        nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
        if nxc < MIN_DIM or nyc < MIN_DIM or len(sizes) == MAX_LEVELS:
            break
        nx, ny = nxc, nyc
        sizes.append((nx, ny))
    cells = [a * b for a, b in sizes]
    for f in range(len(sizes)):
        if cells[f] <= TAIL_CELLS and sum(cells[f:]) <= TAIL_LDS and len(sizes) - f <= TAIL_MAX_LEVELS:
            return sizes, f
    return sizes, -1


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
        absent = A.diagonal() == 0
        if np.any(abs(A)[absent].sum(axis=1) != 0):
            raise ValueError("a row with a zero diagonal has non-zero entries")
        keep0 = sp.diags((~absent).astype(np.float64))
        A = (A @ keep0).tocsr(); A.eliminate_zeros()        # couplings INTO an absent cell are dropped (they multiply x = 0)
        self.levels = []                                   # (A, dinv, nx, ny, P to the next level or None)
        while True:
            d = A.diagonal()
            present = d != 0
            dinv = np.where(present, OMEGA / np.where(present, d, 1.0), 0.0)
            nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
            if nxc < MIN_DIM or nyc < MIN_DIM or len(self.levels) + 1 == MAX_LEVELS:
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

    def dead(self, l):
        """number of absent cells on level l"""
        return int((self.levels[l][1] == 0).sum())

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


def pcg(L, b, nx, ny, per_x, per_y, accuracy, max_iterations, rank_deficient, residual_reset=1 << 30, sweeps=2, history=None, H=None):
    """-> (x, iterations).  Stops when max|r| < accuracy on the recurred residual, tested after every update.  (`H`: the hierarchy
    of this matrix where the caller has it already.)"""
    H = H or Hierarchy(L, nx, ny, per_x, per_y)
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


def residuals(L, b, x, nx, ny, per_x, per_y, rank_deficient):
    """The true residual of (L + c 1 1^T) x = b in float64 on the host, in the two parts the system splits into (header: constant mode):
    -> (max over the present cells of |b - mean - L x|, |c sum(x) - mean|, the round-off floor of the second part) with mean = the mean of
    b over the present cells (0 where not rank deficient; then the second part is 0).  The floor: x is stored in float64, so sum(x)
    carries up to N eps max|x| / 2 however x was computed, and c times that exceeds 1e-10 already on a 130 x 129 grid with max|x| ~ 40;
    the bound is the one test_gpu_mg.py::test_large_grids_converge_in_tens_of_iterations holds its second part to."""
    L = np.asarray(L, np.float64).reshape(nx * ny, 5)
    b, x = np.asarray(b, np.float64).ravel(), np.asarray(x, np.float64).ravel()
    present = L[:, 2] != 0
    mean = b[present].sum() / present.sum() if rank_deficient else 0.0
    c = 0.1 * np.abs(L[:, 2]).sum() / (nx * ny) if rank_deficient else 0.0
    first = np.abs((b - mean - matrix(L, nx, ny, per_x, per_y) @ x)[present]).max()
    return first, abs(c * x.sum() - mean), 4 * c * nx * ny * np.finfo(np.float64).eps * np.abs(x).max()
