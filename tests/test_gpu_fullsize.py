"""Full-size (BASELINE.json) checks on the GPU through size-independent properties -- the oracle is too slow at 2048^2:
manufactured solutions, true residuals, transpose identities, CSR invariants, discrete incompressibility."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 2048


@pytest.fixture(scope="module")
def problem():
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    return bench.build_problem(N, torch.device("cuda"), 1e-6, 10000, 1000)


@pytest.mark.parametrize("walls", [False, True])
def test_persistent_cg_equals_two_kernel_path_2048(walls, piso_option):
    """The persistent kernel at the benchmark size (all 256 CUs, 2048 regions exchanging perimeters and partial sums across
    the 8 XCDs) against the two-kernel iteration: same arithmetic per cell, only the summation order of the dot products
    differs, so after 150 iterations the iterates agree to round-off.  One stale halo cell or one torn exchange record would
    show up at the 1e-3 level.  Repeated to catch timing-dependent failures."""
    from diffpiso.solvers import cg_solve_native, laplace_matrix_native
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    a0 = 0.5 + torch.rand(N * (N + 1) + (N + 1) * N, generator=g)
    a0v = a0[:N * (N + 1)].view(N + 1, N)
    a0u = a0[N * (N + 1):].view(N, N + 1)
    a0v[N] = a0v[0]
    a0u[:, N] = a0u[:, 0]
    a0 = a0.to(dev)
    act = torch.ones((N + 2, N + 2))
    if walls:                                              # closed box: the ghost frame is solid (non-periodic halo paths)
        act[0, :] = 0; act[-1, :] = 0; act[:, 0] = 0; act[:, -1] = 0
    act = act.reshape(-1).to(dev)
    L = laplace_matrix_native(N, N, act, act, a0, torch.float64)
    b = torch.randn(N * N, generator=g, dtype=torch.float64).to(dev)
    b -= b.mean()
    per = not walls
    piso_option("cg_persist", 0)
    xa, ita = cg_solve_native(N, N, per, per, L, b, 1e-30, 150, False, 1000)
    piso_option("cg_persist", 1)
    piso_option("cg_segment", 40)
    scale = float(xa.abs().max())
    # cg_persist1 (one exchange) obtains r.z' and sum r from one-step recurrences instead of dot products: algebraically equal,
    # round-off different -> the iterates separate slightly faster than with a mere change of summation order
    bound = 2e-10        # measured: 2.3e-11 (periodic), ~3e-11 (walls)
    import diffpiso._native as Nn
    f0 = Nn.lib.piso_cg_persist_fallbacks()
    for rep in range(4):
        xb, itb = cg_solve_native(N, N, per, per, L, b, 1e-30, 150, False, 1000)
        assert ita == itb == 150
        d = float((xa - xb).abs().max()) / scale
        print("persistent vs two-kernel after 150 iterations: %.2e" % d)
        assert d <= bound, rep
    assert Nn.lib.piso_cg_persist_fallbacks() == f0, "a grid exchange timed out and the solve fell back to the two-kernel path"


@pytest.mark.parametrize("shape", [(2048, 2048), (1024, 256), (512, 512), (256, 256), (512, 256)])
def test_persistent_cg_is_reproducible_bit_for_bit_from_run_to_run(shape, piso_option):
    """The exchange adds the workgroups' records of an XCD in the order of their workgroup INDEX (cg_persist.h: hier_enter), not in
    the order they happened to arrive at the launch: the same solve on the same input gives the same bits, and - the stopping test of
    the shifted system being as sensitive as it is - the same iteration count.  (By arrival order the 2048^2 benchmark's forward solves
    took 325 - 360 iterations on one input.)  Covers the 16-row instance and the one-region-per-wave instance of the mid-size grids."""
    from tests.cases import pressure_system
    from diffpiso.solvers import cg_solve_native
    nx, ny = shape
    L, b = pressure_system(nx, ny)
    piso_option("cg_persist", 1)
    piso_option("cg_xcd_map", 1)
    import diffpiso._native as Nn
    f0 = Nn.lib.piso_cg_persist_fallbacks()

    def solve(tol, nit):
        x, it = cg_solve_native(nx, ny, True, True, L, b, tol, nit, True, 1000)
        return x, it, Nn.cg_last_xcd_map()
    x0, it0, m0 = solve(1e-30, 400)
    # (256^2 and 512 x 256 run on the workgroups of ONE XCD: there the records are added in the order of the region slots, whichever XCD
    # and whichever workgroups do the work - no precondition, an empty map)
    assert (len(m0) > 0) == (nx * ny >= 512 * 512), "chip-wide launches from 512^2 cells on"
    for rep in range(3):
        x1, it1, m1 = solve(1e-30, 400)
        assert it1 == it0 == 400
        if m1 != m0:            # (the precondition: only on a GPU that somebody else uses as well)
            pytest.skip("the hardware dealt the workgroups to the XCDs differently between two launches: %d of %d differ" % (sum(u != v for u, v in zip(m0, m1)), len(m0)))
        assert torch.equal(x0, x1), "rep %d: %.3e" % (rep, float((x0 - x1).abs().max()))
    xa, ita, ma = solve(1e-3, 3000)      # (with the stopping test and a restart in play)
    xb, itb, mb = solve(1e-3, 3000)
    if ma != mb:
        pytest.skip("the hardware dealt the workgroups to the XCDs differently between two launches")
    assert ita == itb and torch.equal(xa, xb), (ita, itb)
    assert Nn.lib.piso_cg_persist_fallbacks() == f0


def test_persistent_cg_first_iterations_back_to_back_launches_2048(piso_option):
    """Short solves queued back to back (no host synchronisation in between, device copies in flight when the persistent kernel
    starts) against the two-kernel iteration after 3, 4 and 6 iterations: agreement to round-off (measured 2e-16 .. 5e-16).
    Regression for a buffer-store data hazard: a 16-byte perimeter store whose row offset sat in an SGPR was followed directly by
    a VALU write of its first data register; with the memory pipeline busy the last lanes stored the low dword of the NEW value
    (errors of 1e-12 after the third iteration, 1e-7 after the fourth - only when launches followed each other closely)."""
    from diffpiso.solvers import cg_solve_native
    import os, sys
    from tests.cases import pressure_system as case
    L, b = case(N, N)
    for nit in (3, 4, 6):
        piso_option("cg_persist", 0)
        xa, _ = cg_solve_native(N, N, True, True, L, b, 1e-30, nit, False, 1000)
        piso_option("cg_persist", 1)
        piso_option("cg_persist_r", 16)
        outs = []
        for rep in range(6):
            xb, _ = cg_solve_native(N, N, True, True, L, b, 1e-30, nit, False, 1000)
            outs.append(xb.clone())
            junk = [xb.clone() for _ in range(4)]          # keeps the copy engines / CUs busy while the next solve starts
        scale = xa.abs().max()
        errs = [float((xa - xb).abs().max() / scale) for xb in outs]
        assert max(errs) < 1e-13, (nit, errs)


def test_cg_manufactured_solution_2048():
    """b = (L + c 11^T) x_true  ->  the solver must return x_true (the shift pins the mean)."""
    from diffpiso.solvers import cg_solve_native, laplace_matrix_native
    import diffpiso._native as Nn
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    a0 = (0.5 + torch.rand(N * (N + 1) + (N + 1) * N, generator=g)).to(dev)
    a0v = a0[:N * (N + 1)].view(N + 1, N)
    a0u = a0[N * (N + 1):].view(N, N + 1)
    a0v[N] = a0v[0]
    a0u[:, N] = a0u[:, 0]                                  # periodic duplicate faces carry the same coefficient
    ones = torch.ones((N + 2) * (N + 2), device=dev)
    L = laplace_matrix_native(N, N, ones, ones, a0, torch.float64)
    Lr = L.view(N, N, 5)
    # smooth manufactured solution with zero mean (a few low modes: converges in O(10^3) iterations)
    yy, xx = torch.meshgrid(torch.arange(N, device=dev, dtype=torch.float64), torch.arange(N, device=dev, dtype=torch.float64), indexing="ij")
    xt = torch.sin(2 * np.pi * 3 * xx / N) * torch.cos(2 * np.pi * 2 * yy / N) + 0.3 * torch.sin(2 * np.pi * 5 * (xx + yy) / N)
    xt -= xt.mean()
    b = Lr[..., 0] * torch.roll(xt, 1, 0) + Lr[..., 1] * torch.roll(xt, 1, 1) + Lr[..., 2] * xt + \
        Lr[..., 3] * torch.roll(xt, -1, 1) + Lr[..., 4] * torch.roll(xt, -1, 0)
    assert float(b.sum().abs()) < 1e-6 * float(b.abs().sum())          # symmetric operator with zero row sums
    x, it = cg_solve_native(N, N, True, True, L, b, 1e-10, 20000, True, 1000)
    assert it < 20000 and it % 5 == 0
    err = float((x.view(N, N) - xt).abs().max())
    assert err < 1e-5, (err, it)
    # true residual of the returned solution, max-norm (the reference's stopping measure)
    xr = x.view(N, N)
    res = b - (Lr[..., 0] * torch.roll(xr, 1, 0) + Lr[..., 1] * torch.roll(xr, 1, 1) + Lr[..., 2] * xr +
               Lr[..., 3] * torch.roll(xr, -1, 1) + Lr[..., 4] * torch.roll(xr, -1, 0)) - 0.1 * Lr[..., 2].abs().mean() * xr.sum()
    assert float(res.abs().max()) < 1e-7
    # linearity of the solve: solve(2 b) == 2 solve(b) to solver tolerance
    x2, _ = cg_solve_native(N, N, True, True, L, 2 * b, 1e-10, 20000, True, 1000)
    assert float((x2 - 2 * x).abs().max()) < 1e-5


def test_assembly_invariants_and_transpose_identities_2048(problem):
    import diffpiso as dp
    import diffpiso._native as Nn
    P = problem
    ext = dp.Material.extrapolation_mode(P["domain"].boundaries)
    vel = dp.StaggeredGrid(P["vel_t"], P["domain"].box, extrapolation=ext)
    dev = P["vel_t"].device
    sim = P["sim"]
    beta = (2 * np.pi / N) ** 2 / P["dt"]
    val, rp, col, A, nnz, diag = dp.advection_matrix_cuda(vel, sim.dirichlet_mask_flat(dev), 1e-3, beta=beta, no_slip_wall_mask=None,
                                                          bool_periodic=(True, True), active_mask=sim.active_mask_tensor(dev),
                                                          accessible_mask=sim.accessible_mask_tensor(dev))
    n_u = (N + 1) * N
    assert list(nnz) == [5 * n_u, 5 * n_u] and int(rp[n_u]) == 5 * n_u and int(rp[-1]) == 5 * n_u   # fully periodic: 5 per row
    ru = rp[:n_u + 1].long()
    assert bool((ru[1:] - ru[:-1] == 5).all())
    cu = col[:5 * n_u].view(n_u, 5).long()
    assert bool((cu[:, 1:] > cu[:, :-1]).all())                           # columns strictly ascending in every row
    assert bool(((cu >= 0) & (cu < n_u)).all())
    # discrete conservation: row sums of M + beta I vanish for this (discretely solenoidal) field
    rs = val[:5 * n_u].view(n_u, 5).double().sum(1) + beta
    assert float(rs.abs().max()) < 2e-3 * float(val[:5 * n_u].abs().max())
    # <A x, y> == <x, A^T y>
    g = torch.Generator(device="cpu")
    g.manual_seed(3)
    x = torch.randn(2 * n_u, generator=g).to(dev)
    y = torch.randn(2 * n_u, generator=g).to(dev)
    Ax, ATy = torch.empty_like(x), torch.empty_like(y)
    Nn.check(Nn.lib.piso_csr_matvec_f32(Nn.ptr(val), Nn.ptr(rp), Nn.ptr(col), Nn.ptr(x), Nn.ptr(Ax), N, N, 0, Nn.stream_ptr()), "mv")
    Nn.check(Nn.lib.piso_csr_matvec_f32(Nn.ptr(val), Nn.ptr(rp), Nn.ptr(col), Nn.ptr(y), Nn.ptr(ATy), N, N, 1, Nn.stream_ptr()), "mvT")
    lhs, rhs = float((Ax.double() * y.double()).sum()), float((x.double() * ATy.double()).sum())
    assert abs(lhs - rhs) < 1e-6 * max(abs(lhs), float(Ax.double().norm() * y.double().norm()))
    # BiCGStab: true residual, and <A^-1 b1, b2> == <b1, A^-T b2>
    from diffpiso.solvers import multi_bicgstab_ilu_native
    warn = torch.zeros(1, dtype=torch.uint8, device=dev)
    mval = (-val).contiguous()
    s1, its1 = multi_bicgstab_ilu_native(mval, rp, col, x, torch.zeros_like(x), N, N, 1e-4, 200, False, 0, warn)
    s2, its2 = multi_bicgstab_ilu_native(mval, rp, col, y, torch.zeros_like(y), N, N, 1e-4, 200, True, 0, warn)
    assert int(warn.item()) == 0 and max(its1) < 50 and max(its2) < 50
    r = torch.empty_like(x)
    Nn.check(Nn.lib.piso_csr_matvec_f32(Nn.ptr(mval), Nn.ptr(rp), Nn.ptr(col), Nn.ptr(s1), Nn.ptr(r), N, N, 0, Nn.stream_ptr()), "mv")
    for c0, c1 in ((0, n_u), (n_u, 2 * n_u)):
        assert float((r[c0:c1] - x[c0:c1]).double().norm()) < 5e-4 * max(1.0, float(x[c0:c1].double().norm()) * 1e-3 + 1)
    lhs, rhs = float((s1.double() * y.double()).sum()), float((x.double() * s2.double()).sum())
    assert abs(lhs - rhs) < 1e-4 * float(s1.double().norm() * y.double().norm())


def test_piso_step_projects_to_discretely_divergence_free_2048(problem):
    import diffpiso as dp
    P = problem
    ext = dp.Material.extrapolation_mode(P["domain"].boundaries)
    t = P["vel_t"].clone()
    # add a divergent perturbation so the correctors have work to do
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    pert = 0.05 * torch.randn(t.shape, generator=g).to(t.device)
    pert[0, :, N, 0] = 0
    pert[0, N, :, 1] = 0
    pert[0, :N, N, 1] = pert[0, :N, 0, 1]
    pert[0, N, :N, 0] = pert[0, 0, :N, 0]
    vel = dp.StaggeredGrid(t + pert, P["domain"].box, extrapolation=ext)
    prs = dp.CenteredGrid(P["p_t"], P["domain"].box, dp.pressure_extrapolation(P["domain"].boundaries))
    inc = dp.CenteredGrid(torch.zeros_like(P["p_t"]), prs.box, prs.extrapolation)
    div0 = dp.finite_volume_divergence(vel).abs().max()
    with torch.no_grad():
        v3, pn, warn = dp.piso_step(vel, prs, inc, inc, P["dt"], P["sim"], P["sim"].dirichlet_values)
    div3 = dp.finite_volume_divergence(v3).abs().max()
    assert float(warn.sum()) == 0
    assert float(div3) < 2e-3 * float(div0), (float(div0), float(div3))
    tt = v3.staggered_tensor()
    assert torch.isfinite(tt).all() and torch.isfinite(pn.data).all()
    # periodic duplicate faces stay consistent
    assert float((tt[0, :N, N, 1] - tt[0, :N, 0, 1]).abs().max()) < 1e-4
    assert float((tt[0, N, :N, 0] - tt[0, 0, :N, 0]).abs().max()) < 1e-4


def test_persistent_solves_are_verified_against_the_true_residual(piso_option):
    """Every fp64 solve that used the persistent kernel ends with a check of r against b - A^ x (include/piso_hip.h,
    piso_cg_verify_stats): it must run, it must pass on healthy hardware, and a failed check (forced through the test knob) must
    restart the solve on the two-kernel iteration and still return the right answer."""
    import diffpiso._native as N
    from diffpiso.solvers import cg_solve_native
    import os, sys
    from tests.cases import pressure_system as case
    n = 1024
    L, b = case(n, n)
    runs0, fails0 = N.cg_verify_stats()
    fb0 = N.lib.piso_cg_persist_fallbacks()
    x1, it1 = cg_solve_native(n, n, True, True, L, b, 1e-7, 20000, True, 1000)
    runs1, fails1 = N.cg_verify_stats()
    assert runs1 == runs0 + 1 and fails1 == fails0 and N.lib.piso_cg_persist_fallbacks() == fb0
    piso_option("cg_verify", 2)
    x2, it2 = cg_solve_native(n, n, True, True, L, b, 1e-7, 20000, True, 1000)
    runs2, fails2 = N.cg_verify_stats()
    assert runs2 == runs1 + 1 and fails2 == fails1 + 1 and N.lib.piso_cg_persist_fallbacks() == fb0 + 1
    piso_option("cg_persist", 0)
    x3, it3 = cg_solve_native(n, n, True, True, L, b, 1e-7, 20000, True, 1000)
    assert it2 == it3 and float((x2 - x3).abs().max()) == 0.0           # the restarted solve IS the two-kernel solve
    assert float((x1 - x3).abs().max() / x3.abs().max()) < 1e-3          # (both stop at max|r| < 1e-7)
    assert N.cg_verify_stats()[0] == runs2                               # no persistent segment, nothing to verify
