"""Shared synthetic set-ups for the parity tests (inputs only; no reference code).

Each case mirrors a configuration of BASELINE.json / the reference's scripts at test size:
  periodic      decaying turbulence, doubly periodic                       
  xper_ywall    temporally evolving mixing layer: x periodic, y walls, v Dirichlet on the walls
  cavity        lid-driven cavity incl. the solid lid row and no-slip mask   (lid_driven_cavity_2d.py:15-47)
  spatial_ml    spatially evolving mixing layer: inflow/outflow in x, open y (combined_training_integrated.py:481-539)
"""
import numpy as np

f32 = np.float32


def _vel_from_stream(ny, nx, dy, dx, rng, periodic_yx, amp=1.0):
    """Roughly solenoidal random velocity on faces (curl of a smooth random stream function on cell corners)."""
    ky, kx = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    psi = np.zeros((ny + 1, nx + 1))
    for _ in range(6):
        a, b = rng.integers(1, 4, size=2)
        ph = rng.uniform(0, 2 * np.pi, size=2)
        psi += rng.standard_normal() * np.sin(2 * np.pi * a * ky / ny + ph[0]) * np.sin(2 * np.pi * b * kx / nx + ph[1])
    u = (psi[1:, :] - psi[:-1, :]) / dy          # [ny, nx+1]
    v = -(psi[:, 1:] - psi[:, :-1]) / dx         # [ny+1, nx]
    s = amp / max(1e-12, np.sqrt(np.mean(u ** 2) + np.mean(v ** 2)))
    t = np.zeros((1, ny + 1, nx + 1, 2), f32)
    t[0, :, :nx, 0] = v * s
    t[0, :ny, :, 1] = u * s
    if periodic_yx[1]:
        t[0, :ny, nx, 1] = t[0, :ny, 0, 1]
    if periodic_yx[0]:
        t[0, ny, :nx, 0] = t[0, 0, :nx, 0]
    return t


def make_case(name, ny, nx, seed=0, viscosity=1e-2, cfl=0.5, variable_viscosity=False):
    """Returns a dict of plain numpy inputs understood by both the oracle (OracleSetup) and the product package."""
    rng = np.random.default_rng(seed)
    st = (1, ny + 1, nx + 1, 2)
    ones = np.ones((1, ny + 2, nx + 2, 1), f32)
    c = dict(name=name, ny=ny, nx=nx)
    dmask = np.zeros(st, bool)
    dvals = np.zeros(st, f32)
    no_slip = None
    if name == "periodic":
        L = 2 * np.pi
        c.update(periodic_yx=(True, True), p_ext=("periodic", "periodic"), boundaries="PERIODIC")
        active, accessible = ones.copy(), ones.copy()
        size = (L, L * nx / ny)
    elif name == "xper_ywall":
        c.update(periodic_yx=(False, True), p_ext=(("constant", "constant"), "periodic"), boundaries="(CLOSED, PERIODIC)")
        active, accessible = ones.copy(), ones.copy()
        active[0, 0], active[0, -1], accessible[0, 0], accessible[0, -1] = 0, 0, 0, 0
        dmask[0, 0, :nx, 0] = True
        dmask[0, ny, :nx, 0] = True
        size = (1.0 * ny, 1.0 * nx)
    elif name == "cavity":
        c.update(periodic_yx=(False, False), p_ext=(("boundary", "boundary"), ("boundary", "boundary")), boundaries="OPEN")
        active = np.pad(np.ones((1, ny, nx, 1), f32), ((0, 0), (1, 1), (1, 1), (0, 0)))
        active[0, -2] = 0
        accessible = active.copy()
        dmask[0, 0, :nx, 0] = True
        dmask[0, -2:, :nx, 0] = True
        dmask[0, :ny, 0, 1] = True
        dmask[0, :ny, nx, 1] = True
        dmask[0, ny - 1, :, 1] = True
        dvals[0, ny - 1, :, 1] = 1.0
        ns = np.zeros((ny + 2, nx + 2), bool)
        ns[0, :], ns[-2:, :], ns[:, 0], ns[:, -1] = True, True, True, True
        no_slip = ns.ravel()
        size = (1.0 + 1.0 / (ny - 1), 1.0 * nx / (ny - 1))
    elif name == "spatial_ml":
        c.update(periodic_yx=(False, False), p_ext=(("boundary", "boundary"), ("boundary", "constant")),
                 boundaries="((OPEN, OPEN), (OPEN, CLOSED))")
        active = np.pad(np.ones((1, ny, nx, 1), f32), ((0, 0), (1, 1), (1, 1), (0, 0)))
        accessible = ones.copy()
        accessible[0, :, 0], accessible[0, 0, :], accessible[0, -1, :] = 0, 0, 0
        dmask[0, 0, :nx, 0] = True
        dmask[0, ny, :nx, 0] = True
        dmask[0, :ny, 0, 1] = True
        prof = 0.5 * np.tanh(2.0 * (np.linspace(0, ny, ny + 2)[1:-1] - ny / 2) / (ny / 8)) + 1.0
        dvals[0, :ny, 0, 1] = prof
        no_slip = np.zeros((ny + 2) * (nx + 2), bool)
        size = (1.0 * ny, 1.0 * nx)
    else:
        raise ValueError(name)
    dy, dx = size[0] / ny, size[1] / nx
    vel = _vel_from_stream(ny, nx, dy, dx, rng, c["periodic_yx"])
    if name == "spatial_ml":
        vel[0, :ny, :, 1] += dvals[0, :ny, 0:1, 1]
    if name == "cavity":
        vel[...] *= 0.3
    vel = np.where(dmask, dvals, vel).astype(f32)
    umax = float(np.abs(vel).max())
    dt = cfl * min(dx, dy) / max(umax, 1e-6)
    visc = viscosity
    if variable_viscosity:
        n_u, n_v = (nx + 1) * ny, nx * (ny + 1)
        visc = (viscosity * (1.0 + rng.random(n_u + n_v))).astype(f32)
    p = (0.1 * rng.standard_normal((ny, nx))).astype(f32)
    c.update(dx_yx=(dy, dx), vel=vel, p=p, dt=dt, dirichlet_mask=dmask, dirichlet_values=dvals, active=active,
             accessible=accessible, no_slip=no_slip, viscosity=visc)
    return c


def oracle_setup(c, **kw):
    from oracle.piso_ref import OracleSetup
    return OracleSetup(c["nx"], c["ny"], c["dx_yx"], c["periodic_yx"], c["dirichlet_mask"], c["active"], c["accessible"],
                       no_slip=c["no_slip"], p_extrapolation=c["p_ext"], viscosity=c["viscosity"], **kw)


def product_setup(c, lin_tol=1e-5, lin_max_it=2000, lin_double=False, p_tol=1e-5, p_max_it=2000, p_reset=10, p_double=True,
                  band_rows=0, rank_deficient=None, device="cuda"):
    """The same case as oracle_setup, expressed through the product's drop-in API (diffpiso package)."""
    import torch
    import diffpiso as dp
    ny, nx = c["ny"], c["nx"]
    bnd = eval(c["boundaries"], {"PERIODIC": dp.PERIODIC, "CLOSED": dp.CLOSED, "OPEN": dp.OPEN})
    dy, dx = c["dx_yx"]
    domain = dp.Domain([ny, nx], boundaries=bnd, box=dp.box[0:dy * ny, 0:dx * nx])
    lin = dp.LinearSolverCudaMultiBicgstabILU(accuracy=lin_tol, max_iterations=lin_max_it, cast_to_double=lin_double,
                                              band_rows=band_rows)
    ps = dp.PisoPressureSolverCudaCustom(dx=[], accuracy=p_tol, max_iterations=p_max_it, residual_reset=p_reset,
                                         cast_to_double=p_double)
    if rank_deficient is not None:
        ps.laplace_rank_deficient = rank_deficient
    sim = dp.SimulationParameters(dirichlet_mask=c["dirichlet_mask"], dirichlet_values=c["dirichlet_values"],
                                  active_mask=c["active"], accessible_mask=c["accessible"],
                                  bool_periodic=c["periodic_yx"], no_slip_mask=c["no_slip"], viscosity=c["viscosity"],
                                  linear_solver=lin, pressure_solver=ps)
    dev = torch.device(device)
    vel_t = torch.tensor(c["vel"], device=dev)
    velocity = dp.StaggeredGrid.sample(vel_t, domain=domain)
    p_ext = dp.pressure_extrapolation(domain.boundaries)
    pressure = dp.CenteredGrid(torch.tensor(c["p"], device=dev)[None, :, :, None], box=domain.box, extrapolation=p_ext)
    return dict(domain=domain, sim=sim, velocity=velocity, pressure=pressure, lin=lin, ps=ps, vel_tensor=vel_t)


def dev(a, dtype=None):
    """A host array as a contiguous device tensor (optionally converted)."""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def punch_solids(c, solids):
    """Clears the cells `solids` [(j, i), ...] in the padded `active` and `accessible` masks of a case, in place, and wraps the padded
    ring on the periodic axes afterwards: the Laplace assembly reads a cell's neighbour across the seam from the ring, and a ring that
    still says "fluid" next to a solid seam cell leaves a coupling into the solid (an asymmetric matrix whose rows do not sum to zero)."""
    ny, nx = c["ny"], c["nx"]
    per_y, per_x = c["periodic_yx"]
    for m in (c["active"], c["accessible"]):
        for j, i in solids:
            assert 0 <= j < ny and 0 <= i < nx, (j, i)
            m[0, j + 1, i + 1, 0] = 0
        if per_y:
            m[0, 0], m[0, ny + 1] = m[0, ny].copy(), m[0, 1].copy()
        if per_x:
            m[0, :, 0], m[0, :, nx + 1] = m[0, :, nx].copy(), m[0, :, 1].copy()


def laplace_case(name, ny, nx, seed, dtype=np.float64, solids=None):
    """The pressure system of a case at test size, on the host: (oracle set-up, L [nx * ny, 5] from the oracle's Laplace matrix
    of random face weights in [0.5, 1.5), assembled in `dtype`; float64 right-hand side - zero-mean where the operator is rank
    deficient).  `solids`: cells [(j, i), ...] made solid first (punch_solids); the right-hand side is zero there."""
    from oracle import native as O, piso_ref as R
    c = make_case(name, ny, nx, seed=seed)
    if solids:
        punch_solids(c, solids)
    s = oracle_setup(c)
    rng = np.random.default_rng(seed)
    a0_t = np.zeros((1, ny + 1, nx + 1, 2), f32)
    a0_t[0, :, :nx, 0] = 0.5 + rng.random((ny + 1, nx))
    a0_t[0, :ny, :, 1] = 0.5 + rng.random((ny, nx + 1))
    if s.periodic_yx[1]:
        a0_t[0, :ny, nx, 1] = a0_t[0, :ny, 0, 1]
    if s.periodic_yx[0]:
        a0_t[0, ny, :nx, 0] = a0_t[0, 0, :nx, 0]
    L = O.laplace_matrix(nx, ny, s.active, s.accessible, R.flatten_staggered(a0_t, False), dtype)
    act = s.active[0, 1:-1, 1:-1, 0]
    b = rng.standard_normal((ny, nx)) * act
    if s.rank_deficient:
        b -= b.sum() / act.sum() * act
    return s, L, b.ravel()


def check_pressure_matrix(L, nx, ny, per_x, per_y, rank_deficient):
    """What every solver of the pressure system may assume of a matrix with solid cells, asserted: symmetric, no coupling from a present
    into an absent cell, no entries in a zero-diagonal row, rows that sum to zero where `rank_deficient`, and present cells that form
    exactly ONE connected component.  -> the number of absent cells."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from tests.mg_reference import matrix
    A = matrix(L, nx, ny, per_x, per_y)
    d = A.diagonal()
    present = d != 0
    scale = abs(A).max()
    assert abs(A - A.T).max() <= 1e-13 * scale, "not symmetric"
    assert A[present][:, ~present].nnz == 0, "coupling from a present into an absent cell"
    assert A[~present].nnz == 0, "a zero-diagonal row has entries"
    if rank_deficient:
        assert np.abs(A @ np.ones(nx * ny)).max() <= 1e-9 * np.abs(d[present]).mean(), "rows do not sum to zero"
    ncomp, _ = connected_components(sp.csr_matrix(A[present][:, present]), directed=False)
    assert ncomp == 1, "%d connected components of present cells" % ncomp
    return int((~present).sum())


SOLID_PATTERNS = ("none", "cell_ee", "cell_eo", "cell_oe", "cell_oo", "block2", "block4", "block8", "block2_odd", "wall", "corners",
                  "seam", "random10")
# seeds of "random10" by (ny, nx), re-drawn here until check_pressure_matrix passes on all four set-ups and no fluid cell is enclosed by
# four solids (such a cell has a zero diagonal: it would be absent with a right-hand side)
_RANDOM10_SEED = {(33, 70): 1, (130, 129): 2}


def _block(j0, i0, h, w):
    return [(j, i) for j in range(j0, j0 + h) for i in range(i0, i0 + w)]


def solid_pattern(pattern, ny, nx):
    """The named solid patterns of the multigrid tests on a grid of ny x nx: a list of (j, i).  "cell_<j parity><i parity>": one cell;
    "block<k>": k x k cells aligned to the aggregates of level log2 k (a coarse cell with no present cell on k / 2 ... levels);
    "block2_odd": 2 x 2 cells across four aggregates; "wall": one cell thick across most of the height, one gap; "corners": the four
    corner cells (one 2 x 2 block across both seams where both axes are periodic); "seam": a column on each side of the x seam;
    "random10": 10 % of the cells.  Not in SOLID_PATTERNS: "blocks_wall" (an 8 x 8 block, a 32 x 32 block and a 400-cell wall, for a grid of
    about 1030 x 520) and "pocket" (fluid enclosed by solids: what check_pressure_matrix refuses)."""
    j8, i8 = 8 * (ny // 16), 8 * (nx // 16)
    if pattern == "none":
        return []
    if pattern.startswith("cell_"):
        return [(j8 + 2 + (pattern[5] == "o"), i8 + 2 + (pattern[6] == "o"))]
    if pattern in ("block2", "block4", "block8"):
        k = int(pattern[5:])
        return _block(j8, i8, k, k)
    if pattern == "block2_odd":
        return _block(j8 + 1, i8 + 1, 2, 2)
    if pattern == "wall":
        return [(j, nx // 2 + 1) for j in range(2, ny - 2) if j != ny // 2]
    if pattern == "corners":
        return [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)]
    if pattern == "seam":
        return [(j, i) for j in range(ny // 4, ny // 2) for i in (0, nx - 1)]
    if pattern == "random10":
        rng = np.random.default_rng(_RANDOM10_SEED[(ny, nx)])
        k = rng.choice(ny * nx, size=ny * nx // 10, replace=False)
        return [(int(c) // nx, int(c) % nx) for c in np.sort(k)]
    if pattern == "blocks_wall":                           # (large grids: coarse cells with no present cell down to level 5)
        return (_block(8 * (ny // 32), 8 * (nx // 32), 8, 8) + _block(32 * (ny // 64), 32 * (nx // 64), 32, 32) +
                [(j, 3 * nx // 4 + 1) for j in range(ny // 8, ny // 8 + 401) if j != ny // 2])
    if pattern == "pocket":                                # NOT a valid pattern: 3 x 3 fluid cells enclosed by a ring of solids
        return [c for c in _block(j8 + 1, i8 + 1, 5, 5) if c not in _block(j8 + 2, i8 + 2, 3, 3)]
    raise ValueError(pattern)


def pressure_system(nx, ny, walls=False, seed=11):
    """A doubly periodic (or, walls=True, wall-bounded) pressure system at any size for the kernel-level CG tests and benchmarks:
    random A0 face weights in [0.5, 1.5) with consistent periodic duplicates (a symmetric matrix), the HIP Laplace matrix of it
    [nx * ny, 5] float64 on the device and a zero-mean right-hand side."""
    import torch
    from diffpiso.solvers import laplace_matrix_native
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    a0 = 0.5 + torch.rand(nx * (ny + 1) + (nx + 1) * ny, generator=g)
    a0v = a0[:nx * (ny + 1)].view(ny + 1, nx); a0u = a0[nx * (ny + 1):].view(ny, nx + 1)
    a0v[ny] = a0v[0]; a0u[:, nx] = a0u[:, 0]
    a0 = a0.to(dev)
    act = torch.ones((ny + 2, nx + 2))
    if walls:
        act[0, :] = 0; act[-1, :] = 0; act[:, 0] = 0; act[:, -1] = 0
    act = act.reshape(-1).to(dev)
    L = laplace_matrix_native(nx, ny, act, act, a0, torch.float64)
    b = torch.randn(nx * ny, generator=g, dtype=torch.float64).to(dev); b -= b.mean()
    return L, b


# ------------------------------------------------------------------------------------------------ full-size configurations
# (inputs of the full-size oracle fixtures, tests/golden/make_golden_configs.py, and of the GPU tests that load those fixtures)
def tml_case():
    """Config 3 inputs (also used by the GPU test): x periodic, y walls, tanh shear layer + perturbation."""
    ny, nx = 256, 512
    c = make_case("xper_ywall", ny, nx, seed=0, viscosity=1e-3)
    yy = (np.arange(ny) + 0.5) / ny
    c["vel"][0, :ny, :, 1] += np.tanh(2.0 * (yy - 0.5) * 8)[:, None].astype(f32)
    c["vel"] = np.where(c["dirichlet_mask"], c["dirichlet_values"], c["vel"]).astype(f32)
    return c


def sml_case():
    """Config 4 inputs (also used by the GPU test): spatially evolving mixing layer 1024x256 with the sponge viscosity field."""
    from diffpiso.setups import sponge_viscosity_field
    ny, nx = 256, 1024
    c = make_case("spatial_ml", ny, nx, seed=0, viscosity=2e-3)
    c["viscosity"] = sponge_viscosity_field((ny, nx), 2e-3, int(nx * 0.875), 2e-3 * 20)
    return c


CFG4_SIMPAR = dict(HRres=[256, 1024], sponge_ratio=0.875, dx_ratio=1)


def sml_network(dp, torch):
    """The closure of config 4 with seeded weights: VALID padding + restore_shape and zero buffer width
    (spatial_mixing_layer_differentiable_training.py:46,49-50,55), damped so that the forcing stays a perturbation."""
    net, weights, _ = dp.initialise_fullyconv_network([[0, 0], [0, 0]], padding="VALID", restore_shape=True, seed=1,
                                                      initialiser="normal")      # (the draw the committed fixture was made with)
    with torch.no_grad():
        for w in net.weights:
            w.mul_(0.6)
    return net


def sml_wrapper(F):
    def neural_network_wrapper(neural_network, input, fluid, physical_parameters, simulation_parameters, loss_buffer_width, buffer_width):
        # spatial_mixing_layer_differentiable_training.py:6-10: no closure inside the sponge layer
        sponge_start = int(simulation_parameters["HRres"][1] * simulation_parameters["sponge_ratio"]) // simulation_parameters["dx_ratio"]
        out = neural_network(input[:, :, :sponge_start, :])
        return F.pad(out, (0, 0, 0, int(fluid.resolution[1]) - sponge_start))
    return neural_network_wrapper
