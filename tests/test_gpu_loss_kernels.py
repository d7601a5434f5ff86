"""The fused loss kernels of csrc/loss.hip on the WHOLE grid (piso_loss_l2, piso_loss_strain and their gradients, reached through
`L2_field_loss(..., fused=True)` / `strain_rate_loss(..., fused=True)`) against the torch losses and their autograd.

  values            relative 3e-6 (the bound tests/test_eval_golden.py uses for these losses)
  L2 gradient       4 ulp of float32 per element against torch autograd (factor * x and torch's 2 x (factor / 2) differ by a rounding)
  strain gradient   against a float64 numpy evaluation written from the definition in SCATTER form (the kernel gathers), bound
                    8 eps32 sum |weights| per face; the inputs keep every entry's |a - b| above 1e-3 of the largest (asserted), so that no
                    sign is decided by round-off, and hold a block where prediction equals target, whose contribution is exactly zero
Grids 10 x 12, 13 x 9, 12 x 16 (ny x nx) with dy != dx, one block each; 70 x 129 takes several blocks of partials and 1100 x 1030 reaches the
launch cap, where every thread's grid-stride loop runs more than once.  Every test prints its worst ratio of the bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRIDS = [(10, 12), (13, 9), (12, 16)]
EPS32 = float(np.finfo(np.float32).eps)
VALUE_RTOL = 3e-6


def windows(ny):
    """(label, buffer_width, sponge_start)."""
    return [("none", None, 0), ("both axes", [[1, 2], [2, 1]], 0), ("sponge", [[0, 0], [3, 0]], 7), ("one row", [[4, ny - 4], [1, 1]], 0)]


def box_of(ny, nx):
    return [0.61 * ny, 0.37 * nx]                             # dy = 0.61, dx = 0.37


class Pair(object):
    """A seeded prediction (a leaf flat face vector behind a StaggeredGrid of views) and a ground-truth sequence [1, 1, ny + 1, nx + 1, 2]."""

    def __init__(self, ny, nx, seed, flat=None, truth=None):
        from diffpiso.grids import StaggeredGrid
        g = torch.Generator().manual_seed(seed)
        self.ny, self.nx, self.n_u = ny, nx, (nx + 1) * ny
        n = self.n_u + nx * (ny + 1)
        self.flat = (torch.randn(n, generator=g) if flat is None else torch.as_tensor(flat, dtype=torch.float32)).cuda().requires_grad_(True)
        self.truth = (torch.randn((1, 1, ny + 1, nx + 1, 2), generator=g) if truth is None else torch.as_tensor(truth, dtype=torch.float32)).cuda()
        u = self.flat[:self.n_u].view(1, ny, nx + 1, 1)
        v = self.flat[self.n_u:].view(1, ny + 1, nx, 1)
        self.grid = StaggeredGrid([v, u], box_of(ny, nx))

    def grad_of(self, fn, *args, **kw):
        """(value, d value / d flat) of one loss function, both as numpy."""
        self.flat.grad = None
        total, contribution = fn(torch.zeros((), device="cuda"), [[self.grid]], [self.truth], 1, *args, **kw)
        assert float(total.detach()) == float(contribution.detach())
        total.backward()
        return float(total.detach()), self.flat.grad.detach().cpu().numpy().copy()


def ulps(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)))


@pytest.mark.parametrize("shape", GRIDS + [(70, 129)])
def test_l2_value_and_gradient_match_the_torch_loss(shape):
    from diffpiso.losses import L2_field_loss
    ny, nx = shape
    worst_v = worst_g = 0.0
    for k, (label, bw, sponge) in enumerate(windows(ny)):
        P = Pair(ny, nx, 100 + k)
        v_ref, g_ref = P.grad_of(L2_field_loss, bw, 50.0, sponge)
        v_got, g_got = P.grad_of(L2_field_loss, bw, 50.0, sponge, fused=True)
        again, _ = P.grad_of(L2_field_loss, bw, 50.0, sponge, fused=True)
        assert v_got == again, "the value of two identical launches differs"
        assert v_ref > 0 and np.count_nonzero(g_ref) > 0, label
        rv, rg = abs(v_got - v_ref) / abs(v_ref) / VALUE_RTOL, ulps(g_got, g_ref) / 4.0
        worst_v, worst_g = max(worst_v, rv), max(worst_g, rg)
        assert rv <= 1.0, (label, v_got, v_ref)
        assert rg <= 1.0, (label, rg * 4.0)
        assert np.array_equal(g_got == 0, g_ref == 0), "%s: the faces outside the window differ" % label
    print("L2 %dx%d: worst value error / 3e-6 = %.3g, worst gradient error / 4 ulp = %.3g" % (ny, nx, worst_v, worst_g))


# ---------------------------------------------------------------------------------------------------------------- strain: the definition in float64
def strain_reference(u_p, v_p, u_t, v_t, dy, dx, factor):
    """u [ny][nx + 1], v [ny + 1][nx] in float64 -> (value, d value / d u_p, d value / d v_p, sum |weights| per u face, per v face, the
    three arrays of entry differences).  Every entry SCATTERS sign(difference) * weight to the faces it reads."""
    def parts(u, v):
        yy = (v[1:] - v[:-1]) / dy
        xx = (u[:, 1:] - u[:, :-1]) / dx
        off = 0.5 * ((v[1:-1, 1:] - v[1:-1, :-1]) / dx + (u[1:, 1:-1] - u[:-1, 1:-1]) / dy)
        return yy, off, xx
    d = [a - b for a, b in zip(parts(u_p, v_p), parts(u_t, v_t))]
    value = factor * (np.abs(d[0]).sum() + 2 * np.abs(d[1]).sum() + np.abs(d[2]).sum())
    out = []
    for lo, hi in (([-np.sign(x) for x in d], [np.sign(x) for x in d]), ([np.ones_like(x) for x in d], [np.ones_like(x) for x in d])):
        gu, gv = np.zeros_like(u_p), np.zeros_like(v_p)       # (lo / hi: what the entry sends to the face it subtracts / adds)
        gv[1:] += hi[0] / dy; gv[:-1] += lo[0] / dy
        gu[:, 1:] += hi[2] / dx; gu[:, :-1] += lo[2] / dx
        gv[1:-1, 1:] += hi[1] / dx; gv[1:-1, :-1] += lo[1] / dx                # (the entry counts twice: 2 * 1/2)
        gu[1:, 1:-1] += hi[1] / dy; gu[:-1, 1:-1] += lo[1] / dy
        out += [factor * gu, factor * gv]
    return value, out[0], out[1], out[2], out[3], d


def separated_inputs(ny, nx, seed, block):
    """Prediction and target (float32 staggered tensors) whose entry differences are all larger than 2e-3 of the largest - except inside
    `block` = (j0, j1, i0, i1) of cells, on whose faces prediction EQUALS target: the entries that read only those faces are exactly 0.
    Random fields, then the faces (outside the block) that a too-small entry reads are drawn again until none is left."""
    j0, j1, i0, i1 = block
    rng = np.random.RandomState(seed)
    t = rng.standard_normal((1, ny + 1, nx + 1, 2)).astype(np.float32)
    p = (t + rng.standard_normal(t.shape)).astype(np.float32)
    p_u, p_v, t_u, t_v = p[0, :ny, :, 1], p[0, :, :nx, 0], t[0, :ny, :, 1], t[0, :, :nx, 0]       # views
    p_v[j0:j1 + 1, i0:i1] = t_v[j0:j1 + 1, i0:i1]              # v faces of the block's cells
    p_u[j0:j1, i0:i1 + 1] = t_u[j0:j1, i0:i1 + 1]              # u faces
    for _ in range(200):
        d = strain_reference(*(x.astype(np.float64) for x in (p_u, p_v, t_u, t_v)), 0.61, 0.37, 1.0)[5]
        largest = max(np.abs(x).max() for x in d)
        bad_yy, bad_off, bad_xx = [(x != 0) & (np.abs(x) <= 2e-3 * largest) for x in d]
        if not (bad_yy.any() or bad_off.any() or bad_xx.any()):
            return p, t
        mu, mv = np.zeros(p_u.shape, bool), np.zeros(p_v.shape, bool)
        mv[1:] |= bad_yy; mv[:-1] |= bad_yy
        mu[:, 1:] |= bad_xx; mu[:, :-1] |= bad_xx
        mv[1:-1, 1:] |= bad_off; mv[1:-1, :-1] |= bad_off; mu[1:, 1:-1] |= bad_off; mu[:-1, 1:-1] |= bad_off
        mv[j0:j1 + 1, i0:i1] = False
        mu[j0:j1, i0:i1 + 1] = False
        p_v[mv] = t_v[mv] + rng.standard_normal(int(mv.sum())).astype(np.float32)
        p_u[mu] = t_u[mu] + rng.standard_normal(int(mu.sum())).astype(np.float32)
    raise AssertionError("no separated inputs found")


@pytest.mark.parametrize("shape", GRIDS)
def test_strain_value_matches_torch_and_gradient_matches_the_float64_definition(shape):
    from diffpiso.losses import strain_rate_loss
    ny, nx = shape
    block = (3, 8, 2, 7)                                       # cells [3, 8) x [2, 7): 5 x 5 cells where prediction equals target
    p, t = separated_inputs(ny, nx, 7, block)
    P = Pair(ny, nx, 0, flat=np.concatenate([p[0, :ny, :, 1].ravel(), p[0, :, :nx, 0].ravel()]), truth=t[None])
    factor, dy, dx = 2.0, 0.61, 0.37
    v_ref, _ = P.grad_of(strain_rate_loss, None, factor)
    v_got, g_got = P.grad_of(strain_rate_loss, None, factor, fused=True)
    again, _ = P.grad_of(strain_rate_loss, None, factor, fused=True)
    assert v_got == again
    # float64 from the definition, with the spacings the kernel is handed (float32 of dy, dx)
    u_p, v_p, u_t, v_t = (x.astype(np.float64) for x in (p[0, :ny, :, 1], p[0, :, :nx, 0], t[0, :ny, :, 1], t[0, :, :nx, 0]))
    v64, gu, gv, wu, wv, d = strain_reference(u_p, v_p, u_t, v_t, float(np.float32(dy)), float(np.float32(dx)), factor)
    nonzero = np.concatenate([np.abs(x[x != 0]).ravel() for x in d])
    assert nonzero.min() > 1e-3 * nonzero.max(), "a sign of these inputs could be decided by round-off"
    zero_entries = sum(int((x == 0).sum()) for x in d)
    j0, j1, i0, i1 = block
    assert zero_entries == 2 * (j1 - j0) * (i1 - i0) + (j1 - j0 - 1) * (i1 - i0 - 1), "the block of equal faces is not the one intended"
    rv_torch, rv_64 = abs(v_got - v_ref) / abs(v_ref) / VALUE_RTOL, abs(v_got - v64) / abs(v64) / VALUE_RTOL
    assert rv_torch <= 1.0 and rv_64 <= 1.0, (v_got, v_ref, v64)
    g_ref, w = np.concatenate([gu.ravel(), gv.ravel()]), np.concatenate([wu.ravel(), wv.ravel()])
    assert w.min() > 0
    ratio = np.abs(g_got.astype(np.float64) - g_ref) / (8 * EPS32 * w)
    assert ratio.max() <= 1.0, (int(ratio.argmax()), float(ratio.max()))
    # the faces all of whose entries lie inside the block: exactly zero, in the kernel as in the definition
    gu_got, gv_got = g_got[:P.n_u].reshape(ny, nx + 1), g_got[P.n_u:].reshape(ny + 1, nx)
    inner_u, inner_v = gu_got[j0 + 1:j1 - 1, i0 + 1:i1], gv_got[j0 + 1:j1, i0 + 1:i1 - 1]
    assert inner_u.size > 0 and inner_v.size > 0
    assert not inner_u.any() and not inner_v.any() and not gu[j0 + 1:j1 - 1, i0 + 1:i1].any() and not gv[j0 + 1:j1, i0 + 1:i1 - 1].any()
    print("strain %dx%d: value error / 3e-6 = %.3g (torch) %.3g (float64), worst gradient error / (8 eps sum|w|) = %.3g"
          % (ny, nx, rv_torch, rv_64, float(ratio.max())))


def test_strain_of_equal_fields_is_exactly_zero():
    from diffpiso.losses import strain_rate_loss
    ny, nx = 13, 9
    P = Pair(ny, nx, 3)
    with torch.no_grad():
        P.truth[0, 0, :ny, :, 1] = P.flat[:P.n_u].view(ny, nx + 1)
        P.truth[0, 0, :, :nx, 0] = P.flat[P.n_u:].view(ny + 1, nx)
    value, grad = P.grad_of(strain_rate_loss, None, 2.0, fused=True)
    assert value == 0.0 and not grad.any()


def test_values_at_the_launch_cap():
    """1100 x 1030: more than 2048 blocks' worth of faces and cells - the grid is capped at 2048 blocks of partials, the one-workgroup
    reduction walks all of them and every thread's loop runs more than once."""
    from diffpiso.losses import L2_field_loss, strain_rate_loss
    ny, nx = 1100, 1030
    assert ny * nx > 2048 * 512
    P = Pair(ny, nx, 17)
    for name, fn, args in (("L2", L2_field_loss, ([[1, 2], [2, 1]], 50.0, 0)), ("strain", strain_rate_loss, (None, 2.0))):
        v_ref, g_ref = P.grad_of(fn, *args)
        v_got, g_got = P.grad_of(fn, *args, fused=True)
        r = abs(v_got - v_ref) / abs(v_ref) / VALUE_RTOL
        print("%s 1100x1030: value error / 3e-6 = %.3g" % (name, r))
        assert r <= 1.0, (name, v_got, v_ref)
        if name == "L2":
            assert ulps(g_got, g_ref) <= 4.0
        else:                                                  # random inputs: a sign may flip where an entry difference is at round-off level
            assert np.mean(np.abs(g_got - g_ref) > 8 * EPS32 * 6 * 2.0 / 0.37) < 1e-3


def test_fused_losses_refuse_host_tensors_and_bad_windows():
    from diffpiso import _native as N
    from diffpiso.grids import StaggeredGrid
    from diffpiso.losses import L2_field_loss, fused_l2_value
    ny, nx = 10, 12
    grid = StaggeredGrid(torch.randn(1, ny + 1, nx + 1, 2), box_of(ny, nx))
    with pytest.raises(N.PisoNativeError):
        L2_field_loss(torch.zeros(()), [[grid]], [torch.randn(1, 1, ny + 1, nx + 1, 2)], 1, None, 1.0, 0, fused=True)
    flat = torch.randn((nx + 1) * ny + nx * (ny + 1), device="cuda")
    for window in ((-1, 3, 0, 3), (0, ny + 2, 0, 3), (0, 3, 0, nx + 2)):
        with pytest.raises(N.PisoNativeError):
            fused_l2_value(flat, flat, nx, ny, window, 1.0)
