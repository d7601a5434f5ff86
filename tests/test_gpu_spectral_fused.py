"""`spectral_energy_loss(..., fused=True)` - the kernels of csrc/loss_spectrum.hip either side of torch.fft.fft2 - on the GPU.

Inputs: `pred` and `gt` of tests/golden/spectral_loss.npz (12 x 16 cells, 5 steps, outputs of the reference's own losses.py) as float32.
  centre + crop   the planes EQUAL the torch crop of at_centers() for four windows; the adjoint of a random cotangent EQUALS torch autograd's
                  (a face adds at most two products by 0.5, and a float sum of two terms has one value)
  shells          E against the float64 torch spectrum of the same crop, 2e-6 of the maximum (the bound of tests/test_spectral_golden.py);
                  the four windows plus 9 x 16 and 11 x 13 (with 9 x 8 the shapes in which radii of exactly k + 1/2 occur)
  shell adjoint   the map of include/piso_hip.h on a random transform, with the upstream scalar and with NULL for 1
  values          the reference's five loss values and its two per-step lists at the project's rel 2e-5
  gradient        d loss / d faces against autograd through the float64 torch path (on the host), rel L2 <= 1e-5, the project's parity bar:
                  log form with start_wavenumber 0 and 1, absolute form, all six crops
  determinism     five evaluations of forward + backward: identical bits
  edges           pred == gt: value 0, gradient all zero and finite, both forms; an all-zero prediction in the log form: non-finite value;
                  a 2 x 2 crop and a crop one cell high (no shell below the cutoff): 0
  refusals        a host field with fused=True; NULL pointers and crops outside the grid at the C entries
  long shells     random fields on 100 x 128 cells, full crop: cutoff 50, the outer shells hold more than 256 coefficients, so that every
                  thread of a shell's workgroup walks its list more than once; value 2e-5, gradient 1e-5 against float64
  training_run    training_dict["fused_losses"]: the first iteration's loss and four contributions with and without the key, 1e-5 relative
Every comparison prints what it measured.  Measured on an MI355X: shells at most 6.7e-8 of the maximum, the reference's loss values at
most 2.1e-7 (the per-step lists 1.0e-6), gradients at most 1.8e-6 on the fixture and 2.3e-6 on 100 x 128, the training run's first
iteration 8.5e-8 (its spectral term 1.7e-6)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_loss.npz")
NY, NX = 12, 16
# (label, buffer_width, sponge_start, (h, w))
WINDOWS = [("full", [[0, 0], [0, 0]], 0, (12, 16)), ("two-sided", [[1, 2], [2, 1]], 0, (9, 13)), ("sponge", [[0, 0], [1, 1]], 10, (12, 8)),
           ("9x8", [[2, 1], [3, 5]], 0, (9, 8))]
TIE_WINDOWS = [("9x16", [[1, 2], [0, 0]], 0, (9, 16)), ("11x13", [[0, 1], [1, 2]], 0, (11, 13))]
FORMS = [("log w0", dict(log_distance=True, start_wavenumber=0)), ("log w1", dict(log_distance=True, start_wavenumber=1)),
         ("abs", dict(log_distance=False, start_wavenumber=0))]
_cache = {}


def golden():
    if "gold" not in _cache:
        g = np.load(GOLD)
        _cache["gold"] = {k: g[k] for k in g.files}
    return _cache["gold"]


def flat_of(staggered):
    """Staggered tensor [1, ny + 1, nx + 1, 2] -> flat u-first face vector (same dtype and device)."""
    ny, nx = staggered.shape[1] - 1, staggered.shape[2] - 1
    return torch.cat([staggered[0, :ny, :, 1].reshape(-1), staggered[0, :, :nx, 0].reshape(-1)])


def grid_of(flat, ny, nx, box=(6.0, 4.0)):
    """A StaggeredGrid whose components are views of the leaf `flat`."""
    import diffpiso as dp
    n_u = (nx + 1) * ny
    return dp.StaggeredGrid([flat[n_u:].view(1, ny + 1, nx, 1), flat[:n_u].view(1, ny, nx + 1, 1)], dp.box[0:box[0], 0:box[1]],
                            extrapolation="periodic")


def loss_and_gradient(preds, truth, ny, nx, device, dtype, **kw):
    """spectral_energy_loss over all steps of `preds` (staggered tensors) -> (contribution, d / d faces of every step, concatenated)."""
    import diffpiso as dp
    leaves = [flat_of(torch.as_tensor(p)).to(device=device, dtype=dtype).requires_grad_(True) for p in preds]
    grids = [grid_of(f, ny, nx) for f in leaves]
    total, c = dp.spectral_energy_loss(torch.zeros((), dtype=dtype, device=device), [grids], [torch.as_tensor(truth).to(device=device, dtype=dtype)],
                                       len(preds), **kw)
    total.backward()
    return float(c.detach()), np.concatenate([f.grad.detach().cpu().numpy().astype(np.float64) for f in leaves])


def reference(key, preds, truth, ny, nx, **kw):
    """The float64 torch path on the host, once per case."""
    if key not in _cache:
        _cache[key] = loss_and_gradient(preds, truth, ny, nx, "cpu", torch.float64, **kw)
    return _cache[key]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def torch_crop(staggered, bw, sponge):
    """The crop spectral_energy_loss takes of at_centers(): [h, w, 2], component 0 = v."""
    import diffpiso as dp
    central = dp.StaggeredGrid(staggered).at_centers().data
    if sponge == 0:
        sponge = central.shape[2]
    return central[0, bw[0][0]:central.shape[1] - bw[0][1], bw[1][0]:sponge - bw[1][1], :]


@pytest.mark.parametrize("window", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_centre_crop_and_its_adjoint_equal_torch(window):
    from diffpiso.losses import fused_centre_crop, fused_centre_crop_adjoint, spectrum_window
    label, bw, sponge, (h, w) = window
    stag = torch.tensor(golden()["pred"][1]).cuda().requires_grad_(True)
    want = torch_crop(stag, bw, sponge).permute(2, 0, 1)
    assert tuple(want.shape) == (2, h, w)
    win = spectrum_window(bw, sponge, NY, NX)
    got = fused_centre_crop(flat_of(stag.detach()).contiguous(), NX, NY, win)
    assert torch.equal(got, want.detach()), label
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(5)).cuda()
    want.backward(cot)
    d_faces = fused_centre_crop_adjoint(cot.contiguous(), NX, NY, win)
    assert torch.equal(d_faces, flat_of(stag.grad)), label
    assert int((d_faces != 0).sum()) > 0
    # the tensor's padded last row of u / last column of v are no faces: torch sends them nothing either
    assert not stag.grad[0, NY, :, 1].any() and not stag.grad[0, :, NX, 0].any()


@pytest.mark.parametrize("window", WINDOWS + TIE_WINDOWS, ids=[w[0] for w in WINDOWS + TIE_WINDOWS])
def test_shell_sums_match_the_float64_torch_spectrum(window):
    from diffpiso.evaluation_tools import EK_spectrum_2D_tf
    from diffpiso.losses import fused_centre_crop, fused_shell_sums, spectrum_plan, spectrum_window
    label, bw, sponge, (h, w) = window
    stag = torch.tensor(golden()["pred"][3])
    want = EK_spectrum_2D_tf(torch_crop(stag, bw, sponge).to(torch.float64)).numpy()
    win = spectrum_window(bw, sponge, NY, NX)
    plan = spectrum_plan(h, w, "cuda")
    assert plan.shell.is_cuda and plan.perm.is_cuda and plan.offsets.is_cuda
    planes = fused_centre_crop(flat_of(stag).cuda().contiguous(), NX, NY, win)
    got = fused_shell_sums(torch.view_as_real(torch.fft.fft2(planes)).contiguous(), plan)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape == (min(h, w) // 2,)
    err = float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
    print("shells %s (%d x %d): max error / max E = %.3g (bound 2e-6)" % (label, h, w, err))
    assert err <= 2e-6


def test_shell_adjoint_is_the_map_of_the_header():
    """d_spec = (upstream *) 2 * 0.5 / (h w)^2 * dE[shell[q]] * spec, 0 at and beyond the cutoff; with and without the upstream scalar.  The
    same float64 products rounded once to float32, so the comparison is at one float32 rounding (6e-8)."""
    from diffpiso.losses import fused_shell_sums_adjoint, spectrum_plan
    h, w = 9, 16
    plan = spectrum_plan(h, w, "cuda")
    gen = torch.Generator().manual_seed(9)
    spec = torch.randn((2, h, w, 2), generator=gen).cuda()
    d_e = torch.randn(plan.cutoff, generator=gen, dtype=torch.float64).cuda()
    shell = plan.shell.long().reshape(h, w)
    inside = shell < plan.cutoff
    assert 0 < int(inside.sum()) < h * w
    per_cell = torch.where(inside, d_e[shell.clamp(max=plan.cutoff - 1)], torch.zeros((), dtype=torch.float64, device="cuda"))
    want = (per_cell / float(h * w) ** 2)[None, :, :, None] * spec.double()
    for upstream in (None, torch.tensor([0.25], device="cuda")):
        got = fused_shell_sums_adjoint(spec, plan, d_e, upstream)
        ref = want if upstream is None else 0.25 * want
        assert got.dtype == torch.float32 and got.shape == spec.shape
        assert not got[:, ~inside].any()
        assert float((got.double() - ref).abs().max()) <= 6e-8 * float(ref.abs().max())


def test_loss_values_are_the_references():
    import diffpiso as dp
    g = golden()
    steps = g["pred"].shape[0]
    box = dp.box[0:float(g["box"][0]), 0:float(g["box"][1])]
    grids = [dp.StaggeredGrid(torch.tensor(p).cuda(), box, extrapolation="periodic") for p in g["pred"]]
    gtt = torch.tensor(g["gt"]).cuda()
    zero = torch.zeros((), device="cuda")
    cases = {"log_w0": dict(log_distance=True, start_wavenumber=0, buffer_width=[[0, 0], [0, 0]], loss_factor=1.5),
             "log_w1": dict(log_distance=True, start_wavenumber=1, buffer_width=[[0, 0], [0, 0]], loss_factor=1.5),
             "abs": dict(log_distance=False, start_wavenumber=0, buffer_width=[[0, 0], [0, 0]], loss_factor=0.7),
             "log_buffered": dict(log_distance=True, start_wavenumber=0, buffer_width=[[1, 2], [2, 1]], loss_factor=[0.5 + 0.1 * s for s in range(steps)]),
             "abs_sponge_10": dict(log_distance=False, start_wavenumber=0, buffer_width=[[0, 0], [1, 1]], loss_factor=1.0, sponge_start=10)}
    for name, kw in cases.items():
        tot, c = dp.spectral_energy_loss(zero + 2.0, [grids], [gtt], steps, fused=True, **kw)
        assert c.dtype == torch.float32 and c.dim() == 0 and c.is_cuda
        want = float(g["loss_" + name])
        print("loss_%s: fused %.9g, reference %.9g, relative distance %.3g (bound 2e-5)" % (name, float(c), want, abs(float(c) - want) / want))
        assert float(c) == pytest.approx(want, rel=2e-5), name
        assert float(tot) == pytest.approx(float(c) + 2.0)
    per, contrib = dp.spectral_energy_loss([zero] * steps, [grids], [gtt], steps, buffer_width=[[0, 0], [0, 0]], loss_factor=1.0,
                                           sum_steps=False, loss_influence_range=2, fused=True)
    assert len(per) == steps and len(contrib) == steps
    for label, got, want in (("loss_contrib", contrib, g["loss_contrib"]), ("loss_per_step", per, g["loss_per_step"])):
        got = np.array([float(v) for v in got])
        print("%s: largest relative distance %.3g (bound 2e-5)" % (label, float(np.max(np.abs(got - want) / np.abs(want)))))
        np.testing.assert_allclose(got, want, rtol=2e-5)


@pytest.mark.parametrize("window", WINDOWS + TIE_WINDOWS, ids=[w[0] for w in WINDOWS + TIE_WINDOWS])
def test_gradient_matches_autograd_through_the_float64_torch_path(window):
    label, bw, sponge, (h, w) = window
    g = golden()
    for form, kw in FORMS:
        kw = dict(kw, buffer_width=bw, sponge_start=sponge, loss_factor=1.5)
        v_ref, g_ref = reference(("grad", label, form), g["pred"], g["gt"], NY, NX, **kw)
        v_got, g_got = loss_and_gradient(g["pred"], g["gt"], NY, NX, "cuda", torch.float32, fused=True, **kw)
        assert np.isfinite(g_ref).all() and np.linalg.norm(g_ref) > 0
        ev, eg = abs(v_got - v_ref) / abs(v_ref), rel_l2(g_got, g_ref)
        print("gradient %s, %s: value %.3g (bound 2e-5), gradient rel L2 %.3g (bound 1e-5)" % (label, form, ev, eg))
        assert ev <= 2e-5, (label, form, v_got, v_ref)
        assert eg <= 1e-5, (label, form)
        assert np.array_equal(g_got == 0, g_ref == 0), "%s, %s: the faces no cropped cell reads differ" % (label, form)


def test_five_evaluations_give_identical_bits():
    g = golden()
    for form, kw in FORMS[::2]:
        kw = dict(kw, buffer_width=[[1, 2], [2, 1]], loss_factor=1.5)
        runs = [loss_and_gradient(g["pred"], g["gt"], NY, NX, "cuda", torch.float32, fused=True, **kw) for _ in range(5)]
        for v, grad in runs[1:]:
            assert v == runs[0][0] and np.array_equal(grad, runs[0][1]), form


def test_edge_cases():
    g = golden()
    own_truth = torch.tensor(g["pred"][:, 0])[None]             # [1, steps, ny + 1, nx + 1, 2]: every step's truth IS its prediction
    for form, kw in FORMS[::2]:
        v, grad = loss_and_gradient(g["pred"], own_truth, NY, NX, "cuda", torch.float32, fused=True, buffer_width=[[0, 0], [0, 0]], **kw)
        assert v == 0.0 and np.isfinite(grad).all() and not grad.any(), form
    v, _ = loss_and_gradient(np.zeros_like(g["pred"]), g["gt"], NY, NX, "cuda", torch.float32, fused=True, buffer_width=[[0, 0], [0, 0]],
                             log_distance=True)
    assert not np.isfinite(v)
    for bw, shape in (([[5, 5], [7, 7]], "2 x 2"), ([[5, 6], [7, 7]], "1 x 2")):
        for form, kw in FORMS[::2]:
            v, grad = loss_and_gradient(g["pred"], g["gt"], NY, NX, "cuda", torch.float32, fused=True, buffer_width=bw, **kw)
            assert v == 0.0 and not grad.any(), (shape, form)
    # a start_wavenumber at or beyond the cutoff: an empty range, 0
    v, grad = loss_and_gradient(g["pred"], g["gt"], NY, NX, "cuda", torch.float32, fused=True, buffer_width=[[0, 0], [0, 0]], log_distance=True,
                                start_wavenumber=5)
    assert v == 0.0 and not grad.any()


def test_refusals():
    import diffpiso as dp
    from diffpiso import _native as N
    from diffpiso.losses import fused_centre_crop
    g = golden()
    grid = dp.StaggeredGrid(torch.tensor(g["pred"][0]), dp.box[0:6, 0:4], extrapolation="periodic")
    with pytest.raises(N.PisoNativeError, match="fused=True"):
        dp.spectral_energy_loss(torch.zeros(()), [[grid]], [torch.tensor(g["gt"])], 1, fused=True)
    flat = torch.randn((NX + 1) * NY + NX * (NY + 1), device="cuda")
    for window in ((-1, 3, 0, 3), (0, NY + 1, 0, 3), (0, 3, 0, NX + 1), (3, 3, 0, 4), (0, 4, 5, 5)):
        with pytest.raises(N.PisoNativeError, match="piso_loss_centre_crop"):
            fused_centre_crop(flat, NX, NY, window)
    # the C entries themselves: PISO_ERR_INVALID_ARG (1) and a message that names the entry
    some = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, stream = C.c_void_p(some.data_ptr()), N.stream_ptr()
    calls = {"piso_loss_centre_crop": [(None, 4, 4, 0, 4, 0, 4, p, stream), (p, 4, 4, 0, 4, 0, 4, None, stream), (p, 4, 4, 0, 5, 0, 4, p, stream),
                                       (p, 4, 4, 2, 2, 0, 4, p, stream)],
             "piso_loss_centre_crop_adjoint": [(None, 4, 4, 0, 4, 0, 4, p, stream), (p, 4, 4, 0, 4, 0, 4, None, stream),
                                               (p, 4, 4, 0, 4, -1, 4, p, stream)],
             "piso_loss_spectrum_shells": [(None, p, p, 4, 4, 2, p, stream), (p, None, p, 4, 4, 2, p, stream), (p, p, None, 4, 4, 2, p, stream),
                                           (p, p, p, 4, 4, 2, None, stream), (p, p, p, 0, 4, 0, p, stream), (p, p, p, 4, 4, 3, p, stream)],
             "piso_loss_spectrum_shells_adjoint": [(None, p, p, None, 4, 4, 2, p, stream), (p, None, p, None, 4, 4, 2, p, stream),
                                                   (p, p, None, None, 4, 4, 2, p, stream), (p, p, p, None, 4, 4, 2, None, stream),
                                                   (p, p, p, None, 4, 0, 0, p, stream)],
             "piso_loss_spectrum_distance": [(None, p, 2, 0, 1, C.c_double(1.0), p, p, stream), (p, None, 2, 0, 1, C.c_double(1.0), p, p, stream),
                                             (p, p, 2, 0, 1, C.c_double(1.0), None, p, stream), (p, p, 2, 0, 1, C.c_double(1.0), p, None, stream),
                                             (p, p, 2, -1, 1, C.c_double(1.0), p, p, stream), (p, p, -1, 0, 1, C.c_double(1.0), p, p, stream)]}
    for name, arg_lists in calls.items():
        for args in arg_lists:
            assert getattr(N.lib, name)(*args) == 1, (name, args)
            assert (name + ":") in N.lib.piso_last_error_string().decode(), name
    torch.cuda.synchronize()


def test_shells_longer_than_a_workgroup():
    from diffpiso.losses import spectrum_plan
    ny, nx = 100, 128
    plan = spectrum_plan(ny, nx, "cuda")
    lengths = np.diff(plan.offsets.cpu().numpy())
    assert plan.cutoff == 50 and lengths.max() > 256 and lengths.min() >= 1
    gen = torch.Generator().manual_seed(41)
    truth = torch.randn((1, 1, ny + 1, nx + 1, 2), generator=gen)
    preds = (truth[0] + 0.3 * torch.randn((1, 1, ny + 1, nx + 1, 2), generator=gen)).numpy()
    for form, kw in FORMS[::2]:
        kw = dict(kw, buffer_width=[[0, 0], [0, 0]], loss_factor=0.5)
        v_ref, g_ref = reference(("long", form), preds, truth, ny, nx, **kw)
        runs = [loss_and_gradient(preds, truth, ny, nx, "cuda", torch.float32, fused=True, **kw) for _ in range(2)]
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
        ev, eg = abs(runs[0][0] - v_ref) / abs(v_ref), rel_l2(runs[0][1], g_ref)
        print("100 x 128, %s: value %.3g (bound 2e-5), gradient rel L2 %.3g (bound 1e-5)" % (form, ev, eg))
        assert ev <= 2e-5 and eg <= 1e-5, form


def test_training_run_with_fused_losses(tmp_path):
    """One training iteration and one validation sample of a tiny `training_run` in the shape of tests/test_gpu_training_smoke.py, with
    all four losses, once as it always ran and once with training_dict["fused_losses"]."""
    import re
    import diffpiso as dp
    from tests.test_gpu_training_smoke import _frames
    hr, box = (32, 96), dp.box[0:8, 0:24]
    phys = dict(average_velocity=1.0, velocity_difference=0.8, inlet_profile_sharpness=2.0, viscosity=5e-3)
    dt = 0.1
    data = _frames(tmp_path, 6, hr, box, phys, dt)
    sim = dict(HRres=list(hr), dx_ratio=2, box=box, sponge_ratio=0.75, relative_sponge_max=20.0, dt=dt, dt_ratio=1,
               setup_fun=dp.spatialMixingLayer_setup)
    first = {}
    for label, extra in (("torch", {}), ("fused", {"fused_losses": True})):
        base_dir = str(tmp_path) + "/run_" + label
        os.makedirs(base_dir)
        td = dict(HR_buffer_width=[[2, 2], [2, 2]], learning_rate=2e-4, step_count=2, epochs=1, store_interm_ckpts=0, padding="SAME",
                  network_initialiser=lambda buffer_width, padding: dp.initialise_fullyconv_network(None, padding=padding, seed=5)[:2] + ([[1, 1], [1, 1]],),
                  network_wrapper=None, loss_functions=[dp.L2_field_loss, dp.strain_rate_loss, dp.spectral_energy_loss, dp.multistep_averaging_loss],
                  loss_factor=[1.0, 1e-3, 1e-3, 1e-3], sum_steps=True, loss_influence_range=None, dataset=[data], start_frame=[0],
                  frame_count_training=[3], frame_count_validation=[3], dataset_characteristics=[(0.08, 0.05)], perturb_inlet=True,
                  load_model_path=None, lr_decay_fun=None, seed=1, **extra)
        hist, hist_val = dp.training_run(base_dir, phys, sim, td, solver_precision=1e-7)
        assert len(hist) == 1 and hist[0] > 0 and np.isfinite(hist_val).all()
        line = open(os.path.join(base_dir, "loss.log")).readline()
        m = re.match(r"epoch 0  iteration 0  loss: (\S+) warn:False  loss_contribs \[(.*)\]", line)
        assert m, line
        first[label] = [float(m.group(1))] + [float(x) for x in m.group(2).split(",")]
        assert len(first[label]) == 5 and all(v > 0 for v in first[label]), line
        assert os.path.exists(os.path.join(base_dir, "model_epoch_000000.ckpt"))
    ratios = [abs(a - b) / abs(b) for a, b in zip(first["fused"], first["torch"])]
    print("training_run, first iteration (loss, L2, strain, spectral, multistep): fused / torch relative distances %s (bound 1e-5)"
          % ["%.3g" % r for r in ratios])
    assert max(ratios) <= 1e-5, (first, ratios)
