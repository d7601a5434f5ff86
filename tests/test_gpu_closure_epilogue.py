"""Bias, skip connections and ReLU of the closure on the card: conv2d_act and FullyConvNetwork(bias=, activation=, skips=) over the epilogue kernels
(csrc/conv_epilogue.hip), layer and network level.

  layer, exact      conv2d_act equals, bit for bit, the numpy epilogue (tests/test_gpu_conv_epilogue.py: np_forward) of conv2d_leaky(x, w, pad, False); x.grad,
                    w.grad and skip.grad equal, bit for bit, what conv2d_leaky(..., False).backward gives when fed the numpy gpre; the bias gradient keeps
                    the bound of any summation order;
  layer, float64    against F.conv2d in float64 with bias and skip, activation None and "leaky_relu", with the bounds of tests/test_gpu_closure_any.py
                    (output 2e-6, dx and dw 3e-6 relative L2, K <= 784); dbias with activation None within gamma sum |g|;
  routing           from the profiler's kernel names: no epilogue kernel without bias, skip or ReLU; one forward and one backward pass with any of them
                    (no backward pass where there is nothing to compute: no activation and no bias - the cotangent passes through), the band
                    reducer with a bias; the reference's network launches what it launched;
  row windows       the network on rows [a, b) of the input equals the whole-grid output on the rows R away from a cut, bit for bit: what the slab path
                    rests on;
  sharded chain     the machinery of tests/test_gpu_closure_sharded_chain.py with that network: forcing bit for bit, rank-summed weight AND bias
                    gradients within twice the one-GPU float32 error against float64;
  training          two iterations of training_run with bias=True: the biases move, the checkpoint holds weights and biases, restoring reproduces both.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_conv_epilogue import U, np_backward, np_forward, same_bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ACT_CODE = {None: 0, "leaky_relu": 1, "relu": 2}
LAYER_SHAPES = [(3, 8, 8), (5, 16, 16)]                     # the run-time-shaped route; a fixed instance
H, W = 19, 70
RESIDUAL = [(3, 4, 8), (3, 8, 8), (3, 8, 8), (1, 8, 2)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30))


def _layer_data(k, cin, cout, wrapped):
    gen = torch.Generator(device="cpu").manual_seed(k * 100 + cin + cout + int(wrapped))
    x = torch.randn(1, H, W, cin, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) / np.sqrt(k * k * cin)
    b, s, g = torch.randn(cout, generator=gen), torch.randn(1, H, W, cout, generator=gen), torch.randn(1, H, W, cout, generator=gen)
    pad, wrap = ((k // 2, k // 2), (True, True)) if wrapped else (k // 2, (False, False))
    return x, w, b, s, g, pad, wrap


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("wrapped", [False, True], ids=["SAME", "wrapped"])
@pytest.mark.parametrize("k,cin,cout", LAYER_SHAPES, ids=lambda v: str(v))
def test_layer_is_the_numpy_epilogue_of_the_bare_convolution_bit_for_bit(k, cin, cout, wrapped):
    import diffpiso._native as N
    from diffpiso.closure import conv2d_act, conv2d_leaky
    fixed = (k, cin, cout) == (5, 16, 16)
    assert bool(N.conv2d_instantiated(1, k, cin, cout) and N.conv2d_instantiated(2, k, cin, cout)) == fixed
    x0, w0, b0, s0, g0, pad, wrap = _layer_data(k, cin, cout, wrapped)
    g = g0.cuda()
    # the bare convolution, once: its output, and a function feeding a cotangent through its backward
    xz, wz = x0.cuda().requires_grad_(True), w0.cuda().requires_grad_(True)
    z = conv2d_leaky(xz, wz, pad, False, wrap=wrap)
    z_np = _np(z)[0].reshape(H * W, cout)
    for activation in (None, "leaky_relu", "relu"):
        for with_bias in (False, True):
            for with_skip in (False, True):
                x, w = x0.cuda().requires_grad_(True), w0.cuda().requires_grad_(True)
                b = b0.cuda().requires_grad_(True) if with_bias else None
                s = s0.cuda().requires_grad_(True) if with_skip else None
                what = "%s, bias %s, skip %s" % (activation, with_bias, with_skip)
                y = conv2d_act(x, w, pad, activation, b, s, wrap=wrap)
                want = np_forward(z_np, _np(b0) if with_bias else None, _np(s0)[0].reshape(H * W, cout) if with_skip else None, ACT_CODE[activation])
                same_bits(_np(y)[0].reshape(H * W, cout), want, "output, " + what)
                y.backward(g)
                gpre = np_backward(_np(g0)[0].reshape(H * W, cout), want, ACT_CODE[activation])
                xz.grad = wz.grad = None
                z.backward(torch.from_numpy(gpre).reshape(1, H, W, cout).cuda(), retain_graph=True)
                same_bits(_np(x.grad), _np(xz.grad), "x.grad, " + what)
                same_bits(_np(w.grad), _np(wz.grad), "w.grad, " + what)
                if with_skip:
                    same_bits(_np(s.grad)[0].reshape(H * W, cout), gpre, "skip.grad, " + what)
                if with_bias:
                    n = H * W
                    err = np.abs(_np(b.grad).astype(f64) - gpre.astype(f64).sum(axis=0))
                    bound = (n - 1) * U / (1 - (n - 1) * U) * np.abs(gpre.astype(f64)).sum(axis=0)
                    assert (err <= bound).all(), ("bias.grad, " + what, float(err.max()), float(bound[err.argmax()]))


@pytest.mark.parametrize("wrapped", [False, True], ids=["SAME", "wrapped"])
@pytest.mark.parametrize("activation", [None, "leaky_relu"])
@pytest.mark.parametrize("k,cin,cout", LAYER_SHAPES, ids=lambda v: str(v))
def test_layer_matches_float64_convolution_with_bias_and_skip(k, cin, cout, activation, wrapped):
    from diffpiso.closure import conv2d_act
    assert k * k * cin <= 784 and k * k * cout <= 784
    x0, w0, b0, s0, g0, pad, wrap = _layer_data(k, cin, cout, wrapped)
    x, w, b, s = (t.cuda().requires_grad_(True) for t in (x0, w0, b0, s0))
    y = conv2d_act(x, w, pad, activation, b, s, wrap=wrap)
    xd, wd, bd, sd = (t.double().requires_grad_(True) for t in (x0, w0, b0, s0))
    xc = xd.permute(0, 3, 1, 2)
    if wrapped:
        xc = F.pad(xc, (k // 2,) * 4, mode="circular")
    yd = (F.conv2d(xc, wd, padding=0 if wrapped else k // 2).permute(0, 2, 3, 1) + bd) + sd
    if activation == "leaky_relu":
        yd = F.leaky_relu(yd, 0.2)
    assert y.shape == yd.shape == (1, H, W, cout)
    print("output %.3e" % rel(y, yd))
    assert rel(y, yd) < 2e-6
    y.backward(g0.cuda())
    yd.backward(g0.double())
    print("dx %.3e, dw %.3e, dskip %.3e" % (rel(x.grad, xd.grad), rel(w.grad, wd.grad), rel(s.grad, sd.grad)))
    assert rel(x.grad, xd.grad) < 3e-6, ("dx", rel(x.grad, xd.grad))
    assert rel(w.grad, wd.grad) < 3e-6, ("dw", rel(w.grad, wd.grad))
    if activation is None:
        n = H * W
        g2 = g0.double().reshape(n, cout)
        err = (b.grad.double().cpu() - bd.grad).abs()
        bound = (n - 1) * U / (1 - (n - 1) * U) * g2.abs().sum(dim=0)
        print("dbias: max error %.3e, its bound %.3e" % (float(err.max()), float(bound[err.argmax()])))
        assert torch.equal(bd.grad, g2.sum(dim=0)) or rel(bd.grad, g2.sum(dim=0)) < 1e-15
        assert bool((err <= bound).all()), ("dbias", float(err.max()))
        same_bits(_np(s.grad), _np(g0), "skip.grad without an activation is the cotangent")
    else:
        assert rel(b.grad, bd.grad) < 3e-6 and rel(s.grad, sd.grad) < 3e-6


# ------------------------------------------------------------------------------------------------------------------------------------
def _kernel_counts(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages()}


def _count(counts, word):
    return sum(c for name, c in counts.items() if word in name)


def test_routing_one_pass_per_direction_only_where_there_is_an_epilogue():
    import diffpiso as dp
    from diffpiso.closure import conv2d_act
    for k, cin, cout in LAYER_SHAPES:
        x0, w0, b0, s0, g0, pad, wrap = _layer_data(k, cin, cout, False)
        g = g0.cuda()
        for activation in (None, "leaky_relu", "relu"):
            for with_bias in (False, True):
                for with_skip in (False, True):
                    x, w = x0.cuda().requires_grad_(True), w0.cuda().requires_grad_(True)
                    b = b0.cuda().requires_grad_(True) if with_bias else None
                    s = s0.cuda().requires_grad_(True) if with_skip else None
                    counts = _kernel_counts(lambda: conv2d_act(x, w, pad, activation, b, s).backward(g))
                    what = (k, cin, cout, activation, with_bias, with_skip, counts)
                    assert not any("miopen" in n.lower() or "igemm" in n.lower() for n in counts), what
                    fwd, bwd, red = (_count(counts, "conv_epilogue_%s_kernel" % p) for p in ("forward", "backward", "bias_reduce"))
                    if not (with_bias or with_skip or activation == "relu"):
                        assert _count(counts, "conv_epilogue") == 0, what
                        assert _count(counts, "leaky_backward") == (1 if activation else 0), what
                    else:
                        assert fwd == 1 and red == int(with_bias) and _count(counts, "leaky_backward") == 0, what
                        assert bwd == (1 if (activation or with_bias) else 0), what                 # (no activation, no bias: gpre is g - nothing to launch)
                        assert _count(counts, "conv_epilogue") == fwd + bwd + red, what
    # the reference's seven layers: the kernels of before, six fused leaky backward passes, no epilogue
    ref = dp.FullyConvNetwork(seed=1).cuda()
    x = torch.randn(1, 24, 80, 4, generator=torch.Generator().manual_seed(0)).cuda().requires_grad_(True)
    counts = _kernel_counts(lambda: ref(x).sum().backward())
    assert _count(counts, "conv_epilogue") == 0 and _count(counts, "conv_forward_any") == 0 and _count(counts, "conv_wgrad_any") == 0, counts
    assert _count(counts, "leaky_backward") == 6 and _count(counts, "conv_wgrad") >= 7, counts
    assert _count(counts, "conv_forward_kernel") + _count(counts, "conv_forward_lds_kernel") == 14, counts     # 7 forward + 7 input gradients
    assert not any("miopen" in n.lower() or "igemm" in n.lower() for n in counts), counts
    # ... and the residual network: an epilogue behind every layer (bias everywhere), none of torch's element-wise kernels in between
    net = _residual_net((False, False))
    x = torch.randn(1, 20, 24, 4, generator=torch.Generator().manual_seed(0)).cuda().requires_grad_(True)
    g = torch.randn(1, 20, 24, 2, generator=torch.Generator().manual_seed(1)).cuda()
    counts = _kernel_counts(lambda: net(x).backward(g))
    assert (_count(counts, "conv_epilogue_forward_kernel"), _count(counts, "conv_epilogue_backward_kernel"), _count(counts, "conv_epilogue_bias_reduce")) == (4, 4, 4), counts
    assert _count(counts, "leaky_backward") == 0, counts


# ------------------------------------------------------------------------------------------------------------------------------------
def _residual_net(wrap, device="cuda"):
    """layers 4 -> 8 -> 8 -> 8 -> 2, a bias in every layer (non-zero), the pre-activation of layer 2 adds the input of layer 1, ReLU: R = 3"""
    import diffpiso as dp
    net = dp.FullyConvNetwork(seed=4, wrap=wrap, layers=RESIDUAL, bias=True, skips={2: 1}, activation="relu")
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for p in net.biases:
            p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    assert net.reduced_buffer_width == 3 and len(net.biases) == 4
    return net.to(device)


@pytest.mark.parametrize("wrap_x", [False, True], ids=["zero-padded x", "wrapped x"])
def test_network_on_a_row_window_equals_the_whole_grid_away_from_the_cuts(wrap_x):
    net = _residual_net((False, wrap_x))
    R, ny = net.reduced_buffer_width, 20
    x = torch.randn(1, ny, 24, 4, generator=torch.Generator().manual_seed(12)).cuda()
    with torch.no_grad():
        whole = _np(net(x, wrap=(False, wrap_x)))
        assert np.isfinite(whole).all() and (whole != 0).mean() > 0.9
        for a, b in ((0, 9), (5, 14), (11, 20)):
            part = _np(net(x[:, a:b].contiguous(), wrap=(False, wrap_x)))
            lo, hi = R * (a > 0), R * (b < ny)
            assert part.shape == (1, b - a, 24, 2) and b - a - lo - hi > 0
            same_bits(part[:, lo:b - a - hi], whole[:, a + lo:b - hi], "rows [%d, %d) of the window [%d, %d)" % (a + lo, b - hi, a, b))


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["periodic", "cavity"])
def test_sharded_chain_with_biases_a_skip_and_relu(name):
    import diffpiso as dp
    from tests import slab_emulation as E
    from tests.cases import make_case
    from tests.test_gpu_closure_glue_twins import flat_faces, network_input64, torch_fields
    from tests.test_gpu_closure_sharded_chain import rel as rel_flat, sharded_run
    from tests.test_gpu_slab_twins import Inputs
    nx = ny = 24
    c = make_case(name, ny, nx, seed=6)
    wrap = tuple(bool(b) for b in c["periodic_yx"])
    net = _residual_net(wrap)
    params = list(net.weights) + list(net.biases)
    I = Inputs(nx, ny, 23)
    vel, p = torch.as_tensor(c["vel"]).cuda(), torch.as_tensor(c["p"]).cuda()
    g_st = torch.zeros((1, ny + 1, nx + 1, 2), device="cuda")
    g_st[:, :, :nx, 0], g_st[:, :ny, :, 1] = I.randn((ny + 1) * nx).reshape(1, ny + 1, nx), I.randn(ny * (nx + 1)).reshape(1, ny, nx + 1)
    two_dx = 2 * float(np.mean(c["dx_yx"]))

    def grads(ps):
        return torch.cat([q.grad.reshape(-1) for q in ps[:4]]).clone(), torch.cat([q.grad.reshape(-1) for q in ps[4:]]).clone()
    # one GPU, float32: the product's whole-grid path;  float64 on the host: torch's convolution
    net.zero_grad()
    vel_t, p_t, velocity, pressure = torch_fields(c, vel, p, two_dx, grad=True)
    F32 = dp.make_forcing_fn(net, True, wrap=wrap)(0, velocity, pressure)
    F32.backward(g_st)
    one = (flat_faces(F32.detach()), flat_faces(vel_t.grad), p_t.grad.reshape(-1)) + grads(params)
    net64 = copy.deepcopy(net).double().cpu()
    net64.zero_grad()
    v64, p64, nn64 = network_input64(c, vel.cpu(), p.cpu(), two_dx, 4)
    dp.centered_to_staggered(net64(nn64), wrap).backward(g_st.double().cpu())
    ref = (None, flat_faces(v64.grad), p64.grad.reshape(-1)) + grads(list(net64.weights) + list(net64.biases))
    e_one = [rel_flat(one[i], ref[i]) for i in (1, 2, 3, 4)]
    w = dict(vel=flat_faces(vel), p=p.reshape(-1).contiguous(), dF=flat_faces(g_st))
    _, _, velocity, pressure = torch_fields(c, vel, p, two_dx)
    nn_in_whole = dp.network_input(velocity, pressure, True).reshape(-1).contiguous()
    tally, bad = E.Tally(), []
    for world in (2, 3):
        tag = "%s residual network 24 x 24, %d ranks" % (name, world)
        net.zero_grad()
        # (sharded_run asserts, through the tally, that the forcing on every rank's owned faces is one[0] bit for bit)
        du, dpw = sharded_run(tally, tag, world, c, net, wrap, w, nn_in_whole, one)
        assert not torch.isnan(du).any() and not torch.isnan(dpw).any(), tag
        e_sh = [rel_flat(du, ref[1]), rel_flat(dpw, ref[2])] + [rel_flat(a, b) for a, b in zip(grads(params), ref[3:])]
        for what, a, b in zip(("dL/du", "dL/dp", "weight gradients", "bias gradients"), e_sh, e_one):
            print("%s %s: sharded vs float64 %.3e, one GPU vs float64 %.3e, ratio %.3f" % (tag, what, a, b, a / b))
            if not a <= 2 * b:
                bad.append((tag, what, a, b))
    failures = tally.failures()
    assert len(tally) > 0 and not failures, "%d checks; first failures: %s" % (len(tally), failures)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------------
def test_training_run_with_biases_moves_saves_and_restores_them(tmp_path):
    import diffpiso as dp
    import diffpiso.training as T
    from tests.test_gpu_training_smoke import _frames
    hr, box = (32, 96), dp.box[0:8, 0:24]
    phys = dict(average_velocity=1.0, velocity_difference=0.8, inlet_profile_sharpness=2.0, viscosity=5e-3)
    dt = 0.1
    data = _frames(tmp_path, 7, hr, box, phys, dt)
    base_dir = str(tmp_path) + "/run"
    os.makedirs(base_dir)
    sim = dict(HRres=list(hr), dx_ratio=2, box=box, sponge_ratio=0.75, relative_sponge_max=20.0, dt=dt, dt_ratio=1, setup_fun=dp.spatialMixingLayer_setup)
    made = []

    def initialiser(buffer_width, padding):
        net, params, _ = dp.initialise_fullyconv_network(None, padding=padding, seed=5, bias=True)
        made.append((net, params))
        return net, params, [[1, 1], [1, 1]]
    td = dict(HR_buffer_width=[[2, 2], [2, 2]], learning_rate=2e-4, step_count=2, epochs=1, store_interm_ckpts=2, padding="SAME",
              network_initialiser=initialiser, network_wrapper=None, loss_functions=[dp.L2_field_loss], loss_factor=[1.0], sum_steps=True,
              loss_influence_range=None, dataset=[data], start_frame=[0], frame_count_training=[4], frame_count_validation=[3],
              dataset_characteristics=[(0.08, 0.05)], perturb_inlet=True, load_model_path=None, lr_decay_fun=None, seed=1)
    hist, _ = dp.training_run(base_dir, phys, sim, td, solver_precision=1e-7)
    assert len(hist) == 2 and (hist > 0).all() and np.isfinite(hist).all()
    net, params = made[-1]
    assert len(params) == 14 and len(net.biases) == 7
    assert all(float(b.detach().abs().max()) > 0 for b in net.biases), "the biases did not move"
    ckpt = os.path.join(base_dir, "model_epoch_000000.ckpt")
    saved = torch.load(ckpt)
    assert len(saved) == 14 and [tuple(t.shape) for t in saved] == [tuple(q.shape) for q in params]
    assert all(torch.equal(t, q.detach().cpu()) for t, q in zip(saved, params))
    fresh, fresh_params, _ = dp.initialise_fullyconv_network(None, padding="SAME", seed=99, bias=True)
    fresh = fresh.to(params[0].device)
    T._restore(list(fresh.weights) + list(fresh.biases), ckpt)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(fresh.weights, net.weights)) and all(torch.equal(a.detach(), b.detach()) for a, b in zip(fresh.biases, net.biases))
    x = torch.randn(1, 16, 48, 4, generator=torch.Generator().manual_seed(3)).to(params[0].device)
    with torch.no_grad():
        assert torch.equal(fresh(x), net(x))
