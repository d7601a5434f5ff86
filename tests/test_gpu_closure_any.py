"""The closure with layers the fixed kernel instances do not hold, on the card: conv2d_leaky and FullyConvNetwork(layers=...) through the
run-time-shaped family (csrc/conv_any.hip) against float64 on the host, with the bounds of tests/test_gpu_conv.py; which kernels run for which
network; and that the reference's network still runs exactly the calls it ran before.

The network's gradients and the leaky ReLU (tests/test_gpu_closure_wrap.py tells the story): the bounds of the network comparison presuppose that no
pre-activation of the float64 reference lies within round-off of zero.  Required here: every pre-activation farther from zero than 1e-4 of its layer's
r.m.s., asserted before anything is compared.  No seed gives that by itself - 24 x 80 x (24 + 40 + 40) = 2e5 pre-activations with a density of 0.4 per
r.m.s. at zero put 16 of them inside that band on average (the best of 150 seeds: 2.7e-5) - so the INPUT of seed 3 is moved, on the CPU and in float64
alone: for every pre-activation inside 2e-4 r.m.s. the smallest change of the input (along that pre-activation's own gradient) that carries it to
3e-4 r.m.s. on the side it is on.  Such a change moves the few hundred pre-activations around it by a small fraction of that, so two or three rounds
clear the band; the moved input is rounded to float32, and the condition is asserted for exactly the tensor the card is given.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_any_cpu import FWD_ANY
from tests.test_gpu_conv_any import flipped
from tests.test_gpu_conv_wrap import assert_bitwise, call_forward_old, call_wgrad_old

pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES = [(5, 5, 24), (3, 24, 40), (3, 40, 40), (1, 40, 3), (7, 9, 16)]          # each refused by the fixed instances in at least one pass
NET_LAYERS = [(5, 5, 24), (3, 24, 40), (3, 40, 40), (1, 40, 2)]
MARGIN = 1e-4


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30))


@pytest.mark.parametrize("k,cin,cout", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("leaky", [True, False])
def test_layer_forward_and_gradients_match_float64_convolution(k, cin, cout, same, leaky):
    """K = k k cin <= 784 = the largest K the bounds of tests/test_gpu_conv.py were set for"""
    import diffpiso._native as N
    from diffpiso.closure import conv2d_leaky
    assert k * k * cin <= 784 and k * k * cout <= 784
    assert not (N.conv2d_instantiated(1, k, cin, cout) and N.conv2d_instantiated(1, k, cout, cin) and N.conv2d_instantiated(2, k, cin, cout))
    gen = torch.Generator(device="cpu").manual_seed(k * 100 + cin + cout)
    H, W = 19, 70
    x = torch.randn(1, H, W, cin, generator=gen).cuda().requires_grad_(True)
    w = (torch.randn(cout, cin, k, k, generator=gen) / np.sqrt(k * k * cin)).cuda().requires_grad_(True)
    pad = k // 2 if same else 0
    y = conv2d_leaky(x, w, pad, leaky)
    if not N.conv2d_instantiated(1, k, cin, cout):
        assert N.conv_last_dispatch()["family"] == FWD_ANY and N.conv_last_geometry() == dict(pad_y=pad, pad_x=pad, wrap_y=0, wrap_x=0)
    xd, wd = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    yd = F.conv2d(xd.permute(0, 3, 1, 2), wd, padding=pad)
    if leaky:
        yd = F.leaky_relu(yd, 0.2)
    yd = yd.permute(0, 2, 3, 1)
    assert y.shape == yd.shape
    assert rel(y, yd) < 2e-6
    g = torch.randn(y.shape, generator=gen).cuda()
    y.backward(g)                                            # (on autograd's thread: the dispatch record is per thread - the routing test names the kernels)
    yd.backward(g.double())
    assert rel(x.grad, xd.grad) < 3e-6, ("dx", rel(x.grad, xd.grad))
    assert rel(w.grad, wd.grad) < 3e-6, ("dw", rel(w.grad, wd.grad))


# ------------------------------------------------------------------------------------------------------------------------------------
def _pre_activations(net, x):
    """FullyConvNetwork.forward (SAME or wrapped, no crop) on the host path, layer by layer: the output and every layer's pre-activation"""
    from diffpiso.closure import conv2d_leaky
    pres, y, n = [], x, len(net.weights)
    for i, w in enumerate(net.weights):
        k = w.shape[-1]
        pre = conv2d_leaky(y, w, (k // 2, k // 2), False, wrap=net.wrap)
        pres.append(pre)
        y = torch.where(pre > 0, pre, 0.2 * pre) if i < n - 1 else pre
    return y, pres


def _margin(pres):
    """the smallest |pre-activation| of the layers a leaky ReLU follows, in units of its layer's r.m.s."""
    return min(float(p.detach().abs().min() / p.detach().pow(2).mean().sqrt()) for p in pres[:-1])


def _input_clear_of_zero(net_h, x0, rounds=12):
    """module docstring: the float32 input next to x0 whose float64 pre-activations keep 2e-4 r.m.s. from zero"""
    x = x0.double()
    for _ in range(rounds):
        xr = x.float().double().requires_grad_(True)
        _, pres = _pre_activations(net_h, xr)
        step, found = torch.zeros_like(xr), 0
        for p in pres[:-1]:
            rms = float(p.detach().pow(2).mean().sqrt())
            flat = p.reshape(-1)
            for j in torch.nonzero(flat.detach().abs() < 2 * MARGIN * rms).reshape(-1).tolist():
                v = flat[j]
                grad = torch.autograd.grad(v, xr, retain_graph=True)[0]
                v = float(v.detach())
                step += grad * (((1.0 if v > 0 else -1.0) * 3 * MARGIN * rms - v) / float((grad * grad).sum()))
                found += 1
        if found == 0:
            return xr.detach().float()
        x = xr.detach() + step
    raise AssertionError("the band around zero did not clear in %d rounds" % rounds)


@pytest.mark.parametrize("wrap", [(False, False), (True, True)], ids=["zero-padded", "wrapped"])
def test_network_of_given_layers_matches_the_float64_host_path(wrap):
    import diffpiso as dp
    import diffpiso._native as N
    net_h = dp.FullyConvNetwork(seed=3, layers=NET_LAYERS, in_channels=5, wrap=wrap)
    net = copy.deepcopy(net_h).cuda()
    net_h = net_h.double()
    x0 = _input_clear_of_zero(net_h, torch.randn(1, 24, 80, 5, generator=torch.Generator().manual_seed(3)))
    assert x0.dtype == torch.float32 and rel(x0, torch.randn(1, 24, 80, 5, generator=torch.Generator().manual_seed(3))) < 1e-3
    x1, x2 = x0.cuda().requires_grad_(True), x0.double().requires_grad_(True)
    out2, pres = _pre_activations(net_h, x2)
    assert _margin(pres) > MARGIN, _margin(pres)             # the precondition, from the float64 reference alone
    with torch.no_grad():
        assert rel(net_h(x0.double()), out2) < 1e-13          # (the layer loop above is the network's; torch may sum an int padding in another order)
    out1 = net(x1)
    # (the last layer, 1 x 1, 40 -> 2, has no fixed instance: the new family, which always reports its geometry)
    assert N.conv_last_dispatch()["family"] == FWD_ANY and N.conv_last_geometry() == dict(pad_y=0, pad_x=0, wrap_y=int(wrap[0]), wrap_x=int(wrap[1]))
    assert out1.shape == out2.shape == (1, 24, 80, 2)
    assert rel(out1, out2) < 5e-6
    g = torch.randn(out1.shape, generator=torch.Generator().manual_seed(1))
    out1.backward(g.cuda())
    out2.backward(g.double())
    assert rel(x1.grad, x2.grad) < 2e-5, rel(x1.grad, x2.grad)
    for a, b in zip(net.weights, net_h.weights):
        assert rel(a.grad, b.grad) < 2e-5, (tuple(a.shape), rel(a.grad, b.grad))


def _kernel_names(net, x):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net(x).sum().backward()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


def test_routing_new_layers_run_the_new_family_and_the_reference_network_the_old_kernels():
    import diffpiso as dp
    new = dp.FullyConvNetwork(seed=1, layers=NET_LAYERS, in_channels=5).cuda()
    ref = dp.FullyConvNetwork(seed=1).cuda()
    gen = torch.Generator().manual_seed(0)
    names_new = _kernel_names(new, torch.randn(1, 24, 80, 5, generator=gen).cuda().requires_grad_(True))
    names_ref = _kernel_names(ref, torch.randn(1, 24, 80, 4, generator=gen).cuda().requires_grad_(True))
    assert any("conv_forward_any" in n for n in names_new) and any("conv_wgrad_any" in n for n in names_new), names_new
    for names in (names_new, names_ref):
        assert not any("miopen" in n.lower() or "igemm" in n.lower() for n in names), names
    assert not any("conv_forward_any" in n or "conv_wgrad_any" in n for n in names_ref), names_ref
    assert any("conv_forward_kernel" in n or "conv_forward_lds_kernel" in n for n in names_ref) and any("conv_wgrad" in n for n in names_ref), names_ref


@pytest.mark.parametrize("k,cin,cout", [(7, 4, 16), (5, 16, 32), (3, 64, 64), (1, 64, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("leaky", [True, False])
def test_a_reference_layer_equals_the_three_old_entries_called_directly(k, cin, cout, leaky):
    """the code path of before the run-time-shaped family: piso_conv2d_forward, piso_conv2d_forward on the flipped weights, piso_conv2d_wgrad - bit for bit"""
    import diffpiso._native as N
    from diffpiso.closure import conv2d_leaky
    assert N.conv2d_instantiated(1, k, cin, cout) and N.conv2d_instantiated(1, k, cout, cin) and N.conv2d_instantiated(2, k, cin, cout)
    rng = np.random.default_rng(k + cin + cout)
    H, W, pad = 11, 70, k // 2
    x, w = rng.standard_normal((H, W, cin)).astype(f32), (rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(f32)
    g = rng.standard_normal((H, W, cout)).astype(f32)
    xt = torch.from_numpy(x)[None].cuda().requires_grad_(True)
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))).cuda().requires_grad_(True)
    y = conv2d_leaky(xt, wt, pad, leaky)
    assert N.conv_last_dispatch()["family"] in (0, 1) and N.conv_last_geometry() == {}
    y.backward(torch.from_numpy(g)[None].cuda())
    st, out = call_forward_old(x, w, pad, int(leaky))
    assert st == 0
    assert_bitwise(y.detach().cpu().numpy()[0], out, "forward")
    gp = np.where(out > 0, g, f32(0.2) * g).astype(f32) if leaky else g
    st, dx = call_forward_old(gp, flipped(w), k - 1 - pad, 0)
    assert st == 0
    assert_bitwise(xt.grad.cpu().numpy()[0], dx, "input gradient")
    st, dw = call_wgrad_old(x, gp, k, pad)
    assert st == 0
    assert_bitwise(np.ascontiguousarray(wt.grad.cpu().numpy().transpose(2, 3, 1, 0)), dw, "weight gradient")


def test_what_still_raises_states_the_limits():
    from diffpiso._native import PisoNativeError
    from diffpiso.closure import conv2d_leaky
    x = torch.randn(1, 8, 20, 5).cuda()
    for xx, w in ((torch.randn(2, 8, 20, 5).cuda(), torch.randn(24, 5, 5, 5).cuda()),          # batch 2
                  (x.double(), torch.randn(24, 5, 5, 5).cuda().double()),                       # float64
                  (x, torch.randn(24, 5, 4, 4).cuda()),                                          # even kernel size
                  (x, torch.randn(24, 5, 11, 11).cuda()),                                        # kernel size 11
                  (x, torch.randn(257, 5, 3, 3).cuda()),                                         # 257 output channels
                  (torch.randn(1, 4, 6, 257).cuda(), torch.randn(8, 257, 3, 3).cuda())):        # 257 input channels
        with pytest.raises(PisoNativeError, match="1 .. 9.*1 .. 256"):
            conv2d_leaky(xx, w, w.shape[-1] // 2, True)
