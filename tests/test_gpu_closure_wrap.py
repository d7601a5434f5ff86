"""The closure on a periodic domain, on the card: conv2d_leaky(wrap=...), FullyConvNetwork(wrap=...) and the coupling make_forcing_fn(wrap=...)
against the float64 host path (circular F.pad + torch's CPU convolution), with the bounds of tests/test_gpu_conv.py.

The network's GRADIENTS and the leaky ReLU.  A leaky ReLU makes the gradients of two differently rounded evaluations differ by a factor 5 on every
activation whose pre-activation lies within round-off of zero: the float32 and the float64 HOST paths of this very network disagree on the sign
of 1 - 2 of the 4.6 million activations at 250 x 72 for 6 of 8 seeds, which moves dL/dx and dL/dw by 1e-4 .. 2e-3 of their norm - a property of
the comparison, no statement about a kernel.  So:
  24 x 40    the test first requires of the float64 reference alone that every pre-activation is farther from zero than 5e-6 of its layer's
             r.m.s. (several times the float32 round-off of a pre-activation, measured 1e-6 r.m.s.; seed 9 has 7e-6 or more for every wrap):
             then a correct float32 evaluation has the reference's signs, and the gradients are compared as they are;
  250 x 72   the float64 host path is evaluated a second time with the slope of every activation taken from the CARD's sign of it, and the
             gradients are compared with that evaluation: the same bound asks the same of every kernel, and the one discrete choice that no
             bound can hold is pinned.  The card's signs may differ from the reference's only where the reference's pre-activation is within
             1e-5 of its layer's r.m.s. of zero (ten times the measured round-off) - elsewhere a differing sign is an error; the forward pass
             is held to the plain float64 host path at both sizes.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.cases import make_case, product_setup

pytestmark = pytest.mark.gpu
LAYERS = [(7, 4, 16), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 64), (1, 64, 64), (1, 64, 2)]
WRAPS = [(True, True), (False, True), (True, False)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30))


@pytest.mark.parametrize("k,cin,cout", LAYERS)
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("leaky", [True, False])
def test_layer_forward_and_gradients_match_the_float64_host_path(k, cin, cout, wrap, leaky):
    from diffpiso.closure import conv2d_leaky
    gen = torch.Generator(device="cpu").manual_seed(k * 100 + cin + cout)
    H, W = 19, 70
    x0 = torch.randn(1, H, W, cin, generator=gen)
    w0 = torch.randn(cout, cin, k, k, generator=gen) / np.sqrt(k * k * cin)
    pad = (k // 2 if wrap[0] else 0, k // 2 if wrap[1] else k - 1)           # the axis that is not wrapped: VALID in y, full in x
    x, w = x0.cuda().requires_grad_(True), w0.cuda().requires_grad_(True)
    y = conv2d_leaky(x, w, pad, leaky, wrap=wrap)
    xd, wd = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    yd = conv2d_leaky(xd, wd, pad, leaky, wrap=wrap)
    assert y.shape == yd.shape == (1, H + 2 * pad[0] - k + 1, W + 2 * pad[1] - k + 1, cout)
    assert rel(y, yd) < 2e-6
    g = torch.randn(y.shape, generator=gen)
    y.backward(g.cuda())
    yd.backward(g.double())
    assert rel(x.grad, xd.grad) < 3e-6, ("dx", rel(x.grad, xd.grad))
    assert rel(w.grad, wd.grad) < 3e-6, ("dw", rel(w.grad, wd.grad))


def _host_activations(net, x):
    """the outputs of every layer on the host path"""
    import diffpiso.closure as closure
    acts, orig = [], closure.conv2d_leaky

    def rec(*a, **k):
        y = orig(*a, **k)
        acts.append(y.detach())
        return y
    closure.conv2d_leaky = rec
    try:
        out = net(x)
    finally:
        closure.conv2d_leaky = orig
    return out, acts


def _host_forward_with_signs(net, x, signs, hw):
    """FullyConvNetwork.forward on the host path (no buffer_width crop) with the slope of every leaky ReLU given: signs[i] true -> 1, else 0.2"""
    from diffpiso.closure import conv2d_leaky
    same, (wrap_y, wrap_x), n = net.padding == "SAME", net.wrap, len(net.weights)
    y = x
    for i, w in enumerate(net.weights):
        k = w.shape[-1]
        pre = conv2d_leaky(y, w, (k // 2 if same or wrap_y else 0, k // 2 if same or wrap_x else 0), False, wrap=net.wrap)
        y = torch.where(signs[i], pre, 0.2 * pre) if i < n - 1 else pre
    if not same:                                         # restore_shape: zeros back on the axes that shrank
        pn_y, pn_x = (0 if wrap_y else net.reduced_buffer_width), (0 if wrap_x else net.reduced_buffer_width)
        y = F.pad(y, (0, 0, pn_x, hw[1] - y.shape[2] - pn_x, pn_y, hw[0] - y.shape[1] - pn_y))
    return y


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("padding", ["SAME", "VALID"])
def test_network_matches_the_float64_host_path_and_runs_the_ex_kernels(wrap, padding):
    import diffpiso as dp
    import diffpiso._native as N
    bw = None if padding == "SAME" else [[0, 0], [0, 0]]
    net_h, _, _ = dp.initialise_fullyconv_network(bw, padding=padding, restore_shape=True, seed=9, wrap=wrap)
    net = copy.deepcopy(net_h).cuda()
    net_h = net_h.double()
    # ---- 24 x 40: forward and gradients
    x0 = torch.randn(1, 24, 40, 4, generator=torch.Generator().manual_seed(0))
    x1, x2 = x0.cuda().requires_grad_(True), x0.double().requires_grad_(True)
    out1 = net(x1)
    assert N.conv_last_geometry() == dict(pad_y=0, pad_x=0, wrap_y=int(wrap[0]), wrap_x=int(wrap[1]))        # (the last layer: 1 x 1)
    out2, acts = _host_activations(net_h, x2)
    if padding == "SAME":                                # the precondition of the gradient comparison (module docstring), from the reference alone
        for a in acts[:-1]:
            pre = torch.where(a > 0, a, a / 0.2)
            assert float(pre.abs().min() / pre.pow(2).mean().sqrt()) > 5e-6
    assert out1.shape == out2.shape == (1, 24, 40, 2)
    assert rel(out1, out2) < 5e-6
    if padding == "VALID" and wrap != (True, True):      # only the axis that is not wrapped was cropped and padded back
        rb = net.reduced_buffer_width
        cropped = out1[:, :rb] if not wrap[0] else out1[:, :, :rb]
        assert float(cropped.abs().max()) == 0.0
    if padding == "SAME":
        g = torch.randn(out1.shape, generator=torch.Generator().manual_seed(1))
        out1.backward(g.cuda())
        out2.backward(g.double())
        assert rel(x1.grad, x2.grad) < 2e-5
        for a, b in zip(net.weights, net_h.weights):
            assert rel(a.grad, b.grad) < 2e-5
    # ---- 250 x 72: 250 row bands of the weight gradient, two tiles per row
    x0 = torch.randn(1, 250, 72, 4, generator=torch.Generator().manual_seed(2))
    x1, x2 = x0.cuda().requires_grad_(True), x0.double().requires_grad_(True)
    for w in net.weights:
        w.grad = None
    for w in net_h.weights:
        w.grad = None
    out1, acts1 = _host_activations(net, x1)              # (the recorder works on any path: here the card's layer outputs)
    with torch.no_grad():
        out2, acts2 = _host_activations(net_h, x0.double())
    assert out1.shape == out2.shape == (1, 250, 72, 2)
    assert rel(out1, out2) < 5e-6
    signs, flips = [], 0
    for a1, a2 in zip(acts1[:-1], acts2[:-1]):
        pre = torch.where(a2 > 0, a2, a2 / 0.2)
        card = (a1 > 0).cpu()
        differ = card != (pre > 0)
        flips += int(differ.sum())
        assert bool((pre.abs()[differ] < 1e-5 * pre.pow(2).mean().sqrt()).all())          # only inside the round-off of zero
        signs.append(card)
    print("activations whose sign on the card differs from the float64 reference's: %d" % flips)
    out3 = _host_forward_with_signs(net_h, x2, signs, (250, 72))
    assert rel(out1, out3) < 5e-6
    g = torch.randn(out1.shape, generator=torch.Generator().manual_seed(3))
    out1.backward(g.cuda())
    out3.backward(g.double())
    assert rel(x1.grad, x2.grad) < 2e-5
    for a, b in zip(net.weights, net_h.weights):
        assert rel(a.grad, b.grad) < 2e-5


def test_wrapped_network_commutes_with_a_circular_shift_on_the_card():
    from diffpiso.closure import FullyConvNetwork
    x = torch.randn(1, 32, 32, 4, generator=torch.Generator().manual_seed(7)).cuda()
    shift = (3, 5)
    defect = {}
    for wrap in ((True, True), (False, False)):
        net = FullyConvNetwork(seed=1, wrap=wrap).cuda()
        with torch.no_grad():
            defect[wrap] = rel(net(torch.roll(x, shift, (1, 2))), torch.roll(net(x), shift, (1, 2)))
    print("shift defect on the card: wrapped %.3g, zero padded %.3g" % (defect[(True, True)], defect[(False, False)]))
    assert defect[(True, True)] <= 2 * 5e-6
    assert defect[(False, False)] > 0.1                   # the same weights with zeros at the edge: the test discriminates


def test_coupling_averages_across_the_seam_and_unrolls():
    import diffpiso as dp
    c = make_case("periodic", 16, 24, seed=2)
    P = product_setup(c)
    net = dp.FullyConvNetwork(seed=1, wrap=(True, True)).cuda()
    with torch.no_grad():
        for w in net.weights:
            w.mul_(0.3)
    forcing_fn = dp.make_forcing_fn(net, wrap=(True, True))
    with torch.no_grad():
        f = forcing_fn(0, P["velocity"], P["pressure"])
    assert f.shape == (1, 17, 25, 2)
    v, u = f[0, :, :24, 0], f[0, :16, :, 1]
    assert float(v.abs().max()) > 0 and float(u.abs().max()) > 0
    assert torch.equal(v[0], v[16]) and torch.equal(u[:, 0], u[:, 24])          # face 0 and face n are the same face
    with torch.no_grad():
        f0 = dp.make_forcing_fn(net)(0, P["velocity"], P["pressure"])
    assert not torch.equal(f0[0, 0, :24, 0], f0[0, 16, :24, 0])                 # wrap=None: the replicated edge, as ever
    vel_t = P["vel_tensor"].clone().requires_grad_(True)
    velocity = dp.StaggeredGrid(vel_t, P["velocity"].box, extrapolation=P["velocity"].extrapolation)
    _, _, vn, pn, _ = dp.unroll_piso_steps(velocity, P["pressure"], c["dt"], P["sim"], step_count=2, forcing_fn=forcing_fn)
    out = vn.staggered_tensor()
    assert bool(torch.isfinite(out).all())
    (0.5 * (out ** 2).sum()).backward()
    assert bool(torch.isfinite(vel_t.grad).all()) and float(vel_t.grad.abs().max()) > 0
    for w in net.weights:
        assert bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0


def test_buffer_width_on_a_wrapped_axis_is_refused():
    import diffpiso as dp
    with pytest.raises(ValueError, match="buffer_width"):
        dp.FullyConvNetwork(buffer_width=[[0, 0], [3, 3]], wrap=(False, True))
    with pytest.raises(ValueError, match="buffer_width"):
        dp.initialise_fullyconv_network([[1, 0], [0, 0]], wrap=(True, False))
    net = dp.FullyConvNetwork(buffer_width=[[2, 2], [0, 0]], wrap=(False, True)).cuda()                     # the other axis may be cropped
    assert net(torch.randn(1, 20, 24, 4).cuda()).shape == (1, 20, 24, 2)
