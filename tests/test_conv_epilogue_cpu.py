"""Bias, skip connections and ReLU of the closure layers, the parts that need no card.

  * the four entries of csrc/conv_epilogue.hip are declared in include/piso_hip.h, exported by the library and bound by diffpiso._native;
  * the banding of the bias sum (piso_conv_epilogue_plan / piso_conv_epilogue_workspace_bytes) against its rule restated here;
  * conv2d_act on host tensors in float64 against the formula written out with F.conv2d;
  * FullyConvNetwork with the new keywords at their defaults is the network it was; every ValueError; skips and biases in the written-out chain;
  * initialise_fullyconv_network(bias=True) returns the weights followed by the biases.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHANNELS = (1, 2, 3, 4, 5, 16, 20, 64, 256)


def cdiv(a, b):
    return -(-a // b)


def expected_plan(pixels, channels):
    """include/piso_hip.h: pixels_per_band = max(ceil(4096 / channels), ceil(pixels / 1024)), bands = ceil(pixels / pixels_per_band)"""
    ppb = max(cdiv(4096, channels), cdiv(pixels, 1024))
    return cdiv(pixels, ppb), ppb


def test_the_entries_are_declared_exported_and_bound():
    import diffpiso
    import diffpiso._native as N
    hdr = open(os.path.join(ROOT, "include", "piso_hip.h")).read()
    for decl in ("int piso_conv_epilogue_plan(int pixels, int channels, int* bands, int* pixels_per_band);",
                 "size_t piso_conv_epilogue_workspace_bytes(int pixels, int channels);",
                 "int piso_conv_epilogue_forward(const float* z, const float* bias, const float* skip, float* y, int pixels, int channels, int act, piso_stream_t stream);",
                 "int piso_conv_epilogue_backward(const float* g, const float* y, float* gpre, float* dbias, int pixels, int channels, int act, float* ws, size_t ws_elems,"):
        assert decl in hdr, decl
    assert "[pixels][channels]" in hdr and "Summation order of dbias" in hdr and "act((z[p][c] + bias[c]) + skip[p][c])" in hdr
    assert len(N.lib.piso_conv_epilogue_forward.argtypes) == 8 and len(N.lib.piso_conv_epilogue_backward.argtypes) == 10
    assert len(N.lib.piso_conv_epilogue_plan.argtypes) == 4 and len(N.lib.piso_conv_epilogue_workspace_bytes.argtypes) == 2
    assert N.lib.piso_conv_epilogue_forward.restype is C.c_int and N.lib.piso_conv_epilogue_backward.restype is C.c_int
    assert N.lib.piso_conv_epilogue_plan.restype is C.c_int and N.lib.piso_conv_epilogue_workspace_bytes.restype is C.c_size_t
    assert callable(diffpiso.conv2d_act) and "conv2d_act" in diffpiso.__all__


def test_plan_and_workspace_agree_and_are_monotone():
    import diffpiso._native as N
    for channels in CHANNELS:
        base = cdiv(4096, channels)
        last_bytes = 0
        for pixels in sorted({1, 2, base - 1, base, base + 1, 3 * base + 5, 256 * 896, 1024 * base - 1, 1024 * base, 1024 * base + 1, 1025 * base, 2048 * base + 7,
                              2048 * 2048}):
            if pixels < 1:
                continue
            bands, ppb = N.conv_epilogue_plan(pixels, channels)
            assert (bands, ppb) == expected_plan(pixels, channels), (pixels, channels)
            assert bands * ppb >= pixels > (bands - 1) * ppb and 1 <= bands <= 1024
            nbytes = N.lib.piso_conv_epilogue_workspace_bytes(pixels, channels)
            # bands x channels x 4 up to 1024 bands of the smallest size; beyond, its bound 1024 x channels x 4 (bands itself dips there: 1025 base pixels are 513 bands)
            assert nbytes == min(cdiv(pixels, base), 1024) * channels * 4 >= bands * channels * 4
            if pixels <= 1024 * base:
                assert nbytes == bands * channels * 4 and ppb == base
            assert nbytes >= last_bytes
            last_bytes = nbytes
    # refusals of the host-only entries: a status and a message, nothing written
    bands, ppb = C.c_int(-7), C.c_int(-7)
    for pixels, channels, words in ((0, 4, "pixels"), (-1, 4, "pixels"), (10, 0, "channels"), (10, 257, "channels")):
        assert N.lib.piso_conv_epilogue_plan(pixels, channels, C.byref(bands), C.byref(ppb)) == 1
        assert words in N.lib.piso_last_error_string().decode() and (bands.value, ppb.value) == (-7, -7)
        assert N.lib.piso_conv_epilogue_workspace_bytes(pixels, channels) == 0
    with pytest.raises(N.PisoNativeError):
        N.conv_epilogue_plan(0, 4)


def _act(v, activation):
    return {"leaky_relu": lambda t: F.leaky_relu(t, 0.2), "relu": F.relu, None: lambda t: t}[activation](v)


@pytest.mark.parametrize("activation", ["leaky_relu", "relu", None])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("wrap", [(False, False), (True, True), (False, True)])
def test_host_path_of_conv2d_act_is_the_written_out_formula(activation, with_bias, with_skip, wrap):
    from diffpiso.closure import conv2d_act, conv2d_leaky
    gen = torch.Generator().manual_seed(11)
    k, cin, cout, H, W = 3, 5, 5, 9, 11
    x = torch.randn(1, H, W, cin, dtype=torch.float64, generator=gen)
    w = torch.randn(cout, cin, k, k, dtype=torch.float64, generator=gen)
    b = torch.randn(cout, dtype=torch.float64, generator=gen) if with_bias else None
    s = torch.randn(1, H, W, cout, dtype=torch.float64, generator=gen) if with_skip else None
    xc = x.permute(0, 3, 1, 2)
    if wrap[0] or wrap[1]:
        xc = F.pad(xc, (1 if wrap[1] else 0, 1 if wrap[1] else 0, 1 if wrap[0] else 0, 1 if wrap[0] else 0), mode="circular")
    want = F.conv2d(xc, w, padding=(0 if wrap[0] else 1, 0 if wrap[1] else 1)).permute(0, 2, 3, 1)
    if b is not None:
        want = want + b
    if s is not None:
        want = want + s
    want = _act(want, activation)
    pad = 1 if wrap == (False, False) else (1, 1)
    got = conv2d_act(x, w, pad, activation, b, s, wrap=wrap)
    assert got.dtype == torch.float64 and got.shape == (1, H, W, cout) and torch.equal(got, want)
    if b is None and s is None and activation != "relu":
        assert torch.equal(got, conv2d_leaky(x, w, pad, activation == "leaky_relu", wrap=wrap))
    with pytest.raises(ValueError):
        conv2d_act(x, w, pad, "tanh", b, s, wrap=wrap)


REFERENCE = [(7, 4, 16), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 64), (1, 64, 64), (1, 64, 2)]
RESIDUAL = [(3, 4, 8), (3, 8, 8), (3, 8, 8), (1, 8, 2)]


def test_defaults_of_the_new_keywords_give_the_network_of_before():
    from diffpiso.closure import FullyConvNetwork
    x = torch.randn(1, 23, 25, 4, generator=torch.Generator().manual_seed(2))            # (VALID takes 18 rows and columns off the reference's network)
    for kw in (dict(), dict(layers=RESIDUAL), dict(layers=RESIDUAL, wrap=(True, False)), dict(padding="VALID")):
        a = FullyConvNetwork(seed=5, **kw)
        b = FullyConvNetwork(seed=5, bias=False, activation="leaky_relu", skips=None, **kw)
        c = FullyConvNetwork(seed=5, bias=[False] * len(a.weights), skips={}, **kw)
        layers = kw.get("layers", REFERENCE)
        assert list(a.state_dict().keys()) == ["weights.%d" % i for i in range(len(layers))]
        for other in (b, c):
            assert list(other.state_dict().keys()) == list(a.state_dict().keys()) and len(list(other.parameters())) == len(layers)
            assert all(torch.equal(p, q) for p, q in zip(a.parameters(), other.parameters()))
        assert len(a.biases) == 0 and a.activation == "leaky_relu" and a.skips == {}
        # the chain of before, written out
        y = x.permute(0, 3, 1, 2)
        for i, w in enumerate(a.weights):
            k = w.shape[-1]
            same = kw.get("padding", "SAME") == "SAME"
            if kw.get("wrap"):
                y = F.conv2d(F.pad(y, (0, 0, k // 2, k // 2), mode="circular"), w, padding=(0, k // 2))
            else:
                y = F.conv2d(y, w, padding=k // 2 if same else 0)
            if i < len(a.weights) - 1:
                y = F.leaky_relu(y, 0.2)
        with torch.no_grad():
            assert torch.equal(a(x), y.permute(0, 2, 3, 1)) and torch.equal(b(x), a(x)) and torch.equal(c(x), a(x))
    # a bias draws nothing: the weights of a seeded network are the same with and without
    d = FullyConvNetwork(seed=5, bias=True)
    assert all(torch.equal(p, q) for p, q in zip(FullyConvNetwork(seed=5).weights, d.weights))
    assert [tuple(p.shape) for p in d.biases] == [(c,) for _, _, c in REFERENCE] and all(float(p.detach().abs().max()) == 0.0 for p in d.biases)
    assert list(d.state_dict().keys()) == ["weights.%d" % i for i in range(7)] + ["biases.%d" % i for i in range(7)]


def test_the_network_calls_conv2d_leaky_with_the_arguments_of_before():
    """whatever stands in for closure.conv2d_leaky - the torch checker of tests/closure_checker.py takes (x, w, pad, leaky) and nothing else - sees the
    call it always saw: four arguments without a wrapped axis, `wrap=` only with one"""
    import diffpiso.closure as closure
    from tests.closure_checker import torch_convolutions
    x = torch.randn(1, 23, 25, 4, generator=torch.Generator().manual_seed(2))
    for kw in (dict(), dict(padding="VALID"), dict(layers=RESIDUAL, bias=True, skips={2: 1}, activation="relu")):
        net = closure.FullyConvNetwork(seed=5, **kw)
        with torch.no_grad():
            want = net(x)
            with torch_convolutions():
                assert torch.equal(net(x), want)
    calls, orig = [], closure.conv2d_leaky

    def rec(*a, **k):
        calls.append((len(a), dict(k)))
        return orig(*a, **k)
    closure.conv2d_leaky = rec
    try:
        with torch.no_grad():
            closure.FullyConvNetwork(seed=5, layers=RESIDUAL)(x)
            closure.FullyConvNetwork(seed=5, layers=RESIDUAL, wrap=(False, True))(x)
    finally:
        closure.conv2d_leaky = orig
    assert calls[:4] == [(3, dict(leaky=True))] * 3 + [(3, dict(leaky=False))]
    assert calls[4:] == [(3, dict(leaky=True, wrap=(False, True)))] * 3 + [(3, dict(leaky=False, wrap=(False, True)))]


@pytest.mark.parametrize("activation", ["relu", "leaky_relu", None])
def test_residual_network_on_host_tensors_is_the_written_out_chain(activation):
    from diffpiso.closure import FullyConvNetwork
    net = FullyConvNetwork(seed=3, layers=RESIDUAL, bias=[True, False, True, True], skips={2: 1, 1: 1}, activation=activation).double()
    assert len(net.biases) == 3 and net.bias_of_layer == [0, None, 1, 2] and net.reduced_buffer_width == 3
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for p in net.biases:
            p.copy_(torch.randn(p.shape, dtype=torch.float64, generator=gen))
    x = torch.randn(1, 13, 15, 4, dtype=torch.float64, generator=gen)
    w, b = list(net.weights), list(net.biases)
    t = x.permute(0, 3, 1, 2)
    a0 = _act(F.conv2d(t, w[0], padding=1) + b[0].view(1, -1, 1, 1), activation)
    a1 = _act(F.conv2d(a0, w[1], padding=1) + a0, activation)                                    # {1: 1}: its own input
    a2 = _act((F.conv2d(a1, w[2], padding=1) + b[1].view(1, -1, 1, 1)) + a0, activation)         # {2: 1}: the input of layer 1
    want = (F.conv2d(a2, w[3]) + b[2].view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    with torch.no_grad():
        assert torch.equal(net(x), want)
    # reverse mode reaches every parameter, and the biases of a gradient check are those of the formula
    net(x).square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in net.parameters())


def test_bad_keywords_are_refused():
    from diffpiso.closure import FullyConvNetwork
    ok = dict(layers=RESIDUAL)
    FullyConvNetwork(skips={2: 1, 1: 1, 0: 0}, layers=[(3, 8, 8), (3, 8, 8), (3, 8, 8), (1, 8, 2)])
    FullyConvNetwork(skips={2: 1}, padding="VALID", wrap=(True, True), **ok)                      # both axes wrapped: every layer keeps its extent
    FullyConvNetwork(skips={1: 0}, padding="VALID", layers=[(1, 4, 8), (1, 8, 4)])                # k == 1 keeps it too
    for bad in (dict(skips={1: 2}), dict(skips={2: -1}), dict(skips={4: 1}),                      # 0 <= i <= j < layers
                dict(skips={2: 0}), dict(skips={3: 1}), dict(skips={0: 0}),                       # cin_i != cout_j: 4 != 8, 8 != 2, 4 != 8
                dict(skips={2: 1}, padding="VALID"), dict(skips={2: 1}, padding="VALID", wrap=(True, False)), dict(skips={2: 1}, padding="VALID", wrap=(False, True)),
                dict(bias=[True, False]), dict(bias=[True] * 5), dict(activation="tanh"), dict(activation="LEAKY_RELU")):
        with pytest.raises(ValueError):
            FullyConvNetwork(**dict(ok, **bad))


def test_initialise_returns_the_weights_followed_by_the_biases():
    from diffpiso.closure import initialise_fullyconv_network
    net, params, rbw = initialise_fullyconv_network(None, seed=4, layers=RESIDUAL, bias=True, activation="relu", skips={2: 1})
    assert rbw == 3 and net.activation == "relu" and net.skips == {2: 1}
    assert len(params) == 8 and all(p is q for p, q in zip(params, list(net.weights) + list(net.biases)))
    assert [tuple(p.shape) for p in params[4:]] == [(8,), (8,), (8,), (2,)]
    assert {id(p) for p in params} == {id(p) for p in net.parameters()}
    net2, params2, _ = initialise_fullyconv_network(None, seed=4, layers=RESIDUAL, bias=[False, True, False, False])
    assert len(params2) == 5 and params2[4] is net2.biases[0] and tuple(params2[4].shape) == (8,)
    _, params3, _ = initialise_fullyconv_network(None, seed=4)
    assert len(params3) == 7
