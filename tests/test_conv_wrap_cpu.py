"""Wrap-around padding of the closure convolutions, the parts that need no card.

  * conv_plan (csrc/conv_dispatch.h) is walked on the host for the queries of piso_conv2d_forward_ex / piso_conv2d_wgrad_ex
    (tests/conv_plan_ex_driver.cpp): both rules of a wrapped axis, the family chosen by the rules of the old entries, the 15-field record;
  * the three entries are declared in include/piso_hip.h, exported by the library and bound by diffpiso._native;
  * the host path (circular F.pad + torch's convolution) in float64: the wrapped network commutes with a circular shift, the zero-padded one
    does not;
  * centered_to_staggered(wrap=...) against a three-line numpy restatement.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FWD_DIRECT, FWD_LDS, WG_GENERIC, WG_GENERIC_LDS, WG_PACK4, WG_64, WG_64_LDS = range(7)
FIELDS = ("entry", "KS", "C", "NT", "IPW", "family", "leaky", "grid_x", "grid_y", "block", "rows_per_block", "nblocks", "reducer", "Ho", "Wo")


def expected_record(entry, H, W, cin, cout, ks, pad_y, pad_x, leaky, conv_lds):
    """The dispatch rules of the old entries restated (tests/test_gpu_conv_dispatch.py: expected_record) with the output extents of a padding
    per axis: what a *_ex call must report - the geometry changes no choice."""
    Ho, Wo = H + 2 * pad_y - ks + 1, W + 2 * pad_x - ks + 1
    nt = -(-cout // 16)
    if entry == 1:
        cinp = 4 if cin <= 4 else -(-cin // 16) * 16
        tiles = -(-Wo // 64) * Ho
        return dict(entry=1, KS=ks, C=cinp, NT=nt, IPW=0, family=int(bool(conv_lds) and cinp >= 16 and ks >= 3), leaky=int(bool(leaky)), grid_x=-(-tiles // 4),
                    grid_y=1, block=256, rows_per_block=0, nblocks=0, reducer=0, Ho=Ho, Wo=Wo)
    mti = -(-cin // 16)
    rpb = -(-Ho // 256)
    nblocks = -(-Ho // rpb)
    reducer = 4 if cout % 4 == 0 else 1
    if (ks, cin, cout) == (3, 64, 64):
        ipw, family, grid_y, block = 1, WG_64_LDS if conv_lds else WG_64, 3, 192
    elif ks == 7 and cin <= 4 and nt == 1:
        ipw, family, grid_y, block = 1, WG_PACK4, -(-(7 * 2) // 4), 256
    else:
        ipw = {7: 3, 5: 2, 3: 1, 1: 1}[ks]
        family = WG_GENERIC_LDS if (conv_lds and cin % 4 == 0 and cout % 4 == 0) else WG_GENERIC
        grid_y, block = -(-(ks * ks * mti) // (4 * ipw)), 256
    return dict(entry=2, KS=ks, C=mti, NT=nt, IPW=ipw, family=family, leaky=0, grid_x=nblocks, grid_y=grid_y, block=block, rows_per_block=rpb, nblocks=nblocks,
                reducer=reducer, Ho=Ho, Wo=Wo)


f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------------------------
# the float64 references of tests/test_gpu_conv_wrap.py, from the definition of include/piso_hip.h; held to torch below
def _src(n_out, k, pad, n, wrap):
    """source index of tap k for every output index, and whether it contributes"""
    idx = np.arange(n_out) + k - pad
    if wrap:
        return idx % n, np.ones(n_out, bool)
    ok = (idx >= 0) & (idx < n)
    return np.where(ok, idx, 0), ok


def _extents(H, W, ks, pad):
    return H + 2 * pad[0] - ks + 1, W + 2 * pad[1] - ks + 1


def _window(x, ky, kx, Ho, Wo, pad, wrap):
    """in[Y][X][:] of tap (ky, kx) for every output pixel; zero where the tap leaves a zero-padded axis"""
    iy, oky = _src(Ho, ky, pad[0], x.shape[0], wrap[0])
    ix, okx = _src(Wo, kx, pad[1], x.shape[1], wrap[1])
    return np.where((oky[:, None] & okx[None, :])[..., None], x[iy][:, ix].astype(f64), 0.0), iy, ix, oky[:, None] & okx[None, :]


def ref_forward(x, w, pad, wrap):
    ks = w.shape[0]
    Ho, Wo = _extents(x.shape[0], x.shape[1], ks, pad)
    out = np.zeros((Ho, Wo, w.shape[3]), f64)
    for ky in range(ks):
        for kx in range(ks):
            out += _window(x, ky, kx, Ho, Wo, pad, wrap)[0] @ w[ky, kx].astype(f64)
    return out


def ref_wgrad(x, g, ks, pad, wrap):
    Ho, Wo, cout = g.shape
    dw = np.zeros((ks, ks, x.shape[2], cout), f64)
    g2 = g.reshape(Ho * Wo, cout).astype(f64)
    for ky in range(ks):
        for kx in range(ks):
            dw[ky, kx] = _window(x, ky, kx, Ho, Wo, pad, wrap)[0].reshape(Ho * Wo, -1).T @ g2
    return dw


def ref_dgrad(g, w, pad, wrap, H, W):
    """every output pixel scatters its gradient to the input pixels it read: dx[Y][X][ci] += g[y][x][co] w[ky][kx][ci][co]"""
    ks, (Ho, Wo, _) = w.shape[0], g.shape
    dx = np.zeros((H, W, w.shape[2]), f64)
    for ky in range(ks):
        for kx in range(ks):
            iy, oky = _src(Ho, ky, pad[0], H, wrap[0])
            ix, okx = _src(Wo, kx, pad[1], W, wrap[1])
            contrib = np.where((oky[:, None] & okx[None, :])[..., None], g.astype(f64) @ w[ky, kx].astype(f64).T, 0.0)
            np.add.at(dx, (iy[:, None], ix[None, :]), contrib)
    return dx


def leaky32(v64):
    v = v64.astype(f32)
    return np.where(v > 0, v, f32(0.2) * v).astype(f32)



def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cxx in ("c++", "g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        path = shutil.which(cxx)
        if path:
            return [path]
    hipcc = shutil.which("hipcc") or shutil.which(os.path.join(rocm, "bin", "hipcc"))
    return [hipcc, "-x", "c++"] if hipcc else None


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(queries) -> [(status, message, record dict, (ex, pad_y, pad_x, wrap_h, wrap_w))]; a query is (entry, H, W, cin, cout, ks, pad_y, pad_x, wrap_y,
    wrap_x, leaky, conv_lds, null_ptr, operands_off16, result_off16, workspace_bytes)."""
    cxx = _host_compiler()
    assert cxx is not None, "no C++17 host compiler (tried c++, g++, clang++, ROCm's clang++, hipcc -x c++)"
    exe = str(tmp_path_factory.mktemp("conv_plan_ex") / "conv_plan_ex_driver")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "conv_plan_ex_driver.cpp")], check=True)
    # (the driver of the old entries initialises the first 13 fields of ConvQuery positionally: it must keep compiling next to the new fields)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-o", exe + "_old", os.path.join(HERE, "conv_plan_driver.cpp")], check=True)

    def run(queries):
        text = "".join(" ".join(str(int(v)) for v in q) + "\n" for q in queries)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(lines) == len(queries)
        out = []
        for line in lines:
            status, msg, *rest = line.split("\t")
            assert len(rest) == len(FIELDS) + 5
            out.append((int(status), msg, dict(zip(FIELDS, map(int, rest[:len(FIELDS)]))), tuple(map(int, rest[len(FIELDS):]))))
        return out
    return run


# (ks, cin, cout): the layers of the network, their input-gradient shapes, and channel counts only the C ABI reaches
FWD_SHAPES = [(7, 4, 16), (7, 16, 4), (5, 16, 16), (5, 16, 32), (5, 32, 16), (3, 32, 64), (3, 64, 32), (3, 64, 64), (1, 64, 64), (1, 64, 2), (1, 2, 64), (7, 2, 3), (3, 64, 17),
              (1, 3, 63)]
WG_SHAPES = [(7, 4, 16), (7, 16, 4), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 60), (3, 64, 64), (1, 64, 64), (1, 64, 2), (3, 17, 63)]


def test_plan_of_the_ex_entries_chooses_by_the_old_rules(plan):
    """Every shape, wrap, conv_lds value and a few sizes: accepted, the record of the old rules, the geometry as asked."""
    queries, want = [], []
    for entry, shapes in ((1, FWD_SHAPES), (2, WG_SHAPES)):
        for ks, cin, cout in shapes:
            for wrap_y, wrap_x in ((0, 0), (1, 1), (0, 1), (1, 0)):
                for H, W in ((9, 64), (5, 70), (6, 129), (513, 6), (max(ks // 2, 1), max(ks // 2, 1))):
                    for lds in (-1, 0, 1):
                        pad_y = ks // 2 if (wrap_y or H < ks) else 0             # a zero-padded axis: VALID where the image allows it
                        pad_x = ks // 2 if (wrap_x or W < ks) else ks - 1
                        leaky = (H + lds) % 2 if entry == 1 else 0
                        queries.append((entry, H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, leaky, lds, 0, 0, 0, -1))
                        want.append((expected_record(entry, H, W, cin, cout, ks, pad_y, pad_x, leaky, lds), (1, pad_y, pad_x, H if wrap_y else 0, W if wrap_x else 0)))
    bad = {}
    for q, (status, msg, rec, geom), (wrec, wgeom) in zip(queries, plan(queries), want):
        if (status, msg) != (0, "-") or rec != wrec or geom != wgeom:
            bad[q] = (status, msg, rec, wrec, geom, wgeom)
    assert bad == {}
    assert {w[0]["family"] for w in want} == set(range(7))


def test_plan_refuses_what_breaks_a_rule_of_a_wrapped_axis(plan):
    INVALID = 1
    cases = {
        # wrap with pad != ks / 2
        "fwd wrap_y pad_y 0": ((1, 9, 64, 16, 16, 5, 0, 2, 1, 0, 0, -1, 0, 0, 0, 0), "pad == ks / 2"),
        "fwd wrap_x pad_x ks - 1": ((1, 9, 64, 16, 16, 5, 2, 4, 0, 1, 0, -1, 0, 0, 0, 0), "pad == ks / 2"),
        "fwd both, pad_x 1": ((1, 9, 64, 4, 16, 7, 3, 1, 1, 1, 0, -1, 0, 0, 0, 0), "pad == ks / 2"),
        "wg wrap_x pad_x 0": ((2, 9, 64, 64, 64, 3, 1, 0, 0, 1, 0, -1, 0, 0, 0, -1), "pad == ks / 2"),
        "wg wrap_y pad_y 2": ((2, 9, 64, 64, 64, 3, 2, 1, 1, 0, 0, -1, 0, 0, 0, -1), "pad == ks / 2"),
        # extent below the pad
        "fwd H 2 < pad 3": ((1, 2, 64, 4, 16, 7, 3, 3, 1, 1, 0, -1, 0, 0, 0, 0), "extent >= its pad"),
        "fwd W 1 < pad 2": ((1, 9, 1, 16, 16, 5, 2, 2, 0, 1, 0, -1, 0, 0, 0, 0), "extent >= its pad"),
        "wg W 2 < pad 3": ((2, 9, 2, 4, 16, 7, 3, 3, 1, 1, 0, -1, 0, 0, 0, -1), "extent >= its pad"),
        # the refusals of the old entries
        "fwd null": ((1, 9, 64, 16, 16, 5, 2, 2, 1, 1, 0, -1, 1, 0, 0, 0), "piso_conv2d_forward"),
        "fwd off 16": ((1, 9, 64, 16, 16, 5, 2, 2, 1, 1, 0, -1, 0, 1, 0, 0), "16-byte aligned"),
        "fwd cin 5": ((1, 9, 64, 5, 16, 5, 2, 2, 1, 1, 0, -1, 0, 0, 0, 0), "piso_conv2d_forward"),
        "fwd not instantiated": ((1, 9, 64, 64, 64, 5, 2, 2, 1, 1, 0, -1, 0, 0, 0, 0), "not instantiated"),
        "fwd Wo < 1": ((1, 9, 3, 16, 16, 5, 2, 0, 1, 0, 0, -1, 0, 0, 0, 0), "piso_conv2d_forward"),
        "wg workspace short": ((2, 9, 64, 16, 16, 5, 2, 2, 1, 1, 0, -1, 0, 0, 0, 256 * 25 * 16 * 16 * 4 - 1), "piso_conv2d_wgrad"),
        "wg dw off 16": ((2, 9, 64, 16, 16, 5, 2, 2, 1, 1, 0, -1, 0, 0, 1, -1), "16-byte aligned"),
        "wg not instantiated": ((2, 9, 64, 4, 32, 7, 3, 3, 1, 1, 0, -1, 0, 0, 0, -1), "not instantiated"),
    }
    got = plan([q for q, _ in cases.values()])
    bad = {name: (status, msg) for (name, (_, words)), (status, msg, _, _) in zip(cases.items(), got) if status != INVALID or words not in msg}
    assert bad == {}
    # the rule is stated under the entry's own name
    for (name, (q, _)), (_, msg, _, _) in zip(cases.items(), got):
        if "pad" in name or "<" in name and "Wo" not in name:
            assert msg.startswith("piso_conv2d_forward_ex: " if q[0] == 1 else "piso_conv2d_wgrad_ex: "), (name, msg)
    # pad == extent is allowed: an index wraps once
    ok = plan([(1, 3, 3, 4, 16, 7, 3, 3, 1, 1, 0, -1, 0, 0, 0, 0), (2, 2, 2, 16, 16, 5, 2, 2, 1, 1, 0, -1, 0, 0, 0, -1), (1, 1, 1, 64, 64, 3, 1, 1, 1, 1, 0, -1, 0, 0, 0, 0)])
    assert [s for s, _, _, _ in ok] == [0, 0, 0]


def test_the_three_entries_are_declared_exported_and_bound():
    import ctypes as C
    import diffpiso._native as N
    hdr = open(os.path.join(ROOT, "include", "piso_hip.h")).read()
    for decl in ("int piso_conv2d_forward_ex(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,",
                 "int piso_conv2d_wgrad_ex(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,",
                 "int piso_conv_last_geometry(int* out, int capacity);"):
        assert decl in hdr, decl
    assert "modulo the extent" in hdr and "pad is ks / 2" in hdr and "extent is at least its pad" in hdr          # the definition and the two rules
    assert len(N.lib.piso_conv2d_forward_ex.argtypes) == 14 and len(N.lib.piso_conv2d_wgrad_ex.argtypes) == 15
    assert N.lib.piso_conv2d_forward_ex.restype is C.c_int and N.lib.piso_conv2d_wgrad_ex.restype is C.c_int
    assert N.lib.piso_conv2d_wgrad_ex.argtypes[13] is C.c_size_t
    assert N.CONV_GEOMETRY_FIELDS == ("pad_y", "pad_x", "wrap_y", "wrap_x")
    got = N.conv_last_geometry()                          # (no card: no convolution has run in this process unless a GPU test did)
    assert got == {} or set(got) == set(N.CONV_GEOMETRY_FIELDS)


def _defect(net, x, shift=(3, 5)):
    with torch.no_grad():
        a, b = net(torch.roll(x, shift, (1, 2))), torch.roll(net(x), shift, (1, 2))
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


@pytest.mark.parametrize("hw", [(32, 32), (12, 20)])
def test_host_path_wrapped_network_commutes_with_a_circular_shift(hw):
    from diffpiso.closure import FullyConvNetwork
    x = torch.randn(1, hw[0], hw[1], 4, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    wrapped = FullyConvNetwork(seed=1, wrap=(True, True)).double()
    plain = FullyConvNetwork(seed=1).double()
    for a, b in zip(wrapped.weights, plain.weights):
        assert torch.equal(a, b)
    assert wrapped(x).shape == (1, hw[0], hw[1], 2)
    d = _defect(wrapped, x)
    assert d < 1e-10, d
    if hw == (32, 32):
        d0 = _defect(plain, x)
        assert d0 > 0.1, d0
    x32 = x.float()
    assert _defect(FullyConvNetwork(seed=1, wrap=(True, True)), x32) < 1e-6


def test_host_path_one_wrapped_axis_and_valid_padding():
    """A wrapped axis keeps its extent whatever `padding` says; VALID shrinks - and restore_shape pads back - only the other axis; the layer
    equals torch's convolution of the circularly padded input; the rules and the buffer_width refusal are ValueErrors."""
    import torch.nn.functional as F
    from diffpiso.closure import FullyConvNetwork, conv2d_leaky, initialise_fullyconv_network
    x = torch.randn(1, 40, 30, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    rbw = 3 + 2 + 2 + 1 + 1
    assert FullyConvNetwork(padding="VALID", wrap=(False, True), seed=1).double()(x).shape == (1, 40 - 2 * rbw, 30, 2)
    assert FullyConvNetwork(padding="VALID", wrap=(True, False), seed=1).double()(x).shape == (1, 40, 30 - 2 * rbw, 2)
    assert FullyConvNetwork(padding="VALID", wrap=(True, True), seed=1).double()(x).shape == (1, 40, 30, 2)
    net, weights, _ = initialise_fullyconv_network([[0, 0], [0, 0]], padding="VALID", restore_shape=True, seed=1, wrap=(False, True))
    with torch.no_grad():
        out = net.double()(x)
    assert out.shape == (1, 40, 30, 2) and len(weights) == 7
    assert float(out[:, :rbw].abs().max()) == 0.0 and float(out[:, -rbw:].abs().max()) == 0.0 and float(out[:, rbw:-rbw, 0].abs().min()) > 0.0
    # x-shifts commute with it (the y axis is not periodic: only x)
    with torch.no_grad():
        assert float((net(torch.roll(x, 7, 2)) - torch.roll(net(x), 7, 2)).abs().max()) < 1e-12
    w = torch.randn(16, 4, 7, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    got = conv2d_leaky(x, w, (0, 3), True, wrap=(False, True))
    want = F.leaky_relu(F.conv2d(torch.cat([x[:, :, -3:], x, x[:, :, :3]], 2).permute(0, 3, 1, 2), w), 0.2).permute(0, 2, 3, 1)
    assert got.shape == (1, 34, 30, 16) and float((got - want).abs().max()) < 1e-12          # (round-off: torch sums by the operand's memory layout)
    assert float((conv2d_leaky(x, w, (3, 3), False) - conv2d_leaky(x, w, 3, False)).abs().max()) < 1e-12      # (torch may sum a tuple padding in another order)
    with pytest.raises(ValueError):
        conv2d_leaky(x, w, (3, 2), True, wrap=(False, True))                 # pad_x != k // 2 on the wrapped axis
    with pytest.raises(ValueError):
        conv2d_leaky(x[:, :, :2], w, 3, True, wrap=(True, True))             # extent 2 < pad 3
    with pytest.raises(ValueError, match="buffer_width"):
        FullyConvNetwork(buffer_width=[[0, 0], [2, 0]], wrap=(False, True))
    with pytest.raises(ValueError, match="buffer_width"):
        initialise_fullyconv_network([[0, 1], [0, 0]], wrap=(True, True))
    FullyConvNetwork(buffer_width=[[2, 1], [0, 0]], wrap=(False, True))      # cropping the axis that is not wrapped is fine


@pytest.mark.parametrize("wrap", [(True, True), (False, True), (True, False), (False, False), None])
def test_centered_to_staggered_against_numpy(wrap):
    from diffpiso.closure import centered_to_staggered, make_forcing_fn
    c = np.random.default_rng(5).standard_normal((1, 6, 9, 2))
    got = centered_to_staggered(torch.from_numpy(c)) if wrap is None else centered_to_staggered(torch.from_numpy(c), wrap=wrap)
    wy, wx = wrap or (False, False)
    # the restatement: a face is the mean of the two cells it separates; beyond the edge: the cell across the seam, or the edge cell again
    py = np.concatenate([c[:, -1:] if wy else c[:, :1], c, c[:, :1] if wy else c[:, -1:]], 1)[..., 0]
    px = np.concatenate([c[:, :, -1:] if wx else c[:, :, :1], c, c[:, :, :1] if wx else c[:, :, -1:]], 2)[..., 1]
    v, u = 0.5 * (py[:, 1:] + py[:, :-1]), 0.5 * (px[:, :, 1:] + px[:, :, :-1])
    got = got.numpy()
    assert got.shape == (1, 7, 10, 2)
    assert np.array_equal(got[:, :, :9, 0], v) and np.array_equal(got[:, :6, :, 1], u)
    if wy:
        assert np.array_equal(got[:, 0, :9, 0], got[:, 6, :9, 0]) and np.array_equal(got[:, 0, :9, 0], 0.5 * (c[:, -1, :, 0] + c[:, 0, :, 0]))
    if wx:
        assert np.array_equal(got[:, :6, 0, 1], got[:, :6, 9, 1])
    # make_forcing_fn hands its wrap to the resampling; None is the replicated edge
    forcing = make_forcing_fn(lambda t: t[..., :2], pressure_included=False, wrap=wrap)

    class V:
        def at_centers(self):
            class D:
                data = torch.from_numpy(c)
            return D
    assert np.array_equal(forcing(0, V(), None).numpy(), got)


@pytest.mark.parametrize("ks,cin,cout,H,W,wrap", [(7, 4, 5, 9, 12, (1, 1)), (7, 3, 5, 3, 3, (1, 1)), (5, 6, 8, 7, 9, (0, 1)), (5, 2, 3, 2, 6, (1, 0)), (3, 6, 7, 1, 2, (1, 1)),
                                                  (3, 5, 4, 6, 6, (1, 0)), (1, 9, 2, 3, 4, (1, 1)), (3, 4, 4, 5, 8, (0, 0))])
def test_references_against_torch_float64_convolution_of_the_circularly_padded_input(ks, cin, cout, H, W, wrap):
    """ref_forward, ref_wgrad and the scatter ref_dgrad against torch.nn.functional.conv2d and its autograd on the host in float64: wrapped axes
    padded circularly by ks // 2, the others with zeros by 0, ks // 2 or ks - 1."""
    import torch.nn.functional as F
    rng = np.random.default_rng(ks + cin + cout + H)
    for zero_pad in (0, ks // 2, ks - 1):
        pad = tuple(ks // 2 if wr else zero_pad for wr in wrap)
        if H + 2 * pad[0] - ks + 1 < 1 or W + 2 * pad[1] - ks + 1 < 1:
            continue
        x, w = rng.standard_normal((H, W, cin)), rng.standard_normal((ks, ks, cin, cout))
        xt = torch.from_numpy(x).permute(2, 0, 1)[None].requires_grad_(True)
        wt = torch.from_numpy(w).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
        xc = xt
        if wrap[0]:
            xc = torch.cat([xc[:, :, H - pad[0]:], xc, xc[:, :, :pad[0]]], 2)
        if wrap[1]:
            xc = torch.cat([xc[:, :, :, W - pad[1]:], xc, xc[:, :, :, :pad[1]]], 3)
        y = F.conv2d(xc, wt, padding=(0 if wrap[0] else pad[0], 0 if wrap[1] else pad[1]))
        out = ref_forward(x, w, pad, wrap)
        assert out.shape == _extents(H, W, ks, pad) + (cout,)
        np.testing.assert_allclose(out, y[0].permute(1, 2, 0).detach().numpy(), rtol=0, atol=1e-12)
        g = rng.standard_normal(out.shape)
        y.backward(torch.from_numpy(g).permute(2, 0, 1)[None])
        np.testing.assert_allclose(ref_dgrad(g, w, pad, wrap, H, W), xt.grad[0].permute(1, 2, 0).numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(ref_wgrad(x, g, ks, pad, wrap), wt.grad.permute(2, 3, 1, 0).numpy(), rtol=0, atol=1e-12)
