"""Closure convolutions of any channel count and odd kernel size, the parts that need no card.

  * conv_plan (csrc/conv_dispatch.h) is walked on the host with `any` set (tests/conv_plan_any_driver.cpp): every accepted shape's record against a
    plain restatement of the rules, every refusal with its message, and the same queries with `any` clear: the old answers;
  * piso_conv2d_instantiated against a restatement of the instance tables;
  * the weight layout of piso_conv2d_forward_any against the header's formula, element by element;
  * the entries are declared in include/piso_hip.h, exported by the library and bound by diffpiso._native;
  * FullyConvNetwork(layers=...) on host tensors against a chain of F.conv2d / leaky_relu written out here, bit for bit; reduced_buffer_width;
    the default network is the one it was.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_wrap_cpu import FWD_SHAPES, WG_SHAPES, _host_compiler, expected_record

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELDS = ("entry", "KS", "C", "NT", "IPW", "family", "leaky", "grid_x", "grid_y", "block", "rows_per_block", "nblocks", "reducer", "Ho", "Wo")
FWD_ANY, WG_ANY = 7, 8
INVALID = 1
KS_ALL = (1, 3, 5, 7, 9)
CHANNELS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 129, 256)
WRAPS = ((0, 0), (1, 1), (0, 1), (1, 0))


def cdiv(a, b):
    return -(-a // b)


def groups_nt(cout):
    """the tiles of 16 output channels, split evenly over groups of at most 4"""
    tiles = cdiv(cout, 16)
    groups = cdiv(tiles, 4)
    return groups, cdiv(tiles, groups)


def expected_any(entry, H, W, cin, cout, ks, pad_y, pad_x, leaky, result_off16=0):
    """The rules of the run-time-shaped family restated: what a *_any call must report."""
    Ho, Wo = H + 2 * pad_y - ks + 1, W + 2 * pad_x - ks + 1
    groups, nt = groups_nt(cout)
    if entry == 1:
        return dict(entry=1, KS=ks, C=cdiv(cin, 4) * 4, NT=nt, IPW=0, family=FWD_ANY, leaky=int(bool(leaky)), grid_x=cdiv(cdiv(Wo, 64) * Ho, 4), grid_y=groups,
                    block=256, rows_per_block=0, nblocks=0, reducer=0, Ho=Ho, Wo=Wo)
    mti = cdiv(cin, 16)
    rpb = cdiv(Ho, 64)
    nblocks = cdiv(Ho, rpb)
    return dict(entry=2, KS=ks, C=mti, NT=nt, IPW=1, family=WG_ANY, leaky=0, grid_x=nblocks, grid_y=cdiv(ks * ks * mti, 4) * groups, block=256, rows_per_block=rpb,
                nblocks=nblocks, reducer=4 if (cout % 4 == 0 and not result_off16) else 1, Ho=Ho, Wo=Wo)


def any_workspace_bytes(ks, cin, cout, Ho):
    rpb = cdiv(Ho, 64)
    return cdiv(Ho, rpb) * ks * ks * cdiv(cin, 16) * 16 * cdiv(cout, 16) * 16 * 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = _host_compiler()
    assert cxx is not None, "no C++17 host compiler (tried c++, g++, clang++, ROCm's clang++, hipcc -x c++)"
    d = tmp_path_factory.mktemp("conv_plan_any")
    exe = str(d / "conv_plan_any_driver")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "conv_plan_any_driver.cpp")], check=True)
    # (the two older drivers initialise ConvQuery positionally, without the appended `any`: they must keep compiling)
    for old in ("conv_plan_driver", "conv_plan_ex_driver"):
        subprocess.run(cxx + ["-std=c++17", "-O1", "-o", str(d / old), os.path.join(HERE, old + ".cpp")], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def plan(driver):
    """plan(queries) -> [(status, message, record dict, (ex, pad_y, pad_x, wrap_h, wrap_w), (groups, item_groups, reduce_grid))]; a query is (any, entry, H, W,
    cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, leaky, conv_lds, null_ptr, operands_off16, result_off16, workspace_bytes)."""
    def run(queries):
        lines = driver("".join(" ".join(str(int(v)) for v in q) + "\n" for q in queries))
        assert len(lines) == len(queries)
        out = []
        for line in lines:
            status, msg, *rest = line.split("\t")
            assert len(rest) == len(FIELDS) + 8
            n = len(FIELDS)
            out.append((int(status), msg, dict(zip(FIELDS, map(int, rest[:n]))), tuple(map(int, rest[n:n + 5])), tuple(map(int, rest[n + 5:]))))
        return out
    return run


def _sizes(ks):
    return ((9, 64), (5, 70), (129, 6), (65, 17), (max(ks // 2, 1), max(ks // 2, 1)))


def test_plan_accepts_every_shape_with_the_record_of_the_rules(plan):
    queries, want = [], []
    for entry in (1, 2):
        for ks in KS_ALL:
            for cin in CHANNELS:
                for cout in CHANNELS:
                    for wi, (wrap_y, wrap_x) in enumerate(WRAPS):
                        for si, (H, W) in enumerate(_sizes(ks)):
                            pad_y = ks // 2 if (wrap_y or H < ks) else 0                       # a zero-padded axis: VALID where the image allows it
                            pad_x = ks // 2 if (wrap_x or W < ks) else (ks - 1 if (si + wi) % 2 else 0)
                            leaky = (H + cin) % 2 if entry == 1 else 0
                            off = (cin + cout + si) % 2                                          # no alignment rule: misaligned pointers are accepted
                            queries.append((1, entry, H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, leaky, -1, 0, off, off, -1))
                            want.append((expected_any(entry, H, W, cin, cout, ks, pad_y, pad_x, leaky, off), (1, pad_y, pad_x, H if wrap_y else 0, W if wrap_x else 0)))
    bad = {}
    for q, (status, msg, rec, geom, extra), (wrec, wgeom) in zip(queries, plan(queries), want):
        groups, _ = groups_nt(q[5])
        wextra = (groups, cdiv(q[6] * q[6] * cdiv(q[4], 16), 4) if q[1] == 2 else 1)
        if (status, msg) != (0, "-") or rec != wrec or geom != wgeom or extra[:2] != wextra:
            bad[q] = (status, msg, rec, wrec, geom, wgeom, extra, wextra)
        if q[1] == 2:                                          # the reducers: 64 weights, or 64 x 4, per workgroup
            n = q[6] * q[6] * q[4] * q[5]
            assert extra[2] == (cdiv(n // 4, 64) if wrec["reducer"] == 4 else cdiv(n, 64))
    assert len(bad) == 0, list(bad.items())[:3]
    assert {w[0]["NT"] for w in want} == {1, 2, 3, 4} and {w[0]["grid_y"] for w in want if w[0]["entry"] == 1} == {1, 2, 3, 4}
    assert {w[0]["rows_per_block"] for w in want if w[0]["entry"] == 2} >= {1, 2, 3} and max(w[0]["nblocks"] for w in want) <= 64
    assert {w[0]["reducer"] for w in want} == {0, 1, 4}


def test_the_balanced_groups():
    assert [groups_nt(c) for c in (1, 16, 17, 48, 64, 65, 80, 129, 256)] == [(1, 1), (1, 1), (1, 2), (1, 3), (1, 4), (2, 3), (2, 3), (3, 3), (4, 4)]


def test_workspace_of_a_wide_layer_stays_small(driver):
    import diffpiso._native as N
    assert N.lib.piso_conv2d_wgrad_any_workspace_bytes(5, 128, 128, 256) == 64 * 25 * 128 * 128 * 4      # 105 MB (256 bands: 420)
    for ks, cin, cout, Ho in ((5, 128, 128, 256), (3, 5, 24, 1), (9, 17, 65, 65), (1, 256, 256, 129), (7, 1, 1, 63)):
        want = any_workspace_bytes(ks, cin, cout, Ho)
        assert N.lib.piso_conv2d_wgrad_any_workspace_bytes(ks, cin, cout, Ho) == want
        assert int(driver("ws %d %d %d %d\n" % (ks, cin, cout, Ho))[0]) == want


def test_plan_refuses_with_the_entrys_name(plan):
    ok_f = (1, 1, 9, 64, 5, 24, 5, 2, 2, 0, 0, 0, -1, 0, 0, 0, 0)
    ok_w = (1, 2, 9, 64, 5, 24, 5, 2, 2, 0, 0, 0, -1, 0, 0, 0, -1)
    assert [s for s, *_ in plan([ok_f, ok_w])] == [0, 0]

    def q(base, **kw):
        names = ("any", "entry", "H", "W", "cin", "cout", "ks", "pad_y", "pad_x", "wrap_y", "wrap_x", "leaky", "conv_lds", "null_ptr", "off_op", "off_res", "ws")
        v = dict(zip(names, base))
        v.update(kw)
        return tuple(v[n] for n in names)
    cases = {}
    for tag, base in (("fwd", ok_f), ("wg", ok_w)):
        for ks in (2, 4, 11, 0, -1):
            cases["%s ks %d" % (tag, ks)] = (q(base, ks=ks, pad_y=max(ks // 2, 0), pad_x=max(ks // 2, 0)), "kernel size: odd, 1 .. 9")
        for cin in (0, 257, -3):
            cases["%s cin %d" % (tag, cin)] = (q(base, cin=cin), "channels: 1 .. 256")
        for cout in (0, 257):
            cases["%s cout %d" % (tag, cout)] = (q(base, cout=cout), "channels: 1 .. 256")
        cases[tag + " Ho < 1"] = (q(base, H=4, pad_y=0), "at least one row and one column")
        cases[tag + " Wo < 1"] = (q(base, W=2, pad_x=1), "at least one row and one column")
        cases[tag + " H 0"] = (q(base, H=0, pad_y=4), "at least one row and one column")
        cases[tag + " null"] = (q(base, null_ptr=1), "a pointer is NULL")
        cases[tag + " wrap_y, pad_y 0"] = (q(base, wrap_y=1, pad_y=0), "pad == ks / 2")
        cases[tag + " wrap_x, pad_x ks - 1"] = (q(base, wrap_x=1, pad_x=4), "pad == ks / 2")
        cases[tag + " H 1 < pad 2"] = (q(base, H=1, wrap_y=1), "extent >= its pad")
        cases[tag + " W 1 < pad 2"] = (q(base, W=1, wrap_x=1, wrap_y=1), "extent >= its pad")
    cases["wg workspace one byte short"] = (q(ok_w, ws=-2), "workspace_bytes")
    cases["wg workspace 0"] = (q(ok_w, ws=0), "workspace_bytes")
    got = plan([c for c, _ in cases.values()])
    bad = {}
    for (name, (query, words)), (status, msg, _, _, _) in zip(cases.items(), got):
        start = "piso_conv2d_forward_any: " if query[1] == 1 else "piso_conv2d_wgrad_any: "
        if status != INVALID or words not in msg or not msg.startswith(start):
            bad[name] = (status, msg)
    assert bad == {}
    # pad == extent is allowed (an index wraps once), and so are misaligned pointers
    ok = plan([(1, 1, 2, 2, 5, 24, 5, 2, 2, 1, 1, 0, -1, 0, 0, 0, 0), (1, 2, 4, 4, 40, 40, 9, 4, 4, 1, 1, 0, -1, 0, 1, 1, -1), (1, 1, 1, 1, 256, 256, 9, 4, 4, 0, 0, 1, -1, 0, 1, 0, 0)])
    assert [s for s, *_ in ok] == [0, 0, 0]


def test_with_any_clear_the_old_answers(plan):
    """The same driver, the same struct, `any` clear: the *_ex entries' plan as before - the records of the old rules, and the old refusals."""
    queries, want = [], []
    for entry, shapes in ((1, FWD_SHAPES), (2, WG_SHAPES)):
        for ks, cin, cout in shapes:
            for H, W in ((9, 64), (6, 129), (513, 6)):
                for lds in (-1, 0):
                    pad_y, pad_x = (ks // 2 if H < ks else 0), ks // 2
                    queries.append((0, entry, H, W, cin, cout, ks, pad_y, pad_x, 0, 1, 0, lds, 0, 0, 0, -1))
                    want.append(expected_record(entry, H, W, cin, cout, ks, pad_y, pad_x, 0, lds))
    got = plan(queries)
    assert [(s, m) for s, m, *_ in got] == [(0, "-")] * len(queries)
    assert [r for _, _, r, _, _ in got] == want
    assert {r["family"] for r in want} == set(range(7))
    refused = {"cin 5": ((0, 1, 9, 64, 5, 16, 5, 2, 2, 0, 0, 0, -1, 0, 0, 0, 0), "1..4 or a multiple of 16"),
               "cout 65": ((0, 1, 9, 64, 16, 65, 5, 2, 2, 0, 0, 0, -1, 0, 0, 0, 0), "piso_conv2d_forward: invalid argument"),
               "5x5 64>64": ((0, 1, 9, 64, 64, 64, 5, 2, 2, 0, 0, 0, -1, 0, 0, 0, 0), "not instantiated"),
               "3x3 16>16": ((0, 1, 9, 64, 16, 16, 3, 1, 1, 0, 0, 0, -1, 0, 0, 0, 0), "not instantiated"),
               "9x9": ((0, 1, 9, 64, 4, 16, 9, 4, 4, 0, 0, 0, -1, 0, 0, 0, 0), "not instantiated"),
               "wg 7x7 4>32": ((0, 2, 9, 64, 4, 32, 7, 3, 3, 0, 0, 0, -1, 0, 0, 0, -1), "not instantiated"),
               "wg cin 65": ((0, 2, 9, 64, 65, 16, 5, 2, 2, 0, 0, 0, -1, 0, 0, 0, -1), "piso_conv2d_wgrad: invalid argument"),
               "fwd off 16": ((0, 1, 9, 64, 16, 16, 5, 2, 2, 0, 0, 0, -1, 0, 1, 0, 0), "16-byte aligned")}
    got = plan([c for c, _ in refused.values()])
    assert {n: (s, m) for (n, (_, words)), (s, m, *_) in zip(refused.items(), got) if s != INVALID or words not in m} == {}


# ---- the instance tables restated (csrc/conv_dispatch.h: kConvFwd, kConvWg, PACK4, 64 -> 64) as (KS, C, NT)
TABLE_FWD = {(7, 4, 1), (7, 16, 1), (5, 16, 1), (5, 16, 2), (5, 32, 1), (3, 32, 4), (3, 64, 2), (3, 64, 4), (1, 64, 4), (1, 64, 1), (1, 4, 4)}
TABLE_WG = {(7, 1, 1), (5, 1, 1), (5, 1, 2), (3, 2, 4), (3, 4, 4), (1, 4, 4), (1, 4, 1)}


def table_says(entry, ks, cin, cout):
    if not (1 <= cin <= 64 and 1 <= cout <= 64):
        return 0
    nt = cdiv(cout, 16)
    if entry == 1:
        return int((cin <= 4 or cin % 16 == 0) and (ks, 4 if cin <= 4 else cin, nt) in TABLE_FWD)
    return int((ks, cin, cout) == (3, 64, 64) or (ks == 7 and cin <= 4 and nt == 1) or (ks, cdiv(cin, 16), nt) in TABLE_WG)


def test_instantiated_equals_the_tables(driver):
    import diffpiso._native as N
    inst = N.lib.piso_conv2d_instantiated
    bad = [(e, ks, cin, cout) for e in (1, 2) for ks in range(0, 11) for cin in list(range(0, 70)) + [128, 256, 257] for cout in list(range(0, 70)) + [128, 256, 257]
           if inst(e, ks, cin, cout) != table_says(e, ks, cin, cout)]
    assert bad == []
    # the 11 forward rows, the table's weight-gradient rows, PACK4 and 64 -> 64, through a channel count of each row
    for ks, c, nt in TABLE_FWD:
        assert inst(1, ks, c, 16 * nt) == 1 and inst(1, ks, c, 16 * nt - 15) == 1 and N.conv2d_instantiated(1, ks, c, 16 * nt)
    for ks, mti, nt in TABLE_WG:
        assert inst(2, ks, 16 * mti, 16 * nt) == 1 and inst(2, ks, 16 * mti - 15, 16 * nt - 15) == 1
    assert inst(2, 7, 4, 16) == 1 and inst(2, 7, 1, 1) == 1 and inst(2, 3, 64, 64) == 1
    for entry, ks, cin, cout in ((1, 5, 5, 24), (1, 3, 24, 40), (1, 3, 40, 40), (1, 1, 40, 3), (1, 7, 9, 16), (1, 5, 64, 64), (1, 3, 16, 16), (1, 7, 4, 32), (1, 9, 4, 16),
                                 (1, 3, 128, 128), (2, 3, 24, 40), (2, 3, 40, 40), (2, 7, 4, 32), (2, 9, 4, 16), (2, 3, 128, 128), (2, 5, 64, 64), (3, 3, 64, 64),
                                 (0, 7, 4, 16), (1, 2, 4, 16)):
        assert inst(entry, ks, cin, cout) == 0, (entry, ks, cin, cout)
    # the driver asks the header alone: the same answers without the library
    probe = [(1, 7, 4, 16), (1, 5, 5, 24), (2, 3, 64, 64), (2, 3, 24, 40), (2, 5, 5, 24), (1, 1, 64, 2)]
    assert [int(v) for v in driver("".join("inst %d %d %d %d\n" % p for p in probe))] == [table_says(*p) for p in probe]


@pytest.mark.parametrize("ks,cin,cout", [(5, 5, 24), (3, 40, 40), (1, 40, 3), (7, 9, 16), (3, 4, 16), (9, 1, 1), (3, 17, 65)])
def test_layout_of_the_any_entry_is_the_headers_formula(ks, cin, cout, driver):
    """element ((ky ks + kx) CINP4 + ci) COUTP + co = W[ky][kx][ci][co], zero where ci >= cin or co >= cout"""
    import diffpiso._native as N
    from diffpiso.closure import _laid_out_any
    w = torch.randn(ks, ks, cin, cout, generator=torch.Generator().manual_seed(ks + cin + cout))
    cinp4, coutp = cdiv(cin, 4) * 4, cdiv(cout, 16) * 16
    got = _laid_out_any(w)
    assert got.is_contiguous() and got.dtype == torch.float32
    flat = got.reshape(-1).numpy()
    assert flat.size == ks * ks * cinp4 * coutp == N.lib.piso_conv2d_weight_elems_any(ks, cin, cout) == int(driver("elems %d %d %d\n" % (ks, cin, cout))[0])
    wn = w.numpy()
    for ky in range(ks):
        for kx in range(ks):
            for ci in range(cinp4):
                row = flat[((ky * ks + kx) * cinp4 + ci) * coutp:][:coutp]
                want = np.zeros(coutp, np.float32)
                if ci < cin:
                    want[:cout] = wn[ky, kx, ci]
                assert np.array_equal(row, want), (ky, kx, ci)


def test_the_entries_are_declared_exported_and_bound():
    import diffpiso
    import diffpiso._native as N
    hdr = open(os.path.join(ROOT, "include", "piso_hip.h")).read()
    for decl in ("size_t piso_conv2d_weight_elems_any(int ks, int cin, int cout);",
                 "size_t piso_conv2d_wgrad_any_workspace_bytes(int ks, int cin, int cout, int Ho);",
                 "int piso_conv2d_instantiated(int entry, int ks, int cin, int cout);",
                 "int piso_conv2d_forward_any(const float* in, const float* w_laid_out, float* out, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,",
                 "int piso_conv2d_wgrad_any(const float* in, const float* grad_out, float* dw, int H, int W, int cin, int cout, int ks, int pad_y, int pad_x,"):
        assert decl in hdr, decl
    assert "[ks][ks][CINP4][COUTP]" in hdr and "7 conv_forward_any_kernel" in hdr and "8 conv_wgrad_any_kernel" in hdr
    assert len(N.lib.piso_conv2d_forward_any.argtypes) == 14 and len(N.lib.piso_conv2d_wgrad_any.argtypes) == 15
    assert N.lib.piso_conv2d_forward_any.argtypes == N.lib.piso_conv2d_forward_ex.argtypes and N.lib.piso_conv2d_wgrad_any.argtypes == N.lib.piso_conv2d_wgrad_ex.argtypes
    assert N.lib.piso_conv2d_forward_any.restype is C.c_int and N.lib.piso_conv2d_wgrad_any.restype is C.c_int and N.lib.piso_conv2d_instantiated.restype is C.c_int
    assert N.lib.piso_conv2d_weight_elems_any.restype is C.c_size_t and N.lib.piso_conv2d_wgrad_any_workspace_bytes.restype is C.c_size_t
    assert len(N.lib.piso_conv2d_wgrad_any_workspace_bytes.argtypes) == 4 and len(N.lib.piso_conv2d_instantiated.argtypes) == 4
    assert callable(diffpiso.conv2d_leaky)


# ---- the network
LAYERS = [(5, 5, 24), (3, 24, 40), (3, 40, 40), (1, 40, 2)]


def _chain(x_nhwc, weights, padding):
    y = x_nhwc.permute(0, 3, 1, 2)
    for i, w in enumerate(weights):
        y = F.conv2d(y, w, padding=w.shape[-1] // 2 if padding == "SAME" else 0)
        if i < len(weights) - 1:
            y = F.leaky_relu(y, 0.2)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("layers,in_channels", [(LAYERS, None), (LAYERS, 7), ([(9, 3, 5)], None), ([(1, 2, 300 - 44), (7, 256, 1)], None),
                                                ([(3, 4, 8), (3, 8, 8), (3, 8, 8), (3, 8, 8), (3, 8, 8), (3, 8, 8), (3, 8, 8), (3, 8, 8), (1, 8, 2)], None)])
@pytest.mark.parametrize("padding", ["SAME", "VALID"])
def test_network_of_given_layers_on_host_tensors_is_the_written_out_chain(layers, in_channels, padding):
    from diffpiso.closure import FullyConvNetwork, initialise_fullyconv_network
    net = FullyConvNetwork(padding=padding, seed=3, layers=layers, in_channels=in_channels)
    cin0 = in_channels if in_channels is not None else layers[0][1]
    assert [tuple(w.shape) for w in net.weights] == [(cout, cin0 if i == 0 else cin, k, k) for i, (k, cin, cout) in enumerate(layers)]
    assert net.reduced_buffer_width == sum(k // 2 for k, _, _ in layers)
    x = torch.randn(1, 21, 23, cin0, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got, want = net(x), _chain(x, list(net.weights), padding)
    assert got.shape == want.shape and torch.equal(got, want)
    shrink = 0 if padding == "SAME" else 2 * net.reduced_buffer_width
    assert got.shape == (1, 21 - shrink, 23 - shrink, layers[-1][2])
    # float64, and the Glorot scale per layer
    with torch.no_grad():
        assert torch.equal(net.double()(x.double()), _chain(x.double(), list(net.weights), padding))
    for w in net.weights:
        cout, cin, k, _ = w.shape
        std = float(np.sqrt(2.0 / (k * k * (cin + cout))))
        assert float(w.detach().abs().max()) <= 2.0 * std / 0.87962566103423978 + 1e-12
        if w.numel() > 2000:
            assert 0.8 * std < float(w.detach().float().std()) < 1.2 * std
    net2, weights, rbw = initialise_fullyconv_network(None, padding=padding, seed=3, layers=layers)
    assert rbw == sum(k // 2 for k, _, _ in layers) and len(weights) == len(layers)
    if in_channels is None:
        assert all(torch.equal(a, b) for a, b in zip(weights, net.float().weights))


def test_wrap_buffer_width_and_restore_shape_work_with_given_layers():
    from diffpiso.closure import FullyConvNetwork, initialise_fullyconv_network
    x = torch.randn(1, 30, 26, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    rbw = 2 + 1 + 1
    assert FullyConvNetwork(padding="VALID", wrap=(False, True), seed=1, layers=LAYERS).double()(x).shape == (1, 30 - 2 * rbw, 26, 2)
    wrapped = FullyConvNetwork(wrap=(True, True), seed=1, layers=LAYERS).double()
    with torch.no_grad():
        a, b = wrapped(torch.roll(x, (3, 5), (1, 2))), torch.roll(wrapped(x), (3, 5), (1, 2))
    assert float((a - b).abs().max()) < 1e-12
    net, _, r = initialise_fullyconv_network([[2, 1], [0, 3]], padding="VALID", restore_shape=True, seed=1, layers=LAYERS)
    assert r == [[2 + rbw, 1 + rbw], [0 + rbw, 3 + rbw]]
    with torch.no_grad():
        out = net.double()(x)
    assert out.shape == (1, 30, 26, 2)
    assert float(out[:, :2 + rbw].abs().max()) == 0.0 and float(out[:, :, -(3 + rbw):].abs().max()) == 0.0 and float(out[:, 2 + rbw:-(1 + rbw), rbw:-(3 + rbw)].abs().min()) > 0.0


def test_bad_layer_lists_are_refused():
    from diffpiso.closure import FullyConvNetwork
    for layers in ([], [(3, 4)], [(4, 4, 8)], [(11, 4, 8)], [(3, 4, 257)], [(3, 0, 8)], [(3, 4, 8), (3, 9, 2)]):
        with pytest.raises(ValueError):
            FullyConvNetwork(layers=layers)


def test_the_default_network_is_unchanged():
    """Same parameter shapes and, for a seed, the same draw: restated from the reference's initialiser (a normal distribution truncated at two standard
    deviations, sampled with sigma / 0.8796...), layer by layer from one generator."""
    from diffpiso.closure import FullyConvNetwork
    reference = [(7, 4, 16), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 64), (1, 64, 64), (1, 64, 2)]
    for kw, cin0 in ((dict(), 4), (dict(in_channels=2), 2), (dict(layers=None, in_channels=4), 4), (dict(layers=reference), 4)):
        net = FullyConvNetwork(seed=11, **kw)
        gen = torch.Generator().manual_seed(11)
        assert len(net.weights) == 7 and net.reduced_buffer_width == 9
        for i, ((k, cin, cout), w) in enumerate(zip(reference, net.weights)):
            cin = cin0 if i == 0 else cin
            sig = float(np.sqrt(2.0 / (k * k * cin + k * k * cout))) / 0.87962566103423978
            want = torch.empty(cout, cin, k, k)
            torch.nn.init.trunc_normal_(want, mean=0.0, std=sig, a=-2.0 * sig, b=2.0 * sig, generator=gen)
            assert tuple(w.shape) == (cout, cin, k, k) and torch.equal(w.detach(), want)
    a, b = FullyConvNetwork(seed=4, initialiser="normal"), FullyConvNetwork(seed=4, initialiser="normal", layers=reference)
    assert all(torch.equal(p, q) for p, q in zip(a.weights, b.weights))
