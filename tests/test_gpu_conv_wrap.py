"""Wrap-around padding of the closure convolutions on the card: piso_conv2d_forward_ex / piso_conv2d_wgrad_ex (csrc/conv.hip: the *_ex_kernel
instances, csrc/conv_dispatch.h: conv_plan), term by term.

Built like tests/test_gpu_conv_dispatch.py, with its two legs and its bounds.  The float64 references restate the definition of
include/piso_hip.h with the index taken modulo the extent on a wrapped axis (tests/test_conv_wrap_cpu.py, which holds them to torch's float64
convolution of the circularly padded input: ref_forward / ref_wgrad; ref_dgrad is the SCATTER of the forward
definition, not a convolution with flipped weights - it holds the input-gradient rule pad' = ks - 1 - pad, same wrap, of the autograd path):
  exact      integers in -3 .. 3: every partial sum is an integer below 2^24 (the largest weight gradient adds 513 x 6 products of magnitude
             <= 9), float32 arithmetic is exact in any order, the card must equal the reference bit for bit, element by element;
  round-off  normal data, |got - ref| <= C_ROUND sqrt(K) u S with C_ROUND = 4, u = 2^-24, K the number of terms and S the same sum over
             absolute values.
64 sentinel floats before and after every output.  Each row also requires the dispatch record to equal the OLD entries' rules for the shape
(the geometry changes no choice) and piso_conv_last_geometry to report the call.
Sizes: pad x pad (the extent equals the pad: every index wraps, once), 9 x 64 (one tile, the seam wraps inside it), 5 x 70 (two tiles, the
second partial: the seam lies between tile 1 and tile 0), 6 x 129 (three tiles, the last of one pixel; the four waves of a workgroup span two
output rows), 513 x 6 (weight gradient: bands of three rows, wrapped rows cross band seams).
Then: the *_ex entries with wrap (0, 0) equal the old entries bit for bit on normal data, every family; a circular shift of the input
shifts the output (bit for bit on integers, within twice the round-off bound on normal data) and leaves the weight gradient as it is; one NaN
reaches exactly the outputs whose wrapped window holds it; refusals write nothing.
"""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

from tests.test_conv_wrap_cpu import FWD_SHAPES, WG_SHAPES, _extents, expected_record, leaky32, ref_dgrad, ref_forward, ref_wgrad

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -24
C_ROUND = 4.0
GUARD = 64
SENTINEL = -12345.5
FWD_LDS = 1
WRAPS = ((1, 1), (0, 1), (1, 0))
SIZES = ((9, 64), (5, 70), (6, 129))


# ------------------------------------------------------------------------------------------------------------------------------------
# calling the C ABI
def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guard_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def call_forward_ex(x, w_hwio, pad, wrap, leaky):
    import diffpiso._native as N
    from diffpiso.closure import _laid_out
    H, W, cin = x.shape
    ks, cout = w_hwio.shape[0], w_hwio.shape[3]
    Ho, Wo = _extents(H, W, ks, pad)
    xd, wl = torch.from_numpy(x).cuda(), _laid_out(torch.from_numpy(w_hwio).cuda())
    buf, out = _guarded(Ho * Wo * cout)
    st = N.lib.piso_conv2d_forward_ex(N.ptr(xd), N.ptr(wl), C.c_void_p(out.data_ptr()), H, W, cin, cout, ks, pad[0], pad[1], wrap[0], wrap[1], leaky, N.stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy().reshape(Ho, Wo, cout), _guard_intact(buf, out.numel())


def call_wgrad_ex(x, g, ks, pad, wrap):
    import diffpiso._native as N
    H, W, cin = x.shape
    cout = g.shape[2]
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    nbytes = N.lib.piso_conv2d_wgrad_workspace_bytes(ks, cin, cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    buf, dw = _guarded(ks * ks * cin * cout)
    st = N.lib.piso_conv2d_wgrad_ex(N.ptr(xd), N.ptr(gd), C.c_void_p(dw.data_ptr()), H, W, cin, cout, ks, pad[0], pad[1], wrap[0], wrap[1], N.ptr(ws),
                                    C.c_size_t(nbytes), N.stream_ptr())
    torch.cuda.synchronize()
    return st, dw.cpu().numpy().reshape(ks, ks, cin, cout), _guard_intact(buf, dw.numel())


def call_forward_old(x, w_hwio, pad, leaky):
    import diffpiso._native as N
    from diffpiso.closure import _laid_out
    H, W, cin = x.shape
    ks, cout = w_hwio.shape[0], w_hwio.shape[3]
    Ho, Wo = _extents(H, W, ks, (pad, pad))
    xd, wl = torch.from_numpy(x).cuda(), _laid_out(torch.from_numpy(w_hwio).cuda())
    out = torch.empty(Ho * Wo * cout, dtype=torch.float32, device="cuda")
    st = N.lib.piso_conv2d_forward(N.ptr(xd), N.ptr(wl), N.ptr(out), H, W, cin, cout, ks, pad, leaky, N.stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy().reshape(Ho, Wo, cout)


def call_wgrad_old(x, g, ks, pad):
    import diffpiso._native as N
    H, W, cin = x.shape
    cout = g.shape[2]
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    nbytes = N.lib.piso_conv2d_wgrad_workspace_bytes(ks, cin, cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dw = torch.empty(ks * ks * cin * cout, dtype=torch.float32, device="cuda")
    st = N.lib.piso_conv2d_wgrad(N.ptr(xd), N.ptr(gd), N.ptr(dw), H, W, cin, cout, ks, pad, N.ptr(ws), C.c_size_t(nbytes), N.stream_ptr())
    torch.cuda.synchronize()
    return st, dw.cpu().numpy().reshape(ks, ks, cin, cout)


def forward_ex(x, w, pad, wrap, leaky):
    st, out, intact = call_forward_ex(x, w, pad, wrap, leaky)
    assert st == 0 and intact
    return out


def wgrad_ex(x, g, ks, pad, wrap):
    st, dw, intact = call_wgrad_ex(x, g, ks, pad, wrap)
    assert st == 0 and intact
    return dw


def _first_bad(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def assert_bitwise(got, want, what):
    bad = got.view(np.int32) != np.ascontiguousarray(want.astype(f32)).view(np.int32)
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, bad.sum(), bad.size, i, got[i], want[i]))


def assert_roundoff(got, want, S, K, what, factor=1.0):
    bound = factor * C_ROUND * math.sqrt(K) * U * S
    bad = ~(np.abs(got.astype(f64) - want) <= bound)
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: %d elements beyond %g x %g sqrt(%d) u S, first at %s: got %r, want %r, bound %g" % (what, bad.sum(), factor, C_ROUND, K, i, got[i], want[i], bound[i]))


def _set_lds(piso_option, lds):
    piso_option("conv_lds", -1 if lds else 0)


def _has_lds_form(entry, ks, cin, cout):
    """does conv_lds choose between two families for this shape"""
    if entry == 1:
        return cin >= 16 and ks >= 3
    return (ks, cin, cout) == (3, 64, 64) or (not (ks == 7 and cin <= 4 and cout <= 16) and cin % 4 == 0 and cout % 4 == 0)


# ------------------------------------------------------------------------------------------------------------------------------------
# the table: rows of (entry, ks, cin, cout, H, W, pad, wrap, leaky, lds)
def _pads(ks, H, W, wrap, alt):
    """a wrapped axis: ks // 2.  A zero-padded one: none where the image allows it (wrap_x with pad_y 0 is the VALID-in-y network), else ks // 2;
    alt: ks - 1 in x (what the input gradient of a VALID axis runs)"""
    pad_y = ks // 2 if (wrap[0] or H < ks) else 0
    pad_x = ks // 2 if wrap[1] else (ks - 1 if alt else (0 if W >= ks else ks // 2))
    return pad_y, pad_x


ROWS = []
for entry, shapes in ((1, FWD_SHAPES), (2, WG_SHAPES)):
    for n, (ks, cin, cout) in enumerate(shapes):
        for lds in ((1, 0) if _has_lds_form(entry, ks, cin, cout) else (1,)):
            for wi, wrap in enumerate(WRAPS):
                sizes = list(SIZES) + ([(513, 6)] if entry == 2 else [])
                if wrap == (1, 1) and ks > 1:
                    sizes.append((ks // 2, ks // 2))
                for si, (H, W) in enumerate(sizes):
                    ROWS.append((entry, ks, cin, cout, H, W, _pads(ks, H, W, wrap, (n + si) % 2), wrap, (n + wi + si + lds) % 2 if entry == 1 else 0, lds))
assert len(set(ROWS)) == len(ROWS)


def _id(r):
    return "%s %dx%d %d>%d %dx%d p%d.%d w%d%d%s%s" % (("fwd", "wg")[r[0] - 1], r[1], r[1], r[2], r[3], r[4], r[5], r[6][0], r[6][1], r[7][0], r[7][1],
                                                     " leaky" if r[8] else "", "" if r[9] else " nolds")


def _data(r, kind):
    rng = np.random.default_rng(2 * zlib.crc32(_id(r).encode()) + (kind == "int"))
    draw = (lambda s: rng.integers(-3, 4, s).astype(f32)) if kind == "int" else (lambda s: rng.standard_normal(s).astype(f32))
    entry, ks, cin, cout, H, W, pad = r[:7]
    Ho, Wo = _extents(H, W, ks, pad)
    return draw((H, W, cin)), draw((ks, ks, cin, cout)), draw((Ho, Wo, cout))


def _check_records(r):
    import diffpiso._native as N
    entry, ks, cin, cout, H, W, pad, wrap, leaky, lds = r
    assert N.conv_last_dispatch() == expected_record(entry, H, W, cin, cout, ks, pad[0], pad[1], leaky, lds)
    assert N.conv_last_geometry() == dict(pad_y=pad[0], pad_x=pad[1], wrap_y=wrap[0], wrap_x=wrap[1])


@pytest.mark.parametrize("r", [r for r in ROWS if r[0] == 1], ids=_id)
def test_forward_ex_row(r, piso_option):
    import diffpiso._native as N
    entry, ks, cin, cout, H, W, pad, wrap, leaky, lds = r
    _set_lds(piso_option, lds)
    K = ks * ks * cin
    x, w, _ = _data(r, "int")
    want = ref_forward(x, w, pad, wrap)
    assert np.abs(want).max() < 2 ** 24
    st, got, intact = call_forward_ex(x, w, pad, wrap, leaky)
    assert st == 0, N.lib.piso_last_error_string()
    _check_records(r)
    assert intact, "written outside out[Ho][Wo][cout]"
    assert_bitwise(got, leaky32(want) if leaky else want, "forward, integer data")
    x, w, _ = _data(r, "normal")
    want, S = ref_forward(x, w, pad, wrap), ref_forward(np.abs(x), np.abs(w), pad, wrap)
    if leaky:
        want = np.where(want > 0, want, 0.2 * want)
    st, got, intact = call_forward_ex(x, w, pad, wrap, leaky)
    assert st == 0 and intact
    assert_roundoff(got, want, S, K + 1, "forward, normal data")


@pytest.mark.parametrize("r", [r for r in ROWS if r[0] == 2], ids=_id)
def test_wgrad_ex_row(r, piso_option):
    import diffpiso._native as N
    entry, ks, cin, cout, H, W, pad, wrap, leaky, lds = r
    _set_lds(piso_option, lds)
    Ho, Wo = _extents(H, W, ks, pad)
    x, _, g = _data(r, "int")
    want = ref_wgrad(x, g, ks, pad, wrap)
    assert np.abs(want).max() < 2 ** 24
    st, got, intact = call_wgrad_ex(x, g, ks, pad, wrap)
    assert st == 0, N.lib.piso_last_error_string()
    _check_records(r)
    assert intact, "written outside dw[ks][ks][cin][cout]"
    assert_bitwise(got, want, "weight gradient, integer data")
    x, _, g = _data(r, "normal")
    want, S = ref_wgrad(x, g, ks, pad, wrap), ref_wgrad(np.abs(x), np.abs(g), ks, pad, wrap)
    st, got, intact = call_wgrad_ex(x, g, ks, pad, wrap)
    assert st == 0 and intact
    assert_roundoff(got, want, S, Ho * Wo, "weight gradient, normal data")


def test_the_rows_reach_every_family_both_ways():
    want = {(1, 0), (1, 1), (2, 2), (2, 3), (2, 4), (2, 5), (2, 6)}
    got = {(r[0], expected_record(r[0], r[4], r[5], r[2], r[3], r[1], r[6][0], r[6][1], r[8], r[9])["family"]) for r in ROWS}
    assert got == want
    assert {r[8] for r in ROWS if r[0] == 1} == {0, 1}
    assert {expected_record(2, r[4], r[5], r[2], r[3], r[1], r[6][0], r[6][1], 0, r[9])["rows_per_block"] for r in ROWS if r[0] == 2} >= {1, 3}


# ---- the autograd path: conv2d_leaky(wrap=...), every layer of the network, integer data, exact; the input gradient is the new forward entry on
# the flipped, transposed weights with pad' = ks - 1 - pad and the same wrap - held to the scatter of the forward definition
LAYERS = [(7, 4, 16), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 64), (1, 64, 64), (1, 64, 2)]


@pytest.mark.parametrize("ks,cin,cout", LAYERS)
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("leaky", [True, False])
def test_autograd_path_is_exact_on_integer_data(ks, cin, cout, wrap, leaky):
    import diffpiso._native as N
    from diffpiso.closure import conv2d_leaky
    rng = np.random.default_rng(1000 * ks + cin + cout + 2 * wrap[0] + wrap[1])
    H, W = 11, 70
    pad = (ks // 2 if wrap[0] else 0, ks // 2)                # (x: wrapped or SAME; y: wrapped or VALID)
    x = rng.integers(-3, 4, (H, W, cin)).astype(f32)
    w = rng.integers(-3, 4, (ks, ks, cin, cout)).astype(f32)
    xt = torch.from_numpy(x)[None].cuda().requires_grad_(True)
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))).cuda().requires_grad_(True)
    y = conv2d_leaky(xt, wt, pad, leaky, wrap=(bool(wrap[0]), bool(wrap[1])))
    assert N.conv_last_geometry() == dict(pad_y=pad[0], pad_x=pad[1], wrap_y=wrap[0], wrap_x=wrap[1])
    pre = ref_forward(x, w, pad, wrap)
    assert_bitwise(y.detach().cpu().numpy()[0], leaky32(pre) if leaky else pre, "forward")
    g = rng.integers(-3, 4, pre.shape).astype(f32)
    if leaky:
        g = np.where(pre > 0, g, 5 * g).astype(f32)           # 0.2f * (5 m) rounds to m: the exact leg stays exact
    y.backward(torch.from_numpy(g)[None].cuda())
    gp = np.where(pre > 0, g, f32(0.2) * g).astype(f32) if leaky else g
    assert np.array_equal(gp, np.round(gp)) and np.abs(gp).max() <= 3
    assert_bitwise(xt.grad.cpu().numpy()[0], ref_dgrad(gp, w, pad, wrap, H, W), "input gradient")
    assert_bitwise(np.ascontiguousarray(wt.grad.cpu().numpy().transpose(2, 3, 1, 0)), ref_wgrad(x, gp, ks, pad, wrap), "weight gradient")


def test_an_int_pad_without_wrap_still_runs_the_old_entries():
    import diffpiso._native as N
    from diffpiso.closure import conv2d_leaky
    x, w = torch.randn(1, 6, 20, 16).cuda().requires_grad_(True), torch.randn(16, 16, 5, 5).cuda().requires_grad_(True)
    conv2d_leaky(x, w, 2, True).sum().backward()
    assert N.conv_last_geometry() == {}
    conv2d_leaky(x, w, 2, True, wrap=(False, False)).sum().backward()
    assert N.conv_last_geometry() == {}
    conv2d_leaky(x, w, (2, 2), True).sum().backward()
    assert N.conv_last_geometry() == dict(pad_y=2, pad_x=2, wrap_y=0, wrap_x=0)


# ---- neutrality: wrap (0, 0), pad_y == pad_x - the old entries' bits and the old entries' record, every family, normal data
@pytest.mark.parametrize("ks,cin,cout", FWD_SHAPES, ids=lambda v: str(v))
def test_forward_ex_without_wrap_equals_the_old_entry_bitwise(ks, cin, cout, piso_option):
    import diffpiso._native as N
    rng = np.random.default_rng(ks + cin + cout)
    for H, W in ((9, 70), (6, 129)):
        x, w = rng.standard_normal((H, W, cin)).astype(f32), rng.standard_normal((ks, ks, cin, cout)).astype(f32)
        for pad in sorted({0, ks // 2, ks - 1}):
            if H + 2 * pad - ks + 1 < 1:
                continue
            for lds in ((1, 0) if _has_lds_form(1, ks, cin, cout) else (1,)):
                _set_lds(piso_option, lds)
                st, old = call_forward_old(x, w, pad, 1)
                rec = N.conv_last_dispatch()
                assert st == 0 and N.conv_last_geometry() == {}
                st, new, intact = call_forward_ex(x, w, (pad, pad), (0, 0), 1)
                assert st == 0 and intact and N.conv_last_dispatch() == rec and rec["family"] == (FWD_LDS if lds and _has_lds_form(1, ks, cin, cout) else 0)
                assert np.array_equal(old.view(np.int32), new.view(np.int32)), (H, W, pad, lds)


@pytest.mark.parametrize("ks,cin,cout", WG_SHAPES, ids=lambda v: str(v))
def test_wgrad_ex_without_wrap_equals_the_old_entry_bitwise(ks, cin, cout, piso_option):
    import diffpiso._native as N
    rng = np.random.default_rng(ks + cin + cout)
    fams = set()
    for H, W in ((9, 70), (513, 6)):
        for pad in sorted({0, ks // 2} if W >= ks else {ks // 2}):
            Ho, Wo = _extents(H, W, ks, (pad, pad))
            x, g = rng.standard_normal((H, W, cin)).astype(f32), rng.standard_normal((Ho, Wo, cout)).astype(f32)
            for lds in ((1, 0) if _has_lds_form(2, ks, cin, cout) else (1,)):
                _set_lds(piso_option, lds)
                st, old = call_wgrad_old(x, g, ks, pad)
                rec = N.conv_last_dispatch()
                assert st == 0 and N.conv_last_geometry() == {}
                st, new, intact = call_wgrad_ex(x, g, ks, (pad, pad), (0, 0))
                assert st == 0 and intact and N.conv_last_dispatch() == rec
                fams.add(rec["family"])
                assert np.array_equal(old.view(np.int32), new.view(np.int32)), (H, W, pad, lds)
    assert len(fams) == (2 if _has_lds_form(2, ks, cin, cout) else 1)


# ---- shift equivariance, both axes wrapped
@pytest.mark.parametrize("ks,cin,cout", FWD_SHAPES, ids=lambda v: str(v))
def test_forward_ex_commutes_with_a_circular_shift(ks, cin, cout, piso_option):
    pad, wrap, K = (ks // 2, ks // 2), (1, 1), ks * ks * cin
    rng = np.random.default_rng(7 * ks + cin + cout)
    for (H, W), shift in (((5, 70), (2, 37)), ((6, 129), (5, 64))):
        w = rng.integers(-3, 4, (ks, ks, cin, cout)).astype(f32)
        xi, xn = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.standard_normal((H, W, cin)).astype(f32)
        wn = rng.standard_normal(w.shape).astype(f32)
        for lds in ((1, 0) if _has_lds_form(1, ks, cin, cout) else (1,)):
            _set_lds(piso_option, lds)
            a = forward_ex(np.roll(xi, shift, (0, 1)), w, pad, wrap, 1)
            b = np.roll(forward_ex(xi, w, pad, wrap, 1), shift, (0, 1))
            assert_bitwise(a, b, "forward of the shifted input against the shifted forward, integer data")
            a = forward_ex(np.roll(xn, shift, (0, 1)), wn, pad, wrap, 0)
            b = np.roll(forward_ex(xn, wn, pad, wrap, 0), shift, (0, 1))
            S = np.roll(ref_forward(np.abs(xn), np.abs(wn), pad, wrap), shift, (0, 1))
            assert_roundoff(a, b.astype(f64), S, K + 1, "forward of the shifted input against the shifted forward, normal data", factor=2.0)


@pytest.mark.parametrize("ks,cin,cout", WG_SHAPES, ids=lambda v: str(v))
def test_wgrad_ex_is_invariant_under_a_common_circular_shift(ks, cin, cout, piso_option):
    pad, wrap = (ks // 2, ks // 2), (1, 1)
    rng = np.random.default_rng(11 * ks + cin + cout)
    for (H, W), shift in (((5, 70), (2, 37)), ((513, 6), (100, 5))):
        xi, gi = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (H, W, cout)).astype(f32)
        xn, gn = rng.standard_normal((H, W, cin)).astype(f32), rng.standard_normal((H, W, cout)).astype(f32)
        for lds in ((1, 0) if _has_lds_form(2, ks, cin, cout) else (1,)):
            _set_lds(piso_option, lds)
            a = wgrad_ex(np.roll(xi, shift, (0, 1)), np.roll(gi, shift, (0, 1)), ks, pad, wrap)
            assert_bitwise(a, wgrad_ex(xi, gi, ks, pad, wrap), "weight gradient of the shifted pair, integer data")
            a = wgrad_ex(np.roll(xn, shift, (0, 1)), np.roll(gn, shift, (0, 1)), ks, pad, wrap)
            b = wgrad_ex(xn, gn, ks, pad, wrap)
            S = ref_wgrad(np.abs(xn), np.abs(gn), ks, pad, wrap)
            assert_roundoff(a, b.astype(f64), S, H * W, "weight gradient of the shifted pair, normal data", factor=2.0)


# ---- one NaN at in[0][0][0]: exactly the outputs whose wrapped window holds it are NaN, the rest equal the reference bit for bit
@pytest.mark.parametrize("wrap", [(1, 1), (0, 1)])
@pytest.mark.parametrize("ks,cin,cout", [(7, 2, 3), (7, 16, 4), (5, 16, 32), (3, 64, 64), (1, 64, 2)], ids=lambda v: str(v))
def test_forward_ex_nan_stays_in_its_wrapped_window(ks, cin, cout, wrap, piso_option):
    H, W = 9, 70
    pad = _pads(ks, H, W, wrap, 0)
    rng = np.random.default_rng(ks + cin)
    x, w = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (ks, ks, cin, cout)).astype(f32)
    hit = np.zeros(x.shape, f64)
    hit[0, 0, 0] = 1.0
    nanmask = ref_forward(hit, np.ones_like(w), pad, wrap) > 0
    assert nanmask.any() and not nanmask.all()
    if ks > 1:
        assert nanmask[:, -1].any() and (nanmask[-1].any() == bool(wrap[0]))          # across the x seam; across the y seam only if y wraps
    want = ref_forward(x, w, pad, wrap).astype(f32)
    x[0, 0, 0] = np.nan
    for lds in ((1, 0) if _has_lds_form(1, ks, cin, cout) else (1,)):
        _set_lds(piso_option, lds)
        st, got, intact = call_forward_ex(x, w, pad, wrap, 0)
        assert st == 0 and intact
        assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern", _first_bad(np.isnan(got) != nanmask))
        assert_bitwise(np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), want), "forward beside the NaN")


@pytest.mark.parametrize("wrap", [(1, 1), (0, 1)])
@pytest.mark.parametrize("ks,cin,cout", [(7, 4, 16), (7, 16, 4), (5, 16, 32), (3, 64, 64), (3, 17, 63), (1, 64, 2)], ids=lambda v: str(v))
def test_wgrad_ex_nan_reaches_the_taps_that_read_it(ks, cin, cout, wrap, piso_option):
    H, W = 9, 70
    pad = _pads(ks, H, W, wrap, 0)
    Ho, Wo = _extents(H, W, ks, pad)
    rng = np.random.default_rng(ks + cout)
    x, g = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (Ho, Wo, cout)).astype(f32)
    hit = np.zeros(x.shape, f64)
    hit[0, 0, 0] = 1.0
    nanmask = ref_wgrad(hit, np.ones_like(g), ks, pad, wrap) > 0
    assert nanmask.any() and not nanmask.all()
    if wrap == (1, 1):
        assert nanmask[:, :, 0, :].all()                                               # every tap reads pixel (0, 0) from some output pixel
    want = ref_wgrad(x, g, ks, pad, wrap).astype(f32)
    x[0, 0, 0] = np.nan
    for lds in ((1, 0) if _has_lds_form(2, ks, cin, cout) else (1,)):
        _set_lds(piso_option, lds)
        st, got, intact = call_wgrad_ex(x, g, ks, pad, wrap)
        assert st == 0 and intact
        assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern (ky, kx, ci, co)", _first_bad(np.isnan(got) != nanmask))
        assert_bitwise(np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), want), "weight gradient beside the NaN")


# ---- refusals launch nothing: PISO_ERR_INVALID_ARG, the output's sentinel fill, the record and the geometry untouched
# name, entry, pointers ("p" valid, "0" NULL, "+4" off 16-byte alignment), H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, wg: workspace
REFUSALS = [("wrap_y with pad_y 0", "fwd", "p p p", 9, 64, 16, 16, 5, 0, 2, 1, 0), ("wrap_x with pad_x ks - 1", "fwd", "p p p", 9, 64, 16, 16, 5, 2, 4, 0, 1),
            ("both wrapped, pad_x 1", "fwd", "p p p", 9, 64, 4, 16, 7, 3, 1, 1, 1), ("H below the pad", "fwd", "p p p", 2, 64, 4, 16, 7, 3, 3, 1, 1),
            ("W below the pad", "fwd", "p p p", 9, 1, 16, 16, 5, 2, 2, 0, 1), ("null in", "fwd", "0 p p", 9, 64, 16, 16, 5, 2, 2, 1, 1),
            ("null w", "fwd", "p 0 p", 9, 64, 16, 16, 5, 2, 2, 1, 1), ("null out", "fwd", "p p 0", 9, 64, 16, 16, 5, 2, 2, 1, 1),
            ("Wo < 1", "fwd", "p p p", 9, 3, 16, 16, 5, 2, 0, 1, 0), ("cin 5", "fwd", "p p p", 9, 64, 5, 16, 5, 2, 2, 1, 1),
            ("cout 65", "fwd", "p p p", 9, 64, 16, 65, 5, 2, 2, 1, 1), ("not instantiated 5x5 64>64", "fwd", "p p p", 9, 64, 64, 64, 5, 2, 2, 1, 1),
            ("in off 16-byte alignment", "fwd", "+4 p p", 9, 64, 16, 16, 5, 2, 2, 1, 1), ("w off 16-byte alignment", "fwd", "p +4 p", 9, 64, 16, 16, 5, 2, 2, 1, 1),
            ("wg wrap_x with pad_x 0", "wg", "p p p p", 9, 64, 64, 64, 3, 1, 0, 0, 1, "roomy"), ("wg wrap_y with pad_y 2", "wg", "p p p p", 9, 64, 64, 64, 3, 2, 1, 1, 0, "roomy"),
            ("wg W below the pad", "wg", "p p p p", 9, 2, 4, 16, 7, 3, 3, 1, 1, "roomy"), ("wg null in", "wg", "0 p p p", 9, 64, 16, 16, 5, 2, 2, 1, 1, "nbytes"),
            ("wg null workspace", "wg", "p p p 0", 9, 64, 16, 16, 5, 2, 2, 1, 1, "nbytes"), ("wg workspace one byte short", "wg", "p p p p", 9, 64, 16, 16, 5, 2, 2, 1, 1, "short"),
            ("wg Ho < 1", "wg", "p p p p", 4, 64, 16, 16, 5, 0, 2, 0, 1, "nbytes"), ("wg cin 65", "wg", "p p p p", 9, 64, 65, 16, 5, 2, 2, 1, 1, "roomy"),
            ("wg not instantiated 7x7 4>32", "wg", "p p p p", 9, 64, 4, 32, 7, 3, 3, 1, 1, "roomy"), ("wg g off 16-byte alignment", "wg", "p +4 p p", 9, 64, 16, 16, 5, 2, 2, 1, 1, "nbytes"),
            ("wg dw off 16-byte alignment", "wg", "p p +4 p", 9, 64, 16, 16, 5, 2, 2, 1, 1, "nbytes")]


def test_refusals_leave_record_geometry_and_output_untouched():
    import diffpiso._native as N
    INVALID = 1
    st, _, _ = call_forward_ex(np.ones((6, 20, 16), f32), np.ones((5, 5, 16, 16), f32), (2, 2), (1, 1), 0)
    assert st == 0
    before, geom = N.conv_last_dispatch(), N.conv_last_geometry()
    assert before["entry"] == 1 and geom == dict(pad_y=2, pad_x=2, wrap_y=1, wrap_x=1)
    big = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    buf, out = _guarded(1 << 16)
    nb = {"nbytes": N.lib.piso_conv2d_wgrad_workspace_bytes(5, 16, 16), "roomy": N.lib.piso_conv2d_wgrad_workspace_bytes(5, 64, 64)}
    nb["short"] = nb["nbytes"] - 1
    ws = torch.empty(nb["roomy"], dtype=torch.uint8, device="cuda")

    def pointer(token, base):
        return None if token == "0" else C.c_void_p(base + 4) if token == "+4" else C.c_void_p(base)

    cases, msgs = {}, {}
    for name, entry, ptrs, H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, *rest in REFUSALS:
        t = ptrs.split()
        a = [pointer(t[0], big.data_ptr()), pointer(t[1], big.data_ptr()), pointer(t[2], out.data_ptr())]
        if entry == "fwd":
            cases[name] = N.lib.piso_conv2d_forward_ex(a[0], a[1], a[2], H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, 0, N.stream_ptr())
        else:
            cases[name] = N.lib.piso_conv2d_wgrad_ex(a[0], a[1], a[2], H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, pointer(t[3], ws.data_ptr()),
                                                     C.c_size_t(nb[rest[0]]), N.stream_ptr())
        msgs[name] = N.lib.piso_last_error_string().decode()
    torch.cuda.synchronize()
    assert {k: v for k, v in cases.items() if v != INVALID} == {}
    for name, msg in msgs.items():                       # the message states the rule
        if "with pad" in name or "pad_x 1" in name:
            assert "pad == ks / 2" in msg, (name, msg)
        if "below the pad" in name:
            assert "extent >= its pad" in msg, (name, msg)
    assert N.conv_last_dispatch() == before and N.conv_last_geometry() == geom
    assert bool((buf == SENTINEL).all())


def test_last_geometry_reports_what_ran():
    import diffpiso._native as N
    x, w = np.ones((9, 20, 16), f32), np.ones((5, 5, 16, 16), f32)
    assert call_forward_ex(x, w, (0, 2), (0, 1), 0)[0] == 0
    assert N.conv_last_geometry() == dict(pad_y=0, pad_x=2, wrap_y=0, wrap_x=1)
    assert call_wgrad_ex(x, np.ones((9, 24, 16), f32), 5, (2, 4), (1, 0))[0] == 0
    assert N.conv_last_geometry() == dict(pad_y=2, pad_x=4, wrap_y=1, wrap_x=0) and N.conv_last_dispatch()["entry"] == 2
    assert call_forward_old(x, w, 2, 0)[0] == 0
    assert N.conv_last_geometry() == {}                  # an old entry: no fields
    buf = (C.c_int * 2)(7, 7)
    assert call_forward_ex(x, w, (2, 2), (1, 1), 0)[0] == 0
    assert N.lib.piso_conv_last_geometry(buf, 1) == 4 and list(buf) == [2, 7]            # capacity is respected
