"""The run-time-shaped convolution family on the card: piso_conv2d_forward_any / piso_conv2d_wgrad_any (csrc/conv_any.hip: conv_forward_any_kernel,
conv_wgrad_any_kernel; csrc/conv_dispatch.h: conv_plan with `any` set), term by term, through the C ABI.

Built like tests/test_gpu_conv_dispatch.py / test_gpu_conv_wrap.py, with their two legs, their bounds, their sentinels and their float64 references
(tests/test_conv_wrap_cpu.py: ref_forward / ref_wgrad, and ref_dgrad - the SCATTER of the forward definition - for the input gradient, which is the
forward entry on the flipped, transposed weights with pad' = ks - 1 - pad and the same wrap):
  exact      integers in -3 .. 3: the largest sum is 9 x 81 x 130 < 2^17, float32 arithmetic is exact in any order, the card must equal the reference bit
             for bit, element by element;
  round-off  normal data, |got - ref| <= 4 sqrt(K) u S per element, u = 2^-24, K the number of terms, S the same sum over absolute values.
Every row also requires the dispatch record to equal the restated rules (tests/test_conv_any_cpu.py: expected_any) and the geometry record the call.
The rows are a table, not a product: channel seams (every NT, the group seam, partial K steps), kernel sizes, image seams (tiles, images smaller than
the kernel, the three pads), weight-gradient bands, wrap.  Then: a circular shift, NaN containment, the new family against the fixed instances on
every shape that has one, refusals.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.test_conv_any_cpu import FWD_ANY, WG_ANY, expected_any, table_says
from tests.test_conv_wrap_cpu import FWD_SHAPES, WG_SHAPES, _extents, leaky32, ref_dgrad, ref_forward, ref_wgrad
from tests.test_gpu_conv_wrap import (SENTINEL, _first_bad, _guard_intact, _guarded, assert_bitwise, assert_roundoff, call_forward_old, call_wgrad_old)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
INVALID = 1


# ------------------------------------------------------------------------------------------------------------------------------------
# calling the C ABI
def call_forward_any(x, w_hwio, pad, wrap, leaky):
    import diffpiso._native as N
    from diffpiso.closure import _laid_out_any
    H, W, cin = x.shape
    ks, cout = w_hwio.shape[0], w_hwio.shape[3]
    Ho, Wo = _extents(H, W, ks, pad)
    xd, wl = torch.from_numpy(x).cuda(), _laid_out_any(torch.from_numpy(w_hwio).cuda())
    assert wl.numel() == N.lib.piso_conv2d_weight_elems_any(ks, cin, cout)
    buf, out = _guarded(Ho * Wo * cout)
    st = N.lib.piso_conv2d_forward_any(N.ptr(xd), N.ptr(wl), C.c_void_p(out.data_ptr()), H, W, cin, cout, ks, pad[0], pad[1], wrap[0], wrap[1], leaky, N.stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy().reshape(Ho, Wo, cout), _guard_intact(buf, out.numel())


def call_wgrad_any(x, g, ks, pad, wrap):
    import diffpiso._native as N
    H, W, cin = x.shape
    Ho, Wo, cout = g.shape
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    nbytes = N.lib.piso_conv2d_wgrad_any_workspace_bytes(ks, cin, cout, Ho)
    wbuf, ws = _guarded((nbytes + 3) // 4)                  # (the partials are guarded too: a band or a tile written beyond them would show)
    buf, dw = _guarded(ks * ks * cin * cout)
    st = N.lib.piso_conv2d_wgrad_any(N.ptr(xd), N.ptr(gd), C.c_void_p(dw.data_ptr()), H, W, cin, cout, ks, pad[0], pad[1], wrap[0], wrap[1], C.c_void_p(ws.data_ptr()),
                                     C.c_size_t(nbytes), N.stream_ptr())
    torch.cuda.synchronize()
    return st, dw.cpu().numpy().reshape(ks, ks, cin, cout), _guard_intact(buf, dw.numel()) and _guard_intact(wbuf, ws.numel())


def flipped(w):
    """Wd[ky][kx][co][ci] = W[ks - 1 - ky][ks - 1 - kx][ci][co]: the weights of the input gradient"""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


def _check_records(entry, ks, cin, cout, H, W, pad, wrap, leaky):
    import diffpiso._native as N
    assert N.conv_last_dispatch() == expected_any(entry, H, W, cin, cout, ks, pad[0], pad[1], leaky)
    assert N.conv_last_geometry() == dict(pad_y=pad[0], pad_x=pad[1], wrap_y=wrap[0], wrap_x=wrap[1])


def _draw(seed, kind):
    rng = np.random.default_rng(2 * zlib.crc32(repr(seed).encode()) + (kind == "int"))
    return (lambda s: rng.integers(-3, 4, s).astype(f32)) if kind == "int" else (lambda s: rng.standard_normal(s).astype(f32))


def check_forward(ks, cin, cout, H, W, pad, wrap, leaky):
    import diffpiso._native as N
    for kind in ("int", "normal"):
        draw = _draw(("fwd", ks, cin, cout, H, W, pad, wrap), kind)
        x, w = draw((H, W, cin)), draw((ks, ks, cin, cout))
        want = ref_forward(x, w, pad, wrap)
        st, got, intact = call_forward_any(x, w, pad, wrap, leaky)
        assert st == 0, N.lib.piso_last_error_string()
        _check_records(1, ks, cin, cout, H, W, pad, wrap, leaky)
        assert intact, "written outside out[Ho][Wo][cout]"
        if kind == "int":
            assert np.abs(want).max() < 2 ** 17
            assert_bitwise(got, leaky32(want) if leaky else want, "forward, integer data")
        else:
            S = ref_forward(np.abs(x), np.abs(w), pad, wrap)
            assert_roundoff(got, np.where(want > 0, want, 0.2 * want) if leaky else want, S, ks * ks * cin + 1, "forward, normal data")


def check_dgrad(ks, cin, cout, H, W, pad, wrap):
    """the input gradient of the layer cin -> cout: the forward entry on cout -> cin channels"""
    import diffpiso._native as N
    Ho, Wo = _extents(H, W, ks, pad)
    padd = (ks - 1 - pad[0], ks - 1 - pad[1])
    for kind in ("int", "normal"):
        draw = _draw(("dgrad", ks, cin, cout, H, W, pad, wrap), kind)
        g, w = draw((Ho, Wo, cout)), draw((ks, ks, cin, cout))
        want = ref_dgrad(g, w, pad, wrap, H, W)
        st, got, intact = call_forward_any(g, flipped(w), padd, wrap, 0)
        assert st == 0, N.lib.piso_last_error_string()
        _check_records(1, ks, cout, cin, Ho, Wo, padd, wrap, 0)
        assert intact and got.shape == (H, W, cin)
        if kind == "int":
            assert_bitwise(got, want, "input gradient, integer data")
        else:
            assert_roundoff(got, want, ref_dgrad(np.abs(g), np.abs(w), pad, wrap, H, W), ks * ks * cout, "input gradient, normal data")


def check_wgrad(ks, cin, cout, H, W, pad, wrap):
    import diffpiso._native as N
    Ho, Wo = _extents(H, W, ks, pad)
    for kind in ("int", "normal"):
        draw = _draw(("wg", ks, cin, cout, H, W, pad, wrap), kind)
        x, g = draw((H, W, cin)), draw((Ho, Wo, cout))
        want = ref_wgrad(x, g, ks, pad, wrap)
        st, got, intact = call_wgrad_any(x, g, ks, pad, wrap)
        assert st == 0, N.lib.piso_last_error_string()
        _check_records(2, ks, cin, cout, H, W, pad, wrap, 0)
        assert intact, "written outside dw[ks][ks][cin][cout] or the workspace"
        if kind == "int":
            assert np.abs(want).max() < 2 ** 17
            assert_bitwise(got, want, "weight gradient, integer data")
        else:
            assert_roundoff(got, want, ref_wgrad(np.abs(x), np.abs(g), ks, pad, wrap), Ho * Wo, "weight gradient, normal data")


# ------------------------------------------------------------------------------------------------------------------------------------
# channel seams, forward and input gradient: 6 x 67, SAME, 3 x 3; cin at cout 17 (partial K steps, one to 33 steps per tap), cout at cin 5 (every NT, the
# group seam: 65 and 80 are two groups of 3 tiles with the last partly beyond COUTP, 129 three groups, 256 four)
CIN_SEAMS = [(3, c, 17) for c in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 65, 130)]
COUT_SEAMS = [(3, 5, c) for c in (1, 15, 16, 17, 48, 63, 64, 65, 80, 129, 256)]
KERNEL_SIZES = [(ks, 5, 24) for ks in (1, 5, 7, 9)]


@pytest.mark.parametrize("leaky", [1, 0])
@pytest.mark.parametrize("ks,cin,cout", CIN_SEAMS + COUT_SEAMS + KERNEL_SIZES, ids=lambda v: str(v))
def test_forward_channel_seams_and_kernel_sizes(ks, cin, cout, leaky):
    check_forward(ks, cin, cout, 6, 67, (ks // 2, ks // 2), (0, 0), leaky)


@pytest.mark.parametrize("ks,cin,cout", CIN_SEAMS + COUT_SEAMS + KERNEL_SIZES, ids=lambda v: str(v))
def test_input_gradient_channel_seams_and_kernel_sizes(ks, cin, cout):
    check_dgrad(ks, cin, cout, 6, 67, (ks // 2, ks // 2), (0, 0))


def test_the_forward_rows_reach_every_nt_and_group_count():
    recs = [expected_any(1, 6, 67, cin, cout, ks, ks // 2, ks // 2, 0) for ks, cin, cout in CIN_SEAMS + COUT_SEAMS]
    recs += [expected_any(1, 6, 67, cout, cin, ks, ks // 2, ks // 2, 0) for ks, cin, cout in CIN_SEAMS + COUT_SEAMS]
    assert {r["NT"] for r in recs} == {1, 2, 3, 4} and {r["grid_y"] for r in recs} == {1, 2, 3, 4}
    assert {r["C"] for r in recs} >= {4, 8, 12, 16, 20, 36, 68, 132}


# ---- channel seams, weight gradient
WG_ROWS = [(3, c, 17) for c in (1, 5, 16, 17, 33, 65)] + [(3, 5, c) for c in (1, 3, 16, 17, 64, 65, 129)] + [(ks, 5, 24) for ks in (1, 3, 5, 9)]


@pytest.mark.parametrize("ks,cin,cout", WG_ROWS, ids=lambda v: str(v))
def test_wgrad_channel_seams_and_kernel_sizes(ks, cin, cout):
    check_wgrad(ks, cin, cout, 6, 67, (ks // 2, ks // 2), (0, 0))


def test_the_wgrad_rows_reach_both_reducers_every_nt_and_several_groups():
    recs = [expected_any(2, 6, 67, cin, cout, ks, ks // 2, ks // 2, 0) for ks, cin, cout in WG_ROWS]
    assert {r["reducer"] for r in recs} == {1, 4} and {r["NT"] for r in recs} == {1, 2, 3, 4} and {r["C"] for r in recs} == {1, 2, 3, 5}
    assert {r["grid_y"] for r in recs} >= {3 * 2, 3 * 3, 12, 21}                                         # (item groups x groups: 65 and 129 out; 65 in; 9 x 9)


# ---- image seams: tiles of 64 pixels (Wo 1 .. 129), Ho 1 .. 5 (workgroups of four tiles span rows), the three pads, images smaller than the kernel
def _in_extent(out, ks, pad):
    return out - 2 * pad + ks - 1


IMAGE_ROWS = []
for i, (Ho, Wo) in enumerate(((1, 1), (2, 15), (3, 16), (4, 17), (5, 63), (1, 64), (2, 65), (3, 129))):
    ks = 3
    pad = (min((0, 1, 2)[i % 3], (Ho + ks - 2) // 2), min((1, 2, 0)[i % 3], (Wo + ks - 2) // 2))     # (the largest pad that leaves an input pixel)
    IMAGE_ROWS.append((ks, 5, 24, _in_extent(Ho, ks, pad[0]), _in_extent(Wo, ks, pad[1]), pad))
IMAGE_ROWS += [(7, 5, 24, 1, 1, (3, 3)), (9, 5, 24, 1, 1, (4, 4)), (7, 5, 24, 2, 1, (3, 3)), (9, 5, 24, 2, 1, (4, 4)), (9, 17, 3, 1, 2, (4, 4))]
IMAGE_ROWS += [(5, 5, 24, 7, 20, (p, p)) for p in (0, 2, 4)] + [(5, 5, 24, 7, 20, (0, 4)), (5, 5, 24, 7, 20, (4, 0))]


@pytest.mark.parametrize("ks,cin,cout,H,W,pad", IMAGE_ROWS, ids=lambda v: str(v).replace(" ", ""))
def test_image_seams(ks, cin, cout, H, W, pad):
    assert H >= 1 and W >= 1
    check_forward(ks, cin, cout, H, W, pad, (0, 0), (H + W) % 2)
    check_dgrad(ks, cin, cout, H, W, pad, (0, 0))
    check_wgrad(ks, cin, cout, H, W, pad, (0, 0))


def test_the_image_rows_reach_the_output_sizes():
    outs = {_extents(H, W, ks, pad) for ks, _, _, H, W, pad in IMAGE_ROWS}
    assert all(H >= 1 and W >= 1 for _, _, _, H, W, _ in IMAGE_ROWS)
    assert {p for ks, _, _, _, _, pad in IMAGE_ROWS if ks == 3 for p in pad} == {0, 1, 2} and {pad for ks, _, _, _, _, pad in IMAGE_ROWS if ks == 5} >= {(0, 0), (2, 2), (4, 4)}
    assert {wo for _, wo in outs} >= {1, 15, 16, 17, 63, 64, 65, 129} and {ho for ho, _ in outs} >= {1, 2, 3, 4, 5}


# ---- weight-gradient bands: 64 rows (one per band), 65 (two per band, 33 bands), 129 (three per band)
@pytest.mark.parametrize("Ho", [64, 65, 129])
def test_wgrad_row_bands(Ho):
    import diffpiso._native as N
    check_wgrad(3, 5, 24, Ho, 6, (1, 1), (0, 0))
    rec = N.conv_last_dispatch()
    assert (rec["rows_per_block"], rec["nblocks"]) == {64: (1, 64), 65: (2, 33), 129: (3, 43)}[Ho]


# ---- wrap
@pytest.mark.parametrize("wrap", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("size", ["pad", (5, 70), (9, 64)], ids=str)
@pytest.mark.parametrize("ks,cin,cout", [(5, 5, 24), (3, 40, 40)], ids=lambda v: str(v))
def test_wrapped_axes(ks, cin, cout, size, wrap):
    H, W = (ks // 2, ks // 2) if size == "pad" else size
    pad = (ks // 2, ks // 2)
    check_forward(ks, cin, cout, H, W, pad, wrap, (H + wrap[0]) % 2)
    check_dgrad(ks, cin, cout, H, W, pad, wrap)
    check_wgrad(ks, cin, cout, H, W, pad, wrap)


@pytest.mark.parametrize("ks,cin,cout", [(5, 5, 24), (3, 40, 40), (9, 3, 65)], ids=lambda v: str(v))
def test_a_circular_shift_of_the_input_shifts_the_output_bit_for_bit(ks, cin, cout):
    """both axes wrapped: every output pixel adds the same sequence of terms, wherever it lies"""
    pad, wrap = (ks // 2, ks // 2), (1, 1)
    rng = np.random.default_rng(7 * ks + cin + cout)
    for (H, W), shift in (((5, 70), (2, 37)), ((9, 64), (5, 63))):
        for kind, draw in (("int", lambda s: rng.integers(-3, 4, s).astype(f32)), ("normal", lambda s: rng.standard_normal(s).astype(f32))):
            x, w = draw((H, W, cin)), draw((ks, ks, cin, cout))
            st, a, ia = call_forward_any(np.roll(x, shift, (0, 1)), w, pad, wrap, 1)
            st2, b, ib = call_forward_any(x, w, pad, wrap, 1)
            assert st == 0 and st2 == 0 and ia and ib
            assert_bitwise(a, np.roll(b, shift, (0, 1)), "forward of the shifted input against the shifted forward, %s data" % kind)
            if kind == "int":                                # (the weight gradient adds its pixels in another order after a shift: exact on integers only)
                g = draw((H, W, cout))
                st, da, ia = call_wgrad_any(np.roll(x, shift, (0, 1)), np.roll(g, shift, (0, 1)), ks, pad, wrap)
                st2, db, ib = call_wgrad_any(x, g, ks, pad, wrap)
                assert st == 0 and st2 == 0 and ia and ib
                assert_bitwise(da, db, "weight gradient of the shifted pair, integer data")


# ---- NaN containment
@pytest.mark.parametrize("wrap", [(0, 0), (1, 1)])
@pytest.mark.parametrize("ks,cin,cout", [(5, 5, 24), (3, 40, 40), (9, 17, 65)], ids=lambda v: str(v))
def test_one_nan_in_the_input_reaches_exactly_its_terms(ks, cin, cout, wrap):
    H, W = 9, 70
    pad = (ks // 2, ks // 2)
    rng = np.random.default_rng(ks + cin)
    x, w = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (ks, ks, cin, cout)).astype(f32)
    g = rng.integers(-3, 4, (H, W, cout)).astype(f32)
    for where in ((0, 0, 0), (4, 63, cin - 1)):
        hit = np.zeros(x.shape, f64)
        hit[where] = 1.0
        xn = x.copy()
        xn[where] = np.nan
        nanmask = ref_forward(hit, np.ones_like(w), pad, wrap) > 0
        assert nanmask.any() and not nanmask.all()
        st, got, intact = call_forward_any(xn, w, pad, wrap, 0)
        assert st == 0 and intact
        assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern", _first_bad(np.isnan(got) != nanmask))
        assert_bitwise(np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), ref_forward(x, w, pad, wrap).astype(f32)), "forward beside the NaN")
        nanmask = ref_wgrad(hit, np.ones_like(g), ks, pad, wrap) > 0
        assert nanmask.any() and not nanmask.all()
        st, got, intact = call_wgrad_any(xn, g, ks, pad, wrap)
        assert st == 0 and intact
        assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern (ky, kx, ci, co)", _first_bad(np.isnan(got) != nanmask))
        assert_bitwise(np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), ref_wgrad(x, g, ks, pad, wrap).astype(f32)), "weight gradient beside the NaN")


@pytest.mark.parametrize("ks,cin,cout", [(5, 5, 24), (3, 40, 40), (9, 17, 65)], ids=lambda v: str(v))
def test_one_nan_in_grad_out_reaches_exactly_its_output_channel(ks, cin, cout):
    """placed where no tap leaves the image: every (ky, kx, ci) of that output channel has the term, no other weight has"""
    H, W = 9, 70
    pad = (ks // 2, ks // 2)
    rng = np.random.default_rng(ks + cout)
    x, g = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (H, W, cout)).astype(f32)
    where = (4, 33, cout - 1)
    gn = g.copy()
    gn[where] = np.nan
    nanmask = np.zeros((ks, ks, cin, cout), bool)
    nanmask[..., where[2]] = True
    hit = np.zeros(g.shape, f64)
    hit[where] = 1.0
    assert np.array_equal(ref_wgrad(np.ones_like(x), hit, ks, pad, (0, 0)) > 0, nanmask)
    st, got, intact = call_wgrad_any(x, gn, ks, pad, (0, 0))
    assert st == 0 and intact
    assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern (ky, kx, ci, co)", _first_bad(np.isnan(got) != nanmask))
    assert_bitwise(np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), ref_wgrad(x, g, ks, pad, (0, 0)).astype(f32)), "weight gradient beside the NaN")


# ---- one family against the other: every shape with a fixed instance
@pytest.mark.parametrize("ks,cin,cout", FWD_SHAPES, ids=lambda v: str(v))
def test_forward_any_against_the_fixed_instance(ks, cin, cout, piso_option):
    import diffpiso._native as N
    assert table_says(1, ks, cin, cout) == 1 and N.conv2d_instantiated(1, ks, cin, cout)
    rng = np.random.default_rng(ks + cin + cout)
    for H, W in ((9, 70), (6, 129)):
        for lds in (1, 0):
            piso_option("conv_lds", -1 if lds else 0)
            pad = ks // 2
            xi, wi = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (ks, ks, cin, cout)).astype(f32)
            st, old = call_forward_old(xi, wi, pad, 1)
            rec_old = N.conv_last_dispatch()
            st2, new, intact = call_forward_any(xi, wi, (pad, pad), (0, 0), 1)
            rec_new = N.conv_last_dispatch()
            assert st == 0 and st2 == 0 and intact
            assert rec_old["family"] in (0, 1) and rec_new["family"] == FWD_ANY and rec_new == expected_any(1, H, W, cin, cout, ks, pad, pad, 1)
            assert_bitwise(new, old, "the new family against the fixed instance, integer data")
            xn, wn = rng.standard_normal((H, W, cin)).astype(f32), rng.standard_normal((ks, ks, cin, cout)).astype(f32)
            want, S = ref_forward(xn, wn, (pad, pad), (0, 0)), ref_forward(np.abs(xn), np.abs(wn), (pad, pad), (0, 0))
            st, old = call_forward_old(xn, wn, pad, 0)
            st2, new, intact = call_forward_any(xn, wn, (pad, pad), (0, 0), 0)
            assert st == 0 and st2 == 0 and intact
            assert_roundoff(old, want, S, ks * ks * cin + 1, "the fixed instance, normal data")
            assert_roundoff(new, want, S, ks * ks * cin + 1, "the new family, normal data")


@pytest.mark.parametrize("ks,cin,cout", WG_SHAPES, ids=lambda v: str(v))
def test_wgrad_any_against_the_fixed_instance(ks, cin, cout, piso_option):
    import diffpiso._native as N
    assert table_says(2, ks, cin, cout) == 1 and N.conv2d_instantiated(2, ks, cin, cout)
    rng = np.random.default_rng(ks + cin + cout)
    for H, W in ((9, 70), (130, 6)):
        for lds in (1, 0):
            piso_option("conv_lds", -1 if lds else 0)
            pad = ks // 2
            xi, gi = rng.integers(-3, 4, (H, W, cin)).astype(f32), rng.integers(-3, 4, (H, W, cout)).astype(f32)
            st, old = call_wgrad_old(xi, gi, ks, pad)
            rec_old = N.conv_last_dispatch()
            st2, new, intact = call_wgrad_any(xi, gi, ks, (pad, pad), (0, 0))
            rec_new = N.conv_last_dispatch()
            assert st == 0 and st2 == 0 and intact
            assert rec_old["family"] in (2, 3, 4, 5, 6) and rec_new["family"] == WG_ANY and rec_new == expected_any(2, H, W, cin, cout, ks, pad, pad, 0)
            assert_bitwise(new, old, "the new family against the fixed instance, integer data")
            xn, gn = rng.standard_normal((H, W, cin)).astype(f32), rng.standard_normal((H, W, cout)).astype(f32)
            want, S = ref_wgrad(xn, gn, ks, (pad, pad), (0, 0)), ref_wgrad(np.abs(xn), np.abs(gn), ks, (pad, pad), (0, 0))
            st, old = call_wgrad_old(xn, gn, ks, pad)
            st2, new, intact = call_wgrad_any(xn, gn, ks, (pad, pad), (0, 0))
            assert st == 0 and st2 == 0 and intact
            assert_roundoff(old, want, S, H * W, "the fixed instance, normal data")
            assert_roundoff(new, want, S, H * W, "the new family, normal data")


# ---- refusals launch nothing: PISO_ERR_INVALID_ARG, the output's sentinel fill, the record and the geometry untouched
# name, entry, pointers ("p" valid, "0" NULL), H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, words of the message, wg: workspace
REFUSALS = [("ks 2", "fwd", "p p p", 9, 64, 5, 24, 2, 1, 1, 0, 0, "kernel size"), ("ks 4", "fwd", "p p p", 9, 64, 5, 24, 4, 2, 2, 0, 0, "kernel size"),
            ("ks 11", "fwd", "p p p", 19, 64, 5, 24, 11, 5, 5, 0, 0, "kernel size"), ("cin 0", "fwd", "p p p", 9, 64, 0, 24, 5, 2, 2, 0, 0, "channels"),
            ("cin 257", "fwd", "p p p", 9, 64, 257, 24, 5, 2, 2, 0, 0, "channels"), ("cout 0", "fwd", "p p p", 9, 64, 5, 0, 5, 2, 2, 0, 0, "channels"),
            ("cout 257", "fwd", "p p p", 9, 64, 5, 257, 5, 2, 2, 0, 0, "channels"), ("Ho < 1", "fwd", "p p p", 4, 64, 5, 24, 5, 0, 2, 0, 0, "at least one row"),
            ("null in", "fwd", "0 p p", 9, 64, 5, 24, 5, 2, 2, 0, 0, "NULL"), ("null w", "fwd", "p 0 p", 9, 64, 5, 24, 5, 2, 2, 0, 0, "NULL"),
            ("null out", "fwd", "p p 0", 9, 64, 5, 24, 5, 2, 2, 0, 0, "NULL"), ("wrap_y with pad_y 0", "fwd", "p p p", 9, 64, 5, 24, 5, 0, 2, 1, 0, "pad == ks / 2"),
            ("wrap_x with pad_x ks - 1", "fwd", "p p p", 9, 64, 5, 24, 5, 2, 4, 0, 1, "pad == ks / 2"), ("H below the pad", "fwd", "p p p", 1, 64, 5, 24, 5, 2, 2, 1, 1, "extent >= its pad"),
            ("wg ks 4", "wg", "p p p p", 9, 64, 5, 24, 4, 2, 2, 0, 0, "kernel size", "roomy"), ("wg cin 257", "wg", "p p p p", 9, 64, 257, 24, 5, 2, 2, 0, 0, "channels", "roomy"),
            ("wg cout 0", "wg", "p p p p", 9, 64, 5, 0, 5, 2, 2, 0, 0, "channels", "roomy"), ("wg Ho < 1", "wg", "p p p p", 4, 64, 5, 24, 5, 0, 2, 0, 0, "at least one row", "roomy"),
            ("wg null grad_out", "wg", "p 0 p p", 9, 64, 5, 24, 5, 2, 2, 0, 0, "NULL", "nbytes"), ("wg null workspace", "wg", "p p p 0", 9, 64, 5, 24, 5, 2, 2, 0, 0, "NULL", "nbytes"),
            ("wg workspace one byte short", "wg", "p p p p", 9, 64, 5, 24, 5, 2, 2, 0, 0, "workspace_bytes", "short"),
            ("wg wrap_x with pad_x 0", "wg", "p p p p", 9, 64, 5, 24, 5, 2, 0, 0, 1, "pad == ks / 2", "roomy"), ("wg W below the pad", "wg", "p p p p", 9, 1, 5, 24, 5, 2, 2, 1, 1, "extent >= its pad", "roomy")]


def test_refusals_leave_record_geometry_and_output_untouched():
    import diffpiso._native as N
    st, _, _ = call_forward_any(np.ones((6, 20, 5), f32), np.ones((5, 5, 5, 24), f32), (2, 2), (1, 1), 0)
    assert st == 0
    before, geom = N.conv_last_dispatch(), N.conv_last_geometry()
    assert before["family"] == FWD_ANY and geom == dict(pad_y=2, pad_x=2, wrap_y=1, wrap_x=1)
    big = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    buf, out = _guarded(1 << 16)
    nb = {"nbytes": N.lib.piso_conv2d_wgrad_any_workspace_bytes(5, 5, 24, 9), "roomy": 1 << 24}
    nb["short"] = nb["nbytes"] - 1
    ws = torch.empty(nb["roomy"], dtype=torch.uint8, device="cuda")

    def pointer(token, base):
        return None if token == "0" else C.c_void_p(base)

    cases, msgs = {}, {}
    for name, entry, ptrs, H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, words, *rest in REFUSALS:
        t = ptrs.split()
        a = [pointer(t[0], big.data_ptr()), pointer(t[1], big.data_ptr()), pointer(t[2], out.data_ptr())]
        if entry == "fwd":
            cases[name] = N.lib.piso_conv2d_forward_any(a[0], a[1], a[2], H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, 0, N.stream_ptr())
        else:
            cases[name] = N.lib.piso_conv2d_wgrad_any(a[0], a[1], a[2], H, W, cin, cout, ks, pad_y, pad_x, wrap_y, wrap_x, pointer(t[3], ws.data_ptr()),
                                                      C.c_size_t(nb[rest[0]]), N.stream_ptr())
        msgs[name] = (N.lib.piso_last_error_string().decode(), "piso_conv2d_forward_any: " if entry == "fwd" else "piso_conv2d_wgrad_any: ", words)
    torch.cuda.synchronize()
    assert {k: v for k, v in cases.items() if v != INVALID} == {}
    assert {k: m for k, (m, start, words) in msgs.items() if not m.startswith(start) or words not in m} == {}
    assert N.conv_last_dispatch() == before and N.conv_last_geometry() == geom
    assert bool((buf == SENTINEL).all())
    # no alignment rule: `in`, the weights and `out` four bytes off a 16-byte boundary
    x, w = np.arange(6 * 20 * 5, dtype=f32).reshape(6, 20, 5) % 7 - 3, np.arange(25 * 5 * 24, dtype=f32).reshape(5, 5, 5, 24) % 5 - 2
    from diffpiso.closure import _laid_out_any
    wl = _laid_out_any(torch.from_numpy(w))
    xb, wb = torch.zeros(x.size + 1, device="cuda"), torch.zeros(wl.numel() + 1, device="cuda")
    xb[1:], wb[1:] = torch.from_numpy(x).reshape(-1).cuda(), wl.reshape(-1).cuda()
    obuf, o = _guarded(6 * 20 * 24 + 1)
    st = N.lib.piso_conv2d_forward_any(C.c_void_p(xb.data_ptr() + 4), C.c_void_p(wb.data_ptr() + 4), C.c_void_p(o.data_ptr() + 4), 6, 20, 5, 24, 5, 2, 2, 0, 0, 0, N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and _guard_intact(obuf, o.numel()) and float(o[0]) == SENTINEL
    assert_bitwise(o[1:].cpu().numpy().reshape(6, 20, 24), ref_forward(x, w, (2, 2), (0, 0)), "forward off 16-byte alignment")
    # ... and the weight gradient with cout % 4 == 0 and a misaligned dw: the scalar reducer, the same bits
    g = np.arange(6 * 20 * 24, dtype=f32).reshape(6, 20, 24) % 5 - 2
    gb = torch.zeros(g.size + 1, device="cuda")
    gb[1:] = torch.from_numpy(g).reshape(-1).cuda()
    nbytes = N.lib.piso_conv2d_wgrad_any_workspace_bytes(5, 5, 24, 6)
    ws2 = torch.empty(nbytes + 4, dtype=torch.uint8, device="cuda")
    dbuf, d = _guarded(25 * 5 * 24 + 1)
    st = N.lib.piso_conv2d_wgrad_any(C.c_void_p(xb.data_ptr() + 4), C.c_void_p(gb.data_ptr() + 4), C.c_void_p(d.data_ptr() + 4), 6, 20, 5, 24, 5, 2, 2, 0, 0,
                                     C.c_void_p(ws2.data_ptr() + 4), C.c_size_t(nbytes), N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and _guard_intact(dbuf, d.numel()) and float(d[0]) == SENTINEL and N.conv_last_dispatch()["reducer"] == 1
    assert_bitwise(d[1:].cpu().numpy().reshape(5, 5, 5, 24), ref_wgrad(x, g, 5, (2, 2), (0, 0)), "weight gradient off 16-byte alignment")
