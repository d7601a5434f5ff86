"""The epilogue kernels of a closure layer on the card, through the C ABI: piso_conv_epilogue_forward / piso_conv_epilogue_backward
(csrc/conv_epilogue.hip; include/piso_hip.h).

Shapes: with ppb = pixels_per_band of the plan, pixels in {1, ppb - 1, ppb, ppb + 1, 3 ppb + 5} x channels in {1, 2, 3, 4, 5, 16, 20, 64, 256}: one band and its
two edges, several bands with a ragged last one; both access forms (channels % 4), columns that are and are not a power of two, one to 256 columns.
  y, gpre   bit for bit against numpy float32 written with the same expressions (adds and one multiply: nothing to contract, no order to choose) - every
            activation, bias and skip each NULL and given, in place and out of place, once with every pointer 4 bytes off a 16-byte boundary (the
            scalar form); the inputs hold exact zeros and negative zeros;
  dbias     against the float64 sum of the checked gpre: |error| <= gamma sum |gpre[:, c]| per channel, gamma = (n - 1) u / (1 - (n - 1) u), u = 2^-24,
            n = pixels - the bound of ANY order of float32 additions of n terms;
  dbias     bit-identical between two runs, and between a run alone and a run on a stream with other work queued;
  refusals  status, message, and every output buffer (pre-filled with NaN) untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -24
GUARD = 64
CHANNELS = (1, 2, 3, 4, 5, 16, 20, 64, 256)
ACTS = (0, 1, 2)
INVALID = 1


def pixel_counts(channels):
    import diffpiso._native as N
    ppb = N.conv_epilogue_plan(1, channels)[1]
    counts = sorted({1, ppb - 1, ppb, ppb + 1, 3 * ppb + 5} - {0})
    assert all(N.conv_epilogue_plan(p, channels) == (-(-p // ppb), ppb) for p in counts)          # (the band size does not move below 1024 bands)
    return ppb, counts


def np_act(v, act):
    if act == 1:
        return np.where(v > 0, v, f32(0.2) * v).astype(f32)
    if act == 2:
        return np.where(v > 0, v, f32(0)).astype(f32)
    return v


def np_forward(z, bias, skip, act):
    v = z
    if bias is not None:
        v = (v + bias[None, :]).astype(f32)
    if skip is not None:
        v = (v + skip).astype(f32)
    return np_act(v, act)


def np_backward(g, y, act):
    if act == 1:
        return np.where(y > 0, g, f32(0.2) * g).astype(f32)
    if act == 2:
        return np.where(y > 0, g, f32(0)).astype(f32)
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def same_bits(got, want, what):
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        pytest.fail("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, bad.sum(), bad.size, i, got[i], want[i]))


def draw(rng, shape):
    """normal data with exact zeros and negative zeros sprinkled in"""
    a = rng.standard_normal(shape).astype(f32)
    flat = a.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return a


class Buf:
    """a device array between two guards of NaN, optionally `off` floats beyond a 16-byte boundary"""

    def __init__(self, data=None, n=None, off=0):
        n = data.size if data is not None else n
        self.n, self.off = n, off
        self.raw = torch.full((n + 2 * GUARD + off,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw[GUARD + off:GUARD + off + n]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def get(self, shape):
        return self.view.cpu().numpy().reshape(shape)

    def guards_intact(self):
        lo, hi = self.raw[:GUARD + self.off], self.raw[GUARD + self.off + self.n:]
        return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())

    def untouched(self):
        return bool(torch.isnan(self.raw).all())


def ptr_of(buf):
    return None if buf is None else buf.ptr


def run_forward(z, bias, skip, act, in_place, off=0):
    import diffpiso._native as N
    pixels, channels = z.shape
    zb = Buf(z, off=off)
    bb = None if bias is None else Buf(bias, off=off)
    sb = None if skip is None else Buf(skip, off=off)
    yb = zb if in_place else Buf(n=z.size, off=off)
    st = N.lib.piso_conv_epilogue_forward(zb.ptr, ptr_of(bb), ptr_of(sb), yb.ptr, pixels, channels, act, N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0, N.lib.piso_last_error_string()
    assert all(b.guards_intact() for b in (zb, yb) + tuple(b for b in (bb, sb) if b is not None)), "written outside an operand"
    if not in_place:
        same_bits(zb.get(z.shape), z, "z after an out-of-place call")
    return yb.get(z.shape)


def run_backward(g, y, act, with_bias, off=0, stream_noise=False):
    """-> (gpre or None when the call must not write it, dbias or None)"""
    import diffpiso._native as N
    pixels, channels = g.shape
    gb = Buf(g, off=off)
    yb = None if (act == 0 and pixels % 2) else Buf(y, off=off)             # (act 0: y may be NULL - given on the even shapes, NULL on the odd ones)
    pb = None if (act == 0 and pixels % 2) else Buf(n=g.size, off=off)
    db = Buf(n=channels, off=off) if with_bias else None
    nfloats = N.lib.piso_conv_epilogue_workspace_bytes(pixels, channels) // 4
    wb = Buf(n=nfloats, off=off) if with_bias else None
    st = N.lib.piso_conv_epilogue_backward(gb.ptr, ptr_of(yb), ptr_of(pb), ptr_of(db), pixels, channels, act, ptr_of(wb), C.c_size_t(nfloats if with_bias else 0),
                                           N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0, N.lib.piso_last_error_string()
    assert all(b.guards_intact() for b in (gb, yb, pb, db, wb) if b is not None), "written outside an operand, dbias or the workspace"
    same_bits(gb.get(g.shape), g, "g after the call")
    if act == 0:
        assert pb is None or pb.untouched(), "act 0 wrote gpre"
    return (pb.get(g.shape) if act else None), (db.get((channels,)) if with_bias else None)


def gamma_bound(gpre, n):
    gam = (n - 1) * U / (1.0 - (n - 1) * U)
    return gam * np.abs(gpre.astype(f64)).sum(axis=0)


@pytest.mark.parametrize("channels", CHANNELS)
def test_forward_is_the_numpy_expression_bit_for_bit(channels):
    _, counts = pixel_counts(channels)
    rng = np.random.default_rng(100 + channels)
    for pixels in counts:
        z, bias, skip = draw(rng, (pixels, channels)), draw(rng, (channels,)), draw(rng, (pixels, channels))
        skip[1::5] = -z[1::5]                                                # (sums that cancel to an exact zero)
        for act in ACTS:
            for b in (None, bias):
                for s in (None, skip):
                    want = np_forward(z, b, s, act)
                    for in_place in (False, True):
                        same_bits(run_forward(z, b, s, act, in_place), want, "forward, %d x %d, act %d, bias %s, skip %s, in place %s"
                                  % (pixels, channels, act, b is not None, s is not None, in_place))
            same_bits(run_forward(z, bias, skip, act, pixels % 2 == 0, off=1), np_forward(z, bias, skip, act), "forward off 16-byte alignment, %d x %d, act %d" % (pixels, channels, act))


@pytest.mark.parametrize("channels", CHANNELS)
def test_backward_is_the_numpy_expression_and_the_bias_sum_within_the_bound_of_any_order(channels):
    _, counts = pixel_counts(channels)
    rng = np.random.default_rng(200 + channels)
    for pixels in counts:
        g, y = draw(rng, (pixels, channels)), draw(rng, (pixels, channels))
        for act in ACTS:
            want = np_backward(g, y, act)
            for with_bias in (False, True):
                for off in (0, 1):
                    what = "%d x %d, act %d, dbias %s, offset %d" % (pixels, channels, act, with_bias, off)
                    gpre, dbias = run_backward(g, y, act, with_bias, off)
                    if act:
                        same_bits(gpre, want, "gpre, " + what)
                    if with_bias:
                        ref = want.astype(f64).sum(axis=0)
                        err, bound = np.abs(dbias.astype(f64) - ref), gamma_bound(want, pixels)
                        print("dbias %s: max error %.3e, its bound %.3e" % (what, err.max(), bound[err.argmax()]))
                        assert np.isfinite(dbias).all() and (err <= bound).all(), ("dbias, " + what, int(err.argmax()), float(err.max()), float(bound[err.argmax()]))


@pytest.mark.parametrize("channels", CHANNELS)
def test_bias_sum_is_the_same_bits_on_every_run_and_beside_other_work(channels):
    _, counts = pixel_counts(channels)
    rng = np.random.default_rng(300 + channels)
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device="cuda")
    for pixels in counts[-2:]:
        g, y = draw(rng, (pixels, channels)), draw(rng, (pixels, channels))
        for act in (0, 1):
            for off in (0, 1):
                _, first = run_backward(g, y, act, True, off)
                _, second = run_backward(g, y, act, True, off)
                same_bits(second, first, "dbias of a second run, %d x %d" % (pixels, channels))
                for _ in range(4):                                           # other work on the default stream, and ahead of the call on the side stream
                    a = torch.tanh(a @ a * 1e-3)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    b = a @ a
                    _, third = run_backward(g, y, act, True, off)
                torch.cuda.current_stream().wait_stream(side)
                same_bits(third, first, "dbias on a stream with other work queued, %d x %d" % (pixels, channels))
                assert bool(torch.isfinite(b).all())


def test_refusals_return_their_status_and_message_and_write_nothing():
    import diffpiso._native as N
    pixels, channels = 37, 8
    data = np.ones((pixels, channels), f32)
    z, skip, bias, g, yin = Buf(data), Buf(data), Buf(np.ones(channels, f32)), Buf(data), Buf(data)
    y, gpre, dbias = Buf(n=data.size), Buf(n=data.size), Buf(n=channels)
    nfloats = N.lib.piso_conv_epilogue_workspace_bytes(pixels, channels) // 4
    assert nfloats == channels                                               # one band
    ws = Buf(n=nfloats)
    fwd, bwd = N.lib.piso_conv_epilogue_forward, N.lib.piso_conv_epilogue_backward
    s, sz = N.stream_ptr(), C.c_size_t
    cases = {
        "fwd z NULL": (fwd, (None, bias.ptr, skip.ptr, y.ptr, pixels, channels, 1, s), "NULL"),
        "fwd y NULL": (fwd, (z.ptr, bias.ptr, skip.ptr, None, pixels, channels, 1, s), "NULL"),
        "fwd channels 0": (fwd, (z.ptr, bias.ptr, skip.ptr, y.ptr, pixels, 0, 1, s), "channels: 1 .. 256"),
        "fwd channels 257": (fwd, (z.ptr, bias.ptr, skip.ptr, y.ptr, pixels, 257, 1, s), "channels: 1 .. 256"),
        "fwd pixels 0": (fwd, (z.ptr, bias.ptr, skip.ptr, y.ptr, 0, channels, 1, s), "pixels: at least 1"),
        "fwd pixels -1": (fwd, (z.ptr, bias.ptr, skip.ptr, y.ptr, -1, channels, 1, s), "pixels: at least 1"),
        "fwd act 3": (fwd, (z.ptr, bias.ptr, skip.ptr, y.ptr, pixels, channels, 3, s), "act: 0 none, 1 leaky ReLU, 2 ReLU"),
        "fwd act -1": (fwd, (z.ptr, bias.ptr, skip.ptr, y.ptr, pixels, channels, -1, s), "act: 0 none, 1 leaky ReLU, 2 ReLU"),
        "fwd skip is y": (fwd, (z.ptr, bias.ptr, y.ptr, y.ptr, pixels, channels, 1, s), "skip must not alias y"),
        "bwd g NULL": (bwd, (None, yin.ptr, gpre.ptr, dbias.ptr, pixels, channels, 1, ws.ptr, sz(nfloats), s), "NULL"),
        "bwd channels 0": (bwd, (g.ptr, yin.ptr, gpre.ptr, dbias.ptr, pixels, 0, 1, ws.ptr, sz(nfloats), s), "channels: 1 .. 256"),
        "bwd channels 257": (bwd, (g.ptr, yin.ptr, gpre.ptr, dbias.ptr, pixels, 257, 1, ws.ptr, sz(1 << 20), s), "channels: 1 .. 256"),
        "bwd pixels 0": (bwd, (g.ptr, yin.ptr, gpre.ptr, dbias.ptr, 0, channels, 1, ws.ptr, sz(nfloats), s), "pixels: at least 1"),
        "bwd act 3": (bwd, (g.ptr, yin.ptr, gpre.ptr, dbias.ptr, pixels, channels, 3, ws.ptr, sz(nfloats), s), "act: 0 none, 1 leaky ReLU, 2 ReLU"),
        "bwd y NULL, act 1": (bwd, (g.ptr, None, gpre.ptr, dbias.ptr, pixels, channels, 1, ws.ptr, sz(nfloats), s), "NULL with act != 0"),
        "bwd y NULL, act 2": (bwd, (g.ptr, None, gpre.ptr, None, pixels, channels, 2, None, sz(0), s), "NULL with act != 0"),
        "bwd gpre NULL, act 1": (bwd, (g.ptr, yin.ptr, None, dbias.ptr, pixels, channels, 1, ws.ptr, sz(nfloats), s), "NULL with act != 0"),
        "bwd ws one short": (bwd, (g.ptr, yin.ptr, gpre.ptr, dbias.ptr, pixels, channels, 1, ws.ptr, sz(nfloats - 1), s), "ws too small"),
        "bwd ws 0, act 0": (bwd, (g.ptr, None, None, dbias.ptr, pixels, channels, 0, ws.ptr, sz(0), s), "ws too small"),
        "bwd ws NULL": (bwd, (g.ptr, yin.ptr, gpre.ptr, dbias.ptr, pixels, channels, 1, None, sz(nfloats), s), "ws too small"),
    }
    status, msgs = {}, {}
    for name, (fn, args, words) in cases.items():
        status[name] = fn(*args)
        msgs[name] = (N.lib.piso_last_error_string().decode(), fn.__name__ + ": ", words)
    torch.cuda.synchronize()
    assert {k: v for k, v in status.items() if v != INVALID} == {}
    assert {k: m for k, (m, start, words) in msgs.items() if not m.startswith(start) or words not in m} == {}
    assert y.untouched() and gpre.untouched() and dbias.untouched() and ws.untouched()
    same_bits(z.get(data.shape), data, "z after the refusals")
    # accepted beside them: act 0 without a bias is no work at all (gpre is g), with NULL y and gpre
    assert bwd(g.ptr, None, None, None, pixels, channels, 0, None, sz(0), s) == 0
    torch.cuda.synchronize()
    assert gpre.untouched() and dbias.untouched()
