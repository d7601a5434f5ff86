"""Which kernel instance does a closure convolution run, and is every instance, seam and edge of csrc/conv.hip right - term by term?

piso_conv2d_forward / piso_conv2d_wgrad pick (csrc/conv_dispatch.h: conv_plan, the instance table)
  forward  the instance (KS, CINP, NT) of conv_forward_kernel, or of conv_forward_lds_kernel where CINP >= 16, KS >= 3 and option conv_lds is
           not 0; LEAKY as asked; one workgroup per four 64-pixel tiles
  wgrad    PACK4 (7 x 7, cin <= 4), conv_wgrad64[_lds]_kernel (3 x 3, 64 -> 64) or the generic instance (KS, MTI, NT, IPW), staged through LDS
           where cin % 4 == 0, cout % 4 == 0 and conv_lds is not 0; rows_per_block = ceil(Ho / 256) output rows per band; the 4-wide reducer
           where cout % 4 == 0, else the scalar one
Every row of ROWS calls the C ABI with ctypes on torch buffers (shapes autograd never builds are reachable that way; the weight layout comes
from diffpiso.closure._laid_out), requires the dispatch record (piso_conv_last_dispatch) to EQUAL an expectation written in the table, and
compares with a plain float64 restatement of the definition (ref_forward / ref_wgrad / ref_dgrad below: numpy, nothing from the card and no
convolution library) in two legs:
  exact      inputs, weights and output gradients are integers in -3 .. 3.  Every product is an integer of magnitude <= 9 and every partial
             sum of a row an integer below 2^24 (the largest weight gradient adds 513 x 70 = 35 910 products: < 2^19; the largest forward
             sum 7 x 7 x 16 or 3 x 3 x 64 products: < 2^13), so float32 arithmetic is exact in ANY summation order and the card must equal
             the reference bit for bit, element by element.  A dropped, doubled or misplaced term - a band seam, a chunk seam, a permuted
             weight index, a C/D register mapped to another pixel - fails and is named by its index.  With LEAKY the expectation is the
             single float32 product the kernel forms (v > 0 ? v : 0.2f * v).
  round-off  normal data, bound per element from the reference instead of fitted: |got - ref| <= C_ROUND sqrt(K) u S, K the number of terms
             of the element's sum, u = 2^-24, S the same sum over absolute values (the same reference function on |data|).  Each of the K
             additions rounds by at most u times a partial sum, which is at most S: K u S in the worst case, ~ sqrt(K / 3) u S if the errors
             are independent.  C_ROUND = 4 keeps the worst of a million elements inside while one missing term (~ S / K) is outside for
             K < 10^4, which the exact leg does not need.
A sentinel fills 64 floats before and after every output (out, dw, grad_pre are slices of larger buffers): nothing is written outside.
NaN rows: one NaN in `in` (wgrad: or in grad_out) - exactly the elements whose sum has a term with it are NaN, the rest equal the reference
bit for bit.  (A NaN in grad_out is placed where no tap leaves the image: whether 0-padding x NaN is a term is left open by the header.)
The CPU-only tests at the end hold the reference to torch's float64 convolution, _laid_out to the header's formula and the table's literal
expectations to a restatement of the dispatch rules in plain Python.
"""
import ctypes as C
import math
import os
import zlib

import numpy as np
import pytest
import torch

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
C_ROUND = 4.0
GUARD = 64                       # sentinel floats before and after every output (a multiple of 4: the slice stays 16-byte aligned)
SENTINEL = -12345.5
FWD_DIRECT, FWD_LDS, WG_GENERIC, WG_GENERIC_LDS, WG_PACK4, WG_64, WG_64_LDS = range(7)


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference: float64, from the definitions
def _padded(x, pad):
    H, W, c = x.shape
    xp = np.zeros((H + 2 * pad, W + 2 * pad, c), f64)
    xp[pad:pad + H, pad:pad + W] = x
    return xp


def ref_forward(x, w, pad):
    """out[y][x][co] = sum over (ky, kx, ci) of in[y + ky - pad][x + kx - pad][ci] w[ky][kx][ci][co]; x [H][W][cin], w HWIO."""
    ks, xp = w.shape[0], _padded(x, pad)
    Ho, Wo = xp.shape[0] - ks + 1, xp.shape[1] - ks + 1
    out = np.zeros((Ho, Wo, w.shape[3]), f64)
    for ky in range(ks):
        for kx in range(ks):
            out += xp[ky:ky + Ho, kx:kx + Wo, :] @ w[ky, kx].astype(f64)
    return out


def ref_wgrad(x, g, ks, pad):
    """dw[ky][kx][ci][co] = sum over output pixels (y, x) of in[y + ky - pad][x + kx - pad][ci] g[y][x][co]."""
    xp, (Ho, Wo, cout) = _padded(x, pad), g.shape
    dw = np.zeros((ks, ks, x.shape[2], cout), f64)
    g2 = g.reshape(Ho * Wo, cout).astype(f64)
    for ky in range(ks):
        for kx in range(ks):
            dw[ky, kx] = xp[ky:ky + Ho, kx:kx + Wo, :].reshape(Ho * Wo, -1).T @ g2
    return dw


def ref_dgrad(g, w, pad, H, W):
    """dx[yy][xx][ci] = sum over (ky, kx, co) of g[yy - ky + pad][xx - kx + pad][co] w[ky][kx][ci][co]: every output pixel scatters its
    gradient to the input pixels it read (written from the forward definition, not as a convolution with flipped weights)."""
    ks, (Ho, Wo, _) = w.shape[0], g.shape
    dxp = np.zeros((H + 2 * pad, W + 2 * pad, w.shape[2]), f64)
    for ky in range(ks):
        for kx in range(ks):
            dxp[ky:ky + Ho, kx:kx + Wo, :] += g.astype(f64) @ w[ky, kx].astype(f64).T
    return dxp[pad:pad + H, pad:pad + W]


def leaky32(v64):
    """What the kernel stores for an exactly representable pre-activation: one float32 product."""
    v = v64.astype(f32)
    return np.where(v > 0, v, f32(0.2) * v).astype(f32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the table.  Instances are written out literally; expected_record() at the end restates the dispatch rules and a CPU test compares.
# forward shapes: name -> (ks, cin, cout, (KS, CINP, NT), an LDS form exists)
FWD = {"7x7 4>16": (7, 4, 16, (7, 4, 1), 0), "7x7 16>4": (7, 16, 4, (7, 16, 1), 1), "5x5 16>16": (5, 16, 16, (5, 16, 1), 1),
       "5x5 16>32": (5, 16, 32, (5, 16, 2), 1), "5x5 32>16": (5, 32, 16, (5, 32, 1), 1), "3x3 32>64": (3, 32, 64, (3, 32, 4), 1),
       "3x3 64>32": (3, 64, 32, (3, 64, 2), 1), "3x3 64>64": (3, 64, 64, (3, 64, 4), 1), "1x1 64>64": (1, 64, 64, (1, 64, 4), 0),
       "1x1 64>2": (1, 64, 2, (1, 64, 1), 0), "1x1 2>64": (1, 2, 64, (1, 4, 4), 0),
       # channel counts only the C ABI reaches
       "7x7 1>1": (7, 1, 1, (7, 4, 1), 0), "7x7 2>3": (7, 2, 3, (7, 4, 1), 0), "7x7 3>15": (7, 3, 15, (7, 4, 1), 0), "7x7 16>2": (7, 16, 2, (7, 16, 1), 1),
       "5x5 16>17": (5, 16, 17, (5, 16, 2), 1), "5x5 32>15": (5, 32, 15, (5, 32, 1), 1), "3x3 64>63": (3, 64, 63, (3, 64, 4), 1),
       "3x3 64>17": (3, 64, 17, (3, 64, 2), 1), "1x1 3>63": (1, 3, 63, (1, 4, 4), 0), "1x1 1>49": (1, 1, 49, (1, 4, 4), 0), "1x1 64>1": (1, 64, 1, (1, 64, 1), 0)}
# weight-gradient shapes: name -> (ks, cin, cout, (KS, MTI, NT, IPW), family with conv_lds on, family with conv_lds 0, grid_y, block, reducer)
WG = {"7x7 4>16": (7, 4, 16, (7, 1, 1, 1), WG_PACK4, WG_PACK4, 4, 256, 4), "7x7 16>4": (7, 16, 4, (7, 1, 1, 3), WG_GENERIC_LDS, WG_GENERIC, 5, 256, 4),
      "5x5 16>16": (5, 16, 16, (5, 1, 1, 2), WG_GENERIC_LDS, WG_GENERIC, 4, 256, 4), "5x5 16>32": (5, 16, 32, (5, 1, 2, 2), WG_GENERIC_LDS, WG_GENERIC, 4, 256, 4),
      "3x3 32>64": (3, 32, 64, (3, 2, 4, 1), WG_GENERIC_LDS, WG_GENERIC, 5, 256, 4), "3x3 64>60": (3, 64, 60, (3, 4, 4, 1), WG_GENERIC_LDS, WG_GENERIC, 9, 256, 4),
      "3x3 64>64": (3, 64, 64, (3, 4, 4, 1), WG_64_LDS, WG_64, 3, 192, 4), "1x1 64>64": (1, 64, 64, (1, 4, 4, 1), WG_GENERIC_LDS, WG_GENERIC, 1, 256, 4),
      "1x1 64>2": (1, 64, 2, (1, 4, 1, 1), WG_GENERIC, WG_GENERIC, 1, 256, 1), "1x1 64>4": (1, 64, 4, (1, 4, 1, 1), WG_GENERIC_LDS, WG_GENERIC, 1, 256, 4),
      # channel counts only the C ABI reaches
      "7x7 8>16": (7, 8, 16, (7, 1, 1, 3), WG_GENERIC_LDS, WG_GENERIC, 5, 256, 4), "7x7 1>1": (7, 1, 1, (7, 1, 1, 1), WG_PACK4, WG_PACK4, 4, 256, 1),
      "7x7 2>2": (7, 2, 2, (7, 1, 1, 1), WG_PACK4, WG_PACK4, 4, 256, 1), "7x7 3>15": (7, 3, 15, (7, 1, 1, 1), WG_PACK4, WG_PACK4, 4, 256, 1),
      "7x7 5>3": (7, 5, 3, (7, 1, 1, 3), WG_GENERIC, WG_GENERIC, 5, 256, 1), "5x5 5>17": (5, 5, 17, (5, 1, 2, 2), WG_GENERIC, WG_GENERIC, 4, 256, 1),
      "5x5 3>15": (5, 3, 15, (5, 1, 1, 2), WG_GENERIC, WG_GENERIC, 4, 256, 1), "5x5 5>16": (5, 5, 16, (5, 1, 1, 2), WG_GENERIC, WG_GENERIC, 4, 256, 4),
      "3x3 17>63": (3, 17, 63, (3, 2, 4, 1), WG_GENERIC, WG_GENERIC, 5, 256, 1), "3x3 63>63": (3, 63, 63, (3, 4, 4, 1), WG_GENERIC, WG_GENERIC, 9, 256, 1),
      "3x3 63>64": (3, 63, 64, (3, 4, 4, 1), WG_GENERIC, WG_GENERIC, 9, 256, 4), "1x1 63>1": (1, 63, 1, (1, 4, 1, 1), WG_GENERIC, WG_GENERIC, 1, 256, 1),
      "1x1 63>63": (1, 63, 63, (1, 4, 4, 1), WG_GENERIC, WG_GENERIC, 1, 256, 1), "1x1 49>3": (1, 49, 3, (1, 4, 1, 1), WG_GENERIC, WG_GENERIC, 1, 256, 1)}

ROWS = []


def fwd(tag, shape, H, W, pad=None, leaky=0, lds=1, grid=None, nan=None):
    """grid: workgroups, written out where the row is about the tiling; else ceil(tiles / 4)."""
    ks, cin, cout, (KS, CINP, NT), has_lds = FWD[shape]
    pad = ks // 2 if pad is None else pad
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    assert Ho >= 1 and Wo >= 1
    expect = dict(entry=1, KS=KS, C=CINP, NT=NT, IPW=0, family=FWD_LDS if (has_lds and lds) else FWD_DIRECT, leaky=leaky,
                  grid_x=grid if grid is not None else -(-(-(-Wo // 64) * Ho) // 4), grid_y=1, block=256, rows_per_block=0, nblocks=0, reducer=0, Ho=Ho, Wo=Wo)
    ROWS.append(dict(id="fwd %s %s %dx%d p%d%s%s" % (tag, shape, H, W, pad, " leaky" if leaky else "", "" if lds else " nolds"), entry="fwd", H=H, W=W, cin=cin,
                     cout=cout, ks=ks, pad=pad, leaky=leaky, lds=lds, nan=nan, nan_g=None, expect=expect))


def wg(tag, shape, H, W, pad=None, lds=1, bands=None, nan=None, nan_g=None):
    """bands: (rows_per_block, nblocks), written out where the row is about the bands; else (1, Ho) - only valid for Ho <= 256."""
    ks, cin, cout, (KS, MTI, NT, IPW), fam_on, fam_off, grid_y, block, reducer = WG[shape]
    pad = ks // 2 if pad is None else pad
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    assert Ho >= 1 and Wo >= 1 and (bands is not None or Ho <= 256)
    rpb, nblocks = bands if bands is not None else (1, Ho)
    expect = dict(entry=2, KS=KS, C=MTI, NT=NT, IPW=IPW, family=fam_on if lds else fam_off, leaky=0, grid_x=nblocks, grid_y=grid_y, block=block,
                  rows_per_block=rpb, nblocks=nblocks, reducer=reducer, Ho=Ho, Wo=Wo)
    ROWS.append(dict(id="wg %s %s %dx%d p%d%s" % (tag, shape, H, W, pad, "" if lds else " nolds"), entry="wg", H=H, W=W, cin=cin, cout=cout, ks=ks, pad=pad,
                     leaky=0, lds=lds, nan=nan, nan_g=nan_g, expect=expect))


# ---- 1. every instance: all forward shapes with LEAKY on and off, the LDS forms on and off; all weight-gradient instances, staged and direct
for name, (ks, cin, cout, inst, has_lds) in FWD.items():
    for leaky in (0, 1):
        for lds in ((1, 0) if has_lds else (1,)):
            fwd("inst", name, 6, 67, leaky=leaky, lds=lds)
for name, v in WG.items():
    for lds in ((1, 0) if v[4] != v[5] else (1,)):
        wg("inst", name, 6, 67, lds=lds)
# ---- 2. seams in x: a wave owns 64 pixels, a staged wgrad chunk 32, the direct wgrad loop 16; heights so that the tile count is 1, 2, 3, 5, ...
# and the four waves of a workgroup lie on two output rows (grid = workgroups, written out: ceil(Wo / 64) Ho tiles, four per workgroup)
for i, (Wo, Ho, grid) in enumerate(((1, 1, 1), (15, 2, 1), (16, 3, 1), (17, 5, 2), (31, 2, 1), (32, 3, 1), (33, 5, 2), (63, 1, 1), (64, 3, 1), (65, 1, 1), (65, 3, 2),
                                    (127, 5, 3), (128, 1, 1), (129, 1, 1), (129, 3, 3), (193, 2, 2), (193, 5, 5), (129, 5, 4))):
    for shape, lds in (("7x7 4>16", 1), ("3x3 64>64", 1), ("3x3 64>64", 0), ("5x5 16>32", 1), ("5x5 32>16", 0), ("1x1 64>2", 1)):
        fwd("seam", shape, Ho, Wo, leaky=i % 2, lds=lds, grid=grid)                       # (SAME padding: the output has the input's size)
    for shape, lds in (("7x7 4>16", 1), ("3x3 64>64", 1), ("3x3 64>64", 0), ("5x5 16>16", 1), ("5x5 16>32", 0), ("3x3 32>64", 1), ("1x1 64>2", 1), ("3x3 17>63", 1)):
        wg("seam", shape, Ho, Wo, lds=lds)
# ---- 3. padding: none, SAME, and ks - 1 (what the input gradient of a VALID layer runs)
for shape in ("7x7 4>16", "7x7 16>4", "5x5 16>16", "3x3 64>64", "3x3 32>64"):
    ks = FWD[shape][0]
    for pad in (0, ks // 2, ks - 1):
        for lds in ((1, 0) if FWD[shape][4] else (1,)):
            fwd("pad", shape, 9, 70, pad=pad, lds=lds)
for shape in ("7x7 4>16", "5x5 16>32", "3x3 64>64", "3x3 64>60", "7x7 5>3"):
    ks = WG[shape][0]
    for pad in (0, ks // 2, ks - 1):
        for lds in ((1, 0) if WG[shape][4] != WG[shape][5] else (1,)):
            wg("pad", shape, 9, 70, pad=pad, lds=lds)
# ---- 4. images smaller than the kernel, SAME padding: most tap rows and columns are outside (the wave-uniform `continue`, zero staging)
for H, W in ((1, 1), (1, 2), (2, 1), (2, 2)):
    for shape, lds in (("7x7 4>16", 1), ("7x7 16>4", 1), ("7x7 16>4", 0), ("5x5 16>16", 1), ("5x5 16>16", 0), ("3x3 64>64", 1), ("3x3 64>64", 0)):
        fwd("small", shape, H, W, leaky=(H + W) % 2, lds=lds)
        wg("small", shape, H, W, lds=lds)
# ---- 5. row bands of 1, 2 and 3 rows (rows_per_block = ceil(Ho / 256), nblocks = ceil(Ho / rows_per_block)), last band short or full
for Ho, rpb, nblocks in ((255, 1, 255), (256, 1, 256), (257, 2, 129), (300, 2, 150), (511, 2, 256), (512, 2, 256), (513, 3, 171)):
    Wo = 70 if Ho == 513 else 35
    for shape, lds in (("3x3 64>64", 1), ("3x3 64>64", 0), ("5x5 16>32", 1), ("5x5 16>32", 0), ("7x7 4>16", 1), ("1x1 64>2", 1)):
        wg("band", shape, Ho, Wo, lds=lds, bands=(rpb, nblocks))
# ---- 6. the reducers: nblocks = Ho around the 4-wave stride and the 8-deep unrolled body (b + 28 < nblocks) of the 4-wide one
for Ho in (1, 2, 3, 4, 5, 28, 29, 32, 33, 35, 36, 60, 64, 65):
    for shape in ("5x5 16>16", "1x1 64>2", "3x3 63>63"):
        wg("reduce", shape, Ho, 17, bands=(1, Ho))
# ---- 7. NaN containment: first and last pixel, a row end, the last true channel where cin < CINP
for shape, lds in (("7x7 3>15", 1), ("5x5 16>16", 1), ("5x5 16>16", 0), ("3x3 64>64", 1), ("3x3 64>64", 0)):
    cin = FWD[shape][1]
    for nan in ((0, 0, 0), (8, 69, cin - 1), (4, 69, cin // 2), (5, 0, cin - 1)):
        fwd("nan%d.%d.%d" % nan, shape, 9, 70, lds=lds, nan=nan)
        fwd("nan%d.%d.%d" % nan, shape, 9, 70, pad=0, lds=lds, nan=nan)
for shape, lds in (("7x7 3>15", 1), ("5x5 16>16", 1), ("5x5 16>16", 0), ("3x3 64>64", 1), ("3x3 64>64", 0), ("3x3 17>63", 1)):
    cin, cout = WG[shape][1], WG[shape][2]
    for nan in ((0, 0, 0), (8, 69, cin - 1), (4, 69, cin // 2), (5, 0, cin - 1), (4, 66, 0)):
        wg("nan%d.%d.%d" % nan, shape, 9, 70, lds=lds, nan=nan)
        wg("nan%d.%d.%d" % nan, shape, 9, 70, pad=0, lds=lds, nan=nan)
    ks = WG[shape][0]
    wg("nang-first", shape, 9, 70, pad=0, lds=lds, nan_g=(0, 0, 0))
    wg("nang-last", shape, 9, 70, pad=0, lds=lds, nan_g=(9 - ks, 70 - ks, cout - 1))
    wg("nang-inner", shape, 9, 70, lds=lds, nan_g=(4, 35, cout // 2))
assert len({r["id"] for r in ROWS}) == len(ROWS)


def ids(entry=None):
    return [r["id"] for r in ROWS if entry is None or r["entry"] == entry]


ROW = {r["id"]: r for r in ROWS}


# ------------------------------------------------------------------------------------------------------------------------------------
# calling the C ABI
def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guard_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def call_forward(x, w_hwio, pad, leaky):
    """(status, out [Ho][Wo][cout] as numpy, guard cells intact) of piso_conv2d_forward on host arrays."""
    import diffpiso._native as N
    from diffpiso.closure import _laid_out
    H, W, cin = x.shape
    ks, cout = w_hwio.shape[0], w_hwio.shape[3]
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    xd, wl = torch.from_numpy(x).cuda(), _laid_out(torch.from_numpy(w_hwio).cuda())
    assert wl.numel() == N.lib.piso_conv2d_weight_elems(ks, cin, cout)
    buf, out = _guarded(Ho * Wo * cout)
    st = N.lib.piso_conv2d_forward(N.ptr(xd), N.ptr(wl), C.c_void_p(out.data_ptr()), H, W, cin, cout, ks, pad, leaky, N.stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy().reshape(Ho, Wo, cout), _guard_intact(buf, out.numel())


def call_wgrad(x, g, ks, pad):
    import diffpiso._native as N
    H, W, cin = x.shape
    cout = g.shape[2]
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    nbytes = N.lib.piso_conv2d_wgrad_workspace_bytes(ks, cin, cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    buf, dw = _guarded(ks * ks * cin * cout)
    st = N.lib.piso_conv2d_wgrad(N.ptr(xd), N.ptr(gd), C.c_void_p(dw.data_ptr()), H, W, cin, cout, ks, pad, N.ptr(ws), C.c_size_t(nbytes), N.stream_ptr())
    torch.cuda.synchronize()
    return st, dw.cpu().numpy().reshape(ks, ks, cin, cout), _guard_intact(buf, dw.numel())


def _data(r, kind):
    rng = np.random.default_rng(2 * zlib.crc32(r["id"].encode()) + (kind == "int"))          # a fixed seed per row and leg
    draw = (lambda s: rng.integers(-3, 4, s).astype(f32)) if kind == "int" else (lambda s: rng.standard_normal(s).astype(f32))
    Ho, Wo = r["expect"]["Ho"], r["expect"]["Wo"]
    return draw((r["H"], r["W"], r["cin"])), draw((r["ks"], r["ks"], r["cin"], r["cout"])), draw((Ho, Wo, r["cout"]))


def _first_bad(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def assert_bitwise(got, want, what):
    bad = got.view(np.int32) != want.astype(f32).view(np.int32)
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: %d of %d elements differ from the float64 reference, first at %s: got %r, want %r" % (what, bad.sum(), bad.size, i, got[i], want[i]))


def assert_roundoff(got, want, S, K, what):
    bound = C_ROUND * math.sqrt(K) * U * S
    bad = ~(np.abs(got.astype(f64) - want) <= bound)
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: %d elements beyond %g sqrt(%d) u S, first at %s: got %r, want %r, bound %g" % (what, bad.sum(), C_ROUND, K, i, got[i], want[i], bound[i]))


def _set_lds(piso_option, lds):
    piso_option("conv_lds", -1 if lds else 0)


# ------------------------------------------------------------------------------------------------------------------------------------
pytest_gpu = pytest.mark.gpu


@pytest_gpu
@pytest.mark.parametrize("rid", ids("fwd"))
def test_forward_row(rid, piso_option):
    import diffpiso._native as N
    r = ROW[rid]
    _set_lds(piso_option, r["lds"])
    pad, leaky, K = r["pad"], r["leaky"], r["ks"] * r["ks"] * r["cin"]
    # exact leg
    x, w, _ = _data(r, "int")
    nanmask = None
    if r["nan"] is not None:
        hit = np.zeros(x.shape, f64)
        hit[r["nan"]] = 1.0
        nanmask = ref_forward(hit, np.ones_like(w), pad) > 0            # the outputs whose sum has a term with that element
        assert nanmask.any() and not nanmask.all()
    want = ref_forward(x, w, pad)
    assert np.abs(want).max() < 2 ** 24
    if r["nan"] is not None:
        x[r["nan"]] = np.nan
    st, got, intact = call_forward(x, w, pad, leaky)
    assert st == 0, N.lib.piso_last_error_string()
    assert N.conv_last_dispatch() == r["expect"]
    assert intact, "written outside out[Ho][Wo][cout]"
    want32 = leaky32(want) if leaky else want.astype(f32)
    if nanmask is not None:
        assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern", _first_bad(np.isnan(got) != nanmask))
        got, want32 = np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), want32)
    assert_bitwise(got, want32, "forward, integer data")
    if r["nan"] is not None:
        return
    # round-off leg
    x, w, _ = _data(r, "normal")
    want, S = ref_forward(x, w, pad), ref_forward(np.abs(x), np.abs(w), pad)
    if leaky:
        want = np.where(want > 0, want, 0.2 * want)
    st, got, intact = call_forward(x, w, pad, leaky)
    assert st == 0 and intact
    assert_roundoff(got, want, S, K + 1, "forward, normal data")


@pytest_gpu
@pytest.mark.parametrize("rid", ids("wg"))
def test_wgrad_row(rid, piso_option):
    import diffpiso._native as N
    r = ROW[rid]
    _set_lds(piso_option, r["lds"])
    pad, ks, K = r["pad"], r["ks"], r["expect"]["Ho"] * r["expect"]["Wo"]
    x, _, g = _data(r, "int")
    nanmask = None
    if r["nan"] is not None or r["nan_g"] is not None:
        hx, hg = np.zeros(x.shape, f64), np.zeros(g.shape, f64)
        if r["nan"] is not None:
            hx[r["nan"]] = 1.0
            nanmask = ref_wgrad(hx, np.ones_like(g), ks, pad) > 0
        else:
            hg[r["nan_g"]] = 1.0
            nanmask = ref_wgrad(np.ones_like(x), hg, ks, pad) > 0
        assert nanmask.any() and not nanmask.all()
    want = ref_wgrad(x, g, ks, pad)
    assert np.abs(want).max() < 2 ** 24
    if r["nan"] is not None:
        x[r["nan"]] = np.nan
    if r["nan_g"] is not None:
        g[r["nan_g"]] = np.nan
    st, got, intact = call_wgrad(x, g, ks, pad)
    assert st == 0, N.lib.piso_last_error_string()
    assert N.conv_last_dispatch() == r["expect"]
    assert intact, "written outside dw[ks][ks][cin][cout]"
    want32 = want.astype(f32)
    if nanmask is not None:
        assert np.array_equal(np.isnan(got), nanmask), ("NaN pattern (ky, kx, ci, co)", _first_bad(np.isnan(got) != nanmask))
        got, want32 = np.where(nanmask, f32(0), got), np.where(nanmask, f32(0), want32)
    assert_bitwise(got, want32, "weight gradient, integer data")
    if nanmask is not None:
        return
    x, _, g = _data(r, "normal")
    want, S = ref_wgrad(x, g, ks, pad), ref_wgrad(np.abs(x), np.abs(g), ks, pad)
    st, got, intact = call_wgrad(x, g, ks, pad)
    assert st == 0 and intact
    assert_roundoff(got, want, S, K, "weight gradient, normal data")


# ---- the autograd path: conv2d_leaky, every layer and padding mode, integer data, exact.  The input gradient runs piso_conv2d_forward with
# the flipped, transposed layout of closure._cached_layouts; the expectation is ref_dgrad, written from the definition
LAYERS = [(7, 4, 16), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 64), (1, 64, 64), (1, 64, 2)]


@pytest_gpu
@pytest.mark.parametrize("ks,cin,cout", LAYERS)
@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("leaky", [True, False])
def test_autograd_path_is_exact_on_integer_data(ks, cin, cout, same, leaky):
    from diffpiso.closure import conv2d_leaky
    rng = np.random.default_rng(1000 * ks + cin + cout + same)
    H, W, pad = 11, 70, (ks // 2 if same else 0)
    x = rng.integers(-3, 4, (H, W, cin)).astype(f32)
    w = rng.integers(-3, 4, (ks, ks, cin, cout)).astype(f32)
    xt = torch.from_numpy(x)[None].cuda().requires_grad_(True)
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))).cuda().requires_grad_(True)        # OIHW
    y = conv2d_leaky(xt, wt, pad, leaky)
    pre = ref_forward(x, w, pad)
    assert_bitwise(y.detach().cpu().numpy()[0], leaky32(pre) if leaky else pre, "forward")
    g = rng.integers(-3, 4, pre.shape).astype(f32)
    if leaky:
        # the gradient of the pre-activation: g or 0.2f g (one float32 product, inexact); keep the exact leg exact with multiples of 5 where
        # the slope applies - 0.2f * (5 m) rounds to m for small m (0.2f = 0.2 (1 + 7.5e-9))
        g = np.where(pre > 0, g, 5 * g).astype(f32)
    y.backward(torch.from_numpy(g)[None].cuda())
    gp = np.where(pre > 0, g, f32(0.2) * g).astype(f32) if leaky else g
    assert np.array_equal(gp, np.round(gp)) and np.abs(gp).max() <= 3
    assert_bitwise(xt.grad.cpu().numpy()[0], ref_dgrad(gp, w, pad, H, W), "input gradient")
    dw = wt.grad.cpu().numpy().transpose(2, 3, 1, 0)                                                        # OIHW -> HWIO
    assert_bitwise(np.ascontiguousarray(dw), ref_wgrad(x, gp, ks, pad), "weight gradient")


# ---- conv_lds is bitwise neutral: forward, input gradient, weight gradient, normal data
@pytest_gpu
@pytest.mark.parametrize("shape", [n for n, v in FWD.items() if v[4]])
@pytest.mark.parametrize("hw", [(19, 70), (7, 129)])
def test_conv_lds_is_bitwise_neutral_forward_and_input_gradient(shape, hw, piso_option):
    import diffpiso._native as N
    ks, cin, cout, _, _ = FWD[shape]
    rng = np.random.default_rng(ks + cin + cout)
    x, w = rng.standard_normal(hw + (cin,)).astype(f32), rng.standard_normal((ks, ks, cin, cout)).astype(f32)
    for pad in (0, ks // 2, ks - 1):                         # (ks - 1: the input gradient of a VALID layer)
        res = {}
        for lds in (1, 0):
            _set_lds(piso_option, lds)
            st, out, _ = call_forward(x, w, pad, 1)
            assert st == 0 and N.conv_last_dispatch()["family"] == (FWD_LDS if lds else FWD_DIRECT)
            res[lds] = out
        assert np.array_equal(res[0].view(np.int32), res[1].view(np.int32)), (shape, pad)


@pytest_gpu
@pytest.mark.parametrize("shape", [n for n, v in WG.items() if v[4] != v[5]])
@pytest.mark.parametrize("hw", [(19, 70), (300, 33)])
def test_conv_lds_is_bitwise_neutral_weight_gradient(shape, hw, piso_option):
    import diffpiso._native as N
    ks, cin, cout = WG[shape][:3]
    rng = np.random.default_rng(ks + cin + cout)
    for pad in (0, ks // 2):
        Ho, Wo = hw[0] + 2 * pad - ks + 1, hw[1] + 2 * pad - ks + 1
        x, g = rng.standard_normal(hw + (cin,)).astype(f32), rng.standard_normal((Ho, Wo, cout)).astype(f32)
        res = {}
        for lds in (1, 0):
            _set_lds(piso_option, lds)
            st, dw, _ = call_wgrad(x, g, ks, pad)
            assert st == 0 and N.conv_last_dispatch()["family"] == (WG[shape][4] if lds else WG[shape][5])
            res[lds] = dw
        assert np.array_equal(res[0].view(np.int32), res[1].view(np.int32)), (shape, pad)


# ---- piso_leaky_relu_backward against torch's own rule, bit for bit
LEAKY_CAP = 4096 * 512           # float4 elements one sweep of the capped grid covers (grid_for(n4, 512, 4096) workgroups of 256 threads x 2)


@pytest_gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * LEAKY_CAP + 4 * 1000 + 3])
def test_leaky_relu_backward_matches_torch_bitwise(n):
    import diffpiso._native as N
    rng = np.random.default_rng(n)
    out = rng.standard_normal(n).astype(f32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, np.nan, np.inf, -np.inf, 1.0, -1.0], f32)
    # at the start, around the middle and in the last elements: the float4 body, its grid-stride repeats and the scalar tail all meet them
    idx = np.unique(np.clip(np.concatenate([np.arange(9), n // 2 + np.arange(9), n - 9 + np.arange(9)]), 0, n - 1))
    out[idx] = special[np.arange(len(idx)) % len(special)]
    g = rng.standard_normal(n).astype(f32)
    if n > 8:
        g[n - 2], g[5] = np.nan, np.inf
    pre = torch.from_numpy(out).clone().requires_grad_(True)                  # torch's CPU rule on the pre-activation: the kernel sees the OUTPUT,
    y = torch.nn.functional.leaky_relu(pre, 0.2)                              # which has the pre-activation's sign (and its zeros, denormals, NaN)
    y.backward(torch.from_numpy(g))
    want = pre.grad.numpy()
    buf, gp = _guarded(n)
    od = y.detach().cuda()
    assert torch.equal(torch.signbit(od.cpu()) | od.cpu().isnan(), torch.signbit(pre.detach()) | pre.detach().isnan())
    st = N.lib.piso_leaky_relu_backward(N.ptr(torch.from_numpy(g).cuda()), N.ptr(od), C.c_void_p(gp.data_ptr()), C.c_size_t(n), N.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and _guard_intact(buf, n)
    got = gp.cpu().numpy()
    both_nan = np.isnan(got) & np.isnan(want)
    bad = (got.view(np.int32) != want.view(np.int32)) & ~both_nan
    assert not bad.any(), (int(bad.sum()), _first_bad(bad), got[bad][:4], want[bad][:4], out[bad][:4])


# ---- refusals launch nothing: status PISO_ERR_INVALID_ARG, the record and the output untouched
# name, entry, pointers (fwd: in, w_laid_out, out; wg: in, grad_out, dw, workspace - "p" a valid one, "0" NULL, "+4" four bytes off 16-byte
# alignment), H, W, cin, cout, ks, pad, wg: workspace_bytes ("nbytes": what 5 x 5 16 -> 16 needs, "short": one byte less, "roomy": what
# 5 x 5 64 -> 64 needs - enough for every shape below, were it to launch)
REFUSALS = [("null in", "fwd", "0 p p", 6, 20, 16, 16, 5, 2), ("null w", "fwd", "p 0 p", 6, 20, 16, 16, 5, 2), ("null out", "fwd", "p p 0", 6, 20, 16, 16, 5, 2),
            ("Ho < 1", "fwd", "p p p", 4, 20, 16, 16, 5, 0), ("Wo < 1", "fwd", "p p p", 6, 3, 16, 16, 5, 0), ("cin 5", "fwd", "p p p", 6, 20, 5, 16, 5, 2),
            ("cin 0", "fwd", "p p p", 6, 20, 0, 16, 5, 2), ("cout 65", "fwd", "p p p", 6, 20, 16, 65, 5, 2), ("cout 0", "fwd", "p p p", 6, 20, 16, 0, 5, 2),
            ("cin 80", "fwd", "p p p", 6, 20, 80, 16, 5, 2), ("not instantiated 5x5 64>64", "fwd", "p p p", 6, 20, 64, 64, 5, 2),
            ("not instantiated 2x2", "fwd", "p p p", 6, 20, 16, 16, 2, 0), ("in off 16-byte alignment", "fwd", "+4 p p", 6, 20, 16, 16, 5, 2),
            ("w off 16-byte alignment", "fwd", "p +4 p", 6, 20, 16, 16, 5, 2),
            ("wg null in", "wg", "0 p p p", 6, 20, 16, 16, 5, 2, "nbytes"), ("wg null g", "wg", "p 0 p p", 6, 20, 16, 16, 5, 2, "nbytes"),
            ("wg null dw", "wg", "p p 0 p", 6, 20, 16, 16, 5, 2, "nbytes"), ("wg null workspace", "wg", "p p p 0", 6, 20, 16, 16, 5, 2, "nbytes"),
            ("wg workspace one byte short", "wg", "p p p p", 6, 20, 16, 16, 5, 2, "short"), ("wg Ho < 1", "wg", "p p p p", 4, 20, 16, 16, 5, 0, "nbytes"),
            ("wg Wo < 1", "wg", "p p p p", 6, 4, 16, 16, 5, 0, "nbytes"), ("wg cout 65", "wg", "p p p p", 6, 20, 16, 65, 5, 2, "roomy"),
            ("wg cin 65", "wg", "p p p p", 6, 20, 65, 16, 5, 2, "roomy"), ("wg cin 0", "wg", "p p p p", 6, 20, 0, 16, 5, 2, "nbytes"),
            ("wg not instantiated 5x5 64>64", "wg", "p p p p", 6, 20, 64, 64, 5, 2, "roomy"), ("wg not instantiated 7x7 4>32", "wg", "p p p p", 9, 20, 4, 32, 7, 3, "roomy"),
            ("wg in off 16-byte alignment", "wg", "+4 p p p", 6, 20, 16, 16, 5, 2, "nbytes"), ("wg g off 16-byte alignment", "wg", "p +4 p p", 6, 20, 16, 16, 5, 2, "nbytes"),
            ("wg dw off 16-byte alignment", "wg", "p p +4 p", 6, 20, 16, 16, 5, 2, "nbytes"),
            ("wg workspace off 16-byte alignment", "wg", "p p p +4", 6, 20, 16, 16, 5, 2, "nbytes")]
assert len({c[0] for c in REFUSALS}) == len(REFUSALS) == 30


def workspace_bytes(ks, cin, cout):
    """include/piso_hip.h: 256 band partials of [ks][ks][cin rounded up to 16][cout rounded up to 16] floats."""
    return 256 * ks * ks * (-(-cin // 16) * 16) * (-(-cout // 16) * 16) * 4


REFUSAL_BYTES = {"nbytes": workspace_bytes(5, 16, 16), "short": workspace_bytes(5, 16, 16) - 1, "roomy": workspace_bytes(5, 64, 64)}


@pytest_gpu
def test_refusals_leave_record_and_output_untouched(piso_option):
    import diffpiso._native as N
    INVALID = 1
    x, w = np.ones((6, 20, 16), f32), np.ones((5, 5, 16, 16), f32)
    st, _, _ = call_forward(x, w, 2, 0)
    assert st == 0
    before = N.conv_last_dispatch()
    assert before["entry"] == 1 and before["KS"] == 5

    big = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")            # operands large enough for every shape below, were it to launch
    buf, out = _guarded(1 << 16)
    assert N.lib.piso_conv2d_wgrad_workspace_bytes(5, 16, 16) == REFUSAL_BYTES["nbytes"] and N.lib.piso_conv2d_wgrad_workspace_bytes(5, 64, 64) == REFUSAL_BYTES["roomy"]
    ws = torch.empty(REFUSAL_BYTES["roomy"], dtype=torch.uint8, device="cuda")
    p, po = C.c_void_p(big.data_ptr()), C.c_void_p(out.data_ptr())

    def pointer(token, base):
        return None if token == "0" else C.c_void_p(base + 4) if token == "+4" else C.c_void_p(base)

    cases = {}
    for name, entry, ptrs, H, W, cin, cout, ks, pad, *nb in REFUSALS:
        t = ptrs.split()
        a = [pointer(t[0], big.data_ptr()), pointer(t[1], big.data_ptr()), pointer(t[2], out.data_ptr())]
        if entry == "fwd":
            cases[name] = N.lib.piso_conv2d_forward(a[0], a[1], a[2], H, W, cin, cout, ks, pad, 0, N.stream_ptr())
        else:
            cases[name] = N.lib.piso_conv2d_wgrad(a[0], a[1], a[2], H, W, cin, cout, ks, pad, pointer(t[3], ws.data_ptr()), C.c_size_t(REFUSAL_BYTES[nb[0]]), N.stream_ptr())
    for n_null in ("g", "out", "gp"):
        a = [p, p, po]
        a["g out gp".split().index(n_null)] = None
        cases["leaky null " + n_null] = N.lib.piso_leaky_relu_backward(a[0], a[1], a[2], C.c_size_t(16), N.stream_ptr())
    torch.cuda.synchronize()
    assert len(cases) == 33
    assert {k: v for k, v in cases.items() if v != INVALID} == {}
    assert N.conv_last_dispatch() == before
    assert bool((buf == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU-only tests
def test_census_of_kernel_instances():
    """Pure Python: the EXPECTED records of the table (each asserted against the card by the row's own test) reach every compiled instance of
    conv.hip: 22 direct and 14 LDS forward kernels, 7 generic wgrad instances direct and staged, PACK4, both 64 -> 64 kernels, both reducers,
    bands of 1, 2 and 3 rows."""
    e = [r["expect"] for r in ROWS]
    fw = {(x["KS"], x["C"], x["NT"], x["leaky"], x["family"]) for x in e if x["entry"] == 1}
    shapes = [(7, 4, 1), (7, 16, 1), (5, 16, 1), (5, 16, 2), (5, 32, 1), (3, 32, 4), (3, 64, 2), (3, 64, 4), (1, 64, 4), (1, 64, 1), (1, 4, 4)]
    direct = {s + (lk, FWD_DIRECT) for s in shapes for lk in (0, 1)}
    lds = {s + (lk, FWD_LDS) for s in shapes if s[1] >= 16 and s[0] >= 3 for lk in (0, 1)}
    assert len(direct) == 22 and len(lds) == 14 and fw == direct | lds, sorted((direct | lds) ^ fw)
    wgs = {(x["KS"], x["C"], x["NT"], x["IPW"], x["family"]) for x in e if x["entry"] == 2}
    generic = [(7, 1, 1, 3), (5, 1, 1, 2), (5, 1, 2, 2), (3, 2, 4, 1), (3, 4, 4, 1), (1, 4, 4, 1), (1, 4, 1, 1)]
    want = {s + (f,) for s in generic for f in (WG_GENERIC, WG_GENERIC_LDS)} | {(7, 1, 1, 1, WG_PACK4), (3, 4, 4, 1, WG_64), (3, 4, 4, 1, WG_64_LDS)}
    assert len(want) == 17 and wgs == want, sorted(want ^ wgs)
    assert {x["reducer"] for x in e if x["entry"] == 2} == {1, 4}
    assert {x["rows_per_block"] for x in e if x["entry"] == 2} == {1, 2, 3}
    for fam in (WG_GENERIC, WG_GENERIC_LDS, WG_PACK4, WG_64, WG_64_LDS):                                     # every family with bands of more than one row
        assert {x["rows_per_block"] for x in e if x["entry"] == 2 and x["family"] == fam} >= {1, 2, 3}, fam
    assert {x["nblocks"] for x in e if x["reducer"] == 4} >= {1, 2, 3, 4, 5, 28, 29, 32, 33, 35, 36, 60, 64, 65, 129, 171, 256}
    assert {x["nblocks"] for x in e if x["reducer"] == 1} >= {1, 2, 3, 4, 5, 28, 29, 32, 33, 35, 36, 60, 64, 65, 129, 171, 256}


def expected_record(entry, H, W, cin, cout, ks, pad, conv_lds):
    """The dispatch rules of conv.hip restated: what piso_conv_last_dispatch must report for a call."""
    Ho, Wo = H + 2 * pad - ks + 1, W + 2 * pad - ks + 1
    nt = -(-cout // 16)
    if entry == "fwd":
        cinp = 4 if cin <= 4 else -(-cin // 16) * 16
        tiles = -(-Wo // 64) * Ho
        return dict(entry=1, KS=ks, C=cinp, NT=nt, IPW=0, family=int(bool(conv_lds) and cinp >= 16 and ks >= 3), grid_x=-(-tiles // 4), grid_y=1, block=256,
                    rows_per_block=0, nblocks=0, reducer=0, Ho=Ho, Wo=Wo)
    mti = -(-cin // 16)
    rpb = -(-Ho // 256)
    nblocks = -(-Ho // rpb)
    reducer = 4 if cout % 4 == 0 else 1
    if (ks, cin, cout) == (3, 64, 64):
        ipw, family, grid_y, block = 1, WG_64_LDS if conv_lds else WG_64, 3, 192
    elif ks == 7 and cin <= 4 and nt == 1:
        ipw, family, grid_y, block = 1, WG_PACK4, -(-(7 * 2) // 4), 256                                     # items: 7 tap rows x 2 groups of 4 tap columns
    else:
        ipw = {7: 3, 5: 2, 3: 1, 1: 1}[ks]
        family = WG_GENERIC_LDS if (conv_lds and cin % 4 == 0 and cout % 4 == 0) else WG_GENERIC
        grid_y, block = -(-(ks * ks * mti) // (4 * ipw)), 256
    return dict(entry=2, KS=ks, C=mti, NT=nt, IPW=ipw, family=family, grid_x=nblocks, grid_y=grid_y, block=block, rows_per_block=rpb, nblocks=nblocks,
                reducer=reducer, Ho=Ho, Wo=Wo)


@pytest.mark.parametrize("rid", ids())
def test_table_literals_agree_with_the_dispatch_rules(rid):
    r = ROW[rid]
    want = expected_record(r["entry"], r["H"], r["W"], r["cin"], r["cout"], r["ks"], r["pad"], r["lds"])
    want["leaky"] = r["leaky"]
    assert r["expect"] == want


def _host_compiler():
    """A C++17 host compiler: (argv prefix, its name), or None."""
    import shutil
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cxx in ("c++", "g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        path = shutil.which(cxx)
        if path:
            return [path], cxx
    hipcc = shutil.which("hipcc") or shutil.which(os.path.join(rocm, "bin", "hipcc"))
    return ([hipcc, "-x", "c++"], "hipcc -x c++") if hipcc else None


def test_conv_plan_on_the_host(tmp_path):
    """conv_plan (csrc/conv_dispatch.h) is pure: tests/conv_plan_driver.cpp, built with a host compiler from a translation unit that includes
    nothing of HIP, plans every row of ROWS - the record it would leave must equal the row's literal expectation field for field - and every
    case of REFUSALS (null and misaligned pointers as the query's flags): PISO_ERR_INVALID_ARG with the entry point's message."""
    import subprocess
    import diffpiso._native as N
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no C++17 host compiler (tried c++, g++, clang++, ROCm's clang++, hipcc -x c++)")
    exe = str(tmp_path / "conv_plan_driver")
    subprocess.run(cxx[0] + ["-std=c++17", "-O1", "-o", exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_plan_driver.cpp")], check=True)
    q = ["%d %d %d %d %d %d %d %d %d 0 0 0 -1" % (1 if r["entry"] == "fwd" else 2, r["H"], r["W"], r["cin"], r["cout"], r["ks"], r["pad"], r["leaky"], -1 if r["lds"] else 0)
         for r in ROWS]
    for name, entry, ptrs, H, W, cin, cout, ks, pad, *nb in REFUSALS:
        t = ptrs.split()
        q.append("%d %d %d %d %d %d %d 0 -1 %d %d %d %d" % (1 if entry == "fwd" else 2, H, W, cin, cout, ks, pad, "0" in t, "+4" in t[:2], "+4" in t[2:],
                                                         REFUSAL_BYTES[nb[0]] if nb else 0))
    res = subprocess.run([exe], input="\n".join(q) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(res) == len(ROWS) + len(REFUSALS)
    bad = {}
    for r, line in zip(ROWS, res):
        status, msg, *rec = line.split("\t")
        got = dict(zip(N.CONV_DISPATCH_FIELDS, map(int, rec)))
        if (status, msg) != ("0", "-") or len(rec) != len(N.CONV_DISPATCH_FIELDS) or got != r["expect"]:
            bad[r["id"]] = (status, msg, got, r["expect"])
    for (name, entry, *_), line in zip(REFUSALS, res[len(ROWS):]):
        status, msg, *rec = line.split("\t")
        if status != "1" or not msg.startswith("piso_conv2d_forward: " if entry == "fwd" else "piso_conv2d_wgrad: "):
            bad[name] = (status, msg)
    assert bad == {}, "planned with %s" % cxx[1]


def test_record_fields_of_the_binding_are_the_header_s():
    """The binding's field names, in order, are the ones include/piso_hip.h documents for piso_conv_last_dispatch."""
    import re
    import diffpiso._native as N
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "piso_hip.h")).read()
    doc = hdr[:hdr.index("int piso_conv_last_dispatch(int* out, int capacity);")]
    doc = doc[doc.rindex("/* Which kernel instance"):]
    fields = re.findall(r"^ \*\s+(\d+) (\w+)\s", doc, re.M)
    assert [int(i) for i, _ in fields] == list(range(len(N.CONV_DISPATCH_FIELDS)))
    assert tuple(n for _, n in fields) == N.CONV_DISPATCH_FIELDS


@pytest.mark.parametrize("ks,cin,cout,pad,H,W", [(7, 4, 16, 3, 9, 12), (7, 3, 5, 6, 4, 5), (5, 16, 8, 0, 7, 9), (5, 2, 3, 4, 2, 3), (3, 6, 7, 1, 1, 2), (3, 5, 4, 2, 6, 6),
                                                 (1, 9, 2, 0, 3, 4), (3, 4, 4, 0, 5, 8)])
def test_reference_against_torch_float64_convolution(ks, cin, cout, pad, H, W):
    """The numpy restatement, forward and both gradients, against torch.nn.functional.conv2d and its autograd on the host in float64."""
    rng = np.random.default_rng(ks + cin + cout + pad)
    x, w = rng.standard_normal((H, W, cin)), rng.standard_normal((ks, ks, cin, cout))
    xt = torch.from_numpy(x).permute(2, 0, 1)[None].requires_grad_(True)
    wt = torch.from_numpy(w).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt, padding=pad)
    out = ref_forward(x, w, pad)
    assert out.shape == (H + 2 * pad - ks + 1, W + 2 * pad - ks + 1, cout)
    np.testing.assert_allclose(out, y[0].permute(1, 2, 0).detach().numpy(), rtol=0, atol=1e-12)
    g = rng.standard_normal(out.shape)
    y.backward(torch.from_numpy(g).permute(2, 0, 1)[None])
    np.testing.assert_allclose(ref_dgrad(g, w, pad, H, W), xt.grad[0].permute(1, 2, 0).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref_wgrad(x, g, ks, pad), wt.grad.permute(2, 3, 1, 0).numpy(), rtol=0, atol=1e-12)
    # integer data: the reference itself is exact
    xi, wi = rng.integers(-3, 4, x.shape).astype(f64), rng.integers(-3, 4, w.shape).astype(f64)
    assert np.array_equal(ref_forward(xi, wi, pad), np.round(ref_forward(xi, wi, pad)))


def _layout_by_the_header(w):
    """include/piso_hip.h, plain loops: cin <= 4: [ks][ks][4][COUTP]; else [ks][ks][cin / 16][4][COUTP][4] with
    element [tap][blk][q][co][j] = W[tap][16 blk + 4 q + j][co]; zero beyond the true channel counts."""
    ks, _, cin, cout = w.shape
    coutp = -(-cout // 16) * 16
    if cin <= 4:
        out = np.zeros((ks, ks, 4, coutp), f32)
        for ci in range(cin):
            for co in range(cout):
                out[:, :, ci, co] = w[:, :, ci, co]
        return out
    out = np.zeros((ks, ks, cin // 16, 4, coutp, 4), f32)
    for blk in range(cin // 16):
        for q in range(4):
            for j in range(4):
                for co in range(cout):
                    out[:, :, blk, q, co, j] = w[:, :, 16 * blk + 4 * q + j, co]
    return out


@pytest.mark.parametrize("ks,cin,cout", [(7, 1, 1), (7, 2, 3), (7, 3, 15), (7, 4, 16), (1, 2, 64), (1, 3, 63), (7, 16, 4), (5, 16, 17), (5, 32, 16), (3, 32, 64), (3, 64, 63),
                                         (3, 64, 64), (1, 64, 2)])
def test_laid_out_against_the_header_formula(ks, cin, cout):
    from diffpiso.closure import _laid_out
    w = np.random.default_rng(ks * cin + cout).standard_normal((ks, ks, cin, cout)).astype(f32)
    got = _laid_out(torch.from_numpy(w)).numpy()
    want = _layout_by_the_header(w)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got.size == ks * ks * (4 if cin <= 4 else cin) * (-(-cout // 16) * 16)
