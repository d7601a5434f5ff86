"""Host side of the fused spectral loss, no GPU: the entry points of csrc/loss_spectrum.hip - declared in include/piso_hip.h, exported from
the library, bound with the header's argument counts - the crop window on cell indices, and the shell tables of `losses.spectrum_plan`
against the torch expression of EK_spectrum_2D_tf they restate.  The crops: both sizes even (16 x 16, 12 x 20), both odd (11 x 13), exactly
one odd (9 x 8, 9 x 16, 7 x 10, 13 x 16 - radii of exactly k + 1/2 occur and torch.round sends them to the EVEN shell), and the smallest
legal ones (2 x 2, 3 x 2: cutoff 1)."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "spectral_loss.npz")
ENTRIES = ["piso_loss_centre_crop", "piso_loss_centre_crop_adjoint", "piso_loss_spectrum_shells", "piso_loss_spectrum_shells_adjoint",
           "piso_loss_spectrum_distance"]
CROPS = [(16, 16), (12, 20), (9, 8), (9, 16), (11, 13), (7, 10), (13, 16), (2, 2), (3, 2)]


def test_spectrum_entries_are_declared_exported_and_bound():
    from diffpiso import _native as N
    header = open(os.path.join(ROOT, "include", "piso_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/piso_hip.h" % name
        fn = getattr(N.lib, name)                            # (AttributeError: the library does not export it)
        assert len(fn.argtypes) == len(m.group(1).split(",")), (name, len(fn.argtypes), m.group(1))
    for phrase in ("piso_loss_centre_crop:", "piso_loss_spectrum_shells:", "piso_loss_spectrum_distance:", "on CELL indices", "UNSHIFTED"):
        assert phrase in header, phrase


def test_spectrum_window_is_the_slicing_of_the_torch_loss():
    from diffpiso.losses import spectrum_window
    checked = 0
    for ny, nx in ((12, 16), (13, 9)):
        grid = np.arange(ny * nx).reshape(ny, nx)
        for a, b, c, d in itertools.product((0, 1, 2, ny - 3, ny + 2), (0, 2, ny + 1), (0, 2, 3), (0, 1, nx + 2)):
            for sponge in (0, 7, nx, nx + 5, 2):
                # losses.py: central[:, bw[0][0]:rows - bw[0][1], bw[1][0]:sponge_start - bw[1][1]], sponge_start 0 = the field's width
                want = grid[slice(a, ny - b), slice(c, (sponge if sponge != 0 else nx) - d)]
                y0, y1, x0, x1 = spectrum_window([[a, b], [c, d]], sponge, ny, nx)
                assert 0 <= y0 <= y1 <= ny and 0 <= x0 <= x1 <= nx
                got = grid[y0:y1, x0:x1]
                assert got.size == want.size and np.array_equal(got.ravel(), want.ravel()), (ny, nx, a, b, c, d, sponge)
                checked += 1
    assert checked > 400
    # the windows of the GPU test on the 12 x 16 golden grid
    assert spectrum_window([[0, 0], [0, 0]], 0, 12, 16) == (0, 12, 0, 16)
    assert spectrum_window([[1, 2], [2, 1]], 0, 12, 16) == (1, 10, 2, 15)
    assert spectrum_window([[0, 0], [1, 1]], 10, 12, 16) == (0, 12, 1, 9)
    assert spectrum_window([[2, 1], [3, 5]], 0, 12, 16) == (2, 11, 3, 11)


def torch_shells(h, w):
    """`wvn` of EK_spectrum_2D_tf (its float32 expression) on the SHIFTED index, [h, w] int64."""
    ii = (torch.arange(h, dtype=torch.float32) - h / 2) ** 2
    jj = (torch.arange(w, dtype=torch.float32) - w / 2) ** 2
    return torch.round(torch.sqrt(ii[:, None] + jj[None, :])).to(torch.int64).numpy()


@pytest.mark.parametrize("crop", CROPS)
def test_plan_is_the_binning_of_the_torch_spectrum(crop):
    from diffpiso.evaluation_tools import EK_spectrum_2D_tf, tf_fftshift
    from diffpiso.losses import spectrum_plan
    h, w = crop
    plan = spectrum_plan(h, w, "cpu")
    assert plan is spectrum_plan(h, w, "cpu"), "the plan is not cached"
    cutoff = min(h, w) // 2
    shell, perm, offsets = plan.shell.numpy(), plan.perm.numpy(), plan.offsets.numpy()
    assert plan.cutoff == cutoff and (plan.h, plan.w) == (h, w)
    assert shell.dtype == perm.dtype == offsets.dtype == np.int32 and shell.shape == (h * w,) and offsets.shape == (cutoff + 1,)
    # shell = wvn read through the shift: the torch path adds shifted[p] into wvn[p], and shifted = tf_fftshift(unshifted)
    q_of_p = tf_fftshift(torch.arange(h * w).reshape(h, w)).numpy()        # the unshifted index that lands at every shifted place
    want = np.empty(h * w, np.int64)
    want[q_of_p.ravel()] = torch_shells(h, w).ravel()
    assert np.array_equal(shell, want)
    # perm: exactly the cells below the cutoff, ordered by (shell, q); offsets partitions it
    below = np.flatnonzero(want < cutoff)
    assert np.array_equal(perm, below[np.lexsort((below, want[below]))])
    assert offsets[0] == 0 and offsets[-1] == len(perm) and np.all(np.diff(offsets) >= 0)
    for k in range(cutoff):
        assert np.all(want[perm[offsets[k]:offsets[k + 1]]] == k)
    # a random float64 field summed through the plan against the torch spectrum in float64
    g = torch.Generator().manual_seed(h * 100 + w)
    vel = torch.randn((h, w, 2), generator=g, dtype=torch.float64)
    e = (torch.fft.fft2(vel[..., 1]).abs() ** 2 + torch.fft.fft2(vel[..., 0]).abs() ** 2).reshape(-1).numpy()
    got = np.array([0.5 / (h * w) ** 2 * e[perm[offsets[k]:offsets[k + 1]]].sum() for k in range(cutoff)])
    ref = EK_spectrum_2D_tf(vel).numpy()
    assert got.shape == ref.shape == (cutoff,)
    assert np.all(np.abs(got - ref) <= 1e-13 * np.abs(ref)), (got, ref)


def test_ties_go_to_the_even_shell():
    """9 x 8: radii of exactly 2.5 exist (e.g. p - centre = (1.5, 2)); torch.round sends them to shell 2, a round-half-up to 3."""
    from diffpiso.losses import spectrum_plan
    h, w = 9, 8
    plan = spectrum_plan(h, w, "cpu")
    shell = plan.shell.numpy().reshape(h, w)
    p0, p1 = (np.arange(h) - h // 2) % h, (np.arange(w) - w // 2) % w       # the shifted place of every unshifted index
    r2 = ((p0 - h / 2) ** 2)[:, None] + ((p1 - w / 2) ** 2)[None, :]
    ties = r2 == 6.25
    assert ties.sum() >= 4 and np.all(shell[ties] == 2)
    every_tie = np.sqrt(r2) % 1 == 0.5
    assert every_tie.sum() == 13 and np.all(shell[every_tie] % 2 == 0)
    assert int((np.floor(np.sqrt(r2[every_tie]) + 0.5) != shell[every_tie]).sum()) == 9


@pytest.mark.parametrize("name", ["sq", "rect"])
def test_plan_meets_the_references_spectra(name):
    """The reference's own spectra (tests/golden/spectral_loss.npz) through the plan: complex64 transforms, float64 shell sums; the bound of
    tests/test_spectral_golden.py, 2e-6 of the maximum."""
    from diffpiso.losses import spectrum_plan
    g = np.load(GOLD)
    vel = torch.tensor(g["spectrum_%s/velocity_centered" % name], dtype=torch.float32)
    want = g["spectrum_%s/E" % name]
    h, w = vel.shape[:2]
    plan = spectrum_plan(h, w, "cpu")
    perm, offsets = plan.perm.numpy(), plan.offsets.numpy()
    spec = torch.view_as_real(torch.fft.fft2(vel.permute(2, 0, 1).contiguous())).numpy().astype(np.float64).reshape(2, h * w, 2)
    e = (spec ** 2).sum(axis=(0, 2))
    got = np.array([0.5 / (h * w) ** 2 * e[perm[offsets[k]:offsets[k + 1]]].sum() for k in range(plan.cutoff)])
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()


def test_plan_cache_is_bounded():
    from diffpiso import losses as L
    for n in range(4, 4 + 2 * L._SPECTRUM_PLANS_MAX):
        L.spectrum_plan(n, 4, "cpu")
    assert len(L._spectrum_plans) <= L._SPECTRUM_PLANS_MAX
