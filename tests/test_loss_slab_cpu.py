"""Host side of the losses on flat face vectors, no GPU: the window arithmetic of `losses.loss_window` (buffer_width, sponge_start ->
y0, y1, x0, x1) and the owned-rows crop of the multistep loss against slicing a numpy index grid, and the new entry points - declared in
include/piso_hip.h, exported from the library, bound with the header's argument counts."""
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["piso_loss_l2", "piso_loss_l2_grad", "piso_loss_strain", "piso_loss_strain_grad"]


def test_loss_window_is_the_slicing_of_the_torch_loss():
    from diffpiso.losses import loss_window
    checked = 0
    for ny, nx in ((10, 12), (13, 9), (4, 5)):
        grid = np.arange((ny + 1) * (nx + 1)).reshape(ny + 1, nx + 1)
        assert loss_window(None, 0, ny, nx) == (0, ny + 1, 0, nx + 1) and loss_window(None, 7, ny, nx) == (0, ny + 1, 0, nx + 1)
        widths = (0, 1, 2, 3, ny - 4, ny + 3)
        for a, b, c, d in itertools.product(widths, widths, (0, 2, 3), (0, 1, nx + 2)):
            for sponge in (0, 7, nx + 1, nx + 5, 2):
                bw = [[a, b], [c, d]]
                # losses.py: data[:, bw[0][0]:rows - bw[0][1], bw[1][0]:sponge_start - bw[1][1]], sponge_start 0 = the tensor's width
                want = grid[slice(a, grid.shape[0] - b), slice(c, (sponge if sponge != 0 else grid.shape[1]) - d)]
                y0, y1, x0, x1 = loss_window(bw, sponge, ny, nx)
                assert 0 <= y0 <= y1 <= ny + 1 and 0 <= x0 <= x1 <= nx + 1, (bw, sponge)
                got = grid[y0:y1, x0:x1]
                assert got.size == want.size and np.array_equal(got.ravel(), want.ravel()), (ny, nx, bw, sponge, (y0, y1, x0, x1))
                checked += 1
    assert checked > 1000
    # the windows of the GPU tests: two-sided, sponge, one row
    assert loss_window([[1, 2], [2, 1]], 0, 10, 12) == (1, 9, 2, 12)
    assert loss_window([[0, 0], [3, 0]], 7, 10, 12) == (0, 11, 3, 7)
    assert loss_window([[4, 6], [1, 1]], 0, 10, 12) == (4, 5, 1, 12)


def test_owned_crop_is_the_window_cut_to_the_owned_rows():
    from diffpiso.losses import _owned_crop
    for rows in (12, 13):
        whole = np.arange(rows)
        for a, b in itertools.product((0, 1, 3, 5, rows), (0, 2, 6, rows + 1)):
            sl = slice(a, rows - b)
            for first, count in ((0, 4), (4, 4), (8, rows - 8), (0, rows), (3, 5)):
                owned = whole[first:first + count]
                want = [j for j in whole[sl] if first <= j < first + count]
                assert list(owned[_owned_crop(rows, sl, first, count)]) == want, (rows, a, b, first, count)


def test_loss_entries_are_declared_exported_and_bound():
    from diffpiso import _native as N
    header = open(os.path.join(ROOT, "include", "piso_hip.h")).read()
    assert re.search(r"size_t\s+piso_loss_workspace_bytes\(void\);", header) and N.lib.piso_loss_workspace_bytes() >= 2048 * 8
    for stem in ENTRIES:
        for name in (stem, stem + "_slab"):
            m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
            assert m, "%s is not declared in include/piso_hip.h" % name
            fn = getattr(N.lib, name)                        # (AttributeError: the library does not export it)
            assert len(fn.argtypes) == len(m.group(1).split(",")), (name, len(fn.argtypes), m.group(1))
        assert "const piso_slab_t* slab" in re.search(r"\bint\s+%s_slab\(([^;]*)\);" % stem, header).group(1)
    for phrase in ("piso_loss_l2:", "piso_loss_strain:", "INTERIOR grid corners", "y0 <= j < y1 and x0 <= i < x1"):
        assert phrase in header, phrase
