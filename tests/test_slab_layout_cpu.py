"""The row map of the slab-decomposed step, three times over and without a GPU: the `piso_slab_t` comment of include/piso_hip.h restated in
numpy (tests/slab_emulation.py: SlabLayout), the library's RowMap (through piso_slab_sizes, a host function) and its Python twin
(diffpiso/sharding.py: StepSharding with a stub communicator) must say the same about every legal slab - and refuse the same slabs."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest
import torch

from diffpiso import _native as N
from tests.slab_emulation import INVALID_ARG, SlabLayout, emulate_exchange, legal_slabs, refused_slabs, slab_struct, whole_row_pointers, with_last


def _sizes(slab, nx, ny, per_x, per_y):
    out = (C.c_int * 8)(*([-7] * 8))
    return N.lib.piso_slab_sizes(C.byref(slab), nx, ny, per_x, per_y, out), list(out)


@pytest.mark.parametrize("ny", [10, 11, 12, 16, 33])
def test_slab_sizes_equal_the_header_for_every_legal_slab(ny):
    """All eight numbers, the stored nnz counted row by row from the closed-form row pointers of the whole grid around the ring."""
    nx = 5
    slabs = with_last(ny, legal_slabs(ny))
    assert len(slabs) >= 8
    for per_x, per_y in itertools.product((0, 1), (0, 1)):
        a, b = C.c_int(), C.c_int()
        N.lib.piso_csr_nnz(nx, ny, per_x, per_y, C.byref(a), C.byref(b))
        rp = whole_row_pointers(nx, ny, per_x, per_y)
        assert (a.value, b.value) == (rp[0][-1], rp[1][-1])
        for rb, re, last in slabs:
            L = SlabLayout(nx, ny, rb, re, last, per_x, per_y)
            st, got = _sizes(L.struct(), nx, ny, per_x, per_y)
            assert st == 0 and got == L.sizes8(), (rb, re, last, per_x, per_y, got, L.sizes8())


def test_slab_sizes_refuses_what_the_header_forbids():
    ny, nx = 16, 5
    for label, (nyg, rb, re, last) in refused_slabs(ny).items():
        st, got = _sizes(slab_struct(nyg, rb, re, last), nx, ny, 0, 0)
        assert st == INVALID_ARG and got == [-7] * 8, (label, st, got)
    # the last cell row without the duplicate face row is a legal slab (nobody writes v[ny] then); it stores what the last slab stores
    st0, got0 = _sizes(slab_struct(ny, ny - 4, ny, 0), nx, ny, 0, 0)
    st1, got1 = _sizes(slab_struct(ny, ny - 4, ny, 1), nx, ny, 0, 0)
    assert st0 == st1 == 0 and got0 == got1
    # the smallest and the largest legal slab
    assert _sizes(slab_struct(ny, 0, 4, 0), nx, ny, 0, 0)[0] == 0 and _sizes(slab_struct(ny, 6, 16, 1), nx, ny, 0, 0)[0] == 0
    assert _sizes(slab_struct(10, 3, 7, 0), nx, 10, 1, 1)[0] == 0


def _shardings(nx, ny, world):
    from diffpiso.sharding import StepSharding
    return [StepSharding(types.SimpleNamespace(world=world, rank=r, device=torch.device("cpu")), nx, ny) for r in range(world)]


@pytest.mark.parametrize("ny", [12, 24, 48, 64])
@pytest.mark.parametrize("world", [2, 3, 4, 6, 8])
def test_step_sharding_is_the_header_s_row_map(ny, world):
    nx = 7
    nyl = ny // world
    if ny % world != 0 or nyl < 4 or nyl + 6 > ny:
        with pytest.raises(ValueError):
            _shardings(nx, ny, world)
        return
    n_u_g, n_faces_g = (nx + 1) * ny, (nx + 1) * ny + nx * (ny + 1)
    seen_faces, seen_cells = np.zeros(n_faces_g, int), np.zeros(nx * ny, int)
    for r, sh in enumerate(_shardings(nx, ny, world)):
        j0, j1, last = r * nyl, (r + 1) * nyl, int(r == world - 1)
        L = SlabLayout(nx, ny, j0, j1, last)
        assert (sh.slab.ny_global, sh.slab.row_begin, sh.slab.row_end, sh.slab.owns_last_face_row) == (ny, j0, j1, last)
        assert (sh.cb, sh.cr, sh.vb, sh.vr) == (L.crows[0], L.crows.size, L.vrows[0], L.vrows.size)
        assert (sh.mb, sh.mr) == (L.mrows[0], L.mrows.size)
        assert (sh.n_u, sh.n_v, sh.n_cells, sh.n_pad) == (L.n_u_stored, L.n_v_stored, L.idx["cells"].size, L.idx["pad"].size)
        # every row of the grid: a stored row maps to its place, every other row falls outside the stored rows
        for rows, fn, stored in ((ny, sh.urow, L.crows), (ny + 1, sh.vrow, L.vrows)):
            for j in range(rows):
                at = np.nonzero(stored == j)[0]
                assert (at.tolist() == [fn(j)]) if at.size else (fn(j) >= stored.size), (r, j, fn(j), stored)
        # scatter_* cut the whole grid into the stored rows, owned_* pick the owned rows out of them
        faces = sh.scatter_faces(torch.arange(n_faces_g, dtype=torch.float64), device="cpu")
        assert faces.long().tolist() == L.idx["faces"].tolist()
        cells = sh.scatter_cells(torch.arange(nx * ny, dtype=torch.float64).reshape(ny, nx), dtype=torch.float64, device="cpu")
        assert cells.reshape(-1).long().tolist() == L.idx["cells"].tolist()
        mask = sh.scatter_mask(1.0 + torch.arange((nx + 2) * (ny + 2), dtype=torch.float64), dtype=torch.float64, device="cpu")
        assert (mask.long() - 1).tolist() == L.idx["mask"].tolist()                  # (rows behind the grid: zero-filled, "-1" here)
        u, v = sh.owned_faces(faces)
        assert u.reshape(-1).long().tolist() == list(range(j0 * (nx + 1), j1 * (nx + 1)))
        assert v.reshape(-1).long().tolist() == list(range(n_u_g + j0 * nx, n_u_g + (j1 + last) * nx))
        assert torch.cat([u.reshape(-1), v.reshape(-1)]).long().tolist() == L.idx["faces"][L.own["faces"]].tolist()
        own_c = sh.owned_cells(cells).reshape(-1).long().tolist()
        assert own_c == list(range(j0 * nx, j1 * nx)) == L.idx["cells"][L.own["cells"]].tolist()
        seen_faces[L.idx["faces"][L.own["faces"]]] += 1
        seen_cells[own_c] += 1
    assert (seen_faces == 1).all() and (seen_cells == 1).all()       # the ranks' owned rows tile the grid once, v[ny] from the last rank


@pytest.mark.parametrize("ny,world", [(12, 2), (24, 3), (24, 4), (48, 8), (64, 4)])
@pytest.mark.parametrize("per_y", [0, 1])
def test_message_tables_deliver_the_halo_rows_and_nothing_else(ny, world, per_y):
    """The four 28-int tables, run through the exchange on the host with every stored element numbered by the whole-grid element it
    should hold: afterwards the owned rows and two rows either side (with the duplicate row v[ny] across the seam) hold their own
    number, everything else is untouched."""
    nx, nyl = 5, ny // world
    shs = _shardings(nx, ny, world)
    Ls = [SlabLayout(nx, ny, r * nyl, (r + 1) * nyl, r == world - 1, 1, per_y) for r in range(world)]
    for sh, L in zip(shs, Ls):
        sh.set_pattern(None, torch.as_tensor(L.rp_local, dtype=torch.int32), L.nnz[0])
    for kind, table in (("faces", "msgs_faces"), ("faces_vfirst", "msgs_faces_vfirst"), ("cells", "msgs_cells"), ("csr", "msgs_csr")):
        arrays = [torch.where(torch.as_tensor(L.own[kind]), torch.as_tensor(L.idx[kind]), torch.tensor(-1)) for L in Ls]
        emulate_exchange([getattr(sh, table) for sh in shs], arrays)
        for r, (L, a) in enumerate(zip(Ls, arrays)):
            want = np.where(L.own[kind] | L.halo[kind], L.idx[kind], -1)
            assert a.tolist() == want.tolist(), (kind, r, np.nonzero(a.numpy() != want)[0][:8])
