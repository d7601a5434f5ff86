"""The host side of the CNN closure on y-slabs (diffpiso/sharding.py: ClosureHalo, make_slab_forcing_fn; FullyConvNetwork.forward(wrap=)),
without a GPU.

The message tables are held to a numpy statement of the row map written here from the text of the issue, not from sharding.py:
  R = the network's reduced_buffer_width, E = R + 1.  Rank r of `world` owns rows [j0, j1) = [r nyl, (r + 1) nyl).  Its NHWC buffer holds the
  EXTENDED rows [j0 - lo, j1 + hi) in order, lo / hi = E on a side with a ring neighbour (y periodic: every side), 0 at a border, and
  behind them 2 E scratch rows.
  forward  - afterwards halo row k holds its whole-grid row: the neighbour's edge row.  Nothing else inside the extended rows is written; a rank
             at a border receives the ring's wrap rows in its scratch rows (the exchange is always a ring with full messages).
  reverse  - scratch rows [0, E) hold the lower neighbour's upper halo rows = partial sums for MY rows [j0, j0 + E); scratch rows [E, 2 E) the
             upper neighbour's lower halo rows = partial sums for my rows [j1 - E, j1).  The extended rows are not written.
  narrow   - forward with one row.
The emulation of the wire is tests/slab_emulation.py's emulate_exchange (every message read before any is written)."""
import types

import numpy as np
import pytest
import torch

import diffpiso as dp
from diffpiso.sharding import StepSharding, check_slab_network, make_slab_forcing_fn
from tests import slab_emulation as E_

NYS, WORLDS, RS = (24, 48, 96), (2, 3, 4, 6, 8), (2, 10)
NX, CH = 5, 4
UNWRITTEN = -7.0


def accepted(ny, world, R):
    nyl = ny // world
    return ny % world == 0 and nyl >= 4 and nyl + 6 <= ny and nyl >= R + 1


COMBOS = [(ny, world, R) for ny in NYS for world in WORLDS for R in RS if accepted(ny, world, R)]


def halos(ny, world, R, per_y, cap=8192, nx=NX, ch=CH):
    shs = [StepSharding(types.SimpleNamespace(world=world, rank=r, device="cpu", row_capacity=cap), nx, ny) for r in range(world)]
    return shs, [sh.closure_halo(R, ch, per_y) for sh in shs]


def extent(r, world, nyl, Eh, per_y):
    return (Eh if (r > 0 or per_y) else 0), (Eh if (r < world - 1 or per_y) else 0)


def coded(rows, rank=0, kind=0):
    """[rows][NX][CH] whose every element names (kind, rank, row, column, channel): nothing can arrive in the wrong place unnoticed."""
    r = np.asarray(rows, np.float64)[:, None, None]
    return (kind * 4000000 + rank * 400000 + r * 1000 + np.arange(NX)[None, :, None] * 10 + np.arange(CH)[None, None, :]).astype(np.float32)


def test_the_grid_of_combinations_is_what_the_issue_lists():
    # R = 2: 24 / {2,3,4,6}, 48 / {2,3,4,6,8}, 96 / {2,3,4,6,8}; R = 10: 24 / 2, 48 / {2,3,4}, 96 / {2,3,4,6,8}
    assert len(COMBOS) == 14 + 9 and (24, 2, 10) in COMBOS and (24, 3, 10) not in COMBOS and (96, 8, 10) in COMBOS and (24, 6, 2) in COMBOS
    assert (24, 8, 2) not in COMBOS                                   # three rows per slab: the step itself refuses


@pytest.mark.parametrize("per_y", [False, True])
@pytest.mark.parametrize("ny,world,R", COMBOS)
def test_forward_and_narrow_tables_deliver_the_whole_grid_rows_and_nothing_else(ny, world, R, per_y):
    Eh, nyl, L = R + 1, ny // world, NX * CH
    shs, Hs = halos(ny, world, R, per_y)
    for tables, w in (("tables_forward", Eh), ("tables_narrow", 1)):
        bufs = []
        for r, H in enumerate(Hs):
            lo, hi = extent(r, world, nyl, Eh, per_y)
            assert (H.E, H.lo, H.hi, H.rows, H.L, H.numel) == (Eh, lo, hi, nyl + lo + hi, L, (nyl + lo + hi + 2 * Eh) * L)
            b = np.full((H.rows + 2 * Eh, NX, CH), UNWRITTEN, np.float32)
            b[lo:lo + nyl] = coded(np.arange(r * nyl, (r + 1) * nyl))                 # owned rows: the whole grid's
            bufs.append(torch.from_numpy(b.reshape(-1)))
        for c in range(len(getattr(Hs[0], tables))):
            E_.emulate_exchange([getattr(H, tables)[c] for H in Hs], bufs)
        for r, H in enumerate(Hs):
            lo, hi = extent(r, world, nyl, Eh, per_y)
            got = bufs[r].numpy().reshape(H.rows + 2 * Eh, NX, CH)
            want = np.full((H.rows, NX, CH), UNWRITTEN, np.float32)
            want[lo:lo + nyl] = coded(np.arange(r * nyl, (r + 1) * nyl))
            if lo:
                want[lo - w:lo] = coded((r * nyl - w + np.arange(w)) % ny)
            if hi:
                want[lo + nyl:lo + nyl + w] = coded(((r + 1) * nyl + np.arange(w)) % ny)
            np.testing.assert_array_equal(got[:H.rows], want, err_msg="rank %d %s" % (r, tables))
            # the scratch rows: untouched where the rank has both neighbours' halos, the ring's wrap rows at a border
            scratch = got[H.rows:]
            if lo:
                assert (scratch[:Eh] == UNWRITTEN).all()
            if hi:
                assert (scratch[Eh:] == UNWRITTEN).all()


@pytest.mark.parametrize("per_y", [False, True])
@pytest.mark.parametrize("ny,world,R", COMBOS)
def test_reverse_tables_bring_the_halo_rows_to_their_owners_scratch(ny, world, R, per_y):
    Eh, nyl = R + 1, ny // world
    shs, Hs = halos(ny, world, R, per_y)
    bufs, before = [], []
    for r, H in enumerate(Hs):
        lo, hi = extent(r, world, nyl, Eh, per_y)
        rows = (r * nyl - lo + np.arange(H.rows)) % ny
        b = np.full((H.rows + 2 * Eh, NX, CH), UNWRITTEN, np.float32)
        b[:H.rows] = coded(rows, rank=r, kind=1)                                       # this rank's partial sums, named by rank and whole-grid row
        before.append(b.copy())
        bufs.append(torch.from_numpy(b.reshape(-1)))
    for c in range(len(Hs[0].tables_reverse)):
        E_.emulate_exchange([H.tables_reverse[c] for H in Hs], bufs)
    for r, H in enumerate(Hs):
        lo, hi = extent(r, world, nyl, Eh, per_y)
        got = bufs[r].numpy().reshape(H.rows + 2 * Eh, NX, CH)
        np.testing.assert_array_equal(got[:H.rows], before[r][:H.rows])                # the extended rows are not written
        lower, upper = (r - 1) % world, (r + 1) % world
        if lo:        # my rows [j0, j0 + E) as the lower neighbour's upper halo holds them
            np.testing.assert_array_equal(got[H.rows:H.rows + Eh], coded(r * nyl + np.arange(Eh), rank=lower, kind=1))
        if hi:
            np.testing.assert_array_equal(got[H.rows + Eh:], coded((r + 1) * nyl - Eh + np.arange(Eh), rank=upper, kind=1))


@pytest.mark.parametrize("ny,world,R", COMBOS)
def test_no_message_is_longer_than_the_row_capacity_and_the_chunks_tile_the_halo(ny, world, R):
    """At the default capacity (8192 elements) one message holds every row of these small grids; at nx = 1024 with 4 channels a row is 4096
    elements (16 KB) and a message holds two; a capacity of one row gives E messages; less than one row is refused."""
    Eh = R + 1
    for nx, ch, cap, per_msg in ((NX, CH, 8192, Eh), (1024, 4, 8192, 2), (NX, CH, NX * CH, 1), (NX, CH, 3 * NX * CH + 7, 3)):
        shs, Hs = halos(ny, world, R, True, cap=cap, nx=nx, ch=ch)
        L = nx * ch
        for H in Hs:
            for tables, w in ((H.tables_forward, Eh), (H.tables_reverse, Eh), (H.tables_narrow, 1)):
                assert len(tables) == -(-w // min(per_msg, w))
                seen = {k: [] for k in E_.MESSAGE_ORDER}
                for t in tables:
                    for key, segs in E_.message_segments(t).items():
                        assert len(segs) == 1 and segs[0][1] % L == 0 and 0 < segs[0][1] <= cap, (key, segs)
                        assert segs[0][0] % L == 0 and segs[0][0] + segs[0][1] <= H.numel
                        seen[key] += list(range(segs[0][0] // L, (segs[0][0] + segs[0][1]) // L))
                for key, rows in seen.items():                                          # w consecutive rows, each once
                    assert rows == list(range(rows[0], rows[0] + w)), (key, rows)
    with pytest.raises(ValueError, match="row_capacity"):
        halos(ny, world, R, True, cap=NX * CH - 1)


def test_refusals_name_their_rule():
    with pytest.raises(ValueError, match=r"E = R \+ 1 = 11 rows.*ny = 40 on 4 ranks gives 10"):
        halos(40, 4, 10, False)
    sh = StepSharding(types.SimpleNamespace(world=2, rank=0, device="cpu"), 8, 48)
    with pytest.raises(ValueError, match="padding must be 'SAME'"):
        make_slab_forcing_fn(dp.FullyConvNetwork([[0, 0], [0, 0]], padding="VALID", restore_shape=True, seed=1), sh)
    with pytest.raises(ValueError, match="y entries of buffer_width must be 0"):
        make_slab_forcing_fn(dp.FullyConvNetwork([[1, 0], [0, 0]], seed=1), sh)
    with pytest.raises(ValueError, match="reduced_buffer_width"):
        make_slab_forcing_fn(lambda x: x, sh)
    with pytest.raises(ValueError, match="wrap y together"):
        make_slab_forcing_fn(dp.FullyConvNetwork(seed=1, wrap=(True, False)), sh, wrap=(False, False))
    assert check_slab_network(dp.FullyConvNetwork([[0, 0], [2, 3]], seed=1)) == 3 + 2 + 2 + 1 + 1     # an x buffer is local: allowed
    make_slab_forcing_fn(dp.FullyConvNetwork([[0, 0], [2, 3]], seed=1), sh)
    with pytest.raises(ValueError, match="SlabStaggered"):                                  # whole-grid fields are not this function's
        c = dp.Domain([48, 8], boundaries=dp.OPEN)
        make_slab_forcing_fn(dp.FullyConvNetwork(seed=1), sh)(0, c.staggered_grid(0.0), c.centered_grid(0.0))


def _integer_network(layers, wrap, seed):
    """Weights and (below) inputs are small integers, the weights of every layer but the last multiples of 5: every pre-activation is then
    an integer multiple of 5 below 2^24, float32 sums of them are exact in ANY order, and 0.2f x (5 m) rounds to m exactly (0.2f = 0.2 (1 + 1.5e-8),
    under half an ulp) - so torch's host convolution, whose summation order depends on the image's shape, gives the same bits on both images."""
    net = dp.FullyConvNetwork(seed=seed, wrap=wrap, layers=layers)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, w in enumerate(net.weights):
            w.copy_(torch.randint(-2, 3, w.shape, generator=g).float() * (5.0 if n < len(net.weights) - 1 else 1.0))
    return net


@pytest.mark.parametrize("wrap_x", [False, True])
@pytest.mark.parametrize("layers", [[(3, 4, 8), (3, 8, 2)], [(5, 2, 4), (3, 4, 4), (1, 4, 2)]])
def test_forward_with_wrap_false_on_a_circularly_extended_input_is_the_wrapped_network(layers, wrap_x):
    net = _integer_network(layers, (True, wrap_x), 3)
    R = net.reduced_buffer_width
    x = torch.randint(-3, 4, (1, 13, 9, layers[0][1]), generator=torch.Generator().manual_seed(5)).float()
    with torch.no_grad():
        whole = net(x)                                                                  # wrap=None: the network's own
        assert torch.equal(whole, net(x, wrap=(True, wrap_x)))
        for ext in (R, R + 1):
            xe = torch.cat([x[:, -ext:], x, x[:, :ext]], dim=1)
            part = net(xe, wrap=(False, wrap_x))
            assert part.shape[1] == 13 + 2 * ext
            assert torch.equal(part[:, ext:-ext], whole)
            if ext > R:                                                                  # rows beyond R from an artificial end are right as well
                assert torch.equal(part[:, R:ext], whole[:, -(ext - R):]) and torch.equal(part[:, -ext:-R], whole[:, :ext - R])
        assert float(whole.abs().max()) > 0 and float(whole.abs().max()) < 2 ** 24
        assert not torch.equal(net(x, wrap=(False, wrap_x)), whole)                     # (the keyword does something)
