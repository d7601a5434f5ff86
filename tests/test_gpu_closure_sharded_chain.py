"""The CNN closure of a sharded step, rank by rank in ONE process: stub communicators, the wide halo exchanges emulated on the host from
the message tables of diffpiso/sharding.py (ClosureHalo; tests/slab_emulation.py: emulate_exchange), every buffer NaN to begin with.

Forward, per rank: piso_closure_input_slab on the halo-filled velocity / pressure -> the emulated forward exchange -> the network on the
extended rows (the product's MFMA convolutions, wrap = (False, wrap_x)) -> piso_closure_force_slab.  Reverse: the faces' cotangent through
the emulated `msgs_faces` exchange -> piso_closure_force_adjoint_slab -> the convolutions' backward -> the emulated reverse exchange + the
adds -> the emulated one-row exchange -> piso_closure_input_adjoint_slab.  Asserted:
  * after the forward exchange the owned plus halo rows hold the whole grid's network input bit for bit and every other element (the
    scratch rows of a rank with both neighbours, the guard bands) holds the pre-fill;
  * the forcing on every rank's owned faces is the whole-grid `make_forcing_fn` output bit for bit (which takes in the network output on
    the owned rows and the row across each cut), nothing else is written, and the owned rows of all ranks tile the whole grid once;
  * dL/du, dL/dp on the owned rows and the rank-summed weight gradients against a float64 torch evaluation of the whole-grid closure: the
    sharded float32 error is at most TWICE the one-GPU float32 error against the same float64 result (rel-L2 per quantity; the margin is
    the one extra rounding where two ranks' partial input gradients are added across a cut)."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import slab_emulation as E
from tests.cases import make_case
from tests.test_gpu_closure_glue_twins import flat_faces, op_force, op_force_adjoint, op_input_adjoint, same_bits, torch_fields
from tests.test_gpu_closure_glue_twins import network_input64
from tests.test_gpu_slab_twins import Inputs, case_modes

pytestmark = pytest.mark.gpu
CASES = ["periodic", "xper_ywall", "cavity", "spatial_ml"]
SEVEN, TWO = None, [(3, 4, 8), (3, 8, 2)]
SETUPS = [("seven layers 48 x 48", SEVEN, 48, 48, (2, 3, 4)), ("seven layers 40 x 96", SEVEN, 40, 96, (2, 3, 4, 6, 8)),
          ("two layers 24 x 24", TWO, 24, 24, (2, 3, 4, 6))]
RATIOS = []


class RankExt(object):
    """A rank's Space plus the NHWC geometry the product's ClosureHalo gives it (lo, hi): what the op_* helpers of the twin tests take."""

    def __init__(self, S, H):
        self.S, self.lo, self.hi = S, H.lo, H.hi

    def call(self, name, *args):
        from diffpiso import _native as N
        st = getattr(N.lib, name + "_slab")(*(args + (self.S.slab_ptr, self.lo, self.hi)))
        assert st == 0, "%s_slab returned %d: %s" % (name, st, N.lib.piso_last_error_string().decode())


def nhwc_kinds(S, H, sh, ny):
    """Layout kinds of a rank's NHWC buffers INCLUDING the scratch rows: nhwc<ch> for the op_* outputs (extended rows only) and
    buf<ch> = extended rows + 2 E scratch rows (whole-grid index -1 on the scratch rows)."""
    rows = (sh.j0 - H.lo + np.arange(H.rows)) % ny
    pos = np.arange(H.rows)
    owned = (pos >= H.lo) & (pos < H.lo + sh.nyl)
    for ch in (2, 4):
        w = sh.nx * ch
        idx = (rows[:, None] * w + np.arange(w)[None, :]).astype(np.int64).ravel()
        S.L.idx["nhwc%d" % ch], S.L.own["nhwc%d" % ch] = idx, np.repeat(owned, w)
        S.L.idx["buf%d" % ch] = np.concatenate([idx, np.full(2 * H.E * w, -1, np.int64)])
        S.L.own["buf%d" % ch] = np.concatenate([np.repeat(owned, w), np.zeros(2 * H.E * w, bool)])


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def reference_runs(c, net, wrap, vel, p, g_st):
    """(forcing, dL/du flat, dL/dp, weight gradients) of the whole-grid closure: float32 on the GPU through make_forcing_fn (the product's
    one-GPU path), and float64 on the host with torch's convolution."""
    import diffpiso as dp
    two_dx = 2 * float(np.mean(c["dx_yx"]))
    net.zero_grad()
    vel_t, p_t, velocity, pressure = torch_fields(c, vel, p, two_dx, grad=True)
    F32 = dp.make_forcing_fn(net, True, wrap=wrap)(0, velocity, pressure)
    F32.backward(g_st)
    one = (F32.detach(), flat_faces(vel_t.grad), p_t.grad.reshape(-1), [w.grad.clone() for w in net.weights])
    net64 = copy.deepcopy(net).double().cpu()
    net64.zero_grad()
    v64, p64, nn64 = network_input64(c, vel.cpu(), p.cpu(), two_dx, 4)
    dp.centered_to_staggered(net64(nn64), wrap).backward(g_st.double().cpu())
    ref = (None, flat_faces(v64.grad), p64.grad.reshape(-1), [w.grad.clone() for w in net64.weights])
    net.zero_grad()
    return one, ref


def sharded_run(tally, tag, world, c, net, wrap, w, nn_in_whole, one):
    """-> (dL/du flat whole grid, dL/dp whole grid) gathered from the ranks' owned rows; the weight gradients accumulate in net.weights."""
    from diffpiso import _native as N
    from diffpiso.sharding import StepSharding, check_slab_network
    ny, nx = c["ny"], c["nx"]
    per_y, per_x = [int(b) for b in c["periodic_yx"]]
    modes, two_dx = case_modes(c), 2 * float(np.mean(c["dx_yx"]))
    nyl, dev = ny // world, torch.device("cuda")
    R = check_slab_network(net)
    # (a row_capacity of three NHWC rows and a bit: the wide exchanges of the seven layers travel in four messages each)
    shs = [StepSharding(types.SimpleNamespace(world=world, rank=r, device=dev, row_capacity=3 * nx * 4 + 5), nx, ny) for r in range(world)]
    H4 = [sh.closure_halo(R, 4, wrap[0]) for sh in shs]
    Ss = [E.Space(E.SlabLayout(nx, ny, r * nyl, (r + 1) * nyl, r == world - 1, per_x, per_y)) for r in range(world)]
    Xs = [RankExt(S, H) for S, H in zip(Ss, H4)]
    for S, H, sh in zip(Ss, H4, shs):
        nhwc_kinds(S, H, sh, ny)
    ranks = range(world)

    def exchange(kind, tables_of, gs):
        for chunk in range(len(tables_of(0))):
            E.emulate_exchange([tables_of(r)[chunk] for r in ranks], [g.t for g in gs])

    def faces_exchange(name):
        gs = [S.put("faces", w[name], owned_only=True) for S in Ss]
        E.emulate_exchange([sh.msgs_faces for sh in shs], [g.t for g in gs])
        return gs
    # ---- forward
    vel = faces_exchange("vel")
    p = [S.put("cells", w["p"], owned_only=True) for S in Ss]
    E.emulate_exchange([sh.msgs_cells for sh in shs], [g.t for g in p])
    bufs = []
    for r in ranks:
        b = Ss[r].out("buf4")
        st = N.lib.piso_closure_input_slab(E.ptr(vel[r]), E.ptr(p[r]), E.ptr(b), nx, ny, 4, E.pad_modes_c(modes), C.c_double(two_dx), E._stream(),
                                           Ss[r].slab_ptr, H4[r].lo, H4[r].hi)
        assert st == 0, N.lib.piso_last_error_string().decode()
        tally.add("%s rank %d: network input, owned rows" % (tag, r), Ss[r].check("buf4", b, nn_in_whole), lambda S=Ss[r], b=b: S.explain("buf4", b, nn_in_whole))
        bufs.append(b)
    exchange("buf4", lambda r: H4[r].tables_forward, bufs)
    for r in ranks:
        H = H4[r]
        filled = torch.zeros(H.numel, dtype=torch.bool, device=dev)
        filled[:H.rows * H.L] = True                                   # every extended row: owned + halo
        ok = Ss[r].check("buf4", bufs[r], nn_in_whole, filled) if H.lo and H.hi else None
        if ok is None:                                                 # a rank at a border: the ring's wrap rows landed in its scratch rows, and only there
            ext = bufs[r].t[:H.rows * H.L]
            ok = same_bits(ext, nn_in_whole.reshape(-1)[Ss[r].idx("buf4")[:H.rows * H.L]])
            fill = E._int_view(E._filled(1, torch.float32, dev))
            ok = ok & (E._int_view(bufs[r].buf[:Ss[r].band]) == fill).all() & (E._int_view(bufs[r].buf[Ss[r].band + H.numel:]) == fill).all()
            for have, a in ((H.lo, H.rows), (H.hi, H.rows + H.E)):
                if have:
                    ok = ok & (E._int_view(bufs[r].t[a * H.L:(a + H.E) * H.L]) == fill).all()
        tally.add("%s rank %d: network input after the wide exchange" % (tag, r), ok)
    forcing, outs, ins = [], [], []
    for r in ranks:
        x = H4[r].extended(bufs[r].t).clone().requires_grad_(True)
        y = net(x, wrap=(False, wrap[1]))
        ins.append(x)
        outs.append(y)
        g = Ss[r].put("nhwc2", torch.zeros(ny * nx * 2, device=dev))    # (a Guarded holder of the right size for the rank's output)
        g.t.copy_(y.detach().reshape(-1))
        o = op_force(Xs[r], g, wrap)
        tally.launch("%s rank %d: forcing == the whole grid's make_forcing_fn" % (tag, r), Ss[r], o, {"faces": ("faces", E.Guarded(one[0], 0, one[0].numel()))})
        forcing.append(o)
    seen = np.zeros(w["vel"].numel(), int)
    for S in Ss:
        seen[S.L.idx["faces"][S.L.own["faces"]]] += 1
    assert (seen == 1).all(), tag
    # ---- reverse
    dF = faces_exchange("dF")
    du = torch.full((w["vel"].numel(),), float("nan"), device=dev)
    dpw = torch.full((ny * nx,), float("nan"), device=dev)
    dbufs = []
    for r in ranks:
        a = op_force_adjoint(Xs[r], dF[r], wrap)
        d_out = a["d_nn_out"][1].t.clone()
        own = Ss[r].own("nhwc2")
        d_out[~own] = 0.0                                              # (the product allocates zeros; the launch writes the owned rows)
        tally.add("%s rank %d: force adjoint writes the owned rows only" % (tag, r), Ss[r].check("nhwc2", a["d_nn_out"][1], None))
        outs[r].backward(d_out.view_as(outs[r]))
        b = Ss[r].out("buf4")
        b.t[:H4[r].rows * H4[r].L] = ins[r].grad.reshape(-1)
        dbufs.append(b)
    exchange("buf4", lambda r: H4[r].tables_reverse, dbufs)
    for r in ranks:
        H4[r].add_received(dbufs[r].t)
    exchange("buf4", lambda r: H4[r].tables_narrow, dbufs)
    for r in ranks:
        a = op_input_adjoint(Xs[r], dbufs[r], 4, modes, two_dx)
        for kind, key, whole in (("faces", "d_faces", du), ("cells", "d_p", dpw)):
            g = a[key][1]
            tally.add("%s rank %d: %s written on the owned rows only" % (tag, r, key), Ss[r].check(kind, g, None))
            own = Ss[r].own(kind)
            whole[Ss[r].idx(kind)[own]] = g.t[own]
    for sh in shs:
        sh.close()
    return du, dpw


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("setup", SETUPS, ids=[s[0].replace(" ", "_") for s in SETUPS])
def test_sharded_closure_chain_equals_the_whole_grid_closure(name, setup):
    import diffpiso as dp
    label, layers, nx, ny, worlds = setup
    c = make_case(name, ny, nx, seed=6)
    wrap = tuple(bool(b) for b in c["periodic_yx"])
    torch.manual_seed(0)
    net = dp.FullyConvNetwork(seed=4, wrap=wrap, layers=layers).cuda()
    I = Inputs(nx, ny, 23)
    vel, p = torch.as_tensor(c["vel"]).cuda(), torch.as_tensor(c["p"]).cuda()
    g_st = torch.zeros((1, ny + 1, nx + 1, 2), device="cuda")
    g_st[:, :, :nx, 0], g_st[:, :ny, :, 1] = I.randn((ny + 1) * nx).reshape(1, ny + 1, nx), I.randn(ny * (nx + 1)).reshape(1, ny, nx + 1)
    one, ref = reference_runs(c, net, wrap, vel, p, g_st)
    w = dict(vel=flat_faces(vel), p=p.reshape(-1).contiguous(), dF=flat_faces(g_st))
    _, _, velocity, pressure = torch_fields(c, vel, p, 2 * float(np.mean(c["dx_yx"])))
    nn_in_whole = dp.network_input(velocity, pressure, True).reshape(-1).contiguous()
    one = (flat_faces(one[0]),) + one[1:]
    e_one = [rel(one[1], ref[1]), rel(one[2], ref[2]), rel(torch.cat([g.reshape(-1) for g in one[3]]), torch.cat([g.reshape(-1) for g in ref[3]]))]
    tally = E.Tally()
    bad = []
    for world in worlds:
        tag = "%s %s, %d ranks" % (name, label, world)
        net.zero_grad()
        du, dpw = sharded_run(tally, tag, world, c, net, wrap, w, nn_in_whole, one)
        assert not torch.isnan(du).any() and not torch.isnan(dpw).any(), "%s: owned rows missing from the gathered gradients" % tag
        e_sh = [rel(du, ref[1]), rel(dpw, ref[2]), rel(torch.cat([wt.grad.reshape(-1) for wt in net.weights]), torch.cat([g.reshape(-1) for g in ref[3]]))]
        for what, a, b in zip(("dL/du", "dL/dp", "weight gradients"), e_sh, e_one):
            ratio = a / b
            RATIOS.append(ratio)
            print("%s %s: sharded vs float64 %.3e, one GPU vs float64 %.3e, ratio %.3f (largest so far %.3f)" % (tag, what, a, b, ratio, max(RATIOS)))
            if not a <= 2 * b:
                bad.append((tag, what, a, b))
    failures = tally.failures()
    assert len(tally) > 0 and not failures, "%d checks; first failures: %s" % (len(tally), failures)
    assert not bad, bad
