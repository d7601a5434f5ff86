"""The launches of one sharded step, rank by rank in ONE process, with the halo exchange emulated on the host from the message tables of
diffpiso/sharding.py (tests/slab_emulation.py: emulate_exchange) - no communicator, no peer mapping, no subprocess.

`world` StepSharding objects are built with stub communicators.  Every buffer starts as NaN: an input holds the rank's OWNED rows
only, halo rows come from the emulated exchange and from nowhere else, outputs are pre-filled with one NaN pattern.  The chain is what
diffpiso/fused.py and diffpiso/piso.py run: pad velocity, the pattern-only assembly (once), assembly, exchange of the CSR values and
the diagonal, both CSR products, A0 v-first and its exchange, both Laplacians, divergence, the three face updates, their reverse mode
on exchanged cotangents, the divergence adjoint, the H contribution and its adjoint.  Asserted:
  * after every launch: the owned rows equal the whole-grid launch bit for bit, nothing else was written, nothing owned was left out -
    so a message table that delivers too little shows as NaN in an owned output;
  * after every exchange: the owned rows and two rows either side (plus the duplicate row v[ny] across the seam) hold the whole
    grid's data and every other stored element, guards included, still holds the pre-fill - so a table that writes anywhere else shows;
  * the padded rows piso_pad_velocity_slab fills are all the assembly of the owned rows reads (the others stay NaN here);
  * the owned rows of all ranks tile every whole-grid output exactly once, v[ny] coming from the last rank."""
import types

import numpy as np
import pytest
import torch

from tests import slab_emulation as E
from tests.cases import make_case
from tests.test_gpu_slab_twins import GEO, Inputs, case_modes, finish, setup_inputs

pytestmark = pytest.mark.gpu
CASES = ["periodic", "xper_ywall", "cavity", "spatial_ml"]
GRIDS = [(12, 9), (24, 20), (48, 33), (64, 129)]
WORLDS = [2, 3, 4, 6, 8]


def accepted(ny, world):
    return ny % world == 0 and ny // world >= 4 and ny // world + 6 <= ny


def whole_chain(W, f, c, visc, visc_is_field):
    per_y, per_x = [int(b) for b in c["periodic_yx"]]
    modes = case_modes(c)
    R = {}
    R["pad"] = E.op_pad_velocity(W, f["vel"], per_x, per_y)
    R["asm"] = E.op_assemble(W, R["pad"]["vel_pad"][1], f["dmask"], f["active"], visc, visc_is_field, f["no_slip"], GEO)
    val, rp, col, diag = [R["asm"][k][1] for k in ("val", "rowptr", "col", "diag")]
    R["mv"] = E.op_matvec(W, val, rp, col, f["x"], 0)
    R["mvT"] = E.op_matvec(W, val, rp, col, f["in2"], 1)
    R["a0"] = E.op_a0_vfirst(W, diag, GEO["beta"], 0.61)
    a0 = R["a0"]["a0"][1]
    R["lap32"] = E.op_laplace(W, torch.float32, f["active"], f["acc"], a0)
    R["lap64"] = E.op_laplace(W, torch.float64, f["active"], f["acc"], a0)
    R["div"] = E.op_divergence(W, f["in0"], GEO)
    R["fwd0"] = E.op_face_forward(W, 0, modes, GEO, f["p"], f["acc"], None, f["vel"], f["in1"], f["in2"], f["dmask"])
    R["fwd1"] = E.op_face_forward(W, 1, modes, GEO, f["p"], f["acc"], diag, f["in0"], None, None, None)
    R["fwd2"] = E.op_face_forward(W, 2, modes, GEO, f["p"], f["acc"], diag, f["in0"], f["in1"], None, None)
    R["bwd0"] = E.op_face_backward(W, 0, modes, GEO, f["acc"], None, f["dmask"], f["d0"], None, True, True)
    R["bwd1"] = E.op_face_backward(W, 1, modes, GEO, f["acc"], diag, None, f["d0"], f["d1"], False, False)
    R["bwd2"] = E.op_face_backward(W, 2, modes, GEO, f["acc"], diag, None, f["d0"], None, True, False)
    R["diva"] = E.op_divergence_adjoint(W, f["dc"], per_x, per_y, GEO)
    R["h"] = E.op_h_contribution(W, R["mv"]["y"][1], f["x"], diag, GEO["beta"])
    R["hadj"] = E.op_h_contribution_adjoint(W, f["d0"], f["d1"], diag, GEO["beta"])
    return R


def sharded_chain(tally, world, w, c, R, visc_w, visc_is_field):
    from diffpiso.sharding import StepSharding
    ny, nx = c["ny"], c["nx"]
    per_y, per_x = [int(b) for b in c["periodic_yx"]]
    modes = case_modes(c)
    nyl = ny // world
    dev = torch.device("cuda")
    shs = [StepSharding(types.SimpleNamespace(world=world, rank=r, device=dev), nx, ny) for r in range(world)]
    Ss = [E.Space(E.SlabLayout(nx, ny, r * nyl, (r + 1) * nyl, r == world - 1, per_x, per_y)) for r in range(world)]
    ranks = range(world)
    tag = "%d ranks" % world

    def owned(kind, name):
        return [S.put(kind, w[name][1], owned_only=True) for S in Ss]

    def const(name):
        """A constant of the simulation: sharding.sim_tensors / cached_scatter_* cut ALL stored rows."""
        return [S.put(w[name][0], w[name][1]) for S in Ss]

    def exchange(kind, table, gs, whole, what):
        E.emulate_exchange([getattr(sh, table) for sh in shs], [g.t for g in gs])
        for r, (S, g) in enumerate(zip(Ss, gs)):
            tally.add("%s, rank %d: %s after its %s exchange" % (tag, r, what, table), S.check(kind, g, whole, S.filled(kind)),
                      lambda S=S, g=g: S.explain(kind, g, whole, S.filled(kind)))
        return gs

    def launch(key, fn):
        outs = [fn(r, Ss[r]) for r in ranks]
        for r in ranks:
            tally.launch("%s, rank %d: %s" % (tag, r, key), Ss[r], outs[r], R[key])
        return outs
    dmask, active, acc, no_slip = const("dmask"), const("active"), const("acc"), const("no_slip")
    visc = const("visc") if visc_is_field else [visc_w] * world
    # 1. pad velocity (after the halo exchange of the velocity)
    vel = exchange("faces", "msgs_faces", owned("faces", "vel"), w["vel"][1], "velocity")
    pad = launch("pad", lambda r, S: E.op_pad_velocity(S, vel[r], per_x, per_y))
    # 2. the pattern of every stored row, once
    pat = [E.op_assemble(S, None, None, None, None, 0, None, GEO, pattern_only=1) for S in Ss]
    for r, (S, sh, o) in enumerate(zip(Ss, shs, pat)):
        all_csr, all_rp = [torch.ones(S.n(k), dtype=torch.bool, device=dev) for k in ("csr", "csr_rp")]
        tally.add("%s, rank %d: pattern" % (tag, r), S.check("csr", o["col"][1], R["asm"]["col"][1].t, all_csr) & S.check("csr_rp", o["rowptr"][1], None, all_rp))
        assert sh.sizes(per_x, per_y) == dict(nnz_u=S.L.nnz[0], nnz_v=S.L.nnz[1], mask_rows=S.L.mrows.size)
        sh.set_pattern(o["col"][1].t, o["rowptr"][1].t, S.L.nnz[0], per_xy=(per_x, per_y), nnz=S.L.nnz)
    # 3. assembly of the owned rows from the padded rows the rank filled itself (every other padded row is NaN)
    asm = [E.op_assemble(S, pad[r]["vel_pad"][1], dmask[r], active[r], visc[r], visc_is_field, no_slip[r], GEO, col=pat[r]["col"][1], rp=pat[r]["rowptr"][1])
           for r, S in enumerate(Ss)]
    for r, S in enumerate(Ss):
        tally.launch("%s, rank %d: assembly" % (tag, r), S, asm[r], R["asm"], skip=("col", "rowptr"))
        all_csr, all_rp = [torch.ones(S.n(k), dtype=torch.bool, device=dev) for k in ("csr", "csr_rp")]
        tally.add("%s, rank %d: the pattern after the assembly" % (tag, r),
                  S.check("csr", asm[r]["col"][1], R["asm"]["col"][1].t, all_csr) & S.check("csr_rp", asm[r]["rowptr"][1], None, all_rp))
    # 4. exchange of the CSR values and of the diagonal
    val = exchange("csr", "msgs_csr", [a["val"][1] for a in asm], R["asm"]["val"][1].t, "CSR values")
    diag = exchange("faces", "msgs_faces", [a["diag"][1] for a in asm], R["asm"]["diag"][1].t, "diagonal")
    rp, col = [p["rowptr"][1] for p in pat], [p["col"][1] for p in pat]
    # 5. both products
    x = exchange("faces", "msgs_faces", owned("faces", "x"), w["x"][1], "x")
    mv = launch("mv", lambda r, S: E.op_matvec(S, val[r], rp[r], col[r], x[r], 0))
    xt = exchange("faces", "msgs_faces", owned("faces", "in2"), w["in2"][1], "the product's cotangent")
    launch("mvT", lambda r, S: E.op_matvec(S, val[r], rp[r], col[r], xt[r], 1))
    # 6. / 7. A0 v-first and its exchange, 8. the Laplacians
    a0 = launch("a0", lambda r, S: E.op_a0_vfirst(S, diag[r], GEO["beta"], 0.61))
    a0 = exchange("faces_vfirst", "msgs_faces_vfirst", [o["a0"][1] for o in a0], R["a0"]["a0"][1].t, "A0")
    launch("lap32", lambda r, S: E.op_laplace(S, torch.float32, active[r], acc[r], a0[r]))
    launch("lap64", lambda r, S: E.op_laplace(S, torch.float64, active[r], acc[r], a0[r]))
    # 9. divergence
    in0 = exchange("faces", "msgs_faces", owned("faces", "in0"), w["in0"][1], "u*")
    launch("div", lambda r, S: E.op_divergence(S, in0[r], GEO))
    # 10. the face updates (element-wise inputs: owned rows only)
    p = exchange("cells", "msgs_cells", owned("cells", "p"), w["p"][1], "pressure")
    vel_o, in0_o, in1_o, in2_o = owned("faces", "vel"), owned("faces", "in0"), owned("faces", "in1"), owned("faces", "in2")
    launch("fwd0", lambda r, S: E.op_face_forward(S, 0, modes, GEO, p[r], acc[r], None, vel_o[r], in1_o[r], in2_o[r], dmask[r]))
    launch("fwd1", lambda r, S: E.op_face_forward(S, 1, modes, GEO, p[r], acc[r], diag[r], in0_o[r], None, None, None))
    launch("fwd2", lambda r, S: E.op_face_forward(S, 2, modes, GEO, p[r], acc[r], diag[r], in0_o[r], in1_o[r], None, None))
    # 11. incoming cotangents exchanged, 12. reverse mode of the face updates
    d0 = exchange("faces", "msgs_faces", owned("faces", "d0"), w["d0"][1], "d_out0")
    d1 = exchange("faces", "msgs_faces", owned("faces", "d1"), w["d1"][1], "d_out1")
    launch("bwd0", lambda r, S: E.op_face_backward(S, 0, modes, GEO, acc[r], None, dmask[r], d0[r], None, True, True))
    launch("bwd1", lambda r, S: E.op_face_backward(S, 1, modes, GEO, acc[r], diag[r], None, d0[r], d1[r], False, False))
    launch("bwd2", lambda r, S: E.op_face_backward(S, 2, modes, GEO, acc[r], diag[r], None, d0[r], None, True, False))
    # 13. divergence adjoint
    dc = exchange("cells", "msgs_cells", owned("cells", "dc"), w["dc"][1], "d_div")
    launch("diva", lambda r, S: E.op_divergence_adjoint(S, dc[r], per_x, per_y, GEO))
    # 14. H and its adjoint: element-wise on the rank's own product
    x_o, d0_o, d1_o = owned("faces", "x"), owned("faces", "d0"), owned("faces", "d1")
    launch("h", lambda r, S: E.op_h_contribution(S, mv[r]["y"][1], x_o[r], diag[r], GEO["beta"]))
    launch("hadj", lambda r, S: E.op_h_contribution_adjoint(S, d0_o[r], d1_o[r], diag[r], GEO["beta"]))
    # the owned rows tile every kind of whole-grid output once
    for kind, total in (("faces", w["vel"][1].numel()), ("faces_vfirst", w["vel"][1].numel()), ("cells", w["p"][1].numel()),
                        ("laplace", 5 * w["p"][1].numel()), ("csr", R["asm"]["val"][1].t.numel())):
        seen = np.zeros(total, int)
        for S in Ss:
            seen[S.L.idx[kind][S.L.own[kind]]] += 1
        assert (seen == 1).all(), (tag, kind)
    n_u_g = (nx + 1) * ny
    assert [bool(np.any(S.L.idx["faces"][S.L.own["faces"]] >= n_u_g + ny * nx)) for S in Ss] == [False] * (world - 1) + [True]
    for sh in shs:
        sh.close()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", GRIDS)
def test_sharded_chain_equals_the_whole_grid_chain(name, shape):
    ny, nx = shape
    worlds = [world for world in WORLDS if accepted(ny, world)]
    assert worlds and (ny != 12 or worlds == [2, 3])                # (12 rows: 2 x 6 is the largest legal slab, 3 x 4 the smallest)
    c = make_case(name, ny, nx, seed=4)
    per_y, per_x = [int(b) for b in c["periodic_yx"]]
    I = Inputs(nx, ny, 13)
    w = setup_inputs(c, I)
    w.update(dc=("cells", I.randn(I.nc)))
    visc_is_field = int(name == "spatial_ml")
    visc_w = E.Guarded(torch.full((1,), 1e-2).cuda(), 0, 1)
    W = E.Space(E.WholeLayout(nx, ny, per_x, per_y))
    f = {k: W.put(kind, v) for k, (kind, v) in w.items()}
    tally = E.Tally()
    R = whole_chain(W, f, c, f["visc"] if visc_is_field else visc_w, visc_is_field)
    for k, o in R.items():
        tally.launch("whole grid %s" % k, W, o, None)
    # the reference of everything below is itself held to the oracle where the chain's own data reaches a kernel nothing else feeds:
    # the Laplacian of the A0 this chain computed (a twin and a kernel that are wrong alike agree with each other)
    from oracle import native as O
    a0_host = R["a0"]["a0"][1].t.cpu().numpy()
    for key, dtype in (("lap64", np.float64), ("lap32", np.float32)):
        np.testing.assert_array_equal(R[key]["laplace"][1].t.cpu().numpy(), O.laplace_matrix(nx, ny, c["active"], c["accessible"], a0_host, dtype))
    for world in worlds:
        sharded_chain(tally, world, w, c, R, visc_w, visc_is_field)
    finish(tally)
