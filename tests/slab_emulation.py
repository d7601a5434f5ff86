"""One rank's rows of a grid cut into y-slabs, restated from the `piso_slab_t` comment of include/piso_hip.h - helpers of the tests
that hold every `*_slab` entry point to its whole-grid entry point (no test in here).

`SlabLayout` is plain numpy and is written from the header's TEXT: it imports neither `diffpiso.sharding` nor anything of
csrc/piso_common.h, so that the row map exists a third time, independently of the two that ship.  For every kind of array it gives,
per STORED element, the whole-grid flat index that element holds (-1: no such element - the padded mask row behind the grid of a
last slab) and whether a launch of the rank WRITES it:

  cells          [stored cell rows][nx]                        faces          stored u rows, then stored v rows (u-first)
  faces_vfirst   stored v rows, then stored u rows             mask           stored rows of a padded [ny + 2][nx + 2] cell mask
  pad            stored padded u rows, then padded v rows      laplace        the OWNED cell rows [rows][nx][5]
  csr            entries of the stored u rows, then v rows     csr_rp         local row pointers [stored u faces + 1][stored v faces + 1]

`Space` puts a layout (or the whole grid: `WholeLayout`) on the device.  Every array it hands out lies inside a larger buffer with a
guard band either side; inputs and their guards are NaN (integers: a sentinel) wherever the layout holds no whole-grid element,
outputs are pre-filled with ONE NaN bit pattern, and `Space.check` compares integer views, so that NaN equals NaN:
  (a) the written elements equal the whole-grid launch bit for bit, (b) every other stored element and both guard bands still hold the
  pre-fill pattern, (c) no written element is the pre-fill pattern.
The `op_*` functions launch one entry point on a Space - the whole-grid entry or its twin, the same argument list."""
import ctypes as C

import numpy as np

PREFILL32 = 0x7FC0DEAD                   # a quiet NaN no arithmetic produces
PREFILL64 = 0x7FF8DEADDEADDEAD
SENTINEL_I32 = -0x5A5A5A5B
SENTINEL_U8 = 0xA5
INVALID_ARG = 1                          # include/piso_hip.h: PISO_ERR_INVALID_ARG


def legal_slabs(ny):
    """Every (row_begin, row_end) the C ABI accepts: 4 <= rows <= ny - 6, inside the grid."""
    return [(b, b + n) for n in range(4, ny - 6 + 1) for b in range(0, ny - n + 1)]


def with_last(ny, slabs):
    """(row_begin, row_end, owns_last_face_row): a slab that ends at the grid's last row runs with and without the duplicate face row."""
    return [(b, e, last) for b, e in slabs for last in ((1, 0) if e == ny else (0,))]


def picked_slabs(ny):
    """First, last, one interior, the 4-row and the (ny - 6)-row slabs of a larger grid."""
    n = max(4, min(ny - 6, ny // 3))
    out = [(0, n), (ny - n, ny), ((ny - n) // 2 + 1, (ny - n) // 2 + 1 + n), (3, 7), (ny - 4, ny), (2, 2 + ny - 6), (6, ny)]
    legal, seen = legal_slabs(ny), []
    for s in out:
        if s in legal and s not in seen:
            seen.append(s)
    return seen


def refused_slabs(ny):
    """label -> (ny_global, row_begin, row_end, owns_last_face_row) of slabs every entry point must refuse on a grid of ny >= 16 rows."""
    return {"fewer than 4 rows": (ny, 0, 3, 0), "more than ny - 6 rows": (ny, 0, ny - 5, 0), "ny_global != ny": (ny - 1, 0, 4, 0),
            "row_end > ny": (ny, ny - 3, ny + 1, 0), "row_begin < 0": (ny, -1, 4, 0),
            "owns the duplicate face row below the last cell row": (ny, 4, 8, 1)}


def row_counts(nx, ny, comp, per_x, per_y):
    """Entries per row of the 5-point matrix of component `comp` (0: u faces [ny][nx + 1], 1: v faces [ny + 1][nx]): the diagonal plus
    every neighbour that lies inside the component's grid or across a periodic seam."""
    W, H = nx + (comp == 0), ny + (comp == 1)
    i = np.arange(W)[None, :]
    j = np.arange(H)[:, None]
    n = 1 + ((i >= 1) | bool(per_x)) + ((i <= W - 2) | bool(per_x)) + ((j >= 1) | bool(per_y)) + ((j <= H - 2) | bool(per_y))
    return (n + np.zeros((H, W), np.int64)).astype(np.int64)


def whole_row_pointers(nx, ny, per_x, per_y):
    """[n_u + 1][n_v + 1]: the two 0-based row pointer segments of the whole grid."""
    return [np.concatenate([[0], np.cumsum(row_counts(nx, ny, c, per_x, per_y).ravel())]) for c in (0, 1)]


class WholeLayout(object):
    """The whole grid in the same terms: every index is itself, a launch writes everything."""
    whole = True

    def __init__(self, nx, ny, per_x=0, per_y=0):
        self.nx, self.ny, self.per_x, self.per_y = int(nx), int(ny), int(per_x), int(per_y)
        n_u, n_v = (nx + 1) * ny, nx * (ny + 1)
        self.rp = whole_row_pointers(nx, ny, per_x, per_y)
        self.nnz = (int(self.rp[0][-1]), int(self.rp[1][-1]))
        sizes = dict(cells=nx * ny, faces=n_u + n_v, faces_vfirst=n_u + n_v, mask=(ny + 2) * (nx + 2),
                     pad=(ny + 2) * (nx + 3) + (ny + 3) * (nx + 2), laplace=5 * nx * ny, csr=sum(self.nnz), csr_rp=n_u + n_v + 2)
        self.idx = {k: np.arange(n, dtype=np.int64) for k, n in sizes.items()}
        self.own = {k: np.ones(n, bool) for k, n in sizes.items()}
        self.rp_local = np.concatenate(self.rp)
        self.n_u_stored = n_u


class SlabLayout(object):
    """include/piso_hip.h, piso_slab_t, for one (row_begin, row_end, owns_last_face_row)."""
    whole = False

    def __init__(self, nx, ny, row_begin, row_end, owns_last, per_x=0, per_y=0):
        nx, ny, rb, re, last = int(nx), int(ny), int(row_begin), int(row_end), 1 if owns_last else 0
        self.nx, self.ny, self.row_begin, self.row_end, self.owns_last, self.per_x, self.per_y = nx, ny, rb, re, last, int(per_x), int(per_y)
        n = re - rb
        self.rows = n
        n_u_g, n_v_g = (nx + 1) * ny, nx * (ny + 1)
        # "cell arrays, u faces: the ring rows [row_begin - 2, row_end + 2) (mod ny_global)"
        self.crows = (rb - 2 + np.arange(n + 4)) % ny
        # "v faces: the ring rows [row_begin - 3, row_end + 3) of the ring v[0] .. v[ny - 1], v[ny]"
        self.vrows = (rb - 3 + np.arange(n + 6)) % (ny + 1)
        # "padded cell masks: rows [row_begin, row_begin + (row_end - row_begin) + 3) of the [ny + 2] padded rows (no ring)"
        self.mrows = rb + np.arange(n + 3)
        self.mrows[self.mrows >= ny + 2] = -1
        # "padded velocities: padded u rows [row_begin, row_end + 2), then padded v rows [row_begin, row_end + 3)"
        self.purows, self.pvrows = rb + np.arange(n + 2), rb + np.arange(n + 3)
        # "A launch writes the OWNED rows (cells / u rows [row_begin, row_end), v rows [row_begin, row_end + owns_last_face_row))"
        self.own_c, self.own_v = np.arange(rb, re), np.arange(rb, re + last)
        # "piso_pad_velocity_slab fills padded u rows [row_begin, row_end + 1 + owns_last_face_row) and padded v rows
        #  [row_begin, row_end + 2 + owns_last_face_row)"
        self.fill_pu, self.fill_pv = np.arange(rb, re + 1 + last), np.arange(rb, re + 2 + last)
        # what a halo exchange leaves filled besides the owned rows (diffpiso/sharding.py's module text: "two rows below / above the slab
        # (incl. the duplicate row v[ny] across the seam)"; "the first slab's lower halo is v[ny - 2], v[ny - 1], v[ny]")
        self.halo_c = np.concatenate([(rb - 2 + np.arange(2)) % ny, (re + np.arange(2)) % ny])
        self.halo_v = np.concatenate([(rb - 2 + np.arange(2)) % ny, [ny] if rb == 0 else [], (re + np.arange(2)) % ny if last else re + np.arange(2)]).astype(np.int64)

        def grid(rows, width, base=0):
            r = np.asarray(rows, np.int64)[:, None]
            out = base + r * width + np.arange(width, dtype=np.int64)[None, :]
            out[np.broadcast_to(r < 0, out.shape)] = -1
            return out.ravel()

        def rowmask(rows, owned, width):
            return np.repeat(np.isin(rows, owned), width)
        u_idx, v_idx = grid(self.crows, nx + 1), grid(self.vrows, nx)
        u_own, v_own = rowmask(self.crows, self.own_c, nx + 1), rowmask(self.vrows, self.own_v, nx)
        u_halo, v_halo = rowmask(self.crows, self.halo_c, nx + 1), rowmask(self.vrows, self.halo_v, nx)
        pu_g = (ny + 2) * (nx + 3)
        self.idx = dict(cells=grid(self.crows, nx), faces=np.concatenate([u_idx, n_u_g + v_idx]),
                        faces_vfirst=np.concatenate([v_idx, n_v_g + u_idx]), mask=grid(self.mrows, nx + 2),
                        pad=np.concatenate([grid(self.purows, nx + 3), grid(self.pvrows, nx + 2, pu_g)]),
                        laplace=np.arange(rb * nx * 5, re * nx * 5, dtype=np.int64))
        self.own = dict(cells=rowmask(self.crows, self.own_c, nx), faces=np.concatenate([u_own, v_own]),
                        faces_vfirst=np.concatenate([v_own, u_own]), mask=np.zeros(self.idx["mask"].size, bool),
                        pad=np.concatenate([rowmask(self.purows, self.fill_pu, nx + 3), rowmask(self.pvrows, self.fill_pv, nx + 2)]),
                        laplace=np.ones(n * nx * 5, bool))
        self.halo = dict(cells=rowmask(self.crows, self.halo_c, nx), faces=np.concatenate([u_halo, v_halo]),
                         faces_vfirst=np.concatenate([v_halo, u_halo]))
        self.n_u_stored, self.n_v_stored = u_idx.size, v_idx.size
        # "CSR: the rows of the stored face rows (u rows, then v rows) in stored order; row pointers [stored u rows (nx + 1) + 1]
        #  [stored v rows nx + 1] are offsets into the stored value / column arrays of each component; column indices keep the whole
        #  grid's numbering"
        rp_g = whole_row_pointers(nx, ny, per_x, per_y)
        slots, owned, halo, rp_local, rp_written, nnz, base = [], [], [], [], [], [], 0
        for comp, rows, own_rows, halo_rows in ((0, self.crows, self.own_c, self.halo_c), (1, self.vrows, self.own_v, self.halo_v)):
            W = nx + (comp == 0)
            counts = row_counts(nx, ny, comp, per_x, per_y)
            at = [np.zeros(1, np.int64)]
            total = 0
            w = np.zeros(len(rows) * W + 1, bool)                              # a values launch writes the two ends of every owned row ...
            for k, j in enumerate(rows):
                lo, hi = int(rp_g[comp][j * W]), int(rp_g[comp][(j + 1) * W])
                mine = bool(np.any(own_rows == j))
                slots.append(base + np.arange(lo, hi, dtype=np.int64))
                owned.append(np.full(hi - lo, mine, bool))
                halo.append(np.full(hi - lo, bool(np.any(halo_rows == j)), bool))
                at.append(total + np.cumsum(counts[j]))
                total += hi - lo
                if mine:
                    w[k * W:(k + 1) * W + 1] = True
            rp_local.append(np.concatenate(at))
            rp_written.append(w)
            nnz.append(int(total))
            base += int(rp_g[comp][-1])
        rp_written[0][0] = rp_written[0][-1] = rp_written[1][0] = True         # ... and the three closed-form segment ends
        self.idx["csr"], self.own["csr"], self.halo["csr"] = np.concatenate(slots), np.concatenate(owned), np.concatenate(halo)
        self.rp_local = np.concatenate(rp_local)
        self.idx["csr_rp"] = np.full(self.rp_local.size, -1, np.int64)         # (local numbers: nothing to gather)
        self.own["csr_rp"] = np.concatenate(rp_written)
        self.nnz = tuple(nnz)

    def sizes8(self):
        """What piso_slab_sizes reports: {stored u rows, stored v rows, stored u faces, stored v faces, stored CSR entries of the u
        matrix, of the v matrix, stored mask rows, elements of the stored padded velocities}."""
        return [self.crows.size, self.vrows.size, self.n_u_stored, self.n_v_stored, self.nnz[0], self.nnz[1], self.mrows.size,
                self.idx["pad"].size]

    def struct(self):
        return slab_struct(self.ny, self.row_begin, self.row_end, self.owns_last)


def slab_struct(ny_global, row_begin, row_end, owns_last):
    from diffpiso import _native as N
    return N.Slab(int(ny_global), int(row_begin), int(row_end), int(owns_last))


# ---------------------------------------------------------------------------------------------------------------- device side
class Guarded(object):
    """A device array `t` inside `buf`, `band` elements of guard either side."""

    def __init__(self, buf, band, n):
        self.buf, self.band, self.t = buf, band, buf[band:band + n]


def _int_view(t):
    import torch
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def _filled(n, dtype, device):
    import torch
    if dtype == torch.float32:
        return torch.full((n,), PREFILL32, dtype=torch.int32, device=device).view(torch.float32)
    if dtype == torch.float64:
        return torch.full((n,), PREFILL64, dtype=torch.int64, device=device).view(torch.float64)
    return torch.full((n,), SENTINEL_I32 if dtype == torch.int32 else SENTINEL_U8, dtype=dtype, device=device)


def ptr(g):
    return None if g is None else C.c_void_p(g.t.data_ptr())


def f32c(v):
    return C.c_float(np.float32(v))


class Space(object):
    """A layout on the device: allocation, scatter, launch and the three checks."""

    def __init__(self, layout, device="cuda"):
        import torch
        self.L, self.device = layout, torch.device(device)
        self.nx, self.ny = layout.nx, layout.ny
        self.band = 4 * 5 * (self.nx + 3) + 6                                 # more than two rows' worth of any kind of array
        self._slab = None if layout.whole else layout.struct()
        self.slab_ptr = None if layout.whole else C.pointer(self._slab)
        self._idx, self._own, self._halo = {}, {}, {}

    def idx(self, kind):
        import torch
        if kind not in self._idx:
            self._idx[kind] = torch.as_tensor(self.L.idx[kind]).to(self.device)
            self._own[kind] = torch.as_tensor(self.L.own[kind]).to(self.device)
        return self._idx[kind]

    def own(self, kind):
        self.idx(kind)
        return self._own[kind]

    def filled(self, kind):
        """Owned rows plus what a halo exchange delivers."""
        import torch
        if kind not in self._halo:
            self._halo[kind] = self.own(kind) | torch.as_tensor(self.L.halo[kind]).to(self.device)
        return self._halo[kind]

    def n(self, kind):
        return int(self.L.idx[kind].size)

    def out(self, kind, dtype=None):
        import torch
        n = self.n(kind)
        return Guarded(_filled(n + 2 * self.band, dtype or torch.float32, self.device), self.band, n)

    def put(self, kind, whole, owned_only=False):
        """Whole-grid array -> the stored elements (halos populated; owned_only: the rows the rank owns, everything else NaN)."""
        if whole is None:
            return None
        idx = self.idx(kind)
        g = self.out(kind, whole.dtype)
        keep = idx >= 0
        if owned_only:
            keep = keep & self.own(kind)
        g.t[keep] = whole.reshape(-1)[idx[keep]]
        return g

    def row_pointers(self):
        """The row pointers of the stored rows as the restatement has them (local offsets)."""
        import torch
        g = self.out("csr_rp", torch.int32)
        g.t.copy_(torch.as_tensor(self.L.rp_local, dtype=torch.int32))
        return g

    def call(self, name, *args):
        from diffpiso import _native as N
        fn = getattr(N.lib, name if self.slab_ptr is None else name + "_slab")
        st = fn(*(args if self.slab_ptr is None else args + (self.slab_ptr,)))
        assert st == 0, "%s%s returned %d: %s" % (name, "" if self.slab_ptr is None else "_slab", st, N.lib.piso_last_error_string().decode())

    def expected(self, kind, g, whole_out, written=None):
        """The buffer a correct launch leaves: the whole-grid launch's value in every written element, the pre-fill everywhere else
        (whole_out None: a whole-grid launch, which has nothing to be compared with but its guards and its pre-fill)."""
        import torch
        w = self.own(kind) if written is None else written
        exp = _filled(g.buf.numel(), g.buf.dtype, self.device)
        if kind == "csr_rp":
            src = torch.as_tensor(self.L.rp_local, dtype=torch.int32).to(self.device)
            exp[self.band:self.band + src.numel()][w] = src[w]
        elif whole_out is None:
            exp[self.band:self.band + w.numel()][w] = g.t[w]
        else:
            exp[self.band:self.band + w.numel()][w] = whole_out.reshape(-1)[self.idx(kind)[w]]
        return exp

    def check(self, kind, g, whole_out, written=None):
        """(a) and (b) and (c) as ONE device boolean (no synchronisation here)."""
        w = self.own(kind) if written is None else written
        exp = self.expected(kind, g, whole_out, written)
        fill = _int_view(_filled(1, g.buf.dtype, self.device))
        return (_int_view(g.buf) == _int_view(exp)).all() & (_int_view(g.t)[w] != fill).all()

    def explain(self, kind, g, whole_out, written=None):
        """Which of the three properties failed, and where (for the assertion message; synchronises)."""
        w = self.own(kind) if written is None else written
        exp = self.expected(kind, g, whole_out, written)
        got, want = _int_view(g.buf), _int_view(exp)
        fill = _int_view(_filled(1, g.buf.dtype, self.device))
        a, b = self.band, self.band + w.numel()
        bad_a = ((got[a:b] != want[a:b]) & w).nonzero().reshape(-1)
        bad_b = ((got[a:b] != want[a:b]) & ~w).nonzero().reshape(-1)
        guard = int((got[:a] != want[:a]).sum() + (got[b:] != want[b:]).sum())
        bad_c = ((got[a:b] == fill) & w).nonzero().reshape(-1)
        return ("%s: %d written elements differ from the whole-grid launch (first stored index %s), %d elements outside the written rows "
                "changed (first %s), %d guard elements changed, %d written elements still hold the pre-fill (first %s)"
                % (kind, bad_a.numel(), bad_a[:1].tolist(), bad_b.numel(), bad_b[:1].tolist(), guard, bad_c.numel(), bad_c[:1].tolist()))


def verify(space, outs, ref, skip=()):
    """AND of Space.check over the outputs of one launch; `ref` holds the whole-grid launch's outputs under the same names (None: the
    launch IS the whole-grid one)."""
    ok = None
    for name, (kind, g) in outs.items():
        if name in skip:
            continue
        one = space.check(kind, g, None if ref is None else ref[name][1].t)
        ok = one if ok is None else ok & one
    return ok


def explain(space, outs, ref, skip=()):
    return "; ".join("%s -> %s" % (name, space.explain(kind, g, None if ref is None else ref[name][1].t)) for name, (kind, g) in outs.items()
                     if name not in skip and not bool(space.check(kind, g, None if ref is None else ref[name][1].t)))


class Tally(object):
    """Collects device booleans with a label each; ONE synchronisation when it is asked."""

    def __init__(self):
        self.flags, self.labels, self.why = [], [], []

    def add(self, label, flag, why=None):
        self.flags.append(flag.reshape(()))
        self.labels.append(label)
        self.why.append(why)

    def launch(self, label, space, outs, ref, skip=()):
        self.add(label, verify(space, outs, ref, skip), lambda: explain(space, outs, ref, skip))

    def __len__(self):
        return len(self.flags)

    def failures(self):
        import torch
        if not self.flags:
            return []
        ok = torch.stack(self.flags).cpu().numpy()
        return ["%s%s" % (self.labels[k], ": " + self.why[k]() if self.why[k] is not None else "") for k in np.nonzero(~ok)[0][:6]]


# ---------------------------------------------------------------------------------------------------------------- the entry points
def _stream():
    from diffpiso import _native as N
    return N.stream_ptr()


def pad_modes_c(modes):
    return (C.c_int * 4)(*[int(m) for m in modes])


def op_pad_velocity(S, vel, per_x, per_y):
    out = S.out("pad")
    S.call("piso_pad_velocity", ptr(vel), ptr(out), S.nx, S.ny, int(per_x), int(per_y), _stream())
    return {"vel_pad": ("pad", out)}


def op_a0_vfirst(S, a_flat, beta, dx_factor):
    out = S.out("faces_vfirst")
    S.call("piso_a0_vfirst", ptr(a_flat), ptr(out), S.nx, S.ny, f32c(beta), f32c(dx_factor), _stream())
    return {"a0": ("faces_vfirst", out)}


def op_face_forward(S, mode, modes, geo, p, acc, a_flat, in0, in1, in2, dmask):
    out0 = S.out("faces")
    out1 = S.out("faces") if mode == 1 else None
    S.call("piso_face_forward", int(mode), S.nx, S.ny, pad_modes_c(modes), f32c(geo["dxdy"]), f32c(geo["hx"]), f32c(geo["hy"]), f32c(geo["beta"]),
           ptr(p), ptr(acc), ptr(a_flat), ptr(in0), ptr(in1), ptr(in2), ptr(dmask), ptr(out0), ptr(out1), _stream())
    outs = {"out0": ("faces", out0)}
    if out1 is not None:
        outs["out1"] = ("faces", out1)
    return outs


def op_face_backward(S, mode, modes, geo, acc, a_flat, dmask, d0, d1, want1, want2):
    g0, dp = S.out("faces"), S.out("cells")
    g1 = S.out("faces") if want1 else None
    g2 = S.out("faces") if want2 else None
    S.call("piso_face_backward", int(mode), S.nx, S.ny, pad_modes_c(modes), f32c(geo["dxdy"]), f32c(geo["hx"]), f32c(geo["hy"]), f32c(geo["beta"]),
           ptr(acc), ptr(a_flat), ptr(dmask), ptr(d0), ptr(d1), ptr(g0), ptr(g1), ptr(g2), ptr(dp), _stream())
    outs = {"d_in0": ("faces", g0), "d_p": ("cells", dp)}
    if g1 is not None:
        outs["d_in1"] = ("faces", g1)
    if g2 is not None:
        outs["d_in2"] = ("faces", g2)
    return outs


def op_divergence(S, faces, geo):
    out = S.out("cells")
    S.call("piso_divergence", ptr(faces), ptr(out), S.nx, S.ny, f32c(geo["dxdy"]), f32c(geo["hx"]), f32c(geo["hy"]), _stream())
    return {"div": ("cells", out)}


def op_divergence_adjoint(S, dc, per_x, per_y, geo):
    out = S.out("faces")
    S.call("piso_divergence_adjoint", ptr(dc), ptr(out), S.nx, S.ny, int(per_x), int(per_y), f32c(geo["dxdy"]), f32c(geo["hx"]), f32c(geo["hy"]),
           _stream())
    return {"d_faces": ("faces", out)}


def op_h_contribution(S, m_delta, delta, a_flat, beta):
    h, hb = S.out("faces"), S.out("faces")
    S.call("piso_h_contribution", ptr(m_delta), ptr(delta), ptr(a_flat), f32c(beta), ptr(h), ptr(hb), S.nx, S.ny, _stream())
    return {"h": ("faces", h), "h_over_bma": ("faces", hb)}


def op_h_contribution_adjoint(S, d_h, d_hb, a_flat, beta):
    dm, dd = S.out("faces"), S.out("faces")
    S.call("piso_h_contribution_adjoint", ptr(d_h), ptr(d_hb), ptr(a_flat), f32c(beta), ptr(dm), ptr(dd), S.nx, S.ny, _stream())
    return {"d_m_delta": ("faces", dm), "d_delta": ("faces", dd)}


def op_laplace(S, dtype, active, fluid, a0):
    import torch
    out = S.out("laplace", dtype)
    S.call("piso_laplace_matrix_f64" if dtype == torch.float64 else "piso_laplace_matrix_f32", S.nx, S.ny, ptr(active), ptr(fluid), ptr(a0),
           ptr(out), _stream())
    return {"laplace": ("laplace", out)}


def op_assemble(S, vel_pad, dmask, active, visc, visc_is_field, no_slip, geo, pattern_only=0, col=None, rp=None):
    """piso_assemble_csr / piso_assemble_csr_slab.  `col`, `rp`: arrays to write into (a values launch of the product writes into the
    arrays its pattern-only launch filled); default: fresh, pre-filled ones."""
    import torch
    from diffpiso import _native as N
    val, diag = S.out("csr"), S.out("faces")
    col = col if col is not None else S.out("csr", torch.int32)
    rp = rp if rp is not None else S.out("csr_rp", torch.int32)
    L = S.L
    args = (ptr(vel_pad), ptr(val), ptr(col), ptr(rp), ptr(diag), ptr(dmask), ptr(active), ptr(visc), int(visc_is_field), S.nx, S.ny, L.per_x,
            L.per_y, f32c(geo["hy"]), f32c(geo["hx"]), f32c(geo["hx"]), f32c(geo["hy"]), ptr(no_slip), f32c(geo["beta"]), _stream())
    if S.slab_ptr is None:
        st = N.lib.piso_assemble_csr(*args)
    else:
        st = N.lib.piso_assemble_csr_slab(*(args + (S.slab_ptr, int(pattern_only))))
    assert st == 0, "piso_assemble_csr returned %d: %s" % (st, N.lib.piso_last_error_string().decode())
    return {"val": ("csr", val), "col": ("csr", col), "rowptr": ("csr_rp", rp), "diag": ("faces", diag)}


def op_matvec(S, val, rp, col, x, transpose):
    from diffpiso import _native as N
    y = S.out("faces")
    if S.slab_ptr is None:
        st = N.lib.piso_csr_matvec_f32(ptr(val), ptr(rp), ptr(col), ptr(x), ptr(y), S.nx, S.ny, int(transpose), _stream())
    else:
        st = N.lib.piso_csr_matvec_f32_slab(ptr(val), ptr(rp), ptr(col), ptr(x), ptr(y), S.nx, S.ny, S.L.per_x, S.L.per_y, int(transpose),
                                            _stream(), S.slab_ptr)
    assert st == 0, "piso_csr_matvec_f32 returned %d: %s" % (st, N.lib.piso_last_error_string().decode())
    return {"y": ("faces", y)}


# ---------------------------------------------------------------------------------------------------------------- halo exchange
MESSAGE_ORDER = ("to_upper", "to_lower", "from_lower", "from_upper")


def message_segments(table):
    """A rank's 28-int table -> {"to_upper": [(offset, length), ...], ...} (7 ints per message: count, 3 offsets, 3 lengths)."""
    t = [int(v) for v in table]
    assert len(t) == 28
    out = {}
    for k, key in enumerate(MESSAGE_ORDER):
        m = t[7 * k:7 * k + 7]
        assert 0 <= m[0] <= 3
        out[key] = [(m[1 + s], m[4 + s]) for s in range(m[0])]
    return out


def emulate_exchange(tables, arrays):
    """piso_comm_exchange for all ranks of a ring at once: rank r's `to_upper` segments land in the upper rank's `from_lower` segments,
    its `to_lower` segments in the lower rank's `from_upper` segments.  tables[r]: rank r's message table, arrays[r]: its stored array
    (a 1-D tensor, modified in place).  Every message is read before any is written, as on the wire."""
    world = len(tables)
    seg = [message_segments(t) for t in tables]
    sent = [a.clone() for a in arrays]
    for r in range(world):
        for send, peer, recv in (("to_upper", (r + 1) % world, "from_lower"), ("to_lower", (r - 1) % world, "from_upper")):
            src, dst = seg[r][send], seg[peer][recv]
            assert [n for _, n in src] == [n for _, n in dst], "rank %d %s %s does not fit rank %d %s %s" % (r, send, src, peer, recv, dst)
            for (so, n), (do, _) in zip(src, dst):
                assert 0 <= so and so + n <= sent[r].numel() and 0 <= do and do + n <= arrays[peer].numel(), "segment outside the stored array"
                arrays[peer][do:do + n] = sent[r][so:so + n]
