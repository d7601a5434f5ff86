"""`spectral_energy_loss(..., fused=True)` on y-slabs: 2 processes on the test box's one GPU (tests/spectral_fused_worker.py in every rank),
on the 64 x 48 (nx x ny) spatial mixing layer of the loss check of tests/test_gpu_training_slab_multiproc.py.

On slab fields every rank gathers the whole face field - an exact copy - and evaluates the SAME deterministic function on it, so nothing is
left to a tolerance: each rank's part times `world` is the one-GPU fused value bit for bit (the part is value / world, a power of two here),
and the gradient on a rank's owned face rows is the one-GPU gradient's rows bit for bit (the upstream 1 / world and the gather's
world x are powers of two as well, and every pass in between is linear in the cotangent).  The default slab path, without the flag, is
not touched here.  Each child runs under `run_ranks`' own time limit."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests.test_gpu_multiproc import run_ranks
from tests.test_gpu_spectral_fused import flat_of, grid_of

pytestmark = pytest.mark.gpu
NX, NY, WORLD = 64, 48, 2


def test_two_ranks_reproduce_the_one_gpu_bits():
    from tests import spectral_fused_worker as S
    from tests import training_slab_worker as W
    from tests.closure_sharded_worker import build
    B = build("spatial_ml", NY, NX, W.STEPS, torch.device("cpu"))
    leaves = [flat_of(p).cuda().requires_grad_(True) for p in S.predictions(B["vel_t"], W.STEPS)]
    value1, grads1 = S.evaluate([grid_of(f, NY, NX) for f in leaves], leaves, W.truth_sequence(B["vel_t"], W.STEPS), W.WINDOW)
    assert np.isfinite(value1) and value1 > 0
    n_u = (NX + 1) * NY
    grads1 = [(g[:n_u].view(NY, NX + 1).cpu().numpy(), g[n_u:].view(NY + 1, NX).cpu().numpy()) for g in grads1]
    assert all(np.isfinite(u).all() and np.isfinite(v).all() and u.any() and v.any() for u, v in grads1)

    out = tempfile.mkdtemp(prefix="spectral_fused_")
    res = run_ranks(WORLD, NX, NY, False, timeout=240, worker="spectral_fused_worker.py", extra=[str(NY), str(NX), out])
    assert len(res) == WORLD
    for r in res:
        assert r["ok"], "rank %d failed: %s" % (r["rank"], r.get("error"))
    for r in res:
        assert np.float32(r["part"]) * np.float32(WORLD) == np.float32(value1), (r["rank"], r["part"], value1)
        rows = np.load(os.path.join(out, "grad%d.npz" % r["rank"]))
        j0, j1, last = r["j0"], r["j1"], 1 if r["last"] else 0
        for s, (u1, v1) in enumerate(grads1):
            u, v = rows["u%d" % s], rows["v%d" % s]
            assert u.shape == (j1 - j0, NX + 1) and v.shape == (j1 - j0 + last, NX)
            assert np.array_equal(u.view(np.int32), u1[j0:j1].view(np.int32)), "rank %d, step %d: u rows differ" % (r["rank"], s)
            assert np.array_equal(v.view(np.int32), v1[j0:j1 + last].view(np.int32)), "rank %d, step %d: v rows differ" % (r["rank"], s)
    assert sorted((r["j0"], r["j1"]) for r in res) == [(0, NY // 2), (NY // 2, NY)]
