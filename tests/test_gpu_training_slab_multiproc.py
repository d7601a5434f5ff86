"""Training on y-slabs with REAL halo exchanges: 2 and 4 processes on the test box's one GPU (hipIpc mailboxes; nothing here has run across
a real link), tests/training_slab_worker.py in every rank.

(a) The four losses of the reference's training configuration (L2, spectral, strain rate, multistep averaging; factors [50, 0.5, 2, 0.5])
    behind two unrolled steps with the closure in the loop, spatial mixing layer at 64 x 48 (nx x ny; 4 ranks: 12-row slabs, the thinnest the
    seven-layer network's halo E = 10 allows).  The ranks' parts add up to the one-GPU loss at 1e-5 relative (the bar of
    test_sharded_step_four_ranks_weak_box_matches_one_gpu), each contribution on its own as well; the all-reduced weight gradients are the
    same bits on every rank and equal the one-GPU run's at 1e-5 relative L2 (the bound tests/test_gpu_closure_sharded_multiproc.py holds
    weight gradients to).
(b) `training_run(..., slab_comm=comm)` on 2 ranks: a solver-generated data set like tests/test_gpu_training_smoke.py's at 32 x 48 cells (two
    16-row slabs: whole 8-row bands of the ILU preconditioner, and wider than the network's halo), one epoch of four iterations; the LAST
    rank alone is told that a linear solve failed in the third.  Both ranks must take the restore branch together (else the next collective
    hangs), end with bit-identical weights and identical histories, the first iteration's loss is the one-GPU run's at 1e-5, and base_dir
    holds exactly one set of files.
Measured on 2 / 4 processes (error over bound): summed loss and the four contributions at most 0.011, weight gradients 0.036 / 0.028,
first-iteration loss of training_run 0.060.
Each child runs under its own time limit and the parent starts nothing more after a failure."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests.test_gpu_sharded_fields import _free_parent_gpu_memory, _rel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NX, NY = 64, 48
_one_gpu = {}


def run_ranks(world, args, timeout=240):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    _free_parent_gpu_memory()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "training_slab_worker.py"), str(r), str(world), str(port)] + [str(a) for a in args],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(world)]
    res = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=timeout)
            lines = [l for l in so.splitlines() if l.startswith("SLAB_WORKER ")]
            assert p.returncode == 0 and lines, "rank ended with code %s and no report:\n%s\n%s" % (p.returncode, so[-2000:], se[-4000:])
            res.append(json.loads(lines[-1][len("SLAB_WORKER "):]))
    finally:
        for q in procs:                                     # a failure or a time limit of one rank ends them all
            if q.poll() is None:
                q.kill()
                q.communicate()
    for r in res:
        if not r.get("ok") and ("piso_comm_peer_create" in r.get("error", "") or "piso_comm_peer_connect" in r.get("error", "")):
            pytest.skip("peer transport unavailable here: %s" % r["error"][:300])
    for r in res:
        assert r["ok"], "rank %d failed: %s" % (r["rank"], r.get("error"))
    return sorted(res, key=lambda r: r["rank"])


def one_gpu_losses():
    """The one-GPU run of (a) in this process, once."""
    if "losses" not in _one_gpu:
        from tests import training_slab_worker as W
        from tests.closure_sharded_worker import build
        B = build("spatial_ml", NY, NX, W.STEPS, torch.device("cuda"))
        loss, parts, wg, warn = W.run_losses(B, None)
        assert warn == 0 and all(np.isfinite(parts)) and all(p > 0 for p in parts), parts
        _one_gpu["losses"] = (loss, parts, wg.cpu().numpy())
    return _one_gpu["losses"]


@pytest.mark.parametrize("world", [2, 4])
def test_four_losses_on_slabs_add_up_to_the_one_gpu_loss(world):
    loss1, parts1, wg1 = one_gpu_losses()
    out = tempfile.mkdtemp(prefix="training_slab_losses_")
    res = run_ranks(world, ["losses", "spatial_ml", NY, NX, out])
    for r in res:
        assert r["warn"] == 0 and r["non_finite"] == 0, r
    loss = sum(r["part"] for r in res)
    parts = [sum(r["parts"][k] for r in res) for k in range(4)]
    ratios = [abs(loss - loss1) / abs(loss1) / 1e-5] + [abs(a - b) / abs(b) / 1e-5 for a, b in zip(parts, parts1)]
    wgs = [np.load(os.path.join(out, "weights%d.npy" % r)) for r in range(world)]
    e = _rel(wgs[0], wg1)
    print("four losses x%d: summed loss and contributions (L2, spectral, strain, multistep) against one GPU, error / 1e-5 = %s; "
          "weight gradients rel-L2 / 1e-5 = %.3g" % (world, ["%.3g" % x for x in ratios], e / 1e-5))
    assert max(ratios) <= 1.0, (loss, loss1, parts, parts1)
    for w in wgs[1:]:
        np.testing.assert_array_equal(w, wgs[0])
    assert np.linalg.norm(wg1) > 0 and e <= 1e-5, e


def test_training_run_on_two_ranks(tmp_path):
    import diffpiso as dp
    import diffpiso.training as T
    from tests import training_slab_worker as W
    from tests.test_gpu_training_smoke import _frames
    phys, sim, td = W.training_dicts(None)
    data = _frames(tmp_path, 9, tuple(sim["HRres"]), sim["box"], phys, sim["dt"])
    # one GPU, in this process: the same run, the same failed solve in the third evaluation
    phys, sim, td = W.training_dicts(data)
    base1 = str(tmp_path) + "/one_gpu"
    os.makedirs(base1)
    saved = (T.run_piso_steps, T._restore)
    try:
        seen = W.flaky_solver(T, on=True)
        hist1, val1 = dp.training_run(base1, phys, sim, td, solver_precision=1e-7)
    finally:
        T.run_piso_steps, T._restore = saved
    assert len(hist1) == 4 and hist1[2] == -1 and seen["restores"] == 1 and (hist1[[0, 1, 3]] > 0).all(), hist1
    # two ranks
    base2, out = str(tmp_path) + "/slabs", str(tmp_path) + "/out"
    os.makedirs(base2)
    os.makedirs(out)
    res = run_ranks(2, ["train", data, base2, out])
    h0, h1 = (np.array(r["history"]) for r in res)
    assert np.array_equal(h0, h1) and res[0]["validation"] == res[1]["validation"], (h0, h1)
    assert len(h0) == 4 and h0[2] == -1 and (h0 == -1).sum() == 1, h0
    # the rank that was NOT told about the failed solve restored as well, once each
    assert [r["restores"] for r in res] == [1, 1] and [r["evaluations"] for r in res] == [7, 7], res          # (4 training + 2 roll-out steps + 1 validation)
    assert not any(r["still_sharded"] for r in res)
    w0, w1 = (np.load(os.path.join(out, "final%d.npy" % r)) for r in range(2))
    assert np.isfinite(w0).all() and np.array_equal(w0.view(np.int32), w1.view(np.int32)), "the ranks' weights differ after the run"
    ratio = abs(h0[0] - hist1[0]) / abs(hist1[0]) / 1e-5
    print("training_run x2: first-iteration loss %r against one GPU %r, error / 1e-5 = %.3g; histories %s / %s" % (h0[0], hist1[0], ratio, h0, hist1))
    assert ratio <= 1.0
    assert np.isfinite(res[0]["validation"]).all() and len(res[0]["validation"]) == 1 and res[0]["validation"][0] > 0
    # exactly one set of files: what the one-GPU run leaves, nothing per rank
    assert sorted(os.listdir(base2)) == sorted(os.listdir(base1)) == sorted(
        ["loss.log", "model_comparison.npz", "model_epoch_000000.ckpt", "model_epoch_000000i000002.ckpt", "model_last_working",
         "training_loss_progression.npz", "validation_loss_progression.npz"])
    # the model comparison after the third iteration: one roll-out on the slabs, its distance summed over the ranks
    c1, c2 = np.load(os.path.join(base1, "model_comparison.npz")), np.load(os.path.join(base2, "model_comparison.npz"))
    assert list(c2["descriptors"]) == list(c1["descriptors"]) == ["000000i000002"] and c2["l2"].shape == (1,)
    print("training_run x2: model comparison l2 %r against one GPU %r (relative difference %.3g)"
          % (float(c2["l2"][0]), float(c1["l2"][0]), abs(float(c2["l2"][0]) - float(c1["l2"][0])) / float(c1["l2"][0])))
    assert np.isfinite(c2["l2"][0]) and c2["l2"][0] > 0
    ckpt = torch.cat([w.reshape(-1) for w in torch.load(os.path.join(base2, "model_epoch_000000.ckpt"))]).numpy()
    assert np.array_equal(ckpt.view(np.int32), w0.view(np.int32)), "the checkpoint is not the weights the ranks hold"
    assert sum(1 for line in open(os.path.join(base2, "loss.log")) if line.startswith("epoch")) == 4
