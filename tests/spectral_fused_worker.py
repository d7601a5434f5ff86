"""One rank of the fused spectral loss on y-slabs (started by tests/test_gpu_spectral_fused_multiproc.py):

    python tests/spectral_fused_worker.py RANK WORLD PORT NY NX OUTDIR

The grid, the initial velocity and the seeded truth sequence of the loss check of tests/training_slab_worker.py (spatial mixing layer); the
prediction of step s is that velocity plus seeded noise (`predictions`) - the solver is not what this is about.  The rank scatters the
predictions to its stored rows, evaluates `spectral_energy_loss(..., fused=True)` on the slab fields (every rank gathers the whole field and
contributes value / world), runs the reverse sweep and reports its part; the gradient on its OWNED face rows goes to OUTDIR/grad<r>.npz.
`predictions` and `evaluate` are also what the test calls in its own process for the one-GPU run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "differentiable-piso_amd"))

FACTOR = 0.5                                                 # the spectral loss's factor in the reference's training configuration


def predictions(vel_t, steps):
    """Seeded whole-grid predictions [steps][1, ny + 1, nx + 1, 2] around the initial velocity (host tensors, the same on every rank)."""
    import torch
    g = torch.Generator().manual_seed(29)
    base = vel_t.detach().cpu().to(torch.float32)
    return [base + 0.02 * (s + 1) * torch.randn(base.shape, generator=g) for s in range(steps)]


def evaluate(fields, leaves, truth, window):
    """-> (the contribution - on slab fields the rank's part - as a float, the leaves' gradients)."""
    import torch
    import diffpiso as dp
    loss, c = dp.spectral_energy_loss(torch.zeros((), device="cuda"), [fields], [truth], len(fields), window, FACTOR, 0, sum_steps=True,
                                      fused=True)
    loss.backward()
    return float(c.detach()), [f.grad for f in leaves]


def main():
    rank, world, port = (int(v) for v in sys.argv[1:4])
    ny, nx, outdir = int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import numpy as np
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    out = {"rank": rank, "world": world, "ok": False}
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = None
    try:
        import diffpiso as dp
        from diffpiso.distributed import SlabCommunicator
        from diffpiso.sharding import StepSharding
        from tests import training_slab_worker as W
        from tests.closure_sharded_worker import build
        B = build("spatial_ml", ny, nx, W.STEPS, torch.device("cpu"))
        comm = SlabCommunicator(rank=rank, world=world, device=device, transport="peer", row_capacity=26 * nx + 64)
        sh = StepSharding(comm, nx, ny)
        ext = dp.Material.extrapolation_mode(B["domain"].boundaries)
        leaves = [sh.scatter_staggered(p).requires_grad_(True) for p in predictions(B["vel_t"], W.STEPS)]
        fields = [sh.staggered_grid(f, B["domain"].box, ext) for f in leaves]
        part, grads = evaluate(fields, leaves, W.truth_sequence(B["vel_t"], W.STEPS), W.WINDOW)
        sh.check()
        rows = {}
        for s, g in enumerate(grads):
            u, v = sh.owned_faces(g)
            rows["u%d" % s], rows["v%d" % s] = u.cpu().numpy(), v.cpu().numpy()
        np.savez(os.path.join(outdir, "grad%d.npz" % rank), **rows)
        out.update(ok=True, part=part, j0=int(sh.j0), j1=int(sh.j1), last=bool(sh.last))
    except Exception as e:        # the parent reads the reason
        import traceback
        out["error"] = "%r\n%s" % (e, traceback.format_exc()[-1500:])
    finally:
        print("SLAB_WORKER " + json.dumps(out), flush=True)
        try:
            if comm is not None:
                comm.close()
        except Exception:
            pass
        try:
            dist.destroy_process_group()
        except Exception:
            pass


if __name__ == "__main__":
    main()
