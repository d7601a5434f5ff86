"""One step's term of the spectral-energy loss, forward + backward, on ONE GPU: `spectral_energy_loss(..., fused=True)` (the kernels of
csrc/loss_spectrum.hip either side of torch.fft.fft2) against the torch expression it replaces.  It REPORTS; nothing is asserted.
Crops of 64 x 256 (a training grid), 1024 x 256 and 2048 x 2048 cells (h x w), the whole field as the window, log distance, random fields.
After a warm-up of both paths the two take turns in the same process; every timing window runs at least --window seconds of calls and ends
in a device synchronise, and the reported time per call is the median over the windows.  The launch count of each path is what the
profiler's kernel records of ONE forward + backward say (null if the profiler records no kernels here).  Every result is one JSON line
(also appended to --out, default profiles/spectral_loss_bench.txt).  Needs a GPU.

    python scripts/bench_spectral_loss.py [--window 0.5] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-piso_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CROPS = [(64, 256), (1024, 256), (2048, 2048)]


def make_case(h, w, fused):
    """-> a function that runs one step's loss term, forward + backward, and returns the value (a device scalar)."""
    import diffpiso as dp
    gen = torch.Generator().manual_seed(h + w)
    n_u = (w + 1) * h
    flat = torch.randn(n_u + w * (h + 1), generator=gen).cuda().requires_grad_(True)
    truth = torch.randn(1, 1, h + 1, w + 1, 2, generator=gen).cuda()
    grid = dp.StaggeredGrid([flat[n_u:].view(1, h + 1, w, 1), flat[:n_u].view(1, h, w + 1, 1)], dp.box[0:float(h), 0:float(w)],
                            extrapolation="periodic")
    zero = torch.zeros((), device="cuda")
    kw = {"fused": True} if fused else {}

    def step():
        flat.grad = None
        loss, c = dp.spectral_energy_loss(zero, [[grid]], [truth], 1, log_distance=True, **kw)
        loss.backward()
        return c.detach()
    return step, flat


def window(fn, seconds):
    """Calls of `fn` for at least `seconds`, ending in a synchronise -> ms per call."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def launches(fn):
    """Kernel records of one call; None where the profiler has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_loss_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spectral_loss.py needs a GPU"
    lines = []
    for h, w in CROPS:
        cases = {"fused": make_case(h, w, True), "torch": make_case(h, w, False)}
        values = {}
        for name, (fn, flat) in cases.items():               # warm-up: code objects, rocFFT plans, the shell tables
            for _ in range(3):
                values[name] = float(fn())
            torch.cuda.synchronize()
        grads = {name: flat.grad.detach().double() for name, (fn, flat) in cases.items()}
        ms = {name: [] for name in cases}
        for _ in range(args.rounds):
            for name, (fn, _) in cases.items():
                ms[name].append(window(fn, args.window))
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = {"bench": "spectral_loss", "crop_h": h, "crop_w": w, "what": "one step's loss term, forward + backward, ms per call (median of windows)",
               "fused_ms": round(med["fused"], 4), "torch_ms": round(med["torch"], 4), "fused_over_torch": round(med["fused"] / med["torch"], 3),
               "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
               "torch_ms_min_max": [round(min(ms["torch"]), 4), round(max(ms["torch"]), 4)],
               "window_s": args.window, "rounds": args.rounds,
               "launches_fused": launches(cases["fused"][0]), "launches_torch": launches(cases["torch"][0]),
               "value_fused": values["fused"], "value_torch": values["torch"],
               "gradient_rel_l2_fused_vs_torch": float((grads["fused"] - grads["torch"]).norm() / grads["torch"].norm()),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del cases, grads
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
