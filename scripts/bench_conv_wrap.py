"""The closure network with wrap-around padding against the zero-padded one: one forward + backward (input and weight gradients) of the
7-layer network at config 4's size, 256 x 896 x 4, SAME padding, batch 1.  Cases
    zero_old   wrap (0, 0): piso_conv2d_forward / piso_conv2d_wgrad, the *_kernel instances - what every current user runs
    zero_ex    wrap (0, 0) through piso_conv2d_forward_ex / piso_conv2d_wgrad_ex (a (pad_y, pad_x) tuple): the same arithmetic on the *_ex_kernel
               instances - what the general geometry costs by itself
    wrap_x     wrap (0, 1) and
    wrap_yx    wrap (1, 1) through the *_ex entries: no tap row or column is skipped at the edges any more
Warmed up, medians of alternated repeats in one process, every timing ends in a device synchronise.  Every result is one JSON line; the last
line holds the ratios to zero_old.  Needs a GPU.

    python scripts/bench_conv_wrap.py [--reps 30] [--size 256x896]
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


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main(reps, H, W):
    import diffpiso._native as N
    from diffpiso.closure import FullyConvNetwork, conv2d_leaky
    net = FullyConvNetwork(seed=1).cuda()
    x = torch.randn(1, H, W, 4, generator=torch.Generator().manual_seed(0)).cuda().requires_grad_(True)

    def evaluate(wrap, ex):
        """the network's layer loop (FullyConvNetwork.forward, SAME) with the entries chosen by hand"""
        y = x
        for i, w in enumerate(net.weights):
            k = w.shape[-1]
            y = conv2d_leaky(y, w, (k // 2, k // 2) if ex else k // 2, i < len(net.weights) - 1, wrap=wrap)
        return y

    cases = {"zero_old": ((False, False), False), "zero_ex": ((False, False), True), "wrap_x": ((False, True), True), "wrap_yx": ((True, True), True)}
    g = torch.randn(1, H, W, 2, generator=torch.Generator().manual_seed(1)).cuda()

    def fwd(k):
        with torch.no_grad():
            return evaluate(*cases[k])

    def fwd_bwd(k):
        x.grad = None
        for w in net.weights:
            w.grad = None
        evaluate(*cases[k]).backward(g)

    for k in cases:                                        # warm-up, and which entries ran
        fwd_bwd(k)
        torch.cuda.synchronize()
        assert (N.conv_last_geometry() != {}) == cases[k][1], k
    ms = {k: {"forward": [], "forward_backward": []} for k in cases}
    for _ in range(reps):                                  # alternated
        for k in cases:
            ms[k]["forward"].append(timed(lambda: fwd(k))[0])
            ms[k]["forward_backward"].append(timed(lambda: fwd_bwd(k))[0])
    med = {}
    for k in cases:
        med[k] = {m: statistics.median(v) for m, v in ms[k].items()}
        print(json.dumps(dict(case=k, wrap=[int(b) for b in cases[k][0]], entries="ex" if cases[k][1] else "old", size=[H, W],
                              forward_ms=med[k]["forward"], forward_ms_spread=(min(ms[k]["forward"]), max(ms[k]["forward"])),
                              forward_backward_ms=med[k]["forward_backward"],
                              forward_backward_ms_spread=(min(ms[k]["forward_backward"]), max(ms[k]["forward_backward"])))), flush=True)
    print(json.dumps(dict(ratios_to_zero_old={k: {m: med[k][m] / med["zero_old"][m] for m in med[k]} for k in cases if k != "zero_old"})), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", default="256x896")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_wrap.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps)), flush=True)
    H, W = (int(v) for v in a.size.split("x"))
    main(a.reps, H, W)
