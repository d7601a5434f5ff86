"""The fused epilogue of a closure layer (csrc/conv_epilogue.hip) measured at config 4's size 256 x 896, batch 1, for 16, 64 and 2 output channels:
    fused     piso_conv_epilogue_forward (z, bias, skip -> y, leaky ReLU, out of place as conv2d_act calls it) and piso_conv_epilogue_backward
              (g, y -> gpre and dbias) through the C ABI, with their GB/s on the bytes they must move (forward: z, skip read, y written; backward: g, y
              read, gpre written; the bias and the band partials are noise beside them);
    torch     the same layer written as torch ops: add, add, leaky_relu under no_grad, and their autograd backward (torch.autograd.grad of y with respect
              to z, bias and skip);
    conv      beside them, the layer's convolution itself (conv2d_leaky, no activation): forward, and input + weight gradient - what the epilogue
              is a share of.  Layers: 5 x 5 16 -> 16, 3 x 3 64 -> 64, 1 x 1 64 -> 2 (the reference's layers with those output channels).
Every timing is a window of --inner back-to-back calls that ends in a device synchronise, divided by --inner (one call is a few microseconds: a window of
one would time the launch); warmed up, medians of alternated repeats in one process.  Every result is one JSON line (also appended to --out, default
profiles/conv_epilogue_bench.txt); ratio = fused / torch.  Needs a GPU.

    python scripts/bench_conv_epilogue.py [--reps 20] [--inner 50] [--size 256x896] [--out FILE]
"""
import argparse
import ctypes as C
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
import torch.nn.functional as F  # noqa: E402

LAYERS = [(5, 16, 16), (3, 64, 64), (1, 64, 2)]


def timed(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / inner


def alternated(cases, reps, inner):
    """{name: fn} -> {name: median ms per call}, the cases taking turns"""
    for fn in cases.values():
        fn()
        fn()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn, inner))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: (min(v), max(v)) for k, v in ms.items()}


def bench(emit, reps, inner, H, W):
    import diffpiso._native as N
    from diffpiso.closure import conv2d_leaky
    lib, s, p = N.lib, N.stream_ptr(), N.ptr
    gen = torch.Generator().manual_seed(0)
    for k, cin, cout in LAYERS:
        pixels, n = H * W, H * W * cout
        z, skip, g = (torch.randn(1, H, W, cout, generator=gen).cuda() for _ in range(3))
        bias = torch.randn(cout, generator=gen).cuda()
        y, gpre, dbias = torch.empty_like(z), torch.empty_like(z), torch.empty_like(bias)
        nfloats = lib.piso_conv_epilogue_workspace_bytes(pixels, cout) // 4
        ws = torch.empty(nfloats, device="cuda")
        N.check(lib.piso_conv_epilogue_forward(p(z), p(bias), p(skip), p(y), pixels, cout, 1, s), "forward")
        # the two sides compute the same thing: y bit for bit, dbias to rounding
        zg, bg, sg = (t.clone().requires_grad_(True) for t in (z, bias, skip))
        yt = F.leaky_relu((zg + bg) + sg, 0.2)
        N.check(lib.piso_conv_epilogue_backward(p(g), p(y), p(gpre), p(dbias), pixels, cout, 1, p(ws), C.c_size_t(nfloats), s), "backward")
        dz, db, ds = torch.autograd.grad(yt, (zg, bg, sg), g, retain_graph=True)
        same = dict(y_equals_torch_bitwise=bool(torch.equal(yt.detach(), y)), gpre_equals_torch_bitwise=bool(torch.equal(dz, gpre)),
                    dbias_max_difference_to_torch=float((db - dbias).abs().max()), dbias_scale=float(gpre.abs().sum(dim=(0, 1, 2)).max()))
        assert torch.allclose(yt.detach(), y, rtol=1e-6, atol=1e-6) and torch.allclose(dz, gpre, rtol=1e-6, atol=1e-6) and same["dbias_max_difference_to_torch"] <= 1e-4 * same["dbias_scale"]

        def torch_forward():
            with torch.no_grad():
                F.leaky_relu((z + bias) + skip, 0.2)
        x = torch.randn(1, H, W, cin, generator=gen).cuda().requires_grad_(True)
        w = (torch.randn(cout, cin, k, k, generator=gen) / (k * k * cin) ** 0.5).cuda().requires_grad_(True)
        yc = conv2d_leaky(x, w, k // 2, False)

        def conv_forward():
            with torch.no_grad():
                conv2d_leaky(x, w, k // 2, False)
        cases = {"fused_forward": lambda: lib.piso_conv_epilogue_forward(p(z), p(bias), p(skip), p(y), pixels, cout, 1, s),
                 "torch_forward": torch_forward,
                 "fused_backward": lambda: lib.piso_conv_epilogue_backward(p(g), p(y), p(gpre), p(dbias), pixels, cout, 1, p(ws), C.c_size_t(nfloats), s),
                 "fused_backward_without_dbias": lambda: lib.piso_conv_epilogue_backward(p(g), p(y), p(gpre), None, pixels, cout, 1, None, C.c_size_t(0), s),
                 "torch_backward": lambda: torch.autograd.grad(yt, (zg, bg, sg), g, retain_graph=True),
                 "conv_forward": conv_forward,
                 "conv_backward": lambda: torch.autograd.grad(yc, (x, w), g, retain_graph=True)}
        med, spread = alternated(cases, reps, inner)
        bands, ppb = N.conv_epilogue_plan(pixels, cout)
        moved = 3 * n * 4
        emit(dict(layer=[k, cin, cout], size=[H, W], channels=cout, bands=bands, pixels_per_band=ppb, bytes_moved_per_pass=moved, **same,
                  **{name + "_ms": v for name, v in med.items()}, **{name + "_ms_spread": v for name, v in spread.items()},
                  fused_forward_GBps=moved / med["fused_forward"] * 1e-6, fused_backward_GBps=moved / med["fused_backward"] * 1e-6,
                  ratio_forward_fused_to_torch=med["fused_forward"] / med["torch_forward"], ratio_backward_fused_to_torch=med["fused_backward"] / med["torch_backward"],
                  epilogue_share_of_layer_forward=med["fused_forward"] / (med["fused_forward"] + med["conv_forward"]),
                  epilogue_share_of_layer_backward=med["fused_backward"] / (med["fused_backward"] + med["conv_backward"])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--size", default="256x896")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_epilogue_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_epilogue.py needs a GPU")
    H, W = (int(v) for v in a.size.split("x"))
    sink = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()
    emit(dict(device=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, script="scripts/bench_conv_epilogue.py"))
    bench(emit, a.reps, a.inner, H, W)
