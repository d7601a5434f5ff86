"""The run-time-shaped convolution family (csrc/conv_any.hip) measured, at config 4's size 256 x 896, SAME padding, batch 1:
    (a) the price of run-time shapes: on every layer of the reference's network - shapes that have a fixed, tuned instance - the *_any entries against
        the old entries through the C ABI, pass by pass (forward, input gradient = the forward entry on the flipped weights, weight gradient);
    (b) shapes the fixed tables lack (default 5 x 5 5 -> 24, 3 x 3 40 -> 40, 3 x 3 128 -> 128): diffpiso.closure.conv2d_leaky - the new family -
        against MIOpen, i.e. the same call inside tests.closure_checker.torch_convolutions(), pass by pass (one graph per gradient, autograd.grad of its one
        operand; where the weight gradient of a shape has a fixed instance - 5 x 5 5 -> 24 - conv2d_leaky runs that, and the line says so).
Warmed up, medians of alternated repeats in one process, every timing ends in a device synchronise.  Every result is one JSON line (also appended to
--out, default profiles/conv_any_bench.txt); ratio = new family / the other side.  Needs a GPU.

    python scripts/bench_conv_any.py [--reps 20] [--size 256x896] [--out FILE]
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

REFERENCE_LAYERS = [(7, 4, 16), (5, 16, 16), (5, 16, 32), (3, 32, 64), (3, 64, 64), (1, 64, 64), (1, 64, 2)]
NEW_SHAPES = [(5, 5, 24), (3, 40, 40), (3, 128, 128)]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternated(cases, reps):
    """{name: fn} -> {name: median ms}, the cases taking turns"""
    for fn in cases.values():
        fn()
        fn()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: (min(v), max(v)) for k, v in ms.items()}


def part_a(emit, reps, H, W):
    import diffpiso._native as N
    from diffpiso.closure import _laid_out, _laid_out_any
    lib, s = N.lib, N.stream_ptr()
    gen = torch.Generator().manual_seed(0)
    for k, cin, cout in REFERENCE_LAYERS:
        pad = k // 2
        x = torch.randn(H, W, cin, generator=gen).cuda()
        g = torch.randn(H, W, cout, generator=gen).cuda()
        w = torch.randn(k, k, cin, cout, generator=gen).cuda() / (k * k * cin) ** 0.5
        wd = w.flip(0, 1).permute(0, 1, 3, 2).contiguous()
        out, dx, dw = torch.empty(H, W, cout, device="cuda"), torch.empty(H, W, cin, device="cuda"), torch.empty(k, k, cin, cout, device="cuda")
        lay = {"fixed": (_laid_out(w), _laid_out(wd)), "any": (_laid_out_any(w), _laid_out_any(wd))}
        nb = {"fixed": lib.piso_conv2d_wgrad_workspace_bytes(k, cin, cout), "any": lib.piso_conv2d_wgrad_any_workspace_bytes(k, cin, cout, H)}
        ws = torch.empty(max(nb.values()), dtype=torch.uint8, device="cuda")
        p = N.ptr
        passes = {
            "forward": {"fixed": lambda: N.check(lib.piso_conv2d_forward(p(x), p(lay["fixed"][0]), p(out), H, W, cin, cout, k, pad, 1, s), "forward"),
                        "any": lambda: N.check(lib.piso_conv2d_forward_any(p(x), p(lay["any"][0]), p(out), H, W, cin, cout, k, pad, pad, 0, 0, 1, s), "forward_any")},
            "input_gradient": {"fixed": lambda: N.check(lib.piso_conv2d_forward(p(g), p(lay["fixed"][1]), p(dx), H, W, cout, cin, k, k - 1 - pad, 0, s), "forward"),
                               "any": lambda: N.check(lib.piso_conv2d_forward_any(p(g), p(lay["any"][1]), p(dx), H, W, cout, cin, k, k - 1 - pad, k - 1 - pad, 0, 0, 0, s),
                                                      "forward_any")},
            "weight_gradient": {"fixed": lambda: N.check(lib.piso_conv2d_wgrad(p(x), p(g), p(dw), H, W, cin, cout, k, pad, p(ws), C.c_size_t(nb["fixed"]), s), "wgrad"),
                                "any": lambda: N.check(lib.piso_conv2d_wgrad_any(p(x), p(g), p(dw), H, W, cin, cout, k, pad, pad, 0, 0, p(ws), C.c_size_t(nb["any"]), s),
                                                       "wgrad_any")}}
        for name, cases in passes.items():
            med, spread = alternated(cases, reps)
            emit(dict(part="a", shape=[k, cin, cout], size=[H, W], **{"pass": name}, fixed_ms=med["fixed"], any_ms=med["any"], fixed_ms_spread=spread["fixed"],
                      any_ms_spread=spread["any"], ratio_any_to_fixed=med["any"] / med["fixed"]))


def part_b(emit, reps, H, W, shapes):
    import diffpiso._native as N
    import diffpiso.closure as closure
    from tests.closure_checker import torch_convolutions
    gen = torch.Generator().manual_seed(1)
    for k, cin, cout in shapes:
        pad = k // 2
        x = torch.randn(1, H, W, cin, generator=gen).cuda()
        w = (torch.randn(cout, cin, k, k, generator=gen) / (k * k * cin) ** 0.5).cuda()
        g = torch.randn(1, H, W, cout, generator=gen).cuda()
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

        def layer(a, b, miopen):
            if not miopen:
                return closure.conv2d_leaky(a, b, pad, False)
            with torch_convolutions():
                return closure.conv2d_leaky(a, b, pad, False)
        with torch.no_grad():
            layer(x, w, False)
        assert N.conv_last_dispatch()["family"] == 7, "the shape has a fixed instance: it does not run the new family"
        # one graph per gradient: the layer's backward computes what its INPUTS ask for, so each graph has one input that asks
        y = {(side, wrt): layer(xg if wrt == "x" else x, wg if wrt == "w" else w, side == "miopen") for side in ("any", "miopen") for wrt in ("x", "w")}

        def fwd(miopen):
            with torch.no_grad():
                layer(x, w, miopen)
        passes = {"forward": {"any": lambda: fwd(False), "miopen": lambda: fwd(True)},
                  "input_gradient": {side: (lambda side=side: torch.autograd.grad(y[side, "x"], xg, g, retain_graph=True)) for side in ("any", "miopen")},
                  "weight_gradient": {side: (lambda side=side: torch.autograd.grad(y[side, "w"], wg, g, retain_graph=True)) for side in ("any", "miopen")}}
        for name, cases in passes.items():
            med, spread = alternated(cases, reps)
            emit(dict(part="b", shape=[k, cin, cout], size=[H, W], **{"pass": name}, weight_gradient_has_fixed_instance=N.conv2d_instantiated(2, k, cin, cout),
                      any_ms=med["any"], miopen_ms=med["miopen"], any_ms_spread=spread["any"], miopen_ms_spread=spread["miopen"],
                      ratio_any_to_miopen=med["any"] / med["miopen"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", default="256x896")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_any_bench.txt"))
    ap.add_argument("--parts", default="ab")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_any.py needs a GPU")
    H, W = (int(v) for v in a.size.split("x"))
    sink = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()
    emit(dict(device=torch.cuda.get_device_name(0), reps=a.reps, script="scripts/bench_conv_any.py"))
    if "a" in a.parts:
        part_a(emit, a.reps, H, W)
    if "b" in a.parts:
        part_b(emit, a.reps, H, W, NEW_SHAPES)
