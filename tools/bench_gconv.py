#!/usr/bin/env python
"""Timings of the grouped conv ops (tn_c8_gconv_* on the 16-bit conv stack, tn_gconv_* in float32; theanet_amd/csrc/gconv.h)
at the three grouped layers of params/cifar_grp.prms -- batch 2048, 3x3 'same': 32 maps of 32x32 in 2 groups, 64 of 16x16
in 4, 128 of 8x8 in 4 -- by tools/bench_dwconv.py's method, each against two things on the same tensors in the same run:

  d2d    tn_d2d of the op's bytes read plus written (forward: x + y; input gradient: dz + prev_a + dx; weight gradient:
         x + dz): the bandwidth yardstick;
  dense  the dense product of the same C and K on the existing kernels ((K, C, 3, 3) weights, the groups on the block
         diagonal: g times the products; bfloat16: the general family tn_c8_convg_*, float32: tn_conv2d_*) -- the only way
         to run the layer without the grouped kernels.

    python tools/bench_gconv.py [--iters N] [--rounds R] [--steps K] [--reps R] [--batch-div D] [--no-net]

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The three are measured
alternately, --rounds times each; the table gives the median of each, the A/A spread of the grouped op ((max - min) /
median over the rounds) and the two ratios.  Back-to-back launches on tensors below the 256 MB Infinity Cache sit in it,
so rates are upper bounds of what a step sees.  Then ms/step of cifar_grp.prms in bfloat16 and float32 (host clock around
--steps enqueued steps ending in a synchronise, median of --reps)."""
import argparse
import ast
import copy
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theanet_amd import NeuralNet  # noqa: E402
from theanet_amd.device import get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch-div", type=int, default=1, help="divide the batch sizes")
ap.add_argument("--no-net", action="store_true")
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
NB = 4


def timeit(fn, iters):
    for _ in range(5):
        fn()
    ctx.sync()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    lib.tn_event_create(ctx.h, ctypes.byref(a))
    lib.tn_event_create(ctx.h, ctypes.byref(b))
    lib.tn_event_record(ctx.h, a)
    for _ in range(iters):
        fn()
    lib.tn_event_record(ctx.h, b)
    ms = ctypes.c_float()
    ctx.call("tn_event_elapsed_ms", a, b, ctypes.byref(ms))
    lib.tn_event_destroy(ctx.h, a)
    lib.tn_event_destroy(ctx.h, b)
    return ms.value * 1e3 / iters


def trio(fns):
    """Alternating rounds of the three: medians, and the spread of the first."""
    t = [[] for _ in fns]
    for _ in range(args.rounds):
        for k, f in enumerate(fns):
            t[k].append(timeit(f, args.iters))
    med = [statistics.median(v) for v in t]
    return med, (max(t[0]) - min(t[0])) / med[0]


def block_diagonal(w, g):
    K, Cg = w.shape[:2]
    out = np.zeros((K, Cg * g, 3, 3), np.float32)
    for grp in range(g):
        ks = slice(grp * K // g, (grp + 1) * K // g)
        out[ks, grp * Cg:(grp + 1) * Cg] = w[ks]
    return out


act, prm = 1, .1                           # relu10
print("%d launches per measurement, %d alternating rounds" % (args.iters, args.rounds))
print("%-9s %-16s %-6s %9s %7s %9s %9s %8s %8s %7s" % ("dtype", "N,C,S,g", "op", "grp us", "spread", "d2d us", "dense us",
                                                      "grp/d2d", "grp/dense", "MB"))
rng = np.random.default_rng(0)
for dtype in ("bfloat16", "float32"):
    ctx.set_matmul_dtype(dtype, 1.0)
    c8 = dtype == "bfloat16"
    for N, C, S, g in ((2048, 32, 32, 2), (2048, 64, 16, 4), (2048, 128, 8, 4)):
        N = max(1, N // args.batch_div)
        if c8:
            shape, item = (N, C // 8, S, S, 8), 2
            mk = lambda: ctx.array((rng.integers(0x3c00, 0x3f80, shape, dtype=np.uint16) & 0xff80))      # bf16 in [.5, 1)
            geom, dgeom = (N, C, S, S, C, g, 3, 1, 1, S, S), (N, C, S, S, C, 3, 1, 1, S, S)
            ops_, dn = "tn_c8_gconv_", "tn_c8_convg_"
            assert lib.tn_c8_gconv_supported(*geom) and lib.tn_c8_convg_supported(*dgeom)
        else:
            shape, item = (N, C, S, S), 4
            mk = lambda: ctx.array(rng.random(shape, dtype=np.float32))
            geom, dgeom = (N, C, S, S, C, g, 3, 1, 1, S, S), (N, C, S, S, C, 3, 1, 1, S, S)
            ops_, dn = "tn_gconv_", "tn_conv2d_"
            assert lib.tn_gconv_supported(*geom)
        x, y, dz, dx, pa = mk(), mk(), mk(), mk(), mk()
        w = (rng.standard_normal((C, C // g, 3, 3)) / 3).astype(np.float32)
        W, Wd, b = ctx.array(w), ctx.array(block_diagonal(w, g)), ctx.array(np.zeros(C, np.float32))
        gW, gWd, gb = ctx.empty(w.shape), ctx.empty((C, C, 3, 3)), ctx.empty((C,))
        nbytes = int(np.prod(shape)) * item
        src, dst = ctx.empty((3 * nbytes,), np.uint8), ctx.empty((3 * nbytes,), np.uint8)

        def three(name, Wp, gWp, gm):
            return (lambda: ctx.call(name + "fwd", x.ptr, Wp.ptr, b.ptr, y.ptr, *gm, act, prm),
                    lambda: ctx.call(name + "dgrad", dz.ptr, Wp.ptr, dx.ptr, *gm, pa.ptr, act, prm),
                    lambda: ctx.call(name + "wgrad", x.ptr, dz.ptr, gWp.ptr, gb.ptr, *gm))
        for op, tensors, f_gr, f_dense in zip(("fwd", "dgrad", "wgrad"), (2, 3, 2), three(ops_, W, gW, geom),
                                              three(dn, Wd, gWd, dgeom)):
            moved = tensors * nbytes               # d2d reads half of it and writes half of it
            (u_gr, u_cp, u_dn), spread = trio((f_gr, lambda: ctx.call("tn_d2d", dst.ptr, src.ptr, moved // 2), f_dense))
            print("%-9s %-16s %-6s %9.2f %6.1f%% %9.2f %9.2f %8.2f %8.2f %7.1f" % (
                dtype, "%d,%d,%d,%d" % (N, C, S, g), op, u_gr, 100 * spread, u_cp, u_dn, u_gr / u_cp, u_gr / u_dn, moved / 1e6))
        del x, y, dz, dx, pa, src, dst

if not args.no_net:
    with open(os.path.join(ROOT, "params", "cifar_grp.prms")) as fh:
        prms = ast.literal_eval(fh.read())
    prms["layers"][0][1]["img_sz"] = 32
    B = max(1, prms["training_params"]["BATCH_SZ"] // args.batch_div)
    x = rng.random((NB * B, 3, 32, 32), dtype=np.float32)
    y = rng.integers(0, 10, NB * B).astype(np.int32)
    for dtype in ("bfloat16", "float32"):
        net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"], BATCH_SZ=B, DTYPE=dtype))
        fn = net.get_trin_model(x, y)
        for s in range(60):
            fn.enqueue(s % NB)
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for s in range(args.steps):
                fn.enqueue(s % NB)
            ctx.sync()
            ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
        assert np.isfinite(float(fn.fetch()[0]))
        print("cifar_grp.prms batch %d %-8s %8.4f ms/step (%.4f .. %.4f)" % (B, dtype, statistics.median(ms), min(ms), max(ms)))
