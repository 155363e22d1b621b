#!/usr/bin/env python
"""Timings of the dilated conv ops (tn_c8_dilconv_* on the 16-bit conv stack, tn_dilconv_* in float32;
theanet_amd/csrc/dilconv.h) at the two dilated layers of params/cifar_dil.prms -- batch 2048, 3x3 'same' on 16x16 maps:
32 -> 64 maps at d = 2, 64 -> 128 maps at d = 4 -- by tools/bench_gconv.py's method, each against two things on the same
tensors in the same run:

  d1     the same op at d = 1 (3x3 'same', the same weights): the same products, so the ratio is the cost of the dilated
         access;
  dense  the zero-stuffed dense layer of filter fe = 2 d + 1 a user would otherwise write ((K, C, fe, fe) weights;
         bfloat16: the general family tn_c8_convg_*, float32: tn_conv2d_*): fe fe / 9 times the products.

    python tools/bench_dilconv.py [--iters N] [--rounds R] [--steps K] [--reps R] [--batch-div D] [--no-net]

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The three are measured
alternately, --rounds times each; the table gives the median of each, the A/A spread of the dilated op ((max - min) /
median over the rounds) and the two ratios.  Back-to-back launches on tensors below the 256 MB Infinity Cache sit in it,
so rates are upper bounds of what a step sees.  Then ms/step of cifar_dil.prms in bfloat16 and float32 (host clock around
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


act, prm = 1, .1                           # relu10
S = 16
print("%d launches per measurement, %d alternating rounds" % (args.iters, args.rounds))
print("%-9s %-16s %-6s %9s %7s %9s %9s %8s %9s" % ("dtype", "N,C,K,d", "op", "dil us", "spread", "d1 us", "dense us", "dil/d1",
                                                 "dil/dense"))
rng = np.random.default_rng(0)
for dtype in ("bfloat16", "float32"):
    ctx.set_matmul_dtype(dtype, 1.0)
    c8 = dtype == "bfloat16"
    for N, C, K, d in ((2048, 32, 64, 2), (2048, 64, 128, 4)):
        N = max(1, N // args.batch_div)
        fe = 2 * d + 1
        if c8:
            mk = lambda m: ctx.array((rng.integers(0x3c00, 0x3f80, (N, m // 8, S, S, 8), dtype=np.uint16) & 0xff80))  # bf16 in [.5, 1)
            dil, one, dns = "tn_c8_dilconv_", "tn_c8_dilconv_", "tn_c8_convg_"
        else:
            mk = lambda m: ctx.array(rng.random((N, m, S, S), dtype=np.float32))
            dil, one, dns = "tn_dilconv_", "tn_dilconv_", "tn_conv2d_"
        g_dil, g_one, g_dns = (N, C, S, S, K, d, 3, 1, d, S, S), (N, C, S, S, K, 1, 3, 1, 1, S, S), (N, C, S, S, K, fe, 1, d, S, S)
        assert getattr(lib, dil + "supported")(*g_dil) and getattr(lib, one + "supported")(*g_one)
        x, pa, dx, y, dz = mk(C), mk(C), mk(C), mk(K), mk(K)
        w = (rng.standard_normal((K, C, 3, 3)) / 3).astype(np.float32)
        wd = np.zeros((K, C, fe, fe), np.float32)
        wd[:, :, ::d, ::d] = w
        W, Wd, b = ctx.array(w), ctx.array(wd), ctx.array(np.zeros(K, np.float32))
        gW, gWd, gb = ctx.empty(w.shape), ctx.empty(wd.shape), ctx.empty((K,))

        def three(name, Wp, gWp, gm):
            return (lambda: ctx.call(name + "fwd", x.ptr, Wp.ptr, b.ptr, y.ptr, *gm, act, prm),
                    lambda: ctx.call(name + "dgrad", dz.ptr, Wp.ptr, dx.ptr, *gm, pa.ptr, act, prm),
                    lambda: ctx.call(name + "wgrad", x.ptr, dz.ptr, gWp.ptr, gb.ptr, *gm))
        for op, f_dil, f_one, f_dns in zip(("fwd", "dgrad", "wgrad"), three(dil, W, gW, g_dil), three(one, W, gW, g_one),
                                           three(dns, Wd, gWd, g_dns)):
            (u_dil, u_one, u_dns), spread = trio((f_dil, f_one, f_dns))
            print("%-9s %-16s %-6s %9.2f %6.1f%% %9.2f %9.2f %8.2f %9.2f" % (
                dtype, "%d,%d,%d,%d" % (N, C, K, d), op, u_dil, 100 * spread, u_one, u_dns, u_dil / u_one, u_dil / u_dns))
        del x, y, dz, dx, pa

if not args.no_net:
    with open(os.path.join(ROOT, "params", "cifar_dil.prms")) as fh:
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
        print("cifar_dil.prms batch %d %-8s %8.4f ms/step (%.4f .. %.4f)" % (B, dtype, statistics.median(ms), min(ms), max(ms)))
