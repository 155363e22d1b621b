#!/usr/bin/env python
"""Timings of the narrow-group conv ops (tn_c8_gconv_*'s narrow branch, theanet_amd/csrc/gconv_c8_narrow.hip) at the three
grouped layers of params/cifar_grpn.prms -- batch 2048, bfloat16, 3x3 'same', 4 maps a group: 32 maps of 32x32 in 8 groups,
64 of 16x16 in 16, 128 of 8x8 in 32 -- by tools/bench_gconv.py's method, each product against two things this family does
not touch, on the same tensors in the same run:

  dense  the dense 3x3 'same' layer of the stack on (K, C, 3, 3) weights with the groups on the block diagonal (C / 4 times
         the products): tn_c8_conv_*, the family a dense 3x3 'same' ConvLayer takes -- what a user runs without the feature;
  dw     tn_c8_dwconv_* on the same tensors: the same activation bytes, the bandwidth yardstick.

    python tools/bench_gconv_narrow.py [--iters N] [--rounds R] [--steps K] [--reps R] [--batch-div D] [--no-net]

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The three are measured
alternately, --rounds times each; the table gives the median of each, the A/A spread of the narrow op ((max - min) /
median over the rounds) and the two ratios.  Back-to-back launches on tensors below the 256 MB Infinity Cache sit in it,
so rates are upper bounds of what a step sees.  Then ms/step of cifar_grpn.prms and cifar_grp.prms in bfloat16 (host clock
around --steps enqueued steps ending in a synchronise, median of --reps)."""
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
print("%-16s %-6s %9s %7s %9s %9s %10s %10s" % ("N,C,S,g", "op", "narrow us", "spread", "dense us", "dw us", "narrow/dense",
                                                "narrow/dw"))
rng = np.random.default_rng(0)
ctx.set_matmul_dtype("bfloat16", 1.0)
for N, C, S in ((2048, 32, 32), (2048, 64, 16), (2048, 128, 8)):
    N, g = max(1, N // args.batch_div), C // 4
    shape = (N, C // 8, S, S, 8)
    mk = lambda: ctx.array((rng.integers(0x3c00, 0x3f80, shape, dtype=np.uint16) & 0xff80))      # bf16 in [.5, 1)
    geom, wgeom = (N, C, S, S, C, g, 3, 1, 1, S, S), (N, C, S, S, 3, 1, 1, S, S)
    assert lib.tn_c8_gconv_supported(*geom) and lib.tn_c8_dwconv_supported(*wgeom)
    assert lib.tn_c8_conv_supported(N, C, S, S, C, 3, 1, 1) and lib.tn_c8_conv_wgrad_supported(N, C, S, S, C)
    x, y, dz, dx, pa = mk(), mk(), mk(), mk(), mk()
    w = (rng.standard_normal((C, 4, 3, 3)) / 3).astype(np.float32)
    W, Wd, Ww = ctx.array(w), ctx.array(block_diagonal(w, g)), ctx.array(np.ascontiguousarray(w[:, :1]))
    b = ctx.array(np.zeros(C, np.float32))
    gW, gWd, gWw, gb = ctx.empty(w.shape), ctx.empty((C, C, 3, 3)), ctx.empty((C, 1, 3, 3)), ctx.empty((C,))
    narrow = (lambda: ctx.call("tn_c8_gconv_fwd", x.ptr, W.ptr, b.ptr, y.ptr, *geom, act, prm),
              lambda: ctx.call("tn_c8_gconv_dgrad", dz.ptr, W.ptr, dx.ptr, *geom, pa.ptr, act, prm),
              lambda: ctx.call("tn_c8_gconv_wgrad", x.ptr, dz.ptr, gW.ptr, gb.ptr, *geom))
    dense = (lambda: ctx.call("tn_c8_conv_fwd", x.ptr, Wd.ptr, b.ptr, y.ptr, None, N, C, S, S, C, act, prm, 0, None),
             lambda: ctx.call("tn_c8_conv_dgrad", dz.ptr, Wd.ptr, dx.ptr, N, C, S, S, C, pa.ptr, act, prm, 0, None, None),
             lambda: ctx.call("tn_c8_conv_wgrad", x.ptr, dz.ptr, gWd.ptr, gb.ptr, N, C, S, S, C, 0, None))
    dw = (lambda: ctx.call("tn_c8_dwconv_fwd", x.ptr, Ww.ptr, b.ptr, y.ptr, *wgeom, act, prm),
          lambda: ctx.call("tn_c8_dwconv_dgrad", dz.ptr, Ww.ptr, dx.ptr, *wgeom, pa.ptr, act, prm),
          lambda: ctx.call("tn_c8_dwconv_wgrad", x.ptr, dz.ptr, gWw.ptr, gb.ptr, *wgeom))
    for op, f_n, f_d, f_w in zip(("fwd", "dgrad", "wgrad"), narrow, dense, dw):
        (u_n, u_d, u_w), spread = trio((f_n, f_d, f_w))
        print("%-16s %-6s %9.2f %6.1f%% %9.2f %9.2f %10.2f %10.2f" % ("%d,%d,%d,%d" % (N, C, S, g), op, u_n, 100 * spread, u_d,
                                                                     u_w, u_n / u_d, u_n / u_w))
    del x, y, dz, dx, pa

if not args.no_net:
    for name in ("cifar_grpn.prms", "cifar_grp.prms"):
        with open(os.path.join(ROOT, "params", name)) as fh:
            prms = ast.literal_eval(fh.read())
        prms["layers"][0][1]["img_sz"] = 32
        B = max(1, prms["training_params"]["BATCH_SZ"] // args.batch_div)
        x = rng.random((NB * B, 3, 32, 32), dtype=np.float32)
        y = rng.integers(0, 10, NB * B).astype(np.int32)
        net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"], BATCH_SZ=B, DTYPE="bfloat16"))
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
        print("%s batch %d bfloat16 %8.4f ms/step (%.4f .. %.4f)" % (name, B, statistics.median(ms), min(ms), max(ms)))
        del net, fn
