#!/usr/bin/env python
"""Timings of the strided PoolLayer ops of the 16-bit conv stack (tn_c8_pool_st_fwd / tn_c8_pool_st_bwd,
theanet_amd/csrc/pools_c8.hip) at 3x3 windows, stride 2, each beside the existing 2x2 stride-2 op on the same tensor
(tn_c8_pool_fwd / tn_c8_pool_bwd, theanet_amd/csrc/pool_c8.hip: the same output side, so the same output bytes), and the
step time of params/cifar_ovl.prms in bfloat16 and float32.

    python tools/bench_pool_st.py [--iters N] [--rounds R] [--dtype f16|bf16] [--steps K] [--reps R] [--no-net]
    python tools/bench_pool_st.py --json          (one arm of tools/ab.py --script: the net alone, one JSON line)

us/launch: HIP events around --iters back-to-back launches after warm-up, one process.  The strided op and the 2x2 op are
measured alternately, --rounds times each; the table gives the median and the run-to-run spread ((max - min) / median) of
each, the achieved bytes per second of each and the ratio of the medians.  Bytes are the algorithmic ones, every tensor
once (window overlap and the backward's repeated reads of y / gout cells come from cache): forward 16 * (cells of x inside
the map + cells of y, pad included: they are written), backward 16 * (cells of x inside the map + 2 * cells of y inside the
map + cells of gin, pad included).  HBM roof: 6.3 TB/s achievable; back-to-back launches on tensors below the 256 MB
Infinity Cache sit in it, so their rates are upper bounds of what a step sees.

The net: ms/step of --steps enqueued steps (host clock around a loop that ends in a synchronise; median of --reps after a
warm-up in which the step plan records and starts replaying).  --json: DTYPE from the environment variable
BENCH_POOL_ST_DTYPE (default bfloat16) and the file from BENCH_POOL_ST_PRMS (default cifar_ovl.prms), so that an arm of
tools/ab.py is an environment."""
import argparse
import ast
import copy
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theanet_amd import NeuralNet  # noqa: E402
from theanet_amd.device import c8_pool_pitch, get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", choices=("f16", "bf16"), default="bf16")
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch-div", type=int, default=1, help="divide the batch sizes (a rehearsal without a GPU)")
ap.add_argument("--no-net", action="store_true")
ap.add_argument("--json", action="store_true")
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
HBM = 6.3e12
NB = 4


def time_net(prms_name, dtype):
    with open(os.path.join(ROOT, "params", prms_name)) as fh:
        prms = ast.literal_eval(fh.read())
    prms["layers"][0][1]["img_sz"] = 32
    B = max(1, prms["training_params"]["BATCH_SZ"] // args.batch_div)
    tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=B, DTYPE=dtype)
    rng = np.random.default_rng(1)
    x = rng.random((NB * B, 3, 32, 32), dtype=np.float32)
    y = rng.integers(0, 10, NB * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), tr)
    fn = net.get_trin_model(x, y)
    for s in range(60):
        fn.enqueue(s % NB)
    ctx.sync()
    ms = []
    for _ in range(args.reps):
        ctx.sync()
        t0 = time.perf_counter()
        for s in range(args.steps):
            fn.enqueue(s % NB)
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    cost = float(fn.fetch()[0])
    assert np.isfinite(cost), cost
    sides = [l.out_sz for l in net.tr_layers if type(l).__name__ == "PoolLayer"]
    return statistics.median(ms), min(ms), max(ms), sides


if args.json:
    name = os.environ.get("BENCH_POOL_ST_PRMS") or "cifar_ovl.prms"
    dtype = os.environ.get("BENCH_POOL_ST_DTYPE") or "bfloat16"
    ms, lo, hi, sides = time_net(name, dtype)
    print(json.dumps({"case": "%s %s" % (name, dtype), "ms_per_step": ms, "min": lo, "max": hi, "pooled_sides": sides}))
    sys.exit(0)


def timeit(fn, iters):
    for _ in range(10):
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
    return ms.value * 1e3 / iters


def pair(f_st, f_22):
    """Alternating rounds of both: (median, spread) of each."""
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timeit(f_st, args.iters))
        b.append(timeit(f_22, args.iters))
    return [(statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for v in (a, b)]


# (N, C, S, pitch): the two PoolLayers of cifar_ovl.prms at its batch size, and wide6's first maps; window 3, stride 2
SHAPES = [(2048, 32, 32, 32), (2048, 64, 16, 16), (128, 64, 64, 64)]
ctx.call("tn_set_matmul_dtype", *((2, 1.0) if args.dtype == "bf16" else (1, 4096.0)))
rng = np.random.default_rng(0)
print("dtype %s, %d launches per measurement, %d alternating rounds" % (args.dtype, args.iters, args.rounds))
print("%-16s %-4s %9s %7s %7s %9s %7s %7s %7s %8s" % ("N,C,S,pitch", "op", "3/2 us", "spread", "TB/s", "2/2 us", "spread",
                                                     "TB/s", "ratio", "MB"))
for N, C, S, P in SHAPES:
    N = max(1, N // args.batch_div)
    p, st = 3, 2
    So = (S - 1 - p + st) // st + 1
    assert So == S // 2                       # the 2x2 pool of an even map has the same output side
    Po, C8 = c8_pool_pitch(So), (C + 7) // 8
    geom_st, geom_22 = (N, C, S, P, p, st, So, Po), (N, C, S, P, 2, So, Po)
    assert lib.tn_c8_pool_st_supported(*geom_st) and lib.tn_c8_pool_supported(*geom_22)
    # patterns 0x3000 .. 0x3fff: positive, finite and with many ties in either element type; pad cells zero
    xr = np.zeros((N, C8, P, P, 8), np.uint16)
    xr[:, :, :S, :S] = rng.integers(0x3000, 0x4000, (N, C8, S, S, 8), dtype=np.uint16) & 0xfff0
    x = ctx.array(xr)
    y_st, y_22 = ctx.empty((N, C8, Po, Po, 8), np.uint16), ctx.empty((N, C8, Po, Po, 8), np.uint16)
    g = ctx.array(np.full((N, C8, Po, Po, 8), 0x3c00, np.uint16))
    gin = ctx.empty((N, C8, P, P, 8), np.uint16)
    del xr
    ctx.call("tn_c8_pool_st_fwd", x.ptr, y_st.ptr, *geom_st)
    ctx.call("tn_c8_pool_fwd", x.ptr, y_22.ptr, *geom_22)

    def fwd_st():
        ctx.call("tn_c8_pool_st_fwd", x.ptr, y_st.ptr, *geom_st)

    def fwd_22():
        ctx.call("tn_c8_pool_fwd", x.ptr, y_22.ptr, *geom_22)

    def bwd_st():
        ctx.call("tn_c8_pool_st_bwd", x.ptr, y_st.ptr, g.ptr, gin.ptr, *geom_st)

    def bwd_22():
        ctx.call("tn_c8_pool_bwd", x.ptr, y_22.ptr, g.ptr, gin.ptr, *geom_22)

    pl = N * C8
    ops = (("fwd", fwd_st, fwd_22, 16 * pl * (S * S + Po * Po)), ("bwd", bwd_st, bwd_22, 16 * pl * (S * S + 2 * So * So + P * P)))
    for op, f_st, f_22, nbytes in ops:
        (u_st, s_st), (u_22, s_22) = pair(f_st, f_22)
        print("%-16s %-4s %9.2f %6.1f%% %7.2f %9.2f %6.1f%% %7.2f %7.2f %8.1f" % (
            "%d,%d,%d,%d" % (N, C, S, P), op, u_st, 100 * s_st, nbytes / (u_st * 1e-6) / 1e12, u_22, 100 * s_22,
            nbytes / (u_22 * 1e-6) / 1e12, u_st / u_22, nbytes / 1e6))
    del x, y_st, y_22, g, gin

if not args.no_net:
    for dtype in ("bfloat16", "float32"):
        ms, lo, hi, sides = time_net("cifar_ovl.prms", dtype)
        print("cifar_ovl.prms batch %d %-8s %8.4f ms/step (%.4f .. %.4f), pooled sides %s" % (
            max(1, 2048 // args.batch_div), dtype, ms, lo, hi, sides))
