#!/usr/bin/env python
"""Timings of an output head on the 16-bit conv stack (STACK_HEAD 'any'; theanet_amd/csrc/head_c8.hip): the head's ops at
the shapes of the nets, and the whole training step of params/cifar_head.prms.

    python tools/bench_c8_head.py [--dtype bf16|f16|f32] [--what op|step] [--shape B,C,HW,n_out] [--prms cifar_head.prms]
                                  [--batch 2048] [--iters N] [--json]

The route is the library's: TN_C8_HEAD unset / 1 = the head kernels (op: tn_c8_head_softmax_nll, ONE launch), TN_C8_HEAD=0 =
the dense family + the row kernel (op: tn_c8_fcg_fwd + tn_softmax_nll, three launches).  Compare the two with tools/ab.py's
interleaved arms and its A/A control:

    python tools/ab.py --script tools/bench_c8_head.py --args "--json --what op --dtype bf16 --shape 2048,128,16,10" "" "TN_C8_HEAD=0"
    python tools/ab.py --script tools/bench_c8_head.py --args "--json --what step --dtype bf16" "" "TN_C8_HEAD=0"

--what op: us per head forward (HIP events around --iters back-to-back calls, after warm-up).  --what step: ms per training
step of --prms at --batch on synthetic data (--dtype f32: the same net on the fp32 kernels, for the cost of the feature in
context; --prms cifar_gap.prms: the net with the MeanLayer in front of the head).  --json: the last line is one JSON
object with "ms_per_step" (what tools/ab.py reads)."""
import argparse
import ast
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theanet_amd import NeuralNet  # noqa: E402
from theanet_amd.device import bf16_bits, get_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=("f16", "bf16", "f32"), default="bf16")
ap.add_argument("--what", choices=("op", "step"), default="op")
ap.add_argument("--shape", default="2048,128,16,10")
ap.add_argument("--prms", default="cifar_head.prms")
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--json", action="store_true")
args = ap.parse_args()
ctx = get_context()
lib = ctx.lib
rng = np.random.default_rng(0)
DTYPES = {"f16": "float16", "bf16": "bfloat16", "f32": "float32"}


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
    return ms.value / iters


def bench_op():
    assert args.dtype != "f32", "--what op times the 16-bit head ops"
    B, C, HW, N = map(int, args.shape.split(","))
    Kc = (C + 7) // 8 * HW * 8
    v = rng.standard_normal((B, Kc)).astype(np.float32)
    x = ctx.array(bf16_bits(v) if args.dtype == "bf16" else v.astype(np.float16).view(np.uint16))
    W = ctx.array((rng.standard_normal((C * HW, N)) / np.sqrt(C * HW)).astype(np.float32))
    b = ctx.array(np.zeros(N, np.float32))
    y = ctx.array(rng.integers(0, N, B).astype(np.int32))
    z, lp, dz = ctx.empty((B, N)), ctx.empty((B, N)), ctx.empty((B, N))
    rl, rp, pr = ctx.empty((B,)), ctx.empty((B,)), ctx.empty((B,), np.int32)
    ctx.call("tn_set_matmul_dtype", *((2, 1.0) if args.dtype == "bf16" else (1, 4096.0)))
    rows = (y.ptr, 0, None, lp.ptr, rl.ptr, pr.ptr, rp.ptr, dz.ptr)
    if lib.tn_c8_head_supported(B, C, HW, N):
        route = "tn_c8_head_softmax_nll"

        def fn():
            ctx.call("tn_c8_head_softmax_nll", x.ptr, W.ptr, b.ptr, z.ptr, B, C, HW, N, *rows, 1.0 / B)
    else:
        route = "tn_c8_fcg_fwd + tn_softmax_nll"

        def fn():
            ctx.call("tn_c8_fcg_fwd", x.ptr, W.ptr, b.ptr, z.ptr, B, C, HW, N, 0, 0.0, None)
            ctx.call("tn_softmax_nll", z.ptr, *rows, B, N, 1.0 / B)
    ms = timeit(fn, args.iters or 2000)
    print("%s  head forward at (%s): %s  %.2f us" % (args.dtype, args.shape, route, ms * 1e3))
    return ms, route


def bench_step():
    with open(os.path.join(ROOT, "params", args.prms)) as fh:
        prms = ast.literal_eval(fh.read())
    B, img = args.batch, 32
    prms["layers"][0][1]["img_sz"] = img
    tp = dict(prms["training_params"], BATCH_SZ=B, DTYPE=DTYPES[args.dtype], STACK_HEAD="any")
    x = rng.random((4 * B, 3, img, img)).astype(np.float32)
    y = rng.integers(0, 10, 4 * B).astype(np.int32)
    net = NeuralNet(prms["layers"], tp)
    head = net.tr_layers[-1]
    route = "fp32" if head.c8 is None else "head kernels" if head.c8_head else head.c8_fc
    fn = net.get_trin_model(x, y)
    iters = args.iters or 200
    for s in range(30):
        fn.enqueue(s % 4)
    fn.fetch()
    ctx.sync()
    t0 = time.perf_counter()
    for s in range(iters):
        fn.enqueue(s % 4)
    cost = fn.fetch()[0]
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    assert np.isfinite(cost)
    print("%s  %s at batch %d, head on %s: %.4f ms/step" % (args.dtype, args.prms, B, route, ms))
    return ms, route


ms, route = bench_op() if args.what == "op" else bench_step()
if args.json:
    print(json.dumps({"ms_per_step": ms, "what": args.what, "dtype": args.dtype, "route": route}))
