#!/usr/bin/env python
"""What a distortion field per image (ElasticLayer 'per_image'; DESIGN.md section 4.9, tn_elastic_apply_img) costs a
training step against the field shared by the minibatch.

    python tools/bench_elastic_img.py [--steps K] [--reps R] [--only NAME] [--json] [--batch-div D]

Cases: params/mnist.prms at batch 4096 in float32, params/mnist_c16.prms (its own batch, 512, and bfloat16) and
params/cifar_like.prms (its own batch, 2048) in bfloat16 -- default schedule.  Per case three nets are built, the shared field
twice (A and the A/A control A') and the per-image field (B), and timed INTERLEAVED: every repetition runs --steps
enqueued steps of A, B and A' in turn (a few untimed steps first, so that the net that takes the context over has its
pipeline full; host clock around a loop that ends in a synchronise).  Reported: median ms/step of each arm, B - A, and
the A/A resolution |A' - A| -- a difference below it is not one."""
import argparse
import ast
import copy
import json
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
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="", help="substring of a case name")
ap.add_argument("--json", action="store_true")
ap.add_argument("--batch-div", type=int, default=1, help="divide the batch sizes (a rehearsal without a GPU)")
args = ap.parse_args()
ctx = get_context()
NB = 5         # coprime with the plan periods (1, 2, 4): every recorded phase sees more than one minibatch

# name, spec, batch (None: the file's), channels, image side, DTYPE (None: the file's)
CASES = (("mnist.prms batch 4096 float32", "mnist.prms", 4096, 1, 28, "float32"),
         ("mnist_c16.prms bfloat16", "mnist_c16.prms", None, 1, 28, None),
         ("cifar_like.prms bfloat16", "cifar_like.prms", None, 3, 32, "bfloat16"))


def build(prms_name, B, ch, img, dtype, per_image):
    with open(os.path.join(ROOT, "params", prms_name)) as fh:
        prms = ast.literal_eval(fh.read())
    layers = copy.deepcopy(prms["layers"])
    layers[0][1]["img_sz"] = img
    if per_image:
        layers[0][1]["per_image"] = True
    B = max(1, (B or prms["training_params"]["BATCH_SZ"]) // args.batch_div)
    tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=B)
    if dtype:
        tr["DTYPE"] = dtype
    rng = np.random.default_rng(1)
    x = rng.random((NB * B, ch, img, img), dtype=np.float32)
    y = rng.integers(0, 10, NB * B).astype(np.int32)
    net = NeuralNet(layers, tr)
    fn = net.get_trin_model(x, y)
    for s in range(60):                 # the step plan watches, records and starts replaying
        fn.enqueue(s % NB)
    ctx.sync()
    return net, fn, B


def timed(fn):
    for s in range(8):
        fn.enqueue(s % NB)
    ctx.sync()
    t0 = time.perf_counter()
    for s in range(args.steps):
        fn.enqueue(s % NB)
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def how(fn):
    seq = getattr(fn, "_seq", None)
    pl = (seq or fn)._plan
    return "%s%s" % (type(seq or fn).__name__, ", replayed" if pl is not None and pl.ready else ", interpreted")


out = {}
for name, prms_name, B, ch, img, dtype in CASES:
    if args.only not in name:
        continue
    arms = {"A": build(prms_name, B, ch, img, dtype, False), "B": build(prms_name, B, ch, img, dtype, True),
            "A'": build(prms_name, B, ch, img, dtype, False)}
    ms = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, (net, fn, _) in arms.items():
            ms[k].append(timed(fn))
    for k, (net, fn, _) in arms.items():
        assert np.isfinite(float(fn.fetch()[0])), (name, k)
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"batch": arms["A"][2], "ms_shared": med["A"], "ms_per_image": med["B"], "ms_shared_control": med["A'"],
           "diff_ms": med["B"] - med["A"], "diff_pct": 100 * (med["B"] / med["A"] - 1), "aa_resolution_ms": abs(med["A'"] - med["A"]),
           "how_shared": how(arms["A"][1]), "how_per_image": how(arms["B"][1]),
           "c8_direct": arms["B"][0].tr_layers[0]._c8_consumer is not None}
    out[name] = row
    if not args.json:
        print("%-36s B %5d  shared %8.4f ms/step (%s) | per image %8.4f (%s) | %+.4f ms = %+.2f %% | A/A %.4f ms" % (
            name, row["batch"], row["ms_shared"], row["how_shared"], row["ms_per_image"], row["how_per_image"], row["diff_ms"],
            row["diff_pct"], row["aa_resolution_ms"]))
    del arms
if args.json:
    print(json.dumps(out))
