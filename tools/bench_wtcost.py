#!/usr/bin/env python
"""Timings of training steps of nets with L1 / L2 weight costs (tn_wtcost_net, TN_UPD_PIPE_REG).

    python tools/bench_wtcost.py [--steps K] [--reps R] [--only NAME] [--json]

ms/step of --steps enqueued steps (host clock around a loop that ends in a synchronise; median of --reps, after a warm-up
in which the step plan watches, records and starts replaying) of
  * params/3flat.prms (L2 .001 on its 784 x 1000 layer) at its own batch, 20, and at 4096, float32;
  * params/wide6.prms (64 x 64 x 3, 128 images) with L2 .001 put on its 16384 x 1024 dense layer, float32 and bfloat16;
each next to the same net with the weight costs taken out (what the fast schedules cost without them), and which
training function ran.  Uses the public training interface only, so the same file times an older tree: the A/B of this
commit against its parent runs it once per tree, interleaved (--json: one line for such a driver)."""
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
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="", help="substring of a case name")
ap.add_argument("--json", action="store_true")
ap.add_argument("--batch-div", type=int, default=1, help="divide the batch sizes (a rehearsal without a GPU)")
args = ap.parse_args()
ctx = get_context()
NB = 4


def prms_of(name):
    with open(os.path.join(ROOT, "params", name)) as fh:
        return ast.literal_eval(fh.read())


def cases():
    flat = prms_of("3flat.prms")
    flat["layers"][0][1].update(img_sz=28, num_maps=1)
    wide = prms_of("wide6.prms")
    wide["layers"][0][1]["img_sz"] = 64
    wide["layers"][-2][1]["reg"] = dict(wide["layers"][-2][1]["reg"], L2=.001)
    for name, prms, B, ch, img, n_cls, dtype in (("3flat.prms batch 20 float32", flat, 20, 1, 28, 457, "float32"),
                                                 ("3flat.prms batch 4096 float32", flat, 4096, 1, 28, 457, "float32"),
                                                 ("wide6.prms + L2 batch 128 float32", wide, 128, 3, 64, 10, "float32"),
                                                 ("wide6.prms + L2 batch 128 bfloat16", wide, 128, 3, 64, 10, "bfloat16")):
        if args.only in name:
            yield name, prms, max(1, B // args.batch_div), ch, img, n_cls, dtype


def without_costs(layers):
    layers = copy.deepcopy(layers)
    for _, a in layers:
        if "reg" in a:
            a["reg"] = dict(a["reg"], L1=0., L2=0.)
    return layers


def time_net(layers, tr, x, y):
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
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
    seq = getattr(fn, "_seq", None)
    pl = (seq or fn)._plan
    how = "%s%s" % (type(seq or fn).__name__, ", replayed" if pl is not None and pl.ready else ", interpreted")
    return statistics.median(ms), min(ms), max(ms), how


out = {}
for name, prms, B, ch, img, n_cls, dtype in cases():
    tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=B, DTYPE=dtype)
    rng = np.random.default_rng(1)
    x = rng.random((NB * B, ch, img, img), dtype=np.float32)
    y = rng.integers(0, n_cls, NB * B).astype(np.int32)
    with_c = time_net(prms["layers"], tr, x, y)
    no_c = time_net(without_costs(prms["layers"]), tr, x, y)
    out[name] = {"ms": with_c[0], "min": with_c[1], "max": with_c[2], "how": with_c[3],
                 "ms_without_costs": no_c[0], "how_without_costs": no_c[3]}
    if not args.json:
        print("%-36s %8.4f ms/step (%.4f .. %.4f)  %-28s | without weight costs %8.4f  %s"
              % (name, with_c[0], with_c[1], with_c[2], with_c[3], no_c[0], no_c[3]))
if args.json:
    print(json.dumps(out))
