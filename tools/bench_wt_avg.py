#!/usr/bin/env python
"""What averaged weights (training param WT_AVG; DESIGN.md section 4.8, tn_avg_net) cost a training step.

    python tools/bench_wt_avg.py [--steps K] [--reps R] [--only NAME] [--wt-avg D] [--json]

ms/step of --steps enqueued steps (host clock around a loop that ends in a synchronise; median of --reps, after a warm-up
in which the step plan watches, records and starts replaying) of
  * params/mnist.prms at batch 4096, float32;
  * params/wide6.prms (64 x 64 x 3) at batch 128, bfloat16;
each with WT_AVG on (--wt-avg, default .999) and off, which training function ran, and the launch's share on paper (12
bytes per averaged weight).  Uses the public training interface only, so the same file times an older tree, which knows
no WT_AVG: there only the off column is timed.

One arm of an interleaved A/B (tools/ab.py --script tools/bench_wt_avg.py, which wants one JSON line with "ms_per_step"):
--json with --only selecting ONE case prints that case alone, WT_AVG taken from the environment variable BENCH_WT_AVG
(unset, empty or 0: off) so that an arm is an environment like every arm of that tool."""
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
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="", help="substring of a case name")
ap.add_argument("--wt-avg", type=float, default=.999)
ap.add_argument("--json", action="store_true")
ap.add_argument("--batch-div", type=int, default=1, help="divide the batch sizes (a rehearsal without a GPU)")
args = ap.parse_args()
ctx = get_context()
NB = 4
KNOWS_WT_AVG = hasattr(NeuralNet, "get_avg_wts")

CASES = (("mnist.prms batch 4096 float32", "mnist.prms", 4096, 1, 28, "float32"),
         ("wide6.prms batch 128 bfloat16", "wide6.prms", 128, 3, 64, "bfloat16"))


def prms_of(name):
    with open(os.path.join(ROOT, "params", name)) as fh:
        return ast.literal_eval(fh.read())


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
    n_avg = sum(a.size for avs in (getattr(net, "_avg", None) or ()) for a in (avs or ()))
    return statistics.median(ms), min(ms), max(ms), how, n_avg


def run_case(name, prms_name, B, ch, img, dtype, d):
    prms = prms_of(prms_name)
    prms["layers"][0][1]["img_sz"] = img
    B = max(1, B // args.batch_div)
    tr = dict(prms["training_params"], SEED=555555, BATCH_SZ=B, DTYPE=dtype)
    if d:
        tr["WT_AVG"] = d
    rng = np.random.default_rng(1)
    x = rng.random((NB * B, ch, img, img), dtype=np.float32)
    y = rng.integers(0, 10, NB * B).astype(np.int32)
    return time_net(prms["layers"], tr, x, y)


picked = [c for c in CASES if args.only in c[0]]
if args.json and len(picked) == 1:
    d = float(os.environ.get("BENCH_WT_AVG") or 0)
    assert not d or KNOWS_WT_AVG, "this tree knows no WT_AVG"
    ms, lo, hi, how, n_avg = run_case(*picked[0], d)
    print(json.dumps({"case": picked[0][0], "wt_avg": d, "ms_per_step": ms, "min": lo, "max": hi, "how": how,
                      "averaged_weights": n_avg}))
    sys.exit(0)

out = {}
for case in picked:
    off = run_case(*case, 0)
    row = {"ms_off": off[0], "min_off": off[1], "max_off": off[2], "how_off": off[3]}
    if KNOWS_WT_AVG:
        on = run_case(*case, args.wt_avg)
        row.update(ms_on=on[0], min_on=on[1], max_on=on[2], how_on=on[3], averaged_weights=on[4],
                   mbytes_per_step=12e-6 * on[4])
    out[case[0]] = row
    if not args.json:
        line = "%-32s off %8.4f ms/step (%.4f .. %.4f)  %s" % (case[0], off[0], off[1], off[2], off[3])
        if KNOWS_WT_AVG:
            line += " | WT_AVG %g: %8.4f (%.4f .. %.4f)  %s, %+.2f %%, %.1f MB per step" % (
                args.wt_avg, on[0], on[1], on[2], on[3], 100 * (on[0] / off[0] - 1), row["mbytes_per_step"])
        print(line)
if args.json:
    print(json.dumps(out))
