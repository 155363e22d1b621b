#!/usr/bin/env python
"""The C-ABI call trace of a net's life, as text: construction, training steps (the interpreted ones, the ones a StepPlan
watches, a few replayed ones) and one test-function call.  Two builds whose traces are byte-identical make the same calls
with the same arguments -- what a host-side refactor has to show.

    python tools/steptrace.py --prms cifar_like.prms --img 32 --batch 16 --dtype bfloat16 --out trace.txt

One line per call through ``ctx.lib`` (``Context.call`` goes through it, and so do the capability queries, tn_free and
tn_net_step): name, arguments, result.  Scalars are written exactly, floats by bit pattern.  A pointer into something the
library handed out -- device memory, page-locked host memory, the context, an event, a plan -- is written as the index of
that allocation in order of appearance plus the offset into it, so the aliasing pattern is compared and the addresses
are not; an allocation that has been freed is forgotten, so an address the allocator hands out again is a new object.
Pageable host memory (numpy arrays: staging copies, tables) is written as ``host``: such arrays come and go with the
interpreter's heap, and whether two of them share an address says nothing about the calls.  The entries of a step plan
(tn_net_plan_add) are decoded the same way.  The last line is a SHA-256 of every weight tensor after the steps (not part
of the recording).

``--drive`` chooses how the steps are issued: ``enqueue`` (nothing read back), ``call`` (the drop-in ``fn(i)``: outputs sent
ahead, the cost summed for them) or ``step_cost`` (``fn.step_cost(i)``, with ``drain_costs()`` after every tenth step and at
the end: the cost ring).  The costs that come back are part of the trace, as ``cost <step number> f:<bits>`` lines where
they were returned.  The data-parallel and pipelining switches (TN_DP_FORCE, TN_DP_OVERLAP, TN_PIPELINE, TN_DP_BUCKETS)
need no option: the net reads them from the environment, so set them for the run to be traced.

``trace(layers, training_params, ...)`` does the same for a net given as Python objects."""
import argparse
import ast
import ctypes
import gc
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = 6 + 12 + 6          # StepPlan.WARM, the steps it records, replayed steps
NBATCH = 5                  # minibatches in the dataset: odd, so that every phase of a plan sees more than one
DRIVES = ("enqueue", "call", "step_cost")
DRAIN_EVERY = 10            # --drive step_cost: drain_costs() after this many steps (train.py does at the end of an epoch)


class _Recorder:
    """Stands in for ``ctx.lib``: every entry point looked up on it logs its call."""

    # entry points that hand out / take back something pointers are named after: (argument of the handle, of its size)
    _NEW = {"tn_alloc": (2, 1), "tn_host_alloc": (2, 1), "tn_event_create": (1, None), "tn_net_plan_create": (1, None)}
    _DEL = ("tn_free", "tn_host_free", "tn_event_destroy", "tn_net_plan_destroy")

    def __init__(self, lib, signatures, lines, ctx_handle):
        self._lib, self._sig, self._lines = lib, signatures, lines
        self._live, self._count = {ctx_handle.value: (0, 1)}, 1          # base address -> (index, bytes)

    def _ptr(self, v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if not v:
            return "null"
        for base, (idx, size) in self._live.items():
            if base <= v < base + size:
                return "p%d" % idx + ("+%d" % (v - base) if v != base else "")
        return "host"

    def _arg(self, t, a):
        if t is ctypes.c_float:
            return "f:%08x" % int(np.float32(a).view(np.uint32))
        if t is ctypes.c_double:
            return "d:%016x" % int(np.float64(a).view(np.uint64))
        if hasattr(a, "_obj"):                                  # byref(): an output, read after the call
            return "out:" + (self._ptr(a._obj) if isinstance(a._obj, ctypes.c_void_p) else "value")
        if t is ctypes.c_void_p:
            return "table" if isinstance(a, ctypes.Array) else self._ptr(a)
        if isinstance(a, bytes):
            return repr(a)
        if a is None:
            return "null"
        if isinstance(a, (int, np.integer)):
            return str(int(a))
        return "host"                                           # string buffers

    def _plan_entry(self, args):
        """tn_net_plan_add(h, plan, name, n, kinds, values, strides): the planned call, decoded by its own signature."""
        name, n = args[2].decode(), args[3]
        types = self._sig[name][1][1:]
        vals = []
        for t, k, v, s in zip(types, args[4][:n], args[5][:n], args[6][:n]):
            vals.append("%s%s" % (self._ptr(v) if t is ctypes.c_void_p else "%d:%x" % (k, v), "+i*%d" % s if s else ""))
        return "%s %s(%s)" % (self._ptr(args[1]), name, ", ".join(vals))

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        types = self._sig[name][1]

        def logged(*args):
            rc = fn(*args)
            if name in self._NEW and rc == 0:
                out, size = self._NEW[name]
                self._live[args[out]._obj.value] = (self._count, max(int(args[size]), 1) if size else 1)
                self._count += 1
            if name == "tn_net_plan_add":
                text = self._plan_entry(args)
            else:
                text = ", ".join(self._arg(t, a) for t, a in zip(types, args))
            self._lines.append("%s(%s) -> %r" % (name, text, rc))
            if name in self._DEL:
                self._live.pop(args[1].value if isinstance(args[1], ctypes.c_void_p) else args[1], None)
            return rc
        return logged


def _cost_line(k, cost):
    return "cost %d f:%08x" % (k, int(np.float32(cost).view(np.uint32)))


def trace(layers, training_params, channels, img, out=None, steps=STEPS, drive="enqueue"):
    """Builds the net, runs ``steps`` training steps (issued as ``drive`` says) and one test call with recording on; returns
    the trace's lines, the weight hash last (and writes them to ``out``)."""
    assert drive in DRIVES, drive
    from theanet_amd import NeuralNet, _lib
    from theanet_amd.device import get_context
    ctx = get_context()
    lines = []
    gc.collect()                # when the cycle collector frees device arrays is the interpreter's business: not while recording
    gc.disable()
    real, ctx.lib, ctx._fns = ctx.lib, _Recorder(ctx.lib, _lib.SIGNATURES, lines, ctx.h), {}
    try:
        B = training_params["BATCH_SZ"]
        rng = np.random.RandomState(1)
        x = rng.rand(NBATCH * B, channels, img, img).astype(np.float32)
        y = rng.randint(0, 10, NBATCH * B).astype(np.int32)
        net = NeuralNet(layers, dict(training_params))
        fn = net.get_trin_model(x, y)
        for s in range(steps):
            if drive == "enqueue":
                fn.enqueue(s % NBATCH)
            elif drive == "call":
                lines.append(_cost_line(s, fn(s % NBATCH)[0]))
            else:
                lines.extend(_cost_line(k, c) for k, c in fn.step_cost(s % NBATCH))
                if (s + 1) % DRAIN_EVERY == 0 or s + 1 == steps:
                    lines.extend(_cost_line(k, c) for k, c in fn.drain_costs())
        ctx.sync()
        net.get_test_model(x, y)(0)
    finally:
        ctx.lib, ctx._fns = real, {}
        gc.enable()
    h = hashlib.sha256()
    for lyr in net.tr_layers:
        for w in lyr.get_wts():
            h.update(np.ascontiguousarray(w).tobytes())
    lines.append("weights sha256 " + h.hexdigest())
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--prms", required=True, help="a file under params/")
    ap.add_argument("--img", type=int, default=None, help="image side (default: 32 for 3-channel nets, else 28)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float16", "bfloat16"))
    ap.add_argument("--matmul", default=None, help="MATMUL training param (default: the file's)")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--drive", default="enqueue", choices=DRIVES, help="how the steps are issued")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    with open(os.path.join(ROOT, "params", args.prms)) as fh:
        prms = ast.literal_eval(fh.read())
    first = prms["layers"][0][1]
    channels = first.get("num_maps", 1)
    first["img_sz"] = args.img or (32 if channels == 3 else 28)
    tp = dict(prms["training_params"], SEED=555555, BATCH_SZ=args.batch, DTYPE=args.dtype)
    if args.matmul:
        tp["MATMUL"] = args.matmul
    lines = trace(prms["layers"], tp, channels, first["img_sz"], args.out, args.steps, args.drive)
    print("%s %s %s: %d lines, %s" % (args.prms, args.dtype, args.drive, len(lines) - 1, lines[-1]))


if __name__ == "__main__":
    main()
