"""When a data-parallel net all-reduces its flat gradient buffer.  ``plain``: once, between backward pass and update.
``overlap`` (TN_DP_OVERLAP=1): the dense group on top of the net, the tail of the buffer, on the second stream under the conv
blocks' backward.  ``delayed`` (=2): under the whole of the next step, which updates with the previous step's reduced
gradient.  ``pipelined``: two steps in flight (_PipeTrainFn), on the communication stream.  Same weights bit for bit -- and so the
same averaged weights (WT_AVG): the averages' launch follows the update wherever the schedule puts it (the end of
NeuralNet._train_step, behind ``end_sequential``'s delayed update too; _PipeTrainFn._update_for), never this module."""
import ctypes
import os
import sys

import numpy as np

from . import _lib
from .layer import HiddenLayer


class DpSchedule:
    TUNE_PRE, TUNE_WARM, TUNE_STEPS = 32, 8, 24      # settle-in steps, per-leg warm-up, timed

    def __init__(self, net):
        """Every net has one; on a net that is not data-parallel it stays as it is here and does nothing."""
        self.net, self.schedule = net, "plain"
        self.cand = self.bucket = None      # (the dense group's first layer, its offset); pipelined: = cand if its own bucket
        self.split, self.off = None, 0      # overlap is on: = cand
        self.can_delay = self.delayed = False       # the delayed schedule is possible / on
        self.flat_ab = self.grads_ab = self.segs_ab = None      # ... its two flat buffers, their gradient views, segment tables
        self.cur = 0                # ... and the one of the two this step's gradients go to
        self.pending = False        # delayed: the last step's reduced gradient is still to be folded into the velocity
        self.tune = self.tuned_ms = None    # TN_DP_OVERLAP=auto: the tuner's record while timing / {schedule: ms per step}
        self.ar_done_ev = None      # pipelined: recorded behind a step's last collective (set by _PipeTrainFn)
        self._joined = self._bucket_sent = False    # this step: the dense group's gradients have left already

    def prepare(self, slots, host):
        """``slots``: (layer, parameter, offset in the flat buffer) of every tensor; ``host``: the update's segment table."""
        net = self.net
        if not net._dp:
            return
        j = len(net.tr_layers)
        while j > 0 and isinstance(net.tr_layers[j - 1], HiddenLayer):
            j -= 1
        top = [l for l in net.tr_layers[j:] if l.params]
        if 0 < j < len(net.tr_layers) and top and any(l.has_updates() for l in net.tr_layers[:j]):
            self.cand = (j, (top[0].grads[0].ptr - net.flat_grads.ptr) // 4)
            # pipelined schedule: a bucket of its own for the dense group when what is left for the second
            # collective (the conv layers' gradients) is worth one -- mnist.prms: 780 floats, one all-reduce;
            # cifar_like: 93 k + 1.05 M, wide6: 1.15 M + 16.8 M floats, two.  TN_DP_BUCKETS=0/1 overrides.
            want = os.environ.get("TN_DP_BUCKETS", "auto")
            if want == "1" or (want == "auto" and self.cand[1] * 4 >= (64 << 10)):
                self.bucket = self.cand
        # delayed: a second flat buffer (g_{t+1} is produced while G_t is in flight), gradients free of the weights (no L1/L2).
        # Nets with weight costs stay off it: when G_t arrives the weights have moved on, and the L1 / L2 terms of g_t are
        # taken at the weights g_t was computed at -- which this schedule, unlike the single-GPU pipelined one (whose
        # stepping stream still holds them, TN_UPD_PIPE_REG), no longer has.
        self.can_delay = len(host) > 0 and not net._has_wtcost
        if self.can_delay:
            self.flat_ab = [net.flat_grads, net.ctx.zeros(net.flat_grads.shape)]
            self.grads_ab, self.segs_ab = [], [net._d_segs]
            for buf in self.flat_ab:
                self.grads_ab.append({id(lyr): [buf.view(off, p.shape) for l2, p, off in slots if l2 is lyr]
                                      for lyr in net.tr_layers if lyr.params})
            host_b = host.copy()
            host_b['g'] = host['g'] - net.flat_grads.ptr + self.flat_ab[1].ptr
            self.segs_ab.append(net.ctx.array(host_b.view(np.uint8)))
        # which is fastest depends on the node (RCCL latency vs. 18 us of extra launches and joins): with > 1 rank it is MEASURED
        mode = os.environ.get("TN_DP_OVERLAP", "auto" if net.world.size > 1 else "0")
        if (self.cand and mode == "1") or (self.can_delay and mode == "2"):
            self.set_schedule("overlap" if mode == "1" else "delayed")
        elif mode == "auto":
            cands = ["plain"] + (["overlap"] if self.cand else []) + (["delayed"] if self.can_delay else [])
            if len(cands) > 1:
                self.tune = {"k": 0, "ev": {}, "cands": cands, "ms": []}

    def bind(self, cur):
        """Point the layers' gradient views, the cost slot and the update's segment table at flat buffer ``cur``."""
        net = self.net
        if not self.can_delay or net.flat_grads is self.flat_ab[cur]:
            return
        net.flat_grads = self.flat_ab[cur]
        for lyr in net.tr_layers:
            if lyr.params:
                lyr.grads = self.grads_ab[cur][id(lyr)]
        net.d_cost = net.flat_grads.view(net.n_flat - 1, (1,))
        net.tr_layers[-1].d_cost = net.d_cost
        net._d_segs = self.segs_ab[cur]

    def catch_up(self, d_segs, d_step=None, inc=0, which=3):
        """The velocity is one gradient behind, the one table ``d_segs`` names (of a net of this net's layout): fold it in.
        (The delayed schedule's own update is the same launch with a step counter and another ``which``; ``which`` + 4: with
        the segments' L1 / L2 terms at their ``p`` -- the pipelined schedule of a weight-cost net, whose ``p`` is what the
        gradient was taken at.)"""
        net = self.net
        net.ctx.call("tn_sgd_update_net", _lib.TN_UPD_DELAYED, d_segs.ptr, None, net._n_segs, net._max_seg,
                     net.cur_learn_rate.ptr, 1.0, d_step, inc, which, None, 0, 0.0, None)

    def set_schedule(self, name):
        """Switch the schedule between steps (all ranks at the same step index)."""
        if self.delayed and name != "delayed" and self.pending:
            self.net.ctx.call("tn_stream_wait", 0, 1)
            self.catch_up(self.segs_ab[1 - self.cur])
            self.pending = False
        if name != "delayed":
            self.cur = 0
        self.schedule, self.delayed = name, name == "delayed"
        self.split, self.off = self.cand if name == "overlap" else (None, 0)

    def go_pipelined(self, twin):
        """Two steps in flight, every second one on ``twin`` (not prepared yet): ONE communicator, nothing to tune.  (The
        twin keeps the split its own prepare() chose under TN_DP_OVERLAP=1 -- as it always has.)"""
        if self.net._dp:
            twin._dev_group = self.net._group()
        twin._prepare_training()
        if self.net._dp:
            self.set_schedule("plain")
            for dp in (self, twin.dp):
                dp.tune, dp.schedule = None, "pipelined"

    def segs_rebuilt(self):
        """The net's segment table was rebuilt (the twin's, on the shared velocities)."""
        if self.can_delay:
            self.segs_ab[0] = self.net._d_segs

    def drop_pending(self):
        """The velocities are being zeroed: the reduced gradient still to be folded in is zeroed with them."""
        if self.delayed and self.pending:
            self.net.ctx.call("tn_stream_wait", 0, 1)
            self.pending = False

    def pending_grads(self):
        """{id(layer): views} of the reduced gradient the velocity is behind by (second stream: synchronise first), or None."""
        return self.grads_ab[1 - self.cur] if self.delayed and self.pending else None

    def tune_tick(self):
        """TN_DP_OVERLAP=auto: every candidate runs W warm-up + M timed (ordinary) steps under a pair of HIP events; then every
        rank takes the max over ranks and keeps the fastest.  All ranks switch at the same step: the collectives differ."""
        net, ctx, T = self.net, self.net.ctx, self.tune
        W, M = self.TUNE_WARM, self.TUNE_STEPS
        k, cands = T["k"] - self.TUNE_PRE, T["cands"]
        T["k"] += 1
        if k < 0:                                 # the first steps of a run are not representative
            return
        leg, pos = divmod(k, W + M)

        def mark(name):
            e = ctypes.c_void_p()
            ctx.call("tn_event_create", ctypes.byref(e))
            ctx.call("tn_event_record", e)
            T["ev"][name] = e

        if pos == 0:
            if leg > 0:
                mark("e%d" % (leg - 1))
            if leg < len(cands):
                self.set_schedule(cands[leg])
        if pos == W and leg < len(cands):
            mark("s%d" % leg)
        if leg == len(cands) and pos == 0:
            ctx.sync()
            ms = []
            for q in range(len(cands)):
                v = ctypes.c_float()
                ctx.call("tn_event_elapsed_ms", T["ev"]["s%d" % q], T["ev"]["e%d" % q], ctypes.byref(v))
                ms.append(v.value)
            for e in T["ev"].values():
                ctx.lib.tn_event_destroy(ctx.h, e)
            t = ctx.array(np.asarray(ms, np.float32))
            net._group().allreduce_max(t)
            ms = [float(v) / M for v in t.get_value()]
            self.tuned_ms = dict(zip(cands, ms))
            self.tune = None
            self.set_schedule(cands[int(np.argmin(ms))])
            if net.world.rank == 0:
                sys.stderr.write("theanet_amd: data-parallel schedule '%s' (%s)\n" % (
                    self.schedule, ", ".join("%s %.1f us/step" % (c, 1e3 * m) for c, m in zip(cands, ms))))

    def begin_step(self, pipe_stride):
        if self.tune is not None and not pipe_stride:
            self.tune_tick()
        self.bind(self.cur if self.delayed else 0)
        self._joined = self._bucket_sent = False

    def _allreduce_beside(self, darr, count=None):
        """The sum on the second stream, behind what the first holds so far and beside what it does next."""
        ctx = self.net.ctx
        ctx.call("tn_stream_wait", 1, 0)
        ctx.call("tn_stream_select", 1)
        self.net._group().allreduce_sum(darr, count)
        ctx.call("tn_stream_select", 0)

    def after_backward(self, idx, pipe_stride):
        net, ctx = self.net, self.net.ctx
        if idx == self.split:
            # the dense group is done: finish its slab sums and reduce its gradients on the second stream, under the conv backward
            ctx.call("tn_defer_reductions", 0)
            ctx.call("tn_defer_reductions", 1)
            self._allreduce_beside(net.flat_grads.view(self.off, (net.n_flat - self.off,)))
            self._joined = True
        elif pipe_stride and self.bucket is not None and idx == self.bucket[0]:
            # two steps in flight, bucketed (SURVEY 8e "bucket by layer"): the dense group's gradients exist NOW -- the bucket
            # [dense gradients | cost] leaves on the communication stream under the conv backward; the conv bucket follows
            ctx.call("tn_defer_reductions", 0)
            ctx.call("tn_defer_reductions", 1)
            off = self.bucket[1]
            net._group().allreduce_sum_async(net.flat_grads.view(off, (net.n_flat - off,)), None, None)
            self._bucket_sent = True

    def end_pipelined(self):
        """Two steps in flight: every collective goes through the ONE communication stream (one order of collectives whatever
        stream the step ran on, no compute stream waits inside one); the consumer, a step away, waits for ``ar_done_ev``."""
        net = self.net
        if net._dp:
            n = self.bucket[1] if self._bucket_sent else net.n_flat
            net._group().allreduce_sum_async(net.flat_grads, n, self.ar_done_ev)

    def end_sequential(self, tail):
        """After a sequential step's backward pass (``tail``: an elastic field joins the update).  True: it issued the update."""
        net, ctx = self.net, self.net.ctx
        if self.delayed and tail:
            self.set_schedule("plain")            # (configuration-determined: the same on every rank)
        if self.delayed:
            # layer.py:82-86 applies the OLD velocity: p_{t+1} = p_t - s*v_t needs the gradient of step t-1.  Update with its
            # REDUCED gradient (that all-reduce had this whole step), then start this step's beside the next.  Same bits.
            cur = self.cur
            if self.pending:
                ctx.call("tn_stream_wait", 0, 1)
            self.catch_up(self.segs_ab[1 - cur if self.pending else cur], net.d_step.ptr, 1, 1 if self.pending else 2)
            self._allreduce_beside(self.flat_ab[cur], net.n_flat)
            self.pending, self.cur = True, 1 - cur
            return True
        if net._dp:
            if self._joined:
                if self.off:
                    net._group().allreduce_sum(net.flat_grads, self.off)      # the conv head
                ctx.call("tn_stream_wait", 0, 1)                              # join the tail
            else:
                net._group().allreduce_sum(net.flat_grads, net.n_flat)
        return False
