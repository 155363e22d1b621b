"""What ``get_trin_model`` / ``get_test_model`` return -- the counterparts of the reference's compiled Theano functions
(neuralnet.py:236-241, :270-277): ``fn(i) -> [cost, features, logprob]`` one step at a time (``_TrainFn``) or with two
steps in flight (``_PipeTrainFn``), ``fn(i) -> [sym_err, P(MLE)]`` (``_TestFn``; ``sweep(indices)``: a run of minibatches,
read back once).  ``enqueue(i)`` issues a step without reading anything back; once the calls of a function have been seen to repeat, a step is ONE C call (plan.py,
tn_net_step).  ``set_order(order)`` makes the minibatches of an epoch slices of a device-resident row order (one
tn_gather_batch launch per step) without giving any of that up."""
import os

import numpy as np

from . import _lib
from .device import share  # noqa: F401
from .layer import ElasticLayer
from .plan import StepPlan


def _features_logprob(out):
    """[features, logprob] of the output head (neuralnet.py:236-241); for Softmax and Hinge heads features IS
    logprob (outlayers.py:92-93, :137-139)."""
    logprob = out.logprob.get_value()
    feats = logprob if out.features is out.logprob else out.features.get_value()
    return [feats, logprob]


def _step_outputs(net, out):
    """[cost, features, logprob] of the step ``net`` ran last, on the stream currently selected (the one that
    holds the launch summing the cost).  When the step sent features / logprob ahead (``NeuralNet._send_outputs``:
    copies into page-locked memory that ran under the backward pass) the cost follows them through the copy
    stream and one wait covers all three; otherwise three blocking copies."""
    early = net._early
    if early is not None and early["live"]:
        early["live"] = False
        if not early["cost_sent"]:
            net.ctx.call("tn_d2h_early", early["cost"].ptr, net.d_cost.ptr, 4)
        net.ctx.call("tn_copy_sync")
        logprob = early["logprob"].array.copy()
        feats = logprob if out.features is out.logprob else early["features"].array.copy()
        return [np.float32(early["cost"].array[0]), feats, logprob]
    cost = net.d_cost.get_value()[0]
    return [cost] + _features_logprob(out)


class _CostLedger:
    """The costs of enqueued steps, read a few steps LATER so that the loop of train.py (train.py:207-226: it sums the
    cost of every step and raises on NaN) never waits for the GPU: a step's cost (4 bytes) leaves for one of four
    page-locked slots as soon as it exists (tn_d2h_early_ev: copy stream, behind the launch that sums it, an event
    behind the copy) and the host picks it up ``lag`` calls later -- by then it has long arrived; if not, the host
    waits for that slot's event only.

    Which costs belong to a step_cost() loop is recorded when a step is issued: the slot of step t (t % R) holds the
    number k of the step_cost() call that issued it, or None (enqueue(), fn(i): nobody's).  The costs handed out are
    the owned ones, in order, with their k; k counts the step_cost() calls since the last drain_costs().  ONE ledger
    per training function: the one-step-at-a-time fallback of a pipelined function shares it and its numbering."""
    R = 4

    def __init__(self, ctx):
        self.ctx = ctx
        self.k = 0                  # step_cost() calls since the last drain_costs()
        self.cur = None             # the k of the step being issued (None: not a step_cost() call's)
        self.owed = []              # owned costs taken off the ring early, handed out first
        self.live = False           # the ring is on (a step_cost() loop has started)
        self.buf, self.ev = None, []

    def open(self, t, lag):
        """Ring on from step t (the steps before it are nobody's)."""
        if self.buf is None:
            import ctypes
            from .device import HostBuffer
            self.buf = HostBuffer(self.ctx, (self.R,), np.float32)
            for _ in range(self.R):
                e = ctypes.c_void_p()
                self.ctx.call("tn_event_create", ctypes.byref(e))
                self.ev.append(e)
        self.live, self.lag = True, lag
        self.own = [None] * self.R
        self.next = self.sent = t   # steps below `next` are handed out or nobody's; copies are issued below `sent`

    def issue(self, t, s, d_cost, net):
        """Step t is issued (its owner: ``cur``) and the cost of step s (t itself, or t - 2 with two steps in flight)
        has been summed into ``d_cost``: off it goes to slot s % R -- unless it is not the ring's to send (s below
        ``sent``: summed before the ring was on, or read directly by ``rest``).  ``d_cost`` None: a replayed step,
        whose C call has issued the copy already.  The copy is ordered behind the launch that summed the cost, on the
        copy stream; nothing else holds the compute stream back, so the NEXT launch that writes ``d_cost`` must wait
        for the slot's event first: ``net._guard_cost()`` (NeuralNet) does, in front of every such launch -- a step or
        two later in the lazy schedules (the copy has long run), a few tens of microseconds later where the cost is
        summed mid-step (data-parallel pipelined steps, weight-cost nets)."""
        old = t - self.R
        if old >= self.next:
            # slot t % R passes from step t - R to step t: an owned cost nobody has taken yet (plain enqueue() calls
            # behind a step_cost() loop) is taken now; inside a loop the lag has handed it out already
            if self.own[t % self.R] is not None:
                assert self.cur is None, "cost ring overrun"
                self.owed.append((self.own[t % self.R], self._take(old)))
            self.next = old + 1
        self.own[t % self.R] = self.cur
        if s >= self.sent:
            assert s == self.sent, "cost ring out of step"
            if d_cost is not None:
                self.ctx.call("tn_d2h_early_ev", self.buf.ptr + 4 * (s % self.R), d_cost.ptr, 4, self.ev[s % self.R])
            net._cost_guard_ev = self.ev[s % self.R]
            self.sent = s + 1

    def step(self, t, enqueue, i):
        """One step_cost() call: the owned costs that have become due (t steps issued so far), then step i."""
        out, self.owed = self.owed, []
        while self.next <= t - self.lag:
            if self.own[self.next % self.R] is not None:
                out.append((self.own[self.next % self.R], self._take(self.next)))
            self.next += 1
        self.cur = self.k
        try:
            enqueue(i)
        finally:
            self.cur = None
        self.k += 1
        return out

    def rest(self, t, read=None):
        """Everything still owed, in order (t steps issued so far): the costs taken early, the copies under way, then
        ``read(s)`` for the steps whose cost nobody has sent.  What follows starts from step t."""
        out, self.owed = self.owed, []
        if self.live:
            for s in range(self.next, t):
                if self.own[s % self.R] is not None:
                    out.append((self.own[s % self.R], self._take(s) if s < self.sent else read(s)))
            self.next = self.sent = t
        return out

    def _take(self, s):
        self.ctx.lib.tn_event_sync(self.ctx.h, self.ev[s % self.R])
        return np.float32(self.buf.array[s % self.R])

    def __del__(self):
        try:
            for e in self.ev:
                self.ctx.lib.tn_event_destroy(self.ctx.h, e)
        except Exception:       # interpreter teardown
            pass


def _batch_in_range(i, n_rows, batch_sz):
    """Minibatch i must lie inside the dataset (the reference's ``data[i*B:(i+1)*B]`` would come out short and fail in the
    compiled function; the kernels here would read past the array)."""
    i = int(i)
    if i < 0 or (i + 1) * batch_sz > n_rows:
        raise IndexError("minibatch %d of %d rows each in a dataset of %d rows" % (i, batch_sz, n_rows))


class _RowOrder:
    """The row order of a shuffled epoch (``set_order``), resident on the device, and the per-net buffers its
    minibatches are staged in.  ONE per training function: the one-step-at-a-time fallback of a pipelined function
    shares it.  ``buf`` (int32, one entry per dataset row) is allocated when the first order arrives and never moves:
    recorded steps bake its address (and the stages') into their tn_gather_batch call, so a new order only changes
    what the buffer holds.  A stage belongs to one net -- the twin of the pipelined schedule has its own: a stream's
    previous step is two steps back and complete in stream order when the next gather overwrites the stage."""

    def __init__(self, ctx, x_data, y_data, aux_data=None):
        self.ctx, self.x_data, self.y_data, self.aux_data = ctx, x_data, y_data, aux_data
        self.buf = None
        self.len = None                 # entries of the current order (None: dataset order)
        self.stages = {}                # id(net) -> (net, x_stage, y_stage, aux_stage)
        self.row_bytes = int(np.prod(x_data.shape[1:])) * 4
        self.aux_bytes = int(np.prod(aux_data.shape[1:])) * 4 if aux_data is not None else 0

    def check(self, order, batch_sz):
        """``order`` as a contiguous int32 vector, or the exception set_order documents."""
        rows = self.x_data.shape[0]
        order = np.asarray(order)
        if order.ndim != 1 or order.dtype.kind not in "iu":
            raise ValueError("an order is a 1-D integer array (got %s, %d-D)" % (order.dtype, order.ndim))
        if not batch_sz <= order.shape[0] <= rows:
            raise ValueError("an order holds between %d (one minibatch) and %d (the dataset) row numbers, not %d"
                             % (batch_sz, rows, order.shape[0]))
        if order.min() < 0 or order.max() >= rows:
            raise IndexError("an order holds row numbers of a dataset of %d rows (got [%d, %d])"
                             % (rows, order.min(), order.max()))
        return np.ascontiguousarray(order, np.int32)

    def upload(self, order):
        """(the caller has synchronised: no step in flight reads the buffer)"""
        if order is None:
            self.len = None
            return
        if self.buf is None:
            self.buf = self.ctx.empty((self.x_data.shape[0],), np.int32)
        self.buf.view(0, (order.shape[0],)).set_value(order)
        self.len = order.shape[0]

    def in_range(self, i, batch_sz):
        i = int(i)
        if i < 0 or (i + 1) * batch_sz > self.len:
            raise IndexError("minibatch %d of %d rows each in an order of %d rows" % (i, batch_sz, self.len))

    def gather(self, net, row0):
        """Stage rows order[row0, row0 + local_bsz) for ``net`` on the stream currently selected: (x, y, aux) stages."""
        st = self.stages.get(id(net))
        if st is None:
            n = net.local_bsz
            st = self.stages[id(net)] = (
                net, self.ctx.empty((n,) + tuple(self.x_data.shape[1:])), self.ctx.empty((n,), np.int32),
                self.ctx.empty((n,) + tuple(self.aux_data.shape[1:])) if self.aux_data is not None else None)
        _, xs, ys, auxs = st
        self.ctx.call("tn_gather_batch", self.buf.ptr, int(row0), net.local_bsz, self.x_data.ptr, xs.ptr, self.row_bytes,
                      self.y_data.ptr, ys.ptr, self.aux_data.ptr if auxs is not None else None,
                      auxs.ptr if auxs is not None else None, self.aux_bytes)
        return xs, ys, auxs


def _agree_on_order(net, order):
    """Data-parallel ranks must train on the same order (each takes its shard of every minibatch of it)."""
    if net.world.size > 1:
        import zlib
        from . import comm
        crc = -1.0 if order is None else float(zlib.crc32(order.tobytes()))
        comm.agree(crc, "the row order of set_order (CRC)")


def _enqueue_planned(fn, i, keep=lambda: True):
    """``fn._enqueue(i)`` inside the step plan's bracket (plan.py): a recorded phase is replayed as one C call; otherwise the
    step is interpreted, and recorded when it is an ordinary one (plannable before it, no exception, ``keep()`` after it)."""
    pl = fn._plan
    if pl is None or pl.off:
        return fn._enqueue(i)
    ok = fn._plannable()
    if ok and pl.ready:                      # (the learning rate is a device scalar here: no argument changes with it)
        fn.net._apply_dtype()
        st = pl.step(i, fn._plan_state())
        if st is not None:
            return fn._plan_set_state(st)
    if ok:
        pl.begin(i, fn._plan_state())
    try:
        fn._enqueue(i)
    except Exception:
        ok = False
        raise
    finally:
        ok = ok and keep()
        pl.end(fn._plan_state() if ok else None, ok)


class _TrainFn:
    """What ``get_trin_model`` returns: ``fn(i) -> [cost, features, logprob]``
    (neuralnet.py:236-241).  ``enqueue(i)`` issues the step without reading anything
    back (the GPU runs ahead of the host); ``fetch()`` copies the last step's outputs."""

    def __init__(self, net, x_data, y_data, take_index_list, aux_data=None, ledger=None, order=None):
        self.net, self.x_data, self.y_data = net, x_data, y_data
        self.aux_data = aux_data
        self.take_index_list = take_index_list
        ctx = net.ctx
        self._ord = order or _RowOrder(ctx, x_data, y_data, aux_data)      # set_order(): a shuffled epoch
        if take_index_list:
            row = int(np.prod(x_data.shape[1:]))
            self.x_stage = ctx.empty((net.local_bsz,) + tuple(x_data.shape[1:]))
            self.y_stage = ctx.empty((net.local_bsz,), np.int32)
            self.idx_dev = ctx.empty((net.local_bsz,), np.int32)
            self.row_bytes = row * 4
            if aux_data is not None:
                self.aux_stage = ctx.empty((net.local_bsz,) + tuple(aux_data.shape[1:]))
        # the step as one C call once its calls have been seen to repeat (plan.py); index-list batches upload per step
        self._plan = None if take_index_list else StepPlan(ctx, net.batch_sz, net.shard_lo)
        self._n = 0                            # steps enqueued so far
        self._led = ledger or _CostLedger(ctx)  # step_cost(): costs read two calls late

    def _plan_state(self):
        net = self.net
        first = net.tr_layers[0]
        return (getattr(first, "_cur", None), getattr(first, "_pre_valid", None), net._cost_pending,
                net.dp.cur, net.dp.pending, (self._n & 3) if self._led.live else -1)

    def _plan_set_state(self, st):
        net = self.net
        first = net.tr_layers[0]
        if st[0] is not None:
            first._cur, first._pre_valid = st[0], st[1]
        if st[2] is not None:
            net._cost_pending = st[2]
        net.dp.cur, net.dp.pending = st[3], st[4]
        if self._led.live:                        # (the replayed step has sent its cost like an interpreted one)
            self._led.issue(self._n, self._n, None, net)
        self._n += 1

    def _plannable(self):
        net = self.net
        return not net._want_outputs and net.dp.tune is None and net.ctx.ev_hook is None and not net._injecting()

    def enqueue(self, i):
        if self.take_index_list:
            idx = np.asarray(i)
            if idx.shape != (self.net.batch_sz,) or idx.min() < 0 or idx.max() >= self.x_data.shape[0]:
                raise IndexError("an index list must hold %d row numbers of a dataset of %d rows"
                                 % (self.net.batch_sz, self.x_data.shape[0]))
        elif self._ord.len is not None:
            self._ord.in_range(i, self.net.batch_sz)
        else:
            _batch_in_range(i, self.x_data.shape[0], self.net.batch_sz)
        _enqueue_planned(self, i)

    def set_order(self, order):
        """From now on ``fn(i)`` / ``enqueue(i)`` / ``step_cost(i)`` train on dataset rows ``order[i*B:(i+1)*B]`` (a
        data-parallel rank: on its shard of that slice); ``None``: dataset order again.  ``order``: 1-D integers,
        B <= len <= dataset rows, entries in [0, rows) -- not necessarily a permutation.  The order is an input, not
        state: checkpoints and test functions do not know it.  Meant to be called once per epoch: it waits for the
        steps in flight.  A recorded step plan, the cost ring and its numbering survive a new order; only switching
        between no order and an order changes the calls a step makes, and the plan watches again."""
        if self.take_index_list:
            raise ValueError("set_order: this training function takes an index list per step")
        net = self.net
        if order is not None:
            order = self._ord.check(order, net.batch_sz)
        _agree_on_order(net, order)
        if self._led.live:                        # costs still under way: taken now, handed out by the next call
            self._led.owed = self._ring_rest(keep=True)
        net.ctx.sync()
        switched = (order is None) != (self._ord.len is None)
        self._ord.upload(order)
        if switched:
            self._plan.restart("row order on" if order is not None else "row order off")

    def _enqueue(self, i):
        net, ctx = self.net, self.net.ctx
        B, lo = net.batch_sz, net.shard_lo
        slot = net.x
        slot.d_row0 = None
        if self._ord.len is not None:
            xs, y, auxs = self._ord.gather(net, int(i) * B + lo)
            slot.bind(xs)
            slot.row0, y_row0 = 0, 0
            if auxs is not None:
                net.aux_inpt_tr.bind(auxs)
                net.aux_inpt_tr.row0 = 0
        elif self.take_index_list:
            idx = np.ascontiguousarray(np.asarray(i, np.int32)[lo:lo + net.local_bsz])
            self.idx_dev.set_value(idx)
            ctx.call("tn_gather_rows", self.x_data.ptr, self.idx_dev.ptr, self.x_stage.ptr,
                     net.local_bsz, self.row_bytes)
            ctx.call("tn_gather_rows", self.y_data.ptr, self.idx_dev.ptr, self.y_stage.ptr,
                     net.local_bsz, 4)
            slot.bind(self.x_stage)
            slot.row0, y, y_row0 = 0, self.y_stage, 0
            if self.aux_data is not None:                  # neuralnet.py:233-234
                ctx.call("tn_gather_rows", self.aux_data.ptr, self.idx_dev.ptr, self.aux_stage.ptr, net.local_bsz,
                         int(np.prod(self.aux_data.shape[1:])) * 4)
                net.aux_inpt_tr.bind(self.aux_stage)
                net.aux_inpt_tr.row0 = 0
        else:
            slot.bind(self.x_data)
            slot.row0 = int(i) * B + lo
            y, y_row0 = self.y_data, slot.row0
            if self.aux_data is not None:                  # neuralnet.py:225-226
                net.aux_inpt_tr.bind(self.aux_data)
                net.aux_inpt_tr.row0 = slot.row0
        slot.row_global0 = lo
        if self.aux_data is not None:
            net.aux_inpt_tr.row_global0 = int(i) * B + lo if not self.take_index_list else lo
        net._train_step(y, y_row0)
        if self._led.live:                        # the step's cost exists behind its last launch: off it goes
            self._led.issue(self._n, self._n, net.d_cost, net)
        self._n += 1

    # -- costs a few calls late (what train.py's loop needs of a step; see _CostLedger) --------------------------
    def step_cost(self, i):
        """Enqueue step i; return [(step number, cost), ...] of the steps whose cost has become due (step numbers count
        the step_cost calls since the last drain_costs()).  Do not mix with enqueue() / fn(i) before drain_costs()."""
        net, led = self.net, self._led
        if net.dp.delayed or net.dp.tune is not None or self.take_index_list or net._injecting():
            out = self._ring_rest()               # (the cost travels on the second stream / per-step host work)
            out.append((led.k, np.float32(self(i)[0])))
            led.k += 1
            return out
        if not led.live:
            led.open(self._n, 2)
            self._plan.restart("cost ring on")
        return led.step(self._n, self.enqueue, i)

    def _ring_rest(self, keep=False):
        """Everything the ledger still owes, in order.  ``keep``: the ring (and with it the recorded steps, whose baked
        slot and event pointers follow the step number modulo 4) stays for the next loop."""
        led = self._led
        out = led.rest(self._n)
        if led.live and not keep:
            led.live = False
            self._plan.restart("cost ring off")
        return out

    def drain_costs(self):
        """The costs step_cost() has not handed out yet, in order; afterwards step numbers start from 0 again.  train.py
        calls this at the end of every epoch: ring and plan survive it (an epoch of mnist.prms at batch 4096 is 12
        steps -- fewer than it takes to watch and record a step)."""
        out = self._ring_rest(keep=True)
        self._led.k = 0
        return out

    def fetch(self):
        net = self.net
        out = net.tr_layers[-1]
        if net.dp.pending:
            net.ctx.sync()                        # the cost travels with the all-reduce on the second stream
        return _step_outputs(net, out)

    def __call__(self, i):
        self.net._want_outputs = True       # features / logprob leave right after the forward pass
        try:
            self.enqueue(i)
        finally:
            self.net._want_outputs = False
        return self.fetch()


class _PipeTrainFn:
    """``get_trin_model``'s function for single-GPU training with TWO STEPS IN FLIGHT.

    The reference's update applies the OLD velocity (layer.py:82-86: ``v' = m v + (1-m) g``,
    ``p' = p - rate*lr*v``), so the weights of step t are ``p_{t-1} - s*v_{t-1}`` with ``v_{t-1}`` built
    from the gradient of step t-2: step t does not depend on the backward pass of step t-1.  Even steps
    run on the context's first stream with the net itself, odd steps on the second stream with a twin
    (own weights copy, activations and gradients; the velocities are shared).  Step t starts by waiting
    for the other stream's update, then ``v <- m v + (1-m) g_{t-2}`` (its own gradient of two steps ago)
    and ``p_own <- p_other - s*v`` in one launch (tn_sgd_update_net, TN_UPD_PIPE), then runs its forward and
    backward passes while the other stream is still busy with step t-1 -- the two fill each other's
    launch gaps and lock-step phases (-18 % per step on mnist.prms).  Same weights, costs and outputs as
    the sequential schedule, bit for bit (tests/test_gpu_net.py::test_pipelined_steps_equal_sequential);
    reading weights (get_wts, test functions, checkpoints) first brings the net up to date.  With WT_AVG every update
    launch is followed by the averages' on the same stream (tn_avg_net): each p_t enters them once, in order."""

    def __init__(self, net, x_data, y_data):
        import ctypes
        self.net, self.x_data, self.y_data = net, x_data, y_data
        self.take_index_list = False
        self.t = 0                   # steps enqueued so far
        self._updated = False        # the update for step self.t has already been applied (weights were read)
        self._want = False           # the caller of this step reads its outputs (__call__)
        self._seq = None             # sequential fallback (_TrainFn) once something rules pipelining out
        self._twin = None
        self._last = net
        net._pipe_fn = self
        self._ctypes = ctypes
        self._plan = StepPlan(net.ctx, net.batch_sz, net.shard_lo)
        self._led = _CostLedger(net.ctx)     # step_cost(): costs read four calls late
        self._ord = _RowOrder(net.ctx, x_data, y_data)       # set_order(): a shuffled epoch
        # weight-cost nets: stream k's last gradient is in the velocity already (sync_weights) -- its next update leaves v alone
        self._v_done = [False, False]

    # -- set-up of the twin on first use ---------------------------------------------------------
    def _build(self):
        net, ctx = self.net, self.net.ctx
        import copy
        from .neuralnet import NeuralNet
        twin = NeuralNet.__new__(NeuralNet)
        twin._is_twin = True
        twin._main = net
        tp = dict(net.tr_prms)
        tp.setdefault('SEED', 0)      # (a net loaded from a checkpoint has none; weights and stream seeds are copied below)
        twin.__init__(copy.deepcopy(net.layers), tp)
        net.dp.go_pipelined(twin)
        for a, b in zip(net.tr_layers, twin.tr_layers):
            if hasattr(a, "seed"):
                b.seed = a.seed
            if getattr(a, "drop", None) is not None:
                b.drop.seed = a.drop.seed
            for pa, pb in zip(a.params, b.params):
                ctx.call("tn_d2d", pb.ptr, pa.ptr, pa.size * 4)
            if hasattr(a, "centers") and not a.learn_centers:        # fixed class centers: the same on both streams
                ctx.call("tn_d2d", b.centers.ptr, a.centers.ptr, a.centers.size * 4)
            if a.params:
                b.accumulated_updates = a.accumulated_updates        # ONE velocity per tensor
        # the twin's own velocity buffers are gone with that: its update table must name the shared ones
        # (it is what _fall_back folds the last gradient through when the twin ran the last step)
        twin._build_seg_table()
        twin.dp.segs_rebuilt()
        if net._avg is not None:                 # WT_AVG: ONE average per tensor, fed from whichever stream steps
            twin._build_avg_table(net)
        self._twin = twin
        self.nets = (net, twin)
        # nets with weight costs: tn_pipe_reg_seg rows (TN_UPD_PIPE_REG: the L1 / L2 gradient terms are taken at the
        # stepping stream's own weights, p_{t-2}, before the update overwrites them)
        reg = self._reg = bool(net._has_wtcost)
        self._mode = _lib.TN_UPD_PIPE_REG if reg else _lib.TN_UPD_PIPE
        seg_dt = np.dtype([('p', 'u8'), ('psrc', 'u8'), ('v', 'u8'), ('g', 'u8'), ('n', 'u8'),
                           ('momentum', 'f4'), ('rate', 'f4')] + ([('L1', 'f4'), ('L2', 'f4')] if reg else []))
        self._segs, self._hsegs, self._lr, self._lr_set = [], [], [], [None, None]
        for X, Y in ((net, twin), (twin, net)):
            rows = []
            for lx, ly in zip(X.tr_layers, Y.tr_layers):
                if lx.has_updates():
                    for p, ps, v, g in zip(lx.params, ly.params, lx.accumulated_updates, lx.grads):
                        rows.append((p.ptr, ps.ptr, v.ptr, g.ptr, p.size, lx.reg['momentum'], lx.reg['rate'])
                                    + ((lx.reg['L1'], lx.reg['L2']) if reg else ()))
            host = np.array(rows, dtype=seg_dt)
            self._hsegs.append(host)             # kept alive: the update matches pending slab sums against it
            self._segs.append(ctx.array(host.view(np.uint8)))
            X._cost_pending = False
            self._lr.append(ctx.zeros((1,)))
        self._nseg, self._max_seg = net._n_segs, net._max_seg
        self._ev, arev = [], []
        for _ in range(2):
            for lst in (self._ev, arev):
                e = self._ctypes.c_void_p()
                ctx.call("tn_event_create", self._ctypes.byref(e))
                lst.append(e)
        for k, X in enumerate(self.nets):                  # recorded behind step's last collective (communication stream)
            X.dp.ar_done_ev = arev[k]
        base = int(net.d_step.get_value()[0])            # steps already taken (an earlier training function)
        self._base = base
        ctx.call("tn_set_u32", twin.d_step.ptr, base + 1)    # the twin takes every second step
        self._lr_prev = None

    def _lr_now(self):
        tp = self.net.tr_prms
        return float(np.float32(tp['INIT_LEARNING_RATE'] / (1 + tp['CUR_EPOCH'] / tp['EPOCHS_TO_HALF_RATE'])))

    def _blocked(self):
        return self.net._injecting() or self.net.ctx.ev_hook is not None

    # -- the step as one C call (plan.py) -----------------------------------------------------------
    def _plan_state(self):
        """What a step leaves behind on the host (restored after a replayed step of the same phase)."""
        per_net = []
        for X in self.nets:
            first = X.tr_layers[0]
            per_net.append((X._cost_pending, getattr(first, "_cur", None), getattr(first, "_pre_valid", None)))
        return (self.nets.index(self._last), tuple(per_net), (self.t & 3) if self._led.live else (self.t & 1))

    def _plan_set_state(self, st):
        self._last = self.nets[st[0]]
        for X, (cp, cur, pv) in zip(self.nets, st[1]):
            X._cost_pending = cp
            if cur is not None:
                first = X.tr_layers[0]
                first._cur, first._pre_valid = cur, pv
        self._updated = False
        if self._led.live:                        # (the replayed step has sent the cost of step t - 2)
            self._led.issue(self.t, self.t - 2, None, self.nets[self.t & 1])
        self.t += 1

    def _plannable(self):
        lr = self._lr_now()
        return self._seq is None and self._twin is not None and not self._updated and not self._want \
            and self.t >= 4 and lr == self._lr_prev and self._lr_set[0] == lr and self._lr_set[1] == lr \
            and not self._blocked() and not any(self._v_done)

    # -- the start-of-step update -----------------------------------------------------------------
    def _update_for(self, t):
        """weights (and velocity) for step t on the stream that will run it"""
        ctx, k = self.net.ctx, t & 1
        X = self.nets[k]
        self.net._apply_dtype()
        ctx.call("tn_stream_select", k)
        ctx.call("tn_event_wait", self._ev[1 - k])
        if X._dp and t >= 2:
            ctx.call("tn_event_wait", X.dp.ar_done_ev)    # this stream's gradient of step t-2, back from the all-reduce
        if self._lr_set[k] != self._lr_prev:              # the rate step t-1 was enqueued under
            ctx.call("tn_set_f32", self._lr[k].ptr, self._lr_prev)
            self._lr_set[k] = self._lr_prev
        out = X.tr_layers[-1]
        rider = X._cost_pending
        if rider:
            X._guard_cost()
        upd_v = t >= 2 and not self._v_done[k]
        self._v_done[k] = False
        X._update_and_maxnorm(self._mode, self._segs[k].ptr, self._hsegs[k].ctypes.data, self._nseg,
                              self._max_seg, self._lr[k].ptr, 1.0, X.d_step.ptr, 2 if t >= 2 else 0, 1 if upd_v else 0,
                              out.rowloss.ptr if rider else None, X.local_bsz, 1.0 / X.batch_sz,
                              X.d_cost.ptr if rider else None)
        X._cost_pending = False
        # WT_AVG: these are the weights step t reads, p_t; the averages are one chain across both streams, so the event
        # the other stream's next update waits for covers this launch as well
        X._avg_update()
        ctx.call("tn_event_record", self._ev[k])

    def _catch_up_v(self, t):
        """Weight-cost nets, behind ``_update_for(t)`` when something is about to read the weights: the gradient of step
        t-1 goes into the velocity NOW, on the device, while the net that ran that step still holds the weights it was
        taken at (its L1 / L2 terms need them; bringing the net's own weights up to date may overwrite them, and so does
        nothing else before that stream's next update, which then leaves the velocity alone).  On step t's stream,
        behind its update: v_{t-1} is complete there."""
        ctx, k = self.net.ctx, t & 1
        Y = self.nets[1 - k]
        ctx.call("tn_stream_select", 1 - k)
        ctx.call("tn_defer_reductions", 0)            # the gradient of step t-1: finish its slab sums
        ctx.call("tn_stream_wait", k, 1 - k)
        ctx.call("tn_stream_select", k)
        self.net.dp.catch_up(Y._d_segs, which=3 | 4)
        ctx.call("tn_event_record", self._ev[k])
        self._v_done[1 - k] = True

    def sync_weights(self):
        """Bring the net's own weights up to date (p_t after t steps) before anything reads them."""
        if self._seq is not None or self._twin is None or self.t == 0:
            return
        ctx, t = self.net.ctx, self.t
        if not self._updated:
            self._update_for(t)
            self._updated = True
            if self._reg:
                self._catch_up_v(t)
        if t & 1:                                         # the twin holds p_t: copy into the net
            ctx.call("tn_stream_select", 0)
            ctx.call("tn_event_wait", self._ev[1])
            for a, b in zip(self.net.tr_layers, self._twin.tr_layers):
                for pa, pb in zip(a.params, b.params):
                    ctx.call("tn_d2d", pa.ptr, pb.ptr, pa.size * 4)
        ctx.call("tn_stream_select", 0)
        ctx.sync()

    def _flush_parked(self):
        """Finish the slab sums and costs the last steps left parked with their streams (the gradients
        become ordinary buffers; the next update simply reads them)."""
        if self._twin is None or self._seq is not None:
            return
        ctx = self.net.ctx
        for k, X in enumerate(self.nets):
            ctx.call("tn_stream_select", k)
            ctx.call("tn_defer_reductions", 0)
            self._finish_cost(X)
        ctx.call("tn_stream_select", 0)

    def _fall_back(self):
        """Leave the pipelined schedule for good: bring weights AND velocity to the sequential state."""
        net, ctx = self.net, self.net.ctx
        if self._led.live:                        # costs still owed to a step_cost() loop: collect them first
            self._led.owed = self._leave_ring()
        self._flush_parked()
        if self._twin is not None and self.t > 0:
            self.sync_weights()
            # the velocity is one gradient behind (that of step t-1, held by the stream that ran it)
            Y = self.nets[(self.t - 1) & 1]
            ctx.call("tn_stream_select", 0)
            if not self._v_done[(self.t - 1) & 1]:        # (weight-cost nets: sync_weights has folded it in, L1 / L2 included)
                net.dp.catch_up(Y._d_segs)
            ctx.call("tn_set_u32", net.d_step.ptr, self._base + self.t)
            ctx.sync()
        net._pipe_fn = None
        first = net.tr_layers[0]
        if isinstance(first, ElasticLayer):
            first._pre_valid = False              # a field built ahead was for this stream's step t+2
        self._seq = _TrainFn(net, self.x_data, self.y_data, False, ledger=self._led, order=self._ord)

    # -- the step ---------------------------------------------------------------------------------
    def enqueue(self, i):
        if self._ord.len is not None:
            self._ord.in_range(i, self.net.batch_sz)
        else:
            _batch_in_range(i, self.x_data.shape[0], self.net.batch_sz)
        _enqueue_planned(self, i, keep=lambda: self._seq is None)     # (a step that fell back is not one to record)

    def set_order(self, order):
        """``_TrainFn.set_order`` with two steps in flight: the schedule stays pipelined (both streams are drained, the
        next step carries on from the weights they left), a ready plan stays ready."""
        if self._seq is not None:
            return self._seq.set_order(order)
        net = self.net
        if order is not None:
            order = self._ord.check(order, net.batch_sz)
        _agree_on_order(net, order)
        if self._led.live:                        # costs still under way: taken now, handed out by the next call
            self._led.owed = self._leave_ring(keep=True)
        net.ctx.sync()
        switched = (order is None) != (self._ord.len is None)
        self._ord.upload(order)
        if switched:
            self._plan.restart("row order on" if order is not None else "row order off")

    def _enqueue(self, i):
        if self._seq is None and self._blocked():
            self._fall_back()
        if self._seq is not None:
            self.net._want_outputs = self._want
            try:
                return self._seq.enqueue(i)
            finally:
                self.net._want_outputs = False
        if self._twin is None:
            self._build()
        net, ctx, t = self.net, self.net.ctx, self.t
        k = t & 1
        X = self.nets[k]
        if t >= 1 and not self._updated:
            self._update_for(t)
        elif t == 0:
            ctx.call("tn_stream_select", 0)
            ctx.call("tn_event_record", self._ev[0])
        else:
            ctx.call("tn_stream_select", k)
        if self._led.live:
            # the update that opens step t has summed the cost of this stream's previous step (t - 2): off it goes
            # -- also when that update already ran because something read the weights in between (sync_weights)
            self._led.issue(t, t - 2, X.d_cost, X)
        self._updated = False
        self._lr_prev = self._lr_now()
        slot = X.x
        slot.d_row0 = None
        row0 = int(i) * net.batch_sz + net.shard_lo
        if self._ord.len is not None:             # on this step's own stream, into this net's own stage
            xs, y, _ = self._ord.gather(X, row0)
            slot.bind(xs)
            slot.row0 = 0
        else:
            slot.bind(self.x_data)
            slot.row0, y = row0, self.y_data
        slot.row_global0 = net.shard_lo
        X._want_outputs = self._want
        try:
            X._train_step(y, slot.row0, pipe_stride=2)
        finally:
            X._want_outputs = False
            ctx.call("tn_stream_select", 0)
        self._last = X
        self.t = t + 1

    # -- costs a few calls late (what train.py's loop needs of a step; see _CostLedger) --------------------------
    def step_cost(self, i):
        """Enqueue step i; return [(step number, cost), ...] of the steps whose cost has become due (step numbers count
        the step_cost calls since the last drain_costs()).  With two steps in flight the cost of step t is summed by
        the launch that opens step t + 2 and handed out at call t + 4.  Do not mix with enqueue() / fn(i) before
        drain_costs()."""
        if self._seq is None and self._blocked():
            self._fall_back()                     # (collects what the ring owes) one step at a time from here on
        if self._seq is not None:
            return self._seq.step_cost(i)         # (the same ledger: the numbering goes on)
        if not self._led.live:
            self._led.open(self.t, 4)
            self._plan.restart("cost ring on")
        return self._led.step(self.t, self.enqueue, i)

    def _leave_ring(self, keep=False):
        """Everything the ledger still owes, in order: the costs taken early, the copies already under way, then the
        last two steps' costs read directly (nothing would ever open the steps that sum them).  ``keep`` (drain_costs
        at the end of an epoch): ring and recorded steps stay -- the next steps go through the interpreter until both
        streams have a cost pending again (two steps), then the recorded phases match and replay resumes."""
        led = self._led
        if not led.live:
            return led.rest(self.t)
        assert self._seq is None
        self._flush_parked()
        self.net.ctx.sync()
        out = led.rest(self.t, lambda s: np.float32(self.nets[s & 1].d_cost.get_value()[0]))
        if not keep:
            led.live = False
            self._plan.restart("cost ring off")
        return out

    def drain_costs(self):
        if self._seq is not None:
            return self._seq.drain_costs()
        out = self._leave_ring(keep=True)
        self._led.k = 0
        return out

    def fetch(self):
        if self._seq is not None:
            return self._seq.fetch()
        X = self._last
        X.ctx.call("tn_stream_select", self.nets.index(X))
        if X._dp:
            X.ctx.call("tn_event_wait", X.dp.ar_done_ev)  # the cost travels with the all-reduce (communication stream)
        try:
            early = X._early
            sent = early is not None and early["live"]
            if not (sent and early["cost_sent"]):
                self._finish_cost(X)
            if not sent:
                X.ctx.sync()
            return _step_outputs(X, X.tr_layers[-1])
        finally:
            X.ctx.call("tn_stream_select", 0)

    @staticmethod
    def _finish_cost(X):
        """The cost of X's last step, if nothing has summed it yet (on the stream currently selected)."""
        if X._cost_pending:
            X._sum_cost()
            X._cost_pending = False

    def __call__(self, i):
        self._want = True                   # features / logprob leave right after the forward pass
        try:
            self.enqueue(i)
        finally:
            self._want = False
        return self.fetch()


class _TestFn:
    """``get_test_model``'s function: ``fn(i) -> [sym_err, P(MLE)](, features, y_preds)``; ``sweep(indices)`` evaluates a
    run of minibatches with one weight sync, one collective and one copy back.  ``averaged`` (WT_AVG): a call, whatever the
    number of minibatches, evaluates at the averaged weights (NeuralNet._at_avg_wts)."""

    def __init__(self, net, x_data, y_data, preds_feats, aux_data=None, averaged=False):
        self.net, self.x_data, self.y_data, self.preds_feats = net, x_data, y_data, preds_feats
        self.aux_data = aux_data
        self.averaged = averaged        # WT_AVG: a call runs between two exchanges of weights and averages
        self._sweep_stats = None        # (len, 2) device rows of sweep(), grown when a longer sweep arrives

    def _prepare(self):
        """What a call does once, however many minibatches follow."""
        net = self.net
        net._sync_weights()
        net._apply_dtype()
        net._c8_tiles.arrange(net.te_layers)

    def _enqueue(self, i, d_stats):
        """The test graph on minibatch i and its two statistics into ``d_stats`` (2 floats); nothing is read back."""
        net, ctx = self.net, self.net.ctx
        slot = net.test_x
        slot.bind(self.x_data)
        slot.row0 = int(i) * net.batch_sz + net.shard_lo
        slot.row_global0 = net.shard_lo
        if self.aux_data is not None:                      # neuralnet.py:266-269
            net.aux_inpt_te.bind(self.aux_data)
            net.aux_inpt_te.row0 = slot.row0
        out = net.te_layers[-1]
        for lyr in net.te_layers[:-1]:
            lyr.forward(False)
        ctx.fc_head(True)
        try:
            out.forward(False, y=self.y_data, y_row0=slot.row0)
        finally:
            ctx.fc_head(False)
        ctx.call("tn_error_stats", out.y_preds.ptr, self.y_data.ptr, slot.row0, out.rowp.ptr,
                 net.local_bsz, d_stats.ptr)

    def __call__(self, i):
        _batch_in_range(i, self.x_data.shape[0], self.net.batch_sz)
        with self.net._at_avg_wts(self.averaged):
            return self._call(i)

    def _call(self, i):
        net = self.net
        self._prepare()
        out = net.te_layers[-1]
        self._enqueue(i, out.d_stats)
        if net.world.size > 1:
            net._group().allreduce_sum(out.d_stats)
        stats = out.d_stats.get_value() / net.world.size
        if net.world.size > 1:
            net._group().verify_order()      # the host has synchronised anyway: cheap point to compare
        res = [stats[0], stats[1]]
        if self.preds_feats:
            res += [out.features.get_value(), out.y_preds.get_value().astype(np.int64)]
        return res

    def sweep(self, indices):
        """``[fn(i) for i in indices]`` -- one ``[sym_err, P(MLE)]`` pair of Python floats per index, bit for bit what
        ``fn(i)`` returns at the same weights -- without a host synchronisation between the minibatches: the weights are
        brought up to date once, minibatch k leaves its statistics in row k of a device array (tn_error_stats at
        ``rows + 2 k``), data-parallel ranks sum all rows in ONE collective (element-wise: each row's sum is the one the
        per-call path forms) and one copy brings them back.  ``indices``: any finite iterable, repeats allowed; all of
        them are checked before anything is enqueued."""
        assert not self.preds_feats, "sweep() returns the two error statistics only: this function was built with " \
            "preds_feats=True (features and predictions come from fn(i), one minibatch at a time)"
        net = self.net
        indices = [int(i) for i in indices]
        for i in indices:
            _batch_in_range(i, self.x_data.shape[0], net.batch_sz)
        n = len(indices)
        if n == 0:
            return []
        with net._at_avg_wts(self.averaged):
            return self._sweep(indices)

    def _sweep(self, indices):
        net, n = self.net, len(indices)
        if self._sweep_stats is None or self._sweep_stats.shape[0] < n:
            self._sweep_stats = net.ctx.empty((n, 2))
        rows = self._sweep_stats.view(0, (n, 2))
        self._prepare()
        for k, i in enumerate(indices):
            self._enqueue(i, rows.view(2 * k, (2,)))
        if net.world.size > 1:
            net._group().allreduce_sum(rows)
        stats = rows.get_value() / net.world.size
        if net.world.size > 1:
            net._group().verify_order()
        return [[float(e), float(p)] for e, p in stats]
