"""Every form of the multi-tensor SGD update (tn_sgd_update_net / tn_sgd_update_net_maxnorm in its five modes, and
tn_step_tail) against the plain numpy reference of tests/upd_ref.py, element by element and to the last rounding -- not one
form of the update against another.  Flat gradients in every mode and flag, the pending slab stacks of a
tn_defer_reductions window folded into the LAZY / PIPE / PIPE_REG launches in every walk (16-byte, scalar by size, by
stride and by alignment, flipped, tall), each case proving from tn_defer_pending's record that it reaches the walk it
is named for.  The same file runs on the C++ backend (tests/test_update_modes_cpu.py): nothing is ever pending there
and the results must match the reference all the same."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import upd_ref as R
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from theanet_amd import _lib

pytestmark = pytest.mark.gpu

HIP = _lib.backend() == "hip"       # (the C++ backend finishes every slab sum where it is produced: no records)
PLAIN, LAZY, DELAYED, PIPE, PIPE_REG = (_lib.TN_UPD_PLAIN, _lib.TN_UPD_LAZY, _lib.TN_UPD_DELAYED, _lib.TN_UPD_PIPE,
                                        _lib.TN_UPD_PIPE_REG)
assert (PLAIN, LAZY, DELAYED, PIPE, PIPE_REG) == (R.PLAIN, R.LAZY, R.DELAYED, R.PIPE, R.PIPE_REG)
NAMES = {PLAIN: "plain", LAZY: "lazy", DELAYED: "delayed", PIPE: "pipe", PIPE_REG: "pipe_reg"}
SGD_DT = np.dtype([('p', 'u8'), ('v', 'u8'), ('g', 'u8'), ('n', 'u8'), ('momentum', 'f4'), ('rate', 'f4'), ('L1', 'f4'),
                   ('L2', 'f4')])
PIPE_DT = np.dtype([('p', 'u8'), ('psrc', 'u8'), ('v', 'u8'), ('g', 'u8'), ('n', 'u8'), ('momentum', 'f4'), ('rate', 'f4')])
REG_DT = np.dtype(PIPE_DT.descr + [('L1', 'f4'), ('L2', 'f4')])
MN_DT = np.dtype([('p', 'u8'), ('ndim', 'i4'), ('d0', 'i4'), ('rest', 'i4'), ('mx', 'f4')])
assert (SGD_DT.itemsize, PIPE_DT.itemsize, REG_DT.itemsize, MN_DT.itemsize) == (48, 48, 56, 24)
LR = .1
TERMS = ((0., 0.), (.01, 0.), (0., .02), (.003, .004))      # (L1, L2) patterns across the segments of one launch
SMALL = (1, 3, 4, 255, 256, 1023, 1024, 1025, 4099)
CAP = 2048 * 1024                                           # elements one pass of the capped grid covers
NAN = np.float32(np.nan)


def _pipe(mode):
    return mode in (PIPE, PIPE_REG)


class Tensor:
    """One operand of a segment: host values, the device array, and -- ``off`` -- a view at element 1 of a buffer of
    n + 8 elements (4 bytes off a 16-byte boundary) whose other elements must keep their bytes."""

    def __init__(self, host=None, shape=None, off=False):
        self.host = None if host is None else np.ascontiguousarray(host, np.float32)
        shape = self.host.shape if shape is None else shape
        n = int(np.prod(shape))
        self.n, self.off = n, off
        if off:
            self.outer = np.arange(n + 8, dtype=np.float32) - 7.5
            if self.host is not None:
                self.outer[1:1 + n] = self.host.reshape(-1)
            else:
                self.outer[1:1 + n] = NAN
            self.buf = dev(self.outer)
            self.d = self.buf.view(1, shape)
        elif self.host is not None:
            self.d = dev(self.host)
        else:
            self.d = empty(shape)          # poisoned by the guard: NaN
        assert (self.d.ptr & 15) == (4 if off else 0)

    @property
    def ptr(self):
        return self.d.ptr

    def get(self):
        return self.d.get_value()

    def check_outside(self, what):
        if self.off:
            got = self.buf.get_value()
            keep = np.ones(self.n + 8, bool)
            keep[1:1 + self.n] = False
            assert np.array_equal(R.bits(got[keep]), R.bits(self.outer[keep])), what + ": bytes outside the view changed"

    def check_same(self, what):
        assert np.array_equal(R.bits(self.get()), R.bits(self.host)), what + " must stay untouched"


class Seg:
    """A parameter tensor with its update operands.  p: the weights the launch writes (pipelined forms: the stepping
    stream's own copy, whose OLD values only TN_UPD_PIPE_REG reads); psrc: the other stream's copy."""

    def __init__(self, mode, shape, rng, m=.9, rate=.5, L1=0., L2=0., g=None, g_nan=False, off=None, scale=1.0):
        shape = shape if isinstance(shape, tuple) else (shape,)
        n = int(np.prod(shape))
        self.mode, self.n, self.shape = mode, n, shape
        self.m, self.rate, self.L1, self.L2 = m, rate, L1, L2

        def weights():
            w = (rng.randn(n) * scale).astype(np.float32)
            w[0] = 0.0                              # sign(+0) = 0
            if n > 2:
                w[1] = -0.0                         # sign(-0) = 0
            return w.reshape(shape)

        # TN_UPD_PIPE never reads the stepping stream's own copy: it starts as NaN there
        self.p = Tensor(shape=shape, off=off == "p") if mode == PIPE else Tensor(weights(), off=off == "p")
        self.psrc = Tensor(weights(), off=off == "psrc") if _pipe(mode) else None
        self.v = Tensor((rng.randn(*shape) * scale).astype(np.float32), off=off == "v")
        if g == "device":                           # a gradient an op will write
            self.g = Tensor(shape=shape, off=off == "g")
        elif g_nan:
            self.g = Tensor(np.full(shape, NAN), off=off == "g")
        else:
            self.g = Tensor((rng.randn(*shape) * scale).astype(np.float32), off=off == "g")

    def row(self):
        if self.mode == PIPE:
            return (self.p.ptr, self.psrc.ptr, self.v.ptr, self.g.ptr, self.n, self.m, self.rate)
        if self.mode == PIPE_REG:
            return (self.p.ptr, self.psrc.ptr, self.v.ptr, self.g.ptr, self.n, self.m, self.rate, self.L1, self.L2)
        return (self.p.ptr, self.v.ptr, self.g.ptr, self.n, self.m, self.rate, self.L1, self.L2)

    def check(self, flags, gscale, what, g_in=None):
        """What the launch left against the reference; g_in: the gradient it worked from when an op wrote it."""
        ins = dict(p=self.p.host, v=self.v.host, g=self.g.host if g_in is None else g_in, momentum=self.m, rate=self.rate,
                   L1=self.L1, L2=self.L2)
        if _pipe(self.mode):
            ins["psrc"] = self.psrc.host
            if self.p.host is None:
                ins["p"] = np.zeros(self.shape, np.float32)      # (TN_UPD_PIPE: never read, no terms)
        R.check_update(self.mode, flags, ins, self.p.get(), self.v.get(), LR, gscale, what)
        for t in (self.p, self.psrc, self.v, self.g):
            if t is not None:
                t.check_outside(what)
        if _pipe(self.mode):
            self.psrc.check_same(what + " psrc")
        if g_in is None:
            self.g.check_same(what + " g")


def _launch(mode, flags, segs, gscale=1.0, d_step=None, step_inc=0, rowloss=None, cost_scale=0.0, d_cost=None, mn=None):
    dt = {PIPE: PIPE_DT, PIPE_REG: REG_DT}.get(mode, SGD_DT)
    tab = np.array([s.row() for s in segs], dtype=dt)
    dtab = dev(tab.view(np.uint8)) if len(segs) else None
    h = tab.ctypes.data if mode in (LAZY, PIPE, PIPE_REG) and len(segs) else None
    args = (mode, dtab.ptr if dtab is not None else None, h, len(segs), max([s.n for s in segs] + [0]),
            _lr().ptr, gscale, d_step.ptr if d_step is not None else None, step_inc, flags,
            rowloss.ptr if rowloss is not None else None, rowloss.size if rowloss is not None else 0, cost_scale,
            d_cost.ptr if d_cost is not None else None)
    if mn is not None:
        mtab = np.array(mn, dtype=MN_DT)
        call("tn_sgd_update_net_maxnorm", *args, mtab.ctypes.data, len(mtab))
    else:
        call("tn_sgd_update_net", *args)


def _lr():
    return dev(np.array([LR], np.float32))


def _counter(value=7):
    return dev(np.array([value], np.uint32))


def _pending():
    """The records of the open window: [(n, S, stride, flip)]."""
    c = ctx()
    rec = (ctypes.c_uint32 * 4)()
    n = c.lib.tn_defer_pending(c.h, -1, None)
    out = []
    for i in range(n):
        assert c.lib.tn_defer_pending(c.h, i, rec) == n
        out.append(tuple(int(x) for x in rec))
    return out


def _flat_segments(mode, rng, sizes, g_nan=False):
    """Segment i: term pattern i % 4, momentum .9 / 0 in turns of four, two rates -- every (pattern, momentum) pair occurs
    in the nine small tensors of one launch."""
    segs = []
    for i, n in enumerate(sizes):
        L1, L2 = TERMS[i % 4]
        segs.append(Seg(mode, n, rng, m=(.9, 0.)[(i // 4) % 2], rate=(.5, 1.25)[i % 2], L1=L1, L2=L2, g_nan=g_nan))
    return segs


FLAT = ([(PLAIN, 0, gs) for gs in (1.0, 1 / 3)] + [(LAZY, 0, gs) for gs in (1.0, 1 / 3)] +
        [(DELAYED, f, gs) for f in (1, 3, 1 | 4, 3 | 4) for gs in (1.0, 1 / 3)] + [(DELAYED, 2, 1.0)] +
        [(PIPE, 0, 1.0), (PIPE, 1, 1.0), (PIPE_REG, 0, 1.0), (PIPE_REG, 1, 1.0)])


@pytest.mark.parametrize("mode,flags,gscale", FLAT, ids=["%s-%d-%s" % (NAMES[m], f, "third" if g != 1 else "one")
                                                        for m, f, g in FLAT])
def test_flat_gradients_against_the_reference(mode, flags, gscale):
    """One launch over ten unequal tensors (blockIdx.y picks the descriptor, max_n sizes the shared grid), the last one
    past the grid cap of 2048 blocks x 1024 elements so that the grid-stride loop runs a second trip."""
    rng = np.random.RandomState(100 * mode + flags)
    big = CAP + (4096 if _pipe(mode) else 1027)          # the 16-byte walks of the pipelined forms / the scalar walks
    nan_g = _pipe(mode) and not flags & 1                # the first two pipelined steps: no gradient yet
    segs = _flat_segments(mode, rng, SMALL + (big,), g_nan=nan_g)
    step = _counter()
    _launch(mode, flags, segs, gscale, d_step=step, step_inc=1)
    assert step.get_value()[0] == 8
    for s in segs:
        s.check(flags, gscale, "%s flags %d n %d (L1 %g L2 %g m %g)" % (NAMES[mode], flags, s.n, s.L1, s.L2, s.m))


@pytest.mark.parametrize("off", [None, "p", "psrc", "v", "g"])
@pytest.mark.parametrize("mode,terms", [(PIPE, (0., 0.)), (PIPE_REG, (0., 0.)), (PIPE_REG, (.003, .004))],
                         ids=["pipe", "pipe_reg-no-terms", "pipe_reg-terms"])
def test_pipelined_walks_choose_by_alignment(mode, terms, off):
    """The 16-byte walk is chosen by (p | psrc | v | g) & 15: the same tensor with all four pointers aligned, then with
    exactly one of them 4 bytes off -- a view at element 1 of a larger buffer, whose other elements must keep their
    bytes (a vector access on the shifted tensor would reach them)."""
    rng = np.random.RandomState(7)
    segs = [Seg(mode, 2052, rng, L1=terms[0], L2=terms[1], off=off), Seg(mode, 8, rng, L1=terms[0], L2=terms[1], off=off)]
    _launch(mode, 1, segs)
    for s in segs:
        s.check(1, 1.0, "%s n %d with %s shifted" % (NAMES[mode], s.n, off))


COUNTER = [(PLAIN, 0, 1), (LAZY, 0, 1), (DELAYED, 1, 1), (DELAYED, 2, 1), (DELAYED, 3 | 4, 1)] + \
          [(m, f, inc) for m in (PIPE, PIPE_REG) for f in (0, 1) for inc in (0, 1, 2)]


@pytest.mark.parametrize("mode,flags,inc", COUNTER, ids=["%s-%d-inc%d" % (NAMES[m], f, i) for m, f, i in COUNTER])
def test_step_counter(mode, flags, inc):
    """*d_step += step_inc in the same launch; with d_step == NULL nothing else changes."""
    outs = []
    for with_counter in (True, False):
        segs = _flat_segments(mode, np.random.RandomState(3), SMALL)
        step = _counter()
        _launch(mode, flags, segs, 1.0, d_step=step if with_counter else None, step_inc=inc)
        assert step.get_value()[0] == (7 + inc if with_counter else 7)
        outs.append([R.bits(t.get()) for s in segs for t in (s.p, s.v)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", [PLAIN, LAZY, PIPE, PIPE_REG], ids=lambda m: NAMES[m])
def test_cost_rider(mode):
    """*d_cost = cost_scale * sum(rowloss) by one more block of the launch, alone (nseg == 0) and beside segments."""
    for nrow in (1, 63, 64, 255, 256, 257, 1000):
        rng = np.random.RandomState(nrow)
        rl = (rng.rand(nrow) * 3).astype(np.float32)            # non-negative: upd_ref.check_cost's bound
        rld, scale = dev(rl), 1.0 / nrow
        cost = dev(np.array([NAN], np.float32))
        _launch(mode, 1, [], rowloss=rld, cost_scale=scale, d_cost=cost)
        R.check_cost(cost.get_value(), rl, scale, "%s alone, %d rows" % (NAMES[mode], nrow))
        cost = dev(np.array([NAN], np.float32))
        segs = _flat_segments(mode, rng, (5, 1024, 1500))
        step = _counter()
        _launch(mode, 1, segs, d_step=step, step_inc=1, rowloss=rld, cost_scale=scale, d_cost=cost)
        R.check_cost(cost.get_value(), rl, scale, "%s beside three segments, %d rows" % (NAMES[mode], nrow))
        assert step.get_value()[0] == 8
        for s in segs:
            s.check(1, 1.0, "%s beside the rider n %d" % (NAMES[mode], s.n))
        assert np.array_equal(rld.get_value(), rl)


# ---- pending slab stacks folded into the update -------------------------------------------------------------
class FcWgrad:
    """tn_fc_wgrad; inputs and the bound on dW / db of test_fc_wgrad_large_batch_split_k."""

    def __init__(self, B, n_in, n_out):
        self.key = ("fc", B, n_in, n_out)
        self.B, self.n_in, self.n_out = B, n_in, n_out
        self.shapes = ((n_in, n_out), (n_out,))

    @functools.lru_cache(maxsize=None)
    def host(self):
        rng = np.random.RandomState(self.B + self.n_in)
        x = rng.rand(self.B, self.n_in).astype(np.float32)
        dz = (rng.randn(self.B, self.n_out) / self.B).astype(np.float32)
        return x, dz, x.astype(np.float64).T @ dz.astype(np.float64), dz.astype(np.float64).sum(0)

    def want(self):
        return self.host()[2:]

    def tol(self, want):
        return dict(atol=1e-5)

    def prepare(self):
        x, dz = self.host()[:2]
        self.dev = (dev(x), dev(dz), empty((ctx().lib.tn_fc_wgrad_ws_bytes(self.B, self.n_in, self.n_out) // 4 + 1,)))

    def run(self, gW, gb):
        x, dz, ws = self.dev
        call("tn_fc_wgrad", x.ptr, dz.ptr, gW.ptr, gb.ptr, self.B, self.n_in, self.n_out, ws.ptr)


class ConvWgrad:
    """tn_conv2d_wgrad ('valid', stride 1); inputs and the bound on dW / db of test_conv_wgrad_dgrad."""

    def __init__(self, N, C, H, K, f):
        self.key = ("conv", N, C, H, K, f)
        self.N, self.C, self.H, self.K, self.f = N, C, H, K, f
        self.out = H - f + 1
        self.shapes = ((K, C, f, f), (K,))

    @functools.lru_cache(maxsize=None)
    def host(self):
        rng = np.random.RandomState(self.N + self.K)
        x = rng.randn(self.N, self.C, self.H, self.H).astype(np.float32)
        dz = rng.randn(self.N, self.K, self.out, self.out).astype(np.float32)
        W = np.zeros(self.shapes[0])
        _, dW, db = O.conv2d_bwd(x.astype(np.float64), W, dz.astype(np.float64), 1, "valid", need_dx=False)
        return x, dz, dW, db

    def want(self):
        return self.host()[2:]

    def tol(self, want):
        return dict(atol=max(1e-4, 2e-6 * np.abs(want).max()))

    def prepare(self):
        x, dz = self.host()[:2]
        self.dev = (dev(x), dev(dz))

    def run(self, gW, gb):
        x, dz = self.dev
        call("tn_conv2d_wgrad", x.ptr, dz.ptr, gW.ptr, gb.ptr, self.N, self.C, self.H, self.H, self.K, self.f, 1, 0,
             self.out, self.out)


class ConvpoolBwdMask:
    """tn_convpool_bwd_mask behind tn_convpool_fwd_mask (f = 3, 2 x 2 pooling, 'valid'); inputs and the bound on dW / db of
    test_convpool_mask_backward.  The C++ backend has no fused blocks (its capability queries answer 0): there the weight
    gradient of the same block is tn_conv2d_wgrad on the reference's dz."""

    def __init__(self, N, C, H, K, act):
        self.key = ("convpool", N, C, H, K, act)
        self.N, self.C, self.H, self.K, self.act = N, C, H, K, act
        self.Ho = H - 2
        self.Hp = O.pool_out_sz(self.Ho, 2, False)
        self.shapes = ((K, C, 3, 3), (K,))

    @functools.lru_cache(maxsize=None)
    def host(self):
        N, C, H, K = self.N, self.C, self.H, self.K
        rng = np.random.RandomState(N * 13 + K)
        x = rng.randn(N, C, H, H).astype(np.float32)
        W = (rng.randn(K, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32)
        b = rng.randn(K).astype(np.float32)
        fa, dfa = O.activation(self.act)
        x64, W64 = x.astype(np.float64), W.astype(np.float64)
        z = O.conv2d_fwd(x64, W64, b.astype(np.float64), 1, "valid")
        g = rng.randn(N, K, self.Hp, self.Hp).astype(np.float32)
        dz = O.pool_bwd(fa(z), g.astype(np.float64), 2, False) * dfa(z)
        _, dW, db = O.conv2d_bwd(x64, W64, dz, 1, "valid", need_dx=False)
        return x, W, b, g, dW, db, dz.astype(np.float32)

    def want(self):
        return self.host()[4:6]

    def tol(self, want):
        return dict(atol=max(2e-4, 2e-6 * np.abs(want).max()))

    def prepare(self):
        x, W, b, g = self.host()[:4]
        kind, prm = act_code(self.act)
        self.geom = (self.N, self.C, self.H, self.H, self.K, 3, 0, self.Ho, self.Ho, 2, self.Hp, self.Hp, kind, prm)
        xd, gd = dev(x), dev(g)
        if not HIP:
            self.dev = (xd, dev(self.host()[6]))
            return
        y, mask = empty((self.N, self.K, self.Hp, self.Hp)), empty((self.N, self.K, self.Hp, self.Hp), np.uint8)
        call("tn_convpool_fwd_mask", xd.ptr, dev(W).ptr, dev(b).ptr, y.ptr, mask.ptr, *self.geom)
        self.dev = (xd, gd, y, mask)

    def run(self, gW, gb):
        if not HIP:
            xd, dzd = self.dev
            call("tn_conv2d_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, self.N, self.C, self.H, self.H, self.K, 3, 1, 0, self.Ho,
                 self.Ho)
            return
        xd, gd, y, mask = self.dev
        call("tn_convpool_bwd_mask", xd.ptr, gd.ptr, y.ptr, mask.ptr, None, gW.ptr, gb.ptr, *self.geom)


def _is(n=None, S=None, stride=None, flip=None, vec=None, tall=None):
    """A predicate on a record (n, S, stride, flip): the properties a case is named for.

    What the record proves: n, S, stride and flip are what the update launch dispatches on, so tall / flipped / "scalar
    because of n or stride" follow from it alone.  What it cannot prove: the kernels' 16-byte condition also asks for
    16-byte aligned pointers.  Those of p, psrc, v and g are the test's own (``aligned``, asserted in Tensor); that of
    the slab source (rec.src: the op's workspace or the context's scratch, both 256-byte aligned allocations today) is
    not in the record.  ``vec=True`` therefore says "nothing in the record or in the test's pointers forces the scalar
    walk"; were the library ever to hand out slab memory that is not 16-byte aligned, such a case would take the scalar
    walk without this predicate noticing -- and would still have to match the reference."""
    def pred(rec, aligned=True):
        rn, rS, rstride, rflip = rec
        walk_vec = aligned and rflip == 0 and rn % 4 == 0 and rstride % 4 == 0 and rS <= 32
        ok = all(want is None or got == want for got, want in ((rn, n), (rS, S), (rstride, stride), (rflip, flip)))
        return ok and (vec is None or walk_vec == vec) and (tall is None or (rS > 32) == tall)
    return pred


# name -> (op, what the dW record must be, v of the stacked tensor 4 bytes off)
SLABS = {
    "vec16": (FcWgrad(1024, 128, 96), _is(n=12288, S=8, stride=12288, flip=0, vec=True), False),
    "scalar_by_size": (FcWgrad(1024, 33, 35), _is(n=1155, S=8, stride=1155, flip=0, vec=False), False),
    "scalar_by_alignment": (FcWgrad(1024, 128, 96), _is(n=12288, S=8, stride=12288, flip=0, vec=False), True),
    "flipped": (ConvWgrad(8, 3, 32, 5, 3), _is(n=135, S=2, stride=135, flip=9, vec=False, tall=False), False),
    "flipped_n_mod_4_is_0": (ConvWgrad(8, 3, 32, 4, 3), _is(n=108, S=2, stride=108, flip=9, vec=False, tall=False), False),
    "tall": (ConvWgrad(64, 3, 50, 5, 3), _is(n=135, S=36, stride=135, flip=9, tall=True), False),
    "block_backward": (ConvpoolBwdMask(3, 2, 9, 3, "sigmoid"), _is(n=54, stride=54, flip=9, vec=False), False),
    # the dense layers of at most 16 outputs keep a slab's bias row behind its weight rows: stride != n
    "stride_is_not_n_scalar": (FcWgrad(300, 20, 10), _is(n=200, S=3, stride=210, flip=0, vec=False), False),
    "stride_is_not_n_vec16": (FcWgrad(300, 20, 12), _is(n=240, S=3, stride=252, flip=0, vec=True), False),
}


@functools.lru_cache(maxsize=None)
def _unfused(name):
    """The op outside a window: its own finishing sums, (dW, db)."""
    op = SLABS[name][0]
    op.prepare()
    gW, gb = empty(op.shapes[0]), empty(op.shapes[1])
    op.run(gW, gb)
    return gW.get_value(), gb.get_value()


def _slab_case(name, mode, flags=1, layout="seg0", terms=None):
    """Steps 1 .. 8 of a slab case; returns the records seen.  Segments: the stacked tensor, its bias (a stack of its
    own), and a flat tensor that never had a stack; the step counter and a cost rider ride along.  TN_UPD_LAZY has the
    whole of PLAIN's expression behind the slab sum: there the stacked tensor carries both terms and gscale is 1/3."""
    op, pred, v_off = SLABS[name]
    if terms is None:
        terms = TERMS[3] if mode == LAZY else (0., 0.)
    gscale = 1 / 3 if mode == LAZY else 1.0
    unf = _unfused(name)
    op.prepare()
    rng = np.random.RandomState(len(name) + mode)
    sW = Seg(mode, op.shapes[0], rng, L1=terms[0], L2=terms[1], g="device", off="v" if v_off else None, scale=.1)
    sb = Seg(mode, op.shapes[1], rng, m=0., rate=1.25, g="device")
    sf = Seg(mode, 777, rng, L1=TERMS[1][0] if mode != PIPE else 0.)
    segs = {"seg0": [sW, sb, sf], "seg1": [sf, sW, sb], "maxnorm": [sW, sb, sf]}[layout]
    # a bound no column reaches: the projection's factor is exactly 1 and the weights stay what the update left (so the
    # column sums of squares the launch leaves are NOT checked here: test_update_with_column_norm_rider_* checks them)
    mn = [(sW.p.ptr, 2, op.shapes[0][0], op.shapes[0][1], 1e3)] if layout == "maxnorm" else None
    rl = (rng.rand(300) * 2).astype(np.float32)
    rld, cost, step = dev(rl), dev(np.array([NAN], np.float32)), _counter()
    call("tn_defer_reductions", 1)
    op.run(sW.g.d, sb.g.d)
    recs = _pending()
    if HIP:
        assert len(recs) == 2 and recs[0][0] == sW.n and recs[1][0] == sb.n, recs
        assert pred(recs[0], aligned=not v_off), (name, recs)
    else:
        assert recs == []
    _launch(mode, flags, segs, gscale, d_step=step, step_inc=2 if _pipe(mode) else 1, rowloss=rld, cost_scale=1 / 300,
            d_cost=cost, mn=mn)
    assert _pending() == []
    call("tn_defer_reductions", 0)
    gW, gb = sW.g.get(), sb.g.get()
    for got, want, what in zip((gW, gb), op.want(), ("dW", "db")):
        assert_close(got, want, what="%s %s from the slab stack" % (name, what), **op.tol(want))
    if op.shapes[0][-1] == 3 and len(op.shapes[0]) == 4:        # (and not the correlation layout a vector walk would leave)
        wrong = np.abs(gW.astype(np.float64) - op.want()[0][:, :, ::-1, ::-1])
        assert wrong.max() > 10 * op.tol(op.want()[0])["atol"]
    assert np.array_equal(R.bits(gW), R.bits(unf[0])) and np.array_equal(R.bits(gb), R.bits(unf[1])), \
        name + ": the folded slab sum and the reduction launch disagree"
    what = "%s %s %s" % (name, NAMES[mode], layout)
    sW.check(flags, gscale, what + " W", g_in=gW)
    sb.check(flags, gscale, what + " b", g_in=gb)
    sf.check(flags, gscale, what + " flat")
    assert step.get_value()[0] == (9 if _pipe(mode) else 8)
    R.check_cost(cost.get_value(), rl, 1 / 300, what)
    return recs


@pytest.mark.parametrize("mode", [LAZY, PIPE], ids=lambda m: NAMES[m])
@pytest.mark.parametrize("name", list(SLABS))
def test_pending_slab_stack_folded_into_the_update(name, mode):
    recs = _slab_case(name, mode)
    print("records of %s (%s): %s" % (name, NAMES[mode], recs))


@pytest.mark.parametrize("mode", [LAZY, PIPE], ids=lambda m: NAMES[m])
@pytest.mark.parametrize("layout", ["seg1", "maxnorm"])
def test_stacked_tensor_in_other_places_of_the_launch(layout, mode):
    """The 16-byte case with the stacked tensor as segment 1 (segment 0 flat: the counter advances in the flat block row)
    and as a max-norm tensor of tn_sgd_update_net_maxnorm; test_pending_slab_stack_folded_into_the_update has it as
    segment 0 (the slab branch).  By colnorm_pick's rules (2-D, columns % 4 == 0, aligned operands, no flip, S <= 32) the
    column-norm walk takes the max-norm tensor and the counter then advances in the update kernel's early return; the
    test cannot observe which kernel walked the tensor, and with a bound no column reaches it does not check the column
    sums either (test_update_with_column_norm_rider_* do) -- it checks g, v, p, the counter and the cost."""
    _slab_case("vec16", mode, layout=layout)


@pytest.mark.parametrize("terms", [(0., 0.), (.003, .004)], ids=["no-terms", "terms"])
@pytest.mark.parametrize("name", ["vec16", "flipped"])
def test_pending_slab_stack_under_pipe_reg(name, terms):
    """Zero terms: the stack is folded in; non-zero terms: the reduction launch runs first, then the flat walk with the
    terms at the old p_own.  Either way nothing is pending afterwards."""
    _slab_case(name, PIPE_REG, terms=terms)


def test_pipe_without_velocity_update_leaves_a_pending_stack_to_the_reduction():
    """TN_UPD_PIPE with flags 0 and a stack pending: the gradient is finished by the reduction launch (the unfused bits),
    the velocity stays, p = psrc - step * v."""
    _slab_case("vec16", PIPE, flags=0)


# ---- tn_step_tail -------------------------------------------------------------------------------------------
def test_step_tail_is_the_plain_update_beside_the_next_field():
    h = w = 13                  # the smallest field of test_elastic_field_gen_equals_two_launches
    field = (h, w, 2.0, 1.1, 60.0, 4, 5.0, 0)
    seed, lib = 0x1234_5678_9abc, ctx().lib
    rng = np.random.RandomState(21)
    segs = _flat_segments(PLAIN, rng, (5, 1024, 1500))
    rl = (rng.rand(257) * 2).astype(np.float32)
    rld, cost, step = dev(rl), dev(np.array([NAN], np.float32)), _counter()
    outs = []
    for tail in (True, False):
        draws = empty((lib.tn_elastic_draws_count(h, w),))
        mi, fy, fx, tgt = empty((h * w,), np.int32), empty((h * w,)), empty((h * w,)), empty((2 * h * w,), np.float64)
        if tail:
            tab = np.array([s.row() for s in segs], dtype=SGD_DT)
            call("tn_step_tail", dev(tab.view(np.uint8)).ptr, len(segs), max(s.n for s in segs), _lr().ptr, 1 / 3, rld.ptr,
                 rl.size, 1 / 257, cost.ptr, draws.ptr, seed, step.ptr, *field, mi.ptr, fy.ptr, fx.ptr, tgt.ptr)
        else:
            call("tn_elastic_field_gen", draws.ptr, seed, 0, step.ptr, *field, mi.ptr, fy.ptr, fx.ptr, tgt.ptr)
        outs.append([a.get_value() for a in (draws, mi, fy, fx, tgt)])
    assert step.get_value()[0] == 7                     # (the caller has advanced it already)
    for a, b, what in zip(outs[0], outs[1], ("draws_out", "map_idx", "map_fy", "map_fx", "target")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    for s in segs:
        s.check(0, 1 / 3, "step tail n %d" % s.n)
    R.check_cost(cost.get_value(), rl, 1 / 257, "step tail")
