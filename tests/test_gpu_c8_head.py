"""An output head on the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16', training param STACK_HEAD 'any'): the ops
tn_c8_head_fwd / tn_c8_head_softmax_nll through the C-ABI against numpy's stored-16-bit statement (the references of
tests/test_gpu_c8_fcg.py::_ops: _rowmap, Wp, the rounding of the element type), their refusals, and nets whose head sits
directly on a stack tensor against the stored-16-bit oracle.

The oracle is taught from outside, as tests/test_gpu_c8_dropout.py::_oracle_16 teaches it the DropOutLayer (_teach_head):
OracleNet.forward already rounds a head's operands above Conv / Pool, OracleNet.backward states the stored-16-bit gradient
only for kind "Hidden".  A head on the stack does what that branch does with dz the head's own: dz16 = r16(grad_scale dz),
dW = r16(x)^T dz16 / scale, db = sum dz16 / scale, a learn_centers gradient stays the row kernel's, SoftAux's aux and cross
terms stay fp32, and _f16_down(dz16 r16(W)^T) goes down.

Tolerances: z 2e-5 of the largest entry (the project's bound for fp32 results of this arithmetic: operands rounded to the
16-bit type, exact products, fp32 accumulation); the softmax rows the bounds of tests/test_gpu_kernels.py::_fc_nll_check
(assert_close's defaults, dz atol 1e-7) against the float64 log-softmax of the reference z; nets TOL of
tests/test_gpu_c8_mean.py; repeated calls, the two ops' logits and the schedules bit for bit."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import ROOT, act_code, assert_close, call, ctx, dev
from tests.test_gpu_c8 import _rowmap
from tests.test_gpu_c8_conv1 import _R, _rel
from tests.test_gpu_c8_dropout import _oracle_16
from tests.test_gpu_c8_fcg import _bits
from tests.test_gpu_c8_mean import GS, R16, TOL
from tests.test_gpu_c8_pool import _teach_pool
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["float16", "bfloat16"])
def dtype(request, monkeypatch):
    """The element type; for bfloat16 the oracle's stored-16-bit mode rounds to bf16 (tests/test_gpu_c8_mean.py)."""
    if request.param == "bfloat16":
        monkeypatch.setattr(O, "r16", CB.rbf16)
    ctx().set_matmul_dtype(request.param, GS[request.param])
    yield request.param
    monkeypatch.setattr(O, "r16", R16)
    ctx().set_matmul_dtype("float32")


# ---------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------
# (B, C, HW, n_out)
CASES = [(3, 1, 1, 1),              # one cell, one output
         (4, 10, 1, 5),             # HW 1, a partial second octet
         (7, 3, 25, 10),            # C < 8, 25 cells, HW not a power of two
         (20, 20, 36, 3),
         (37, 32, 49, 10),          # row tail 5
         (130, 24, 9, 16),          # all 16 columns
         (16, 64, 64, 10),          # exact tile, 128 steps
         (300, 128, 16, 13)] + [(21, 16, 9, n) for n in range(1, 17)]
ACTS = ("linear", "sigmoid", "scaled_tanh")      # the heads' activations


def c8_head_launches():
    """(op, B, C, HW, n_out) of every launch of test_c8_head_ops_match_numpy (op 0 tn_c8_head_fwd, 1
    tn_c8_head_softmax_nll): what tests/test_c8_head_cpu.py holds against tn_c8_head_plan."""
    return [(op,) + c for c in CASES for op in (0, 1)]


def _poison(shape, dt=np.float32):
    return dev(np.full(shape, 0xFF, np.uint8).repeat(np.dtype(dt).itemsize, axis=-1).view(dt))


def _operands(case, dtype):
    B, C, HW, N = case
    R = _R(dtype)
    rng = np.random.RandomState(1 + N)
    rm = _rowmap(C, HW)
    Kc, n_in, ok = len(rm), C * HW, rm >= 0
    x = np.zeros((B, Kc)); x[:, ok] = R(rng.randn(B, n_in))[:, rm[ok]]
    W = (rng.randn(n_in, N) / np.sqrt(n_in)).astype(np.float32)
    b = (rng.randn(N) * .1).astype(np.float32)
    Wp = np.zeros((Kc, N)); Wp[ok] = R(W)[rm[ok]]
    return x @ Wp + b, dev(_bits(x, dtype)), dev(W), dev(b)


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_c8_head_ops_match_numpy(dtype, case):
    B, C, HW, N = case
    assert ctx().lib.tn_c8_head_supported(*case)
    z, xd, Wd, bd = _operands(case, dtype)
    # tn_c8_head_fwd over poisoned outputs, twice: the same bits
    lin = None
    for name in ACTS:
        act, prm = act_code(name)
        want = O.activation(name)[0](z)
        a, a2 = _poison((B, N)), _poison((B, N))
        call("tn_c8_head_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, C, HW, N, act, prm)
        call("tn_c8_head_fwd", xd.ptr, Wd.ptr, bd.ptr, a2.ptr, B, C, HW, N, act, prm)
        got = a.get_value()
        e = _rel(got, want)
        print("fwd %s: %.3g" % (name, e))
        assert e < 2e-5
        np.testing.assert_array_equal(got.view(np.uint32), a2.get_value().view(np.uint32))
        if name == "linear":
            lin = got
    # tn_c8_head_softmax_nll: labels at y_row0 = 5, and once through d_row0
    rng = np.random.RandomState(B + N)
    y = rng.randint(0, N, size=B + 5).astype(np.int32)
    lab, r = y[5:], np.arange(B)
    lp = O.log_softmax(z)
    onehot = np.zeros((B, N)); onehot[r, lab] = 1
    yd, d3 = dev(y), dev(np.array([3], np.int64))
    for y_row0, d_row0 in ((5, None), (2, d3.ptr)):
        logits, logprob, dz = _poison((B, N)), _poison((B, N)), _poison((B, N))
        rowloss, rowp, pred = _poison((B,)), _poison((B,)), _poison((B,), np.int32)
        call("tn_c8_head_softmax_nll", xd.ptr, Wd.ptr, bd.ptr, logits.ptr, B, C, HW, N, yd.ptr, y_row0, d_row0, logprob.ptr,
             rowloss.ptr, pred.ptr, rowp.ptr, dz.ptr, 1.0 / B)
        np.testing.assert_array_equal(logits.get_value().view(np.uint32), lin.view(np.uint32))
        e = _rel(logits.get_value(), z)
        print("logits: %.3g" % e)
        assert e < 2e-5
        assert_close(logprob.get_value(), lp, what="logprob")
        assert_close(rowloss.get_value(), -lp[r, lab], what="rowloss")
        assert_close(rowp.get_value(), np.exp(lp[r, lab]), what="P(label)")
        assert_close(dz.get_value(), (np.exp(lp) - onehot) / B, atol=1e-7, what="dlogits")
        got, best = pred.get_value(), z.max(1)
        assert ((got >= 0) & (got < N)).all()
        assert np.all(np.abs(z[r, got] - best) <= 1e-5 * np.maximum(1, np.abs(best)))
    full = (logprob.get_value(), pred.get_value(), rowloss.get_value(), rowp.get_value(), dz.get_value())
    # the forms with NULL outputs: no labels at all (test graphs); labels, each optional output left out
    for args in ((None, 0, None, None, None, None), (yd.ptr, 5, None, None, None, None),
                 (yd.ptr, 5, None, "rowloss", None, None), (yd.ptr, 5, None, None, "rowp", None),
                 (yd.ptr, 5, None, None, None, "dz")):
        logits, logprob, pred = _poison((B, N)), _poison((B, N)), _poison((B,), np.int32)
        bufs = {"rowloss": _poison((B,)), "rowp": _poison((B,)), "dz": _poison((B, N))}
        yp, y0, d0, *outs = args
        ptrs = [bufs[o].ptr if o else None for o in outs]
        call("tn_c8_head_softmax_nll", xd.ptr, Wd.ptr, bd.ptr, logits.ptr, B, C, HW, N, yp, y0, d0, logprob.ptr, ptrs[0],
             pred.ptr, ptrs[1], ptrs[2], 1.0 / B)
        np.testing.assert_array_equal(logits.get_value().view(np.uint32), lin.view(np.uint32))
        np.testing.assert_array_equal(logprob.get_value().view(np.uint32), full[0].view(np.uint32))
        np.testing.assert_array_equal(pred.get_value(), full[1])
        for o, want in zip(outs, full[2:]):
            if o:
                np.testing.assert_array_equal(bufs[o].get_value().view(np.uint32), want.view(np.uint32))


def test_c8_head_ops_refuse_bad_arguments(dtype):
    from theanet_amd import _lib
    lib = ctx().lib
    B, C, HW, N = 4, 10, 1, 5
    Kc = 16
    x = dev(np.zeros((B, Kc), np.uint16))
    W, b = dev(np.zeros((C * HW, 16), np.float32)), dev(np.zeros((16,), np.float32))
    y = dev(np.zeros((B,), np.int32))
    z, lp, dz = (dev(np.full((B, 17), 7., np.float32)) for _ in range(3))
    rl, rp, pr = dev(np.full((B,), 7., np.float32)), dev(np.full((B,), 7., np.float32)), dev(np.full((B,), 7, np.int32))
    huge = ((1 << 20, 8, 1 << 12, 8), (1 << 23, 8, 1, 8), (4, 1 << 20, 1 << 10, 8), (4, 8, 1 << 17, 1 << 14),
            (1 << 28, 8, 1, 8))

    def nll(xp, Wp, bp, zp, shape, yp, lpp, rlp, prp, rpp, dzp):
        call("tn_c8_head_softmax_nll", xp, Wp, bp, zp, *shape, yp, 0, None, lpp, rlp, prp, rpp, dzp, .25)

    bad = ((B, C, HW, 0), (B, C, HW, 17), (0, C, HW, N), (B, 0, HW, N), (B, C, 0, N), (-1, C, HW, N), (B, -3, HW, N),
           (B, C, -1, N)) + huge
    for s in bad:
        assert not lib.tn_c8_head_supported(*s), s
        with pytest.raises(_lib.BackendError, match="tn_c8_head_fwd"):
            call("tn_c8_head_fwd", x.ptr, W.ptr, b.ptr, z.ptr, *s, 0, 0.)
        with pytest.raises(_lib.BackendError, match="tn_c8_head_softmax_nll"):
            nll(x.ptr, W.ptr, b.ptr, z.ptr, s, y.ptr, lp.ptr, rl.ptr, pr.ptr, rp.ptr, dz.ptr)
    g = (B, C, HW, N)
    assert lib.tn_c8_head_supported(*g)
    for args in ((None, W.ptr, b.ptr, z.ptr), (x.ptr, None, b.ptr, z.ptr), (x.ptr, W.ptr, None, z.ptr), (x.ptr, W.ptr, b.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_head_fwd"):
            call("tn_c8_head_fwd", *args, *g, 0, 0.)
        with pytest.raises(_lib.BackendError, match="tn_c8_head_softmax_nll"):
            nll(*args, g, y.ptr, lp.ptr, rl.ptr, pr.ptr, rp.ptr, dz.ptr)
    with pytest.raises(_lib.BackendError, match="tn_c8_head_softmax_nll"):
        nll(x.ptr, W.ptr, b.ptr, z.ptr, g, y.ptr, None, rl.ptr, pr.ptr, rp.ptr, dz.ptr)           # logprob
    with pytest.raises(_lib.BackendError, match="tn_c8_head_softmax_nll"):
        nll(x.ptr, W.ptr, b.ptr, z.ptr, g, y.ptr, lp.ptr, rl.ptr, None, rp.ptr, dz.ptr)           # pred
    with pytest.raises(_lib.BackendError, match="tn_c8_head_softmax_nll"):
        nll(x.ptr, W.ptr, b.ptr, z.ptr, g, None, lp.ptr, rl.ptr, pr.ptr, None, None)              # a loss without labels
    ctx().sync()
    for t in (z, lp, dz, rl, rp):
        assert (t.get_value() == 7.).all()                                                       # nothing was launched
    assert (pr.get_value() == 7).all()


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
B = 16
TP = {"SEED": 7, "BATCH_SZ": B, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2, "STACK_HEAD": "any"}
NCLS = 10


def _conv(k, f, mode="same"):
    return ("ConvLayer", {"num_maps": k, "filter_sz": f, "stride": 1, "mode": mode, "actvn": "relu10"})


POOL = ("PoolLayer", {"pool_sz": 2})
# name -> (layers under the head, input maps, input side)
STACKS = {
    # 24 maps of 3x3 stored at pitch 4: the head reads the cropped copy and embeds its input gradient
    "padded": ([("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(16, 3), POOL, _conv(24, 1, "valid"), POOL], 3, 12),
    # 8 maps of 8x8, dense: no detour
    "dense": ([("InputLayer", {"img_sz": 16, "num_maps": 1}), _conv(8, 3), POOL], 1, 16),
    "dropout": ([("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(16, 3), POOL, _conv(24, 1, "valid"), POOL,
                 ("DropOutLayer", {"pdrop": .25})], 3, 12),
    "pool3": ([("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(16, 3), ("PoolLayer", {"pool_sz": 3})], 3, 12),
    # the net tests/test_gpu_c8.py::test_c8_unsupported_shapes_are_errors_not_fallbacks builds (refused without STACK_HEAD)
    "conv": ([("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16, 3)], 3, 16),
}
AUX = {"n_aux": (4, 3), "aux_type": "LocationInfo", "boost": 1.5}
HEADS = {
    "softmax-nll": ("SoftmaxLayer", {"n_out": NCLS}),
    "softmax-nllsq": ("SoftmaxLayer", {"n_out": NCLS, "loss": "nllsq"}),
    "softmax-hinge": ("SoftmaxLayer", {"n_out": NCLS, "loss": "hinge"}),
    "exploss": ("ExpLossLayer", {"n_out": NCLS}),
    "hinge": ("HingeLayer", {"n_out": NCLS}),
    "logit": ("CenteredOutLayer", {"n_features": 12, "n_classes": NCLS, "kind": "LOGIT"}),
    # 20 features: beyond the head kernels, the dense family's forward + the row kernel
    "rbf-learn": ("CenteredOutLayer", {"n_features": 20, "n_classes": NCLS, "kind": "RBF", "learn_centers": True, "junk_dist": 3.0}),
    "softaux": ("SoftAuxLayer", dict(AUX, n_out=NCLS)),
}
NETS = [("padded", h) for h in HEADS] + [(s, "softmax-nll") for s in ("dense", "dropout", "pool3", "conv")]


def _layers(stack, head):
    lyrs, C, img = STACKS[stack]
    return copy.deepcopy(lyrs) + [copy.deepcopy(HEADS[head])], C, img


def _tr(tp, dtype):
    return dict(tp, DTYPE=dtype, GRAD_SCALE=GS[dtype]) if dtype in GS else dict(tp, DTYPE=dtype)


def _data(C, img, n=2, seed=1):
    rng = np.random.RandomState(seed)
    return (rng.rand(n * B, C, img, img).astype(np.float32), rng.randint(0, NCLS, n * B).astype(np.int32),
            rng.rand(n * B, 2, 2).astype(np.float32))


def _teach_head(monkeypatch, ora):
    """The stored-16-bit oracle taught an output head on the stack, from outside (module docstring).  Goes on top of
    _oracle_16 / _teach_pool: their forward and _f16_down are the ones called here."""
    hi = len(ora.L) - 1
    head, kinds = ora.L[hi], [l.kind for l in ora.L]
    assert kinds[hi - 1] in ("Conv", "Pool", "DropOut") and head.kind in ("Softmax", "SoftAux", "ExpLoss", "Hinge", "Centered")
    forward = ora.forward

    def fwd(x, train, draws=None, keep=False, aux=None):
        # 16-bit operands whatever the head and whatever stack layer is below it: x is stored 16-bit, W is rounded here
        w = head.params[0]
        head.params[0] = np.asarray(O.r16(w), w.dtype)
        try:
            h, cache = forward(x, train, draws, keep, aux)
        finally:
            head.params[0] = w
        cache[hi]["c8"] = True
        return h, cache

    def bwd(cache, y):
        l, c, gs, dt = head, cache[hi], ora.grad_scale, ora.dtype
        dcent = None
        if l.kind in ("Softmax", "SoftAux"):
            dz = O.nll_dlogits(c["out"], y) if l.loss in (None, "nll") else O.softmax_head(c["z"], y, l.loss)[4]
        else:
            hd = ora.head(c["out"], y)
            dz = hd["dA"]
            if l.kind == "Centered":
                dz, dcent = dz * O.activation(l.actvn)[1](c["z"]), hd["dcenters"]
        dz = np.asarray(dz, np.float64)
        dz16 = O.r16(dz, gs)                                         # (the scale is divided out again: O.r16)
        g = [O.r16(c["in"]).T @ dz16, dz16.sum(axis=0)]
        if l.kind == "SoftAux":                                      # the aux perceptron and the cross term: fp32, on dz
            g += l.aux.backward(dz @ l.params[6].T, c["aux_saved"]) + [c["aux_out"].T @ dz, dz.sum(0)]
        elif l.kind == "Centered" and l.learn_centers:               # the row kernel's
            g.append(dcent)
        grads = [None] * len(ora.L)
        grads[hi] = [np.asarray(gg, dt) + O.wtcost_grad(p, l.reg) for gg, p in zip(g, l.params)]
        first_param = min(i for i, ll in enumerate(ora.L) if ll.params)
        g = ora._f16_down(dz16 @ O.r16(l.params[0]).T, hi, cache)
        # under the head: the stack layers' branches of OracleNet.backward
        for i in range(hi - 1, first_param - 1, -1):
            l, c = ora.L[i], cache[i]
            if l.kind == "DropOut":
                if "mask" in c:
                    g = g.reshape(c["mask"].shape) * c["mask"]
            elif l.kind == "Pool":
                g = O.pool_bwd(c["in"], g.reshape(c["out"].shape), l.p, l.ignore_border)
            else:
                assert l.kind == "Conv", l.kind
                g, dW, db = O.conv2d_bwd(c["in"], l.params[0], np.asarray(g, np.float64).reshape(c["z"].shape), l.stride,
                                         l.mode, need_dx=i > first_param, f16=True, grad_scale=gs)
                grads[i] = [dW + O.wtcost_grad(l.params[0], l.reg), db + O.wtcost_grad(l.params[1], l.reg)]
                if g is not None:
                    g = ora._f16_down(g, i, cache)
        return grads

    monkeypatch.setattr(ora, "forward", fwd)
    monkeypatch.setattr(ora, "backward", bwd)


def _oracle(monkeypatch, net, lyrs, tr):
    ora = O.OracleNet(copy.deepcopy(lyrs), dict(tr, DTYPE="float16"), dtype=np.float64)
    alone = {i for i, l in enumerate(net.tr_layers) if getattr(l, "c8_alone", False)}
    if alone:
        _teach_pool(monkeypatch, ora, alone)
    else:
        _oracle_16(monkeypatch, ora)
    _teach_head(monkeypatch, ora)
    return ora


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_c8_head_needs_the_param(dt):
    """Without STACK_HEAD, and with 'dense', the head on the stack is refused as before, now with the hint; 'any' admits no
    AuxConcatLayer."""
    from theanet_amd import NeuralNet
    lyrs, _, _ = _layers("padded", "softmax-nll")
    try:
        for extra in ({}, {"STACK_HEAD": "dense"}):
            tp = dict({k: v for k, v in TP.items() if k != "STACK_HEAD"}, **extra)
            # (a CenteredOutLayer too -- on a padded and on a dense stack tensor -- which the grammar used to let through to
            # a constructor that could not take the tensor)
            for stack, head in (("padded", "softmax-nll"), ("padded", "hinge"), ("padded", "logit"), ("dense", "rbf-learn")):
                with pytest.raises(AssertionError,
                                   match="DTYPE %s: a HiddenLayer must follow the conv stack .*STACK_HEAD: 'any'" % dt):
                    NeuralNet(_layers(stack, head)[0], _tr(tp, dt))
        with pytest.raises(AssertionError, match="a HiddenLayer must follow the conv stack .got AuxConcatLayer.$"):
            NeuralNet(copy.deepcopy(lyrs[:-1]) + [("AuxConcatLayer", dict(AUX)), HEADS["softmax-nll"]], _tr(TP, dt))
    finally:
        ctx().set_matmul_dtype("float32")


def _calls(fn, *args):
    """The entry points one call of ``fn`` issues (Context.call records while nobody else does: TN_NET_PLAN 0)."""
    c, calls = ctx(), []
    assert c.rec is None
    c.rec = calls
    try:
        out = fn(*args)
    finally:
        c.rec, c.rec_tainted = None, False
    return out, [name for name, _ in calls]


@pytest.mark.parametrize("stack,head", NETS, ids=["%s-%s" % n for n in NETS])
def test_c8_head_nets_match_16bit_oracle(dtype, stack, head, monkeypatch):
    """Two training steps (forward, every gradient, momentum update) with the oracle's draws and masks injected against the
    stored-16-bit oracle, then test mode through get_test_model; the route taken; for Softmax 'nll' the step's calls and
    that the logprob is measurably closer to the 16-bit oracle than to the fp32 one."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_NET_PLAN", "0")
    lyrs, C, img = _layers(stack, head)
    tr = _tr(TP, dtype)
    x, y, aux = _data(C, img)
    net = NeuralNet(copy.deepcopy(lyrs), dict(tr))
    kind, args = HEADS[head]
    n_head = args.get("n_out", args.get("n_features"))
    for ls in (net.tr_layers, net.te_layers):
        hl = ls[-1]
        assert type(hl).__name__ == kind and hl.c8 is not None and hl.c8_head == (n_head <= 16)
        assert hl.c8_fc in ("tn_c8_fc", "tn_c8_fcg")
        if stack != "pool3":
            assert (hl.c8_src is not None) == (stack in ("padded", "dropout"))       # the crop / embed route
        assert all(not getattr(l, "c8_head", False) for l in ls[:-1])
    softaux = kind == "SoftAuxLayer"
    nll = head == "softmax-nll"
    ora = _oracle(monkeypatch, net, lyrs, tr)
    ora32 = O.OracleNet(copy.deepcopy(lyrs), dict(tr, DTYPE="float32"), dtype=np.float64) if nll else None
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y, aux) if softaux else net.get_trin_model(x, y)
    hi = len(lyrs) - 1
    for s in range(2):
        draws = _inject_draws(net, ora, B, C, img)
        if softaux:
            draws[hi] = ora.L[hi].aux.draw(B)
            net.tr_layers[hi].aux.inject(draws[hi])
            ora.set_aux(aux[s * B:(s + 1) * B])
        cost_w, _, lp_w = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        (cost, _, lp), names = _calls(fn, s)
        fin = np.isfinite(lp_w)
        print("%s %s %s step %d: cost %.6f (oracle %.6f), max |dlogprob| %.3g" % (stack, head, dtype, s, cost, cost_w,
                                                                                  np.abs(lp - lp_w)[fin].max()))
        assert_close(np.where(fin, lp, 0), np.where(fin, lp_w, 0), rt, at, what="%s %s logprob step %d" % (stack, head, s))
        assert (lp[~fin] < -1e30).all()
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (stack, head, s))
        if nll:
            np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
            assert "tn_c8_head_softmax_nll" in names and not [n for n in names if n.startswith("tn_fc_")], names
            if s == 0:      # the mode is not a no-op: the fp32 oracle is measurably further away
                lp32 = ora32.forward(x[:B], True, draws)[0]
                assert np.abs(lp - lp_w).max() < .5 * np.abs(lp32 - lp_w).max() + 1e-6
        elif n_head <= 16:
            assert "tn_c8_head_fwd" in names and "tn_head_rows" in names, names
        else:
            assert net.tr_layers[-1].c8_fc + "_fwd" in names and "tn_head_rows" in names, names
        if kind == "SoftmaxLayer":
            assert not net.tr_layers[-1]._bwd_done          # no fused training op on the stack
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        got = lyr.get_wts()
        for j, p in enumerate(ol.params):           # (a CenteredOutLayer's get_wts also lists centers it does not learn)
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(got[j] - p).max(), np.abs(p).max()))
            assert_close(got[j], p, rt, wat, what="%s %s %s w %d %d" % (stack, head, dtype, i, j))
    tfn = net.get_test_model(x, y, aux, preds_feats=True) if softaux else net.get_test_model(x, y, preds_feats=True)
    _, _, feats, preds = tfn(1)
    if softaux:
        ora.set_aux(aux[B:2 * B])
    h_w = ora.forward(x[B:2 * B], False)[0]
    if kind in ("SoftmaxLayer", "SoftAuxLayer"):
        feats_w = lp_w = h_w
        preds_w = h_w.argmax(1)
    else:
        hd = ora.head(h_w, y[B:2 * B])
        feats_w, lp_w, preds_w = hd["feats"], hd["logprob"], hd["preds"]
    print("%s %s %s test: max |dfeatures| %.3g" % (stack, head, dtype, np.abs(feats[:B] - feats_w).max()))
    assert_close(feats[:B], feats_w, rt, at, what="%s %s test features" % (stack, head))
    # the predictions, tie-proof: where they differ the oracle's two scores are within the bound of each other
    r, got = np.arange(B), preds[:B]
    gap = np.abs(lp_w[r, got] - lp_w[r, preds_w])
    assert (gap <= at + rt * np.abs(lp_w[r, preds_w])).all(), (got, preds_w)


def test_c8_head_net_schedules_are_bit_identical(dtype, monkeypatch):
    """Two steps in flight against one at a time, replayed (tn_net_plan_*) against interpreted steps, on the padded net with
    DropOut (device RNG) and Softmax 'nll': costs, logprobs, a test-function result and the weights, bit for bit."""
    from theanet_amd import NeuralNet
    lyrs, C, img = _layers("dropout", "softmax-nll")
    x, y, _ = _data(C, img, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(lyrs), _tr(TP, dtype))
        assert net.tr_layers[-1].c8_head
        fn = net.get_trin_model(x, y)
        te = net.get_test_model(x, y)
        outs, mids = [], []
        for s in range(40):
            if s in (30, 39):
                outs.append(fn(s % 6))
            else:
                fn.enqueue(s % 6)
            if s == 34:
                mids.append((te(1), [w.copy() for l in net.tr_layers for w in l.get_wts()]))
        outs.append(fn.fetch())
        pl = getattr(fn, "_plan", None)
        replayed = pl is not None and pl.ready
        if fn.__class__.__name__ == "_PipeTrainFn" and fn._seq is not None:
            replayed = fn._seq._plan.ready
        assert replayed == (plan == "1"), (pipe, plan, getattr(pl, "why", None))
        runs.append((outs, mids, [w.copy() for l in net.tr_layers for w in l.get_wts()]))
    for outs, mids, ws in runs[1:]:
        for a, b in zip(runs[0][0], outs):
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[2], b[2])
        for (t0, w0), (t1, w1) in zip(runs[0][1], mids):
            for u, v in zip(t0, t1):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
            for u, v in zip(w0, w1):
                np.testing.assert_array_equal(u, v)
        for a, b in zip(runs[0][2], ws):
            np.testing.assert_array_equal(a, b)


_KNOB_CHILD = """
import copy, sys
import numpy as np
from tests import test_gpu_c8_head as T
from theanet_amd import NeuralNet
dtype = sys.argv[1]
lyrs, C, img = T._layers("padded", "softmax-nll")
x, y, _ = T._data(C, img)
net = NeuralNet(copy.deepcopy(lyrs), T._tr(T.TP, dtype))
head = net.tr_layers[-1]
print("ROUTE", int(head.c8_head), head.c8_fc)
(_, _, lp), names = T._calls(net.get_trin_model(x, y), 0)
print("CALLS", " ".join(names))
np.save(sys.argv[2], lp)
"""


def test_c8_head_knob_off_takes_the_dense_families(dtype, tmp_path):
    """TN_C8_HEAD=0 in a child process: the same net on the dense family's forward + tn_softmax_nll; the first-step logprob
    within the net tolerance of the default route's."""
    from theanet_amd import NeuralNet
    lyrs, C, img = _layers("padded", "softmax-nll")
    x, y, _ = _data(C, img)
    net = NeuralNet(copy.deepcopy(lyrs), _tr(TP, dtype))
    assert net.tr_layers[-1].c8_head
    lp = net.get_trin_model(x, y)(0)[2]
    out = str(tmp_path / "lp.npy")
    env = dict(os.environ, TN_C8_HEAD="0", TN_NET_PLAN="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, dtype, out], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ROUTE 0 tn_c8_fcg" in r.stdout, r.stdout
    names = r.stdout.split("CALLS", 1)[1].split()
    assert "tn_c8_fcg_fwd" in names and "tn_softmax_nll" in names and not [n for n in names if n.startswith("tn_c8_head")]
    (rt, at), _ = TOL[dtype]
    lp0 = np.load(out)
    print("max |dlogprob| TN_C8_HEAD 0 - 1: %.3g" % np.abs(lp0 - lp).max())
    assert_close(lp0, lp, rt, at, what="logprob of the dense-family route against the head kernels'")


def test_c8_head_fp32_and_bf16_nets_share_weights():
    """The same net under DTYPE float32 and bfloat16: get_wts shapes agree (the head keeps the reference's (n_in, n_out) in
    NCHW row order), and the fp32 net's weights, loaded into the bf16 net (allwts: the checkpoint route), give a first-step
    logprob within the bf16 net tolerance of the fp32 net's."""
    from theanet_amd import NeuralNet
    lyrs, C, img = _layers("padded", "softmax-nll")
    x, y, _ = _data(C, img)
    n32 = NeuralNet(copy.deepcopy(lyrs), _tr(TP, "float32"))
    assert n32.tr_layers[-1].c8 is None and not n32.tr_layers[-1].c8_head
    wts = n32.get_init_params()["allwts"]
    n16 = NeuralNet(copy.deepcopy(lyrs), _tr(dict(TP, SEED=8), "bfloat16"), allwts=wts)
    head = n16.tr_layers[-1]
    assert head.c8_head and head.get_wts()[0].shape == (24 * 9, NCLS)
    for a, b in zip(n32.tr_layers, n16.tr_layers):
        assert [w.shape for w in a.get_wts()] == [w.shape for w in b.get_wts()]
        for u, v in zip(a.get_wts(), b.get_wts()):
            np.testing.assert_array_equal(u, v)
    lp32 = n32.get_trin_model(x, y)(0)[2]
    lp16 = n16.get_trin_model(x, y)(0)[2]
    (rt, at), _ = TOL["bfloat16"]
    print("max |dlogprob| bf16 - fp32: %.3g" % np.abs(lp16 - lp32).max())
    assert_close(lp16, lp32, rt, at, what="bf16 logprob against the fp32 net's")
