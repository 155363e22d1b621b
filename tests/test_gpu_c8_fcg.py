"""A HiddenLayer of any size on the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16'): the general dense products
tn_c8_fcg_fwd / _fwd_dropout / _dgrad / _wgrad through the C-ABI against numpy's stored-16-bit statement (the references
of tests/test_gpu_c8.py::test_c8_fc_ops: _rowmap, Wp, dz16, with the rounding of the element type), the refusals, the CPU
library's stubs, and nets whose dense layer the tiled family tn_c8_fc_* refuses against the unchanged stored-16-bit oracle.

Tolerances are the project's own for this arithmetic (operands rounded to the 16-bit type, exact products, fp32
accumulation): fp32 results (a, gW, gb) 2e-5 of the largest entry, the stored 16-bit dx 1e-3 for fp16 and 1e-2 for bf16
(TOL16 of tests/test_gpu_c8_conv1.py), nets TOL of tests/test_gpu_c8_mean.py, dropout bits, masked outputs, repeated calls
and schedules bit for bit."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8_util as U
from tests import c8b_util as CB
from tests.gpu_util import ROOT, act_code, assert_close, call, ctx, dev, empty, load_prms
from tests.test_gpu_c8 import _rowmap
from tests.test_gpu_c8_conv1 import TOL16, _act, _act_grad_from_out, _code, _R, _rel
from tests.test_gpu_c8_dropout import _oracle_16
from tests.test_gpu_c8_mean import GS, R16, TOL
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


def _bits(v, dtype):
    """Values that are exact in the element type -> their 16-bit patterns."""
    return CB.bf16_bits(v) if dtype == "bfloat16" else np.asarray(v).astype(np.float16).view(np.uint16)


def _vals(bits, dtype):
    return (CB.bf16_value(bits) if dtype == "bfloat16" else bits.view(np.float16)).astype(np.float64)


# (B, C, HW, n_out); the last two are shapes the tiled family takes as well
CASES = [(20, 20, 36, 500), (37, 32, 49, 500), (4, 10, 1, 32), (3, 1, 1, 1), (130, 24, 9, 1000), (7, 3, 25, 10),
         (300, 128, 16, 457), (2048, 32, 49, 500), (5, 16, 4, 32), (300, 128, 16, 512)]
BOTH = CASES[-2:]


def _ops(case, name, dtype):
    B, C, HW, N = case
    R, tol, gs = _R(dtype), TOL16[dtype], GS[dtype]
    act, prm = _code(name)
    lib = ctx().lib
    assert lib.tn_c8_fcg_supported(B, C, HW, N)
    tiled = bool(lib.tn_c8_fc_supported(B, C, HW, N))
    assert tiled == (case in BOTH)
    rng = np.random.RandomState(1)
    rm = _rowmap(C, HW)
    Kc, n_in, ok = len(rm), C * HW, rm >= 0
    x = np.zeros((B, Kc)); x[:, ok] = R(rng.randn(B, n_in))[:, rm[ok]]
    W = (rng.randn(n_in, N) / np.sqrt(n_in)).astype(np.float32)
    b = (rng.randn(N) * .1).astype(np.float32)
    mask = (rng.rand(B, N) < .5).astype(np.uint8)
    Wp = np.zeros((Kc, N)); Wp[ok] = R(W)[rm[ok]]
    z = _act(name, x @ Wp + b)
    xd, Wd, bd = dev(_bits(x, dtype)), dev(W), dev(b)
    # forward: mask given, mask NULL
    a = dev(np.full((B, N), 7., np.float32))
    call("tn_c8_fcg_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, C, HW, N, act, prm, dev(mask).ptr)
    e = _rel(a.get_value(), z * mask)
    print("fwd masked: %.3g" % e)
    assert e < 2e-5
    a0 = dev(np.full((B, N), 7., np.float32))
    call("tn_c8_fcg_fwd", xd.ptr, Wd.ptr, bd.ptr, a0.ptr, B, C, HW, N, act, prm, None)
    e = _rel(a0.get_value(), z)
    print("fwd: %.3g" % e)
    assert e < 2e-5
    if tiled:
        at = empty((B, N))
        call("tn_c8_fc_fwd", xd.ptr, Wd.ptr, bd.ptr, at.ptr, B, C, HW, N, act, prm, None)
        e = _rel(a0.get_value(), at.get_value().astype(np.float64))
        print("fwd against the tiled family: %.3g" % e)
        assert e < 2e-5
    # the mask drawn in the launch: the bits of tn_dropout_mask, the masked output of tn_c8_fcg_fwd with them
    want, got_mask, a2 = empty((B * N,), np.uint8), empty((B * N,), np.uint8), empty((B, N))
    for elem0 in (1000, 1003):
        call("tn_dropout_mask", want.ptr, B * N, .3, 99, 5, None, elem0)
        call("tn_c8_fcg_fwd_dropout", xd.ptr, Wd.ptr, bd.ptr, a2.ptr, B, C, HW, N, act, prm, got_mask.ptr, .3, 99, 5, None,
             elem0)
        np.testing.assert_array_equal(got_mask.get_value(), want.get_value())
        call("tn_c8_fcg_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, C, HW, N, act, prm, want.ptr)
        np.testing.assert_array_equal(a2.get_value().view(np.uint32), a.get_value().view(np.uint32))
    # input gradient over garbage: y16 given (exact zeros planted: the tie derivative) and NULL; channels past C exactly 0
    dz = (rng.randn(B, N) * 1e-3).astype(np.float32)
    dz16 = R(gs * dz.astype(np.float64))
    if name == "leaky":
        y = R(rng.randn(B, Kc))
        y[0, :3] = 0
    else:
        y = R(_act(name, 2 * rng.randn(B, Kc)))
    y[:, ~ok] = 0
    lin = dz16 @ Wp.T
    dzd, yd = dev(dz), dev(_bits(y, dtype))
    for yp, wantx in ((yd.ptr, lin * _act_grad_from_out(name, y)), (None, lin)):
        dxo = dev(np.full((B, Kc), 0x5555, np.uint16))
        call("tn_c8_fcg_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, B, C, HW, N, yp, act, prm)
        raw = dxo.get_value()
        assert not raw[:, ~ok].any(), "channels past the last one must be written as 0"
        e = _rel(_vals(raw, dtype)[:, ok], R(wantx)[:, ok])
        print("dgrad (y16 %s): %.3g" % ("given" if yp else "NULL", e))
        assert e < tol
    # weight / bias gradient (fp32, the scale removed) over garbage: OVERWRITE; twice: the same bits
    dWw = np.zeros((n_in, N)); dWw[rm[ok]] = (x.T @ dz16)[ok] / gs
    gW, gb = dev(np.full((n_in, N), 7., np.float32)), dev(np.full((N,), 7., np.float32))
    call("tn_c8_fcg_wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, B, C, HW, N)
    eW, eb = _rel(gW.get_value(), dWw), _rel(gb.get_value(), dz16.sum(0) / gs)
    print("wgrad: dW %.3g db %.3g" % (eW, eb))
    assert eW < 2e-5 and eb < 2e-5
    g2, b2 = dev(np.full((n_in, N), -3., np.float32)), dev(np.full((N,), -3., np.float32))
    call("tn_c8_fcg_wgrad", xd.ptr, dzd.ptr, g2.ptr, b2.ptr, B, C, HW, N)
    np.testing.assert_array_equal(gW.get_value().view(np.uint32), g2.get_value().view(np.uint32))
    np.testing.assert_array_equal(gb.get_value().view(np.uint32), b2.get_value().view(np.uint32))
    if tiled:
        gt, bt = empty((n_in, N)), empty((N,))
        call("tn_c8_fc_wgrad", xd.ptr, dzd.ptr, gt.ptr, bt.ptr, B, C, HW, N)
        eW = _rel(gW.get_value(), gt.get_value().astype(np.float64))
        eb = _rel(gb.get_value(), bt.get_value().astype(np.float64))
        print("wgrad against the tiled family: dW %.3g db %.3g" % (eW, eb))
        assert eW < 2e-5 and eb < 2e-5


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_c8_fcg_ops_match_numpy(dtype, case):
    """Forward (mask given / NULL / drawn at elem0 1000 and 1003), input gradient (y16 given / NULL, over garbage, channels
    past C zero), weight gradient (over garbage, twice) with the leaky-ReLU epilogue; the shapes the tiled family takes
    as well also against tn_c8_fc_*."""
    _ops(case, "leaky", dtype)


@pytest.mark.parametrize("name,case", [("tanh", CASES[0]), ("sigmoid", CASES[5])], ids=["tanh", "sigmoid"])
def test_c8_fcg_ops_generic_activation(dtype, name, case):
    _ops(case, name, dtype)


def test_c8_fcg_ops_refuse_bad_arguments(dtype):
    from theanet_amd import _lib
    lib = ctx().lib
    B, C, HW, N = 4, 10, 1, 32
    Kc = 16
    x = dev(np.zeros((B, Kc), np.uint16))
    W, b = dev(np.zeros((C * HW, N), np.float32)), dev(np.zeros((N,), np.float32))
    dz = dev(np.zeros((B, N), np.float32))
    a = dev(np.full((B, N), 7., np.float32))
    dx = dev(np.full((B, Kc), 0x5555, np.uint16))
    gW, gb = dev(np.full((C * HW, N), 7., np.float32)), dev(np.full((N,), 7., np.float32))
    mk = dev(np.full((B * N,), 0x55, np.uint8))
    huge = ((1 << 20, 8, 1 << 12, 8), (1 << 23, 8, 1, 8), (4, 8, 1, 1 << 23), (1 << 16, 8, 1, 1 << 16), (4, 1 << 20, 1 << 10, 8),
            (4, 8, 1 << 17, 1 << 14))
    bad = ((0, C, HW, N), (B, 0, HW, N), (B, C, 0, N), (B, C, HW, 0), (-1, C, HW, N)) + huge
    for s in bad:
        assert not lib.tn_c8_fcg_supported(*s), s
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_fwd"):
            call("tn_c8_fcg_fwd", x.ptr, W.ptr, b.ptr, a.ptr, *s, 0, 0., None)
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_fwd_dropout"):
            call("tn_c8_fcg_fwd_dropout", x.ptr, W.ptr, b.ptr, a.ptr, *s, 0, 0., mk.ptr, .3, 99, 5, None, 0)
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_dgrad"):
            call("tn_c8_fcg_dgrad", dz.ptr, W.ptr, dx.ptr, *s, None, 0, 0.)
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_wgrad"):
            call("tn_c8_fcg_wgrad", x.ptr, dz.ptr, gW.ptr, gb.ptr, *s)
    g = (B, C, HW, N)
    assert lib.tn_c8_fcg_supported(*g)
    for args in ((None, W.ptr, b.ptr, a.ptr), (x.ptr, None, b.ptr, a.ptr), (x.ptr, W.ptr, None, a.ptr), (x.ptr, W.ptr, b.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_fwd"):
            call("tn_c8_fcg_fwd", *args, *g, 0, 0., None)
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_fwd_dropout"):
            call("tn_c8_fcg_fwd_dropout", *args, *g, 0, 0., mk.ptr, .3, 99, 5, None, 0)
    with pytest.raises(_lib.BackendError, match="tn_c8_fcg_fwd_dropout"):
        call("tn_c8_fcg_fwd_dropout", x.ptr, W.ptr, b.ptr, a.ptr, *g, 0, 0., None, .3, 99, 5, None, 0)
    for args in ((None, W.ptr, dx.ptr), (dz.ptr, None, dx.ptr), (dz.ptr, W.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_dgrad"):
            call("tn_c8_fcg_dgrad", *args, *g, None, 0, 0.)
    for args in ((None, dz.ptr, gW.ptr, gb.ptr), (x.ptr, None, gW.ptr, gb.ptr), (x.ptr, dz.ptr, None, gb.ptr),
                 (x.ptr, dz.ptr, gW.ptr, None)):
        with pytest.raises(_lib.BackendError, match="tn_c8_fcg_wgrad"):
            call("tn_c8_fcg_wgrad", *args, *g)
    ctx().sync()
    assert (a.get_value() == 7.).all() and (dx.get_value() == 0x5555).all()            # nothing was launched
    assert (gW.get_value() == 7.).all() and (gb.get_value() == 7.).all() and (mk.get_value() == 0x55).all()


def test_c8_fcg_cpu_backend_has_only_stubs():
    code = ("from theanet_amd.device import get_context\nc = get_context()\n"
            "assert c.lib.tn_c8_fcg_supported(4, 10, 1, 32) == 0\n"
            "for name, args in (('tn_c8_fcg_fwd', (None,) * 4 + (4, 10, 1, 32, 0, 0., None)),\n"
            "                   ('tn_c8_fcg_fwd_dropout', (None,) * 4 + (4, 10, 1, 32, 0, 0., None, .3, 99, 5, None, 0)),\n"
            "                   ('tn_c8_fcg_dgrad', (None,) * 3 + (4, 10, 1, 32, None, 0, 0.)),\n"
            "                   ('tn_c8_fcg_wgrad', (None,) * 4 + (4, 10, 1, 32))):\n"
            "    try:\n        c.call(name, *args)\n    except Exception as e:\n        print('STUB', name, e)\n"
            "    else:\n        raise SystemExit(name + ' ran')\n")
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("STUB") == 4, (r.stdout[-2000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
TP = {"SEED": 7, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


def _conv(k, f, mode="same"):
    return ("ConvLayer", {"num_maps": k, "filter_sz": f, "stride": 1, "mode": mode, "actvn": "relu10"})


POOL = ("PoolLayer", {"pool_sz": 2})


def _small(drop=True):
    """3x12x12 -> conv3(16) + pool -> conv1(24) + pool -> DropOut -> Hidden 100 -> Softmax: a 9-pixel map at pitch 4 (the
    dense layer reads the cropped copy and embeds its input gradient), 216 c8 inputs, 100 outputs."""
    return [("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(16, 3), POOL, _conv(24, 1, "valid"), POOL] + \
        ([("DropOutLayer", {"pdrop": .25})] if drop else []) + [("HiddenLayer", {"n_out": 100}), ("SoftmaxLayer", {"n_out": 10})]


def _net_prms(name, B):
    if name == "mnist_c8.prms":
        prms = load_prms(name, 28, batch=B)
        return prms["layers"], prms["training_params"], 1, 28
    return _small(), dict(TP, BATCH_SZ=B), 3, 12


def _tr(tp, dtype):
    return dict(tp, DTYPE=dtype, GRAD_SCALE=GS[dtype]) if dtype in GS else dict(tp, DTYPE=dtype)


def _data(B, C, img, n=2, seed=1):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, C, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


def _hidden(layers):
    return [l for l in layers if type(l).__name__ == "HiddenLayer"]


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_c8_fcg_nets_build_16bit_resident(dt):
    """Fails on a build without the general family: construction asserts (1568 / 216 c8 inputs, 500 / 100 outputs)."""
    from theanet_amd import NeuralNet
    for name in ("mnist_c8.prms", "small"):
        layers, tp, _, _ = _net_prms(name, 16)
        net = NeuralNet(copy.deepcopy(layers), _tr(tp, dt))
        convs = [l for l in net.tr_layers if type(l).__name__ == "ConvLayer"]
        assert convs and all(l.f16 for l in convs)
        for ls in (net.tr_layers, net.te_layers):
            hid = _hidden(ls)
            assert len(hid) == 1 and hid[0].c8 is not None and hid[0].c8_fc == "tn_c8_fcg", name
            assert hid[0].c8_src is not None                   # (a padded stack tensor: the crop / embed route)
    # shapes the tiled family takes stay on it
    prms = load_prms("mnist_c16.prms", 28, batch=16)
    net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms["training_params"], dt))
    for ls in (net.tr_layers, net.te_layers):
        assert [h.c8_fc for h in _hidden(ls)] == ["tn_c8_fc"]


NETS = [("mnist_c8.prms", 16), ("small", 16)]


@pytest.mark.parametrize("name,B", NETS)
def test_c8_fcg_nets_match_16bit_oracle(dtype, name, B, monkeypatch):
    """Two training steps (forward, every gradient, momentum update, maxnorm) with the oracle's draws and dropout masks
    injected against the stored-16-bit oracle -- and measurably closer to it than to the fp32 oracle; then test mode
    through get_test_model."""
    from theanet_amd import NeuralNet
    layers, tp, C, img = _net_prms(name, B)
    tr = _tr(tp, dtype)
    x, y = _data(B, C, img)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    assert [h.c8_fc for h in _hidden(net.tr_layers)] == ["tn_c8_fcg"]
    ora = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float16"), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float32"), dtype=np.float64)
    _oracle_16(monkeypatch, ora)
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y)
    for s in range(2):
        draws = _inject_draws(net, ora, B, C, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        print("%s %s step %d: cost %.6f (oracle %.6f), max |dlogprob| %.3g" % (name, dtype, s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dtype, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dtype, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:      # the mode is not a no-op: the fp32 oracle is measurably further away
            lp32 = ora32.forward(x[:B], True, draws)[0]
            assert np.abs(lp - lp_w).max() < .5 * np.abs(lp32 - lp_w).max() + 1e-6
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
            assert_close(w, ol.params[j], rt, wat, what="%s %s w %d %d" % (name, dtype, i, j))
    tfn = net.get_test_model(x, y, preds_feats=True)
    _, _, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:2 * B], y[B:2 * B])
    assert_close(feats[:B], lp_w, rt, at, what="%s %s test logprob" % (name, dtype))
    np.testing.assert_array_equal(preds[:B], preds_w)


def test_c8_fcg_net_schedules_are_bit_identical(dtype, monkeypatch):
    """Two steps in flight against one at a time, replayed (tn_net_plan_*) against interpreted steps, on params/mnist_c8.prms
    at 28 (device draws and dropout): costs, logprobs, a test-function result and the weights, bit for bit."""
    from theanet_amd import NeuralNet
    B = 16
    prms = load_prms("mnist_c8.prms", 28, batch=B)
    x, y = _data(B, 1, 28, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms["training_params"], dtype))
        assert [h.c8_fc for h in _hidden(net.tr_layers)] == ["tn_c8_fcg"]
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


def test_c8_fcg_fp32_and_bf16_nets_share_weights():
    """The same net under DTYPE float32 and bfloat16: get_wts shapes agree (the dense layer keeps the reference's (n_in, n_out)
    in NCHW row order), and the fp32 net's weights, loaded into the bf16 net (allwts: the checkpoint route), give a
    first-step logprob within the bf16 net tolerance of the fp32 net's."""
    from theanet_amd import NeuralNet
    B = 16
    layers = _small(drop=False)
    x, y = _data(B, 3, 12)
    n32 = NeuralNet(copy.deepcopy(layers), _tr(TP, "float32"))
    other = NeuralNet(copy.deepcopy(layers), _tr(dict(TP, SEED=8), "bfloat16"))
    for a, b in zip(n32.tr_layers, other.tr_layers):
        assert [w.shape for w in a.get_wts()] == [w.shape for w in b.get_wts()]
    wts = n32.get_init_params()["allwts"]
    n16 = NeuralNet(copy.deepcopy(layers), _tr(dict(TP, SEED=8), "bfloat16"), allwts=wts)
    hid = _hidden(n16.tr_layers)[0]
    assert hid.c8_fc == "tn_c8_fcg" and hid.get_wts()[0].shape == (24 * 9, 100)
    for a, b in zip(n32.tr_layers, n16.tr_layers):
        for u, v in zip(a.get_wts(), b.get_wts()):
            np.testing.assert_array_equal(u, v)
    lp32 = n32.get_trin_model(x, y)(0)[2]
    lp16 = n16.get_trin_model(x, y)(0)[2]
    (rt, at), _ = TOL["bfloat16"]
    print("max |dlogprob| bf16 - fp32: %.3g" % np.abs(lp16 - lp32).max())
    assert_close(lp16, lp32, rt, at, what="bf16 logprob against the fp32 net's")
