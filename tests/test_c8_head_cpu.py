"""An output head on the 16-bit conv stack (training param STACK_HEAD; tests/test_gpu_c8_head.py) -- what needs no GPU: the
param, the stack's grammar with the new keyword, the CPU library's stubs, that the GPU test's launches reach every
instantiation and every edge tn_c8_head_plan reports, and the example file.

Edges of a launch (theanet_amd/csrc/head_c8.hip: block = 16 samples; a reduction step = 4 cells; the block's n waves, n =
ceil(steps / 4) up to 16, take contiguous runs of steps, wave w the steps [w S / n, (w + 1) S / n)):
  row_tail    B % 16 != 0: the last row tile is partial
  cell_tail   cells % 4 != 0: the last step is fed zeros past the last cell
  one_wave    a block of one wave: nothing but its own partial sum meets in LDS
  multi_step  several steps per wave; deep: more than the 4 whose loads are in flight together (the loop runs again)
  uneven      steps % waves != 0: the runs differ in length, a short run's last batch is fed zeros past its end
  C_odd       C % 8 != 0: rows of W for the last octet's missing channels are not read
  HW1         HW == 1: the row map without its division
(Fewer steps than waves cannot happen: the launcher starts no more waves than there are steps, which
test_plan_never_starts_an_idle_wave checks over the sweep.)
"""
import ast
import ctypes
import functools
import os
import subprocess
import sys

import pytest

from tests import test_gpu_c8_head as G
from tests.test_c8_pool_cpu import GRAMMAR, _below

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("SoftmaxLayer", "ExpLossLayer", "HingeLayer", "CenteredOutLayer", "SoftAuxLayer")
HINT = "training param STACK_HEAD: 'any' lets an output head close the stack"


# ---------------------------------------------------------------------------------------------------------------------
# the grammar
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", ["ConvLayer", "PoolLayer", "DropOutLayer"])
@pytest.mark.parametrize("kind", HEADS)
def test_heads_are_accepted_with_the_keyword_only(below, kind):
    from theanet_amd.layer.c8 import check_follows
    check_follows("bfloat16", _below(below, 8), kind, None, True, stack_head=True)
    for kw in ({}, {"stack_head": False}):
        with pytest.raises(AssertionError, match="a HiddenLayer must follow the conv stack") as e:
            check_follows("bfloat16", _below(below, 8), kind, None, True, **kw)
        assert str(e.value).endswith(HINT) and "DTYPE bfloat16" in str(e.value)


@pytest.mark.parametrize("below", ["ConvLayer", "PoolLayer", "DropOutLayer"])
def test_other_layers_stay_refused_with_the_keyword(below):
    from theanet_amd.layer.c8 import check_follows
    with pytest.raises(AssertionError, match="a HiddenLayer must follow the conv stack") as e:
        check_follows("float16", _below(below, 8), "AuxConcatLayer", None, True, stack_head=True)
    assert HINT not in str(e.value)             # (the param does not admit it: no hint)
    for kind in ("ElasticLayer", "ColorLayer"):
        with pytest.raises(AssertionError, match="only Conv / Pool / Mean / DropOut layers take"):
            check_follows("float16", _below(below, 8), kind, None, True, stack_head=True)


@pytest.mark.parametrize("below,kind,pool_sz,fused,refusal", GRAMMAR)
def test_the_keyword_changes_nothing_else(below, kind, pool_sz, fused, refusal):
    """tests/test_c8_pool_cpu.py's table with the keyword on: what it accepts is accepted, what it refuses is refused in the
    same words -- but for the heads, which the keyword admits."""
    from theanet_amd.layer.c8 import check_follows
    if refusal is None or kind in HEADS:
        check_follows("bfloat16", _below(*below), kind, pool_sz, fused, stack_head=True)
    else:
        with pytest.raises(AssertionError, match=refusal):
            check_follows("bfloat16", _below(*below), kind, pool_sz, fused, stack_head=True)


# ---------------------------------------------------------------------------------------------------------------------
# the param and the CPU library (child processes on THEANET_BACKEND=cpu)
# ---------------------------------------------------------------------------------------------------------------------
def _cpu(code):
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT, TN_NET_PLAN="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


PARAM = """
import numpy as np
from theanet_amd import NeuralNet
layers = [("InputLayer", {"img_sz": 12, "num_maps": 1}),
          ("ConvLayer", {"num_maps": 4, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"}),
          ("PoolLayer", {"pool_sz": 2}), ("SoftmaxLayer", {"n_out": 10})]
tp = {"SEED": 3, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}
rng = np.random.RandomState(0)
x, y = rng.rand(32, 1, 12, 12).astype(np.float32), rng.randint(0, 10, 32).astype(np.int32)
for bad in ("sparse", "ANY", True, None):
    try:
        NeuralNet(layers, dict(tp, STACK_HEAD=bad))
    except AssertionError as e:
        assert "STACK_HEAD" in str(e) and "'dense'" in str(e) and "'any'" in str(e), e
        print("ASSERTED", bad)
outs = []
for extra in ({}, {"STACK_HEAD": "dense"}, {"STACK_HEAD": "any"}):
    net = NeuralNet(layers, dict(tp, **extra))
    head = net.tr_layers[-1]
    assert net.stack_head == extra.get("STACK_HEAD", "dense") and head.c8 is None and not head.c8_head
    calls = []
    net.ctx.rec = calls
    fn = net.get_trin_model(x, y)
    res = [fn(s) for s in range(2)]
    net.ctx.rec = None
    outs.append(([type(l).__name__ for l in net.tr_layers], [n for n, _ in calls], [r[0] for r in res], [r[2] for r in res],
                 [w for l in net.tr_layers for w in l.get_wts()]))
for o in outs[1:]:
    assert o[0] == outs[0][0] and o[1] == outs[0][1] and o[2] == outs[0][2]
    assert any(n.startswith("tn_fc_softmax") for n in o[1]) and not [n for n in o[1] if n.startswith("tn_c8_")]
    for a, b in zip(outs[0][3] + outs[0][4], o[3] + o[4]):
        np.testing.assert_array_equal(a, b)
print("SAME NET")
"""


def test_stack_head_param_values_and_float32():
    """A bad value is an assertion that names the two values; under DTYPE float32 'any' builds the net that 'dense' and no
    param build: the same layers, the same calls, the same costs, logprobs and weights after two steps."""
    out = _cpu(PARAM)
    assert out.count("ASSERTED") == 4 and "SAME NET" in out, out


def test_c8_head_cpu_backend_has_only_stubs():
    code = ("import ctypes\nfrom theanet_amd.device import get_context\nc = get_context()\n"
            "assert c.lib.tn_c8_head_supported(4, 10, 1, 5) == 0\n"
            "out = (ctypes.c_int * 9)()\n"
            "assert c.lib.tn_c8_head_plan(0, 4, 10, 1, 5, out, 9) == -2 and c.lib.tn_c8_head_plan(1, 4, 10, 1, 5, out, 9) == -2\n"
            "for name, args in (('tn_c8_head_fwd', (None,) * 4 + (4, 10, 1, 5, 0, 0.)),\n"
            "                   ('tn_c8_head_softmax_nll', (None,) * 4 + (4, 10, 1, 5, None, 0) + (None,) * 6 + (.25,))):\n"
            "    try:\n        c.call(name, *args)\n    except Exception as e:\n        print('STUB', name, e)\n"
            "    else:\n        raise SystemExit(name + ' ran')\n")
    assert _cpu(code).count("STUB") == 2


def test_knob_off_answers_unsupported_without_a_device():
    """TN_C8_HEAD=0: tn_c8_head_supported (the HIP library's, no device needed) answers 0 for a shape it takes otherwise."""
    code = ("import ctypes, sys\nlib = ctypes.CDLL(sys.argv[1])\nprint('SUPPORTED', lib.tn_c8_head_supported(4, 10, 1, 5))\n")
    from theanet_amd import _lib
    for val, want in ((None, 1), ("1", 1), ("0", 0)):
        env = {k: v for k, v in os.environ.items() if k != "TN_C8_HEAD"}
        if val is not None:
            env["TN_C8_HEAD"] = val
        r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "SUPPORTED %d" % want in r.stdout, (val, r.stdout, r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# dispatch coverage
# ---------------------------------------------------------------------------------------------------------------------
EDGES = ("row_tail", "cell_tail", "one_wave", "multi_step", "deep", "uneven", "C_odd", "HW1")


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    out = (ctypes.c_int * 9)()

    def plan(op, B, C, HW, n_out):
        n = lib.tn_c8_head_plan(op, B, C, HW, n_out, out, 9)
        return tuple(out[:n]) if n > 0 else None
    assert plan(0, 4, 10, 1, 5), "tn_c8_head_plan answers nothing (CPU backend loaded, or TN_C8_HEAD=0?)"
    return plan


def classify(op, B, C, HW, n_out):
    """(instantiation, set of edges) of one tn_c8_head_fwd / tn_c8_head_softmax_nll call, or None if it refuses the shape."""
    p = _query()(op, B, C, HW, n_out)
    if p is None:
        return None
    inst, tiles, steps, waves, per_wave, row_pad, cell_pad, c_pad, hw1 = p
    assert tiles == (B + 15) // 16 and steps == ((C + 7) // 8 * HW + 3) // 4
    assert waves == min(16, (steps + 3) // 4) and per_wave == (steps + waves - 1) // waves
    edges = {"row_tail": row_pad != 0, "cell_tail": cell_pad != 0, "one_wave": waves == 1, "multi_step": per_wave > 1,
             "deep": per_wave > 4, "uneven": steps % waves != 0, "C_odd": c_pad != 0, "HW1": hw1 != 0}
    return ("head", inst), {e for e, on in edges.items() if on}


def _reach(calls):
    insts, pairs = set(), set()
    for c in calls:
        r = classify(*c)
        if r is not None:
            insts.add(r[0])
            pairs.update((r[0], e) for e in r[1])
    return insts, pairs


def _sweep():
    return _reach((op, B, C, HW, n) for op in (0, 1) for B in (1, 15, 16, 17, 300) for C in (1, 3, 8, 10, 16, 24, 128)
                  for HW in (1, 2, 9, 16, 25, 49, 64) for n in (1, 5, 10, 16))


def test_plan_query_reports_the_launch():
    plan = _query()
    assert plan(0, 3, 1, 1, 1) == (0, 1, 1, 1, 1, 13, 3, 7, 1)
    assert plan(1, 37, 32, 49, 10) == (1, 3, 49, 13, 4, 11, 0, 0, 0)
    assert plan(1, 16, 64, 64, 10) == (1, 1, 128, 16, 8, 0, 0, 0, 0)
    for bad in ((0, 16, 64, 64, 17), (0, 16, 64, 64, 0), (2, 16, 64, 64, 10), (0, 0, 64, 64, 10), (1, 1 << 23, 8, 1, 8)):
        assert plan(*bad) is None, bad


def test_plan_never_starts_an_idle_wave():
    plan = _query()
    for C in range(1, 200, 3):
        for HW in (1, 2, 3, 9, 16, 25, 49, 64, 100):
            _, _, steps, waves, per_wave = plan(0, 16, C, HW, 10)[:5]
            assert 1 <= waves <= min(16, steps) and (waves - 1) * steps // waves < steps and per_wave * waves >= steps


def test_gpu_cases_reach_every_instantiation_and_edge():
    """The launches of tests/test_gpu_c8_head.py reach both instantiations, and every edge of each that the sweep reaches
    (all of them: no (instantiation, edge) pair is unreachable)."""
    insts, pairs = _sweep()
    assert insts == {("head", 0), ("head", 1)} and pairs == {(i, e) for i in insts for e in EDGES}
    got_i, got_p = _reach(G.c8_head_launches())
    assert got_i == insts, (got_i, insts)
    assert not pairs - got_p, "(instantiation, edge) pairs no GPU case reaches: %s" % sorted(pairs - got_p)
    # and the cases the issue lists are among them
    for c in ((3, 1, 1, 1), (4, 10, 1, 5), (7, 3, 25, 10), (20, 20, 36, 3), (37, 32, 49, 10), (130, 24, 9, 16),
              (16, 64, 64, 10), (300, 128, 16, 13)) + tuple((21, 16, 9, n) for n in range(1, 17)):
        assert (0,) + c in G.c8_head_launches() and (1,) + c in G.c8_head_launches()


# ---------------------------------------------------------------------------------------------------------------------
# the example file
# ---------------------------------------------------------------------------------------------------------------------
def test_cifar_head_prms_is_cifar_gap_without_the_mean():
    def load(name):
        with open(os.path.join(ROOT, "params", name)) as fh:
            return fh.read()
    src = load("cifar_head.prms")
    head, gap = ast.literal_eval(src), ast.literal_eval(load("cifar_gap.prms"))
    assert head["layers"] == [l for l in gap["layers"] if l[0] != "MeanLayer"] and head["layers"][-2][0] == "PoolLayer"
    assert head["training_params"] == gap["training_params"]
    comment = " ".join(l.lstrip("# ") for l in src.splitlines() if l.startswith("#"))
    assert "STACK_HEAD: 'any'" in comment and "DTYPE" in comment
