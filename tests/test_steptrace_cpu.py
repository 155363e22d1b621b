"""tools/steptrace.py on the CPU backend: the C-ABI call trace of a net is reproducible -- two runs of one drive mode are
byte-identical -- and the three ways of driving a training function (enqueue / fn(i) / step_cost) are three different
traces, so a host-side refactor can be checked on the cost paths too."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")
pytestmark = pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")

_SCRIPT = r"""
import ast, copy, json, os, sys
sys.path.insert(0, os.path.join(%(root)r, "tools"))
import steptrace
with open(os.path.join(%(root)r, "params", "mlp3.prms")) as fh:
    prms = ast.literal_eval(fh.read())
prms["layers"][0][1]["img_sz"] = 28
# (the CPU backend computes the dense products in float32 only)
tp = dict(prms["training_params"], SEED=555555, BATCH_SZ=8, MATMUL="float32")
# a process's first net finds the context unowned, every later one takes it over from a collected net (one more call):
# a throw-away net first, so that all six traces start alike
steptrace.trace(copy.deepcopy(prms["layers"]), tp, 1, 28, steps=1)
out = {d: [steptrace.trace(copy.deepcopy(prms["layers"]), tp, 1, 28, steps=24, drive=d) for _ in range(2)]
       for d in steptrace.DRIVES}
print("TRACES " + json.dumps(out))
"""


def test_steptrace_drive_modes_are_reproducible_and_distinct():
    env = dict(os.environ, THEANET_BACKEND="cpu")
    for k in ("TN_DP_FORCE", "TN_DP_OVERLAP", "TN_PIPELINE", "TN_DP_BUCKETS", "RANK", "WORLD_SIZE"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-c", _SCRIPT % {"root": ROOT}], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("TRACES ")][-1]
    traces = json.loads(line[len("TRACES "):])
    assert sorted(traces) == ["call", "enqueue", "step_cost"]
    for drive, (a, b) in traces.items():
        assert len(a) > 24 and a[-1].startswith("weights sha256 ")
        assert a == b, "two %s runs differ" % drive
    firsts = [tuple(t[0]) for t in traces.values()]
    assert len(set(firsts)) == 3, "drive modes with the same trace"
    # every mode trains the same net on the same minibatches: the weights agree (the schedules are re-orderings)
    assert len({t[0][-1] for t in traces.values()}) == 1
    # step_cost: all 24 costs come back, numbered from 0 after every drain (steps 10, 20 and the end)
    ks = [int(l.split()[1]) for l in traces["step_cost"][0] if l.startswith("cost ")]
    assert ks == list(range(10)) + list(range(10)) + list(range(4))
    # fn(i): one cost per step, in order; enqueue reads none
    assert [int(l.split()[1]) for l in traces["call"][0] if l.startswith("cost ")] == list(range(24))
    assert not [l for l in traces["enqueue"][0] if l.startswith("cost ")]
