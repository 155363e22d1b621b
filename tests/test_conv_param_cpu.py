"""The CONV training param on the CPU backend (THEANET_BACKEND=cpu, in a child process): 'bfloat16' is a mode of the
HIP library only -- construction fails with an error that names the param and the mode, before any step runs --
'float32' on the same net still trains there, and an unknown value is an assertion that names the param."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")
pytestmark = pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")

CODE = """
import numpy as np
from theanet_amd import NeuralNet
layers = [("InputLayer", {"img_sz": 12, "num_maps": 1}),
          ("ConvLayer", {"num_maps": 4, "filter_sz": 3, "stride": 1, "mode": "valid", "actvn": "relu10"}),
          ("PoolLayer", {"pool_sz": 2}), ("HiddenLayer", {"n_out": 24, "actvn": "tanh"}), ("SoftmaxLayer", {"n_out": 10})]
tp = {"SEED": 3, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2, "CONV": %r}
rng = np.random.RandomState(0)
x, y = rng.rand(32, 1, 12, 12).astype(np.float32), rng.randint(0, 10, 32).astype(np.int32)
steps = 0
try:
    net = NeuralNet(layers, tp)
    fn = net.get_trin_model(x, y)
    for s in range(2):
        cost = fn(s)[0]
        assert np.isfinite(cost)
        steps += 1
except AssertionError as e:
    print("ASSERTED steps=%%d: %%s" %% (steps, e))
except Exception as e:
    print("REFUSED steps=%%d: %%s" %% (steps, e))
else:
    print("TRAINED steps=%%d cost=%%.4f" %% (steps, cost))
"""


def _run(mode):
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CODE % mode], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_conv_bfloat16_is_refused_on_the_cpu_backend_by_name():
    out = _run("bfloat16")
    assert "REFUSED steps=0" in out and "bfloat16" in out and "CONV" in out, out


def test_conv_float32_still_trains_on_the_cpu_backend():
    out = _run("float32")
    assert "TRAINED steps=2" in out, out


def test_conv_unknown_value_is_an_assertion_that_names_the_param():
    out = _run("float16")
    assert "ASSERTED steps=0" in out and "CONV" in out, out
