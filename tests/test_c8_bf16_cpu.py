"""DTYPE 'bfloat16' without a GPU: the rounding that specifies the mode (tests/c8b_util.py rbf16) against torch's bf16
conversion, the bf16 op tests' launch list against the fp16 one (so tests/test_c8_dispatch.py's instantiation and edge
sweep covers the bf16 kernels too: the launchers map the same plan onto the same templates with the other element
type), the host's bf16 encoding, and the CPU backend's refusal of the mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import c8b_util as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# torch runs in a child process (see tests/test_oracle_kat.py: its wheel brings a HIP runtime of its own)
TORCH_SIDE = r"""
import sys
import numpy as np
import torch
x = np.load(sys.argv[1])
b = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
np.save(sys.argv[2], b)
"""


def _cases():
    rng = np.random.RandomState(7)
    ties = []
    for m in range(1, 128):                            # exact ties: 8 significant bits + one half
        ties += [1 + (m + .5) / 128, -(1 + (m + .5) / 128)]
    vals = np.concatenate([
        rng.randn(20000) * np.exp(rng.uniform(-40, 40, 20000)),      # random values of every magnitude
        np.ldexp(np.array(ties), rng.randint(-120, 120, len(ties))),
        [3.3e38, -3.39e38, 3.4e38, 1e38, 65504., 65520., 7e4, 1e5, 2.0 ** 127 * (2 - 2 ** -8)],   # large values
        [1e-38, 1.2e-38, 2.0 ** -126, 2.0 ** -130, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -135, 1e-40, 1e-44, -1e-45],  # tiny
        [0., -0., np.inf, -np.inf],
    ])
    return vals.astype(np.float32)


def test_rbf16_agrees_bit_for_bit_with_torch(tmp_path):
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        pytest.skip("could not import 'torch'")
    x = _cases()
    np.save(tmp_path / "x.npy", x)
    r = subprocess.run([sys.executable, "-c", TORCH_SIDE, str(tmp_path / "x.npy"), str(tmp_path / "b.npy")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = np.load(tmp_path / "b.npy")
    got = B.bf16_bits(B.rbf16(x.astype(np.float64)))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def test_rbf16_properties():
    x = _cases().astype(np.float64)
    r = B.rbf16(x)
    f = np.isfinite(r)
    assert np.array_equal(B.bf16_value(B.bf16_bits(r[f])), r[f].astype(np.float32))          # exactly representable
    assert B.rbf16(1 + 1.5 / 128) == 1 + 2 / 128 and B.rbf16(1 + .5 / 128) == 1          # ties to even
    assert B.rbf16(70000.) == 70144. and np.isinf(B.rbf16(3.4e38))                       # fp32's range, not fp16's
    assert B.rbf16(2.0 ** -133) == 2.0 ** -133 and B.rbf16(2.0 ** -135) == 0             # subnormals
    np.testing.assert_array_equal(B.rbf16(x, 4096.), B.rbf16(x * 4096.) / 4096.)


def test_host_bf16_encoding_matches_rbf16():
    """device.bf16_bits (C8Array.set_value) rounds as rbf16 and the kernels' v_cvt_pk_bf16_f32 (nearest even)."""
    from theanet_amd.device import bf16_bits, bf16_value
    x = _cases()
    np.testing.assert_array_equal(bf16_bits(x), B.bf16_bits(B.rbf16(x.astype(np.float64))))
    f = np.isfinite(x)
    np.testing.assert_array_equal(bf16_value(bf16_bits(x[f])), B.rbf16(x[f].astype(np.float64)).astype(np.float32))
    assert bf16_bits(np.float32(np.nan)) == 0x7FC0


def test_bf16_op_tests_reach_the_fp16_op_tests_launches():
    from tests import test_gpu_c8 as F, test_gpu_c8_bf16 as G
    for name in ("C8_CASES", "C8_FWD_CASES", "WGRAD_RING_CASES", "C8_ACT_NAMES", "C8_GENERIC_ACTS", "ACTS"):
        assert getattr(G, name) == getattr(F, name), name
    assert G.c8_launches() == F.c8_launches()


def test_bfloat16_net_fails_at_construction_on_the_cpu_backend():
    code = ("from theanet_amd import NeuralNet\n"
            "tp = {'SEED': 1, 'BATCH_SZ': 4, 'INIT_LEARNING_RATE': .1, 'EPOCHS_TO_HALF_RATE': 1, 'DTYPE': 'bfloat16'}\n"
            "try:\n"
            "    NeuralNet([('InputLayer', {'img_sz': 16, 'num_maps': 3}),\n"
            "               ('ConvLayer', {'num_maps': 16, 'filter_sz': 3, 'stride': 1, 'mode': 'same'}),\n"
            "               ('PoolLayer', {'pool_sz': 2}), ('HiddenLayer', {'n_out': 64}), ('SoftmaxLayer', {'n_out': 10})], tp)\n"
            "except Exception as e:\n"
            "    print('REFUSED', type(e).__name__, e)\n"
            "else:\n"
            "    print('BUILT')\n")
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "REFUSED" in r.stdout and "float32 only" in r.stdout, r.stdout[-2000:]
