"""Shuffled epochs (set_order / tn_gather_batch / train.py's SHUFFLE) without a GPU, on the C++ backend behind the same
C-ABI (THEANET_BACKEND=cpu): the two GPU test files of the feature run against it, two data-parallel ranks with an order
equal one, ranks with different orders refuse at set_order, and train.py shuffles reproducibly."""
import ast
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")
pytestmark = pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")


def _env(**kw):
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    env.update(kw)
    return env


def test_gather_and_shuffle_suites_run_against_the_cpu_backend():
    """(the 16-bit conv stack is MI355X-only)"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_gather_batch.py", "tests/test_gpu_shuffle.py", "-k", "not 16bit"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 47, tail          # 35 of the op + 12 of the training functions


def _ranks(tmp_path, world, port, out, disagree=0, **env):
    worker = os.path.join(ROOT, "tests", "dp_shuffle_worker.py")
    procs = []
    for rank in range(world):
        e = _env(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(port), TN_DP_CHECK_ORDER="1", OMP_NUM_THREADS="2", **env)
        procs.append(subprocess.Popen([sys.executable, worker, out, "32", "14", "5", str(disagree)], env=e,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    res = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        res.append((p.returncode, o.decode()))
    return res


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_two_ranks_with_an_order_equal_one(tmp_path, pipe):
    """Each rank gathers its shard [i*B + shard_lo, + local_bsz) of the order's slice: the same global minibatches as the
    one-rank run (tolerances of test_product_data_parallel_step_world_size_2: summation order)."""
    port = _free_port()
    outs = []
    for world in (1, 2):
        out = str(tmp_path / ("w%d.npz" % world))
        for rc, o in _ranks(tmp_path, world, port + world, out, TN_PIPELINE=pipe):
            assert rc == 0, o[-3000:]
        outs.append(np.load(out))
    one, two = outs
    assert bool(two["pipelined"]) == (pipe == "1")
    np.testing.assert_allclose(two["costs"], one["costs"], rtol=2e-5)
    for k in one.files:
        if k.startswith("w"):
            np.testing.assert_allclose(two[k], one[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_ranks_with_different_orders_refuse_at_set_order(tmp_path):
    out = str(tmp_path / "d.npz")
    for rc, o in _ranks(tmp_path, 2, _free_port(), out, disagree=1):
        assert rc != 0 and "disagree on the row order of set_order" in o, o[-3000:]
    assert not os.path.isfile(out)


def _train_py(tmp_path, name, **more):
    with open(os.path.join(ROOT, "params", "mnist.prms")) as fh:
        prms = ast.literal_eval(fh.read())
    prms["training_params"].update(SEED=11, BATCH_SZ=20, NUM_EPOCHS=2, TEST_SAMP_SZ=200, **more)
    d = tmp_path / name
    d.mkdir()
    prm = d / "mnist.prms"
    prm.write_text(repr(prms))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "synthetic", str(prm)], cwd=str(d),
                       env=_env(THEANET_SYNTH_TRAIN="400", THEANET_SYNTH_TEST="200", THEANET_NO_PICKLE="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Epoch   Cost  Tr_Error Tr_P(MLE)    Te_Error Te_P(MLE)" in r.stdout
    rows = [l for l in r.stdout.splitlines() if l.strip().startswith(("0 ", "1 ", "2 "))]
    assert len(rows) == 3, r.stdout
    return [l.split()[1] for l in rows[:2]]             # the epochs' total costs as printed


def test_train_py_shuffles_reproducibly(tmp_path):
    a = _train_py(tmp_path, "a", SHUFFLE=True)
    b = _train_py(tmp_path, "b", SHUFFLE=True)
    plain = _train_py(tmp_path, "c")
    assert a == b
    assert a != plain, (a, plain)
    other = _train_py(tmp_path, "d", SHUFFLE=True, SHUFFLE_SEED=12)
    assert other != a, (a, other)
