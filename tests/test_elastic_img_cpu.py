"""ElasticLayer per_image on the CPU backend (THEANET_BACKEND=cpu; runs without a GPU):

  * the cases of tests/test_gpu_elastic_img.py -- per-op checks against the oracle and whole nets on every schedule --
    against libtheanet_cpu.so's tn_elastic_apply_img (same Philox keying, same operation order as the HIP kernel), minus
    the 16-bit stack, which the CPU backend does not have;
  * the product's data-parallel step with two ranks: rank r distorts its rows exactly like the one-rank run distorts
    rows [shard_lo, shard_hi) of the global minibatch;
  * nets WITHOUT the key are untouched: train.py on params/mnist.prms prints what it printed before the mode existed."""
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


def test_per_image_cases_run_against_the_cpu_backend():
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider",
                        "tests/test_gpu_elastic_img.py", "-k", "not (c8 or bf16 or f16)"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 47, tail


def test_two_ranks_distort_their_rows_like_one_rank(tmp_path):
    worker = os.path.join(ROOT, "tests", "elastic_img_dp_worker.py")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    runs = {}
    for world in (1, 2):
        stem = str(tmp_path / ("w%d" % world))
        procs = []
        for rank in range(world):
            env = _env(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port + world), TN_PIPELINE="0", OMP_NUM_THREADS="2")
            procs.append(subprocess.Popen([sys.executable, worker, stem], env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT))
        for p in procs:
            try:
                o, _ = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, o.decode()[-3000:]
        runs[world] = [np.load("%s_r%d.npz" % (stem, rank)) for rank in range(world)]
    one = runs[1][0]
    assert int(one["rows"]) == 8 and one["outs"].shape == (2, 8, 1, 12, 12)
    covered = 0
    for r in runs[2]:
        lo, rows = int(r["lo"]), int(r["rows"])
        assert int(r["world"]) == 2 and rows == 4 and r["outs"].shape == (2, 4, 1, 12, 12)
        np.testing.assert_array_equal(r["outs"], one["outs"][:, lo:lo + rows])
        np.testing.assert_allclose(r["costs"], one["costs"], rtol=2e-5)
        covered += rows
    assert covered == 8 and sorted(int(r["lo"]) for r in runs[2]) == [0, 4]
    for n in range(1, 8):           # (and the rows ARE distorted image by image: no two by the same field)
        assert not np.array_equal(one["outs"][0, n], one["outs"][0, 0])


def _report(text):
    """train.py's stdout without the lines that name the run: the command line (it carries the checkout's path), the
    time, the host and the device."""
    lines = text.splitlines()[1:]
    return "\n".join(l for l in lines if not l.startswith(("Time", "Host", "Device"))) + "\n"


def test_train_py_on_mnist_prms_prints_what_it_printed_before(tmp_path):
    """`train.py synthetic params/mnist.prms` (SEED 11, two epochs of 200 synthetic images: the file itself draws a seed
    per run and trains for 101 epochs) on the CPU backend: stdout byte for byte as recorded from the commit before the
    per_image mode (tests/golden/train_mnist_cpu_stdout.txt)."""
    with open(os.path.join(ROOT, "params", "mnist.prms")) as fh:
        prms = ast.literal_eval(fh.read())
    prms["training_params"].update(SEED=11, NUM_EPOCHS=2, TEST_SAMP_SZ=100)
    (tmp_path / "mnist.prms").write_text(repr(prms))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "synthetic", "mnist.prms"], cwd=str(tmp_path),
                       env=_env(THEANET_SYNTH_TRAIN="200", THEANET_SYNTH_TEST="100", THEANET_NO_PICKLE="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(os.path.join(ROOT, "tests", "golden", "train_mnist_cpu_stdout.txt")) as fh:
        want = fh.read()
    assert _report(r.stdout) == want
    # ... and the per-image spec trains through the same command line
    with open(os.path.join(ROOT, "params", "mnist_img.prms")) as fh:
        prms = ast.literal_eval(fh.read())
    prms["training_params"].update(SEED=11, NUM_EPOCHS=2, TEST_SAMP_SZ=100)
    (tmp_path / "mnist_img.prms").write_text(repr(prms))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "synthetic", "mnist_img.prms"], cwd=str(tmp_path),
                       env=_env(THEANET_SYNTH_TRAIN="200", THEANET_SYNTH_TEST="100", THEANET_NO_PICKLE="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Fields:PerImage" in r.stdout and "per_image : \tTrue" in r.stdout
    rows = [l for l in r.stdout.splitlines() if l.strip().startswith(("0 ", "1 ", "2 "))]
    assert len(rows) == 3 and all(np.isfinite(float(l.split()[1])) for l in rows), r.stdout[-1500:]
