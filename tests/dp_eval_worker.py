"""Worker of tests/test_eval_sweep_cpu.py: one rank of a data-parallel job that trains a few steps and then evaluates a
run of minibatches both ways -- ``fn(i)`` per minibatch (one collective and one copy back each) and ``sweep(indices)``
(one of each for the run).  Every rank stores both results as float32 bit patterns; the test compares the forms and the
ranks."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_stem, B, steps):
    from tests.gpu_util import load_prms
    from theanet_amd import NeuralNet, comm
    prms = load_prms("mnist.prms", 28, batch=B)
    rng = np.random.RandomState(3)
    x = rng.rand(4 * B, 1, 28, 28).astype(np.float32)
    y = rng.randint(0, 10, 4 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
    fn, te = net.get_trin_model(x, y), net.get_test_model(x, y)
    world = comm.get_world()
    idx = [0, 1, 2, 3, 1, 0]
    res = {}
    for phase in ("a", "b"):                # (the second phase: a sweep behind further steps, into the array it has kept)
        for s in range(steps):
            fn.enqueue(s % 4)
        res["sweep_" + phase] = np.array(te.sweep(idx), np.float32).view(np.uint32)
        res["calls_" + phase] = np.array([te(i) for i in idx], np.float32).view(np.uint32)
    if world.size > 1:
        issued = net._group().n_issued
        te.sweep(idx)
        assert net._group().n_issued == issued + 1, "a sweep is ONE collective"
        net._group().verify_order()
    np.savez("%s.rank%d.npz" % (out_stem, world.rank), **res)


if __name__ == "__main__":
    from tests import guard_util
    guard_util.install()            # guard bands and 0xFF poison around every device buffer of this rank
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    guard_util.check_all()
