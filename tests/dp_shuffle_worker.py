"""Worker of tests/test_shuffle_cpu.py: one rank of a data-parallel job whose training function has a row order set
(set_order).  Every rank draws the order from ``order_seed`` (+ its rank when ``disagree`` is 1: the ranks must then fail
at set_order with the agreement error); a second order follows half way.  Rank 0 stores the costs and the weights after
the last step."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_path, B, steps, order_seed, disagree):
    from tests.gpu_util import load_prms
    from theanet_amd import NeuralNet, comm
    prms = load_prms("mnist.prms", 28, batch=B)
    rng = np.random.RandomState(3)
    x = rng.rand(4 * B, 1, 28, 28).astype(np.float32)
    y = rng.randint(0, 10, 4 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
    fn = net.get_trin_model(x, y)
    world = comm.get_world()
    seed = order_seed + (world.rank if disagree else 0)
    fn.set_order(np.random.RandomState(seed).permutation(4 * B))
    costs = []
    for s in range(steps):
        if s == steps // 2:
            fn.set_order(np.random.RandomState(seed + 100).permutation(4 * B)[:3 * B])
        costs.append(float(fn(s % 3)[0]))
    wts = [w for l in net.tr_layers for w in l.get_wts()]
    if world.size > 1:
        net._group().verify_order()
    if world.rank == 0:
        np.savez(out_path, costs=np.array(costs), pipelined=type(fn).__name__ == "_PipeTrainFn" and fn._seq is None,
                 **{"w%d" % i: w for i, w in enumerate(wts)})


if __name__ == "__main__":
    from tests import guard_util
    guard_util.install()            # guard bands and 0xFF poison around every device buffer of this rank
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    guard_util.check_all()
