"""Worker of tests/test_elastic_img_cpu.py::test_two_ranks_distort_their_rows_like_one_rank: one rank of a data-parallel
job training the tiny per-image net of tests/test_gpu_elastic_img.py for two steps with GENERATED draws.  Every rank
stores its rows of the first layer's output after each step and where they sit in the global minibatch."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_stem):
    from tests.test_gpu_elastic_img import _data, _tiny
    from theanet_amd import NeuralNet, comm
    layers, tr = _tiny()
    x, y = _data(2)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    fn = net.get_trin_model(x, y)
    outs, costs = [], []
    for s in range(2):
        costs.append(float(fn(s)[0]))
        outs.append(net.tr_layers[0].output.get_value())
    world = comm.get_world()
    np.savez("%s_r%d.npz" % (out_stem, world.rank), outs=np.stack(outs), costs=np.array(costs), lo=net.shard_lo,
             rows=net.local_bsz, world=world.size)


if __name__ == "__main__":
    main(sys.argv[1])
