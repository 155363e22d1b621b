"""NeuralNet -- the drop-in for theanet/neuralnet.py on MI355X.

Same constructor, same ``.prms`` layer-spec surface and the same methods as the
reference class (neuralnet.py:59-332), but instead of building twin Theano graphs
and compiling them, construction plans device buffers (weights, activations,
gradients all resident in HBM) and the step functions enqueue hand-written HIP
kernels through the C-ABI of libtheanet_hip.so.  Per training step only the
minibatch index crosses the host/device boundary.

Data-parallel: one process per GPU (RANK/WORLD_SIZE from torch.distributed.run);
rank r works on rows [i*B + r*B/R, i*B + (r+1)*B/R) of minibatch i and the flat
gradient buffer (+ the scalar cost) is sum-all-reduced once per step over RCCL.
"""
import contextlib
import numbers
import os
import sys
import weakref
from functools import reduce
from operator import mul

import numpy as np

from . import _lib, comm, layer
from .dpsched import DpSchedule
from .plan import StepPlan
from .device import DeviceArray, get_context, is_c8, share
from .layer.c8 import OperandTiles, check_follows, pool_stands_alone
from .layer.convpool import pool_mask_enabled
from .layer import (AuxConcatLayer, SoftAuxLayer, CenteredOutLayer, ColorLayer, ConvLayer, DropOutLayer, ElasticLayer, ExpLossLayer, HiddenLayer,
                    HingeLayer, InputLayer, InputSlot, MeanLayer, OutputLayer, PoolLayer, SoftmaxLayer)

# ########################### Helper Functions #################################


def get_layers_info(layers):
    out = []
    for name, args in layers:
        out.append('\n{} : '.format(name))
        out.extend('\n\t{} : \t{}'.format(key, args[key]) for key in args)
    return ''.join(out)


def get_wts_info(wts, detailed=False):
    out, n_wts = [], 0
    for l, ww in enumerate(wts):
        out.append("\nLayer {}:".format(l))
        for w in ww:
            n_ww = reduce(mul, w.shape)
            n_wts += n_ww
            out.append('\n\t {} {} ❲{}❳'.format(w.shape, w.dtype, n_ww))
            if detailed:
                out.append(" ❲{:.2e}, {:.2e}, {:.2e}❳".format(w.min(), w.mean(), w.max()))
    out.append('\n\nTotal Number of Weights : {:,}'.format(n_wts))
    return ''.join(out)


def get_training_params_info(training_params):
    return "Training Parameters:" + ''.join(
        '\n\t{} : \t{}'.format(key, training_params[key]) for key in sorted(training_params))


_GRAD_ALIGN = 64      # floats: every tensor in the flat gradient buffer starts 256-byte aligned


# The "compiled functions" get_trin_model / get_test_model return live in trainfn.py
from .trainfn import _PipeTrainFn, _TestFn, _TrainFn  # noqa: E402,F401


# ###############################################################################
#                            The Neural Network
# ###############################################################################


def _fma32(m, v, c):
    """fl32(m * v + c) with ONE rounding, element-wise (the device's __fmaf_rn; numpy has no fma).  m * v is exact in
    float64 (24 + 24 bits); the float64 sum may round, and rounding that to float32 rounds twice -- wrong only when the
    float64 sum lands exactly on a float32 midpoint that the exact sum is not on.  The error of the float64 addition
    (TwoSum) says which side the exact sum lies on."""
    p = np.float64(m) * np.asarray(v, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # exact: p + c = s + err
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)                         # exact (both on the float64 grid near r)
    up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
    half_up = (up.astype(np.float64) - r.astype(np.float64)) / 2
    half_dn = (r.astype(np.float64) - dn.astype(np.float64)) / 2
    tie_up, tie_dn = (d == half_up) & (d > 0), (-d == half_dn) & (d < 0)
    # on a midpoint the float64 -> float32 step went to even; the exact sum is off the midpoint by err
    r = np.where(tie_up & (err > 0), up, r)              # exact sum above the midpoint: the upper neighbour
    r = np.where(tie_dn & (err < 0), dn, r)
    return r.astype(np.float32)


class NeuralNet():
    fuse_conv_pool = True     # class-level switch (tests run both the fused and unfused paths)
    # ... and the step-level fusions (slab sums and cost inside the update launch, the next minibatch's elastic field riding in a backward launch or beside the update, two steps in flight):
    # False = the generic schedule, one launch per piece of work -- what the fused schedules are tested against
    fused_step = True
    # the C-ABI ops that carry a net's conv products (bench.py brackets them for the conv roofline legs)
    CONV_FWD_OPS = ("tn_conv2d_fwd", "tn_convpool_fwd_mask", "tn_elastic_convpool_fwd_mask", "tn_c8_conv_fwd",
                    "tn_c8_conv1_fwd")
    CONV_BWD_OPS = ("tn_conv2d_wgrad", "tn_conv2d_dgrad", "tn_convpool_bwd_mask_dx", "tn_convpool_bwd_mask",
                    "tn_convblock_bwd_mask", "tn_convblock_bwd", "tn_convpool_bwd", "tn_c8_conv_wgrad", "tn_c8_conv_dgrad",
                    "tn_c8_conv1_wgrad", "tn_c8_conv1_dgrad")

    # step state (class-level: the twin of the pipelined schedule is given _is_twin / _main before its __init__ runs)
    _is_twin, _main = False, None     # the second net of a _PipeTrainFn (odd steps) and the net it is the twin of
    _pipe_fn = None           # the _PipeTrainFn that has two steps of this net in flight
    _want_outputs = False     # the caller of this step reads [cost, features, logprob]: they are sent ahead
    _early = None             # page-locked landing buffers of _send_outputs
    _cost_pending = None      # pipelined: the last step's cost waits for the update that opens the stream's next step
    _cost_guard_ev = None     # a step_cost() loop's copy of d_cost that the next launch writing d_cost must wait for
    _mn_tab = None            # _maxnorm_table's table
    _wc_tab = None            # _wtcost_table's table
    # WT_AVG: per layer the averages of its tensors (None: a layer without updates), tn_avg_net's device table for this
    # net's own weight buffers (the twin of the pipelined schedule: its weights, the SAME averages), rows, largest row
    _avg = _avg_tab = None
    _avg_nseg = _avg_max = 0
    _avg_swapped = False      # inside _at_avg_wts: the weight buffers hold the averages
    # what bench.py and the data-parallel workers read of the schedules (dpsched.py)
    dp_schedule = property(lambda self: self.dp.schedule)
    dp_tuned_ms = property(lambda self: self.dp.tuned_ms)
    _dp_bucket = property(lambda self: self.dp.bucket)
    _dp_cand = property(lambda self: self.dp.cand)
    _dp_can_delay = property(lambda self: self.dp.can_delay)
    _dp_tune = property(lambda self: self.dp.tune)

    def __init__(self, layers, training_params, allwts=None,
                 test_x=None):
        # Either a random seed or the weights of a previously trained net (neuralnet.py:63-68)
        if allwts is None:
            self.rand_gen = np.random.RandomState(training_params['SEED'])
        else:
            self.rand_gen = None

        self.ctx = get_context()             # raises without libtheanet_hip.so / a GPU
        # the SoftmaxLayer's training step as one kernel (tn_fc_softmax_train) or as its three ops: a choice of kernels
        # (results agree to rounding, not bit for bit) -- the library's TN_SOFTMAX_TRAIN, which gemm.hip reads too
        self._softmax_train = self.ctx.knobs()["TN_SOFTMAX_TRAIN"] != 0
        # DTYPE: 'float32' (default = the reference's floatX, weights.py:8), 'float16' = fp16 operands /
        # fp32 accumulation for the conv products, fp32 master weights, or 'bfloat16' = the same with bf16 (fp32's
        # exponent range); GRAD_SCALE: power of two applied to dz before it is rounded to the 16-bit type (results are
        # scaled back: exact), default 4096 for float16 and 1 for bfloat16 (which needs none)
        self.dtype = training_params.get('DTYPE', 'float32')
        assert self.dtype in ('float32', 'float16', 'bfloat16'), "DTYPE must be 'float32', 'float16' or 'bfloat16'"
        self.grad_scale = float(training_params.get('GRAD_SCALE', 1. if self.dtype == 'bfloat16' else 4096.))
        # MATMUL: 'float32' (default: exact fp32 MFMA), 'bf16x3' -- the dense layers' products as six bf16 MFMA
        # products of exactly split operands (fp32-grade accuracy, not the same bits; gemm_b3.hip) -- or 'bfloat16':
        # every HiddenLayer's three products on bf16-rounded operands with fp32 accumulation (gemm_bf16.hip; reduced
        # precision, the conv stack's 16-bit arithmetic; any layer shape; the output heads stay fp32).  Independent
        # of DTYPE: the dense layer directly on a 16-bit conv stack keeps tn_c8_fc_*.
        self.matmul = training_params.get('MATMUL', 'float32')
        assert self.matmul in ('float32', 'bf16x3', 'bfloat16'), "MATMUL must be 'float32', 'bf16x3' or 'bfloat16'"
        # CONV: 'float32' (default: the fp32 conv kernels, fused conv+pool blocks included) or 'bfloat16': every ConvLayer's
        # three products on bf16-rounded operands with fp32 accumulation, for every shape a ConvLayer can be built with
        # (conv_bf16.hip; reduced precision; tensors and weights stay fp32; conv layers are not fused with their pool or
        # elastic layer).  Independent of MATMUL; not a mode of the 16-bit conv stack, which has its own kernels.
        self.conv_mm = training_params.get('CONV', 'float32')
        assert self.conv_mm in ('float32', 'bfloat16'), "CONV must be 'float32' or 'bfloat16'"
        assert not (self.conv_mm == 'bfloat16' and self.dtype in ('float16', 'bfloat16')), (
            "CONV 'bfloat16' with DTYPE '{}': the 16-bit conv stack already runs 16-bit products on every conv layer it "
            "takes; CONV is for float32 nets".format(self.dtype))
        # CONV_SHAPES: 'tiled' (default) -- under a 16-bit DTYPE a ConvLayer must be one of the two tiled shapes (3x3 stride-1
        # 'same', 1x1 stride-1) or construction fails -- or 'any': every other filter, mode and stride runs on the general
        # family (convg_c8.hip), unfused: a PoolLayer above such a layer, or a 2x2 one on an odd map, stands alone.  The
        # tiled shapes keep their kernels and their bits.  No effect under DTYPE 'float32' (the fp32 kernels take every shape).
        self.conv_shapes = training_params.get('CONV_SHAPES', 'tiled')
        assert self.conv_shapes in ('tiled', 'any'), "CONV_SHAPES must be 'tiled' or 'any', not {!r}".format(self.conv_shapes)
        # STACK_HEAD: 'dense' (default) -- under a 16-bit DTYPE a HiddenLayer must follow the conv stack -- or 'any': an output
        # head (Softmax, ExpLoss, Hinge, CenteredOut, SoftAux layer) may sit on a stack tensor; it reads the 16-bit tensor as a
        # HiddenLayer does, a head of at most 16 outputs on kernels of its own (head_c8.hip).  No effect under DTYPE 'float32'.
        self.stack_head = training_params.get('STACK_HEAD', 'dense')
        assert self.stack_head in ('dense', 'any'), "STACK_HEAD must be 'dense' or 'any', not {!r}".format(self.stack_head)
        # WT_AVG: d, 0 < d < 1 -- an exponential moving average of the weights (Polyak averaging) that test functions and
        # checkpoints use: a_t = a_{t-1} + c (p_t - a_{t-1}), c = fl(1 - d), p_t = the weights after step t's update and
        # max-norm projection, a_0 = the weights the net starts from (include/theanet_hip.h, tn_avg_net).  Absent, None
        # or 0: off -- no buffer, no call.
        d = training_params.get('WT_AVG')
        assert d is None or (isinstance(d, numbers.Real) and not isinstance(d, bool) and (d == 0 or 0 < d < 1)), \
            "WT_AVG must be a decay d with 0 < d < 1 (None or 0: no averaging), not {!r}".format(d)
        self.wt_avg = float(d) if d else 0.0
        self._avg_c = float(np.float32(1.0 - self.wt_avg))        # rounded once, here
        self._apply_dtype()
        self.world = comm.get_world()
        self._dev_group = None
        self.dp = DpSchedule(self)           # when the gradients are all-reduced (inert on a single GPU)

        self.tr_prms = training_params
        self.layers = layers
        self.allwts = allwts
        self.tr_layers = []
        self.te_layers = []
        self.batch_sz = training_params['BATCH_SZ']
        self.shard_lo, hi = comm.shard_rows(self.batch_sz, self.world.size, self.world.rank)
        self.local_bsz = hi - self.shard_lo
        self.num_layers = 0

        # "symbolic variables": windows into device-resident datasets
        self.x = InputSlot(self.local_bsz)
        self.y = None
        if test_x is None:
            self.test_x = InputSlot(self.local_bsz)
        else:
            self.test_x = InputSlot(self.local_bsz)
            self.test_x.bind(share(test_x))

        # device-side step state (read by the kernels, so a captured graph can be replayed)
        self._c8_tiles = OperandTiles(self.ctx)            # the 16-bit stack's 3x3 conv weights as operand tiles
        self.d_step = self.ctx.zeros((1,), np.uint32)       # RNG step counter
        self.d_row0 = self.ctx.zeros((1,), np.int64)        # first dataset row of the minibatch
        self.cur_learn_rate = self.ctx.zeros((1,), np.float32)
        # Input Layer
        input_layer_type = getattr(layer, layers[0][0])
        assert input_layer_type in (InputLayer, ElasticLayer, ColorLayer), \
            "First layer needs to be Input or Elastic or Color Layer"

        self.tr_layers.append(input_layer_type(self.x, rand_gen=self.rand_gen,
                                               **layers[0][1]))
        self.te_layers.append(self.tr_layers[0].TestVersion(self.test_x))
        self.num_layers += 1

        # Rest of the layers
        while self.num_layers < len(layers):
            self.append_next_layer()

        # (CONV 'bfloat16': the fused conv+pool / elastic+conv+pool blocks compute in fp32 and are not used -- every conv
        # layer runs tn_conv2d_*, its pool tn_pool_*)
        if self.fuse_conv_pool and self.conv_mm != 'bfloat16':
            self._fuse(self.tr_layers)
            self._fuse(self.te_layers)

        # Handle Auxiliary input (neuralnet.py:100-105)
        for tr_layer, te_layer in zip(self.tr_layers, self.te_layers):
            if type(tr_layer) in (AuxConcatLayer, SoftAuxLayer):
                assert not hasattr(self, 'aux_inpt_tr'), "Multiple Aux Inputs"
                self.aux_inpt_tr = tr_layer.aux_inpt
                self.aux_inpt_te = te_layer.aux_inpt
                tr_layer.aux.d_step = self.d_step

        assert isinstance(self.tr_layers[-1], OutputLayer), \
            "the last layer must be an output head (Softmax, ExpLoss, Hinge or CenteredOut layer)"

        # random streams read the device step counter; masks/noise are keyed by the
        # position inside the GLOBAL minibatch so that sharding does not change them
        for lyr in self.tr_layers:
            if isinstance(lyr, (ElasticLayer, ColorLayer)):
                lyr.d_step = self.d_step
                lyr.shard_lo = self.shard_lo      # (a per-image ElasticLayer in the middle of a net keys its draws by it)
            drop = getattr(lyr, "drop", None)
            if drop is not None:
                drop.d_step = self.d_step
                drop.elem0 = self.shard_lo * int(np.prod(drop.shape[1:]))
        out = self.tr_layers[-1]
        out.inv_batch = 1.0 / self.batch_sz          # global batch: grads sum to the mean
        self.te_layers[-1].inv_batch = 1.0 / self.batch_sz

        self._grads_ready = False
        if self.wt_avg and not self._is_twin:
            self._avg = [[self.ctx.empty(p.shape) for p in lyr.params] if lyr.has_updates() else None
                         for lyr in self.tr_layers]
            for lyr, avs in zip(self.tr_layers, self._avg):
                for p, a in zip(lyr.params, avs or ()):
                    self.ctx.call("tn_d2d", a.ptr, p.ptr, p.size * 4)
            self._build_avg_table(self)

        # Set Epoch and learning rate
        if 'CUR_EPOCH' not in training_params:
            training_params['CUR_EPOCH'] = 0
        self.set_rate()

    def append_next_layer(self):
        layer_type, layer_args = self.layers[self.num_layers]
        prev_tr_layer = self.tr_layers[self.num_layers - 1]
        prev_te_layer = self.te_layers[self.num_layers - 1]
        wts = self.allwts[self.num_layers] if self.allwts else None

        tr_inpt = prev_tr_layer.output
        te_inpt = prev_te_layer.output
        curr_layer_type = getattr(layer, layer_type)
        if is_c8(tr_inpt):
            # 16-bit-resident tensors of the conv stack (device.C8Array) pass from layer to layer as they are
            check_follows(self.dtype, prev_tr_layer, layer_type, layer_args.get("pool_sz"), self.fuse_conv_pool,
                          self.conv_shapes == 'any', stack_head=self.stack_head == 'any', stride=layer_args.get("stride"))

        if curr_layer_type in (ElasticLayer, ColorLayer, ConvLayer, PoolLayer, MeanLayer):
            use_tr_layer, k = prev_tr_layer, self.num_layers - 1
            while type(use_tr_layer) is DropOutLayer:
                k -= 1
                use_tr_layer = self.tr_layers[k]
            num_prev_maps = use_tr_layer.num_maps
            prev_out_sz = use_tr_layer.out_sz
            if not is_c8(tr_inpt) and tr_inpt.ndim != 4:
                tr_inpt = tr_inpt.reshape(self.local_bsz, num_prev_maps, prev_out_sz, prev_out_sz)
                te_inpt = te_inpt.reshape(self.local_bsz, num_prev_maps, prev_out_sz, prev_out_sz)

        if curr_layer_type in (ElasticLayer, ColorLayer):
            layer_args = dict(layer_args)
            layer_args.pop("num_maps", None)
            layer_args.pop("img_sz", None)
            curr_layer = curr_layer_type(tr_inpt,
                                         num_maps=num_prev_maps,
                                         img_sz=prev_out_sz,
                                         rand_gen=self.rand_gen,
                                         **layer_args)
            if getattr(curr_layer, "img_field", False) and any(lyr.has_updates() for lyr in self.tr_layers):
                raise ValueError("ElasticLayer per_image in the middle of a net with a trainable layer below it (layer %d): "
                                 "the backward pass of a per-image field is not implemented -- move the layer below the "
                                 "first trainable layer or drop 'per_image'" % self.num_layers)

        elif curr_layer_type is ConvLayer:
            curr_layer = ConvLayer(tr_inpt,
                                   wts,
                                   self.rand_gen,
                                   self.local_bsz,
                                   num_prev_maps,
                                   prev_out_sz,
                                   dtype=self.dtype,
                                   conv_shapes=self.conv_shapes,
                                   **layer_args)

        elif curr_layer_type in (PoolLayer, MeanLayer):
            if curr_layer_type is PoolLayer and is_c8(tr_inpt):
                # 16-bit stack: half of a fused conv + pool block, or a layer of its own that -- like a DropOutLayer --
                # stands for the block below it (PoolLayer.act_info)
                layer_args = dict(layer_args, c8_alone=pool_stands_alone(layer_args.get("pool_sz"), self.fuse_conv_pool,
                                                                         prev_tr_layer, self.conv_shapes == 'any',
                                                                         stride=layer_args.get("stride")))
            curr_layer = curr_layer_type(tr_inpt,
                                         num_maps=num_prev_maps,
                                         in_sz=prev_out_sz,
                                         **layer_args)
            if curr_layer_type is PoolLayer:
                curr_layer.below = prev_tr_layer

        elif curr_layer_type is DropOutLayer:
            curr_layer = DropOutLayer(tr_inpt,
                                      self.rand_gen,
                                      prev_tr_layer.n_out,
                                      **layer_args)
            # on the 16-bit stack the layer stands for the block below it (DropOutLayer.act_info)
            curr_layer.below = prev_tr_layer

        elif curr_layer_type is CenteredOutLayer:
            # Needs the hidden layer's weights (or a seed) and CENTERS (n_classes x n_features): neuralnet.py:175-194
            centers = None
            if wts:
                centers = wts[2] if len(wts) > 2 else None
                wts = wts[:2]
            if not is_c8(tr_inpt):          # (STACK_HEAD 'any': a head takes the stack tensor as it is, like a HiddenLayer)
                tr_inpt, te_inpt = tr_inpt.flatten(2), te_inpt.flatten(2)
            curr_layer = CenteredOutLayer(tr_inpt,
                                          wts, centers,
                                          self.rand_gen,
                                          prev_tr_layer.n_out,
                                          **layer_args)

        elif curr_layer_type is HiddenLayer and is_c8(tr_inpt):
            # 16-bit stack: the dense layer above the conv stack reads the 16-bit-resident tensor in ITS order (the
            # kernels walk W through the NCHW row map of flatten(2), neuralnet.py:168-173)
            curr_layer = HiddenLayer(tr_inpt, wts, self.rand_gen, prev_tr_layer.n_out, **layer_args)

        elif curr_layer_type in (AuxConcatLayer, HiddenLayer, SoftmaxLayer, SoftAuxLayer, HingeLayer, ExpLossLayer):
            if not is_c8(tr_inpt):          # (STACK_HEAD 'any': a head takes the stack tensor as it is, like a HiddenLayer)
                tr_inpt, te_inpt = tr_inpt.flatten(2), te_inpt.flatten(2)
            curr_layer = curr_layer_type(tr_inpt,
                                         wts,
                                         self.rand_gen,
                                         prev_tr_layer.n_out,
                                         **layer_args)
        else:
            raise NotImplementedError("Unknown Layer Type" + layer_type)

        self.tr_layers.append(curr_layer)
        self.te_layers.append(curr_layer.TestVersion(te_inpt))
        if not self._is_twin:
            curr_layer._wts_hook = self.te_layers[-1]._wts_hook = self._sync_weights
        self.num_layers += 1

    @staticmethod
    def _fuse(lyrs):
        """Pair every ConvLayer that is directly followed by a 2x2 PoolLayer (and is small
        enough for the register-resident kernel) into one fused conv+act+pool launch."""
        for conv, pool in zip(lyrs[:-1], lyrs[1:]):
            family = conv.can_fuse_with(pool) if isinstance(conv, ConvLayer) and isinstance(pool, PoolLayer) else None
            if family:
                conv.fuse(pool, family)
        # 16-bit stack: the first conv layer packs its c8 input straight from the dataset window
        if len(lyrs) >= 2 and isinstance(lyrs[0], InputLayer) and isinstance(lyrs[1], ConvLayer) and lyrs[1].f16:
            lyrs[1]._pack_from, lyrs[0]._packed_by_conv = lyrs[0].inpt, True
        # ... or has it written by the distortion stage below it (tn_c8_elastic_apply): no fp32 image, no packing pass
        if len(lyrs) >= 2 and isinstance(lyrs[0], ElasticLayer) and lyrs[0].active and isinstance(lyrs[1], ConvLayer) \
                and lyrs[1].f16 and lyrs[1].x16 is not None and (lyrs[0].img_sz * lyrs[0].img_sz) % 4 == 0 \
                and not lyrs[1].x16.padded:
            # (maps stored at a pitch > their side: the stage writes its fp32 output and the conv layer packs it into the
            # padded layout, tn_c8_pack_pitch)  (a per-image layer writes it through tn_c8_elastic_apply_img)
            lyrs[0]._c8_consumer, lyrs[1]._c8_prefilled = lyrs[1], True
        # an active single-channel ElasticLayer feeding such a block: the block's forward resamples
        # the raw images itself (tn_elastic_convpool_fwd_mask)
        # (not a per-image layer: the block reads ONE sample map)
        if len(lyrs) >= 3 and isinstance(lyrs[0], ElasticLayer) and lyrs[0].active and not lyrs[0].img_field and \
                lyrs[0].num_maps == 1 and not getattr(lyrs[1], "f16", False) and isinstance(lyrs[1], ConvLayer) and \
                lyrs[1].fused_pool is lyrs[2]:
            el, conv, pool = lyrs[0], lyrs[1], lyrs[2]
            if conv.ctx.lib.tn_elastic_convpool_supported(
                    el.img_sz, el.img_sz, conv.num_maps, conv.filter_sz, conv.pad_lo, conv.out_sz,
                    conv.out_sz, pool.pool_sz, pool.out_sz, pool.out_sz) and not pool.ignore_border:
                el.fused_conv, pool.fused_elastic = conv, el

    _ctx_owner = None       # weakref to the net whose pipelined steps may have work parked in the context

    def _apply_dtype(self):
        """Called at the start of everything this net enqueues: sets the context's matmul dtype and takes
        over the context from whichever net used it last.  A pipelined training function leaves a step's
        slab sums and cost parked with its stream until the stream's next step; before another net's work
        goes onto those streams they are finished (the other net is alive: its buffers exist) or forgotten
        (it has been collected: the recorded outputs are dangling)."""
        self.ctx.set_matmul_dtype(self.dtype, self.grad_scale)
        self.ctx.set_fc_matmul(self.matmul)
        self.ctx.set_conv_matmul(self.conv_mm)
        me = self._main or self
        ref = NeuralNet._ctx_owner
        prev = ref() if ref is not None else None
        if prev is me:
            return
        if prev is not None and prev._pipe_fn is not None:
            prev._pipe_fn._flush_parked()
        elif ref is not None:
            self.ctx.call("tn_defer_discard")
        NeuralNet._ctx_owner = weakref.ref(me)

    # ------------------------------------------------------------------------------
    def _group(self):
        if self._dev_group is None:
            self._dev_group = comm.DeviceGroup(self.ctx, self.world)
        return self._dev_group

    def _prepare_training(self):
        """Flat gradient buffer (all dW/db as views, + the scalar cost at the end so that
        ONE all-reduce moves everything) and the velocity buffers (layer.py:77-79)."""
        if self._grads_ready:
            return
        plist = [(lyr, p) for lyr in self.tr_layers for p in lyr.params]
        offs, total, self.n_flat = comm.flat_layout([p.size for _, p in plist], _GRAD_ALIGN)
        slots = [(lyr, p, off) for (lyr, p), off in zip(plist, offs)]
        self.flat_grads = self.ctx.zeros((total + _GRAD_ALIGN,))
        self.d_cost = self.flat_grads.view(total, (1,))
        for lyr in self.tr_layers:
            if lyr.params:
                lyr.grads = []
                lyr.accumulated_updates = []
        for lyr, p, off in slots:
            lyr.grads.append(self.flat_grads.view(off, p.shape))
            lyr.accumulated_updates.append(self.ctx.zeros(p.shape))
        self.tr_layers[-1].d_cost = self.d_cost
        host = self._build_seg_table()
        # the minibatch cost can ride in the update launch unless something must be added to it
        # first (weight costs) or it has to travel through the all-reduce (data-parallel ranks)
        self._has_wtcost = has_wtcost = any(getattr(l, 'reg', None) and l.params and (l.reg['L1'] or l.reg['L2'])
                                            for l in self.tr_layers)
        # data-parallel step (TN_DP_FORCE=1: exercise it with a 1-rank communicator)
        self._dp = self.world.size > 1 or os.environ.get("TN_DP_FORCE") == "1"
        self._cost_rider = self.fused_step and (not has_wtcost) and not self._dp
        # ... and with weight costs on a single GPU: ONE launch of its own right behind the output layer's forward, when
        # the step's weights are current and its row losses exist (tn_wtcost_net)
        self._cost_net = self.fused_step and has_wtcost and not self._dp
        self._wtcost_table()
        # which layers must propagate a gradient to their input
        self._need_gin = []
        seen = False
        for lyr in self.tr_layers:
            self._need_gin.append(seen)
            seen = seen or lyr.has_updates()
        if self._dp and not self.world.dry:
            self._group()
            if self.world.size > 1 and not self._is_twin:
                # replicas must start from identical weights (same SEED or same checkpoint on every rank)
                chk = float(sum(np.float64(w.astype(np.float64).sum()) for l in self.tr_layers for w in l.get_wts()))
                comm.agree(chk, "the initial weights (checksum)")
                # The ORDER in which partial sums are added is part of a gradient's bits, and replicas must stay
                # bit-identical: the library's switches that set slab counts / kernel forms (as it resolved them), the
                # Python-side ones that pick kernels and the CU count the slab geometry is cut for must be the same on
                # every rank (a rank with another TN_C8_WSLAB_DIV or another device would round differently, silently)
                import zlib
                sig = "|".join("%s=%s" % kv for kv in self.ctx.knobs().items())
                sig += "|TN_POOL_MASK=%d|TN_MN_FUSED=%s" % (pool_mask_enabled(), os.environ.get("TN_MN_FUSED", ""))
                # (the head's route -- TN_C8_HEAD, seen through tn_c8_head_supported -- fixes the order of its sums)
                sig += "|CONV_SHAPES=%s|STACK_HEAD=%s|C8_HEAD=%d" % (self.conv_shapes, self.stack_head,
                                                                    any(getattr(l, "c8_head", False) for l in self.tr_layers))
                sig += "|cus=%s" % self.ctx.info()[1]
                comm.agree(float(zlib.crc32(sig.encode())), "the kernel tunables / CU count (%s)" % sig)
        self.dp.prepare(slots, host)
        self._grads_ready = True

    def _build_seg_table(self):
        """One multi-tensor momentum-SGD launch for every parameter tensor (layer.py:70-107): the table
        of (param, velocity, gradient, ...) segments, on the device and (for the lazy update) on the host.
        Rebuilt whenever a layer's velocity buffers are re-pointed (the twin of the pipelined schedule)."""
        seg_dt = np.dtype([('p', 'u8'), ('v', 'u8'), ('g', 'u8'), ('n', 'u8'),
                           ('momentum', 'f4'), ('rate', 'f4'), ('L1', 'f4'), ('L2', 'f4')])
        segs = []
        for lyr in self.tr_layers:
            if lyr.has_updates():
                for p, v, g in zip(lyr.params, lyr.accumulated_updates, lyr.grads):
                    segs.append((p.ptr, v.ptr, g.ptr, p.size, lyr.reg['momentum'], lyr.reg['rate'],
                                 lyr.reg['L1'], lyr.reg['L2']))
        self._n_segs = len(segs)
        self._max_seg = max([sg[3] for sg in segs] or [0])
        host = np.array(segs, dtype=seg_dt)
        if segs:
            self._d_segs = self.ctx.array(host.view(np.uint8))
            self._h_segs = host                       # kept alive: tn_sgd_update_net (TN_UPD_LAZY) reads it
        return host

    def _build_avg_table(self, main):
        """tn_avg_net's table (tn_avg_seg rows) for THIS net's weight buffers and ``main``'s averages (the twin of the
        pipelined schedule keeps none of its own: the averages are one chain across both streams).  Built once."""
        seg_dt = np.dtype([('p', 'u8'), ('a', 'u8'), ('n', 'u8'), ('reserved', 'u8')])
        assert seg_dt.itemsize == 32          # tn_avg_seg
        rows = [(p.ptr, a.ptr, p.size, 0) for lyr, avs in zip(self.tr_layers, main._avg)
                for p, a in zip(lyr.params, avs or ())]
        self._avg_nseg, self._avg_max = len(rows), max([r[2] for r in rows] or [0])
        self._avg_tab = self.ctx.array(np.array(rows, dtype=seg_dt).view(np.uint8)) if rows else None

    def _avg_update(self):
        """Behind whatever has just produced p_t in this net's weight buffers (update and max-norm projection), on its
        stream: p_t enters the averages.  Without WT_AVG: nothing."""
        if self._avg_tab is not None:
            self.ctx.call("tn_avg_net", self._avg_tab.ptr, self._avg_nseg, self._avg_max, self._avg_c, _lib.TN_AVG_UPDATE)

    def _avg_exchange(self):
        """Weights and averages change places (tn_avg_net, TN_AVG_EXCHANGE: bit copies); the 16-bit stack's arranged
        operand tiles are no longer the weights'."""
        self.ctx.call("tn_avg_net", self._avg_tab.ptr, self._avg_nseg, self._avg_max, self._avg_c, _lib.TN_AVG_EXCHANGE)
        self._c8_tiles.stale()

    def _averaged(self, averaged):
        """What ``averaged`` of get_test_model / get_data_test_model means for this net: None = iff WT_AVG is on."""
        if averaged is None:
            return self._avg_tab is not None
        assert not averaged or self._avg_tab is not None, "averaged=True: this net keeps no averaged weights (WT_AVG is off)"
        return bool(averaged)

    @contextlib.contextmanager
    def _at_avg_wts(self, averaged):
        """An evaluation at the averaged weights: ONE exchange in front of everything it does and one behind it (also when
        it raises), whatever the number of minibatches in between.  The net is brought up to date first; afterwards the
        device is idle, so a training step on either stream finds the weights back."""
        if not averaged:
            yield
            return
        assert not self._avg_swapped, "an evaluation at the averaged weights inside another"
        self._sync_weights()
        self._apply_dtype()
        self._avg_exchange()
        self._avg_swapped = True
        try:
            yield
        finally:
            self._avg_swapped = False
            self._avg_exchange()
            self.ctx.sync()

    def _send_outputs(self, out, with_cost=False):
        """The step's features / logprob start travelling to page-locked host memory now (ordered behind the
        output layer's forward, on the context's copy stream): the copies run under the backward pass instead
        of after the step (the drop-in call fn(i) reads them every step, neuralnet.py:236-241)."""
        from .device import HostBuffer
        early = self._early
        if early is None:
            early = self._early = {"live": False, "logprob": HostBuffer(self.ctx, out.logprob.shape),
                                   "cost": HostBuffer(self.ctx, (1,))}
            if out.features is not out.logprob:
                early["features"] = HostBuffer(self.ctx, out.features.shape)
        self.ctx.call("tn_d2h_early", early["logprob"].ptr, out.logprob.ptr, out.logprob.nbytes)
        if out.features is not out.logprob:
            self.ctx.call("tn_d2h_early", early["features"].ptr, out.features.ptr, out.features.nbytes)
        if with_cost:
            self.ctx.call("tn_d2h_early", early["cost"].ptr, self.d_cost.ptr, 4)
        early["cost_sent"] = with_cost
        early["live"] = True

    def _train_step(self, y, y_row0, d_row0=None, pipe_stride=0):
        """forward + backward + all-reduce + update for the minibatch the input slot
        currently points at.  Everything is enqueued; nothing is read back."""
        ctx = self.ctx
        self._apply_dtype()
        out = self.tr_layers[-1]
        first = self.tr_layers[0]
        self.dp.begin_step(pipe_stride)
        self._c8_tiles.arrange(self.tr_layers, self._need_gin)
        for lyr in self.tr_layers[:-1]:
            lyr.forward(True)
        # the weight-gradient ops only record their finishing slab sums; one launch does them all
        ctx.call("tn_defer_reductions", 1)
        n_lyr = len(self.tr_layers)
        fuse_out = self._softmax_train and n_lyr >= 2 and self._need_gin[n_lyr - 1] \
            and isinstance(out, SoftmaxLayer) and out.loss == "nll"
        ctx.fc_head(True)
        try:
            out.forward(True, y=y, y_row0=y_row0, d_row0=d_row0,
                        below=self.tr_layers[-2] if fuse_out else None)
        except Exception:
            ctx.call("tn_defer_reductions", 0)
            raise
        finally:
            ctx.fc_head(False)
        # Where the step's cost (-mean logprob[n, y_n], this rank's share of the global mean) is summed -- one of:
        whole = self._cost_net          # here, weight costs included, in one launch: nothing is parked, nothing pending
        leaf = not self._cost_rider and not whole   # here: it travels through the all-reduce, or the generic schedule
        rides = self._cost_rider and not pipe_stride    # in the update launch at the end of the step
        # two steps in flight: it, and the finishing slab sums, wait for the update launch that opens this stream's next step
        parks = (self._cost_rider or whole) and bool(pipe_stride)
        # ... and when the caller reads it, ALSO now: the update's cost block on its own (same order, same bits)
        sent = self._cost_rider and self._want_outputs
        if sent:
            self._sum_cost()
        if whole:
            self._guard_cost()
            tab = self._wc_tab
            ctx.call("tn_wtcost_net", tab.ctypes.data, len(tab), out.rowloss.ptr, self.local_bsz, 1.0 / self.batch_sz,
                     self.d_cost.ptr, 0)
        if self._want_outputs:
            self._send_outputs(out, sent or whole)
        if self._cost_rider and (sent or parks):
            self._cost_pending = not sent
        if leaf:
            self._guard_cost()
            ctx.call("tn_reduce_sum", out.rowloss.ptr, self.local_bsz, 1.0 / self.batch_sz, self.d_cost.ptr, 0)
        g = out.dlogits
        # The elastic field of the NEXT minibatch only depends on the step counter.  It is left with
        # the context as a rides (offset +1: the counter advances at the end of the step) and
        # travels as extra blocks of the backward pass's paired GEMM launch; nets without such a
        # launch build it beside the update instead (tn_step_tail).
        ahead = (isinstance(first, ElasticLayer) and first.active and first.has_field and
                 not first._inj_draws and first.d_step is not None and (self._n_segs or rides) and
                 self.fused_step)
        if ahead:
            nxt = 1 - first._cur
            m = first._maps[nxt]
            hw = first.img_sz
            field_args = (hw, hw, float(first.translation), float(first.zoom), float(first.magnitude),
                          int(first.sigma), float(first.angle), int(first.nearest), m[0].ptr, m[1].ptr,
                          m[2].ptr, m[3].ptr)
            ctx.call("tn_rider_elastic_field", first.draws.ptr, first.seed, pipe_stride or 1,
                     self.d_step.ptr, *field_args)
        tail = False
        # single-GPU steps leave the finishing slab sums to the update launch (tn_sgd_update_net, TN_UPD_LAZY)
        lazy = False
        try:
            for idx in range(len(self.tr_layers) - 1, -1, -1):
                lyr = self.tr_layers[idx]
                below = self.tr_layers[idx - 1] if idx > 0 else None
                if lyr is out:
                    ctx.fc_head(True)
                    try:
                        g = lyr.backward(g, self._need_gin[idx], below)
                    finally:
                        ctx.fc_head(False)
                else:
                    g = lyr.backward(g, self._need_gin[idx], below)
                if self._dp and g is not None:
                    self.dp.after_backward(idx, pipe_stride)
                if g is None:
                    break
            lazy = self.fused_step and not self._dp and 0 < self._n_segs <= 32
        finally:
            waiting = bool(ctx.lib.tn_rider_pending(ctx.h))
            if waiting:
                ctx.call("tn_rider_cancel")       # nobody carried it: it joins the update launch
            rode = ahead and not waiting
            tail = ahead and not rode
            if pipe_stride:                       # pipelined schedule: the update is not part of the step
                ahead, tail, lazy = rode, False, False
            lazy = lazy and not tail
            if tail:
                ctx.call("tn_defer_flush_step", self.d_step.ptr)      # the counter advances here
            elif not lazy and not parks:
                ctx.call("tn_defer_reductions", 0)
        if pipe_stride:
            self.dp.end_pipelined()               # two steps in flight: this stream's next step starts with the update
            if ahead:
                first._cur, first._pre_valid = nxt, True
            self._c8_tiles.stale()
            return
        delayed = self.dp.end_sequential(tail)    # the all-reduce (the delayed schedule: with its update)
        if whole:
            pass
        elif self.fused_step and self._has_wtcost:
            # data-parallel: the row losses have travelled through the all-reduce; every rank adds the weight costs
            tab = self._wc_tab
            ctx.call("tn_wtcost_net", tab.ctypes.data, len(tab), None, 0, 0.0, self.d_cost.ptr, 1)
        else:
            for lyr in self.tr_layers:
                lyr.get_wtcost(self.d_cost)
        if rides:
            self._guard_cost()
        cost_args = (out.rowloss.ptr if rides else None, self.local_bsz, 1.0 / self.batch_sz, self.d_cost.ptr if rides else None)
        mn_done = False
        if delayed:
            pass
        elif tail:
            ctx.call("tn_step_tail", self._d_segs.ptr if self._n_segs else None, self._n_segs,
                     self._max_seg, self.cur_learn_rate.ptr, 1.0, *cost_args, first.draws.ptr, first.seed, self.d_step.ptr,
                     *field_args)
        elif lazy:
            self._update_and_maxnorm(_lib.TN_UPD_LAZY, self._d_segs.ptr, self._h_segs.ctypes.data, self._n_segs,
                                     self._max_seg, self.cur_learn_rate.ptr, 1.0, self.d_step.ptr, 1, 0, *cost_args)
            mn_done = True
        elif self._n_segs or rides:               # also advances the RNG step counter
            ctx.call("tn_sgd_update_net", _lib.TN_UPD_PLAIN, self._d_segs.ptr if self._n_segs else None, None,
                     self._n_segs, self._max_seg, self.cur_learn_rate.ptr, 1.0, self.d_step.ptr, 1, 0, *cost_args)
        else:
            ctx.call("tn_add_u32", self.d_step.ptr, 1)
        if ahead:
            first._cur, first._pre_valid = nxt, True
        if not mn_done:
            self._apply_maxnorm_all()
        self._avg_update()
        self._c8_tiles.stale()

    def _update_and_maxnorm(self, *args):
        """Layer.get_updates of every tensor (layer.py:70-107) as ONE call: tn_sgd_update_net + the max-norm projection,
        the column sums of the dense matrices left by the update launch itself (tn_sgd_update_net_maxnorm)."""
        tab = self._maxnorm_table()
        if 0 < len(tab) <= 32 and os.environ.get("TN_MN_FUSED", "1") != "0":
            self.ctx.call("tn_sgd_update_net_maxnorm", *args, tab.ctypes.data, len(tab))
        else:
            self.ctx.call("tn_sgd_update_net", *args)
            self._apply_maxnorm_all()

    def _guard_cost(self):
        """In front of a launch that writes ``d_cost``: a step_cost() loop may still owe the host the previous value (a
        4-byte copy on the copy stream, _CostLedger.issue) -- the stream waits for that copy's event."""
        if self._cost_guard_ev is not None:
            self.ctx.call("tn_event_wait", self._cost_guard_ev)
            self._cost_guard_ev = None

    def _sum_cost(self):
        """The last step's cost into ``d_cost``, on the stream currently selected: the update launch's cost block on its own."""
        self._guard_cost()
        self.ctx.call("tn_sgd_update_net", _lib.TN_UPD_PLAIN, None, None, 0, 0, self.cur_learn_rate.ptr, 1.0, None, 0, 0,
                      self.tr_layers[-1].rowloss.ptr, self.local_bsz, 1.0 / self.batch_sz, self.d_cost.ptr)

    def _injecting(self):
        """A parity test has injected random draws somewhere (dropout masks, elastic / color draws)."""
        for lyr in self.tr_layers:
            drop = getattr(lyr, "drop", None)
            if (drop is not None and drop.injected) or getattr(lyr, "_inj_draws", False) or \
                    getattr(lyr, "_inj", None) is not None or getattr(lyr, "_inj_flip", None) is not None:
                return True
        return False

    def _apply_maxnorm_all(self):
        """layer.py:88-103 for every parameter of the net in ONE call (tn_maxnorm_multi: the biases and conv kernels
        share a launch; Layer.apply_maxnorm is the per-layer form of the same projection)."""
        tab = self._maxnorm_table()
        for i in range(0, len(tab), 32):
            chunk = tab[i:i + 32]
            self.ctx.call("tn_maxnorm_multi", chunk.ctypes.data, len(chunk))

    def _wtcost_table(self):
        """tn_wtcost_net's table (tn_wc_seg rows): every parameter tensor of every layer with a non-zero L1 or L2, frozen
        layers included (Layer.get_wtcost adds their cost too, layer.py:109-117).  Kept alive: recorded steps bake its address."""
        tab = self._wc_tab
        if tab is None:
            rows = []
            for lyr in self.tr_layers:
                reg = getattr(lyr, "reg", None)
                if reg and lyr.params and (reg['L1'] or reg['L2']):
                    rows.extend((p.ptr, p.size, float(reg['L1']), float(reg['L2'])) for p in lyr.params)
            dt = np.dtype([('p', 'u8'), ('n', 'u8'), ('L1', 'f4'), ('L2', 'f4')])
            assert dt.itemsize == 24          # tn_wc_seg
            tab = self._wc_tab = np.array(rows, dtype=dt) if rows else np.zeros((0,), dt)
        return tab

    def _maxnorm_table(self):
        tab = self._mn_tab
        if tab is None:
            rows = []
            for lyr in self.tr_layers:
                if not lyr.has_updates() or not lyr.reg['maxnorm']:
                    continue
                for p in lyr.params:
                    if p.ndim in (1, 2, 4):
                        rows.append((p.ptr, p.ndim, p.shape[0],
                                     1 if p.ndim == 1 else int(np.prod(p.shape[1:])), float(lyr.reg['maxnorm'])))
            dt = np.dtype([('p', 'u8'), ('ndim', 'i4'), ('d0', 'i4'), ('rest', 'i4'), ('mx', 'f4')])
            assert dt.itemsize == 24          # tn_mn_seg
            tab = self._mn_tab = np.array(rows, dtype=dt) if rows else np.zeros((0,), dt)
        return tab

    # ------------------------------------------------------------------------------
    def _check_images(self, x_data, y_data=None):
        """The dataset must have the image shape the net was built for (Theano reports the mismatch when the compiled
        function first runs; here the kernels index the dataset with the net's shape, so it is checked up front) and at
        least one minibatch."""
        first = self.tr_layers[0]
        want = (first.num_maps, first.out_sz, first.out_sz)
        shape = tuple(x_data.shape)
        assert len(shape) == 4 and shape[1:] == want, \
            "image data of shape {} for a net built for (N, {}, {}, {}) images".format(shape, *want)
        assert shape[0] >= self.batch_sz, "{} images for minibatches of {}".format(shape[0], self.batch_sz)
        if y_data is not None:
            assert y_data.shape[0] == shape[0], "{} labels for {} images".format(y_data.shape[0], shape[0])
            # labels index the rows of logprob / the class centres (outlayers.py:50-51: logprob[arange, y] -- an IndexError
            # in the reference)
            last = self.tr_layers[-1]
            n_cls = last.centers.shape[0] if getattr(last, "centers", None) is not None else last.n_out
            yv = y_data.get_value() if hasattr(y_data, "get_value") else np.asarray(y_data)
            if yv.size and (int(yv.min()) < 0 or int(yv.max()) >= n_cls):
                raise IndexError("labels in [{}, {}] for an output layer of {} classes".format(
                    int(yv.min()), int(yv.max()), n_cls))

    def get_trin_model(self, x_data, y_data, aux_data=None,
                       take_index_list=False):
        print('Compiling training function...')
        self.tr_layers[-1].cost(None)            # validates the loss name (outlayers.py:12-36)
        self._check_images(x_data, y_data)
        if hasattr(self, 'aux_inpt_tr'):
            assert aux_data is not None, "Auxillary data not supplied"        # neuralnet.py:216-217
            aux_data = share(aux_data)
        else:
            aux_data = None
        self._prepare_training()
        if self._pipe_fn is not None:
            self._pipe_fn._fall_back()           # an earlier training function: bring the net up to date
        if aux_data is None and self._pipe_ok(take_index_list):
            return _PipeTrainFn(self, share(x_data), share(y_data, np.int32))
        return _TrainFn(self, share(x_data), share(y_data, np.int32), take_index_list, aux_data)

    def _sync_weights(self):
        """With two steps in flight (_PipeTrainFn) the net's own weight buffers lag behind: catch up."""
        if self._avg_swapped:
            return      # up to date since _at_avg_wts began -- and the twin's copy of the weights must not land on the averages
        if self._pipe_fn is not None:
            self._pipe_fn.sync_weights()

    def _pipe_ok(self, take_index_list):
        """Two-steps-in-flight schedule (_PipeTrainFn): single GPU, plain momentum-SGD nets."""
        if self._is_twin or not self.fused_step or os.environ.get("TN_PIPELINE", "1") == "0":
            return False
        if self._dp and os.environ.get("TN_DP_PIPELINE", "1") == "0":
            return False
        if self._has_wtcost and not self._cost_net:
            return False        # data-parallel steps add the weight costs behind the all-reduce, at the end of the step
        return not take_index_list and self._n_segs > 0 and not self._injecting()

    def reset_accumulated_gradients(self):
        self._prepare_training()
        if self._pipe_fn is not None:
            self._pipe_fn._fall_back()           # steps in flight: apply their gradients first
        # (a reduced gradient the delayed schedule has still to fold into the velocity: the reference zeroes it too)
        self.dp.drop_pending()
        for lyr in self.tr_layers:
            for au in (lyr.accumulated_updates or ()):
                au.fill_bytes(0)

    def get_test_model(self, x_data, y_data, aux_data=None, preds_feats=False, averaged=None):
        """``averaged``: evaluate at the averaged weights (WT_AVG) -- None: iff the net keeps them; False: at the last
        iterate; True without WT_AVG is an assertion."""
        print('Compiling testing function... ')
        self._check_images(x_data, y_data)
        if hasattr(self, 'aux_inpt_te'):
            assert aux_data is not None, "Auxillary data not supplied"        # neuralnet.py:266-267
            aux_data = share(aux_data)
        else:
            aux_data = None
        return _TestFn(self, share(x_data), share(y_data, np.int32), preds_feats, aux_data, self._averaged(averaged))

    def takes_aux(self):
        return hasattr(self, 'aux_inpt_te')

    def get_data_test_model(self, get_output_of_layers=(), averaged=None):
        print('Compiling full test function...')
        averaged = self._averaged(averaged)       # (as in get_test_model)
        if self.tr_prms['BATCH_SZ'] != 1:
            print("\n****WARNING****: BATCH SIZE IS NOT 1. "
                  "WILL BE EXPECTING A BATCH OF INPUT IMAGES AT A TIME.\n")
        first = self.te_layers[0]
        stage = self.ctx.empty((self.local_bsz, first.num_maps, first.out_sz, first.out_sz))

        for index in get_output_of_layers:          # a requested conv map must be materialised
            lyr = self.te_layers[index]
            if isinstance(lyr, ConvLayer) and lyr.fused_pool is not None:
                lyr.unfuse()

        def fn(x, aux=None):
            with self._at_avg_wts(averaged):
                return run(x, aux)

        def run(x, aux):
            self._sync_weights()
            self._apply_dtype()
            self._c8_tiles.arrange(self.te_layers)
            x = np.ascontiguousarray(x, np.float32).reshape(stage.shape)
            stage.set_value(x)
            if self.takes_aux():                           # neuralnet.py:289-290
                assert aux is not None, "Auxillary data not supplied"
                self.aux_inpt_te.bind(share(np.ascontiguousarray(aux, np.float32)))
                self.aux_inpt_te.row0 = 0
            slot = self.test_x
            slot.bind(stage)
            slot.row0 = slot.row_global0 = 0
            for lyr in self.te_layers[:-1]:
                lyr.forward(False)
            out = self.te_layers[-1]
            self.ctx.fc_head(True)
            try:
                out.forward(False)
            finally:
                self.ctx.fc_head(False)
            res = [out.features.get_value(), out.y_preds.get_value().astype(np.int64)]
            for index in get_output_of_layers:
                res.append(self.te_layers[index].output.get_value())
            return res

        return fn

    def get_init_params(self, with_opt_state=None):
        """neuralnet.py:298-301: {"layers", "training_params", "allwts"} -- what the reference pickles.  With
        ``with_opt_state`` (default: training param SAVE_OPT_STATE, off) one more key, "opt_state": the velocities
        (layer.py:77-79; the reference drops them, so a resumed run restarts its momentum), the RNG step counter and the
        seeds of the dropout / distortion streams; ``load_opt_state`` puts them back.  Readers of the reference's pickles ignore
        the extra key."""
        out = {"layers": self.layers,
               "training_params": self.tr_prms,
               "allwts": [l.get_wts() for l in self.tr_layers]}
        if self._avg is not None:                 # WT_AVG: the averaged weights beside the raw ones (load_avg_wts)
            out["avg_wts"] = self.get_avg_wts()
        if with_opt_state is None:
            with_opt_state = bool(self.tr_prms.get('SAVE_OPT_STATE', False))
        if with_opt_state:
            out["opt_state"] = self._opt_state()
        return out

    def get_avg_wts(self):
        """The averaged weights (WT_AVG) in the nesting of ``[l.get_wts() for l in tr_layers]``; a tensor that is never
        updated has no average and comes as it is.  None when averaging is off."""
        if self._avg is None:
            return None
        self._sync_weights()                      # two steps in flight: the last p_t enters the averages first
        out = []
        for lyr, avs in zip(self.tr_layers, self._avg):
            wts = lyr.get_wts()
            for j, a in enumerate(avs or ()):
                wts[j] = a.get_value()
            out.append(wts)
        return out

    def load_avg_wts(self, lst):
        """Averaged weights saved by get_avg_wts / get_init_params()["avg_wts"]: training carries the averages on from them."""
        assert self._avg is not None, "load_avg_wts: this net keeps no averaged weights (WT_AVG is off)"
        assert len(lst) == len(self.tr_layers), "load_avg_wts: {} layers for a net of {}".format(len(lst), len(self.tr_layers))
        self._sync_weights()
        for avs, wts in zip(self._avg, lst):
            for a, w in zip(avs or (), wts):
                w = np.asarray(w, np.float32)
                assert w.shape == a.shape, "load_avg_wts: a tensor of shape {} for one of {}".format(w.shape, a.shape)
                a.set_value(w)

    def _opt_state(self):
        self._prepare_training()
        fn = self._pipe_fn
        pend, step = None, int(self.d_step.get_value()[0])
        if fn is not None and fn._seq is None and fn._twin is not None and fn.t > 0:
            # two steps in flight: the velocity on the device is one gradient behind (that of step t-1, still with the
            # stream that ran it, and folded in by that stream's next update): fold it in on the host, same expression
            # as the kernels (common.h tn_vel: fma(m, v, rn((1-m) g))).  A net with weight costs has folded it in on
            # the device when its weights were brought up to date (_PipeTrainFn.sync_weights): nothing is pending.
            fn._flush_parked()
            if self._has_wtcost:
                fn.sync_weights()
            self.ctx.sync()
            X = fn.nets[(fn.t - 1) & 1]
            step = fn._base + fn.t
            if not fn._v_done[(fn.t - 1) & 1]:
                pend = lambda i, j: X.tr_layers[i].grads[j].get_value()
        elif self.dp.pending_grads() is not None:
            # delayed all-reduce (TN_DP_OVERLAP=2): the same situation, the last reduced gradient travels on the second stream
            self.ctx.sync()
            prev = self.dp.pending_grads()
            pend = lambda i, j: prev[id(self.tr_layers[i])][j].get_value()
        vel = []
        for i, lyr in enumerate(self.tr_layers):
            row = []
            for j, v in enumerate(lyr.accumulated_updates or ()):
                a = v.get_value()
                if pend is not None and lyr.has_updates():
                    a = _fma32(np.float32(lyr.reg['momentum']), a, (np.float32(1) - np.float32(lyr.reg['momentum'])) * pend(i, j))
                row.append(a)
            vel.append(row)
        seeds = [(getattr(l, "seed", None), l.drop.seed if getattr(l, "drop", None) is not None else None)
                 for l in self.tr_layers]
        return {"velocities": vel, "rng_step": step, "stream_seeds": seeds}

    def load_opt_state(self, state):
        """Velocities and RNG step counter saved by get_init_params(with_opt_state=True); call before training."""
        self._prepare_training()
        if self._pipe_fn is not None:
            self._pipe_fn._fall_back()
        for lyr, row in zip(self.tr_layers, state["velocities"]):
            for v, a in zip(lyr.accumulated_updates or (), row):
                v.set_value(np.asarray(a, np.float32))
        self.ctx.call("tn_set_u32", self.d_step.ptr, int(state["rng_step"]))
        # a net rebuilt from weights draws fresh stream seeds (neuralnet.py:63-68: no SEED chain): put the run's back
        for lyr, (seed, dseed) in zip(self.tr_layers, state.get("stream_seeds", ())):
            if seed is not None and hasattr(lyr, "seed"):
                lyr.seed = seed
            if dseed is not None and getattr(lyr, "drop", None) is not None:
                lyr.drop.seed = dseed

    def set_rate(self):
        self.cur_learn_rate.set_value(np.float32(
            self.tr_prms['INIT_LEARNING_RATE'] /
            (1 + self.tr_prms['CUR_EPOCH'] /
             self.tr_prms['EPOCHS_TO_HALF_RATE'])))

    def inc_epoch_set_rate(self):
        self.tr_prms['CUR_EPOCH'] += 1
        self.set_rate()

    def get_epoch(self):
        return self.tr_prms['CUR_EPOCH']

    def __str__(self):
        prmstr = '; '.join([', '.join([getattr(prm, "name", "param") for prm in lyr.params])
                            for lyr in self.tr_layers])
        return \
            '\nTrain Layers\n\t' + \
            '\n\t'.join([str(l) for l in self.tr_layers]) + \
            '\nTest Layers\n\t' + \
            '\n\t'.join([str(l) for l in self.te_layers]) + \
            '\nParams ' + prmstr

    def get_layers_info(self):
        return get_layers_info(self.layers)

    def get_wts_info(self, detailed=False):
        return get_wts_info((l.get_wts() for l in self.tr_layers), detailed)

    def get_training_params_info(self):
        return get_training_params_info(self.tr_prms)
