"""What the layers of the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16': device.C8Array tensors, the tn_c8_*
kernels) share on the host: the stack's grammar, the two conv families, the detour of a padded tensor through a dense
copy, and the table of the conv weights arranged as MFMA operand tiles."""
from collections import namedtuple

import numpy as np

from ..device import C8Array


def pool_stands_alone(pool_sz, fused=True):
    """Which of its two forms a PoolLayer on the stack takes: a 2x2 one is the second half of the fused conv + pool block
    of the ConvLayer below it while the net fuses (``fused``: NeuralNet.fuse_conv_pool); every other one -- and every one
    of a net that does not fuse -- stands alone (tn_c8_pool_fwd / tn_c8_pool_bwd)."""
    return not (fused and pool_sz == 2)


def check_follows(dtype, below, kind, pool_sz=None, fused=True):
    """The stack's grammar, asserted before a layer of class ``kind`` (its name) is built on the stack tensor that layer
    ``below`` puts out: Conv / Pool / Mean / DropOut layers pass stack tensors on (a MeanLayer closes the stack with an
    fp32 (N, C) output), a HiddenLayer consumes one.  A fused PoolLayer (pool_stands_alone) exists only inside the block
    of the ConvLayer directly below it, 2x2 on even maps; a stand-alone one follows any layer that puts out a stack tensor
    (its geometry is the constructor's to refuse: tn_c8_pool_supported)."""
    below_kind = type(below).__name__
    if kind == "PoolLayer" and pool_stands_alone(pool_sz, fused):
        assert below_kind in ("ConvLayer", "PoolLayer", "DropOutLayer"), \
            "DTYPE {}: a stand-alone PoolLayer follows a Conv, Pool or DropOut layer (got {})".format(dtype, below_kind)
        return
    if kind in ("ElasticLayer", "ColorLayer"):
        raise AssertionError("DTYPE {}: only Conv / Pool / Mean / DropOut layers take the conv stack's 16-bit-resident "
                             "tensors (got {})".format(dtype, kind))
    if kind in ("AuxConcatLayer", "SoftmaxLayer", "SoftAuxLayer", "HingeLayer", "ExpLossLayer"):
        raise AssertionError("DTYPE {}: a HiddenLayer must follow the conv stack (got {})".format(dtype, kind))
    if kind == "PoolLayer":
        assert below_kind != "DropOutLayer", \
            "DTYPE {}: a DropOutLayer between a ConvLayer and its PoolLayer breaks the fused conv + pool block " \
            "of the 16-bit stack; put the DropOutLayer after the PoolLayer".format(dtype)
        assert fused and below_kind == "ConvLayer", "DTYPE {}: a PoolLayer must directly follow a ConvLayer".format(dtype)
        assert pool_sz == 2 and below.out_sz % 2 == 0, "DTYPE {}: pooling layers are 2x2 on even maps".format(dtype)


# The stack's two conv shapes differ in their ops, one entry of the geometry the ops take, whether fwd / dgrad take the
# weights as arranged operand tiles (a trailing pointer; OperandTiles) and whether a product leaves the pad cells of a
# padded output to be zeroed afterwards (tn_c8_pad_zero).
ConvFamily = namedtuple("ConvFamily", "fwd wgrad dgrad geom tiles pad_zero")


def conv_family(one_by_one, n, c, side, pitch, k):
    """3x3 stride-1 'same' (conv_c8.hip: runs on the pitch x pitch shape) or 1x1 stride-1 (conv1_c8.hip: rounds its
    operand tiles per call, writes its output's pad cells itself)."""
    if one_by_one:
        return ConvFamily("tn_c8_conv1_fwd", "tn_c8_conv1_wgrad", "tn_c8_conv1_dgrad", (n, c, side, pitch, k), False, False)
    return ConvFamily("tn_c8_conv_fwd", "tn_c8_conv_wgrad", "tn_c8_conv_dgrad", (n, c, pitch, pitch, k), True, True)


class DenseDetour:
    """In front of an op that reads dense maps (tn_c8_mean_*, the dense products tn_c8_fc_* / tn_c8_fcg_*): a stack
    tensor ``src`` whose maps are stored at a pitch above their side is cropped to a dense copy first (``crop``), and
    the gradient the op writes (into ``dense_gin()``) is put back into the padded layout (``embed``).  A dense ``src``
    passes through untouched.  The copy is allocated here, the gradient buffers by the first backward."""

    def __init__(self, src):
        self.src, self.call = src, src.ctx.call
        self.dense = C8Array.dense_like(src) if src.padded else src
        self.gin = self.gin_padded = None
        self._geom = (src.shape[0], src.c8[0], src.c8[1], src.pitch)

    def crop(self):
        if self.src.padded:
            self.call("tn_c8_crop", self.src.ptr, self.dense.ptr, *self._geom)
        return self.dense

    def act_ptr(self, ptr):
        """``ptr``: the output act' is taken from (layer.below_info) -- ``src``'s own: its cropped copy (same values)."""
        assert ptr is None or ptr == self.src.ptr
        return ptr and self.dense.ptr

    def dense_gin(self):
        if self.gin is None:
            self.gin = C8Array.dense_like(self.src)
            self.gin_padded = C8Array.like(self.src) if self.src.padded else self.gin
        return self.gin

    def embed(self):
        if self.src.padded:
            self.call("tn_c8_embed", self.gin.ptr, self.gin_padded.ptr, *self._geom)
        return self.gin_padded


class OperandTiles:
    """The 3x3 conv weights of a net's stack as 16-bit MFMA operand tiles: every product of a pass arranged in ONE
    launch per 32 (tn_c8_arrange_multi) at the start of the pass, valid until the next update (``stale``).  One table
    per graph (training / test), built when the graph first runs."""
    _SEG = np.dtype([('W', 'u8'), ('wt', 'u8'), ('K', 'i4'), ('C', 'i4'), ('dgrad', 'i4'), ('pad', 'i4')])
    assert _SEG.itemsize == 32          # tn_c8_wt_seg

    def __init__(self, ctx):
        self.ctx, self._tabs = ctx, {}

    def arrange(self, lyrs, need_gin=None):
        """``need_gin`` (training graph): which layers propagate a gradient and so need the dgrad arrangement too."""
        tab = self._tabs.get(need_gin is not None)
        if tab is None:
            rows, convs = [], []
            for idx, lyr in enumerate(lyrs):
                fam = getattr(lyr, "c8_fam", None)
                if fam is None or not fam.tiles:           # (K, C, 3, 3) weights only
                    continue
                convs.append(lyr)
                rows.append((lyr.W.ptr, lyr.wt_fwd.ptr, lyr.num_maps, lyr.num_prev_maps, 0, 0))
                if need_gin is not None and need_gin[idx]:
                    if lyr.wt_bwd is None:
                        n = self.ctx.lib.tn_c8_wt_elems(lyr.num_maps, lyr.num_prev_maps, 1)
                        lyr.wt_bwd = self.ctx.empty((n,), np.uint16)
                    rows.append((lyr.W.ptr, lyr.wt_bwd.ptr, lyr.num_maps, lyr.num_prev_maps, 1, 0))
            tab = self._tabs[need_gin is not None] = (np.array(rows, dtype=self._SEG), convs)
        segs, convs = tab
        for i in range(0, len(segs), 32):
            chunk = segs[i:i + 32]
            self.ctx.call("tn_c8_arrange_multi", chunk.ctypes.data, len(chunk))
        for lyr in convs:
            lyr.wt_valid = True

    def stale(self):
        """The weights are about to change: the arranged tiles of both graphs are no longer theirs."""
        for _, convs in self._tabs.values():
            for lyr in convs:
                lyr.wt_valid = False
