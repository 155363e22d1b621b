"""What the layers of the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16': device.C8Array tensors, the tn_c8_*
kernels) share on the host: the stack's grammar, the conv families, the detour of a padded tensor through a dense
copy, and the table of the conv weights arranged as MFMA operand tiles."""
from collections import namedtuple

import numpy as np

from ..device import C8Array, c8_pitch, c8_pool_pitch


def pool_stands_alone(pool_sz, fused=True, below=None, any_shapes=False, stride=None):
    """Which of its two forms a PoolLayer on the stack takes: a 2x2 one is the second half of the fused conv + pool block
    of the ConvLayer below it while the net fuses (``fused``: NeuralNet.fuse_conv_pool); every other one -- and every one
    of a net that does not fuse -- stands alone (tn_c8_pool_fwd / tn_c8_pool_bwd).  ``any_shapes`` (the net's
    CONV_SHAPES 'any') with the layer ``below``: a 2x2 one stands alone too where the block cannot take it -- above a
    ConvLayer of the general family (ConvFamily.pools false: never fused) and on an odd map.  A pool whose ``stride``
    differs from its window (None: the window) always stands alone (tn_c8_pool_st_fwd / tn_c8_pool_st_bwd)."""
    if stride is not None and stride != pool_sz:
        return True
    if not (fused and pool_sz == 2):
        return True
    if any_shapes and type(below).__name__ == "ConvLayer":
        fam = getattr(below, "c8_fam", None)
        return (fam is not None and not fam.pools) or below.out_sz % 2 != 0
    return False


# the output heads that can close the stack (STACK_HEAD 'any'): each is a HiddenLayer -- which consumes stack tensors --
# plus a row kernel on its fp32 output.  (AuxConcatLayer is not one: it concatenates fp32 features.)
STACK_HEADS = ("SoftmaxLayer", "SoftAuxLayer", "HingeLayer", "ExpLossLayer", "CenteredOutLayer")
HEAD_HINT = "training param STACK_HEAD: 'any' lets an output head close the stack"


def check_follows(dtype, below, kind, pool_sz=None, fused=True, any_shapes=False, stack_head=False, stride=None):
    """The stack's grammar, asserted before a layer of class ``kind`` (its name) is built on the stack tensor that layer
    ``below`` puts out: Conv / Pool / Mean / DropOut layers pass stack tensors on (a MeanLayer closes the stack with an
    fp32 (N, C) output), a HiddenLayer consumes one -- and so does, with ``stack_head`` (the net's STACK_HEAD 'any'), an
    output head (STACK_HEADS).  A fused PoolLayer (pool_stands_alone) exists only inside the block
    of the ConvLayer directly below it, 2x2 on even maps; a stand-alone one follows any layer that puts out a stack tensor
    (its geometry is the constructor's to refuse: tn_c8_pool_supported / tn_c8_pool_st_supported).  ``stride``: the
    PoolLayer's, None for its window."""
    below_kind = type(below).__name__
    if kind == "PoolLayer" and pool_stands_alone(pool_sz, fused, below, any_shapes, stride=stride):
        assert below_kind in ("ConvLayer", "PoolLayer", "DropOutLayer"), \
            "DTYPE {}: a stand-alone PoolLayer follows a Conv, Pool or DropOut layer (got {})".format(dtype, below_kind)
        return
    if kind in ("ElasticLayer", "ColorLayer"):
        raise AssertionError("DTYPE {}: only Conv / Pool / Mean / DropOut layers take the conv stack's 16-bit-resident "
                             "tensors (got {})".format(dtype, kind))
    if stack_head and kind in STACK_HEADS:
        return
    if kind == "AuxConcatLayer" or kind in STACK_HEADS:
        raise AssertionError("DTYPE {}: a HiddenLayer must follow the conv stack (got {}){}".format(
            dtype, kind, "; " + HEAD_HINT if kind in STACK_HEADS else ""))
    if kind == "PoolLayer":
        assert below_kind != "DropOutLayer", \
            "DTYPE {}: a DropOutLayer between a ConvLayer and its PoolLayer breaks the fused conv + pool block " \
            "of the 16-bit stack; put the DropOutLayer after the PoolLayer".format(dtype)
        assert fused and below_kind == "ConvLayer", "DTYPE {}: a PoolLayer must directly follow a ConvLayer".format(dtype)
        assert pool_sz == 2 and below.out_sz % 2 == 0, "DTYPE {}: pooling layers are 2x2 on even maps".format(dtype)


# The stack's conv families differ in their ops, the geometry the ops take, whether fwd / dgrad take the weights as
# arranged operand tiles (a trailing pointer; OperandTiles), whether a product leaves the pad cells of a padded output
# to be zeroed afterwards (tn_c8_pad_zero) and whether the ops can pool: take the arguments of a fused conv + 2x2 pool
# block (forward: the mask to write and the pool flag; gradients: the pooled flag and the mask) -- a family that cannot
# is never fused (pool_stands_alone).
ConvFamily = namedtuple("ConvFamily", "fwd wgrad dgrad geom tiles pad_zero pools")


def conv_family(one_by_one, n, c, side, pitch, k, general=None):
    """3x3 stride-1 'same' (conv_c8.hip: runs on the pitch x pitch shape), 1x1 stride-1 (conv1_c8.hip: rounds its
    operand tiles per call, writes its output's pad cells itself) or -- ``general``: (filter, stride, low padding, output
    side, output pitch) -- any shape (convg_c8.hip: like the 1x1 family, an output pitch of its own, no pooling)."""
    if general is not None:
        return ConvFamily("tn_c8_convg_fwd", "tn_c8_convg_wgrad", "tn_c8_convg_dgrad", (n, c, side, pitch, k) + tuple(general),
                          False, False, False)
    if one_by_one:
        return ConvFamily("tn_c8_conv1_fwd", "tn_c8_conv1_wgrad", "tn_c8_conv1_dgrad", (n, c, side, pitch, k), False, False,
                          True)
    return ConvFamily("tn_c8_conv_fwd", "tn_c8_conv_wgrad", "tn_c8_conv_dgrad", (n, c, pitch, pitch, k), True, True, True)


def choose_conv(lib, dtype, conv_shapes, n, c, side, in_pitch, k, f, stride, mode, pad_lo, out_side):
    """The family that runs a ConvLayer of the stack and the pitches of its maps: (ConvFamily, 1x1 family?, input pitch,
    output pitch), from the library's capability queries alone (no device).  Maps of S pixels a side are stored at a pitch
    P: the input's (``in_pitch``), or -- first conv layer, None -- the smallest power of two >= max(S, 8); the tiled
    kernels run on the P x P shape, S < P pads every plane with zero rows and columns (device.C8Array), which the 'same'
    products read as their padding, and their output keeps the pitch.  Two tiled shapes run on the stack: 3x3 stride-1
    'same' (conv_c8.hip) and 1x1 stride-1 (conv1_c8.hip: 'valid' and 'same' are the same layer, any number of filters).
    ``conv_shapes`` (the net's CONV_SHAPES) 'any': a shape those two refuse takes the general family (convg_c8.hip: any
    filter, mode and stride).  Its input pitch is the input's own or -- first conv layer -- c8_pool_pitch(S): a power of
    two up to 64 pixels (tn_c8_pack_pitch), dense above (tn_c8_pack); its output pitch is c8_pool_pitch(out_side), so
    that any layer of the stack can follow."""
    P = in_pitch if in_pitch is not None else c8_pitch(side)
    one_by_one = f == 1 and stride == 1 and mode in ('valid', 'same')
    if one_by_one:
        ok = bool(lib.tn_c8_conv1_supported(n, c, side, P, k))
    else:
        ok = bool((side == P or side <= 64) and P >= 8 and mode == 'same' and
                  lib.tn_c8_conv_supported(n, c, P, P, k, f, stride, pad_lo) and lib.tn_c8_conv_wgrad_supported(n, c, P, P, k))
    if not ok and conv_shapes == 'any':
        P = in_pitch if in_pitch is not None else c8_pool_pitch(side)
        Po = c8_pool_pitch(out_side)
        general = (f, stride, pad_lo, out_side, Po)
        assert lib.tn_c8_convg_supported(n, c, side, P, k, *general), (
            "DTYPE {} with CONV_SHAPES 'any' takes conv layers whose tensors have fewer than 2^32 cells and whose weights "
            "fewer than 2^28 elements (got {}->{} maps, {}x{} at pitch {}, {} filter {} stride {}: {}x{} at pitch {})".format(
                dtype, c, k, side, side, P, mode, f, stride, out_side, out_side, Po))
        return conv_family(False, n, c, side, P, k, general), False, P, Po
    assert ok, (
        "DTYPE {} needs 3x3 stride-1 'same' conv layers with a multiple of 8 filters on maps of at most 64 "
        "pixels a side, stored at a pitch of at least 8, or 1x1 stride-1 conv layers (got {}->{} maps, {}x{} at "
        "pitch {}, {} filter {} stride {})".format(dtype, c, k, side, side, P, mode, f, stride))
    return conv_family(one_by_one, n, c, side, P, k), one_by_one, P, P


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
