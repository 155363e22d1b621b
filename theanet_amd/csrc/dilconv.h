// Dilated convolution (ConvLayer(..., dilation=d): the taps of the f x f filter are d pixels apart, Theano's
// filter_dilation=(d, d); W (K, C, f, f) in tn_conv2d_*'s orientation, b (K); stride 1 when d > 1) -- what the two families
// share: dilconv.hip (fp32 NCHW, tn_dilconv_*) and dilconv_c8.hip (the 16-bit conv stack, tn_c8_dilconv_*).  With
// fe = (f - 1) d + 1 the layer computes what a dense layer of filter fe computes whose weights are W zero-stuffed; its
// geometry (padding, output side) is that layer's.
//
// The polyphase split.  Output coordinate o reads source coordinates o + off0 + i d, i < f (off0 = -pad forward,
// pad - (fe - 1) input gradient: gconv.h's MODE 0 and MODE 1, there is no strided form).  All of them lie on the lattice of
// o's residue mod d: with o = p + d m the source is (p + off0) + d (m + i).  So the layer is d d independent DENSE f x f
// convolutions, phase (py, px) mapping the sub-lattice plane m -> p + off0 + d m of the source onto the sub-lattice plane
// m -> p + d m of the output.  dc_count says how many outputs a phase has along an axis (ceil or floor of So / d; none
// for p >= So: the grid has min(d, stored side) phases an axis, a phase without an output issues no load and no product,
// and on a padded plane its blocks only write the +0 pad cells).
//
// Forward / input gradient.  grid (images x tiles of the phase plane, phases, groups of output row tiles).  A block owns a
// TH x TW tile of ONE phase's outputs and stages that phase's source tile -- (TH + f - 1) x (TW + f - 1) sub-lattice pixels
// of the reduced maps, read at a stride of d pixels, +0 outside the map -- in LDS; every tap is then a dense offset into the
// tile and the halo is f - 1 whatever d is.  Neighbouring phases read the other pixels of the same lines: L2 serves them.
// The waves of a block divide the tile's pixel units AND, where the phase plane is too small for four waves of pixels, the
// output row tiles (WU waves over pixels x WM = 4 / WU over rows).  A wave keeps the accumulators of up to DC_MTB row tiles
// and reads a step's B operand from LDS ONCE for all of them (gconv.h reads it once a row tile); the reduced maps go through
// LDS in chunks where the smallest tile of all of them does not fit GC_LDS_MAX, the accumulators staying in registers
// across the chunks.  There is no HBM-direct form.
//
// LDS row pitch (dilconv_c8.hip).  A step's operand is one ds_read_b128 per lane; the LDS serves it a quarter wave -- 16
// lanes, 256 bytes, every one of the 64 banks once -- at a time, and a quarter wave reads 16 pixels of ONE staged cell
// plane: 16 / TW rows of TW neighbouring cells.  With TW = 16 that is one contiguous 256-byte run at any pitch.  With TW = 8
// or 4 the rows must fall into different 16 TW-byte slots of the 256: the pitch IWp (in cells) is the smallest >= TW + f - 1
// with IWp = TW (mod 2 TW), so that r IWp 16 mod 256 runs through the slots once for r < 16 / TW (dc_pitch; the reasoning is
// the bank arithmetic, not a measurement).  The fp32 family reads 4 bytes a lane and takes gconv.hip's odd pitch.
//
// Weight gradient.  Pixels are the reduction dimension of the matrix core, so phases buy nothing: the x operand of tap
// (i, j) is the output pixel tile shifted by (i d, j d) -- as contiguous along a row as at d = 1 -- and is read at those
// dilated offsets, +0 outside the map (gconv's weight gradients with the tap offsets multiplied by d).
#pragma once
#include "gconv.h"

#define DC_MTB 4         // row tiles a wave accumulates at once (16-row tiles; half as many 32-row ones)
#define DC_F_MAX 32
#define DC_D_MAX 255

// outputs of phase p along an axis of So outputs
__host__ __device__ __forceinline__ int dc_count(int So, int p, int d) { return p < So ? (So - p + d - 1) / d : 0; }

// the filter side of the zero-stuffed dense layer
static inline long long dc_fe(int f, int d) { return (long long)(f - 1) * d + 1; }

// consistent geometry along one axis: gc_axis_ok's rule with fe for f, stride 1 when d > 1
static inline bool dc_axis_ok(int S, int f, int d, int stride, int pad, int So) {
    if (d < 1 || d > DC_D_MAX || f < 1 || f > DC_F_MAX || (d > 1 && stride != 1)) return false;
    return gc_axis_ok(S, (int)dc_fe(f, d), stride, pad, So);
}

// LDS row pitch in cells of a staged tile of IW cells a row read by units of TW columns (above)
static inline int dc_pitch(int IW, int TW) {
    if (TW >= 16) return IW;
    int p = IW;
    while (p % (2 * TW) != TW) ++p;
    return p;
}

// waves of a block over pixel units along the rows of a phase plane of `cnt` rows, RU rows a unit; the others go over row tiles
static inline int dc_waves_over_pixels(int cnt, int RU) {
    const int units = (cnt + RU - 1) / RU;
    return units >= 3 ? 4 : (units == 2 ? 2 : 1);
}
