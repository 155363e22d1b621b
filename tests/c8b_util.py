"""Host-side helpers of the bf16-resident ("c8", DTYPE 'bfloat16') tests: the rounding that specifies the mode and the
layout in bf16.  The arithmetic statement is the fp16 one of tests/c8_util.py with rbf16 in place of r16 (operands
rounded to bf16, products exact, float64 sums standing in for the fp32 accumulation, one rounding on store)."""
import numpy as np


def rbf16(a, scale=1.0):
    """float64 -> the nearest bf16 value (round to nearest, ties to even: 8 significant bits, fp32's exponent range with
    its subnormals, overflow to inf), widened back to float64; scale as in oracle.theanet_oracle.r16 (a power of two:
    exact)."""
    a = np.asarray(a, np.float64) * scale
    _, e = np.frexp(a)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)         # the bf16 quantum at a: 2^(e-8), 2^-133 in the subnormal range
    r = np.round(a / q) * q                            # np.round: ties to even
    big = np.abs(r) >= 2.0 ** 128
    r = np.where(big, np.copysign(np.inf, a), r)
    return np.where(np.isfinite(a), r, a) / scale


def bf16_bits(a):
    """float values that are bf16 already (e.g. rbf16's) -> their uint16 bit patterns."""
    return (np.asarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_c8(x):
    """(N, C, H, W) float -> raw uint16 image of the bf16 c8 tensor [N][C8][H][W][8] (values rounded by rbf16)."""
    x = np.asarray(x, np.float64)
    N, C, H, W = x.shape
    C8 = (C + 7) // 8
    buf = np.zeros((N, C8 * 8, H, W), np.uint16)
    buf[:, :C] = bf16_bits(rbf16(x))
    return np.ascontiguousarray(buf.reshape(N, C8, 8, H, W).transpose(0, 1, 3, 4, 2))


def from_c8(raw, C):
    """[N][C8][H][W][8] bf16 bit patterns (uint16) -> (N, C, H, W) float32."""
    N, C8, H, W, _ = raw.shape
    return bf16_value(raw).transpose(0, 1, 4, 2, 3).reshape(N, C8 * 8, H, W)[:, :C].astype(np.float32)
