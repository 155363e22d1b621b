// What the pool families of the 16-bit conv stack share (pool_c8.hip: stride = window; pools_c8.hip: any stride): a
// 16-byte cell as packed 16-bit lanes, the ordered integer key the stored values are compared through, the mask of a
// ragged last octet, the cell index -> (plane, row, column) split, and the host's cell-count rule.
#pragma once
#include "common.h"

// A cell as four dwords of two 16-bit lanes: every step below is one packed (v_pk_*_i16 / _u16) or one 32-bit bitwise
// instruction per dword.
typedef short c8p_i16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short c8p_u16x2 __attribute__((ext_vector_type(2)));

struct c8p_cell {
    c8p_i16x2 d[4];
};

__device__ __forceinline__ c8p_cell c8p_load(const uint4* p) {
    union { uint4 q; c8p_cell c; } u;
    u.q = *p;
    return u.c;
}

__device__ __forceinline__ uint4 c8p_quad(c8p_cell c) {
    union { uint4 q; c8p_cell c; } u;
    u.c = c;
    return u.q;
}

// the ordered key of two stored values: the sign-magnitude pattern as a two's-complement integer, -(u & 0x7fff) for a
// negative pattern -- grows with the value, 0 for +0 and for -0
__device__ __forceinline__ c8p_i16x2 c8p_key(c8p_i16x2 v) {
    const c8p_i16x2 neg = v >> (short)15;                       // 0xffff in the lanes of negative patterns
    return ((v & (short)0x7fff) ^ neg) - neg;
}

// 0xffff in the lanes where key k is greater than key kb (keys lie in [-0x7fff, 0x7fff]: the saturated difference keeps
// its sign).  The packed subtraction, and the bitwise select in c8p_take, are spelled out: from their C++ forms hipcc
// derives a 16-bit compare and a select for every lane, three times the instructions plus wait states.
__device__ __forceinline__ c8p_i16x2 c8p_gt(c8p_i16x2 k, c8p_i16x2 kb) {
    c8p_i16x2 d;
    asm("v_pk_sub_i16 %0, %1, %2 clamp" : "=v"(d) : "v"(kb), "v"(k));
    return d >> (short)15;
}

// 0xffff in the lanes where the keys are equal
__device__ __forceinline__ c8p_i16x2 c8p_eq(c8p_i16x2 ka, c8p_i16x2 kb) {
    const c8p_u16x2 one = (unsigned short)1;
    return (c8p_i16x2)(__builtin_elementwise_min((c8p_u16x2)(ka ^ kb), one) - one);
}

// best <- c where c is strictly greater, lane by lane; kb: best's keys
__device__ __forceinline__ void c8p_take(c8p_cell& best, c8p_cell& kb, const c8p_cell& c) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const c8p_i16x2 k = c8p_key(c.d[q]), m = c8p_gt(k, kb.d[q]);
        asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(best.d[q]) : "v"(m), "v"(c.d[q]));          // (c & m) | (best & ~m)
        kb.d[q] = __builtin_elementwise_max(k, kb.d[q]);
    }
}

// the lanes of a cell that hold channels < C: all of them except in the last octet of a C that is no multiple of 8
__device__ __forceinline__ uint4 c8p_valid(unsigned pair, int C, unsigned C8) {
    uint4 m = make_uint4(~0u, ~0u, ~0u, ~0u);
    if ((C & 7) && pair % C8 == C8 - 1u) {
        const unsigned long long lo = (C & 7) >= 4 ? ~0ull : (1ull << (16 * (C & 7))) - 1ull;
        const unsigned long long hi = (C & 7) > 4 ? (1ull << (16 * ((C & 7) - 4))) - 1ull : 0ull;
        m = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
    }
    return m;
}

__device__ __forceinline__ uint4 c8p_and(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }

// cell index -> (plane = n * C8 + octet, row, column) of a tensor at pitch P; SH: P = 1 << lg
template <bool SH>
__device__ __forceinline__ void c8p_where(unsigned cell, unsigned P, int lg, unsigned& pair, unsigned& h, unsigned& w) {
    if (SH) {
        const unsigned row = cell >> lg;
        w = cell & (P - 1u);
        pair = row >> lg;
        h = row & (P - 1u);
    } else {
        const unsigned row = cell / P;
        w = cell - row * P;
        pair = row / P;
        h = row - pair * P;
    }
}

// log2 of a power of two, -1 otherwise
static int c8p_lg(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// cells of a c8 tensor of N x C maps of S pixels a side at pitch P (c8_drop_cells' rule), or -1
static long long c8p_cells(int N, int C, int S, int P) {
    if (N <= 0 || C <= 0 || S <= 0 || P < S || (P != S && (P & (P - 1)))) return -1;
    const long long cells = (long long)N * ((C + 7) / 8) * P * P;
    return cells < (1ll << 32) - 256 ? cells : -1;
}
