// The operand staging of the all-pairs tile kernels (pairwise.hip, manifold.hip): a T x KC chunk of rows goes from global memory to
// registers (fetch) and from there to LDS TRANSPOSED (stage): image[kk][row], rows of T + 4 floats, T = 64 R.  A thread of the 16 x 16
// micro-tile grid then reads its operands of one kk as 16-byte words at 4 ty (a broadcast over the 16 lanes that share ty) and at 4 tx (16
// consecutive words: the 64 banks once): every lane group of ds_read_b128 is conflict-free (MI355X_MICROARCH, LDS).  The staging stores are
// 4-byte and 4-way conflicted (LD = 4 mod 32); they are 1 / 32 of the LDS cycles of the chunk's reads.
#pragma once
#include <cstdint>

#include "common.h"

namespace gc_tile {

constexpr int KC = 32;                 // columns per LDS chunk
constexpr int NT = 256;                // threads per workgroup of a tile kernel

// This thread's share of a T x KC operand chunk: 2 R words of 4 columns (8 words per row, consecutive lanes along the row).  Columns past k
// and rows past `rows` are ZERO and never addressed.  GATHER: tile row r is row gather[r] of `base` (gather has `rows` entries).
template <int R, bool VEC, bool GATHER = false>
__device__ __forceinline__ void fetch(float4 (&reg)[2 * R], const float* __restrict__ base, long long stride, int rows, int row0, int k, int k0,
                                      int tid, const int32_t* __restrict__ gather = nullptr) {
#pragma unroll
    for (int u = 0; u < 2 * R; ++u) {
        const int f = tid + u * NT;
        const int row = row0 + (f >> 3), col = k0 + (f & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < rows && col < k) {
            const float* p = base + (long long)(GATHER ? gather[row] : row) * stride + col;
            if (VEC) {          // k % 4 == 0: the word ends inside the row
                v = *reinterpret_cast<const float4*>(p);
            } else {
                v.x = p[0];
                if (col + 1 < k) v.y = p[1];
                if (col + 2 < k) v.z = p[2];
                if (col + 3 < k) v.w = p[3];
            }
        }
        reg[u] = v;
    }
}

template <int R>
__device__ __forceinline__ void stage(const float4 (&reg)[2 * R], float* image, int tid) {
    constexpr int LD = 64 * R + 4;
#pragma unroll
    for (int u = 0; u < 2 * R; ++u) {
        const int f = tid + u * NT;
        float* dst = image + (f & 7) * 4 * LD + (f >> 3);
        dst[0] = reg[u].x; dst[LD] = reg[u].y; dst[2 * LD] = reg[u].z; dst[3 * LD] = reg[u].w;
    }
}

}  // namespace gc_tile
