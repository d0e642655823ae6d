// Row access of the gather kernels (field.hip, neighbor.hip): consecutive lanes take consecutive channels of one row, VEC
// floats per lane -- 4 (one 16-byte access) when C % 4 == 0 and the rows are 16-byte aligned, else 1; CV = C / VEC lanes per row.
#pragma once
#include "common.h"

namespace ms3d_rows {

template <int VEC>
__device__ __forceinline__ void load_row(const float *__restrict__ p, size_t row, int C, int cv, float (&v)[VEC])
{
    if constexpr (VEC == 4) {
        const float4 r = reinterpret_cast<const float4 *>(p + row * C)[cv];
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
        v[0] = p[row * C + cv];
    }
}

template <int VEC>
__device__ __forceinline__ void store_row(float *__restrict__ p, size_t row, int C, int cv, const float (&v)[VEC])
{
    if constexpr (VEC == 4)
        reinterpret_cast<float4 *>(p + row * C)[cv] = make_float4(v[0], v[1], v[2], v[3]);
    else
        p[row * C + cv] = v[0];
}

static inline bool vec4(int C, const void *a, const void *b, const void *c = nullptr)
{
    return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// grid of one thread per (row, lane of the row); false when it does not fit a launch
static inline bool grid_of(long rows, int CV, unsigned *blocks)
{
    const long b = (rows * CV + 255) / 256;
    if (b > 0x7fffffffL) return false;
    *blocks = (unsigned)b;
    return true;
}

}  // namespace ms3d_rows
