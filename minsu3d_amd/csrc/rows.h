// The row layout of the gather kernels (pool.hip, chconv.hip, setops.hip, field.hip, neighbor.hip): one thread per (row, lane
// of the row), consecutive lanes taking consecutive channels, so the lanes of a row read one contiguous run of the row they
// gather and the table entry of (k, row) is the same word for all of them.  A lane holds VEC floats: 4 (one 16-byte access)
// when C % 4 == 0 and every row pointer is 16-byte aligned, else 1; CV = C / VEC lanes per row.  An argmax row beside the
// floats (uint8 or int per channel) is accessed in the same units: 4 or 16 bytes per lane, or one element.
#pragma once
#include "common.h"

namespace ms3d_rows {

// ---- device: the VEC floats at p
template <int VEC>
__device__ __forceinline__ void load_vec(const float *__restrict__ p, float (&v)[VEC])
{
    if constexpr (VEC == 4) {
        const float4 r = *reinterpret_cast<const float4 *>(p);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
        v[0] = *p;
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *__restrict__ p, const float (&v)[VEC])
{
    if constexpr (VEC == 4)
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *p = v[0];
}

// lane cv of row `row` of p, whose rows are ld floats apart
template <int VEC>
__device__ __forceinline__ void load_row(const float *__restrict__ p, size_t row, int ld, int cv, float (&v)[VEC])
{
    load_vec<VEC>(p + (row * ld + (size_t)cv * VEC), v);
}

template <int VEC>
__device__ __forceinline__ void store_row(float *__restrict__ p, size_t row, int ld, int cv, const float (&v)[VEC])
{
    store_vec<VEC>(p + (row * ld + (size_t)cv * VEC), v);
}

// the same lane of an argmax row: uint8 (one 4-byte access) or int (one 16-byte access) per channel, as ints
template <int VEC>
__device__ __forceinline__ void load_arg(const unsigned char *__restrict__ arg, size_t row, int ld, int cv, int (&w)[VEC])
{
    if constexpr (VEC == 4) {
        const uchar4 a = *reinterpret_cast<const uchar4 *>(arg + (row * ld + (size_t)cv * VEC));
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else {
        w[0] = arg[row * ld + (size_t)cv * VEC];
    }
}

template <int VEC>
__device__ __forceinline__ void store_arg(unsigned char *__restrict__ arg, size_t row, int ld, int cv, const int (&w)[VEC])
{
    if constexpr (VEC == 4)
        *reinterpret_cast<uchar4 *>(arg + (row * ld + (size_t)cv * VEC)) =
            make_uchar4((unsigned char)w[0], (unsigned char)w[1], (unsigned char)w[2], (unsigned char)w[3]);
    else
        arg[row * ld + (size_t)cv * VEC] = (unsigned char)w[0];
}

template <int VEC>
__device__ __forceinline__ void load_arg(const int *__restrict__ arg, size_t row, int ld, int cv, int (&w)[VEC])
{
    if constexpr (VEC == 4) {
        const int4 a = *reinterpret_cast<const int4 *>(arg + (row * ld + (size_t)cv * VEC));
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else {
        w[0] = arg[row * ld + (size_t)cv * VEC];
    }
}

template <int VEC>
__device__ __forceinline__ void store_arg(int *__restrict__ arg, size_t row, int ld, int cv, const int (&w)[VEC])
{
    if constexpr (VEC == 4)
        *reinterpret_cast<int4 *>(arg + (row * ld + (size_t)cv * VEC)) = make_int4(w[0], w[1], w[2], w[3]);
    else
        arg[row * ld + (size_t)cv * VEC] = w[0];
}

// The prologue of every kernel of the layout, in a launch of grid_of(rows, CV) blocks: declares this thread's `row` and its
// lane `cv` of the row, and leaves the kernel when the thread is past the last row.  (A macro: as a function that reports
// "no work" the same three lines compile to other code in every kernel -- the dead path's values meet the live ones.)
#define MS3D_ROW_LANE(rows, CV, row, cv)                                      \
    const long t_ = (long)blockIdx.x * blockDim.x + threadIdx.x;              \
    if (t_ >= (long)(rows) * (CV)) return;                                    \
    const int row = (int)(t_ / (CV)), cv = (int)(t_ - (long)row * (CV))

// ---- host: which instantiation runs, and its grid

// the 16-byte route: C % 4 == 0 and every row pointer 16-byte aligned (NULL counts as aligned)
template <typename... P> static inline bool vec4(int C, const P *...p) { return C % 4 == 0 && ms3d_aligned16(p...); }

// a uint8 argmax row of the 16-byte route is one 4-byte access per lane (NULL counts as aligned)
static inline bool arg_aligned4(const unsigned char *arg) { return ((uintptr_t)arg & 3) == 0; }

// grid of one thread per (row, lane of the row); false when it does not fit a launch
static inline bool grid_of(long rows, int CV, unsigned *blocks)
{
    const long b = (rows * CV + 255) / 256;
    if (b > 0x7fffffffL) return false;
    *blocks = (unsigned)b;
    return true;
}

}  // namespace ms3d_rows
