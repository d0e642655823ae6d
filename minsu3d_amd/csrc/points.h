// What the per-sample point kernels (csrc/fps.hip, csrc/knn.hip) share: the float32 distance and the two clamps through which
// the batch grouping (order, seg_start) is read.  The integer distances stay with their kernels: fps.hip uses plain 32-bit
// products and knn.hip 24-bit ones, which agree bit for bit over the packable range; which is faster in the other kernel has
// not been measured.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// (dx*dx + dy*dy) + dz*dz with dx = a.x - b.x, seven float32 roundings.  hipcc contracts a * b + c into an FMA by default --
// HIP's __fmul_rn and __fadd_rn are the plain operators and are contracted like them -- so contraction is switched off for this
// body alone: an FMA changes picks and neighbours, and both kernels must measure the same distance.
__device__ __forceinline__ float dist_f32(float ax, float ay, float az, float bx, float by, float bz)
{
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// the held row at position p of `order`, kept inside [0, V): an index outside its array is never followed
__device__ __forceinline__ long held_row(const long long *__restrict__ order, long p, int V)
{
    const long long h = order[p];
    return h < 0 ? 0 : (h >= V ? V - 1 : (long)h);
}

// a segment bound (seg_start, q_start) kept inside [0, hi]
__device__ __forceinline__ int clamp_to(int v, int hi) { return min(max(v, 0), hi); }
#endif
