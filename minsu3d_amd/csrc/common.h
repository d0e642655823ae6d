// Shared host/device helpers for the gfx950 kernels (wave = 64 everywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#define MS3D_WAVE 64
#define MS3D_PL_ROWS 64  // output rows per tile of a pair list (ms3d_kmap_pairlist_build)
#define MS3D_PL_PARTS 256  // a pair list is cut into this many parts of near-equal batch count (one per block of a launch)
// int offset of the pick list (int4 per tile, 16-byte aligned) inside the tile_start array of a pair list
#define MS3D_PL_SCHED_OFFSET(tiles) (((tiles) + 1 + MS3D_PL_PARTS + 1 + 3) & ~3)

// Every launcher returns 0 on success or a non-zero hipError_t; nothing ever calls exit().
#define MS3D_CHECK(expr)                                   \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return (int)_e;              \
    } while (0)
#define MS3D_LAUNCH_CHECK() MS3D_CHECK(hipGetLastError())

static inline int ms3d_divup(long a, long b) { return (int)((a + b - 1) / b); }
static inline size_t ms3d_align(size_t x) { return (x + 255) & ~(size_t)255; }

// every pointer 16-byte aligned; NULL counts as aligned, so a pointer that is not asked for does not decide the route
template <typename... P> static inline bool ms3d_aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15) == 0; }

// f(std::integral_constant<int, M>()) for the M of the list that equals mode; the last of the list when none does (the
// launcher has checked the range of mode).  The call stands before the recursion so that what f instantiates is emitted in
// the order of the list.
template <int M, int... REST, typename F> static inline void ms3d_with_mode(int mode, F f)
{
    if (mode == M || sizeof...(REST) == 0) f(std::integral_constant<int, M>());
    else if constexpr (sizeof...(REST) > 0) ms3d_with_mode<REST...>(mode, f);
}

// The two instantiations kernel<VEC> of a kernel template, one argument list: VEC = 4 when v4, else 1; returns the
// launch's error from the calling function.
#define MS3D_LAUNCH_VEC(v4, kernel, grid, threads, lds, stream, ...)                  \
    do {                                                                              \
        if (v4) kernel<4><<<grid, threads, lds, stream>>>(__VA_ARGS__);               \
        else kernel<1><<<grid, threads, lds, stream>>>(__VA_ARGS__);                  \
        MS3D_LAUNCH_CHECK();                                                          \
    } while (0)

// The same for kernel<MODE, VEC>: the instantiation of the run-time mode among the parenthesised list `modes`.
#define MS3D_LAUNCH_MODE_VEC(modes, mode, v4, kernel, grid, threads, lds, stream, ...)                         \
    do {                                                                                                       \
        ms3d_with_mode<MS3D_UNPAREN modes>(mode, [&](auto m_) {                                                \
            if (v4) kernel<decltype(m_)::value, 4><<<grid, threads, lds, stream>>>(__VA_ARGS__);               \
            else kernel<decltype(m_)::value, 1><<<grid, threads, lds, stream>>>(__VA_ARGS__);                  \
        });                                                                                                    \
        MS3D_LAUNCH_CHECK();                                                                                   \
    } while (0)
#define MS3D_UNPAREN(...) __VA_ARGS__

#ifdef __HIPCC__
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ int wave_id() { return (int)(threadIdx.x >> 6); }

// inclusive prefix sum across the 64 lanes of a wave
__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(v, d, 64);
        if (l >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_min_f(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_max_f(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
// number of set bits of a wave ballot below this lane
__device__ __forceinline__ int ballot_rank(unsigned long long m)
{
    return __popcll(m & ((1ull << lane_id()) - 1ull));
}
#endif
