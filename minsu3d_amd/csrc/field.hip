// Points in, points out: the feature kernels of TensorField (points -> voxels), trilinear interpolation (voxels -> points)
// and their gradients.  The maps they walk come from ms3d_sparse_quantize and ms3d_interp_map (coords.hip).
//
// Every direction is a GATHER with a single writer per output element, so nothing here adds floats atomically and a
// training step stays bit-reproducible:
//   interp forward    out[n]  = sum_j  w[j][n] * x[rows[j][n]]            the 8 corners in ascending j, one fmaf each
//   interp backward   din[v]  = sum_e  w[e] * dout[point of e]            over the entries of voxel row v in ascending point
//                                                                          (entry_sorted / seg_start: a stable sort of the
//                                                                          table by row, built once per map by the caller)
//   reduce forward    out[v]  = avg | sum | max over the points of voxel v in ascending point index (order / seg_start: a
//                               stable sort of the point -> voxel map)
//   reduce backward   dfeat[n] = dvox[inverse[n]] / count | as is | where arg == n
// Layout: csrc/rows.h.  A voxel that holds thousands of points is walked serially by its thread group: untuned.
#include "rows.h"
#include "../../include/minsu3d_hip.h"

namespace {

using namespace ms3d_rows;

enum { RED_AVG = 0, RED_SUM = 1, RED_MAX = 2 };

template <int VEC>
__global__ __launch_bounds__(256) void interp_forward_kernel(const float *__restrict__ x, const int *__restrict__ rows,
                                                             const float *__restrict__ weights, int N, int C, int CV,
                                                             float *__restrict__ out)
{
    MS3D_ROW_LANE(N, CV, n, cv);
    float acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) acc[c] = 0.f;
    for (int j = 0; j < 8; j++) {
        const int r = rows[(size_t)j * N + n];
        if (r < 0) continue;
        const float w = weights[(size_t)j * N + n];
        float v[VEC];
        load_row<VEC>(x, (size_t)r, C, cv, v);
#pragma unroll
        for (int c = 0; c < VEC; c++) acc[c] = fmaf(w, v[c], acc[c]);
    }
    store_row<VEC>(out, (size_t)n, C, cv, acc);
}

// entry e = 8 * point + corner (the point-major numbering of the table); its weight sits at weights[corner][point]
template <int VEC>
__global__ __launch_bounds__(256) void interp_backward_kernel(const float *__restrict__ dout, const float *__restrict__ weights,
                                                              const long long *__restrict__ entry_sorted,
                                                              const int *__restrict__ seg_start, int Vin, int N, int C, int CV,
                                                              float *__restrict__ din)
{
    MS3D_ROW_LANE(Vin, CV, v, cv);
    float acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) acc[c] = 0.f;
    const int end = seg_start[v + 1];
    for (int s = seg_start[v]; s < end; s++) {
        const long long e = entry_sorted[s];
        const long long n = e >> 3;
        const int j = (int)(e & 7);
        if (n < 0 || n >= N) continue;           // (a grouping that names no point of this map: nothing is read)
        const float w = weights[(size_t)j * N + (size_t)n];
        float g[VEC];
        load_row<VEC>(dout, (size_t)n, C, cv, g);
#pragma unroll
        for (int c = 0; c < VEC; c++) acc[c] = fmaf(w, g[c], acc[c]);
    }
    store_row<VEC>(din, (size_t)v, C, cv, acc);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void field_reduce_kernel(const float *__restrict__ feats, const long long *__restrict__ order,
                                                           const int *__restrict__ seg_start, int V, int C, int CV,
                                                           float *__restrict__ out, int *__restrict__ arg)
{
    MS3D_ROW_LANE(V, CV, v, cv);
    float acc[VEC];
    int win[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) { acc[c] = 0.f; win[c] = -1; }
    const int begin = seg_start[v], end = seg_start[v + 1];
    for (int s = begin; s < end; s++) {
        const long long n = order[s];
        float f[VEC];
        load_row<VEC>(feats, (size_t)n, C, cv, f);
#pragma unroll
        for (int c = 0; c < VEC; c++) {
            if constexpr (MODE == RED_MAX) {
                if (s == begin || f[c] > acc[c]) { acc[c] = f[c]; win[c] = (int)n; }
            } else {
                acc[c] += f[c];
            }
        }
    }
    if constexpr (MODE == RED_AVG) {
        if (end > begin) {
            const float cnt = (float)(end - begin);
#pragma unroll
            for (int c = 0; c < VEC; c++) acc[c] = acc[c] / cnt;
        }
    }
    store_row<VEC>(out, (size_t)v, C, cv, acc);
    if constexpr (MODE == RED_MAX) store_arg<VEC>(arg, (size_t)v, C, cv, win);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void field_reduce_backward_kernel(const float *__restrict__ dvox, const int *__restrict__ inverse,
                                                                    const int *__restrict__ seg_start,
                                                                    const int *__restrict__ arg, int N, int C, int CV,
                                                                    float *__restrict__ dfeat)
{
    MS3D_ROW_LANE(N, CV, n, cv);
    const int v = inverse[n];
    float g[VEC];
    load_row<VEC>(dvox, (size_t)v, C, cv, g);
    if constexpr (MODE == RED_AVG) {
        const float cnt = (float)(seg_start[v + 1] - seg_start[v]);      // >= 1: point n itself lies in voxel v
#pragma unroll
        for (int c = 0; c < VEC; c++) g[c] = g[c] / cnt;
    } else if constexpr (MODE == RED_MAX) {
        int w[VEC];
        load_arg<VEC>(arg, (size_t)v, C, cv, w);
#pragma unroll
        for (int c = 0; c < VEC; c++) g[c] = (w[c] == n) ? g[c] : 0.f;
    }
    store_row<VEC>(dfeat, (size_t)n, C, cv, g);
}

}  // namespace

extern "C" {

int ms3d_interp_forward(const float *x, const int *rows, const float *weights, long N, int C, float *out, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || N < 0 || N > 0x7fffffffL / 8) return MS3D_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!x || !rows || !weights || !out) return MS3D_E_UNSUPPORTED;
    const bool v4 = vec4(C, x, out);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(N, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, interp_forward_kernel, blocks, 256, 0, stream, x, rows, weights, (int)N, C, CV, out);
    return 0;
}

int ms3d_interp_backward(const float *dout, const float *weights, const long long *entry_sorted, const int *seg_start, long Vin,
                         long N, int C, float *din, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || N < 0 || N > 0x7fffffffL / 8 || Vin < 0 || Vin > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (Vin == 0) return 0;
    if (!seg_start || !din || (N > 0 && (!dout || !weights || !entry_sorted))) return MS3D_E_UNSUPPORTED;
    const bool v4 = vec4(C, dout, din);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(Vin, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, interp_backward_kernel, blocks, 256, 0, stream, dout, weights, entry_sorted, seg_start, (int)Vin, (int)N,
                    C, CV, din);
    return 0;
}

int ms3d_field_reduce(int mode, const float *feats, const long long *order, const int *seg_start, long V, int C, float *out,
                      int *arg, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < RED_AVG || mode > RED_MAX || C < 1 || V < 0 || V > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (V == 0) return 0;
    if (!feats || !order || !seg_start || !out || (mode == RED_MAX && !arg)) return MS3D_E_UNSUPPORTED;
    const bool v4 = vec4(C, feats, out, mode == RED_MAX ? arg : nullptr);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(V, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_MODE_VEC((RED_AVG, RED_SUM, RED_MAX), mode, v4, field_reduce_kernel, blocks, 256, 0, stream, feats, order,
                         seg_start, (int)V, C, CV, out, arg);
    return 0;
}

int ms3d_field_reduce_backward(int mode, const float *dvox, const int *inverse, const int *seg_start, const int *arg, long N,
                               int C, float *dfeat, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < RED_AVG || mode > RED_MAX || C < 1 || N < 0 || N > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!dvox || !inverse || !dfeat || (mode == RED_AVG && !seg_start) || (mode == RED_MAX && !arg)) return MS3D_E_UNSUPPORTED;
    const bool v4 = vec4(C, dvox, dfeat, mode == RED_MAX ? arg : nullptr);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(N, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_MODE_VEC((RED_AVG, RED_SUM, RED_MAX), mode, v4, field_reduce_backward_kernel, blocks, 256, 0, stream, dvox,
                         inverse, seg_start, arg, (int)N, C, CV, dfeat);
    return 0;
}

}  // extern "C"
