// Sparse pooling over the engine's offset-major kernel maps (the tables the convolutions walk): max / average / sum.
//
// Both directions are GATHERS, so nothing here adds floats atomically and a training step stays bit-reproducible:
//   forward   out[o]  = reduce_k  in[nbr[k][o]]                        over the present inputs, ascending k
//   backward  din[i]  = sum_k     dout[nbr_inv[k][i]] * weight         through the inverse table (ms3d_kmap_invert; a
//                                                                        submanifold map is its own inverse up to k <-> K-1-k,
//                                                                        the caller passes whichever table names, per offset,
//                                                                        the output row an input row feeds)
// Layout: csrc/rows.h (one thread per (row, lane of the row)).
// Max keeps the winning offset index per output element (uint8, 255 = the row had no input); ties go to the lowest k
// (strict >).  Average divides by the number of PRESENT inputs of the row.
#include "rows.h"
#include "../../include/minsu3d_hip.h"

namespace {

using namespace ms3d_rows;

enum { POOL_MAX = 0, POOL_AVG = 1, POOL_SUM = 2 };
constexpr int ARG_NONE = 255;

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void pool_forward_kernel(const float *__restrict__ in, const int *__restrict__ nbr, int Vout,
                                                           int K, int C, int CV, float *__restrict__ out,
                                                           unsigned char *__restrict__ arg, int *__restrict__ count)
{
    MS3D_ROW_LANE(Vout, CV, o, cv);
    float acc[VEC];
    int win[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) { acc[j] = 0.f; win[j] = ARG_NONE; }
    int n = 0;
    for (int k = 0; k < K; k++) {
        const int i = nbr[(size_t)k * Vout + o];
        if (i < 0) continue;
        float v[VEC];
        load_row<VEC>(in, (size_t)i, C, cv, v);
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            if constexpr (MODE == POOL_MAX) {
                if (n == 0 || v[j] > acc[j]) { acc[j] = v[j]; win[j] = k; }
            } else {
                acc[j] += v[j];
            }
        }
        n++;
    }
    if constexpr (MODE == POOL_AVG) {
        if (n > 0) {
#pragma unroll
            for (int j = 0; j < VEC; j++) acc[j] = acc[j] / (float)n;
        }
        if (cv == 0) count[o] = n;
    }
    store_row<VEC>(out, (size_t)o, C, cv, acc);
    if constexpr (MODE == POOL_MAX) store_arg<VEC>(arg, (size_t)o, C, cv, win);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void pool_backward_kernel(const float *__restrict__ dout, const int *__restrict__ nbr_inv,
                                                            int Vin, int K, int C, int CV,
                                                            const unsigned char *__restrict__ arg, const int *__restrict__ count,
                                                            float *__restrict__ din)
{
    MS3D_ROW_LANE(Vin, CV, i, cv);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) acc[j] = 0.f;
    for (int k = 0; k < K; k++) {
        const int o = nbr_inv[(size_t)k * Vin + i];
        if (o < 0) continue;
        float g[VEC];
        load_row<VEC>(dout, (size_t)o, C, cv, g);
        if constexpr (MODE == POOL_MAX) {
            int w[VEC];
            load_arg<VEC>(arg, (size_t)o, C, cv, w);
#pragma unroll
            for (int j = 0; j < VEC; j++) acc[j] += (w[j] == k) ? g[j] : 0.f;
        } else if constexpr (MODE == POOL_AVG) {
            const float n = (float)count[o];        // >= 1: row i itself is one of o's inputs
#pragma unroll
            for (int j = 0; j < VEC; j++) acc[j] += g[j] / n;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++) acc[j] += g[j];
        }
    }
    store_row<VEC>(din, (size_t)i, C, cv, acc);
}

}  // namespace

extern "C" {

int ms3d_pool_forward(int mode, const float *in, const int *nbr, int Vout, int K, int C, float *out, unsigned char *arg,
                      int *count, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < POOL_MAX || mode > POOL_SUM || K < 1 || K >= ARG_NONE || C < 1) return MS3D_E_UNSUPPORTED;
    if ((mode == POOL_MAX && !arg) || (mode == POOL_AVG && !count)) return MS3D_E_UNSUPPORTED;
    if (Vout <= 0) return 0;
    const bool v4 = vec4(C, in, out) && arg_aligned4(arg);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(Vout, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_MODE_VEC((POOL_MAX, POOL_AVG, POOL_SUM), mode, v4, pool_forward_kernel, blocks, 256, 0, stream, in, nbr, Vout, K,
                         C, CV, out, arg, count);
    return 0;
}

int ms3d_pool_backward(int mode, const float *dout, const int *nbr_inv, int Vin, int K, int C, const unsigned char *arg,
                       const int *count, float *din, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < POOL_MAX || mode > POOL_SUM || K < 1 || K >= ARG_NONE || C < 1) return MS3D_E_UNSUPPORTED;
    if ((mode == POOL_MAX && !arg) || (mode == POOL_AVG && !count)) return MS3D_E_UNSUPPORTED;
    if (Vin <= 0) return 0;
    const bool v4 = vec4(C, dout, din) && arg_aligned4(arg);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(Vin, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_MODE_VEC((POOL_MAX, POOL_AVG, POOL_SUM), mode, v4, pool_backward_kernel, blocks, 256, 0, stream, dout, nbr_inv,
                         Vin, K, C, CV, arg, count, din);
    return 0;
}

}  // extern "C"
