// Sparse pooling over the engine's offset-major kernel maps (the tables the convolutions walk): max / average / sum.
//
// Both directions are GATHERS, so nothing here adds floats atomically and a training step stays bit-reproducible:
//   forward   out[o]  = reduce_k  in[nbr[k][o]]                        over the present inputs, ascending k
//   backward  din[i]  = sum_k     dout[nbr_inv[k][i]] * weight         through the inverse table (ms3d_kmap_invert; a
//                                                                        submanifold map is its own inverse up to k <-> K-1-k,
//                                                                        the caller passes whichever table names, per offset,
//                                                                        the output row an input row feeds)
// Layout: consecutive lanes take consecutive channels of one row (16 bytes per lane when C % 4 == 0), so the lanes of a
// row read one contiguous run of its neighbour's row; the table entry of (k, row) is the same word for all of them.
// Max keeps the winning offset index per output element (uint8, 255 = the row had no input); ties go to the lowest k
// (strict >).  Average divides by the number of PRESENT inputs of the row.
#include "common.h"
#include "../../include/minsu3d_hip.h"

namespace {

enum { POOL_MAX = 0, POOL_AVG = 1, POOL_SUM = 2 };
constexpr int ARG_NONE = 255;

// VEC = floats per lane (4: C % 4 == 0, rows 16-byte aligned; 1 otherwise); CV = C / VEC lanes per row
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void pool_forward_kernel(const float *__restrict__ in, const int *__restrict__ nbr, int Vout,
                                                           int K, int C, int CV, float *__restrict__ out,
                                                           unsigned char *__restrict__ arg, int *__restrict__ count)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)Vout * CV) return;
    const int o = (int)(t / CV), cv = (int)(t - (long)o * CV);
    float acc[VEC];
    int win[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) { acc[j] = 0.f; win[j] = ARG_NONE; }
    int n = 0;
    for (int k = 0; k < K; k++) {
        const int i = nbr[(size_t)k * Vout + o];
        if (i < 0) continue;
        float v[VEC];
        if constexpr (VEC == 4) {
            const float4 r = reinterpret_cast<const float4 *>(in + (size_t)i * C)[cv];
            v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
        } else {
            v[0] = in[(size_t)i * C + cv];
        }
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
    if constexpr (VEC == 4) {
        reinterpret_cast<float4 *>(out + (size_t)o * C)[cv] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        if constexpr (MODE == POOL_MAX)
            reinterpret_cast<uchar4 *>(arg + (size_t)o * C)[cv] =
                make_uchar4((unsigned char)win[0], (unsigned char)win[1], (unsigned char)win[2], (unsigned char)win[3]);
    } else {
        out[(size_t)o * C + cv] = acc[0];
        if constexpr (MODE == POOL_MAX) arg[(size_t)o * C + cv] = (unsigned char)win[0];
    }
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void pool_backward_kernel(const float *__restrict__ dout, const int *__restrict__ nbr_inv,
                                                            int Vin, int K, int C, int CV,
                                                            const unsigned char *__restrict__ arg, const int *__restrict__ count,
                                                            float *__restrict__ din)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)Vin * CV) return;
    const int i = (int)(t / CV), cv = (int)(t - (long)i * CV);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) acc[j] = 0.f;
    for (int k = 0; k < K; k++) {
        const int o = nbr_inv[(size_t)k * Vin + i];
        if (o < 0) continue;
        float g[VEC];
        if constexpr (VEC == 4) {
            const float4 r = reinterpret_cast<const float4 *>(dout + (size_t)o * C)[cv];
            g[0] = r.x; g[1] = r.y; g[2] = r.z; g[3] = r.w;
        } else {
            g[0] = dout[(size_t)o * C + cv];
        }
        if constexpr (MODE == POOL_MAX) {
            int w[VEC];
            if constexpr (VEC == 4) {
                const uchar4 a = reinterpret_cast<const uchar4 *>(arg + (size_t)o * C)[cv];
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            } else {
                w[0] = arg[(size_t)o * C + cv];
            }
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
    if constexpr (VEC == 4)
        reinterpret_cast<float4 *>(din + (size_t)i * C)[cv] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else
        din[(size_t)i * C + cv] = acc[0];
}

bool rows_vec4(int C, const void *a, const void *b, const void *arg)
{
    return C % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && ((uintptr_t)arg & 3) == 0;
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
    const bool v4 = rows_vec4(C, in, out, arg);
    const int CV = v4 ? C / 4 : C;
    const long blocks = ((long)Vout * CV + 255) / 256;
    if (blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
#define MS3D_POOL_FWD(M)                                                                                               \
    if (v4) pool_forward_kernel<M, 4><<<(unsigned)blocks, 256, 0, stream>>>(in, nbr, Vout, K, C, CV, out, arg, count);    \
    else pool_forward_kernel<M, 1><<<(unsigned)blocks, 256, 0, stream>>>(in, nbr, Vout, K, C, CV, out, arg, count);
    if (mode == POOL_MAX) { MS3D_POOL_FWD(POOL_MAX) }
    else if (mode == POOL_AVG) { MS3D_POOL_FWD(POOL_AVG) }
    else { MS3D_POOL_FWD(POOL_SUM) }
#undef MS3D_POOL_FWD
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_pool_backward(int mode, const float *dout, const int *nbr_inv, int Vin, int K, int C, const unsigned char *arg,
                       const int *count, float *din, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < POOL_MAX || mode > POOL_SUM || K < 1 || K >= ARG_NONE || C < 1) return MS3D_E_UNSUPPORTED;
    if ((mode == POOL_MAX && !arg) || (mode == POOL_AVG && !count)) return MS3D_E_UNSUPPORTED;
    if (Vin <= 0) return 0;
    const bool v4 = rows_vec4(C, dout, din, arg);
    const int CV = v4 ? C / 4 : C;
    const long blocks = ((long)Vin * CV + 255) / 256;
    if (blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
#define MS3D_POOL_BWD(M)                                                                                               \
    if (v4) pool_backward_kernel<M, 4><<<(unsigned)blocks, 256, 0, stream>>>(dout, nbr_inv, Vin, K, C, CV, arg, count, din); \
    else pool_backward_kernel<M, 1><<<(unsigned)blocks, 256, 0, stream>>>(dout, nbr_inv, Vin, K, C, CV, arg, count, din);
    if (mode == POOL_MAX) { MS3D_POOL_BWD(POOL_MAX) }
    else if (mode == POOL_AVG) { MS3D_POOL_BWD(POOL_AVG) }
    else { MS3D_POOL_BWD(POOL_SUM) }
#undef MS3D_POOL_BWD
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
