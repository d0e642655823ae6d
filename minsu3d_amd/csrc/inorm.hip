// Instance normalisation of sparse rows: per batch index (segment) and channel.  x, y, dy, dx, weight, bias and the parameter
// gradients are float32; every sum, the statistics (mean, invstd: double [B, C]) and the arithmetic of the row passes are
// float64, rounded once at the store.  The backward is a difference of nearly equal terms when a segment is short (two rows:
// dx is 2 eps / (x1 - x2)^2 of its terms, below what float32 statistics can resolve), and the passes are bound by the row
// traffic, not by the arithmetic.
//
//   forward   mean[s,c] = (1/n_s) sum_r x[r,c]      var[s,c] = (1/n_s) sum_r (x[r,c] - mean[s,c])^2      (biased)
//             invstd[s,c] = 1 / sqrt(var[s,c] + eps)     y[r,c] = (x[r,c] - mean[s,c]) * invstd[s,c] * weight[c] + bias[c]
//   backward  xhat = (x - mean) * invstd (recomputed)    S1[s,c] = sum_r dy[r,c]    S2[s,c] = sum_r dy[r,c] * xhat[r,c]
//             dx[r,c] = weight[c] * invstd[s,c] * (dy[r,c] - S1[s,c] / n_s - xhat[r,c] * S2[s,c] / n_s)
//             dweight[c] = sum_s S2[s,c]     dbias[c] = sum_s S1[s,c]                       (ascending s)
//
// The rows of segment s are order[seg_start[s] .. seg_start[s + 1]) (CoordinateManager.batch_rows): they are read where they
// lie, no permuted copy of x exists.  Every sum has ONE fixed order and nothing adds floats atomically (the scheme of
// ms3d_broadcast_reduce in csrc/setops.hip): a segment is cut into INORM_SLICES slices of ceil(n_s / INORM_SLICES)
// consecutive positions of `order`, one workgroup sums one slice (each thread its rows in ascending order, the threads of a
// column in ascending order), and a small second kernel merges the slice partials in ascending slice order, skipping the
// empty ones.  The order is a function of (n_s, C) alone -- not of the CU count, not of the vector width.
//
// Statistics: never E[x^2] - E[x]^2 of the raw values.  A slice shifts by its first row K, sums (x - K) and (x - K)^2 in one
// pass and emits (mean, M2) = (K + t1 / n, t2 - t1^2 / n); the merge is Chan's: delta = mean_b - mean_a, mean += delta *
// n_b / n, M2 += M2_b + delta^2 * n_a * n_b / n.
//
// Layout: a lane takes FOUR consecutive channels of a row in both routes -- one 16-byte access when C % 4 == 0 and every
// pointer is 16-byte aligned, four guarded 4-byte accesses otherwise -- so the two routes run the same arithmetic on the
// same values in the same order and give the same bits.  A workgroup is CW column lanes (a power of two, at most 32 = 128
// channels per pass) by 256 / CW row lanes; wider rows take more passes.
#include "common.h"
#include "../../include/minsu3d_hip.h"

// what is written is what runs: no a * b + c contracted in one instantiation and not in the other
#pragma clang fp contract(off)

namespace {

constexpr int INORM_SLICES = 256;     // slices per segment: a constant of the library, NOT derived from the device
constexpr int INORM_CW_MAX = 32;      // column lanes (4 channels each) of a pass at most
constexpr int INORM_UNROLL = 4;       // row loads in flight per lane

// (not the load_row / store_row of csrc/rows.h: guarded four-channel accesses that give both routes the same bits)
template <bool V4>
__device__ __forceinline__ void load4(const float *__restrict__ p, int c, int C, float (&v)[4])
{
    if constexpr (V4) {
        const float4 r = *reinterpret_cast<const float4 *>(p + c);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = c + k < C ? p[c + k] : 0.f;
    }
}
// p may be NULL: the constant d (a missing weight is 1, a missing bias 0)
template <bool V4>
__device__ __forceinline__ void load4_or(const float *__restrict__ p, int c, int C, float d, float (&v)[4])
{
    if (p) {
        load4<V4>(p, c, C, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = d;
    }
}
template <bool V4>
__device__ __forceinline__ void store4(float *__restrict__ p, int c, int C, const float (&v)[4])
{
    if constexpr (V4) {
        *reinterpret_cast<float4 *>(p + c) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c + k < C) p[c + k] = v[k];
    }
}

// the small double arrays (partials, statistics, segment sums): four guarded 8-byte accesses in both routes
__device__ __forceinline__ void load4d(const double *__restrict__ p, int c, int C, double (&v)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = c + k < C ? p[c + k] : 0.0;
}
__device__ __forceinline__ void store4d(double *__restrict__ p, int c, int C, const double (&v)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (c + k < C) p[c + k] = v[k];
}

// positions [s0, s1) of slice p of a segment of len rows (empty when s0 == s1)
__device__ __forceinline__ void slice_of(int p, int len, int &s0, int &s1)
{
    const int per = (len + INORM_SLICES - 1) / INORM_SLICES;           // p * per <= 255 * 2^23 < 2^31
    s0 = min(p * per, len);
    s1 = min(s0 + per, len);
}

// Stage 1 of both directions.  Block (p, s) takes slice p of segment s.  Thread (ty, tx) of the CW x (256 / CW) layout adds
// the rows ty, ty + RY, ... of the slice in ascending order for the four channels of column lane tx (+ CW per pass); the RY
// row lanes are then added in ascending ty by one thread per column lane.
//   BACKWARD = false: a1 = sum (x - K), a2 = sum (x - K)^2 with K = the slice's first row -> partial (mean, M2)
//   BACKWARD = true:  a1 = sum dy,      a2 = sum dy * xhat                                -> partial (S1, S2)
// partial [B][INORM_SLICES][2][C]; an empty slice writes nothing and is never read.
template <bool V4, bool BACKWARD>
__global__ __launch_bounds__(256) void inorm_partial_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                            const double *__restrict__ mean, const double *__restrict__ invstd,
                                                            int C, int CL, int CW, const long long *__restrict__ order,
                                                            const int *__restrict__ seg_start, double *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) double lds[2 * 256 * 4];
    const int p = blockIdx.x, s = blockIdx.y;
    const int begin = seg_start[s];
    const int len = seg_start[s + 1] - begin;
    int s0, s1;
    slice_of(p, len, s0, s1);
    if (s0 >= s1) return;                                              // (uniform over the workgroup)
    const int RY = 256 / CW;
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    const long long *__restrict__ ord = order + begin;
    const size_t first = (size_t)ord[s0];
    double *__restrict__ dst = partial + ((size_t)s * INORM_SLICES + p) * 2 * C;
    for (int c0 = 0; c0 < CL; c0 += CW) {                              // uniform trip count: every thread reaches the barriers
        const int cl = c0 + tx, c = 4 * cl;
        double a1[4], a2[4], k0[4], k1[4];                             // forward: k0 = the shift; backward: k0 = mean, k1 = invstd
#pragma unroll
        for (int k = 0; k < 4; k++) a1[k] = a2[k] = k0[k] = k1[k] = 0.0;
        if (cl < CL) {
            if constexpr (BACKWARD) {
                load4d(mean + (size_t)s * C, c, C, k0);
                load4d(invstd + (size_t)s * C, c, C, k1);
            } else {
                float kf[4];
                load4<V4>(x + first * C, c, C, kf);
#pragma unroll
                for (int k = 0; k < 4; k++) k0[k] = (double)kf[k];
            }
            for (int i = s0 + ty; i < s1; i += INORM_UNROLL * RY) {
                float v[INORM_UNROLL][4], g[INORM_UNROLL][4];
#pragma unroll
                for (int u = 0; u < INORM_UNROLL; u++) {
                    const int iu = i + u * RY;
                    if (iu < s1) {
                        const size_t r = (size_t)ord[iu];
                        load4<V4>(x + r * C, c, C, v[u]);
                        if constexpr (BACKWARD) load4<V4>(dy + r * C, c, C, g[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < INORM_UNROLL; u++) {
                    if (i + u * RY >= s1) continue;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if constexpr (BACKWARD) {
                            const double xhat = ((double)v[u][k] - k0[k]) * k1[k];
                            a1[k] = a1[k] + (double)g[u][k];
                            a2[k] = fma((double)g[u][k], xhat, a2[k]);
                        } else {
                            const double d = (double)v[u][k] - k0[k];
                            a1[k] = a1[k] + d;
                            a2[k] = fma(d, d, a2[k]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            lds[threadIdx.x * 4 + k] = a1[k];
            lds[1024 + threadIdx.x * 4 + k] = a2[k];
        }
        __syncthreads();
        if (ty == 0 && cl < CL) {
            double t1[4], t2[4];
#pragma unroll
            for (int k = 0; k < 4; k++) t1[k] = t2[k] = 0.0;
            for (int y = 0; y < RY; y++) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    t1[k] = t1[k] + lds[(y * CW + tx) * 4 + k];
                    t2[k] = t2[k] + lds[1024 + (y * CW + tx) * 4 + k];
                }
            }
            if constexpr (!BACKWARD) {
                const double n = (double)(s1 - s0);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double m = t1[k] / n;
                    t2[k] = fmax(t2[k] - t1[k] * m, 0.0);              // M2 about the slice mean
                    t1[k] = k0[k] + m;
                }
            }
            store4d(dst, c, C, t1);
            store4d(dst + C, c, C, t2);
        }
        __syncthreads();
    }
}

// Stage 2 forward: Chan's merge of the slice (n, mean, M2) in ascending slice order, one thread per (segment, channel)
__global__ __launch_bounds__(256) void inorm_stats_merge_kernel(const double *__restrict__ partial, int B, int C,
                                                                const int *__restrict__ seg_start, float eps,
                                                                double *__restrict__ mean, double *__restrict__ invstd)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * C) return;
    const int s = (int)(t / C), c = (int)(t - (long)s * C);
    const int len = seg_start[s + 1] - seg_start[s];
    const double *__restrict__ src = partial + (size_t)s * INORM_SLICES * 2 * C + c;
    // the running mean is kept as m0 + off with m0 = the first slice's mean: `off` is small, so that the up to 255 updates
    // round at the size of the spread of the slice means, not at the size of the mean itself
    double m0 = 0.0, off = 0.0, M2 = 0.0;
    int na = 0;
    for (int p = 0; p < INORM_SLICES; p++) {
        int s0, s1;
        slice_of(p, len, s0, s1);
        const int nb = s1 - s0;
        if (nb <= 0) continue;
        const double mb = src[(size_t)p * 2 * C], Mb = src[(size_t)p * 2 * C + C];
        if (na == 0) {
            m0 = mb;
            M2 = Mb;
        } else {
            const double n = (double)(na + nb);
            const double delta = (mb - m0) - off;
            off = off + delta * ((double)nb / n);
            M2 = M2 + Mb + delta * delta * ((double)na * (double)nb / n);
        }
        na += nb;
    }
    mean[t] = m0 + off;
    invstd[t] = 1.0 / sqrt(M2 / (double)(len > 0 ? len : 1) + (double)eps);
}

// Stage 2 backward: S[s][0][c] = S1, S[s][1][c] = S2, the slice sums added in ascending slice order
__global__ __launch_bounds__(256) void inorm_sums_merge_kernel(const double *__restrict__ partial, int B, int C,
                                                               const int *__restrict__ seg_start, double *__restrict__ S)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * C) return;
    const int s = (int)(t / C), c = (int)(t - (long)s * C);
    const int len = seg_start[s + 1] - seg_start[s];
    const double *__restrict__ src = partial + (size_t)s * INORM_SLICES * 2 * C + c;
    double t1 = 0.0, t2 = 0.0;
    for (int p = 0; p < INORM_SLICES; p++) {
        int s0, s1;
        slice_of(p, len, s0, s1);
        if (s1 <= s0) continue;
        t1 = t1 + src[(size_t)p * 2 * C];
        t2 = t2 + src[(size_t)p * 2 * C + C];
    }
    S[(size_t)s * 2 * C + c] = t1;
    S[(size_t)s * 2 * C + C + c] = t2;
}

// dbias[c] = sum_s S1[s][c], dweight[c] = sum_s S2[s][c], ascending s; one thread per channel
__global__ __launch_bounds__(256) void inorm_param_grad_kernel(const double *__restrict__ S, int B, int C,
                                                               float *__restrict__ dweight, float *__restrict__ dbias)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double t1 = 0.0, t2 = 0.0;
    for (int s = 0; s < B; s++) {
        t1 = t1 + S[(size_t)s * 2 * C + c];
        t2 = t2 + S[(size_t)s * 2 * C + C + c];
    }
    if (dbias) dbias[c] = (float)t1;
    if (dweight) dweight[c] = (float)t2;
}

// The row passes (the pattern of ms3d_bn_apply): one lane per (held row, four channels), rows where they lie.
//   BACKWARD = false: out = y;  BACKWARD = true: out = dx, S = the merged (S1, S2)
template <bool V4, bool BACKWARD>
__global__ __launch_bounds__(256) void inorm_apply_kernel(const float *__restrict__ x, const float *__restrict__ dy, long V,
                                                          int C, int CL, const int *__restrict__ seg_of_row,
                                                          const int *__restrict__ seg_start, const double *__restrict__ mean,
                                                          const double *__restrict__ invstd, const float *__restrict__ weight,
                                                          const float *__restrict__ bias, const double *__restrict__ S,
                                                          float *__restrict__ out)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= V * CL) return;
    const long r = t / CL;
    const int c = 4 * (int)(t - r * CL);
    const int s = seg_of_row[r];
    float v[4], w[4], o[4];
    double m[4], is[4];
    load4<V4>(x + (size_t)r * C, c, C, v);
    load4d(mean + (size_t)s * C, c, C, m);
    load4d(invstd + (size_t)s * C, c, C, is);
    load4_or<V4>(weight, c, C, 1.f, w);
    if constexpr (BACKWARD) {
        float g[4];
        double t1[4], t2[4];
        load4<V4>(dy + (size_t)r * C, c, C, g);
        load4d(S + (size_t)s * 2 * C, c, C, t1);
        load4d(S + (size_t)s * 2 * C + C, c, C, t2);
        const double n = (double)(seg_start[s + 1] - seg_start[s]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double xhat = ((double)v[k] - m[k]) * is[k];
            const double d = ((double)g[k] - t1[k] / n) - xhat * (t2[k] / n);
            o[k] = (float)(((double)w[k] * is[k]) * d);
        }
    } else {
        float b[4];
        load4_or<V4>(bias, c, C, 0.f, b);
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = (float)fma(((double)v[k] - m[k]) * is[k], (double)w[k], (double)b[k]);
    }
    store4<V4>(out + (size_t)r * C, c, C, o);
}

// lanes per row CL = ceil(C / 4); column lanes of a workgroup CW = the power of two >= CL, at most INORM_CW_MAX
void lanes_of(int C, int &CL, int &CW)
{
    CL = (C + 3) / 4;
    CW = 1;
    while (CW < CL && CW < INORM_CW_MAX) CW <<= 1;
}

}  // namespace

extern "C" {

int ms3d_inorm_slices(void) { return INORM_SLICES; }

size_t ms3d_inorm_workspace_bytes(int B, int C)
{
    if (B <= 0 || C < 1) return 0;
    return sizeof(double) * 2 * (size_t)B * (size_t)(INORM_SLICES + 1) * (size_t)C;
}

int ms3d_inorm_forward(const float *x, long V, int C, const long long *order, const int *seg_start, int B,
                       const int *seg_of_row, float eps, const float *weight, const float *bias, double *mean, double *invstd,
                       float *y, void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || B > 65535) return MS3D_E_UNSUPPORTED;                  // one grid row per segment
    if (V <= 0 || B <= 0) return 0;
    if (!x || !order || !seg_start || !seg_of_row || !mean || !invstd || !y || !workspace) return MS3D_E_UNSUPPORTED;
    if (ms3d_inorm_workspace_bytes(B, C) > workspace_bytes) return MS3D_E_WORKSPACE;
    int CL, CW;
    lanes_of(C, CL, CW);
    const long blocks = (V * CL + 255) / 256;
    if (V > 0x7fffffffL || blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    double *partial = (double *)workspace;
    if (((uintptr_t)partial & 7) || ((uintptr_t)mean & 7) || ((uintptr_t)invstd & 7)) return MS3D_E_UNSUPPORTED;
    const bool v4 = C % 4 == 0 && ms3d_aligned16(x, y, weight, bias);
    const dim3 grid(INORM_SLICES, (unsigned)B);
    if (v4)
        inorm_partial_kernel<true, false><<<grid, 256, 0, stream>>>(x, nullptr, nullptr, nullptr, C, CL, CW, order, seg_start,
                                                                    partial);
    else
        inorm_partial_kernel<false, false><<<grid, 256, 0, stream>>>(x, nullptr, nullptr, nullptr, C, CL, CW, order, seg_start,
                                                                     partial);
    MS3D_LAUNCH_CHECK();
    inorm_stats_merge_kernel<<<ms3d_divup((long)B * C, 256), 256, 0, stream>>>(partial, B, C, seg_start, eps, mean, invstd);
    MS3D_LAUNCH_CHECK();
    if (v4)
        inorm_apply_kernel<true, false><<<(unsigned)blocks, 256, 0, stream>>>(x, nullptr, V, C, CL, seg_of_row, seg_start, mean,
                                                                              invstd, weight, bias, nullptr, y);
    else
        inorm_apply_kernel<false, false><<<(unsigned)blocks, 256, 0, stream>>>(x, nullptr, V, C, CL, seg_of_row, seg_start, mean,
                                                                               invstd, weight, bias, nullptr, y);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_inorm_backward(const float *dy, const float *x, long V, int C, const long long *order, const int *seg_start, int B,
                        const int *seg_of_row, const double *mean, const double *invstd, const float *weight, float *dx,
                        float *dweight, float *dbias, void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || B > 65535) return MS3D_E_UNSUPPORTED;
    if (V <= 0 || B <= 0) return 0;                                     // (dweight / dbias are not written: the caller's zero)
    if (!dx && !dweight && !dbias) return 0;
    if (!dy || !x || !order || !seg_start || !seg_of_row || !mean || !invstd || !workspace) return MS3D_E_UNSUPPORTED;
    if (ms3d_inorm_workspace_bytes(B, C) > workspace_bytes) return MS3D_E_WORKSPACE;
    int CL, CW;
    lanes_of(C, CL, CW);
    const long blocks = (V * CL + 255) / 256;
    if (V > 0x7fffffffL || blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    double *partial = (double *)workspace;
    if (((uintptr_t)partial & 7) || ((uintptr_t)mean & 7) || ((uintptr_t)invstd & 7)) return MS3D_E_UNSUPPORTED;
    double *S = partial + (size_t)B * INORM_SLICES * 2 * C;             // [B][2][C] behind the slice partials
    const bool v4 = C % 4 == 0 && ms3d_aligned16(dy, x, weight, dx);
    const dim3 grid(INORM_SLICES, (unsigned)B);
    if (v4)
        inorm_partial_kernel<true, true><<<grid, 256, 0, stream>>>(x, dy, mean, invstd, C, CL, CW, order, seg_start, partial);
    else
        inorm_partial_kernel<false, true><<<grid, 256, 0, stream>>>(x, dy, mean, invstd, C, CL, CW, order, seg_start, partial);
    MS3D_LAUNCH_CHECK();
    inorm_sums_merge_kernel<<<ms3d_divup((long)B * C, 256), 256, 0, stream>>>(partial, B, C, seg_start, S);
    MS3D_LAUNCH_CHECK();
    if (dweight || dbias) {
        inorm_param_grad_kernel<<<ms3d_divup(C, 256), 256, 0, stream>>>(S, B, C, dweight, dbias);
        MS3D_LAUNCH_CHECK();
    }
    if (dx) {
        if (v4)
            inorm_apply_kernel<true, true><<<(unsigned)blocks, 256, 0, stream>>>(x, dy, V, C, CL, seg_of_row, seg_start, mean,
                                                                                 invstd, weight, nullptr, S, dx);
        else
            inorm_apply_kernel<false, true><<<(unsigned)blocks, 256, 0, stream>>>(x, dy, V, C, CL, seg_of_row, seg_start, mean,
                                                                                  invstd, weight, nullptr, S, dx);
        MS3D_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
