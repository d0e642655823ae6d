// Pooling and weighted sums over a neighbour index (ME.neighbor_pool / neighbor_sum / knn_interpolate), with gradients.
// idx [N][k] names, per query, k rows of x [V][C] as they are held, or < 0 for "no neighbour" in any slot.
//
// Every direction is a GATHER with a single writer per output element, as in field.hip: no float atomics, the same bytes on
// every run.
//   pool forward      out[n]   = max | avg | sum over the valid slots of x[idx[n][j]] in ascending j; max saves the winning slot
//                                as arg uint8 [N][C] (255: the query has no valid slot)
//   wsum forward      out[n]   = sum_j w[n][j] * x[idx[n][j]]                 one fmaf per valid slot, ascending j, from 0
//   feature backward  dx[v]    = sum over the entries e = n * k + j of row v, ascending e, of
//                                dout[n] | dout[n] / float(valid[n]) | w[e] * dout[n] (one fmaf) | dout[n][c] where arg[n][c] == j
//                                (entry_sorted / seg_start: a stable sort of the index by row, built once per map by the caller)
//   weight backward   dw[n][j] = <dout[n], x[idx[n][j]]>, 0 for an invalid slot
// Layout: csrc/rows.h.
//
// Long rows.  Carrying M picks back to all rows gives the feature backward few destinations with hundreds of entries each, so a
// row of more than MS3D_NBR_CHUNK entries is cut into chunks of that many: a thread group per chunk sums it, in the same ascending
// order, into a partial in the workspace, and the row's thread group adds the partials in chunk order.  chunk_start int32 [V + 1]
// counts the chunks of the rows that have more than one (the others count 0), so a row of at most one chunk is the plain chain
// and never touches the workspace.
#include "rows.h"
#include "../../include/minsu3d_hip.h"

#ifndef MS3D_NBR_CHUNK
#define MS3D_NBR_CHUNK 128
#endif

namespace {

using namespace ms3d_rows;

enum { NBR_MAX = 0, NBR_AVG = 1, NBR_SUM = 2, NBR_WEIGHTED = 3 };
#define NBR_MODES (NBR_MAX, NBR_AVG, NBR_SUM, NBR_WEIGHTED)       // the modes of the backward; the pooling forward has the first three

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void nbr_pool_forward_kernel(const float *__restrict__ x, const long long *__restrict__ idx,
                                                               int N, int k, int C, int CV, float *__restrict__ out,
                                                               unsigned char *__restrict__ arg)
{
    MS3D_ROW_LANE(N, CV, n, cv);
    float acc[VEC];
    int win[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) { acc[c] = 0.f; win[c] = 255; }
    const long long *row = idx + (size_t)n * k;
    int seen = 0;
#pragma unroll 4
    for (int j = 0; j < k; j++) {
        const long long r = row[j];
        if (r < 0) continue;
        float f[VEC];
        load_row<VEC>(x, (size_t)r, C, cv, f);
#pragma unroll
        for (int c = 0; c < VEC; c++) {
            if constexpr (MODE == NBR_MAX) {
                if (seen == 0 || f[c] > acc[c]) { acc[c] = f[c]; win[c] = j; }
            } else {
                acc[c] += f[c];
            }
        }
        seen++;
    }
    if constexpr (MODE == NBR_AVG) {
        if (seen > 0) {
            const float cnt = (float)seen;
#pragma unroll
            for (int c = 0; c < VEC; c++) acc[c] = acc[c] / cnt;
        }
    }
    store_row<VEC>(out, (size_t)n, C, cv, acc);
    if constexpr (MODE == NBR_MAX) store_arg<VEC>(arg, (size_t)n, C, cv, win);
}

template <int VEC>
__global__ __launch_bounds__(256) void nbr_wsum_forward_kernel(const float *__restrict__ x, const long long *__restrict__ idx,
                                                               const float *__restrict__ w, int N, int k, int C, int CV,
                                                               float *__restrict__ out)
{
    MS3D_ROW_LANE(N, CV, n, cv);
    float acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) acc[c] = 0.f;
    const long long *row = idx + (size_t)n * k;
    const float *wrow = w + (size_t)n * k;
#pragma unroll 4
    for (int j = 0; j < k; j++) {
        const long long r = row[j];
        if (r < 0) continue;                     // (the weight of an invalid slot is never read)
        const float wj = wrow[j];
        float f[VEC];
        load_row<VEC>(x, (size_t)r, C, cv, f);
#pragma unroll
        for (int c = 0; c < VEC; c++) acc[c] = fmaf(wj, f[c], acc[c]);
    }
    store_row<VEC>(out, (size_t)n, C, cv, acc);
}

// the addend of entry e for the channels of lane cv -> g, and for NBR_WEIGHTED its factor; false: the entry names no query
template <int MODE, int VEC>
__device__ __forceinline__ bool nbr_addend(long long e, const float *__restrict__ dout, const float *__restrict__ w,
                                           const unsigned char *__restrict__ arg, const int *__restrict__ valid, int N, int k,
                                           int C, int cv, float (&g)[VEC], float &factor)
{
    factor = 1.f;
    if (e < 0 || e >= (long long)N * k) return false;
    const int n = (int)e / k, j = (int)e - n * k;
    load_row<VEC>(dout, (size_t)n, C, cv, g);
    if constexpr (MODE == NBR_AVG) {
        const float cnt = (float)valid[n];      // >= 1: this entry is a valid slot of query n
#pragma unroll
        for (int c = 0; c < VEC; c++) g[c] = g[c] / cnt;
    } else if constexpr (MODE == NBR_WEIGHTED) {
        factor = w[e];
    } else if constexpr (MODE == NBR_MAX) {
        int a[VEC];
        load_arg<VEC>(arg, (size_t)n, C, cv, a);
#pragma unroll
        for (int c = 0; c < VEC; c++) g[c] = (a[c] == j) ? g[c] : 0.f;
    }
    return true;
}

// the chain over entry_sorted[begin .. end) in ascending position; four entries are fetched ahead of their additions
template <int MODE, int VEC>
__device__ __forceinline__ void nbr_chain(int begin, int end, const long long *__restrict__ entry_sorted,
                                          const float *__restrict__ dout, const float *__restrict__ w,
                                          const unsigned char *__restrict__ arg, const int *__restrict__ valid, int N, int k, int C,
                                          int cv, float (&acc)[VEC])
{
    for (int s = begin; s < end; s += 4) {
        float g[4][VEC], factor[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ok[u] = s + u < end;
            if (ok[u]) ok[u] = nbr_addend<MODE, VEC>(entry_sorted[s + u], dout, w, arg, valid, N, k, C, cv, g[u], factor[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!ok[u]) continue;
#pragma unroll
            for (int c = 0; c < VEC; c++) {
                if constexpr (MODE == NBR_WEIGHTED) acc[c] = fmaf(factor[u], g[u][c], acc[c]);
                else acc[c] += g[u][c];
            }
        }
    }
}

// one thread group per chunk of a long row: partial[chunk] = the chain over the chunk's entries
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void nbr_backward_chunk_kernel(const float *__restrict__ dout, const float *__restrict__ w,
                                                                 const unsigned char *__restrict__ arg,
                                                                 const int *__restrict__ valid,
                                                                 const long long *__restrict__ entry_sorted,
                                                                 const int *__restrict__ seg_start,
                                                                 const int *__restrict__ chunk_start, int n_chunks, int V, int N,
                                                                 int k, int C, int CV, float *__restrict__ partial)
{
    MS3D_ROW_LANE(n_chunks, CV, q, cv);
    int lo = 0, hi = V;                          // the last row v with chunk_start[v] <= q owns chunk q
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
        const int mid = lo + ((hi - lo) >> 1);
        if (chunk_start[mid] <= q) lo = mid; else hi = mid;
    }
    const int first = seg_start[lo], last = seg_start[lo + 1];
    const long b = (long)first + (long)(q - chunk_start[lo]) * MS3D_NBR_CHUNK;
    const int begin = (int)(b < last ? b : last);
    const int end = last - begin > MS3D_NBR_CHUNK ? begin + MS3D_NBR_CHUNK : last;
    float acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) acc[c] = 0.f;
    if (begin >= first) nbr_chain<MODE, VEC>(begin, end, entry_sorted, dout, w, arg, valid, N, k, C, cv, acc);
    store_row<VEC>(partial, (size_t)q, C, cv, acc);
}

// one thread group per row: the plain chain, or the partials of a long row in chunk order
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void nbr_backward_row_kernel(const float *__restrict__ dout, const float *__restrict__ w,
                                                               const unsigned char *__restrict__ arg, const int *__restrict__ valid,
                                                               const long long *__restrict__ entry_sorted,
                                                               const int *__restrict__ seg_start, const int *__restrict__ chunk_start,
                                                               int n_chunks, const float *__restrict__ partial, int V, int N,
                                                               int k, int C, int CV, float *__restrict__ dx)
{
    MS3D_ROW_LANE(V, CV, v, cv);
    float acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) acc[c] = 0.f;
    int c0 = chunk_start[v], c1 = chunk_start[v + 1];
    if (c1 > n_chunks) c1 = n_chunks;            // (the workspace holds n_chunks partials: nothing beyond them is read)
    if (c0 < 0) c0 = c1;
    if (c1 > c0) {
        for (int q = c0; q < c1; q++) {
            float p[VEC];
            load_row<VEC>(partial, (size_t)q, C, cv, p);
#pragma unroll
            for (int c = 0; c < VEC; c++) acc[c] += p[c];
        }
    } else {
        nbr_chain<MODE, VEC>(seg_start[v], seg_start[v + 1], entry_sorted, dout, w, arg, valid, N, k, C, cv, acc);
    }
    store_row<VEC>(dx, (size_t)v, C, cv, acc);
}

// one wave per query: lane l sums the channels l, l + 64, ... in ascending order, then the 64 lane sums are folded by xor
// shuffles over 32, 16, ... 1 -- an order fixed by C alone
__global__ __launch_bounds__(256) void nbr_wsum_backward_w_kernel(const float *__restrict__ dout, const float *__restrict__ x,
                                                                  const long long *__restrict__ idx, int N, int k, int C,
                                                                  float *__restrict__ dw)
{
    const long n = (long)blockIdx.x * 4 + wave_id();
    if (n >= N) return;                          // (the same for all lanes of a wave)
    const int l = lane_id();
    const float *g = dout + (size_t)n * C;
    for (int j = 0; j < k; j++) {
        const long long r = idx[(size_t)n * k + j];
        float s = 0.f;
        if (r >= 0) {
            const float *f = x + (size_t)r * C;
            for (int c = l; c < C; c += 64) s = fmaf(g[c], f[c], s);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (l == 0) dw[(size_t)n * k + j] = s;
    }
}

bool nbr_shape(long V, long N, int k, int C)
{
    return C >= 1 && k >= 1 && k <= 254 && V >= 0 && V <= 0x7fffffffL && N >= 0 && N <= 0x7fffffffL / k;
}

}  // namespace

extern "C" {

int ms3d_nbr_chunk_entries(void) { return MS3D_NBR_CHUNK; }

size_t ms3d_nbr_ws_bytes(long n_chunks, int C)
{
    return n_chunks > 0 && C >= 1 ? (size_t)n_chunks * (size_t)C * sizeof(float) : 0;
}

int ms3d_nbr_pool_forward(int mode, const float *x, long V, const long long *idx, long N, int k, int C, float *out,
                          unsigned char *arg, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < NBR_MAX || mode > NBR_SUM || !nbr_shape(V, N, k, C)) return MS3D_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!idx || !out || (V > 0 && !x) || (mode == NBR_MAX && !arg)) return MS3D_E_UNSUPPORTED;
    const bool v4 = vec4(C, x, out) && (mode != NBR_MAX || arg_aligned4(arg));
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(N, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_MODE_VEC((NBR_MAX, NBR_AVG, NBR_SUM), mode, v4, nbr_pool_forward_kernel, blocks, 256, 0, stream, x, idx, (int)N, k,
                         C, CV, out, arg);
    return 0;
}

int ms3d_nbr_wsum_forward(const float *x, long V, const long long *idx, const float *w, long N, int k, int C, float *out,
                          ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!nbr_shape(V, N, k, C)) return MS3D_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!idx || !w || !out || (V > 0 && !x)) return MS3D_E_UNSUPPORTED;
    const bool v4 = vec4(C, x, out);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(N, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, nbr_wsum_forward_kernel, blocks, 256, 0, stream, x, idx, w, (int)N, k, C, CV, out);
    return 0;
}

int ms3d_nbr_backward(int mode, const float *dout, const float *w, const unsigned char *arg, const int *valid,
                      const long long *entry_sorted, const int *seg_start, const int *chunk_start, long n_chunks, long V, long N,
                      int k, int C, float *dx, void *ws, size_t ws_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < NBR_MAX || mode > NBR_WEIGHTED || !nbr_shape(V, N, k, C) || n_chunks < 0 || n_chunks > 0x7fffffffL)
        return MS3D_E_UNSUPPORTED;
    if (V == 0) return 0;
    if (!seg_start || !chunk_start || !dx) return MS3D_E_UNSUPPORTED;
    if (N > 0 && (!dout || !entry_sorted || (mode == NBR_WEIGHTED && !w) || (mode == NBR_MAX && !arg) || (mode == NBR_AVG && !valid)))
        return MS3D_E_UNSUPPORTED;
    if (n_chunks > 0 && (!ws || !ms3d_aligned16(ws))) return MS3D_E_UNSUPPORTED;
    if (ws_bytes < ms3d_nbr_ws_bytes(n_chunks, C)) return MS3D_E_WORKSPACE;
    float *partial = (float *)ws;
    const bool v4 = vec4(C, dout, dx) && (mode != NBR_MAX || arg_aligned4(arg));
    const int CV = v4 ? C / 4 : C;
    unsigned blocks, cblocks = 0;
    if (!grid_of(V, CV, &blocks) || !grid_of(n_chunks, CV, &cblocks)) return MS3D_E_UNSUPPORTED;
    if (n_chunks > 0)
        MS3D_LAUNCH_MODE_VEC(NBR_MODES, mode, v4, nbr_backward_chunk_kernel, cblocks, 256, 0, stream, dout, w, arg, valid,
                             entry_sorted, seg_start, chunk_start, (int)n_chunks, (int)V, (int)N, k, C, CV, partial);
    MS3D_LAUNCH_MODE_VEC(NBR_MODES, mode, v4, nbr_backward_row_kernel, blocks, 256, 0, stream, dout, w, arg, valid, entry_sorted,
                         seg_start, chunk_start, (int)n_chunks, partial, (int)V, (int)N, k, C, CV, dx);
    return 0;
}

int ms3d_nbr_wsum_backward_w(const float *dout, const float *x, const long long *idx, long N, int k, int C, float *dw,
                             ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!nbr_shape(0, N, k, C)) return MS3D_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!dout || !x || !idx || !dw) return MS3D_E_UNSUPPORTED;
    nbr_wsum_backward_w_kernel<<<(unsigned)((N + 3) / 4), 256, 0, stream>>>(dout, x, idx, (int)N, k, C, dw);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
