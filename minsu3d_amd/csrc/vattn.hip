// Per-sample voxel attention: every voxel row attends to the Q queries of its own sample, optionally through a mask -- the second
// leg of a two-way mask-transformer decoder, the mirror of csrc/qattn.hip.  x [V, C] as the manager HOLDS the rows, keys / values
// [B, Q, C], C = H * D, float32 throughout.
//
//   s[i, q, h]   = scale * <x[i, h, :], keys[b, q, h, :]>        b = seg_of_row[i], q over the queries the mask does not block
//   p            = softmax over those q (the maximum is always subtracted before exp)
//   out[i, h, :] = sum_q p * values[b, q, h, :]      lse[i, h] = m + log sum exp(s - m)       (no unblocked query: out = 0, lse = 0)
//
// mask [V, Q] (bytes, non-zero = may not attend) is the mask of qattn.hip: its rows in the CALLER's order, the mask row of a held
// row i is row_map[i] (the manager's held-to-caller index) or i itself when row_map is NULL.  Nothing of size V x Q is written.
//   forward      one (held row, head) item per group loops over the Q queries of the row's sample in ascending q, one
//                online-softmax sweep; out and lse are written by the item itself: no scratch, no partials
//   backward_x   the same sweep with p = exp(s - lse) recomputed: sum p e k, sum p k and delta = sum p e with e = <dout, v - out>
//                taken per channel before the sum (see csrc/attn_core.h for why); delta is complete when the sweep ends, so
//                dx = scale (sum p e k - delta sum p k) is finished by the item
//   backward_kv  dkeys / dvalues are sums over the rows of a sample.  A segment of CoordinateManager.batch_rows is cut into the
//                chunks of qattn.hip (SATTN_ROWS_PER_CHUNK positions of `order`, the same chunk list); a workgroup = one chunk
//                and one tile of (query, head) items walks the chunk's rows in ascending position: dv = sum p dout,
//                dk = sum p (e - delta) x, one partial per chunk; the merge kernel adds the partials of a sample in ascending
//                chunk order, applies scale to dk and writes every element of dkeys / dvalues
// No atomics of any kind, one writer per element, the same bytes on every run.
//
// Lane layout, accumulation steps and the four-row gather stages: csrc/attn_core.h.  Here an item is a (held row, head) in
// forward and backward_x and a (query, head) in backward_kv.  The keys / values of a sample are read through the cache, not
// staged in LDS: a sample's tile is Q * C * 8 bytes (100 KiB at Q = 100, C = 128, 8 MiB at the limits: no LDS holds the general
// case), the items of a workgroup are consecutive HELD rows and so need not share a sample, and every workgroup of a sample
// reads the same few rows in the same order, which is what the L2 serves best.
#include "attn_core.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int VATTN_THREADS = SATTN_THREADS;

// The score of a dot product, rounded ONCE and the same in all three passes: a plain scale * dot next to `- m` or `- lse` may be
// contracted into one fma on the unrounded product, which differs from the score the maximum and lse were made of.  A row with
// one query open would then get p = 1 + 1e-7 instead of 1, out one ulp off values, and a dx of 1e-14 where it is exactly zero.
__device__ __forceinline__ float score(float scale, float dot)
{
#pragma clang fp contract(off)
    return scale * dot;
}

// what a (held row, head) item of forward / backward_x is: its row, its head, its sample and its mask row
struct RowItem {
    bool on;
    long i;
    int h, b;
    const unsigned char *mrow;
};

__device__ __forceinline__ RowItem row_item(long item, long V, int H, int Q, const unsigned char *__restrict__ mask,
                                            const int *__restrict__ row_map, const int *__restrict__ seg_of_row)
{
    RowItem r;
    r.on = item < V * H;
    r.i = r.on ? item / H : 0;
    r.h = r.on ? (int)(item - r.i * H) : 0;
    r.b = r.on ? seg_of_row[r.i] : 0;
    r.mrow = (r.on && mask) ? mask + (row_map ? (size_t)row_map[r.i] : (size_t)r.i) * Q : nullptr;
    return r;
}

// the rows of keys / values [B * Q, C] of the queries q0 .. q0 + 3 of sample b; -1 past Q, where the mask blocks, or off
__device__ __forceinline__ void queries_of_row(const RowItem &r, int q0, int Q, long (&idx)[4])
{
#pragma unroll
    for (int u = 0; u < 4; u++)
        idx[u] = (r.on && q0 + u < Q && !(r.mrow && r.mrow[q0 + u])) ? (long)r.b * Q + q0 + u : -1;
}

// Forward.  One group: the item (i, h) = blockIdx.x * (256 / G) + group of the V * H (held row, head) items.
template <int VEC>
__global__ __launch_bounds__(VATTN_THREADS) void vattn_forward_kernel(
    const float *__restrict__ x, const float *__restrict__ keys, const float *__restrict__ values,
    const unsigned char *__restrict__ mask, const int *__restrict__ row_map, const int *__restrict__ seg_of_row, long V,
    Shape sh, float *__restrict__ out, float *__restrict__ lse)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const RowItem r = row_item((long)blockIdx.x * (VATTN_THREADS / G) + g, V, H, Q, mask, row_map, seg_of_row);
    const size_t C = (size_t)H * D, hoff = (size_t)r.h * D;
    const Item it{C, hoff, H, r.h, l, G, D};
    float qv[N], acc[N];
    load_slice<VEC>(x + (size_t)r.i * C + hoff, l, G, D, r.on, qv);
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0.f;
    float m = -INFINITY, sum = 0.f;
    for (int q0 = 0; q0 < Q; q0 += 4) {
        long idx[4];
        float kr[4][N], vr[4][N], dot[4];
        queries_of_row(r, q0, Q, idx);
        key_stage<VEC>(keys, values, idx, it, qv, kr, vr, dot);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            push_softmax(score(sh.scale, dot[u]), vr[u], m, sum, acc);
        }
    }
    const float ls = finish_softmax(m, sum, acc);
    store_slice<VEC>(out + (size_t)r.i * C + hoff, l, G, D, r.on, acc);
    if (r.on && l == 0) lse[(size_t)r.i * H + r.h] = ls;
}

// Backward for x: the forward's walk with p = exp(s - lse); delta [V][H] always, dx unless NULL.
template <int VEC>
__global__ __launch_bounds__(VATTN_THREADS) void vattn_backward_x_kernel(
    const float *__restrict__ x, const float *__restrict__ keys, const float *__restrict__ values,
    const unsigned char *__restrict__ mask, const int *__restrict__ row_map, const int *__restrict__ seg_of_row,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ dout, long V, Shape sh,
    float *__restrict__ dx, float *__restrict__ delta)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const RowItem r = row_item((long)blockIdx.x * (VATTN_THREADS / G) + g, V, H, Q, mask, row_map, seg_of_row);
    const size_t C = (size_t)H * D, hoff = (size_t)r.h * D, xrow = (size_t)r.i * C + hoff;
    const Item it{C, hoff, H, r.h, l, G, D};
    float qv[N], dov[N], ov[N], acc[N], pk[N];
    load_slice<VEC>(x + xrow, l, G, D, r.on, qv);
    load_slice<VEC>(dout + xrow, l, G, D, r.on, dov);
    load_slice<VEC>(out + xrow, l, G, D, r.on, ov);
    const float ls = r.on ? lse[(size_t)r.i * H + r.h] : 0.f;
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = pk[j] = 0.f;
    float dl = 0.f;                                                  // sum p e, ascending q
    for (int q0 = 0; q0 < Q; q0 += 4) {
        long idx[4];
        float kr[4][N], vr[4][N], dot[4], dp[4];
        queries_of_row(r, q0, Q, idx);
        key_stage<VEC>(keys, values, idx, it, qv, dov, ov, kr, vr, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            push_dq(expf(score(sh.scale, dot[u]) - ls), dp[u], kr[u], dl, acc, pk);
        }
    }
    if (r.on && l == 0) delta[(size_t)r.i * H + r.h] = dl;
    if (!dx) return;                                                 // (uniform, after the last shuffle)
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = sh.scale * fmaf(-dl, pk[j], acc[j]);
    store_slice<VEC>(dx + xrow, l, G, D, r.on, acc);
}

// Backward sweep for keys and values.  Workgroup (blockIdx.x = chunk, blockIdx.y = item tile); group g takes the item
// blockIdx.y * (256 / G) + g of the Q * H (query, head) items and walks the chunk's positions of `order` in ascending order.
// Partials: w_k [chunks][Q][C] = sum ds x (not yet scaled), w_v [chunks][Q][C] = sum p dout.
template <int VEC>
__global__ __launch_bounds__(VATTN_THREADS) void vattn_backward_kv_kernel(
    const float *__restrict__ x, const float *__restrict__ keys, const float *__restrict__ values,
    const unsigned char *__restrict__ mask, const int *__restrict__ row_map, const long long *__restrict__ order,
    const int *__restrict__ seg_start, const int *__restrict__ chunk_seg, const int *__restrict__ chunk_first,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ delta,
    const float *__restrict__ dout, Shape sh, float *__restrict__ w_k, float *__restrict__ w_v)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int item = blockIdx.y * (VATTN_THREADS / G) + g;
    const bool on = item < Q * H;
    const int q = on ? item / H : 0, h = on ? item - q * H : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const int c = blockIdx.x;
    int b;
    long p0, p1;
    chunk_range(seg_start, chunk_seg, chunk_first, c, b, p0, p1);
    const size_t krow = ((size_t)b * Q + q) * C + hoff;
    const Item it{C, hoff, H, h, l, G, D};
    float kv[N], vv[N], ak[N], av[N];
    load_slice<VEC>(keys + krow, l, G, D, on, kv);
    load_slice<VEC>(values + krow, l, G, D, on, vv);
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] = av[j] = 0.f;
    for (long r0 = p0; r0 < p1; r0 += 4) {
        bool live[4];
        size_t row[4];
        float qr[4][N], dr[4][N], dot[4], dp[4], ls[4], dl[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            live[u] = on && r0 + u < p1;
            row[u] = live[u] ? (size_t)order[r0 + u] : 0;
            if (live[u] && mask) live[u] = !mask[(row_map ? (size_t)row_map[row[u]] : row[u]) * Q + q];
        }
        query_stage<VEC>(x, dout, out, lse, delta, row, live, it, kv, vv, qr, dr, ls, dl, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!live[u]) continue;
            const float p = expf(score(sh.scale, dot[u]) - ls[u]);
            push_dkv(p, p * (dp[u] - dl[u]), dr[u], qr[u], av, ak);
        }
    }
    store_slice<VEC>(w_k + ((size_t)c * Q + q) * C + hoff, l, G, D, on, ak);
    store_slice<VEC>(w_v + ((size_t)c * Q + q) * C + hoff, l, G, D, on, av);
}

// Backward merge for keys and values.  Workgroup (blockIdx.x = sample, blockIdx.y = item tile): the partials of the sample's
// chunks added in ascending order, scale applied to dk; every element of dkeys / dvalues is written (no chunk: zero).
template <int VEC>
__global__ __launch_bounds__(VATTN_THREADS) void vattn_backward_kv_merge_kernel(
    const int *__restrict__ chunk_first, Shape sh, const float *__restrict__ w_k, const float *__restrict__ w_v,
    float *__restrict__ dkeys, float *__restrict__ dvalues)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int item = blockIdx.y * (VATTN_THREADS / G) + g;
    if (item >= Q * H) return;                                       // (no shuffle in this kernel)
    const int q = item / H, h = item - q * H, b = blockIdx.x;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const int c0 = chunk_first[b], c1 = chunk_first[b + 1];
    float ak[N], av[N];
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] = av[j] = 0.f;
    for (int c = c0; c < c1; c++) {
        float a[N], p[N];
        load_slice<VEC>(w_k + ((size_t)c * Q + q) * C + hoff, l, G, D, true, a);
        load_slice<VEC>(w_v + ((size_t)c * Q + q) * C + hoff, l, G, D, true, p);
#pragma unroll
        for (int j = 0; j < N; j++) {
            ak[j] += a[j];
            av[j] += p[j];
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] *= sh.scale;
    if (dkeys) store_slice<VEC>(dkeys + ((size_t)b * Q + q) * C + hoff, l, G, D, true, ak);
    if (dvalues) store_slice<VEC>(dvalues + ((size_t)b * Q + q) * C + hoff, l, G, D, true, av);
}

// the workgroups of a launch over the V * H (held row, head) items; 0 when they do not fit a grid
unsigned row_blocks(long V, int H, int G)
{
    const long per = VATTN_THREADS / G, blocks = (V * H + per - 1) / per;
    return blocks > 0x7fffffffL ? 0u : (unsigned)blocks;
}

}  // namespace

extern "C" {

size_t ms3d_vattn_backward_kv_ws_floats(long chunks, int Q, int H, int D)
{
    if (chunks <= 0 || Q < 1 || H < 1 || D < 1) return 0;
    return (size_t)chunks * (size_t)Q * 2 * (size_t)H * D;
}

int ms3d_vattn_forward(const float *x, const float *keys, const float *values, const unsigned char *mask, const int *row_map,
                       const int *seg_of_row, long V, int B, int Q, int H, int D, float scale, float *out, float *lse,
                       ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!sample_shape_served(V, B, Q, H, D)) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;                         // (out / lse are not written: the caller's zero)
    if (!x || !keys || !values || !seg_of_row || !out || !lse) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(x, keys, values, out);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned blocks = row_blocks(V, H, sh.G);
    if (!blocks) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, vattn_forward_kernel, blocks, VATTN_THREADS, 0, stream, x, keys, values, mask, row_map, seg_of_row, V, sh,
                out, lse);
    return 0;
}

int ms3d_vattn_backward_x(const float *x, const float *keys, const float *values, const unsigned char *mask, const int *row_map,
                          const int *seg_of_row, const float *out, const float *lse, const float *dout, long V, int B, int Q,
                          int H, int D, float scale, float *dx, float *delta, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!sample_shape_served(V, B, Q, H, D)) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;
    if (!x || !keys || !values || !seg_of_row || !out || !lse || !dout || !delta) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(x, keys, values, out, dout, dx);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned blocks = row_blocks(V, H, sh.G);
    if (!blocks) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, vattn_backward_x_kernel, blocks, VATTN_THREADS, 0, stream, x, keys, values, mask, row_map, seg_of_row, out,
                lse, dout, V, sh, dx, delta);
    return 0;
}

int ms3d_vattn_backward_kv(const float *x, const float *keys, const float *values, const unsigned char *mask, const int *row_map,
                           const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first,
                           const float *out, const float *lse, const float *delta, const float *dout, long V, int B, int chunks,
                           int Q, int H, int D, float scale, float *dkeys, float *dvalues, float *ws, size_t ws_floats,
                           ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!sample_shape_served(V, B, Q, H, D) || chunks < 0) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;                         // (dkeys / dvalues are not written: the caller's zero)
    if (!x || !keys || !values || !order || !seg_start || !chunk_first || !out || !lse || !delta || !dout || (!dkeys && !dvalues))
        return MS3D_E_UNSUPPORTED;
    if (chunks > 0 && (!chunk_seg || !ws)) return MS3D_E_UNSUPPORTED;
    if (ws_floats < ms3d_vattn_backward_kv_ws_floats(chunks, Q, H, D)) return MS3D_E_WORKSPACE;
    const size_t nacc = (size_t)chunks * Q * H * D;
    float *w_k = ws, *w_v = ws + nacc;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(x, keys, values, out, dout, dkeys, dvalues, ws);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned tiles = item_tiles(Q, H, sh.G);
    if (!tiles) return MS3D_E_UNSUPPORTED;
    if (chunks > 0) {
        const dim3 grid((unsigned)chunks, tiles);
        MS3D_LAUNCH_VEC(v4, vattn_backward_kv_kernel, grid, VATTN_THREADS, 0, stream, x, keys, values, mask, row_map, order,
                    seg_start, chunk_seg, chunk_first, out, lse, delta, dout, sh, w_k, w_v);
    }
    const dim3 mgrid((unsigned)B, tiles);
    MS3D_LAUNCH_VEC(v4, vattn_backward_kv_merge_kernel, mgrid, VATTN_THREADS, 0, stream, chunk_first, sh, w_k, w_v, dkeys, dvalues);
    return 0;
}

}  // extern "C"
