// Per-sample query attention: Q queries per sample attend to every voxel row of that sample, optionally through a mask -- the
// decoder step of a mask transformer.  queries [B, Q, C], k / v [V, C] as the manager HOLDS them, C = H * D, float32 throughout.
//
//   s[b, q, i, h] = scale * <queries[b, q, h, :], k[i, h, :]>           i over the rows of sample b the mask does not block
//   p             = softmax over those i (the maximum is always subtracted before exp)
//   out[b, q, h, :] = sum_i p * v[i, h, :]      lse[b, q, h] = m + log sum exp(s - m)     (no unblocked row: out = 0, lse = 0)
//
// The rows of sample b are order[seg_start[b] .. seg_start[b + 1]) (CoordinateManager.batch_rows); they are read by index where
// they lie.  mask [V, Q] (bytes, non-zero = may not attend) is in the CALLER's row order: the mask row of a held row i is
// row_map[i] (the manager's held-to-caller index) or i itself when row_map is NULL.  Nothing of size V x Q is written.
//
// A segment is cut into chunks of QATTN_ROWS_PER_CHUNK consecutive positions of `order` -- a constant of the library, so the
// order of every sum depends on the shapes only.  The chunk list (chunk_seg [chunks]: the sample of a chunk; chunk_first
// [B + 1]: the first chunk of a sample) is sorted by sample, then by run; ms3d_qattn_chunk_list makes it on the host.
//   forward      a workgroup = one chunk and one tile of (query, head) items: one online-softmax sweep over the chunk's rows in
//                ascending position, a partial (m, l, acc[D]) per item; the merge kernel folds the partials of a sample in
//                ascending chunk order and writes out and lse
//   backward_q   the same sweep with p = exp(s - lse) recomputed: per chunk sum p e k, sum p k and sum p e with
//                e = <dout, v - out> taken per channel before the sum (see csrc/attn_core.h for why); the merge adds the chunks in
//                ascending order, delta[b, q, h] = sum_i p e, dq = scale (sum p e k - delta sum p k)
//   backward_kv  one (row, head) item per voxel row loops over the Q queries of its sample in ascending q: dv = sum p dout,
//                dk = scale sum p (e - delta) q; one writer per element, no partials
// No atomics of any kind, one writer per element, the same bytes on every run.
//
// Lane layout, accumulation steps and the four-row gather stages: csrc/attn_core.h.  Here an item is a (query, head) in the
// sweeps and a (held row, head) in backward_kv; every group of a sweep's workgroup walks the same rows, so they come from the
// cache.
#include "attn_core.h"
#include "../../include/minsu3d_hip.h"

namespace {

// the limits, the chunk size, Shape and chunk_range are attn_core.h's, shared with csrc/vattn.hip
constexpr int QATTN_MAX_B = SATTN_MAX_B;
constexpr int QATTN_THREADS = SATTN_THREADS;
constexpr int QATTN_ROWS_PER_CHUNK = SATTN_ROWS_PER_CHUNK;

// the held rows at the positions r0 .. r0 + 3 of `order` that query q may attend to; -1 past p1, where the mask blocks, or off
__device__ __forceinline__ void rows_of_query(const long long *__restrict__ order, const unsigned char *__restrict__ mask,
                                              const int *__restrict__ row_map, long r0, long p1, bool on, int Q, int q,
                                              long (&idx)[4])
{
#pragma unroll
    for (int u = 0; u < 4; u++) {
        idx[u] = (on && r0 + u < p1) ? (long)order[r0 + u] : -1;
        if (idx[u] >= 0 && mask) {
            const size_t mr = row_map ? (size_t)row_map[idx[u]] : (size_t)idx[u];
            if (mask[mr * Q + q]) idx[u] = -1;
        }
    }
}

// Forward sweep.  Workgroup (blockIdx.x = chunk, blockIdx.y = item tile); group g takes the item blockIdx.y * (256 / G) + g of
// the Q * H (query, head) items.  Partials: acc [chunks][Q][C] (not normalised), m and l [chunks][Q * H].
template <int VEC>
__global__ __launch_bounds__(QATTN_THREADS) void qattn_forward_kernel(
    const float *__restrict__ queries, const float *__restrict__ k, const float *__restrict__ v,
    const unsigned char *__restrict__ mask, const int *__restrict__ row_map, const long long *__restrict__ order,
    const int *__restrict__ seg_start, const int *__restrict__ chunk_seg, const int *__restrict__ chunk_first, Shape sh,
    float *__restrict__ w_acc, float *__restrict__ w_m, float *__restrict__ w_l)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int item = blockIdx.y * (QATTN_THREADS / G) + g;
    const bool on = item < Q * H;
    const int q = on ? item / H : 0, h = on ? item - q * H : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const int c = blockIdx.x;
    int b;
    long p0, p1;
    chunk_range(seg_start, chunk_seg, chunk_first, c, b, p0, p1);
    const Item it{C, hoff, H, h, l, G, D};
    float qv[N], acc[N];
    load_slice<VEC>(queries + ((size_t)b * Q + q) * C + hoff, l, G, D, on, qv);
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0.f;
    float m = -INFINITY, sum = 0.f;
    for (long r0 = p0; r0 < p1; r0 += 4) {
        long idx[4];
        float kr[4][N], vr[4][N], dot[4];
        rows_of_query(order, mask, row_map, r0, p1, on, Q, q, idx);
        key_stage<VEC>(k, v, idx, it, qv, kr, vr, dot);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            push_softmax(sh.scale * dot[u], vr[u], m, sum, acc);
        }
    }
    store_slice<VEC>(w_acc + ((size_t)c * Q + q) * C + hoff, l, G, D, on, acc);
    if (on && l == 0) {
        w_m[(size_t)c * Q * H + item] = m;
        w_l[(size_t)c * Q * H + item] = sum;
    }
}

// Forward merge.  Workgroup (blockIdx.x = sample, blockIdx.y = item tile): the partials of the sample's chunks in ascending
// order, rescaled to the largest maximum.  One chunk: the weight is exp(0) = 1, nothing is rounded twice.
template <int VEC>
__global__ __launch_bounds__(QATTN_THREADS) void qattn_forward_merge_kernel(
    const int *__restrict__ chunk_first, Shape sh, const float *__restrict__ w_acc, const float *__restrict__ w_m,
    const float *__restrict__ w_l, float *__restrict__ out, float *__restrict__ lse)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int item = blockIdx.y * (QATTN_THREADS / G) + g;
    if (item >= Q * H) return;                                       // (no shuffle in this kernel)
    const int q = item / H, h = item - q * H, b = blockIdx.x;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D, QH = (size_t)Q * H;
    const int c0 = chunk_first[b], c1 = chunk_first[b + 1];
    float M = -INFINITY;
    for (int c = c0; c < c1; c++) M = fmaxf(M, w_m[(size_t)c * QH + item]);
    float acc[N], sum = 0.f;
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0.f;
    if (M > -INFINITY) {
        for (int c = c0; c < c1; c++) {
            const float mc = w_m[(size_t)c * QH + item];
            if (!(mc > -INFINITY)) continue;                         // a chunk whose rows are all blocked for this query
            const float w = expf(mc - M);
            float a[N];
            load_slice<VEC>(w_acc + ((size_t)c * Q + q) * C + hoff, l, G, D, true, a);
            sum = fmaf(w_l[(size_t)c * QH + item], w, sum);
#pragma unroll
            for (int j = 0; j < N; j++) acc[j] = fmaf(a[j], w, acc[j]);
        }
    }
    const float ls = finish_softmax(M, sum, acc);
    store_slice<VEC>(out + ((size_t)b * Q + q) * C + hoff, l, G, D, true, acc);
    if (l == 0) lse[(size_t)b * QH + item] = ls;
}

// Backward sweep for the queries: the forward's walk with p = exp(s - lse).  Partials: w_a [chunks][Q][C] = sum p e k,
// w_p [chunks][Q][C] = sum p k (both only when `rows`), w_d [chunks][Q * H] = sum p e.
template <int VEC>
__global__ __launch_bounds__(QATTN_THREADS) void qattn_backward_q_kernel(
    const float *__restrict__ queries, const float *__restrict__ k, const float *__restrict__ v,
    const unsigned char *__restrict__ mask, const int *__restrict__ row_map, const long long *__restrict__ order,
    const int *__restrict__ seg_start, const int *__restrict__ chunk_seg, const int *__restrict__ chunk_first,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ dout, Shape sh, int rows,
    float *__restrict__ w_a, float *__restrict__ w_p, float *__restrict__ w_d)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int item = blockIdx.y * (QATTN_THREADS / G) + g;
    const bool on = item < Q * H;
    const int q = on ? item / H : 0, h = on ? item - q * H : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const int c = blockIdx.x;
    int b;
    long p0, p1;
    chunk_range(seg_start, chunk_seg, chunk_first, c, b, p0, p1);
    const size_t qrow = ((size_t)b * Q + q) * C + hoff;
    const Item it{C, hoff, H, h, l, G, D};
    float qv[N], dov[N], ov[N], acc[N], pk[N];
    load_slice<VEC>(queries + qrow, l, G, D, on, qv);
    load_slice<VEC>(dout + qrow, l, G, D, on, dov);
    load_slice<VEC>(out + qrow, l, G, D, on, ov);
    const float ls = on ? lse[(size_t)b * Q * H + item] : 0.f;
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = pk[j] = 0.f;
    float dl = 0.f;                                                  // sum p e, ascending position
    for (long r0 = p0; r0 < p1; r0 += 4) {
        long idx[4];
        float kr[4][N], vr[4][N], dot[4], dp[4];
        rows_of_query(order, mask, row_map, r0, p1, on, Q, q, idx);
        key_stage<VEC>(k, v, idx, it, qv, dov, ov, kr, vr, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            push_dq(expf(sh.scale * dot[u] - ls), dp[u], kr[u], dl, acc, pk);
        }
    }
    if (rows) {
        store_slice<VEC>(w_a + ((size_t)c * Q + q) * C + hoff, l, G, D, on, acc);
        store_slice<VEC>(w_p + ((size_t)c * Q + q) * C + hoff, l, G, D, on, pk);
    }
    if (on && l == 0) w_d[(size_t)c * Q * H + item] = dl;
}

// Backward merge for the queries: the chunks of a sample added in ascending order; delta = sum p e,
// dq = scale (sum p e k - delta sum p k) (dq NULL: delta alone).
template <int VEC>
__global__ __launch_bounds__(QATTN_THREADS) void qattn_backward_q_merge_kernel(
    const int *__restrict__ chunk_first, Shape sh, const float *__restrict__ w_a, const float *__restrict__ w_p,
    const float *__restrict__ w_d, float *__restrict__ dq, float *__restrict__ delta)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int item = blockIdx.y * (QATTN_THREADS / G) + g;
    if (item >= Q * H) return;                                       // (no shuffle in this kernel)
    const int q = item / H, h = item - q * H, b = blockIdx.x;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D, QH = (size_t)Q * H;
    const int c0 = chunk_first[b], c1 = chunk_first[b + 1];
    float dl = 0.f;
    for (int c = c0; c < c1; c++) dl += w_d[(size_t)c * QH + item];
    if (l == 0) delta[(size_t)b * QH + item] = dl;
    if (!dq) return;
    float acc[N], pk[N];
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = pk[j] = 0.f;
    for (int c = c0; c < c1; c++) {
        float a[N], p[N];
        load_slice<VEC>(w_a + ((size_t)c * Q + q) * C + hoff, l, G, D, true, a);
        load_slice<VEC>(w_p + ((size_t)c * Q + q) * C + hoff, l, G, D, true, p);
#pragma unroll
        for (int j = 0; j < N; j++) {
            acc[j] += a[j];
            pk[j] += p[j];
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = sh.scale * fmaf(-dl, pk[j], acc[j]);
    store_slice<VEC>(dq + ((size_t)b * Q + q) * C + hoff, l, G, D, true, acc);
}

// Backward for k and v.  One group: the item (i, h) = blockIdx.x * (256 / G) + group of the V * H (held row, head) items; the
// Q queries of the row's sample seg_of_row[i] in ascending q, four at a time.
template <int VEC>
__global__ __launch_bounds__(QATTN_THREADS) void qattn_backward_kv_kernel(
    const float *__restrict__ queries, const float *__restrict__ k, const float *__restrict__ v,
    const unsigned char *__restrict__ mask, const int *__restrict__ row_map, const int *__restrict__ seg_of_row,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ delta,
    const float *__restrict__ dout, long V, Shape sh, float *__restrict__ dk, float *__restrict__ dv)
{
    constexpr int N = Lane<VEC>::N;
    const int Q = sh.Q, H = sh.H, D = sh.D, G = sh.G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * (QATTN_THREADS / G) + g;
    const bool on = item < V * H;
    const long i = on ? item / H : 0;
    const int h = on ? (int)(item - i * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const int b = on ? seg_of_row[i] : 0;
    const unsigned char *__restrict__ mrow =
        (on && mask) ? mask + (row_map ? (size_t)row_map[i] : (size_t)i) * Q : nullptr;
    const Item it{C, hoff, H, h, l, G, D};
    float kv[N], vv[N], ak[N], av[N];
    load_slice<VEC>(k + (size_t)i * C + hoff, l, G, D, on, kv);
    load_slice<VEC>(v + (size_t)i * C + hoff, l, G, D, on, vv);
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] = av[j] = 0.f;
    for (int q0 = 0; q0 < Q; q0 += 4) {
        bool live[4];
        size_t qh[4];
        float qr[4][N], dr[4][N], dot[4], dp[4], ls[4], dl[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            live[u] = on && q0 + u < Q && !(mrow && mrow[q0 + u]);
            qh[u] = (size_t)b * Q + (live[u] ? q0 + u : 0);
        }
        query_stage<VEC>(queries, dout, out, lse, delta, qh, live, it, kv, vv, qr, dr, ls, dl, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!live[u]) continue;
            const float p = expf(sh.scale * dot[u] - ls[u]);
            push_dkv(p, p * (dp[u] - dl[u]), dr[u], qr[u], av, ak);
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] *= sh.scale;
    if (dk) store_slice<VEC>(dk + (size_t)i * C + hoff, l, G, D, on, ak);
    if (dv) store_slice<VEC>(dv + (size_t)i * C + hoff, l, G, D, on, av);
}

}  // namespace

extern "C" {

int ms3d_qattn_rows_per_chunk(void) { return QATTN_ROWS_PER_CHUNK; }

long ms3d_qattn_chunks(const int *seg_start, int B)
{
    if (!seg_start || B <= 0) return 0;
    long n = 0;
    for (int b = 0; b < B; b++) {
        const long len = (long)seg_start[b + 1] - seg_start[b];
        if (len > 0) n += (len + QATTN_ROWS_PER_CHUNK - 1) / QATTN_ROWS_PER_CHUNK;
    }
    return n;
}

int ms3d_qattn_chunk_list(const int *seg_start, int B, int *chunk_seg, int *chunk_first)
{
    if (B < 0 || B > QATTN_MAX_B || !chunk_first || (B > 0 && !seg_start)) return MS3D_E_UNSUPPORTED;
    const long total = ms3d_qattn_chunks(seg_start, B);
    if (total > 0x7fffffffL || (total > 0 && !chunk_seg)) return MS3D_E_UNSUPPORTED;
    int n = 0;
    for (int b = 0; b < B; b++) {
        chunk_first[b] = n;
        const long len = (long)seg_start[b + 1] - seg_start[b];
        const int runs = len > 0 ? (int)((len + QATTN_ROWS_PER_CHUNK - 1) / QATTN_ROWS_PER_CHUNK) : 0;
        for (int j = 0; j < runs; j++) chunk_seg[n++] = b;
    }
    chunk_first[B] = n;
    return 0;
}

size_t ms3d_qattn_ws_floats(long chunks, int Q, int H, int D)
{
    if (chunks <= 0 || Q < 1 || H < 1 || D < 1) return 0;
    return (size_t)chunks * (size_t)Q * ((size_t)H * D + 2 * (size_t)H);
}

size_t ms3d_qattn_backward_ws_floats(long chunks, int Q, int H, int D)
{
    if (chunks <= 0 || Q < 1 || H < 1 || D < 1) return 0;
    return (size_t)chunks * (size_t)Q * (2 * (size_t)H * D + (size_t)H);
}

int ms3d_qattn_forward(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                       const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first, long V, int B,
                       int chunks, int Q, int H, int D, float scale, float *out, float *lse, float *ws, size_t ws_floats,
                       ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!sample_shape_served(V, B, Q, H, D) || chunks < 0) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;
    if (!queries || !k || !v || !order || !seg_start || !chunk_first || !out || !lse) return MS3D_E_UNSUPPORTED;
    if (chunks > 0 && (!chunk_seg || !ws)) return MS3D_E_UNSUPPORTED;
    if (ws_floats < ms3d_qattn_ws_floats(chunks, Q, H, D)) return MS3D_E_WORKSPACE;
    const size_t C = (size_t)H * D, nacc = (size_t)chunks * Q * C, nqh = (size_t)chunks * Q * H;
    float *w_acc = ws, *w_m = ws + nacc, *w_l = ws + nacc + nqh;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(queries, k, v, out, ws);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned tiles = item_tiles(Q, H, sh.G);
    if (!tiles) return MS3D_E_UNSUPPORTED;
    if (chunks > 0) {
        const dim3 grid((unsigned)chunks, tiles);
        MS3D_LAUNCH_VEC(v4, qattn_forward_kernel, grid, QATTN_THREADS, 0, stream, queries, k, v, mask, row_map, order, seg_start,
                    chunk_seg, chunk_first, sh, w_acc, w_m, w_l);
    }
    const dim3 mgrid((unsigned)B, tiles);
    MS3D_LAUNCH_VEC(v4, qattn_forward_merge_kernel, mgrid, QATTN_THREADS, 0, stream, chunk_first, sh, w_acc, w_m, w_l, out, lse);
    return 0;
}

int ms3d_qattn_backward_q(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                          const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first,
                          const float *out, const float *lse, const float *dout, long V, int B, int chunks, int Q, int H, int D,
                          float scale, float *dq, float *delta, float *ws, size_t ws_floats, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!sample_shape_served(V, B, Q, H, D) || chunks < 0) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;
    if (!queries || !k || !v || !order || !seg_start || !chunk_first || !out || !lse || !dout || !delta)
        return MS3D_E_UNSUPPORTED;
    if (chunks > 0 && (!chunk_seg || !ws)) return MS3D_E_UNSUPPORTED;
    if (ws_floats < ms3d_qattn_backward_ws_floats(chunks, Q, H, D)) return MS3D_E_WORKSPACE;
    const size_t C = (size_t)H * D, nacc = (size_t)chunks * Q * C;
    float *w_a = ws, *w_p = ws + nacc, *w_d = ws + 2 * nacc;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(queries, k, v, out, dout, ws, dq);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned tiles = item_tiles(Q, H, sh.G);
    if (!tiles) return MS3D_E_UNSUPPORTED;
    if (chunks > 0) {
        const dim3 grid((unsigned)chunks, tiles);
        const int rows = dq != nullptr;
        MS3D_LAUNCH_VEC(v4, qattn_backward_q_kernel, grid, QATTN_THREADS, 0, stream, queries, k, v, mask, row_map, order, seg_start,
                    chunk_seg, chunk_first, out, lse, dout, sh, rows, w_a, w_p, w_d);
    }
    const dim3 mgrid((unsigned)B, tiles);
    MS3D_LAUNCH_VEC(v4, qattn_backward_q_merge_kernel, mgrid, QATTN_THREADS, 0, stream, chunk_first, sh, w_a, w_p, w_d, dq, delta);
    return 0;
}

int ms3d_qattn_backward_kv(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                           const int *seg_of_row, const float *out, const float *lse, const float *delta, const float *dout,
                           long V, int B, int Q, int H, int D, float scale, float *dk, float *dv, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!sample_shape_served(V, B, Q, H, D)) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;                         // (dk / dv are not written: the caller's zero)
    if (!queries || !k || !v || !seg_of_row || !out || !lse || !delta || !dout || (!dk && !dv)) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(queries, k, v, out, dout, dk, dv);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const long per = QATTN_THREADS / sh.G, blocks = (V * H + per - 1) / per;
    if (blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, qattn_backward_kv_kernel, (unsigned)blocks, QATTN_THREADS, 0, stream, queries, k, v, mask, row_map, seg_of_row,
                out, lse, delta, dout, V, sh, dk, dv);
    return 0;
}

}  // extern "C"
