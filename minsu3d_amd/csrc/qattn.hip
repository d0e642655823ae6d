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
//                e = <dout, v - out> taken per channel before the sum (see csrc/kattn.hip for why); the merge adds the chunks in
//                ascending order, delta[b, q, h] = sum_i p e, dq = scale (sum p e k - delta sum p k)
//   backward_kv  one (row, head) item per voxel row loops over the Q queries of its sample in ascending q: dv = sum p dout,
//                dk = scale sum p (e - delta) q; one writer per element, no partials
// No atomics of any kind, one writer per element, the same bytes on every run.
//
// Lane layout (that of csrc/kattn.hip): an item is served by a GROUP of G lanes (a power of two <= 64, never straddling a
// wave) that hold the D channels of the head: lane l the channels (it * G + l) * VEC + j, VEC = 4 (16-byte accesses: D % 4 == 0
// and 16-byte aligned rows) or 1 (any D, two rounds when D > 64).  A head's dot product is an xor butterfly inside its group,
// which leaves the same bits on every lane.  Rows are taken four at a time so that eight row loads are in flight per lane; every
// group of a workgroup walks the same rows, so they come from the cache.  No lane leaves before the last shuffle: a lane
// without work runs the loops with every load switched off.
#include "common.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int QATTN_MAX_D = 128;           // head dimension at most: two scalar rounds of a 64-lane group
constexpr int QATTN_MAX_Q = 1024;
constexpr int QATTN_MAX_C = 1024;          // H * D
constexpr int QATTN_MAX_B = 65535;
constexpr int QATTN_THREADS = 256;
constexpr int QATTN_ROWS_PER_CHUNK = 512;  // positions of `order` per chunk: a constant of the library, NOT derived from the
                                           // grid or the CU count -- the order of every sum is the same on every machine

template <int VEC> struct Lane { static constexpr int NIT = VEC == 4 ? 1 : 2, N = NIT * VEC; };

// the group size of a head: the smallest power of two that covers D / VEC lanes, 64 at most
int group_of(int D, int VEC)
{
    const int n = (D + VEC - 1) / VEC;
    int G = 1;
    while (G < n && G < 64) G *= 2;
    return G;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the slice of a head this lane holds: x[it * VEC + j] = p[(it * G + l) * VEC + j], zero past D or with the load off
template <int VEC>
__device__ __forceinline__ void load_slice(const float *__restrict__ p, int l, int G, int D, bool on, float (&x)[Lane<VEC>::N])
{
#pragma unroll
    for (int it = 0; it < Lane<VEC>::NIT; it++) {
        const int d0 = (it * G + l) * VEC;
        if constexpr (VEC == 4) {
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (on && d0 < D) r = *reinterpret_cast<const float4 *>(p + d0);
            x[it * 4 + 0] = r.x; x[it * 4 + 1] = r.y; x[it * 4 + 2] = r.z; x[it * 4 + 3] = r.w;
        } else {
            x[it] = (on && d0 < D) ? p[d0] : 0.f;
        }
    }
}

template <int VEC>
__device__ __forceinline__ void store_slice(float *__restrict__ p, int l, int G, int D, bool on, const float (&x)[Lane<VEC>::N])
{
#pragma unroll
    for (int it = 0; it < Lane<VEC>::NIT; it++) {
        const int d0 = (it * G + l) * VEC;
        if (!on || d0 >= D) continue;
        if constexpr (VEC == 4)
            *reinterpret_cast<float4 *>(p + d0) = make_float4(x[it * 4 + 0], x[it * 4 + 1], x[it * 4 + 2], x[it * 4 + 3]);
        else
            p[d0] = x[it];
    }
}

// this lane's share of <a, b>: explicit fmaf in one order, so that all three sweeps recompute a score to the same bits
template <int N>
__device__ __forceinline__ float dot_slice(const float (&a)[N], const float (&b)[N])
{
    float s = a[0] * b[0];
#pragma unroll
    for (int j = 1; j < N; j++) s = fmaf(a[j], b[j], s);
    return s;
}

// this lane's share of <a, b - c>
template <int N>
__device__ __forceinline__ float dot_diff(const float (&a)[N], const float (&b)[N], const float (&c)[N])
{
    float s = a[0] * (b[0] - c[0]);
#pragma unroll
    for (int j = 1; j < N; j++) s = fmaf(a[j], b[j] - c[j], s);
    return s;
}

// sum over the G lanes of a group (G a power of two, the group aligned to G): every lane ends with the same bits
__device__ __forceinline__ float group_sum(float x, int G)
{
    for (int d = G >> 1; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// what every kernel is told about the call
struct Shape {
    int B, Q, H, D, G;
    float scale;
};

// the positions [p0, p1) of `order` that chunk c covers, and its sample
__device__ __forceinline__ void chunk_range(const int *__restrict__ seg_start, const int *__restrict__ chunk_seg,
                                            const int *__restrict__ chunk_first, int c, int &b, long &p0, long &p1)
{
    b = chunk_seg[c];
    p0 = (long)seg_start[b] + (long)(c - chunk_first[b]) * QATTN_ROWS_PER_CHUNK;
    p1 = min(p0 + QATTN_ROWS_PER_CHUNK, (long)seg_start[b + 1]);
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
    float qv[N], acc[N];
    load_slice<VEC>(queries + ((size_t)b * Q + q) * C + hoff, l, G, D, on, qv);
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0.f;
    float m = -INFINITY, sum = 0.f;
    for (long r0 = p0; r0 < p1; r0 += 4) {
        long idx[4];
        float kr[4][N], vr[4][N], dot[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            idx[u] = (on && r0 + u < p1) ? (long)order[r0 + u] : -1;
            if (idx[u] >= 0 && mask) {
                const size_t mr = row_map ? (size_t)row_map[idx[u]] : (size_t)idx[u];
                if (mask[mr * Q + q]) idx[u] = -1;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t row = (size_t)(idx[u] >= 0 ? idx[u] : 0) * C + hoff;
            load_slice<VEC>(k + row, l, G, D, idx[u] >= 0, kr[u]);
            load_slice<VEC>(v + row, l, G, D, idx[u] >= 0, vr[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) dot[u] = group_sum(dot_slice<N>(qv, kr[u]), G);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            const float s = sh.scale * dot[u];
            const float mn = fmaxf(m, s);
            const float cf = expf(m - mn), p = expf(s - mn);         // (m = -inf on the first row: cf = 0)
            sum = fmaf(sum, cf, p);
#pragma unroll
            for (int j = 0; j < N; j++) acc[j] = fmaf(acc[j], cf, p * vr[u][j]);
            m = mn;
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
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] *= inv;
    store_slice<VEC>(out + ((size_t)b * Q + q) * C + hoff, l, G, D, true, acc);
    if (l == 0) lse[(size_t)b * QH + item] = sum > 0.f ? M + logf(sum) : 0.f;
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
#pragma unroll
        for (int u = 0; u < 4; u++) {
            idx[u] = (on && r0 + u < p1) ? (long)order[r0 + u] : -1;
            if (idx[u] >= 0 && mask) {
                const size_t mr = row_map ? (size_t)row_map[idx[u]] : (size_t)idx[u];
                if (mask[mr * Q + q]) idx[u] = -1;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t row = (size_t)(idx[u] >= 0 ? idx[u] : 0) * C + hoff;
            load_slice<VEC>(k + row, l, G, D, idx[u] >= 0, kr[u]);
            load_slice<VEC>(v + row, l, G, D, idx[u] >= 0, vr[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            dot[u] = group_sum(dot_slice<N>(qv, kr[u]), G);
            dp[u] = group_sum(dot_diff<N>(dov, vr[u], ov), G);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            const float p = expf(sh.scale * dot[u] - ls);
            const float ds = p * dp[u];
            dl += ds;
#pragma unroll
            for (int j = 0; j < N; j++) {
                acc[j] = fmaf(ds, kr[u][j], acc[j]);
                pk[j] = fmaf(p, kr[u][j], pk[j]);
            }
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
    float kv[N], vv[N], ak[N], av[N];
    load_slice<VEC>(k + (size_t)i * C + hoff, l, G, D, on, kv);
    load_slice<VEC>(v + (size_t)i * C + hoff, l, G, D, on, vv);
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] = av[j] = 0.f;
    for (int q0 = 0; q0 < Q; q0 += 4) {
        bool live[4];
        float qr[4][N], dr[4][N], orow[4][N], dot[4], dp[4], ls[4], dl[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            live[u] = on && q0 + u < Q && !(mrow && mrow[q0 + u]);
            const size_t qh = ((size_t)b * Q + (live[u] ? q0 + u : 0));
            load_slice<VEC>(queries + qh * C + hoff, l, G, D, live[u], qr[u]);
            load_slice<VEC>(dout + qh * C + hoff, l, G, D, live[u], dr[u]);
            load_slice<VEC>(out + qh * C + hoff, l, G, D, live[u], orow[u]);
            ls[u] = live[u] ? lse[qh * H + h] : 0.f;
            dl[u] = live[u] ? delta[qh * H + h] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            dot[u] = group_sum(dot_slice<N>(qr[u], kv), G);
            dp[u] = group_sum(dot_diff<N>(dr[u], vv, orow[u]), G);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!live[u]) continue;
            const float p = expf(sh.scale * dot[u] - ls[u]);
            const float ds = p * (dp[u] - dl[u]);
#pragma unroll
            for (int j = 0; j < N; j++) {
                av[j] = fmaf(p, dr[u][j], av[j]);
                ak[j] = fmaf(ds, qr[u][j], ak[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] *= sh.scale;
    if (dk) store_slice<VEC>(dk + (size_t)i * C + hoff, l, G, D, on, ak);
    if (dv) store_slice<VEC>(dv + (size_t)i * C + hoff, l, G, D, on, av);
}

// the limits all three calls share; 0 when the shape is served
int shape_check(long V, int B, int Q, int H, int D)
{
    if (H < 1 || D < 1 || D > QATTN_MAX_D || (long)H * D > QATTN_MAX_C) return MS3D_E_UNSUPPORTED;
    if (Q < 0 || Q > QATTN_MAX_Q || B < 0 || B > QATTN_MAX_B || V < 0) return MS3D_E_UNSUPPORTED;
    return 0;
}

// the tiles of (query, head) items of a sweep or merge launch; 0 when they do not fit a grid
unsigned item_tiles(int Q, int H, int G)
{
    const long per = QATTN_THREADS / G, tiles = ((long)Q * H + per - 1) / per;
    return tiles > 65535 ? 0u : (unsigned)tiles;
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
    if (shape_check(V, B, Q, H, D) || chunks < 0) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;
    if (!queries || !k || !v || !order || !seg_start || !chunk_first || !out || !lse) return MS3D_E_UNSUPPORTED;
    if (chunks > 0 && (!chunk_seg || !ws)) return MS3D_E_UNSUPPORTED;
    if (ws_floats < ms3d_qattn_ws_floats(chunks, Q, H, D)) return MS3D_E_WORKSPACE;
    const size_t C = (size_t)H * D, nacc = (size_t)chunks * Q * C, nqh = (size_t)chunks * Q * H;
    float *w_acc = ws, *w_m = ws + nacc, *w_l = ws + nacc + nqh;
    const bool v4 = D % 4 == 0 && aligned16(queries) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(ws);
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned tiles = item_tiles(Q, H, sh.G);
    if (!tiles) return MS3D_E_UNSUPPORTED;
    if (chunks > 0) {
        const dim3 grid((unsigned)chunks, tiles);
        if (v4) qattn_forward_kernel<4><<<grid, QATTN_THREADS, 0, stream>>>(queries, k, v, mask, row_map, order, seg_start,
                                                                            chunk_seg, chunk_first, sh, w_acc, w_m, w_l);
        else qattn_forward_kernel<1><<<grid, QATTN_THREADS, 0, stream>>>(queries, k, v, mask, row_map, order, seg_start,
                                                                         chunk_seg, chunk_first, sh, w_acc, w_m, w_l);
        MS3D_LAUNCH_CHECK();
    }
    const dim3 mgrid((unsigned)B, tiles);
    if (v4) qattn_forward_merge_kernel<4><<<mgrid, QATTN_THREADS, 0, stream>>>(chunk_first, sh, w_acc, w_m, w_l, out, lse);
    else qattn_forward_merge_kernel<1><<<mgrid, QATTN_THREADS, 0, stream>>>(chunk_first, sh, w_acc, w_m, w_l, out, lse);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_qattn_backward_q(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                          const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first,
                          const float *out, const float *lse, const float *dout, long V, int B, int chunks, int Q, int H, int D,
                          float scale, float *dq, float *delta, float *ws, size_t ws_floats, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (shape_check(V, B, Q, H, D) || chunks < 0) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;
    if (!queries || !k || !v || !order || !seg_start || !chunk_first || !out || !lse || !dout || !delta)
        return MS3D_E_UNSUPPORTED;
    if (chunks > 0 && (!chunk_seg || !ws)) return MS3D_E_UNSUPPORTED;
    if (ws_floats < ms3d_qattn_backward_ws_floats(chunks, Q, H, D)) return MS3D_E_WORKSPACE;
    const size_t C = (size_t)H * D, nacc = (size_t)chunks * Q * C;
    float *w_a = ws, *w_p = ws + nacc, *w_d = ws + 2 * nacc;
    const bool v4 = D % 4 == 0 && aligned16(queries) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) &&
                    aligned16(ws) && (!dq || aligned16(dq));
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const unsigned tiles = item_tiles(Q, H, sh.G);
    if (!tiles) return MS3D_E_UNSUPPORTED;
    if (chunks > 0) {
        const dim3 grid((unsigned)chunks, tiles);
        const int rows = dq != nullptr;
        if (v4) qattn_backward_q_kernel<4><<<grid, QATTN_THREADS, 0, stream>>>(queries, k, v, mask, row_map, order, seg_start,
                                                                               chunk_seg, chunk_first, out, lse, dout, sh, rows,
                                                                               w_a, w_p, w_d);
        else qattn_backward_q_kernel<1><<<grid, QATTN_THREADS, 0, stream>>>(queries, k, v, mask, row_map, order, seg_start,
                                                                            chunk_seg, chunk_first, out, lse, dout, sh, rows, w_a,
                                                                            w_p, w_d);
        MS3D_LAUNCH_CHECK();
    }
    const dim3 mgrid((unsigned)B, tiles);
    if (v4) qattn_backward_q_merge_kernel<4><<<mgrid, QATTN_THREADS, 0, stream>>>(chunk_first, sh, w_a, w_p, w_d, dq, delta);
    else qattn_backward_q_merge_kernel<1><<<mgrid, QATTN_THREADS, 0, stream>>>(chunk_first, sh, w_a, w_p, w_d, dq, delta);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_qattn_backward_kv(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                           const int *seg_of_row, const float *out, const float *lse, const float *delta, const float *dout,
                           long V, int B, int Q, int H, int D, float scale, float *dk, float *dv, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (shape_check(V, B, Q, H, D)) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || Q == 0) return 0;                         // (dk / dv are not written: the caller's zero)
    if (!queries || !k || !v || !seg_of_row || !out || !lse || !delta || !dout || (!dk && !dv)) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && aligned16(queries) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) &&
                    (!dk || aligned16(dk)) && (!dv || aligned16(dv));
    const Shape sh{B, Q, H, D, group_of(D, v4 ? 4 : 1), scale};
    const long per = QATTN_THREADS / sh.G, blocks = (V * H + per - 1) / per;
    if (blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (v4) qattn_backward_kv_kernel<4><<<(unsigned)blocks, QATTN_THREADS, 0, stream>>>(queries, k, v, mask, row_map, seg_of_row,
                                                                                       out, lse, delta, dout, V, sh, dk, dv);
    else qattn_backward_kv_kernel<1><<<(unsigned)blocks, QATTN_THREADS, 0, stream>>>(queries, k, v, mask, row_map, seg_of_row, out,
                                                                                    lse, delta, dout, V, sh, dk, dv);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
