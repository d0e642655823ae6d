// Multi-head softmax attention over a neighbour index (ME.neighbor_attention), with gradients.  idx int64 [N][k] names, per
// query, k rows of the support k / v [V][C] as they are held, or < 0 for "no neighbour" in any slot; q [N][C] lives on the
// target, bias [N][k][H] (or NULL) is one additive term per entry and head.  C = H * D, float32 throughout.
//
//   s[n, j, h]   = scale * <q[n, h, :], k[i, h, :]> + bias[n, j, h]       i = idx[n][j], over the VALID slots, ascending j
//   p            = softmax over the valid slots (the maximum is always subtracted before exp)
//   out[n, h, :] = sum_j p * v[i, h, :]        lse[n, h] = m + log sum exp(s - m)       (no valid slot: out = 0, lse = 0)
//
// Every direction is a GATHER with one writer per element, like csrc/kattn.hip and csrc/neighbor.hip: no atomics of any kind,
// every sum in one order fixed by the shapes and the index, the same bytes on every run.
//   forward      one online-softmax sweep over ascending j; rows of q, k, v are read where they lie
//   backward_q   the same sweep: p recomputed from lse, ds = p (<dout, v - out> - delta) (csrc/attn_core.h),
//                dq = scale * (sum ds' k - delta sum p k), delta [N][H], and dbias[n][j][h] = ds for a valid slot, 0.0f for an
//                invalid one.  delta is known only after the sweep, so the bits of p and e of every slot wait in LDS (two
//                floats a slot and group) and the group stores its k elements of dbias after the loop
//   backward_kv  a gather on the support side through the record's transposed table: row i walks its entries e = n * k + j in
//                the order of entry_sorted (ascending e in the caller's numbering of the queries), dv += p dout[n],
//                dk += ds q[n], scaled once at the store; p and ds recomputed from q[n], k[i], v[i], bias[e], lse[n], out[n],
//                delta[n].  A row of more than ms3d_nbr_chunk_entries() entries goes through the record's chunk list as in
//                csrc/neighbor.hip: a group per (chunk, head) sums the chunk from 0 into two partial rows of the workspace,
//                and the row adds its partials from 0 in ascending chunk order.
// A value of idx that is < 0 or >= V, and an entry outside [0, N * k), switch the gather off: nothing outside the rows given is
// ever read.  Lane layout, accumulation steps and the four-row gather stages: csrc/attn_core.h.
#include "attn_core.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int NATTN_MAX_K = 254;          // the limit of the neighbour record (a slot number fits a byte)
constexpr int NATTN_MAX_D = 128;          // head dimension at most: two scalar rounds of a 64-lane group
constexpr int NATTN_THREADS = 256;
constexpr int NATTN_STASH_FLOATS = 16384; // LDS floats (64 KiB) of a backward_q workgroup's stash: [groups][k] p, then e

// the held row slot j of a query names, or -1: off, past k, < 0 or >= V
__device__ __forceinline__ long long nattn_slot(const long long *__restrict__ row, int j, int K, long V, bool on)
{
    if (!on || j >= K) return -1;
    const long long r = row[j];
    return (r >= 0 && r < V) ? r : -1;
}

// One group: the item (n, h) = blockIdx.x * (256 / G) + group.  Online softmax over ascending j.
template <int VEC>
__global__ __launch_bounds__(NATTN_THREADS) void nattn_forward_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ bias,
    const long long *__restrict__ idx, long V, long N, int K, int H, int D, int G, float scale, float *__restrict__ out,
    float *__restrict__ lse)
{
    constexpr int NL = Lane<VEC>::N;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * (NATTN_THREADS / G) + g;
    const bool on = item < N * H;
    const long n = on ? item / H : 0;
    const int h = on ? (int)(item - n * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    const long long *__restrict__ row = idx + (size_t)n * K;
    float qv[NL], acc[NL];
    load_slice<VEC>(q + (size_t)n * C + hoff, l, G, D, on, qv);
#pragma unroll
    for (int j = 0; j < NL; j++) acc[j] = 0.f;
    float m = -INFINITY, sum = 0.f;
    for (int k0 = 0; k0 < K; k0 += 4) {
        long long id[4];
        float kr[4][NL], vr[4][NL], dot[4];
#pragma unroll
        for (int u = 0; u < 4; u++) id[u] = nattn_slot(row, k0 + u, K, V, on);
        key_stage<VEC>(k, v, id, it, qv, kr, vr, dot);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (id[u] < 0) continue;
            const float s = fmaf(scale, dot[u], bias ? bias[((size_t)n * K + (k0 + u)) * H + h] : 0.f);
            push_softmax(s, vr[u], m, sum, acc);
        }
    }
    const float ls = finish_softmax(m, sum, acc);
    store_slice<VEC>(out + (size_t)n * C + hoff, l, G, D, on, acc);
    if (on && l == 0) lse[(size_t)n * H + h] = ls;
}

// One group: the item (n, h) = blockIdx.x * GPB + group, GPB = blockDim.x / G groups a workgroup (sized on the host from k).
// With dbias: s_p [GPB][K] and s_e [GPB][K] in LDS; slot j of a group is written and read back by its lane j % G alone, so no
// barrier is needed; p = -1 marks an invalid slot.  dq and dbias may each be NULL; delta is always written.
template <int VEC>
__global__ __launch_bounds__(NATTN_THREADS) void nattn_backward_q_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ bias,
    const long long *__restrict__ idx, const float *__restrict__ out, const float *__restrict__ lse,
    const float *__restrict__ dout, long V, long N, int K, int H, int D, int G, float scale, float *__restrict__ dq,
    float *__restrict__ dbias, float *__restrict__ delta)
{
    constexpr int NL = Lane<VEC>::N;
    extern __shared__ __attribute__((aligned(16))) float s_p[];      // [GPB][K] p, then [GPB][K] e; dbias != NULL only
    const int GPB = blockDim.x / G;
    float *const s_e = s_p + GPB * K;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * GPB + g;
    const bool on = item < N * H;
    const long n = on ? item / H : 0;
    const int h = on ? (int)(item - n * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    const long long *__restrict__ row = idx + (size_t)n * K;
    float qv[NL], dov[NL], ov[NL], acc[NL], pk[NL];
    load_slice<VEC>(q + (size_t)n * C + hoff, l, G, D, on, qv);
    load_slice<VEC>(dout + (size_t)n * C + hoff, l, G, D, on, dov);
    load_slice<VEC>(out + (size_t)n * C + hoff, l, G, D, on, ov);
    const float ls = on ? lse[(size_t)n * H + h] : 0.f;
#pragma unroll
    for (int j = 0; j < NL; j++) acc[j] = pk[j] = 0.f;
    float dl = 0.f;                                                  // sum_j p e, ascending j
    for (int k0 = 0; k0 < K; k0 += 4) {
        long long id[4];
        float kr[4][NL], vr[4][NL], dot[4], dp[4];
#pragma unroll
        for (int u = 0; u < 4; u++) id[u] = nattn_slot(row, k0 + u, K, V, on);
        key_stage<VEC>(k, v, id, it, qv, dov, ov, kr, vr, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = k0 + u;
            float p = -1.f;
            if (id[u] >= 0) {
                const float s = fmaf(scale, dot[u], bias ? bias[((size_t)n * K + kk) * H + h] : 0.f);
                p = expf(s - ls);
                push_dq(p, dp[u], kr[u], dl, acc, pk);
            }
            if (dbias && kk < K && l == (kk & (G - 1))) {            // (this lane is the only one that touches slot kk)
                s_p[g * K + kk] = p;
                s_e[g * K + kk] = dp[u];
            }
        }
    }
    if (dbias && on) {
        float *__restrict__ dst = dbias + (size_t)n * K * H + h;
        for (int kk = l; kk < K; kk += G) {
            const float p = s_p[g * K + kk];
            dst[(size_t)kk * H] = p >= 0.f ? p * (s_e[g * K + kk] - dl) : 0.0f;
        }
    }
    if (dq) {
#pragma unroll
        for (int j = 0; j < NL; j++) acc[j] = scale * fmaf(-dl, pk[j], acc[j]);
        store_slice<VEC>(dq + (size_t)n * C + hoff, l, G, D, on, acc);
    }
    if (on && l == 0) delta[(size_t)n * H + h] = dl;
}

// what the two kernels of the kv pass read of the query side
struct QuerySide {
    const float *__restrict__ q, *__restrict__ dout, *__restrict__ out, *__restrict__ lse, *__restrict__ delta, *__restrict__ bias;
    const long long *__restrict__ entry_sorted;
    long entries;                         // N * k: an entry outside [0, entries) is skipped
    int K;
    float scale;
};

// the chain over entry_sorted[begin .. end) in ascending position, four entries at a time, against this item's own kv, vv:
// av += p dout[n], ak += ds q[n] (unscaled).  begin and end are the same on every lane of a group.
template <int VEC>
__device__ __forceinline__ void nattn_chain(int begin, int end, const QuerySide &qs, const Item &it,
                                            const float (&kv)[Lane<VEC>::N], const float (&vv)[Lane<VEC>::N],
                                            float (&ak)[Lane<VEC>::N], float (&av)[Lane<VEC>::N])
{
    constexpr int NL = Lane<VEC>::N;
    for (int s0 = begin; s0 < end; s0 += 4) {
        bool live[4];
        size_t n[4], ent[4];
        float qr[4][NL], dr[4][NL], dot[4], dp[4], ls[4], dl[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long e = s0 + u < end ? qs.entry_sorted[s0 + u] : -1;
            live[u] = e >= 0 && e < qs.entries;
            ent[u] = (size_t)(live[u] ? e : 0);
            n[u] = ent[u] / (size_t)qs.K;
        }
        query_stage<VEC>(qs.q, qs.dout, qs.out, qs.lse, qs.delta, n, live, it, kv, vv, qr, dr, ls, dl, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!live[u]) continue;
            const float s = fmaf(qs.scale, dot[u], qs.bias ? qs.bias[ent[u] * it.H + it.h] : 0.f);
            const float p = expf(s - ls[u]);
            push_dkv(p, p * (dp[u] - dl[u]), dr[u], qr[u], av, ak);
        }
    }
}

// One group: the item (chunk c, h) of a long row: partial[c] = (the dk chain, the dv chain) over the chunk's T entries, from 0
template <int VEC>
__global__ __launch_bounds__(NATTN_THREADS) void nattn_backward_kv_chunk_kernel(
    QuerySide qs, const float *__restrict__ k, const float *__restrict__ v, const int *__restrict__ seg_start,
    const int *__restrict__ chunk_start, int n_chunks, int T, int V, int H, int D, int G, float *__restrict__ partial)
{
    constexpr int NL = Lane<VEC>::N;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * (NATTN_THREADS / G) + g;
    const bool on = item < (long)n_chunks * H;
    const int c = on ? (int)(item / H) : 0;
    const int h = on ? (int)(item - (long)c * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    int lo = 0, hi = V;                          // the last row i with chunk_start[i] <= c owns chunk c
    for (int step = 0; step < 32 && hi - lo > 1; step++) {
        const int mid = lo + ((hi - lo) >> 1);
        if (chunk_start[mid] <= c) lo = mid; else hi = mid;
    }
    const int first = seg_start[lo], last = seg_start[lo + 1];
    const long b = (long)first + (long)(c - chunk_start[lo]) * T;
    int begin = (int)(b < last ? b : last);
    int end = last - begin > T ? begin + T : last;
    if (!on || begin < first) begin = end = 0;
    float kv[NL], vv[NL], ak[NL], av[NL];
    load_slice<VEC>(k + (size_t)lo * C + hoff, l, G, D, on, kv);
    load_slice<VEC>(v + (size_t)lo * C + hoff, l, G, D, on, vv);
#pragma unroll
    for (int j = 0; j < NL; j++) ak[j] = av[j] = 0.f;
    nattn_chain<VEC>(begin, end, qs, it, kv, vv, ak, av);
    store_slice<VEC>(partial + (size_t)c * 2 * C + hoff, l, G, D, on, ak);
    store_slice<VEC>(partial + ((size_t)c * 2 + 1) * C + hoff, l, G, D, on, av);
}

// One group: the item (i, h) of the support side: the plain chain over the row's entries, or the partials of a long row in
// ascending chunk order.  A row no entry names stores exact zeros.  dk is scaled once, here.
template <int VEC>
__global__ __launch_bounds__(NATTN_THREADS) void nattn_backward_kv_row_kernel(
    QuerySide qs, const float *__restrict__ k, const float *__restrict__ v, const int *__restrict__ seg_start,
    const int *__restrict__ chunk_start, int n_chunks, const float *__restrict__ partial, int V, int H, int D, int G,
    float *__restrict__ dk, float *__restrict__ dv)
{
    constexpr int NL = Lane<VEC>::N;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * (NATTN_THREADS / G) + g;
    const bool on = item < (long)V * H;
    const int i = on ? (int)(item / H) : 0;
    const int h = on ? (int)(item - (long)i * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    float kv[NL], vv[NL], ak[NL], av[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) ak[j] = av[j] = 0.f;
    int c0 = on ? chunk_start[i] : 0, c1 = on ? chunk_start[i + 1] : 0;
    if (c1 > n_chunks) c1 = n_chunks;            // (the workspace holds n_chunks partials: nothing beyond them is read)
    if (c0 < 0) c0 = c1;
    if (c1 > c0) {
        for (int c = c0; c < c1; c++) {
            float pkk[NL], pvv[NL];
            load_slice<VEC>(partial + (size_t)c * 2 * C + hoff, l, G, D, true, pkk);
            load_slice<VEC>(partial + ((size_t)c * 2 + 1) * C + hoff, l, G, D, true, pvv);
#pragma unroll
            for (int j = 0; j < NL; j++) { ak[j] += pkk[j]; av[j] += pvv[j]; }
        }
    } else {
        load_slice<VEC>(k + (size_t)i * C + hoff, l, G, D, on, kv);
        load_slice<VEC>(v + (size_t)i * C + hoff, l, G, D, on, vv);
        nattn_chain<VEC>(on ? seg_start[i] : 0, on ? seg_start[i + 1] : 0, qs, it, kv, vv, ak, av);
    }
#pragma unroll
    for (int j = 0; j < NL; j++) ak[j] *= qs.scale;
    if (dk) store_slice<VEC>(dk + (size_t)i * C + hoff, l, G, D, on, ak);
    if (dv) store_slice<VEC>(dv + (size_t)i * C + hoff, l, G, D, on, av);
}

// the checks all three calls share; 0 when the shape is served
int nattn_shape_check(long V, long N, int K, int H, int D)
{
    if (K < 1 || K > NATTN_MAX_K || H < 1 || D < 1 || D > NATTN_MAX_D) return MS3D_E_UNSUPPORTED;
    if ((long)H * D > 0x7fffffffL || (long)K * H > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (V < 0 || N < 0 || V > 0x7fffffffL || N > 0x7fffffffL / K) return MS3D_E_UNSUPPORTED;   // (an entry number fits an int32)
    return 0;
}

// blocks of `per` (item, head) groups each; false when they do not fit a launch
bool nattn_grid(long rows, int H, long per, unsigned *blocks)
{
    const long b = (rows * H + per - 1) / per;
    if (b > 0x7fffffffL) return false;
    *blocks = (unsigned)b;
    return true;
}

}  // namespace

extern "C" {

size_t ms3d_nattn_ws_bytes(long n_chunks, int C)
{
    return n_chunks > 0 && C >= 1 ? (size_t)n_chunks * 2 * (size_t)C * sizeof(float) : 0;
}

int ms3d_nattn_forward(const float *q, const float *k, const float *v, const float *bias, const long long *idx, long V, long N,
                       int K, int H, int D, float scale, float *out, float *lse, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (nattn_shape_check(V, N, K, H, D)) return MS3D_E_UNSUPPORTED;
    if (N == 0 || V == 0) return 0;
    if (!q || !k || !v || !idx || !out || !lse) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(q, k, v, out);
    const int G = group_of(D, v4 ? 4 : 1);
    unsigned blocks;
    if (!nattn_grid(N, H, NATTN_THREADS / G, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, nattn_forward_kernel, blocks, NATTN_THREADS, 0, stream, q, k, v, bias, idx, V, N, K, H, D, G, scale, out,
                    lse);
    return 0;
}

int ms3d_nattn_backward_q(const float *q, const float *k, const float *v, const float *bias, const long long *idx,
                          const float *out, const float *lse, const float *dout, long V, long N, int K, int H, int D,
                          float scale, float *dq, float *dbias, float *delta, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (nattn_shape_check(V, N, K, H, D)) return MS3D_E_UNSUPPORTED;
    if (N == 0 || V == 0) return 0;
    if (!q || !k || !v || !idx || !out || !lse || !dout || !delta) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(q, k, v, out, dout, dq);
    const int G = group_of(D, v4 ? 4 : 1);
    int GPB = NATTN_THREADS / G;                                      // groups of a workgroup: a power of two
    if (dbias)
        while (2 * GPB * K > NATTN_STASH_FLOATS) GPB /= 2;            // (K <= 254: GPB >= 32 or 256 / G) -- from k alone
    unsigned blocks;
    if (!nattn_grid(N, H, GPB, &blocks)) return MS3D_E_UNSUPPORTED;
    const size_t lds = dbias ? sizeof(float) * 2 * (size_t)GPB * K : 0;
    MS3D_LAUNCH_VEC(v4, nattn_backward_q_kernel, blocks, GPB * G, lds, stream, q, k, v, bias, idx, out, lse, dout, V, N, K, H, D, G,
                    scale, dq, dbias, delta);
    return 0;
}

int ms3d_nattn_backward_kv(const float *q, const float *k, const float *v, const float *bias, const float *out, const float *lse,
                           const float *delta, const float *dout, const long long *entry_sorted, const int *seg_start,
                           const int *chunk_start, long n_chunks, long V, long N, int K, int H, int D, float scale, float *dk,
                           float *dv, void *ws, size_t ws_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (nattn_shape_check(V, N, K, H, D) || n_chunks < 0 || n_chunks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (N == 0 || V == 0) return 0;
    if (!q || !k || !v || !out || !lse || !delta || !dout || !entry_sorted || !seg_start || !chunk_start || (!dk && !dv))
        return MS3D_E_UNSUPPORTED;
    if (n_chunks > 0 && (!ws || !ms3d_aligned16(ws))) return MS3D_E_UNSUPPORTED;
    if (ws_bytes < ms3d_nattn_ws_bytes(n_chunks, H * D)) return MS3D_E_WORKSPACE;
    float *partial = (float *)ws;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(q, k, v, out, dout, dk, dv);
    const int G = group_of(D, v4 ? 4 : 1);
    unsigned blocks, cblocks = 0;
    if (!nattn_grid(V, H, NATTN_THREADS / G, &blocks) || !nattn_grid(n_chunks, H, NATTN_THREADS / G, &cblocks))
        return MS3D_E_UNSUPPORTED;
    const QuerySide qs{q, dout, out, lse, delta, bias, entry_sorted, N * K, K, scale};
    if (n_chunks > 0)
        MS3D_LAUNCH_VEC(v4, nattn_backward_kv_chunk_kernel, cblocks, NATTN_THREADS, 0, stream, qs, k, v, seg_start, chunk_start,
                        (int)n_chunks, ms3d_nbr_chunk_entries(), (int)V, H, D, G, partial);
    MS3D_LAUNCH_VEC(v4, nattn_backward_kv_row_kernel, blocks, NATTN_THREADS, 0, stream, qs, k, v, seg_start, chunk_start,
                    (int)n_chunks, partial, (int)V, H, D, G, dk, dv);
    return 0;
}

}  // extern "C"
