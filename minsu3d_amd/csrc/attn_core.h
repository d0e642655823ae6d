// What the fused attention kernels share (csrc/kattn.hip over a kernel map, csrc/qattn.hip and csrc/vattn.hip between the rows
// and the queries of a sample): the lane layout of a (row, head) item, the accumulation steps of the three sweeps and the
// four-row gather stages; for the two per-sample families also their limits and the chunking of a sample.  Each file keeps its
// kernels, its loops and where a row index comes from; a score is formed there too.  What lies here is the ONE copy of the
// arithmetic after it, so every sweep of either family recomputes p and ds to the same bits.
//
// Layout: the work item is one (row, head).  A GROUP of G lanes (a power of two, <= 64, so a group never straddles a wave)
// holds the D channels of that head: lane l the channels (it * G + l) * VEC + j, VEC = 4 (16-byte accesses: D % 4 == 0 and
// 16-byte aligned rows) or 1 (any D, two rounds when D > 64).  Consecutive groups take consecutive heads of one row, so a
// wave reads whole runs of a row, and 64 / G items share a wave when D is small.  A head's dot product is summed inside
// its group by an xor butterfly, which leaves the same bits on every lane of the group.  The rows an item attends to are
// taken four at a time so that eight row gathers are in flight per lane.  No lane leaves before the last shuffle: a lane
// without work runs the loops with every load switched off.
//
// Backward: p = exp(s - lse) recomputed.  The textbook ds = p (<dout, v> - <dout, out>) subtracts two dot products that agree
// in every digit float32 keeps when one input carries almost all of a row's weight (out is then that input's v): what is
// left is rounding noise of the size of <dout, v>, not of ds, and it lands on the pair whose p is 1.  Here the difference is
// taken per channel BEFORE the dot product, e = <dout, v - out> (v - out is exact where it is small), and what the float32
// rounding of the saved `out` still costs is measured and taken back: sum p e over a row's inputs would be zero for the exact
// out, so delta = sum p e is the residual, and ds = p (e - delta).  The ds of a row then sum to zero as they must, and each
// keeps its relative accuracy.  In the pass for q delta is known only after the sweep: dq = scale (sum ds' k - delta sum p k)
// with ds' = p e, both sums kept per lane (push_dq); the pass for k and v reads delta (push_dkv).
#pragma once
#include "common.h"

namespace {

template <int VEC> struct Lane { static constexpr int NIT = VEC == 4 ? 1 : 2, N = NIT * VEC; };

// the group size of a head: the smallest power of two that covers D / VEC lanes, 64 at most
int group_of(int D, int VEC)
{
    const int n = (D + VEC - 1) / VEC;
    int G = 1;
    while (G < n && G < 64) G *= 2;
    return G;
}

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

// ---- the accumulation steps, one present input at a time, over this lane's slices

// forward: the online-softmax push of the score s and the input's v slice
template <int N>
__device__ __forceinline__ void push_softmax(float s, const float (&vr)[N], float &m, float &sum, float (&acc)[N])
{
    const float mn = fmaxf(m, s);
    const float c = expf(m - mn), p = expf(s - mn);                  // (m = -inf on the first input: c = 0)
    sum = fmaf(sum, c, p);
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = fmaf(acc[j], c, p * vr[j]);
    m = mn;
}

// forward: acc becomes the out slice; returns lse (nothing was pushed: out = 0, lse = 0)
template <int N>
__device__ __forceinline__ float finish_softmax(float m, float sum, float (&acc)[N])
{
    const float inv = sum > 0.f ? 1.f / sum : 0.f;                   // one input: sum = 1, out = v to the bit
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] *= inv;
    return sum > 0.f ? m + logf(sum) : 0.f;
}

// backward for q: dl = sum p e, acc = sum p e k, pk = sum p k, each in the order of the calls; returns ds' = p e
template <int N>
__device__ __forceinline__ float push_dq(float p, float e, const float (&kr)[N], float &dl, float (&acc)[N], float (&pk)[N])
{
    const float ds = p * e;
    dl += ds;
#pragma unroll
    for (int j = 0; j < N; j++) {
        acc[j] = fmaf(ds, kr[j], acc[j]);
        pk[j] = fmaf(p, kr[j], pk[j]);
    }
    return ds;
}

// backward for k and v: av = sum p dout, ak = sum ds q with ds = p (e - delta)
template <int N>
__device__ __forceinline__ void push_dkv(float p, float ds, const float (&dr)[N], const float (&qr)[N], float (&av)[N],
                                         float (&ak)[N])
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        av[j] = fmaf(p, dr[j], av[j]);
        ak[j] = fmaf(ds, qr[j], ak[j]);
    }
}

// ---- the four-row stages: every gather is issued before the first butterfly

// where an item's slices lie: the row pitch C = H * D, its head h and that head's offset h * D, its lane l of the G, D
struct Item {
    size_t C, hoff;
    int H, h, l, G, D;
};

// the k and v slices of the rows idx[u] (-1 = off: zeros, nothing is read)
template <int VEC, typename I>
__device__ __forceinline__ void gather_kv(const float *__restrict__ k, const float *__restrict__ v, const I (&idx)[4],
                                          const Item &it, float (&kr)[4][Lane<VEC>::N], float (&vr)[4][Lane<VEC>::N])
{
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const size_t row = (size_t)(idx[u] >= 0 ? idx[u] : 0) * it.C + it.hoff;
        load_slice<VEC>(k + row, it.l, it.G, it.D, idx[u] >= 0, kr[u]);
        load_slice<VEC>(v + row, it.l, it.G, it.D, idx[u] >= 0, vr[u]);
    }
}

// key side, forward: dot[u] = <qv, k[idx[u]]>
template <int VEC, typename I>
__device__ __forceinline__ void key_stage(const float *__restrict__ k, const float *__restrict__ v, const I (&idx)[4],
                                          const Item &it, const float (&qv)[Lane<VEC>::N], float (&kr)[4][Lane<VEC>::N],
                                          float (&vr)[4][Lane<VEC>::N], float (&dot)[4])
{
    gather_kv<VEC>(k, v, idx, it, kr, vr);
#pragma unroll
    for (int u = 0; u < 4; u++) dot[u] = group_sum(dot_slice(qv, kr[u]), it.G);
}

// key side, backward: also dp[u] = e = <dov, v[idx[u]] - ov>
template <int VEC, typename I>
__device__ __forceinline__ void key_stage(const float *__restrict__ k, const float *__restrict__ v, const I (&idx)[4],
                                          const Item &it, const float (&qv)[Lane<VEC>::N], const float (&dov)[Lane<VEC>::N],
                                          const float (&ov)[Lane<VEC>::N], float (&kr)[4][Lane<VEC>::N],
                                          float (&vr)[4][Lane<VEC>::N], float (&dot)[4], float (&dp)[4])
{
    gather_kv<VEC>(k, v, idx, it, kr, vr);
#pragma unroll
    for (int u = 0; u < 4; u++) {
        dot[u] = group_sum(dot_slice(qv, kr[u]), it.G);
        dp[u] = group_sum(dot_diff(dov, vr[u], ov), it.G);
    }
}

// query side (the passes for k and v): the q and dout slices, lse and delta of the rows row[u] where live[u], and against
// this item's own kv, vv: dot[u] = <q[row[u]], kv>, dp[u] = e = <dout[row[u]], vv - out[row[u]]>
template <int VEC>
__device__ __forceinline__ void query_stage(const float *__restrict__ q, const float *__restrict__ dout,
                                            const float *__restrict__ out, const float *__restrict__ lse,
                                            const float *__restrict__ delta, const size_t (&row)[4], const bool (&live)[4],
                                            const Item &it, const float (&kv)[Lane<VEC>::N], const float (&vv)[Lane<VEC>::N],
                                            float (&qr)[4][Lane<VEC>::N], float (&dr)[4][Lane<VEC>::N], float (&ls)[4],
                                            float (&dl)[4], float (&dot)[4], float (&dp)[4])
{
    float orow[4][Lane<VEC>::N];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        load_slice<VEC>(q + row[u] * it.C + it.hoff, it.l, it.G, it.D, live[u], qr[u]);
        load_slice<VEC>(dout + row[u] * it.C + it.hoff, it.l, it.G, it.D, live[u], dr[u]);
        load_slice<VEC>(out + row[u] * it.C + it.hoff, it.l, it.G, it.D, live[u], orow[u]);
        ls[u] = live[u] ? lse[row[u] * it.H + it.h] : 0.f;
        dl[u] = live[u] ? delta[row[u] * it.H + it.h] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        dot[u] = group_sum(dot_slice(qr[u], kv), it.G);
        dp[u] = group_sum(dot_diff(dr[u], vv, orow[u]), it.G);
    }
}

// ---- the per-sample families (csrc/qattn.hip, csrc/vattn.hip): one set of limits, one chunking of a sample's rows

constexpr int SATTN_MAX_D = 128;           // head dimension at most: two scalar rounds of a 64-lane group
constexpr int SATTN_MAX_Q = 1024;
constexpr int SATTN_MAX_C = 1024;          // H * D
constexpr int SATTN_MAX_B = 65535;
constexpr int SATTN_THREADS = 256;
constexpr int SATTN_ROWS_PER_CHUNK = 512;  // positions of `order` per chunk: a constant of the library, NOT derived from the
                                           // grid or the CU count -- the order of every sum is the same on every machine

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
    p0 = (long)seg_start[b] + (long)(c - chunk_first[b]) * SATTN_ROWS_PER_CHUNK;
    p1 = min(p0 + SATTN_ROWS_PER_CHUNK, (long)seg_start[b + 1]);
}

// the limits every call shares: whether the shape is served
bool sample_shape_served(long V, int B, int Q, int H, int D)
{
    if (H < 1 || D < 1 || D > SATTN_MAX_D || (long)H * D > SATTN_MAX_C) return false;
    return Q >= 0 && Q <= SATTN_MAX_Q && B >= 0 && B <= SATTN_MAX_B && V >= 0;
}

// the tiles of (query, head) items of a sweep or merge launch; 0 when they do not fit a grid
unsigned item_tiles(int Q, int H, int G)
{
    const long per = SATTN_THREADS / G, tiles = ((long)Q * H + per - 1) / per;
    return tiles > 65535 ? 0u : (unsigned)tiles;
}

}  // namespace
