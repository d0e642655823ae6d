// Local multi-head attention over the engine's offset-major kernel maps: a query row o attends to the inputs its K offsets
// reach, i = nbr[kk][o] (int32, -1 = none).  q [Vout, C], k / v [Vin, C], C = H * D, float32 throughout.
//
//   s[o, kk, h] = scale * <q[o, h, :], k[i, h, :]> + rel_bias[kk, h]        over the PRESENT kk
//   p           = softmax over the present kk (the maximum is always subtracted before exp)
//   out[o, h, :] = sum_kk p * v[i, h, :]        lse[o, h] = m + log sum exp(s - m)      (no input: out = 0, lse = 0)
//
// Every direction is a GATHER with one writer per element, like csrc/chconv.hip and csrc/pool.hip: no atomics of any kind,
// every sum in one fixed order that depends on the shapes only, the same bytes on every run.
//   forward      one online-softmax sweep over ascending kk; rows of q, k, v are read where they lie
//   backward_q   walks the forward table: p recomputed from lse, ds = p (<dout, v - out> - delta) (see below),
//                dq = scale * sum_kk ds k;  dbias[kk, h] = sum_o ds in two stages: a [K, H] partial per run of
//                KATTN_ROWS_PER_PART output rows, then the partials added in ascending part order; writes delta [Vout, H]
//   backward_kv  a gather through the inverse table (o = nbr_inv[kk][i], the offset index NOT mirrored): dv += p dout[o],
//                dk += scale * ds q[o], p and ds recomputed from q[o], k[i], v[i], rel_bias, lse[o], out[o], delta[o]
// Why ds is formed as p (e - delta) with e = <dout, v - out> is told in csrc/attn_core.h.  In the q pass delta is known only
// after the sweep, so the dbias sums are taken over ds' = p e and corrected from the row's p, stashed in LDS.
//
// Lane layout, accumulation steps and the four-row gather stages: csrc/attn_core.h.  Here a row's four are four K table entries.
#include "attn_core.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int KATTN_MAX_K = 254;          // the limit of the tables' other consumers (csrc/pool.hip, csrc/chconv.hip)
constexpr int KATTN_MAX_D = 128;          // head dimension at most: two scalar rounds of a 64-lane group
constexpr int KATTN_THREADS = 256;
constexpr int KATTN_ROWS_PER_PART = 64;   // output rows per dbias partial: a constant of the library, NOT derived from the
                                          // grid or the CU count -- the order of the sum is the same on every machine
constexpr int KATTN_DB_FLOATS = 16384;    // LDS floats (64 KiB) of a backward_q workgroup's dbias sums: [groups][K]

// One group: the item (o, h) = blockIdx.x * (256 / G) + group.  Online softmax over ascending kk.
template <int VEC>
__global__ __launch_bounds__(KATTN_THREADS) void kattn_forward_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ bias,
    const int *__restrict__ nbr, int Vout, int K, int H, int D, int G, float scale, float *__restrict__ out,
    float *__restrict__ lse)
{
    constexpr int N = Lane<VEC>::N;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * (KATTN_THREADS / G) + g;
    const bool on = item < (long)Vout * H;
    const int o = on ? (int)(item / H) : 0;
    const int h = on ? (int)(item - (long)o * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    float qv[N], acc[N];
    load_slice<VEC>(q + (size_t)o * C + hoff, l, G, D, on, qv);
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0.f;
    float m = -INFINITY, sum = 0.f;
    for (int k0 = 0; k0 < K; k0 += 4) {
        int idx[4];
        float kr[4][N], vr[4][N], dot[4];
#pragma unroll
        for (int u = 0; u < 4; u++) idx[u] = (on && k0 + u < K) ? nbr[(size_t)(k0 + u) * Vout + o] : -1;
        key_stage<VEC>(k, v, idx, it, qv, kr, vr, dot);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (idx[u] < 0) continue;
            const float s = fmaf(scale, dot[u], bias ? bias[(size_t)(k0 + u) * H + h] : 0.f);
            push_softmax(s, vr[u], m, sum, acc);
        }
    }
    const float ls = finish_softmax(m, sum, acc);
    store_slice<VEC>(out + (size_t)o * C + hoff, l, G, D, on, acc);
    if (on && l == 0) lse[(size_t)o * H + h] = ls;
}

// One workgroup: the part blockIdx.x (KATTN_ROWS_PER_PART consecutive output rows) and the head tile blockIdx.y (HB heads).
// Its GPB groups are RG = GPB / HB row lanes of HB heads: group (rl, hl) takes the rows rl, rl + RG, ... of the part in
// ascending order for ONE head, so its sums of ds, one per offset, have a single writer -- lane kk % G of the group, which
// also stashes the row's p and applies the row's delta after the sweep: s_db [GPB][K] and s_p [GPB][K] in LDS (only when
// dbias is asked for).  At the end the row lanes are folded in ascending rl: partial [parts][K][H], every element written
// by exactly one thread.  dq and partial may each be NULL; delta is always written.
template <int VEC>
__global__ __launch_bounds__(KATTN_THREADS) void kattn_backward_q_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ bias,
    const int *__restrict__ nbr, const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ dout,
    int Vout, int K, int H, int D, int G, int HB, int RG, float scale, float *__restrict__ dq, float *__restrict__ delta,
    float *__restrict__ partial)
{
    constexpr int N = Lane<VEC>::N;
    extern __shared__ __attribute__((aligned(16))) float s_db[];     // [GPB][K] sums, then [GPB][K] p; partial != NULL only
    const int T = blockDim.x, GPB = T / G;
    float *const s_p = s_db + GPB * K;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int rl = g / HB, hl = g - rl * HB;
    const int h0 = blockIdx.y * HB, HBt = min(HB, H - h0);
    const int h = h0 + (hl < HBt ? hl : 0);
    const bool lane_on = rl < RG && hl < HBt;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    if (partial) {
        for (int e = threadIdx.x; e < GPB * K; e += T) s_db[e] = 0.f;
        __syncthreads();
    }
    const long row0 = (long)blockIdx.x * KATTN_ROWS_PER_PART;
    for (int r0 = 0; r0 < KATTN_ROWS_PER_PART; r0 += RG) {           // (uniform trip count: the shuffles see whole groups)
        const long ol = row0 + r0 + rl;
        const bool on = lane_on && r0 + rl < KATTN_ROWS_PER_PART && ol < Vout;
        const int o = on ? (int)ol : 0;
        float qv[N], dov[N], ov[N], acc[N], pk[N];
        load_slice<VEC>(q + (size_t)o * C + hoff, l, G, D, on, qv);
        load_slice<VEC>(dout + (size_t)o * C + hoff, l, G, D, on, dov);
        load_slice<VEC>(out + (size_t)o * C + hoff, l, G, D, on, ov);
        const float ls = on ? lse[(size_t)o * H + h] : 0.f;
#pragma unroll
        for (int j = 0; j < N; j++) acc[j] = pk[j] = 0.f;
        float dl = 0.f;                                              // sum_kk p e, ascending kk
        for (int k0 = 0; k0 < K; k0 += 4) {
            int idx[4];
            float kr[4][N], vr[4][N], dot[4], dp[4];
#pragma unroll
            for (int u = 0; u < 4; u++) idx[u] = (on && k0 + u < K) ? nbr[(size_t)(k0 + u) * Vout + o] : -1;
            key_stage<VEC>(k, v, idx, it, qv, dov, ov, kr, vr, dot, dp);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int kk = k0 + u;
                float p = 0.f, ds = 0.f;
                if (idx[u] >= 0) {
                    const float s = fmaf(scale, dot[u], bias ? bias[(size_t)kk * H + h] : 0.f);
                    p = expf(s - ls);
                    ds = push_dq(p, dp[u], kr[u], dl, acc, pk);
                }
                if (partial && kk < K && l == (kk & (G - 1))) {      // (this lane is the only one that touches offset kk)
                    s_db[g * K + kk] += ds;
                    s_p[g * K + kk] = p;
                }
            }
        }
        if (partial)
            for (int kk = l; kk < K; kk += G) s_db[g * K + kk] = fmaf(-dl, s_p[g * K + kk], s_db[g * K + kk]);
        if (dq) {
#pragma unroll
            for (int j = 0; j < N; j++) acc[j] = scale * fmaf(-dl, pk[j], acc[j]);
            store_slice<VEC>(dq + (size_t)o * C + hoff, l, G, D, on, acc);
        }
        if (on && l == 0) delta[(size_t)o * H + h] = dl;
    }
    if (partial) {
        __syncthreads();
        float *__restrict__ dst = partial + (size_t)blockIdx.x * K * H;
        for (int e = threadIdx.x; e < K * HBt; e += T) {
            const int kk = e / HBt, j = e - kk * HBt;
            float s = 0.f;
            for (int r = 0; r < RG; r++) s += s_db[(r * HB + j) * K + kk];
            dst[(size_t)kk * H + h0 + j] = s;
        }
    }
}

// dbias[e] = sum_p partial[p][e], p ascending, one thread per element; summed in double, rounded once
__global__ __launch_bounds__(256) void kattn_dbias_reduce_kernel(const float *__restrict__ partial, int parts, int n,
                                                                 float *__restrict__ dbias)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int p = 0; p < parts; p++) s += (double)partial[(size_t)p * n + e];
    dbias[e] = (float)s;
}

// One group: the item (i, h) of the INPUT side; o = nbr_inv[kk][i] walks the output rows that input i feeds, ascending kk.
template <int VEC>
__global__ __launch_bounds__(KATTN_THREADS) void kattn_backward_kv_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ bias,
    const int *__restrict__ nbr_inv, const float *__restrict__ out, const float *__restrict__ lse,
    const float *__restrict__ delta, const float *__restrict__ dout, int Vin, int K, int H, int D, int G, float scale, float *__restrict__ dk,
    float *__restrict__ dv)
{
    constexpr int N = Lane<VEC>::N;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const long item = (long)blockIdx.x * (KATTN_THREADS / G) + g;
    const bool on = item < (long)Vin * H;
    const int i = on ? (int)(item / H) : 0;
    const int h = on ? (int)(item - (long)i * H) : 0;
    const size_t C = (size_t)H * D, hoff = (size_t)h * D;
    const Item it{C, hoff, H, h, l, G, D};
    float kv[N], vv[N], ak[N], av[N];
    load_slice<VEC>(k + (size_t)i * C + hoff, l, G, D, on, kv);
    load_slice<VEC>(v + (size_t)i * C + hoff, l, G, D, on, vv);
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] = av[j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 4) {
        bool live[4];
        size_t o[4];
        float qr[4][N], dr[4][N], dot[4], dp[4], ls[4], dl[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = (on && k0 + u < K) ? nbr_inv[(size_t)(k0 + u) * Vin + i] : -1;
            live[u] = idx >= 0;
            o[u] = (size_t)(live[u] ? idx : 0);
        }
        query_stage<VEC>(q, dout, out, lse, delta, o, live, it, kv, vv, qr, dr, ls, dl, dot, dp);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!live[u]) continue;
            const float s = fmaf(scale, dot[u], bias ? bias[(size_t)(k0 + u) * H + h] : 0.f);
            const float p = expf(s - ls[u]);
            push_dkv(p, p * (dp[u] - dl[u]), dr[u], qr[u], av, ak);
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) ak[j] *= scale;
    if (dk) store_slice<VEC>(dk + (size_t)i * C + hoff, l, G, D, on, ak);
    if (dv) store_slice<VEC>(dv + (size_t)i * C + hoff, l, G, D, on, av);
}

// the checks all three calls share; 0 when the shape is served
int shape_check(int K, int H, int D)
{
    if (K < 1 || K > KATTN_MAX_K || H < 1 || D < 1 || D > KATTN_MAX_D) return MS3D_E_UNSUPPORTED;
    if ((long)H * D > 0x7fffffffL || (long)K * H > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" {

int ms3d_kattn_rows_per_part(void) { return KATTN_ROWS_PER_PART; }

int ms3d_kattn_dbias_parts(int Vout)
{
    return Vout <= 0 ? 0 : (int)(((long)Vout + KATTN_ROWS_PER_PART - 1) / KATTN_ROWS_PER_PART);
}

size_t ms3d_kattn_dbias_ws_floats(int Vout, int K, int H)
{
    if (K < 1 || H < 1) return 0;
    return (size_t)ms3d_kattn_dbias_parts(Vout) * (size_t)K * (size_t)H;
}

int ms3d_kattn_forward(const float *q, const float *k, const float *v, const float *rel_bias, const int *nbr, int Vout, int K,
                       int H, int D, float scale, float *out, float *lse, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (shape_check(K, H, D)) return MS3D_E_UNSUPPORTED;
    if (Vout <= 0) return 0;
    if (!q || !k || !v || !nbr || !out || !lse) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(q, k, v, out);
    const int G = group_of(D, v4 ? 4 : 1);
    const long per = KATTN_THREADS / G, blocks = ((long)Vout * H + per - 1) / per;
    if (blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, kattn_forward_kernel, (unsigned)blocks, KATTN_THREADS, 0, stream, q, k, v, rel_bias, nbr, Vout, K, H, D, G,
                scale, out, lse);
    return 0;
}

int ms3d_kattn_backward_q(const float *q, const float *k, const float *v, const float *rel_bias, const int *nbr,
                          const float *out, const float *lse, const float *dout, int Vout, int K, int H, int D, float scale,
                          float *dq, float *dbias, float *delta, float *partial_ws, size_t ws_floats, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (shape_check(K, H, D)) return MS3D_E_UNSUPPORTED;
    if (Vout <= 0) return 0;                                          // (dbias is not written: an empty sum is the caller's zero)
    if (!q || !k || !v || !nbr || !out || !lse || !dout || !delta) return MS3D_E_UNSUPPORTED;
    if (dbias && (!rel_bias || !partial_ws)) return MS3D_E_UNSUPPORTED;
    if (dbias && ws_floats < ms3d_kattn_dbias_ws_floats(Vout, K, H)) return MS3D_E_WORKSPACE;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(q, k, v, out, dout, dq);
    const int G = group_of(D, v4 ? 4 : 1);
    int GPB = KATTN_THREADS / G;                                      // groups of a workgroup: a power of two
    if (dbias)
        while (2 * GPB * K > KATTN_DB_FLOATS) GPB /= 2;               // (K <= 254: GPB >= 32 or 256 / G)
    const int HB = H < GPB ? H : GPB, RG = GPB / HB;
    const int parts = ms3d_kattn_dbias_parts(Vout), tiles = (H + HB - 1) / HB;
    if (tiles > 65535) return MS3D_E_UNSUPPORTED;
    const dim3 grid((unsigned)parts, (unsigned)tiles);
    const int T = GPB * G;
    const size_t lds = dbias ? sizeof(float) * 2 * (size_t)GPB * K : 0;
    float *partial = dbias ? partial_ws : nullptr;
    MS3D_LAUNCH_VEC(v4, kattn_backward_q_kernel, grid, T, lds, stream, q, k, v, rel_bias, nbr, out, lse, dout, Vout, K, H, D, G, HB,
                RG, scale, dq, delta, partial);
    if (dbias) {
        const int n = K * H;
        kattn_dbias_reduce_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(partial_ws, parts, n, dbias);
        MS3D_LAUNCH_CHECK();
    }
    return 0;
}

int ms3d_kattn_backward_kv(const float *q, const float *k, const float *v, const float *rel_bias, const int *nbr_inv,
                           const float *out, const float *lse, const float *delta, const float *dout, int Vin, int K, int H,
                           int D, float scale, float *dk, float *dv, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (shape_check(K, H, D)) return MS3D_E_UNSUPPORTED;
    if (Vin <= 0) return 0;
    if (!q || !k || !v || !nbr_inv || !out || !lse || !delta || !dout || (!dk && !dv)) return MS3D_E_UNSUPPORTED;
    const bool v4 = D % 4 == 0 && ms3d_aligned16(q, k, v, out, dout, dk, dv);
    const int G = group_of(D, v4 ? 4 : 1);
    const long per = KATTN_THREADS / G, blocks = ((long)Vin * H + per - 1) / per;
    if (blocks > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, kattn_backward_kv_kernel, (unsigned)blocks, KATTN_THREADS, 0, stream, q, k, v, rel_bias, nbr_inv, out, lse,
                delta, dout, Vin, K, H, D, G, scale, dk, dv);
    return 0;
}

}  // extern "C"
