// k nearest neighbours per sample: for every query the k rows of its sample with the smallest keys
//
//   key = (distance bits << 32) | CALLER row            the smallest key wins: the nearer row, then the lower caller row
//
// in ascending key order.  The keys of the rows of one sample are distinct, so the k smallest are one set and one order whatever
// way the rows are walked: the result is a pure function of the coordinates and needs no extra pass to be the same bytes on
// every run.  Caller rows are below 2^31 and no distance has all bits set, so the all-ones key is free as "empty".
//
// The support set is read where it is HELD, exactly as csrc/fps.hip reads it: the rows of sample b are
// order[seg_start[b] .. seg_start[b + 1]), the caller row of held row i is row_map[i], or i when row_map is NULL.  The queries
// come packed: 32-bit words [N_q][4] = (segment, x, y, z), grouped by segment, the queries of segment b at q_start[b] ..
// q_start[b + 1].  out_idx [N_q][k] holds caller rows, out_d2 [N_q][k] the distance bits; a slot no row qualified for holds -1
// and the bits of "none" (i32: all ones, f32: +inf), after every qualifying slot.
//
// Distances are those of csrc/fps.hip.  ms3d_knn_i32: the exact integer dx^2 + dy^2 + dz^2 in UNSIGNED 32-bit arithmetic (up to
// 3 * 32767^2 = 3 221 028 867 over the packable range [-16384, 16384)); |dx| < 2^15 there, so the 24-bit multiply-adds are
// exact.  ms3d_knn_f32: d = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x, every operation rounded to float32 on its own
// (dist_f32 switches contraction off for its body).  A non-negative float32 orders like its bits, so both entry points share
// every line below but dist().  A row qualifies when its distance is <= the cap (the boundary included).
//
// Two launches, no atomics, no spin, no grid barrier, no workgroup waits for another; every loop is counted.
//   pack    the support set into the workspace in segment order, 16 B a row (x, y, z, caller row): position p of `order` goes
//           to ws[p].  Every position of [0, V) is written, so the workspace is never assumed zero; `order` entries are clamped
//           here, and nowhere else is an index followed.
//   search  grid (groups of the sample with most queries, B): workgroup (g, b) takes queries g * KNN_QUERIES .. of sample b, a
//           thread a query -- the "tile list" is the block index, host arithmetic on the cached lengths; a group past its
//           sample's queries leaves at once.  The group streams the sample's packed rows through LDS in tiles of KNN_TILE rows
//           (the next tile is loaded into registers while this one is searched); every thread reads the same row, a broadcast.
//           A tile is not a run of consecutive rows but every tiles-th row of the sample (see `tiles` below): the order the
//           rows are walked in changes nothing in the result and much in the number of insertions.
//           A thread keeps its current worst key in a register; only a row below it is a candidate.  Candidates are not
//           inserted where they are met -- one lane's insertion would hold up the other 63 -- but stashed (their position in the
//           tile, KNN_STASH a lane) and inserted by all lanes together when a lane's stash fills up and at the end of a tile: the
//           work of a wave is then the longest lane's, not the sum over the lanes.  The list of a thread's k smallest keys
//           lives in LDS in column layout list[j][thread], unsorted while rows stream by: a candidate takes the place of the
//           largest key and k independent reads find the new largest; at the end a key's slot is the number of keys below it.
#include <string.h>
#include "points.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int KNN_QUERIES = MS3D_WAVE;      // queries of a group = threads of a workgroup: one wave
constexpr int KNN_TILE = 512;               // rows of the support set in LDS at a time
constexpr int KNN_ROWS_PER_LANE = KNN_TILE / KNN_QUERIES;
constexpr int KNN_MAX_K = 64;
constexpr int KNN_MAX_B = 65535;            // gridDim.y
constexpr int KNN_STASH = 16;               // candidates a lane holds back
constexpr int KNN_UNROLL = 4;               // rows between two looks at the stashes
constexpr int KNN_PACK_THREADS = 256;
constexpr unsigned long long KNN_EMPTY = ~0ull;
constexpr unsigned KNN_F32_INF = 0x7f800000u;

static_assert(KNN_TILE % KNN_QUERIES == 0 && KNN_TILE % KNN_UNROLL == 0 && KNN_STASH > KNN_UNROLL, "tile geometry");

// F32: dist_f32 of points.h, the distance of csrc/fps.hip.  Integers: 24-bit products here, plain 32-bit ones in csrc/fps.hip --
// the same bits over the packable range; the two are kept apart because which is faster there has not been measured.
template <bool F32> __device__ __forceinline__ unsigned dist(unsigned qx, unsigned qy, unsigned qz, unsigned px, unsigned py,
                                                             unsigned pz)
{
    if constexpr (F32) {
        return __float_as_uint(dist_f32(__uint_as_float(qx), __uint_as_float(qy), __uint_as_float(qz), __uint_as_float(px),
                                        __uint_as_float(py), __uint_as_float(pz)));
    } else {      // |dx| < 2^15 over the packable range: signed 24-bit products are exact, the sum is exact modulo 2^32
        const int dx = (int)(qx - px), dy = (int)(qy - py), dz = (int)(qz - pz);
        return (unsigned)__mul24(dx, dx) + (unsigned)__mul24(dy, dy) + (unsigned)__mul24(dz, dz);
    }
}

// data [V][4]: int32 (batch, x, y, z) or float (batch, x, y, z), both read as 32-bit words -> ws [V] of (x, y, z, caller row)
__global__ __launch_bounds__(KNN_PACK_THREADS) void knn_pack_kernel(const unsigned *__restrict__ data,
                                                                    const long long *__restrict__ order,
                                                                    const int *__restrict__ row_map, int V, uint4 *__restrict__ ws)
{
    const long p = (long)blockIdx.x * KNN_PACK_THREADS + threadIdx.x;
    if (p >= V) return;
    const long h = held_row(order, p, V);
    ws[p] = make_uint4(data[4 * h + 1], data[4 * h + 2], data[4 * h + 3], row_map ? (unsigned)row_map[h] : (unsigned)h);
}

template <bool F32>
__global__ __launch_bounds__(KNN_QUERIES) void knn_kernel(const uint4 *__restrict__ sup, const int *__restrict__ seg_start,
                                                          const unsigned *__restrict__ queries, const int *__restrict__ q_start,
                                                          int V, int NQ, int k, unsigned cap, long long *__restrict__ out_idx,
                                                          unsigned *__restrict__ out_d2)
{
    extern __shared__ __align__(16) unsigned char lds[];
    uint4 *const tile = reinterpret_cast<uint4 *>(lds);                                                     // [KNN_TILE]
    unsigned long long *const list = reinterpret_cast<unsigned long long *>(lds + sizeof(uint4) * KNN_TILE);   // [k][KNN_QUERIES]
    unsigned *const stash = reinterpret_cast<unsigned *>(list + (size_t)k * KNN_QUERIES);                    // [KNN_STASH][KNN_QUERIES]

    const int b = blockIdx.y, t = threadIdx.x;
    const int s = clamp_to(seg_start[b], V), n = clamp_to(seg_start[b + 1], V) - s;
    const int qe = clamp_to(q_start[b + 1], NQ);
    const long q0 = (long)clamp_to(q_start[b], NQ) + (long)blockIdx.x * KNN_QUERIES;
    if (q0 >= qe) return;      // the whole workgroup: no barrier is left waiting
    const long q = q0 + t;
    const bool live = q < qe;
    unsigned qx = 0, qy = 0, qz = 0;
    bool mine = false;      // a query filed under another segment than its own, or under none, gets -1 slots
    if (live) {
        mine = queries[4 * q] == (unsigned)b;
        qx = queries[4 * q + 1], qy = queries[4 * q + 2], qz = queries[4 * q + 3];
    }
    for (int j = 0; j < k; j++) list[j * KNN_QUERIES + t] = KNN_EMPTY;
    // a key qualifies below `limit`: distance <= cap (without a cap every real key, the empty one is the largest there is)
    const unsigned long long limit = cap == 0xffffffffu ? KNN_EMPTY : ((unsigned long long)cap + 1) << 32;
    // worst = min(the largest key of the list, limit): a row below it is a candidate; at = where that largest key is
    unsigned long long worst = mine ? limit : 0ull;      // no key is below 0: such a lane never has a candidate
    int at = 0;
    int held = 0;                                        // candidates in this lane's stash

    // the candidates of every lane go into its list, all lanes together.  The list is kept UNSORTED while rows stream by: a
    // candidate takes the place of the largest key, then k reads that do not wait for one another find the new largest --
    // shifting a sorted list up is k / 2 dependent read-compare-write steps an insertion.  The order is made at the end.
    auto flush = [&]() {
        for (int i = 0; i < held; i++) {
            const uint4 p = tile[stash[i * KNN_QUERIES + t]];
            const unsigned long long key = ((unsigned long long)dist<F32>(qx, qy, qz, p.x, p.y, p.z) << 32) | p.w;
            if (key < worst) {      // the worst key may have come down since the row was stashed
                list[at * KNN_QUERIES + t] = key;
                unsigned long long big = 0;
#pragma unroll 8
                for (int j = 0; j < k; j++) {
                    const unsigned long long v = list[j * KNN_QUERIES + t];
                    if (v >= big) big = v, at = j;
                }
                worst = big < limit ? big : limit;
            }
        }
        held = 0;
    };

    uint4 next[KNN_ROWS_PER_LANE];
    // tile j of a sample of `tiles` tiles holds its rows j, j + tiles, j + 2 tiles, ...: slot i is row i * tiles + j.  Every
    // tile is then an even subsample of the whole segment, however its rows are ordered (a Morton-sorted manager holds them
    // along a space-filling curve: walked in that order a query's nearest rows so far are replaced again and again while the
    // walk closes in on it, thousands of insertions instead of about k ln(V_b / k)).
    const int tiles = (n + KNN_TILE - 1) / KNN_TILE;
    auto load = [&](int j) {
#pragma unroll
        for (int i = 0; i < KNN_ROWS_PER_LANE; i++) {
            const long r = (long)(t + i * KNN_QUERIES) * tiles + j;
            next[i] = r < n ? sup[(size_t)s + r] : make_uint4(0, 0, 0, 0);      // slots past the sample are never looked at
        }
    };

    if (n > 0) load(0);
    for (int j = 0; j < tiles; j++) {
        const int m = (n - j + tiles - 1) / tiles;      // the slots of this tile that hold a row: a prefix, at most KNN_TILE
        __syncthreads();      // the last tile has been searched
#pragma unroll
        for (int i = 0; i < KNN_ROWS_PER_LANE; i++) tile[t + i * KNN_QUERIES] = next[i];
        __syncthreads();
        if (j + 1 < tiles) load(j + 1);
        for (int r = 0; r < m; r += KNN_UNROLL) {
#pragma unroll
            for (int u = 0; u < KNN_UNROLL; u++) {
                const uint4 p = tile[r + u];      // r + u < KNN_TILE
                const unsigned d = dist<F32>(qx, qy, qz, p.x, p.y, p.z);
                const unsigned long long key = ((unsigned long long)d << 32) | p.w;
                if (r + u < m && key < worst) stash[held++ * KNN_QUERIES + t] = (unsigned)(r + u);
            }
            if (__any(held > KNN_STASH - KNN_UNROLL)) flush();      // every lane has room for the next KNN_UNROLL rows
        }
        flush();      // the stash names rows of this tile
    }

    // a key's slot is the number of keys below it (real keys are distinct; empty ones keep their order among themselves)
    if (live) {
        const unsigned none = F32 ? KNN_F32_INF : 0xffffffffu;
        for (int i = 0; i < k; i++) {
            const unsigned long long key = list[i * KNN_QUERIES + t];
            int slot = 0;
#pragma unroll 8
            for (int j = 0; j < k; j++) {
                const unsigned long long v = list[j * KNN_QUERIES + t];
                slot += (v < key || (v == key && j < i)) ? 1 : 0;
            }
            out_idx[(size_t)q * k + slot] = key == KNN_EMPTY ? -1ll : (long long)(unsigned)key;
            out_d2[(size_t)q * k + slot] = key == KNN_EMPTY ? none : (unsigned)(key >> 32);
        }
    }
}

size_t lds_bytes(int k)
{
    return sizeof(uint4) * KNN_TILE + sizeof(unsigned long long) * KNN_QUERIES * (size_t)k + sizeof(unsigned) * KNN_QUERIES * KNN_STASH;
}
static_assert(sizeof(uint4) * KNN_TILE + sizeof(unsigned long long) * KNN_QUERIES * KNN_MAX_K +
                      sizeof(unsigned) * KNN_QUERIES * KNN_STASH <= 64 * 1024,
              "the kernel stays below the default dynamic-LDS limit");

template <bool F32>
int knn_launch(const void *data, const long long *order, const int *seg_start, const int *row_map, int V, int B,
               const void *queries, const int *q_start, int NQ, int max_queries, int k, unsigned cap, long long *out_idx,
               void *out_d2, void *ws, size_t ws_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 0 || B < 0 || B > KNN_MAX_B || NQ < 0 || max_queries < 0 || k < 1 || k > KNN_MAX_K) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0 || NQ == 0 || max_queries == 0) return 0;
    if (!data || !order || !seg_start || !queries || !q_start || !out_idx || !out_d2 || !ws || ((uintptr_t)ws & 15))
        return MS3D_E_UNSUPPORTED;
    if (ws_bytes < ms3d_knn_ws_bytes(V)) return MS3D_E_WORKSPACE;
    hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)ms3d_divup(V, KNN_PACK_THREADS)), dim3(KNN_PACK_THREADS), 0, stream,
                       (const unsigned *)data, order, row_map, V, (uint4 *)ws);
    MS3D_LAUNCH_CHECK();
    const int groups = ms3d_divup(max_queries < NQ ? max_queries : NQ, KNN_QUERIES);
    hipLaunchKernelGGL(knn_kernel<F32>, dim3((unsigned)groups, (unsigned)B), dim3(KNN_QUERIES), lds_bytes(k), stream,
                       (const uint4 *)ws, seg_start, (const unsigned *)queries, q_start, V, NQ, k, cap, out_idx,
                       (unsigned *)out_d2);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int ms3d_knn_max_k(void) { return KNN_MAX_K; }
int ms3d_knn_queries_per_group(void) { return KNN_QUERIES; }
int ms3d_knn_rows_per_tile(void) { return KNN_TILE; }

size_t ms3d_knn_ws_bytes(long V) { return V <= 0 ? 0 : sizeof(uint4) * (size_t)V; }

int ms3d_knn_i32(const int *coords, const long long *order, const int *seg_start, const int *row_map, int V, int B,
                 const int *queries, const int *q_start, int NQ, int max_queries, int k, long long max_d2, long long *out_idx,
                 unsigned *out_d2, void *ws, size_t ws_bytes, ms3d_stream_t stream)
{
    const unsigned cap = (max_d2 < 0 || max_d2 > 0xffffffffll) ? 0xffffffffu : (unsigned)max_d2;
    return knn_launch<false>(coords, order, seg_start, row_map, V, B, queries, q_start, NQ, max_queries, k, cap, out_idx, out_d2,
                             ws, ws_bytes, stream);
}

int ms3d_knn_f32(const float *points, const long long *order, const int *seg_start, const int *row_map, int V, int B,
                 const int *queries, const int *q_start, int NQ, int max_queries, int k, float max_d2, long long *out_idx,
                 float *out_d2, void *ws, size_t ws_bytes, ms3d_stream_t stream)
{
    unsigned cap = KNN_F32_INF;      // no cap: every finite distance qualifies
    if (max_d2 >= 0.0f) memcpy(&cap, &max_d2, sizeof cap);
    return knn_launch<true>(points, order, seg_start, row_map, V, B, queries, q_start, NQ, max_queries, k, cap, out_idx, out_d2,
                            ws, ws_bytes, stream);
}

}  // extern "C"
