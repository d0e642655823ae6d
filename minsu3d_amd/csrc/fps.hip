// Farthest point sampling per sample: the query seeding of a mask-transformer decoder, the grouping stage of a point network.
//
//   pick 0 of sample b = start_held[b], or the sample's lowest CALLER row when start_held is NULL
//   pick j             = the row of the sample whose distance to the nearest of the picks 0 .. j-1 is largest; among equal
//                        distances the lowest caller row; rows already picked have distance 0 and take part like any other
//
// The rows of sample b are order[seg_start[b] .. seg_start[b + 1]) (CoordinateManager.batch_rows), read where they are HELD; the
// caller row of held row i is row_map[i], or i when row_map is NULL.  out [B][M] holds caller rows.  The result is a pure
// function of the coordinate set and the rule: it does not depend on how the rows are held or on the launch shape.
//
// Distances.  ms3d_fps_i32: the exact integer dx^2 + dy^2 + dz^2 in UNSIGNED 32-bit arithmetic -- over the packable range
// [-16384, 16384) it reaches 3 * 32767^2 = 3 221 028 867, above 2^31 and below 2^32.  ms3d_fps_f32: d = (dx*dx + dy*dy) + dz*dz
// with dx = p.x - c.x, every operation rounded to float32 on its own (dist_f32 switches contraction off for its body: an FMA
// changes picks).  A non-negative float32 orders like its bits read as an unsigned integer,
// so both entry points keep distances, running minima and coordinates as 32-bit words and share every line below but dist().
//
// One launch, one workgroup of FPS_THREADS per sample; a workgroup loops over its own segment, so samples of very different
// sizes need nothing from the host, and no workgroup waits for another: no spin, no grid barrier, no atomics.  Every loop is
// counted: M picks of ceil(V_b / rows per sweep step) steps.
//
// One pick: every thread updates the running minimum of its rows against the last pick and keeps its best row as ONE 64-bit key,
// (minimum << 32) | ~caller row -- the larger key is the farther row, then the lower caller row; caller rows are below 2^31, so a
// key of a real row is never 0, the key of a padding slot.  The keys are reduced per wave by shuffles, across the waves through
// LDS (barrier 1); the one thread whose key won writes its row's coordinates to LDS and the caller row to out (barrier 2).
//
// Two bodies, chosen per workgroup by the length of its segment:
//   resident   V_b <= FPS_RESIDENT_ROWS: a thread holds FPS_ROWS_PER_THREAD rows -- coordinates, minimum and caller row -- in
//              registers for the whole loop; after the first gather nothing is read from global memory
//   streaming  larger segments: the segment is gathered once, in segment order, into the workspace as word arrays (i32: x | y
//              << 16, z, minimum, caller row = 16 B a row; f32: x, y, z, minimum, caller row = 20 B a row), then every pick sweeps
//              them with 16-byte accesses, a thread four consecutive rows a step.  A thread meets the same rows in every sweep,
//              so the minima need no barrier.  The workspace is never assumed zero: the gather writes every word the sweeps
//              read, the padding up to a multiple of four rows included (minimum 0, caller row ~0: key 0, for ever).
#include "points.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int FPS_THREADS = 1024;
constexpr int FPS_WAVES = FPS_THREADS / MS3D_WAVE;
constexpr int FPS_ROWS_PER_THREAD = 8;
constexpr int FPS_RESIDENT_ROWS = FPS_THREADS * FPS_ROWS_PER_THREAD;
constexpr int FPS_MAX_B = 65535;
constexpr int FPS_SEG_PAD = 8;   // workspace rows between the starts of two samples beyond their rows: ws_rows_of
constexpr unsigned FPS_F32_INF = 0x7f800000u;

// F32: dist_f32 of points.h.  Integers: plain 32-bit products here, 24-bit ones in csrc/knn.hip -- the same bits over the
// packable range; the two are kept apart because which is faster here has not been measured.
template <bool F32> __device__ __forceinline__ unsigned dist(unsigned x, unsigned y, unsigned z, unsigned cx, unsigned cy,
                                                             unsigned cz)
{
    if constexpr (F32) {
        return __float_as_uint(dist_f32(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z), __uint_as_float(cx),
                                        __uint_as_float(cy), __uint_as_float(cz)));
    } else {
        const unsigned dx = x - cx, dy = y - cy, dz = z - cz;      // two's complement: the squares are exact modulo 2^32
        return dx * dx + dy * dy + dz * dz;
    }
}

__device__ __forceinline__ unsigned long long make_key(unsigned hi, unsigned caller)
{
    return ((unsigned long long)hi << 32) | (unsigned)~caller;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v, int from)
{
#pragma unroll
    for (int d = from; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

struct Pick {
    unsigned long long key;   // the best key of this thread, 0: none
    unsigned x, y, z;         // the coordinates of that row
    __device__ __forceinline__ void offer(unsigned long long k, unsigned px, unsigned py, unsigned pz)
    {
        if (k > key) { key = k; x = px; y = py; z = pz; }
    }
};

struct Shared {
    unsigned long long wave_key[FPS_WAVES];
    unsigned pick[3];
};

// The workgroup's best row: every thread brings its Pick and leaves with the winner's coordinates in (cx, cy, cz); the winner's
// caller row goes to *dst.  Two barriers.  wave_key is written before barrier 1 and read before barrier 2, pick is written
// before barrier 2 and read before the next call's barrier 1, so neither needs a second copy.
__device__ __forceinline__ void choose(const Pick &mine, Shared &sh, long long *dst, unsigned &cx, unsigned &cy, unsigned &cz)
{
    const unsigned long long w = wave_max_u64(mine.key, 32);
    if (lane_id() == 0) sh.wave_key[wave_id()] = w;
    __syncthreads();
    const unsigned long long win = wave_max_u64(sh.wave_key[lane_id() & (FPS_WAVES - 1)], FPS_WAVES / 2);
    if (mine.key == win && win != 0) {      // keys of real rows are distinct: one writer
        sh.pick[0] = mine.x, sh.pick[1] = mine.y, sh.pick[2] = mine.z;
        *dst = (long long)(unsigned)~(unsigned)win;
    }
    __syncthreads();
    cx = sh.pick[0], cy = sh.pick[1], cz = sh.pick[2];
}

// data [V][4]: int32 (batch, x, y, z) for F32 == false, float (batch, x, y, z) for F32 == true -- both read as 32-bit words
template <bool F32>
__global__ __launch_bounds__(FPS_THREADS) void fps_kernel(const unsigned *__restrict__ data, const long long *__restrict__ order,
                                                          const int *__restrict__ seg_start, const int *__restrict__ row_map,
                                                          const long long *__restrict__ start_held, int V, int M,
                                                          long long *__restrict__ out, unsigned *__restrict__ ws, size_t ws_rows)
{
    __shared__ Shared sh;
    const int b = blockIdx.x, t = threadIdx.x;
    const int s = clamp_to(seg_start[b], V), e = clamp_to(seg_start[b + 1], V);
    const int n = e - s;
    if (n <= 0) return;      // the whole workgroup: no barrier is left waiting
    long long *const dst = out + (size_t)b * M;
    const long long want = start_held ? start_held[b] : -1;      // -1: no held row is -1, every row offers hi = 0
    const unsigned inf = F32 ? FPS_F32_INF : 0xffffffffu;
    unsigned cx, cy, cz;
    Pick mine;

    if (n <= FPS_RESIDENT_ROWS) {
        unsigned x[FPS_ROWS_PER_THREAD], y[FPS_ROWS_PER_THREAD], z[FPS_ROWS_PER_THREAD], m[FPS_ROWS_PER_THREAD],
            row[FPS_ROWS_PER_THREAD];
        mine = Pick{0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < FPS_ROWS_PER_THREAD; k++) {
            const int p = t + k * FPS_THREADS;
            x[k] = y[k] = z[k] = m[k] = 0, row[k] = 0xffffffffu;      // a padding slot: key 0, for ever
            if (p < n) {
                const long h = held_row(order, (long)s + p, V);
                x[k] = data[4 * h + 1], y[k] = data[4 * h + 2], z[k] = data[4 * h + 3];
                m[k] = inf, row[k] = row_map ? (unsigned)row_map[h] : (unsigned)h;
                mine.offer(make_key(h == want ? 1u : 0u, row[k]), x[k], y[k], z[k]);
            }
        }
        choose(mine, sh, dst, cx, cy, cz);
        for (int j = 1; j < M; j++) {
            mine = Pick{0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < FPS_ROWS_PER_THREAD; k++) {
                m[k] = min(m[k], dist<F32>(x[k], y[k], z[k], cx, cy, cz));
                mine.offer(make_key(m[k], row[k]), x[k], y[k], z[k]);
            }
            choose(mine, sh, dst + j, cx, cy, cz);
        }
        return;
    }

    // streaming: word arrays of ws_rows rows each; this sample's rows start at a multiple of four rows
    const size_t row0 = (((size_t)s + 3) & ~(size_t)3) + (size_t)FPS_SEG_PAD * b;
    const int n4 = (n + 3) & ~3;
    constexpr int NA = F32 ? 3 : 2;      // coordinate arrays
    unsigned *const a0 = ws + row0, *const a1 = a0 + ws_rows, *const a2 = a1 + (NA == 3 ? ws_rows : 0);
    unsigned *const wm = ws + NA * ws_rows + row0, *const wr = wm + ws_rows;
    mine = Pick{0, 0, 0, 0};
    for (long p = t; p < n4; p += FPS_THREADS) {
        unsigned px = 0, py = 0, pz = 0, pm = 0, pr = 0xffffffffu;
        if (p < n) {
            const long h = held_row(order, (long)s + p, V);
            px = data[4 * h + 1], py = data[4 * h + 2], pz = data[4 * h + 3];
            pm = inf, pr = row_map ? (unsigned)row_map[h] : (unsigned)h;
            mine.offer(make_key(h == want ? 1u : 0u, pr), px, py, pz);
        }
        if constexpr (F32) {
            a0[p] = px, a1[p] = py, a2[p] = pz;
        } else {
            a0[p] = (px & 0xffffu) | (py << 16), a1[p] = pz;
        }
        wm[p] = pm, wr[p] = pr;
    }
    choose(mine, sh, dst, cx, cy, cz);      // its first barrier also orders the gather before the sweeps
    for (int j = 1; j < M; j++) {
        mine = Pick{0, 0, 0, 0};
        for (long p = 4 * t; p < n4; p += 4 * FPS_THREADS) {
            const uint4 v0 = *reinterpret_cast<const uint4 *>(a0 + p), v1 = *reinterpret_cast<const uint4 *>(a1 + p);
            uint4 vm = *reinterpret_cast<const uint4 *>(wm + p);
            const uint4 vr = *reinterpret_cast<const uint4 *>(wr + p);
            const unsigned w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w}, r[4] = {vr.x, vr.y, vr.z, vr.w};
            unsigned mm[4] = {vm.x, vm.y, vm.z, vm.w}, w2[4] = {0, 0, 0, 0};
            if constexpr (F32) {
                const uint4 v2 = *reinterpret_cast<const uint4 *>(a2 + p);
                w2[0] = v2.x, w2[1] = v2.y, w2[2] = v2.z, w2[3] = v2.w;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                unsigned px, py, pz;
                if constexpr (F32) {
                    px = w0[u], py = w1[u], pz = w2[u];
                } else {      // sign-extend the 16-bit halves
                    px = (unsigned)(int)(short)(w0[u] & 0xffffu), py = (unsigned)((int)w0[u] >> 16), pz = w1[u];
                }
                mm[u] = min(mm[u], dist<F32>(px, py, pz, cx, cy, cz));
                mine.offer(make_key(mm[u], r[u]), px, py, pz);
            }
            vm.x = mm[0], vm.y = mm[1], vm.z = mm[2], vm.w = mm[3];
            *reinterpret_cast<uint4 *>(wm + p) = vm;
        }
        choose(mine, sh, dst + j, cx, cy, cz);
    }
}

// rows of every word array of the workspace: sample b starts at align4(seg_start[b]) + FPS_SEG_PAD * b and takes its rows
// rounded up to four -- at most seg_start[b] + 3 + FPS_SEG_PAD * b + len_b + 3 < the start of sample b + 1
size_t ws_rows_of(long V, int B) { return (((size_t)V + 3) & ~(size_t)3) + (size_t)FPS_SEG_PAD * ((size_t)B + 1); }

template <bool F32>
int fps_launch(const void *data, const long long *order, const int *seg_start, const int *row_map, const long long *start_held,
               int V, int B, int M, long long *out, void *ws, size_t ws_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 0 || B < 0 || B > FPS_MAX_B || M < 1) return MS3D_E_UNSUPPORTED;
    if (V == 0 || B == 0) return 0;
    if (!data || !order || !seg_start || !out || !ws || ((uintptr_t)ws & 15)) return MS3D_E_UNSUPPORTED;
    if (ws_bytes < ms3d_fps_ws_bytes(V, B)) return MS3D_E_WORKSPACE;
    hipLaunchKernelGGL(fps_kernel<F32>, dim3((unsigned)B), dim3(FPS_THREADS), 0, stream, (const unsigned *)data, order, seg_start,
                       row_map, start_held, V, M, out, (unsigned *)ws, ws_rows_of(V, B));
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int ms3d_fps_resident_rows(void) { return FPS_RESIDENT_ROWS; }

size_t ms3d_fps_ws_bytes(long V, int B)
{
    if (V <= 0 || B <= 0) return 0;
    return 5 * sizeof(unsigned) * ws_rows_of(V, B);      // the five word arrays of the float body; the integer body uses four
}

int ms3d_fps_i32(const int *coords, const long long *order, const int *seg_start, const int *row_map,
                 const long long *start_held, int V, int B, int M, long long *out, void *ws, size_t ws_bytes,
                 ms3d_stream_t stream)
{
    return fps_launch<false>(coords, order, seg_start, row_map, start_held, V, B, M, out, ws, ws_bytes, stream);
}

int ms3d_fps_f32(const float *points, const long long *order, const int *seg_start, const int *row_map,
                 const long long *start_held, int V, int B, int M, long long *out, void *ws, size_t ws_bytes,
                 ms3d_stream_t stream)
{
    return fps_launch<true>(points, order, seg_start, row_map, start_held, V, B, M, out, ws, ws_bytes, stream);
}

}  // extern "C"
