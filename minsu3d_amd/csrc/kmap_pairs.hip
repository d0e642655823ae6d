// Kernel maps as index pairs: an offset-major table nbr[K][Vout] (int32, -1 = none) exported as the packed per-offset pair
// lists a caller indexes feature rows with,
//   start[K + 1]   int32   start[k] = first pair of offset k, start[K] = P = number of valid entries
//   pairs[2][P]    int64   row 0 the VISIBLE input row, row 1 the VISIBLE output row; offset k owns columns start[k] ..
//                          start[k + 1], ascending in the visible output row
// with the caller's row numbering folded in: out_order[j] = the held row of visible output row j, in_rename[i] = the visible
// row of held input row i (either NULL = identity).  The pair of (k, j) exists when v = nbr[k][out_order[j]] lies in [0, Vin);
// it is (in_rename[v], j).  An entry >= Vin (or an out_order entry outside [0, Vout)) is never followed: it counts as -1.
//
// Decomposition (the habit of the coordinate engine: flag -> scan -> emit, no sort, no atomics):
//   1. kp_count_kernel   grid (runs, K), one workgroup of 256 threads per (offset k, run of KP_ROWS = 1024 visible output
//                        rows).  Wave w of the block owns the 256 consecutive rows w * 256 .. of the run and walks them in 4
//                        steps of 64: consecutive lanes read consecutive rows (out_order: coalesced 4-byte reads; the table
//                        row itself is a gather only when out_order is given).  Per step one ballot + popcount; the four
//                        wave totals meet in LDS and thread 0 stores ONE int: counts[k * runs + run] (k-major).
//   2. ms3d_exclusive_scan_i32 over the K * runs counts, in place; its total goes straight into start[K].
//   3. kp_starts_kernel  K threads: start[k] = scanned[k * runs].
//   (the host reads start[K] once and allocates pairs at its exact size)
//   4. kp_fill_kernel    the same decomposition.  Every thread keeps its 4 table entries in registers (the table is read once
//                        per pass, twice in all), recomputes the ballots, the wave totals meet in LDS once, and the base of a
//                        wave is scanned[k * runs + run] + the totals of the waves before it.  Inside a step the rank of a lane
//                        is the mbcnt of the ballot; the 64-bit stores of a step go to consecutive columns of both rows.
// Every slot of start and pairs has exactly one writer and its position depends on the table alone: the same bytes on every
// run.  Memory-bound: 2 x 4 bytes read per table entry (plus the order / rename reads), 16 bytes written per pair.
//
// Range: K * Vout <= 2^31 - 1 is required (refused on the host otherwise), so P and every start fit an int32; positions inside
// the kernels are 64-bit all the same.  K <= 65535 because the offset is the grid's y coordinate.
#include "common.h"
#include "scan.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int KP_THREADS = 256;
constexpr int KP_WAVES = KP_THREADS / 64;
constexpr int KP_STEPS = 4;                        // steps of 64 rows per wave
constexpr int KP_WAVE_ROWS = KP_STEPS * 64;        // 256 consecutive rows per wave
constexpr int KP_ROWS = KP_WAVES * KP_WAVE_ROWS;   // 1024 visible output rows per workgroup

// the valid entry of (offset row nbr_k, visible output row j), or -1
__device__ __forceinline__ int kp_entry(const int *__restrict__ nbr_k, const int *__restrict__ out_order, long long j, int Vout,
                                        int Vin)
{
    if (j >= Vout) return -1;
    const int h = out_order ? out_order[j] : (int)j;
    if ((unsigned)h >= (unsigned)Vout) return -1;
    const int v = nbr_k[h];
    return (unsigned)v < (unsigned)Vin ? v : -1;
}

__device__ __forceinline__ int kp_lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(KP_THREADS) void kp_count_kernel(const int *__restrict__ nbr, int Vout, int Vin,
                                                              const int *__restrict__ out_order, int runs, int *__restrict__ counts)
{
    __shared__ int s_wave[KP_WAVES];
    const int k = blockIdx.y, run = blockIdx.x;
    const int *nbr_k = nbr + (size_t)k * (size_t)Vout;
    const long long j0 = (long long)run * KP_ROWS + wave_id() * KP_WAVE_ROWS + lane_id();
    int c = 0;
#pragma unroll
    for (int s = 0; s < KP_STEPS; s++)
        c += __popcll(__ballot(kp_entry(nbr_k, out_order, j0 + s * 64, Vout, Vin) >= 0));
    if (lane_id() == 0) s_wave[wave_id()] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < KP_WAVES; w++) t += s_wave[w];
        counts[(size_t)k * (size_t)runs + run] = t;
    }
}

__global__ __launch_bounds__(256) void kp_starts_kernel(const int *__restrict__ scanned, int K, int runs, int *__restrict__ start)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) start[k] = scanned[(size_t)k * (size_t)runs];
}

__global__ __launch_bounds__(KP_THREADS) void kp_fill_kernel(const int *__restrict__ nbr, int Vout, int Vin,
                                                             const int *__restrict__ out_order, const int *__restrict__ in_rename,
                                                             int runs, const int *__restrict__ scanned,
                                                             long long *__restrict__ pairs, long long pair_ld)
{
    __shared__ int s_wave[KP_WAVES];
    const int k = blockIdx.y, run = blockIdx.x;
    const int *nbr_k = nbr + (size_t)k * (size_t)Vout;
    const long long j0 = (long long)run * KP_ROWS + wave_id() * KP_WAVE_ROWS + lane_id();
    int v[KP_STEPS];
    unsigned long long m[KP_STEPS];
    int c = 0;
#pragma unroll
    for (int s = 0; s < KP_STEPS; s++) {
        v[s] = kp_entry(nbr_k, out_order, j0 + s * 64, Vout, Vin);
        m[s] = __ballot(v[s] >= 0);
        c += __popcll(m[s]);
    }
    if (lane_id() == 0) s_wave[wave_id()] = c;
    __syncthreads();
    long long base = scanned[(size_t)k * (size_t)runs + run];
#pragma unroll
    for (int w = 0; w < KP_WAVES; w++)
        if (w < wave_id()) base += s_wave[w];
#pragma unroll
    for (int s = 0; s < KP_STEPS; s++) {
        const long long pos = base + kp_lane_rank(m[s]);
        if (v[s] >= 0 && pos < pair_ld) {      // (pos < P always when the arguments are those of the count pass)
            pairs[pos] = in_rename ? (long long)in_rename[v[s]] : (long long)v[s];
            pairs[pair_ld + pos] = j0 + s * 64;
        }
        base += __popcll(m[s]);
    }
}

// 0 when the geometry is one the kernels take, else the code to return
int kp_refuse(int K, int Vout, int Vin)
{
    if (K < 1 || K > 65535 || Vout < 0 || Vin < 0) return MS3D_E_UNSUPPORTED;
    if ((long long)K * (long long)Vout > 2147483647LL) return MS3D_E_UNSUPPORTED;
    return 0;
}

size_t kp_counts_bytes(int K, int Vout) { return ms3d_align(sizeof(int) * (size_t)K * (size_t)ms3d_divup(Vout, KP_ROWS)); }

}  // namespace

extern "C" {

int ms3d_kmap_pairs_rows(void) { return KP_ROWS; }

size_t ms3d_kmap_pairs_workspace_bytes(int K, int Vout)
{
    if (kp_refuse(K, Vout, 0) || Vout == 0) return 0;
    return kp_counts_bytes(K, Vout) + ms3d_scan_workspace_bytes();
}

int ms3d_kmap_pairs_count(const int *nbr, int K, int Vout, int Vin, const int *out_order, int *start, void *workspace,
                          size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > 65535 || Vout < 0 || Vin < 0 || !start) return MS3D_E_UNSUPPORTED;
    if (Vout == 0) return 0;
    if (!nbr || kp_refuse(K, Vout, Vin)) return MS3D_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < ms3d_kmap_pairs_workspace_bytes(K, Vout)) return MS3D_E_WORKSPACE;
    const int runs = ms3d_divup(Vout, KP_ROWS);
    int *counts = (int *)workspace;
    void *scan_ws = (char *)workspace + kp_counts_bytes(K, Vout);
    kp_count_kernel<<<dim3(runs, K), KP_THREADS, 0, stream>>>(nbr, Vout, Vin, out_order, runs, counts);
    MS3D_LAUNCH_CHECK();
    const int rc = ms3d_exclusive_scan_i32(counts, counts, K * runs, start + K, scan_ws, stream);
    if (rc) return rc;
    kp_starts_kernel<<<ms3d_divup(K, 256), 256, 0, stream>>>(counts, K, runs, start);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_pairs_fill(const int *nbr, int K, int Vout, int Vin, const int *out_order, const int *in_rename, long long *pairs,
                         long long pair_ld, const void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > 65535 || Vout < 0 || Vin < 0 || pair_ld < 0) return MS3D_E_UNSUPPORTED;
    if (Vout == 0 || pair_ld == 0) return 0;
    if (!nbr || !pairs || kp_refuse(K, Vout, Vin)) return MS3D_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < ms3d_kmap_pairs_workspace_bytes(K, Vout)) return MS3D_E_WORKSPACE;
    const int runs = ms3d_divup(Vout, KP_ROWS);
    kp_fill_kernel<<<dim3(runs, K), KP_THREADS, 0, stream>>>(nbr, Vout, Vin, out_order, in_rename, runs, (const int *)workspace,
                                                            pairs, pair_ld);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
