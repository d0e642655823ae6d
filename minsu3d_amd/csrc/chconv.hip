// Channel-wise (depthwise) sparse convolution over the engine's offset-major kernel maps: a per-offset, per-channel weight
// w [K, C] instead of the [K, Cin, Cout] matrices of csrc/spconv.hip.  float32 throughout, no matrix product anywhere.
//
// Every direction is a GATHER with one writer per element, so nothing adds floats atomically and a step stays
// bit-reproducible:
//   forward        out[o, c] = bias[c] + sum_k w[k, c] * in[nbr[k][o], c]          over the present inputs, ascending k
//   backward-data  din[i, c] =           sum_k w[k, c] * dout[nbr_inv[k][i], c]    THE SAME KERNEL through the inverse table
//                                                                                  (nbr_inv[k][i] names the output row that
//                                                                                  input i feeds through offset k, so the
//                                                                                  offset index is not mirrored), bias NULL
//   backward-weight  dW[k, c] = sum_o in[nbr[k][o], c] * dout[o, c]                two stages: a [K, C] partial per fixed run
//                                                                                  of CHCONV_WGRAD_ROWS output rows, then the
//                                                                                  partials summed in ascending part order
// Layout: csrc/rows.h, with the rows cut into channel tiles, so a lane's accesses are the header's pointer forms.
// Channels are cut into tiles of at most 64 (blockIdx.y), so that the weights of a tile ([K <= 254][64] floats <= 64 KiB)
// always fit the LDS of a forward workgroup and the staged dout rows of a run ([128][64] floats = 32 KiB) that of a
// backward-weight workgroup, whatever C is.
#include "rows.h"
#include "../../include/minsu3d_hip.h"

namespace {

using namespace ms3d_rows;

constexpr int CHCONV_MAX_K = 254;        // the pooling kernels' limit (their uint8 argmax); the same tables feed both
constexpr int CHCONV_TILE_C = 64;        // channels per tile at most
constexpr int CHCONV_FWD_PASSES = 4;     // row passes of a forward workgroup per fill of its weight tile
constexpr int CHCONV_WGRAD_ROWS = 128;   // output rows per backward-weight partial: a constant of the library, NOT derived
                                         // from the grid or the CU count -- the order of the sum is the same on every machine

// the channel tiling both kernels share: ntiles = ceil(C / 64) tiles of TC channels (a multiple of VEC), LPR lanes per row
struct Tiling { int ntiles, TC, LPR; };
Tiling tiling_of(int C, int VEC)
{
    Tiling t;
    t.ntiles = (C + CHCONV_TILE_C - 1) / CHCONV_TILE_C;
    const int per = (C + t.ntiles - 1) / t.ntiles;
    t.TC = (per + VEC - 1) / VEC * VEC;
    t.LPR = t.TC / VEC;
    return t;
}

// One workgroup: the channel tile blockIdx.y and CHCONV_FWD_PASSES * (256 / LPR) consecutive output rows.  The tile's
// weights are copied to LDS once ([K][TC], read back as one ds_read_b128 per lane and offset); the K table entries of a row
// are read four at a time so that four row gathers are in flight per lane.  The sum runs over ascending k with one fmaf per
// present input in BOTH vector widths: the scalar route gives the same bits as the 16-byte one.
template <int VEC>
__global__ __launch_bounds__(256) void chconv_forward_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                             const float *__restrict__ bias, const int *__restrict__ nbr,
                                                             int Vout, int K, int C, int TC, int LPR, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_w[];        // [K][TC]
    const int c0 = blockIdx.y * TC;
    const int tc = min(TC, C - c0);                                    // channels of this tile (a multiple of VEC)
    for (int e = threadIdx.x; e < K * TC; e += 256) {
        const int k = e / TC, c = e - k * TC;
        s_w[e] = c < tc ? w[(size_t)k * C + c0 + c] : 0.f;
    }
    __syncthreads();
    const int rows_per_pass = 256 / LPR;
    const int r = threadIdx.x / LPR, l = threadIdx.x - r * LPR;
    const int lc = l * VEC;                                            // first channel of this lane inside the tile
    if (r >= rows_per_pass || lc >= tc) return;
    float b[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) b[j] = bias ? bias[c0 + lc + j] : 0.f;
    const long row0 = (long)blockIdx.x * (CHCONV_FWD_PASSES * rows_per_pass);
    for (int pass = 0; pass < CHCONV_FWD_PASSES; pass++) {
        const long ol = row0 + (long)pass * rows_per_pass + r;
        if (ol >= Vout) return;
        const int o = (int)ol;
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) acc[j] = b[j];
        for (int k0 = 0; k0 < K; k0 += 4) {
            int idx[4];
            float v[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; u++) idx[u] = k0 + u < K ? nbr[(size_t)(k0 + u) * Vout + o] : -1;
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int j = 0; j < VEC; j++) v[u][j] = 0.f;
                if (idx[u] >= 0) load_vec<VEC>(in + (size_t)idx[u] * C + c0 + lc, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (idx[u] < 0) continue;
                float wk[VEC];
                load_vec<VEC>(s_w + (k0 + u) * TC + lc, wk);
#pragma unroll
                for (int j = 0; j < VEC; j++) acc[j] = fmaf(wk[j], v[u][j], acc[j]);
            }
        }
        store_vec<VEC>(out + (size_t)o * C + c0 + lc, acc);
    }
}

// Stage one of the backward-weight pass.  One workgroup: the run of CHCONV_WGRAD_ROWS output rows blockIdx.x and the channel
// tile blockIdx.y.  The run's dout rows are staged in LDS once and reused by every offset.  Wave w takes the offsets
// k = w, w + 4, ...: ONE accumulator (VEC floats) per lane whatever K is.  A wave's 64 lanes are G groups of LPR lanes (G a
// power of two); group g takes the rows g, g + G, g + 2G, ... of the run in ascending order, four gathers in flight, and the
// G group sums are then folded by a fixed shuffle tree.  The table entries of (k, 64 rows) are one coalesced load, handed to
// the groups by shuffles.  partial [parts][K][C]: every element written by exactly one lane, nothing read back here.
template <int VEC>
__global__ __launch_bounds__(256) void chconv_wgrad_partial_kernel(const float *__restrict__ in, const float *__restrict__ dout,
                                                                   const int *__restrict__ nbr, int Vout, int K, int C, int TC,
                                                                   int LPR, int G, float *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float s_d[CHCONV_WGRAD_ROWS * CHCONV_TILE_C];      // [rows][TC]
    const int c0 = blockIdx.y * TC;
    const int tc = min(TC, C - c0);
    const long r0 = (long)blockIdx.x * CHCONV_WGRAD_ROWS;
    for (int e = threadIdx.x; e < CHCONV_WGRAD_ROWS * TC; e += 256) {
        const int j = e / TC, c = e - j * TC;
        s_d[e] = (r0 + j < Vout && c < tc) ? dout[(size_t)(r0 + j) * C + c0 + c] : 0.f;
    }
    __syncthreads();
    const int lane = lane_id(), wave = wave_id();
    const int g = lane / LPR, l = lane - g * LPR;
    const int lc = l * VEC;
    const bool active = g < G && lc < tc;
    const int steps = 64 / G;                       // rows of a 64-row chunk per group
    float *__restrict__ dst = partial + (size_t)blockIdx.x * K * C;
    for (int k = wave; k < K; k += 4) {             // (wave-uniform: the shuffles below see all 64 lanes)
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) acc[j] = 0.f;
        for (int chunk = 0; chunk < CHCONV_WGRAD_ROWS / 64; chunk++) {
            const long row = r0 + chunk * 64 + lane;
            const int mine = row < Vout ? nbr[(size_t)k * Vout + row] : -1;
            for (int s0 = 0; s0 < steps; s0 += 4) {
                int idx[4], jr[4];
                float v[4][VEC];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    jr[u] = (s0 + u) * G + (g < G ? g : 0);                    // row of the chunk; < 64 when s0 + u < steps
                    const int t = __shfl(mine, jr[u] & 63, 64);
                    idx[u] = (active && s0 + u < steps) ? t : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
#pragma unroll
                    for (int j = 0; j < VEC; j++) v[u][j] = 0.f;
                    if (idx[u] >= 0) load_vec<VEC>(in + (size_t)idx[u] * C + c0 + lc, v[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (idx[u] < 0) continue;
                    float d[VEC];
                    load_vec<VEC>(s_d + (chunk * 64 + jr[u]) * TC + lc, d);
#pragma unroll
                    for (int j = 0; j < VEC; j++) acc[j] = fmaf(v[u][j], d[j], acc[j]);
                }
            }
        }
        // fold the G groups: group g adds group g + s (s = G/2 ... 1); idle lanes carry zeros and are never read
        for (int s = G >> 1; s >= 1; s >>= 1) {
#pragma unroll
            for (int j = 0; j < VEC; j++) {
                const float t = __shfl_down(acc[j], s * LPR, 64);
                if (g < s) acc[j] += t;
            }
        }
        if (g == 0 && lc < tc) store_vec<VEC>(dst + (size_t)k * C + c0 + lc, acc);
    }
}

// Stage two: dW[e] = sum_p partial[p][e], p ascending, one thread per element (ms3d_reduce_partials folds 64 interleaved
// part lanes instead, which is a fixed order but not the ascending one).  Summed in double, rounded once.
__global__ __launch_bounds__(256) void chconv_wgrad_reduce_kernel(const float *__restrict__ partial, int parts, int n,
                                                                  float *__restrict__ dW)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int p = 0; p < parts; p++) s += (double)partial[(size_t)p * n + e];
    dW[e] = (float)s;
}

}  // namespace

extern "C" {

int ms3d_chconv_wgrad_rows_per_part(void) { return CHCONV_WGRAD_ROWS; }

int ms3d_chconv_wgrad_parts(int Vout)
{
    return Vout <= 0 ? 0 : (int)(((long)Vout + CHCONV_WGRAD_ROWS - 1) / CHCONV_WGRAD_ROWS);
}

size_t ms3d_chconv_wgrad_ws_floats(int Vout, int K, int C)
{
    if (K < 1 || C < 1) return 0;
    return (size_t)ms3d_chconv_wgrad_parts(Vout) * (size_t)K * (size_t)C;
}

int ms3d_chconv_forward(const float *in, const float *w, const float *bias, const int *nbr, int Vout, int K, int C, float *out,
                        ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > CHCONV_MAX_K || C < 1) return MS3D_E_UNSUPPORTED;
    if (Vout <= 0) return 0;
    const bool v4 = vec4(C, in, out);
    const Tiling t = tiling_of(C, v4 ? 4 : 1);
    const int rows_per_block = CHCONV_FWD_PASSES * (256 / t.LPR);
    const long blocks = ((long)Vout + rows_per_block - 1) / rows_per_block;
    if (blocks > 0x7fffffffL || t.ntiles > 65535) return MS3D_E_UNSUPPORTED;
    const dim3 grid((unsigned)blocks, (unsigned)t.ntiles);
    const size_t lds = sizeof(float) * (size_t)K * t.TC;              // <= 254 * 64 * 4 = 65,024 bytes
    MS3D_LAUNCH_VEC(v4, chconv_forward_kernel, grid, 256, lds, stream, in, w, bias, nbr, Vout, K, C, t.TC, t.LPR, out);
    return 0;
}

int ms3d_chconv_backward_weight(const float *in, const float *dout, const int *nbr, int Vout, int K, int C, float *partial_ws,
                                float *dW, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > CHCONV_MAX_K || C < 1) return MS3D_E_UNSUPPORTED;
    if ((long)K * C > 0x7fffffffL) return MS3D_E_UNSUPPORTED;
    if (Vout <= 0) return 0;                                          // (dW is not written: an empty sum is the caller's zero)
    const bool v4 = vec4(C, in, dout, partial_ws);
    const Tiling t = tiling_of(C, v4 ? 4 : 1);
    if (t.ntiles > 65535) return MS3D_E_UNSUPPORTED;
    int G = 1;                                                        // largest power of two <= 64 / LPR
    while (2 * G * t.LPR <= 64) G *= 2;
    const int parts = ms3d_chconv_wgrad_parts(Vout);
    const dim3 grid((unsigned)parts, (unsigned)t.ntiles);
    MS3D_LAUNCH_VEC(v4, chconv_wgrad_partial_kernel, grid, 256, 0, stream, in, dout, nbr, Vout, K, C, t.TC, t.LPR, G, partial_ws);
    const int n = K * C;
    chconv_wgrad_reduce_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(partial_ws, parts, n, dW);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
