// The crossing between sparse rows F [V, C] and a dense grid [B, C, X, Y, Z] (SparseTensor.dense, to_sparse), float32.
//
// A CELL is one (b, x', y', z') of the grid, numbered ((b * X + x') * Y + y') * Z + z' (< 2^31); S = X * Y * Z is the
// volume of one batch index, so a channel plane (b, c) is S contiguous floats and element (b, c, s) lies at
// (b * C + c) * S + s.  Four pieces:
//
//   cell map    coordinates -> cell_row [B * S] (the row at each cell, -1 where none) and row_cell [V] (the cell of each row,
//               -1 for a row outside the grid or off the stride lattice).  One pass over the rows; a cell named by several
//               rows keeps the LOWEST row (an integer atomicMin on the table: the result does not depend on the order in
//               which the rows arrive).  The three counts the caller turns into errors come back with one sync.
//   scatter     rows -> grid.  A gather by cell: every element of the grid is written exactly once (the row's value or 0),
//               no memset in front, no atomics.
//   gather      grid -> rows for a list of cells; one writer per element, a cell listed twice is read twice.
//   occupancy   grid -> keep [B * S] (any channel != 0: NaN counts, -0.0 does not), the scan of the flags and the kept
//               cells as coordinates, in ascending cell order (the order of torch.nonzero on the [B, X, Y, Z] mask).
//
// The two feature kernels turn a DENSE_CELLS x DENSE_CH tile (64 cells x 32 channels) in LDS: the rows are contiguous along
// the channels, the grid along the cells, and each side of the tile is read or written with the lanes along ITS contiguous
// axis (128 B per row, 256 B per channel plane and wave).  LDS layout: tile[cell][DENSE_PAD = 33] floats.  By the bank rule
// (ds_write / ds_read_b32: bank = (byte / 4) % 32, conflicts within a 32-lane half only):
//   lanes along the channels (32 lanes = one cell, channel c):  bank = (33 * cell + c) % 32 = (cell + c) % 32, c = 0..31
//   lanes along the cells (32 lanes = one channel, 32 consecutive cells):  bank = (cell + c) % 32, cell = 32 h .. 32 h + 31
// both are 32 distinct banks: conflict degree 1 for the write and the read, in both directions.  (Unpadded, stride 32, the
// cell-side access would be 32-way.)
//
// Nothing here adds floats, atomically or otherwise: the same bytes on every run.
#include <algorithm>
#include "common.h"
#include "scan.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr int DENSE_CELLS = 64;      // cells (scatter) / list entries (gather) per workgroup
constexpr int DENSE_CH = 32;         // channels per workgroup
constexpr int DENSE_PAD = 33;        // floats per cell of the LDS tile
constexpr long long DENSE_MAX_CELLS = 2147483647LL;
constexpr int DENSE_MAX_BLOCKS = 1 << 16;       // grid-stride kernels

struct DenseGrid {
    int B, X, Y, Z;
};

// true when the grid can be addressed: every size >= 0, B * X * Y * Z <= 2^31 - 1 (and, with C, B * C * X * Y * Z < 2^63 --
// implied for every C an int can hold: 2^31 * 2^31 < 2^63)
inline bool grid_ok(int B, int X, int Y, int Z, long long &ncells)
{
    ncells = 0;
    if (B < 0 || X < 0 || Y < 0 || Z < 0) return false;
    unsigned __int128 n = (unsigned __int128)(unsigned)B * (unsigned)X;
    n *= (unsigned)Y;
    n *= (unsigned)Z;
    if (n > (unsigned __int128)DENSE_MAX_CELLS) return false;
    ncells = (long long)n;
    return true;
}
inline bool channels_ok(int C, long long ncells)
{
    if (C < 0) return false;
    // the channel tiles are the y dimension of the launch
    return (long long)ms3d_divup(C, DENSE_CH) <= 65535 && (unsigned __int128)ncells * (unsigned)C < ((unsigned __int128)1 << 63);
}
inline int stride_blocks(long long n) { return (int)std::min<long long>((n + 255) / 256, DENSE_MAX_BLOCKS); }

// ------------------------------------------------------------------ cell map
__global__ __launch_bounds__(256) void dense_fill_kernel(int *__restrict__ p, long long n, int v)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) p[i] = v;
}

// counts[0] rows outside the grid, [1] rows off the stride lattice, [2] rows that were the first to claim their cell
// (rows that lost their cell = rows with a cell - distinct cells; the launcher subtracts)
__global__ __launch_bounds__(256) void dense_cell_map_kernel(const int *__restrict__ coords, int V, int ox, int oy, int oz,
                                                             int divisor, DenseGrid g, unsigned *__restrict__ cell_row,
                                                             int *__restrict__ row_cell, int *__restrict__ counts)
{
    int outside = 0, offgrid = 0, claimed = 0;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < V; r += step) {
        const int4 c = reinterpret_cast<const int4 *>(coords)[r];
        // (64-bit: a coordinate near INT_MIN minus a positive origin must not wrap into the grid)
        const long long dx = (long long)c.y - ox, dy = (long long)c.z - oy, dz = (long long)c.w - oz;
        int cell = -1;
        if (dx % divisor != 0 || dy % divisor != 0 || dz % divisor != 0) {
            offgrid++;
        } else {
            const long long x = dx / divisor, y = dy / divisor, z = dz / divisor;
            if (c.x < 0 || c.x >= g.B || x < 0 || x >= g.X || y < 0 || y >= g.Y || z < 0 || z >= g.Z) {
                outside++;
            } else {
                cell = (int)((((long long)c.x * g.X + x) * g.Y + y) * g.Z + z);
                if (atomicMin(&cell_row[cell], (unsigned)r) == 0xffffffffu) claimed++;
            }
        }
        row_cell[r] = cell;
    }
    outside = wave_sum(outside);
    offgrid = wave_sum(offgrid);
    claimed = wave_sum(claimed);
    if (lane_id() == 0) {
        if (outside) atomicAdd(&counts[0], outside);
        if (offgrid) atomicAdd(&counts[1], offgrid);
        if (claimed) atomicAdd(&counts[2], claimed);
    }
}

// ------------------------------------------------------------------ rows -> grid
// Workgroup (b, run, channel tile): cells s0 .. s0 + 63 of batch index b, channels c0 .. c0 + 31.  blockIdx.x = b * runs +
// run, blockIdx.y = the channel tile.
__global__ __launch_bounds__(256) void dense_scatter_kernel(const float *__restrict__ F, long long ld,
                                                            const int *__restrict__ cell_row,
                                                            const int *__restrict__ row_index, int n_rows, int C,
                                                            long long S, int runs, float *__restrict__ out)
{
    __shared__ float tile[DENSE_CELLS * DENSE_PAD];
    __shared__ int rows[DENSE_CELLS];
    const int t = threadIdx.x;
    const int b = blockIdx.x / runs;
    const long long s0 = (long long)(blockIdx.x % runs) * DENSE_CELLS;
    const int c0 = blockIdx.y * DENSE_CH;
    int r = -1;
    if (t < DENSE_CELLS) {
        if (s0 + t < S) {
            r = cell_row[(long long)b * S + s0 + t];
            if (r >= 0 && row_index) r = row_index[r];
            if (r >= n_rows) r = -1;                     // (a table that names a row the features do not have: never read)
        }
        rows[t] = r;
    }
    const int any = __syncthreads_or(r >= 0);            // (also orders rows[] in front of the reads below)
    // grid side: lane = cell, 4 channels per pass
    const int sc = t & (DENSE_CELLS - 1), cq = t >> 6;
    const bool cell_ok = s0 + sc < S;
    float *__restrict__ o = out + ((long long)b * C + c0) * S + s0 + sc;
    if (!any) {                                          // (uniform) an empty run: zeros straight from registers
#pragma unroll
        for (int k = 0; k < DENSE_CH / 4; k++) {
            const int c = cq + 4 * k;
            if (cell_ok && c0 + c < C) o[(long long)c * S] = 0.f;
        }
        return;
    }
    // row side: lane = channel, 8 cells per pass
    const int lc = t & (DENSE_CH - 1), lr = t >> 5;
    const bool ch_ok = c0 + lc < C;
#pragma unroll
    for (int k = 0; k < DENSE_CELLS / 8; k++) {
        const int cell = lr + 8 * k;
        const int row = rows[cell];
        float v = 0.f;
        if (row >= 0 && ch_ok) v = F[(long long)row * ld + c0 + lc];
        tile[cell * DENSE_PAD + lc] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DENSE_CH / 4; k++) {
        const int c = cq + 4 * k;
        if (cell_ok && c0 + c < C) o[(long long)c * S] = tile[sc * DENSE_PAD + c];
    }
}

// ------------------------------------------------------------------ grid -> rows
// Workgroup (run, channel tile): list entries i0 .. i0 + 63, channels c0 .. c0 + 31.  A cell outside [0, ncells) gives a
// zero row.
__global__ __launch_bounds__(256) void dense_gather_kernel(const float *__restrict__ grid, const int *__restrict__ cells,
                                                           long long n, long long ncells, int C, long long S,
                                                           float *__restrict__ out)
{
    __shared__ float tile[DENSE_CELLS * DENSE_PAD];
    const int t = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * DENSE_CELLS;
    const int c0 = blockIdx.y * DENSE_CH;
    // grid side: lane = list entry, 4 channels per pass
    const int sc = t & (DENSE_CELLS - 1), cq = t >> 6;
    long long base = -1;                                 // element (b, c0, s) of the entry's cell
    if (i0 + sc < n) {
        const long long cell = cells[i0 + sc];
        if (cell >= 0 && cell < ncells) {
            const long long b = cell / S;
            base = (b * C + c0) * S + (cell - b * S);
        }
    }
#pragma unroll
    for (int k = 0; k < DENSE_CH / 4; k++) {
        const int c = cq + 4 * k;
        float v = 0.f;
        if (base >= 0 && c0 + c < C) v = grid[base + (long long)c * S];
        tile[sc * DENSE_PAD + c] = v;
    }
    __syncthreads();
    // row side: lane = channel, 8 entries per pass
    const int lc = t & (DENSE_CH - 1), lr = t >> 5;
    if (c0 + lc >= C) return;
#pragma unroll
    for (int k = 0; k < DENSE_CELLS / 8; k++) {
        const int e = lr + 8 * k;
        if (i0 + e < n) out[(i0 + e) * C + c0 + lc] = tile[e * DENSE_PAD + lc];
    }
}

// ------------------------------------------------------------------ occupancy
// thread = cell (consecutive lanes read consecutive floats of a channel plane); all != 0: every cell is kept, grid is not read
__global__ __launch_bounds__(256) void dense_occupancy_kernel(const float *__restrict__ grid, int all, long long ncells, int C,
                                                              long long S, unsigned char *__restrict__ keep,
                                                              int *__restrict__ flag)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x; cell < ncells; cell += step) {
        int any = all;
        if (!all) {
            const long long b = cell / S;
            const float *__restrict__ p = grid + b * C * S + (cell - b * S);
            for (int c = 0; c < C && !any; c += 4) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = c + k < C ? p[(long long)(c + k) * S] : 0.f;
                // (v != 0 is true for NaN and false for -0.0)
                any = (v[0] != 0.f) | (v[1] != 0.f) | (v[2] != 0.f) | (v[3] != 0.f);
            }
        }
        keep[cell] = (unsigned char)any;
        flag[cell] = any;
    }
}

// kept cell -> (b, x, y, z) and its cell number at position rank[cell]
__global__ __launch_bounds__(256) void dense_emit_kernel(const unsigned char *__restrict__ keep, const int *__restrict__ rank,
                                                         long long ncells, DenseGrid g, int *__restrict__ out_coords,
                                                         int *__restrict__ out_cells)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x; cell < ncells; cell += step) {
        if (!keep[cell]) continue;
        const int r = rank[cell];
        long long q = cell;
        const int z = (int)(q % g.Z); q /= g.Z;
        const int y = (int)(q % g.Y); q /= g.Y;
        const int x = (int)(q % g.X); q /= g.X;
        reinterpret_cast<int4 *>(out_coords)[r] = make_int4((int)q, x, y, z);
        out_cells[r] = (int)cell;
    }
}

}  // namespace

extern "C" {

int ms3d_dense_tile_cells(void) { return DENSE_CELLS; }
int ms3d_dense_tile_channels(void) { return DENSE_CH; }

int ms3d_dense_cell_map(const int *coords, int V, const int *origin, int divisor, int B, int X, int Y, int Z, int *cell_row,
                        int *row_cell, int *counts_dev, int *counts, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long ncells;
    if (!grid_ok(B, X, Y, Z, ncells) || divisor < 1 || V < 0) return MS3D_E_UNSUPPORTED;
    counts[0] = counts[1] = counts[2] = 0;
    if (ncells > 0) {
        dense_fill_kernel<<<stride_blocks(ncells), 256, 0, stream>>>(cell_row, ncells, -1);
        MS3D_LAUNCH_CHECK();
    }
    if (V == 0) return 0;
    MS3D_CHECK(hipMemsetAsync(counts_dev, 0, sizeof(int) * 4, stream));
    const DenseGrid g = {B, X, Y, Z};
    dense_cell_map_kernel<<<stride_blocks(V), 256, 0, stream>>>(coords, V, origin[0], origin[1], origin[2], divisor, g,
                                                               reinterpret_cast<unsigned *>(cell_row), row_cell, counts_dev);
    MS3D_LAUNCH_CHECK();
    int h[4];
    MS3D_CHECK(hipMemcpyAsync(h, counts_dev, sizeof(int) * 4, hipMemcpyDeviceToHost, stream));
    MS3D_CHECK(hipStreamSynchronize(stream));
    counts[0] = h[0];
    counts[1] = h[1];
    counts[2] = V - h[0] - h[1] - h[2];
    return 0;
}

int ms3d_dense_scatter(const float *F, long n_rows, long ld, const int *cell_row, const int *row_index, int B, int C, int X,
                       int Y, int Z, float *out, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long ncells;
    if (!grid_ok(B, X, Y, Z, ncells) || !channels_ok(C, ncells) || n_rows < 0 || n_rows > 2147483647L || ld < C)
        return MS3D_E_UNSUPPORTED;
    if (ncells == 0 || C == 0) return 0;
    const long long S = (long long)X * Y * Z;
    const int runs = ms3d_divup(S, DENSE_CELLS);
    const dim3 grid((unsigned)((long long)B * runs), (unsigned)ms3d_divup(C, DENSE_CH));     // B * runs <= ncells < 2^31
    dense_scatter_kernel<<<grid, 256, 0, stream>>>(F, ld, cell_row, row_index, (int)n_rows, C, S, runs, out);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_dense_gather(const float *grid_, int B, int C, int X, int Y, int Z, const int *cells, long n, float *out,
                      ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long ncells;
    if (!grid_ok(B, X, Y, Z, ncells) || !channels_ok(C, ncells) || n < 0 || n > 2147483647L * DENSE_CELLS)
        return MS3D_E_UNSUPPORTED;
    if (n == 0 || C == 0) return 0;
    const long long S = std::max<long long>((long long)X * Y * Z, 1);
    const dim3 grid((unsigned)ms3d_divup(n, DENSE_CELLS), (unsigned)ms3d_divup(C, DENSE_CH));
    dense_gather_kernel<<<grid, 256, 0, stream>>>(grid_, cells, n, ncells, C, S, out);
    MS3D_LAUNCH_CHECK();
    return 0;
}

size_t ms3d_dense_occupancy_workspace_bytes(void) { return ms3d_align(sizeof(int) * 4) + ms3d_scan_workspace_bytes(); }

int ms3d_dense_occupancy(const float *grid_, int B, int C, int X, int Y, int Z, unsigned char *keep, int *rank, int *n_kept,
                         void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long ncells;
    if (!grid_ok(B, X, Y, Z, ncells) || !channels_ok(C, ncells)) return MS3D_E_UNSUPPORTED;
    *n_kept = 0;
    if (ncells == 0) return 0;
    if (workspace_bytes < ms3d_dense_occupancy_workspace_bytes()) return MS3D_E_WORKSPACE;
    int *total = (int *)workspace;
    void *scan_ws = (char *)workspace + ms3d_align(sizeof(int) * 4);
    const long long S = (long long)X * Y * Z;
    dense_occupancy_kernel<<<stride_blocks(ncells), 256, 0, stream>>>(grid_, grid_ == nullptr, ncells, C, S, keep, rank);
    MS3D_LAUNCH_CHECK();
    int rc = ms3d_exclusive_scan_i32(rank, rank, (int)ncells, total, scan_ws, stream);
    if (rc) return rc;
    MS3D_CHECK(hipMemcpyAsync(n_kept, total, sizeof(int), hipMemcpyDeviceToHost, stream));
    MS3D_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int ms3d_dense_cells_emit(const unsigned char *keep, const int *rank, int B, int X, int Y, int Z, int *out_coords,
                          int *out_cells, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    long long ncells;
    if (!grid_ok(B, X, Y, Z, ncells)) return MS3D_E_UNSUPPORTED;
    if (ncells == 0) return 0;
    const DenseGrid g = {B, X, Y, Z};
    dense_emit_kernel<<<stride_blocks(ncells), 256, 0, stream>>>(keep, rank, ncells, g, out_coords, out_cells);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
