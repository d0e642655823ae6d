// Coordinate engine for the sparse-voxel backbone (the part of MinkowskiEngine's coordinate manager the
// reference relies on: call sites model/module/backbone.py:38, common.py:69,77, general_model.py:187-191,
// data/dataset/general_dataset.py:159-163).
//
//   * 64-bit key (batch:19 | x:15 | y:15 | z:15, biased) in an open-addressing table in HBM
//   * sparse_quantize / stride-2 downsample: value = atomicMin(row) so the FIRST row of every
//     coordinate is its representative and unique rows come out in first-occurrence order
//     (flag -> exclusive scan -> rank); deterministic, no sort
//   * kernel maps as OUTPUT-STATIONARY neighbour tables, stored offset-major  nbr[k][V_out]  so that the
//     16 output rows a wave owns read 64 contiguous bytes per offset:
//       k3 s1 : nbr[k][i] = row at c_i + o_k*ts            (k = ix + 3*iy + 9*iz, x fastest)
//       k2 s2 : down[k][p] = child of coarse row p at offset k;  up[k][f] = (k == koff[f]) ? parent[f] : -1
//       general: nbr[k][o] = row at c_o + offsets[k] for any offset list (any kernel size, stride, dilation), and the
//               inverse table nbr_inv[k][i] = o of a map that is not its own mirror image
//       region: a set onto itself over any offset list (a cross, a hand-written list), table and inverse from one pass:
//               one lookup per pair of opposite offsets, four stores (kmap_region_kernel)
#include <algorithm>
#include <mutex>
#include <unordered_map>
#include "common.h"
#include "scan.h"
#include "../../include/minsu3d_hip.h"

namespace {

constexpr unsigned long long EMPTY_KEY = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}
__device__ __forceinline__ bool in_range(int v) { return v >= -16384 && v < 16384; }
__device__ __forceinline__ unsigned long long pack_key(int b, int x, int y, int z)
{
    return ((unsigned long long)(unsigned)(b & 0x7FFFF) << 45) | ((unsigned long long)(unsigned)((x + 16384) & 0x7FFF) << 30) |
           ((unsigned long long)(unsigned)((y + 16384) & 0x7FFF) << 15) | (unsigned long long)(unsigned)((z + 16384) & 0x7FFF);
}
__device__ __forceinline__ int floor_div(int v, int d) { return (v >= 0) ? (v / d) : -((-v + d - 1) / d); }

__global__ void table_clear_kernel(unsigned long long *keys, int *vals, int H, int *range_flag)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < H) {
        keys[t] = EMPTY_KEY;
        vals[t] = 0x7fffffff;
    }
    if (t == 0) *range_flag = 0;
}

// insert (optionally the stride-`q` floored coordinate) with value = min row; slot_of_row remembers the slot
// A coordinate outside [-16384, 16384) or a batch / cluster id outside [0, 524288) does not fit the key and would alias
// another voxel: range_flag is raised and the entry points that read a count back return MS3D_E_UNSUPPORTED.
__global__ void table_insert_kernel(const int *__restrict__ coords, int n, int q, unsigned long long *keys, int *vals,
                                    unsigned mask, int *__restrict__ slot_of_row, int *range_flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    int x = c.y, y = c.z, z = c.w;
    if (!(in_range(x) && in_range(y) && in_range(z) && c.x >= 0 && c.x <= 0x7FFFF) && *range_flag == 0) atomicOr(range_flag, 1);
    if (q > 1) {
        x = floor_div(x, q) * q;
        y = floor_div(y, q) * q;
        z = floor_div(z, q) * q;
    }
    const unsigned long long key = pack_key(c.x, x, y, z);
    unsigned slot = (unsigned)mix64(key) & mask;
    for (;;) {
        const unsigned long long prev = atomicCAS(&keys[slot], EMPTY_KEY, key);
        if (prev == EMPTY_KEY || prev == key) break;
        slot = (slot + 1) & mask;
    }
    atomicMin(&vals[slot], i);
    if (slot_of_row) slot_of_row[i] = (int)slot;
}

__global__ void first_flag_kernel(int n, const int *__restrict__ slot_of_row, const int *__restrict__ vals,
                                  int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (vals[slot_of_row[i]] == i) ? 1 : 0;
}

// unique_idx[rank[i]] = i for representatives; inverse[i] = rank[representative(i)]
__global__ void unique_emit_kernel(int n, const int *__restrict__ slot_of_row, const int *__restrict__ vals,
                                   const int *__restrict__ rank, int *__restrict__ unique_idx,
                                   int *__restrict__ inverse)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int rep = vals[slot_of_row[i]];
    if (rep == i && unique_idx) unique_idx[rank[i]] = i;
    inverse[i] = rank[rep];
}

// coarse coords + in-cell offset index for the stride-2 map
__global__ void downsample_emit_kernel(int n, int ts, const int *__restrict__ coords, const int *__restrict__ slot_of_row,
                                       const int *__restrict__ vals, const int *__restrict__ rank,
                                       int *__restrict__ out_coords, int *__restrict__ parent, int *__restrict__ koff)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    const int t2 = ts * 2;
    const int qx = floor_div(c.y, t2) * t2, qy = floor_div(c.z, t2) * t2, qz = floor_div(c.w, t2) * t2;
    const int rep = vals[slot_of_row[i]];
    const int p = rank[rep];
    parent[i] = p;
    koff[i] = (c.y - qx) / ts + 2 * ((c.z - qy) / ts) + 4 * ((c.w - qz) / ts);
    if (rep == i) reinterpret_cast<int4 *>(out_coords)[p] = make_int4(c.x, qx, qy, qz);
}

__device__ __forceinline__ int table_lookup(const unsigned long long *__restrict__ keys, const int *__restrict__ vals,
                                            unsigned mask, unsigned long long key)
{
    unsigned slot = (unsigned)mix64(key) & mask;
    for (;;) {
        const unsigned long long k = keys[slot];
        if (k == key) return vals[slot];
        if (k == EMPTY_KEY) return -1;
        slot = (slot + 1) & mask;
    }
}

// validation of a caller-supplied coordinate set (ms3d_coords_check), behind table_clear / table_insert (which raise bit 0 for
// a row that does not fit the key): one thread per row; bit 1 = a coordinate is not a multiple of `lattice` (the floor_div
// arithmetic of the strided sets: floor(v / q) * q == v), bit 2 = the row is not the first holder of its key's slot (the
// coordinate occurs twice).  A row that does not fit the key aliases another coordinate, so it is not asked about repeats.
// One device int collects the bits; a thread ORs only the bits it does not see up yet (a handful of atomics per call).
__global__ __launch_bounds__(256) void coords_check_kernel(const int *__restrict__ coords, int n, int lattice,
                                                           const int *__restrict__ slot_of_row, const int *__restrict__ vals,
                                                           int *flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    int bits = 0;
    if (floor_div(c.y, lattice) * lattice != c.y || floor_div(c.z, lattice) * lattice != c.z ||
        floor_div(c.w, lattice) * lattice != c.w)
        bits |= MS3D_COORDS_OFF_LATTICE;
    const bool fits = in_range(c.y) && in_range(c.z) && in_range(c.w) && c.x >= 0 && c.x <= 0x7FFFF;
    if (fits && vals[slot_of_row[i]] != i) bits |= MS3D_COORDS_REPEATED;
    if (bits && (*flags & bits) != bits) atomicOr(flags, bits);
}

// one thread per (offset, row): writes nbr[k][i]; consecutive threads -> consecutive rows (coalesced stores)
__global__ void kmap_k3_kernel(const int *__restrict__ coords, int V, int ts, const unsigned long long *__restrict__ keys,
                               const int *__restrict__ vals, unsigned mask, int *__restrict__ nbr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= V) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    const int x = c.y + (k % 3 - 1) * ts, y = c.z + ((k / 3) % 3 - 1) * ts, z = c.w + (k / 9 - 1) * ts;
    int r = -1;
    if (k == 13)
        r = i;
    else if (in_range(x) && in_range(y) && in_range(z))
        r = table_lookup(keys, vals, mask, pack_key(c.x, x, y, z));
    nbr[(size_t)k * V + i] = r;
}

// The same table from HALF the lookups (round 6): j = nbr[k][i] <=> i = nbr[26 - k][j], so offsets 0..12 are looked up and
// every hit also writes its mirror entry (each (26 - k, j) has at most one such writer; the rest of offsets 14..26 was
// pre-filled with -1).  A full-resolution level is 27 x 427k probes of which 80 % miss and walk to an empty slot: the
// lookups, not the stores, are what the kernel costs (it runs on the input pipeline's stream inside the grouping window).
__global__ void kmap_k3_sym_kernel(const int *__restrict__ coords, int V, int ts, const unsigned long long *__restrict__ keys,
                                   const int *__restrict__ vals, unsigned mask, int *__restrict__ nbr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;          // 0..13
    if (i >= V) return;
    if (k == 13) { nbr[(size_t)13 * V + i] = i; return; }
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    const int x = c.y + (k % 3 - 1) * ts, y = c.z + ((k / 3) % 3 - 1) * ts, z = c.w + (k / 9 - 1) * ts;
    int r = -1;
    if (in_range(x) && in_range(y) && in_range(z)) r = table_lookup(keys, vals, mask, pack_key(c.x, x, y, z));
    nbr[(size_t)k * V + i] = r;
    if (r >= 0) nbr[(size_t)(26 - k) * V + r] = i;
}

__global__ void fill_minus1_kernel(int *p, long n)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = -1;
}
// General kernel map: one thread per (offset, output row), nbr[k][o] = input row at (batch of o, xyz of o + offsets[k]) or
// -1; consecutive threads -> consecutive rows of one offset (coalesced stores, as kmap_k3_kernel).  A shifted coordinate
// that leaves the packable range has no key of its own (pack_key would wrap it onto another voxel): -1 without a probe.
__global__ void kmap_general_kernel(const int *__restrict__ out_coords, int Vout, const int *__restrict__ offsets, int K,
                                    const unsigned long long *__restrict__ keys, const int *__restrict__ vals, unsigned mask,
                                    int *__restrict__ nbr)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (o >= Vout || k >= K) return;
    const int4 c = reinterpret_cast<const int4 *>(out_coords)[o];
    int r = -1;
    if (in_range(c.y) && in_range(c.z) && in_range(c.w) && c.x >= 0 && c.x <= 0x7FFFF) {
        const int x = c.y + offsets[3 * k], y = c.z + offsets[3 * k + 1], z = c.w + offsets[3 * k + 2];
        if (in_range(x) && in_range(y) && in_range(z)) r = table_lookup(keys, vals, mask, pack_key(c.x, x, y, z));
    }
    nbr[(size_t)k * Vout + o] = r;
}

// Trilinear interpolation map: one thread per (corner, point), tables corner-major like every kernel map.  Per axis q = p / ts
// (an exact scaling: ts is a power of two), f = floor(q), r = q - f; corner j = bx + 2 by + 4 bz sits at (f + b) * ts and has
// weight ((wx * wy) * wz), w = b ? r : 1 - r, every step rounded to float32 on its own.  rows[j][n] = the row of the set at the
// corner (batch index = the integer part of the point's first column) or -1: no such voxel, a corner or batch index outside
// the packable range (no probe: pack_key would wrap it onto another voxel), or a point with a non-finite entry -- whose
// weights are 0 as well.
__device__ __forceinline__ bool in_range_f(float v) { return v >= -16384.f && v < 16384.f; }
__global__ __launch_bounds__(256) void interp_map_kernel(const float *__restrict__ points, int N, float ts,
                                                         const unsigned long long *__restrict__ keys,
                                                         const int *__restrict__ vals, unsigned mask, int *__restrict__ rows,
                                                         float *__restrict__ weights)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (n >= N || j >= 8) return;
    const float4 p = reinterpret_cast<const float4 *>(points)[n];
    int r = -1;
    float w = 0.f;
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w)) {
        const float qx = __fdiv_rn(p.y, ts), qy = __fdiv_rn(p.z, ts), qz = __fdiv_rn(p.w, ts);
        const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
        const float rx = __fsub_rn(qx, fx), ry = __fsub_rn(qy, fy), rz = __fsub_rn(qz, fz);
        const int bx = j & 1, by = (j >> 1) & 1, bz = j >> 2;
        const float wx = bx ? rx : __fsub_rn(1.f, rx), wy = by ? ry : __fsub_rn(1.f, ry), wz = bz ? rz : __fsub_rn(1.f, rz);
        w = __fmul_rn(__fmul_rn(wx, wy), wz);
        // (exact in float wherever the corner is in range; beyond 2^24 it is out of range whatever the rounding does)
        const float cx = __fmul_rn(fx + (float)bx, ts), cy = __fmul_rn(fy + (float)by, ts), cz = __fmul_rn(fz + (float)bz, ts);
        if (in_range_f(cx) && in_range_f(cy) && in_range_f(cz) && p.x >= 0.f && p.x < 524288.f)
            r = table_lookup(keys, vals, mask, pack_key((int)p.x, (int)cx, (int)cy, (int)cz));
    }
    rows[(size_t)j * N + n] = r;
    weights[(size_t)j * N + n] = w;
}

// nbr_inv[k][nbr[k][o]] = o: for one offset an input row feeds at most one output row (distinct output coordinates), so
// the stores of one launch never meet; entries that name no row of [0, Vin) are skipped
__global__ void kmap_invert_kernel(const int *__restrict__ nbr, int Vout, int Vin, int *__restrict__ nbr_inv)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (o >= Vout) return;
    const int i = nbr[(size_t)k * Vout + o];
    if (i >= 0 && i < Vin) nbr_inv[(size_t)k * Vin + i] = o;
}
// Region map (ms3d_kmap_region): a coordinate set onto ITSELF over any offset list, forward table and inverse from one pass.
// partner.p[k] = index of -offsets[k] in the list (k itself for the zero offset, REGION_NO_PARTNER when the list lacks it),
// handed over by value.  One thread per (offset, row); both tables were pre-filled with -1 and only hits are stored.
//   j = nbr_fwd[k][i] over distinct rows  <=>  nbr_fwd[p][j] = i, nbr_inv[k][j] = i, nbr_inv[p][i] = j   (p = partner of k)
// so of a partnered pair only the lower index k is looked up and the thread stores all four entries; the blocks of the higher
// index leave at once.  An offset without a partner (or its own partner) is one lookup plus the scatter into nbr_inv.
// Rows that repeat: the table names the FIRST row of a coordinate, so only a row the table names for its own key writes
// mirrored entries and entries of nbr_inv -- each such entry then has exactly one writer (the first row at the other end
// of the offset) -- and any other row looks both offsets of the pair up itself and writes its own column of nbr_fwd alone,
// which nobody mirrors into.  nbr_fwd is therefore kmap_general_kernel's table for any input.  A set with a row outside the
// packable range (range_flag, raised by table_insert_kernel: such a row aliases another key) is walked without mirroring at
// all: every (offset, row) does its own lookup.
constexpr int REGION_NO_PARTNER = 255;
struct RegionPartner {
    unsigned char p[256];
};
__device__ __forceinline__ int region_lookup(const int4 c, const int *__restrict__ offsets, int k,
                                             const unsigned long long *__restrict__ keys, const int *__restrict__ vals,
                                             unsigned mask)
{
    const int x = c.y + offsets[3 * k], y = c.z + offsets[3 * k + 1], z = c.w + offsets[3 * k + 2];
    if (!(in_range(x) && in_range(y) && in_range(z))) return -1;
    return table_lookup(keys, vals, mask, pack_key(c.x, x, y, z));
}
__global__ __launch_bounds__(256) void kmap_region_kernel(const int *__restrict__ coords, int V, const int *__restrict__ offsets,
                                                          int K, const RegionPartner partner,
                                                          const unsigned long long *__restrict__ keys,
                                                          const int *__restrict__ vals, unsigned mask,
                                                          const int *__restrict__ slot_of_row,
                                                          const int *__restrict__ range_flag, int *__restrict__ nbr_fwd,
                                                          int *__restrict__ nbr_inv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= V || k >= K) return;
    const int p = partner.p[k];
    const bool pair = *range_flag == 0 && p != REGION_NO_PARTNER && p != k;
    if (pair && p < k) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    if (!(in_range(c.y) && in_range(c.z) && in_range(c.w) && c.x >= 0 && c.x <= 0x7FFFF)) return;
    const int own = vals[slot_of_row[i]];          // the row the table names for this row's key: no probe
    const bool first = own == i;
    const bool zero = (offsets[3 * k] | offsets[3 * k + 1] | offsets[3 * k + 2]) == 0;
    const int r = zero ? own : region_lookup(c, offsets, k, keys, vals, mask);
    if (r >= 0) {
        nbr_fwd[(size_t)k * V + i] = r;
        if (first) nbr_inv[(size_t)k * V + r] = i;
    }
    if (!pair) return;
    if (first) {
        if (r >= 0) {
            nbr_fwd[(size_t)p * V + r] = i;
            nbr_inv[(size_t)p * V + i] = r;
        }
    } else {
        const int r2 = region_lookup(c, offsets, p, keys, vals, mask);
        if (r2 >= 0) nbr_fwd[(size_t)p * V + i] = r2;
    }
}
__global__ void kmap_k2_kernel(const int *__restrict__ parent, const int *__restrict__ koff, int Vf, int Vc,
                               int *__restrict__ nbr_down, int *__restrict__ nbr_up)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= Vf) return;
    const int p = parent[f], k = koff[f];
    nbr_down[(size_t)k * Vc + p] = f;
    nbr_up[(size_t)k * Vf + f] = p;
}

// ------------------------------------------------------------------ coordinate generation / pruning
// Candidate c = i * K + k of ms3d_coords_expand is (batch of input row i, xyz of row i + offsets[k]); it is computed where it
// is needed, never stored.  The launches below are grid-stride over the candidates with a bounded grid (EXPAND_MAX_BLOCKS
// workgroups); every index that can pass 2^31 is 64 bits wide, slots are unsigned (a table of up to 2^32 slots).
constexpr int EXPAND_MAX_BLOCKS = 8192;

__device__ __forceinline__ int4 expand_candidate(const int *__restrict__ coords, const int *__restrict__ offsets, int K,
                                                 long long c, bool *ok)
{
    const long long i = c / K;
    const int k = (int)(c - i * K);
    const int4 p = reinterpret_cast<const int4 *>(coords)[i];
    // the sums in 64 bits: an input row or an offset that is garbage must raise the flag, not overflow an int (and the input
    // row itself is checked too: a sum of two out-of-range values could land back inside the range)
    const long long x = (long long)p.y + offsets[3 * k], y = (long long)p.z + offsets[3 * k + 1],
                    z = (long long)p.w + offsets[3 * k + 2];
    *ok = in_range(p.y) && in_range(p.z) && in_range(p.w) && p.x >= 0 && p.x <= 0x7FFFF && x >= -16384 && x < 16384 &&
          y >= -16384 && y < 16384 && z >= -16384 && z < 16384;
    const int4 q = make_int4(p.x, (int)x, (int)y, (int)z);
    return q;
}

__global__ __launch_bounds__(256) void expand_clear_kernel(unsigned long long *keys, int *vals, size_t H, int *range_flag)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += step) {
        keys[t] = EMPTY_KEY;
        vals[t] = 0x7fffffff;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *range_flag = 0;
}

// the insert of table_insert_kernel (64-bit CAS on the key, atomicMin of the candidate index on the value) per candidate.  A
// candidate that does not fit the key raises range_flag and is left out of the table (slot = none): the entry point then
// returns MS3D_E_UNSUPPORTED, nothing is aliased onto another voxel.
__global__ __launch_bounds__(256) void expand_insert_kernel(const int *__restrict__ coords, const int *__restrict__ offsets,
                                                            int K, long long N, unsigned long long *keys, int *vals,
                                                            unsigned mask, unsigned *__restrict__ slot_of_cand,
                                                            int *range_flag)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += step) {
        bool ok;
        const int4 q = expand_candidate(coords, offsets, K, c, &ok);
        if (!ok) {
            if (*range_flag == 0) atomicOr(range_flag, 1);
            slot_of_cand[c] = 0xFFFFFFFFu;
            continue;
        }
        const unsigned long long key = pack_key(q.x, q.y, q.z, q.w);
        unsigned slot = (unsigned)mix64(key) & mask;
        for (;;) {
            const unsigned long long prev = atomicCAS(&keys[slot], EMPTY_KEY, key);
            if (prev == EMPTY_KEY || prev == key) break;
            slot = (slot + 1) & mask;
        }
        atomicMin(&vals[slot], (int)c);
        slot_of_cand[c] = slot;
    }
}

// has_range: the table of up to 2^32 slots needs every slot number, so "no slot" is told by the flag of the whole call: the
// flag kernel only runs its lookups when no candidate was out of range (otherwise every flag is 0 and nothing is emitted)
__global__ __launch_bounds__(256) void expand_flag_kernel(long long N, const unsigned *__restrict__ slot_of_cand,
                                                          const int *__restrict__ vals, const int *__restrict__ range_flag,
                                                          int *__restrict__ flag)
{
    const bool bad = *range_flag != 0;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += step)
        flag[c] = (!bad && vals[slot_of_cand[c]] == (int)c) ? 1 : 0;
}

__global__ __launch_bounds__(256) void expand_emit_kernel(const int *__restrict__ coords, const int *__restrict__ offsets,
                                                          int K, long long N, const unsigned *__restrict__ slot_of_cand,
                                                          const int *__restrict__ vals, const int *__restrict__ rank,
                                                          int *__restrict__ out_coords)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += step) {
        if (vals[slot_of_cand[c]] != (int)c) continue;
        bool ok;
        const int4 q = expand_candidate(coords, offsets, K, c, &ok);
        reinterpret_cast<int4 *>(out_coords)[rank[c]] = q;     // rank[c] < number of distinct candidates <= capacity
    }
}

struct ExpandWs {
    unsigned long long *keys;
    int *vals, *rank, *total;
    unsigned *slot_of_cand;
    void *scan_ws;
    size_t H;
};
size_t carve_expand(ExpandWs &w, long long N, void *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void *r = base ? (void *)((char *)base + off) : nullptr;
        off += ms3d_align(bytes);
        return r;
    };
    w.H = 1024;
    while (w.H < 2 * (size_t)N) w.H <<= 1;                      // load factor <= 1/2, as table_size(); at most 2^32 slots
    w.keys = (unsigned long long *)take(sizeof(unsigned long long) * w.H);
    w.vals = (int *)take(sizeof(int) * w.H);
    w.slot_of_cand = (unsigned *)take(sizeof(unsigned) * (size_t)N);
    w.rank = (int *)take(sizeof(int) * (size_t)N);             // first-occurrence flags, scanned in place
    w.total = (int *)take(sizeof(int) * 2);
    w.scan_ws = take(ms3d_scan_workspace_bytes());
    return off;
}
inline int expand_grid(long long n) { return (int)std::min<long long>((n + 255) / 256, EXPAND_MAX_BLOCKS); }

__global__ __launch_bounds__(256) void prune_flag_kernel(int V, const unsigned char *__restrict__ keep, int *__restrict__ flag)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += step) flag[i] = keep[i] ? 1 : 0;
}
// kept rows keep their relative order: kept row rank[i] <- source row i
__global__ __launch_bounds__(256) void prune_emit_kernel(int V, const int *__restrict__ coords,
                                                         const unsigned char *__restrict__ keep, const int *__restrict__ rank,
                                                         int *__restrict__ out_coords, int *__restrict__ src_row,
                                                         int *__restrict__ dst_row)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += step) {
        const bool k = keep[i] != 0;
        const int r = rank[i];
        if (k) {
            reinterpret_cast<int4 *>(out_coords)[r] = reinterpret_cast<const int4 *>(coords)[i];
            src_row[r] = (int)i;
        }
        dst_row[i] = k ? r : -1;
    }
}

// ------------------------------------------------------------------ union of coordinate sets
// The sets lie back to back in one array; set_start (by value, N <= 16) names their first rows.  Row r of the concatenation
// belongs to the last set whose start is <= r (empty sets share a start with their successor and own nothing).
constexpr int UNION_MAX_SETS = 16;
struct UnionSets {
    int n;
    int start[UNION_MAX_SETS + 1];
};
__device__ __forceinline__ int union_set_of(const UnionSets &s, int r)
{
    int i = 0;
#pragma unroll
    for (int j = 1; j < UNION_MAX_SETS; j++) i += (j < s.n && s.start[j] <= r) ? 1 : 0;
    return i;
}
// first-occurrence flag per row.  Every slot keeps one bit per set (N <= 16): the row that finds its set's bit already raised
// repeats a coordinate of its own set -- whichever set won the slot.
__global__ __launch_bounds__(256) void union_flag_kernel(int n, UnionSets sets, const int *__restrict__ slot_of_row,
                                                         const int *__restrict__ vals, int *__restrict__ seen,
                                                         int *__restrict__ flag, int *__restrict__ dup_flag)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int slot = slot_of_row[r];
    flag[r] = (vals[slot] == r) ? 1 : 0;
    const int bit = 1 << union_set_of(sets, r);
    if ((atomicOr(&seen[slot], bit) & bit) && *dup_flag == 0) atomicOr(dup_flag, 1);
}
// out_row[r] = union row of input row r; in_row[i][u] = row of set i at union row u (plain stores: rows are distinct inside
// a set, so (i, u) has one writer); the first occurrence also writes the coordinate
__global__ __launch_bounds__(256) void union_emit_kernel(int n, int n_out, UnionSets sets, const int *__restrict__ coords,
                                                         const int *__restrict__ slot_of_row, const int *__restrict__ vals,
                                                         const int *__restrict__ rank, int *__restrict__ out_coords,
                                                         int *__restrict__ out_row, int *__restrict__ in_row)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int rep = vals[slot_of_row[r]];
    const int u = rank[rep];                                   // < n_out: rank counts the first occurrences in front of rep
    const int i = union_set_of(sets, r);
    out_row[r] = u;
    in_row[(size_t)i * n_out + u] = r - sets.start[i];
    if (rep == r) reinterpret_cast<int4 *>(out_coords)[u] = reinterpret_cast<const int4 *>(coords)[r];
}

// 64-bit spatial sort key: batch index, then the 45-bit Morton code of the biased (x,y,z)
__device__ __forceinline__ unsigned long long spread3(unsigned v)
{
    unsigned long long x = v & 0x7FFFull;  // 15 bits -> every third bit
    x = (x | (x << 32)) & 0x1F00000000FFFFull;
    x = (x | (x << 16)) & 0x1F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
__global__ void morton_keys_kernel(const int *__restrict__ coords, int V, long long *__restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];
    const unsigned long long m = spread3((unsigned)(c.y + 16384)) | (spread3((unsigned)(c.z + 16384)) << 1) |
                                 (spread3((unsigned)(c.w + 16384)) << 2);
    keys[i] = (long long)(((unsigned long long)(unsigned)(c.x & 0x3FFFF) << 45) | m);
}

struct CoordWs {
    unsigned long long *keys;
    int *vals, *slot_of_row, *flag, *rank, *total;
    void *scan_ws;
    int H;
};
int table_size(int n)
{
    int H = 1024;
    while (H < 2 * n) H <<= 1;
    return H;
}
size_t carve(CoordWs &w, int n, void *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void *r = base ? (void *)((char *)base + off) : nullptr;
        off += ms3d_align(bytes);
        return r;
    };
    w.H = table_size(n);
    w.keys = (unsigned long long *)take(sizeof(unsigned long long) * w.H);
    w.vals = (int *)take(sizeof(int) * w.H);
    w.slot_of_row = (int *)take(sizeof(int) * n);
    w.flag = (int *)take(sizeof(int) * n);
    w.rank = (int *)take(sizeof(int) * n);
    w.total = (int *)take(sizeof(int) * 2);
    w.scan_ws = take(ms3d_scan_workspace_bytes());
    return off;
}

int build_table(CoordWs &w, const int *coords, int n, int q, hipStream_t stream)
{
    table_clear_kernel<<<ms3d_divup(w.H, 256), 256, 0, stream>>>(w.keys, w.vals, w.H, w.total + 1);
    MS3D_LAUNCH_CHECK();
    table_insert_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(coords, n, q, w.keys, w.vals, (unsigned)w.H - 1u,
                                                              w.slot_of_row, w.total + 1);
    MS3D_LAUNCH_CHECK();
    return 0;
}
int rank_first(CoordWs &w, int n, int *count_host, hipStream_t stream)
{
    first_flag_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(n, w.slot_of_row, w.vals, w.flag);
    MS3D_LAUNCH_CHECK();
    int rc = ms3d_exclusive_scan_i32(w.flag, w.rank, n, w.total, w.scan_ws, stream);
    if (rc) return rc;
    if (count_host) {
        int h[2] = {0, 0};   // [0] number of distinct coordinates  [1] a coordinate did not fit the key (table_insert_kernel)
        MS3D_CHECK(hipMemcpyAsync(h, w.total, sizeof(int) * 2, hipMemcpyDeviceToHost, stream));
        MS3D_CHECK(hipStreamSynchronize(stream));
        *count_host = h[0];
        if (h[1]) return MS3D_E_UNSUPPORTED;
    }
    return 0;
}


constexpr int UNION_MAX_ROWS = 0x3fffffff;      // the table of >= 2 n slots is indexed by ints
size_t carve_union(CoordWs &w, int **seen, int **dup_flag, int n, void *base)
{
    size_t off = carve(w, n, base);
    *seen = base ? (int *)((char *)base + off) : nullptr;      // one int per slot: the sets that hold the slot's coordinate
    off += ms3d_align(sizeof(int) * (size_t)w.H);
    *dup_flag = base ? (int *)((char *)base + off) : nullptr;
    return off + ms3d_align(sizeof(int));
}

// ------------------------------------------------------------------ pair lists (tile-compacted kernel maps)
// One wave per tile of MS3D_PL_ROWS output rows.  Per offset the valid (input row, output row) pairs of the tile are
// compacted with a ballot and padded to a multiple of 16 (a "batch": one MFMA group in the convolution kernels).
// entry = (input row, (k << 8) | local output row); pad entries read input row 0 and carry local row MS3D_PL_ROWS.
// RPT = rows per tile: 64 (one row per lane) or 128 (lane l owns rows l and 64 + l; the pairs of the lower half come
// first inside an (offset) group, both halves in ascending row)
template <int KT, int RPT>
__global__ __launch_bounds__(256) void pairlist_count_kernel(const int *__restrict__ nbr, int K, int Vout, int tiles,
                                                             int *__restrict__ tile_nb)
{
    constexpr int H = RPT >= 64 ? RPT / 64 : 1, LIVE = RPT >= 64 ? 64 : RPT;   // RPT = 32: the upper half of the wave idles
    const int tile = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (tile > tiles) return;
    if (tile == tiles) {  // slot for the grand total of the exclusive scan
        if (lane_id() == 0) tile_nb[tiles] = 0;
        return;
    }
    int nb = 0;
    int cnt[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) cnt[k] = 0;
#pragma unroll
    for (int h = 0; h < H; h++) {
        const int row = tile * RPT + 64 * h + lane_id();
        const bool ok = row < Vout && lane_id() < LIVE;
#pragma unroll
        for (int k = 0; k < KT; k++) {
            const int v = (ok && k < K) ? nbr[(size_t)min(k, K - 1) * Vout + (ok ? row : 0)] : -1;
            cnt[k] += __popcll(__ballot(v >= 0));
        }
    }
#pragma unroll
    for (int k = 0; k < KT; k++) nb += (cnt[k] + 15) >> 4;
    if (lane_id() == 0) tile_nb[tile] = nb;
}

template <int KT, int RPT>
__global__ __launch_bounds__(256) void pairlist_fill_kernel(const int *__restrict__ nbr, int K, int Vout, int tiles,
                                                            const int *__restrict__ tile_start, int2 *__restrict__ entries)
{
    constexpr int H = RPT >= 64 ? RPT / 64 : 1, LIVE = RPT >= 64 ? 64 : RPT;
    const int tile = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (tile >= tiles) return;
    const int l = lane_id();
    int v[H][KT];   // all table entries of the tile first (one round trip), then the compaction
#pragma unroll
    for (int h = 0; h < H; h++) {
        const int row = tile * RPT + 64 * h + l;
        const bool ok = row < Vout && l < LIVE;
#pragma unroll
        for (int k = 0; k < KT; k++) v[h][k] = (ok && k < K) ? nbr[(size_t)min(k, K - 1) * Vout + (ok ? row : 0)] : -1;
    }
    size_t base = (size_t)tile_start[tile] * 16;
#pragma unroll
    for (int k = 0; k < KT; k++) {
        int n = 0;
#pragma unroll
        for (int h = 0; h < H; h++) {
            const unsigned long long m = __ballot(v[h][k] >= 0);
            if (v[h][k] >= 0) entries[base + n + ballot_rank(m)] = make_int2(v[h][k], (k << 8) | (64 * h + l));
            n += __popcll(m);
        }
        const int n16 = (n + 15) & ~15;
        if (l < n16 - n) entries[base + n + l] = make_int2(0, (k << 8) | RPT);
        base += n16;
    }
}

// Schedule of a pair list for the kernels that walk it.  A wave works through a tile as a chain of dependent round
// trips per batch group, tiles differ ~4x in batches (14..63 on 2 cm scans) and neighbouring tiles are correlated, so
// a launch lasts as long as its most loaded wave.  The tiles are therefore cut into MS3D_PL_PARTS parts of near-equal
// batch count (a tile belongs to the part its first batch falls into; one part per block), and inside a part the
// tiles are listed longest first (per run of 64 tiles), the order in which the block's waves pick them up.
__global__ __launch_bounds__(256) void pairlist_parts_kernel(const int *__restrict__ tile_start, int tiles,
                                                             int *__restrict__ part_start)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles) return;
    const long total = tile_start[tiles];
    auto part_of = [&](int tile) {
        const long p = total > 0 ? (long)tile_start[tile] * MS3D_PL_PARTS / total : 0;
        return (int)(p < MS3D_PL_PARTS - 1 ? p : MS3D_PL_PARTS - 1);
    };
    const int mine = part_of(t), prev = t > 0 ? part_of(t - 1) : -1;
    for (int q = prev + 1; q <= mine; q++) part_start[q] = t;
    if (t == tiles - 1)
        for (int q = mine + 1; q <= MS3D_PL_PARTS; q++) part_start[q] = tiles;
}

__global__ __launch_bounds__(64) void pairlist_order_kernel(const int *__restrict__ tile_start,
                                                            const int *__restrict__ part_start, int4 *__restrict__ order)
{
    const int l = lane_id();
    const int t0 = part_start[blockIdx.x], t1 = part_start[blockIdx.x + 1];
    for (int c = t0; c < t1; c += 64) {
        const int tile = c + l;
        const bool ok = tile < t1;
        const int cnt = ok ? tile_start[tile + 1] - tile_start[tile] : -1;
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const int cj = __builtin_amdgcn_readlane(cnt, j);
            rank += (cj > cnt || (cj == cnt && j < l)) ? 1 : 0;
        }
        if (ok) order[c + rank] = make_int4(tile, tile_start[tile], tile_start[tile + 1], 0);  // all a wave needs to start the tile
    }
}

// Part cut of an offset-major list.  kt_start is an exclusive scan in (offset, tile) order, so the number of pairs in
// tiles [0, t) over all offsets is sum_k (kt_start[k * tiles + t] - kt_start[k * tiles]): no second scan.  Writes that
// per-tile prefix ([tiles + 1]) and part_start (same rule as pairlist_parts_kernel: a tile belongs to the part its
// first pair falls into).
__global__ __launch_bounds__(256) void offsetlist_parts_kernel(const int *__restrict__ kt_start, int K, int tiles,
                                                               int *__restrict__ part_start, int *__restrict__ tile_prefix)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > tiles) return;
    const long total = kt_start[(size_t)K * tiles];
    long mine = 0, prev = 0;
    for (int k = 0; k < K; k++) {
        const int base = kt_start[(size_t)k * tiles];
        mine += kt_start[(size_t)k * tiles + t] - base;
        if (t > 0) prev += kt_start[(size_t)k * tiles + t - 1] - base;
    }
    tile_prefix[t] = (int)mine;
    if (t == tiles) return;
    auto part_of = [&](long first) {
        const long p = total > 0 ? first * MS3D_PL_PARTS / total : 0;
        return (int)(p < MS3D_PL_PARTS - 1 ? p : MS3D_PL_PARTS - 1);
    };
    const int q1 = part_of(mine), q0 = t > 0 ? part_of(prev) : -1;
    for (int q = q0 + 1; q <= q1; q++) part_start[q] = t;
    if (t == tiles - 1)
        for (int q = q1 + 1; q <= MS3D_PL_PARTS; q++) part_start[q] = tiles;
}

// Offset-major pair lists (the classic in/out index pairs per kernel offset) for the backward-weight kernel:
// kt_start[k * tiles + tile] = first pair of (offset k, 64-row tile), pairs in ascending output row inside it.
template <int KT>
__global__ __launch_bounds__(256) void offsetlist_count_kernel(const int *__restrict__ nbr, int K, int Vout, int tiles,
                                                               int *__restrict__ kt_count)
{
    const int tile = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (tile >= tiles) return;
    const int l = lane_id();
    const int row = tile * MS3D_PL_ROWS + l;
    const bool ok = row < Vout;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < KT; k++) {
        const int v = (ok && k < K) ? nbr[(size_t)min(k, K - 1) * Vout + (ok ? row : 0)] : -1;
        const int n = __popcll(__ballot(v >= 0));
        if (l == k) mine = n;
    }
    if (l < K) kt_count[(size_t)l * tiles + tile] = mine;
    if (tile == 0 && l == 0) kt_count[(size_t)K * tiles] = 0;  // slot for the grand total
}

template <int KT>
__global__ __launch_bounds__(256) void offsetlist_fill_kernel(const int *__restrict__ nbr, int K, int Vout, int tiles,
                                                              const int *__restrict__ kt_start, int2 *__restrict__ entries)
{
    const int tile = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (tile >= tiles) return;
    const int l = lane_id();
    const int row = tile * MS3D_PL_ROWS + l;
    const bool ok = row < Vout;
    int v[KT], st[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        v[k] = (ok && k < K) ? nbr[(size_t)min(k, K - 1) * Vout + (ok ? row : 0)] : -1;
        st[k] = kt_start[(size_t)min(k, K - 1) * tiles + tile];
    }
#pragma unroll
    for (int k = 0; k < KT; k++) {
        const unsigned long long m = __ballot(v[k] >= 0);
        if (v[k] >= 0) entries[(size_t)st[k] + ballot_rank(m)] = make_int2(v[k], row);
    }
}

}  // namespace

extern "C" {

size_t ms3d_coord_workspace_bytes(int n)
{
    CoordWs w;
    return carve(w, n > 0 ? n : 1, nullptr);
}

int ms3d_sparse_quantize(const int *coords, int n, int *unique_idx, int *inverse, int *n_unique, void *workspace,
                         size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    *n_unique = 0;
    if (n <= 0) return 0;
    CoordWs w;
    if (carve(w, n, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    int rc = build_table(w, coords, n, 1, stream);
    if (rc) return rc;
    rc = rank_first(w, n, n_unique, stream);
    if (rc) return rc;
    unique_emit_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(n, w.slot_of_row, w.vals, w.rank, unique_idx, inverse);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_k3(const int *coords, int V, int tensor_stride, int *nbr, void *workspace, size_t workspace_bytes,
                 ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V <= 0) return 0;
    CoordWs w;
    if (carve(w, V, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    int rc = build_table(w, coords, V, 1, stream);
    if (rc) return rc;
    static const bool sym = [] { const char *e = getenv("MS3D_KMAP_SYM"); return !e || atoi(e) != 0; }();
    if (sym) {
        MS3D_CHECK(hipMemsetAsync(nbr + (size_t)14 * V, 0xFF, sizeof(int) * (size_t)13 * V, stream));
        dim3 grid(ms3d_divup(V, 256), 14);
        kmap_k3_sym_kernel<<<grid, 256, 0, stream>>>(coords, V, tensor_stride, w.keys, w.vals, (unsigned)w.H - 1u, nbr);
    } else {
        dim3 grid(ms3d_divup(V, 256), 27);
        kmap_k3_kernel<<<grid, 256, 0, stream>>>(coords, V, tensor_stride, w.keys, w.vals, (unsigned)w.H - 1u, nbr);
    }
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_downsample(const int *coords, int V, int tensor_stride, int *out_coords, int *parent, int *koff, int *n_coarse,
                    void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    *n_coarse = 0;
    if (V <= 0) return 0;
    CoordWs w;
    if (carve(w, V, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    int rc = build_table(w, coords, V, tensor_stride * 2, stream);
    if (rc) return rc;
    rc = rank_first(w, V, n_coarse, stream);
    if (rc) return rc;
    downsample_emit_kernel<<<ms3d_divup(V, 256), 256, 0, stream>>>(V, tensor_stride, coords, w.slot_of_row, w.vals, w.rank,
                                                                 out_coords, parent, koff);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_morton_keys(const int *coords, int V, long long *keys, ms3d_stream_t stream)
{
    if (V <= 0) return 0;
    morton_keys_kernel<<<ms3d_divup(V, 256), 256, 0, (hipStream_t)stream>>>(coords, V, keys);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_k2(const int *parent, const int *koff, int Vf, int Vc, int *nbr_down, int *nbr_up, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (Vf <= 0) return 0;
    fill_minus1_kernel<<<ms3d_divup((long)Vc * 8, 256), 256, 0, stream>>>(nbr_down, (long)Vc * 8);
    MS3D_LAUNCH_CHECK();
    fill_minus1_kernel<<<ms3d_divup((long)Vf * 8, 256), 256, 0, stream>>>(nbr_up, (long)Vf * 8);
    MS3D_LAUNCH_CHECK();
    kmap_k2_kernel<<<ms3d_divup(Vf, 256), 256, 0, stream>>>(parent, koff, Vf, Vc, nbr_down, nbr_up);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_general(const int *in_coords, int Vin, const int *out_coords, int Vout, const int *offsets, int K, int *nbr,
                      void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > 65535) return MS3D_E_UNSUPPORTED;
    if (Vout <= 0) return 0;
    if (Vin <= 0) {
        fill_minus1_kernel<<<ms3d_divup((long)Vout * K, 256), 256, 0, stream>>>(nbr, (long)Vout * K);
        MS3D_LAUNCH_CHECK();
        return 0;
    }
    CoordWs w;
    if (carve(w, Vin, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    int rc = build_table(w, in_coords, Vin, 1, stream);
    if (rc) return rc;
    dim3 grid(ms3d_divup(Vout, 256), K);
    kmap_general_kernel<<<grid, 256, 0, stream>>>(out_coords, Vout, offsets, K, w.keys, w.vals, (unsigned)w.H - 1u, nbr);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_region(const int *coords, int V, const int *offsets, const int *partner, int K, int *nbr_fwd, int *nbr_inv,
                     void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > 254 || !partner) return MS3D_E_UNSUPPORTED;
    RegionPartner rp;
    for (int k = 0; k < K; ++k) {
        const int p = partner[k];
        if (p != -1 && (p < 0 || p >= K || partner[p] != k)) return MS3D_E_UNSUPPORTED;     // not an involution
        rp.p[k] = (unsigned char)(p < 0 ? REGION_NO_PARTNER : p);
    }
    for (int k = K; k < 256; ++k) rp.p[k] = (unsigned char)REGION_NO_PARTNER;
    if (V < 0) return MS3D_E_UNSUPPORTED;
    CoordWs w;
    if (carve(w, V > 0 ? V : 1, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    if (V == 0) return 0;
    if (!coords || !offsets || !nbr_fwd || !nbr_inv || !workspace) return MS3D_E_UNSUPPORTED;
    int rc = build_table(w, coords, V, 1, stream);
    if (rc) return rc;
    const long n = (long)V * K;
    if (nbr_inv == nbr_fwd + n) {           // one allocation [2][K][V] (what the Python backend hands over): one fill
        fill_minus1_kernel<<<ms3d_divup(2 * n, 256), 256, 0, stream>>>(nbr_fwd, 2 * n);
        MS3D_LAUNCH_CHECK();
    } else {
        fill_minus1_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(nbr_fwd, n);
        MS3D_LAUNCH_CHECK();
        fill_minus1_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(nbr_inv, n);
        MS3D_LAUNCH_CHECK();
    }
    dim3 grid(ms3d_divup(V, 256), K);
    kmap_region_kernel<<<grid, 256, 0, stream>>>(coords, V, offsets, K, rp, w.keys, w.vals, (unsigned)w.H - 1u, w.slot_of_row,
                                                 w.total + 1, nbr_fwd, nbr_inv);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_interp_map(const int *coords, int Vin, const float *points, long N, int tensor_stride, int *rows, float *weights,
                    void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (tensor_stride < 1 || (tensor_stride & (tensor_stride - 1)) != 0) return MS3D_E_UNSUPPORTED;
    if (N < 0 || N > 0x7fffffffL / 8 || Vin < 0) return MS3D_E_UNSUPPORTED;      // 8 N entries are numbered by ints
    if (N == 0 || Vin == 0) return 0;
    if (!coords || !points || !rows || !weights || !workspace) return MS3D_E_UNSUPPORTED;
    CoordWs w;
    if (carve(w, Vin, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    int rc = build_table(w, coords, Vin, 1, stream);
    if (rc) return rc;
    dim3 grid(ms3d_divup(N, 256), 8);
    interp_map_kernel<<<grid, 256, 0, stream>>>(points, (int)N, (float)tensor_stride, w.keys, w.vals, (unsigned)w.H - 1u, rows,
                                                weights);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_invert(const int *nbr, int K, int Vout, int Vin, int *nbr_inv, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > 65535) return MS3D_E_UNSUPPORTED;
    if (Vin <= 0) return 0;
    fill_minus1_kernel<<<ms3d_divup((long)Vin * K, 256), 256, 0, stream>>>(nbr_inv, (long)Vin * K);
    MS3D_LAUNCH_CHECK();
    if (Vout <= 0) return 0;
    dim3 grid(ms3d_divup(Vout, 256), K);
    kmap_invert_kernel<<<grid, 256, 0, stream>>>(nbr, Vout, Vin, nbr_inv);
    MS3D_LAUNCH_CHECK();
    return 0;
}

size_t ms3d_coords_expand_workspace_bytes(int Vin, int K)
{
    ExpandWs w;
    const long long N = (long long)(Vin > 0 ? Vin : 0) * (K > 0 ? K : 0);
    if (N > 0x7fffffffll) return 0;
    return carve_expand(w, N > 0 ? N : 1, nullptr);
}

int ms3d_coords_expand(const int *in_coords, int Vin, const int *offsets, int K, int *out_coords, int *n_out, void *workspace,
                       size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    *n_out = 0;
    if (K < 1) return MS3D_E_UNSUPPORTED;
    if (Vin <= 0) return 0;
    const long long N = (long long)Vin * K;
    if (N > 0x7fffffffll) return MS3D_E_UNSUPPORTED;       // candidate indices are the int values of the table
    ExpandWs w;
    if (carve_expand(w, N, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    const int grid = expand_grid(N);
    expand_clear_kernel<<<expand_grid((long long)w.H), 256, 0, stream>>>(w.keys, w.vals, w.H, w.total + 1);
    MS3D_LAUNCH_CHECK();
    expand_insert_kernel<<<grid, 256, 0, stream>>>(in_coords, offsets, K, N, w.keys, w.vals, (unsigned)(w.H - 1), w.slot_of_cand,
                                                   w.total + 1);
    MS3D_LAUNCH_CHECK();
    expand_flag_kernel<<<grid, 256, 0, stream>>>(N, w.slot_of_cand, w.vals, w.total + 1, w.rank);
    MS3D_LAUNCH_CHECK();
    int rc = ms3d_exclusive_scan_i32(w.rank, w.rank, (int)N, w.total, w.scan_ws, stream);
    if (rc) return rc;
    int h[2] = {0, 0};   // [0] number of distinct candidates  [1] a candidate did not fit the key
    MS3D_CHECK(hipMemcpyAsync(h, w.total, sizeof(int) * 2, hipMemcpyDeviceToHost, stream));
    MS3D_CHECK(hipStreamSynchronize(stream));
    if (h[1]) return MS3D_E_UNSUPPORTED;
    *n_out = h[0];
    expand_emit_kernel<<<grid, 256, 0, stream>>>(in_coords, offsets, K, N, w.slot_of_cand, w.vals, w.rank, out_coords);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_coords_prune(const int *coords, int V, const unsigned char *keep, int *out_coords, int *src_row, int *dst_row,
                      int *n_kept, void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    *n_kept = 0;
    if (V <= 0) return 0;
    CoordWs w;
    if (carve(w, V, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    const int grid = expand_grid(V);
    prune_flag_kernel<<<grid, 256, 0, stream>>>(V, keep, w.rank);
    MS3D_LAUNCH_CHECK();
    int rc = ms3d_exclusive_scan_i32(w.rank, w.rank, V, w.total, w.scan_ws, stream);
    if (rc) return rc;
    MS3D_CHECK(hipMemcpyAsync(n_kept, w.total, sizeof(int), hipMemcpyDeviceToHost, stream));
    prune_emit_kernel<<<grid, 256, 0, stream>>>(V, coords, keep, w.rank, out_coords, src_row, dst_row);
    MS3D_LAUNCH_CHECK();
    MS3D_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int ms3d_coords_check(const int *coords, int V, int lattice, int *flags, void *workspace, size_t workspace_bytes,
                      ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!flags) return MS3D_E_UNSUPPORTED;
    *flags = 0;
    if (lattice < 1 || V < 0) return MS3D_E_UNSUPPORTED;
    if (V == 0) return 0;
    if (!coords || !workspace) return MS3D_E_UNSUPPORTED;
    CoordWs w;
    if (carve(w, V, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    int rc = build_table(w, coords, V, 1, stream);      // (clears w.total[1] and raises MS3D_COORDS_OUT_OF_RANGE in it)
    if (rc) return rc;
    coords_check_kernel<<<ms3d_divup(V, 256), 256, 0, stream>>>(coords, V, lattice, w.slot_of_row, w.vals, w.total + 1);
    MS3D_LAUNCH_CHECK();
    int h = 0;
    MS3D_CHECK(hipMemcpyAsync(&h, w.total + 1, sizeof(int), hipMemcpyDeviceToHost, stream));
    MS3D_CHECK(hipStreamSynchronize(stream));
    *flags = h;
    return 0;
}

size_t ms3d_coords_union_workspace_bytes(int total_rows)
{
    if (total_rows > UNION_MAX_ROWS) return 0;
    CoordWs w;
    int *seen, *dup;
    return carve_union(w, &seen, &dup, total_rows > 0 ? total_rows : 1, nullptr);
}

int ms3d_coords_union(const int *coords, const int *set_start, int n_sets, int *out_coords, int *out_row, int *in_row,
                      int *n_out, void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    *n_out = 0;
    if (n_sets < 1 || n_sets > UNION_MAX_SETS || !set_start) return MS3D_E_UNSUPPORTED;
    UnionSets sets;
    sets.n = n_sets;
    for (int i = 0; i <= UNION_MAX_SETS; i++) sets.start[i] = set_start[i <= n_sets ? i : n_sets];
    if (sets.start[0] != 0) return MS3D_E_UNSUPPORTED;
    for (int i = 0; i < n_sets; i++)
        if (sets.start[i + 1] < sets.start[i]) return MS3D_E_UNSUPPORTED;
    const int n = sets.start[n_sets];
    if (n > UNION_MAX_ROWS) return MS3D_E_UNSUPPORTED;
    if (n == 0) return 0;                                      // every set is empty: the empty set, nothing is launched
    CoordWs w;
    int *seen, *dup;
    if (carve_union(w, &seen, &dup, n, workspace) > workspace_bytes) return MS3D_E_WORKSPACE;
    MS3D_CHECK(hipMemsetAsync(seen, 0, sizeof(int) * (size_t)w.H, stream));
    MS3D_CHECK(hipMemsetAsync(dup, 0, sizeof(int), stream));
    int rc = build_table(w, coords, n, 1, stream);
    if (rc) return rc;
    union_flag_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(n, sets, w.slot_of_row, w.vals, seen, w.flag, dup);
    MS3D_LAUNCH_CHECK();
    rc = ms3d_exclusive_scan_i32(w.flag, w.rank, n, w.total, w.scan_ws, stream);
    if (rc) return rc;
    int h[3] = {0, 0, 0};   // [0] distinct coordinates  [1] a row did not fit the key  [2] a row repeats inside its set
    MS3D_CHECK(hipMemcpyAsync(h, w.total, sizeof(int) * 2, hipMemcpyDeviceToHost, stream));
    MS3D_CHECK(hipMemcpyAsync(h + 2, dup, sizeof(int), hipMemcpyDeviceToHost, stream));
    MS3D_CHECK(hipStreamSynchronize(stream));
    if (h[1] || h[2]) return MS3D_E_UNSUPPORTED;
    *n_out = h[0];
    const long cells = (long)n_sets * h[0];
    fill_minus1_kernel<<<ms3d_divup(cells, 256), 256, 0, stream>>>(in_row, cells);
    MS3D_LAUNCH_CHECK();
    union_emit_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(n, h[0], sets, coords, w.slot_of_row, w.vals, w.rank, out_coords,
                                                            out_row, in_row);
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_pairlist_tiles(int Vout) { return ms3d_divup(Vout, MS3D_PL_ROWS); }

// ints of the tile_start array: tiles + 1 batch offsets, part_start[MS3D_PL_PARTS + 1], (pad to 16 bytes,) the pick
// list int4[tiles] = (tile, first batch, end batch, 0)
int ms3d_kmap_pairlist_header_ints_rows(int Vout, int rows_per_tile)
{
    const int tiles = ms3d_divup(Vout, rows_per_tile);
    return MS3D_PL_SCHED_OFFSET(tiles) + 4 * tiles;
}
int ms3d_kmap_pairlist_header_ints(int Vout) { return ms3d_kmap_pairlist_header_ints_rows(Vout, MS3D_PL_ROWS); }

size_t ms3d_kmap_pairlist_capacity_rows(int K, int Vout, int rows_per_tile)
{
    // every (tile, offset) group pads by < 16 entries; + one group of slack (an empty last tile still reads its first slots)
    return (size_t)K * ((size_t)Vout + 15 * (size_t)ms3d_divup(Vout, rows_per_tile)) + 128;
}
size_t ms3d_kmap_pairlist_capacity(int K, int Vout) { return ms3d_kmap_pairlist_capacity_rows(K, Vout, MS3D_PL_ROWS); }

// host-side note of every list's tile size, keyed by the address of its header (see the header file)
static std::mutex g_pl_rows_lock;
static std::unordered_map<const int *, int> g_pl_rows;
int ms3d_kmap_pairlist_rows_of(const int *tile_start)
{
    if (!tile_start) return 0;
    std::lock_guard<std::mutex> guard(g_pl_rows_lock);
    auto it = g_pl_rows.find(tile_start);
    return it == g_pl_rows.end() ? MS3D_PL_ROWS : it->second;
}

int ms3d_kmap_pairlist_build_rows(const int *nbr, int K, int Vout, int rows_per_tile, int *tile_start, int *entries,
                                  void *workspace, size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (Vout <= 0) return 0;
    if (K > 27 || (rows_per_tile != 32 && rows_per_tile != 64 && rows_per_tile != 128)) return MS3D_E_UNSUPPORTED;
    {
        std::lock_guard<std::mutex> guard(g_pl_rows_lock);
        if (g_pl_rows.size() > 65536)                        // addresses of long-gone lists: entries that say the default go
            for (auto it = g_pl_rows.begin(); it != g_pl_rows.end();) it = it->second == MS3D_PL_ROWS ? g_pl_rows.erase(it) : std::next(it);
        g_pl_rows[tile_start] = rows_per_tile;
    }
    if (workspace_bytes < ms3d_scan_workspace_bytes()) return MS3D_E_WORKSPACE;
    const int tiles = ms3d_divup(Vout, rows_per_tile);
    const int grid = ms3d_divup((long)(tiles + 1) * 64, 256);
    const bool wide = rows_per_tile == 128, narrow = rows_per_tile == 32;
    if (K <= 8) {
        if (wide) pairlist_count_kernel<8, 128><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start);
        else if (narrow) pairlist_count_kernel<8, 32><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start);
        else pairlist_count_kernel<8, 64><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start);
    } else {
        if (wide) pairlist_count_kernel<27, 128><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start);
        else if (narrow) pairlist_count_kernel<27, 32><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start);
        else pairlist_count_kernel<27, 64><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start);
    }
    MS3D_LAUNCH_CHECK();
    int rc = ms3d_exclusive_scan_i32(tile_start, tile_start, tiles + 1, nullptr, workspace, stream);
    if (rc) return rc;
    int *part_start = tile_start + tiles + 1;
    int4 *order = reinterpret_cast<int4 *>(tile_start + MS3D_PL_SCHED_OFFSET(tiles));
    pairlist_parts_kernel<<<ms3d_divup(tiles, 256), 256, 0, stream>>>(tile_start, tiles, part_start);
    MS3D_LAUNCH_CHECK();
    pairlist_order_kernel<<<MS3D_PL_PARTS, 64, 0, stream>>>(tile_start, part_start, order);
    MS3D_LAUNCH_CHECK();
    int2 *ent = reinterpret_cast<int2 *>(entries);
    if (K <= 8) {
        if (wide) pairlist_fill_kernel<8, 128><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start, ent);
        else if (narrow) pairlist_fill_kernel<8, 32><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start, ent);
        else pairlist_fill_kernel<8, 64><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start, ent);
    } else {
        if (wide) pairlist_fill_kernel<27, 128><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start, ent);
        else if (narrow) pairlist_fill_kernel<27, 32><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start, ent);
        else pairlist_fill_kernel<27, 64><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, tile_start, ent);
    }
    MS3D_LAUNCH_CHECK();
    return 0;
}

int ms3d_kmap_pairlist_build(const int *nbr, int K, int Vout, int *tile_start, int *entries, void *workspace,
                             size_t workspace_bytes, ms3d_stream_t stream)
{
    return ms3d_kmap_pairlist_build_rows(nbr, K, Vout, MS3D_PL_ROWS, tile_start, entries, workspace, workspace_bytes, stream);
}

// ints of the kt_start array: K * tiles + 1 pair offsets, part_start[MS3D_PL_PARTS + 1], pair prefix per tile [tiles + 1]
size_t ms3d_kmap_offsetlist_header_ints(int K, int Vout)
{
    const size_t tiles = ms3d_divup(Vout > 0 ? Vout : 0, MS3D_PL_ROWS);
    return (size_t)K * tiles + 1 + MS3D_PL_PARTS + 1 + tiles + 1;
}

size_t ms3d_kmap_offsetlist_capacity(int K, int Vout) { return (size_t)K * (size_t)(Vout > 0 ? Vout : 0); }

int ms3d_kmap_offsetlist_build(const int *nbr, int K, int Vout, int *kt_start, int *entries, void *workspace,
                               size_t workspace_bytes, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (Vout <= 0) return 0;
    if (K > 27) return MS3D_E_UNSUPPORTED;
    if (workspace_bytes < ms3d_scan_workspace_bytes()) return MS3D_E_WORKSPACE;
    const int tiles = ms3d_divup(Vout, MS3D_PL_ROWS);
    const int grid = ms3d_divup((long)tiles * 64, 256);
    if (K <= 8)
        offsetlist_count_kernel<8><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, kt_start);
    else
        offsetlist_count_kernel<27><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, kt_start);
    MS3D_LAUNCH_CHECK();
    int rc = ms3d_exclusive_scan_i32(kt_start, kt_start, K * tiles + 1, nullptr, workspace, stream);
    if (rc) return rc;
    if (K <= 8)
        offsetlist_fill_kernel<8><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, kt_start, reinterpret_cast<int2 *>(entries));
    else
        offsetlist_fill_kernel<27><<<grid, 256, 0, stream>>>(nbr, K, Vout, tiles, kt_start, reinterpret_cast<int2 *>(entries));
    MS3D_LAUNCH_CHECK();
    // tile ranges of near-equal pair count for the workgroups of the backward-weight kernel (equal ROW ranges differ
    // ~1.4x in pairs on a scan, and the launch lasts as long as its fullest workgroup)
    int *part_start = kt_start + (size_t)K * tiles + 1, *tile_prefix = part_start + MS3D_PL_PARTS + 1;
    offsetlist_parts_kernel<<<ms3d_divup(tiles + 1, 256), 256, 0, stream>>>(kt_start, K, tiles, part_start, tile_prefix);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
