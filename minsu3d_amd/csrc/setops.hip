// Feature arithmetic across coordinate sets (MinkowskiUnion, SparseTensor + - *, the MinkowskiBroadcast family).
//
// Every kernel is a GATHER with one writer per output element and a fixed order of additions; nothing adds floats
// atomically, so forward and backward give the same bytes on every run:
//   union combine   out[o] = F_0[in_row[0][o]] (op) F_1[in_row[1][o]] ...   ascending input order, through the maps of
//                   ms3d_coords_union; an absent operand is skipped (sum), or follows the zero-fill rule below
//   its backward    din_i[r] = dout[out_row_i[r]] (negated / scaled by the other operand's row)
//   broadcast       out[r] = x[r] (op) g[grow[r]]; the gradient of x is the identity, a column slice or the same kernel
//   its reduction   dg[j] = sum over the rows of g row j's batch of dout[r] (* x[r]): per-slice partial sums in a fixed
//                   thread order, then a combine in slice order
// Layout: csrc/rows.h.
//
// The rule for a coordinate only one operand holds (MinkowskiEngine's, as recalled): the result is zero-filled, receives a
// at a's rows and is then set to fn(out, b) at b's rows -- a + b, a - b (only b: -b), a * b (only a: a; only b: 0 * b).
#include "rows.h"
#include "../../include/minsu3d_hip.h"

namespace {

using namespace ms3d_rows;

enum { OP_SUM = 0, OP_SUB = 1, OP_MUL = 2 };
enum { BC_ADD = 0, BC_MUL = 1, BC_CAT = 2, BC_COPY = 3 };
constexpr int MAX_SETS = 16;
constexpr int REDUCE_SLICES = 64;      // partial sums per global row (ms3d_broadcast_reduce)

struct RowPtrs {
    const float *f[MAX_SETS];
};

template <int VEC>
__global__ __launch_bounds__(256) void union_combine_kernel(RowPtrs in, int n_sets, const int *__restrict__ in_row, int n_out,
                                                            int op, int C, int CV, float *__restrict__ out)
{
    MS3D_ROW_LANE(n_out, CV, o, cv);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) acc[j] = 0.f;
    for (int i = 0; i < n_sets; i++) {
        const int r = in_row[(size_t)i * n_out + o];
        if (r < 0) continue;
        float v[VEC];
        load_row<VEC>(in.f[i], (size_t)r, C, cv, v);
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            if (op == OP_SUM || i == 0) acc[j] = acc[j] + v[j];
            else if (op == OP_SUB) acc[j] = acc[j] - v[j];
            else acc[j] = acc[j] * v[j];
        }
    }
    store_row<VEC>(out, (size_t)o, C, cv, acc);
}

// gradient of operand `which`: one thread group per INPUT row.  other / other_row (multiply only): the features of the other
// operand and its row per union row (in_row[1 - which]).
template <int VEC>
__global__ __launch_bounds__(256) void union_combine_backward_kernel(const float *__restrict__ dout,
                                                                     const int *__restrict__ out_row, int V, int op, int which,
                                                                     const float *__restrict__ other,
                                                                     const int *__restrict__ other_row, int C, int CV,
                                                                     float *__restrict__ din)
{
    MS3D_ROW_LANE(V, CV, r, cv);
    const int o = out_row[r];
    float g[VEC];
    load_row<VEC>(dout, (size_t)o, C, cv, g);
    if (op == OP_SUB && which == 1) {
#pragma unroll
        for (int j = 0; j < VEC; j++) g[j] = -g[j];
    } else if (op == OP_MUL) {
        const int q = other_row[o];
        if (q >= 0) {
            float v[VEC];
            load_row<VEC>(other, (size_t)q, C, cv, v);
#pragma unroll
            for (int j = 0; j < VEC; j++) g[j] = g[j] * v[j];
        } else if (which == 1) {
            // only b holds the coordinate: the forward wrote 0 * b, whose derivative in b is the zero it multiplied
#pragma unroll
            for (int j = 0; j < VEC; j++) g[j] = 0.f;
        }
    }
    store_row<VEC>(din, (size_t)r, C, cv, g);
}

// out [V][Cout]: add / multiply Cout = C = Cg; concatenate Cout = C + Cg (x in front); copy Cout = Cg.  CxV / CoV: C / VEC
// and Cout / VEC.  grow[r] < 0: the voxel's batch index has no global row, it sees the zero vector.  MODE is a template
// parameter: every instance is one straight line of loads, one operation and a store.
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void broadcast_forward_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                                const int *__restrict__ grow, int V, int C, int Cg, int Cout,
                                                                int CxV, int CoV, float *__restrict__ out)
{
    MS3D_ROW_LANE(V, CoV, r, cv);
    float v[VEC];
    if (MODE == BC_CAT && cv < CxV) {
        load_row<VEC>(x, (size_t)r, C, cv, v);
    } else {
        const int q = grow[r];
        float w[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) w[j] = 0.f;
        if (q >= 0) load_row<VEC>(g, (size_t)q, Cg, MODE == BC_CAT ? cv - CxV : cv, w);
        if constexpr (MODE == BC_ADD || MODE == BC_MUL) {
            load_row<VEC>(x, (size_t)r, C, cv, v);
#pragma unroll
            for (int j = 0; j < VEC; j++) v[j] = (MODE == BC_ADD) ? v[j] + w[j] : v[j] * w[j];
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++) v[j] = w[j];
        }
    }
    store_row<VEC>(out, (size_t)r, Cout, cv, v);
}

// Stage 1 of the reduction: block (p, j) sums slice p of the REDUCE_SLICES near-equal slices of the segment of global row j.
// Thread (ty, tx) of the CW x (256 / CW) layout adds the rows ty, ty + RY, ... of the slice in ascending order for the
// columns tx, tx + CW, ...; the RY row lanes are then combined in ascending ty by one thread per column.  Everything is a
// function of (segment length, C) alone: the same bytes on every run.
template <int VEC>
__global__ __launch_bounds__(256) void broadcast_reduce_partial_kernel(const float *__restrict__ dout, int ldd, int col_off,
                                                                       const float *__restrict__ x, int C, int CV, int CW,
                                                                       const long long *__restrict__ order,
                                                                       const int *__restrict__ seg_start,
                                                                       const int *__restrict__ seg_of_g,
                                                                       float *__restrict__ partial)
{
    __shared__ float lds[256 * VEC];
    const int p = blockIdx.x, j = blockIdx.y;
    const int seg = seg_of_g[j];
    int begin = 0, len = 0;
    if (seg >= 0) {
        begin = seg_start[seg];
        len = seg_start[seg + 1] - begin;
    }
    const int per = (len + REDUCE_SLICES - 1) / REDUCE_SLICES;
    const int s0 = min(p * per, len), s1 = min(s0 + per, len);
    const int RY = 256 / CW;
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    float *dst = partial + ((size_t)j * REDUCE_SLICES + p) * C;
    for (int c0 = 0; c0 < CV; c0 += CW) {           // uniform trip count: every thread reaches the barriers
        const int cv = c0 + tx;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[k] = 0.f;
        if (cv < CV) {
            for (int i = s0 + ty; i < s1; i += RY) {
                const size_t r = (size_t)order[begin + i];
                float d[VEC];
                load_vec<VEC>(dout + r * ldd + col_off + VEC * cv, d);
                if (x) {
                    float v[VEC];
                    load_row<VEC>(x, r, C, cv, v);
#pragma unroll
                    for (int k = 0; k < VEC; k++) d[k] = d[k] * v[k];
                }
#pragma unroll
                for (int k = 0; k < VEC; k++) acc[k] = acc[k] + d[k];
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; k++) lds[(ty * CW + tx) * VEC + k] = acc[k];
        __syncthreads();
        if (ty == 0 && cv < CV) {
            float sum[VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) sum[k] = 0.f;
            for (int y = 0; y < RY; y++) {
#pragma unroll
                for (int k = 0; k < VEC; k++) sum[k] = sum[k] + lds[(y * CW + tx) * VEC + k];
            }
            store_row<VEC>(dst, 0, C, cv, sum);
        }
        __syncthreads();
    }
}

// Stage 2: dg[j][c] = partial[j][0][c] + partial[j][1][c] + ... in slice order
__global__ __launch_bounds__(256) void broadcast_reduce_combine_kernel(const float *__restrict__ partial, int G, int C,
                                                                       float *__restrict__ dg)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)G * C) return;
    const int j = (int)(t / C), c = (int)(t - (long)j * C);
    float s = 0.f;
    for (int p = 0; p < REDUCE_SLICES; p++) s = s + partial[((size_t)j * REDUCE_SLICES + p) * C + c];
    dg[t] = s;
}

}  // namespace

extern "C" {

int ms3d_union_combine(int op, const float *const *in_feats, int n_sets, const int *in_row, int n_out, int C, float *out,
                       ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_sets < 1 || n_sets > MAX_SETS || !in_feats || C < 1) return MS3D_E_UNSUPPORTED;
    if (op < OP_SUM || op > OP_MUL || (op != OP_SUM && n_sets != 2)) return MS3D_E_UNSUPPORTED;
    if (n_out <= 0) return 0;
    RowPtrs in;
    bool v4 = vec4(C, out);
    for (int i = 0; i < MAX_SETS; i++) {
        in.f[i] = i < n_sets ? in_feats[i] : nullptr;
        v4 = v4 && ms3d_aligned16(in.f[i]);
    }
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(n_out, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, union_combine_kernel, blocks, 256, 0, stream, in, n_sets, in_row, n_out, op, C, CV, out);
    return 0;
}

int ms3d_union_combine_backward(int op, int which, const float *dout, const int *out_row, int V, const float *other,
                                const int *other_row, int C, float *din, ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (op < OP_SUM || op > OP_MUL || which < 0 || which >= MAX_SETS || C < 1) return MS3D_E_UNSUPPORTED;
    if (op != OP_SUM && which > 1) return MS3D_E_UNSUPPORTED;
    if (op == OP_MUL && !other_row) return MS3D_E_UNSUPPORTED;
    if (V <= 0) return 0;
    const bool v4 = vec4(C, dout, din, other);
    const int CV = v4 ? C / 4 : C;
    unsigned blocks;
    if (!grid_of(V, CV, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_VEC(v4, union_combine_backward_kernel, blocks, 256, 0, stream, dout, out_row, V, op, which, other, other_row, C, CV,
                    din);
    return 0;
}

int ms3d_broadcast_forward(int mode, const float *x, const float *g, const int *grow, int V, int C, int Cg, float *out,
                           ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (mode < BC_ADD || mode > BC_COPY || Cg < 1) return MS3D_E_UNSUPPORTED;
    if (mode == BC_COPY) C = 0;
    else if (C < 1 || !x) return MS3D_E_UNSUPPORTED;
    if ((mode == BC_ADD || mode == BC_MUL) && C != Cg) return MS3D_E_UNSUPPORTED;
    if (V <= 0) return 0;
    const int Cout = (mode == BC_CAT) ? C + Cg : Cg;
    const bool v4 = vec4(C, x, g, out) && Cg % 4 == 0;
    const int vec = v4 ? 4 : 1;
    unsigned blocks;
    if (!grid_of(V, Cout / vec, &blocks)) return MS3D_E_UNSUPPORTED;
    MS3D_LAUNCH_MODE_VEC((BC_ADD, BC_MUL, BC_CAT, BC_COPY), mode, v4, broadcast_forward_kernel, blocks, 256, 0, stream, x, g, grow,
                         V, C, Cg, Cout, C / vec, Cout / vec, out);
    return 0;
}

size_t ms3d_broadcast_reduce_workspace_bytes(int G, int C)
{
    return sizeof(float) * (size_t)(G > 0 ? G : 1) * REDUCE_SLICES * (size_t)(C > 0 ? C : 1);
}

int ms3d_broadcast_reduce(const float *dout, int ldd, int col_off, const float *x, int C, const long long *order,
                          const int *seg_start, const int *seg_of_g, int G, float *dg, void *workspace, size_t workspace_bytes,
                          ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || col_off < 0 || ldd < col_off + C) return MS3D_E_UNSUPPORTED;
    if (G <= 0) return 0;
    if (G > 65535) return MS3D_E_UNSUPPORTED;                  // one grid row per global row
    if (ms3d_broadcast_reduce_workspace_bytes(G, C) > workspace_bytes) return MS3D_E_WORKSPACE;
    float *partial = (float *)workspace;
    const bool v4 = vec4(C, dout, x, partial) && ldd % 4 == 0 && col_off % 4 == 0;
    const int CV = v4 ? C / 4 : C;
    int CW = 1;
    while (CW < CV && CW < 64) CW <<= 1;
    dim3 grid(REDUCE_SLICES, G);
    MS3D_LAUNCH_VEC(v4, broadcast_reduce_partial_kernel, grid, 256, 0, stream, dout, ldd, col_off, x, C, CV, CW, order, seg_start,
                    seg_of_g, partial);
    broadcast_reduce_combine_kernel<<<ms3d_divup((long)G * C, 256), 256, 0, stream>>>(partial, G, C, dg);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
