// Labels through quantisation: the label of every voxel of ms3d_sparse_quantize from the labels of its points.
//
// Rule (MinkowskiEngine's sequential wording: the first point sets the voxel's label, any later point with another label
// turns it into ignore_label for good) in its order-independent form:
//   out[u] = the common label of all rows i with inverse[i] == u, else ignore_label.
//
// TWO launches on one stream:
//   1. labels_init_kernel     one thread per voxel u:  out[u] = labels[unique_idx[u]]
//   2. labels_dissent_kernel  one thread per row i:    u = inverse[i]; if labels[i] != labels[unique_idx[u]] out[u] = ignore_label
// Why not one: folded into one launch, the first-occurrence row's store of labels[unique_idx[u]] and a dissenting row's
// store of ignore_label go to the same word with DIFFERENT values from threads of different blocks, and nothing orders
// them -- whichever lands last would win.  Letting the first-occurrence row "only initialise" does not remove that pair of
// stores.  Stream order does: every store of launch 1 is complete before launch 2 starts.  Inside launch 2 a row compares
// against the label ARRAY (never against out), so what it decides does not depend on any other thread, and all writers of
// one slot store the same value: plain vector stores, no atomics, no sort, the same bytes on every run.  The
// first-occurrence row agrees with itself and stores nothing.
//
// Layout: consecutive lanes take consecutive rows (labels, inverse: coalesced 4-byte reads); labels[unique_idx[u]] and the
// store to out[u] are gathers / scatters by voxel, as in the reduce-backward kernels of field.hip.  Memory-bound; untuned.
// An index outside its array (a map that is not ms3d_sparse_quantize's) is never followed: such a voxel gets ignore_label,
// such a row stores nothing.
#include "common.h"
#include "../../include/minsu3d_hip.h"

namespace {

__global__ __launch_bounds__(256) void labels_init_kernel(const int *__restrict__ labels, const int *__restrict__ unique_idx,
                                                          int n, int m, int ignore_label, int *__restrict__ out)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= m) return;
    const int f = unique_idx[u];
    out[u] = (unsigned)f < (unsigned)n ? labels[f] : ignore_label;
}

__global__ __launch_bounds__(256) void labels_dissent_kernel(const int *__restrict__ labels, const int *__restrict__ unique_idx,
                                                             const int *__restrict__ inverse, int n, int m, int ignore_label,
                                                             int *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int u = inverse[i];
    if ((unsigned)u >= (unsigned)m) return;
    const int f = unique_idx[u];
    if ((unsigned)f >= (unsigned)n) return;
    if (labels[i] != labels[f]) out[u] = ignore_label;
}

}  // namespace

extern "C" {

int ms3d_quantize_labels(const int *labels, const int *unique_idx, const int *inverse, int n, int m, int ignore_label, int *out,
                         ms3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || m < 0) return MS3D_E_UNSUPPORTED;
    if (n == 0 || m == 0) return 0;
    if (m > n) return MS3D_E_UNSUPPORTED;           // every voxel holds at least its first-occurrence row
    if (!labels || !unique_idx || !inverse || !out) return MS3D_E_UNSUPPORTED;
    labels_init_kernel<<<ms3d_divup(m, 256), 256, 0, stream>>>(labels, unique_idx, n, m, ignore_label, out);
    MS3D_LAUNCH_CHECK();
    labels_dissent_kernel<<<ms3d_divup(n, 256), 256, 0, stream>>>(labels, unique_idx, inverse, n, m, ignore_label, out);
    MS3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
