/*
 * minsu3d_hip.h -- C ABI of libminsu3d_hip.so (hand-written gfx950 HIP kernels).
 *
 * Drop-in boundary for the reference's native layer: every entry point below replaces one
 * function a `COMMON_OPS` / MinkowskiEngine binding calls on the hot path.  Plain pointers and
 * sizes only (no torch types).  All pointers are DEVICE pointers unless a parameter is marked
 * [host].  `stream` is a hipStream_t (pass NULL for the default stream).  Every function
 * returns 0 on success or a non-zero hipError_t / MS3D_E_* code; nothing prints or exits
 * (the reference's launchers fprintf+exit(-1): bfs_cluster.cu:82-86).
 *
 * Citations are file:line into /root/reference/minsu3d/common_ops/src unless noted.
 */
#ifndef MINSU3D_HIP_H
#define MINSU3D_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS3D_E_WORKSPACE 10001 /* workspace too small */
#define MS3D_E_UNSUPPORTED 10002 /* shape outside what the kernels support */
#define MS3D_E_INTERNAL 10003 /* an invariant of the algorithm does not hold (a bug): results are not to be used */

typedef void *ms3d_stream_t; /* hipStream_t */

const char *ms3d_version(void);

/* ---- ball query: replaces ballquery_batch_p_cuda, bfs_cluster/bfs_cluster.h:16, kernel
 * bfs_cluster.cu:15-60.  Same arguments plus the scene count, a workspace and the stream.
 * Canonical output: start_len[i] = (exclusive prefix sum of len, len); lists in
 * ascending index, self included, len = min(hits, 1000).  Entries at positions >= n*meanActive
 * are not written (bfs_cluster.cu:51-58) and the total is returned through *n_active [host]
 * so the wrapper's retry loop (functions/common_ops.py:31-38) behaves identically.
 * Uniform hash grid (cell = 1.01*radius) + count / scan / fill; no per-thread 1000-int stack. */
size_t ms3d_ballquery_workspace_bytes(int n);
int ms3d_ballquery_batch_p(int n, int meanActive, float radius, const float *xyz, const uint8_t *batch_idxs,
                           const int *batch_offsets, int n_scenes, int max_scene_points, int *idx,
                           int *start_len, int *n_active /*[host]*/, int *capped /*[host] or NULL: 1 if any list hit 1000*/,
                           void *workspace, size_t workspace_bytes, ms3d_stream_t stream);

/* ---- BFS clustering: replaces pg_bfs_cluster / sg_bfs_cluster, bfs_cluster/bfs_cluster.h:18-19
 * (host C++ bfs_cluster.cpp:28-187).  Runs on the DEVICE (the reference copies the ball-query
 * result to the host and runs a serial FIFO BFS); output order is identical to the serial BFS:
 * clusters by ascending seed, members in FIFO visit order, including the directed case when
 * the 1000-neighbour cap bites.  cluster_idxs has capacity [N,2], cluster_offsets [N+1];
 * counts[0] = nCluster, counts[1] = sumNPoint are returned to the [host]. */
size_t ms3d_bfs_workspace_bytes(int N);
/* capped_hint: what ms3d_ballquery_batch_p reported for this graph: 0 = no list reached 1000 -> symmetric graph with
 * ascending lists that contain the point itself; 1 = some did (directed: a capped list holds the point's lowest-index
 * neighbours).  -1 = NOBODY VOUCHES for the graph -- any adjacency lists, as the reference's host BFS accepts them
 * (bfs_cluster.cpp:28-54): nothing is assumed (no symmetry, no order inside a list, lists laid out in any order, any
 * length), at the price of a validation pass and two host syncs.  Then MS3D_E_UNSUPPORTED is returned -- instead of a
 * wrong answer or an out-of-bounds read -- for a list header outside [0, n_edges], a target outside [0, N), or a list that
 * names one neighbour twice (the serial loop skips the second mention; the parallel claims cannot). */
int ms3d_pg_bfs_cluster(const int16_t *semantic_label, const int *ball_query_idxs, long n_edges /* = nActive */,
                        const int *start_len, int N, int threshold, int capped_hint, int *cluster_idxs, int *cluster_offsets, int *counts /*[host,2]*/,
                        void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
int ms3d_sg_bfs_cluster(const float *class_numpoint_mean /*[host]*/, const int *ball_query_idxs, long n_edges,
                        const int *start_len, int N, float threshold, int capped_hint, int class_id, int *cluster_idxs,
                        int *cluster_offsets, int *counts /*[host,2]*/, void *workspace, size_t workspace_bytes,
                        ms3d_stream_t stream);

/* all SoftGroup classes in one call: group_of_point u8[N] (class*B + scene, non-decreasing), thr_per_group f32[G]
 * (device); output clusters are class-major = the reference's per-class concatenation (model/softgroup.py:43-83) */
int ms3d_sg_bfs_cluster_batched(const uint8_t *group_of_point, const float *thr_per_group, const int *ball_query_idxs,
                                long n_edges, const int *start_len, int N, int capped_hint, int *cluster_idxs,
                                int *cluster_offsets,
                                int *counts /*[host,2]*/, void *workspace, size_t workspace_bytes, ms3d_stream_t stream);

/* ---- HAIS: replaces hierarchical_aggregation, hierarchical_aggregation/hierarchical_aggregation.h:14-28
 * (host .cpp:8-184 + .cu:20-204) AND the kept/primary merge of functions/hais_ops.py:55-73: the output is the final
 * (cluster_idxs, cluster_offsets) pair -- kept fragments first, then primaries with their absorbed fragments
 * (ascending fragment index).  cluster_idxs capacity [2N,2], cluster_offsets [N+1]; counts -> (nCluster, rows). */
size_t ms3d_hais_workspace_bytes(int N, int nclass);
int ms3d_hierarchical_aggregation(const int16_t *semantic_label, const float *coord_shift, const uint8_t *batch_idxs,
                                  const int *ball_query_idxs, long n_edges, const int *start_len, int N,
                                  int capped_hint /* as for ms3d_pg_bfs_cluster */,
                                  int using_set_aggr, const float *point_num_avg /*[host]*/,
                                  const float *radius_avg /*[host]*/, int nclass, int *cluster_idxs,
                                  int *cluster_offsets, int *counts /*[host,2]*/, void *workspace,
                                  size_t workspace_bytes, ms3d_stream_t stream);

/* The same operator with the reference's OWN output contract (hierarchical_aggregation/hierarchical_aggregation.h:14-28,
 * .cpp:105-184): kept fragments, primaries and -- with set aggregation -- all fragments and the primaries with their
 * absorbed fragments, each as idxs [rows,2], offsets [n+1], centers [n,5] (x, y, z, class, scene).  Used by the
 * `COMMON_OPS.hierarchical_aggregation` shim (minsu3d_amd/dropin/COMMON_OPS.py) so that the reference's wrapper
 * (functions/hais_ops.py:6-79) runs unchanged.  Capacities: N rows / N+1 offsets / 5N floats per list; post_idxs rows
 * beyond post_offsets[n_primary] are zero.  counts [host,8] = n_kept, kept rows, n_primary, post rows, n_fragment,
 * fragment rows, primary rows, 0. */
int ms3d_hierarchical_aggregation_parts(const int16_t *semantic_label, const float *coord_shift, const uint8_t *batch_idxs,
                                        const int *ball_query_idxs, long n_edges, const int *start_len, int N,
                                        int capped_hint, int using_set_aggr, const float *point_num_avg /*[host]*/,
                                        const float *radius_avg /*[host]*/, int nclass, int *kept_idxs, int *kept_offsets,
                                        float *kept_centers, int *prim_idxs, int *prim_offsets, float *prim_centers,
                                        int *frag_idxs, int *frag_offsets, float *frag_centers, int *post_idxs,
                                        int *post_offsets, int *counts /*[host,8]*/, void *workspace,
                                        size_t workspace_bytes, ms3d_stream_t stream);

/* ---- segment ops: replace sec_mean_cuda / sec_min_cuda / sec_max_cuda, sec_mean/sec_mean.h:15-21
 * (kernels sec_mean.cu:12-79).  sec_mean keeps the reference's sequential divide-then-add order
 * per (proposal, channel), so results are bit-identical. */
int ms3d_sec_mean(int nProposal, int C, const float *inp, const int *offsets, float *out, ms3d_stream_t stream);
int ms3d_sec_min(int nProposal, int C, const float *inp, const int *offsets, float *out, ms3d_stream_t stream);
int ms3d_sec_max(int nProposal, int C, const float *inp, const int *offsets, float *out, ms3d_stream_t stream);

/* ---- proposal voxelisation: the arithmetic of clusters_voxelization (minsu3d/model/general_model.py:152-193) between
 * the proposal lists and sparse_quantize -- gather the member coordinates, centre them on the proposal mean
 * (sec_mean's serial order), per-proposal scale = clamp(1 / max_c((hi - lo) / spatial_shape) - 0.01, max = scale),
 * random placement inside the cube with the two U(0,1)^3 draws rand6 = (u1, u2) (device memory), truncate.
 * clusters_idx [S,2] int64 (proposal, point) grouped by proposal; offsets [P+1]; out [S,4] int32 (proposal, x, y, z).
 * Every float operation is the correctly rounded f32 operation of the reference's torch expression, in its order.
 * workspaces: xyz_ws 3*S, mean_ws 3*P, param_ws 4*P floats. */
int ms3d_proposal_voxel_coords(const long long *clusters_idx, int S, const int *offsets, int P, const float *coords,
                               float scale, int spatial_shape, const float *rand6, float *xyz_ws, float *mean_ws,
                               float *param_ws, int *out, ms3d_stream_t stream);

/* ---- pools: replace roipool_fp_cuda / roipool_bp_cuda / global_avg_pool_fp_cuda / _bp_cuda,
 * roipool/roipool.h:17-37 (kernels roipool.cu:12-108).  argmax = first maximum (strict >). */
int ms3d_roipool_fp(int nProposal, int C, const float *feats, const int *proposals_offset, float *output_feats,
                    int *output_maxidx, ms3d_stream_t stream);
int ms3d_roipool_bp(int nProposal, int C, float *d_feats, const int *proposals_offset, const int *output_maxidx,
                    const float *d_output_feats, ms3d_stream_t stream);
int ms3d_global_avg_pool_fp(int nProposal, int C, const float *feats, const int *proposals_offset,
                            float *output_feats, ms3d_stream_t stream);
int ms3d_global_avg_pool_bp(int nProposal, int C, float *d_feats, const int *proposals_offset,
                            const float *d_output_feats, ms3d_stream_t stream);
/* the same with the number of rows the proposals cover (offsets[nProposal] - offsets[0], which the Python wrapper
 * knows as sum_npoint, common_ops.py:160): element-parallel launch instead of one wave per proposal */
int ms3d_global_avg_pool_bp_rows(int nProposal, int C, long n_rows, float *d_feats, const int *proposals_offset,
                                 const float *d_output_feats, ms3d_stream_t stream);

/* out[i, :] = x[idx[i], :] (f32 rows, int64 index): the forward of the row gathers whose backward is
 * ms3d_scatter_add_rows (`features[v2p_map]`, backbone.py:40; `feats[p2v]`, pointgroup.py:89) */
int ms3d_gather_rows(const float *x, const long long *idx /* int64 */, long n, int C, float *out, ms3d_stream_t stream);

/* dst[idx[i], :] = src[i, :] for an index that names no row twice (dst pre-zeroed by the caller): the backward of a row
 * selection such as pruning -- one writer per row, plain stores, bit-reproducible */
int ms3d_scatter_rows(const float *src, const long long *idx /* int64 */, long n, int C, float *dst, ms3d_stream_t stream);

/* dst[idx[i], :] += src[i, :] (dst pre-zeroed by the caller): backward of the row gathers features[v2p_map],
 * feats[c_idxs], features[p2v_map] (reference backbone.py:40, general_model.py:156, pointgroup.py:88) */
int ms3d_scatter_add_rows(const float *src, const long long *idx /* int64 */, long n, int C, float *dst,
                          ms3d_stream_t stream);
/* The same sum in a FIXED order (bit-reproducible; the float atomics of ms3d_scatter_add_rows add in arrival order, which
 * is only harmless while no destination row has more than two sources): keys_sorted = idx sorted ascending by a STABLE
 * sort, order[p] = the source row at sorted position p.  dst pre-zeroed by the caller; one writer per destination row. */
int ms3d_scatter_add_rows_sorted(const float *src, const long long *keys_sorted, const long long *order, long n, int C,
                                 float *dst, ms3d_stream_t stream);

/* ---- IoU family: replace get_iou_cuda (get_iou/get_iou.h:16, get_iou.cu:12-38) and
 * get_mask_iou_on_cluster_cuda / get_mask_iou_on_pred_cuda / get_mask_label_cuda
 * (cal_iou_and_masklabel/cal_iou_and_masklabel.h:28-47, .cu:14-140).  One LDS histogram per
 * proposal instead of the reference's O(P*I*np) rescans; same integer counts, same
 * double-precision quotient rounded to f32. */
int ms3d_get_iou(int nInstance, int nProposal, const int *proposals_idx, const int *proposals_offset,
                 const int16_t *instance_labels, const int *instance_pointnum, float *proposals_iou,
                 ms3d_stream_t stream);
int ms3d_get_mask_iou_on_cluster(int nInstance, int nProposal, const int *proposals_idx,
                                 const int *proposals_offset, const int16_t *instance_labels,
                                 const int *instance_pointnum, float *proposals_iou, ms3d_stream_t stream);
int ms3d_get_mask_iou_on_pred(int nInstance, int nProposal, const int *proposals_idx, const int *proposals_offset,
                              const int16_t *instance_labels, const int *instance_pointnum, float *proposals_iou,
                              const float *mask_scores_sigmoid, ms3d_stream_t stream);
int ms3d_get_mask_label(int nInstance, int nProposal, int ignored_label, float iou_thr, const int *proposals_idx,
                        const int *proposals_offset, const int16_t *instance_labels, const int16_t *instance_cls,
                        const float *proposals_iou, uint8_t *mask_label /*bool*/, uint8_t *mask_label_mask /*bool*/,
                        ms3d_stream_t stream);

/* ======================================================================================
 * Sparse-voxel engine: the MinkowskiEngine subset the reference backbone calls.  MinkowskiEngine is a
 * third-party dependency of the reference (un-pinned, README.md:45,73) and is NOT under /root/reference;
 * the entry points below are what a binding for the reference's call sites would need:
 *   ME.utils.sparse_quantize      data/dataset/general_dataset.py:159-163, model/general_model.py:187-189
 *   ME.SparseTensor / coordinate manager + kernel maps   model/module/backbone.py:38, common.py:69,77
 *   ME.MinkowskiConvolution / ConvolutionTranspose fwd+bwd  model/module/common.py:31,37,40,69,77
 *   ME.MinkowskiBatchNorm / MinkowskiReLU (fused into the conv gather)  common.py:35-39,67-68,75-76
 * Kernel maps are output-stationary neighbour tables stored offset-major: nbr[k * V_out + i] = input row
 * feeding output row i through kernel offset k, or -1.
 * ====================================================================================== */
size_t ms3d_coord_workspace_bytes(int n);
/* first-occurrence unique of int32 rows [n,4] (b,x,y,z): unique_idx[u] ascending, inverse[i] = u;
 * *n_unique -> [host].  unique_idx may be NULL. */
int ms3d_sparse_quantize(const int *coords, int n, int *unique_idx, int *inverse, int *n_unique /*[host]*/,
                         void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
/* labels through that quantisation (csrc/labels.hip): out[u] = the label all rows i with inverse[i] == u share, else
 * ignore_label -- ME's "the first point sets the label, a later point with another label turns it into ignore_label for good"
 * in its order-independent form.  unique_idx [m] and inverse [n] are what ms3d_sparse_quantize returned for the n rows.  Two
 * launches (initialise from the first-occurrence rows, then every dissenting row stores ignore_label: all writers of a slot
 * store one value), plain stores, no atomics, no sort, the same bytes on every run.  n == 0 or m == 0: returns 0, launches
 * nothing; n < 0, m < 0, m > n or a NULL array: MS3D_E_UNSUPPORTED.  An index outside its array is never followed. */
int ms3d_quantize_labels(const int *labels /*[n]*/, const int *unique_idx /*[m]*/, const int *inverse /*[n]*/, int n, int m,
                         int ignore_label, int *out /*[m]*/, ms3d_stream_t stream);
/* submanifold 3x3x3 table nbr[27][V]; offset k = ix + 3*iy + 9*iz <-> (ix-1, iy-1, iz-1)*tensor_stride */
int ms3d_kmap_k3(const int *coords, int V, int tensor_stride, int *nbr, void *workspace, size_t workspace_bytes,
                 ms3d_stream_t stream);
/* stride-2 coarse coordinate set (first-occurrence order), parent row and in-cell offset of every fine row */
int ms3d_downsample(const int *coords, int V, int tensor_stride, int *out_coords, int *parent, int *koff,
                    int *n_coarse /*[host]*/, void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
/* k2 s2 tables: nbr_down[8][Vc] (conv) and nbr_up[8][Vf] (transposed conv) */
int ms3d_kmap_k2(const int *parent, const int *koff, int Vf, int Vc, int *nbr_down, int *nbr_up,
                 ms3d_stream_t stream);

/* General kernel map (any kernel size, stride and dilation): nbr[k][o] = row of in_coords at (batch of o, xyz of o +
 * offsets[k]), or -1.  offsets: DEVICE int[K][3] in voxel units (not multiples of the kernel index: the caller folds
 * dilation and tensor stride in).  A row of in_coords that occurs twice is named by its first occurrence.  A shifted
 * coordinate outside the packable range [-16384, 16384) gives -1.  1 <= K <= 65535; workspace:
 * ms3d_coord_workspace_bytes(Vin).  For a strided layer out_coords is what ms3d_downsample produced. */
int ms3d_kmap_general(const int *in_coords, int Vin, const int *out_coords, int Vout, const int *offsets, int K, int *nbr,
                      void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
/* Inverse table nbr_inv[K][Vin]: nbr_inv[k][i] = o where nbr[k][o] == i, else -1 -- what ms3d_kmap_k2 returns as nbr_up for
 * its one geometry.  Needs distinct output coordinates (then an input row feeds at most one output row per offset and the
 * scatter is collision free: plain stores).  Backward-data of a strided convolution, pooling backward and transposed
 * convolutions onto a cached coordinate set walk it. */
int ms3d_kmap_invert(const int *nbr, int K, int Vout, int Vin, int *nbr_inv, ms3d_stream_t stream);
/* Region map: the kernel map of a coordinate set onto ITSELF over an arbitrary offset list (a cross, a hand-written list:
 * lists that are not their own mirror image k <-> K-1-k), the forward table nbr_fwd[K][V] -- ms3d_kmap_general(coords, coords,
 * offsets) for ANY input, repeated rows included -- AND its inverse nbr_inv[K][V] -- ms3d_kmap_invert of it -- from one pass
 * over one hash table.  nbr_inv is specified for DISTINCT rows only (with repeated rows its bytes are still the same on every
 * run: only the first row of a coordinate writes into it).  offsets: DEVICE int[K][3] in voxel units, distinct rows.
 * partner: HOST int[K], partner[k] = the index of -offsets[k] in the list: k itself for the zero offset, -1 when the list
 * lacks the opposite offset; it is read before anything is launched and handed to the kernel by value.  For distinct rows
 * nbr_fwd[k][i] = j implies nbr_fwd[p][j] = i, nbr_inv[p][i] = j and nbr_inv[k][j] = i with p = partner[k], so only one
 * offset of each partnered pair is looked up and the thread stores all four entries; an unpartnered offset costs one lookup
 * plus one collision-free scatter into nbr_inv, the zero offset none.  Only the row that the table names for its own key (the
 * first occurrence) writes mirrored entries; any other row does its own lookups and writes only its own column: every entry
 * has exactly one writer, no atomics on the tables, no host synchronisation, the same bytes on every run.  A shifted
 * coordinate outside the packable range [-16384, 16384) gives -1, in both tables.
 * Decided on the host before anything is launched: K < 1 or K > 254, or a partner that is not an involution (out of range, or
 * partner[partner[k]] != k): MS3D_E_UNSUPPORTED; a short workspace: MS3D_E_WORKSPACE; V == 0 with valid arguments: returns
 * 0, launches nothing.  workspace: ms3d_coord_workspace_bytes(V). */
int ms3d_kmap_region(const int *coords, int V, const int *offsets /*DEVICE [K][3]*/, const int *partner /*HOST [K]*/, int K,
                     int *nbr_fwd /*[K][V]*/, int *nbr_inv /*[K][V]*/, void *workspace, size_t workspace_bytes,
                     ms3d_stream_t stream);

/* Kernel maps as index pairs (csrc/kmap_pairs.hip): an offset-major table nbr[K][Vout] (int32, -1 = none, valid entries in
 * [0, Vin)) exported as packed per-offset pair lists in the CALLER's row numbering.
 *   out_order [Vout] or NULL  out_order[j] = the row of the table (the held row) of visible output row j; NULL = identity
 *   in_rename [Vin] or NULL   in_rename[i] = the visible row of held input row i; NULL = identity
 *   start [K + 1], DEVICE     int32: start[k] = first pair of offset k, start[K] = P = the number of valid entries
 *   pairs [2][pair_ld]        int64 (so that features[pairs[0]] indexes as it is): row 0 the visible input row, row 1 the
 *                             visible output row; offset k owns columns start[k] .. start[k + 1]; inside an offset the pairs
 *                             ascend in the visible output row j (the kernel walks j and reads nbr[k][out_order[j]]).
 *                             pair_ld >= P is the length of a row of the buffer; columns >= P are not written.
 * An entry >= Vin is never followed into in_rename: it is treated as -1, as is the entry behind an out_order value outside
 * [0, Vout).
 * Two calls with one host read between them: ms3d_kmap_pairs_count (one workgroup per offset and run of
 * ms3d_kmap_pairs_rows() visible output rows: wave ballots and popcounts -> one int per (k, run), k-major; one exclusive scan
 * over them; start[]), the host reads start[K] and allocates pairs, then ms3d_kmap_pairs_fill with the SAME arguments and the
 * SAME, untouched workspace (the same decomposition: ballot again, lane rank by mbcnt, wave bases through LDS, both rows
 * stored at consecutive columns).  No atomics and no sort: every slot has one writer, the same bytes on every run.
 * Decided on the host before anything is launched: K < 1, K > 65535 (the offset is a grid coordinate), Vout < 0, Vin < 0, a NULL
 * nbr / start / pairs, pair_ld < 0 or K * Vout > 2^31 - 1 (P must fit start's int32): MS3D_E_UNSUPPORTED; a workspace shorter
 * than ms3d_kmap_pairs_workspace_bytes(K, Vout) (pure host arithmetic, 4 bytes per (k, run) plus the scan's; 0 for a refused
 * geometry or Vout == 0): MS3D_E_WORKSPACE.  Vout == 0 (or, for the fill, pair_ld == 0): returns 0 and launches nothing -- start
 * is then the caller's to zero. */
int ms3d_kmap_pairs_rows(void);
size_t ms3d_kmap_pairs_workspace_bytes(int K, int Vout);
int ms3d_kmap_pairs_count(const int *nbr, int K, int Vout, int Vin, const int *out_order, int *start /*DEVICE [K + 1]*/,
                          void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
int ms3d_kmap_pairs_fill(const int *nbr, int K, int Vout, int Vin, const int *out_order, const int *in_rename,
                         long long *pairs /*[2][pair_ld]*/, long long pair_ld, const void *workspace, size_t workspace_bytes,
                         ms3d_stream_t stream);

/* ---- coordinate sets that are not derived by flooring: generation and pruning.
 * ms3d_coords_expand: the set of distinct (batch of row i, xyz of row i + offsets[k]) over all input rows i and offsets k, in
 * first-occurrence order of the candidate sequence c = i * K + k (input row major, offset minor) -- the rule
 * ms3d_sparse_quantize and ms3d_downsample follow; deterministic, no sort.  Input rows may repeat.  offsets: DEVICE int[K][3]
 * in voxel units.  Candidates are computed from (i, k) where they are needed; no [Vin * K, 4] array of them is written.
 * out_coords: capacity Vin * K rows of (b, x, y, z); *n_out -> [host] (one sync).  A candidate (or an input row) outside the
 * packable range [-16384, 16384) / batch index outside [0, 524288), or Vin * K > 2^31 - 1: MS3D_E_UNSUPPORTED (never dropped,
 * never aliased; out_coords is then not to be used).  Vin == 0: *n_out = 0, nothing is launched.  workspace:
 * ms3d_coords_expand_workspace_bytes(Vin, K) -- a table of the next power of two >= 2 Vin K slots of 12 bytes plus 8 bytes
 * per candidate (0 when Vin * K is out of range). */
size_t ms3d_coords_expand_workspace_bytes(int Vin, int K);
int ms3d_coords_expand(const int *in_coords, int Vin, const int *offsets, int K, int *out_coords, int *n_out /*[host]*/,
                       void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
/* ms3d_coords_prune: the rows of coords [V, 4] with keep[i] != 0, in their relative order (flag -> scan -> emit).
 * src_row [n_kept] (capacity V): kept row -> source row, ascending; dst_row [V]: source row -> kept row or -1; out_coords
 * capacity V rows; *n_kept -> [host] (one sync).  V == 0: nothing is launched.  workspace: ms3d_coord_workspace_bytes(V).
 * The feature rows move with ms3d_gather_rows over src_row, their gradient with ms3d_scatter_rows. */
int ms3d_coords_prune(const int *coords, int V, const unsigned char *keep, int *out_coords, int *src_row, int *dst_row,
                      int *n_kept /*[host]*/, void *workspace, size_t workspace_bytes, ms3d_stream_t stream);

/* ms3d_coords_check: is a coordinate set that a CALLER supplied (the target of a layer's `coordinates=`) usable as an output
 * set, and if not, why.  *flags -> [host] (one sync), the OR of
 *   MS3D_COORDS_OUT_OF_RANGE  a row lies outside the packable range [-16384, 16384) or its batch index outside [0, 524288)
 *   MS3D_COORDS_OFF_LATTICE   a coordinate (x, y or z) is not a multiple of `lattice` (the tensor stride of the set; >= 1)
 *   MS3D_COORDS_REPEATED      a coordinate occurs twice (ms3d_kmap_invert needs distinct output rows); a row that does not fit
 *                             the key aliases another coordinate and is not asked, so read this bit with the first one down
 * The table of ms3d_sparse_quantize is built (clear, insert: 64-bit CAS on the key, atomicMin of the row) and one kernel, one
 * thread per row, tests floor(v / lattice) * lattice == v and "this row is the first of its slot"; the bits are ORed into one
 * device int, by the threads that do not see their bit up yet.  Returns 0 WHATEVER the flags say -- the caller names the reason;
 * MS3D_E_UNSUPPORTED is for bad arguments only (flags NULL, lattice < 1, V < 0, NULL coords / workspace with V > 0).  V == 0:
 * *flags = 0, nothing is launched.  workspace: ms3d_coord_workspace_bytes(V). */
#define MS3D_COORDS_OUT_OF_RANGE 1
#define MS3D_COORDS_OFF_LATTICE 2
#define MS3D_COORDS_REPEATED 4
int ms3d_coords_check(const int *coords, int V, int lattice, int *flags /*[host]*/, void *workspace, size_t workspace_bytes,
                      ms3d_stream_t stream);

/* ---- arithmetic across coordinate sets: union of sets, feature combine, broadcast of one row per batch index.
 * ms3d_coords_union: the distinct coordinates of N sets (1 <= N <= 16) of one tensor stride, handed over back to back as coords
 * [set_start[N], 4] with HOST offsets set_start [N + 1] (set_start[0] = 0, ascending; set i = rows set_start[i] ..
 * set_start[i + 1]).  Order: first occurrence in the concatenation -- all rows of set 0 in their order, then the rows of set 1
 * that set 0 lacks, and so on (the rule of ms3d_sparse_quantize / ms3d_downsample / ms3d_coords_expand; 64-bit CAS on the key,
 * atomicMin of the row, flag -> scan -> emit at rank; no sort, no float atomics, the same bytes on every run).
 *   out_coords [n_out, 4]   capacity set_start[N] rows
 *   out_row [set_start[N]]  input row of the concatenation -> union row
 *   in_row [N][n_out]       union row -> row of set i (counted from the set's first row) or -1; PACKED with the row length
 *                           n_out that the call returns, capacity N * set_start[N] ints; plain stores, one writer per cell
 *   *n_out -> [host]        one sync
 * A coordinate that repeats INSIDE one set (every slot keeps one bit per set; a row that finds its set's bit raised), a row outside the packable range
 * [-16384, 16384) / batch index outside [0, 524288), N outside 1..16, a NULL or descending set_start, or more than 2^30 - 1
 * rows: MS3D_E_UNSUPPORTED (repeats are never merged silently; the outputs are then not to be used).  An empty set is legal;
 * all sets empty: *n_out = 0 and nothing is launched.  workspace: ms3d_coords_union_workspace_bytes(set_start[N]) -- a table of
 * the next power of two >= 2 rows slots of 16 bytes (key, row, set bits: 32 .. 64 bytes per row) plus 12 bytes per row (0 when
 * out of range). */
size_t ms3d_coords_union_workspace_bytes(int total_rows);
int ms3d_coords_union(const int *coords, const int *set_start /*[host] N + 1*/, int n_sets, int *out_coords, int *out_row,
                      int *in_row, int *n_out /*[host]*/, void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
/* ms3d_union_combine (float32, any C; 16-byte row accesses when C % 4 == 0 and the rows are 16-byte aligned): out [n_out, C]
 * from the N feature arrays in_feats (HOST array of N device pointers; set i is [V_i, C]) gathered through in_row [N][n_out]
 * in ASCENDING input order.  op 0 sum (any N): out[o] = sum over the inputs present; op 1 subtract, op 2 multiply (N = 2).
 * A coordinate one operand lacks: the result is zero-filled, receives a at a's rows and is then set to fn(out, b) at b's rows
 * -- a - b gives -b where only b is, a * b gives a where only a is and 0 * b where only b is.  The in_row entries name rows of
 * the arrays as they are passed (the caller composes any row permutation of its own into them).
 * backward (operand `which`): a gather, din [V, C] with din[r] = dout[out_row[r]] -- negated for the second operand of
 * subtract; for multiply scaled by the other operand's row other[other_row[o]] (other_row = in_row[1 - which]), passed through
 * unscaled for operand 0 where the other is absent, zero for operand 1 where the other is absent (the derivative of 0 * b).
 * other / other_row may be NULL unless op == 2. */
int ms3d_union_combine(int op, const float *const *in_feats /*[host] N*/, int n_sets, const int *in_row, int n_out, int C,
                       float *out, ms3d_stream_t stream);
int ms3d_union_combine_backward(int op, int which, const float *dout, const int *out_row, int V, const float *other,
                                const int *other_row, int C, float *din, ms3d_stream_t stream);
/* ms3d_broadcast_forward: out[r] = x[r] (mode) g[grow[r]] for x [V, C], g [G, Cg], grow [V] = the row of g that carries the
 * voxel's batch index.  mode 0 add, 1 multiply (C == Cg, out [V, C]); 2 concatenate (out [V, C + Cg], x in front); 3 copy (out
 * [V, Cg]; x and C are not read).  grow[r] = -1 (no global row for that batch index): the voxel sees the zero vector -- the
 * caller's map says so, nothing is checked per call.  The gradient of x is the identity (add), a column slice (concatenate) or
 * this kernel with dout in place of x (multiply).
 * ms3d_broadcast_reduce: the gradient of g, dg [G, C] with dg[j] = sum over the rows r of g row j's batch of dout[r, col_off :
 * col_off + C] (times x[r] when x != NULL: multiply, never materialised).  dout has leading dimension ldd (a column slice of a
 * wider gradient is read in place).  The rows of a batch are order[seg_start[s] .. seg_start[s + 1]) (int64 rows, int32
 * offsets: CoordinateManager.batch_rows), s = seg_of_g[j] or -1 (dg[j] = 0).  Fixed order: the segment is cut into 64 slices
 * of ceil(len / 64) rows, a block sums one slice (each thread its rows in ascending order, the threads of a column in ascending
 * order), a second kernel adds the 64 partial sums in slice order.  workspace: ms3d_broadcast_reduce_workspace_bytes(G, C) = 64
 * G C floats.  G <= 65535. */
int ms3d_broadcast_forward(int mode, const float *x, const float *g, const int *grow, int V, int C, int Cg, float *out,
                           ms3d_stream_t stream);
size_t ms3d_broadcast_reduce_workspace_bytes(int G, int C);
int ms3d_broadcast_reduce(const float *dout, int ldd, int col_off, const float *x, int C, const long long *order,
                          const int *seg_start, const int *seg_of_g, int G, float *dg, void *workspace, size_t workspace_bytes,
                          ms3d_stream_t stream);

/* ---- pooling over a kernel map (float32, any C; 16-byte row accesses when C % 4 == 0).  mode: 0 max, 1 average, 2 sum.
 * forward: out[o] = reduce over the PRESENT inputs in[nbr[k][o]] in ascending k; max writes arg [Vout][C] = the winning k
 * (lowest k on ties; 255 and out = 0 for a row without input), average divides by the number of present inputs and writes
 * it to count [Vout].  arg / count may be NULL for the modes that do not use them.  K <= 254.
 * backward: a gather through the inverse table, din[i] = sum_k [o = nbr_inv[k][i] >= 0] dout[o] * (max: arg[o][c] == k |
 * average: 1 / count[o] | sum: 1).  No atomics: both directions are bit-reproducible. */
int ms3d_pool_forward(int mode, const float *in, const int *nbr, int Vout, int K, int C, float *out, unsigned char *arg,
                      int *count, ms3d_stream_t stream);
int ms3d_pool_backward(int mode, const float *dout, const int *nbr_inv, int Vin, int K, int C, const unsigned char *arg,
                       const int *count, float *din, ms3d_stream_t stream);

/* ---- channel-wise (depthwise) convolution over a kernel map (csrc/chconv.hip; float32, any C; 16-byte row accesses when
 * C % 4 == 0 and the rows are 16-byte aligned, scalar otherwise -- both give the same bits forward).  w [K][C], K <= 254.
 * forward: out[o][c] = (bias ? bias[c] : 0) + sum over the PRESENT inputs in ascending k of w[k][c] * in[nbr[k][o]][c].
 * backward-data is the same call: din = ms3d_chconv_forward(dout, w, NULL, nbr_inv, Vin, ...) through the inverse table
 * (nbr_inv[k][i] = the output row that input i feeds through offset k: the offset index is NOT mirrored).
 * backward-weight: dW[k][c] = sum_o in[nbr[k][o]][c] * dout[o][c] in two stages without atomics: one [K][C] partial per run
 * of ms3d_chconv_wgrad_rows_per_part() consecutive output rows (a constant of the library, independent of the device, so the
 * order of the sum is too), then the partials added in ascending part order.  partial_ws: ms3d_chconv_wgrad_ws_floats(Vout,
 * K, C) = ms3d_chconv_wgrad_parts(Vout) * K * C floats, parts = ceil(Vout / rows_per_part) (pure host arithmetic; 0 for
 * Vout <= 0).  The bias gradient is ms3d_column_sum(dout).
 * K < 1, K > 254 or C < 1: MS3D_E_UNSUPPORTED.  Vout <= 0: 0, nothing is launched (dW is not written).  Every direction is
 * bit-reproducible. */
int ms3d_chconv_forward(const float *in, const float *w, const float *bias, const int *nbr, int Vout, int K, int C, float *out,
                        ms3d_stream_t stream);
int ms3d_chconv_backward_weight(const float *in, const float *dout, const int *nbr, int Vout, int K, int C, float *partial_ws,
                                float *dW, ms3d_stream_t stream);
int ms3d_chconv_wgrad_rows_per_part(void);
int ms3d_chconv_wgrad_parts(int Vout);
size_t ms3d_chconv_wgrad_ws_floats(int Vout, int K, int C);

/* ---- local multi-head attention over a kernel map (csrc/kattn.hip; float32 throughout).  q [Vout][C], k / v [Vin][C] row-
 * contiguous, C = H * D (H heads of D channels); nbr [K][Vout] the forward table, nbr_inv [K][Vin] its inverse (int32, -1 =
 * none; the offset index is NOT mirrored, as in ms3d_chconv_forward's backward-data); rel_bias [K][H] or NULL; i = nbr[kk][o]:
 *   s[o][kk][h] = scale * sum_d q[o][hD+d] * k[i][hD+d] + rel_bias[kk][h]        over the PRESENT kk (i >= 0)
 *   p[o][kk][h] = exp(s - m[o][h]) / sum_kk' exp(s' - m[o][h]),  m = the maximum over the present kk (always subtracted)
 *   out[o][hD+d] = sum_kk p[o][kk][h] * v[i][hD+d];   lse[o][h] = m + log sum exp(s - m)
 * A row without a present input gives out = 0 and lse = 0 and contributes to no gradient.
 * forward: out [Vout][C] and lse [Vout][H], one online-softmax sweep over ascending kk; rows are read by index where they lie,
 * nothing of size [pairs, .] is written.
 * backward_q walks the forward table: p recomputed from lse, ds = p * (dout[o][h][:] . v[i][h][:] - sum_d dout * out), evaluated
 * as ds = p * (e - delta[o][h]) with e = sum_d dout[o][hD+d] * (v[i][hD+d] - out[o][hD+d]) and delta[o][h] = sum_kk p * e: the
 * difference is taken per channel before the sum, so a row whose weight sits on one input (out = that v) does not subtract
 * two nearly equal dot products, and delta -- zero for an exactly rounded out -- takes back what the float32 rounding of the
 * saved out costs; the ds of a row sum to zero.  delta [Vout][H] is written for backward_kv.
 * dq[o][h][:] = scale * sum_kk ds * k[i][h][:]; dbias[kk][h] = sum_o ds in two stages without atomics: one [K][H] partial per run of ms3d_kattn_rows_per_part() consecutive output rows (a constant of the
 * library, independent of the device, so the order of the sum is too), then the partials added in ascending part order.
 * partial_ws: ms3d_kattn_dbias_ws_floats(Vout, K, H) = ms3d_kattn_dbias_parts(Vout) * K * H floats, parts = ceil(Vout /
 * rows_per_part) (pure host arithmetic; 0 for Vout <= 0), read only when dbias != NULL.  dq and dbias may each be NULL
 * (skipped; both NULL: delta alone); dbias != NULL needs rel_bias and partial_ws.
 * backward_kv gathers through nbr_inv: for o = nbr_inv[kk][i] >= 0, dv[i][h][:] += p * dout[o][h][:] and dk[i][h][:] += scale *
 * ds * q[o][h][:], p and ds recomputed from q[o], k[i], v[i], rel_bias[kk][h], lse[o][h], the row out[o] and delta[o][h]; dk or
 * dv may be NULL (not both).
 * Every sum runs in one fixed order that depends on the shapes only; no atomics; the same bytes on every run, in all three.
 * 16-byte row accesses when D % 4 == 0 and every row pointer is 16-byte aligned, a scalar path otherwise; 64-bit offsets.
 * Limits: 1 <= K <= 254, H >= 1, 1 <= D <= 128; H * D is bounded only by int (H * D and K * H <= 2^31 - 1), far past the
 * H * D <= 1024 of practical layers.  Outside them, or a NULL pointer that would be read or written: MS3D_E_UNSUPPORTED; a short
 * workspace: MS3D_E_WORKSPACE; both decided on the host before any launch.  Vout <= 0 (Vin <= 0 in backward_kv) with a served
 * shape: 0, nothing is launched, no pointer is looked at (dbias is not written). */
int ms3d_kattn_forward(const float *q, const float *k, const float *v, const float *rel_bias, const int *nbr, int Vout, int K,
                       int H, int D, float scale, float *out, float *lse, ms3d_stream_t stream);
int ms3d_kattn_backward_q(const float *q, const float *k, const float *v, const float *rel_bias, const int *nbr,
                          const float *out, const float *lse, const float *dout, int Vout, int K, int H, int D, float scale,
                          float *dq, float *dbias, float *delta, float *partial_ws, size_t ws_floats, ms3d_stream_t stream);
int ms3d_kattn_backward_kv(const float *q, const float *k, const float *v, const float *rel_bias, const int *nbr_inv,
                           const float *out, const float *lse, const float *delta, const float *dout, int Vin, int K, int H,
                           int D, float scale, float *dk, float *dv, ms3d_stream_t stream);
int ms3d_kattn_rows_per_part(void);
int ms3d_kattn_dbias_parts(int Vout);
size_t ms3d_kattn_dbias_ws_floats(int Vout, int K, int H);

/* ---- per-sample query attention over voxel rows (csrc/qattn.hip; float32 throughout).  queries [B][Q][C], k / v [V][C] row-
 * contiguous in the order the rows are HELD, C = H * D (H heads of D channels).  The rows of sample b are
 * order[seg_start[b] .. seg_start[b + 1]) (order int64 [V], seg_start int32 [B + 1]: CoordinateManager.batch_rows); they are
 * read by index where they lie.  mask [V][Q] bytes or NULL, non-zero = may not attend, one mask for all heads, its rows in the
 * CALLER's order: the mask row of held row i is row_map[i] (int32 [V], the manager's held-to-caller index) or i when row_map
 * is NULL.  Over the rows i of sample b that the mask does not block for query q:
 *   s[b][q][i][h] = scale * sum_d queries[b][q][hD+d] * k[i][hD+d]
 *   p             = exp(s - m) / sum_i' exp(s' - m),  m = the maximum over those rows (always subtracted)
 *   out[b][q][hD+d] = sum_i p * v[i][hD+d];   lse[b][q][h] = m + log sum exp(s - m)
 * A (b, q) without an unblocked row gives out = 0 and lse = 0, contributes to no gradient and receives none.
 * Chunks: a segment is cut into runs of ms3d_qattn_rows_per_chunk() consecutive positions of `order` (a constant of the
 * library, independent of the device, so the order of every sum is too).  ms3d_qattn_chunks(seg_start, B): the number of
 * chunks, sum_b ceil(len_b / rows_per_chunk); ms3d_qattn_chunk_list fills chunk_seg [chunks] (the sample of every chunk) and
 * chunk_first [B + 1] (the first chunk of every sample; chunk_first[B] = chunks): sorted by sample, then by run.  Both are
 * pure HOST arithmetic over HOST arrays; the launches take DEVICE copies of chunk_seg and chunk_first.
 * forward: one workgroup per chunk and tile of (query, head) items does one online-softmax sweep over the chunk's rows in
 * ascending position and stores a partial (m, l, acc[D]) per item; a second kernel merges the partials of a sample in
 * ascending chunk order and writes out [B][Q][C] and lse [B][Q][H].  ws: ms3d_qattn_ws_floats(chunks, Q, H, D) =
 * chunks * Q * (H * D + 2 * H) floats, the only scratch; nothing of size [V][Q] is written.
 * backward_q: the same sweep with p = exp(s - lse) recomputed; ds = p * (e - delta[b][q][h]) with e = sum_d dout[b][q][hD+d] *
 * (v[i][hD+d] - out[b][q][hD+d]) -- the difference per channel before the sum, as in ms3d_kattn_backward_q -- and
 * delta[b][q][h] = sum_i p * e, the residual that the float32 rounding of the saved out leaves.  Per chunk sum p e k, sum p k
 * and sum p e are stored and added in ascending chunk order: dq[b][q][h][:] = scale * (sum p e k - delta * sum p k).  delta
 * [B][Q][H] is always written (backward_kv reads it); dq may be NULL (delta alone).  ws: ms3d_qattn_backward_ws_floats(chunks,
 * Q, H, D) = chunks * Q * (2 * H * D + H) floats.
 * backward_kv: one (row, head) item per voxel row loops over the Q queries of its sample seg_of_row[i] (int32 [V], the segment
 * of every held row: CoordinateManager.batch_segments) in ascending q: dv[i][h][:] = sum_q p * dout[b][q][h][:],
 * dk[i][h][:] = scale * sum_q ds * queries[b][q][h][:]; one writer per element, no scratch; dk or dv may be NULL (not both).
 * Every sum runs in one fixed order that depends on the shapes only; no atomics; the same bytes on every run, in all three.
 * 16-byte row accesses when D % 4 == 0 and every row pointer (ws included) is 16-byte aligned, a scalar path otherwise;
 * 64-bit offsets.
 * Limits: 1 <= D <= 128, H >= 1, H * D <= 1024, 0 <= Q <= 1024, 0 <= B <= 65535, V >= 0, chunks >= 0.  Outside them, or a NULL
 * pointer that would be read or written: MS3D_E_UNSUPPORTED; a short workspace: MS3D_E_WORKSPACE; both decided on the host
 * before any launch.  V == 0, B == 0 or Q == 0 with a served shape: 0, nothing is launched, no pointer is looked at.  The
 * index arrays are trusted: order and row_map name rows in [0, V), seg_of_row and chunk_seg samples in [0, B). */
int ms3d_qattn_rows_per_chunk(void);
long ms3d_qattn_chunks(const int *seg_start /*HOST [B + 1]*/, int B);
int ms3d_qattn_chunk_list(const int *seg_start /*HOST [B + 1]*/, int B, int *chunk_seg /*HOST [chunks]*/,
                          int *chunk_first /*HOST [B + 1]*/);
size_t ms3d_qattn_ws_floats(long chunks, int Q, int H, int D);
size_t ms3d_qattn_backward_ws_floats(long chunks, int Q, int H, int D);
int ms3d_qattn_forward(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                       const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first, long V, int B,
                       int chunks, int Q, int H, int D, float scale, float *out, float *lse, float *ws, size_t ws_floats,
                       ms3d_stream_t stream);
int ms3d_qattn_backward_q(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                          const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first,
                          const float *out, const float *lse, const float *dout, long V, int B, int chunks, int Q, int H, int D,
                          float scale, float *dq, float *delta, float *ws, size_t ws_floats, ms3d_stream_t stream);
int ms3d_qattn_backward_kv(const float *queries, const float *k, const float *v, const unsigned char *mask, const int *row_map,
                           const int *seg_of_row, const float *out, const float *lse, const float *delta, const float *dout,
                           long V, int B, int Q, int H, int D, float scale, float *dk, float *dv, ms3d_stream_t stream);

/* ---- per-sample voxel attention: every voxel row attends to the queries of its own sample (csrc/vattn.hip; float32
 * throughout) -- the reverse direction of the block above.  x [V][C] row-contiguous in the order the rows are HELD, keys /
 * values [B][Q][C], C = H * D.  The sample of held row i is seg_of_row[i] (int32 [V]: CoordinateManager.batch_segments); mask
 * [V][Q] bytes or NULL is the mask of ms3d_qattn_forward, the same object: non-zero = may not attend, one mask for all heads,
 * its rows in the CALLER's order, the mask row of held row i is row_map[i] or i when row_map is NULL.  Over the queries q of
 * sample b = seg_of_row[i] that the mask does not block for row i:
 *   s[i][q][h] = scale * sum_d x[i][hD+d] * keys[b][q][hD+d]
 *   p          = exp(s - m) / sum_q' exp(s' - m),  m = the maximum over those queries (always subtracted)
 *   out[i][hD+d] = sum_q p * values[b][q][hD+d];   lse[i][h] = m + log sum exp(s - m)
 * A row whose queries are all blocked gives out = 0 and lse = 0, contributes to no gradient and receives none.
 * forward: one (held row, head) item per group of lanes loops over the Q queries in ascending q, four at a time, one
 * online-softmax sweep; writes out [V][C] and lse [V][H]; no scratch.
 * backward_x: the same sweep with p = exp(s - lse) recomputed; ds = p * (e - delta[i][h]) with e = sum_d dout[i][hD+d] *
 * (values[b][q][hD+d] - out[i][hD+d]) -- the difference per channel before the sum, as in ms3d_kattn_backward_q -- and
 * delta[i][h] = sum_q p * e, complete when the row's sweep ends: dx[i][h][:] = scale * (sum p e keys - delta * sum p keys).
 * delta [V][H] is always written (backward_kv reads it); dx may be NULL (delta alone).  No scratch.
 * backward_kv: dvalues[b][q][h][:] = sum_i p * dout[i][h][:], dkeys[b][q][h][:] = scale * sum_i ds * x[i][h][:] over the rows i
 * of sample b that the mask does not block for q.  The rows of sample b are order[seg_start[b] .. seg_start[b + 1]) cut into
 * the chunks of ms3d_qattn_chunk_list (the SAME chunk list, ms3d_qattn_rows_per_chunk() positions each): one workgroup per
 * chunk and tile of (query, head) items walks the chunk's rows in ascending position and stores one partial of each sum; a
 * second kernel adds the partials of a sample in ascending chunk order and writes EVERY element of dkeys / dvalues [B][Q][C]
 * (zero for a (b, q) that no row may attend to).  ws: ms3d_vattn_backward_kv_ws_floats(chunks, Q, H, D) = chunks * Q * 2 * H * D
 * floats (0 for empty shapes), the only scratch; dkeys or dvalues may be NULL (not both).
 * Every sum runs in one fixed order that depends on the shapes only; no atomics; the same bytes on every run, in all three.
 * 16-byte row accesses when D % 4 == 0 and every row pointer (ws included) is 16-byte aligned, a scalar path otherwise;
 * 64-bit offsets.
 * Limits: 1 <= D <= 128, H >= 1, H * D <= 1024, 0 <= Q <= 1024, 0 <= B <= 65535, V >= 0, chunks >= 0; V * H row items in at most
 * 2^31 - 1 workgroups.  Outside them, or a NULL pointer that would be read or written: MS3D_E_UNSUPPORTED; a short workspace:
 * MS3D_E_WORKSPACE; both decided on the host before any launch.  V == 0, B == 0 or Q == 0 with a served shape: 0, nothing is
 * launched, no pointer is looked at.  The index arrays are trusted, as in the block above. */
size_t ms3d_vattn_backward_kv_ws_floats(long chunks, int Q, int H, int D);
int ms3d_vattn_forward(const float *x, const float *keys, const float *values, const unsigned char *mask, const int *row_map,
                       const int *seg_of_row, long V, int B, int Q, int H, int D, float scale, float *out, float *lse,
                       ms3d_stream_t stream);
int ms3d_vattn_backward_x(const float *x, const float *keys, const float *values, const unsigned char *mask, const int *row_map,
                          const int *seg_of_row, const float *out, const float *lse, const float *dout, long V, int B, int Q,
                          int H, int D, float scale, float *dx, float *delta, ms3d_stream_t stream);
int ms3d_vattn_backward_kv(const float *x, const float *keys, const float *values, const unsigned char *mask, const int *row_map,
                           const long long *order, const int *seg_start, const int *chunk_seg, const int *chunk_first,
                           const float *out, const float *lse, const float *delta, const float *dout, long V, int B, int chunks,
                           int Q, int H, int D, float scale, float *dkeys, float *dvalues, float *ws, size_t ws_floats,
                           ms3d_stream_t stream);

/* ---- farthest point sampling per sample (csrc/fps.hip): M rows of every sample, the seeds of the queries the two blocks above
 * take.  The rows of sample b are order[seg_start[b] .. seg_start[b + 1]) (order int64 [V], seg_start int32 [B + 1]:
 * CoordinateManager.batch_rows, or a stable sort of a field's batch column), read by index where they lie in coords [V][4] int32
 * (batch, x, y, z) / points [N][4] float32 (batch, x, y, z), N = V; the batch column is not looked at.  The CALLER's row of held
 * row i is row_map[i] (int32 [V], the manager's held-to-caller index) or i when row_map is NULL.  out [B][M] int64 holds caller
 * rows:
 *   out[b][0] = start_held[b] (int64 [B], a HELD row of sample b), or the sample's lowest caller row when start_held is NULL
 *   out[b][j] = the row of sample b whose distance to the nearest of out[b][0 .. j-1] is largest; among equal distances the
 *               lowest caller row; rows already picked have distance 0 and take part like any other row
 * so the result is a pure function of the coordinate set and does not depend on how the rows are held.  M > len_b is served by
 * the same rule (once every distance is 0 the lowest caller row repeats); the Python layer refuses it.
 * Distances.  i32: the exact integer dx^2 + dy^2 + dz^2 in unsigned 32-bit arithmetic; the coordinates are trusted to lie in the
 * packable range [-16384, 16384), where it reaches 3 * 32767^2 = 3 221 028 867 (above 2^31, below 2^32).  f32: d = (dx*dx + dy*dy)
 * + dz*dz with dx = p.x - c.x, every operation rounded to float32 on its own, never contracted into an FMA; the running minimum
 * is fminf on finite values; finite coordinates are a precondition and are not checked; duplicate points are legal.
 * One launch, one workgroup per sample, which loops over its own segment; no workgroup waits for another (no spin, no grid
 * barrier, no atomics), every loop is counted: M * ceil(len_b / rows per step) steps.  A thread keeps its best row as one 64-bit
 * key, (distance bits << 32) | ~caller row, reduced per wave by shuffles and across waves through LDS; two workgroup barriers a
 * pick.  A sample of at most ms3d_fps_resident_rows() rows is held in registers for the whole loop (nothing is read from global
 * memory after the first gather); a larger one is gathered once, in segment order, into ws (i32: 16 B a row, f32: 20 B a row)
 * and swept with 16-byte accesses every pick.  ws: ms3d_fps_ws_bytes(V, B) bytes, 16-byte aligned, never assumed zero; the same
 * size serves both entry points; it grows with V and with B.
 * V < 0, B < 0, B > 65535, M < 1: MS3D_E_UNSUPPORTED.  V == 0 or B == 0 otherwise: 0, nothing is launched, no pointer is looked
 * at.  Then a NULL coords / points, order, seg_start, out or ws, or a ws that is not 16-byte aligned: MS3D_E_UNSUPPORTED; a short
 * workspace: MS3D_E_WORKSPACE; all decided on the host before the launch.  The index arrays are trusted to name what they
 * should; an order entry outside [0, V) and a seg_start outside [0, V] are clamped, a start_held outside its sample is ignored
 * (lowest caller row), so no index is followed outside its array. */
int ms3d_fps_resident_rows(void);
size_t ms3d_fps_ws_bytes(long V, int B);
int ms3d_fps_i32(const int *coords /*[V][4] as held*/, const long long *order /*[V]*/, const int *seg_start /*[B + 1]*/,
                 const int *row_map /*[V] held -> caller, or NULL*/, const long long *start_held /*[B] or NULL*/, int V, int B,
                 int M, long long *out /*[B][M] caller rows*/, void *ws, size_t ws_bytes, ms3d_stream_t stream);
int ms3d_fps_f32(const float *points /*[N][4], N = V*/, const long long *order /*[V]*/, const int *seg_start /*[B + 1]*/,
                 const int *row_map /*[V] held -> caller, or NULL*/, const long long *start_held /*[B] or NULL*/, int V, int B,
                 int M, long long *out /*[B][M] caller rows*/, void *ws, size_t ws_bytes, ms3d_stream_t stream);

/* ---- k nearest neighbours per sample (csrc/knn.hip): what follows the sampling above -- grouping rows around the picks,
 * carrying features of the picks back to every row, kNN graphs.  The support set is given exactly as to ms3d_fps_*: coords
 * [V][4] int32 / points [V][4] float32 (batch, x, y, z) as held, the rows of sample b are order[seg_start[b] .. seg_start[b + 1]),
 * the CALLER's row of held row i is row_map[i], or i when row_map is NULL.  The queries come packed: 32-bit words [NQ][4] =
 * (segment, x, y, z) -- int32 coordinates for i32, the bits of float32 points for f32 -- grouped by segment, the queries of
 * segment b at q_start[b] .. q_start[b + 1] (int32 [B + 1]); max_queries: the largest number of queries any segment has (host
 * arithmetic on the segment lengths; it sizes the grid, queries beyond it in a segment are not served).
 *   out_idx[q][0 .. k) = the caller rows of the k rows of the query's segment with the smallest keys (distance bits << 32) | caller
 *                        row, in ascending key order: nearer first, among equal distances the lower caller row; the query's own
 *                        row, if it is one of the set, is found like any other (first, at distance 0)
 *   out_d2[q][0 .. k)  = their distances (i32: unsigned 32-bit words; f32: float32)
 * A row qualifies when its distance is <= max_d2 (the boundary included; max_d2 < 0: no cap; i32 caps above 2^32 - 1 are no
 * cap).  Slots no row qualifies for -- a segment of fewer than k rows, a cap, a query whose segment word is not the segment it
 * is filed under -- hold -1 and the distance word of "none" (i32: all ones; f32: +inf), after every qualifying slot.  Real keys
 * are distinct, so the result is a pure function of the coordinates and does not depend on how the rows are held.
 * Distances are ms3d_fps_*'s: i32 the exact integer dx^2 + dy^2 + dz^2 in unsigned 32-bit arithmetic over the packable range
 * [-16384, 16384) of BOTH sets (up to 3 221 028 867); f32 d = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x, every operation rounded
 * to float32 on its own, never contracted into an FMA; finite coordinates are a precondition and are not checked.
 * Two launches: the support set is packed into ws in segment order, 16 B a row (every word read is written first: ws is never
 * assumed zero; `order` is clamped there); then workgroup (g, b) of ms3d_knn_queries_per_group() threads takes that many queries
 * of segment b, a thread a query, and streams the segment through LDS in tiles of ms3d_knn_rows_per_tile() rows; a thread's
 * list of its k smallest keys lives in LDS and is put in order at the end.  No atomics, no spin, no grid barrier; every loop is counted.  ws: ms3d_knn_ws_bytes(V)
 * bytes, 16-byte aligned.
 * V < 0, B < 0, B > 65535, NQ < 0, max_queries < 0, k < 1, k > ms3d_knn_max_k(): MS3D_E_UNSUPPORTED.  Otherwise V == 0, B == 0,
 * NQ == 0 or max_queries == 0: 0, nothing is launched, no pointer is looked at.  Then a NULL coords / points, order, seg_start,
 * queries, q_start, out_idx, out_d2 or ws, or a ws that is not 16-byte aligned: MS3D_E_UNSUPPORTED; a short workspace:
 * MS3D_E_WORKSPACE; all decided on the host before a launch.  seg_start and q_start values are clamped to their arrays. */
int ms3d_knn_max_k(void);
int ms3d_knn_queries_per_group(void);
int ms3d_knn_rows_per_tile(void);
size_t ms3d_knn_ws_bytes(long V);
int ms3d_knn_i32(const int *coords /*[V][4] as held*/, const long long *order /*[V]*/, const int *seg_start /*[B + 1]*/,
                 const int *row_map /*[V] held -> caller, or NULL*/, int V, int B, const int *queries /*[NQ][4]*/,
                 const int *q_start /*[B + 1]*/, int NQ, int max_queries, int k, long long max_d2 /*< 0: none*/,
                 long long *out_idx /*[NQ][k] caller rows*/, unsigned *out_d2 /*[NQ][k]*/, void *ws, size_t ws_bytes,
                 ms3d_stream_t stream);
int ms3d_knn_f32(const float *points /*[V][4] as held*/, const long long *order /*[V]*/, const int *seg_start /*[B + 1]*/,
                 const int *row_map /*[V] held -> caller, or NULL*/, int V, int B, const int *queries /*[NQ][4] words*/,
                 const int *q_start /*[B + 1]*/, int NQ, int max_queries, int k, float max_d2 /*< 0: none*/,
                 long long *out_idx /*[NQ][k] caller rows*/, float *out_d2 /*[NQ][k]*/, void *ws, size_t ws_bytes,
                 ms3d_stream_t stream);

/* ---- instance normalisation: per batch index (segment) and channel (csrc/inorm.hip; float32 rows and parameters, any C >= 1;
 * every sum, the statistics mean / invstd (DOUBLE [B, C]) and the arithmetic of the row passes are float64, rounded once at the
 * store: with few rows in a segment dx is a difference of nearly equal terms that float32 statistics cannot resolve; a lane takes four
 * channels of a row -- one 16-byte access when C % 4 == 0 and every pointer is 16-byte aligned, four guarded 4-byte accesses
 * otherwise; both routes run the same arithmetic in the same order and give the same bits).  The rows of segment s are
 * order[seg_start[s] .. seg_start[s + 1]) (int64 rows, int32 offsets [B + 1]: CoordinateManager.batch_rows, one segment per
 * batch index present), n_s of them; seg_of_row int32 [V] names the segment of every held row (CoordinateManager.
 * batch_segments).  Rows are read and written where they lie: no permuted copy of x is made.
 * forward:  mean[s][c] = (1/n_s) sum_r x[r][c];  var[s][c] = (1/n_s) sum_r (x[r][c] - mean[s][c])^2 (biased);
 *           invstd[s][c] = 1 / sqrt(var[s][c] + eps);  y[r][c] = (x[r][c] - mean[s][c]) * invstd[s][c] * weight[c] + bias[c].
 * backward: xhat = (x - mean) * invstd recomputed from the saved x, mean, invstd;  S1[s][c] = sum_r dy[r][c];
 *           S2[s][c] = sum_r dy[r][c] * xhat[r][c];  dx[r][c] = weight[c] * invstd[s][c] * (dy[r][c] - S1[s][c] / n_s -
 *           xhat[r][c] * S2[s][c] / n_s);  dweight[c] = sum_s S2[s][c], dbias[c] = sum_s S1[s][c] in ascending s.
 * weight / bias may be NULL (1 / 0); dx, dweight, dbias may each be NULL (skipped; all three NULL: nothing is launched).
 * Order of summation (the scheme of ms3d_broadcast_reduce): a segment is cut into ms3d_inorm_slices() slices of ceil(n_s /
 * slices) consecutive positions of `order`; a workgroup sums one slice, each thread its rows in ascending order, the threads
 * of a column in ascending order; a second kernel merges the slice partials in ascending slice order, skipping empty
 * slices.  The slice count is a constant of the library, not of the device: no float atomics, no dependence on the CU count,
 * the same bytes on every run.  The statistics are NOT E[x^2] - E[x]^2 of the raw values: a slice sums (x - K) and (x - K)^2
 * with K = its first row and hands on (n, mean, M2), the merge is Chan's (delta = mean_b - mean_a; mean += delta n_b / n;
 * M2 += M2_b + delta^2 n_a n_b / n).  A segment of one row gives y = bias and dx = 0 exactly.
 * workspace: ms3d_inorm_workspace_bytes(B, C) = 8 * 2 * B * (slices + 1) * C bytes (doubles) for either direction (pure host
 * arithmetic; 0 for B <= 0 or C < 1); less: MS3D_E_WORKSPACE.  C < 1 or B > 65535: MS3D_E_UNSUPPORTED, as is a NULL pointer
 * that would be read or written.  V <= 0 or B <= 0: 0, nothing is launched (dweight / dbias are then not written). */
int ms3d_inorm_slices(void);
size_t ms3d_inorm_workspace_bytes(int B, int C);
int ms3d_inorm_forward(const float *x, long V, int C, const long long *order, const int *seg_start, int B,
                       const int *seg_of_row, float eps, const float *weight, const float *bias, double *mean /*[B, C]*/,
                       double *invstd /*[B, C]*/, float *y, void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
int ms3d_inorm_backward(const float *dy, const float *x, long V, int C, const long long *order, const int *seg_start, int B,
                        const int *seg_of_row, const double *mean, const double *invstd, const float *weight, float *dx,
                        float *dweight /*[C]*/, float *dbias /*[C]*/, void *workspace, size_t workspace_bytes,
                        ms3d_stream_t stream);

/* ---- points <-> voxels: TensorField quantisation and trilinear interpolation (csrc/field.hip; the map: csrc/coords.hip).
 * float32, any C; 16-byte row accesses when C % 4 == 0 and the rows are 16-byte aligned.  Every direction is a gather with one
 * writer per output element: no float atomics, the same bytes on every run.  Contracts shared by the five entry points,
 * decided on the host: an unknown mode returns MS3D_E_UNSUPPORTED; zero output rows return 0 and launch nothing; a NULL pointer
 * that would be read or written returns MS3D_E_UNSUPPORTED; row counts beyond 2^31 - 1 (points of a map: 8 N entries, so
 * N <= (2^31 - 1) / 8) return MS3D_E_UNSUPPORTED.  Nothing is allocated inside a call.
 *
 * ms3d_interp_map: the eight corners of every query point in the set coords [Vin, 4] (distinct rows of tensor stride ts, a
 * positive power of two -- anything else returns MS3D_E_UNSUPPORTED).  points: float [N, 4] (batch index, x, y, z in voxel
 * units of stride 1), 16-byte aligned; the batch column is truncated to an integer.  Per axis q = p / ts, f = floor(q),
 * r = q - f; corner j = bx + 2 by + 4 bz (x fastest) is the voxel (f + b) * ts with weight (wx * wy) * wz, w = b ? r : 1 - r,
 * each operation rounded to float32.  rows int32 [8][N] = the row of coords at the corner or -1 (absent; a corner or batch
 * index outside the packable key range; a point with a non-finite entry), weights float [8][N] (0 for a point with a
 * non-finite entry; otherwise the weight whether the corner is present or not).  N == 0 or Vin == 0 launches nothing and
 * returns 0 (with Vin == 0 the caller's tables are left as they are).  workspace: ms3d_coord_workspace_bytes(Vin).
 *
 * ms3d_interp_forward: out[n] = sum_j weights[j][n] * x[rows[j][n]] over the corners with rows >= 0, ascending j, one fmaf per
 * corner and element starting from 0 -- a point on a voxel's own coordinate returns that row bit for bit, a point without any
 * corner exact zeros.
 * ms3d_interp_backward: din [Vin, C], din[v] = sum over the entries of row v of weight * dout[point], one fmaf each.  An entry
 * is e = 8 * point + corner; entry_sorted [number of entries with rows >= 0] holds them grouped by row -- row v owns
 * entry_sorted[seg_start[v] .. seg_start[v + 1]) (seg_start int32 [Vin + 1]) -- in ascending e inside a row, which is ascending
 * point because a point names a row at most once (a stable sort of the point-major table by row, built once per map by the
 * caller).  Entries whose point is outside [0, N) are skipped.
 *
 * ms3d_field_reduce: voxel features from point features.  mode 0 average, 1 sum, 2 max.  The points of voxel v are
 * order[seg_start[v] .. seg_start[v + 1]) (int64 point indices, int32 offsets [V + 1]: a stable sort of the point -> voxel
 * map), walked in that -- ascending -- order: the sum is a chain of float32 additions from 0, the average that sum divided
 * once by float(count), the maximum takes the first point and then every strictly greater one (lowest point index on ties)
 * and writes the winning point to arg int32 [V][C] (read and written for max only; NULL otherwise).
 * ms3d_field_reduce_backward: dfeat[n] = dvox[v] / float(count of v) (average) | dvox[v] (sum) | dvox[v] where arg[v][c] == n
 * else 0 (max), v = inverse[n] (int32 [N]); seg_start is read for average only, arg for max only. */
int ms3d_interp_map(const int *coords, int Vin, const float *points, long N, int tensor_stride, int *rows, float *weights,
                    void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
int ms3d_interp_forward(const float *x, const int *rows, const float *weights, long N, int C, float *out, ms3d_stream_t stream);
int ms3d_interp_backward(const float *dout, const float *weights, const long long *entry_sorted, const int *seg_start, long Vin,
                         long N, int C, float *din, ms3d_stream_t stream);
int ms3d_field_reduce(int mode, const float *feats, const long long *order, const int *seg_start, long V, int C, float *out,
                      int *arg, ms3d_stream_t stream);
int ms3d_field_reduce_backward(int mode, const float *dvox, const int *inverse, const int *seg_start, const int *arg, long N,
                               int C, float *dfeat, ms3d_stream_t stream);

/* ---- pooling and weighted sums over a neighbour index, with gradients (csrc/neighbor.hip): what a kNN index is used for --
 * max over the k neighbours of a pick, inverse-distance interpolation of M picks onto all rows, scalar attention over a kNN
 * graph.  float32, any C; the row layout and the contracts of the field.hip block above: every direction is a gather with one
 * writer per output element, no float atomics, the same bytes on every run; an unknown mode, a NULL pointer that would be read
 * or written, k < 1, k > 254 (a slot number fits a byte with 255 free), C < 1, V or N beyond 2^31 - 1 or N * k beyond 2^31 - 1
 * (an entry number fits an int32) return MS3D_E_UNSUPPORTED; zero output rows return 0 and launch nothing; nothing is allocated
 * inside a call.  x [V][C]: the support rows as held.  idx int64 [N][k]: per query k rows of x, or < 0 = no neighbour, in any
 * slot; a negative index is skipped.  Values >= V are a precondition (the caller's record validated them; the kernels do not
 * re-check).  Modes: 0 max, 1 avg, 2 sum, 3 weighted (backward only).
 *
 * ms3d_nbr_pool_forward (modes 0 .. 2), over the slots with idx >= 0 in ascending slot:
 *   sum  the chain of float32 additions from 0 (ms3d_field_reduce's rule);  avg  that sum divided once by float(valid slots), a
 *   query without one exact zeros;  max  per channel the first valid slot, then every strictly greater one: the lowest slot wins
 *   ties, a NaN wins only from the first slot; the winning slot goes to arg uint8 [N][C] (read and written for max only), a
 *   query without a valid slot stores 255 and yields zeros.
 * ms3d_nbr_wsum_forward: out[n] = sum_j w[n][j] * x[idx[n][j]] over the valid slots, ascending j, one fmaf per slot and element
 *   from 0 (ms3d_interp_forward's rule); the weight of an invalid slot is never read; a query whose single neighbour has weight 1
 *   returns that row bit for bit.
 * ms3d_nbr_backward: dx [V][C], written in full (no memset in front), dx[v] = the sum over the entries e = n * k + j of row v in
 *   ascending e of  dout[n][c] where arg[n][c] == j (max) | dout[n] / float(valid[n]) (avg, valid int32 [N]: the valid slots of
 *   every query) | dout[n] (sum) | w[e] * dout[n], one fmaf (weighted).  entry_sorted int64 [E] holds the entries with idx >= 0
 *   grouped by row -- row v owns entry_sorted[seg_start[v] .. seg_start[v + 1]), seg_start int32 [V + 1] -- and a row is summed
 *   in the order of its list: ascending e (one stable sort of the index by row, built once per map by the caller; where the
 *   caller numbers the queries otherwise than they are held, ascending in ITS numbering, so that the sums do not depend on how
 *   the rows are held); an entry outside [0, N * k) is skipped.  A row
 *   of more than T = ms3d_nbr_chunk_entries() entries is cut into ceil(entries / T) chunks of T consecutive entries; each chunk
 *   is summed the same way by its own thread group into a partial in ws, and the row adds its partials from 0 in chunk order.
 *   chunk_start int32 [V + 1]: chunk_start[v + 1] - chunk_start[v] = the chunks of row v when it has more than one, else 0
 *   (chunk_start[0] = 0); n_chunks = chunk_start[V].  A row of at most T entries is the plain chain.  ws: ms3d_nbr_ws_bytes(
 *   n_chunks, C) = 4 * n_chunks * C bytes, 16-byte aligned, never assumed zero (0 and NULL are fine without long rows); less:
 *   MS3D_E_WORKSPACE.  w, arg, valid: read for their mode only, NULL otherwise.  At most two launches.
 * ms3d_nbr_wsum_backward_w: dw[n][j] = <dout[n], x[idx[n][j]]>, 0 for an invalid slot.  One wave per query: lane l takes the
 *   channels l, l + 64, ... in ascending order (one fmaf each, from 0), then the 64 lane sums are folded by xor shuffles over
 *   32, 16, .. 1 -- an order fixed by C alone.
 * No atomics, no spin, no grid barrier; every loop is counted. */
int ms3d_nbr_chunk_entries(void);
size_t ms3d_nbr_ws_bytes(long n_chunks, int C);
int ms3d_nbr_pool_forward(int mode, const float *x, long V, const long long *idx /*[N][k] held rows or < 0*/, long N, int k, int C,
                          float *out, unsigned char *arg /*[N][C], max only*/, ms3d_stream_t stream);
int ms3d_nbr_wsum_forward(const float *x, long V, const long long *idx, const float *w /*[N][k]*/, long N, int k, int C,
                          float *out, ms3d_stream_t stream);
int ms3d_nbr_backward(int mode, const float *dout, const float *w, const unsigned char *arg, const int *valid,
                      const long long *entry_sorted, const int *seg_start, const int *chunk_start, long n_chunks, long V, long N,
                      int k, int C, float *dx, void *ws, size_t ws_bytes, ms3d_stream_t stream);
int ms3d_nbr_wsum_backward_w(const float *dout, const float *x, const long long *idx, long N, int k, int C, float *dw,
                             ms3d_stream_t stream);

/* ---- multi-head softmax attention over a neighbour index, with gradients (csrc/nattn.hip, on csrc/attn_core.h): the local
 * self-attention of a point or voxel transformer over its k nearest rows, the cross-attention of picks over their groups.
 * float32; q [N][C] on the target, k / v [V][C] the support rows as held, C = H * D, D <= 128; idx int64 [N][k] as above; bias
 * float32 [N][k][H] (one additive term per entry and head) or NULL:
 *   out[n][h][:] = sum_j softmax_j(scale * <q[n][h], k[i][h]> + bias[n][j][h]) v[i][h][:],  i = idx[n][j],
 * over the slots with 0 <= i < V in ascending slot; the maximum is always subtracted before exp; lse [N][H] = m + log sum
 * exp(s - m).  A query without a valid slot gives out = 0 and lse = 0; a query with one valid slot returns that v row bit for
 * bit.  The bias of an invalid slot is never read.  A value of idx that is < 0 or >= V switches the gather off: nothing is read
 * outside [0, V) in any pass.  Every direction is a gather with one writer per element: no atomics of any kind, no spin, no grid
 * barrier, every loop counted, every sum in an order fixed by the shapes and the index alone; nothing is allocated inside a
 * call and nothing of size N * k * C exists.
 * ms3d_nattn_backward_q: the same sweep with p recomputed from lse; writes delta [N][H] (always; the residual the kv pass
 *   subtracts, csrc/attn_core.h), dq = scale * (sum ds' k - delta * sum p k) (or NULL) and dbias [N][k][H] (or NULL):
 *   p * (e - delta) for a valid slot, 0.0f for an invalid one, every element stored by exactly one thread.  The bits of p and e of
 *   a slot wait in LDS until delta is known; the workgroup is sized from k alone so that the stash stays within 64 KiB.
 * ms3d_nattn_backward_kv: a gather on the support side: row i walks entry_sorted[seg_start[i] .. seg_start[i + 1]) (the table of
 *   ms3d_nbr_backward: entries e = n * k + j grouped by row, in the order the caller laid down) with p = exp(s - lse[n]),
 *   dv += p dout[n], dk += p (e_val - delta[n]) q[n], dk scaled once at the store; an entry outside [0, N * k) is skipped; a row no
 *   entry names stores exact zeros (no memset in front).  One of dk, dv may be NULL.  A row of more than T =
 *   ms3d_nbr_chunk_entries() entries uses chunk_start / n_chunks as ms3d_nbr_backward does: each chunk is summed from 0 into a
 *   partial (a dk row and a dv row) in ws, the row adds its partials from 0 in ascending chunk order; at most two launches.
 *   ws: ms3d_nattn_ws_bytes(n_chunks, C) = 8 * n_chunks * C bytes, 16-byte aligned, never assumed zero; less: MS3D_E_WORKSPACE,
 *   NULL or misaligned with n_chunks > 0: MS3D_E_UNSUPPORTED.
 * Checks, in this order: k < 1, k > 254, H < 1, D < 1, D > 128, H * D or k * H or N * k beyond 2^31 - 1, V or N negative or
 * beyond 2^31 - 1: MS3D_E_UNSUPPORTED; then N == 0 or V == 0: 0, nothing is launched and no pointer is looked at; then a NULL
 * pointer that would be read or written: MS3D_E_UNSUPPORTED; a grid beyond 2^31 - 1 blocks: MS3D_E_UNSUPPORTED.  The 16-byte
 * route is taken when D % 4 == 0 and every row pointer is 16-byte aligned, else the scalar one (two rounds for D > 64). */
size_t ms3d_nattn_ws_bytes(long n_chunks, int C);
int ms3d_nattn_forward(const float *q, const float *k, const float *v, const float *bias /*[N][k][H] or NULL*/,
                       const long long *idx /*[N][k] held rows or < 0*/, long V, long N, int k_slots, int H, int D, float scale,
                       float *out, float *lse /*[N][H]*/, ms3d_stream_t stream);
int ms3d_nattn_backward_q(const float *q, const float *k, const float *v, const float *bias, const long long *idx,
                          const float *out, const float *lse, const float *dout, long V, long N, int k_slots, int H, int D,
                          float scale, float *dq /*or NULL*/, float *dbias /*[N][k][H] or NULL*/, float *delta /*[N][H], always*/,
                          ms3d_stream_t stream);
int ms3d_nattn_backward_kv(const float *q, const float *k, const float *v, const float *bias, const float *out, const float *lse,
                           const float *delta, const float *dout, const long long *entry_sorted, const int *seg_start,
                           const int *chunk_start, long n_chunks, long V, long N, int k_slots, int H, int D, float scale,
                           float *dk, float *dv /*one may be NULL*/, void *ws, size_t ws_bytes, ms3d_stream_t stream);

/* Pair list = tile-compacted form of an offset-major table, built once per table and shared by every convolution of
 * the level (forward, backward-data, backward-weight).  Output rows are cut into tiles of 64; per tile and offset the
 * valid (input row, output row) pairs are stored contiguously, padded to a multiple of 16 ("batch" = one MFMA group).
 *   tile_start[header_ints] tiles + 1 batch offsets (exclusive scan; last = number of batches), then the schedule of
 *                           the kernels that walk the list: part_start[257] cuts the tiles into 256 parts of near-equal
 *                           batch count (tile t is in part floor(256 * tile_start[t] / batches)); then, 16-byte aligned,
 *                           the pick list int4[tiles] = (tile, first batch, end batch, 0): the tiles of each part by
 *                           descending batch count (stable, per run of 64 tiles)
 *   entries[2 * 16 * batches]  int2 per pair: (input row, (k << 8) | output row inside the tile); pad = (0, k<<8 | 64)
 * capacity() is the worst case in entries (allocate 8 bytes each); only the used prefix is ever touched. */
int ms3d_kmap_pairlist_tiles(int Vout);
int ms3d_kmap_pairlist_header_ints(int Vout);
size_t ms3d_kmap_pairlist_capacity(int K, int Vout);
int ms3d_kmap_pairlist_build(const int *nbr, int K, int Vout, int *tile_start, int *entries, void *workspace,
                             size_t workspace_bytes /* >= ms3d_coord_workspace_bytes(1) */, ms3d_stream_t stream);
/* The same list with tiles of rows_per_tile = 64 (above) or 128 output rows: the convolution kernel for layers with more
 * than 32 channels on a side reads its weights from L2 once per run of batches with the same offset, and a 128-row tile
 * has ~3 batches per offset where a 64-row tile has ~1.5 (and pads 2 % of its slots instead of 25 %). */
int ms3d_kmap_pairlist_header_ints_rows(int Vout, int rows_per_tile);
size_t ms3d_kmap_pairlist_capacity_rows(int K, int Vout, int rows_per_tile);
int ms3d_kmap_pairlist_build_rows(const int *nbr, int K, int Vout, int rows_per_tile, int *tile_start, int *entries,
                                  void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
/* rows_per_tile may also be 32 (round 6): the list a 32 -> 32 layer walks with BOTH column blocks in one wave when the table
 * is dense enough (ms3d_spconv_pairlist_rows_dense).  The library remembers on the host which tile size every list it built
 * has (keyed by the tile_start address; the newest build at an address wins), so that the convolution entry points -- whose
 * signatures carry the two list pointers only -- launch the kernel variant the list was built for: */
int ms3d_kmap_pairlist_rows_of(const int *tile_start);   /* 32 / 64 / 128; 64 for a list this library did not build */

/* Offset-major pair list of a table (the classic per-offset in/out index pairs) for the backward-weight kernel:
 *   kt_start[header_ints]    K * tiles + 1 pair offsets: first pair of (offset k, 64-row tile t) at [k * tiles + t],
 *                            last = number of pairs; then part_start[257] (tile ranges of near-equal pair count, the
 *                            workgroups of the backward-weight kernel) and the per-tile pair prefix [tiles + 1] it is cut from
 *   entries[2 * pairs]       int2 per pair: (input row, output row), ascending output row inside an offset */
size_t ms3d_kmap_offsetlist_header_ints(int K, int Vout);
size_t ms3d_kmap_offsetlist_capacity(int K, int Vout);
int ms3d_kmap_offsetlist_build(const int *nbr, int K, int Vout, int *kt_start, int *entries, void *workspace,
                               size_t workspace_bytes, ms3d_stream_t stream);

/* spatial sort keys (batch | 45-bit Morton code): rows sorted by this key keep a voxel's 26 neighbours close in
 * memory, so the conv gathers of one XCD stay inside its own L2 slice */
int ms3d_morton_keys(const int *coords, int V, long long *keys, ms3d_stream_t stream);

/* weights W[K][Cin][Cout] -> MFMA-fragment order.  transpose=1 (+mirror=1 for k3) gives the backward-data
 * operator: Weff[k] = W[mirror ? K-1-k : k]^T with Cin_eff = Cout, Cout_eff = Cin. */
size_t ms3d_spconv_wf_floats(int K, int Cin_eff, int Cout_eff);
/* wf_stream (same size as wf, or NULL): the same weights in "streamed" order, read 16 bytes per lane straight from L2 by
 * the kernels for layers whose weights do not fit LDS (more than 32 channels on a side, pair-listed tables) */
int ms3d_spconv_prep_weights(const float *W, int K, int Cin_eff, int Cout_eff, int transpose, int mirror, float *wf,
                             float *wf_stream, ms3d_stream_t stream);
/* out[i,:] = sum_k act(in[nbr[k][i],:]) @ Weff[k] (+ residual); act = optional x*pre_scale+pre_shift (+ReLU).
 * With bn_x != NULL the epilogue is the backward of a fused BN+ReLU: out = dz = acc * [bn_x*bn_scale+bn_shift > 0]
 * and bn_partial [ms3d_spconv_partial_blocks()][2][Cout] receives per-block sums of dz and dz*xhat. */
int ms3d_spconv_partial_blocks(int Vout, int K, int Cin, int Cout, int with_pairlist /* 0 = no list; 1 = a 64-row list;
                               otherwise the list's rows per tile (ms3d_kmap_pairlist_rows_of) */);
/* The forward / backward-data plan, read-only: the kernel family ms3d_spconv_forward (and the layer entry points) launch
 * for a call of this shape, and its launch geometry.  The launch reads the same plan function and nothing else.
 *   pl_rows     rows per tile of the pair list the call is given: 0 = none, else 32 / 64 / 128 (1 = 64, as above)
 *   aux_kind    what the call's aux image holds (ms3d_spconv_aux_kind_p; 0 = none, as ms3d_spconv_forward without wf_stream)
 *   with_stats  the call writes bn_partial (bn_x != NULL, or out_stats with a bn_partial)
 *   plan8[0]    family, MS3D_FWD_* below
 *   plan8[1]    nbt: 16-column blocks per wave        plan8[2]  ny: column slices (gridDim.y; weight-stationary: per row part)
 *   plan8[3]    gridDim.x as launched                 plan8[4]  threads per block
 *   plan8[5]    dynamic LDS bytes
 *   plan8[6]    small families: 16-row tiles per block (1 or 3); pair-list / stream family: 16-row tiles per tile of the
 *               list (2 or 4 / 8); otherwise 1
 *   plan8[7]    rows of bn_partial a call with statistics writes = ms3d_spconv_partial_blocks(Vout, K, Cin, Cout, pl_rows)
 * Returns 0, or MS3D_E_UNSUPPORTED exactly where the launch would (plan8 is then all zero).  Vout <= 0: 0 and an all-zero
 * plan (nothing is launched). */
#define MS3D_FWD_WS 1            /* spconv_fwd_ws_kernel: weight-stationary, coarse levels */
#define MS3D_FWD_SMALL 2         /* spconv_fwd_small_kernel: one block per 16-row tile (or per 3 on the bf16 geometry), f32 */
#define MS3D_FWD_SMALL_BF3 3     /* spconv_fwd_small_bf3_kernel: the same on the bf16 image, one tile per block */
#define MS3D_FWD_SMALL_BF3_RT 4  /* spconv_fwd_small_bf3_rt_kernel: three tiles per block on the bf16 image */
#define MS3D_FWD_PAIRSTREAM 5    /* spconv_fwd_pairstream_kernel: 128-row pair list, weights streamed from L2 */
#define MS3D_FWD_PAIRLIST 6      /* spconv_fwd_pairlist_kernel: 64-row or 32-row pair list, weights in LDS */
#define MS3D_FWD_BF3 7           /* spconv_fwd_bf3_kernel: table walk on the bf16 image */
#define MS3D_FWD_RESIDENT 8      /* spconv_fwd_kernel, all weights LDS resident, persistent waves */
#define MS3D_FWD_STREAMED 9      /* spconv_fwd_kernel, weights streamed through LDS in offset groups */
int ms3d_spconv_forward_plan(int Vout, int K, int Cin, int Cout, int pl_rows, int aux_kind, int with_stats, int *plan8);
/* rows per tile of the pair list a forward / backward-data convolution of this shape wants in pl_tile_start / pl_entries:
 * 0 = none, 64 = ms3d_kmap_pairlist_build, 128 = ms3d_kmap_pairlist_build_rows(.., 128, ..) */
int ms3d_spconv_pairlist_rows(int Vout, int K, int Cin, int Cout);
/* the same for a DENSE table (about 8+ of 27 neighbours per row: every level but the full-resolution one): 32 for the
 * 32 -> 32 layers (both column blocks per wave on 32-row tiles: every row gathered once instead of once per 16-column
 * slice; at 5.5 neighbours per row a 32-row tile pads 6.5 pairs per offset to 16 and loses), otherwise
 * ms3d_spconv_pairlist_rows.  The caller decides from the table's pair count which of the two lists to build. */
int ms3d_spconv_pairlist_rows_dense(int Vout, int K, int Cin, int Cout);
/* 1 when the convolution kernels have a pair-list variant worth building the list for (full-resolution levels) */
int ms3d_kmap_pairlist_wanted(int K, int Vout);
int ms3d_spconv_forward(const float *in, const float *wf, const int *nbr, int Vout, int K, int Cin, int Cout,
                        float *out, const float *pre_scale, const float *pre_shift, int pre_relu,
                        const float *residual, const float *bn_x, const float *bn_scale, const float *bn_shift,
                        const float *bn_mean, const float *bn_invstd, float *bn_partial, int out_stats,
                        const float *bias /* [Cout] or NULL */,
                        const int *pl_tile_start /* pair list of `nbr` (ms3d_kmap_pairlist_build) or NULL */,
                        const int *pl_entries,
                        const float *wf_stream /* streamed image of the same weights; required when a pair list is given
                                                  and a side has more than 32 channels, NULL otherwise */,
                        ms3d_stream_t stream);
/* out_stats != 0 (forward only): bn_partial [ms3d_spconv_partial_blocks()][2][Cout] receives per-block
 * (sum, sum of squares) of the OUTPUT rows (after the residual add) -> feed ms3d_bn_finalize, no extra pass. */
int ms3d_spconv_prep_weights_pair(const float *W, int K, int Cin, int Cout, int mirror_bwd, float *wf, float *wft,
                                  float *wf_stream /* or NULL */, float *wft_stream /* or NULL */, ms3d_stream_t stream);
/* 1 if a layer of this shape can be served by the weight-streaming kernel (then its descriptor in
 * ms3d_spconv_prep_weights_multi must ask for the streamed images: field `stream`) */
int ms3d_spconv_wants_stream_image(int K, int Cin, int Cout);
/* what the aux slot (2n floats) behind each weight image of a layer buffer holds: 0 nothing, 1 the streamed f32 image,
 * 2 the three-piece bf16 image (wide square layers; 3 / 4: two- / one-piece, ms3d_spconv_aux_kind_p).  Layer buffer = [image n | aux 2n | transposed image n | aux 2n],
 * n = ms3d_spconv_wf_floats(K, Cin, Cout). */
int ms3d_spconv_aux_kind(int K, int Cin, int Cout);
/* Both images of n layers in ONE launch (a U-Net re-lays ~90 weight tensors per step, ~5 us of dispatch each).
 * descs: device array of n 48-byte records {const float *W; float *wf; float *wft; int K, Cin, Cout, mirror_bwd,
 * block_begin, stream}, stream = ms3d_spconv_aux_kind(K, Cin, Cout), block_begin = running sum of ms3d_spconv_prep_blocks(K, Cin, Cout); total_blocks = the full sum.
 * wf and wft each have room for 3 * ms3d_spconv_wf_floats() floats: the image, then its aux image (slot of 2n). */
int ms3d_spconv_prep_blocks(int K, int Cin, int Cout);
int ms3d_spconv_prep_weights_multi(const void *descs, int n, int total_blocks, ms3d_stream_t stream);
int ms3d_bn_finalize(const float *partial, int nparts, long V, int C, float eps, float momentum, const float *gamma,
                     const float *beta, float *running_mean, float *running_var, float *mean, float *invstd,
                     float *scale, float *shift, ms3d_stream_t stream);
/* dW[k] = sum_i act(in[nbr[k][i],:])^T dout[i,:].  Deterministic: per-row-chunk partial slabs reduced in a fixed
 * order.  partial_ws MUST hold ms3d_spconv_wgrad_ws_floats(Vout, K, Cin, Cout) floats: the slab count depends on the
 * kernel that serves the shape (K = 1 heads: up to 1024 slabs; bf16x3 layers: the operand images behind the slabs).
 * ms3d_spconv_wgrad_row_chunks(Vout) is the row count's share of that decision only: a route may take fewer slabs or
 * more (the two-chunk list kernel: 128 parts from 65 row chunks on) -- size nothing from it. */
int ms3d_spconv_wgrad_row_chunks(int Vout);
/* Backward-weight workspace.  Every workgroup along the rows leaves one partial dW slab of n = K*Cin*Cout floats at
 * partial_ws + slab * n; the slabs are then summed in slab order.  Layout of partial_ws, in floats:
 *   [0, ms3d_spconv_wgrad_slab_floats)     the slabs; a call writes the first ms3d_spconv_wgrad_slabs() * n of them
 *   [slab_floats, slab_floats + 64)        alignment slack
 *   only when ms3d_spconv_wgrad_is_bf16x3_g(Vout, K, Cin, Cout, 0, 1), from the next 16-byte boundary behind slab_floats:
 *     divup(Vout, 32) * divup(Cout, 16) * P * 64 * 4 + 8    the dout operand image (P = 3 - precision bf16 pieces)
 *     Vout * Cin * P / 2 + 8                                the activated input in P bf16 pieces
 * ms3d_spconv_wgrad_ws_floats_p is the sum of these, ms3d_spconv_wgrad_ws_floats its precision-0 value.
 * ms3d_spconv_wgrad_slabs: the slabs a call of this shape leaves (offset_list: an offset list is passed; submanifold: as
 * the *_g entry points take it, 1 for the entry points without the flag); 0 for Vout <= 0, MS3D_E_UNSUPPORTED where the
 * launch returns it.  With wgrad_deferred_nblk this is the value the layer entry point reports.
 * ms3d_spconv_wgrad_slab_floats: the largest slab count over offset_list 0 / 1 and submanifold 0 / 1, times n.
 * The launch and these queries read ONE plan, so the chunk knobs (MS3D_WGRAD_*_CHUNKS, MS3D_WGRAD_*_ROUNDS) may be
 * raised above their defaults without outgrowing the workspace: the sizes follow. */
int ms3d_spconv_wgrad_slabs(int Vout, int K, int Cin, int Cout, int offset_list, int submanifold, int precision);
size_t ms3d_spconv_wgrad_slab_floats(int Vout, int K, int Cin, int Cout);
/* floats of partial_ws a backward-weight call may use (slabs; wide K = 27 layers add the three-piece bf16 images of both
 * operands).  K = 27 is the SUBMANIFOLD case: `in` and `dout` have the same Vout rows -- a 27-offset table whose input row
 * set differs from its output row set is outside this entry point's contract (the bf16x3 path splits Vout rows of `in`). */
size_t ms3d_spconv_wgrad_ws_floats(int Vout, int K, int Cin, int Cout);
/* 1 when a backward-weight call of this shape runs on three-piece bf16 operands (offset_list: an offset list is passed) */
int ms3d_spconv_wgrad_is_bf16x3(int Vout, int K, int Cin, int Cout, int offset_list);
int ms3d_spconv_backward_weight(const float *in, const float *dout, const int *nbr, int Vout, int K, int Cin,
                                int Cout, float *dW, const float *pre_scale, const float *pre_shift, int pre_relu,
                                float *partial_ws,
                                const int *ol_kt_start /* offset list of `nbr` (ms3d_kmap_offsetlist_build) or NULL */,
                                const int *ol_entries, ms3d_stream_t stream);
/* One-call layer entry points (forward / backward of a fused [BN -> ReLU ->] conv): same kernels as above, enqueued
 * from native code.  wf_buf holds both weight images, each followed by its streamed form
 * (4 * ms3d_spconv_wf_floats(K,Cin,Cout) floats: [wf | wf streamed | wft | wft streamed]) and is
 * kept by the caller between forward and backward; ws: ms3d_spconv_layer_ws_floats() floats of scratch.
 * layer_forward with W == NULL skips the re-lay: wf_buf already holds the current images (prep_weights_multi). */
size_t ms3d_spconv_layer_ws_floats(int Vin, int Vout, int K, int Cin, int Cout);
int ms3d_spconv_layer_forward(const float *x, const float *W, const int *nbr_fwd, int Vout, int K, int Cin, int Cout,
                              int mirror_bwd, const float *pre_scale, const float *pre_shift, int pre_relu,
                              const float *residual, const float *bias, float *wf_buf, float *y, float *stat_partial,
                              const int *pl_tile_start /* pair list of nbr_fwd or NULL */, const int *pl_entries,
                              void *ev_start /* hipEvent_t or NULL */, void *ev_stop, ms3d_stream_t stream);
/* HIP events for timing a launch on the stream it is issued on (recorded inside ms3d_spconv_layer_forward around
 * the convolution kernel only) */
void *ms3d_event_create(void);
void ms3d_event_destroy(void *event);
int ms3d_event_record(void *event, ms3d_stream_t stream);
float ms3d_event_elapsed_ms(void *start, void *stop);
int ms3d_spconv_layer_backward(const float *x, const float *dy, const float *wf_buf, const int *nbr_fwd,
                               const int *nbr_bwd, int Vin, int Vout, int K, int Cin, int Cout, const float *scale,
                               const float *shift, const float *mean, const float *invstd, int pre_relu, int training,
                               int need_dx, float *dx,
                               const float *dx_add /* or NULL: [Vin, Cin] added to dx -- the gradient that reaches x over a skip
                                                      connection (fused into the BatchNorm-backward pass / the residual epilogue) */,
                               float *dgb, float *dW, float *ws,
                               const int *ol_fwd_kt_start /* offset list of nbr_fwd or NULL */, const int *ol_fwd_entries,
                               const int *pl_bwd_tile_start /* pair list of nbr_bwd or NULL */, const int *pl_bwd_entries,
                               void *ev_start /* hipEvent_t or NULL: around the backward-data kernel */, void *ev_stop,
                               void *ev_wg_start /* hipEvent_t or NULL: around the backward-weight kernels */, void *ev_wg_stop,
                               float *ws_wgrad /* slab workspace of the second stream (ms3d_spconv_layer_ws_floats) or NULL */,
                               ms3d_stream_t wgrad_stream /* NULL: backward-weight on `stream`; else it runs on this
                                                             stream beside the backward-data chain */,
                               int join /* 1: `stream` waits for the backward-weight before the call returns control
                                           of it; 0: the caller joins the streams before dW is read */,
                               float *wgrad_slabs /* NULL, or ms3d_spconv_wgrad_ws_floats() floats of the caller's that outlive
                                                     the call: the backward-weight slabs go there instead of into ws */,
                               int *wgrad_deferred_nblk /* [host] NULL, or (with wgrad_slabs): the slab reduction is NOT
                                                           launched; receives the number of slabs to reduce later with
                                                           ms3d_wgrad_reduce_multi (0: dW is final) */,
                               void *wgrad_deferred_launch /* [host] NULL, or (with the two above, no timing events) a buffer of
                                                              ms3d_spconv_wgrad_launch_bytes(): when the layer's backward-weight
                                                              takes the f32 table walk (the small levels) the KERNEL is not
                                                              launched either but described here; int[4] of the buffer =
                                                              variant (0: it was launched as usual), int[1..3] = its grid */,
                               ms3d_stream_t stream);
/* Matmul precision (torch.set_float32_matmul_precision) of the *_p entry points: precision 0 = "highest", 1 = "high",
 * 2 = "medium"; anything else returns MS3D_E_UNSUPPORTED (size queries: 0).  It changes only the routes that run on
 * bf16 pieces at precision 0 -- forward / backward-data with both sides >= 48 channels, backward-weight of the wide
 * K = 27 layers -- which then keep P = 3 / 2 / 1 pieces of the same split, x0 = bf16_rne(x), x1 = bf16_rne(x - x0),
 * x2 = bf16_rne(x - x0 - x1), taken of the activated input (after the fused BatchNorm / ReLU) and of the weights / dy:
 *   P = 3: x0w0 + x0w1 + x1w0 + x1w1 + x0w2 + x2w0 (float32 grade), P = 2: x0w0 + x0w1 + x1w0, P = 1: x0w0,
 * each product exact in the f32 accumulator.  Every other route is exact float32 at every precision.  The existing
 * entry points are the precision-0 forms of these.
 * aux_kind_p: the aux image kind of a layer at that precision (2 / 3 / 4 = bf16 image of 3 / 2 / 1 pieces; what
 * ms3d_spconv_prep_weights_multi's `stream` field takes).  layer_backward_p must be given the precision its
 * layer_forward_p laid wf_buf out with.  wgrad_pieces: pieces of the backward-weight kernel (0 = f32 kernel).
 * wgrad_ws_floats_p <= ms3d_spconv_wgrad_ws_floats; ms3d_spconv_layer_ws_floats bounds every precision. */
int ms3d_spconv_aux_kind_p(int K, int Cin, int Cout, int precision);
/* ms3d_spconv_prep_weights_multi for the descriptors of one precision: bf16 images are written for the layers whose
 * `stream` is ms3d_spconv_aux_kind_p(.., precision) (the precision-0 entry point writes those of kind 2) */
int ms3d_spconv_prep_weights_multi_p(const void *descs, int n, int total_blocks, int precision, ms3d_stream_t stream);
int ms3d_spconv_wgrad_pieces(int Vout, int K, int Cin, int Cout, int offset_list, int precision);
size_t ms3d_spconv_wgrad_ws_floats_p(int Vout, int K, int Cin, int Cout, int precision);
int ms3d_spconv_backward_weight_p(const float *in, const float *dout, const int *nbr, int Vout, int K, int Cin,
                                  int Cout, float *dW, const float *pre_scale, const float *pre_shift, int pre_relu,
                                  float *partial_ws, const int *ol_kt_start, const int *ol_entries, int precision,
                                  ms3d_stream_t stream);
int ms3d_spconv_layer_forward_p(const float *x, const float *W, const int *nbr_fwd, int Vout, int K, int Cin, int Cout,
                                int mirror_bwd, const float *pre_scale, const float *pre_shift, int pre_relu,
                                const float *residual, const float *bias, float *wf_buf, float *y, float *stat_partial,
                                const int *pl_tile_start, const int *pl_entries, void *ev_start, void *ev_stop,
                                int precision, ms3d_stream_t stream);
int ms3d_spconv_layer_backward_p(const float *x, const float *dy, const float *wf_buf, const int *nbr_fwd,
                                 const int *nbr_bwd, int Vin, int Vout, int K, int Cin, int Cout, const float *scale,
                                 const float *shift, const float *mean, const float *invstd, int pre_relu, int training,
                                 int need_dx, float *dx, const float *dx_add, float *dgb, float *dW, float *ws,
                                 const int *ol_fwd_kt_start, const int *ol_fwd_entries, const int *pl_bwd_tile_start,
                                 const int *pl_bwd_entries, void *ev_start, void *ev_stop, void *ev_wg_start,
                                 void *ev_wg_stop, float *ws_wgrad, ms3d_stream_t wgrad_stream, int join,
                                 float *wgrad_slabs, int *wgrad_deferred_nblk, void *wgrad_deferred_launch, int precision,
                                 ms3d_stream_t stream);
/* Tables of ANY geometry (ms3d_kmap_general / ms3d_kmap_invert: other kernel sizes, strided and dilated layers, their
 * transposes).  The forward / backward-data entry points read their input through the table only and serve every table
 * (K > 27 and small levels of K > 36 take the general table walk; no pair list or offset list exists for K > 27).  The
 * backward-weight side has one route that takes the input row set for the output row set (three-piece bf16 operands of the
 * wide K = 27 layers): the *_g forms are told Vin and whether the table is a SUBMANIFOLD map (same coordinate set on both
 * sides, row for row) and keep every other table off it.  submanifold != 0 with Vin != Vout is MS3D_E_UNSUPPORTED.  The
 * entry points without the flag take a K = 27 table for a submanifold map, as they always did
 * (ms3d_spconv_layer_backward_p: when also Vin == Vout).  The workspace sizes of the forms without the flag bound these. */
int ms3d_spconv_wgrad_is_bf16x3_g(int Vout, int K, int Cin, int Cout, int offset_list, int submanifold);
int ms3d_spconv_backward_weight_g(const float *in, const float *dout, const int *nbr, int Vin, int Vout, int K, int Cin,
                                  int Cout, float *dW, const float *pre_scale, const float *pre_shift, int pre_relu,
                                  float *partial_ws, const int *ol_kt_start, const int *ol_entries, int submanifold,
                                  int precision, ms3d_stream_t stream);
int ms3d_spconv_layer_backward_g(const float *x, const float *dy, const float *wf_buf, const int *nbr_fwd,
                                 const int *nbr_bwd, int Vin, int Vout, int K, int Cin, int Cout, const float *scale,
                                 const float *shift, const float *mean, const float *invstd, int pre_relu, int training,
                                 int need_dx, float *dx, const float *dx_add, float *dgb, float *dW, float *ws,
                                 const int *ol_fwd_kt_start, const int *ol_fwd_entries, const int *pl_bwd_tile_start,
                                 const int *pl_bwd_entries, void *ev_start, void *ev_stop, void *ev_wg_start,
                                 void *ev_wg_stop, float *ws_wgrad, ms3d_stream_t wgrad_stream, int join,
                                 float *wgrad_slabs, int *wgrad_deferred_nblk, void *wgrad_deferred_launch, int precision,
                                 int submanifold, ms3d_stream_t stream);
/* Deferred backward-weight launches of MANY layers of one variant as one launch: descs = DEVICE array of the 128-byte
 * descriptions, each with its first int set to the layer's first block (blocks are numbered layer after layer, a layer
 * has int[1] * int[2] * int[3] of them), total_blocks = their sum.  x, dy, the tables and the slab areas the descriptions
 * point to must still be alive.  Follow with ms3d_wgrad_reduce_multi over the same layers. */
size_t ms3d_spconv_wgrad_launch_bytes(void);
int ms3d_spconv_wgrad_is_table_walk(int Vout, int K, int Cin, int Cout, int offset_list);
int ms3d_spconv_wgrad_multi(const void *descs, int n_desc, int total_blocks, int variant, ms3d_stream_t stream);
/* The slab reductions dW = sum of slabs of MANY layers in one launch, bit-identical to the per-layer reduction.
 * descs: DEVICE array of n_desc records {const float *slabs; float *dW; int64_t n (floats per slab); int32_t nblk (slabs);
 * int32_t block_begin} (32 bytes each) in ascending block order; a layer takes ms3d_wgrad_reduce_blocks() blocks and sets
 * bit 31 of block_begin when that call reports the 16-byte geometry (*wide = 1); total_blocks = their sum. */
int ms3d_wgrad_reduce_blocks(long n, const float *slabs, const float *dW, int *wide /*[host]*/);
int ms3d_wgrad_reduce_multi(const void *descs, int n_desc, int total_blocks, ms3d_stream_t stream);

/* BatchNorm1d over rows, training mode (biased var for normalisation, unbiased into running_var) */
int ms3d_bn_stats(const float *x, long V, int C, float eps, float momentum, const float *gamma, const float *beta,
                  float *running_mean, float *running_var, float *mean, float *invstd, float *scale, float *shift,
                  float *partial_ws, int partial_rows, ms3d_stream_t stream);
int ms3d_bn_apply(const float *x, long V, int C, const float *scale, const float *shift, int relu, float *y,
                  ms3d_stream_t stream);
int ms3d_reduce_partials(const float *partial, int nparts, int n, float *out, ms3d_stream_t stream);
/* column sums of x [V, C] -> out2c[0..C) (out2c[C..2C) = column sums of squares); partial_ws: partial_rows*2*C floats */
int ms3d_column_sum(const float *x, long V, int C, float *partial_ws, int partial_rows, float *out2c, ms3d_stream_t stream);
int ms3d_bn_bwd_apply(const float *dz, const float *x, long V, int C, const float *scale, const float *mean,
                      const float *invstd, const float *s1s2, float *dx, ms3d_stream_t stream);
/* ms3d_reduce_partials + ms3d_bn_bwd_apply_add in ONE launch, bit-identical: s1s2 [2][C] = column sums of partial
 * [nparts][2][C]; dx (or NULL: sums only) = scale * (dz - s1/V - xhat * s2/V) [+ add]; dz == dx allowed.  2C <= 1024. */
int ms3d_bn_bwd_reduce_apply(const float *partial, int nparts, const float *dz, const float *x, long V, int C,
                             const float *scale, const float *mean, const float *invstd, const float *add, float *dx,
                             float *s1s2, ms3d_stream_t stream);
/* the same with `add` [V, C] (or NULL) added to the result */
int ms3d_bn_bwd_apply_add(const float *dz, const float *x, long V, int C, const float *scale, const float *mean,
                          const float *invstd, const float *s1s2, const float *add, float *dx, ms3d_stream_t stream);
int ms3d_bn_bwd_partial(const float *dy, const float *x, long V, int C, const float *scale, const float *shift,
                        const float *mean, const float *invstd, int relu, float *dz, float *partial_ws,
                        int partial_rows, int *nparts_out /*[host]*/, ms3d_stream_t stream);

/* ======================================================================================
 * Dense tensors in and out (csrc/dense.hip): sparse rows F [V, C] <-> a dense grid float [B, C, X, Y, Z].  A CELL is one
 * (b, x', y', z') of the grid, numbered ((b * X + x') * Y + y') * Z + z'; element (b, c, cell) of the grid lies at
 * (b * C + c) * X * Y * Z + (cell - b * X * Y * Z).  Every entry point returns MS3D_E_UNSUPPORTED WITHOUT touching a pointer
 * or launching when a size is negative, the grid has more than 2^31 - 1 cells or B * C * X * Y * Z >= 2^63.  Nothing adds
 * floats; every result is the same bytes on every run.
 * ====================================================================================== */
/* the tile of the two feature kernels: cells (list entries) and channels per workgroup */
int ms3d_dense_tile_cells(void);
int ms3d_dense_tile_channels(void);
/* Cell map of a coordinate set: coords int32 [V, 4] (b, x, y, z); origin [host, 3]; the cell index of a row per axis is
 * (x - origin_x) / divisor (divisor >= 1: the tensor stride when strides are contracted, else 1).  cell_row [B*X*Y*Z]: the row
 * at each cell, -1 where none -- where several rows name one cell, the LOWEST row; row_cell [V]: the cell of each row, -1 for a
 * row outside the grid or with a difference the divisor does not divide.  counts [host, 3] = (rows outside the grid, rows not
 * divisible by the divisor, rows that lost their cell to another row); counts_dev: 4 ints of device scratch.  V == 0 fills
 * the table with -1.  One host sync (none for V == 0). */
int ms3d_dense_cell_map(const int *coords, int V, const int *origin /*[host,3]*/, int divisor, int B, int X, int Y, int Z,
                        int *cell_row, int *row_cell, int *counts_dev, int *counts /*[host,3]*/, ms3d_stream_t stream);
/* Rows -> grid: out[b, c, cell] = F[row * ld + c] with row = cell_row[cell] (through row_index[row] when row_index is not
 * NULL: the table names rows of one order, the features are held in another), 0 where the cell has no row (or the row is
 * >= n_rows).  Every element of out is written exactly once; no memset is needed in front.  ld >= C: floats between rows. */
int ms3d_dense_scatter(const float *F, long n_rows, long ld, const int *cell_row, const int *row_index, int B, int C, int X,
                       int Y, int Z, float *out /*[B,C,X,Y,Z]*/, ms3d_stream_t stream);
/* Grid -> rows: out[i, c] = grid[b, c, cells[i]] for i < n (out [n, C], contiguous); a cell outside [0, B*X*Y*Z) gives a zero
 * row; a cell listed twice is read twice. */
int ms3d_dense_gather(const float *grid, int B, int C, int X, int Y, int Z, const int *cells, long n, float *out,
                      ms3d_stream_t stream);
/* Occupancy: keep [B*X*Y*Z] = 1 where any channel of the cell is != 0 (NaN counts, -0.0 does not), every cell when grid is
 * NULL; rank [B*X*Y*Z] = the exclusive scan of keep; *n_kept [host] = the number kept (one host sync).
 * ms3d_dense_cells_emit then writes the kept cells in ascending cell order: out_coords int32 [n_kept, 4] (b, x, y, z) and
 * out_cells int32 [n_kept]. */
size_t ms3d_dense_occupancy_workspace_bytes(void);
int ms3d_dense_occupancy(const float *grid, int B, int C, int X, int Y, int Z, unsigned char *keep, int *rank,
                         int *n_kept /*[host]*/, void *workspace, size_t workspace_bytes, ms3d_stream_t stream);
int ms3d_dense_cells_emit(const unsigned char *keep, const int *rank, int B, int X, int Y, int Z, int *out_coords,
                          int *out_cells, ms3d_stream_t stream);

/* ======================================================================================
 * Instance post-processing (validation / test time): replaces the dense [P, N] mask algebra of
 * model/pointgroup.py:197-265 (cross IoU by mask matrix product on the host + numpy greedy NMS).
 * ====================================================================================== */
/* inter[a][b] = number of points shared by proposals a and b (diagonal = proposal sizes).  The (cluster, point) pairs
 * must be unique and sorted by point: pair_point[S] ascending, pair_cluster[S] the proposal of each pair. */
int ms3d_proposal_cross_intersection(const int *pair_point, const int *pair_cluster, int S, int P, int *inter /*[P,P]*/,
                                     ms3d_stream_t stream);
/* greedy non-maximum suppression in the given order (descending score): a proposal is picked unless an earlier pick
 * has IoU = inter/(n_a+n_b-inter) > threshold with it (float32, as the reference).  pick[P], *n_pick on the device;
 * suppressed_ws: P bytes of scratch. */
int ms3d_nms_greedy(const int *inter, const int *order, int P, float threshold, unsigned char *suppressed_ws, int *pick,
                    int *n_pick, ms3d_stream_t stream);

/* ======================================================================================
 * Augmentation: elastic distortion (util/transform.py:65-84, called twice per training scene from
 * data/dataset/general_dataset.py:118-120).  noise: three float32 grids [3][bx][by][bz] drawn by the caller
 * (host RNG, same shapes/order as the reference), blurred in place (noise_tmp: same size scratch);
 * out = xyz + mag * trilinear(noise)(xyz), float64, grid nodes at linspace(-(b-1)*gran, (b-1)*gran, b).
 * ====================================================================================== */
int ms3d_elastic_distort(const double *xyz /*[N,3]*/, int N, float *noise, float *noise_tmp, int bx, int by, int bz,
                         double gran, double mag, double *out /*[N,3]*/, ms3d_stream_t stream);

/* ---- optimizer: one Adam step over all parameter tensors of a model in one launch (the reference's optimizer is
 * torch.optim.Adam through Hydra, config/model/base.yaml:23-28; arithmetic as torch's fused Adam, f32).
 * chunks: int2 (tensor, chunk index) per workgroup, ms3d_adam_chunk_elems() elements per chunk; p / g / m / v: device
 * arrays of device pointers (parameter, gradient, exp_avg, exp_avg_sq), sizes: elements per tensor (device, int64).
 * bias_correction_i = 1 - beta_i^step. */
int ms3d_adam_chunk_elems(void);
int ms3d_adam_step(const int *chunks, int n_chunks, void *const *p_ptrs, const void *const *g_ptrs, void *const *m_ptrs,
                   void *const *v_ptrs, const long *sizes, float lr, float beta1, float beta2, float eps,
                   float weight_decay, double bias_correction1, double bias_correction2, ms3d_stream_t stream);
/* the same with a step counter PER TENSOR (torch.optim.Adam starts a parameter's counter with its first gradient):
 * coef = device float2 per tensor (lr / bias_correction1, sqrt(bias_correction2)) of that tensor's own step */
int ms3d_adam_step_multi(const int *chunks, int n_chunks, void *const *p_ptrs, const void *const *g_ptrs,
                         void *const *m_ptrs, void *const *v_ptrs, const long *sizes, const float *coef, float beta1,
                         float beta2, float eps, float weight_decay, ms3d_stream_t stream);

/* ---- device-wide exclusive prefix sum of int32 (the utility behind the ball query's cell / list starts, the clustering
 * output assembly and the coordinate engine): out[i] = in[0] + .. + in[i-1], in == out allowed, *total_out_dev (device,
 * optional) = the sum of all.  One launch (decoupled look-back between workgroups).  workspace: ms3d_scan_i32_workspace_bytes(). */
size_t ms3d_scan_i32_workspace_bytes(void);
int ms3d_scan_i32(const int *in, int *out, int n, int *total_out_dev, void *workspace, ms3d_stream_t stream);

/* ---- per-point losses of the backbone heads, forward and gradients (the reference: GeneralModel._loss,
 * model/general_model.py:36-50 -- cross_entropy(ignore_index=-1) -- and PTOffsetLoss, loss/pt_offset_loss.py:11-38 -- mean
 * L1 norm of the offset error and mean negative cosine over the points with instance_ids != -1; with no valid point a
 * loss is 0).  forward: out5 = (semantic loss, offset norm loss, offset direction loss, 1 / #labelled, 1 / #instance
 * points); d_scores [N, C], d_norm / d_dir [N, 3] receive the UNNORMALISED gradients; partial_ws: 5 doubles per block of
 * ms3d_point_losses_blocks(N).  scale_grads (backward): d_scores *= *g_sem * out5[3] in place and
 * d_norm = (*g_norm * d_norm + *g_dir * d_dir) * out5[4]; g_* are DEVICE scalars (the upstream gradients) or NULL (= 0). */
int ms3d_point_losses_blocks(long N);
int ms3d_point_losses_forward(const float *scores /*[N,C]*/, const short *labels /*[N]*/, const float *pred_offsets /*[N,3]*/,
                              const float *centre /*[N,3]*/, const float *xyz /*[N,3]*/, const short *instance_ids /*[N]*/,
                              long N, int C, float *d_scores, float *d_norm, float *d_dir, double *partial_ws, float *out5,
                              ms3d_stream_t stream);
int ms3d_point_losses_scale_grads(float *d_scores, long n_scores, float *d_norm, const float *d_dir, long n_off,
                                  const float *out5, const float *g_sem, const float *g_norm, const float *g_dir,
                                  ms3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSU3D_HIP_H */
