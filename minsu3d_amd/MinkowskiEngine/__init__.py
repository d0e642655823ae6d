"""The MinkowskiEngine subset the reference models import (`import MinkowskiEngine as ME`), served by the
gfx950 sparse-voxel engine.  The 9 symbols the reference uses:

    SparseTensor, MinkowskiConvolution, MinkowskiConvolutionTranspose, MinkowskiBatchNorm, MinkowskiReLU,
    cat, utils.sparse_quantize, utils.sparse_collate  (+ tensor attributes .features/.F, .coordinates/.C)

and what other networks written against that API use: convolutions of any kernel size and dilation at stride 1 or 2
with an optional bias, and

    MinkowskiMaxPooling, MinkowskiAvgPooling, MinkowskiSumPooling, MinkowskiGlobalMaxPooling,
    MinkowskiGlobalAvgPooling, MinkowskiGlobalSumPooling, MinkowskiLinear, MinkowskiDropout

and the layers of networks that create and drop coordinates (completion, reconstruction, decoders without an encoder of
the same shape):

    MinkowskiGenerativeConvolutionTranspose, MinkowskiPruning, SparseTensor.features_at_coordinates
    (+ SparseTensor.coordinate_rows, CoordinateManager.rooted: engine extras)

A generated or pruned tensor lives on a coordinate manager rooted at its own tensor stride; every layer above works on it.

Tensors on DIFFERENT coordinate sets of one tensor stride meet on the union of their sets (a manager rooted at that stride),
and one row per batch index meets every voxel of its batch:

    MinkowskiUnion, SparseTensor + - * (SparseTensors, Python scalars, torch tensors that broadcast to the rows),
    MinkowskiBroadcastAddition, MinkowskiBroadcastMultiplication, MinkowskiBroadcastConcatenation, MinkowskiBroadcast,
    MinkowskiSigmoid  (+ CoordinateManager.union / broadcast_map: engine extras)

Points in, points out -- how a network gets from a point cloud to voxels and back:

    TensorField (.sparse / .slice / .cat_slice / .inverse_mapping), SparseTensorQuantizationMode,
    SparseTensor.slice / .cat_slice / .interpolate, MinkowskiInterpolation, MinkowskiPoolingTranspose
    (+ CoordinateManager.interpolation_map: engine extra)

The depthwise layer of separable blocks, ConvNeXt-style sparse backbones and large-kernel context blocks:

    MinkowskiChannelwiseConvolution  (kernel (K, C), bias (1, C); the convolutions' geometries; float32 HIP gather kernels,
    csrc/chconv.hip; outside prepare_conv_weights: it is not a dense-weight convolution)

Normalisation per sample and the activations of the decoders, generators and registration networks that use it:

    MinkowskiInstanceNorm (eps 1e-8), MinkowskiStableInstanceNorm (eps 1e-6): `weight`, `bias` of shape (1, C), no running
    statistics; per batch index and channel, biased variance; segmented HIP reductions in a fixed order, shifted sums merged
    by Chan's formula (csrc/inorm.hip); rows read where they are held  (+ CoordinateManager.batch_group, the grouping of the
    rows by batch index as ONE record, backend.BatchGroup, that every per-sample op below reads; batch_rows, batch_segments,
    batch_chunks, batch_lengths, batch_indices and caller_rows are views onto it: engine extras)
    MinkowskiELU, MinkowskiLeakyReLU, MinkowskiPReLU, MinkowskiSELU, MinkowskiCELU, MinkowskiGELU, MinkowskiSiLU,
    MinkowskiTanh, MinkowskiSoftplus, MinkowskiHardswish, MinkowskiHardtanh, MinkowskiReLU6, MinkowskiSoftmax,
    MinkowskiLogSoftmax: the torch operator as `self.module`, applied to the rows

Dense tensors in and out, and the per-sample views of a batch:

    SparseTensor.dense(shape=None, min_coordinate=None, contract_stride=True) -> (dense [B, C, X, Y, Z], min_coordinate
    int32 [1, 3], tensor_stride int32 [3]); to_sparse(x, format=None, coordinates=None, device=None), to_sparse_all(x);
    MinkowskiToSparseTensor, MinkowskiToDenseTensor, MinkowskiToFeature; SparseTensor.decomposition_permutations,
    .decomposed_coordinates, .decomposed_features, .decomposed_coordinates_and_features, .coordinates_at(b), .features_at(b)
    (+ CoordinateManager.dense_map / extent / decomposition: engine extras)

    A transposing HIP kernel pair over a cached cell map (csrc/dense.hip): rows -> grid writes every element once (no fill in
    front), grid -> rows is its backward and the feature read of to_sparse; bit-exact copies, the same bytes on every run.
    Chosen here without a copy of MinkowskiEngine to compare against: min_coordinate=None takes the per-axis minimum of the
    coordinates as the origin (and returns it), an int means that value on every axis; to_sparse keeps a cell when ANY
    channel is != 0 (NaN counts, -0.0 does not) and orders the rows like torch.nonzero; a row outside the grid, a coordinate
    off the stride lattice and a repeated coordinate raise ValueError (nothing is clipped or summed silently).  "BXXXC" input is permuted and copied contiguous once.

Coordinate map keys, and layers onto coordinates the caller names:

    CoordinateMapKey (a manager plus a tensor stride: hashable, get_tensor_stride(), get_coordinate_size()),
    SparseTensor.coordinate_map_key, CoordinateManager.get_coordinates(key),
    SparseTensor(features, coordinate_map_key=key[, coordinate_manager=...]): a new tensor on an existing set, features in the
    order of that set's .coordinates (SparseTensor(F, coordinate_manager=cm, tensor_stride=ts) stays the engine's form: rows
    as the manager HOLDS them);
    `coordinates=` on MinkowskiConvolution (keyword only), MinkowskiConvolutionTranspose, MinkowskiChannelwiseConvolution,
    MinkowskiMaxPooling / AvgPooling / SumPooling and MinkowskiPoolingTranspose: an integer tensor [M, 4] (validated once by
    ms3d_coords_check, csrc/coords.hip: out of range, off the stride lattice and repeated rows raise ValueError), a
    CoordinateMapKey or a SparseTensor; the output lives on that set, a row no input reaches is zero or the bias;
    expand_coordinates=True on MinkowskiConvolution (stride 1), MinkowskiConvolutionTranspose and MinkowskiPoolingTranspose:
    the output set is every coordinate the kernel reaches  (+ CoordinateManager.target_map / expand: engine extras)

Kernel regions -- crosses and hand-written offset lists:

    RegionType (HYPER_CUBE, HYPER_CROSS, CUSTOM), KernelGenerator(kernel_size, stride, dilation, is_transpose, region_type,
    region_offsets, expand_coordinates, axis_types, dimension) and `kernel_generator=` on MinkowskiConvolution,
    MinkowskiConvolutionTranspose, MinkowskiGenerativeConvolutionTranspose, MinkowskiChannelwiseConvolution,
    MinkowskiMaxPooling / AvgPooling / SumPooling and MinkowskiPoolingTranspose  (+ KernelGenerator.offsets(tensor_stride),
    `region=` on CoordinateManager.kernel_map / kernel_map_inverse / target_map / generate / expand: engine extras)

    The offset rules, chosen here -- MinkowskiEngine's as recalled, not pinned, like the conventions above:
    HYPER_CUBE is kernel_offsets(kernel_size, dilation, ts), K = kernel_size ** 3, and the layer is the plain layer (same
    tables, same tuned routes).  HYPER_CROSS (odd kernel sizes, h = (kernel_size - 1) // 2, K = 6 h + 1): the centre first,
    then axis x at -h .. -1, +1 .. +h, then y, then z, each times dilation * ts; size 1 is the cube of size 1.  CUSTOM:
    region_offsets, an integer tensor or array [K, 3] with 1 <= K <= 254 and distinct rows, in the order given, times ts only
    (dilation must be 1, kernel_size is ignored).  `kernel` is (K, in, out) -- (K, C) channel-wise --, init bound 1 / sqrt(in
    * K).  A cross or custom layer always works between "two sets", even at stride 1 on its own set: forward table and
    inverse table from one pass of ms3d_kmap_region (csrc/coords.hip: one lookup per partnered pair of offsets, four stores),
    no mirrored weight image, never the K = 27 / K = 8 tuned routes; `residual=` / `skip=` are refused on it (ValueError).
    A layer argument that contradicts the generator, an even cross, repeated custom rows and CUSTOM with dilation != 1 raise
    ValueError.

Kernel, stride and origin maps as index pairs -- what a layer the user writes (local attention over a kernel map, a pooling,
a correspondence loss, a plot) indexes x.F with:

    CoordinateManager.kernel_map(in_key, out_key, stride=1, kernel_size=3, dilation=1, region_type=RegionType.HYPER_CUBE,
    region_offsets=None, is_transpose=False, is_pool=False, kernel_generator=None) -> {k: int64 [2, N_k]} (input row, output
    row), CoordinateManager.stride(key, stride=2) -> CoordinateMapKey, CoordinateManager.stride_map(in_key, stride_key) ->
    (in_rows, out_rows), CoordinateManager.origin_map(key) -> {0: int64 [2, V]}; a key is a CoordinateMapKey or a
    SparseTensor  (+ CoordinateManager.kernel_map_pairs -> (pairs int64 [2, P], start int32 [K + 1]): the packed form the dict
    is made of views of; kernel_map_tables: the engine's tables under a name of their own: engine extras)

    The rows are the rows of `.coordinates` / `.features` as the CALLER sees them, also on a Morton-sorted manager.  Column
    (i, o) of entry k: C_out[o] + off_k == C_in[i] with off = kernel_offsets / region_offsets at the input's tensor stride;
    is_transpose=True: C_out[o] - off_k == C_in[i] with off at the output's tensor stride (the rule of the generative
    layer); y.F = sum_k index_add(o, x.F[i] @ W[k]) is the layer.  The tables are the layers' own (kernel_map_tables,
    kernel_map_inverse, target_map for a set of another manager); ms3d_kmap_pairs_count / ms3d_kmap_pairs_fill (csrc/
    kmap_pairs.hip) pack them: ballot and popcount per (offset, run of rows), one scan, one host read of the pair count,
    then both int64 rows stored at their ranks, the caller's numbering folded in; no atomics, no sort, the same bytes on
    every run.  Cached per (keys, geometry, direction).  kernel_map(ts, kernel_size, ...) with a tensor stride first stays
    the engine's form.  stride_map pairs every row of the finer set with its parent, floor(c / s) * s, from the k2 tables;
    origin_map names, per row, the row of a MinkowskiGlobal*Pooling output its sample lands in (the rank of its batch index
    among those present -- checked against the global pooling layers).
    Chosen here without a copy of MinkowskiEngine to compare against, recalled, not pinned: int64 pairs; the dict holds only
    the offsets that have a pair, in ascending k; inside an entry the output row ascends; is_pool changes nothing (pooling
    and convolution share their tables); the keys' tensor strides must agree with `stride` (ValueError), as must the
    arguments with a kernel_generator given beside them.

Labels and batches in -- what a segmentation, completion or detection script calls before its first layer:

    utils.sparse_quantize(..., labels=, ignore_label=-100, return_maps_only=False)  (keyword-only: the positional order is the
    reference's call form, not MinkowskiEngine's), utils.batched_coordinates, utils.sparse_collate(coords, feats, labels),
    utils.batch_sparse_collate, utils.SparseCollation(limit_numpoints)

    Returns coords[, features][, labels][, index][, inverse]; one label per returned row, in the labels' own integer dtype.
    On the GPU the vote is ms3d_quantize_labels (csrc/labels.hip) over the maps of ms3d_sparse_quantize: two launches
    (initialise from the first-occurrence rows, then every dissenting row stores ignore_label), plain stores, no atomics, no
    sort, the same bytes on every run; on CPU tensors, numpy input and in DataLoader workers the same rule as a torch
    expression.  Chosen here without a copy of MinkowskiEngine to compare against: a voxel keeps a label only when ALL of
    its points carry it, else it gets ignore_label; ignore_label defaults to -100 and votes like any other label (a voxel
    whose points all carry it keeps it, a real label beside it does not win the voxel); labels that are not integers, not of
    shape [N] or outside int32, an ignore_label outside int32 or the labels' dtype, and return_maps_only with labels raise
    ValueError.  batched_coordinates floors float input and numbers the samples by their position in the list, empty
    samples included; sparse_collate hands a list of labels that are not arrays back as it is.

Local attention over a kernel map -- the block of window / neighbourhood transformers (engine extras: MinkowskiEngine has
no such layer, and nothing here is pinned to it):

    kernel_attention(q, k, v, num_heads, rel_bias=None, scale=None, kernel_size=3, stride=1, dilation=1,
    kernel_generator=None) -> a SparseTensor on q's coordinate set;
    MinkowskiKernelAttention(in_channels, num_heads, kernel_size=3, dilation=1, qkv_bias=True, rel_pos_bias=True,
    dimension=3, kernel_generator=None): proj(kernel_attention(q, k, v)) of qkv(x) on the tensor's own set; parameters
    qkv.weight, qkv.bias, proj.weight, proj.bias (nn.Linear) and rel_bias (K, num_heads), zero-initialised

    out[o, h, :] = sum_kk softmax_kk(scale * <q[o, h], k[i, h]> + rel_bias[kk, h]) v[i, h, :] over the inputs i that the
    kernel's offsets reach from row o and that are PRESENT (the pairs of CoordinateManager.kernel_map, the offsets in its
    order); C = num_heads * D, scale = D ** -0.5 unless given; a row that reaches no input is zero.  k and v share a
    coordinate set of tensor stride ts; q sits on the same manager at ts * stride or on a set of another manager at that stride
    (target_map); the geometries and their refusals are the convolutions', regions included.  csrc/kattn.hip: three float32
    gather kernels over the layers' own tables -- forward (one online-softmax sweep, the maximum always subtracted, saves the
    log-sum-exp), backward for q and rel_bias along the forward table, backward for k and v through the inverse table; the
    probabilities are recomputed, nothing of the size of the pair list is ever stored; no atomics, every sum in an order
    fixed by the shapes (the rel_bias gradient: one partial per run of ms3d_kattn_rows_per_part() rows, added in order), the
    same bytes on every run.  K <= 254, D <= 128.  Frozen k and v skip the kv pass; a frozen q and rel_bias skip the q pass when k and v
    are frozen too (the kv pass reads a per-row residual the q pass leaves).
    Out of scope: attention dropout, masks, a value head dimension different from D, float16 / bfloat16 rows, gradients
    through the coordinates.  Outside prepare_conv_weights: the block is not a dense-weight convolution.

Per-sample query attention -- the global block of a sparse transformer, the decoder step of the mask-transformer family
(engine extras: MinkowskiEngine has no such layer, and nothing here is pinned to it):

    query_attention(queries, k, v, num_heads, attn_mask=None, scale=None) -> a float32 tensor [B, Q, C];
    MinkowskiQueryAttention(embed_dim, num_heads, in_channels=None, bias=True): forward(queries, x, attn_mask=None) =
    out_proj(query_attention(q_proj(queries), k_proj(x), v_proj(x))); parameters q_proj, k_proj, v_proj, out_proj (nn.Linear;
    k_proj and v_proj map in_channels to embed_dim)

    out[b, q, h, :] = sum_i softmax_i(scale * <queries[b, q, h], k[i, h]>) v[i, h, :] over the rows i of sample b that attn_mask
    does not block; C = num_heads * D, scale = D ** -0.5 unless given.  k and v: SparseTensors on one coordinate set; queries
    [B, Q, C] with B the number of batch indices PRESENT, queries[b] for the b-th of them in ascending order (the numbering of
    CoordinateManager.batch_rows, of origin_map and of the global pooling layers' output rows; gaps in the batch indices and
    interleaved rows are fine; another B is a ValueError).  attn_mask: bool [V, Q], row i the i-th row of k.F / k.C as the
    caller sees them, column q the query of that row's own sample, True = may NOT attend, one mask for all heads.  A (b, q)
    whose rows are all blocked is zero, contributes to no gradient and receives none (torch.nn.MultiheadAttention gives NaN
    there).  csrc/qattn.hip: the rows of a sample are batch_rows' segment, read by index where they are held (on a
    Morton-sorted manager the mask row is found through the held-to-caller index); a segment is cut into chunks of
    ms3d_qattn_rows_per_chunk() positions (the record's `chunks`: one host read per coordinate set), one workgroup
    per chunk and tile of (query, head) items does an online-softmax sweep and leaves a partial, a second kernel merges the
    partials in chunk order and saves the log-sum-exp; the backward recomputes the probabilities -- a second sweep for the
    queries, a loop over the queries per voxel row for k and v.  Nothing of size V x Q is stored, no atomics, every sum in an
    order fixed by the shapes, the same bytes on every run.  D <= 128, Q <= 1024, C <= 1024, B <= 65535.  Frozen k and v skip
    their pass; frozen queries skip theirs when k and v are frozen too (the kv pass reads a per-query residual the q pass
    leaves).
    Out of scope (each raises ValueError, TypeError or NotImplementedError naming it): a different Q per sample, float or
    per-head masks, attention dropout, a value head dimension different from D, float16 / bfloat16, CPU tensors
    (NotImplementedError naming ms3d_qattn_forward); the reverse direction (voxels attending to queries) is voxel_attention
    below, and the TypeError says so.  The mask logits x.F @ queries[b].T are a per-sample matmul of the caller's.  Outside
    prepare_conv_weights.

Per-sample voxel attention -- the reverse direction, every voxel reads the queries of its own sample back: the second leg of
a two-way mask-transformer decoder (engine extras: MinkowskiEngine has no such layer, and nothing here is pinned to it):

    voxel_attention(x, keys, values, num_heads, attn_mask=None, scale=None) -> a SparseTensor on x's coordinate set;
    MinkowskiVoxelAttention(embed_dim, num_heads, query_channels=None, bias=True): forward(x, queries, attn_mask=None) =
    out_proj(voxel_attention(q_proj(x), k_proj(queries), v_proj(queries))); parameters q_proj, k_proj, v_proj, out_proj
    (nn.Linear; k_proj and v_proj map query_channels to embed_dim)

    out[i, h, :] = sum_q softmax_q(scale * <x[i, h], keys[b, q, h]>) values[b, q, h, :] over the queries q of the row's sample b
    that attn_mask does not block; C = num_heads * D, scale = D ** -0.5 unless given.  x: a SparseTensor; keys, values
    [B, Q, C] with the sample numbering of query_attention (another B is a ValueError).  attn_mask: the same object
    query_attention takes -- bool [V, Q], rows as the caller sees them, True = may NOT attend, one mask for all heads -- so one
    mask serves both legs.  A row whose queries are all blocked is zero, contributes to no gradient and receives none; a (b, q)
    that no row may attend to gets a zero gradient.  csrc/vattn.hip: forward and the backward for x are one loop over the Q
    queries per (held row, head) item -- an online-softmax sweep that saves the log-sum-exp, then the probabilities recomputed
    -- without scratch; the backward for keys and values sweeps the chunks of query_attention (the same
    `chunks` of the same record: no second host read), one partial per chunk, merged in chunk order.  The keys and
    values of a sample are read through the cache.  Nothing of size V x Q is stored, no atomics, every sum in an order fixed
    by the shapes, the same bytes on every run.  D <= 128, Q <= 1024, C <= 1024, B <= 65535.  Frozen keys and values skip their
    pass; a frozen x skips its own when keys and values are frozen too (the kv pass reads a per-row residual the x pass leaves).
    Out of scope (each raises ValueError, TypeError or NotImplementedError naming it): a different Q per sample, float or
    per-head masks, attention dropout, keys.shape != values.shape, float16 / bfloat16, CPU tensors (NotImplementedError naming
    ms3d_vattn_forward).  Outside prepare_conv_weights.

Farthest point sampling per sample -- where the queries of the two blocks above come from, and the grouping stage of a point
network (an engine extra: MinkowskiEngine has no such function, and nothing here is pinned to it):

    farthest_point_sampling(x, num_samples, start=None) -> int64 [B, M]

    x: a SparseTensor (any tensor stride its manager holds; a plain, Morton-sorted or rooted manager) or a TensorField; M =
    num_samples, a Python int >= 1; B the number of batch indices PRESENT, row b for the b-th of them in ascending order (the
    numbering of query_attention, CoordinateManager.batch_rows, origin_map and the global pooling layers; gaps and interleaved
    rows are fine).  The values are rows of x.F / x.C as the caller sees them, on a Morton-sorted manager too: x.F[idx] is
    [B, M, C], ready for MinkowskiQueryAttention, x.C[idx][..., 1:] are the positions.
    The rule, all of it: pick 0 of a sample is start[b] (without `start`: its lowest caller row); pick j is the row whose
    distance to the nearest of the picks 0 .. j-1 is largest; among equal distances the lowest caller row wins; rows already
    picked have distance 0 and take part like any other row.  The result is a pure function of the coordinates: the same
    bytes on every run, whatever order the manager holds its rows in.
    Distances: on a SparseTensor the exact integer dx^2 + dy^2 + dz^2 at the tensor's stride, in unsigned 32-bit arithmetic (up
    to 3 * 32767^2 = 3 221 028 867 over the packable range [-16384, 16384)); on a TensorField its float32 points (float64 is
    taken to float32 first), d = (dx*dx + dy*dy) + dz*dz with dx = p.x - c.x, every operation rounded to float32 on its own, no
    FMA, the running minimum by fminf; finite coordinates are a precondition and are not checked; duplicate points are legal
    (once every remaining distance is 0 the lowest row repeats).
    start: int64 [B] caller rows, one inside each sample (one host read, only when it is given).  ValueError: num_samples that
    is not an int >= 1 or is larger than the smallest sample (naming the sample and its size; the segment lengths are read on
    the host once per coordinate set or field: the record's `lengths`), a start of the wrong shape or dtype,
    for another B or with a row outside its sample, integer coordinates outside the packable range.  An empty tensor gives an
    empty [0, M] result.
    csrc/fps.hip: one launch, one workgroup per sample looping over its own segment of batch_rows, rows read where they are
    held (cm.coords and the record are passed as they are); no atomics and no waiting between workgroups; a
    thread's best row is one 64-bit key, (distance bits << 32) | ~caller row, reduced by shuffles and through LDS, two
    barriers a pick.  A sample of at most ms3d_fps_resident_rows() rows stays in registers for the whole loop; a larger one
    is gathered once into a workspace and swept every pick.  CPU tensors take the same rule as a torch expression, a loop
    of M steps.  The index is not differentiable: gradients reach x.F through x.F[idx] or gather_rows.
    Out of scope: other metrics, feature-space sampling, a different M per sample, float16 or float64 distances, gradients
    with respect to the coordinates; a backend without the kernels raises NotImplementedError naming ms3d_fps_i32 for device
    tensors.  Grouping rows around the picks: knn_query(x, k, idx), below.

k nearest neighbours per sample -- what follows the sampling: grouping rows around the picks, carrying features of M picks
back to all V rows (three-nearest inverse-distance unpooling), kNN graphs for vector attention (an engine extra: MinkowskiEngine
has no such function, and nothing here is pinned to it):

    knn_query(x, k, queries=None, max_squared_distance=None) -> (idx int64 [..., k], d2 [..., k])

    x, the support set: a SparseTensor (any tensor stride its manager holds; a plain, Morton-sorted or rooted manager) or a
    TensorField; k a Python int, 1 <= k <= 64 (ms3d_knn_max_k()).  queries: None -- every row of x queries its own sample,
    [V, k], row i answers caller row i; an int64 tensor [B, M] of caller rows of x, exactly what farthest_point_sampling
    returns (row b inside the b-th batch index present; duplicates are legal; one host read to check it, only for this form) --
    [B, M, k]; or another tensor y of the same kind (SparseTensor with SparseTensor, strides and managers may differ, or
    TensorField with TensorField): every row of y queries the sample of x with the same batch index VALUE, [V_y, k] in y's
    caller row order (a batch index of y that x lacks is a ValueError naming it, samples of x without queries are fine,
    mixed kinds are a TypeError).
    The rule, all of it: for a query at position p in sample b, the k rows of sample b of x with the smallest keys (distance
    to p, caller row of x), in ascending key order; among equal distances the lowest caller row comes first; a query that is
    itself a row of x finds itself first, at distance 0.  A pure function of the coordinates: the same bytes on every run,
    whatever order the manager holds its rows in.  The values are rows of x.F / x.C as the caller sees them: x.F[idx] is
    [..., k, C].
    Distances are farthest_point_sampling's: on a SparseTensor the exact integer dx^2 + dy^2 + dz^2 in unsigned 32-bit
    arithmetic over the packable range [-16384, 16384) of both sets, returned as int64 (it reaches 3 221 028 867); on a
    TensorField float32, d = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x, every operation rounded on its own, no FMA, returned
    as float32.  max_squared_distance: a Python int (SparseTensor) or float (TensorField, taken to float32) >= 0; a row
    qualifies when d2 <= cap, the boundary included; slots nothing qualifies for hold idx = -1 and d2 = -1 / +inf, after all
    the qualifying slots -- mask before indexing.  Without a cap the result never contains -1.
    ValueError: k out of range or larger than the smallest sample of x that has queries (naming it; from the record's cached
    `lengths`), a cap of the wrong type or negative, a bad [B, M] tensor, coordinates outside the packable range, more
    than 65535 samples.  Empty x or queries give empty [0, k] / [B, 0, k] results.
    csrc/knn.hip: the support set is read where it is held (cm.coords and the record as they are) and packed
    once in segment order, 16 B a row; then one workgroup takes ms3d_knn_queries_per_group() queries of one sample, a thread a
    query, and streams the sample through LDS in tiles of ms3d_knn_rows_per_tile() rows.  A thread's list of its k smallest 64-bit
    keys, (distance bits << 32) | caller row, lives in LDS; candidates are held back and inserted by all lanes of a wave
    together.  No atomics, no waiting between workgroups, every loop counted.  CPU tensors take the same rule as a torch
    expression, at most 2^22 (query, row) pairs at a time.  The index is not differentiable; gradients reach x.F through
    x.F[idx].
    Out of scope: spatial acceleration (a grid or hash walk), mixed voxel / point queries (pooling, weighted
    sums and interpolation over the index: knn_map and neighbor_pool / neighbor_sum / knn_interpolate, below), other metrics, a different k per query, k above 64, float16 or float64 distances, gradients with respect
    to the coordinates, a ball query's first-k-inside-the-radius order; a backend without the kernels raises
    NotImplementedError naming ms3d_knn_i32 for device tensors.

Pooling and weighted sums over a neighbour index -- what a kNN index is used for: max over the k neighbours of a pick (the
"down" block of an FPS + kNN network), inverse-distance interpolation of M picks back onto all rows (the "up" block), scalar
attention over a kNN graph once the caller has taken a softmax over [N, k] (an engine extra, nothing of MinkowskiEngine's):

    knn_map(x, k, queries=None, max_squared_distance=None) -> NeighborMap
    NeighborMap.from_index(idx, num_rows, d2=None) -> NeighborMap
    neighbor_pool(x, nmap, mode="max")          mode: "max" | "avg" | "sum"
    neighbor_sum(x, nmap, weights)              weights float32 [..., k]
    knn_interpolate(x, nmap, eps=1e-8)

    A NeighborMap (backend.NeighbourGroup) is the record of one index, built once and shared by every op and layer over the
    same graph: idx and d2 as given, N, k (1 <= k <= 254: a slot number fits a byte), V, idx_held int64 [N, k] -- the index in
    the rows as the support and the target set HOLD them, translated once by torch gathers, so features are read and written
    where they lie (no permuted copy of x.F) --, valid int32 [N], and on first use the transposed table (entry_sorted,
    seg_start: the entries e = n * k + j grouped by support row, ascending e in the caller's numbering of the queries, one
    stable sort) and -- only when a feature
    gradient runs on the device -- the chunk list (chunk_start, n_chunks; one host read).  knn_map runs knn_query with the
    same arguments and remembers the support (x's coordinate set or field) and the target: x itself (queries=None), y, or
    none for an int64 [B, M] tensor of picks (results are then plain [B, M, C]).  from_index wraps a hand-made int64 index
    [..., k] over plain rows [num_rows, C]; a negative value means no neighbour and may sit in any slot; another dtype, a
    value >= num_rows or k > 254 is a ValueError (one host read, once).  An op given a map and an x of another set or
    another number of rows refuses on the host (ValueError); x is the SparseTensor / TensorField the map was made for or, for
    from_index maps, a float32 tensor [V, C]; the result is a SparseTensor / TensorField on the target's set, or a tensor.
    The rules, all of them, over the slots with idx >= 0 in ascending slot: sum -- the chain of float32 additions from 0;
    avg -- that sum divided once by float(valid[n]), a query without a valid slot exact zeros; max -- per channel the first
    valid slot, then every strictly greater one (the lowest slot wins ties, a NaN wins only from the first slot), a query
    without a valid slot zeros; neighbor_sum -- one fmaf per slot and element from 0, the weight of an invalid slot is never
    read, a single neighbour of weight 1 returns that row bit for bit; knn_interpolate -- r = 1 / (float32(d2) + eps),
    w = r / sum_j r over the valid slots, a torch expression on [N, k] that is not differentiable, then neighbor_sum (a map
    without d2: ValueError).  Gradients: to the features, per support row the sum over its entries in ascending e of dout[n]
    (sum), dout[n] / float(valid[n]) (avg), w[n, j] * dout[n] (one fmaf), dout[n, c] where the saved slot is j (max) -- a row
    of more than ms3d_nbr_chunk_entries() entries is cut into chunks of that many, each summed the same way into a partial,
    the partials added in chunk order; to the weights (neighbor_sum) dw[n, j] = <dout[n], x[idx[n, j]]>, 0 for an invalid
    slot; none to idx, d2 or the coordinates.  A frozen x skips the feature pass (the chunk list is then never built), frozen
    weights the weight pass.  csrc/neighbor.hip: gathers with one writer per element, no atomics, the same bytes on every run;
    nothing of size [N, k, C] is ever made.  CPU tensors take the same rules as torch expressions (x[idx.clamp(min=0)]
    masked, then reduced in slot order).  Modules without parameters: MinkowskiKNNPooling(k, mode="max") -- forward(x,
    queries=None, nmap=None) -- and MinkowskiKNNInterpolation(k=3, eps=1e-8) -- forward(x, y, nmap=None).
    Out of scope (each raises where it can be asked for): per-head or per-channel weights [N, k, H] in neighbor_sum (multi-head
    softmax attention over the slots: neighbor_attention, below), vector attention itself, a fused x_j - x_i /
    relative-position edge feature, a materialising differentiable
    [N, k, C] gather with masked slots, float16 / bfloat16 rows, k above 254, gradients with respect to coordinates or
    distances, mixed voxel / point maps (knn_query refuses them); a backend without the kernels raises NotImplementedError
    naming ms3d_nbr_pool_forward for device tensors.

Multi-head attention over a neighbour index -- the local self-attention of a point or voxel transformer over its k nearest rows,
the cross-attention of picks over their groups; the block the FPS + kNN layers exist to feed (an engine extra, nothing of
MinkowskiEngine's):

    neighbor_attention(q, k, v, nmap, num_heads, bias=None, scale=None)
    MinkowskiNeighborAttention(in_channels, num_heads, k=16, qkv_bias=True, pos_bias=True, pos_hidden=16)
    NeighborMap.relative_positions()          # float32 [..., k, 3]

    The rule, all of it: out[n, h, :] = sum_j softmax_j(scale * <q[n, h], k[i, h]> + bias[n, j, h]) v[i, h, :] over the slots j
    of query n with i = idx[n, j] >= 0, in ascending slot; C = num_heads * D, scale = D ** -0.5 unless given; the maximum is
    always subtracted before exp; a query without a valid slot is exact zeros, contributes to no gradient and receives none;
    a query with a single valid slot returns that v row bit for bit.
    k and v, the support: SparseTensors or TensorFields on the set the map was made for, or float32 [V, C] for a from_index
    map; both of the same kind and set, with the same C.  q lives on the map's TARGET: the support's own set (queries=None),
    y's set (a tensor y), or a plain float32 tensor [..., C] in the shape of the index's leading dimensions ([B, M] picks, a
    from_index map).  The record knows its target beside its support (`target`, a keyword of the record that defaults to "not
    checked"; knn_map and from_index fill it): a q on another set, or with another row count, is a ValueError on the host.
    bias: float32 [..., k, num_heads] in the caller's numbering of the queries, differentiable; the value of an invalid slot is
    never read and its gradient is 0; where the target holds its rows in another order it is permuted once (PermuteRowsFn), as
    neighbor_sum permutes its weights.  The result is a SparseTensor / TensorField on the target's set, or a plain [..., C]
    tensor.  Gradients go to q, k, v and bias; none to idx, d2 or the coordinates.  Frozen k and v skip their pass (the
    transposed table and the chunk list are then never built); frozen q and bias skip theirs only when k and v are frozen
    too, because the kv pass reads the per-row residual delta the q pass leaves (csrc/attn_core.h).
    NeighborMap.relative_positions(): float32 [..., k, 3], the position of support row idx[n, j] minus the position of query
    n -- integer coordinates cast to float32 (coordinate units) for voxels, the field's float32 points for points --, zeros in
    the invalid slots, in the caller's numbering, not differentiable; made on first use by torch gathers of the three
    coordinate columns and kept (knn_map remembers references to the position tensors of both sides, no copies); a
    from_index map has none: ValueError.  It is the only input a position bias needs, and 3 channels wide, so it stays torch.
    MinkowskiNeighborAttention: forward(x, nmap=None) = proj(neighbor_attention(q, k, v, nmap, num_heads, bias)) over
    knn_map(x, k) or a given map (its k wins), (q, k, v) the column blocks of qkv(x); `qkv` nn.Linear(C, 3C), `proj`
    nn.Linear(C, C), and with pos_bias `pos` = Sequential(Linear(3, pos_hidden), ReLU, Linear(pos_hidden, num_heads)) applied
    to relative_positions(), its last layer zero-initialised so the block starts as plain attention.  Outside
    prepare_conv_weights, like the other attention blocks.
    csrc/nattn.hip on csrc/attn_core.h: three gathers with one writer per element, float32, rows read where they are held, no
    atomics, every sum in an order fixed by the shapes and the index -- the same bytes on every run and whether the managers
    hold their rows Morton-sorted or not.  Forward and the q pass: one group of lanes per (query, head), the slots four at a
    time; dbias [N, k, H] is stored by the q pass after its sweep from the bits of p and e it stashed in LDS.  The kv pass
    walks the record's transposed table per (support row, head); a row of more than ms3d_nbr_chunk_entries() entries goes
    through the record's chunk list and a workspace of two partial rows per chunk.  Nothing of size [N, k, C] is made.  CPU
    tensors (float32 or float64) take the same rule as a torch expression over the masked [N, k, C] gather, with autograd's
    backward.
    Refusals, each naming neighbor_attention: C % num_heads != 0, num_heads < 1, D > 128 (ValueError; k > 254 is the
    record's), a bias of another shape, dtype or device, mixed k / v kinds or sets (ValueError), float16 / bfloat16 rows
    (NotImplementedError); a backend without the kernels raises NotImplementedError naming ms3d_nattn_forward for device
    tensors.
    Out of scope: vector attention (per-channel weights from an MLP), a value-side position term v_j + delta_ij, attention
    dropout, a value head dimension different from D, gradients to positions.

Not supported (each raises NotImplementedError naming it): `axis_types` of a KernelGenerator, a region of more than 254
offsets, a dense grid of more than 2^31 - 1 cells, to_sparse of a tensor
that is not 5-D ([B, C, X, Y, Z]: dimension 3) or in a format other than "BCXXX" / "BXXXC", dense() on a per-axis tensor stride, strides other than 1 and 2, a generative layer at stride 2 on an odd
tensor stride, MinkowskiConvolutionTranspose onto a coordinate set that is not cached when neither `coordinates=` nor
expand_coordinates says where to, expand_coordinates on a stride-2 MinkowskiConvolution, forward pooling that creates
coordinates, `+=` and ME.cat across different coordinate sets, a union of more than 16 tensors,
the `quantization_mode` argument of SparseTensor itself (quantise with a field), interpolation gradients with respect to the
coordinates, pooling transpose at strides other than 1 and 2 or (without `coordinates=` / expand_coordinates) onto a set that is not
cached, dimension != 3, per-axis kernel
tuples; and, as ValueError, an even HYPER_CROSS kernel size and a CUSTOM region with dilation != 1.

Module/parameter names match ME so reference state_dicts keep their keys (`kernel`, `bn.weight`, ...).
"""
from . import utils  # noqa: F401
from .tensor import SparseTensor, CoordinateManager, CoordinateMapKey, cat, prefetch_coordinates  # noqa: F401
from .tensor import TensorField, SparseTensorQuantizationMode  # noqa: F401
from .tensor import to_sparse, to_sparse_all  # noqa: F401
from .tensor import RegionType, KernelGenerator  # noqa: F401
from .tensor import farthest_point_sampling  # noqa: F401  (engine extra: the seeds of the attention blocks' queries)
from .tensor import knn_query  # noqa: F401  (engine extra: the k nearest rows of a query's own sample)
from .tensor import knn_map, NeighborMap  # noqa: F401  (engine extra: a neighbour index as a record the ops below read)
from .functional import neighbor_pool, neighbor_sum, knn_interpolate  # noqa: F401  (engine extra: csrc/neighbor.hip)
from .functional import neighbor_attention  # noqa: F401  (engine extra: csrc/nattn.hip)
from .modules import (MinkowskiConvolution, MinkowskiConvolutionTranspose, MinkowskiBatchNorm,  # noqa: F401
                      MinkowskiReLU, prepare_conv_weights, release_conv_weights,
                      MinkowskiMaxPooling, MinkowskiAvgPooling, MinkowskiSumPooling, MinkowskiGlobalMaxPooling,
                      MinkowskiGlobalAvgPooling, MinkowskiGlobalSumPooling, MinkowskiLinear, MinkowskiDropout,
                      MinkowskiGenerativeConvolutionTranspose, MinkowskiPruning,
                      MinkowskiUnion, MinkowskiBroadcastAddition, MinkowskiBroadcastMultiplication,
                      MinkowskiBroadcastConcatenation, MinkowskiBroadcast, MinkowskiSigmoid,
                      MinkowskiPoolingTranspose, MinkowskiInterpolation, MinkowskiChannelwiseConvolution,
                      MinkowskiInstanceNorm, MinkowskiStableInstanceNorm,
                      MinkowskiKernelAttention, kernel_attention, MinkowskiQueryAttention, query_attention,
                      MinkowskiVoxelAttention, voxel_attention, MinkowskiKNNPooling, MinkowskiKNNInterpolation,
                      MinkowskiNeighborAttention,
                      MinkowskiToSparseTensor, MinkowskiToDenseTensor, MinkowskiToFeature,
                      MinkowskiELU, MinkowskiLeakyReLU, MinkowskiPReLU, MinkowskiSELU, MinkowskiCELU, MinkowskiGELU,
                      MinkowskiSiLU, MinkowskiTanh, MinkowskiSoftplus, MinkowskiHardswish, MinkowskiHardtanh,
                      MinkowskiReLU6, MinkowskiSoftmax, MinkowskiLogSoftmax)
from .tensor import kernel_offsets  # noqa: F401  (engine extra: the offset list of a kernel, in weight order)
from .functional import gather_rows  # noqa: F401  (engine extra: x[idx] with a scatter-add backward)
from .functional import SkipLink  # noqa: F401  (engine extra: a residual block's skip gradient, see functional.py)
