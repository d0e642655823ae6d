"""seeded inputs for the segment-reduction / IoU parity tests (CPU: the oracle against a numpy transcription, GPU: the HIP
kernels against the oracle).  Plain numpy: segment lengths pinned to the tile, unroll and route edges of
csrc/segment_ops.hip, proposal counts past every grid cap, special float values, crafted IoU matrices."""
import numpy as np

# ---- the kernels' constants, each stated once (the line it mirrors in minsu3d_amd/csrc)
WAVES_PER_BLOCK = 4        # segment_ops.hip:19   a wave kernel's block owns 4 proposals
MAX_C_STAGE = 64           # segment_ops.hip:20   channels staged per pass of seg_serial_sum_kernel
SUM_TILE_FLOATS = 2048     # segment_ops.hip:32   TF: a tile holds 2048 // cw rows of a cw-channel stage (:40)
SUM_UNROLL = 8             # segment_ops.hip:74   adds per unrolled group
SUM3_TILE_ROWS = 256       # segment_ops.hip:103  RT of seg_serial_sum3_kernel (C = 3)
SUM3_UNROLL = 32           # segment_ops.hip:141  adds per unrolled group
WAVE = 64                  # segment_ops.hip:202  the row stride of a lane in seg_extreme_kernel's general path
BLOCK_WAVES = 8            # segment_ops.hip:248  step = 8 * rstep: the 8 waves of seg_extreme_block_kernel
BLOCK_UNROLL = 8           # segment_ops.hip:250  loads in flight per lane -> 64 * rstep rows per unrolled step
WAVE_GRID_CAP = 4096       # segment_ops.hip:550  grid_for: the wave kernels stride after 4096 * 4 proposals
BLOCK_GRID_CAP = 4096      # segment_ops.hip:571  the block kernel strides after 4096 proposals
PV_GRID_CAP = 2048         # segment_ops.hip:685  pv_params_kernel
IOU_THREADS = 256          # iou.hip:14
MAX_LDS_BINS = 12288       # iou.hip:15           more instances -> tiled histogram passes
IOU_GRID_CAP = 8192        # iou.hip:121, :150    iou_kernel and mask_label_kernel

MANY_SHORT_P = WAVE_GRID_CAP * WAVES_PER_BLOCK + 37     # past every cap above in one input


def channel_stages(C):
    """the channel widths cw of seg_serial_sum_kernel's passes over a C-channel row (segment_ops.hip:38-39)"""
    return [min(MAX_C_STAGE, C)] + ([C % MAX_C_STAGE] if C > MAX_C_STAGE and C % MAX_C_STAGE else [])


def is_pow2_route(C):
    """C takes a (row slot, channel) lane layout: seg_extreme_kernel's pow2 path or the block kernel (:168, :551)"""
    return C & (C - 1) == 0 and C <= 64


def rstep(C):
    return 64 // C if is_pow2_route(C) else 1


def edge_lengths(C):
    """(tile edges, unroll edges) of every kernel a C-channel input goes through"""
    tiles, unrolls = set(), {WAVE}
    if C == 3:
        tiles.add(SUM3_TILE_ROWS); unrolls.add(SUM3_UNROLL)
    else:
        unrolls.add(SUM_UNROLL)
        for cw in channel_stages(C):
            tiles.add(SUM_TILE_FLOATS // cw)
    if is_pow2_route(C):
        unrolls.update((rstep(C), BLOCK_WAVES * rstep(C)))
        tiles.add(BLOCK_WAVES * BLOCK_UNROLL * rstep(C))
    return sorted(tiles), sorted(unrolls)


def edge_offsets(C, seed=0):
    """i32 offsets (from 0) of segments whose lengths sit on the edges above: E-1, E, E+1 for every edge, 2E-1, 2E, 2E+1
    and 3E+1 for a tile edge (the double buffer needs three tiles), the lengths 0, 1, 2 and two adjacent empty segments;
    in a seeded shuffled order"""
    tiles, unrolls = edge_lengths(C)
    lens = {0, 1, 2}
    for E in tiles + unrolls:
        lens.update((E - 1, E, E + 1))
    for E in tiles:
        lens.update((2 * E - 1, 2 * E, 2 * E + 1, 3 * E + 1))
    lens = np.array(sorted(lens), np.int64)
    rng = np.random.default_rng(1000 * C + seed)
    rng.shuffle(lens)
    at = int(rng.integers(0, lens.size + 1))
    lens = np.concatenate([lens[:at], [0, 0], lens[at:]])
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def many_short_offsets(P, seed=0):
    """P segments of 0 to 4 rows"""
    lens = np.random.default_rng(seed + P).integers(0, 5, P)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _distinct_rows(rng, draw):
    while True:
        rows = draw()
        if len(set(int(r) for r in rows)) == len(rows):
            return rows


def special_values(x, off, rng):
    """a copy of the rows x with, per channel, a duplicated maximum and a duplicated minimum in the two longest
    segments (at least 64 * rstep rows apart in the longest, in adjacent rows in the second) and six further segments
    of at least 4 rows turned into: a constant, +0.0 / -0.0 only, +inf and -inf entries, a few NaN among finite values,
    all NaN, all -inf.  -> (rows, {name: segment index})"""
    x = np.array(x, np.float32, copy=True)
    C = x.shape[1]
    off = np.asarray(off, np.int64)
    lens = np.diff(off)
    order = np.argsort(-lens, kind="stable")
    far, near = int(order[0]), int(order[1])
    gap = 64 * rstep(C)
    assert lens[far] >= gap + 4 and lens[near] >= 8

    def far_rows():                      # (first, second) row of the maximum pair, then of the minimum pair
        a = rng.integers(0, lens[far] - gap, 2)
        b = a + gap + rng.integers(0, lens[far] - gap - a)
        return [a[0], b[0], a[1], b[1]]

    def near_rows():
        a = rng.integers(0, lens[near] - 1, 2)
        return [a[0], a[0] + 1, a[1], a[1] + 1]

    for seg, draw in ((far, far_rows), (near, near_rows)):
        s, e = off[seg], off[seg + 1]
        for c in range(C):
            r = s + np.array(_distinct_rows(rng, draw))
            col = x[s:e, c]
            hi, lo = col.max() + np.float32(1), col.min() - np.float32(1)
            x[r[:2], c] = hi
            x[r[2:], c] = lo
    pool = [int(p) for p in order[2:] if lens[p] >= 4]
    picks = [pool[i] for i in rng.choice(len(pool), 6, replace=False)]
    names = ("constant", "zeros", "inf", "some_nan", "all_nan", "all_neg_inf")
    where = dict(zip(names, picks), dup_far=far, dup_near=near)
    even = np.arange(C) % 2 == 0
    for name, p in zip(names, picks):
        s, e = off[p], off[p + 1]
        n = e - s
        if name == "constant":
            x[s:e] = x[s]
        elif name == "zeros":
            x[s:e] = np.where(rng.random((n, C)) < 0.5, np.float32(0.0), np.float32(-0.0))
            x[s] = np.where(even, np.float32(-0.0), np.float32(0.0))        # both orders of the first two rows
            x[s + 1] = np.where(even, np.float32(0.0), np.float32(-0.0))
        elif name == "inf":
            x[s] = np.where(even, np.inf, -np.inf)                           # every channel holds both, in both orders
            x[s + 1] = np.where(even, -np.inf, np.inf)
            x[e - 1] = np.where(rng.random(C) < 0.5, np.inf, -np.inf)
        elif name == "some_nan":
            m = rng.random((n, C)) < 0.2
            m[0], m[1], m[2] = even, False, ~even                            # a NaN and a finite value per channel,
            x[s:e][m] = np.nan                                               # NaN in the first row of every other one
        elif name == "all_nan":
            x[s:e] = np.nan
        else:
            x[s:e] = -np.inf
    return x, where


def shifted(x, off, front=7, back=5, sentinel=np.inf):
    """the same segments behind `front` rows (and in front of `back` rows) that hold `sentinel`: offsets[0] = front"""
    C = x.shape[1]
    pad = lambda n: np.full((n, C), sentinel, np.float32)
    return np.concatenate([pad(front), x, pad(back)]), (np.asarray(off) + front).astype(np.int32)


# ---------------------------------------------------------------------------------------------- IoU family
def iou_inputs(I, off, N, seed):
    """prop_idx, int16 instance labels in [-1, I), instance point counts and sigmoid values (0.5 exactly and the next
    float above it among them) for proposals with the offsets `off`.  The points 0 .. 4 carry the labels I-1,
    min(I-1, MAX_LDS_BINS), min(I-1, MAX_LDS_BINS-1), 0 and -1 and lead every proposal of 5 and more points."""
    rng = np.random.default_rng(seed)
    inst = rng.integers(-1, I, N).astype(np.int16)
    inst[:5] = [I - 1, min(I - 1, MAX_LDS_BINS), min(I - 1, MAX_LDS_BINS - 1), 0, -1]
    pn = np.bincount(inst[inst >= 0], minlength=I).astype(np.int32)
    S = int(off[-1])
    pidx = rng.integers(0, N, S).astype(np.int32)
    for p in range(len(off) - 1):
        if off[p + 1] - off[p] >= 5:
            pidx[off[p]:off[p] + 5] = np.arange(5)
    sig = rng.random(S).astype(np.float32)
    k = rng.random(S)
    sig[k < 0.1] = np.float32(0.5)
    sig[k > 0.9] = np.nextafter(np.float32(0.5), np.float32(1))
    return pidx, inst, pn, sig


TILED_IOU_SIZES = [0, 1, 300, 5000, 255, 256, 257, 12289, 2]       # P = 9


def sizes_to_offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- mask labels
MASK_LABEL_I = (1, 64, 65, 256, 257, 1000)
IGNORED = -1


def mask_label_cases():
    """crafted f32 IoU matrices for get_mask_label: a list of dicts with I, iou [P, I], inst_cls [I], thr, and per row
    the index that must be chosen (`want`) and whether anything may be written (`written`)"""
    cases = []
    for I in MASK_LABEL_I:
        rng = np.random.default_rng(I)
        base = lambda: (rng.random(I) * 0.5).astype(np.float32)      # background strictly below the maxima
        top = np.float32(0.75)
        # -- ties: the smaller index wins.  Thread t owns the indices t, t + 256, ...; a wave is 64 threads.
        k = 3 if I > 67 and I != IOU_THREADS + 1 else 0
        rows, want, names = [np.zeros(I, np.float32)], [0], ["zeros"]
        for name, a, b in (("next_wave", k, k + 64), ("next_stripe", k, k + IOU_THREADS),
                           ("later_stripe_of_lower_thread", k + 1, k + IOU_THREADS)):
            if b < I:
                r = base(); r[[a, b]] = top
                rows.append(r); want.append(a); names.append(name)
        cls = rng.integers(0, 18, I).astype(np.int16)
        if I >= 64:                                                  # the first maximum is ignored: the next one wins
            r = base(); r[[10, 20]] = top
            cls[10] = IGNORED
            rows.append(r); want.append(20); names.append("first_ignored")
        cases.append(dict(name=f"ties_I{I}", I=I, iou=np.stack(rows), inst_cls=cls, thr=np.float32(0.25), want=want,
                          written=[n != "zeros" for n in names], rows=names))
        # the same at threshold 0: the all-zero row is written too (0 >= 0), with index 0
        cases.append(dict(cases[-1], name=f"ties_thr0_I{I}", thr=np.float32(0.0), written=[True] * len(rows)))
        # -- every class ignored: best stays 0 / index 0
        r = base(); r[I - 1] = top
        cases.append(dict(name=f"all_ignored_I{I}", I=I, iou=r[None].copy(), inst_cls=np.full(I, IGNORED, np.int16),
                          thr=np.float32(0.0), want=[0], written=[True], rows=["all_ignored"]))
        cases.append(dict(cases[-1], name=f"all_ignored_thr_I{I}", thr=np.float32(0.05), written=[False]))
        # -- the threshold: >= writes, one ulp below writes nothing
        thr = np.float32(0.3)
        j = I - 1
        r0 = np.minimum(base(), np.float32(0.2)); r0[j] = thr
        r1 = r0.copy(); r1[j] = np.nextafter(thr, np.float32(0))
        cases.append(dict(name=f"threshold_I{I}", I=I, iou=np.stack([r0, r1]),
                          inst_cls=np.full(I, 3, np.int16), thr=thr, want=[j, j], written=[True, False],
                          rows=["at_threshold", "ulp_below"]))
    return cases


def mask_label_points(case):
    """proposals for a case: every proposal lists one point of every instance label (so the winning and the losing
    labels are both among its points) and one unlabelled point.  -> prop_idx, prop_off, inst_labels"""
    I, P = case["I"], case["iou"].shape[0]
    inst = np.concatenate([np.arange(I), [-1]]).astype(np.int16)
    pidx = np.tile(np.arange(I + 1, dtype=np.int32), P)
    off = (np.arange(P + 1) * (I + 1)).astype(np.int32)
    return pidx, off, inst


def mask_label_expected(case):
    """what the crafted rows must give, from the construction alone (no loop over the matrix)"""
    I, P = case["I"], case["iou"].shape[0]
    ml = np.zeros(P * (I + 1), bool); mlm = np.zeros(P * (I + 1), bool)
    for p in range(P):
        if case["written"][p]:
            mlm[p * (I + 1):(p + 1) * (I + 1)] = True
            ml[p * (I + 1) + case["want"][p]] = True
    return ml, mlm
