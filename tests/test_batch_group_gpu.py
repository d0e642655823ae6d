"""The batch grouping record on the device: the five per-sample ops of one tensor stand on ONE BatchGroup per coordinate set
(and one per field), a second round of calls builds nothing new and gives the same bytes, and the backend refuses a record made
for other rows on the host, before anything is launched."""
import numpy as np
import pytest
import torch

from fps_ref import random_voxels

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, H, Q = 8, 2, 5
# the set of the FPS and kNN tests (too few rows for the manager to reorder them), and one large enough to be held in Morton order
SETS = {"gaps": [70, 9, 300], "gaps, Morton order": [3900, 9, 300]}


@pytest.fixture(scope="module")
def ME():
    import minsu3d_amd.MinkowskiEngine as me
    return me


def _round(ME, x, feats, norm, queries):
    """the five ops once each, forward and backward where there is one -> everything they returned"""
    out = []
    for leaf in (feats, queries, norm.weight, norm.bias):
        leaf.grad = None
    y = norm(x)
    y.F.square().sum().backward()
    out += [y.F, feats.grad.clone(), norm.weight.grad.clone()]
    feats.grad = None
    refined = ME.query_attention(queries, x, x, H)
    refined.square().sum().backward()
    out += [refined, feats.grad.clone(), queries.grad.clone()]
    feats.grad = queries.grad = None
    z = ME.voxel_attention(x, queries, queries, H)
    z.F.square().sum().backward()
    out += [z.F, feats.grad.clone(), queries.grad.clone()]
    idx = ME.farthest_point_sampling(x, 4)
    out += [idx, *ME.knn_query(x, 4, idx)]
    return [t.detach() for t in out]


def _built(g):
    return {name: id(value) for name, value in vars(g).items()}


@pytest.mark.parametrize("name", list(SETS))
def test_five_ops_stand_on_one_record(ME, name):
    coords = random_voxels(SETS[name], seed=9, side=12, batch_indices=[0, 2, 5])
    V = coords.shape[0]
    c = torch.from_numpy(coords).to(DEV)
    cm = ME.CoordinateManager(c, spatial_sort=True)
    assert (cm.perm is not None) == (name != "gaps")
    torch.manual_seed(3)
    feats = torch.randn(V, C, device=DEV).requires_grad_(True)
    x = ME.SparseTensor(feats, coordinate_manager=cm)
    queries = torch.randn(3, Q, C, device=DEV).requires_grad_(True)
    norm = ME.MinkowskiInstanceNorm(C).to(DEV)
    field = ME.TensorField(torch.randn(V, 2, device=DEV), torch.cat([c[:, :1].float(), c[:, 1:].float() * 0.25], 1))
    assert cm._batch_groups == {}

    first = _round(ME, x, feats, norm, queries)
    f_first = [ME.farthest_point_sampling(field, 4), *ME.knn_query(field, 4, field)]
    assert list(cm._batch_groups) == [1]
    g, fg = cm.batch_group(1), field._batch_group()
    assert (g.V, g.B, g.lengths, g.indices) == (V, 3, tuple(SETS[name]), (0, 2, 5)) and (g.row_map is not None) == (name != "gaps")
    assert cm.batch_chunks(1) is g.chunks and cm.batch_lengths(1) is g.lengths and cm.batch_segments(1) is g.seg_of_row
    assert cm.caller_rows(1) is g.row_map and cm.batch_rows(1)[0] is g.order and cm.batch_rows(1)[2] is g.seg_start
    assert fg.lengths == g.lengths and fg.indices == (0, 2, 5) and fg.row_map is None and "chunks" not in vars(fg)
    assert all(bool(torch.isfinite(t).all()) for t in first if t.is_floating_point())
    assert torch.from_numpy(coords[:, 0]).long()[first[9].cpu()].tolist() == [[0] * 4, [2] * 4, [5] * 4]

    built, f_built = _built(g), _built(fg)
    second = _round(ME, x, feats, norm, queries)
    f_second = [ME.farthest_point_sampling(field, 4), *ME.knn_query(field, 4, field)]
    assert cm.batch_group(1) is g and list(cm._batch_groups) == [1] and field._batch_group() is fg
    assert _built(g) == built and _built(fg) == f_built                 # nothing new, nothing rebuilt
    for a, b in zip(first + f_first, second + f_second):
        assert torch.equal(a, b)


def test_a_stale_record_is_refused_on_the_host(ME):
    from minsu3d_amd.backend import get_backend
    be = get_backend()
    coords = random_voxels([70, 9, 300], seed=9, side=12, batch_indices=[0, 2, 5])
    V = coords.shape[0]
    c = torch.from_numpy(coords).to(DEV)
    group = ME.CoordinateManager(c).batch_group(1)
    stale = ME.CoordinateManager(c[:-5].contiguous()).batch_group(1)                      # another V
    merged = c.clone()
    merged[:, 0] = merged[:, 0].clamp(max=2)
    fewer = ME.CoordinateManager(merged).batch_group(1)                                   # the same V, another B
    on_host = ME.CoordinateManager(torch.from_numpy(coords)).batch_group(1)               # another device
    assert (stale.V, stale.B, fewer.V, fewer.B) == (V - 5, 3, V, 2) and not on_host.order.is_cuda
    x, dy = torch.randn(V, C, device=DEV), torch.randn(V, C, device=DEV)
    q = torch.randn(3, Q, C, device=DEV)
    lse_q, lse_x = torch.zeros(3, Q, H, device=DEV), torch.zeros(V, H, device=DEV)
    stat = torch.zeros(3, C, dtype=torch.float64, device=DEV)
    words = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
    q_start = torch.tensor([0, 4, 4, 4], dtype=torch.int32, device=DEV)
    calls = {
        "inorm_forward": lambda g: be.inorm_forward(x, g, 1e-5, None, None),
        "inorm_backward": lambda g: be.inorm_backward(dy, x, g, stat, stat, None),
        "qattn_forward": lambda g: be.qattn_forward(q, x, x, None, g, H, 0.5),
        "qattn_backward_q": lambda g: be.qattn_backward_q(q, x, x, None, g, q, lse_q, q, H, 0.5),
        "qattn_backward_kv": lambda g: be.qattn_backward_kv(q, x, x, None, g, q, lse_q, lse_q, q, H, 0.5),
        "vattn_forward": lambda g: be.vattn_forward(x, q, q, None, g, H, 0.5),
        "vattn_backward_x": lambda g: be.vattn_backward_x(x, q, q, None, g, x, lse_x, dy, H, 0.5),
        "vattn_backward_kv": lambda g: be.vattn_backward_kv(x, q, q, None, g, x, lse_x, lse_x, dy, H, 0.5),
        "fps": lambda g: be.fps(c, g, None, 2),
        "knn": lambda g: be.knn(c, g, words, q_start, 4, 2, None),
    }
    for name, call in calls.items():
        for bad in (stale, on_host):
            with pytest.raises(AssertionError):
                call(bad)
        if "attn" in name:
            with pytest.raises(AssertionError):
                call(fewer)
    torch.cuda.synchronize()
    # the record made for these rows is taken by every one of them
    for name in ("inorm_forward", "qattn_forward", "vattn_forward", "fps", "knn"):
        calls[name](group)
    torch.cuda.synchronize()
