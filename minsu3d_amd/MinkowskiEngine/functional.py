"""autograd glue around the engine kernels.  Two functions carry the whole backbone:

  SparseConvFn : y = conv(act(x)),  act = the (lazy) BatchNorm[+ReLU] in front of the convolution, applied in the
                 gather.  Backward = one backward-data launch whose epilogue applies the ReLU mask and collects the
                 BN-backward channel sums, one elementwise BN-backward pass, one backward-weight launch.
  BNActFn      : stand-alone BN(+ReLU) for tensors whose consumer is not a convolution.
"""
import contextlib
import threading

import torch

from ..backend import NBR_MODES, NBR_WEIGHTED, NeighbourGroup, get_backend

# ---- matmul precision of the convolutions (torch.set_float32_matmul_precision)
# "highest" = float32 grade everywhere; "high" / "medium" let the wide layers' bf16 kernels keep two / one of the three
# bf16 pieces of each operand (csrc/spconv.hip, include/minsu3d_hip.h: the *_p entry points).  A forward pass reads the
# switch ONCE (GeneralModel.__call__, or every convolution called outside a model forward) and its autograd nodes keep
# that value for their backward, whatever the switch says by then.
PRECISION_CODES = {"highest": 0, "high": 1, "medium": 2}
_pass = threading.local()


def precision_code(name):
    """torch.get_float32_matmul_precision() string -> the C ABI's code (0 highest, 1 high, 2 medium)"""
    try:
        return PRECISION_CODES[name]
    except KeyError:
        raise ValueError(f"unknown float32 matmul precision {name!r}") from None


@contextlib.contextmanager
def pass_precision(code):
    """every convolution inside the block runs at `code` (GeneralModel.__call__: one read of the switch per forward)"""
    prev = getattr(_pass, "code", None)
    _pass.code = code
    try:
        yield
    finally:
        _pass.code = prev


def conv_precision(be=None):
    """the precision code a convolution forward runs at: the enclosing pass's, else the switch's current value.  0 for
    a backend without bf16 kernels (the float64 oracle)."""
    code = getattr(_pass, "code", None)     # (set only to what this function returned for the pass's backend)
    if code is not None:
        return code
    be = be if be is not None else get_backend()
    if not getattr(be, "matmul_precision_aware", False):
        return 0
    return precision_code(torch.get_float32_matmul_precision())


_PK = ({}, {"precision": 1}, {"precision": 2})


def _pk(code):
    """keyword argument of the backend's convolution calls (absent at 0: every backend takes that call); read only"""
    return _PK[code]


def _ready(W, tok, code):
    """the weight buffer prepare_conv_weights stamped on W for this window AND this precision, else None (the
    convolution then lays its images out itself: a kernel never reads an image laid out for another piece count)"""
    r = getattr(W, "_ms3d_wf", None)
    return r[0] if (r is not None and r[1] == tok and r[2] == code) else None


class ConvSpec:
    """non-tensor launch description shared by forward and backward"""
    __slots__ = ("nbr_fwd", "nbr_bwd", "vin", "vout", "K", "cin", "cout", "mirror", "sub")

    def __init__(self, nbr_fwd, nbr_bwd, vin, vout, K, cin, cout, mirror, sub=None):
        self.nbr_fwd, self.nbr_bwd, self.vin, self.vout = nbr_fwd, nbr_bwd, vin, vout
        self.K, self.cin, self.cout, self.mirror = K, cin, cout, mirror
        # sub: None for the three geometries of the reference's models (the library's own rule: a 27-offset table is a
        # submanifold map); True / False for a table of CoordinateManager.kernel_map -- said to the backward-weight call,
        # whose wide K = 27 route takes the input rows for the output rows
        self.sub = sub


def _sk(spec):
    """keyword argument of the backend's backward calls that says the table's kind (absent for the old geometries)"""
    return {} if spec.sub is None else {"submanifold": spec.sub}


class SkipLink:
    """The gradient of a residual connection, handed from the LAST convolution of the block (whose epilogue added the
    skip) to the FIRST one (whose input is the skipped tensor): `out = x + branch(x)` sends dy to x twice -- through the
    branch and directly -- and autograd would add the two with an elementwise kernel per block and step.  The tail keeps
    its dy here instead of returning it for `residual`; the head's backward-data pass adds it to dx inside the
    BatchNorm-backward kernel it runs anyway (same two operands, same sum)."""
    __slots__ = ("grad", "armed")

    def __init__(self):
        self.grad = None
        self.armed = False     # set by the head's forward: only then may the tail keep its dy back


class GroupFlushFn(torch.autograd.Function):
    """Identity on a GROUP of convolution kernels whose backward runs once, after the last layer of the group has produced
    its weight gradient: there the group's queued backward-weight slab reductions are launched as ONE kernel
    (backend.WgradQueue) and the -- now complete -- gradients go on to the parameters.  Everything downstream of a
    parameter gradient (accumulation into an existing .grad, DistributedDataParallel's bucket hooks, the optimizer) sits
    behind this node, so it never sees an unreduced dW.  Built per forward by modules.prepare_conv_weights."""

    @staticmethod
    def forward(ctx, queue, *kernels):
        ctx.queue = queue
        ctx.set_materialize_grads(False)
        return tuple(k.view_as(k) for k in kernels)

    @staticmethod
    def backward(ctx, *grads):
        ctx.queue.flush()
        return (None,) + grads


def _defer_of(W, tok):
    """The deferred-reduction stamp of a kernel alias for this forward (prepare_conv_weights) -> (queue, use counter) or
    None, counting this use.  The deferral hands autograd a dW that is only filled when the group's GroupFlushFn node
    runs, which is sound while nothing computes on dW in between: a SECOND convolution on the same alias in one forward
    (weight sharing, a module called in a loop) makes autograd's input buffer add the two still-unwritten tensors before
    the flush.  The decision is therefore taken at BACKWARD time, when the count is final: `_queue`."""
    d = getattr(W, "_ms3d_defer", None)
    if d is None or d[1] != tok:
        return None
    d[2][0] += 1
    return (d[0], d[2])


def _queue(defer):
    """the queue a backward may defer to: only when its kernel alias was used exactly once in the forward"""
    return defer[0] if (defer is not None and defer[1][0] == 1) else None


class SparseConvFn(torch.autograd.Function):
    """(y, stats) = conv(act(x)) [+ residual];  stats = per-block (sum, sum of squares) of y from the kernel epilogue
    (non-differentiable side output that lets the next BatchNorm skip its statistics pass)"""

    @staticmethod
    def forward(ctx, x, W, gamma, beta, residual, spec, bn, want_stats, skip=None, bias=None):
        be = get_backend()
        pre = (bn["scale"], bn["shift"]) if bn is not None else None
        prec = ctx.prec = conv_precision(be)
        # weight images laid out for the whole model in one launch at the start of its forward (modules.prepare_conv_weights):
        # the stamp on the parameter says whether that buffer still holds the current weights, laid out for this precision
        ready = _ready(W, getattr(be, "weight_token", None), prec)
        y, stats, wf_buf = be.conv_layer_forward(x, W.view(spec.K, spec.cin, spec.cout), spec.nbr_fwd, spec.vout, spec.K,
                                                 spec.cin, spec.cout, spec.mirror, pre, bool(bn and bn["relu"]), residual,
                                                 None if bias is None else bias.reshape(-1), want_stats, **({"wf_ready": ready} if ready is not None else {}),
                                                 **_pk(prec))
        if stats is None:
            stats = x.new_zeros(0)
        ctx.spec, ctx.bn, ctx.wf_buf, ctx.has_res = spec, bn, wf_buf, residual is not None
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        # (deferred slab reduction: the queue of this kernel's group, stamped by prepare_conv_weights for this forward)
        ctx.defer = _defer_of(W, getattr(be, "weight_token", None))
        ctx.w_direct = W.is_leaf or ctx.defer is not None    # nobody computes on dW before the parameter / the flush node
        if skip is not None:     # None | ("head", SkipLink) | ("tail", SkipLink)
            if skip[0] == "head":
                skip[1].armed = True
            elif not (skip[1].armed and residual is not None):
                skip = None      # no head took the link: the skip gradient goes the ordinary way
        ctx.skip = skip
        ctx.save_for_backward(x, W)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        be = get_backend()
        spec, bn = ctx.spec, ctx.bn
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        role, link = ctx.skip if ctx.skip is not None else (None, None)
        add = None
        if role == "head":
            add, link.grad = link.grad, None
        if bn is not None and not bn["relu"]:
            # BatchNorm without ReLU in front of a convolution (not used by the reference): unfused path
            wft = be.prep_weights(W.view(spec.K, spec.cin, spec.cout), spec.K, spec.cout, spec.cin, transpose=True,
                                  mirror=spec.mirror)
            da = be.conv_forward(dy, wft, spec.nbr_bwd, spec.vin, spec.K, spec.cout, spec.cin)
            dz, dgb = be.bn_bwd_reduce(da, x, bn["scale"], bn["shift"], bn["mean"], bn["invstd"], False)
            dx = (be.bn_bwd_apply(dz, x, bn["scale"], bn["mean"], bn["invstd"], dgb) if bn["training"] else dz * bn["scale"])
            dW = be.conv_backward_weight(x, dy, spec.nbr_fwd, spec.vout, spec.K, spec.cin, spec.cout,
                                         pre=(bn["scale"], bn["shift"]), pre_relu=False, **_pk(ctx.prec), **_sk(spec))
        else:
            fused = add is not None and ctx.needs_input_grad[0] and be.fuses_dx_add(bn)
            extra = {"dx_add": add} if fused else {}
            if _queue(ctx.defer) is not None:
                extra["defer"] = _queue(ctx.defer)
            elif (not ctx.w_direct or (W.is_leaf and W.grad is not None)) and hasattr(be, "wgrad_stream_mode") \
                    and be.wgrad_stream_mode() == 2:
                # MS3D_WGRAD_STREAM=2 only: dW is consumed on this stream right away (a slice of a padded kernel's
                # gradient, the accumulation into an existing .grad): this layer's backward-weight is joined now
                extra["join_now"] = True
            dx, dgb, dW = be.conv_layer_backward(x, dy, ctx.wf_buf, spec.nbr_fwd, spec.nbr_bwd, spec.vin, spec.vout,
                                                 spec.K, spec.cin, spec.cout, bn, ctx.needs_input_grad[0], **extra,
                                                 **_pk(ctx.prec), **_sk(spec))
            if fused:
                add = None
        if add is not None and dx is not None:
            dx = dx + add
        dgamma = dgb[1] if dgb is not None else None
        dbeta = dgb[0] if dgb is not None else None
        d_res = dy if ctx.has_res else None
        if role == "tail" and ctx.has_res:
            link.grad, d_res = dy, None      # the head adds it to its dx
        db = None
        if ctx.bias_shape is not None and ctx.needs_input_grad[9]:
            # the bias is added to every output row: its gradient is the column sum of dy
            db = (be.column_sum(dy) if (hasattr(be, "column_sum") and dy.is_cuda) else dy.sum(0)).view(ctx.bias_shape)
        return dx, dW.view_as(W), dgamma, dbeta, d_res, None, None, None, None, db


class ResBlockFn(torch.autograd.Function):
    """A whole identity-skip residual block in training mode -- out = x + conv2(relu(bn1(conv1(relu(bn0(x)))))) -- as ONE
    autograd node over the same four library calls the module chain makes (bn_finalize, conv, bn_finalize, conv with the
    residual in its epilogue; backward: the two fused backward calls, the skip gradient added inside the first one's
    BatchNorm-backward pass, exactly what SparseConvFn + SkipLink do).  Nothing is computed differently: what goes away is
    interpreter work -- five nn.Module calls, four SparseTensor wrappers, one autograd node and the BatchNorm modules'
    bookkeeping per block (~150 -> ~55 us of host time; 21 of the 28 blocks of the backbone and 4 of the 6 of a proposal
    network qualify), which is what the lock-step phases of a step and a slow host wait for."""

    @staticmethod
    def forward(ctx, x, W1, g0, b0, W2, g1, b1, spec, stats_in, bn0, bn1, want_stats):
        be = get_backend()
        V = spec.vout
        tok = getattr(be, "weight_token", None)
        prec = ctx.prec = conv_precision(be)
        r1, r2 = _ready(W1, tok, prec), _ready(W2, tok, prec)
        fast = None
        if (r1 is not None and r2 is not None and spec.cin == spec.cout and torch.is_tensor(stats_in) and x.is_contiguous()
                and hasattr(be, "res_block_forward")):
            # round 6: the four calls below from ONE host call (same library calls, same order, same stream)
            fast = be.res_block_forward(x, stats_in, r1, r2, spec.nbr_fwd, V, spec.cout, bn0, g0.detach(), b0.detach(), bn1,
                                        g1.detach(), b1.detach(), want_stats, **_pk(prec))
        if fast is not None:
            y1, y2, st2, (m0, i0, s0, h0), (m1, i1, s1, h1) = fast
            wf1, wf2 = r1, r2
        else:
            m0, i0, s0, h0 = be.bn_finalize(stats_in, V, bn0.eps, bn0.momentum, g0.detach(), b0.detach(), bn0.running_mean,
                                            bn0.running_var)
            y1, st1, wf1 = be.conv_layer_forward(x, W1, spec.nbr_fwd, V, 27, spec.cin, spec.cout, True, (s0, h0), True, None,
                                                 None, True, **({"wf_ready": r1} if r1 is not None else {}), **_pk(prec))
            m1, i1, s1, h1 = be.bn_finalize(st1, V, bn1.eps, bn1.momentum, g1.detach(), b1.detach(), bn1.running_mean,
                                            bn1.running_var)
            y2, st2, wf2 = be.conv_layer_forward(y1, W2, spec.nbr_fwd, V, 27, spec.cout, spec.cout, True, (s1, h1), True, x,
                                                 None, want_stats, **({"wf_ready": r2} if r2 is not None else {}), **_pk(prec))
        ctx.spec, ctx.wf = spec, (wf1, wf2)
        ctx.bn = (dict(scale=s0, shift=h0, mean=m0, invstd=i0, relu=True, training=True),
                  dict(scale=s1, shift=h1, mean=m1, invstd=i1, relu=True, training=True))
        ctx.defer = (_defer_of(W1, tok), _defer_of(W2, tok))
        ctx.save_for_backward(x, y1, W1, W2)
        if st2 is None:
            st2 = x.new_zeros(0)
        ctx.mark_non_differentiable(st2)
        ctx.set_materialize_grads(False)
        return y2, st2

    @staticmethod
    def backward(ctx, dy, _dstats):
        be = get_backend()
        spec = ctx.spec
        x, y1, W1, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        V, c0, c1 = spec.vout, spec.cin, spec.cout
        e2 = {"defer": _queue(ctx.defer[1])} if _queue(ctx.defer[1]) is not None else {}
        dx1, dgb1, dW2 = be.conv_layer_backward(y1, dy, ctx.wf[1], spec.nbr_fwd, spec.nbr_bwd, V, V, 27, c1, c1, ctx.bn[1], True, **e2,
                                                **_pk(ctx.prec))
        e1 = {"defer": _queue(ctx.defer[0])} if _queue(ctx.defer[0]) is not None else {}
        dx, dgb0, dW1 = be.conv_layer_backward(x, dx1, ctx.wf[0], spec.nbr_fwd, spec.nbr_bwd, V, V, 27, c0, c1, ctx.bn[0],
                                               ctx.needs_input_grad[0], dx_add=dy, **e1, **_pk(ctx.prec))
        return dx, dW1.view_as(W1), dgb0[1], dgb0[0], dW2.view_as(W2), dgb1[1], dgb1[0], None, None, None, None, None


class ResBlockDownFn(torch.autograd.Function):
    """The residual block with a 1x1 projection on its skip path (the first block behind a skip concatenation):
    out = x W_d + conv2(relu(bn1(conv1(relu(bn0(x)))))) as one autograd node -- the projection (K = 1 convolution), the
    two bn_finalize (bn0 over the concatenation's parts) and the two fused convolutions forward; backward: the two fused
    backward calls of the branch, then the projection's, whose residual epilogue adds the branch's dx (the module chain
    leaves that sum to an elementwise autograd kernel)."""

    @staticmethod
    def forward(ctx, x, Wd, W1, g0, b0, W2, g1, b1, spec, ident, stats_in, bn0, bn1):
        be = get_backend()
        V, cin, cout = spec.vout, spec.cin, spec.cout
        tok = getattr(be, "weight_token", None)
        prec = ctx.prec = conv_precision(be)

        def ready(W):
            r = _ready(W, tok, prec)
            return dict({"wf_ready": r} if r is not None else {}, **_pk(prec))

        skip, _, wfd = be.conv_layer_forward(x, Wd.view(1, cin, cout), ident, V, 1, cin, cout, False, None, False, None, None,
                                             False, **ready(Wd))
        if isinstance(stats_in, tuple):
            m0, i0, s0, h0 = be.bn_finalize_parts(stats_in, V, bn0.eps, bn0.momentum, g0.detach(), b0.detach(),
                                                  bn0.running_mean, bn0.running_var)
        else:
            m0, i0, s0, h0 = be.bn_finalize(stats_in, V, bn0.eps, bn0.momentum, g0.detach(), b0.detach(), bn0.running_mean,
                                            bn0.running_var)
        y1, st1, wf1 = be.conv_layer_forward(x, W1, spec.nbr_fwd, V, 27, cin, cout, True, (s0, h0), True, None, None, True,
                                             **ready(W1))
        m1, i1, s1, h1 = be.bn_finalize(st1, V, bn1.eps, bn1.momentum, g1.detach(), b1.detach(), bn1.running_mean,
                                        bn1.running_var)
        y2, st2, wf2 = be.conv_layer_forward(y1, W2, spec.nbr_fwd, V, 27, cout, cout, True, (s1, h1), True, skip, None, True,
                                             **ready(W2))
        ctx.spec, ctx.wf, ctx.ident = spec, (wfd, wf1, wf2), ident
        ctx.bn = (dict(scale=s0.contiguous(), shift=h0.contiguous(), mean=m0.contiguous(), invstd=i0.contiguous(), relu=True,
                       training=True),
                  dict(scale=s1, shift=h1, mean=m1, invstd=i1, relu=True, training=True))

        ctx.defer = (_defer_of(Wd, tok), _defer_of(W1, tok), _defer_of(W2, tok))
        ctx.save_for_backward(x, y1, Wd, W1, W2)
        ctx.mark_non_differentiable(st2)
        ctx.set_materialize_grads(False)
        return y2, st2

    @staticmethod
    def backward(ctx, dy, _dstats):
        be = get_backend()
        spec = ctx.spec
        x, y1, Wd, W1, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        V, cin, cout = spec.vout, spec.cin, spec.cout
        ex = lambda d: dict({"defer": _queue(d)} if _queue(d) is not None else {}, **_pk(ctx.prec))
        dx1, dgb1, dW2 = be.conv_layer_backward(y1, dy, ctx.wf[2], spec.nbr_fwd, spec.nbr_bwd, V, V, 27, cout, cout, ctx.bn[1],
                                                True, **ex(ctx.defer[2]))
        need = ctx.needs_input_grad[0]
        dxb, dgb0, dW1 = be.conv_layer_backward(x, dx1, ctx.wf[1], spec.nbr_fwd, spec.nbr_bwd, V, V, 27, cin, cout, ctx.bn[0],
                                                need, **ex(ctx.defer[1]))
        dx, _, dWd = be.conv_layer_backward(x, dy, ctx.wf[0], ctx.ident, ctx.ident, V, V, 1, cin, cout, None, need,
                                            **({"dx_add": dxb} if need else {}), **ex(ctx.defer[0]))
        return dx, dWd.view_as(Wd), dW1.view_as(W1), dgb0[1], dgb0[0], dW2.view_as(W2), dgb1[1], dgb1[0], None, None, None, None, None


class BnReluConvFn(torch.autograd.Function):
    """[BatchNorm, ReLU, convolution] in training mode -- the strided / transposed convolutions between the U-Net levels --
    as one autograd node: bn_finalize + the fused convolution forward, the fused backward call (see ResBlockFn: the same
    library calls as the module chain, without its interpreter work)."""

    @staticmethod
    def forward(ctx, x, W, g, b, spec, stats_in, bn, want_stats):
        be = get_backend()
        tok = getattr(be, "weight_token", None)
        if isinstance(stats_in, tuple):
            m0, i0, s0, h0 = be.bn_finalize_parts(stats_in, spec.vin, bn.eps, bn.momentum, g.detach(), b.detach(),
                                                  bn.running_mean, bn.running_var)
        else:
            m0, i0, s0, h0 = be.bn_finalize(stats_in, spec.vin, bn.eps, bn.momentum, g.detach(), b.detach(), bn.running_mean,
                                            bn.running_var)
        prec = ctx.prec = conv_precision(be)
        r = _ready(W, tok, prec)
        y, st, wf = be.conv_layer_forward(x, W.view(spec.K, spec.cin, spec.cout), spec.nbr_fwd, spec.vout, spec.K, spec.cin,
                                          spec.cout, spec.mirror, (s0, h0), True, None, None, want_stats,
                                          **({"wf_ready": r} if r is not None else {}), **_pk(prec))
        ctx.spec, ctx.wf = spec, wf
        ctx.bn = dict(scale=s0.contiguous(), shift=h0.contiguous(), mean=m0.contiguous(), invstd=i0.contiguous(), relu=True,
                      training=True)
        ctx.defer = _defer_of(W, tok)
        ctx.save_for_backward(x, W)
        if st is None:
            st = x.new_zeros(0)
        ctx.mark_non_differentiable(st)
        ctx.set_materialize_grads(False)
        return y, st

    @staticmethod
    def backward(ctx, dy, _dstats):
        be = get_backend()
        spec = ctx.spec
        x, W = ctx.saved_tensors
        e = {"defer": _queue(ctx.defer)} if _queue(ctx.defer) is not None else {}
        dx, dgb, dW = be.conv_layer_backward(x, dy.contiguous(), ctx.wf, spec.nbr_fwd, spec.nbr_bwd, spec.vin, spec.vout, spec.K,
                                             spec.cin, spec.cout, ctx.bn, ctx.needs_input_grad[0], **e, **_pk(ctx.prec), **_sk(spec))
        return dx, dW.view_as(W), dgb[1], dgb[0], None, None, None, None


class BNActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, bn):
        ctx.bn = bn
        ctx.save_for_backward(x)
        return get_backend().bn_apply(x, bn["scale"], bn["shift"], bn["relu"])

    @staticmethod
    def backward(ctx, dy):
        be = get_backend()
        bn = ctx.bn
        (x,) = ctx.saved_tensors
        dz, s1s2 = be.bn_bwd_reduce(dy.contiguous(), x, bn["scale"], bn["shift"], bn["mean"], bn["invstd"], bn["relu"])
        dx = be.bn_bwd_apply(dz, x, bn["scale"], bn["mean"], bn["invstd"], s1s2) if bn["training"] else dz * bn["scale"]
        return dx, s1s2[1], s1s2[0], None


def bn_act(x, pending):
    if pending.get("gamma") is None:   # plain ReLU without a BatchNorm in front
        return torch.relu(x)
    return BNActFn.apply(x, pending["gamma"], pending["beta"], pending)


def conv(x, W, spec, pending, residual=None, want_stats=False, skip=None, bias=None):
    """-> (features, stats or None).  skip: ("head" | "tail", SkipLink) of a residual block, see SkipLink.
    bias [1, cout] or None: added in the kernel epilogue"""
    if pending is not None and pending.get("gamma") is None:
        x, pending = torch.relu(x), None
        if skip is not None and skip[0] == "head":
            skip = None       # x is no longer the skipped tensor itself: leave that block to autograd
    if pending is None:
        y, st = SparseConvFn.apply(x, W, None, None, residual, spec, None, want_stats, skip, bias)
    else:
        y, st = SparseConvFn.apply(x, W, pending["gamma"], pending["beta"], residual, spec, pending, want_stats, skip, bias)
    return y, (st if want_stats else None)


class DenseLinearFn(torch.autograd.Function):
    """y = x @ weight.T + bias for tall-skinny per-point matrices (N ~ 10^5..10^6, 16..32 channels) through the
    K = 1 path of the conv kernels: one coalesced pass over x instead of a library GEMM tuned for square shapes."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        be = get_backend()
        n, cin, cout = x.size(0), weight.size(1), weight.size(0)
        W3 = weight.t().contiguous().view(1, cin, cout)
        wf, wft = be.prep_weights_pair(W3, 1, cin, cout, mirror_bwd=False)
        ident = be.identity_table(n, x.device)
        y = be.conv_forward(x.contiguous(), wf, ident, n, 1, cin, cout, bias=bias)
        ctx.wft, ctx.dims, ctx.has_bias = wft, (n, cin, cout), bias is not None
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        be = get_backend()
        (x,) = ctx.saved_tensors
        n, cin, cout = ctx.dims
        dy = dy.contiguous()
        ident = be.identity_table(n, x.device)
        dx = be.conv_forward(dy, ctx.wft, ident, n, 1, cout, cin) if ctx.needs_input_grad[0] else None
        dW = be.conv_backward_weight(x, dy, ident, n, 1, cin, cout).view(cin, cout).t()
        db = None
        if ctx.has_bias:
            db = be.column_sum(dy) if (hasattr(be, "column_sum") and dy.is_cuda and dy.dtype == torch.float32) else dy.sum(0)
        return dx, dW, db


def dense_linear(x, weight, bias):
    return DenseLinearFn.apply(x, weight, bias)


def _rows(x, idx):
    """x[idx]: the library's row gather for device f32 rows (copy speed), torch indexing otherwise"""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and idx.dim() == 1 and idx.dtype == torch.int64:
        return get_backend().gather_rows(x, idx)
    return x[idx]


class GatherRowsFn(torch.autograd.Function):
    """y = x[idx] with a many-to-one index (voxel -> points).  torch's backward (index_put_ with accumulate) sorts the
    indices on every call; here the backward is one scatter-add kernel."""

    PRESORT_MIN_ROWS = 1 << 16

    @staticmethod
    def forward(ctx, x, idx, max_dup=None):
        ctx.save_for_backward(idx)
        ctx.n_rows, ctx.max_dup, ctx.sorted = x.size(0), max_dup, None
        be = get_backend()
        if idx.is_cuda and (max_dup is None or max_dup > 2) and hasattr(be, "presort_rows") and be.deterministic():
            # the backward sums in a fixed order over a stable sort of idx: the one the loader's prefetch or an earlier
            # gather over the same index (HAIS: features and mask scores) left, or one queued now on the helper thread
            ctx.sorted = be.presort_rows(idx, GatherRowsFn.PRESORT_MIN_ROWS)
        return _rows(x, idx)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        extra = {}
        if ctx.max_dup is not None:
            extra["max_dup"] = ctx.max_dup
        if ctx.sorted is not None:
            extra["sorted_"] = ctx.sorted
        return get_backend().scatter_add_rows(dy.contiguous(), idx, ctx.n_rows, **extra), None, None


class PermuteRowsFn(torch.autograd.Function):
    """y = x[inv] for a PERMUTATION inv (perm = its inverse): the backward is the gather dy[perm], no accumulation"""

    @staticmethod
    def forward(ctx, x, inv, perm):
        ctx.save_for_backward(perm)
        return _rows(x, inv)

    @staticmethod
    def backward(ctx, dy):
        (perm,) = ctx.saved_tensors
        return _rows(dy, perm), None, None


class SelectRowsFn(torch.autograd.Function):
    """y = x[idx] for an int64 index that names no row twice (pruning): the backward stores dy through the same index into a
    zeroed buffer -- one writer per row, no atomics, dropped rows get exactly zero"""

    @staticmethod
    def forward(ctx, x, idx):
        be = get_backend()
        if not hasattr(be, "scatter_rows"):
            raise NotImplementedError("pruning needs the HIP backend (ms3d_coords_prune / ms3d_scatter_rows)")
        ctx.save_for_backward(idx)
        ctx.n_rows = x.size(0)
        if idx.numel() == 0:             # an all-false mask: no launch on an empty grid
            return x.new_empty((0, x.size(1)))
        return be.gather_rows(x.contiguous(), idx)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        if idx.numel() == 0:
            return dy.new_zeros((ctx.n_rows, dy.size(1))), None
        return get_backend().scatter_rows(dy.contiguous(), idx, ctx.n_rows), None


def select_rows(x, idx):
    return SelectRowsFn.apply(x, idx)


def gather_rows(x, idx, max_dup=None):
    """differentiable x[idx] for 2-D float features and an int64 row index.  max_dup: the caller's bound on how many
    NON-ZERO addends one element of the gradient can collect -- how many entries of idx name the same row, or fewer when
    the caller knows the incoming gradient is sparse (<= 2: the backward's float atomics are order-independent -- a + b =
    b + a and adding zeros is exact -- no sort needed)"""
    if x.dim() == 2 and idx.dim() == 1 and idx.dtype == torch.int64 and x.requires_grad:
        return GatherRowsFn.apply(x, idx, max_dup)
    return _rows(x, idx) if x.dim() == 2 and idx.dim() == 1 else x[idx]


class SparsePoolFn(torch.autograd.Function):
    """y = pool(x) over a kernel map: mode 0 max, 1 average (over the PRESENT inputs of a row), 2 sum.  Forward walks the
    forward table, backward gathers through its inverse (csrc/pool.hip): no atomics in either direction."""

    @staticmethod
    def forward(ctx, x, nbr_fwd, nbr_inv, vin, vout, K, mode):
        be = get_backend()
        if not hasattr(be, "pool_forward"):
            raise NotImplementedError("sparse pooling needs the HIP backend (ms3d_pool_forward)")
        y, arg, count = be.pool_forward(mode, x, nbr_fwd, vout, K)
        ctx.geom = (nbr_inv, vin, K, mode, arg, count)
        return y

    @staticmethod
    def backward(ctx, dy):
        nbr_inv, vin, K, mode, arg, count = ctx.geom
        return get_backend().pool_backward(mode, dy.contiguous(), nbr_inv, vin, K, arg, count), None, None, None, None, None, None


def sparse_pool(x, nbr_fwd, nbr_inv, vin, vout, K, mode):
    return SparsePoolFn.apply(x, nbr_fwd, nbr_inv, vin, vout, K, mode)


class ChannelwiseConvFn(torch.autograd.Function):
    """y[o, c] = bias[c] + sum_k w[k, c] * x[nbr_fwd[k][o], c] over the present inputs (csrc/chconv.hip; float32, no matmul).
    Backward-data is the forward kernel through the inverse table with the same w (no mirrored offsets), backward-weight a
    two-stage reduction in a fixed order, the bias gradient a column sum: no atomics, the same bytes on every run.  A frozen
    kernel skips the weight pass, an input without grad the data pass."""

    @staticmethod
    def forward(ctx, x, w, bias, nbr_fwd, nbr_inv, vin, vout, K):
        be = get_backend()
        if not hasattr(be, "chconv_forward"):
            raise NotImplementedError("channel-wise convolution needs the HIP backend (ms3d_chconv_forward)")
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        ctx.geom = (nbr_fwd, nbr_inv, vin, vout, K, None if bias is None else tuple(bias.shape))
        return be.chconv_forward(x, w, bias, nbr_fwd, vout, K)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        nbr_fwd, nbr_inv, vin, vout, K, bias_shape = ctx.geom
        be = get_backend()
        dy = dy.contiguous()
        dx = be.chconv_forward(dy, w, None, nbr_inv, vin, K) if ctx.needs_input_grad[0] else None
        dw = be.chconv_backward_weight(x, dy, nbr_fwd, vout, K).view_as(w) if ctx.needs_input_grad[1] else None
        db = be.column_sum(dy).view(bias_shape) if bias_shape is not None and ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None, None, None, None


def channelwise_conv(x, w, bias, nbr_fwd, nbr_inv, vin, vout, K):
    return ChannelwiseConvFn.apply(x, w, bias, nbr_fwd, nbr_inv, vin, vout, K)


class KernelAttentionFn(torch.autograd.Function):
    """out[o, h, :] = sum_kk softmax_kk(scale * <q[o, h], k[i, h]> + rel_bias[kk, h]) * v[i, h, :] over the present inputs
    i = nbr_fwd[kk][o] (csrc/kattn.hip; float32, C = num_heads * D; a row without input is zero).  Saves q, k, v, out and the
    log-sum-exp lse [vout, H]; the backward recomputes the probabilities from lse.  The q pass walks the forward table (dq,
    dbias in two stages, and delta [vout, H], the residual the kv pass subtracts), the kv pass gathers through the inverse
    table: no atomics, the same bytes on every run.  Frozen q and bias skip the q pass unless the kv pass needs its delta
    (the pass then stores nothing else); frozen k and v skip the kv pass."""

    @staticmethod
    def forward(ctx, q, k, v, rel_bias, nbr_fwd, nbr_inv, vin, vout, K, num_heads, scale):
        be = get_backend()
        if not hasattr(be, "kattn_forward"):
            raise NotImplementedError("kernel-map attention needs the HIP backend (ms3d_kattn_forward)")
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = be.kattn_forward(q, k, v, rel_bias, nbr_fwd, vout, K, num_heads, scale)
        ctx.save_for_backward(q, k, v, rel_bias, out, lse)
        ctx.geom = (nbr_fwd, nbr_inv, vin, vout, K, num_heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, rel_bias, out, lse = ctx.saved_tensors
        nbr_fwd, nbr_inv, vin, vout, K, H, scale = ctx.geom
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        need_b = rel_bias is not None and ctx.needs_input_grad[3]
        be = get_backend()
        dout = dout.contiguous()
        dq = dk = dv = db = None
        if need_q or need_b or need_k or need_v:
            dq, db, delta = be.kattn_backward_q(q, k, v, rel_bias, nbr_fwd, out, lse, dout, vout, K, H, scale,
                                                need_dq=need_q, need_dbias=need_b)
            if need_k or need_v:
                dk, dv = be.kattn_backward_kv(q, k, v, rel_bias, nbr_inv, out, lse, delta, dout, vin, K, H, scale,
                                              need_dk=need_k, need_dv=need_v)
        return dq, dk, dv, db, None, None, None, None, None, None, None


def kernel_attention_rows(q, k, v, rel_bias, nbr_fwd, nbr_inv, vin, vout, K, num_heads, scale):
    """attention of the rows q [vout, C] over k / v [vin, C] through the tables of a kernel map (rows as the managers hold
    them) -> out [vout, C]"""
    return KernelAttentionFn.apply(q, k, v, rel_bias, nbr_fwd, nbr_inv, vin, vout, K, num_heads, scale)


class QueryAttentionFn(torch.autograd.Function):
    """out[b, q, h, :] = sum_i softmax_i(scale * <queries[b, q, h], k[i, h]>) * v[i, h, :] over the rows i of sample b that
    mask [V, Q] does not block (csrc/qattn.hip; float32, C = num_heads * D; a query with nothing to attend to is zero).  k / v:
    rows as the manager holds them; mask: rows as the caller sees them; group: the backend.BatchGroup of the rows
    (CoordinateManager.batch_group), which knows the held -> caller index, the chunk list and the segment of every row.
    Saves queries, k, v, out and the log-sum-exp lse [B, Q, H]; the backward recomputes the probabilities from lse.  The q pass sweeps the chunks again (dq and delta [B, Q, H], the residual the kv pass subtracts; one partial per
    chunk, added in chunk order), the kv pass loops over the queries per row: no atomics, the same bytes on every run.
    Frozen queries skip the q pass unless the kv pass needs its delta (the pass then stores nothing else); frozen k and v
    skip the kv pass."""

    @staticmethod
    def forward(ctx, queries, k, v, mask, group, num_heads, scale):
        be = get_backend()
        if not hasattr(be, "qattn_forward"):
            raise NotImplementedError("query attention needs the HIP backend (ms3d_qattn_forward)")
        queries, k, v = queries.contiguous(), k.contiguous(), v.contiguous()
        out, lse = be.qattn_forward(queries, k, v, mask, group, num_heads, scale)
        ctx.save_for_backward(queries, k, v, out, lse)
        ctx.geom = (mask, group, num_heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        queries, k, v, out, lse = ctx.saved_tensors
        mask, group, H, scale = ctx.geom
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        be = get_backend()
        dout = dout.contiguous()
        dq = dk = dv = None
        if need_q or need_k or need_v:
            dq, delta = be.qattn_backward_q(queries, k, v, mask, group, out, lse, dout, H, scale, need_dq=need_q)
            if need_k or need_v:
                dk, dv = be.qattn_backward_kv(queries, k, v, mask, group, out, lse, delta, dout, H, scale, need_dk=need_k,
                                              need_dv=need_v)
        return dq, dk, dv, None, None, None, None


def query_attention_rows(queries, k, v, mask, group, num_heads, scale):
    """attention of queries [B, Q, C] over the rows k / v [V, C] of their own sample (rows as the manager holds them, the mask's
    as the caller sees them) -> out [B, Q, C]"""
    return QueryAttentionFn.apply(queries, k, v, mask, group, num_heads, scale)


class VoxelAttentionFn(torch.autograd.Function):
    """out[i, h, :] = sum_q softmax_q(scale * <x[i, h], keys[b, q, h]>) * values[b, q, h, :] over the queries q of the row's
    sample b = group.seg_of_row[i] that mask [V, Q] does not block (csrc/vattn.hip; float32, C = num_heads * D; a row with nothing to
    attend to is zero) -- QueryAttentionFn's reverse direction, on the same mask and group.  Saves x, keys,
    values, out and the log-sum-exp lse [V, H]; the backward recomputes the probabilities from lse.  The x pass loops over the
    queries per row again (dx and delta [V, H], the residual the kv pass subtracts), the kv pass sweeps the chunks of every
    sample (one partial per chunk, added in chunk order): no atomics, the same bytes on every run.  Frozen keys and values
    skip the kv pass; a frozen x skips the x pass unless the kv pass needs its delta (the pass then stores nothing else)."""

    @staticmethod
    def forward(ctx, x, keys, values, mask, group, num_heads, scale):
        be = get_backend()
        if not hasattr(be, "vattn_forward"):
            raise NotImplementedError("voxel attention needs the HIP backend (ms3d_vattn_forward)")
        x, keys, values = x.contiguous(), keys.contiguous(), values.contiguous()
        out, lse = be.vattn_forward(x, keys, values, mask, group, num_heads, scale)
        ctx.save_for_backward(x, keys, values, out, lse)
        ctx.geom = (mask, group, num_heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, keys, values, out, lse = ctx.saved_tensors
        mask, group, H, scale = ctx.geom
        need_x, need_k, need_v = ctx.needs_input_grad[:3]
        be = get_backend()
        dout = dout.contiguous()
        dx = dk = dv = None
        if need_x or need_k or need_v:
            dx, delta = be.vattn_backward_x(x, keys, values, mask, group, out, lse, dout, H, scale, need_dx=need_x)
            if need_k or need_v:
                dk, dv = be.vattn_backward_kv(x, keys, values, mask, group, out, lse, delta, dout, H, scale, need_dk=need_k,
                                              need_dv=need_v)
        return dx, dk, dv, None, None, None, None


def voxel_attention_rows(x, keys, values, mask, group, num_heads, scale):
    """attention of the rows x [V, C] (as the manager holds them, the mask's as the caller sees them) over the queries keys /
    values [B, Q, C] of their own sample -> out [V, C]"""
    return VoxelAttentionFn.apply(x, keys, values, mask, group, num_heads, scale)


class InstanceNormFn(torch.autograd.Function):
    """y[r, c] = (x[r, c] - mean[s, c]) * invstd[s, c] * weight[c] + bias[c] with the statistics of the row's segment s (its
    batch index) and the biased variance (csrc/inorm.hip).  group: the backend.BatchGroup of the rows (CoordinateManager.
    batch_group); the rows are read where they are held, nothing is permuted.  Every sum runs in one
    fixed order without atomics: the same bytes on every run; sums and statistics (mean, invstd: float64 [B, C]) are double, the
    rows float32.  A frozen affine skips dweight / dbias, an input without grad
    skips dx."""

    @staticmethod
    def forward(ctx, x, weight, bias, group, eps):
        be = get_backend()
        if not hasattr(be, "inorm_forward"):
            raise NotImplementedError("instance normalisation needs the HIP backend (ms3d_inorm_forward)")
        x = x.contiguous()
        y, mean, invstd = be.inorm_forward(x, group, eps, weight, bias)
        ctx.save_for_backward(x, mean, invstd, weight)
        ctx.group = group
        ctx.shapes = (None if weight is None else tuple(weight.shape), None if bias is None else tuple(bias.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight = ctx.saved_tensors
        w_shape, b_shape = ctx.shapes
        need_x = ctx.needs_input_grad[0]
        need_w = w_shape is not None and ctx.needs_input_grad[1]
        need_b = b_shape is not None and ctx.needs_input_grad[2]
        dx, dw, db = get_backend().inorm_backward(dy.contiguous(), x, ctx.group, mean, invstd, weight, need_x, need_w, need_b)
        return dx, dw.view(w_shape) if need_w else None, db.view(b_shape) if need_b else None, None, None


def instance_norm(x, weight, bias, group, eps):
    return InstanceNormFn.apply(x, weight, bias, group, eps)


class UnionCombineFn(torch.autograd.Function):
    """out [n_out, C] = combine of the operands' rows on the union of their coordinate sets (op 0 sum of any number, 1
    subtract, 2 multiply of two; csrc/setops.hip).  maps: per operand (in_row int32 [n_out]: union row -> operand row in the
    order the operand's rows are HELD in, or -1; out_row int32 [V_i]: the other way), in_rows their [N, n_out] stack.  Both
    directions are gathers in a fixed order."""

    @staticmethod
    def forward(ctx, op, in_rows, out_rows, n_out, *feats):
        be = get_backend()
        ctx.op, ctx.in_rows, ctx.out_rows = op, in_rows, out_rows
        ctx.save_for_backward(*(feats if op == 2 else ()))
        if n_out == 0:
            return feats[0].new_empty((0, feats[0].size(1)))
        return be.union_combine(op, feats, in_rows, n_out)

    @staticmethod
    def backward(ctx, dout):
        be = get_backend()
        op, feats = ctx.op, ctx.saved_tensors
        grads = []
        for i, out_row in enumerate(ctx.out_rows):
            if not ctx.needs_input_grad[4 + i]:
                grads.append(None)
            elif out_row.numel() == 0:
                grads.append(dout.new_empty((0, dout.size(1))))
            elif op == 2:
                grads.append(be.union_combine_backward(op, i, dout, out_row, feats[1 - i], ctx.in_rows[1 - i]))
            else:
                grads.append(be.union_combine_backward(op, i, dout, out_row))
        return (None, None, None, None, *grads)


def union_combine(op, in_rows, out_rows, n_out, feats):
    return UnionCombineFn.apply(op, in_rows, out_rows, n_out, *feats)


class BroadcastFn(torch.autograd.Function):
    """y[r] = x[r] (mode) g[grow[r]]: mode 0 add, 1 multiply, 2 concatenate, 3 copy (x = None).  red = (order, seg_start,
    seg_of_g): the rows of x grouped by batch index and the segment of every row of g -- the fixed summation order of g's
    gradient (ms3d_broadcast_reduce).  x's gradient is dy itself, a column slice of it, or dy * g[grow]."""

    @staticmethod
    def forward(ctx, mode, x, g, grow, red):
        be = get_backend()
        ctx.mode, ctx.grow, ctx.red = mode, grow, red
        ctx.cx = 0 if x is None else x.size(1)
        ctx.save_for_backward(*((x, g) if mode == 1 else ()))
        if grow.numel() == 0:
            return g.new_empty((0, ctx.cx + g.size(1) if mode == 2 else g.size(1)))
        return be.broadcast(mode, x, g, grow)

    @staticmethod
    def backward(ctx, dy):
        be = get_backend()
        mode, cx = ctx.mode, ctx.cx
        dx = dg = None
        dy = dy.contiguous()
        if mode != 3 and ctx.needs_input_grad[1]:
            if mode == 0:
                dx = dy
            elif mode == 2:
                dx = dy[:, :cx]
            elif dy.size(0) == 0:
                dx = dy
            else:
                dx = be.broadcast(1, dy, ctx.saved_tensors[1], ctx.grow)
        if ctx.needs_input_grad[2]:
            cg = dy.size(1) - (cx if mode == 2 else 0)
            order, seg_start, seg_of_g = ctx.red
            if dy.size(0) == 0:
                dg = dy.new_zeros((seg_of_g.numel(), cg))
            else:
                dg = be.broadcast_reduce(dy, cx if mode == 2 else 0, cg, ctx.saved_tensors[0] if mode == 1 else None, order,
                                         seg_start, seg_of_g)
        return None, dx, dg, None, None


def broadcast(mode, x, g, grow, red):
    return BroadcastFn.apply(mode, x, g, grow, red)


def _field_backend(what, *methods):
    be = get_backend()
    if not all(hasattr(be, m) for m in methods):
        raise NotImplementedError(f"{what} needs the HIP backend (ms3d_{methods[0]})")
    return be


class FieldReduceFn(torch.autograd.Function):
    """voxel rows from point rows (TensorField.sparse): mode 0 average, 1 sum, 2 max over the points of every voxel in
    ascending point index (csrc/field.hip).  order / seg_start: the stable sort of `inverse` (int32 [N], point -> voxel row as
    the engine HOLDS the rows) and its segment offsets.  The backward is a gather per point."""

    @staticmethod
    def forward(ctx, feats, mode, inverse, order, seg_start, n_vox):
        be = _field_backend("TensorField.sparse", "field_reduce", "field_reduce_backward")
        if n_vox == 0:
            out, arg = feats.new_empty((0, feats.size(1))), None
        else:
            out, arg = be.field_reduce(mode, feats, order, seg_start, n_vox)
        ctx.geom = (mode, inverse, seg_start, arg)
        return out

    @staticmethod
    def backward(ctx, dvox):
        mode, inverse, seg_start, arg = ctx.geom
        if inverse.numel() == 0:
            return dvox.new_empty((0, dvox.size(1))), None, None, None, None, None
        return get_backend().field_reduce_backward(mode, dvox.contiguous(), inverse, seg_start, arg), None, None, None, None, None


def field_reduce(feats, mode, inverse, order, seg_start, n_vox):
    return FieldReduceFn.apply(feats, mode, inverse, order, seg_start, n_vox)


class InterpolateFn(torch.autograd.Function):
    """out [N, C] = trilinear interpolation of the rows x [V, C] (as the engine holds them) through an interpolation map
    (rows, weights: [8, N]; group = (entry_sorted, seg_start): the map's entries grouped by voxel row, the fixed summation
    order of the backward).  Gradients flow to x only: the query coordinates get none."""

    @staticmethod
    def forward(ctx, x, rows, weights, group):
        be = _field_backend("interpolation", "interp_forward", "interp_backward")
        ctx.geom = (rows, weights, group, x.size(0))
        if rows.size(1) == 0 or x.size(0) == 0:
            return x.new_zeros((rows.size(1), x.size(1)))
        return be.interp_forward(x, rows, weights)

    @staticmethod
    def backward(ctx, dout):
        rows, weights, (entry_sorted, seg_start), vin = ctx.geom
        if vin == 0 or rows.size(1) == 0:
            return dout.new_zeros((vin, dout.size(1))), None, None, None
        return get_backend().interp_backward(dout.contiguous(), weights, entry_sorted, seg_start, vin), None, None, None


def interpolate(x, rows, weights, group):
    return InterpolateFn.apply(x, rows, weights, group)


class NeighborPoolFn(torch.autograd.Function):
    """out [N, C] = max | avg | sum of the rows x [V, C] (as held) over the valid slots of every query of a NeighbourGroup, in
    ascending slot (csrc/neighbor.hip).  The backward is a gather through the record's table grouped by support row: one
    writer per element, no float atomics; max keeps the winning slot as uint8 [N, C]."""

    @staticmethod
    def forward(ctx, x, nmap, mode):
        out, arg = get_backend().nbr_pool_forward(mode, x.contiguous(), nmap)
        ctx.geom = (nmap, mode, arg)
        return out

    @staticmethod
    def backward(ctx, dout):
        nmap, mode, arg = ctx.geom
        return get_backend().nbr_backward(mode, dout.contiguous(), nmap, arg=arg), None, None


class NeighborSumFn(torch.autograd.Function):
    """out [N, C] = sum_j w[n, j] * x[idx[n, j]] over the valid slots (rows as held, w [N, k] in the row order of the record's
    idx_held), one fmaf per slot.  Gradients: to x through the record's table (skipped for a frozen x, the chunk list is then
    never built), to w one dot product per slot (skipped for frozen weights)."""

    @staticmethod
    def forward(ctx, x, w, nmap):
        x, w = x.contiguous(), w.contiguous()
        ctx.nmap = nmap
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, w if ctx.needs_input_grad[0] else None)
        return get_backend().nbr_wsum_forward(x, nmap, w)

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        be, nmap, dout = get_backend(), ctx.nmap, dout.contiguous()
        dx = be.nbr_backward(NBR_WEIGHTED, dout, nmap, w=w) if ctx.needs_input_grad[0] else None
        dw = be.nbr_wsum_backward_w(dout, x, nmap) if ctx.needs_input_grad[1] else None
        return dx, dw, None


def _nbr_input(x, nmap, name):
    """-> the rows of x as held [V, C], after the record has refused an x it was not made for"""
    if not isinstance(nmap, NeighbourGroup):
        raise TypeError(f"{name}: nmap must be a NeighborMap (knn_map or NeighborMap.from_index), got {type(nmap).__name__}")
    if torch.is_tensor(x):
        support, rows = (None, None), x
        if x.dim() != 2:
            raise ValueError(f"{name}: plain features must be [V, C], got {list(x.shape)}")
    elif hasattr(x, "coordinate_manager"):
        support, rows = (x.coordinate_manager, x.tensor_stride), x._raw()
    elif hasattr(x, "_shared"):
        support, rows = (x._shared, None), x._F
    else:
        raise TypeError(f"{name}: x must be a SparseTensor, a TensorField or a float tensor [V, C], got {type(x).__name__}")
    nmap.check(support, rows.size(0), rows.device)
    if rows.dtype in (torch.float16, torch.bfloat16) or not rows.is_floating_point():
        raise NotImplementedError(f"{name}: {rows.dtype} rows (float32; float64 on the CPU path)")
    if rows.is_cuda:
        if rows.dtype != torch.float32:
            raise NotImplementedError(f"{name}: {rows.dtype} rows on the device (float32)")
        if not hasattr(get_backend(), "nbr_pool_forward"):
            raise NotImplementedError(f"{name} on device tensors needs the HIP backend (ms3d_nbr_pool_forward)")
    return rows


def _nbr_result(out, nmap):
    return out.view(*nmap.lead, out.size(1)) if nmap.wrap is None else nmap.wrap(out)


def _nbr_gathered(rows, nmap):
    """the CPU path's [N, k, C] gather with the invalid slots zeroed, and the mask [N, k]"""
    ok = nmap.idx_held >= 0
    if nmap.V == 0:
        return (rows.sum() * 0).expand(nmap.N, nmap.k, rows.size(1)), ok
    g = rows[nmap.idx_held.clamp(min=0)]
    return torch.where(ok.unsqueeze(-1), g, torch.zeros((), dtype=g.dtype, device=g.device)), ok


def neighbor_pool(x, nmap, mode="max"):
    """max | avg | sum of x's rows over the neighbours of every query of nmap: the rules are in the package docstring."""
    name = "neighbor_pool"
    if mode not in NBR_MODES:
        raise ValueError(f"{name}: mode must be 'max', 'avg' or 'sum', got {mode!r}")
    rows = _nbr_input(x, nmap, name)
    if rows.is_cuda:
        if nmap.N == 0 or nmap.V == 0:           # no launch on an empty grid; x stays in the graph, its gradient is zeros
            return _nbr_result((rows.sum() * 0).expand(nmap.N, rows.size(1)), nmap)
        return _nbr_result(NeighborPoolFn.apply(rows, nmap, NBR_MODES[mode]), nmap)
    g, ok = _nbr_gathered(rows, nmap)
    acc = rows.new_zeros((nmap.N, rows.size(1)))
    seen = torch.zeros((nmap.N, 1), dtype=torch.bool)
    for j in range(nmap.k):                      # the chain in ascending slot; an invalid slot adds +0, which changes nothing
        if mode == "max":
            take = ok[:, j:j + 1] & (~seen | (g[:, j] > acc))
            acc = torch.where(take, g[:, j], acc)
            seen = seen | ok[:, j:j + 1]
        else:
            acc = acc + g[:, j]
    if mode == "avg":
        cnt = nmap.valid.to(rows.dtype).view(-1, 1)
        acc = torch.where(cnt > 0, acc / cnt.clamp(min=1), acc)
    return _nbr_result(acc, nmap)


def neighbor_sum(x, nmap, weights):
    """sum_j weights[n, j] * x[idx[n, j]] over the valid slots; weights float32 [..., k], differentiable."""
    name = "neighbor_sum"
    rows = _nbr_input(x, nmap, name)
    if not torch.is_tensor(weights) or not weights.is_floating_point():
        raise ValueError(f"{name}: weights must be a float tensor {list(nmap.lead) + [nmap.k]}")
    if tuple(weights.shape) != nmap.lead + (nmap.k,):
        if weights.dim() == len(nmap.lead) + 2 and tuple(weights.shape[:-1]) == nmap.lead + (nmap.k,):
            raise NotImplementedError(f"{name}: per-head or per-channel weights {list(weights.shape)}: one weight per slot, "
                                      f"{list(nmap.lead) + [nmap.k]}")
        raise ValueError(f"{name}: weights must have the shape of the index, {list(nmap.lead) + [nmap.k]}, got "
                         f"{list(weights.shape)}")
    if weights.dtype != rows.dtype or weights.device != rows.device:
        raise ValueError(f"{name}: weights are {weights.dtype} on {weights.device}, the rows {rows.dtype} on {rows.device}")
    w = weights.reshape(nmap.N, nmap.k)
    if nmap.row_perm is not None:                # the caller's query rows -> the order the target set holds them in
        w = PermuteRowsFn.apply(w, *nmap.row_perm)
    if rows.is_cuda:
        if nmap.N == 0 or nmap.V == 0:
            zero = (rows.sum() + w.sum()) * 0    # keeps both inputs in the graph: their gradients are zeros of the right shape
            return _nbr_result(zero.expand(nmap.N, rows.size(1)), nmap)
        return _nbr_result(NeighborSumFn.apply(rows, w, nmap), nmap)
    g, ok = _nbr_gathered(rows, nmap)
    w = torch.where(ok, w, torch.zeros((), dtype=w.dtype))             # the weight of an invalid slot is never read
    acc = rows.new_zeros((nmap.N, rows.size(1)))
    for j in range(nmap.k):
        acc = acc + w[:, j:j + 1] * g[:, j]
    return _nbr_result(acc, nmap)


def knn_interpolate(x, nmap, eps=1e-8):
    """inverse-distance interpolation: r = 1 / (float32(d2) + eps), w = r / sum_j r over the valid slots, then neighbor_sum.
    The weights are plumbing: not differentiable."""
    name = "knn_interpolate"
    if not isinstance(nmap, NeighbourGroup):
        raise TypeError(f"{name}: nmap must be a NeighborMap, got {type(nmap).__name__}")
    if nmap.d2 is None:
        raise ValueError(f"{name}: the map holds no distances (d2)")
    rows = _nbr_input(x, nmap, name)
    with torch.no_grad():
        ok = nmap.idx >= 0
        r = 1.0 / (nmap.d2.to(torch.float32) + eps)
        r = torch.where(ok, r, torch.zeros((), dtype=torch.float32, device=r.device))
        w = torch.where(ok, r / r.sum(-1, keepdim=True), r).to(rows.dtype)
    return neighbor_sum(x, nmap, w)


class NeighborAttentionFn(torch.autograd.Function):
    """out[n, h, :] = sum_j softmax_j(scale * <q[n, h], k[i, h]> + bias[n, j, h]) * v[i, h, :] over the valid slots i =
    idx_held[n, j] of a NeighbourGroup (csrc/nattn.hip; float32, C = num_heads * D; a query without a valid slot is zero).  q
    and bias in the row order of the record's idx_held, k / v as held.  Saves q, k, v, bias, out and the log-sum-exp lse [N, H];
    the backward recomputes the probabilities from lse.  The q pass repeats the forward sweep (dq, dbias [N, k, H] and delta
    [N, H], the residual the kv pass subtracts), the kv pass gathers through the record's table grouped by support row: no
    atomics, the same bytes on every run.  Frozen q and bias skip the q pass unless the kv pass needs its delta (the pass then
    stores nothing else); frozen k and v skip the kv pass, and the table and the chunk list are then never built."""

    @staticmethod
    def forward(ctx, q, k, v, bias, nmap, num_heads, scale):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        bias = None if bias is None else bias.contiguous()
        out, lse = get_backend().nattn_forward(q, k, v, bias, nmap, num_heads, scale)
        ctx.save_for_backward(q, k, v, bias, out, lse)
        ctx.geom = (nmap, num_heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, bias, out, lse = ctx.saved_tensors
        nmap, H, scale = ctx.geom
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        need_b = bias is not None and ctx.needs_input_grad[3]
        be = get_backend()
        dout = dout.contiguous()
        dq = dk = dv = db = None
        if need_q or need_b or need_k or need_v:
            dq, db, delta = be.nattn_backward_q(q, k, v, bias, nmap, out, lse, dout, H, scale, need_dq=need_q, need_dbias=need_b)
            if need_k or need_v:
                dk, dv = be.nattn_backward_kv(q, k, v, bias, nmap, out, lse, delta, dout, H, scale, need_dk=need_k,
                                              need_dv=need_v)
        return dq, dk, dv, db, None, None, None


_NATTN_MAX_D = 128                       # the limit of csrc/nattn.hip


def _nattn_query(q, nmap, name):
    """-> the rows of q [N, C] in the row order of the record's idx_held, after the record has refused a q that does not live
    on its target"""
    if torch.is_tensor(q):
        target = (None, None)
        if q.dim() < 1 or tuple(q.shape[:-1]) != nmap.lead:
            raise ValueError(f"{name}: plain q must be {list(nmap.lead) + ['C']}, one row per query of the map, got "
                             f"{list(q.shape)}")
        rows = q.reshape(nmap.N, q.size(-1))
    elif hasattr(q, "coordinate_manager"):
        target, rows = (q.coordinate_manager, q.tensor_stride), q._raw()
    elif hasattr(q, "_shared"):
        target, rows = (q._shared, None), q._F
    else:
        raise TypeError(f"{name}: q must be a SparseTensor, a TensorField or a float tensor [..., C], got {type(q).__name__}")
    nmap.check_target(target, rows.size(0), rows.device)
    return rows


def neighbor_attention(q, k, v, nmap, num_heads, bias=None, scale=None):
    """multi-head softmax attention of every query of nmap over its neighbours, with a per-entry, per-head additive bias: the
    rules are in the package docstring."""
    name = "neighbor_attention"
    held = k if torch.is_tensor(k) else getattr(k, "_F", None)
    if torch.is_tensor(held) and held.is_cuda and not hasattr(get_backend(), "nattn_forward"):
        raise NotImplementedError(f"{name} on device tensors needs the HIP backend (ms3d_nattn_forward)")
    krows = _nbr_input(k, nmap, name)
    if type(k) is not type(v) and not (torch.is_tensor(k) and torch.is_tensor(v)):
        raise ValueError(f"{name}: k and v must be of the same kind on the same set, got {type(k).__name__} and "
                         f"{type(v).__name__}")
    try:
        vrows = _nbr_input(v, nmap, name)
    except ValueError as e:
        raise ValueError(f"{name}: k and v must live on the same set -- {e}") from None
    qrows = _nattn_query(q, nmap, name)
    C = krows.size(1)
    if vrows.size(1) != C or qrows.size(1) != C:
        raise ValueError(f"{name}: q, k and v must have the same number of channels, got {qrows.size(1)}, {C}, {vrows.size(1)}")
    if isinstance(num_heads, bool) or not isinstance(num_heads, int) or num_heads < 1:
        raise ValueError(f"{name}: num_heads must be a Python int >= 1, got {num_heads!r}")
    if C % num_heads != 0:
        raise ValueError(f"{name}: {C} channels do not divide into num_heads={num_heads}")
    H, D = num_heads, C // num_heads
    if D > _NATTN_MAX_D:
        raise ValueError(f"{name}: head dimension D = {D} is above the kernels' limit of {_NATTN_MAX_D}")
    if qrows.dtype != krows.dtype or vrows.dtype != krows.dtype or qrows.device != krows.device:
        if torch.float16 in (qrows.dtype, vrows.dtype) or torch.bfloat16 in (qrows.dtype, vrows.dtype):
            raise NotImplementedError(f"{name}: float16 / bfloat16 rows (float32; float64 on the CPU path)")
        raise ValueError(f"{name}: q, k and v must share one dtype and device, got {qrows.dtype}, {krows.dtype}, {vrows.dtype}")
    b = None
    if bias is not None:
        want = nmap.lead + (nmap.k, H)
        if not torch.is_tensor(bias) or tuple(bias.shape) != want:
            raise ValueError(f"{name}: bias must be a tensor {list(want)} (one term per query, slot and head), got "
                             f"{list(bias.shape) if torch.is_tensor(bias) else type(bias).__name__}")
        if bias.dtype != krows.dtype or bias.device != krows.device:
            raise ValueError(f"{name}: bias is {bias.dtype} on {bias.device}, the rows {krows.dtype} on {krows.device}")
        b = bias.reshape(nmap.N, nmap.k * H)
        if nmap.row_perm is not None:            # the caller's query rows -> the order the target set holds them in
            b = PermuteRowsFn.apply(b, *nmap.row_perm)
        b = b.view(nmap.N, nmap.k, H)
    scale = float(D ** -0.5 if scale is None else scale)
    if krows.is_cuda:
        if nmap.N == 0 or nmap.V == 0:           # no launch on an empty grid; the inputs stay in the graph, their gradients are zeros
            zero = (qrows.sum() + krows.sum() + vrows.sum() + (0 if b is None else b.sum())) * 0
            return _nbr_result(zero.expand(nmap.N, C), nmap)
        return _nbr_result(NeighborAttentionFn.apply(qrows, krows, vrows, b, nmap, H, scale), nmap)
    kg, ok = _nbr_gathered(krows, nmap)          # the CPU path: the same rule as a torch expression; makes [N, k, C]
    vg, _ = _nbr_gathered(vrows, nmap)
    s = torch.einsum("nhd,njhd->njh", qrows.view(nmap.N, H, D), kg.reshape(nmap.N, nmap.k, H, D)) * scale
    if b is not None:
        s = s + torch.where(ok.unsqueeze(-1), b, torch.zeros((), dtype=b.dtype))     # an invalid slot's bias is never used
    s = s.masked_fill(~ok.unsqueeze(-1), float("-inf"))
    m = s.amax(1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros((), dtype=m.dtype))            # a query without a valid slot: exp(-inf) = 0
    p = torch.exp(s - m.detach())
    den = p.sum(1, keepdim=True)
    p = torch.where(den > 0, p / torch.where(den > 0, den, torch.ones((), dtype=den.dtype)), p)
    out = torch.einsum("njh,njhd->nhd", p, vg.reshape(nmap.N, nmap.k, H, D)).reshape(nmap.N, C)
    return _nbr_result(out, nmap)


class DenseScatterFn(torch.autograd.Function):
    """rows -> grid (SparseTensor.dense): out [B, C, X, Y, Z] with out[b, :, cell] = x[cell_row[cell]], zeros where the cell has
    no row (csrc/dense.hip).  cell_row / row_cell: the two directions of one cell map over the rows as the engine HOLDS them.
    The backward is the other kernel over the same map: dx[r] = dout[b, :, row_cell[r]].  No float is added in either
    direction: the same bytes on every run."""

    @staticmethod
    def forward(ctx, x, cell_row, row_cell, shape):
        be = _field_backend("SparseTensor.dense", "dense_scatter", "dense_gather")
        ctx.row_cell = row_cell
        return be.dense_scatter(x, cell_row, shape)

    @staticmethod
    def backward(ctx, dout):
        return get_backend().dense_gather(dout.contiguous(), ctx.row_cell), None, None, None


def dense_scatter(x, cell_row, row_cell, shape):
    return DenseScatterFn.apply(x, cell_row, row_cell, shape)


class DenseGatherFn(torch.autograd.Function):
    """grid -> rows (to_sparse): out [n, C] with out[i] = x[b, :, cells[i]] for x [B, C, X, Y, Z].  coords: the coordinates
    int32 [n, 4] of the cells (b, x, y, z with origin 0), in the order of `cells` -- the backward builds the cell map from them
    once and scatters: dx[b, :, cell] = dout[row of the cell], zeros at the cells not listed.  Where the list names a cell
    twice (only to_sparse(coordinates=...) can), the rows of one cell are first summed in ascending row order onto its lowest
    row (scatter_add_rows: a fixed order, no float atomics)."""

    @staticmethod
    def forward(ctx, x, cells, coords):
        be = _field_backend("to_sparse", "dense_gather", "dense_scatter", "dense_cell_map")
        ctx.geom = (cells, coords, tuple(x.shape))
        return be.dense_gather(x, cells)

    @staticmethod
    def backward(ctx, dout):
        cells, coords, shape = ctx.geom
        be = get_backend()
        B, _, X, Y, Z = shape
        cell_row, _, (_, _, lost) = be.dense_cell_map(coords, (0, 0, 0), 1, (B, X, Y, Z))
        dout = dout.contiguous()
        if lost:
            winner = cell_row[cells.long()].long()
            dout = be.scatter_add_rows(dout, winner, dout.size(0))
        return be.dense_scatter(dout, cell_row, shape), None, None


def dense_gather(x, cells, coords):
    return DenseGatherFn.apply(x, cells, coords)
