"""nn.Module surface of the MinkowskiEngine subset (same constructor arguments, parameter names and init as ME
v0.5.4): `kernel` of shape (K, in, out) -- (in, out) for kernel_size 1 -- and, when asked for,
`bias` of shape (1, out), both uniform(-1/sqrt(in*K), +1/sqrt(in*K)); MinkowskiBatchNorm wraps `self.bn =
nn.BatchNorm1d`.

Convolutions take any integer kernel size and dilation with stride 1 (odd sizes) or 2; pooling layers walk the same
kernel maps.  `kernel_generator=` (tensor.KernelGenerator) hands the same geometry over as one object, and with it the
crosses and hand-written offset lists (_layer_geometry).  What MinkowskiEngine does for the geometries beyond the
reference's three -- the offset order of even kernels, the offset order of a cross, average pooling dividing by the number of inputs PRESENT, the bias shape -- is written down from memory of
its v0.5 sources: MinkowskiEngine is not installed where this package is developed (as SURVEY Appendix A says of the
conventions it recalls), so these are this engine's definitions, checked against dense torch operators."""
import math
import os

import torch
import torch.nn as nn

from ..backend import get_backend
from . import functional as Fn
from .tensor import SparseTensor, CoordinateMapKey, check_geometry, union_op, to_sparse, to_sparse_all, target_key
from .tensor import KernelGenerator, knn_map


def _layer_geometry(layer, kernel_size, stride, dilation, kernel_generator, expand_coordinates=False):
    """the geometry of a layer built with `kernel_generator=` -> (kernel_size, stride, dilation, region, expand_coordinates,
    kernel volume).  Without a generator: the layer's own arguments through check_geometry, region None.  With one, kernel
    size, stride, dilation and region come from it; a layer argument that was given (is not its default -1 / 1 / 1) and
    says otherwise is a ValueError (the kernel size of a CUSTOM region is ignored); expand_coordinates is "layer argument
    or generator attribute".  A HYPER_CUBE generator comes back with region None: the layer IS the plain layer."""
    if kernel_generator is None:
        check_geometry(kernel_size, stride, dilation)
        return kernel_size, stride, dilation, None, bool(expand_coordinates), kernel_size ** 3
    g = kernel_generator
    if not isinstance(g, KernelGenerator):
        raise TypeError(f"{layer}: kernel_generator must be a KernelGenerator, got {type(g).__name__}")
    given = (("stride", stride, 1, g.stride), ("dilation", dilation, 1, g.dilation))
    if not (g.region_key is not None and g.region_key[0] == "CUSTOM"):
        given = (("kernel_size", kernel_size, -1, g.kernel_size),) + given
    for name, value, default, theirs in given:
        if value != default and value != theirs:
            raise ValueError(f"{layer}: {name}={value} contradicts the kernel_generator's {name}={theirs}")
    return (g.kernel_size, g.stride, g.dilation, g.region_key, bool(expand_coordinates) or g.expand_coordinates,
            g.kernel_volume)


def _region_name(region):
    """how extra_repr names a region"""
    return "" if region is None else f", region={region[0]}[{region[1] if region[0] == 'HYPER_CROSS' else len(region[1])}]"


class _ConvBase(nn.Module):
    _two_sets = False     # True: input and output coordinate sets differ at every stride (no mirrored backward-data weights)

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, dimension=3,
                 expand_coordinates=False, kernel_generator=None):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError(f"dimension={dimension}: only 3-D sparse tensors are supported")
        # region: None for a cube (a HYPER_CUBE generator included), else the key of a cross or a custom offset list -- such a
        # layer works between "two sets" at every stride: CoordinateManager.kernel_map(region=), mirror = sub = False
        kernel_size, stride, dilation, self.region, self.expand_coordinates, K = _layer_geometry(
            type(self).__name__, kernel_size, stride, dilation, kernel_generator, expand_coordinates)
        self._check_expand(kernel_size, stride, dilation)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation
        self.kernel_volume = K
        shape = (in_channels, out_channels) if (kernel_size == 1 and stride == 1 and self.region is None) \
            else (K, in_channels, out_channels)
        self.kernel = nn.Parameter(torch.empty(shape, dtype=torch.float32))
        s = 1.0 / math.sqrt(in_channels * K)
        # ME's name and shape, so that state_dict keys carry over; same uniform bound as the kernel
        self.bias = nn.Parameter(torch.empty((1, out_channels), dtype=torch.float32)) if bias else None
        with torch.no_grad():
            self.kernel.uniform_(-s, s)
            if bias:
                self.bias.uniform_(-s, s)

    def _spec(self, cm, ts):
        """-> (ConvSpec of the forward convolution from tensor stride ts, output tensor stride)"""
        cin, cout = self.in_channels, self.out_channels
        nbr_fwd, nbr_bwd, vin, vout, K, out_ts, mirror = cm.kernel_map_tables(ts, self.kernel_size, self.stride, self.dilation,
                                                                              region=self.region)
        if self.region is not None:
            # (sub = False: a custom list of 27 or 8 offsets is neither the 3x3x3 submanifold map nor the k2 map)
            return Fn.ConvSpec(nbr_fwd, nbr_bwd, vin, vout, K, cin, cout, False, False), out_ts
        # the three maps of the reference's models keep the library's own rule for what a table is (sub = None); the
        # general ones say whether they map a coordinate set onto itself
        old = (self.kernel_size, self.stride, self.dilation) in ((3, 1, 1), (2, 2, 1)) or K == 1
        return Fn.ConvSpec(nbr_fwd, nbr_bwd, vin, vout, K, cin, cout, mirror, None if old else mirror), out_ts

    def _check_expand(self, kernel_size, stride, dilation):
        """refusals of expand_coordinates=True at construction (the subclasses that restrict it)"""

    def _image_mirror(self):
        """does prepare_conv_weights lay this module's backward-data image out with mirrored offsets: the layers that map a
        coordinate set onto ITSELF (odd kernel, stride 1, one set) -- never a module constructed with expand_coordinates,
        whose output set is another one on every call"""
        return (self.region is None and self.kernel_size % 2 == 1 and self.kernel_size > 1 and self.stride == 1
                and not self._two_sets and not self.expand_coordinates)

    def _kernel_two_sets(self):
        """the kernel of a call whose table maps the input set onto ANOTHER set (mirror = False: a target given by
        `coordinates=`): where prepare_conv_weights laid this module's image out mirrored, an UNSTAMPED alias of the parameter
        -- the call lays its own images out and its weight gradient goes straight to the parameter, not through the window's
        mirrored image or its deferred-reduction group; otherwise the kernel of any call"""
        return self.kernel.view_as(self.kernel) if self._image_mirror() else self._kernel()

    def _conv_onto(self, x, out_cm, out_ts, table):
        """y = conv(x) over `table` = (nbr_fwd, nbr_bwd, vin, vout, K) between two different coordinate sets -> SparseTensor on
        (out_cm, out_ts).  sub = False keeps a K = 27 table off the submanifold backward-weight route, as the generative layer
        does; a pending BatchNorm / ReLU flows into the gather.  An empty target gives an empty tensor (no launch)."""
        nbr_fwd, nbr_bwd, vin, vout, K = table
        cin, cout = self.in_channels, self.out_channels
        kernel = self._kernel_two_sets()
        if vout == 0:
            y = x._raw()[:0] @ kernel.reshape(-1, cin, cout)[0]
            return SparseTensor(y if self.bias is None else y + self.bias, coordinate_manager=out_cm, tensor_stride=out_ts)
        spec = Fn.ConvSpec(nbr_fwd, nbr_bwd, vin, vout, K, cin, cout, False, False)
        y, stats = Fn.conv(x._F, kernel, spec, x._pending, want_stats=self.training, bias=self.bias)
        return SparseTensor(y, coordinate_manager=out_cm, tensor_stride=out_ts, _stats=stats)

    def _kernel(self):
        """the kernel this forward uses: the parameter, or -- inside a prepare_conv_weights window in training -- its
        alias behind the group's GroupFlushFn node (same storage; the gradient reaches the parameter through that node)"""
        eff = self.__dict__.get("_kernel_eff")
        if eff is not None and eff[1] == getattr(get_backend(), "weight_token", None):
            return eff[0]
        return self.kernel

    def extra_repr(self):
        return (f"in={self.in_channels}, out={self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"dilation={self.dilation}, bias={self.bias is not None}" + _region_name(self.region)
                + (", expand_coordinates=True" if self.expand_coordinates else ""))


def _flush_group(name):
    """Which deferred-reduction group a convolution belongs to, from its module path.  A group's slab reductions run when
    its LAST layer has finished its backward pass, and only then do its gradients reach the parameters (and a
    data-parallel wrapper's bucket hooks), so the groups follow the order of the backward pass and keep the bulk of the
    bytes early: the proposal network first; then the decoder side of the three finest U-Net levels; then everything
    from level 3 down (~90 % of the parameter bytes, complete half way through the pass); last the encoder side of the
    finest levels and the input convolution (~1.5 MB at m = 16)."""
    parts = name.split(".")
    if "backbone" not in parts:
        return 0
    depth = parts.count("u")
    if depth >= 3:
        return 2
    return 1 if ("blocks_tail" in parts or "deconv" in parts) else 3


def prepare_conv_weights(root, precision=None):
    """Lay out the kernel-side images of EVERY convolution weight under `root` in one launch (instead of one ~5 us
    launch per layer inside each convolution call; ~90 per U-Net step) and stamp the parameters.  The stamp is valid
    until `release_conv_weights()`: call the pair around a forward pass during which the weights do not change
    (GeneralModel.__call__ does).  Convolutions called outside such a window lay out their own weights as before.
    The images are laid out for the matmul precision code `precision` (functional.precision_code; default: what a
    convolution would run at now) and the stamp is (buffer, weight_token, precision): a convolution that runs at another
    precision lays its own images out.
    In training the convolutions are also handed their kernels through `GroupFlushFn` nodes (functional.py): the slab
    reductions behind the backward-weight kernels of a whole group of layers then run as one launch.
    Not part of ME's API."""
    be = get_backend()
    if not hasattr(be, "prep_weights_multi") or os.environ.get("MS3D_WEIGHT_MULTI", "1") == "0":
        return
    layers = []
    convs = root.__dict__.get("_ms3d_convs")
    if convs is None:
        # (walking the module tree costs 0.7 ms per step on the 400-module networks; the set of convolutions of a built
        # model does not change -- `del model._ms3d_convs` after surgery on it)
        named = [(n, m) for n, m in root.named_modules() if isinstance(m, _ConvBase)]
        convs = root.__dict__["_ms3d_convs"] = tuple(m for _, m in named)
        root.__dict__["_ms3d_conv_groups"] = tuple(_flush_group(n) for n, _ in named)
    for m, grp in zip(convs, root.__dict__["_ms3d_conv_groups"]):
        m.__dict__.pop("_kernel_eff", None)
        if m.kernel.is_cuda:
            K, cin, cout = m.kernel_volume, m.in_channels, m.out_channels
            if m.kernel.dim() == 2:
                K = 1
            buf = m.__dict__.get("_wf_buf")
            if buf is None or buf.device != m.kernel.device:
                buf = m.__dict__["_wf_buf"] = torch.empty(be.wf_floats(K, cin, cout), dtype=torch.float32, device=m.kernel.device)
            # same orientation rule as the forward() of the module: 3x3x3 maps mirror their offsets in backward-data
            # (per module: _ConvBase._image_mirror)
            layers.append((m.kernel, buf, K, cin, cout, m._image_mirror(), m, grp))
    prec = Fn.conv_precision(be) if precision is None else precision
    be.prep_weights_multi([l[:6] for l in layers], **Fn._pk(prec))
    token = be.weight_token
    defer = torch.is_grad_enabled() and hasattr(be, "wgrad_queue")
    if defer:
        groups = {}
        for w, buf, *_, m, grp in layers:
            if w.requires_grad:
                groups.setdefault(grp, []).append((w, buf, m))
        for g, members in groups.items():
            queue = be.wgrad_queue()
            if queue is None:
                defer = False
                break
            eff = Fn.GroupFlushFn.apply(queue, *[w for w, _, _ in members])
            for e, (w, buf, m) in zip(eff, members):
                e._ms3d_wf = (buf, token, prec)
                e._ms3d_defer = (queue, token, [0])      # [uses of this alias in the forward]: functional._defer_of
                m.__dict__["_kernel_eff"] = (e, token)
    for w, buf, *_ in layers:
        w._ms3d_wf = (buf, token, prec)


def release_conv_weights():
    be = get_backend()
    if hasattr(be, "release_weights"):
        be.release_weights()


class MinkowskiConvolution(_ConvBase):
    """Any kernel size and dilation at stride 1 (odd sizes: submanifold, output coords = input coords) or stride 2 (output on
    the stride-2 coordinate set, whatever the kernel size).  k3 s1, k2 s2 and k1 s1 -- the reference's layers -- run on the
    tables, pair lists and fused blocks tuned for them; every other geometry walks its table with the general kernels,
    untuned.  Strides other than 1 and 2, even kernels at stride 1 and per-axis tuples raise NotImplementedError.

    forward(x, coordinates=target) writes onto a coordinate set the caller names -- an integer tensor [M, 4], a
    CoordinateMapKey or a SparseTensor (tensor.target_key) at tensor stride ts * stride: out[o] = bias + sum_k x[o + off_k]
    W[k], off = kernel_offsets(kernel_size, dilation, ts); a row no input reaches is the bias.  A target that names the set
    the layer lands on anyway takes the ordinary path.  expand_coordinates=True (stride 1 only): the output set is every
    coordinate the kernel reaches, CoordinateManager.expand, on a manager rooted at the tensor stride.

    kernel_generator= (a KernelGenerator): a HYPER_CUBE generator is this layer as its plain arguments build it.  A cross or a
    custom offset list is a layer between "two sets" on every path, its own set at stride 1 included: forward and inverse
    tables of CoordinateManager.kernel_map(region=), mirror = sub = False, no residual / skip."""

    def _check_expand(self, kernel_size, stride, dilation):
        if self.expand_coordinates and stride != 1:
            raise NotImplementedError(f"MinkowskiConvolution(kernel_size={kernel_size}, stride={stride}, "
                                      f"expand_coordinates=True): expand_coordinates is supported at stride 1 only")

    def _forward_onto(self, x, residual, skip, coordinates):
        if coordinates is not None and self.expand_coordinates:
            raise ValueError("MinkowskiConvolution: expand_coordinates=True derives the output set, coordinates= names it: "
                             "not both")
        if residual is not None or skip is not None:
            raise ValueError("MinkowskiConvolution: residual / skip (engine extras of the submanifold layers) cannot be "
                             "combined with " + ("coordinates=" if coordinates is not None else "expand_coordinates=True"
                                                 if self.expand_coordinates else "a kernel_generator region"))
        cm, ts = x.coordinate_manager, x.tensor_stride
        if coordinates is None and not self.expand_coordinates:
            # a cross or a custom list on the layer's own sets: the region's forward and inverse tables, no mirrored image
            spec, out_ts = self._spec(cm, ts)
            y, stats = Fn.conv(x._F, self._kernel(), spec, x._pending, want_stats=self.training, bias=self.bias)
            return x._like(y, tensor_stride=out_ts, stats=stats)
        if coordinates is None:
            gen = cm.expand(ts, self.kernel_size, self.dilation, region=self.region)
            return self._conv_onto(x, gen[0], ts, gen[1:])
        out_ts = ts * self.stride
        key = target_key(coordinates, out_ts, x.device)
        if key.coordinate_manager is cm:
            return self.forward(x)          # the set this layer lands on anyway: its own at stride 1, the cached one at 2
        table = cm.target_map(ts, key, self.kernel_size, self.stride, self.dilation, region=self.region)
        return self._conv_onto(x, key.coordinate_manager, out_ts, table)

    def forward(self, x: SparseTensor, residual: SparseTensor = None, skip=None, *, coordinates=None):
        """`residual` (same coordinate map as the output) is added in the kernel epilogue -- used by ResidualBlock
        instead of a separate `+=` pass; `skip` = ("head" | "tail", functional.SkipLink) routes the skip connection's
        gradient through the block's first convolution instead of an elementwise add.  Neither is part of ME's API.
        `coordinates` (keyword only): the set to write onto, see the class."""
        if coordinates is not None or self.expand_coordinates or self.region is not None:
            return self._forward_onto(x, residual, skip, coordinates)
        cm, ts = x.coordinate_manager, x.tensor_stride
        cin, cout = self.in_channels, self.out_channels
        ks, stride = self.kernel_size, self.stride
        # (the three layers of the reference's models first, as they always were: a model step makes this call ~100 times)
        if ks == 3 and stride == 1 and self.dilation == 1:
            nbr = cm.k3(ts)
            V = cm.size(ts)
            spec = Fn.ConvSpec(nbr, nbr, V, V, 27, cin, cout, True)
            out_ts = ts
        elif ks == 2 and stride == 2 and self.dilation == 1:
            down, up = cm.k2(ts)
            spec = Fn.ConvSpec(down, up, cm.size(ts), cm.size(2 * ts), 8, cin, cout, False)
            out_ts = 2 * ts
        elif ks == 1 and stride == 1:
            ident = cm.identity(ts)
            V = cm.size(ts)
            spec = Fn.ConvSpec(ident, ident, V, V, 1, cin, cout, False)
            out_ts = ts
        else:
            spec, out_ts = self._spec(cm, ts)
        feats, kernel, pending = x._F, self._kernel(), x._pending
        if cin % 16 != 0 and cin < 16 and self.kernel_volume > 1 and pending is None and spec.vout >= 30000:
            # the network's input convolution (6 channels) at full resolution: zero-padding rows and weights to one
            # 16-channel chunk lets it take the aligned pair-list kernels (16-byte row gathers) instead of the
            # scalar-load table walk; the padded weight rows see zeros, autograd slices their gradient away
            pad = 16 - cin
            feats = torch.nn.functional.pad(feats, (0, pad))
            kernel = torch.nn.functional.pad(kernel, (0, 0, 0, pad))
            spec = Fn.ConvSpec(spec.nbr_fwd, spec.nbr_bwd, spec.vin, spec.vout, spec.K, 16, cout, spec.mirror, spec.sub)
        if skip is not None and feats is not x._F:
            skip = None            # (padded input rows: not the skipped tensor any more)
        y, stats = Fn.conv(feats, kernel, spec, pending,
                           residual=None if residual is None else residual._raw(), want_stats=self.training, skip=skip,
                           bias=self.bias)
        return x._like(y, tensor_stride=out_ts, stats=stats)


class MinkowskiConvolutionTranspose(_ConvBase):
    """stride-2 transposed convolution of any kernel size: the output lives on the cached coordinate set of stride ts/2
    (the encoder's) and the table is the inverse of the matching strided map.  A transposed convolution that would have to
    CREATE coordinates (stride 1, or an input that was never downsampled from a finer set) is not supported -- unless the
    caller names the output set or asks for all of it:

    forward(x, coordinates) / forward(x, coordinates=target): onto an integer tensor [M, 4], a CoordinateMapKey or a
    SparseTensor (tensor.target_key) at tensor stride ts // stride, at stride 1 or 2: out[o] = bias + sum_k x[o - off_k] W[k],
    off = kernel_offsets(kernel_size, dilation, ts // stride) -- the rule of generate(); the cached finer set of the same
    manager at stride 2 takes the ordinary path.  expand_coordinates=True: the code path of
    MinkowskiGenerativeConvolutionTranspose (the same CoordinateManager.generate entry, hence the same output manager)."""

    def forward(self, x: SparseTensor, coordinates=None):
        cm, ts = x.coordinate_manager, x.tensor_stride
        if coordinates is not None or self.expand_coordinates:
            if coordinates is not None and self.expand_coordinates:
                raise ValueError("MinkowskiConvolutionTranspose: expand_coordinates=True derives the output set, coordinates= "
                                 "names it: not both")
            if coordinates is None:
                return MinkowskiGenerativeConvolutionTranspose.forward(self, x)
            out_ts = _transposed_stride(self, ts)
            key = target_key(coordinates, out_ts, x.device)
            if not (key.coordinate_manager is cm and self.stride == 2):
                return self._conv_onto(x, key.coordinate_manager, out_ts,
                                       cm.target_map(ts, key, self.kernel_size, self.stride, self.dilation, transposed=True,
                                                     region=self.region))
            # (the cached finer set of this manager: the ordinary path below)
        if self.stride != 2 or ts % 2 != 0 or (ts // 2) not in cm.coords:
            raise NotImplementedError(f"MinkowskiConvolutionTranspose(kernel_size={self.kernel_size}, stride={self.stride}) on "
                                      f"tensor stride {ts}: only stride 2 onto a cached finer coordinate set; generating "
                                      "new coordinates is not supported")
        fine = ts // 2
        fwd, _ = self._spec(cm, fine)      # the strided map fine -> ts (cached by the encoder's strided convolution)
        spec = Fn.ConvSpec(fwd.nbr_bwd, fwd.nbr_fwd, fwd.vout, fwd.vin, fwd.K, self.in_channels, self.out_channels, False,
                           fwd.sub)
        y, stats = Fn.conv(x._F, self._kernel(), spec, x._pending, want_stats=self.training, bias=self.bias)
        return x._like(y, tensor_stride=fine, stats=stats)


def _transposed_stride(layer, ts):
    """output tensor stride of a transposed layer onto given coordinates; an input stride the layer's stride does not divide
    is refused in the wording of CoordinateManager.generate"""
    if ts % layer.stride != 0:
        raise NotImplementedError(f"kernel_size={layer.kernel_size}, stride={layer.stride}, dilation={layer.dilation} on tensor "
                                  f"stride {ts}: a generative stride-2 layer needs an even tensor stride")
    return ts // layer.stride


class MinkowskiGenerativeConvolutionTranspose(_ConvBase):
    """transposed convolution that CREATES its output coordinates: out[c + off_k] += x[c] @ W[k] over every input row c and
    every kernel offset, off = kernel_offsets(kernel_size, dilation, ts // stride) -- the arithmetic of
    MinkowskiConvolutionTranspose, on the set of all coordinates the kernel reaches instead of a cached one.  Stride 1 (odd
    kernel sizes) keeps the tensor stride, stride 2 halves it (the input's must be even).  The output lives on its own
    coordinate manager, rooted at the output tensor stride and shared by every generative layer of the same geometry on the
    same input; it is usually followed by MinkowskiPruning."""
    _two_sets = True

    def forward(self, x: SparseTensor):
        cm, ts = x.coordinate_manager, x.tensor_stride
        out_cm, nbr_fwd, nbr_bwd, vin, vout, K, out_ts = cm.generate(ts, self.kernel_size, self.stride, self.dilation,
                                                                     region=self.region)
        # (sub = False: a K = 27 table between two different sets stays off the submanifold backward-weight route)
        spec = Fn.ConvSpec(nbr_fwd, nbr_bwd, vin, vout, K, self.in_channels, self.out_channels, False, False)
        y, stats = Fn.conv(x._F, self._kernel(), spec, x._pending, want_stats=self.training, bias=self.bias)
        return SparseTensor(y, coordinate_manager=out_cm, tensor_stride=out_ts, _stats=stats)


class MinkowskiChannelwiseConvolution(nn.Module):
    """Depthwise convolution: out[o, c] = bias[c] + sum_k kernel[k, c] * in[nbr[k][o], c] over the inputs present, offsets in
    kernel_offsets() order (x fastest).  `kernel` has shape (K, in_channels), K = kernel_size ** 3 -- (1, in_channels) for
    kernel size 1, always 2-D -- and `bias`, when asked for, (1, in_channels); both are initialised uniform(-s, s) with
    s = 1 / sqrt(in_channels * K), the rule of the dense-weight convolutions.  The geometries are the convolutions': stride 1
    with an odd kernel on the same coordinate set, stride 2 onto the stride-2 set, any dilation.  A pending BatchNorm / ReLU in
    front is materialised first.  The arithmetic is float32 always (there is no matrix product for
    torch.set_float32_matmul_precision to act on).

    Not a _ConvBase: prepare_conv_weights lays out (K, cin, cout) weight images and deferred backward-weight groups for every
    _ConvBase, and a (K, C) kernel has no place in either."""

    def __init__(self, in_channels, kernel_size=-1, stride=1, dilation=1, bias=False, dimension=3, kernel_generator=None):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError(f"dimension={dimension}: only 3-D sparse tensors are supported")
        kernel_size, stride, dilation, self.region, _, K = _layer_geometry(type(self).__name__, kernel_size, stride, dilation,
                                                                          kernel_generator)
        self.in_channels = self.out_channels = in_channels
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation
        self.kernel_volume = K
        self.kernel = nn.Parameter(torch.empty((K, in_channels), dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty((1, in_channels), dtype=torch.float32)) if bias else None
        s = 1.0 / math.sqrt(in_channels * K)
        with torch.no_grad():
            self.kernel.uniform_(-s, s)
            if bias:
                self.bias.uniform_(-s, s)

    def forward(self, x: SparseTensor, coordinates=None):
        """coordinates: the set to write onto (an integer tensor [M, 4], a CoordinateMapKey or a SparseTensor at tensor stride
        ts * stride, tensor.target_key); a row no input reaches is the bias"""
        cm, ts = x.coordinate_manager, x.tensor_stride
        geom = (self.kernel_size, self.stride, self.dilation)
        if coordinates is not None:
            key = target_key(coordinates, ts * self.stride, x.device)
            if key.coordinate_manager is not cm:
                nbr_fwd, nbr_inv, vin, vout, K = cm.target_map(ts, key, *geom, region=self.region)
                if vout == 0:
                    y = x._raw()[:0] * self.kernel[:1]
                    y = y if self.bias is None else y + self.bias
                else:
                    y = Fn.channelwise_conv(x._raw(), self.kernel, self.bias, nbr_fwd, nbr_inv, vin, vout, K)
                return SparseTensor(y, coordinate_manager=key.coordinate_manager, tensor_stride=key.tensor_stride)
        nbr_fwd, _, vin, vout, K, out_ts, _ = cm.kernel_map_tables(ts, *geom, region=self.region)
        nbr_inv = cm.kernel_map_inverse(ts, *geom, region=self.region)
        y = Fn.channelwise_conv(x._raw(), self.kernel, self.bias, nbr_fwd, nbr_inv, vin, vout, K)
        return x._like(y, tensor_stride=out_ts)

    def extra_repr(self):
        return (f"in={self.in_channels}, kernel_size={self.kernel_size}, stride={self.stride}, dilation={self.dilation}, "
                f"bias={self.bias is not None}" + _region_name(self.region))


def kernel_attention(q, k, v, num_heads, rel_bias=None, scale=None, kernel_size=3, stride=1, dilation=1, kernel_generator=None):
    """Local multi-head attention over a kernel map (an engine extra: MinkowskiEngine has no such layer).  Row o of q attends
    to the rows of k / v that the kernel's offsets reach from its coordinate -- the inputs a convolution of the same geometry
    would sum for it --:  out[o, h, :] = sum_kk softmax_kk(scale * <q[o, h], k[i, h]> + rel_bias[kk, h]) * v[i, h, :], the
    softmax over the inputs PRESENT; a row that reaches none is zero.  q, k, v: SparseTensors of the same channel count C =
    num_heads * D; k and v on one coordinate set of tensor stride ts; q on the same manager at ts * stride (the layer's own
    output set: kernel_map_tables / kernel_map_inverse), or on any set of another manager at that stride (target_map).
    rel_bias: a float32 tensor (K, num_heads) in the kernel's offset order, or None; scale defaults to D ** -0.5.
    -> a SparseTensor on q's coordinate set.  A pending BatchNorm / ReLU on q, k or v is materialised first.  float32 HIP gather
    kernels without atomics (csrc/kattn.hip): forward and every gradient are the same bytes on every run.
    Not offered: attention dropout, masks, a value head dimension other than D, float16 / bfloat16 rows, gradients through the
    coordinates."""
    # (the default kernel size beside a generator is "not given", as in CoordinateManager.kernel_map(in_key, out_key, ...))
    given_ks = -1 if kernel_generator is not None and kernel_size == 3 else kernel_size
    kernel_size, stride, dilation, region, _, K = _layer_geometry("kernel_attention", given_ks, stride, dilation,
                                                                  kernel_generator)
    cm, ts = k.coordinate_manager, k.tensor_stride
    if v.coordinate_manager is not cm or v.tensor_stride != ts:
        raise ValueError("kernel_attention: k and v must be on the same coordinate set (one manager, one tensor stride)")
    C = k._F.size(1)
    if q._F.size(1) != C or v._F.size(1) != C:
        raise ValueError(f"kernel_attention: q, k and v must have the same number of channels, got {q._F.size(1)}, {C}, "
                         f"{v._F.size(1)}")
    if not isinstance(num_heads, int) or num_heads < 1 or C % num_heads != 0:
        raise ValueError(f"kernel_attention: {C} channels do not divide into num_heads={num_heads}")
    if q.tensor_stride != ts * stride:
        raise ValueError(f"kernel_attention: q is at tensor stride {q.tensor_stride}, k and v at {ts}: stride={stride} needs q "
                         f"at {ts * stride}")
    if rel_bias is not None and tuple(rel_bias.shape) != (K, num_heads):
        raise ValueError(f"kernel_attention: rel_bias must have shape (K, num_heads) = ({K}, {num_heads}), got "
                         f"{tuple(rel_bias.shape)}")
    if scale is None:
        scale = (C // num_heads) ** -0.5
    geom = (kernel_size, stride, dilation)
    if q.coordinate_manager is cm:
        nbr_fwd, _, vin, vout, K, _, _ = cm.kernel_map_tables(ts, *geom, region=region)
        nbr_inv = cm.kernel_map_inverse(ts, *geom, region=region)
    else:
        nbr_fwd, nbr_inv, vin, vout, K = cm.target_map(ts, q.coordinate_map_key, *geom, region=region)
    rows = q._raw()
    y = rows[:0] if vout == 0 else Fn.kernel_attention_rows(rows, k._raw(), v._raw(), rel_bias, nbr_fwd, nbr_inv, vin, vout, K,
                                                            num_heads, float(scale))
    return q._like(y)


class MinkowskiKernelAttention(nn.Module):
    """The stride-1 self-attention block on the tensor's own coordinate set (an engine extra: MinkowskiEngine has no such
    layer): forward(x) = proj(kernel_attention(q, k, v)) with (q, k, v) = the three C-wide column blocks of qkv(x).  `qkv` is
    nn.Linear(C, 3C) (bias when qkv_bias), `proj` nn.Linear(C, C), `rel_bias` a (K, num_heads) parameter initialised to zero --
    one learned bias per kernel offset and head, absent with rel_pos_bias=False; scale = (C / num_heads) ** -0.5.  The
    geometries are the stride-1 convolutions' (an odd kernel size, any dilation, a cross or custom region through
    kernel_generator=).

    Not a _ConvBase: prepare_conv_weights lays out (K, cin, cout) weight images, and this block has none."""

    def __init__(self, in_channels, num_heads, kernel_size=3, dilation=1, qkv_bias=True, rel_pos_bias=True, dimension=3,
                 kernel_generator=None):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError(f"dimension={dimension}: only 3-D sparse tensors are supported")
        given_ks = -1 if kernel_generator is not None and kernel_size == 3 else kernel_size
        kernel_size, stride, dilation, self.region, _, K = _layer_geometry(type(self).__name__, given_ks, 1, dilation,
                                                                          kernel_generator)
        if stride != 1:
            raise ValueError(f"{type(self).__name__}: a self-attention block works at stride 1, the kernel_generator has "
                             f"stride={stride}")
        if not isinstance(num_heads, int) or num_heads < 1 or in_channels % num_heads != 0:
            raise ValueError(f"{type(self).__name__}: {in_channels} channels do not divide into num_heads={num_heads}")
        self.in_channels = self.out_channels = in_channels
        self.num_heads = num_heads
        self.kernel_size, self.stride, self.dilation = kernel_size, 1, dilation
        self.kernel_volume = K
        self.kernel_generator = kernel_generator
        self.scale = (in_channels // num_heads) ** -0.5
        self.qkv = nn.Linear(in_channels, 3 * in_channels, bias=qkv_bias)
        self.proj = nn.Linear(in_channels, in_channels)
        self.rel_bias = nn.Parameter(torch.zeros((K, num_heads), dtype=torch.float32)) if rel_pos_bias else None

    def forward(self, x: SparseTensor):
        C = self.in_channels
        q, k, v = (x._like(t.contiguous()) for t in self.qkv(x._raw()).split(C, dim=1))
        y = kernel_attention(q, k, v, self.num_heads, self.rel_bias, self.scale, self.kernel_size, 1, self.dilation,
                             self.kernel_generator)
        return x._like(self.proj(y._raw()))

    def extra_repr(self):
        return (f"in={self.in_channels}, num_heads={self.num_heads}, kernel_size={self.kernel_size}, dilation={self.dilation}, "
                f"rel_pos_bias={self.rel_bias is not None}" + _region_name(self.region))


_QATTN_MAX_D, _QATTN_MAX_Q, _QATTN_MAX_C, _QATTN_MAX_B = 128, 1024, 1024, 65535      # the limits of csrc/qattn.hip


def query_attention(queries, k, v, num_heads, attn_mask=None, scale=None, dropout=0.0):
    """Per-sample multi-head attention of a fixed number of queries over the voxels of their own sample (an engine extra:
    MinkowskiEngine has no such layer) -- the decoder step of a mask transformer.  k, v: SparseTensors on one coordinate set
    (one manager, one tensor stride) with V rows of C = num_heads * D float32 channels.  queries: a float32 tensor [B, Q, C] on
    the same device; B is the number of batch indices PRESENT in the set and queries[b] belongs to the b-th of them in ascending
    order -- the numbering of CoordinateManager.batch_rows, of origin_map and of the MinkowskiGlobal*Pooling output rows,
    whatever gaps the batch indices have and wherever the rows of a sample lie.  For sample b, query q, head h, over the rows i
    of that sample:  out[b, q, hD:hD+D] = sum_i softmax_i(scale * <queries[b, q, hD:hD+D], k[i, hD:hD+D]>) * v[i, hD:hD+D], scale =
    D ** -0.5 unless given.  -> a float32 tensor [B, Q, C].

    attn_mask: a bool tensor [V, Q] or None: row i is the i-th row of k.F / k.C as the caller sees them, column q the query of
    that row's own sample, True = may NOT attend (torch's convention), one mask for all heads -- the layout in which a mask
    transformer makes its mask (voxel features times query embeddings).  A (b, q) whose rows are all blocked gives out = 0,
    contributes to no gradient and receives none -- the rule of kernel_attention for a row that reaches no input, and NOT that
    of torch.nn.MultiheadAttention, which gives NaN there; a caller who wants "attend everywhere instead" clears those
    mask columns first.

    Gradients flow to queries, k.F and v.F.  A pending BatchNorm / ReLU on k or v is materialised first.  float32 HIP kernels
    without atomics (csrc/qattn.hip): the rows are read where the manager holds them, nothing of size V x Q is stored, forward
    and every gradient are the same bytes on every run.  D <= 128, Q <= 1024, C <= 1024, B <= 65535.
    Not offered: a different Q per sample (pad the queries and block the padding's columns), float or per-head masks, attention
    dropout, a value head dimension other than D, float16 / bfloat16, CPU tensors.  The reverse direction (voxels attending to
    queries) is voxel_attention."""
    name = "query_attention"
    if isinstance(queries, SparseTensor) or not isinstance(k, SparseTensor) or not isinstance(v, SparseTensor):
        raise TypeError(f"{name}: queries is a dense tensor [B, Q, C], k and v are SparseTensors; the reverse direction (voxels "
                        "attending to queries) is voxel_attention(x, keys, values, ...)")
    if isinstance(queries, (list, tuple)):
        raise NotImplementedError(f"{name}: a different Q per sample (a list of query tensors) is not offered: pad the queries to "
                                  "one Q and block the padding's columns in attn_mask")
    if not torch.is_tensor(queries):
        raise TypeError(f"{name}: queries must be a float32 tensor [B, Q, C], got {type(queries).__name__}")
    if dropout:
        raise NotImplementedError(f"{name}: attention dropout (dropout={dropout}) is not offered")
    cm, ts = k.coordinate_manager, k.tensor_stride
    if v.coordinate_manager is not cm or v.tensor_stride != ts:
        raise ValueError(f"{name}: k and v must be on the same coordinate set (one manager, one tensor stride)")
    for what, t in (("queries", queries), ("k", k._F), ("v", v._F)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: {what} is {t.dtype}; float32 only (float16 / bfloat16 are not offered)")
    V, C = k._F.shape
    if v._F.size(1) != C:
        raise ValueError(f"{name}: v has {v._F.size(1)} channels, k has {C}: a value head dimension different from D is not "
                         "offered")
    if queries.dim() != 3 or queries.size(2) != C:
        raise ValueError(f"{name}: queries must have shape [B, Q, C] with C = {C}, the channels of k and v, got "
                         f"{tuple(queries.shape)}")
    if not isinstance(num_heads, int) or num_heads < 1 or C % num_heads != 0:
        raise ValueError(f"{name}: {C} channels do not divide into num_heads={num_heads}")
    if queries.device != k._F.device:
        raise ValueError(f"{name}: queries are on {queries.device}, k and v on {k._F.device}")
    group = cm.batch_group(ts)
    B, Q, D = group.B, queries.size(1), C // num_heads
    if queries.size(0) != B:
        raise ValueError(f"{name}: queries has B = {queries.size(0)} samples, the coordinate set holds {B} batch indices")
    if attn_mask is not None:
        if not torch.is_tensor(attn_mask) or attn_mask.dtype != torch.bool:
            raise TypeError(f"{name}: attn_mask must be a bool tensor [V, Q] (True = may not attend), got "
                            f"{getattr(attn_mask, 'dtype', type(attn_mask).__name__)}; float masks are not offered")
        if attn_mask.dim() == 3:
            raise ValueError(f"{name}: attn_mask has shape {tuple(attn_mask.shape)}; per-head masks are not offered, one [V, Q] "
                             "mask serves all heads")
        if tuple(attn_mask.shape) != (V, Q):
            raise ValueError(f"{name}: attn_mask must have shape [V, Q] = [{V}, {Q}], got {list(attn_mask.shape)}")
        if attn_mask.device != k._F.device:
            raise ValueError(f"{name}: attn_mask is on {attn_mask.device}, k and v on {k._F.device}")
    for what, got, cap in (("head dimension D", D, _QATTN_MAX_D), ("Q", Q, _QATTN_MAX_Q), ("C = num_heads * D", C, _QATTN_MAX_C),
                           ("B", B, _QATTN_MAX_B)):
        if got > cap:
            raise ValueError(f"{name}: {what} = {got} is above the kernels' limit of {cap}")
    if B == 0 or Q == 0:
        return queries.new_zeros((B, Q, C))
    be = get_backend()
    if not hasattr(be, "qattn_forward") or not k._F.is_cuda:
        raise NotImplementedError(f"{name} needs the HIP backend and device tensors, CPU tensors are not offered "
                                  "(ms3d_qattn_forward)")
    if scale is None:
        scale = D ** -0.5
    mask = None if attn_mask is None else attn_mask.contiguous()
    return Fn.query_attention_rows(queries, k._raw(), v._raw(), mask, group, num_heads, float(scale))


class MinkowskiQueryAttention(nn.Module):
    """The cross-attention block of a mask-transformer decoder (an engine extra: MinkowskiEngine has no such layer):
    forward(queries, x, attn_mask=None) = out_proj(query_attention(q_proj(queries), k_proj(x), v_proj(x), num_heads,
    attn_mask)) -> [B, Q, embed_dim].  `q_proj` and `out_proj` are nn.Linear(embed_dim, embed_dim), `k_proj` and `v_proj`
    nn.Linear(in_channels, embed_dim) applied to the rows of the SparseTensor x (in_channels defaults to embed_dim); `bias`
    switches the bias of all four.  Positional terms are the caller's to add (x + pos works on a SparseTensor); a query whose
    rows are all blocked comes out as out_proj's bias (query_attention gives zero there, not NaN).  The reverse direction
    (voxels attending to queries) is MinkowskiVoxelAttention.

    Not a _ConvBase: prepare_conv_weights lays out (K, cin, cout) weight images, and this block has none."""

    def __init__(self, embed_dim, num_heads, in_channels=None, bias=True, dropout=0.0):
        super().__init__()
        if dropout:
            raise NotImplementedError(f"{type(self).__name__}: attention dropout (dropout={dropout}) is not offered")
        if not isinstance(num_heads, int) or num_heads < 1 or embed_dim % num_heads != 0:
            raise ValueError(f"{type(self).__name__}: {embed_dim} channels do not divide into num_heads={num_heads}")
        self.embed_dim = int(embed_dim)
        self.in_channels = self.embed_dim if in_channels is None else int(in_channels)
        self.num_heads = num_heads
        self.q_proj = nn.Linear(self.embed_dim, self.embed_dim, bias=bias)
        self.k_proj = nn.Linear(self.in_channels, self.embed_dim, bias=bias)
        self.v_proj = nn.Linear(self.in_channels, self.embed_dim, bias=bias)
        self.out_proj = nn.Linear(self.embed_dim, self.embed_dim, bias=bias)

    def forward(self, queries, x: SparseTensor, attn_mask=None):
        if not isinstance(x, SparseTensor) or isinstance(queries, SparseTensor):
            raise TypeError(f"{type(self).__name__}: forward(queries, x) takes a dense tensor [B, Q, C] and a SparseTensor; the "
                            "reverse direction (voxels attending to queries) is MinkowskiVoxelAttention")
        if x._F.size(1) != self.in_channels:
            raise ValueError(f"{type(self).__name__}: the input has {x._F.size(1)} channels, the layer in_channels="
                             f"{self.in_channels}")
        rows = x._raw()
        k, v = x._like(self.k_proj(rows)), x._like(self.v_proj(rows))
        return self.out_proj(query_attention(self.q_proj(queries), k, v, self.num_heads, attn_mask))

    def extra_repr(self):
        return f"embed_dim={self.embed_dim}, num_heads={self.num_heads}, in_channels={self.in_channels}"


def voxel_attention(x, keys, values, num_heads, attn_mask=None, scale=None, dropout=0.0):
    """Per-sample multi-head attention of every voxel over the queries of its own sample (an engine extra: MinkowskiEngine has
    no such layer) -- the reverse direction of query_attention, the second leg of a two-way mask-transformer decoder: the voxel
    features read the refined queries back.  x: a SparseTensor with V rows of C = num_heads * D float32 channels.  keys, values:
    float32 tensors [B, Q, C] on the same device; B is the number of batch indices PRESENT in x's coordinate set and keys[b]
    belongs to the b-th of them in ascending order -- the numbering of query_attention, of CoordinateManager.batch_rows, of
    origin_map and of the MinkowskiGlobal*Pooling output rows.  For row i of sample b, head h, over the queries q:
    out[i, hD:hD+D] = sum_q softmax_q(scale * <x[i, hD:hD+D], keys[b, q, hD:hD+D]>) * values[b, q, hD:hD+D], scale = D ** -0.5
    unless given.  -> a SparseTensor on x's coordinate set, its rows in the caller's order as x's are.

    attn_mask: the very object query_attention takes, so one mask serves both legs: a bool tensor [V, Q] or None, row i the
    i-th row of x.F / x.C as the caller sees them, column q the query of that row's own sample, True = may NOT attend, one
    mask for all heads.  A row whose queries are all blocked gives out = 0, contributes to no gradient and receives none --
    NOT the NaN of torch.nn.MultiheadAttention; a (b, q) that no row of its sample may attend to gets a zero gradient.

    Gradients flow to x.F, keys and values.  A pending BatchNorm / ReLU on x is materialised first.  float32 HIP kernels
    without atomics (csrc/vattn.hip): the rows are read where the manager holds them, nothing of size V x Q is stored, forward
    and every gradient are the same bytes on every run.  D <= 128, Q <= 1024, C <= 1024, B <= 65535.
    Not offered: a different Q per sample (pad the queries and block the padding's columns), float or per-head masks, attention
    dropout, a value head dimension other than D, float16 / bfloat16, CPU tensors."""
    name = "voxel_attention"
    if not isinstance(x, SparseTensor) or isinstance(keys, SparseTensor) or isinstance(values, SparseTensor):
        raise TypeError(f"{name}: x is a SparseTensor, keys and values are dense tensors [B, Q, C]; queries attending to voxels is "
                        "query_attention(queries, k, v, ...)")
    if isinstance(keys, (list, tuple)) or isinstance(values, (list, tuple)):
        raise NotImplementedError(f"{name}: a different Q per sample (a list of query tensors) is not offered: pad the queries to "
                                  "one Q and block the padding's columns in attn_mask")
    if not torch.is_tensor(keys) or not torch.is_tensor(values):
        raise TypeError(f"{name}: keys and values must be float32 tensors [B, Q, C], got {type(keys).__name__} and "
                        f"{type(values).__name__}")
    if dropout:
        raise NotImplementedError(f"{name}: attention dropout (dropout={dropout}) is not offered")
    cm, ts = x.coordinate_manager, x.tensor_stride
    for what, t in (("x", x._F), ("keys", keys), ("values", values)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: {what} is {t.dtype}; float32 only (float16 / bfloat16 are not offered)")
    V, C = x._F.shape
    if keys.dim() != 3 or keys.size(2) != C:
        raise ValueError(f"{name}: keys must have shape [B, Q, C] with C = {C}, the channels of x, got {tuple(keys.shape)}")
    if tuple(values.shape) != tuple(keys.shape):
        raise ValueError(f"{name}: values has shape {tuple(values.shape)}, keys {tuple(keys.shape)}: keys.shape != values.shape, "
                         "a value head dimension different from D is not offered")
    if not isinstance(num_heads, int) or num_heads < 1 or C % num_heads != 0:
        raise ValueError(f"{name}: {C} channels do not divide into num_heads={num_heads}")
    if keys.device != x._F.device or values.device != x._F.device:
        raise ValueError(f"{name}: keys and values are on {keys.device} and {values.device}, x on {x._F.device}")
    group = cm.batch_group(ts)
    B, Q, D = group.B, keys.size(1), C // num_heads
    if keys.size(0) != B:
        raise ValueError(f"{name}: keys has B = {keys.size(0)} samples, the coordinate set holds {B} batch indices")
    if attn_mask is not None:
        if not torch.is_tensor(attn_mask) or attn_mask.dtype != torch.bool:
            raise TypeError(f"{name}: attn_mask must be a bool tensor [V, Q] (True = may not attend), got "
                            f"{getattr(attn_mask, 'dtype', type(attn_mask).__name__)}; float masks are not offered")
        if attn_mask.dim() == 3:
            raise ValueError(f"{name}: attn_mask has shape {tuple(attn_mask.shape)}; per-head masks are not offered, one [V, Q] "
                             "mask serves all heads")
        if tuple(attn_mask.shape) != (V, Q):
            raise ValueError(f"{name}: attn_mask must have shape [V, Q] = [{V}, {Q}], got {list(attn_mask.shape)}")
        if attn_mask.device != x._F.device:
            raise ValueError(f"{name}: attn_mask is on {attn_mask.device}, x on {x._F.device}")
    for what, got, cap in (("head dimension D", D, _QATTN_MAX_D), ("Q", Q, _QATTN_MAX_Q), ("C = num_heads * D", C, _QATTN_MAX_C),
                           ("B", B, _QATTN_MAX_B)):
        if got > cap:
            raise ValueError(f"{name}: {what} = {got} is above the kernels' limit of {cap}")
    if B == 0 or Q == 0:
        return x._like(x._F.new_zeros((V, C)))
    be = get_backend()
    if not hasattr(be, "vattn_forward") or not x._F.is_cuda:
        raise NotImplementedError(f"{name} needs the HIP backend and device tensors, CPU tensors are not offered "
                                  "(ms3d_vattn_forward)")
    if scale is None:
        scale = D ** -0.5
    group.chunks                    # the kv pass sweeps them: their one host read is made here, not inside the backward
    mask = None if attn_mask is None else attn_mask.contiguous()
    return x._like(Fn.voxel_attention_rows(x._raw(), keys, values, mask, group, num_heads, float(scale)))


class MinkowskiVoxelAttention(nn.Module):
    """The second leg of a two-way mask-transformer decoder, the mirror of MinkowskiQueryAttention (an engine extra:
    MinkowskiEngine has no such layer): forward(x, queries, attn_mask=None) = out_proj(voxel_attention(q_proj(x),
    k_proj(queries), v_proj(queries), num_heads, attn_mask)) -> a SparseTensor of embed_dim channels on x's coordinate set.
    `q_proj` and `out_proj` are nn.Linear(embed_dim, embed_dim) applied to the rows of the SparseTensor x, `k_proj` and `v_proj`
    nn.Linear(query_channels, embed_dim) applied to the dense queries [B, Q, query_channels] (query_channels defaults to
    embed_dim); `bias` switches the bias of all four.  A row whose queries are all blocked comes out as out_proj's bias
    (voxel_attention gives zero there, not NaN).

    Not a _ConvBase: prepare_conv_weights lays out (K, cin, cout) weight images, and this block has none."""

    def __init__(self, embed_dim, num_heads, query_channels=None, bias=True, dropout=0.0):
        super().__init__()
        if dropout:
            raise NotImplementedError(f"{type(self).__name__}: attention dropout (dropout={dropout}) is not offered")
        if not isinstance(num_heads, int) or num_heads < 1 or embed_dim % num_heads != 0:
            raise ValueError(f"{type(self).__name__}: {embed_dim} channels do not divide into num_heads={num_heads}")
        self.embed_dim = int(embed_dim)
        self.query_channels = self.embed_dim if query_channels is None else int(query_channels)
        self.num_heads = num_heads
        self.q_proj = nn.Linear(self.embed_dim, self.embed_dim, bias=bias)
        self.k_proj = nn.Linear(self.query_channels, self.embed_dim, bias=bias)
        self.v_proj = nn.Linear(self.query_channels, self.embed_dim, bias=bias)
        self.out_proj = nn.Linear(self.embed_dim, self.embed_dim, bias=bias)

    def forward(self, x: SparseTensor, queries, attn_mask=None):
        if not isinstance(x, SparseTensor) or isinstance(queries, SparseTensor):
            raise TypeError(f"{type(self).__name__}: forward(x, queries) takes a SparseTensor and a dense tensor [B, Q, C]; queries "
                            "attending to voxels is MinkowskiQueryAttention")
        if x._F.size(1) != self.embed_dim:
            raise ValueError(f"{type(self).__name__}: the input has {x._F.size(1)} channels, the layer embed_dim={self.embed_dim}")
        if not torch.is_tensor(queries) or queries.dim() != 3 or queries.size(2) != self.query_channels:
            raise ValueError(f"{type(self).__name__}: queries must have shape [B, Q, {self.query_channels}] (query_channels), got "
                             f"{tuple(queries.shape) if torch.is_tensor(queries) else type(queries).__name__}")
        q = x._like(self.q_proj(x._raw()))
        y = voxel_attention(q, self.k_proj(queries), self.v_proj(queries), self.num_heads, attn_mask)
        return y._like(self.out_proj(y._raw()))

    def extra_repr(self):
        return f"embed_dim={self.embed_dim}, num_heads={self.num_heads}, query_channels={self.query_channels}"


class MinkowskiPruning(nn.Module):
    """forward(x, mask): the rows of x whose entry of the bool mask [V] is set -- mask in the order of x.features /
    x.coordinates -- on a coordinate manager of their own, rooted at x's tensor stride.  .features is x.features[mask] and
    .coordinates is x.coordinates[mask] bit for bit; dropped rows receive a zero gradient.  A pending BatchNorm / ReLU is
    materialised first."""

    def forward(self, x: SparseTensor, mask):
        cm, ts = x.coordinate_manager, x.tensor_stride
        be = get_backend()
        if not hasattr(be, "coords_prune"):
            raise NotImplementedError("MinkowskiPruning needs the HIP backend (ms3d_coords_prune)")
        coords = x.coordinates
        if mask.dtype != torch.bool or mask.dim() != 1 or mask.numel() != coords.size(0):
            raise ValueError(f"MinkowskiPruning: the mask must be bool [{coords.size(0)}], one entry per row of the input")
        out_coords, src_row, _ = be.coords_prune(coords, mask.to(coords.device))
        idx = src_row.long()
        if ts == 1 and cm.inv is not None:
            # the mask (and the rows that come out) are in the caller's order, the features are held in the engine's: one
            # gather through the composed index instead of un-permuting all rows first
            idx = cm.inv[idx]
        y = Fn.select_rows(x._raw(), idx)
        return SparseTensor(y, coordinate_manager=type(cm).rooted(out_coords, ts), tensor_stride=ts)


class MinkowskiToSparseTensor(nn.Module):
    """forward(x): dense [B, C, X, Y, Z] -> SparseTensor at tensor stride 1 on a new manager: the cells with a non-zero channel
    (remove_zeros=True: to_sparse) or every cell (remove_zeros=False: to_sparse_all); coordinates (int [n, 4]): exactly those
    cells, in that order.  Gradients flow to x."""

    def __init__(self, remove_zeros=True, coordinates=None):
        super().__init__()
        self.remove_zeros = remove_zeros
        self.coordinates = coordinates

    def forward(self, x):
        if self.coordinates is not None:
            return to_sparse(x, coordinates=self.coordinates)
        return to_sparse(x) if self.remove_zeros else to_sparse_all(x)

    def extra_repr(self):
        return f"remove_zeros={self.remove_zeros}"


class MinkowskiToDenseTensor(nn.Module):
    """forward(x): SparseTensor -> its dense tensor [B, C, X, Y, Z] alone: x.dense(shape=shape)[0], so the origin is the
    per-axis minimum of x's coordinates (SparseTensor.dense); shape: torch.Size / tuple (B, C, X, Y, Z) or None."""

    def __init__(self, shape=None):
        super().__init__()
        self.shape = None if shape is None else tuple(int(v) for v in shape)

    def forward(self, x: SparseTensor):
        return x.dense(shape=self.shape)[0]

    def extra_repr(self):
        return f"shape={self.shape}"


class MinkowskiToFeature(nn.Module):
    """forward(x): x.F -- the feature rows in the caller's order, for the torch layers behind a sparse network"""

    def forward(self, x: SparseTensor):
        return x.F


class MinkowskiBatchNorm(nn.Module):
    """BatchNorm1d over the rows of .F.  Statistics are reduced by a HIP kernel now; normalisation itself is
    deferred to the consumer (see tensor.py)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)
        # `num_batches_tracked += 1` is one tiny launch per BatchNorm per step (80 per step in the backbone); the
        # count is kept on the host and added to the buffer whenever somebody reads it (state_dict / checkpoint)
        self._pending_batches = 0
        self.register_state_dict_pre_hook(lambda module, prefix, keep_vars: module.flush_batches_tracked())
        # a loaded num_batches_tracked replaces the count, it is not added to what this instance had pending
        self.register_load_state_dict_pre_hook(lambda module, *a, **k: setattr(module, "_pending_batches", 0))

    def flush_batches_tracked(self):
        if self._pending_batches and self.bn.num_batches_tracked is not None:
            self.bn.num_batches_tracked += self._pending_batches
        self._pending_batches = 0

    def forward(self, x: SparseTensor):
        bn = self.bn
        feats = x._raw()  # materialise anything pending in front of this BN (engine row order)
        use_batch = self.training or not bn.track_running_stats
        if use_batch:
            with torch.no_grad():
                rm = bn.running_mean if (self.training and bn.track_running_stats) else None
                rv = bn.running_var if rm is not None else None
                if bn.momentum is None:     # cumulative moving average: 1 / (batches seen so far, this one included)
                    seen = self._pending_batches + (int(bn.num_batches_tracked) if rm is not None else 0)
                    mom = 1.0 / (seen + 1)
                else:
                    mom = bn.momentum
                g = bn.weight.detach() if bn.affine else None
                b = bn.bias.detach() if bn.affine else None
                st = x._stats
                if isinstance(st, tuple) and x._pending is None and hasattr(get_backend(), "bn_finalize_parts") \
                        and sum(p.size(2) for p in st) == feats.size(1):
                    # a concatenation of convolution outputs (ME.cat): finalize every part's partials into its slice
                    mean, invstd, scale, shift = get_backend().bn_finalize_parts(st, feats.size(0), bn.eps, mom, g, b,
                                                                                 rm, rv)
                elif torch.is_tensor(st) and st.numel() > 0 and x._pending is None:
                    # the convolution that produced these rows already summed them in its epilogue
                    mean, invstd, scale, shift = get_backend().bn_finalize(st, feats.size(0), bn.eps, mom, g, b,
                                                                           rm, rv)
                else:
                    mean, invstd, scale, shift = get_backend().bn_stats(feats.detach(), bn.eps, mom, g, b, rm, rv)
                if rm is not None:
                    self._pending_batches += 1
        else:
            with torch.no_grad():
                invstd = torch.rsqrt(bn.running_var + bn.eps)
                mean = bn.running_mean
                scale = bn.weight * invstd if bn.affine else invstd
                shift = (bn.bias if bn.affine else 0) - mean * scale
        pending = dict(gamma=bn.weight if bn.affine else torch.ones_like(scale),
                       beta=bn.bias if bn.affine else torch.zeros_like(scale), mean=mean.contiguous(),
                       invstd=invstd.contiguous(), scale=scale.contiguous(), shift=shift.contiguous(), relu=False,
                       training=use_batch)
        return x._like(feats, pending=pending)


class MinkowskiReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()

    def forward(self, x: SparseTensor):
        if x._pending is not None and x._pending.get("gamma") is not None and not x._pending["relu"]:
            p = dict(x._pending)
            p["relu"] = True
            return x._like(x._F, pending=p)
        return x._like(torch.relu(x._raw()))


def _pool_onto(x, key, table, mode):
    """pooling (mode 0 max, 1 average, 2 sum) of x over `table` = (nbr_fwd, nbr_inv, vin, vout, K) onto the set `key` names"""
    nbr_fwd, nbr_inv, vin, vout, K = table
    rows = x._raw()
    y = rows[:0] if vout == 0 else Fn.sparse_pool(rows, nbr_fwd, nbr_inv, vin, vout, K, mode)
    return SparseTensor(y, coordinate_manager=key.coordinate_manager, tensor_stride=key.tensor_stride)


class _PoolBase(nn.Module):
    """pooling over the kernel map of (kernel_size, stride, dilation): same geometries as the convolutions (stride 1 with an
    odd kernel: output coords = input coords; stride 2: the stride-2 coordinate set).  A pending BatchNorm / ReLU in front
    is materialised first."""
    MODE = None

    def __init__(self, kernel_size, stride=1, dilation=1, dimension=3, kernel_generator=None):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError(f"dimension={dimension}: only 3-D sparse tensors are supported")
        kernel_size, stride, dilation, self.region, _, self.kernel_volume = _layer_geometry(
            type(self).__name__, kernel_size, stride, dilation, kernel_generator)
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation

    def forward(self, x: SparseTensor, coordinates=None):
        """coordinates: the set to write onto (an integer tensor [M, 4], a CoordinateMapKey or a SparseTensor at tensor stride
        ts * stride, tensor.target_key); a row no input reaches is zero"""
        cm, ts = x.coordinate_manager, x.tensor_stride
        if coordinates is not None:
            key = target_key(coordinates, ts * self.stride, x.device)
            if key.coordinate_manager is not cm:
                table = cm.target_map(ts, key, self.kernel_size, self.stride, self.dilation, region=self.region)
                return _pool_onto(x, key, table, self.MODE)
        nbr_fwd, _, vin, vout, K, out_ts, _ = cm.kernel_map_tables(ts, self.kernel_size, self.stride, self.dilation, region=self.region)
        nbr_inv = cm.kernel_map_inverse(ts, self.kernel_size, self.stride, self.dilation, region=self.region)
        y = Fn.sparse_pool(x._raw(), nbr_fwd, nbr_inv, vin, vout, K, self.MODE)
        return x._like(y, tensor_stride=out_ts)

    def extra_repr(self):
        return f"kernel_size={self.kernel_size}, stride={self.stride}, dilation={self.dilation}" + _region_name(self.region)


class MinkowskiMaxPooling(_PoolBase):
    """max over the inputs present under the kernel (lowest offset index wins a tie)"""
    MODE = 0


class MinkowskiAvgPooling(_PoolBase):
    """mean over the inputs PRESENT under the kernel -- not over the kernel volume (how MinkowskiEngine's average pooling is
    recalled to behave; see the module docstring)"""
    MODE = 1


class MinkowskiSumPooling(_PoolBase):
    MODE = 2


class MinkowskiPoolingTranspose(nn.Module):
    """parameter-free upsampling: out[o] = sum_k in[nbr_up[k][o]] over the transposed table of the pooling of the same
    (kernel_size, stride, dilation) -- a SUM, not an average; with kernel 2 stride 2 every fine voxel copies its parent.
    Stride 2 maps from tensor stride ts onto the CACHED finer set at ts / 2 (the refusals of MinkowskiConvolutionTranspose: an
    uncached target raises NotImplementedError), stride 1 (odd kernels) stays on the set.  Sum pooling (csrc/pool.hip) over
    the transposed table forward, through the forward table backward.  Strides other than 1 and 2 are not supported."""

    def __init__(self, kernel_size, stride, dilation=1, dimension=3, expand_coordinates=False, kernel_generator=None):
        super().__init__()
        if dimension != 3:
            raise NotImplementedError(f"dimension={dimension}: only 3-D sparse tensors are supported")
        kernel_size, stride, dilation, self.region, self.expand_coordinates, self.kernel_volume = _layer_geometry(
            type(self).__name__, kernel_size, stride, dilation, kernel_generator, expand_coordinates)
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation

    def forward(self, x: SparseTensor, coordinates=None):
        """coordinates: the set to write onto (an integer tensor [M, 4], a CoordinateMapKey or a SparseTensor at tensor stride
        ts // stride, tensor.target_key): out[o] = sum_k x[o - off_k], off = kernel_offsets(kernel_size, dilation, ts //
        stride).  expand_coordinates=True: the same sum onto every coordinate the kernel reaches (CoordinateManager.generate:
        the set and the tables of the generative transposed convolution of this geometry)."""
        cm, ts = x.coordinate_manager, x.tensor_stride
        geom = (self.kernel_size, self.stride, self.dilation)
        if coordinates is not None or self.expand_coordinates:
            if coordinates is not None and self.expand_coordinates:
                raise ValueError("MinkowskiPoolingTranspose: expand_coordinates=True derives the output set, coordinates= names "
                                 "it: not both")
            if coordinates is None:
                out_cm, nbr_fwd, nbr_bwd, vin, vout, K, out_ts = cm.generate(ts, *geom, region=self.region)
                return _pool_onto(x, CoordinateMapKey(out_cm, out_ts), (nbr_fwd, nbr_bwd, vin, vout, K), 2)
            key = target_key(coordinates, _transposed_stride(self, ts), x.device)
            if key.coordinate_manager is not cm:
                return _pool_onto(x, key, cm.target_map(ts, key, *geom, transposed=True, region=self.region), 2)
            # (a set of this manager: its own at stride 1, the cached finer one at stride 2 -- the ordinary paths below)
        if self.stride == 1:
            # the transpose of a submanifold table is its mirror image, and a sum does not care about the offset order
            nbr, _, vin, vout, K, _, _ = cm.kernel_map_tables(ts, *geom, region=self.region)
            inv = cm.kernel_map_inverse(ts, *geom, region=self.region)
            if self.region is not None:
                nbr, inv = inv, nbr        # out[o] = sum_k in[o - off_k]: the inverse table forward (a region has no mirror rule)
            y = Fn.sparse_pool(x._raw(), nbr, inv, vin, vout, K, 2)
            return x._like(y)
        if ts % 2 != 0 or (ts // 2) not in cm.coords:
            raise NotImplementedError(f"MinkowskiPoolingTranspose(kernel_size={self.kernel_size}, stride={self.stride}) on "
                                      f"tensor stride {ts}: only onto a cached finer coordinate set; generating new "
                                      "coordinates is not supported")
        fine = ts // 2
        down, _, v_fine, v_coarse, K, _, _ = cm.kernel_map_tables(fine, *geom, region=self.region)    # the strided map fine -> ts
        up = cm.kernel_map_inverse(fine, *geom, region=self.region)           # [K, v_fine]: the coarse row a fine row feeds
        y = Fn.sparse_pool(x._raw(), up, down, v_coarse, v_fine, K, 2)
        return x._like(y, tensor_stride=fine)

    def extra_repr(self):
        return (f"kernel_size={self.kernel_size}, stride={self.stride}, dilation={self.dilation}" + _region_name(self.region)
                + (", expand_coordinates=True" if self.expand_coordinates else ""))


class MinkowskiInterpolation(nn.Module):
    """forward(x, tfield_coordinates) -> the trilinear interpolation of x's rows at the float coordinates [N, 4] (batch index
    first, voxel units): a tensor [N, C]; with return_kernel_map the table rows int32 [8, N] (corner j = bx + 2 by + 4 bz; the
    row of x.features / x.coordinates at the corner or -1) and with return_weights the weights float32 [8, N] follow.  Absent
    voxels count as zeros, nothing is renormalised.  Gradients flow to x's features only: like MinkowskiEngine, the query
    coordinates get none."""

    def __init__(self, return_kernel_map=False, return_weights=False):
        super().__init__()
        self.return_kernel_map, self.return_weights = return_kernel_map, return_weights

    def forward(self, x: SparseTensor, tfield_coordinates):
        cm, ts = x.coordinate_manager, x.tensor_stride
        rows, weights, group = cm.interpolation_map(ts, tfield_coordinates)
        out = [Fn.interpolate(x._raw(), rows, weights, group)]
        if self.return_kernel_map:
            out.append(cm.visible_rows(ts, rows))
        if self.return_weights:
            out.append(weights)
        return out[0] if len(out) == 1 else tuple(out)


class MinkowskiKNNPooling(nn.Module):
    """forward(x, queries=None, nmap=None): max | avg | sum of x's rows over the k nearest rows of every query's sample
    (ME.neighbor_pool over ME.knn_map(x, k, queries)) -- the "down" block of an FPS + kNN network.  queries as knn_query takes
    them; the result lives on the target of the map: x's own set, y's set, or a plain [B, M, C] tensor for picks.  nmap: a
    NeighborMap made for the same x and queries, shared by every layer over one graph (its k wins).  No parameters.  An engine
    extra."""

    def __init__(self, k, mode="max"):
        super().__init__()
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"{type(self).__name__}: k must be a Python int >= 1, got {k!r}")
        if mode not in ("max", "avg", "sum"):
            raise ValueError(f"{type(self).__name__}: mode must be 'max', 'avg' or 'sum', got {mode!r}")
        self.k, self.mode = k, mode

    def forward(self, x, queries=None, nmap=None):
        if nmap is None:
            nmap = knn_map(x, self.k, queries)
        return Fn.neighbor_pool(x, nmap, self.mode)

    def extra_repr(self):
        return f"k={self.k}, mode={self.mode!r}"


class MinkowskiKNNInterpolation(nn.Module):
    """forward(x, y, nmap=None): x's features carried onto y's coordinate set or points by inverse-distance weights over the k
    nearest rows of x in every row's sample (ME.knn_interpolate over ME.knn_map(x, k, y)) -- the "up" block of an FPS + kNN
    network.  nmap must be knn_map(x, k, y) when given.  No parameters.  An engine extra."""

    def __init__(self, k=3, eps=1e-8):
        super().__init__()
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"{type(self).__name__}: k must be a Python int >= 1, got {k!r}")
        self.k, self.eps = k, float(eps)

    def forward(self, x, y, nmap=None):
        if nmap is None:
            nmap = knn_map(x, self.k, y)
        return Fn.knn_interpolate(x, nmap, self.eps)

    def extra_repr(self):
        return f"k={self.k}, eps={self.eps}"


class MinkowskiNeighborAttention(nn.Module):
    """The self-attention block over the kNN graph of a SparseTensor or TensorField (an engine extra): forward(x, nmap=None) =
    proj(neighbor_attention(q, k, v, nmap, num_heads, bias)) with (q, k, v) = the three C-wide column blocks of qkv(x) and nmap
    = knn_map(x, k) unless one is given (its k wins).  `qkv` is nn.Linear(C, 3C) (bias when qkv_bias), `proj` nn.Linear(C, C);
    with pos_bias, `pos` = Sequential(Linear(3, pos_hidden), ReLU, Linear(pos_hidden, num_heads)) turns
    nmap.relative_positions() into the bias [N, k, num_heads]; its last layer starts at zero, so the block starts as plain
    attention.  scale = (C / num_heads) ** -0.5.

    Not a _ConvBase: prepare_conv_weights lays out (K, cin, cout) weight images, and this block has none."""

    def __init__(self, in_channels, num_heads, k=16, qkv_bias=True, pos_bias=True, pos_hidden=16):
        super().__init__()
        name = type(self).__name__
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"{name}: k must be a Python int >= 1, got {k!r}")
        if isinstance(num_heads, bool) or not isinstance(num_heads, int) or num_heads < 1 or in_channels % num_heads != 0:
            raise ValueError(f"{name}: {in_channels} channels do not divide into num_heads={num_heads}")
        self.in_channels = self.out_channels = in_channels
        self.num_heads, self.k = num_heads, k
        self.qkv = nn.Linear(in_channels, 3 * in_channels, bias=qkv_bias)
        self.proj = nn.Linear(in_channels, in_channels)
        self.pos = None
        if pos_bias:
            self.pos = nn.Sequential(nn.Linear(3, pos_hidden), nn.ReLU(), nn.Linear(pos_hidden, num_heads))
            with torch.no_grad():
                self.pos[2].weight.zero_()
                self.pos[2].bias.zero_()

    def forward(self, x, nmap=None):
        if nmap is None:
            nmap = knn_map(x, self.k)
        C = self.in_channels
        rows = x._raw() if isinstance(x, SparseTensor) else x._F
        like = x._like
        q, k, v = (like(t.contiguous()) for t in self.qkv(rows).split(C, dim=1))
        bias = None if self.pos is None else self.pos(nmap.relative_positions())
        y = Fn.neighbor_attention(q, k, v, nmap, self.num_heads, bias)
        return like(self.proj(y._raw() if isinstance(y, SparseTensor) else y._F))

    def extra_repr(self):
        return f"in={self.in_channels}, num_heads={self.num_heads}, k={self.k}, pos_bias={self.pos is not None}"


class _GlobalPoolBase(nn.Module):
    """one output row per batch index present, in ascending batch order.  The result is a plain tensor wrapper on its own
    coordinate set (batch index, 0, 0, 0); rows are grouped by batch through a cached stable sort, not assumed contiguous."""
    MODE = None

    def forward(self, x: SparseTensor):
        from ..common_ops.functions.common_ops import roipool
        from ..common_ops.functions.softgroup_ops import global_avg_pool
        cm, ts = x.coordinate_manager, x.tensor_stride
        group = cm.batch_group(ts)
        order, offsets = group.order, group.seg_start
        rows = Fn.PermuteRowsFn.apply(x._raw(), order, group.inverse)        # a permutation: the backward is the gather dy[inv]
        if self.MODE == 0:
            y = roipool(rows, offsets)
        else:
            y = global_avg_pool(rows, offsets)
            if self.MODE == 2:
                y = y * group.counts
        b = cm.coords[ts][order[offsets[:-1].long()], 0]
        coords = torch.zeros((b.numel(), 4), dtype=torch.int32, device=b.device)
        coords[:, 0] = b
        return SparseTensor(y, coordinates=coords)


class MinkowskiGlobalMaxPooling(_GlobalPoolBase):
    MODE = 0


class MinkowskiGlobalAvgPooling(_GlobalPoolBase):
    MODE = 1


class MinkowskiGlobalSumPooling(_GlobalPoolBase):
    MODE = 2


class MinkowskiLinear(nn.Module):
    """nn.Linear on the rows of .F (`linear.weight`, `linear.bias` as in ME)"""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, x: SparseTensor):
        feats = x._raw()
        if feats.is_cuda and feats.dtype == torch.float32:
            y = Fn.dense_linear(feats, self.linear.weight, self.linear.bias)
        else:
            y = self.linear(feats)
        return x._like(y)


class MinkowskiDropout(nn.Module):
    def __init__(self, p=0.5, inplace=False):
        super().__init__()
        self.dropout = nn.Dropout(p)

    def forward(self, x: SparseTensor):
        return x._like(self.dropout(x._raw()))


class MinkowskiSigmoid(nn.Module):
    """elementwise on the rows (the gate of a squeeze-and-excitation block)"""

    def forward(self, x: SparseTensor):
        return x._like(torch.sigmoid(x._raw()))


class _NonlinearityBase(nn.Module):
    """MODULE(*args, **kwargs) of torch.nn kept as `self.module` (MinkowskiEngine's layout, so a parameter of the operator keeps
    its key: MinkowskiPReLU's is `module.weight`) and applied to the rows; a pending BatchNorm / ReLU in front is materialised
    first, the result lives on the input's coordinate set.  Plain torch operators: rows are independent, no kernel of the
    engine's own is involved.  A TensorField passes through the same way."""
    MODULE = None

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.module = self.MODULE(*args, **kwargs)

    def forward(self, x):
        return x._like(self.module(x._raw() if isinstance(x, SparseTensor) else x.F))

    def __repr__(self):
        return type(self).__name__ + "(" + self.module.extra_repr() + ")"


class MinkowskiELU(_NonlinearityBase):
    MODULE = nn.ELU


class MinkowskiLeakyReLU(_NonlinearityBase):
    MODULE = nn.LeakyReLU


class MinkowskiPReLU(_NonlinearityBase):
    MODULE = nn.PReLU


class MinkowskiSELU(_NonlinearityBase):
    MODULE = nn.SELU


class MinkowskiCELU(_NonlinearityBase):
    MODULE = nn.CELU


class MinkowskiGELU(_NonlinearityBase):
    MODULE = nn.GELU


class MinkowskiSiLU(_NonlinearityBase):
    MODULE = nn.SiLU


class MinkowskiTanh(_NonlinearityBase):
    MODULE = nn.Tanh


class MinkowskiSoftplus(_NonlinearityBase):
    MODULE = nn.Softplus


class MinkowskiHardswish(_NonlinearityBase):
    MODULE = nn.Hardswish


class MinkowskiHardtanh(_NonlinearityBase):
    MODULE = nn.Hardtanh


class MinkowskiReLU6(_NonlinearityBase):
    MODULE = nn.ReLU6


class MinkowskiSoftmax(_NonlinearityBase):
    MODULE = nn.Softmax


class MinkowskiLogSoftmax(_NonlinearityBase):
    MODULE = nn.LogSoftmax


class MinkowskiInstanceNorm(nn.Module):
    """normalisation per sample: every channel of the rows of ONE batch index is shifted to mean 0 and scaled to variance 1
    (biased variance, as torch's instance_norm), then times `weight` plus `bias` -- both (1, num_features), ones and zeros,
    state-dict keys `weight` and `bias`.  No running statistics: train() and eval() do the same.  The result lives on the
    input's coordinate set and tensor stride; a pending BatchNorm / ReLU in front is materialised first.

    `eps` as a keyword is an engine extra.  The default 1e-8 is how MinkowskiEngine's layer is recalled to behave (it adds
    1e-8 to the variance); MinkowskiEngine is not installed where this package is developed (see the module docstring), so
    this is this engine's definition, checked against torch.nn.functional.instance_norm in float64.

    One HIP pass for the statistics (shifted sums per slice, merged by Chan's formula: csrc/inorm.hip), one for the rows; the
    backward likewise.  Rows are grouped through CoordinateManager.batch_rows / batch_segments and read where they are held;
    every sum runs in a fixed order: the same bytes on every run."""

    def __init__(self, num_features, eps=1e-8):
        super().__init__()
        self.num_features = int(num_features)
        self.eps = float(eps)
        self.weight = nn.Parameter(torch.ones((1, self.num_features), dtype=torch.float32))
        self.bias = nn.Parameter(torch.zeros((1, self.num_features), dtype=torch.float32))

    def forward(self, x: SparseTensor):
        c = x._F.size(1)
        if c != self.num_features:
            raise ValueError(f"{type(self).__name__}: the input has {c} channels, the layer num_features={self.num_features}")
        cm, ts = x.coordinate_manager, x.tensor_stride
        if not hasattr(get_backend(), "inorm_forward"):
            raise NotImplementedError(f"{type(self).__name__} needs the HIP backend (ms3d_inorm_forward)")
        y = Fn.instance_norm(x._raw(), self.weight, self.bias, cm.batch_group(ts), self.eps)
        return x._like(y)

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}"


class MinkowskiStableInstanceNorm(MinkowskiInstanceNorm):
    """MinkowskiInstanceNorm with eps = 1e-6 by default: how MinkowskiEngine's second instance normalisation layer (built from
    global pooling and broadcast layers there) is recalled to behave.  Here both classes run the same kernels -- the statistics
    never form E[x^2] - E[x]^2 -- and differ in the default `eps` alone."""

    def __init__(self, num_features, eps=1e-6):
        super().__init__(num_features, eps)


class MinkowskiUnion(nn.Module):
    """forward(*inputs): the sum of up to 16 tensors of one tensor stride and channel count on the UNION of their coordinate
    sets -- the first input's rows in their order, then the rows of the second that the first lacks, and so on; an input that
    lacks a coordinate adds nothing there.  The result lives on a coordinate manager rooted at that tensor stride, shared by
    every union / + / - / * of the same operands.  Inputs on one set are added row by row; one input comes back as an equal
    tensor."""

    def forward(self, *inputs):
        if not inputs:
            raise ValueError("MinkowskiUnion needs at least one input")
        first = inputs[0]
        for t in inputs[1:]:
            if t.tensor_stride != first.tensor_stride:
                raise ValueError(f"MinkowskiUnion: tensor strides {first.tensor_stride} and {t.tensor_stride} differ")
            if t._F.size(1) != first._F.size(1):
                raise ValueError(f"MinkowskiUnion: channel counts {first._F.size(1)} and {t._F.size(1)} differ")
        if len(inputs) > 16:
            raise NotImplementedError(f"MinkowskiUnion of {len(inputs)} inputs: at most 16")
        if all(t.coordinate_manager is first.coordinate_manager for t in inputs[1:]):
            y = first._raw()
            for t in inputs[1:]:
                y = y + t._raw()
            return first._like(y)
        return union_op(0, *inputs)


class _BroadcastBase(nn.Module):
    """forward(x, x_glob): x_glob holds one row per batch index (what the global poolings return; only the batch column of
    its coordinates is read), every voxel of x meets the row of its batch index.  The result lives on x's coordinate manager
    and tensor stride.  A batch index of x without a row in x_glob sees the zero vector; a batch index that occurs twice in
    x_glob raises ValueError.  A pending BatchNorm / ReLU is materialised first."""
    MODE = None

    def forward(self, x: SparseTensor, x_glob: SparseTensor):
        cx, cg = x._F.size(1), x_glob._F.size(1)
        if self.MODE in (0, 1) and cx != cg:
            raise ValueError(f"{type(self).__name__}: channel counts {cx} and {cg} differ")
        grow, red = x.coordinate_manager.broadcast_map(x.tensor_stride, x_glob.coordinate_manager, x_glob.tensor_stride)
        if not hasattr(get_backend(), "broadcast"):
            raise NotImplementedError(f"{type(self).__name__} needs the HIP backend (ms3d_broadcast_forward)")
        y = Fn.broadcast(self.MODE, None if self.MODE == 3 else x._raw(), x_glob._raw(), grow, red)
        return x._like(y)


class MinkowskiBroadcastAddition(_BroadcastBase):
    MODE = 0


class MinkowskiBroadcastMultiplication(_BroadcastBase):
    MODE = 1


class MinkowskiBroadcastConcatenation(_BroadcastBase):
    """[V, C + Cg]: x's channels in front"""
    MODE = 2


class MinkowskiBroadcast(_BroadcastBase):
    """[V, Cg]: the global row of every voxel's batch index, on x's coordinates"""
    MODE = 3
