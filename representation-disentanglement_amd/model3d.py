"""3-D networks of the reference on the HIP kernels: `BasicBlock`, `VAEBranch`, `UNet3D`,
`NVNet3D` (reference src/model.py:1856-2060) -- same class names, constructor arguments, submodule names (so
`state_dict()` keys and the seeded initialisation are the reference's), forward signatures and return values.

Activations are NDHWC (`torch.channels_last_3d`) fp32.  Every Conv3d (3x3x3 stride 1/2 and 1x1x1), every
GroupNorm+ReLU pair and every nearest x2 upsampling (+ skip) runs in csrc/mrdis_conv3d.hip / mrdis_elem3d.hip; the
VAE bottleneck (global average of an 8^3 map, three Linear layers on (B, 32) rows, reparameterisation) stays in torch.
There is no CPU fallback: without libmrdis_hip.so the first forward raises `MrdisLibraryError`.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import hip, ops, patch3d, tilepred

_GN_TAP = __import__('os').environ.get('MRDIS_GN_TAP', '1') != '0'      # BasicBlock: residual gradient summed inside the GroupNorm backward (0: autograd's add)


# --------------------------------------------------------------------------- autograd pairing
class _Conv3d(Function):
    """nn.Conv3d(k=3, padding=1, stride s) (+ fused residual addition)."""

    @staticmethod
    def forward(ctx, x, w_tck, w_tkc, bias, stride, residual):
        y = hip.conv3d_fwd(x, w_tck, bias, 3, stride, 1, residual)
        ctx.geom = (stride, tuple(x.shape), bias is not None, residual is not None)
        ctx.save_for_backward(x, w_tkc)
        return y

    @staticmethod
    def backward(ctx, dy):
        stride, in_shape, has_bias, has_res = ctx.geom
        x, w_tkc = ctx.saved_tensors
        dx = hip.conv3d_bwd_data(dy, w_tkc, in_shape, 3, stride, 1) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[3]):
            dw, db = hip.conv3d_bwd_weight(x, dy, 3, stride, 1, has_bias)
        return dx, dw, None, db, None, (dy if has_res else None)


class _GroupNormReLU(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, relu):
        y, mean, rstd = hip.groupnorm_relu_fwd(x, gamma, beta, G, eps, relu)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.cfg = (G, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        G, relu = ctx.cfg
        dx, dg, db = hip.groupnorm_relu_bwd(dy, x, gamma, beta, mean, rstd, G, relu)
        return dx, dg, db, None, None, None


class _GroupNormReLUTap(Function):
    """(relu(gn(x)), x): the second output is x itself for a consumer beside the normalised branch (BasicBlock's residual addition, model.py:1873).  Both
    gradients of x then arrive in ONE backward call and are summed inside the GroupNorm backward pass (mrdis_groupnorm_relu_bwd_add) instead of by an
    extra three-tensor add of autograd (537 MB per tensor at 4 x 16 x 128^3)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, relu):
        y, mean, rstd = hip.groupnorm_relu_fwd(x, gamma, beta, G, eps, relu)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.cfg = (G, relu)
        return y, x.detach()

    @staticmethod
    def backward(ctx, dy, dx_tap):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        G, relu = ctx.cfg
        if dy is None:                      # (only the tap was used)
            return dx_tap, None, None, None, None, None
        dx, dg, db = hip.groupnorm_relu_bwd(dy, x, gamma, beta, mean, rstd, G, relu, add=dx_tap)
        return dx, dg, db, None, None, None


class _Upsample2xAdd(Function):
    @staticmethod
    def forward(ctx, x, skip):
        ctx.has_skip = skip is not None
        return hip.upsample2x_add_fwd(x, skip)

    @staticmethod
    def backward(ctx, dy):
        dx = hip.upsample2x_bwd(dy) if ctx.needs_input_grad[0] else None
        return dx, (dy if ctx.has_skip else None)


def groupnorm_relu(x, gn, relu=True):
    return _GroupNormReLU.apply(x, gn.weight, gn.bias, gn.num_groups, gn.eps, relu)


def groupnorm_relu_tap(x, gn, relu=True):
    """(relu(gn(x)), x for the residual connection): see _GroupNormReLUTap"""
    return _GroupNormReLUTap.apply(x, gn.weight, gn.bias, gn.num_groups, gn.eps, relu)


def upsample2x(x, skip=None):
    """nn.Upsample(scale_factor=2) (nearest) [+ skip]."""
    return _Upsample2xAdd.apply(x, skip)


class HipConv3d(nn.Conv3d):
    """nn.Conv3d whose forward/backward run in the HIP kernels; parameters, init and state_dict are nn.Conv3d's.
    Covers what the reference's 3-D nets use: 3x3x3 / padding 1 / stride 1 or 2, and 1x1x1."""

    def forward(self, x, residual=None):
        k = self.kernel_size
        if self.dilation != (1, 1, 1) or self.groups != 1 or self.padding_mode != 'zeros' or k[0] != k[1] or k[1] != k[2]:
            raise NotImplementedError
        one = torch.ones(1, dtype=torch.float32, device=x.device)
        Co, Ci = self.weight.shape[:2]
        if k[0] == 1:
            if self.stride != (1, 1, 1) or self.padding != (0, 0, 0) or residual is not None:
                raise NotImplementedError
            # 1x1x1: the 2-D kernels on the (N*D, H, W) view of the NDHWC tensor (no copy)
            x, _ = hip.ndhwc(x)
            N, _, D, H, W = x.shape
            x2 = x.permute(0, 2, 1, 3, 4).reshape(N * D, Ci, H, W)
            w_tck, w_tkc = ops.cached_mix((id(self), 0, 0), lambda: ops.mix_experts(self.weight.reshape(1, Co, Ci, 1, 1), one))
            y2 = ops.conv2d(x2, w_tck, w_tkc, self.bias, 1, 1, 1, 0, False)
            return y2.reshape(N, D, Co, H, W).permute(0, 2, 1, 3, 4)
        if k[0] != 3 or self.padding != (1, 1, 1) or self.stride[0] not in (1, 2) or len(set(self.stride)) != 1:
            raise NotImplementedError
        w_tck, w_tkc = ops.cached_mix((id(self), 0, 0), lambda: ops.mix_experts(self.weight.reshape(1, Co, Ci, 27, 1), one))
        return _Conv3d.apply(x, w_tck, w_tkc, self.bias, self.stride[0], residual)


# --------------------------------------------------------------------------- modules (model.py:1856-2060)
class BasicBlock(nn.Module):
    """model.py:1856-1876.  QUIRK kept: gn2 is built with `in_channels` (every call site has in == out)."""

    def __init__(self, in_channels, out_channels, n_groups=8):
        super().__init__()
        self.gn1 = nn.GroupNorm(n_groups, in_channels)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = HipConv3d(in_channels, out_channels, kernel_size=(3, 3, 3), padding=(1, 1, 1))
        self.gn2 = nn.GroupNorm(n_groups, in_channels)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = HipConv3d(out_channels, out_channels, kernel_size=(3, 3, 3), padding=(1, 1, 1))

    def forward(self, x):
        if _GN_TAP and x.requires_grad and torch.is_grad_enabled():
            g, x = groupnorm_relu_tap(x, self.gn1)                         # the residual path's gradient joins the branch's inside the GroupNorm backward
        else:
            g = groupnorm_relu(x, self.gn1)
        h = self.conv1(g)
        return self.conv2(groupnorm_relu(h, self.gn2), residual=x)        # `x + residul` in the conv epilogue


class _ConvUp(nn.Sequential):
    """nn.Sequential(Conv3d, Upsample[, BasicBlock]) with the reference's child indices (state_dict keys '0', '2')."""

    def forward(self, x):
        x = upsample2x(self[0](x))
        return self[2](x) if len(self) > 2 else x


class VAEBranch(nn.Module):
    """model.py:1879-1949."""

    def __init__(self, input_shape, init_channels, out_channels, squeeze_channels=None):
        super().__init__()
        self.input_shape = input_shape
        self.squeeze_channels = squeeze_channels if squeeze_channels else init_channels * 4
        c = init_channels
        self.hidden_conv = nn.Sequential(nn.GroupNorm(8, c * 8), nn.ReLU(inplace=True),
                                         HipConv3d(c * 8, self.squeeze_channels, (3, 3, 3), padding=(1, 1, 1)),
                                         nn.AdaptiveAvgPool3d(1))
        self.mu_fc = nn.Linear(self.squeeze_channels // 2, self.squeeze_channels // 2)
        self.logvar_fc = nn.Linear(self.squeeze_channels // 2, self.squeeze_channels // 2)
        recon_shape = int(np.prod(self.input_shape)) // (16 ** 3)
        self.reconstraction = nn.Sequential(nn.Linear(self.squeeze_channels // 2, c * 8 * recon_shape), nn.ReLU(inplace=True))
        self.vconv4 = _ConvUp(HipConv3d(c * 8, c * 8, (1, 1, 1)), nn.Upsample(scale_factor=2))
        self.vconv3 = _ConvUp(HipConv3d(c * 8, c * 4, (3, 3, 3), padding=(1, 1, 1)), nn.Upsample(scale_factor=2),
                              BasicBlock(c * 4, c * 4))
        self.vconv2 = _ConvUp(HipConv3d(c * 4, c * 2, (3, 3, 3), padding=(1, 1, 1)), nn.Upsample(scale_factor=2),
                              BasicBlock(c * 2, c * 2))
        self.vconv1 = _ConvUp(HipConv3d(c * 2, c, (3, 3, 3), padding=(1, 1, 1)), nn.Upsample(scale_factor=2),
                              BasicBlock(c, c))
        self.vconv0 = HipConv3d(c, out_channels, (1, 1, 1))

    def reparameterize(self, mu, logvar):
        std = torch.exp(0.5 * logvar)
        eps = ops.to_device(torch.randn(std.shape, dtype=std.dtype), std.device)   # CPU generator, as the reference on its CPU path
        return eps.mul(std).add_(mu)

    def forward(self, x):
        h = self.hidden_conv[2](groupnorm_relu(x, self.hidden_conv[0]))
        batch_size = h.size(0)
        h = h.mean(dim=(2, 3, 4)).view((batch_size, -1))                  # AdaptiveAvgPool3d(1)
        half = self.squeeze_channels // 2
        mu = self.mu_fc(h[:, :half])
        logvar = self.logvar_fc(h[:, half:])
        z = self.reparameterize(mu, logvar)
        re_x = self.reconstraction(z)
        re_x = re_x.view([batch_size, -1, self.input_shape[0] // 16, self.input_shape[1] // 16, self.input_shape[2] // 16])
        x = self.vconv4(re_x)
        x = self.vconv3(x)
        x = self.vconv2(x)
        x = self.vconv1(x)
        return self.vconv0(x), mu, logvar


class UNet3D(nn.Module):
    """model.py:1952-2048."""

    def __init__(self, input_shape, in_channels=4, out_channels=3, init_channels=32, p=0.2):
        super().__init__()
        self.input_shape = input_shape
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.init_channels = init_channels
        self.make_encoder()
        self.make_decoder()
        self.dropout = nn.Dropout(p=p)

    def make_encoder(self):
        c = self.init_channels
        self.conv1a = HipConv3d(self.in_channels, c, (3, 3, 3), padding=(1, 1, 1))
        self.conv1b = BasicBlock(c, c)
        self.ds1 = HipConv3d(c, c * 2, (3, 3, 3), stride=(2, 2, 2), padding=(1, 1, 1))
        self.conv2a = BasicBlock(c * 2, c * 2)
        self.conv2b = BasicBlock(c * 2, c * 2)
        self.ds2 = HipConv3d(c * 2, c * 4, (3, 3, 3), stride=(2, 2, 2), padding=(1, 1, 1))
        self.conv3a = BasicBlock(c * 4, c * 4)
        self.conv3b = BasicBlock(c * 4, c * 4)
        self.ds3 = HipConv3d(c * 4, c * 8, (3, 3, 3), stride=(2, 2, 2), padding=(1, 1, 1))
        self.conv4a = BasicBlock(c * 8, c * 8)
        self.conv4b = BasicBlock(c * 8, c * 8)
        self.conv4c = BasicBlock(c * 8, c * 8)
        self.conv4d = BasicBlock(c * 8, c * 8)

    def make_decoder(self):
        c = self.init_channels
        self.up4conva = HipConv3d(c * 8, c * 4, (1, 1, 1))
        self.up4 = nn.Upsample(scale_factor=2)
        self.up4convb = BasicBlock(c * 4, c * 4)
        self.up3conva = HipConv3d(c * 4, c * 2, (1, 1, 1))
        self.up3 = nn.Upsample(scale_factor=2)
        self.up3convb = BasicBlock(c * 2, c * 2)
        self.up2conva = HipConv3d(c * 2, c, (1, 1, 1))
        self.up2 = nn.Upsample(scale_factor=2)
        self.up2convb = BasicBlock(c, c)
        self.up1conv = HipConv3d(c, self.out_channels, (1, 1, 1))

    def forward(self, x):
        c1 = self.conv1b(self.conv1a(x))
        c2 = self.conv2b(self.conv2a(self.ds1(c1)))
        c3 = self.conv3b(self.conv3a(self.ds2(c2)))
        c4d = self.conv4d(self.conv4c(self.conv4b(self.conv4a(self.ds3(c3)))))
        c4d = self.dropout(c4d)
        u4 = self.up4convb(upsample2x(self.up4conva(c4d), c3))             # up + skip in one kernel
        u3 = self.up3convb(upsample2x(self.up3conva(u4), c2))
        u2 = self.up2convb(upsample2x(self.up2conva(u3), c1))
        return self.up1conv(u2), c4d


class NVNet3D(nn.Module):
    """model.py:2050-2060."""

    def __init__(self, input_shape, in_channels=4, out_channels=3, init_channels=16, p=0.2):
        super().__init__()
        self.unet = UNet3D(input_shape, in_channels, out_channels, init_channels, p)
        self.vae_branch = VAEBranch(input_shape, init_channels, out_channels=in_channels)

    def forward(self, x):
        uout, c4d = self.unet(x)
        vout, mu, logvar = self.vae_branch(c4d)
        return uout, vout, mu, logvar


def nvnet_loss(uout, vout, mu, logvar, x, target):
    """The reference ships no objective for NVNet3D; this is the one of the paper its docstring cites (Myronenko 2018:
    soft Dice of sigmoid(uout) + 0.1 * L2 of the VAE reconstruction + 0.1 * KL), used by bench3d.py and the parity tests
    to drive the backward pass.  `target` has one channel per output channel of the net: with out_channels = 3 that is the three region
    channels (label == 1, label == 2, label == 3) that `VolumeLoader3D(region_channels=3)` writes.  Like the objective itself this is the
    package's own convention, not the reference's: its 3-D dataset returns the label volume and nothing consumes it."""
    p = torch.sigmoid(uout)
    dice = 1 - 2 * (p * target).sum() / ((p * p).sum() + (target * target).sum() + 1e-6)
    l2 = ((vout - x) ** 2).mean()
    kl = (mu ** 2 + logvar.exp() - logvar - 1).sum() / x[0].numel()
    return dice + 0.1 * l2 + 0.1 * kl, {'dice': dice, 'l2': l2, 'kl': kl}


# --------------------------------------------------------------------------- fused objective and segmentation metrics (csrc/mrdis_loss3d.hip)
class _NVNetLossFn(Function):
    """(dice + 0.1 * l2, dice, l2) of `nvnet_loss` in one pass over uout, target, vout, x; the backward writes both gradients in one pass.
    Only the first output carries a gradient; the other two are the `parts` for the log."""

    @staticmethod
    def forward(ctx, uout, target, vout, x):
        sums, terms = hip.nvnet_loss_fwd(uout, target, vout, x, 0.1)
        ctx.save_for_backward(uout, target, vout, x, sums)
        dice, l2 = terms[0], terms[1]
        ctx.mark_non_differentiable(dice, l2)
        return terms[2], dice, l2

    @staticmethod
    def backward(ctx, g, _gd, _gl):
        uout, target, vout, x, sums = ctx.saved_tensors
        du, dv = hip.nvnet_loss_bwd(g, sums, uout, target, vout, x, 0.1, need_du=ctx.needs_input_grad[0],
                                    need_dv=vout is not None and ctx.needs_input_grad[2])
        return du, None, dv, None


def nvnet_loss_hip(uout, vout, mu, logvar, x, target):
    """`nvnet_loss` with the Dice and reconstruction terms in the fused HIP kernels (mrdis_nvnet_loss_fwd / _bwd): same tuple, same `parts`
    keys.  uout / target and vout / x must each share one dense memory layout (channels-last-3d as the nets and the loader write them): a
    mismatch raises `MrdisError`, nothing is copied.  The KL term on the (B, 16) rows stays in torch.  `vout=None` (then mu / logvar may be
    None too) is the Dice-only objective for `UNet3D`: l2 and kl are zeros."""
    obj, dice, l2 = _NVNetLossFn.apply(uout, target, vout, x if vout is not None else None)
    if vout is None or mu is None:
        kl = torch.zeros((), dtype=torch.float32, device=uout.device)
        return obj, {'dice': dice, 'l2': l2, 'kl': kl}
    kl = (mu ** 2 + logvar.exp() - logvar - 1).sum() / x[0].numel()
    return obj + 0.1 * kl, {'dice': dice, 'l2': l2, 'kl': kl}


def seg_metrics_from_counts(counts):
    """counts (B, C, 3) integers [intersection I, predicted P, labelled T] -> {'dice': (B,), 'iou': (B,)} float64: the reference's
    compute_segmentation_metrics_single (util.py:980-992), dice_c = (2 I + 1) / (T + P + 1), iou_c = (I + 1) / (T + P - I + 1), averaged over
    the region channels."""
    c = np.asarray(counts).astype(np.float64)
    i, p, t = c[..., 0], c[..., 1], c[..., 2]
    dice = (2.0 * i + 1) / (t + p + 1)
    iou = (i + 1) / (t + p - i + 1)
    return {'dice': torch.from_numpy(dice.mean(axis=1)), 'iou': torch.from_numpy(iou.mean(axis=1))}


def seg_metrics(pred_or_logits, target, logits=True):
    """Dice and IoU per sample of the reference's compute_segmentation_metrics (util.py:946-992): `target` holds the region channels
    (channel c = (label == c + 1), what `VolumeLoader3D(region_channels=3)` yields), a voxel is predicted where the probability is strictly
    above 0.5.  The integer counts come from ONE kernel launch (mrdis_seg_counts; `logits`: it applies the sigmoid), the ratios are
    formed in float64 on the host (one small D2H copy).  Inputs that are not channels-last-3d are copied into that layout first (hip.seg_counts).
    -> {'dice': (B,), 'iou': (B,)} float64 CPU tensors."""
    return seg_metrics_from_counts(hip.seg_counts(pred_or_logits, target, logits=logits).cpu().numpy())


# --------------------------------------------------------------------------- whole-volume sliding-window prediction (csrc/mrdis_segvol.hip)
def window_offsets(D, Dz, stride):
    """depth offsets of the windows [z0, z0 + Dz) that slide along D: 0, stride, 2 stride, ... below D - Dz, then D - Dz itself (no duplicate);
    [0] when D == Dz.  A stride above Dz leaves depths no window covers (they are predicted as label 0)."""
    D, Dz, stride = int(D), int(Dz), int(stride)
    if D < Dz or Dz < 1:
        raise ValueError(f'a window of {Dz} slices does not fit a depth of {D}')
    if stride < 1:
        raise ValueError(f'stride {stride}: at least 1')
    return list(range(0, D - Dz, stride)) + [D - Dz]


def window_cover(D, Dz, offsets, flips=1):
    """(D,) int32: how many accumulations touch each depth -- windows that hold it times `flips`"""
    cover = np.zeros(D, dtype=np.int32)
    for z0 in offsets:
        cover[z0:z0 + Dz] += flips
    return cover


def predict_volumes(model, loader, stride=None, flip=False, limit=None):
    """Label volumes over the FULL depth of every subject a VolumeLoader3D serves, as a generator over its batches:
        {'subj_id': list, 'labels': (B, H, W, D) uint8 on the device, 'counts': (B, 3, 3) int32 on the device, 'acc': (B, H, W, D, C) fp32,
         'target_ptrs': (B,) int64 on the device, the addresses of the subjects' full label volumes (0 = none; `surfdist.region_scores`)}
    The trained depth window (Dz = the loader's crop depth) slides along D at `window_offsets(D, Dz, stride)` (stride None: Dz // 2); the sigmoid
    probabilities of overlapping windows -- and, with `flip`, of the H-flipped input, un-flipped -- are averaged; a voxel's label is 0 if no
    region's mean probability is above 0.5, else 1 + the most probable region (lowest on a tie), region 3 written as 4 for BraTS: the store's
    own labels 0 / 1 / 2 / 4 in its own (H, W, D) geometry.  `counts` are the reference's Dice / IoU counts (`seg_metrics_from_counts`) of the
    mean probabilities against the subject's full label volume; `acc` holds the summed probabilities.  Overlap rule and label rule are this
    package's own convention, like `nvnet_loss`: the reference ships no 3-D inference.

    Eval mode, no_grad.  An `NVNet3D` runs its `unet` only: the VAE branch is training-time regularisation and is bound to the crop shape.
    Per batch: one `hip.seg_accum` launch per window (and per flip), then one `hip.seg_label_volume`; nothing syncs with the host.  The loader
    must serve the items as stored (aug and dropoff off), otherwise ValueError.  The batches are those of `loader.plain_plan`: dataset order
    even for a loader that shuffles, drawn ONCE and shared by all windows, and no random stream is touched.  `limit`: stop after that many
    batches.  `acc` stays alive as long as the caller holds the yielded dict (57 MB per BraTS subject): drop it if it is not wanted."""
    ds = loader.dataset
    if ds.aug or ds.dropoff:
        raise ValueError('predict_volumes reads the volumes as stored: the loader must have aug=False and dropoff=False')
    H, W, D = ds.store.shape
    _, Dz = ds.crop()
    offsets = window_offsets(D, Dz, Dz // 2 if stride is None else stride)
    flips = (False, True) if flip else (False,)
    net = model.unet if isinstance(model, NVNet3D) else model
    C = net.out_channels
    dev = ds.store.device
    cover = torch.from_numpy(window_cover(D, Dz, offsets, len(flips))).to(dev)
    relabel = ds.dataset_name == 'BraTS'
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            # ONE plan for all windows: every window and flip of a batch gathers the same subjects into the same rows
            for k, _, metas in loader.plain_plan(limit):
                subj_id = [m[0] for m in metas]
                acc = torch.zeros((len(metas), H, W, D, C), dtype=torch.float32, device=dev)
                ptrs = None
                for z0 in offsets:
                    for f in flips:
                        batch = loader.window(k, metas, z0, flip=f)
                        if batch['subj_id'] != subj_id:
                            raise RuntimeError(f'window {z0} of batch {k} serves {batch["subj_id"]}, not {subj_id}')
                        if ptrs is None:
                            ptrs = loader.target_ptrs(batch)
                        hip.seg_accum(net(batch['inputs'])[0], acc, z0, flip_h=f)
                        del batch
                labels, counts = hip.seg_label_volume(acc, cover, ptrs, relabel=relabel)
                yield {'subj_id': subj_id, 'labels': labels, 'counts': counts, 'acc': acc, 'target_ptrs': ptrs}
    finally:
        net.train(was_training)


# --------------------------------------------------------------------------- tile-wise prediction (csrc/mrdis_segvol.hip: mrdis_tile_accum, mrdis_tile_label_volume)
TILE_WEIGHTS = ('gaussian', 'uniform')
TILE_WEIGHT_FLOOR = 2.0 ** -20          # every weight entry is at least this: no product of three underflows
TILE_SIGMA = (0.05, 1.0)


def _triple(v, what, lo=1):
    """three integers >= lo as a tuple, else ValueError naming `what`"""
    try:
        ok = len(v) == 3 and all(not isinstance(x, bool) and int(x) == x and x >= lo for x in v)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what} {v!r}: three integers >= {lo}')
    return tuple(int(x) for x in v)


def tile_weights(T, kind='gaussian', sigma=0.125):
    """(T,) float32: the weight of one tile axis.  'uniform': ones.  'gaussian': exp(-0.5 ((x - (T - 1) / 2) / (sigma T))^2) evaluated in float64
    and rounded once to fp32, every entry at least 2^-20; sigma in 0.05 .. 1.  Symmetric: w[x] == w[T - 1 - x] to the bit."""
    T = int(T)
    if T < 1:
        raise ValueError(f'tile extent {T}: at least 1')
    if kind not in TILE_WEIGHTS:
        raise ValueError(f'weight {kind!r}: one of {TILE_WEIGHTS}')
    if kind == 'uniform':
        return np.ones(T, dtype=np.float32)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not TILE_SIGMA[0] <= sigma <= TILE_SIGMA[1]:
        raise ValueError(f'sigma {sigma!r}: a number in {TILE_SIGMA[0]} .. {TILE_SIGMA[1]} (the share of the tile extent)')
    x = (np.arange(T, dtype=np.float64) - (T - 1) / 2.0) / (float(sigma) * T)
    return np.maximum(np.exp(-0.5 * x * x), TILE_WEIGHT_FLOOR).astype(np.float32)


def tile_offsets(shape, tile, stride=None):
    """([h0 ...], [w0 ...], [d0 ...]): `window_offsets` per axis; the tiles are their Cartesian product, visited with h0 outermost and d0 innermost.
    `stride` None: max(1, T // 2) per axis.  A tile larger than the volume is refused (nothing is padded)."""
    shape, tile = _triple(shape, 'shape'), _triple(tile, 'tile')
    stride = tuple(max(1, t // 2) for t in tile) if stride is None else _triple(stride, 'stride')
    if any(t > n for t, n in zip(tile, shape)):
        raise ValueError(f'tile {tile} does not fit the volume {shape}: no padding past the border')
    return tuple(window_offsets(n, t, s) for n, t, s in zip(shape, tile, stride))


def tile_norm(n, T, offsets, w, scale=1):
    """(n,) float32: the summed weight of one axis, n[x] = scale * sum over the offsets o of w[x - o], summed in float64 from the fp32 weights and
    rounded once.  The summed weight of a voxel is the product of its three axis sums (the tiles are a Cartesian product); `scale` carries
    the number of views into the depth axis."""
    w = np.asarray(w)
    if w.dtype != np.float32 or w.shape != (int(T),):
        raise ValueError(f'weights of dtype {w.dtype} and shape {w.shape}: float32 ({T},)')
    s = np.zeros(int(n), dtype=np.float64)
    for o in offsets:
        if not 0 <= o <= n - T:
            raise ValueError(f'offset {o} outside [0, {n - T}]')
        s[o:o + T] += w.astype(np.float64)
    return (s * float(scale)).astype(np.float32)


def tile_views(mirror=''):
    """the flag masks of the 2^len(mirror) mirrored views, in launch order: `mirror` names distinct axes of 'hwd'; view v counts in binary over
    the named axes in h, w, d order, the first named axis the lowest bit; view 0 is the identity.  Bits: patch3d.FLIP_H | FLIP_W | FLIP_D."""
    if not isinstance(mirror, str) or any(a not in 'hwd' for a in mirror) or len(set(mirror)) != len(mirror):
        raise ValueError(f'mirror {mirror!r}: distinct letters of "hwd" (or the empty string)')
    bits = [patch3d.FLIP_BITS[a] for a in 'hwd' if a in mirror]
    return [sum(b for i, b in enumerate(bits) if v >> i & 1) for v in range(1 << len(bits))]


def predict_tiles(model, loader, tile, stride=None, weight='gaussian', sigma=0.125, mirror='', limit=None):
    """`predict_volumes` tile by tile: the net runs on (TH, TW, TD) tiles that overlap along all three axes (`tile_offsets`), the sigmoid
    probabilities are blended with a separable weight (`tile_weights`) and averaged over the mirrored views of `mirror` (`tile_views`), each view
    put back before it is added.  Yields `predict_volumes`' dict plus 'tiles', the list of origins (h0, w0, d0), and 'views', the list of flag
    masks, both in launch order; `acc` holds the weighted sums.  The rule -- offsets, views, weights, fp32 order, normalisation by the product
    of three axis sums -- is stated in include/mrdis.h and is this package's own convention.

    Eval mode, no_grad; an `NVNet3D` runs its `unet` only.  Per batch: per tile and view one gather of the inputs (`loader.tile`), one forward
    and one `tilepred.tile_accum` launch, then one `tilepred.tile_label_volume`; the weights and axis sums are uploaded once; nothing syncs with the
    host.  The batches are those of `loader.plain_plan`, and no random stream is touched.  The loader must serve the items as stored."""
    ds = loader.dataset
    if ds.aug or ds.dropoff:
        raise ValueError('predict_tiles reads the volumes as stored: the loader must have aug=False and dropoff=False')
    shape = tuple(ds.store.shape)
    tile = _triple(tile, 'tile')
    offsets = tile_offsets(shape, tile, stride)
    views = tile_views(mirror)
    w = [tile_weights(t, weight, sigma) for t in tile]
    norms = [tile_norm(n, t, o, wa, len(views) if a == 2 else 1) for a, (n, t, o, wa) in enumerate(zip(shape, tile, offsets, w))]
    origins = [(h0, w0, d0) for h0 in offsets[0] for w0 in offsets[1] for d0 in offsets[2]]
    net = model.unet if isinstance(model, NVNet3D) else model
    C = net.out_channels
    dev = ds.store.device
    w = tuple(torch.from_numpy(a).to(dev) for a in w)
    norms = tuple(torch.from_numpy(a).to(dev) for a in norms)
    relabel = ds.dataset_name == 'BraTS'
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            for k, _, metas in loader.plain_plan(limit):
                subj_id = [m[0] for m in metas]
                acc = torch.zeros((len(metas), *shape, C), dtype=torch.float32, device=dev)
                ptrs = None
                for origin in origins:
                    for flips in views:
                        batch = loader.tile(k, metas, origin, flips=flips, tile=tile)
                        if batch['subj_id'] != subj_id:
                            raise RuntimeError(f'tile {origin} of batch {k} serves {batch["subj_id"]}, not {subj_id}')
                        if ptrs is None:
                            ptrs = loader.target_ptrs(batch)
                        tilepred.tile_accum(net(batch['inputs'])[0], acc, w, origin, flips)
                        del batch
                labels, counts = tilepred.tile_label_volume(acc, norms, ptrs, relabel=relabel)
                yield {'subj_id': subj_id, 'labels': labels, 'counts': counts, 'acc': acc, 'target_ptrs': ptrs, 'tiles': list(origins),
                       'views': list(views)}
    finally:
        net.train(was_training)
