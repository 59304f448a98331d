"""face-vid2vid's keypoint detector and head-pose estimator (src/pretrained/face_vid2vid/) -- MI355X-native.  Frames -> canonical
keypoints, head pose in degrees, and the transformed keypoints `make_animation` (driven_demo.py:182-211) hands to its generator.

This is everything `make_animation` computes before it calls the generator; the generator's dense motion and 3-D feature warp are
reenact_warp.py, its SPADE decoder spade.py.  `KPDetector` and `HEEstimator` take the reference's constructor arguments and
hold the reference's parameter tree (modules/keypoint_detector.py, modules/util.py), so a checkpoint's ['kp_detector'] and ['he_estimator'] load with
load_state_dict(strict=True).  The modules hold parameters only; execution is on channels-last buffers:

    reference                                               here
    ------------------------------------------------------  ------------------------------------------------------------------
    AntiAliasInterpolation2d (pad, 13x13 depthwise conv,    e4s_aa_down_f32: the separable Gaussian at the kept positions only
      [::4, ::4])
    DownBlock2d: conv 3x3 + BatchNorm2d + ReLU, AvgPool2d   e4s_conv_smallcin_f32 (3 channels in) / e4s_rconv_f32 with the BatchNorm
                                                              folded on the host, then e4s_avgpool2_f32
    KPHourglass.conv 1x1 and .view(b, c / d, d, h, w)       e4s_rconv_f32 with its output channels permuted (reshape_permutation):
                                                              the NHWC result IS the volume, read through strides -- no copy
    UpBlock3d: F.interpolate (1, 2, 2), Conv3d + BatchNorm  e4s_conv3d_f32 (the up-sampling folded into its reads, BatchNorm3d
      3d + ReLU; the kp and jacobian Conv3d heads             folded on the host)
    softmax(logits / T), gaussian2kp, the jacobian sum      e4s_softargmax3d_f32
    HEEstimator: conv1 7x7 / 2, maxpool, 1x1 convs,         e4s_conv_smallcin_f32, e4s_maxpool3s2p1_f32, e4s_rconv_f32 (the residual
      ResBottlenecks                                          and the strided 1x1 skip in conv3's epilogue)
    adaptive_avg_pool2d, fc_roll / pitch / yaw / t / exp,   e4s_pose_f32 (one launch)
      headpose_pred_to_degree, get_rotation_matrix,
      keypoint_transformation

The reference's quirks are kept (they are what its checkpoints were trained with):
  * HEEstimator returns 'yaw' from fc_roll and 'roll' from fc_yaw (keypoint_detector.py:172-174).
  * get_rotation_matrix converts degrees with pi = 3.14 (driven_demo.py:108-110).
  * The rotation is pitch_mat @ yaw_mat @ roll_mat (driven_demo.py:131).
  * headpose_pred_to_degree calls F.softmax without dim on a 2-D tensor, which means dim 1, and always uses 66 bin indices.
  * KPDetector.jacobian starts with zero weights and an identity bias (keypoint_detector.py:34-35).
One quirk is NOT kept: the reference's keypoint_transformation reshapes he['t'] in place (t.unsqueeze_(1)), which makes a second
call with the same dict fail; here the argument is left alone.

Arithmetic follows kernels.PRECISION: "f32" runs the exact fp32 MFMA, "bf16x3" and "auto" the split-bf16 path.  Folded weights are
re-packed once per weight version and precision; the working set is cached per frame shape; results are fresh tensors.  Eval mode
only, no CPU path."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K
from . import packs


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------------
def fold_conv_bn_bias(weight, bias, bn):
    """Conv (2-D or 3-D, with bias) followed by eval-mode BatchNorm as one conv: (W * s[co], beta + (b - mean) * s) with s = gamma /
    sqrt(var + eps).  Computed in fp64, returned in the dtype of weight."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w = weight.double() * s.view(-1, *([1] * (weight.dim() - 1)))
    b0 = bias.double() if bias is not None else torch.zeros_like(s)
    b = bn.bias.double() + (b0 - bn.running_mean.double()) * s
    return w.to(weight.dtype), b.to(weight.dtype)


def antialias_taps(scale):
    """The normalised 1-D Gaussian of AntiAliasInterpolation2d(scale) (util.py:374-397; its 2-D kernel is the outer product of this
    with itself) and the step int(1 / scale): (float64 numpy taps, step).  sigma = (1 / scale - 1) / 2, size 2 round(4 sigma) + 1."""
    sigma = (1 / scale - 1) / 2
    size = 2 * round(sigma * 4) + 1
    i = np.arange(size, dtype=np.float64)
    g = np.exp(-(i - (size - 1) / 2) ** 2 / (2 * sigma ** 2))
    return g / g.sum(), int(1 / scale)


def antialias_size(n, scale):
    """Rows kept by AntiAliasInterpolation2d(scale) of n rows: the padded conv keeps n, [::step] keeps ceil(n / step)."""
    return n if scale == 1 else -(-n // int(1 / scale))


def kp_map_sizes(h, w, scale_factor, num_blocks):
    """[(h, w) after the anti-alias down-sampling, then after each DownBlock2d (AvgPool2d(2) floors)] of an h x w frame."""
    out = [(antialias_size(h, scale_factor), antialias_size(w, scale_factor))]
    for _ in range(num_blocks):
        h2, w2 = out[-1][0] // 2, out[-1][1] // 2
        if h2 < 1 or w2 < 1:
            raise ValueError(f"KPDetector: a {h} x {w} frame vanishes in the {num_blocks} down blocks")
        out.append((h2, w2))
    return out


def he_map_sizes(h, w):
    """[(h, w) after conv1 (7x7 / 2), the max pool, block2, block4, block6] of an h x w frame: ceil(n / 2) each."""
    out = []
    for _ in range(5):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append((h, w))
    return out


def reshape_permutation(channels, depth):
    """KPHourglass views its 1x1 conv's output [B,C,h,w] as [B,C/depth,depth,h,w]: channel c is (feature c // depth, depth c %
    depth).  perm[depth_index * (C / depth) + feature] = c, so that a conv with weight[perm] writes, channels-last, [B,h,w,depth,C /
    depth]: the volume the 3-D conv reads as [B,depth,h,w,C/depth] through strides."""
    if channels % depth:
        raise ValueError(f"reshape_channel {channels} is no multiple of reshape_depth {depth}")
    return torch.arange(channels).view(channels // depth, depth).t().reshape(-1)


def headpose_pred_to_degree(pred):
    """driven_demo.py:67-74: softmax over dim 1 (F.softmax without dim on a 2-D tensor), sum p * idx over 66 bins, * 3 - 99."""
    idx = torch.arange(66, device=pred.device, dtype=torch.float32)
    pred = F.softmax(pred, dim=1)
    return torch.sum(pred * idx, axis=1) * 3 - 99


def get_rotation_matrix(yaw, pitch, roll):
    """driven_demo.py:107-133: degrees [B] -> [B,3,3] = Rx(pitch) @ Ry(yaw) @ Rz(roll), with the reference's pi = 3.14."""
    yaw, pitch, roll = (a / 180 * 3.14 for a in (yaw, pitch, roll))
    roll, pitch, yaw = roll.unsqueeze(1), pitch.unsqueeze(1), yaw.unsqueeze(1)
    one, zero = torch.ones_like, torch.zeros_like
    pitch_mat = torch.cat([one(pitch), zero(pitch), zero(pitch), zero(pitch), torch.cos(pitch), -torch.sin(pitch),
                           zero(pitch), torch.sin(pitch), torch.cos(pitch)], dim=1).view(-1, 3, 3)
    yaw_mat = torch.cat([torch.cos(yaw), zero(yaw), torch.sin(yaw), zero(yaw), one(yaw), zero(yaw),
                         -torch.sin(yaw), zero(yaw), torch.cos(yaw)], dim=1).view(-1, 3, 3)
    roll_mat = torch.cat([torch.cos(roll), -torch.sin(roll), zero(roll), torch.sin(roll), torch.cos(roll), zero(roll),
                          zero(roll), zero(roll), one(roll)], dim=1).view(-1, 3, 3)
    return torch.einsum("bij,bjk,bkm->bim", pitch_mat, yaw_mat, roll_mat)


def keypoint_transformation(kp_canonical, he, estimate_jacobian=True, free_view=False, yaw=0, pitch=0, roll=0):
    """driven_demo.py:135-180 on torch tensors of any device and dtype: {'value' [B,K,3], 'jacobian' [B,K,3,3] | None}.  free_view:
    an angle given as a number replaces the estimate (None keeps it).  he['t'] is not reshaped in place (see the module docstring)."""
    kp = kp_canonical["value"]
    angles = {}
    for name, fixed in (("yaw", yaw), ("pitch", pitch), ("roll", roll)):
        if free_view and fixed is not None:
            angles[name] = torch.tensor([fixed], device=kp.device, dtype=kp.dtype)
        else:
            angles[name] = headpose_pred_to_degree(he[name])
    t, exp = he["t"], he["exp"]
    rot_mat = get_rotation_matrix(angles["yaw"], angles["pitch"], angles["roll"])
    kp_rotated = torch.einsum("bmp,bkp->bkm", rot_mat, kp)
    kp_t = kp_rotated + t.unsqueeze(1).repeat(1, kp.shape[1], 1)
    kp_transformed = kp_t + exp.view(exp.shape[0], -1, 3)
    jacobian_transformed = torch.einsum("bmp,bkps->bkms", rot_mat, kp_canonical["jacobian"]) if estimate_jacobian else None
    return {"value": kp_transformed, "jacobian": jacobian_transformed}


# ---- the reference's parameter trees ------------------------------------------------------------------------------------------------
class DownBlock2d(nn.Module):
    def __init__(self, in_features, out_features, kernel_size=3, padding=1, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(in_features, out_features, kernel_size=kernel_size, padding=padding, groups=groups)
        self.norm = nn.BatchNorm2d(out_features, affine=True)


class UpBlock3d(nn.Module):
    def __init__(self, in_features, out_features, kernel_size=3, padding=1, groups=1):
        super().__init__()
        self.conv = nn.Conv3d(in_features, out_features, kernel_size=kernel_size, padding=padding, groups=groups)
        self.norm = nn.BatchNorm3d(out_features, affine=True)


class KPHourglass(nn.Module):
    """util.py:333-366"""

    def __init__(self, block_expansion, in_features, reshape_features, reshape_depth, num_blocks=3, max_features=256):
        super().__init__()
        self.down_blocks = nn.Sequential()
        for i in range(num_blocks):
            self.down_blocks.add_module("down" + str(i), DownBlock2d(in_features if i == 0 else min(max_features, block_expansion * (2 ** i)),
                                                                    min(max_features, block_expansion * (2 ** (i + 1)))))
        in_filters = min(max_features, block_expansion * (2 ** num_blocks))
        self.conv = nn.Conv2d(in_filters, reshape_features, kernel_size=1)
        self.up_blocks = nn.Sequential()
        out_filters = None
        for i in range(num_blocks):
            in_filters = min(max_features, block_expansion * (2 ** (num_blocks - i)))
            out_filters = min(max_features, block_expansion * (2 ** (num_blocks - i - 1)))
            self.up_blocks.add_module("up" + str(i), UpBlock3d(in_filters, out_filters))
        self.reshape_depth = reshape_depth
        self.out_filters = out_filters


class AntiAliasInterpolation2d(nn.Module):
    """util.py:370-416: holds the reference's buffer `weight` [channels,1,k,k], built in float32 as the reference builds it."""

    def __init__(self, channels, scale):
        super().__init__()
        sigma = (1 / scale - 1) / 2
        size = 2 * round(sigma * 4) + 1
        i = torch.arange(size, dtype=torch.float32)
        g = torch.exp(-(i - (size - 1) / 2) ** 2 / (2 * sigma ** 2))
        kernel = g[:, None] * g[None, :]
        kernel = kernel / torch.sum(kernel)
        self.register_buffer("weight", kernel.view(1, 1, size, size).repeat(channels, 1, 1, 1))
        self.scale = scale
        self.int_inv_scale = int(1 / scale)


class _Native(nn.Module):
    """Eval-only holder of a reference parameter tree with cached packs and per-shape buffers."""

    def _init_native(self):
        self._e4s_bufs = {}
        self._weights_loaded = False
        super().train(False)

    def train(self, mode=True):
        if mode:
            raise RuntimeError(f"{type(self).__name__}: the native module is inference only (eval mode); train() is refused")
        return super().train(False)

    def load_state_dict(self, state_dict, strict=True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self._weights_loaded = True
        return res

    def _require_weights(self):
        from . import criteria
        if not self._weights_loaded and not criteria.ALLOW_UNINITIALIZED:
            raise RuntimeError(f"{type(self).__name__}: no weights were loaded (load_state_dict of the checkpoint's entry first).  Running "
                               "a randomly initialised network is silently meaningless; set E4S_ALLOW_UNINITIALIZED_LOSS_NETS=1 for "
                               "synthetic-weight runs.")

    def release_workspace(self):
        """Drop every cached buffer set (a captured graph that used one keeps it alive)."""
        self._e4s_bufs = {}

    def _workspace(self, bsz, h, w, device):
        ws = self._e4s_bufs.setdefault((bsz, h, w, str(device)), {})

        def new(tag, *shape, dtype=torch.float32):
            k = (tag,) + tuple(shape)
            if k not in ws:
                ws[k] = torch.empty(bsz, *shape, device=device, dtype=dtype)
            return ws[k]
        return new

    def _folded(self, name, conv, bn, pack, perm=None):
        """pack(folded weight, f32) and the folded bias of conv (+ eval BatchNorm), cached per weight version and precision.  perm: the
        output channels are re-ordered (new channel i is old channel perm[i]) before packing."""
        f32 = K.sr_f32()
        tensors = [conv.weight, conv.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])

        def build():
            if bn is not None:
                w, b = fold_conv_bn_bias(conv.weight.detach().float(), conv.bias.detach().float(), bn)
            else:
                w, b = conv.weight.detach().float(), conv.bias.detach().float()
            if perm is not None:
                w, b = w[perm.to(w.device)], b[perm.to(b.device)]
            return pack(w.contiguous(), f32), b.contiguous()
        return packs.cached(self, name, tensors, build, (f32,))

    def _rconv(self, name, conv, bn, x, y, perm=None, **kw):
        w, b = self._folded(name, conv, bn, K.rconv_pack, perm)
        return K.rconv(x, conv.in_channels, w, conv.out_channels, conv.kernel_size[0], y, bias=b, stride=conv.stride[0], **kw)

    def _smallcin(self, name, conv, bn, x, y):
        w, b = self._folded(name, conv, bn, lambda w, f32: K.pack_smallcin(w))
        return K.conv_smallcin_into(x, w, b, y, conv.kernel_size[0], conv.stride[0], conv.padding[0], relu=True)

    def _conv3d(self, name, conv, bn, x, y, **kw):
        w, b = self._folded(name, conv, bn, K.conv3d_pack)
        return K.conv3d(x, w, conv.out_channels, y, bias=b, **kw)

    def forward(self, *a, **kw):
        raise NotImplementedError(f"{type(self).__name__}: call run(frames) or PoseFrontEnd (the net runs on channels-last device frames)")


def _frames(frames, device, what):
    """[H,W,3] or [B,H,W,3] float in [0,1] or uint8, numpy or tensor -> a contiguous device tensor [B,H,W,3] (fp32 or uint8)."""
    t = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
    if isinstance(t, (list, tuple)):
        t = torch.stack([torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f for f in t])
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"{what}: frames [H,W,3] or [B,H,W,3], float in [0,1] or uint8")
    if t.dtype != torch.uint8:
        if not t.is_floating_point():
            raise ValueError(f"{what}: frames are float in [0,1] or uint8, got {t.dtype}")
        t = t.float()
    t = t if t.dim() == 4 else t[None]
    if min(t.shape[:3]) < 1:
        raise ValueError(f"{what}: empty frames")
    return t.to(device).contiguous()


def _device_frames(frames, what):
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise RuntimeError(f"{what}: device frames only (there is no CPU path)")
    return _frames(frames, frames.device, what)


class KPDetector(_Native):
    """keypoint_detector.py:9-82.  run(frames) -> {'value' [B,K,3], 'jacobian' [B,K,3,3] (with estimate_jacobian)}.  `jacobian` is
    zero-weight / identity-bias at construction, as in the reference."""

    def __init__(self, block_expansion, feature_channel, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks,
                 temperature, estimate_jacobian=False, scale_factor=1, single_jacobian_map=False):
        super().__init__()
        if image_channel != 3:
            raise NotImplementedError("KPDetector: the native detector takes 3-channel frames")
        self.predictor = KPHourglass(block_expansion, in_features=image_channel, max_features=max_features,
                                     reshape_features=reshape_channel, reshape_depth=reshape_depth, num_blocks=num_blocks)
        self.kp = nn.Conv3d(self.predictor.out_filters, num_kp, kernel_size=3, padding=1)
        if estimate_jacobian:
            self.num_jacobian_maps = 1 if single_jacobian_map else num_kp
            self.jacobian = nn.Conv3d(self.predictor.out_filters, 9 * self.num_jacobian_maps, kernel_size=3, padding=1)
            self.jacobian.weight.data.zero_()
            self.jacobian.bias.data.copy_(torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1] * self.num_jacobian_maps, dtype=torch.float))
        else:
            self.jacobian = None
        self.temperature = temperature
        self.scale_factor = scale_factor
        if self.scale_factor != 1:
            self.down = AntiAliasInterpolation2d(image_channel, self.scale_factor)
        p = self.predictor
        for i, blk in enumerate(p.down_blocks):
            if blk.conv.out_channels % 64 or (i > 0 and blk.conv.in_channels % 32):
                raise NotImplementedError("KPDetector: down blocks of 64 j output and (past the first) 32 k input channels")
        if reshape_channel % reshape_depth or (reshape_channel // reshape_depth) != p.up_blocks[0].conv.in_channels:
            raise ValueError("KPDetector: reshape_channel / reshape_depth must equal the first up block's input channels")
        if reshape_channel % 64 or any(b.conv.in_channels % 32 for b in p.up_blocks) or p.out_filters % 32:
            raise NotImplementedError("KPDetector: a reshape_channel of 64 j and 3-D blocks of 32 k input channels")
        self._perm = reshape_permutation(reshape_channel, reshape_depth)
        self._init_native()

    def _taps(self, device):
        def build():
            taps, step = antialias_taps(self.scale_factor) if self.scale_factor != 1 else (np.ones(1), 1)
            return torch.from_numpy(taps).float().to(device), step
        return packs.cached(self, "aa", (), build, (str(device),))       # no weight pack, a per-device constant: no tensors in its key (an
                                                                         # invalidate_packs() rebuilds it with the rest, which costs one tiny copy)

    def logits_ndhwc(self, frames, taps=None):
        """Device frames [B,H,W,3] (fp32 in [0,1] or uint8) -> (kp logits [B,D,H,W,K], jacobian maps [B,D,H,W,9 J] | None), in the
        shape's cached workspace (valid until the next call at the shape).  taps: a dict that receives named intermediate buffers."""
        self._require_weights()
        bsz, h, w, _ = frames.shape
        new = self._workspace(bsz, h, w, frames.device)

        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t
        p = self.predictor
        sizes = kp_map_sizes(h, w, self.scale_factor, len(p.down_blocks))
        g, step = self._taps(frames.device)
        x = tap("aa", K.aa_down(frames, g, step, out=new("aa", *sizes[0], 3)))
        for i, blk in enumerate(p.down_blocks):
            c = blk.conv.out_channels
            y = new(f"down{i}.c", *sizes[i], c)
            if i == 0:
                self._smallcin("down0", blk.conv, blk.norm, x, y)
            else:
                self._rconv(f"down{i}", blk.conv, blk.norm, x, y, act=True)
            x = tap(f"down{i}", K.avgpool2(y, new(f"down{i}", *sizes[i + 1], c)))
        hh, ww = sizes[-1]
        d, c3 = p.reshape_depth, p.conv.out_channels // p.reshape_depth
        flat = self._rconv("reshape", p.conv, None, x, new("reshape", hh, ww, d * c3), perm=self._perm)
        x = tap("reshape", flat.view(bsz, hh, ww, d, c3).permute(0, 3, 1, 2, 4))         # [B,D,h,w,C]: no copy
        for i, blk in enumerate(p.up_blocks):
            hh, ww = 2 * hh, 2 * ww
            x = tap(f"up{i}", self._conv3d(f"up{i}", blk.conv, blk.norm, x, new(f"up{i}", d, hh, ww, blk.conv.out_channels), relu=True, up2=True))
        logits = tap("logits", self._conv3d("kp", self.kp, None, x, new("logits", d, hh, ww, self.kp.out_channels)))
        jmaps = None
        if self.jacobian is not None:
            jmaps = tap("jmaps", self._conv3d("jacobian", self.jacobian, None, x, new("jmaps", d, hh, ww, self.jacobian.out_channels)))
        return logits, jmaps

    @torch.no_grad()
    def run(self, frames, taps=None):
        f = _device_frames(frames, "KPDetector.run")
        logits, jmaps = self.logits_ndhwc(f, taps)
        value, jac = K.softargmax3d(logits, self.temperature, jmaps, channels_last=True)
        out = {"value": value}
        if jac is not None:
            out["jacobian"] = jac
        return out


class ResBottleneck(nn.Module):
    """util.py:72-101"""

    def __init__(self, in_features, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(in_features, in_features // 4, kernel_size=1)
        self.conv2 = nn.Conv2d(in_features // 4, in_features // 4, kernel_size=3, padding=1, stride=stride)
        self.conv3 = nn.Conv2d(in_features // 4, in_features, kernel_size=1)
        self.norm1 = nn.BatchNorm2d(in_features // 4, affine=True)
        self.norm2 = nn.BatchNorm2d(in_features // 4, affine=True)
        self.norm3 = nn.BatchNorm2d(in_features, affine=True)
        self.stride = stride
        if self.stride != 1:
            self.skip = nn.Conv2d(in_features, in_features, kernel_size=1, stride=stride)
            self.norm4 = nn.BatchNorm2d(in_features, affine=True)


class HEEstimator(_Native):
    """keypoint_detector.py:85-178.  run(frames) -> {'yaw' [B,bins], 'pitch', 'roll', 't' [B,3], 'exp' [B,3 K]}; 'yaw' comes from
    fc_roll and 'roll' from fc_yaw, as in the reference.  max_features is accepted and, as in the reference, unused."""

    def __init__(self, block_expansion, feature_channel, num_kp, image_channel, max_features, num_bins=66, estimate_jacobian=True):
        super().__init__()
        if image_channel != 3 or block_expansion % 32 or block_expansion < 32:
            raise NotImplementedError("HEEstimator: 3-channel frames and a block_expansion of 32 k")
        self.conv1 = nn.Conv2d(image_channel, block_expansion, kernel_size=7, padding=3, stride=2)
        self.norm1 = nn.BatchNorm2d(block_expansion, affine=True)
        self.conv2 = nn.Conv2d(block_expansion, 256, kernel_size=1)
        self.norm2 = nn.BatchNorm2d(256, affine=True)
        self.block1 = nn.Sequential()
        for i in range(3):
            self.block1.add_module("b1_" + str(i), ResBottleneck(256, 1))
        self.conv3 = nn.Conv2d(256, 512, kernel_size=1)
        self.norm3 = nn.BatchNorm2d(512, affine=True)
        self.block2 = ResBottleneck(512, 2)
        self.block3 = nn.Sequential()
        for i in range(3):
            self.block3.add_module("b3_" + str(i), ResBottleneck(512, 1))
        self.conv4 = nn.Conv2d(512, 1024, kernel_size=1)
        self.norm4 = nn.BatchNorm2d(1024, affine=True)
        self.block4 = ResBottleneck(1024, 2)
        self.block5 = nn.Sequential()
        for i in range(5):
            self.block5.add_module("b5_" + str(i), ResBottleneck(1024, 1))
        self.conv5 = nn.Conv2d(1024, 2048, kernel_size=1)
        self.norm5 = nn.BatchNorm2d(2048, affine=True)
        self.block6 = ResBottleneck(2048, 2)
        self.block7 = nn.Sequential()
        for i in range(2):
            self.block7.add_module("b7_" + str(i), ResBottleneck(2048, 1))
        self.fc_roll = nn.Linear(2048, num_bins)
        self.fc_pitch = nn.Linear(2048, num_bins)
        self.fc_yaw = nn.Linear(2048, num_bins)
        self.fc_t = nn.Linear(2048, 3)
        self.fc_exp = nn.Linear(2048, 3 * num_kp)
        self.num_bins, self.num_kp = num_bins, num_kp
        self._init_native()

    def _heads(self):
        """w [3 bins + 3 + 3 K, 2048], bias: rows in the reference's OUTPUT order yaw (fc_roll), pitch, roll (fc_yaw), t, exp."""
        fcs = [self.fc_roll, self.fc_pitch, self.fc_yaw, self.fc_t, self.fc_exp]
        return packs.cached(self, "heads", [t for fc in fcs for t in (fc.weight, fc.bias)],
                            lambda: (torch.cat([fc.weight.detach().float() for fc in fcs]).contiguous(),
                                     torch.cat([fc.bias.detach().float() for fc in fcs]).contiguous()))

    def _bottleneck(self, name, blk, x, new, tag, k):
        """One ResBottleneck on NHWC x into the stage's output buffer k & 1 (x is the other one, or the stage's first conv)."""
        b, h, w, c = x.shape
        ho, wo = K.rconv_out_size(h, 3, blk.stride), K.rconv_out_size(w, 3, blk.stride)
        t1 = self._rconv(name + ".1", blk.conv1, blk.norm1, x, new(tag + ".t1", h, w, c // 4), act=True)
        t2 = self._rconv(name + ".2", blk.conv2, blk.norm2, t1, new(tag + ".t2", ho, wo, c // 4), act=True)
        idt = x if blk.stride == 1 else self._rconv(name + ".skip", blk.skip, blk.norm4, x, new(tag + ".skip", ho, wo, c))
        return self._rconv(name + ".3", blk.conv3, blk.norm3, t2, new(f"{tag}.o{k & 1}", ho, wo, c), act=True, r0=idt)

    def features_nhwc(self, frames, taps=None):
        """Device frames [B,H,W,3] -> the last map [B,h,w,2048], in the shape's cached workspace."""
        self._require_weights()
        bsz, h, w, _ = frames.shape
        new = self._workspace(bsz, h, w, frames.device)

        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t
        sizes = he_map_sizes(h, w)
        if frames.dtype == torch.uint8:
            one = packs.cached(self, "one", (), lambda: torch.ones(1, device=frames.device), (str(frames.device),))      # (a constant, as "aa")
            frames = K.aa_down(frames, one, 1, out=new("x0", h, w, 3))
        x = tap("conv1", self._smallcin("conv1", self.conv1, self.norm1, frames, new("conv1", *sizes[0], self.conv1.out_channels)))
        x = tap("pool", K.retina_pool(x, new("pool", *sizes[1], x.shape[3])))
        stages = ((self.conv2, self.norm2, self.block1, None), (self.conv3, self.norm3, self.block3, self.block2),
                  (self.conv4, self.norm4, self.block5, self.block4), (self.conv5, self.norm5, self.block7, self.block6))
        for si, (conv, norm, same, strided) in enumerate(stages):
            n = si + 2
            x = self._rconv(f"conv{n}", conv, norm, x, new(f"conv{n}", x.shape[1], x.shape[2], conv.out_channels), act=True)
            blocks = ([(f"block{2 * si}", strided)] if strided is not None else []) + [(f"block{2 * si + 1}.{bi}", blk) for bi, blk in enumerate(same)]
            for k, (name, blk) in enumerate(blocks):
                x = self._bottleneck(name, blk, x, new, f"s{n}", k)
            tap(f"stage{n}", x)
        return x

    def pose(self, frames, kp_value=None, kp_jacobian=None, fixed=(None, None, None), taps=None):
        """Device frames -> dict of FRESH tensors: raw [B,3 bins + 3 + 3 K], degrees [B,3] (yaw, pitch, roll), rot [B,3,3], and with
        kp_value [1|B,K,3] the transformed value [B,K,3] (with kp_jacobian the transformed jacobian [B,K,3,3])."""
        x = self.features_nhwc(frames, taps)
        b, dev = x.shape[0], x.device
        nout = 3 * self.num_bins + 3 + 3 * self.num_kp
        out = {"raw": torch.empty(b, nout, device=dev), "degrees": torch.empty(b, 3, device=dev), "rot": torch.empty(b, 3, 3, device=dev)}
        if kp_value is not None:
            out["value"] = torch.empty(b, self.num_kp, 3, device=dev)
            if kp_jacobian is not None:
                out["jacobian"] = torch.empty(b, self.num_kp, 3, 3, device=dev)
        w, bias = self._heads()
        return K.pose(x, w, bias, self.num_bins, self.num_kp, out, kp_value, kp_jacobian, fixed)

    def split_raw(self, raw):
        """raw [B,3 bins + 3 + 3 K] -> the reference's output dict (views)."""
        nb = self.num_bins
        return {"yaw": raw[:, :nb], "pitch": raw[:, nb:2 * nb], "roll": raw[:, 2 * nb:3 * nb], "t": raw[:, 3 * nb:3 * nb + 3],
                "exp": raw[:, 3 * nb + 3:]}

    @torch.no_grad()
    def run(self, frames, taps=None):
        return self.split_raw(self.pose(_device_frames(frames, "HEEstimator.run"), taps=taps)["raw"])


class PoseFrontEnd(object):
    """What make_animation (driven_demo.py:182-211) computes before it calls the generator.  kp_detector / he_estimator: the native
    modules above, on the device, with their weights loaded; estimate_jacobian: the checkpoint's common_params flag."""

    def __init__(self, kp_detector, he_estimator, estimate_jacobian):
        if not isinstance(kp_detector, KPDetector) or not isinstance(he_estimator, HEEstimator):
            raise TypeError("PoseFrontEnd: e4s_amd.reenact.KPDetector and HEEstimator")
        if estimate_jacobian and kp_detector.jacobian is None:
            raise ValueError("PoseFrontEnd: estimate_jacobian needs a KPDetector built with estimate_jacobian=True")
        if he_estimator.num_bins != 66:
            raise ValueError("PoseFrontEnd: headpose_pred_to_degree knows 66 bins")
        if he_estimator.num_kp != kp_detector.kp.out_channels:
            raise ValueError("PoseFrontEnd: the two networks disagree on num_kp")
        self.kp_detector, self.he_estimator, self.estimate_jacobian = kp_detector, he_estimator, bool(estimate_jacobian)

    @property
    def device(self):
        return self.he_estimator.fc_t.weight.device

    @torch.no_grad()
    def head_pose_device(self, frames):
        """Device frames [H,W,3] or [B,H,W,3] -> {'yaw', 'pitch', 'roll': degrees [B]; 't' [B,3]; 'exp' [B,3 K]}.  Stream-ordered, no
        host synchronisation."""
        out = self.he_estimator.pose(_device_frames(frames, "PoseFrontEnd.head_pose_device"))
        he = self.he_estimator.split_raw(out["raw"])
        deg = out["degrees"]
        return {"yaw": deg[:, 0], "pitch": deg[:, 1], "roll": deg[:, 2], "t": he["t"], "exp": he["exp"]}

    def head_pose(self, frames):
        """Frames (numpy or tensor, float in [0,1] or uint8) -> head_pose_device's dict (device tensors)."""
        return self.head_pose_device(_frames(frames, self.device, "PoseFrontEnd.head_pose"))

    @torch.no_grad()
    def keypoints_device(self, source, driving=None, free_view=False, yaw=0, pitch=0, roll=0):
        """Device source frame [H,W,3] and driving frames [N,H,W,3] (or None) -> (kp_source, [kp_driving per frame]): the dicts
        {'value' [1,K,3], 'jacobian' [1,K,3,3] | None} make_animation hands to the generator.  free_view with yaw / pitch / roll in
        degrees (None keeps the estimate) applies to the driving frames, as in make_animation.  No host synchronisation."""
        src = _device_frames(source, "PoseFrontEnd.keypoints_device")
        if src.shape[0] != 1:
            raise ValueError("PoseFrontEnd.keypoints: one source frame")
        kp_can = self.kp_detector.run(src)
        kv, kj = kp_can["value"], kp_can.get("jacobian") if self.estimate_jacobian else None
        s = self.he_estimator.pose(src, kv, kj)
        kp_source = {"value": s["value"], "jacobian": s.get("jacobian")}
        kp_driving = []
        if driving is not None:
            drv = _device_frames(driving, "PoseFrontEnd.keypoints_device")
            fixed = (yaw, pitch, roll) if free_view else (None, None, None)
            d = self.he_estimator.pose(drv, kv, kj, fixed)
            for i in range(drv.shape[0]):
                kp_driving.append({"value": d["value"][i:i + 1], "jacobian": d["jacobian"][i:i + 1] if kj is not None else None})
        return kp_source, kp_driving

    def keypoints(self, source, driving=None, free_view=False, yaw=0, pitch=0, roll=0):
        """The same for numpy or tensor frames: source [H,W,3], driving a list of frames or [N,H,W,3]."""
        dev = self.device
        drv = None if driving is None or len(driving) == 0 else _frames(driving, dev, "PoseFrontEnd.keypoints")
        return self.keypoints_device(_frames(source, dev, "PoseFrontEnd.keypoints"), drv, free_view, yaw, pitch, roll)
