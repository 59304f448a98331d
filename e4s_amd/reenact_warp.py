"""face-vid2vid's dense motion and 3-D feature warp (src/pretrained/face_vid2vid/modules/dense_motion.py, generator.py:211-246) --
MI355X-native.  Everything OcclusionAwareSPADEGenerator.forward does before `self.decoder(out)`: the appearance encoder and its
reshape into a feature volume, the ResBlock3d stack, the whole DenseMotionNetwork, the 3-D grid_sample warp, `third`, `fourth` and the
occlusion product.  The result is the map the SPADE decoder reads; the SPADE decoder itself is spade.py, whose
OcclusionAwareSPADEGenerator is FeatureWarp plus that decoder.

`DenseMotionNetwork` and `FeatureWarp` take the reference's constructor arguments and hold the reference's parameter tree
(`FeatureWarp` without `decoder.*`), so a checkpoint's ['generator'] entry loads with FeatureWarp.load_generator_state_dict.  The
modules hold parameters only; execution is on channels-last buffers:

    reference                                              here
    -----------------------------------------------------  -------------------------------------------------------------------
    first, down_blocks, second, third, fourth              e4s_conv_smallcin_f32 / e4s_rconv_f32 / e4s_avgpool2_f32 with the BatchNorm
                                                             folded; `second`'s output channels and `third`'s input channels are
                                                             permuted on the host, so the volume and the warped map need no transpose
    ResBlock3d: BN, ReLU, conv, BN, ReLU, conv, + x        e4s_bnrelu3d_f32 (norm1 sits in front of a zero-padded conv: a padded tap
                                                             must contribute an exact zero, not relu(shift), so it cannot be folded and
                                                             runs as a streaming launch), then two e4s_conv3dx_f32: norm2 folded into
                                                             conv1, the residual in conv2's epilogue
    compress 1x1x1 + BN + ReLU                             e4s_conv3dx_f32, ksize 1
    create_sparse_motions, create_deformed_feature,        e4s_kp_jacobian_f32 (J_source inverse(J_driving)) and e4s_sparse_warp_f32:
      create_heatmap_representations, torch.cat              the 80-channel hourglass input, written straight into the last concat
                                                             buffer; the [N 16,4,D,H,W] intermediate is never made
    Hourglass: DownBlock3d, UpBlock3d, torch.cat           e4s_conv3dx_f32 + e4s_avgpool2s_f32; every up block and every skip's
                                                             producer write into a channel slice of the concat buffer (no cat copies);
                                                             channel counts 80 and 112 run through strides padded to 96 and 128 whose
                                                             pad channels are zeroed once and meet zero weight columns
    mask 7x7x7, softmax, the deformation sum               e4s_conv3dx_f32 (ksize 7), e4s_motion_combine_f32
    occlusion 7x7 + sigmoid                                e4s_occlusion_f32 (a reduction, one block per pixel)
    deform_input (F.grid_sample), .view(bs, c d, h, w)     e4s_warp3d_f32 (writes NHWC [N,h,w,D C])
    out * occlusion_map                                    e4s_scale_rows_f32

The reference's quirks are kept: the "identity" grid is an align_corners=True grid sampled with align_corners=False; `third`'s
LeakyReLU has slope 0.01; the heat maps' spatial size is the compressed volume's (d, h, w).  The F.interpolate branches (a
deformation or an occlusion map at another size than the volume) are not built: the shipped config never takes them.

The source is encoded ONCE (encode_source) and N driving frames run as one batch against it; make_animation re-encodes the source
for every frame.  Arithmetic follows kernels.PRECISION as in reenact.py.  Eval mode only, no CPU path, no host synchronisation."""
import torch
from torch import nn

from . import kernels as K
from . import packs
from .reenact import DownBlock2d, PoseFrontEnd, UpBlock3d, _Native, _device_frames, _frames, reshape_permutation


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------------
def pad32(c):
    return -(-c // 32) * 32


def third_input_permutation(channels, depth):
    """The warped volume [B,c,d,h,w] is viewed as [B,c d,h,w]: `third`'s input channel c * depth + d.  e4s_warp3d_f32 writes channel
    d * channels + c; perm[d * channels + c] = c * depth + d, so weight[:, perm] reads it (the inverse trick of reshape_permutation)."""
    return reshape_permutation(channels * depth, depth)


def encoder_map_sizes(h, w, num_down_blocks):
    """[(h, w) of `first`, then after each DownBlock2d (AvgPool2d(2) floors)]."""
    out = [(h, w)]
    for _ in range(num_down_blocks):
        h, w = h // 2, w // 2
        if h < 1 or w < 1:
            raise ValueError(f"FeatureWarp: the frame vanishes in the {num_down_blocks} down blocks")
        out.append((h, w))
    return out


def hourglass_layout(block_expansion, in_features, num_blocks, max_features):
    """The concat buffers of Hourglass(block_expansion, in_features, num_blocks, max_features).  Level i (0 = full size) holds
    torch.cat([up block's output, skip]) as {'up': channels of the up block, 'skip': channels of the skip, 'stride': the buffer's
    channel stride (their sum padded to a multiple of 32), 'skip_read': the channels a conv reads of the skip slice (padded to 32)};
    'bottom': the channels of the deepest map."""
    feat = lambda i: min(max_features, block_expansion * (2 ** i))
    levels = []
    for i in range(num_blocks):
        up, skip = feat(i), in_features if i == 0 else feat(i)
        levels.append({"up": up, "skip": skip, "stride": pad32(up + skip), "skip_read": pad32(skip)})
    return {"levels": levels, "bottom": feat(num_blocks)}


def hourglass_map_sizes(h, w, num_blocks):
    """[(h, w) of level 0 .. num_blocks]; every level must halve exactly (the reference's torch.cat fails otherwise)."""
    out = [(h, w)]
    for _ in range(num_blocks):
        if h % 2 or w % 2:
            raise ValueError(f"DenseMotionNetwork: a {out[0][0]} x {out[0][1]} volume does not halve {num_blocks} times")
        h, w = h // 2, w // 2
        out.append((h, w))
    return out


def inverse3x3(m):
    """The inverse of [...,3,3] matrices by cofactors, as e4s_kp_jacobian_f32 takes it."""
    a = m.reshape(-1, 9).unbind(1)
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = a[0] * c00 + a[1] * c01 + a[2] * c02
    inv = torch.stack([c00, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                       c01, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                       c02, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]], 1) / det[:, None]
    return inv.view(m.shape)


# ---- the reference's parameter trees ------------------------------------------------------------------------------------------------
class SameBlock2d(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.conv = nn.Conv2d(in_features, out_features, kernel_size=3, padding=1)
        self.norm = nn.BatchNorm2d(out_features, affine=True)


class ResBlock3d(nn.Module):
    def __init__(self, in_features):
        super().__init__()
        self.conv1 = nn.Conv3d(in_features, in_features, kernel_size=3, padding=1)
        self.conv2 = nn.Conv3d(in_features, in_features, kernel_size=3, padding=1)
        self.norm1 = nn.BatchNorm3d(in_features, affine=True)
        self.norm2 = nn.BatchNorm3d(in_features, affine=True)


class DownBlock3d(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.conv = nn.Conv3d(in_features, out_features, kernel_size=3, padding=1)
        self.norm = nn.BatchNorm3d(out_features, affine=True)


class Encoder(nn.Module):
    def __init__(self, block_expansion, in_features, num_blocks, max_features):
        super().__init__()
        self.down_blocks = nn.ModuleList(
            DownBlock3d(in_features if i == 0 else min(max_features, block_expansion * (2 ** i)), min(max_features, block_expansion * (2 ** (i + 1))))
            for i in range(num_blocks))


class Decoder(nn.Module):
    def __init__(self, block_expansion, in_features, num_blocks, max_features):
        super().__init__()
        self.up_blocks = nn.ModuleList(
            UpBlock3d((1 if i == num_blocks - 1 else 2) * min(max_features, block_expansion * (2 ** (i + 1))), min(max_features, block_expansion * (2 ** i)))
            for i in range(num_blocks)[::-1])
        self.out_filters = block_expansion + in_features
        self.conv = nn.Conv3d(self.out_filters, self.out_filters, kernel_size=3, padding=1)
        self.norm = nn.BatchNorm3d(self.out_filters, affine=True)


class Hourglass(nn.Module):
    def __init__(self, block_expansion, in_features, num_blocks=3, max_features=256):
        super().__init__()
        self.encoder = Encoder(block_expansion, in_features, num_blocks, max_features)
        self.decoder = Decoder(block_expansion, in_features, num_blocks, max_features)
        self.out_filters = self.decoder.out_filters


class _NativeWarp(_Native):
    def _bufset(self, key, device):
        """new(tag, *shape, zero=False): the cached fp32 buffer of the key's working set; zero / one: allocated as zeros (a buffer
        whose pad channels are never written keeps them) / ones."""
        ws = self._e4s_bufs.setdefault(key + (str(device),), {})

        def new(tag, *shape, zero=False, one=False):
            k = (tag,) + tuple(shape)
            if k not in ws:
                ws[k] = (torch.zeros if zero else torch.ones if one else torch.empty)(*shape, device=device, dtype=torch.float32)
            return ws[k]
        return new

    def _cached(self, name, tensors, make):
        """make() cached per version of `tensors` and precision."""
        return packs.cached(self, name, tensors, make, (K.sr_f32(),))

    def _conv3dx(self, name, conv, bn, x, y, cin_pad=None, **kw):
        w, b = self._folded(name, conv, bn, lambda w, f32: K.conv3dx_pack(w, f32, cin_pad))
        return K.conv3dx(x, w, conv.out_channels, y, bias=b, **kw)


def _kp_batch(kp_source, kp_driving, num_kp, what):
    """(source value [1,K,3], source jacobian | None, driving value [N,K,3], driving jacobian | None) from the dicts of
    PoseFrontEnd.keypoints: kp_driving a list of dicts or one batched dict."""
    if isinstance(kp_driving, dict):
        kp_driving = [kp_driving]
    if not kp_driving:
        raise ValueError(f"{what}: no driving keypoints")
    dv = torch.cat([k["value"] for k in kp_driving]).float().contiguous()
    sv = kp_source["value"].float().contiguous()
    if dv.dim() != 3 or tuple(dv.shape[1:]) != (num_kp, 3) or sv.shape[0] not in (1, dv.shape[0]) or tuple(sv.shape[1:]) != (num_kp, 3):
        raise ValueError(f"{what}: keypoint values [1|N,{num_kp},3] and [N,{num_kp},3], got {tuple(sv.shape)} and {tuple(dv.shape)}")
    has = [k.get("jacobian") is not None for k in kp_driving]
    if any(has) != all(has):
        raise ValueError(f"{what}: some driving keypoints carry a jacobian and some do not")
    sj = dj = None
    if all(has):
        if kp_source.get("jacobian") is None:
            raise ValueError(f"{what}: kp_driving carries jacobians, kp_source does not")
        dj = torch.cat([k["jacobian"] for k in kp_driving]).float().contiguous()
        sj = kp_source["jacobian"].float().contiguous()
    return sv, sj, dv, dj


class DenseMotionNetwork(_NativeWarp):
    """dense_motion.py:9-128.  run(feature volume [1,D,H,W,C], kp_source, kp_driving) -> {'mask' [N,K+1,D,H,W] (a view),
    'deformation' [N,D,H,W,3], 'occlusion_map' [N,1,H,W] (with estimate_occlusion_map)}: fresh tensors."""

    def __init__(self, block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress,
                 estimate_occlusion_map=False):
        super().__init__()
        self.hourglass = Hourglass(block_expansion=block_expansion, in_features=(num_kp + 1) * (compress + 1), max_features=max_features,
                                   num_blocks=num_blocks)
        self.mask = nn.Conv3d(self.hourglass.out_filters, num_kp + 1, kernel_size=7, padding=3)
        self.compress = nn.Conv3d(feature_channel, compress, kernel_size=1)
        self.norm = nn.BatchNorm3d(compress, affine=True)
        self.occlusion = nn.Conv2d(self.hourglass.out_filters * reshape_depth, 1, kernel_size=7, padding=3) if estimate_occlusion_map else None
        self.num_kp, self.num_blocks, self.reshape_depth = num_kp, num_blocks, reshape_depth
        if compress != 4:
            raise NotImplementedError(f"DenseMotionNetwork: the native sparse warp takes compress = 4 channels, got {compress}")
        if num_kp + 1 > 32:
            raise NotImplementedError(f"DenseMotionNetwork: at most 31 keypoints, got {num_kp}")
        if num_blocks < 1 or block_expansion % 32 or max_features % 32 or feature_channel % 32 or block_expansion < 32 or feature_channel < 32:
            raise NotImplementedError("DenseMotionNetwork: block_expansion, max_features and feature_channel of 32 k and one or more blocks")
        self.layout = hourglass_layout(block_expansion, (num_kp + 1) * (compress + 1), num_blocks, max_features)
        self._init_native()

    def compress_volume(self, vol, out=None):
        """The feature volume [1,D,H,W,C] (any strides) -> relu(norm(compress(.))) [1,D,H,W,4], a fresh tensor unless out is given."""
        self._require_weights()
        b, d, h, w, _ = vol.shape
        out = torch.empty(b, d, h, w, self.compress.out_channels, device=vol.device) if out is None else out
        return self._conv3dx("compress", self.compress, self.norm, vol, out, relu=True)

    def _occlusion_pack(self):
        return self._cached("occlusion", [self.occlusion.weight, self.occlusion.bias],
                            lambda: (K.occlusion_pack(self.occlusion.weight.detach().float(), self.reshape_depth), self.occlusion.bias.detach().float().contiguous()))

    @torch.no_grad()
    def run_compressed(self, comp, sv, sj, dv, dj, taps=None):
        """comp: compress_volume's [1,D,H,W,4]; keypoints as _kp_batch returns them -> (mask [N,D,H,W,K+1], deformation [N,D,H,W,3],
        occlusion [N,H,W] | None), fresh tensors."""
        self._require_weights()
        n, (_, d, h, w, _) = dv.shape[0], comp.shape
        if self.occlusion is not None and d != self.reshape_depth:
            raise ValueError(f"DenseMotionNetwork: a volume of depth {d}, reshape_depth {self.reshape_depth}")
        dev, hg, lay, nb = comp.device, self.hourglass, self.layout, self.num_blocks
        sizes = hourglass_map_sizes(h, w, nb)
        new = self._bufset((n, d, h, w), dev)

        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t
        jac = K.kp_jacobian(sj, dj, new("jac", n, self.num_kp, 3, 3)) if dj is not None else None
        cat = [new(f"cat{i}", n, d, *sizes[i], lv["stride"], zero=True) for i, lv in enumerate(lay["levels"])]
        l0 = lay["levels"][0]
        K.sparse_warp(comp, sv, dv, jac, cat[0], y_coff=l0["up"])
        tap("hg_input", cat[0][..., l0["up"]:l0["up"] + l0["skip"]])
        # encoder: block i reads the skip slice of level i; its pooled output IS the skip slice of level i + 1
        bottom = None
        for i, blk in enumerate(hg.encoder.down_blocks):
            lv, c = lay["levels"][i], blk.conv.out_channels
            x = cat[i][..., lv["up"]:lv["up"] + lv["skip_read"]]
            y = self._conv3dx(f"enc{i}", blk.conv, blk.norm, x, new(f"enc{i}", n, d, *sizes[i], c), cin_pad=lv["skip_read"], relu=True)
            hh, ww = sizes[i + 1]
            if i + 1 < nb:
                dst, off = cat[i + 1], lay["levels"][i + 1]["up"]
            else:
                dst, off = new("bottom", n, d, hh, ww, c), 0
                bottom = dst
            K.avgpool2_into(y.view(n * d, *sizes[i], c), c, dst.view(n * d, hh, ww, dst.shape[4]), off)
            tap(f"enc{i}", dst[..., off:off + c])
        # decoder: up block j writes the first channels of level nb - 1 - j
        x = bottom
        for j, blk in enumerate(hg.decoder.up_blocks):
            i = nb - 1 - j
            self._conv3dx(f"dec{j}", blk.conv, blk.norm, x, cat[i], relu=True, up2=True)
            tap(f"dec{j}", cat[i][..., :blk.conv.out_channels])
            x = cat[i]
        cf = hg.out_filters
        pred = self._conv3dx("dec.conv", hg.decoder.conv, hg.decoder.norm, cat[0], new("pred", n, d, h, w, pad32(cf), zero=True),
                             cin_pad=l0["stride"], relu=True)
        tap("prediction", pred[..., :cf])
        logits = tap("logits", self._conv3dx("mask", self.mask, None, pred, new("logits", n, d, h, w, self.num_kp + 1), cin_pad=pad32(cf)))
        mask, deformation = K.motion_combine(logits, sv, dv, jac)
        occ = None
        if self.occlusion is not None:
            wp, bias = self._occlusion_pack()
            occ = K.occlusion(pred, cf, wp, bias)
        return mask, deformation, occ

    def run(self, feature, kp_source, kp_driving, taps=None):
        sv, sj, dv, dj = _kp_batch(kp_source, kp_driving, self.num_kp, "DenseMotionNetwork.run")
        K._vol(feature, "DenseMotionNetwork.run: feature")
        if feature.shape[0] != 1:
            raise NotImplementedError("DenseMotionNetwork.run: ONE source volume [1,D,H,W,C], broadcast over the driving keypoints")
        comp = self.compress_volume(feature)
        if taps is not None:
            taps["compressed"] = comp
        mask, deformation, occ = self.run_compressed(comp, sv, sj, dv, dj, taps)
        out = {"mask": mask.permute(0, 4, 1, 2, 3), "deformation": deformation}
        if occ is not None:
            out["occlusion_map"] = occ.unsqueeze(1)
        return out


class SourceFeatures(object):
    """encode_source's handle: volume [1,D,h,w,C] (the ResBlock3d stack's output) and compressed [1,D,h,w,4], fresh tensors of the
    weights and the precision they were computed with."""

    def __init__(self, volume, compressed):
        self.volume, self.compressed = volume, compressed


class FeatureWarp(_NativeWarp):
    """generator.py:162-246: OcclusionAwareSPADEGenerator without its SPADE decoder.  encode_source(frame) -> SourceFeatures;
    run(frame or SourceFeatures, kp_source, kp_driving) -> {'mask', 'deformation', 'occlusion_map', 'feature'}."""

    def __init__(self, image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, reshape_depth,
                 num_resblocks, estimate_occlusion_map=False, dense_motion_params=None, estimate_jacobian=False):
        super().__init__()
        if dense_motion_params is None:
            raise NotImplementedError("FeatureWarp: a generator without a dense motion network has nothing to warp (dense_motion_params)")
        if image_channel != 3:
            raise NotImplementedError("FeatureWarp: the native encoder takes 3-channel frames")
        self.dense_motion_network = DenseMotionNetwork(num_kp=num_kp, feature_channel=feature_channel,
                                                       estimate_occlusion_map=estimate_occlusion_map, **dense_motion_params)
        self.first = SameBlock2d(image_channel, block_expansion)
        out_features = block_expansion
        blocks = []
        for i in range(num_down_blocks):
            in_features, out_features = min(max_features, block_expansion * (2 ** i)), min(max_features, block_expansion * (2 ** (i + 1)))
            blocks.append(DownBlock2d(in_features, out_features, kernel_size=(3, 3), padding=(1, 1)))
        self.down_blocks = nn.ModuleList(blocks)
        self.second = nn.Conv2d(out_features, max_features, kernel_size=1, stride=1)
        self.reshape_channel, self.reshape_depth = reshape_channel, reshape_depth
        self.resblocks_3d = nn.Sequential()
        for i in range(num_resblocks):
            self.resblocks_3d.add_module("3dr" + str(i), ResBlock3d(reshape_channel))
        out_features = block_expansion * (2 ** num_down_blocks)
        self.third = SameBlock2d(max_features, out_features)
        self.fourth = nn.Conv2d(out_features, out_features, kernel_size=1, stride=1)
        self.estimate_occlusion_map, self.image_channel, self.num_kp = estimate_occlusion_map, image_channel, num_kp
        if reshape_channel * reshape_depth != max_features:
            raise ValueError("FeatureWarp: reshape_channel x reshape_depth must equal max_features (the .view of `second`'s output)")
        if reshape_channel != feature_channel or dense_motion_params.get("reshape_depth", reshape_depth) != reshape_depth:
            raise ValueError("FeatureWarp: the dense motion network's feature_channel / reshape_depth differ from the generator's")
        if block_expansion % 32 or block_expansion < 32 or max_features % 64 or out_features % 64 or reshape_channel % 32 or num_down_blocks < 1 \
                or any(b.conv.out_channels % 64 for b in blocks):
            raise NotImplementedError("FeatureWarp: block_expansion and reshape_channel of 32 k; max_features and every 2-D block past `first` of 64 j channels")
        self._second_perm = reshape_permutation(max_features, reshape_depth)
        self._third_perm = third_input_permutation(reshape_channel, reshape_depth)
        self._init_native()

    def load_generator_state_dict(self, state_dict):
        """Load a checkpoint's ['generator'] entry (OcclusionAwareSPADEGenerator.state_dict()).  Every key outside `decoder.` must
        match this module's tree exactly (a missing or an unexpected one raises, as strict=True does); the `decoder.*` entries -- the
        SPADE decoder, which is not part of this module -- are ignored."""
        return self.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("decoder.")}, strict=True)

    def load_state_dict(self, state_dict, strict=True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self.dense_motion_network._weights_loaded = True                        # its entries came with this module's
        return res

    def _bn_affine(self, name, bn):
        def make():
            s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            return s.float().contiguous(), (bn.bias.double() - bn.running_mean.double() * s).float().contiguous()
        return self._cached(name, [bn.weight, bn.bias, bn.running_mean, bn.running_var], make)

    @torch.no_grad()
    def encode_source(self, frame, taps=None):
        """One source frame [H,W,3] or [1,H,W,3] (float in [0,1] or uint8; a device tensor) -> SourceFeatures."""
        self._require_weights()
        f = _device_frames(frame, "FeatureWarp.encode_source")
        if f.shape[0] != 1:
            raise ValueError("FeatureWarp.encode_source: one source frame")
        _, h, w, _ = f.shape
        dev = f.device
        new = self._bufset(("enc", h, w), dev)

        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t
        if f.dtype == torch.uint8:
            f = K.aa_down(f, new("one", 1, one=True), 1, out=new("x0", 1, h, w, 3))
        sizes = encoder_map_sizes(h, w, len(self.down_blocks))
        x = tap("first", self._smallcin("first", self.first.conv, self.first.norm, f, new("first", 1, h, w, self.first.conv.out_channels)))
        for i, blk in enumerate(self.down_blocks):
            c = blk.conv.out_channels
            y = self._rconv(f"down{i}", blk.conv, blk.norm, x, new(f"down{i}.c", 1, *sizes[i], c), act=True)
            x = tap(f"down{i}", K.avgpool2(y, new(f"down{i}", 1, *sizes[i + 1], c)))
        hh, ww = sizes[-1]
        d, c3, nres = self.reshape_depth, self.reshape_channel, len(self.resblocks_3d)
        flat = new("second", 1, hh, ww, d * c3) if nres else torch.empty(1, hh, ww, d * c3, device=dev)
        self._rconv("second", self.second, None, x, flat, perm=self._second_perm)
        vol = tap("second", flat.view(1, hh, ww, d, c3).permute(0, 3, 1, 2, 4))          # [1,D,h,w,C]: no copy
        for i, blk in enumerate(self.resblocks_3d):
            s, t = self._bn_affine(f"res{i}.norm1", blk.norm1)
            a = K.bnrelu3d(vol, s, t, new("res.a", 1, d, hh, ww, c3))
            b = self._conv3dx(f"res{i}.1", blk.conv1, blk.norm2, a, new("res.b", 1, d, hh, ww, c3), relu=True)
            out = torch.empty(1, d, hh, ww, c3, device=dev) if i == nres - 1 else new(f"res.o{i & 1}", 1, d, hh, ww, c3)
            vol = tap(f"res{i}", self._conv3dx(f"res{i}.2", blk.conv2, None, b, out, res=vol))
        comp = tap("compressed", self.dense_motion_network.compress_volume(vol))
        return SourceFeatures(vol, comp)

    @torch.no_grad()
    def run(self, source, kp_source, kp_driving, taps=None):
        """source: a frame or encode_source's handle; kp_source: {'value' [1,K,3], 'jacobian' [1,K,3,3] | None}; kp_driving: a list of
        such dicts (PoseFrontEnd.keypoints) or one batched dict of N.  -> fresh tensors {'mask' [N,K+1,D,h,w] (a view), 'deformation'
        [N,D,h,w,3], 'occlusion_map' [N,1,h,w] (when estimated), 'feature' [N,C,h,w] (a channels-last view): the decoder's input}."""
        self._require_weights()
        src = source if isinstance(source, SourceFeatures) else self.encode_source(source, taps)
        dm = self.dense_motion_network
        sv, sj, dv, dj = _kp_batch(kp_source, kp_driving, self.num_kp, "FeatureWarp.run")
        if sv.device != src.volume.device or dv.device != src.volume.device:
            raise RuntimeError("FeatureWarp.run: the keypoints are on another device than the source features")
        mask, deformation, occ = dm.run_compressed(src.compressed, sv, sj, dv, dj, taps)
        n, (_, d, h, w, c) = dv.shape[0], src.volume.shape
        new = self._bufset(("run", n, d, h, w), src.volume.device)

        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t
        warped = tap("warped", K.warp3d(src.volume, deformation, new("warped", n, h, w, d * c)))
        tc = self.third.conv
        w3, b3 = self._folded("third", tc, self.third.norm, lambda wt, f32: K.rconv_pack(wt[:, self._third_perm.to(wt.device)].contiguous(), f32))
        t3 = tap("third", K.rconv(warped, tc.in_channels, w3, tc.out_channels, 3, new("third", n, h, w, tc.out_channels), bias=b3, act=True, slope=0.01))
        feat = self._rconv("fourth", self.fourth, None, t3, torch.empty(n, h, w, self.fourth.out_channels, device=t3.device))
        out = {"mask": mask.permute(0, 4, 1, 2, 3), "deformation": deformation}
        if occ is not None:
            K.scale_rows(feat, occ)
            out["occlusion_map"] = occ.unsqueeze(1)
        out["feature"] = feat.permute(0, 3, 1, 2)
        return out


class ReenactWarp(object):
    """PoseFrontEnd then FeatureWarp: frames in, the SPADE decoder's input out."""

    def __init__(self, front_end, feature_warp):
        if not isinstance(front_end, PoseFrontEnd) or not isinstance(feature_warp, FeatureWarp):
            raise TypeError("ReenactWarp: a PoseFrontEnd and a FeatureWarp")
        if front_end.kp_detector.kp.out_channels != feature_warp.num_kp:
            raise ValueError("ReenactWarp: the front end and the generator disagree on num_kp")
        self.front_end, self.feature_warp = front_end, feature_warp

    def run(self, source, driving, **free_view):
        """source [H,W,3], driving a list of frames or [N,H,W,3] (numpy or tensors); free_view, yaw, pitch, roll as
        PoseFrontEnd.keypoints -> FeatureWarp.run's dict for the N driving frames."""
        dev = self.front_end.device
        src = _frames(source, dev, "ReenactWarp.run")
        kp_source, kp_driving = self.front_end.keypoints_device(src, _frames(driving, dev, "ReenactWarp.run"), **free_view)
        return self.feature_warp.run(src, kp_source, kp_driving)
