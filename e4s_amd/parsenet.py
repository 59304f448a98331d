"""GPEN's face parser ParseNet (src/pretrained/gpen/face_parse/) -- MI355X-native.  A restored 512^2 face -> its uint8 soft-mask seed.

FaceEnhancement.process (face_enhancement.py:89) runs `FaceParse.process` on every restored face and blends the face into the frame
through the mask it returns.  Here that is `FaceParse.process(im)` (the reference's signature) or `FaceParse.masks(faces_u8)` on a
device batch.

Module tree / state_dict identical to the reference (blocks.py, parse_model.py), so `ParseNet-latest.pth` loads with strict=True.
The modules hold parameters only; execution is on NHWC buffers with csrc/parsenet.hip:

    reference                                           here
    --------------------------------------------------  ------------------------------------------------------------------
    img[..., ::-1] / 255 * 2 - 1, encoder[0]            e4s_parsenet_head_f32 (uint8 HWC in, one pass)
    ReflectionPad2d(1) + Conv2d(3x3, stride 1 or 2)     e4s_pconv_f32: the reflect map is part of the halo staging
    nn.functional.interpolate(nearest, 2) + pad + conv  e4s_pconv_f32(up2): neither the 4x nor the padded map is written
    BatchNorm2d (eval) behind a conv                    folded into the conv's weights and bias on the host (fold_conv_bn)
    LeakyReLU(0.2)                                      the conv's epilogue
    identity + res                                      conv2's epilogue (+ r0)
    feat + body(feat)                                   the last body block's conv2 epilogue (+ r1)
    out_mask_conv, argmax, MASK_COLORMAP                e4s_parsenet_tail_f32 (one pass; out_img_conv is never used and never run)

Arithmetic follows kernels.PRECISION: "f32" runs the exact fp32 MFMA, "bf16x3" and "auto" the split-bf16 path (three bf16 MFMAs per
product, fp32 accumulate).  Folded weights are re-packed once per weight version and precision (cached on each ConvLayer).  The
working set belongs to the ParseNet, one set per input shape; after the first call at a shape nothing is allocated but the results.
There is no CPU path.  Only norm_type 'bn' / 'none' and relu_type 'LeakyReLU' / 'none' are provided."""
import os

import numpy as np
import torch
from torch import nn

from . import kernels as K
from .face_parser import fold_conv_bn
from . import packs

MASK_COLORMAP = [0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 255, 255, 255, 0]    # face_parsing.py:30


class NormLayer(nn.Module):
    """blocks.py:9-38 for norm_type 'bn' and 'none'."""

    def __init__(self, channels, normalize_shape=None, norm_type="bn", ref_channels=None):
        super().__init__()
        norm_type = norm_type.lower()
        self.norm_type = norm_type
        if norm_type == "bn":
            self.norm = nn.BatchNorm2d(channels, affine=True)
        elif norm_type != "none":
            raise NotImplementedError(f"NormLayer(norm_type={norm_type!r}): the native ParseNet knows 'bn' and 'none'")


class ReluLayer(nn.Module):
    """blocks.py:41-70 for relu_type 'LeakyReLU' (slope 0.2) and 'none'."""

    def __init__(self, channels, relu_type="relu"):
        super().__init__()
        relu_type = relu_type.lower()
        if relu_type not in ("leakyrelu", "none"):
            raise NotImplementedError(f"ReluLayer(relu_type={relu_type!r}): the native ParseNet knows 'LeakyReLU' and 'none'")
        self.relu_type = relu_type


class ConvLayer(nn.Module):
    """blocks.py:73-102: [nearest x2] + ReflectionPad2d(1) + Conv2d(3x3, stride 2 for scale 'down') + norm + relu."""

    def __init__(self, in_channels, out_channels, kernel_size=3, scale="none", norm_type="none", relu_type="none", use_pad=True, bias=True):
        super().__init__()
        if kernel_size != 3 or not use_pad:
            raise NotImplementedError("ConvLayer: the native kernels are reflect-padded 3x3 convs")
        self.norm_type = norm_type
        if norm_type in ["bn"]:
            bias = False
        self.scale = scale
        self.stride = 2 if scale == "down" else 1
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, self.stride, bias=bias)
        self.relu = ReluLayer(out_channels, relu_type)
        self.norm = NormLayer(out_channels, norm_type=norm_type)

    def folded(self):
        """(weight, bias) of the layer as ONE conv: eval-mode BatchNorm folded in (fp64 on the host); bias may be None."""
        w = self.conv2d.weight.detach().float()
        if self.norm.norm_type == "bn":
            return fold_conv_bn(w, self.norm.norm)
        return w, (self.conv2d.bias.detach().float() if self.conv2d.bias is not None else None)

    def _tensors(self):
        t = [self.conv2d.weight] + ([self.conv2d.bias] if self.conv2d.bias is not None else [])
        if self.norm.norm_type == "bn":
            bn = self.norm.norm
            t += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return t

    def packed(self):
        """(weights packed for e4s_pconv_f32 in the current precision, bias or None), cached on the layer."""
        f32 = K.sr_f32()

        def build():
            w, b = self.folded()
            return K.pconv_pack(w.contiguous(), f32), b.contiguous() if b is not None else None
        return packs.cached(self, "pconv", self._tensors(), build, (f32,))

    def run(self, x, y, r0=None, r1=None):
        """The layer on NHWC buffers: x [B,H,W,Cin] -> y [B,Ho,Wo,Cout] (+ r0, + r1 after the activation)."""
        w, b = self.packed()
        return K.pconv(x, self.conv2d.in_channels, w, self.conv2d.out_channels, y, bias=b, lrelu=self.relu.relu_type == "leakyrelu",
                       r0=r0, r1=r1, stride=self.stride, up2=self.scale == "up")


class ResidualBlock(nn.Module):
    """blocks.py:105-128"""

    def __init__(self, c_in, c_out, relu_type="prelu", norm_type="bn", scale="none"):
        super().__init__()
        if scale == "none" and c_in == c_out:
            self.shortcut_func = None                                            # the reference's `lambda x: x` (no module either)
        else:
            self.shortcut_func = ConvLayer(c_in, c_out, 3, scale)
        scale_conf = {"down": ["none", "down"], "up": ["up", "none"], "none": ["none", "none"]}[scale]
        self.scale, self.c_out = scale, c_out
        self.conv1 = ConvLayer(c_in, c_out, 3, scale_conf[0], norm_type=norm_type, relu_type=relu_type)
        self.conv2 = ConvLayer(c_out, c_out, 3, scale_conf[1], norm_type=norm_type, relu_type="none")

    def run(self, x, new, extra=None):
        """identity + conv2(conv1(x)) [+ extra] on NHWC buffers; new(tag, h, w, c) hands out this block's buffers."""
        b, h, w, _ = x.shape
        up = self.scale == "up"
        h1, w1 = K.pconv_out_size(h, 1, up), K.pconv_out_size(w, 1, up)
        ho, wo = K.pconv_out_size(h1, self.conv2.stride), K.pconv_out_size(w1, self.conv2.stride)
        identity = x if self.shortcut_func is None else self.shortcut_func.run(x, new("sc", ho, wo, self.c_out))
        t = self.conv1.run(x, new("t", h1, w1, self.c_out))
        return self.conv2.run(t, new("y", ho, wo, self.c_out), r0=identity, r1=extra)


class ParseNet(nn.Module):
    """parse_model.py:21-86"""

    def __init__(self, in_size=128, out_size=128, min_feat_size=32, base_ch=64, parsing_ch=19, res_depth=10, relu_type="prelu",
                 norm_type="bn", ch_range=[32, 512]):
        super().__init__()
        if parsing_ch != 19:
            raise NotImplementedError("ParseNet: the native tail is the 19-class mask conv")
        if res_depth < 1:
            raise NotImplementedError("ParseNet: res_depth >= 1 (feat + body(feat) is the last body block's epilogue)")
        self.res_depth = res_depth
        act_args = {"norm_type": norm_type, "relu_type": relu_type}
        min_ch, max_ch = ch_range

        def ch_clip(x):
            return max(min_ch, min(x, max_ch))

        min_feat_size = min(in_size, min_feat_size)
        down_steps = int(np.log2(in_size // min_feat_size))
        up_steps = int(np.log2(out_size // min_feat_size))
        encoder = [ConvLayer(3, base_ch, 3, 1)]
        head_ch = base_ch
        for _ in range(down_steps):
            encoder.append(ResidualBlock(ch_clip(head_ch), ch_clip(head_ch * 2), scale="down", **act_args))
            head_ch = head_ch * 2
        body = [ResidualBlock(ch_clip(head_ch), ch_clip(head_ch), **act_args) for _ in range(res_depth)]
        decoder = []
        for _ in range(up_steps):
            decoder.append(ResidualBlock(ch_clip(head_ch), ch_clip(head_ch // 2), scale="up", **act_args))
            head_ch = head_ch // 2
        self.encoder = nn.Sequential(*encoder)
        self.body = nn.Sequential(*body)
        self.decoder = nn.Sequential(*decoder)
        self.out_img_conv = ConvLayer(ch_clip(head_ch), 3)                        # in the state_dict; FaceParse never uses its output
        self.out_mask_conv = ConvLayer(ch_clip(head_ch), parsing_ch)
        self._e4s_bufs = {}

    def release_workspace(self):
        """Drop every cached buffer set (a captured graph that used one keeps it alive)."""
        self._e4s_bufs = {}

    def _small(self):
        """Head [27][Cout] ((ky, kx, ci)-major) and tail [9][Cin][20] (class-minor, zero-padded) weights: layout only, cached."""
        head, tail = self.encoder[0].conv2d, self.out_mask_conv.conv2d

        def build():
            hw = head.weight.detach().float().permute(2, 3, 1, 0).reshape(27, head.out_channels).contiguous()
            tw = tail.weight.detach().float().permute(2, 3, 1, 0).reshape(9, tail.in_channels, 19)
            return hw, nn.functional.pad(tw, (0, 1)).contiguous()
        return packs.cached(self, "small", (head.weight, tail.weight), build)

    def features_nhwc(self, src, flip=False, taps=None):
        """Everything before out_mask_conv: src uint8 NHWC [B,H,W,3] or fp32 NCHW [B,3,H,W] -> NHWC [B,H',W',C].  taps: a dict that
        receives named intermediate buffers ('head', 'enc<i>', 'body<i>', 'trunk', 'dec<i>'; valid until the next call)."""
        if not src.is_cuda:
            raise RuntimeError("ParseNet runs on the ROCm device only (no CPU path)")
        u8 = src.dtype == torch.uint8
        if src.dim() != 4 or (src.shape[3] if u8 else src.shape[1]) != 3 or not (u8 or src.dtype == torch.float32):
            raise ValueError(f"ParseNet: uint8 NHWC [B,H,W,3] or fp32 NCHW [B,3,H,W] images, got {tuple(src.shape)} {src.dtype}")
        bsz, h, w = (src.shape[0], src.shape[1], src.shape[2]) if u8 else (src.shape[0], src.shape[2], src.shape[3])
        ws = self._e4s_bufs.setdefault((bsz, h, w, str(src.device)), {})

        def scope(name):
            def new(tag, hh, ww, c):
                k = f"{name}.{tag}"
                if k not in ws:
                    ws[k] = torch.empty(bsz, hh, ww, c, device=src.device, dtype=torch.float32)
                return ws[k]
            return new

        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t

        hw, _ = self._small()
        head = self.encoder[0]
        x = tap("head", K.parsenet_head(src.contiguous(), hw, head.conv2d.bias.detach(), scope("head")("y", h, w, head.conv2d.out_channels),
                                        flip=flip))
        for i, block in enumerate(list(self.encoder)[1:]):
            x = tap(f"enc{i}", block.run(x, scope(f"enc{i}")))
        feat = x
        for i, block in enumerate(self.body):
            last = i == len(self.body) - 1
            x = tap("trunk" if last else f"body{i}", block.run(x, scope(f"body{i}"), extra=feat if last else None))
        for i, block in enumerate(self.decoder):
            x = tap(f"dec{i}", block.run(x, scope(f"dec{i}")))
        return x

    def _tail(self, x, **kw):
        _, tw = self._small()
        return K.parsenet_tail(x, self.out_mask_conv.conv2d.in_channels, tw, self.out_mask_conv.conv2d.bias.detach(), **kw)

    @torch.no_grad()
    def forward(self, x):
        """fp32 NCHW [B,3,H,W] on the device -> the mask logits fp32 NCHW [B,19,H,W] (the reference's out_mask; out_img is not
        computed)."""
        return self._tail(self.features_nhwc(x), mask=False, logits=True)[2]

    @torch.no_grad()
    def masks_u8(self, images, bgr=False, logits=False):
        """uint8 NHWC [B,H,W,3] -> uint8 [B,H,W] of MASK_COLORMAP[argmax] (and the logits [B,19,H,W] when asked for)."""
        m, _, lg = self._tail(self.features_nhwc(images, flip=bgr), mask=True, logits=logits)
        return (m, lg) if logits else m


class FaceParse(object):
    """face_parsing.py:13-47.  base_dir given: loads base_dir/weights/<model>.pth; base_dir None: refused unless
    E4S_ALLOW_UNINITIALIZED_LOSS_NETS=1 (load your own state dict into .faceparse afterwards)."""

    def __init__(self, base_dir="./", model="ParseNet-latest", device="cuda"):
        from .criteria import _have_weights
        self.mfile = os.path.join(base_dir, "weights", model + ".pth") if base_dir is not None else None
        self.size = 512
        self.device = device
        self.MASK_COLORMAP = list(MASK_COLORMAP)
        self.faceparse = ParseNet(self.size, self.size, 32, 64, 19, norm_type="bn", relu_type="LeakyReLU", ch_range=[32, 256])
        if _have_weights("FaceParse (the GPEN checkpoint weights/ParseNet-latest.pth)", self.mfile):
            self.faceparse.load_state_dict(torch.load(self.mfile, map_location=torch.device("cpu")), strict=True)
        for p in self.faceparse.parameters():
            p.requires_grad = False
        self.faceparse.to(self.device)
        self.faceparse.eval()

    def masks(self, faces_u8, bgr=True):
        """Device uint8 [B,512,512,3] -> device uint8 [B,512,512] of 0 / 255.  Stream-ordered, no host synchronisation; the working
        set is allocated on the first call at a batch size (capture it in a torch.cuda.graph after one warm-up call)."""
        if faces_u8.dim() != 4 or faces_u8.dtype != torch.uint8 or tuple(faces_u8.shape[1:]) != (self.size, self.size, 3):
            raise ValueError(f"FaceParse.masks: uint8 [B,{self.size},{self.size},3] faces, got {tuple(faces_u8.shape)} {faces_u8.dtype} "
                             "(the reference's cv2.resize is the identity at this size only; resize before)")
        if not faces_u8.is_cuda:
            raise RuntimeError("FaceParse runs on the ROCm device only (no CPU path)")
        return self.faceparse.masks_u8(faces_u8.contiguous(), bgr=bgr)

    def process(self, im):
        """The reference's call: numpy HWC BGR uint8 512 x 512 -> [uint8 mask 512 x 512]."""
        arr = np.asarray(im)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("FaceParse.process: an HWC BGR uint8 array")
        t = torch.from_numpy(np.ascontiguousarray(arr))[None].to(self.device)
        return [m for m in self.masks(t, bgr=True).cpu().numpy()]

    def process_tensor(self, imt):
        raise NotImplementedError("FaceParse.process_tensor is not provided (face_enhancement.py never calls it)")
