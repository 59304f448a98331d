"""GPEN's face detector RetinaFace-R50 (src/pretrained/gpen/face_detect/) -- MI355X-native.  A frame -> boxes and five landmarks.

FaceEnhancement.process (face_enhancement.py:68) sends every non-aligned frame through `RetinaFaceDetection.detect` first.  Here that
is `RetinaFaceDetection.detect(img_raw, ...)` (the reference's signature and return) or `detect_device(frames_u8)` on device frames.

Module tree / state_dict identical to the reference `RetinaFace(cfg_re50)` (facemodels/retinaface.py, net.py; the backbone is
torchvision's ResNet-50 v1.5 up to layer4, no fc), so `RetinaFace-R50.pth` loads with strict=True.  The modules hold parameters only;
execution is on NHWC buffers with csrc/retinaface.hip:

    reference                                               here
    ------------------------------------------------------  ------------------------------------------------------------------
    np.float32(img), cv2.resize for max(H, W) > 1500,       e4s_retina_prep_f32 (uint8 BGR HWC in, one pass; the shrink restated as
      img -= (104, 117, 123)                                  half-pixel bilinear, dsize = round(src * ss): not pinned to cv2)
    conv1 7x7 / 2 + bn1 + relu, maxpool 3 / 2               e4s_conv_smallcin_f32, e4s_maxpool3s2p1_f32 (both bounds-checked per tap)
    every other Conv2d + BatchNorm2d (eval) [+ ReLU]        e4s_rconv_f32, BatchNorm folded on the host (face_parser.fold_conv_bn)
    relu(out + identity) of a Bottleneck                    conv3's epilogue (+ r0, then ReLU)
    lateral + F.interpolate(up, size, "nearest")            the lateral conv's epilogue (ReLU, then + r0 read through the upsampling)
    F.relu(torch.cat([conv3X3, conv5X5, conv7X7], 1))       each branch's epilogue writes its ReLU at its channel offset of one buffer
    Class / Bbox / LandmarkHead, softmax, PriorBox,         e4s_retina_head_f32 per level (no prior table)
      decode, decode_landm, * scale / resize
    scores > thr, argsort()[::-1][:top_k], py_cpu_nms,      torch.sort (stable, descending) + e4s_retina_select_f32
      [:keep_top_k], landmark re-layout, / ss

Ties: the reference orders equal scores by numpy's argsort()[::-1], which leaves their order unspecified; here equal scores keep the
lower prior index first.  Arithmetic follows kernels.PRECISION: "f32" runs the exact fp32 MFMA, "bf16x3" and "auto" the split-bf16
path.  Folded weights are re-packed once per weight version and precision; the working set is cached per frame shape, and after the
first call at a shape nothing is allocated but the results.  There is no CPU path.  Only cfg_re50 is provided."""
import os

import numpy as np
import torch
from torch import nn

from . import kernels as K
from .face_parser import fold_conv_bn
from . import packs

cfg_re50 = {                                                                     # data/config.py:23-41 (the fields inference reads)
    "name": "Resnet50", "min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "variance": [0.1, 0.2], "clip": False,
    "pretrain": False, "return_layers": {"layer2": 1, "layer3": 2, "layer4": 3}, "in_channel": 256, "out_channel": 256,
}
MEAN_BGR = (104, 117, 123)


def conv_out_size(n, k, stride):
    """Rows out of a zero-padded (k // 2) k x k conv / pool at `stride`: ceil(n / 2) at stride 2."""
    return (n + 2 * (k // 2) - k) // stride + 1


def feature_sizes(h, w):
    """[(h, w) of the stem, the pool / layer1, layer2, layer3, layer4] for an h x w network input."""
    out = []
    for _ in range(5):
        h, w = conv_out_size(h, 3, 2), conv_out_size(w, 3, 2)                    # 7x7 pad 3 and 3x3 pad 1 at stride 2: the same size
        out.append((h, w))
    return out


def shrink_size(h, w):
    """retinaface_detection.py:65-70: (ss, network-input h, w).  ss = 1 and the frame's size unless max(h, w) > 1500; then ss =
    1000 / max and dsize = round(src * ss) (half to even, as cvRound and Python's round)."""
    if max(h, w) > 1500:
        ss = 1000.0 / max(h, w)
        return ss, int(round(h * ss)), int(round(w * ss))
    return 1.0, h, w


def prior_boxes(h, w, cfg=cfg_re50):
    """The host mirror of the per-cell prior formula of csrc/retinaface.hip (prior_box.py:14-34): float32 [N,4] (cx, cy, w, h), computed
    in float64 and rounded once."""
    rows = []
    for k, step in enumerate(cfg["steps"]):
        fh, fw = -(-h // step), -(-w // step)
        i, j = np.meshgrid(np.arange(fh, dtype=np.float64), np.arange(fw, dtype=np.float64), indexing="ij")
        for_level = []
        for ms in cfg["min_sizes"][k]:
            for_level.append(np.stack([(j + 0.5) * step / w, (i + 0.5) * step / h, np.full_like(i, ms / w), np.full_like(i, ms / h)], -1))
        rows.append(np.stack(for_level, 2).reshape(-1, 4))
    out = np.concatenate(rows).astype(np.float32)
    return np.clip(out, 0, 1) if cfg["clip"] else out


# ---- the reference's parameter tree ---------------------------------------------------------------------------------------------
class Bottleneck(nn.Module):
    """torchvision's ResNet v1.5 bottleneck: the stride sits on the 3x3 conv; downsample = 1x1 conv + BatchNorm."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.stride = stride
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
        else:
            self.downsample = None


class ResNet50Body(nn.Module):
    """IntermediateLayerGetter(resnet50, return_layers): conv1 .. layer4 (avgpool and fc are dropped)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, (planes, blocks, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))):
            layer = [Bottleneck(inplanes, planes, stride, downsample=True)]
            inplanes = planes * 4
            layer += [Bottleneck(inplanes, planes) for _ in range(1, blocks)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))


def _conv_bn(inp, oup, k, stride=1):
    return nn.Sequential(nn.Conv2d(inp, oup, k, stride, k // 2, bias=False), nn.BatchNorm2d(oup))     # net.py:9-27 (the activation has no state)


class FPN(nn.Module):
    """net.py:68-98"""

    def __init__(self, in_channels_list, out_channels):
        super().__init__()
        if out_channels <= 64:
            raise NotImplementedError("FPN: out_channels <= 64 (leaky 0.1) belongs to the MobileNet config, which is not provided")
        self.output1 = _conv_bn(in_channels_list[0], out_channels, 1)
        self.output2 = _conv_bn(in_channels_list[1], out_channels, 1)
        self.output3 = _conv_bn(in_channels_list[2], out_channels, 1)
        self.merge1 = _conv_bn(out_channels, out_channels, 3)
        self.merge2 = _conv_bn(out_channels, out_channels, 3)


class SSH(nn.Module):
    """net.py:40-66"""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        if out_channel <= 64 or out_channel % 4:
            raise NotImplementedError("SSH: out_channel <= 64 (leaky 0.1) belongs to the MobileNet config, which is not provided")
        self.conv3X3 = _conv_bn(in_channel, out_channel // 2, 3)
        self.conv5X5_1 = _conv_bn(in_channel, out_channel // 4, 3)
        self.conv5X5_2 = _conv_bn(out_channel // 4, out_channel // 4, 3)
        self.conv7X7_2 = _conv_bn(out_channel // 4, out_channel // 4, 3)
        self.conv7x7_3 = _conv_bn(out_channel // 4, out_channel // 4, 3)


class _Head(nn.Module):
    def __init__(self, inchannels, num_anchors, per_anchor):
        super().__init__()
        self.num_anchors = num_anchors
        self.conv1x1 = nn.Conv2d(inchannels, num_anchors * per_anchor, kernel_size=(1, 1), stride=1, padding=0)


class ClassHead(_Head):
    def __init__(self, inchannels=512, num_anchors=3):
        super().__init__(inchannels, num_anchors, 2)


class BboxHead(_Head):
    def __init__(self, inchannels=512, num_anchors=3):
        super().__init__(inchannels, num_anchors, 4)


class LandmarkHead(_Head):
    def __init__(self, inchannels=512, num_anchors=3):
        super().__init__(inchannels, num_anchors, 10)


class RetinaFace(nn.Module):
    """facemodels/retinaface.py:48-127 for cfg_re50, phase 'test'."""

    def __init__(self, cfg=None, phase="test"):
        super().__init__()
        cfg = cfg_re50 if cfg is None else cfg
        if cfg.get("name") != "Resnet50":
            raise NotImplementedError(f"RetinaFace(cfg name {cfg.get('name')!r}): the native detector knows cfg_re50 (Resnet50) only; "
                                      "the MobileNet config is not provided")
        if phase != "test":
            raise NotImplementedError("RetinaFace: the native detector is inference only (phase 'test')")
        if cfg["in_channel"] != 256 or cfg["out_channel"] != 256 or cfg["clip"]:
            raise NotImplementedError("RetinaFace: cfg_re50's in_channel = out_channel = 256, clip False")
        self.cfg, self.phase = cfg, phase
        self.body = ResNet50Body()
        c = cfg["in_channel"]
        self.fpn = FPN([c * 2, c * 4, c * 8], cfg["out_channel"])
        self.ssh1 = SSH(cfg["out_channel"], cfg["out_channel"])
        self.ssh2 = SSH(cfg["out_channel"], cfg["out_channel"])
        self.ssh3 = SSH(cfg["out_channel"], cfg["out_channel"])
        self.ClassHead = nn.ModuleList(ClassHead(cfg["out_channel"], 2) for _ in range(3))
        self.BboxHead = nn.ModuleList(BboxHead(cfg["out_channel"], 2) for _ in range(3))
        self.LandmarkHead = nn.ModuleList(LandmarkHead(cfg["out_channel"], 2) for _ in range(3))
        self._e4s_bufs = {}

    def release_workspace(self):
        """Drop every cached buffer set (a captured graph that used one keeps it alive)."""
        self._e4s_bufs = {}

    # -- weights --------------------------------------------------------------------------------------------------------------
    def _unit(self, name, conv, bn):
        """(packed weights, bias) of conv + eval BatchNorm as one conv for e4s_rconv_f32, cached per weight version and precision."""
        f32 = K.sr_f32()

        def build():
            w, b = fold_conv_bn(conv.weight.detach().float(), bn)
            return K.rconv_pack(w.contiguous(), f32), b.contiguous()
        return packs.cached(self, name, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), build, (f32,))

    def _stem(self):
        conv, bn = self.body.conv1, self.body.bn1

        def build():
            w, b = fold_conv_bn(conv.weight.detach().float(), bn)
            return K.pack_smallcin(w), b.contiguous()
        return packs.cached(self, "stem", (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), build)

    def _heads(self, level):
        """wp [256,32], bias [32]: column anchor * 16 + t, t 0..3 loc, 4..5 conf, 6..15 landmarks (layout only)."""
        convs = [self.BboxHead[level].conv1x1, self.ClassHead[level].conv1x1, self.LandmarkHead[level].conv1x1]

        def build():
            ws = [c.weight.detach().float().reshape(2, -1, 256) for c in convs]           # [anchor][per-anchor][256]
            bs = [c.bias.detach().float().reshape(2, -1) for c in convs]
            return torch.cat(ws, 1).reshape(32, 256).t().contiguous(), torch.cat(bs, 1).reshape(32).contiguous()
        return packs.cached(self, f"head{level}", [t for c in convs for t in (c.weight, c.bias)], build)

    # -- execution ------------------------------------------------------------------------------------------------------------
    def _workspace(self, bsz, h, w, device):
        ws = self._e4s_bufs.setdefault((bsz, h, w, str(device)), {})

        def new(tag, *shape, dtype=torch.float32):
            k = (tag,) + tuple(shape)
            if k not in ws:
                ws[k] = torch.empty(bsz, *shape, device=device, dtype=dtype)
            return ws[k]
        return new

    def _cb(self, name, seq_or_pair, x, y, **kw):
        conv, bn = seq_or_pair
        w, b = self._unit(name, conv, bn)
        return K.rconv(x, conv.in_channels, w, conv.out_channels, conv.kernel_size[0], y, bias=b, stride=conv.stride[0], **kw)

    def features_nhwc(self, x0, new, taps=None):
        """The network up to the SSH outputs on the prepared NHWC input x0 [B,H,W,3]: -> [ssh1, ssh2, ssh3] NHWC maps of 256 channels."""
        def tap(name, t):
            if taps is not None:
                taps[name] = t
            return t

        sizes = feature_sizes(x0.shape[1], x0.shape[2])
        wp, bias = self._stem()
        x = tap("stem", K.retina_stem(x0, wp, bias, new("stem", *sizes[0], 64)))
        x = tap("pool", K.retina_pool(x, new("pool", *sizes[1], 64)))
        feats = []
        for li in range(1, 5):
            layer = getattr(self.body, f"layer{li}")
            for bi, blk in enumerate(layer):
                name = f"body.layer{li}.{bi}"
                h, w = x.shape[1], x.shape[2]
                ho, wo = conv_out_size(h, 3, blk.stride), conv_out_size(w, 3, blk.stride)
                planes = blk.conv1.out_channels
                t1 = self._cb(name + ".1", (blk.conv1, blk.bn1), x, new(f"l{li}.t1", h, w, planes), act=True)
                t2 = self._cb(name + ".2", (blk.conv2, blk.bn2), t1, new(f"l{li}.t2", ho, wo, planes), act=True)
                idt = x if blk.downsample is None else self._cb(name + ".ds", tuple(blk.downsample), x, new(f"l{li}.ds", ho, wo, planes * 4))
                out_tag = f"l{li}.out" if bi == len(layer) - 1 else f"l{li}.o{bi & 1}"
                x = self._cb(name + ".3", (blk.conv3, blk.bn3), t2, new(out_tag, ho, wo, planes * 4), act=True, r0=idt)
            tap(f"layer{li}", x)
            if li >= 2:
                feats.append(x)
        c2, c3, c4 = feats
        f = self.fpn
        oc = f.output1[0].out_channels
        o3 = self._cb("fpn.o3", tuple(f.output3), c4, new("fpn.o3", c4.shape[1], c4.shape[2], oc), act=True)
        o2 = self._cb("fpn.o2", tuple(f.output2), c3, new("fpn.o2", c3.shape[1], c3.shape[2], oc), act=True, r0=o3, r0_after=True)
        m2 = self._cb("fpn.m2", tuple(f.merge2), o2, new("fpn.m2", c3.shape[1], c3.shape[2], oc), act=True)
        o1 = self._cb("fpn.o1", tuple(f.output1), c2, new("fpn.o1", c2.shape[1], c2.shape[2], oc), act=True, r0=m2, r0_after=True)
        m1 = self._cb("fpn.m1", tuple(f.merge1), o1, new("fpn.m1", c2.shape[1], c2.shape[2], oc), act=True)
        outs = []
        for i, (ssh, x) in enumerate(((self.ssh1, m1), (self.ssh2, m2), (self.ssh3, o3))):
            tap(f"fpn{i + 1}", x)
            n, (h, w) = f"ssh{i + 1}", x.shape[1:3]
            y = new(n + ".y", h, w, oc)
            self._cb(n + ".3", tuple(ssh.conv3X3), x, y, act=True)
            c51 = self._cb(n + ".51", tuple(ssh.conv5X5_1), x, new(n + ".51", h, w, oc // 4), act=True)
            self._cb(n + ".52", tuple(ssh.conv5X5_2), c51, y, y_coff=oc // 2, act=True)
            c72 = self._cb(n + ".72", tuple(ssh.conv7X7_2), c51, new(n + ".72", h, w, oc // 4), act=True)
            self._cb(n + ".73", tuple(ssh.conv7x7_3), c72, y, y_coff=oc // 2 + oc // 4, act=True)
            outs.append(tap(n, y))
        return outs

    def run(self, frames_u8, resize=1.0, want_raw=False, taps=None):
        """Device uint8 BGR [B,H,W,3] -> (geom, ss, boxes [B,N,4], scores [B,N], landms [B,N,10], raw | None): everything before the
        selection, in the shape's cached workspace (valid until the next call at the shape)."""
        bsz, h, w, _ = frames_u8.shape
        ss, hn, wn = shrink_size(h, w)
        new = self._workspace(bsz, h, w, frames_u8.device)
        x0 = K.retina_prep(frames_u8, new("x0", hn, wn, 3), scale=1.0 / ss)
        if taps is not None:
            taps["prep"] = x0
        feats = self.features_nhwc(x0, new, taps)
        geom = K.retina_geom(hn, wn, resize, self.cfg["steps"], self.cfg["min_sizes"])
        boxes, scores, landms = new("boxes", geom.N, 4), new("scores", geom.N), new("landms", geom.N, 10)
        raw = (new("raw.loc", geom.N, 4), new("raw.conf", geom.N, 2), new("raw.lm", geom.N, 10)) if want_raw else None
        for level, x in enumerate(feats):
            wp, bias = self._heads(level)
            K.retina_head(x, wp, bias, geom, level, boxes, scores, landms, raw)
        return geom, ss, boxes, scores, landms, raw, new

    def forward(self, frames_u8):
        raise NotImplementedError("RetinaFace: call RetinaFaceDetection.raw / detect_device (the net runs on uint8 NHWC frames)")


def _check_frames(frames_u8, what):
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (3, 4) or frames_u8.shape[-1] != 3:
        got = (tuple(frames_u8.shape), frames_u8.dtype) if isinstance(frames_u8, torch.Tensor) else type(frames_u8)
        raise ValueError(f"{what}: device uint8 BGR frames [H,W,3] or [B,H,W,3], got {got}")
    if not frames_u8.is_cuda:
        raise RuntimeError("RetinaFaceDetection runs on the ROCm device only (no CPU path)")
    f = frames_u8 if frames_u8.dim() == 4 else frames_u8[None]
    if f.shape[0] < 1 or f.shape[1] < 1 or f.shape[2] < 1:
        raise ValueError(f"{what}: empty frames")
    return f.contiguous()


class RetinaFaceDetection(object):
    """retinaface_detection.py:20-131.  base_dir given: loads base_dir/weights/<network>.pth; base_dir None: refused unless
    E4S_ALLOW_UNINITIALIZED_LOSS_NETS=1 (load your own state dict into .net afterwards)."""

    def __init__(self, base_dir, device="cuda", network="RetinaFace-R50"):
        from .criteria import _have_weights
        if network != "RetinaFace-R50":
            raise NotImplementedError(f"RetinaFaceDetection(network={network!r}): the native detector is RetinaFace-R50 (cfg_re50); the "
                                      "MobileNet config is not provided")
        self.pretrained_path = os.path.join(base_dir, "weights", network + ".pth") if base_dir is not None else None
        self.device = device
        self.cfg = cfg_re50
        self.net = RetinaFace(cfg=self.cfg, phase="test")
        if _have_weights("RetinaFaceDetection (the GPEN checkpoint weights/RetinaFace-R50.pth)", self.pretrained_path):
            self.load_model()
        for p in self.net.parameters():
            p.requires_grad = False
        self.net.to(device)
        self.net.eval()

    @staticmethod
    def remove_prefix(state_dict, prefix):
        """Old checkpoints store every name behind 'module.' (retinaface_detection.py:42-45)."""
        return {(k.split(prefix, 1)[-1] if k.startswith(prefix) else k): v for k, v in state_dict.items()}

    def load_model(self):
        sd = torch.load(self.pretrained_path, map_location=torch.device("cpu"))
        sd = self.remove_prefix(sd["state_dict"] if "state_dict" in sd.keys() else sd, "module.")
        self.net.load_state_dict(sd, strict=True)

    # -- device interface -------------------------------------------------------------------------------------------------------
    def _select(self, new, boxes, scores, landms, ss, confidence_threshold, nms_threshold, top_k, keep_top_k):
        b, n = scores.shape
        top_k, keep_top_k = int(top_k), int(keep_top_k)
        if top_k < 1 or keep_top_k < 1:
            raise ValueError("RetinaFaceDetection: top_k and keep_top_k are 1 or more")
        skeys, sidx = new("sort.keys", n), new("sort.idx", n, dtype=torch.int64)
        torch.sort(scores, dim=1, descending=True, stable=True, out=(skeys, sidx))
        dev = scores.device
        dets = torch.empty(b, keep_top_k, 5, device=dev, dtype=torch.float32)
        lm = torch.empty(b, keep_top_k, 10, device=dev, dtype=torch.float32)
        counts = torch.empty(b, device=dev, dtype=torch.int32)
        K.retina_select(boxes, landms, skeys, sidx, confidence_threshold, nms_threshold, top_k, keep_top_k, ss, dets, lm, counts)
        return dets, lm, counts

    @torch.no_grad()
    def detect_device(self, frames_u8, resize=1, confidence_threshold=0.9, nms_threshold=0.4, top_k=5000, keep_top_k=750):
        """Device uint8 BGR [H,W,3] or [B,H,W,3] -> device (dets [B,K,5] (x1, y1, x2, y2, score), landms [B,K,10] (five x, then five
        y), counts int32 [B]); K = keep_top_k, rows past counts[b] are zero.  Stream-ordered, no host synchronisation."""
        f = _check_frames(frames_u8, "RetinaFaceDetection.detect_device")
        _, ss, boxes, scores, landms, _, new = self.net.run(f, resize=float(resize))
        return self._select(new, boxes, scores, landms, ss, confidence_threshold, nms_threshold, top_k, keep_top_k)

    @torch.no_grad()
    def raw(self, frames_u8, taps=None):
        """The reference net's output for the (shrunk, mean-subtracted) frames: (loc [B,N,4], conf [B,N,2] after the softmax, landms
        [B,N,10]).  taps: a dict that receives named intermediate NHWC buffers (valid until the next call at the shape)."""
        f = _check_frames(frames_u8, "RetinaFaceDetection.raw")
        raw = self.net.run(f, want_raw=True, taps=taps)[5]
        return tuple(t.clone() for t in raw)

    @torch.no_grad()
    def postprocess(self, loc, conf, landms, image_size, resize=1, confidence_threshold=0.9, nms_threshold=0.4, top_k=5000, keep_top_k=750,
                    ss=1.0):
        """retinaface_detection.py:81-131 on the network's raw outputs (device [B,N,4], [B,N,2], [B,N,10]) for a network input of
        image_size = (h, w); ss: the shrink factor the results are divided by.  Returns what detect_device returns."""
        if not loc.is_cuda:
            raise RuntimeError("RetinaFaceDetection runs on the ROCm device only (no CPU path)")
        geom = K.retina_geom(int(image_size[0]), int(image_size[1]), float(resize), self.cfg["steps"], self.cfg["min_sizes"])
        b = loc.shape[0]
        new = self.net._workspace(b, -int(image_size[0]), int(image_size[1]), loc.device)          # its own buffer set
        boxes, scores, lms = new("boxes", geom.N, 4), new("scores", geom.N), new("landms", geom.N, 10)
        K.retina_decode(loc.contiguous(), conf.contiguous(), landms.contiguous(), geom, boxes, scores, lms)
        return self._select(new, boxes, scores, lms, ss, confidence_threshold, nms_threshold, top_k, keep_top_k)

    # -- the reference's interface --------------------------------------------------------------------------------------------------
    def detect(self, img_raw, resize=1, confidence_threshold=0.9, nms_threshold=0.4, top_k=5000, keep_top_k=750, save_image=False):
        """The reference's call: numpy HWC BGR image -> numpy (dets float32 [n,5], landms float32 [n,10])."""
        arr = np.asarray(img_raw)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("RetinaFaceDetection.detect: an HWC BGR uint8 array")
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
        dets, lm, counts = self.detect_device(t, resize, confidence_threshold, nms_threshold, top_k, keep_top_k)
        n = int(counts[0])
        both = torch.cat((dets[0, :n], lm[0, :n]), 1).cpu().numpy()
        return both[:, :5].copy(), both[:, 5:].copy()

    def detect_tensor(self, img, *args, **kwargs):
        raise NotImplementedError("RetinaFaceDetection.detect_tensor is not provided (face_enhancement.py never calls it)")
