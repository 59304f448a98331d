"""Real-ESRNet x4 super-resolution (src/pretrained/gpen/sr_model/) -- MI355X-native.  256^2 frame -> 1024^2 background.

scripts/face_swap.py builds `FaceEnhancement(use_sr=True, sr_model="realesrnet", sr_scale=4)`; FaceEnhancement.process
(face_enhancement.py:63-66,105-106) first runs `RealESRNet.process` on the driven frame and blends the restored face into its
result.  Here that is `RealESRNet.process(img)` (the reference's signature) or `RealESRNet.upscale(images_u8)` on a device batch.

Module tree / state_dict identical to the reference (rrdbnet_arch.py:8-120), so a real `realesrnet_x4.pth["params_ema"]` loads
with strict=True.  The modules hold parameters only; execution is on NHWC buffers with csrc/rrdb.hip:

    reference                                         here
    ------------------------------------------------  --------------------------------------------------------------------
    img / 255, BGR -> RGB, conv_first                  e4s_rrdb_head_f32 (uint8 HWC in, one pass)
    ResidualDenseBlock: 5 convs over torch.cat(...)    e4s_rrdb_conv_f32 x 5 on ONE 160-channel buffer: conv k reads channels
                                                       [0, 32 k) and writes [32 k, 32 k + 32); no concatenation copy
    x5 * 0.2 + x                                       conv5's epilogue (into the next block's buffer)
    RRDB: out * 0.2 + x                                the third block's conv5 epilogue: (acc * 0.2 + r0) * 0.2 + r1
    feat + conv_body(body(feat))                       conv_body's epilogue
    F.interpolate(nearest, 2) + conv_up + lrelu        e4s_rrdb_conv_f32(up2): the upsampled map is never written
    conv_hr + lrelu                                    e4s_rrdb_conv_f32 (Cin = 32)
    conv_last, clamp, * 255, round, uint8, RGB -> BGR  e4s_rrdb_tail_f32 (one pass)

Arithmetic follows kernels.PRECISION: "f32" runs the exact fp32 MFMA, "bf16x3" and "auto" the split-bf16 path (three bf16 MFMAs per
product, fp32 accumulate).  Weights are re-packed once per weight version and precision (cached on each conv: packs.cached).  The
working set -- three 160-channel buffers at the input resolution, one 32-channel copy of conv_first's output, two 32-channel buffers
at 4x -- belongs to the RRDBNet, one set per input shape; nothing else is allocated after the first call at a shape but the result.
There is no CPU path; scales 2 and 1 (the reference's pixel-unshuffle variants) are not provided."""
import os

import numpy as np
import torch
from torch import nn

from . import kernels as K
from . import packs


class ResidualDenseBlock(nn.Module):
    """rrdbnet_arch.py:8-40"""

    def __init__(self, num_feat=32, num_grow_ch=32):
        super().__init__()
        self.conv1 = nn.Conv2d(num_feat, num_grow_ch, 3, 1, 1)
        self.conv2 = nn.Conv2d(num_feat + num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv3 = nn.Conv2d(num_feat + 2 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv4 = nn.Conv2d(num_feat + 3 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)


class RRDB(nn.Module):
    """rrdbnet_arch.py:43-64"""

    def __init__(self, num_feat=32, num_grow_ch=32):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch)


def _packed(conv):
    """(weights packed for e4s_rrdb_conv_f32 in the current precision, bias), cached on the conv."""
    f32 = K.sr_f32()
    w = packs.cached(conv, "rrdb", (conv.weight,), lambda: K.rrdb_pack(conv.weight.detach().float().contiguous(), f32), (f32,))
    return w, conv.bias.detach()


def _packed_small(conv):
    """conv_first [32,3,3,3] -> [27][32] ((ky, kx, ci)-major); conv_last [3,32,3,3] -> [9][3][32]: layout only, cached on the conv."""
    def build():
        w = conv.weight.detach().float()
        if w.shape[1] == 3:
            p = w.permute(2, 3, 1, 0).reshape(27, w.shape[0])
        else:
            p = w.permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1])
        return p.contiguous()
    return packs.cached(conv, "small", (conv.weight,), build), conv.bias.detach()


def dense_block(rdb, buf, out, *, outer=None):
    """ResidualDenseBlock.forward on the 160-channel NHWC buffer `buf` whose channels [0, 32) hold x: x1..x4 go into channels
    [32, 160) of buf, x5 * 0.2 + x into channels [0, 32) of `out` (another buffer).  outer: the RRDB's input buffer -- the result is
    (x5 * 0.2 + x) * 0.2 + outer[..., :32] (rrdbnet_arch.py:62-64), and `out` may be `outer` itself."""
    for k, conv in enumerate((rdb.conv1, rdb.conv2, rdb.conv3, rdb.conv4)):
        w, b = _packed(conv)
        K.rrdb_conv(buf, 32 * (k + 1), w, b, buf, 32 * (k + 1), epilogue=0)
    w, b = _packed(rdb.conv5)
    if outer is None:
        return K.rrdb_conv(buf, 160, w, b, out, 0, epilogue=1, r0=buf, s0=0.2)
    return K.rrdb_conv(buf, 160, w, b, out, 0, epilogue=2, r0=buf, s0=0.2, r1=outer, s1=0.2)


def rrdb(block, a, b, c):
    """RRDB.forward: input in channels [0, 32) of buffer a, result in the same place; b and c are the other two buffers."""
    dense_block(block.rdb1, a, b)
    dense_block(block.rdb2, b, c)
    return dense_block(block.rdb3, c, a, outer=a)


class RRDBNet(nn.Module):
    """rrdbnet_arch.py:66-120 for scale 4 and num_feat = num_grow_ch = 32 (the RealESRNet of the face-swap pipeline)."""

    def __init__(self, num_in_ch=3, num_out_ch=3, scale=4, num_feat=32, num_block=23, num_grow_ch=32):
        super().__init__()
        if scale in (1, 2):
            raise NotImplementedError(f"RRDBNet(scale={scale}): the pixel-unshuffle variants are not provided, only scale=4")
        if scale != 4:
            raise ValueError(f"RRDBNet(scale={scale}): the reference knows 4, 2 and 1")
        if num_feat != 32 or num_grow_ch != 32:
            raise NotImplementedError("RRDBNet: the native kernels are built for num_feat = num_grow_ch = 32")
        if num_in_ch != 3 or num_out_ch != 3:
            raise NotImplementedError("RRDBNet: 3-channel images in and out")
        self.scale = scale
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self._e4s_bufs = {}

    def workspace(self, b, h, w, device):
        """The buffers of one input shape (allocated on first use, then kept): a, b, c [B,h,w,160]; feat [B,h,w,32]; up1
        [B,2h,2w,32] (a view of buffer a, which is free by then); up2, hr [B,4h,4w,32]."""
        key = (b, h, w, str(device))
        ws = self._e4s_bufs.get(key)
        if ws is None:
            def new(*shape):
                return torch.empty(*shape, device=device, dtype=torch.float32)
            a = new(b, h, w, 160)
            ws = dict(a=a, b=new(b, h, w, 160), c=new(b, h, w, 160), feat=new(b, h, w, 32),
                      up1=a.view(-1)[:b * 4 * h * w * 32].view(b, 2 * h, 2 * w, 32),
                      up2=new(b, 4 * h, 4 * w, 32), hr=new(b, 4 * h, 4 * w, 32))
            self._e4s_bufs[key] = ws
        return ws

    def release_workspace(self):
        """Drop every cached buffer set (a captured graph that used one keeps it alive)."""
        self._e4s_bufs = {}

    def trunk_nhwc(self, ws):
        """body + conv_body + the skip: conv_first's output in ws['a'][..., :32] and ws['feat'] -> channels [0, 32) of ws['b']."""
        a, b, c = ws["a"], ws["b"], ws["c"]
        for block in self.body:
            rrdb(block, a, b, c)
        w, bias = _packed(self.conv_body)
        return K.rrdb_conv(a, 32, w, bias, b, 0, epilogue=1, r0=ws["feat"], s0=1.0)

    def features_nhwc(self, src, flip=False):
        """Everything before conv_last: src uint8 NHWC [B,H,W,3] or fp32 NCHW [B,3,H,W] in [0,1] -> NHWC [B,4H,4W,32]."""
        if not src.is_cuda:
            raise RuntimeError("RRDBNet runs on the ROCm device only (no CPU path)")
        if src.dtype == torch.uint8:
            bsz, h, w = src.shape[0], src.shape[1], src.shape[2]
        else:
            bsz, h, w = src.shape[0], src.shape[2], src.shape[3]
        ws = self.workspace(bsz, h, w, src.device)
        wp, bias = _packed_small(self.conv_first)
        K.rrdb_head(src, wp, bias, ws["a"], ws["feat"], flip=flip)
        feat = self.trunk_nhwc(ws)
        w1, b1 = _packed(self.conv_up1)
        K.rrdb_conv(feat, 32, w1, b1, ws["up1"], 0, epilogue=0, up2=True)
        w2, b2 = _packed(self.conv_up2)
        K.rrdb_conv(ws["up1"], 32, w2, b2, ws["up2"], 0, epilogue=0, up2=True)
        w3, b3 = _packed(self.conv_hr)
        return K.rrdb_conv(ws["up2"], 32, w3, b3, ws["hr"], 0, epilogue=0)

    @torch.no_grad()
    def forward(self, x):
        """fp32 NCHW [B,3,H,W] in [0,1] on the device -> fp32 NCHW [B,3,4H,4W], before any clamp (rrdbnet_arch.py:104-120)."""
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError(f"RRDBNet: fp32 NCHW [B,3,H,W] images, got {tuple(x.shape)} {x.dtype}")
        hr = self.features_nhwc(x)
        wp, bias = _packed_small(self.conv_last)
        return K.rrdb_tail(hr, wp, bias, nchw=True)

    @torch.no_grad()
    def upscale_u8(self, images, bgr=False):
        """uint8 NHWC [B,H,W,3] -> uint8 NHWC [B,4H,4W,3]: real_esrnet.py:26-55 without the host round trip.  bgr: the images are
        BGR (cv2) and so is the result; the network itself sees RGB."""
        if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
            raise ValueError(f"RRDBNet: uint8 NHWC [B,H,W,3] images, got {tuple(images.shape)} {images.dtype}")
        hr = self.features_nhwc(images, flip=bgr)
        wp, bias = _packed_small(self.conv_last)
        return K.rrdb_tail(hr, wp, bias, u8=True, flip=bgr)


def round_half_even_u8(v):
    """The uint8 rule of real_esrnet.py:53-55 on a float array / tensor in any range: clamp(v, 0, 1) * 255 in fp32, rounded half to
    even (numpy.round), as uint8.  Host-side statement of what e4s_rrdb_tail_f32 applies."""
    t = torch.as_tensor(np.asarray(v, dtype=np.float32) if not isinstance(v, torch.Tensor) else v).float()
    return torch.round(t.clamp(0, 1) * 255.0).to(torch.uint8)


class RealESRNet(object):
    """real_esrnet.py:9-59 for scale 4.  base_dir given: loads base_dir/weights/<model>_x4.pth["params_ema"] (model None:
    "realesrnet", the reference's default name); base_dir None: the net keeps its initial weights (load your own into .srmodel)."""

    def __init__(self, base_dir=None, model=None, scale=4, device="cuda"):
        self.base_dir, self.scale, self.device = base_dir, scale, device
        self.srmodel = RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=32, num_block=23, num_grow_ch=32, scale=scale)
        if base_dir is not None:
            path = os.path.join(base_dir, "weights", (model or "realesrnet") + "_x%d.pth" % scale)
            loadnet = torch.load(path, map_location="cpu")
            self.srmodel.load_state_dict(loadnet["params_ema"], strict=True)
        for p in self.srmodel.parameters():
            p.requires_grad = False
        self.srmodel.eval()
        self.srmodel = self.srmodel.to(device)

    def upscale(self, images_u8, bgr=False):
        """Device uint8 [B,H,W,3] -> device uint8 [B,4H,4W,3].  Stream-ordered, no host synchronisation; the working set is
        allocated on the first call at a shape (capture it in a torch.cuda.graph after one warm-up call)."""
        if not images_u8.is_cuda:
            raise RuntimeError("RealESRNet runs on the ROCm device only (no CPU path)")
        return self.srmodel.upscale_u8(images_u8.contiguous(), bgr=bgr)

    def process(self, img):
        """The reference's call: numpy HWC BGR uint8 -> numpy HWC BGR uint8 at 4x."""
        arr = np.asarray(img)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("RealESRNet.process: an HWC BGR uint8 array")
        t = torch.from_numpy(np.ascontiguousarray(arr))[None].to(self.device)
        return self.upscale(t, bgr=True)[0].cpu().numpy()
