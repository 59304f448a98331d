"""BiSeNet face parser (src/pretrained/face_parsing/) -- MI355X-native.  Image batch -> 19-class or 12-class label maps.

scripts/face_swap.py:195-228 parses the target T and the GPEN-restored driven face D with `faceParsing_demo`, maps the 19
CelebAMask-HQ classes to the 12 E4S classes (src/datasets/dataset.py:60-108) and one-hot encodes them for Net3.  Here that
is `FaceParser.parse(images, seg12=True, onehot=True)` on a batch, every step on the device, no host synchronisation.

Module tree / state_dict identical to the reference (model.py:20-289, resnet.py:14-80), so a real `79999_iter.pth`
loads with strict=True.  BatchNorm is folded into the conv weights once per weight version (packs.cached, on
the module).  Execution on NHWC tensors:

    reference                                         here
    ------------------------------------------------  --------------------------------------------------------------------
    BicubicDownSample(2) + clamp + normalise           e4s_parser_preprocess_f32 (one pass, uint8 NHWC or fp32 NCHW in)
    conv1 7x7/2 + bn1 + relu                           e4s_conv_smallcin_f32
    maxpool 3x3/2 pad 1                                e4s_maxpool3s2p1_f32
    BasicBlock 3x3 convs                               encoders._conv3x3 (Winograd / split-bf16 / fp32) and _conv_strided
    BasicBlock relu(shortcut + bn2(conv2))             fp32 conv: the epilogue's per-channel noise term (noise_w = 1);
                                                       otherwise e4s_add_relu_f32 after the conv
    downsample 1x1/2 + bn                              _conv_strided(ntaps=1)
    ARM gate / conv_avg (pool, 1x1, BN, act)           e4s_mean_hw_f32 + e4s_parser_fc_f32
    up2_nearest(feat * gate + add)                     e4s_gate_add_up2_f32
    FFM cat + 1x1 ConvBNReLU                           e4s_add_relu_f32 (copies into channel slices) + 1x1 conv
    FFM gate, feat * (1 + gate)                        e4s_se_gate_f32; 1 + gate is the main head conv's in_scale
    conv_out 1x1 (19 classes)                          1x1 conv, 19 outputs padded to 32 with zero weights
    bilinear(align_corners) + argmax [+ 19->12]        e4s_parser_head_f32 (the 19 x H x W logits are never written)

There is no CPU path and nothing is downloaded: Resnet18 is built without the reference's ImageNet fetch (resnet.py:82-89)."""
import numpy as np
import torch
from torch import nn

from . import kernels as K
from .encoders import _conv3x3, _conv_strided, _pack3x3
from . import packs

N_CLASSES = 19
# src/datasets/dataset.py:60-108 (__ffhq_masks_to_faceParser_mask_detailed); 15, 16, 18 (neck, necklace, cloth) -> background
SEG19_TO_12 = (0, 6, 2, 2, 3, 3, 10, 7, 7, 11, 5, 9, 1, 1, 8, 0, 0, 4, 0)
_RELU = dict(act=1, alpha=0.0, gain=1.0)


def seg19_to_12(labels):
    """The 19 -> 12 class map on an integer array / tensor (host-side reference of what e4s_parser_head_f32 applies)."""
    table = np.asarray(SEG19_TO_12, dtype=np.uint8)
    if isinstance(labels, torch.Tensor):
        return torch.as_tensor(table, device=labels.device)[labels.long()]
    return table[np.asarray(labels)]


def bicubic_taps(factor=2, a=-0.5):
    """BicubicDownSample's normalised 1-D filter (face_parsing_demo.py:16-37), computed with the same fp32 torch operations."""
    size = factor * 4

    def kern(x):
        ax = torch.abs(x)
        if ax <= 1.0:
            return (a + 2.0) * torch.pow(ax, 3.0) - (a + 3.0) * torch.pow(ax, 2.0) + 1
        if 1.0 < ax < 2.0:
            return a * torch.pow(ax, 3) - 5.0 * a * torch.pow(ax, 2.0) + 8.0 * a * ax - 4.0 * a
        return 0.0

    k = torch.tensor([kern((i - torch.floor(torch.tensor(size / 2)) + 0.5) / factor) for i in range(size)], dtype=torch.float32)
    return k / torch.sum(k)


def parse_size(h, w):
    """Parse resolution of an h x w image: FaceParser(size=1024) downsamples by 1024 // 512 = 2 whatever the input size
    (a 1024^2 T is parsed at 512^2, a 512^2 GPEN output at 256^2).  Inputs below 512 take the reference's PIL bilinear
    branch, which is not provided."""
    if min(h, w) < 512:
        raise ValueError(f"FaceParser: inputs below 512 px take the reference's PIL-bilinear branch, which is not supported "
                         f"(got {h}x{w})")
    if h % 64 or w % 64:
        raise ValueError(f"FaceParser: height and width must be multiples of 64 (the /2 input then /32 in the network), got {h}x{w}")
    return h // 2, w // 2


# ---------------------------------------------------------------------------------------------------------------
# module tree (parameter holders; state_dict keys and shapes of the reference)
# ---------------------------------------------------------------------------------------------------------------
class ConvBNReLU(nn.Module):
    """model.py:20-40"""

    def __init__(self, in_chan, out_chan, ks=3, stride=1, padding=1):
        super().__init__()
        self.conv = nn.Conv2d(in_chan, out_chan, kernel_size=ks, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_chan)


class BiSeNetOutput(nn.Module):
    """model.py:42-70"""

    def __init__(self, in_chan, mid_chan, n_classes):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, mid_chan, ks=3, stride=1, padding=1)
        self.conv_out = nn.Conv2d(mid_chan, n_classes, kernel_size=1, bias=False)


class AttentionRefinementModule(nn.Module):
    """model.py:72-98"""

    def __init__(self, in_chan, out_chan):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, out_chan, ks=3, stride=1, padding=1)
        self.conv_atten = nn.Conv2d(out_chan, out_chan, kernel_size=1, bias=False)
        self.bn_atten = nn.BatchNorm2d(out_chan)
        self.sigmoid_atten = nn.Sigmoid()


class BasicBlock(nn.Module):
    """resnet.py:20-48"""

    def __init__(self, in_chan, out_chan, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_chan, out_chan, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(out_chan)
        self.conv2 = nn.Conv2d(out_chan, out_chan, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chan)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if in_chan != out_chan or stride != 1:
            self.downsample = nn.Sequential(nn.Conv2d(in_chan, out_chan, kernel_size=1, stride=stride, bias=False),
                                            nn.BatchNorm2d(out_chan))


def create_layer_basic(in_chan, out_chan, bnum, stride=1):
    return nn.Sequential(BasicBlock(in_chan, out_chan, stride=stride), *[BasicBlock(out_chan, out_chan) for _ in range(bnum - 1)])


class Resnet18(nn.Module):
    """resnet.py:51-80, without init_weight's ImageNet download (the parser's checkpoint holds every weight)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = create_layer_basic(64, 64, bnum=2, stride=1)
        self.layer2 = create_layer_basic(64, 128, bnum=2, stride=2)
        self.layer3 = create_layer_basic(128, 256, bnum=2, stride=2)
        self.layer4 = create_layer_basic(256, 512, bnum=2, stride=2)


class ContextPath(nn.Module):
    """model.py:101-150"""

    def __init__(self):
        super().__init__()
        self.resnet = Resnet18()
        self.arm16 = AttentionRefinementModule(256, 128)
        self.arm32 = AttentionRefinementModule(512, 128)
        self.conv_head32 = ConvBNReLU(128, 128, ks=3, stride=1, padding=1)
        self.conv_head16 = ConvBNReLU(128, 128, ks=3, stride=1, padding=1)
        self.conv_avg = ConvBNReLU(512, 128, ks=1, stride=1, padding=0)


class FeatureFusionModule(nn.Module):
    """model.py:192-235"""

    def __init__(self, in_chan, out_chan):
        super().__init__()
        self.convblk = ConvBNReLU(in_chan, out_chan, ks=1, stride=1, padding=0)
        self.conv1 = nn.Conv2d(out_chan, out_chan // 4, kernel_size=1, stride=1, padding=0, bias=False)
        self.conv2 = nn.Conv2d(out_chan // 4, out_chan, kernel_size=1, stride=1, padding=0, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.sigmoid = nn.Sigmoid()


# ---------------------------------------------------------------------------------------------------------------
# folded weights
# ---------------------------------------------------------------------------------------------------------------
class _Folded:
    """A conv with its eval-mode BatchNorm folded in: .weight [Cout,Cin,k,k], .bias [Cout] (or None).  The conv helpers cache
    their packs (tap-packed, split-bf16, Winograd) on this holder, which lives as long as the fold."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


def fold_conv_bn(weight, bn):
    """(W * s[co], beta - mean * s) with s = gamma / sqrt(var + eps): Conv2d(bias=False) -> BatchNorm2d(eval) as one conv.
    Computed in fp64, returned in the dtype of weight."""
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w = weight.double() * s.view(-1, *([1] * (weight.dim() - 1)))
    b = bn.bias.double() - bn.running_mean.double() * s
    return w.to(weight.dtype), b.to(weight.dtype)


def _fold(owner, conv, bn=None, cout_pad=None, smallcin=False):
    """The cached fold of (conv, bn) -- or of conv alone, its outputs zero-padded to cout_pad -- stored on `owner`."""
    tensors = [conv.weight] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])

    def build():
        w = conv.weight.detach().float()
        if bn is not None:
            w, b = fold_conv_bn(w, bn)
            b = b.contiguous()
        else:
            b = None
        if cout_pad is not None and cout_pad > w.shape[0]:
            w = nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, cout_pad - w.shape[0]))
        f = _Folded(w.contiguous(), b)
        if smallcin:
            f.small = K.pack_smallcin(f.weight)
        return f
    return packs.cached(owner, "fold", tensors, build, (cout_pad,))


def _cbr(m, **kw):
    """ConvBNReLU's fold (cached on the ConvBNReLU)."""
    return _fold(m, m.conv, m.bn, **kw)


def _mat(f):
    """A 1x1 fold's weight as a [Cout, Cin] matrix."""
    return f.weight.view(f.weight.shape[0], -1)


_ONES = {}


def _one(device):
    """Device scalar 1.0: the noise weight that turns the fp32 conv's per-channel noise term into the residual add."""
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones(1, device=device, dtype=torch.float32)
    return t


def _exact_f32(x, cout):
    """Whether encoders._conv3x3 runs this stride-1 3x3 conv (without an in_scale) on the exact fp32 kernel."""
    b, h, w, cin = x.shape
    return not K.wino_eligible(b, h, w, cin, cout) and not K.want_bf16x3(b, h, w, cin, cout)


def _conv3(x, f, **kw):
    return _conv3x3(x, f, f.weight.shape[0], bias=f.bias, **kw)


def _conv1(x, f, stride=1, **kw):
    return _conv_strided(x, f, f.weight.shape[0], stride, 1, bias=f.bias, **kw)


def basic_block(blk, x):
    """resnet.py:37-48 on NHWC: relu(shortcut + bn2(conv2(relu(bn1(conv1(x))))))."""
    c1 = _fold(blk.conv1, blk.conv1, blk.bn1)
    c2 = _fold(blk.conv2, blk.conv2, blk.bn2)
    cout = c1.weight.shape[0]
    stride = blk.conv1.stride[0]
    if stride == 1:
        r = _conv3(x, c1, **_RELU)
    else:
        r = _conv_strided(x, c1, cout, stride, 9, bias=c1.bias, **_RELU)
    if blk.downsample is None:
        sc = x
    else:
        sc = _conv1(x, _fold(blk.downsample, blk.downsample[0], blk.downsample[1]), stride=stride)
    if _exact_f32(r, cout):
        # the exact fp32 kernel's epilogue: v + noise_w * noise[b,y,x,c] + bias, then act -- the residual add in the conv
        return K.conv_mfma(r, _pack3x3(c2), cout, noise=sc, noise_w=_one(r.device), noise_per_channel=True, bias=c2.bias, **_RELU)
    return K.add_relu(_conv3(r, c2), sc)


def _arm(arm, x):
    """model.py:83-90: (feat, gate) with feat = ConvBNReLU(x), gate = sigmoid(bn(conv1x1(mean(feat))))."""
    feat = _conv3(x, _cbr(arm.conv), **_RELU)
    f = _fold(arm, arm.conv_atten, arm.bn_atten)
    return feat, K.parser_fc(K.mean_hw(feat), _mat(f), f.bias, act=2)


class BiSeNet(nn.Module):
    """model.py:238-289 (n_classes = 19).  forward(x NCHW, normalised) -> (out, out16, out32) NCHW logits at x's size."""

    def __init__(self, n_classes=N_CLASSES):
        super().__init__()
        if n_classes != N_CLASSES:
            raise ValueError("the face parser is the 19-class CelebAMask-HQ BiSeNet")
        self.cp = ContextPath()
        self.ffm = FeatureFusionModule(256, 256)
        self.conv_out = BiSeNetOutput(256, 256, n_classes)
        self.conv_out16 = BiSeNetOutput(128, 64, n_classes)
        self.conv_out32 = BiSeNetOutput(128, 64, n_classes)

    def context_nhwc(self, x):
        """ContextPath.forward (model.py:110-137) on NHWC x [B,H,W,3] -> (feat8, feat_cp8, feat_cp16)."""
        r = self.cp.resnet
        st = _fold(r, r.conv1, r.bn1, smallcin=True)
        x = K.conv_smallcin(x, st.small, st.bias, 64, 7, 2, 3, relu=True)
        x = K.maxpool3s2p1(x)
        for blk in r.layer1:
            x = basic_block(blk, x)
        for blk in r.layer2:
            x = basic_block(blk, x)
        feat8 = x
        for blk in r.layer3:
            x = basic_block(blk, x)
        feat16 = x
        for blk in r.layer4:
            x = basic_block(blk, x)
        feat32 = x
        cp = self.cp
        f = _cbr(cp.conv_avg)
        avg = K.parser_fc(K.mean_hw(feat32), _mat(f), f.bias, act=1)                  # conv_avg on the pooled [B,512]
        a32, g32 = _arm(cp.arm32, feat32)
        feat32_up = _conv3(K.gate_add_up2(a32, g32, avg), _cbr(cp.conv_head32), **_RELU)
        a16, g16 = _arm(cp.arm16, feat16)
        feat16_up = _conv3(K.gate_add_up2(a16, g16, feat32_up), _cbr(cp.conv_head16), **_RELU)
        return feat8, feat16_up, feat32_up

    def _head(self, out_mod, x, in_scale=None):
        """BiSeNetOutput at its own resolution: NHWC logits [B,h,w,32] (classes 19..31 are zero padding)."""
        kw = dict(_RELU)
        if in_scale is not None:
            kw["in_scale"] = in_scale
        hmid = _conv3(x, _cbr(out_mod.conv), **kw)
        return _conv1(hmid, _fold(out_mod, out_mod.conv_out, cout_pad=32))

    def main_logits_nhwc(self, x):
        """The first head's logits at 1/8 of x NHWC [B,H,W,3] (the only head FaceParser reads) -> NHWC [B,H/8,W/8,32]."""
        feat8, cp8, _ = self.context_nhwc(x)
        return self._main_head(feat8, cp8)

    def _main_head(self, feat8, cp8):
        b, h, w, c = feat8.shape
        fcat = torch.empty(b, h, w, 2 * c, device=feat8.device, dtype=torch.float32)     # torch.cat([fsp, fcp], dim=1)
        K.add_relu(feat8, out=fcat, coff=0)                                             # (both are ReLU outputs: exact copies)
        K.add_relu(cp8, out=fcat, coff=c)
        ffm = self.ffm
        feat = _conv1(fcat, _cbr(ffm.convblk), **_RELU)
        gate = K.se_gate(K.mean_hw(feat), ffm.conv1.weight.detach().view(ffm.conv1.weight.shape[0], -1),
                         ffm.conv2.weight.detach().view(ffm.conv2.weight.shape[0], -1))
        scale = K.parser_fc(gate, None, None, act=0, offset=1.0)                       # feat * atten + feat = feat * (1 + atten)
        return self._head(self.conv_out, feat, in_scale=scale)

    @torch.no_grad()
    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("BiSeNet runs on the ROCm device only (no CPU path)")
        size = tuple(x.shape[2:])
        if size[0] % 32 or size[1] % 32:
            raise ValueError(f"BiSeNet: input height and width must be multiples of 32, got {size}")
        feat8, cp8, cp16 = self.context_nhwc(K.nchw_to_nhwc(x))
        heads = (self._main_head(feat8, cp8), self._head(self.conv_out16, cp8), self._head(self.conv_out32, cp16))
        return tuple(K.parser_head(lg, N_CLASSES, size, labels=False, nchw=True)[2] for lg in heads)


class FaceParser(nn.Module):
    """face_parsing_demo.py:127-175 (size = 1024): parse(images) -> label maps at half the input resolution."""

    def __init__(self, seg_ckpt=None, size=1024, device="cuda"):
        super().__init__()
        from .criteria import _have_weights
        if size // 512 != 2:
            raise ValueError("FaceParser(size): the face-swap pipeline uses size=1024 (BicubicDownSample factor 2)")
        self.size = size
        self.seg = BiSeNet(N_CLASSES)
        if _have_weights("FaceParser (seg_ckpt: the BiSeNet checkpoint 79999_iter.pth)", seg_ckpt):
            self.seg.load_state_dict(torch.load(seg_ckpt, map_location="cpu"), strict=True)
        for p in self.seg.parameters():
            p.requires_grad = False
        self.seg.eval()
        self.taps = [float(t) for t in bicubic_taps(size // 512)]
        self.seg.to(device)

    def preprocess(self, images):
        """uint8 NHWC [B,H,W,3] or fp32 NCHW [B,3,H,W] in [0,1] -> the network input NHWC [B,H/2,W/2,3]."""
        if images.dtype == torch.uint8:
            if images.dim() != 4 or images.shape[3] != 3:
                raise ValueError(f"FaceParser: uint8 images are NHWC [B,H,W,3], got {tuple(images.shape)}")
            h, w = images.shape[1:3]
        else:
            if images.dim() != 4 or images.shape[1] != 3:
                raise ValueError(f"FaceParser: float images are NCHW [B,3,H,W], got {tuple(images.shape)}")
            h, w = images.shape[2:]
        parse_size(h, w)
        if not images.is_cuda:
            raise RuntimeError("FaceParser runs on the ROCm device only (no CPU path)")
        return K.parser_preprocess(images, self.taps)

    @torch.no_grad()
    def parse(self, images, seg12=True, onehot=False):
        """Labels uint8 [B,H/2,W/2] (12 E4S classes with seg12, else the 19 parser classes); with onehot=True also the fp32
        one-hot [B,12|19,H/2,W/2] (what torch_utils.labelMap2OneHot makes of the labels).  Stream-ordered, no host sync."""
        x = self.preprocess(images)
        logits = self.seg.main_logits_nhwc(x)
        lab, oh, _ = K.parser_head(logits, N_CLASSES, tuple(x.shape[1:3]), seg12=seg12, onehot=onehot)
        return (lab, oh) if onehot else lab

    def forward(self, img):
        return self.parse(img, seg12=False)


def face_parsing_demo(model, img, convert_to_seg12=True):
    """face_parsing_demo.py:187-208 (model_name 'default'): a PIL image or an HWC uint8 array -> numpy uint8 [h, w]."""
    arr = np.asarray(img)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] < 3:
        raise ValueError("face_parsing_demo: an RGB PIL image or an HWC uint8 array")
    dev = next(model.seg.parameters()).device
    t = torch.from_numpy(np.ascontiguousarray(arr[:, :, :3]))[None].to(dev)
    return model.parse(t, seg12=convert_to_seg12)[0].cpu().numpy()
