"""face-vid2vid's SPADE decoder and the whole re-enactment step (src/pretrained/face_vid2vid/modules/generator.py:121-159,
modules/util.py:419-481) -- MI355X-native.  `SPADEDecoder.run` turns FeatureWarp's map into the driven frame; with it
`OcclusionAwareSPADEGenerator` is the reference's generator whole and `Reenactor` is drive_source_demo / make_animation: frames in,
re-enacted frames out, nothing imported from the reference.

`SPADE`, `SPADEResnetBlock`, `SPADEDecoder` and `OcclusionAwareSPADEGenerator` hold the reference's parameter tree, the
torch.nn.utils.spectral_norm entries included (`conv_0.weight_orig`, `.weight_u`, `.weight_v`, no `.weight`), so a checkpoint's
['generator'] entry loads strictly.  The modules hold parameters only; execution is on channels-last buffers:

    reference                                              here
    -----------------------------------------------------  -------------------------------------------------------------------
    fc, conv_0, conv_1 (+ x_s), conv_s                     e4s_rconv_f32; the spectral norm is folded on the host in fp64 (eval: no power
                                                             iteration, weight_orig / dot(u, W v)); the residual sits in conv_1's epilogue
    nn.Upsample(2), F.interpolate(seg, nearest)            never made: index >> 1 and >> 2 inside the gathers
    InstanceNorm2d                                         e4s_instnorm_stats_f32 on the map BEFORE the upsampling (its statistics are the
                                                             upsampled map's); one pass serves norm_0 and norm_s of an up block
    mlp_shared of every SPADE of one resolution            ONE e4s_spade_shared_f32 per resolution (12, 3 and 3 SPADEs; the weights'
                                                             rows concatenated); each SPADE reads its 128-channel slice
    mlp_gamma, mlp_beta, n * (1 + gamma) + beta, leaky     e4s_spade_conv_f32: one implicit GEMM 128 -> 2 C (rows interleaved), the
                                                             modulation and the activation in its epilogue
    conv_img(leaky_relu(x)), sigmoid                       e4s_spade_tail_f32 (fp32 NCHW, or the uint8 frame)

Launches per frame: 1 fc + 3 mlp_shared + 8 blocks x (2 or 3 modulating convs, 2 or 3 plain convs, 2 statistics passes) + the tail.
Arithmetic follows kernels.PRECISION as in reenact.py.  Eval mode only, no CPU path, no host synchronisation."""
import torch
from torch import nn

from . import kernels as K
from .reenact import PoseFrontEnd, _frames
from .reenact_warp import FeatureWarp, _NativeWarp

NHIDDEN = 128                                                                    # SPADE's hidden width (util.py:424)
DECODER_IN = 256                                                                 # SPADEDecoder's ic = label_nc (generator.py:124-127)


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------------
def spectral_weight(weight_orig, u, v):
    """The weight torch.nn.utils.spectral_norm uses in eval mode: weight_orig / sigma, sigma = dot(u, weight_orig.view(Cout, -1) @ v),
    in fp64 (no power iteration runs in eval)."""
    w = weight_orig.detach().double()
    sigma = torch.dot(u.detach().double(), torch.mv(w.reshape(w.shape[0], -1), v.detach().double()))
    return w / sigma


def interleave_gamma_beta(gamma, beta):
    """Rows (or entries) of mlp_gamma and mlp_beta interleaved [g_0, b_0, g_1, b_1, ...]: conv channel 2 c is gamma of channel c, 2 c + 1
    its beta (what e4s_spade_conv_f32's epilogue expects)."""
    if gamma.shape != beta.shape:
        raise ValueError("interleave_gamma_beta: two tensors of one shape")
    return torch.stack([gamma, beta], 1).reshape(2 * gamma.shape[0], *gamma.shape[1:]).contiguous()


def concat_shared(spades):
    """(weight [n 128,label_nc,3,3], bias [n 128]) of the SPADEs' mlp_shared convs, concatenated in order: SPADE i owns channels
    128 i .. 128 i + 127 of the one launch."""
    return (torch.cat([s.mlp_shared[0].weight.detach().float() for s in spades]).contiguous(),
            torch.cat([s.mlp_shared[0].bias.detach().float() for s in spades]).contiguous())


# ---- the reference's parameter tree -------------------------------------------------------------------------------------------------
class SpectralConv2d(nn.Module):
    """The state a Conv2d under torch.nn.utils.spectral_norm leaves in a checkpoint: bias, weight_orig (parameters), weight_u [Cout],
    weight_v [Cin k k] (buffers)."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, (kernel_size, kernel_size)
        ref = nn.Conv2d(in_channels, out_channels, kernel_size, padding=kernel_size // 2, bias=bias)
        if bias:
            self.bias = nn.Parameter(ref.bias.detach().clone())
        else:
            self.register_parameter("bias", None)
        self.weight_orig = nn.Parameter(ref.weight.detach().clone())
        self.register_buffer("weight_u", nn.functional.normalize(torch.randn(out_channels), dim=0, eps=1e-12))
        self.register_buffer("weight_v", nn.functional.normalize(torch.randn(in_channels * kernel_size * kernel_size), dim=0, eps=1e-12))


class SPADE(nn.Module):
    def __init__(self, norm_nc, label_nc):
        super().__init__()
        self.param_free_norm = nn.InstanceNorm2d(norm_nc, affine=False)
        self.mlp_shared = nn.Sequential(nn.Conv2d(label_nc, NHIDDEN, kernel_size=3, padding=1), nn.ReLU())
        self.mlp_gamma = nn.Conv2d(NHIDDEN, norm_nc, kernel_size=3, padding=1)
        self.mlp_beta = nn.Conv2d(NHIDDEN, norm_nc, kernel_size=3, padding=1)
        self.norm_nc = norm_nc


class SPADEResnetBlock(nn.Module):
    def __init__(self, fin, fout, label_nc):
        super().__init__()
        self.learned_shortcut = fin != fout
        fmiddle = min(fin, fout)
        self.conv_0 = SpectralConv2d(fin, fmiddle, 3)
        self.conv_1 = SpectralConv2d(fmiddle, fout, 3)
        if self.learned_shortcut:
            self.conv_s = SpectralConv2d(fin, fout, 1, bias=False)
        self.norm_0 = SPADE(fin, label_nc)
        self.norm_1 = SPADE(fmiddle, label_nc)
        if self.learned_shortcut:
            self.norm_s = SPADE(fin, label_nc)
        self.fin, self.fmiddle, self.fout = fin, fmiddle, fout

    def spades(self):
        return [self.norm_0, self.norm_1] + ([self.norm_s] if self.learned_shortcut else [])


class SPADEDecoder(_NativeWarp):
    """generator.py:121-159.  run(feature [N,256,h,w] channels-last or [N,h,w,256]) -> prediction [N,3,4h,4w] fp32, or with u8 the
    frames [N,4h,4w,3] uint8: fresh tensors.  Any h, w >= 1."""

    def __init__(self):
        super().__init__()
        ic, oc, label_nc = DECODER_IN, 64, DECODER_IN
        self.fc = nn.Conv2d(ic, 2 * ic, 3, padding=1)
        for i in range(6):
            setattr(self, f"G_middle_{i}", SPADEResnetBlock(2 * ic, 2 * ic, label_nc))
        self.up_0 = SPADEResnetBlock(2 * ic, ic, label_nc)
        self.up_1 = SPADEResnetBlock(ic, oc, label_nc)
        self.conv_img = nn.Conv2d(oc, 3, 3, padding=1)
        self.up = nn.Upsample(scale_factor=2)
        self._init_native()

    def middle_blocks(self):
        return [getattr(self, f"G_middle_{i}") for i in range(6)]

    def stages(self):
        """[(shift of the resolution, [(name, block)])]: the blocks that share one mlp_shared launch."""
        return [(0, [(f"G_middle_{i}", b) for i, b in enumerate(self.middle_blocks())]), (1, [("up_0", self.up_0)]), (2, [("up_1", self.up_1)])]

    # ---- cached packs ----
    def _shared_pack(self, shift, spades):
        tensors = [t for s in spades for t in (s.mlp_shared[0].weight, s.mlp_shared[0].bias)]

        def make():
            w, b = concat_shared(spades)
            return K.rconv_pack(w, K.sr_f32()), b
        return self._cached(f"shared{shift}", tensors, make)

    def _mod_pack(self, name, spade):
        g, b = spade.mlp_gamma, spade.mlp_beta

        def make():
            w = interleave_gamma_beta(g.weight.detach().float(), b.weight.detach().float())
            return K.rconv_pack(w, K.sr_f32()), interleave_gamma_beta(g.bias.detach().float(), b.bias.detach().float())
        return self._cached(name, [g.weight, g.bias, b.weight, b.bias], make)

    def _spectral_pack(self, name, conv):
        def make():
            w = spectral_weight(conv.weight_orig, conv.weight_u, conv.weight_v).float().contiguous()
            return K.rconv_pack(w, K.sr_f32()), None if conv.bias is None else conv.bias.detach().float().contiguous()
        return self._cached(name, [conv.weight_orig, conv.weight_u, conv.weight_v] + ([] if conv.bias is None else [conv.bias]), make)

    def _sconv(self, name, conv, x, y, r0=None):
        w, b = self._spectral_pack(name, conv)
        return K.rconv(x, conv.in_channels, w, conv.out_channels, conv.kernel_size[0], y, bias=b, r0=r0)

    def _tail_pack(self):
        c = self.conv_img
        return self._cached("conv_img", [c.weight, c.bias], lambda: (K.spade_tail_pack(c.weight.detach().float()), c.bias.detach().float().contiguous()))

    def _stats_ws(self, key, device, doubles):
        """The fp64 partial-sum workspace of the key's working set, grown to the largest statistics pass (launches are stream-ordered)."""
        ws = self._e4s_bufs.setdefault(key + (str(device), "f64"), {})
        if "ws" not in ws or ws["ws"].numel() < doubles:
            ws["ws"] = torch.empty(max(1, doubles), device=device, dtype=torch.float64)
        return ws["ws"]

    @staticmethod
    def _nhwc_view(feature):
        if not isinstance(feature, torch.Tensor) or not feature.is_cuda:
            raise RuntimeError("SPADEDecoder.run: a device tensor (there is no CPU path)")
        if feature.dim() == 4 and feature.dtype == torch.float32:
            if feature.shape[3] == DECODER_IN and feature.is_contiguous():
                return feature
            if feature.shape[1] == DECODER_IN and feature.permute(0, 2, 3, 1).is_contiguous():
                return feature.permute(0, 2, 3, 1)
        raise RuntimeError(f"SPADEDecoder.run: an fp32 feature [N,{DECODER_IN},h,w] in channels-last memory (as FeatureWarp.run returns it) or a "
                           f"contiguous [N,h,w,{DECODER_IN}]; it is read in place, never copied")

    @torch.no_grad()
    def run(self, feature, u8=False, taps=None):
        self._require_weights()
        seg = self._nhwc_view(feature)
        n, h, w, _ = seg.shape
        if min(n, h, w) < 1:
            raise ValueError("SPADEDecoder.run: an empty feature")
        dev = seg.device
        new = self._bufset((n, h, w), dev)

        def tap(name, t):
            if taps is not None:
                taps[name] = t.clone()                                          # the working buffers are reused further down
            return t

        # mlp_shared of every SPADE, one launch per resolution
        actv = []
        for shift, blocks in self.stages():
            spades = [s for _, b in blocks for s in b.spades()]
            wp, bias = self._shared_pack(shift, spades)
            cout = NHIDDEN * len(spades)
            actv.append(K.spade_shared(seg, DECODER_IN, wp, cout, bias, new(f"actv{shift}", n, h << shift, w << shift, cout), shift=shift))

        def stats_of(x, tag):
            b_, hh, ww, c = x.shape
            return K.instnorm_stats_into(x, new(tag, b_, c, 2), self._stats_ws((n, h, w), dev, K.lib.load().e4s_instnorm_ws_doubles(b_, hh * ww, c)))

        def modulate(name, spade, a, slot, x, stats, xs, act, y):
            wp, bias = self._mod_pack(name, spade)
            if taps is not None and act:                                        # the reference's hook sees the SPADE before the activation
                taps[name] = K.spade_conv(a, slot * NHIDDEN, NHIDDEN, wp, bias, x, stats, torch.empty_like(y), xs=xs, act=False)
            return K.spade_conv(a, slot * NHIDDEN, NHIDDEN, wp, bias, x, stats, y, xs=xs, act=act)

        fcw, fcb = self._folded("fc", self.fc, None, K.rconv_pack)
        x = tap("fc", K.rconv(seg, DECODER_IN, fcw, self.fc.out_channels, 3, new("x0", n, h, w, self.fc.out_channels), bias=fcb))
        flip = 0
        for (shift, blocks), a in zip(self.stages(), actv):
            hh, ww = h << shift, w << shift
            xs = 1 if shift else 0                                              # an up block reads x through nn.Upsample(2)
            slot = 0
            for name, blk in blocks:
                st = stats_of(x, f"stats{blk.fin}")
                m0 = modulate(f"{name}.norm_0", blk.norm_0, a, slot, x, st, xs, True, new(f"m0.{shift}", n, hh, ww, blk.fin))
                if blk.learned_shortcut:
                    ms = modulate(f"{name}.norm_s", blk.norm_s, a, slot + 2, x, st, xs, False, new(f"ms.{shift}", n, hh, ww, blk.fin))
                    if taps is not None:
                        taps[f"{name}.norm_s"] = ms.clone()
                    r0 = self._sconv(f"{name}.conv_s", blk.conv_s, ms, new(f"xs.{shift}", n, hh, ww, blk.fout))
                else:
                    r0 = x
                dx = tap(f"{name}.conv_0", self._sconv(f"{name}.conv_0", blk.conv_0, m0, new(f"dx.{shift}", n, hh, ww, blk.fmiddle)))
                st1 = stats_of(dx, f"stats1.{blk.fmiddle}")
                m1 = modulate(f"{name}.norm_1", blk.norm_1, a, slot + 1, dx, st1, 0, True, new(f"m1.{shift}", n, hh, ww, blk.fmiddle))
                flip ^= 1
                x = tap(name, self._sconv(f"{name}.conv_1", blk.conv_1, m1, new(f"x{shift}.{flip}", n, hh, ww, blk.fout), r0=r0))
                slot += len(blk.spades())
        wt, bt = self._tail_pack()
        logits = torch.empty(n, 3, 4 * h, 4 * w, device=dev) if taps is not None else None
        out = K.spade_tail(x, wt, bt, u8=u8, logits=logits)
        if taps is not None:
            taps["logits"] = logits
        return out


class OcclusionAwareSPADEGenerator(FeatureWarp):
    """generator.py:162-251 whole: FeatureWarp plus the SPADE decoder.  run(...) -> FeatureWarp.run's dict plus 'prediction'
    [N,3,H,W]."""

    def __init__(self, image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, reshape_depth,
                 num_resblocks, estimate_occlusion_map=False, dense_motion_params=None, estimate_jacobian=False):
        width = block_expansion * 2 ** num_down_blocks
        if width != DECODER_IN:
            raise NotImplementedError(f"OcclusionAwareSPADEGenerator: block_expansion * 2 ** num_down_blocks = {width}, but the SPADE decoder's "
                                      f"input width is fixed at {DECODER_IN} (generator.py:124)")
        super().__init__(image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, reshape_depth,
                         num_resblocks, estimate_occlusion_map=estimate_occlusion_map, dense_motion_params=dense_motion_params,
                         estimate_jacobian=estimate_jacobian)
        self.decoder = SPADEDecoder()                                            # last, as in the reference: the key order is the checkpoint's

    def load_generator_state_dict(self, state_dict):
        """Load a checkpoint's ['generator'] entry: every key must match, `decoder.*` included (a missing or an unexpected one raises)."""
        return self.load_state_dict(state_dict, strict=True)

    def load_state_dict(self, state_dict, strict=True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self.decoder._weights_loaded = True                                     # its entries came with this module's
        return res

    def release_workspace(self):
        super().release_workspace()
        self.decoder.release_workspace()

    @torch.no_grad()
    def run(self, source, kp_source, kp_driving, taps=None, u8=False):
        out = FeatureWarp.run(self, source, kp_source, kp_driving, taps)
        out["prediction"] = self.decoder.run(out["feature"], u8=u8, taps=taps)
        return out


class Reenactor(object):
    """PoseFrontEnd then OcclusionAwareSPADEGenerator: a source frame and N driving frames in, the N driven frames out (the
    reference's make_animation with relative = False, adapt_movement_scale = False)."""

    def __init__(self, front_end, generator):
        if not isinstance(front_end, PoseFrontEnd) or not isinstance(generator, OcclusionAwareSPADEGenerator):
            raise TypeError("Reenactor: a PoseFrontEnd and an OcclusionAwareSPADEGenerator")
        if front_end.kp_detector.kp.out_channels != generator.num_kp:
            raise ValueError("Reenactor: the front end and the generator disagree on num_kp")
        self.front_end, self.generator = front_end, generator

    @torch.no_grad()
    def run(self, source, driving, u8=False, **free_view):
        """source [H,W,3], driving a list of frames or [N,H,W,3] (numpy or tensors; float in [0,1] or uint8); free_view, yaw, pitch,
        roll as PoseFrontEnd.keypoints -> the driven frames [N,H,W,3] on the device: fp32 in [0,1], or uint8 with u8.  The source is
        encoded once."""
        dev = self.front_end.device
        src = _frames(source, dev, "Reenactor.run")
        kp_source, kp_driving = self.front_end.keypoints_device(src, _frames(driving, dev, "Reenactor.run"), **free_view)
        gen = self.generator
        feat = FeatureWarp.run(gen, gen.encode_source(src), kp_source, kp_driving)["feature"]
        out = gen.decoder.run(feat, u8=u8)
        return out if u8 else out.permute(0, 2, 3, 1)

    def make_animation(self, source, driving, **free_view):
        """What the reference's make_animation returns: a list of N [H,W,3] float32 numpy arrays in [0,1]."""
        frames = self.run(source, driving, **free_view).contiguous().cpu().numpy()
        return [f for f in frames]
