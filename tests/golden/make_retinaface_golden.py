"""Fixture of the RetinaFace-R50 detector (e4s_amd/retinaface.py): the REFERENCE's own RetinaFace, PriorBox, decode, decode_landm and
py_cpu_nms run on CPU, imported where they lie (src/pretrained/gpen/face_detect/; cv2 and the other absent third-party packages are
stubbed by oracle/ref_shim.stub_third_party).

torchvision is absent as well, and the reference builds its backbone from it.  Before the import this script therefore puts stand-in
modules into sys.modules (they win over the stub finder): `torchvision.models` with a plain-torch ResNet-50 v1.5 written below (the
stride on the 3x3 conv, downsample = 1x1 conv + BatchNorm), `torchvision.models._utils.IntermediateLayerGetter` and
`torchvision.models.detection.backbone_utils`.  The backbone is thus pinned to THIS restatement of torchvision's ResNet-50, not to
torchvision itself; its state_dict keys and shapes are the published ones.  Likewise the shrink of frames above 1500 pixels is pinned
to the fp64 half-pixel bilinear restatement below (dsize = round(src * ss), source coordinate (d + 0.5) / ss - 0.5), not to cv2.resize.

Weights: synth.synth_retinaface_state_dict(net), the same seeded tensors the tests load into e4s_amd.retinaface.RetinaFace.  Inputs are
recorded as seeds, never as tensors: a frame is synth.synth_retinaface_frame_u8(b, h, w, seed) (uint8 BGR), fed to the reference as
float(frame) - (104, 117, 123), NCHW.

Recorded:
    keys / shapes          the reference's state_dict
    A.*                    frame A, 75 x 109 (odd maps at every level: 38x55, 19x28, 10x14, 5x7, 3x4; N = 374): loc / conf / landms of the
                           fp64 forward (fp64), A.e32 = max |fp32 forward - fp64 forward| of the reference itself per output, A.priors
                           (the reference's PriorBox, float32), A.tap.<name> = the fp64 layer2/3/4, fpn1..3 and ssh1..3 outputs at
                           every position and every A.tap_cstep-th channel (stored fp32, NCHW) with A.tap.<name>.scale = max |.| of
                           the whole map
    B.*                    two frames of 64 x 96 in one batch: loc / conf / landms (fp64) and B.priors
    post                   crafted (loc, conf, landms) on frame A's prior grid with the arguments and the reference's result for each:
                           (i) about 40 candidates in 6 overlapping clusters, (ii) nothing above the threshold, (iii) top_k = 10 cutting
                           before NMS and keep_top_k = 3 after, (iv) ss != 1
    thin.*                 a 1504 x 64 frame (-> 1000 x 43): the fp64 shrink at thin.rows, every column (before the mean is subtracted)
The script asserts while it generates, re-drawing the seed of the crafted cases until it holds: scores pairwise distinct, every score
at least 1e-3 from the threshold, and every overlap the greedy NMS evaluates at least 1e-3 from the NMS threshold.  It also asserts
that every tapped stage has max |.| within [1e-2, 1e3] (the synthetic weights neither kill nor blow up the activations).

Run in the build container:  python tests/golden/make_retinaface_golden.py   (writes tests/golden/retinaface.pt)"""
import math
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FRAME_A = (75, 109, 51)            # h, w, seed
FRAME_B = (64, 96, 52)
FRAME_THIN = (1504, 64, 53)
TAP_CSTEP = 8
MEAN = (104, 117, 123)


# ---- stand-ins for the absent torchvision -----------------------------------------------------------------------------------------
class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        return self.relu(self.bn3(self.conv3(out)) + identity)


class _ResNet50(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, blocks, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))):
            ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
            layer = [_Bottleneck(inplanes, planes, stride, ds)]
            inplanes = planes * 4
            layer += [_Bottleneck(inplanes, planes) for _ in range(1, blocks)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, 1000)


class _IntermediateLayerGetter(nn.ModuleDict):
    """Keeps the model's children up to the last returned one and returns the named outputs, as torchvision's does."""

    def __init__(self, model, return_layers):
        want = dict(return_layers)
        layers = OrderedDict()
        left = set(want)
        for name, module in model.named_children():
            layers[name] = module
            left.discard(name)
            if not left:
                break
        super().__init__(layers)
        self.return_layers = want

    def forward(self, x):
        out = OrderedDict()
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def install_torchvision_stand_ins():
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    utils = types.ModuleType("torchvision.models._utils")
    det = types.ModuleType("torchvision.models.detection")
    bu = types.ModuleType("torchvision.models.detection.backbone_utils")
    for m in (tv, models, det):
        m.__path__ = []
    models.resnet50 = lambda pretrained=False, **kw: _ResNet50()
    utils.IntermediateLayerGetter = _IntermediateLayerGetter
    tv.models, models._utils, models.detection, det.backbone_utils = models, utils, det, bu
    for m in (tv, models, utils, det, bu):
        sys.modules[m.__name__] = m


def reference_detector():
    """The reference's retinaface_detection module (RetinaFace, PriorBox, decode, decode_landm, py_cpu_nms, cfg_re50), offline on CPU."""
    from oracle import ref_shim
    ref_shim.stub_third_party()
    install_torchvision_stand_ins()
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    try:
        import importlib
        return importlib.import_module("src.pretrained.gpen.face_detect.retinaface_detection")
    finally:
        sys.path[:] = saved


# ---- the fp64 restatement of the shrink -------------------------------------------------------------------------------------------
def shrink64(img, ss, rows):
    """img uint8 [H,W,3] -> float64 [len(rows), Wd, 3]: half-pixel bilinear to (round(H ss), round(W ss)), clamped at the border."""
    h, w = img.shape[:2]
    wd = int(round(w * ss))
    src = img.astype(np.float64)

    def coords(n_dst, n_src, idx):
        s = (np.asarray(idx, dtype=np.float64) + 0.5) / ss - 0.5
        i0 = np.floor(s)
        f = s - i0
        f = np.where(i0 < 0, 0.0, f)
        i0 = np.clip(i0, 0, None)
        f = np.where(i0 >= n_src - 1, 0.0, f)
        i0 = np.clip(i0, None, n_src - 1).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_src - 1), f
    y0, y1, fy = coords(None, h, rows)
    x0, x1, fx = coords(None, w, np.arange(wd))
    fx = fx[None, :, None]
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    fy = fy[:, None, None]
    return top * (1 - fy) + bot * fy


# ---- the reference's post-processing, composed as retinaface_detection.py:81-131 composes it ----------------------------------------------
def reference_post(ref, loc, conf, landms, im_hw, resize, thr, nms_thr, top_k, keep_top_k, ss):
    """loc [N,4], conf [N,2], landms [N,10] float32 -> (dets [n,5], landms [n,10], order of the candidates, kept positions)."""
    im_h, im_w = im_hw
    priors = ref.PriorBox(ref.cfg_re50, image_size=(im_h, im_w)).forward()
    boxes = (ref.decode(loc, priors, ref.cfg_re50["variance"]) * torch.Tensor([im_w, im_h, im_w, im_h]) / resize).numpy()
    scores = conf.numpy()[:, 1]
    lm = (ref.decode_landm(landms, priors, ref.cfg_re50["variance"]) * torch.Tensor([im_w, im_h] * 5) / resize).numpy()
    inds = np.where(scores > thr)[0]
    boxes, lm, scores = boxes[inds], lm[inds], scores[inds]
    order = scores.argsort()[::-1][:top_k]
    boxes, lm, scores = boxes[order], lm[order], scores[order]
    dets = np.hstack((boxes, scores[:, np.newaxis])).astype(np.float32, copy=False)
    cand = dets
    keep = ref.py_cpu_nms(dets, nms_thr)
    dets, lm = dets[keep, :][:keep_top_k, :], lm[keep][:keep_top_k, :]
    lm = lm.reshape((-1, 5, 2)).transpose((0, 2, 1)).reshape(-1, 10)
    return (dets / ss).astype(np.float32), (lm / ss).astype(np.float32), cand, inds[order]


def margins_ok(cand_dets, scores_all, thr, nms_thr):
    """The generation-time conditions on a crafted case (fp64): distinct scores, scores and evaluated overlaps 1e-3 off the thresholds."""
    s = np.sort(scores_all.astype(np.float64))
    if len(s) > 1 and np.min(np.diff(s)) <= 0:
        return False
    if np.min(np.abs(scores_all.astype(np.float64) - thr)) < 1e-3:
        return False
    d = cand_dets.astype(np.float64)
    area = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
    alive = list(range(len(d)))                                    # cand_dets is score-ordered already
    while alive:
        i, rest = alive[0], alive[1:]
        nxt = []
        for j in rest:
            w = max(0.0, min(d[i, 2], d[j, 2]) - max(d[i, 0], d[j, 0]) + 1)
            h = max(0.0, min(d[i, 3], d[j, 3]) - max(d[i, 1], d[j, 1]) + 1)
            ovr = w * h / (area[i] + area[j] - w * h)
            if abs(ovr - nms_thr) < 1e-3:
                return False
            if ovr <= nms_thr:
                nxt.append(j)
        alive = nxt
    return True


def craft(priors, im_hw, seed, n_cand, n_clusters):
    """(loc, conf, landms) float32 on the prior grid: n_cand candidates whose decoded boxes jitter around n_clusters boxes."""
    g = torch.Generator().manual_seed(seed)
    n = priors.shape[0]
    im_h, im_w = im_hw
    loc = 0.5 * torch.randn(n, 4, generator=g)
    landms = torch.randn(n, 10, generator=g)
    p1 = 0.05 + 0.8 * torch.rand(n, generator=g)                    # below 0.9 - 1e-3 by construction
    if n_cand:
        centres = torch.stack([8 + (im_w - 16) * torch.rand(n_clusters, generator=g), 8 + (im_h - 16) * torch.rand(n_clusters, generator=g)], 1)
        sizes = 14 + 16 * torch.rand(n_clusters, 2, generator=g)
        chosen = torch.randperm(n - 40, generator=g)[:n_cand]       # the two coarsest priors' exp() range is not needed
        for t, pi in enumerate(chosen.tolist()):
            c = t % n_clusters
            cx, cy = (centres[c] + 3.0 * torch.randn(2, generator=g)).tolist()
            bw, bh = (sizes[c] * (1 + 0.15 * torch.randn(2, generator=g))).tolist()
            pr = priors[pi].double()
            loc[pi, 0] = (cx / im_w - pr[0]) / (0.1 * pr[2])
            loc[pi, 1] = (cy / im_h - pr[1]) / (0.1 * pr[3])
            loc[pi, 2] = math.log(bw / im_w / pr[2]) / 0.2
            loc[pi, 3] = math.log(bh / im_h / pr[3]) / 0.2
            p1[pi] = 0.905 + 0.09 * torch.rand(1, generator=g).item()
    conf = torch.stack([1 - p1, p1], 1)
    return loc.float(), conf.float(), landms.float()


def main():
    from e4s_amd import synth
    ref = reference_detector()
    torch.manual_seed(0)
    net = ref.RetinaFace(cfg=ref.cfg_re50, phase="test").eval()
    sd = synth.synth_retinaface_state_dict(net, seed=7)
    net.load_state_dict(sd, strict=True)
    out = {"keys": list(net.state_dict().keys()), "shapes": [tuple(v.shape) for v in net.state_dict().values()], "weights_seed": 7,
           "frame_A": FRAME_A, "frame_B": FRAME_B, "frame_thin": FRAME_THIN, "A.tap_cstep": TAP_CSTEP}

    def net_input(b, h, w, seed):
        f = synth.synth_retinaface_frame_u8(b, h, w, seed)
        return (f.double() - torch.tensor(MEAN, dtype=torch.float64)).permute(0, 3, 1, 2).contiguous()

    net64 = ref.RetinaFace(cfg=ref.cfg_re50, phase="test").eval().double()
    net64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    taps = {}
    net64.body.register_forward_hook(lambda m, i, o: taps.update({f"layer{k + 1}": v for k, v in o.items()}))
    net64.fpn.register_forward_hook(lambda m, i, o: taps.update({f"fpn{k + 1}": v for k, v in enumerate(o)}))
    for k in (1, 2, 3):
        getattr(net64, f"ssh{k}").register_forward_hook(lambda m, i, o, k=k: taps.update({f"ssh{k}": o}))
    with torch.no_grad():
        xa = net_input(1, *FRAME_A)
        loc, conf, lm = net64(xa)
        for name, t in taps.items():
            scale = float(t.abs().max())
            assert math.isfinite(scale) and 1e-2 <= scale <= 1e3, (name, scale)
            print(f"stage {name}: shape {tuple(t.shape)} max |.| {scale:.4g}")
            out[f"A.tap.{name}"] = t[0, ::TAP_CSTEP].float().clone()
            out[f"A.tap.{name}.scale"] = scale
        loc32, conf32, lm32 = net(xa.float())
        out.update({"A.loc": loc[0].clone(), "A.conf": conf[0].clone(), "A.landms": lm[0].clone(),
                    "A.e32": [float((a.double() - b).abs().max()) for a, b in ((loc32, loc), (conf32, conf), (lm32, lm))]})
        print("frame A: N", loc.shape[1], "scales", [float(t.abs().max()) for t in (loc, conf, lm)], "e32", out["A.e32"],
              "scores > 0.9:", int((conf[0, :, 1] > 0.9).sum()))
        assert loc.shape[1] == 374
        pri_a = ref.PriorBox(ref.cfg_re50, image_size=FRAME_A[:2]).forward()
        out["A.priors"] = pri_a.clone()
        xb = net_input(2, *FRAME_B)
        locb, confb, lmb = net64(xb)
        out.update({"B.loc": locb.clone(), "B.conf": confb.clone(), "B.landms": lmb.clone(),
                    "B.priors": ref.PriorBox(ref.cfg_re50, image_size=FRAME_B[:2]).forward().clone()})

    # ---- crafted post-processing cases ----
    ss4 = 1000.0 / 1504.0
    specs = [("i", 40, 6, dict(thr=0.9, nms_thr=0.4, top_k=5000, keep_top_k=750, ss=1.0, resize=1)),
             ("ii", 0, 0, dict(thr=0.9, nms_thr=0.4, top_k=5000, keep_top_k=750, ss=1.0, resize=1)),
             ("iii", 40, 6, dict(thr=0.9, nms_thr=0.4, top_k=10, keep_top_k=3, ss=1.0, resize=1)),
             ("iv", 40, 6, dict(thr=0.9, nms_thr=0.4, top_k=5000, keep_top_k=750, ss=ss4, resize=1))]
    post = []
    for ci, (name, n_cand, n_cl, args) in enumerate(specs):
        seed = 1000 * (ci + 1)
        while True:
            l, c, m = craft(pri_a, FRAME_A[:2], seed, n_cand, n_cl)
            dets, lms, cand, _ = reference_post(ref, l, c, m, FRAME_A[:2], args["resize"], args["thr"], args["nms_thr"], args["top_k"],
                                                args["keep_top_k"], args["ss"])
            unlimited = reference_post(ref, l, c, m, FRAME_A[:2], args["resize"], args["thr"], args["nms_thr"], 5000, 750, 1.0)[0]
            ok = margins_ok(cand, c.numpy()[:, 1], args["thr"], args["nms_thr"])
            if name == "i" or name == "iv":
                ok = ok and 3 <= len(dets) < n_cand                  # NMS both keeps and drops
            if name == "iii":
                ok = ok and len(cand) == 10 and len(dets) == 3 and len(unlimited) > 3
            if name == "ii":
                ok = ok and dets.shape == (0, 5) and lms.shape == (0, 10)
            if ok:
                break
            seed += 1
        print(f"post case ({name}): seed {seed}, {len(cand)} candidates -> {len(dets)} kept")
        post.append(dict(name=name, loc=l, conf=c, landms=m, dets=torch.from_numpy(dets), lm=torch.from_numpy(lms), **args))
    out["post"] = post

    # ---- the thin frame's shrink ----
    h, w, seed = FRAME_THIN
    frame = synth.synth_retinaface_frame_u8(1, h, w, seed)[0].numpy()
    ss = 1000.0 / max(h, w)
    rows = sorted(set(range(0, 4)) | set(range(996, 1000)) | set(range(0, 1000, 37)))
    out["thin.rows"] = rows
    out["thin.size"] = (int(round(h * ss)), int(round(w * ss)))
    out["thin.values"] = torch.from_numpy(shrink64(frame, ss, rows))
    assert out["thin.size"] == (1000, 43)

    path = os.path.join(HERE, "retinaface.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
