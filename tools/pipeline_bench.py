"""Times FaceSwapPipeline.swap (e4s_amd/pipeline.py) with every native stage at synthetic weights, each stage alone, and the four
join kernels (csrc/pipeline.hip) beside their torch-eager statements.

    python tools/pipeline_bench.py [--iters 30] [--warmup 3] [--batches 1,8] [--precisions f32,bf16x3] [--no-pipeline]

1024^2 source and target faces (no quads: crop and paste-back are timed by tools/frame_io_time.py), the swap captured in a
GraphedFaceSwap of the batch's size.  HIP events around the whole call and, in separate loops on the intermediates of one call
(`taps`), around each stage; `overhead_ms` = whole - sum of the stages is what the pipeline itself costs (stacking the restored
frames, argument checks, allocations).  Synthetic weights find no face, so the real detector runs (its time and its one
device-to-host copy are in the figures) and its answer is replaced by one fixed face, which sends a face through GPEN, ParseNet and the
paste.  Joins: bytes moved / time beside the 8 TB/s of bench.py's roofline_hbm; at 3-12 MB per image they are launch-bound and no
threshold is set.  One JSON line per configuration."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

from e4s_amd import kernels as K, postproc, reenact, spade, synth  # noqa: E402
from tools.spade_bench import GEN, HE, KP, timed  # noqa: E402

HBM_TBS = 8.0
DEV = "cuda"


class FixedFaceDetector(object):
    """Runs the real detector, answers with one fixed face (see the module docstring)."""

    def __init__(self, detector):
        self.detector = detector
        self.dets = torch.tensor([[[230.0, 180.0, 800.0, 860.0, 0.99]]], device=DEV)
        self.lms = torch.tensor([[[400.0, 640.0, 530.0, 430.0, 630.0, 450.0, 430.0, 570.0, 660.0, 645.0]]], device=DEV)

    def detect_device(self, frame_u8):
        _, _, counts = self.detector.detect_device(frame_u8)
        counts.cpu()                                                              # the copy FaceRestorer.process would wait for
        return self.dets, self.lms, torch.ones(1, dtype=torch.int32)


def build_stages():
    from e4s_amd.face_parser import FaceParser
    from e4s_amd.face_paste import FaceRestorer, gpen_restore
    from e4s_amd.gpen import FullGenerator
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    from e4s_amd.parsenet import FaceParse
    from e4s_amd.retinaface import RetinaFaceDetection
    from e4s_amd.sr import RealESRNet
    net = Net3(make_opts(out_size=1024))
    net.load_state_dict(synth.synth_state_dict(1024, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(1024).to(DEV)
    net = net.to(DEV).eval()
    dec = spade.SPADEDecoder()
    gen = spade.OcclusionAwareSPADEGenerator(**GEN)
    sd = synth.synth_vid2vid_generator_state_dict(gen, seed=1)
    sd.update({"decoder." + k: v for k, v in synth.synth_vid2vid_decoder_state_dict(dec, seed=1).items()})
    gen.load_generator_state_dict(sd)
    kp, he = reenact.KPDetector(**KP), reenact.HEEstimator(**HE)
    kp.load_state_dict(synth.synth_vid2vid_state_dict(kp, seed=1), strict=True)
    he.load_state_dict(synth.synth_vid2vid_state_dict(he, seed=2), strict=True)
    reenactor = spade.Reenactor(reenact.PoseFrontEnd(kp.to(DEV), he.to(DEV), False), gen.to(DEV))
    sr = RealESRNet(device="cpu")
    sr.srmodel.load_state_dict(synth.synth_rrdb_state_dict(sr.srmodel), strict=True)
    sr.srmodel, sr.device = sr.srmodel.to(DEV), DEV
    gpen = FullGenerator(512, 512, 8, channel_multiplier=2, narrow=1)
    gpen.load_state_dict(synth.synth_gpen_state_dict(512, n_mlp=8), strict=True)
    fp = FaceParse(base_dir=None, device=DEV)
    fp.faceparse.load_state_dict(synth.synth_parsenet_state_dict(fp.faceparse), strict=True)
    det = RetinaFaceDetection(None, device=DEV)
    det.net.load_state_dict(synth.synth_retinaface_state_dict(det.net, seed=7), strict=True)
    restorer = FaceRestorer(gpen_restore(gpen.to(DEV).eval()), fp, in_size=512, detector=FixedFaceDetector(det))
    parser = FaceParser(None, device="cpu")
    parser.seg.load_state_dict(synth.synth_module_state_dict(parser.seg, tag="bisenet."), strict=True)
    parser.seg.to(DEV)
    return net, reenactor, sr, restorer, parser


# ---- the joins as torch-eager statements (the baseline) --------------------------------------------------------------------
def eager_resize_aa4(x_u8, g13):
    x = F.pad(x_u8.permute(0, 3, 1, 2).float() / 255.0, (6, 6, 6, 6), mode="reflect")
    x = F.conv2d(F.conv2d(x, g13.view(1, 1, 13, 1).expand(3, 1, 13, 1), groups=3), g13.view(1, 1, 1, 13).expand(3, 1, 1, 13), groups=3)
    return F.interpolate(x, scale_factor=0.25, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()


def eager_driven_seam(pred):
    u8 = (pred * 255).to(torch.uint8).flip(1)
    big = (F.interpolate(u8.float(), scale_factor=4, mode="bilinear", align_corners=False) + 0.5).to(torch.uint8)
    return u8.permute(0, 2, 3, 1).contiguous(), big.permute(0, 2, 3, 1).contiguous()


def eager_face_to_net(x_u8, bgr):
    rgb = x_u8.flip(-1).contiguous() if bgr else x_u8.clone()
    return rgb, rgb.permute(0, 3, 1, 2).float().div(255).sub_(0.5).div_(0.5).contiguous()


def join_rows(b, iters, warmup):
    faces = synth.synth_sr_input_u8(b, 1024, 1024, seed=3).to(DEV)
    pred = torch.rand(b, 3, 256, 256, device=DEV)
    k = torch.arange(-6, 7, device=DEV, dtype=torch.float32)
    g13 = torch.exp(-0.5 / 2.25 * k * k)
    g13 = g13 / g13.sum()
    px, small = 1024 * 1024, 256 * 256
    cases = (("resize_aa4", b * (px * 3 + small * 12), lambda: K.resize_aa4(faces), lambda: eager_resize_aa4(faces, g13)),
             ("driven_seam", b * (small * 12 + small * 3 + px * 3), lambda: K.driven_seam(pred), lambda: eager_driven_seam(pred)),
             ("face_to_net", b * (px * 3 + px * 3 + px * 12), lambda: K.face_to_net(faces, bgr=True), lambda: eager_face_to_net(faces, True)))
    for name, nbytes, native, eager in cases:
        med, best = timed(native, iters, warmup)
        emed, ebest = timed(eager, iters, warmup)
        print(json.dumps({"what": "join", "kernel": name, "batch": b, "mbytes": round(nbytes / 1e6, 2), "ms": round(med, 4), "best_ms": round(best, 4),
                          "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "frac_of_hbm": round(nbytes / (med * 1e-3) / 1e12 / HBM_TBS, 4),
                          "eager_ms": round(emed, 4), "eager_best_ms": round(ebest, 4)}), flush=True)


def pipeline_rows(stages, b, prec, iters, warmup):
    from e4s_amd.pipeline import FaceSwapPipeline
    K.PRECISION = prec
    net, reenactor, sr, restorer, parser = stages
    pipe = FaceSwapPipeline(net, reenactor, sr, restorer, parser, batch=b, graph=True)
    src = synth.synth_sr_input_u8(1, 1024, 1024, seed=5)[0].to(DEV)
    tgt = synth.synth_sr_input_u8(b, 1024, 1024, seed=6).to(DEV)
    t = {}
    pipe.swap(src, tgt, taps=t)
    whole, whole_best = timed(lambda: pipe.swap(src, tgt), iters, warmup)
    g = pipe.graphed
    pred = torch.rand(b, 3, 256, 256, device=DEV)

    def onehots_and_swap():
        for lab, out in ((t["D_labels"], g.static[1]), (t["T_labels"], g.static[3]), (t["swapped_labels"], g.static[4])):
            postproc.labelMap2OneHot(lab[:, None], pipe.num_cls, out=out)
        return g.replay()
    face = t["swapped_face"]
    d_rgb = K.face_to_net(t["D_bgr"], bgr=True, net=False)[0]
    alone = (("resize_aa4 S+T", lambda: (K.resize_aa4(src[None]), K.resize_aa4(tgt))),
             ("parse T", lambda: parser.parse(tgt)),
             ("reenactor.run", lambda: reenactor.run(t["S_256"][0], t["T_256"])),
             ("driven_seam", lambda: K.driven_seam(pred)),
             ("sr.upscale", lambda: sr.upscale(t["pred_bgr"], bgr=True)),
             ("restorer.process x B", lambda: [restorer.process(t["enlarged"][i], background=t["sr"][i])[0] for i in range(b)]),
             ("face_to_net D+T", lambda: (K.face_to_net(t["D_bgr"], bgr=True, out_net=g.static[0]), K.face_to_net(tgt, rgb=False, out_net=g.static[2]))),
             ("parse D", lambda: parser.parse(d_rgb)),
             ("mask swap", lambda: postproc.swap_head_mask_revisit_considerGlass(t["D_labels"], t["T_labels"])),
             ("one-hots + swap replay", onehots_and_swap),
             ("stitch", lambda: postproc.stitch(face, tgt, t["swapped_labels"], t["hole"], pipe.lap_bld, pipe.outer_dilation)))
    row = {"what": "FaceSwapPipeline.swap", "batch": b, "precision": prec, "whole_ms": round(whole, 3), "whole_best_ms": round(whole_best, 3), "stages_ms": {}}
    total = 0.0
    for name, fn in alone:
        med, _ = timed(fn, iters, warmup)
        row["stages_ms"][name] = round(med, 3)
        total += med
    row["sum_of_stages_ms"], row["overhead_ms"] = round(total, 3), round(whole - total, 3)
    row["ms_per_frame"] = round(whole / b, 3)
    print(json.dumps(row), flush=True)
    pipe.validate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--precisions", default="f32,bf16x3")
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_bench: needs the GPU (no CPU timing is meaningful)")
    batches = [int(v) for v in a.batches.split(",")]
    with torch.no_grad():
        for b in batches:
            join_rows(b, a.iters, a.warmup)
        if not a.no_pipeline:
            stages = build_stages()
            for prec in a.precisions.split(","):
                for b in batches:
                    pipeline_rows(stages, b, prec, a.iters, a.warmup)


if __name__ == "__main__":
    main()
