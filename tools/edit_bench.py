"""Times face editing (e4s_amd/edit.py) on one GPU: the generator with the editor's per-channel noise maps on the split-bf16
epilogues, beside the dispatch before them (stylegan2.PC_NOISE_SPLIT = False: every StyledConv on the exact-fp32 kernels) and beside
per-pixel noise; the captured edit; every touched conv kernel alone with both noise layouts; the three mask joins.

    python tools/edit_bench.py [--iters 30] [--warmup 3] [--batches 1,8] [--precisions f32,bf16x3] [--runs 2] [--no-layers]

HIP events around each call, median (and minimum) of --iters calls, the whole list --runs times in one process.  Net3(1024) at
synthetic weights, face-like label maps.  `gen_img` rows: noise = pixel | channel | channel_fallback; mode = eager | graph
(gen_img alone in a torch.cuda.graph, the style codes computed once outside).  `noise_gb` = bytes of the noise maps one call reads if every layer reads its
map once per sample: the distance between the pixel and the channel row is to be explained by it.  Layer rows: the largest generator
shape of each kernel, B = 8.  Joins: bytes moved / time beside the 8 TB/s of bench.py's roofline_hbm; at 0.26-1 MB per map they are
launch-bound and no threshold is set.  One JSON line per row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from e4s_amd import edit, kernels as K, postproc, stylegan2 as S, synth  # noqa: E402
from tools.spade_bench import timed  # noqa: E402

HBM_TBS = 8.0
DEV = "cuda"


def build_net():
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    net = Net3(make_opts(out_size=1024))
    net.load_state_dict(synth.synth_state_dict(1024, 13), strict=True)
    net.latent_avg = synth.synth_latent_avg(1024).to(DEV)
    return net.to(DEV).eval()


def noise_bytes(noise, batch):
    return sum(n.numel() * 4 * (batch if n.shape[0] == 1 else 1) for n in noise)


def emit(row):
    print(json.dumps(row), flush=True)


def gen_rows(net, b, prec, iters, warmup, run):
    K.PRECISION = prec
    labels = synth.synth_labels_face(b, 512, seed=3)[:, 0].to(torch.uint8).to(DEV)
    onehot = postproc.labelMap2OneHot(labels[:, None], 12)
    sv = torch.randn(b, 12, 1280, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.5
    codes = net.cal_style_codes(sv)
    pc = edit.make_noise(1024, DEV, seed=0)
    pp = [n[:, :1].contiguous() for n in pc]
    for name, noise, split in (("pixel", pp, True), ("channel", pc, True), ("channel_fallback", pc, False)):
        S.PC_NOISE_SPLIT = split

        def fn():
            return net.gen_img(None, codes, onehot, randomize_noise=False, noise=noise)[0]
        med, lo = timed(fn, iters, warmup)
        emit(dict(what="gen_img", run=run, precision=prec, batch=b, noise=name, mode="eager", ms=round(med, 3), min_ms=round(lo, 3),
                  noise_gb=round(noise_bytes(noise, b) / 1e9, 3)))
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            out = fn()
        med, lo = timed(g.replay, iters, warmup)
        emit(dict(what="gen_img", run=run, precision=prec, batch=b, noise=name, mode="graph", ms=round(med, 3), min_ms=round(lo, 3),
                  noise_gb=round(noise_bytes(noise, b) / 1e9, 3)))
        del g, out
    S.PC_NOISE_SPLIT = True
    ge = edit.GraphedFaceEdit(net, b, pc)
    ge.load(src_sv=sv, ref_sv=torch.flip(sv, [1]), labels=labels, regions=["hair", "skin", "lip"], alpha=0.3)
    med, lo = timed(ge.replay, iters, warmup)
    ge.validate()
    emit(dict(what="GraphedFaceEdit.replay", run=run, precision=prec, batch=b, ms=round(med, 3), min_ms=round(lo, 3)))
    del ge


# the largest generator shape of each touched kernel: (what, cin, cout, res, up, masked, polyphase)
LAYERS = [("conv_region (8-wave rows)", 512, 512, 64, False, True, False), ("conv_region (polyphase rows)", 512, 512, 32, True, True, False),
          ("conv_region (packed 4^2)", 512, 512, 4, False, True, False), ("conv_bf16x3 plain 128", 128, 128, 256, False, False, False),
          ("conv_bf16x3 plain 64", 64, 64, 512, False, False, False), ("conv_bf16x3 polyphase", 256, 128, 128, True, False, True),
          ("upconv_bf16x3", 256, 128, 128, True, False, False), ("upconv_bf16x3 64->32", 64, 32, 512, True, False, False),
          ("conv_c32", 32, 32, 1024, False, False, False)]


def layer_rows(b, iters, warmup, run):
    K.PRECISION = "bf16x3"
    g = torch.Generator().manual_seed(2)
    for what, cin, cout, res, up, masked, poly in LAYERS:
        S.UPCONV_BF16X3_EXACT = not poly
        m = S.StyledConv(cin, cout, 3, 512, upsample=up, mask_op=masked).to(DEV)
        x = torch.randn(b, res, res, cin, device=DEV)
        style = torch.randn(b * 12 if masked else b, 512, generator=g).to(DEV)
        s = K.modulate_vec(style, m.conv.modulation.weight, m.conv.modulation.bias)
        lab = synth.synth_labels_face(b, 512, seed=3)[:, 0].to(torch.uint8).to(DEV) if masked else None
        ho = 2 * res if up else res
        pc = torch.randn(1, cout, ho, ho, device=DEV).contiguous(memory_format=torch.channels_last)
        pp = pc[:, :1].contiguous()
        row = dict(what="layer", run=run, kernel=what, batch=b, cin=cin, cout=cout, out_res=ho, noise_mb=round(b * pc.numel() * 4 / 1e6, 1),
                   out_mb=round(b * ho * ho * cout * 4 / 1e6, 1))
        for name, nz, split in (("pixel", pp, True), ("channel", pc, True), ("channel_fallback", pc, False)):
            S.PC_NOISE_SPLIT = split
            med, lo = timed(lambda: m.run_nhwc(x, s, nz, lab, 12 if masked else 1), iters, warmup)
            row[name + "_ms"] = round(med, 4)
            if masked:
                row[name + "_path"] = K.LAST_REGION_PATH
        emit(row)
        del m, x, pc, pp
    S.PC_NOISE_SPLIT, S.UPCONV_BF16X3_EXACT = True, True


def join_rows(b, iters, warmup, run):
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 19, (b, 512, 512), generator=g).to(torch.uint8).to(DEV)
    rgb = edit.label_map_to_colored_mask(labels)
    brush = (torch.rand(b, 512, 512, 4, generator=g) < 0.1).to(torch.uint8).to(DEV) * 255
    src, ref = torch.randn(b, 12, 1280, generator=g).to(DEV), torch.randn(b, 12, 1280, generator=g).to(DEV)
    sel, a0, a1 = (t.to(DEV) for t in edit.mix_coefficients(["hair", "skin", "lip"], 0.3, b))
    n = labels.numel()
    for what, fn, nbytes in (("e4s_labels_to_color_u8", lambda: edit.label_map_to_colored_mask(labels), 4 * n),
                             ("e4s_color_to_labels_u8", lambda: edit.colored_mask_to_label_map(rgb), 4 * n),
                             ("e4s_mask_brush_u8", lambda: edit.edit_mask(labels, brush, "hair"), 6 * n),
                             ("e4s_texture_mix_f32", lambda: K.texture_mix(src, ref, sel, a0, a1), src.numel() * 4 * 2 + src.numel() * 4 * 3 // 12)):        # src in, out, 3 of 12 rows of ref
        med, lo = timed(fn, iters, warmup)
        emit(dict(what="join", run=run, kernel=what, batch=b, ms=round(med, 4), min_ms=round(lo, 4), mb=round(nbytes / 1e6, 2),
                  share_of_hbm=round(nbytes / (med * 1e-3) / (HBM_TBS * 1e12), 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--precisions", default="f32,bf16x3")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_bench needs the GPU: nothing here is measured on a CPU")
    batches = [int(v) for v in a.batches.split(",")]
    with torch.no_grad():
        net = build_net()
        for run in range(a.runs):
            for prec in a.precisions.split(","):
                for b in batches:
                    gen_rows(net, b, prec, a.iters, a.warmup, run)
            if not a.no_layers:
                layer_rows(max(batches), a.iters, a.warmup, run)
            for b in batches:
                join_rows(b, a.iters, a.warmup, run)


if __name__ == "__main__":
    main()
