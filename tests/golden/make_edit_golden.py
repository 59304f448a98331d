"""Generate tests/golden/edit.pt and edit1024.pt by running the REAL reference on the CPU (build container only; the GPU box reads
the .pt files):  python tests/golden/make_edit_golden.py

Face editing as scripts/face_edit.py:81-97 and demo/gradio_demo.py:157-185 state it -- texture vectors mixed per region,
cal_style_codes, gen_img(randomize_noise=False) with the editor's per-channel noise maps [1,C,H,W] -- on synthetic weights
(synth.synth_state_dict).  Nothing large is stored: the source / reference texture vectors are the driven / target ones already in
net256.pt / net1024.pt, the label maps are synth's, and the noise is re-drawn from NOISE_SEED on both sides (torch.manual_seed here,
edit.make_noise(seed=) there: the same CPU stream).

  edit.pt      Net3(out_size=256): alpha in {0, 0.3, 1} over {hair, skin, lip}: the mixed rows, the full 256^2 image at alpha 0.3 and
               the images at alpha 0 and 1 strided ::4 (three full images would pass the 1 MiB limit of a committed file);
               demo/gradio_utils.py's label_map_to_colored_mask / colored_mask_to_label_map and the brush statement of
               gradio_demo.py:126-131 on a 64^2 map with id 255, an id >= 19 and off-palette colours
  edit1024.pt  Net3(out_size=1024): the same three edits, images strided ::8 plus a 128^2 centre crop (alpha 0.3 and 1), as net1024.pt
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from e4s_amd import edit, synth  # noqa: E402
from oracle import ref_shim  # noqa: E402

REGIONS = ["hair", "skin", "lip"]
ALPHAS = [0.0, 0.3, 1.0]
NOISE_SEED = {256: 11, 1024: 12}
K = 13


def reference_noise(out_size):
    """The list of face_edit.py:49-52, drawn in its order from torch's global generator."""
    torch.manual_seed(NOISE_SEED[out_size])
    return [torch.randn(*s) for s in edit.noise_shapes(out_size)]


def labels_for(out_size):
    return synth.synth_labels_blocks(1, 512, 64, seed=3) if out_size == 256 else synth.synth_labels_face(1, 512, seed=3)


@torch.no_grad()
def net_case(out_size):
    net = ref_shim.build_reference_net3(synth.synth_state_dict(out_size, K), synth.synth_latent_avg(out_size), out_size, K)
    base = torch.load(os.path.join(HERE, f"net{out_size}.pt"))
    src, ref = base["driven_sv"], base["target_sv"]
    onehot = synth.onehot(labels_for(out_size))
    noise = reference_noise(out_size)
    idx = [edit.COMP2INDEX[r] for r in REGIONS]
    rec = dict(out_size=out_size, K=K, regions=REGIONS, alphas=ALPHAS, noise_seed=NOISE_SEED[out_size], mixed_rows=[])
    imgs = []
    for alpha in ALPHAS:
        mixed = src.clone()
        for i in idx:                                         # face_edit.py:84-87
            mixed[0, i, :] = (1 - alpha) * src[0, i, :] + alpha * ref[0, i, :]
        codes = net.cal_style_codes(mixed)
        img, _, _ = net.gen_img(torch.zeros(1, 512, 32, 32), codes, onehot, randomize_noise=False, noise=noise)
        rec["mixed_rows"].append(mixed[0, idx].clone())
        imgs.append(img)
        print(f"  {out_size}: alpha {alpha} done", flush=True)
    rec["mixed_rows"] = torch.stack(rec["mixed_rows"])        # [alpha, region, 1280]
    if out_size == 256:
        rec["img"] = imgs[1].clone()
        rec["img_stride4"] = torch.cat([imgs[0], imgs[2]])[:, :, ::4, ::4].clone()
    else:
        c0 = out_size // 2 - 64
        rec["img_stride8"] = torch.cat(imgs)[:, :, ::8, ::8].clone()
        rec["img_crop"] = torch.cat(imgs[1:])[:, :, c0:c0 + 128, c0:c0 + 128].clone()
    return rec


def joins_case():
    if "gradio" not in sys.modules:                           # demo/gradio_utils.py imports gradio at its top and never uses it
        try:
            import gradio  # noqa: F401
        except ImportError:
            sys.modules["gradio"] = types.ModuleType("gradio")
            stubbed = True
        else:
            stubbed = False
    else:
        stubbed = False
    try:
        gu = ref_shim._load("ref_gradio_utils", os.path.join(ref_shim.REF_ROOT, "demo", "gradio_utils.py"))
    finally:
        if stubbed:
            del sys.modules["gradio"]
    g = np.random.RandomState(7)
    labels = g.randint(0, 19, size=(64, 64)).astype(np.uint8)
    labels[0, :4] = 255
    labels[1, :4] = 23                                        # an id outside the table
    labels[2, :4] = 19
    colored = gu.label_map_to_colored_mask(labels)
    colored_in = colored.copy()
    colored_in[5, 5] = (1, 2, 3)                              # off the palette
    colored_in[5, 6] = (204, 0, 1)                            # one off 'lip'
    colored_in[5, 7] = (0, 204, 204)
    labels_back = gu.colored_mask_to_label_map(colored_in)
    brush = np.zeros((64, 64, 4), dtype=np.uint8)             # gradio's RGBA sketch
    brush[10:20, 10:31, :3] = g.randint(1, 256, size=(10, 21, 3))
    brush[30, 30] = (0, 0, 0, 255)                            # alpha alone does not select
    brush[31, 33] = (0, 0, 7, 0)
    brush[32, 1] = (255, 255, 255, 255)                       # sums past a byte
    comp_idx = gu.COMP2INDEX["hair"]
    mask = np.sum(brush[:, :, 0:3], axis=-1) != 0             # gradio_demo.py:126-131
    brushed = gu.colored_mask_to_label_map(colored)
    brushed[mask] = comp_idx
    brushed_colored = gu.label_map_to_colored_mask(brushed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return dict(labels=t(labels), colored=t(colored), colored_in=t(colored_in), labels_back=t(labels_back), brush=t(brush),
                comp_idx=int(comp_idx), brushed=t(brushed), brushed_colored=t(brushed_colored), comp=list(gu.COMP),
                comp2index=dict(gu.COMP2INDEX), colors=t(np.asarray(gu.COMP_COLORS_NUMPY)))


def main():
    if "--1024-only" not in sys.argv:
        rec = net_case(256)
        rec["joins"] = joins_case()
        torch.save(rec, os.path.join(HERE, "edit.pt"))
        print("edit.pt done")
    if "--256-only" not in sys.argv:
        torch.save(net_case(1024), os.path.join(HERE, "edit1024.pt"))
        print("edit1024.pt done")


if __name__ == "__main__":
    main()
