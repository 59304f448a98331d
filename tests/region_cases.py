"""Operands of one masked StyledConv launch (shared by tests/test_gpu_parity.py and tests/test_gpu_region_rows_bits.py): seeded input,
weights, label map of the given kind and the epilogue's tables, on the GPU."""
import math

import torch

from e4s_amd import synth

DEV = "cuda"


def region_case(b, h, w, cin, cout, up, kind, R=12, seed=41):
    g = torch.Generator().manual_seed(seed)
    ncls = 4 if up else 1
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    wt = torch.randn(ncls, 9, cout, cin, generator=g).to(DEV) / math.sqrt(cin * 9)
    if kind == "face":                      # 512^2 face-like map, legacy-nearest lookup inside the kernel
        lab = synth.synth_labels_face(b, 512, seed=seed).view(b, 512, 512)
    elif kind == "blocks":                  # 8x8-pixel blocks at output resolution: boundaries inside every tile
        lab = torch.randint(0, R, (b, (ho + 7) // 8, (wo + 7) // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :ho, :wo]
    elif kind == "noise":                   # per-pixel random regions: every tile needs more variant rows than the kernel has
        lab = torch.randint(0, R, (b, ho, wo), generator=g)
    elif kind == "half-noise":              # left half noise (tiles overflow -> region-select kernel), right half two regions
        lab = torch.randint(0, R, (b, ho, wo), generator=g)
        lab[:, :, wo // 2:] = 3
        lab[:, ho // 3:, wo // 2 + 5:] = R - 1
    labels = lab.to(torch.uint8).contiguous().to(DEV)
    kw = dict(labels=labels, num_regions=R, ncls=ncls, ostride=2 if up else 1,
              in_scale=(torch.rand(b * R, cin, generator=g) + 0.5).to(DEV), out_scale=(torch.rand(b * R, cout, generator=g) + 0.5).to(DEV),
              noise=torch.randn(b, 1, ho, wo, generator=g).to(DEV), noise_w=torch.tensor([0.2], device=DEV),
              bias=(torch.randn(cout, generator=g) * 0.1).to(DEV), act=1)
    return x, wt, kw
