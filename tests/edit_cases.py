"""Face editing (e4s_amd/edit.py): the host statements the kernels of csrc/edit.hip are held to, the fixtures of
tests/golden/make_edit_golden.py and the StyledConv cases of the per-channel-noise tests.  No GPU here."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_CACHE = {}


def golden(name):
    if name not in _CACHE:
        _CACHE[name] = torch.load(os.path.join(GOLDEN, name), map_location="cpu", weights_only=False)
    return _CACHE[name]


# ---- host statements ---------------------------------------------------------------------------------------------------------------
def mix_ref(src, ref, sel, a0, a1):
    """torch-CPU statement of e4s_texture_mix_f32: separate float32 products and sum (no FMA: three ATen kernels), rows with
    sel = 0 copied.  src / ref [1|B,R,C], sel / a0 / a1 [B,R]."""
    b = a0.shape[0]
    s, r = src.expand(b, -1, -1), ref.expand(b, -1, -1)
    mixed = a0[:, :, None] * s + a1[:, :, None] * r
    out = s.clone()
    on = sel.bool()
    out[on] = mixed[on]
    return out


def colors():
    from e4s_amd import edit
    return np.asarray(edit.COMP_COLORS_NUMPY, dtype=np.uint8)


def labels_to_color_ref(labels):
    """numpy statement of label_map_to_colored_mask: a table look-up; ids outside the 19 colours (255 among them) black."""
    tab = np.zeros((256, 3), dtype=np.uint8)
    tab[:19] = colors()
    return tab[np.asarray(labels)]


def color_to_labels_ref(rgb):
    """numpy statement of colored_mask_to_label_map: exact match of all three bytes; unmatched 0."""
    rgb = np.asarray(rgb)
    out = np.zeros(rgb.shape[:-1], dtype=np.uint8)
    for i, c in enumerate(colors()):
        out[np.all(rgb == c, axis=-1)] = i
    return out


def brush_ref(labels, brush, comp_idx):
    """numpy statement of gradio_demo.py:126-130 (the sum in int64, as numpy promotes it)."""
    out = np.array(labels, copy=True)
    out[np.sum(np.asarray(brush)[..., 0:3].astype(np.int64), axis=-1) != 0] = comp_idx
    return out


# ---- StyledConv cases with per-channel noise: (cin, cout, res, up, cells, masked, polyphase) --------------------------------------
# the nine shapes of test_styled_conv_bf16x3_vs_oracle ...
NINE = [(512, 512, 16, False, 16, True), (512, 512, 8, True, 4, True), (256, 256, 32, False, 8, True),
        (512, 256, 16, True, 32, True), (512, 512, 4, False, 64, True), (512, 512, 4, True, 64, True),
        (128, 128, 32, False, 64, True), (256, 128, 16, True, 8, False), (128, 128, 16, False, 8, False)]
# ... and the unmasked tail: 64 -> 64 at 32^2, 128 -> 64 up-sampling at 16^2 (upconv_bf16x3), 32 -> 32 at 64^2 (conv_c32); then the
# launches that keep their epilogue in the conv kernel (Cin < 128: no K split), one per column tile of the plain kernel (128 / 32
# wide), the masked 8-wave kernel without a split, and the polyphase form of the unmasked up-convs, split and whole
EXTRA = [(64, 64, 32, False, 8, False), (128, 64, 16, True, 8, False), (32, 32, 64, False, 8, False),
         (64, 128, 32, False, 8, False), (64, 32, 32, False, 8, False), (64, 128, 32, False, 16, True)]
POLY = [(256, 128, 16, True, 8, False), (64, 32, 16, True, 8, False)]
STYLED = [c + (False,) for c in NINE + EXTRA] + [c + (True,) for c in POLY]


def styled_id(c):
    cin, cout, res, up, cells, masked, poly = c
    return f"{cin}to{cout}-{res}{'-up' if up else ''}{'-masked' + str(cells) if masked else ''}{'-polyphase' if poly else ''}"
