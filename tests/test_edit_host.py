"""Face editing without a GPU: the host statements of the mix and the mask joins (tests/edit_cases.py) against what the reference
recorded (tests/golden/edit.pt), the editor's noise list, and Editor's option handling."""
import types

import numpy as np
import pytest
import torch

import edit_cases as ec
from e4s_amd import edit


def test_mix_statement_reproduces_the_reference_rows_bit_for_bit(golden):
    """mix_coefficients + the torch-CPU statement == `(1 - alpha) * src + alpha * ref` as the reference ran it."""
    for name in ("edit.pt", "edit1024.pt"):
        rec = ec.golden(name)
        base = golden(f"net{rec['out_size']}.pt")
        src, ref = base["driven_sv"], base["target_sv"]
        idx = edit.region_indices(rec["regions"])
        order = [edit.COMP2INDEX[r] for r in rec["regions"]]
        for k, alpha in enumerate(rec["alphas"]):
            sel, a0, a1 = edit.mix_coefficients(rec["regions"], alpha, 1)
            out = ec.mix_ref(src, ref, sel, a0, a1)
            assert torch.equal(out[0, order], rec["mixed_rows"][k])
            rest = [i for i in range(12) if i not in idx]
            assert torch.equal(out[0, rest], src[0, rest])


def test_mix_coefficients():
    sel, a0, a1 = edit.mix_coefficients(["hair", 6], 0.3, 2)
    assert sel.dtype == torch.uint8 and sel.tolist() == [[0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0]] * 2
    assert float(a0[0, 0]) == float(np.float32(1 - 0.3)) and float(a1[1, 3]) == float(np.float32(0.3))
    # 1 - alpha in double, THEN rounded: at alpha = 0.6 float32(1) - float32(alpha) is another number
    _, b0, _ = edit.mix_coefficients(["hair"], 0.6, 1)
    assert float(b0[0, 0]) == float(np.float32(1 - 0.6)) != float(np.float32(1) - np.float32(0.6))
    sel, a0, a1 = edit.mix_coefficients([], torch.tensor([0.0, 1.0, 0.25]), 3)
    assert int(sel.sum()) == 0 and a1[:, 0].tolist() == [0.0, 1.0, 0.25] and a0[:, 5].tolist() == [1.0, 0.0, 0.75]
    with pytest.raises(ValueError):
        edit.mix_coefficients(["hair"], torch.tensor([0.1, 0.2]), 3)
    with pytest.raises(ValueError):
        edit.mix_coefficients(["beard"], 0.5, 1)


def test_join_statements_equal_the_reference():
    j = ec.golden("edit.pt")["joins"]
    assert j["comp"] == edit.COMP and j["comp2index"] == edit.COMP2INDEX
    assert np.array_equal(j["colors"].numpy(), np.asarray(edit.COMP_COLORS_NUMPY))
    labels = j["labels"].numpy()
    assert (labels == 255).any() and ((labels >= 19) & (labels != 255)).any()
    assert np.array_equal(ec.labels_to_color_ref(labels), j["colored"].numpy())
    assert np.array_equal(ec.color_to_labels_ref(j["colored_in"].numpy()), j["labels_back"].numpy())
    back = ec.color_to_labels_ref(j["colored"].numpy())
    brushed = ec.brush_ref(back, j["brush"].numpy(), j["comp_idx"])
    assert np.array_equal(brushed, j["brushed"].numpy())
    assert np.array_equal(ec.labels_to_color_ref(brushed), j["brushed_colored"].numpy())


def test_noise_list_shapes():
    s1024, s256 = edit.noise_shapes(1024), edit.noise_shapes(256)
    assert len(s1024) == 17 and len(s256) == 13 and s1024[:13] == s256
    assert s1024[0] == (1, 512, 4, 4)
    chans = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}
    for k, res in enumerate([8, 16, 32, 64, 128, 256, 512, 1024]):
        assert s1024[1 + 2 * k] == s1024[2 + 2 * k] == (1, chans[res], res, res)
    with pytest.raises(ValueError):
        edit.noise_shapes(100)


def test_make_noise_draws_the_reference_stream_channels_last():
    noise = edit.make_noise(256, "cpu", seed=11)
    torch.manual_seed(11)
    want = [torch.randn(*s) for s in edit.noise_shapes(256)]
    assert len(noise) == 13
    for n, w in zip(noise, want):
        assert torch.equal(n, w)
        assert n.permute(0, 2, 3, 1).is_contiguous()         # the layout the conv epilogues read: a view, no transpose launch
    torch.manual_seed(5)
    a = edit.make_noise(8, "cpu")                            # seed=None: torch's global generator, as the reference
    torch.manual_seed(5)
    assert torch.equal(a[0], torch.randn(1, 512, 4, 4))


class _StubNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.opts = types.SimpleNamespace(num_seg_cls=12)

    def get_style_vectors(self, img, mask):
        raise AssertionError("not reached")

    def gen_img(self, *a, **k):
        raise AssertionError("not reached")


class _StubParser:
    def parse(self, images):
        raise AssertionError("not reached")


def _opts(**kw):
    base = dict(regions=["hair"], checkpoint_path=None, faceParser_name="default", faceParsing_ckpt=None, segnext_config="", device="cpu",
                out_size=256, num_seg_cls=12, start_from_latent_avg=True, alpha=0.5, source="s.jpg", reference="r.jpg")
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_editor_option_handling():
    ed = edit.Editor(_opts(regions=["skin", "hair", "hair"]), net=_StubNet(), parser=_StubParser())
    assert ed.regions == [4, 6] and len(ed.noise) == 13 and ed.noise[-1].shape == (1, 128, 256, 256)
    assert ed.opts.alpha == 0.5 and ed.faceParsing_model is not None
    with pytest.raises(ValueError, match="beard"):
        edit.Editor(_opts(regions=["beard"]), net=_StubNet(), parser=_StubParser())
    with pytest.raises(ValueError, match="pre-trained weights"):
        edit.Editor(_opts(), net=None, parser=_StubParser())               # no checkpoint, no net: nothing is downloaded
    with pytest.raises(NotImplementedError):
        edit.Editor(_opts(faceParser_name="segnext"), net=_StubNet(), parser=None)
    with pytest.raises(TypeError):
        edit.FaceEditor(object())
    with pytest.raises(TypeError):
        edit.FaceEditor(_StubNet(), parser=object())
