"""GPU tests of the two opt-in paths built on resize.pil_resize: crop_image's shrink branch (align.crop_faces_by_quads(shrink=True))
and FaceSwapPipeline(any_size=True), against live Pillow.

The crop is held to the bounds the existing crop test holds the same kernel to (align_cases.MAX_LEVELS, MAX_SHARE); the resize in
front of it is byte-equal to Pillow's and adds no error of its own.  Frames [4,400,600,3], size 64, quads of shrink 1, 2, 3, 4 in
one call."""
import numpy as np
import pytest
import torch

import align_cases as ac
import pil_resize_cases as rc
import pipeline_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_shrink_crop_follows_crop_image():
    from e4s_amd import align
    frames = ac.frames(len(rc.SHRINK_QUADS), *rc.SHRINK_HW, seed=11)
    before = rc.SHRINK_QUADS.copy()
    with pytest.raises(NotImplementedError):
        align.crop_faces_by_quads(_dev(frames), rc.SHRINK_QUADS, rc.SHRINK_S)                 # the default keeps refusing
    taps = {}
    faces, norm = align.crop_faces_by_quads(_dev(frames), rc.SHRINK_QUADS, rc.SHRINK_S, normalized=True, shrink=True, taps=taps)
    assert np.array_equal(rc.SHRINK_QUADS, before)
    assert faces.shape == (4, rc.SHRINK_S, rc.SHRINK_S, 3) and norm.shape == (4, 3, rc.SHRINK_S, rc.SHRINK_S)
    assert [t[:2] for t in taps["shrunk"]] == [(1, 2), (2, 3), (3, 4)]
    subs = {}
    for i, quad in enumerate(rc.SHRINK_QUADS):
        want, subs[i] = rc.pil_shrink_crop(frames[i], quad, rc.SHRINK_S)
        levels, share = ac.score(faces[i].cpu().numpy(), want)
        print(f"face {i} (shrink {rc.SHRINKS[i]}): max level difference {levels}, share of unequal pixels {share:.2e}")
        assert levels <= ac.MAX_LEVELS and share <= ac.MAX_SHARE
        assert want.any(), "an empty crop proves nothing"
    assert torch.equal(norm.cpu(), (((faces.cpu().float() / 255) - 0.5) / 0.5).permute(0, 3, 1, 2))      # torch on the CPU divides
    # the window of the shrunk frame that the crop kernel read is Pillow's, byte for byte
    for i, shrink, win, buf in taps["shrunk"]:
        assert tuple(buf.shape) == subs[i].shape and np.array_equal(buf.cpu().numpy(), subs[i]), (i, shrink, win)
    # a batch that needs no shrinking is today's single launch, bit for bit
    small = np.stack([rc.SHRINK_QUADS[0]] * 4)
    assert torch.equal(align.crop_faces_by_quads(_dev(frames), small, rc.SHRINK_S, shrink=True),
                       align.crop_faces_by_quads(_dev(frames), small, rc.SHRINK_S))


def test_paste_back_takes_the_unshrunk_quads():
    """The inverse transforms are built from the quads as given (face_swap.py:110-113), so the paste of a size x size face is what
    it is today and matches live Pillow."""
    from e4s_amd import align
    frames = ac.frames(2, *rc.SHRINK_HW, seed=12)
    quads = rc.SHRINK_QUADS[1:3]
    faces = align.crop_faces_by_quads(_dev(frames), quads, rc.SHRINK_S, shrink=True)
    swapped = 255 - faces
    got = align.paste_back(swapped, _dev(frames), quads).cpu().numpy()
    for i in range(2):
        want, alpha = ac.pil_paste(swapped[i].cpu().numpy(), frames[i], ac.inverse_coefficients(quads[i], rc.SHRINK_S))
        levels, share = ac.score(got[i], want)
        print(f"paste {i}: max level difference {levels}, share of unequal pixels {share:.2e}")
        assert levels <= ac.MAX_LEVELS and share <= ac.MAX_SHARE and alpha.any()


def _image(h, w, seed):
    rng = np.random.RandomState(seed)
    base = np.kron(rng.randint(0, 256, size=(h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w]
    return np.clip(base + rng.randint(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def test_pipeline_resizes_uncropped_images_as_pillow_does():
    from e4s_amd.pipeline import FaceSwapPipeline
    stages = pc.stub_stages()
    src, tgt = _image(300, 260, 1), np.stack([_image(200, 340, 2), _image(200, 340, 3)])
    got = FaceSwapPipeline(*stages, graph=False, any_size=True).swap(_dev(src), _dev(tgt))
    big = lambda a: rc.pillow(a, (1024, 1024), rc.BICUBIC)
    want, _ = pc.compose(stages, _dev(big(src)), _dev(np.stack([big(t) for t in tgt])))
    assert got.shape == (2, 1024, 1024, 3) and torch.equal(got, want)
    with pytest.raises(ValueError):
        FaceSwapPipeline(*stages, graph=False).swap(_dev(src), _dev(tgt))                     # the default keeps refusing


def test_pipeline_with_target_quads_is_unchanged_by_any_size():
    from e4s_amd.pipeline import FaceSwapPipeline
    stages = pc.stub_stages()
    src, tgt = _dev(_image(1024, 1024, 4)), _dev(_image(700, 900, 5)[None])
    tq = ac.square((450.0, 350.0), 300.0, 8.0)[None]
    a = FaceSwapPipeline(*stages, graph=False, any_size=True).swap(src, tgt, target_quads=tq)
    b = FaceSwapPipeline(*stages, graph=False).swap(src, tgt, target_quads=tq)
    assert a.shape == tgt.shape and torch.equal(a, b) and not torch.equal(a, tgt)
