"""GPU tests of e4s_amd.resize.pil_resize (csrc/resize.hip) against live Pillow: every byte equal, no tolerance.

Shapes: the case list of tests/pil_resize_cases.py (up, down, one axis only, a 0/255 image for the overshoot of the negative lobes,
5 x 7 -> 3 x 11, the identity) x five filters x {no box, a fractional box}; a batch of three; 300 x 500 <-> 257 x 129, which
takes several tiles of both kernels and ends all of them raggedly; windows of that result; out=; a captured graph."""
import functools

import numpy as np
import pytest
import torch

import pil_resize_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} bytes differ from Pillow, largest difference " \
                     f"{int(np.abs(got.astype(int) - want.astype(int)).max())}"


@functools.lru_cache(maxsize=None)
def _ragged(i, resample):
    """(image, Pillow's result) of a RAGGED case, computed once."""
    in_wh, size = pc.RAGGED[i]
    img = pc.image("ragged", *in_wh, seed=i)
    return img, pc.pillow(img, size, resample)


@pytest.mark.parametrize("name,in_wh,size", pc.CASES, ids=[c[0] for c in pc.CASES])
def test_equals_live_pillow(name, in_wh, size):
    from e4s_amd import resize
    img = pc.image(name, *in_wh)
    x = _dev(img)
    for resample in pc.FILTERS:
        for box in (None, pc.fractional_box(*in_wh)):
            got = resize.pil_resize(x[None], size, int(resample), box=box)
            assert got.shape == (1, size[1], size[0], 3)
            _same(got[0], pc.pillow(img, size, resample, box), (name, int(resample), box))
    _same(resize.pil_resize(x, size), pc.pillow(img, size, pc.BICUBIC), (name, "[H,W,3], default filter"))


@pytest.mark.parametrize("in_wh,size", [pc.CASES[0][1:], pc.CASES[5][1:]], ids=["up", "down4"])
def test_batch_of_distinct_images(in_wh, size):
    from e4s_amd import resize
    imgs = np.stack([pc.image("batch", *in_wh, seed=s) for s in (1, 2, 3)])
    assert not np.array_equal(imgs[0], imgs[1])
    for resample in (pc.BICUBIC, pc.LANCZOS):
        got = resize.pil_resize(_dev(imgs), size, int(resample))
        for i in range(3):
            _same(got[i], pc.pillow(imgs[i], size, resample), (in_wh, size, int(resample), i))


@pytest.mark.parametrize("resample", [pc.BICUBIC, pc.LANCZOS], ids=["bicubic", "lanczos"])
@pytest.mark.parametrize("i", [0, 1], ids=["down", "up"])
def test_several_ragged_tiles(i, resample):
    from e4s_amd import resize
    img, want = _ragged(i, resample)
    _same(resize.pil_resize(_dev(img), pc.RAGGED[i][1], int(resample)), want, (pc.RAGGED[i], int(resample)))


def test_window_is_a_slice_of_the_full_result():
    from e4s_amd import resize
    (w, h) = pc.RAGGED[0][1]
    for resample in (pc.BICUBIC, pc.LANCZOS):
        img, want = _ragged(0, resample)
        x = _dev(img)
        for win in ((0, 0, w, h), (41, 17, 170, 90), (130, 60, w, h), (200, 100, 201, 101), (0, h - 1, w, h)):
            got = resize.pil_resize(x, (w, h), int(resample), window=win)
            _same(got, want[win[1]:win[3], win[0]:win[2]], (int(resample), win))
        got = resize.pil_resize(x, (w, h), int(resample), box=pc.fractional_box(*pc.RAGGED[0][0]), window=(33, 9, 140, 77))
        _same(got, pc.pillow(img, (w, h), resample, pc.fractional_box(*pc.RAGGED[0][0]))[9:77, 33:140], (int(resample), "box + window"))
    for win in ((0, 0, w + 1, h), (-1, 0, 5, 5), (5, 5, 5, 9), (0, 0, w, h + 1)):
        with pytest.raises(ValueError):
            resize.pil_resize(x, (w, h), window=win)


def test_out_and_refusals():
    from e4s_amd import resize
    in_wh, size = pc.CASES[0][1:]
    img = pc.image("up", *in_wh)
    x, want = _dev(img), pc.pillow(img, size, pc.BICUBIC)
    out = torch.full((1, size[1], size[0], 3), 9, dtype=torch.uint8, device=DEV)
    got = resize.pil_resize(x[None], size, out=out)
    assert got.data_ptr() == out.data_ptr()
    _same(out[0], want, "out=")
    sentinel = out.clone()
    for bad_out in (out.float(), out[:, :-1].contiguous(), out.cpu(), out[0]):
        with pytest.raises((ValueError, RuntimeError)):
            resize.pil_resize(x[None], size, out=bad_out)
    with pytest.raises(RuntimeError):
        resize.pil_resize(x.cpu(), size, out=out)
    with pytest.raises(ValueError):
        resize.pil_resize(x, size, resize.NEAREST, out=out[0])
    with pytest.raises(RuntimeError):
        resize.pil_resize(x[:, ::2], size, out=out[0])                          # not contiguous
    with pytest.raises(ValueError):
        resize.pil_resize(x.float(), size, out=out[0])
    with pytest.raises(ValueError):
        resize.pil_resize(x[..., :2].contiguous(), size, out=out[0])
    with pytest.raises(ValueError):
        resize.pil_resize(x, (0, 5))
    with pytest.raises(ValueError):
        resize.pil_resize(x, size, box=(0, 0, in_wh[0] + 1, in_wh[1]), out=out[0])
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel), "a refused call wrote to out"


def test_captured_graph_replays_on_new_pixels():
    from e4s_amd import resize
    in_wh, size = pc.RAGGED[0]
    first, second = pc.image("graph", *in_wh, seed=5), pc.image("graph", *in_wh, seed=6)
    x = _dev(first)[None].clone()
    out = torch.zeros(1, size[1], size[0], 3, dtype=torch.uint8, device=DEV)
    resize.pil_resize(x, size, resize.LANCZOS, out=out)                         # the eager call uploads the tables
    _same(out[0], pc.pillow(first, size, pc.LANCZOS), "eager")
    cached = len(resize._cache)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):                                               # one chain on the capture stream, no side stream
        resize.pil_resize(x, size, resize.LANCZOS, out=out)
    assert len(resize._cache) == cached, "the captured call built tables again"
    x.copy_(_dev(second)[None])
    graph.replay()
    torch.cuda.synchronize()
    _same(out[0], pc.pillow(second, size, pc.LANCZOS), "replay on new pixels")
