"""GPU tests of e4s_amd.align (csrc/align.hip): the aligned crop out of a frame and the paste back into it, against live Pillow --
the reference's own method (src/utils/alignmengt.py: crop_image; scripts/face_swap.py:313-327).

Bounds, per image and with no pixel excluded: no level difference above 1 and at most 1e-4 of the pixels unequal.  The float64
numpy statement of Pillow's arithmetic (tests/align_cases.py) scores exactly 0 on these inputs -- asserted here as well, so the cap
cannot hide a broken yardstick -- while float32 coordinates leave 1e-4 .. 6e-4 of the pixels off by one
(tests/test_align_host.py::test_float32_coordinates_would_not_pass).

Shapes: frames [3,271,483,3] (odd H; W * 3 = 1 mod 4, so the rows start at every byte alignment and the 4-pixel groups end in a
ragged edge), S = 128, three quads (interior and turned 30 deg, down-scaling | up-scaling | ~40 % beyond the frame's corner); S = 125 for
the crop's own ragged edge; and the pipeline's S = 1024 on one 1080 x 1920 frame."""
import numpy as np
import pytest
import torch

import align_cases as ac
from conftest import unz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _within_bounds(got, want, what):
    """The issue's two bounds for every image of a batch; prints the figures first."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    for i, (g, w) in enumerate(zip(got, want)):
        levels, share = ac.score(g, w)
        print(f"{what}[{i}]: max level difference {levels}, share of unequal pixels {share:.3e}")
        assert levels <= ac.MAX_LEVELS and share <= ac.MAX_SHARE, (what, i, levels, share)


class Case:
    """Frames, quads, faces and what live Pillow makes of them -- computed once per shape and never modified."""

    def __init__(self, hw, size, quads, seed):
        self.size, self.quads = size, quads
        self.frames = ac.frames(len(quads), *hw, seed=seed)
        self.faces = ac.frames(len(quads), size, size, seed=seed + 1)
        self.crops, self.pasted, self.alpha, self.inv = [], [], [], []
        for frame, face, quad in zip(self.frames, self.faces, quads):
            crop, sub, passed = ac.pil_crop(frame, quad, size)
            assert np.array_equal(ac.quad_warp(sub, passed, size)[0], crop), "the restatement must score 0 against Pillow"
            coeffs = ac.inverse_coefficients(quad, size)
            pasted, alpha = ac.pil_paste(face, frame, coeffs)
            got, valid = ac.perspective_warp(face, coeffs, hw[1], hw[0])
            assert np.array_equal(np.where(valid[..., None], got, frame), pasted), "the restatement must score 0 against Pillow"
            assert np.array_equal(valid, alpha == 255)
            self.crops.append(crop), self.pasted.append(pasted), self.alpha.append(alpha), self.inv.append(coeffs)


@pytest.fixture(scope="module")
def small():
    return Case(ac.SMALL_HW, ac.SMALL_S, ac.SMALL_QUADS, seed=0)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("align.pt")


def test_crop_matches_pillow_and_normalised_output_is_its_own_crop(small):
    from e4s_amd import align
    frames = _dev(small.frames)
    crop, norm = align.crop_faces_by_quads(frames, small.quads, small.size, normalized=True)
    torch.cuda.synchronize()
    assert crop.dtype == torch.uint8 and tuple(crop.shape) == (3, small.size, small.size, 3)
    _within_bounds(crop, small.crops, "crop")
    assert float((crop[2].sum(-1) == 0).float().mean()) > 0.3                     # the corner quad: outside the frame is 0
    # ToTensor + Normalize on the CPU (a true division by 255, as the reference's), of the kernel's own uint8 crop: bit-equal
    want = ((crop.cpu().float() / 255) - 0.5) / 0.5
    assert norm.dtype == torch.float32 and torch.equal(norm.cpu(), want.permute(0, 3, 1, 2))
    assert torch.equal(align.crop_faces_by_quads(frames, small.quads, small.size), crop)      # the same without the second output


def test_crop_at_an_odd_size(small):
    """S = 125: S * 3 is odd, the 4-pixel groups end in a single pixel and the fp32 rows are not 16-byte aligned."""
    from e4s_amd import align
    s = 125
    want = [ac.pil_crop(f, q, s)[0] for f, q in zip(small.frames, small.quads)]
    guard = torch.full((3 * s * s * 3 + 64,), 77, device=DEV, dtype=torch.uint8)
    out = guard[:3 * s * s * 3].view(3, s, s, 3)
    coeffs, windows = align.crop_parameters(small.quads, ac.SMALL_HW, s)
    crop, norm = align.crop_faces_by_coeffs(_dev(small.frames), _dev(coeffs), _dev(windows), s, normalized=True, out=out)
    torch.cuda.synchronize()
    _within_bounds(crop, want, "crop125")
    assert bool((guard[3 * s * s * 3:] == 77).all())                               # nothing written past the last pixel
    assert torch.equal(norm.cpu(), (((crop.cpu().float() / 255) - 0.5) / 0.5).permute(0, 3, 1, 2))


def test_paste_back_matches_pillow(small):
    from e4s_amd import align
    frames, faces = _dev(small.frames), _dev(small.faces)
    before = frames.clone()
    out = align.paste_back(faces, frames, small.quads)
    torch.cuda.synchronize()
    assert torch.equal(frames, before) and out.data_ptr() != frames.data_ptr()
    _within_bounds(out, small.pasted, "paste")
    got = out.cpu().numpy()
    for i in range(3):                                   # where the back-projection misses the face: the frame's own bits
        outside = small.alpha[i] == 0
        assert 0.05 < outside.mean() < 1.0
        assert np.array_equal(got[i][outside], small.frames[i][outside])
        assert not np.array_equal(got[i][~outside], small.frames[i][~outside])
    inplace = align.paste_back(faces, frames, small.quads, out=frames)
    torch.cuda.synchronize()
    assert inplace is frames and torch.equal(frames, out)
    assert torch.equal(align.swap_into_frames(faces, before, small.quads), out)


def test_fixture_of_the_reference(fx):
    """The crop and the pasted frame the reference's own crop_image / paste-back lines produced (make_align_golden.py)."""
    from e4s_amd import align
    frame, crop, pasted = (unz(fx[k]) for k in ("frame", "crop", "pasted"))
    quad, s = fx["quad"].numpy(), fx["size"]
    frames = frame[None].to(DEV)
    got = align.crop_faces_by_quads(frames, quad, s)
    _within_bounds(got, crop[None].numpy(), "fixture crop")
    face = (255 - crop)[None].to(DEV)
    _within_bounds(align.paste_back(face, frames, quad, size=s), pasted[None].numpy(), "fixture paste")
    # and through the stored coefficients, on tensors that are already on the device
    win = torch.tensor([fx["window"]], dtype=torch.int32, device=DEV)
    got = align.crop_faces_by_coeffs(frames, fx["quad_coeffs"][None].to(DEV), win, s)
    _within_bounds(got, crop[None].numpy(), "fixture crop (coefficients)")
    got = align.paste_back_by_coeffs(face, frames, fx["inv_coeffs"][None].to(DEV))
    _within_bounds(got, pasted[None].numpy(), "fixture paste (coefficients)")


def test_chain_crop_modify_paste(small):
    """crop -> invert the face -> paste back: the link postproc.stitch -> paste_back forms, against the same chain in Pillow."""
    from e4s_amd import align
    frames = _dev(small.frames)
    face = 255 - align.crop_faces_by_quads(frames, small.quads, small.size)
    out = align.paste_back(face, frames, small.quads)
    torch.cuda.synchronize()
    want = [ac.pil_paste(255 - crop, frame, inv)[0] for crop, frame, inv in zip(small.crops, small.frames, small.inv)]
    _within_bounds(out, want, "chain")


def test_pipeline_size_on_a_1080p_frame():
    from e4s_amd import align
    case = Case(ac.LARGE_HW, ac.LARGE_S, ac.LARGE_QUAD, seed=3)
    frames = _dev(case.frames)
    crop, norm = align.crop_faces_by_quads(frames, case.quads, normalized=True)                 # size defaults to 1024
    _within_bounds(crop, case.crops, "crop1024")
    assert torch.equal(norm.cpu(), (((crop.cpu().float() / 255) - 0.5) / 0.5).permute(0, 3, 1, 2))
    out = align.paste_back(_dev(case.faces), frames, case.quads, out=frames)
    _within_bounds(out, case.pasted, "paste1080p")


def test_graph_capture_replays_with_new_frames_and_quads(small):
    """One capture of crop + paste with device-resident coefficients; frames and coefficients overwritten in place; the replay
    equals the eager result for the second set bit for bit.  One linear graph on the capturing stream."""
    from e4s_amd import align
    s, hw = small.size, ac.SMALL_HW
    second_frames = _dev(ac.frames(3, *hw, seed=9))

    def tables(quads):
        coeffs, windows = align.crop_parameters(quads, hw, s)
        return _dev(coeffs), _dev(windows), _dev(align.paste_parameters(quads, s))

    def run(frames, qc, win, pc):
        face = 255 - align.crop_faces_by_coeffs(frames, qc, win, s)
        return face, align.paste_back_by_coeffs(face, frames, pc)

    eager = run(second_frames, *tables(ac.SECOND_QUADS))
    frames, (qc, win, pc) = _dev(small.frames), tables(small.quads)
    first = run(frames, qc, win, pc)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        face, out = run(frames, qc, win, pc)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(face, first[0]) and torch.equal(out, first[1])
    frames.copy_(second_frames)
    for dst, src in zip((qc, win, pc), tables(ac.SECOND_QUADS)):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, first[1])
    assert torch.equal(face, eager[0]) and torch.equal(out, eager[1])


def test_error_paths_raise_before_any_launch(small):
    from e4s_amd import align
    frames, faces = _dev(small.frames), _dev(small.faces)
    coeffs, windows = align.crop_parameters(small.quads, ac.SMALL_HW, small.size)
    qc, win, pc = _dev(coeffs), _dev(windows), _dev(align.paste_parameters(small.quads, small.size))
    bad = [
        lambda: align.crop_faces_by_quads(frames.float(), small.quads, small.size),                       # dtype
        lambda: align.crop_faces_by_quads(frames.permute(0, 2, 1, 3), small.quads, small.size),            # not contiguous
        lambda: align.crop_faces_by_quads(frames, small.quads[:2], small.size),                            # B mismatch
        lambda: align.crop_faces_by_coeffs(frames, qc.float(), win, small.size),
        lambda: align.crop_faces_by_coeffs(frames, qc, win.long(), small.size),
        lambda: align.crop_faces_by_coeffs(frames, qc[:2], win, small.size),
        lambda: align.crop_faces_by_coeffs(frames, qc.t().contiguous().t(), win, small.size),
        lambda: align.crop_faces_by_coeffs(frames, qc, win, small.size, out_normalized=torch.empty(3, 3, 128, 128, device=DEV, dtype=torch.float64)),
        lambda: align.paste_back(faces.float(), frames, small.quads),
        lambda: align.paste_back(faces, frames[:, :, ::2], small.quads),
        lambda: align.paste_back(faces[:2], frames, small.quads[:2]),
        lambda: align.paste_back(faces, frames, small.quads[:2]),
        lambda: align.paste_back(faces, frames, small.quads, size=256),
        lambda: align.paste_back_by_coeffs(faces, frames, pc.float()),
        lambda: align.paste_back_by_coeffs(faces, frames, pc, out=torch.empty(3, 271, 480, 3, device=DEV, dtype=torch.uint8)),
        lambda: align.paste_back_by_coeffs(faces, frames.cpu(), pc),
    ]
    before = frames.clone()
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"case {i} did not raise")
    torch.cuda.synchronize()
    assert torch.equal(frames, before)
