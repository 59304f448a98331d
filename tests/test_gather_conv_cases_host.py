"""The cases of tests/test_gpu_gather_conv_bits.py checked on the CPU (tests/gather_conv_cases.py): the seeded inputs are the ones the
fixture was recorded with, and every case reaches the path its name says."""
import json

import gather_conv_cases as gc

BM = 128


def _fixture():
    with open(gc.FIXTURE) as fh:
        return json.load(fh)


def test_the_seeded_inputs_are_the_recorded_ones():
    """A generator that drifted (another torch, another seed) shows here, on the CPU, and is not read as a changed kernel."""
    fx = _fixture()
    assert sorted(fx) == sorted(gc.cases())
    for name in gc.cases():
        assert gc.input_hashes(name) == fx[name]["inputs"], name
        for precision in gc.PRECISIONS:
            assert sorted(fx[name][precision]) == ["out", "pack"] and all(len(v) == 64 for v in fx[name][precision].values()), name
    # the two precisions pack and compute other bits
    assert all(fx[n]["f32"][k] != fx[n]["bf16x3"][k] for n in fx for k in ("pack", "out"))


def _bn(cout, allowed):
    pad = -(-cout // 32) * 32
    return next(bn for bn in allowed if pad % bn == 0)


def test_every_case_reaches_its_path():
    seen = set()
    for name, (kind, inp, opt) in gc.cases().items():
        cout, cin = inp["w"].shape[:2]
        if kind == "2d":
            b, h, w, _ = inp["x"].shape
            s = opt.get("stride", 1)
            m = b * -(-h // s) * -(-w // s)
            bn = _bn(cout, (128, 64))
        else:
            b, d, h, w = opt["y_shape"][:4]
            m = b * d * h * w
            bn = _bn(cout, (128, 64, 32))
        seen.add((kind, inp["w"].shape[2], bn))
        if "ragged" in name:
            assert m > BM and m % BM
        if "sub_tile" in name:
            assert m < BM
        if "one_tile" in name:
            assert m == BM
        if "bn" in name:
            assert name.endswith(f"bn{bn}")
    assert seen == {("2d", 1, 128), ("2d", 3, 64), ("2d", 3, 128), ("3d", 1, 64), ("3d", 3, 32), ("3d", 3, 128), ("3d", 7, 32)}
    c = gc.cases()
    assert tuple(c["2d_k3_lrelu_nearest_r0_at_y_coff"][1]["r0"].shape[1:3]) == (3, 4)
    assert c["3d_k3_cout15_guarded_stores_bn32"][2]["y_shape"][4] == 15 + 1
    x = c["3d_k3_up2_strided_view"][2]["x_view"](c["3d_k3_up2_strided_view"][1]["x"])
    assert tuple(x.shape) == (2, 4, 3, 5, 64) and not x.is_contiguous() and x.stride(4) == 1
    r = c["3d_k1_strided_res_channel_slice"][2]["res_view"](c["3d_k1_strided_res_channel_slice"][1]["res"])
    assert r.shape[4] == 64 and r.stride(3) == 80 and r.storage_offset() == 8
    assert c["3d_k3_broadcast_batch_bn128"][1]["x"].shape[0] == 1 and c["3d_k3_broadcast_batch_bn128"][2]["y_shape"][0] == 2


def test_the_k7_cases_take_both_sides_of_the_plane_skip():
    # [2,4,8,8]: 64 voxels per plane, a tile is two planes of one sample; tile 0 (planes 0 and 1) leaves kd 0 and 1 out, a whole sample none
    assert gc.skipped_kd_planes(4, 8, 8, 0, 512) == [0, 1]
    assert gc.skipped_kd_planes(4, 8, 8, 128, 512) == [5, 6] and gc.skipped_kd_planes(4, 8, 8, 0, 512, bm=256) == []
    # [3,2,4,4]: a sample is 32 voxels, the one tile spans all three: only what a depth of 2 never reaches is left out, as for a whole
    # sample -- nothing that depends on the tile
    assert 3 * 2 * 4 * 4 < BM
    assert gc.skipped_kd_planes(2, 4, 4, 0, 96) == gc.skipped_kd_planes(2, 4, 4, 0, 32, bm=32) == [0, 1, 5, 6]
    assert gc.skipped_kd_planes(2, 4, 4, 0, 16, bm=16) == [0, 1, 2, 5, 6]                # a tile of plane 0 alone would skip more
