"""Host-side checks of face-vid2vid's SPADE decoder (e4s_amd/spade.py): the parameter trees against the reference's recorded key
lists (tests/golden/spade.pt, tests/golden/reenact_warp.pt), the spectral-norm fold against the reference module's recorded effective
weights, strict loading, the host re-ordering of the packs against plain fp64 convs, the refusals and the synthetic weights.  No GPU."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from e4s_amd import synth

SMALL_GEN = dict(image_channel=3, feature_channel=32, num_kp=15, block_expansion=64, max_features=256, num_down_blocks=2, reshape_channel=32,
                 reshape_depth=8, num_resblocks=1, estimate_occlusion_map=True,
                 dense_motion_params=dict(block_expansion=32, max_features=128, num_blocks=2, reshape_depth=8, compress=4))
_STATE = {}


@pytest.fixture(scope="module")
def g(golden):
    return golden("spade.pt")


def _decoder(g):
    from e4s_amd import spade
    if "dec" not in _STATE:
        dec = spade.SPADEDecoder()
        sd = synth.synth_vid2vid_decoder_state_dict(dec, seed=g["dec_seed"])
        dec.load_state_dict(sd, strict=True)
        _STATE["dec"], _STATE["sd"] = dec, sd
    return _STATE["dec"], _STATE["sd"]


def _generator_sd(gen, seed=3):
    sd = synth.synth_vid2vid_generator_state_dict(gen, seed=seed)
    sd.update({"decoder." + k: v for k, v in synth.synth_vid2vid_decoder_state_dict(gen.decoder, seed=seed).items()})
    return sd


def test_parameter_trees_are_the_references(g, golden):
    from e4s_amd import spade
    w = golden("reenact_warp.pt")
    with torch.device("meta"):
        dec = spade.SPADEDecoder()
        gen = spade.OcclusionAwareSPADEGenerator(**w["gen_shipped"])
    assert list(dec.state_dict().keys()) == g["dec.keys"]
    assert [tuple(v.shape) for v in dec.state_dict().values()] == g["dec.shapes"]
    assert list(gen.state_dict().keys()) == w["gen.keys"]
    assert [tuple(v.shape) for v in gen.state_dict().values()] == w["gen.shapes"]
    assert [k for k in w["gen.keys"] if k.startswith("decoder.")] == ["decoder." + k for k in g["dec.keys"]]
    params, buffers = dict(dec.named_parameters()), dict(dec.named_buffers())
    assert "G_middle_0.conv_0.weight_orig" in params and "G_middle_0.conv_0.weight" not in params
    assert "G_middle_0.conv_0.weight_u" in buffers and "G_middle_0.conv_0.weight_v" in buffers
    assert "up_1.conv_s.weight_orig" in params and "up_1.conv_s.bias" not in params


def test_spectral_weight_matches_the_reference_modules_effective_weight(g):
    from e4s_amd import spade
    dec, _ = _decoder(g)
    cs = dec.up_1.conv_s
    got = spade.spectral_weight(cs.weight_orig, cs.weight_u, cs.weight_v)
    assert got.dtype == torch.float64 and tuple(got.shape) == (64, 256, 1, 1)
    assert float((got - g["weight.up_1.conv_s"]).abs().max()) <= 1e-12
    c0 = dec.G_middle_0.conv_0
    got = spade.spectral_weight(c0.weight_orig, c0.weight_u, c0.weight_v).reshape(512, -1)
    ref = g["weight.G_middle_0.conv_0"]
    sub = got[::g["weight.G_middle_0.conv_0.rows"], ::g["weight.G_middle_0.conv_0.cols"]]
    assert sub.shape == ref.shape and float(ref.abs().max()) > 1e-3
    assert float((sub - ref).abs().max()) <= 1e-12
    # the fold is not a no-op, and is not the division by the true norm either
    assert float((got - c0.weight_orig.detach().double().reshape(512, -1)).abs().max()) > 1e-4
    for name in ("up_0", "up_1"):
        conv = getattr(dec, name).conv_s
        wm = conv.weight_orig.detach().double().reshape(conv.out_channels, -1)
        ratio = float(torch.dot(conv.weight_u.double(), torch.mv(wm, conv.weight_v.double())) / torch.linalg.matrix_norm(wm, 2))
        assert abs(ratio - g[f"sigma_ratio.{name}"]) <= 1e-6 and 0.7 <= ratio < 1.0


def test_strict_loading_names_missing_and_unexpected_keys_and_feature_warp_still_ignores_the_decoder():
    from e4s_amd import reenact_warp as rw, spade
    gen = spade.OcclusionAwareSPADEGenerator(**SMALL_GEN)
    sd = _generator_sd(gen)
    assert list(sd.keys()) == list(gen.state_dict().keys())
    gen.load_generator_state_dict(sd)
    assert gen._weights_loaded and gen.decoder._weights_loaded and gen.dense_motion_network._weights_loaded
    assert torch.equal(gen.decoder.up_0.conv_s.weight_u, sd["decoder.up_0.conv_s.weight_u"])
    missing = {k: v for k, v in sd.items() if k != "decoder.up_0.norm_s.mlp_gamma.weight"}
    with pytest.raises(RuntimeError, match=r"decoder\.up_0\.norm_s\.mlp_gamma\.weight"):
        gen.load_generator_state_dict(missing)
    extra = dict(sd)
    extra["decoder.G_middle_6.conv_0.bias"] = torch.zeros(512)
    with pytest.raises(RuntimeError, match=r"decoder\.G_middle_6\.conv_0\.bias"):
        gen.load_generator_state_dict(extra)
    no_decoder = {k: v for k, v in sd.items() if not k.startswith("decoder.")}
    with pytest.raises(RuntimeError, match=r"decoder\.fc\.weight"):
        gen.load_generator_state_dict(no_decoder)
    fw = rw.FeatureWarp(**SMALL_GEN)
    assert not any(k.startswith("decoder.") for k in fw.state_dict())
    fw.load_generator_state_dict(sd)                                        # the decoder.* entries are ignored, as before
    fw.load_generator_state_dict(no_decoder)
    assert torch.equal(fw.fourth.weight, gen.fourth.weight)


def test_gamma_beta_interleave_and_shared_concatenation_against_plain_fp64_convs(g):
    from e4s_amd import spade
    dec, _ = _decoder(g)
    gen = torch.Generator().manual_seed(5)
    sp = dec.up_1.norm_1                                                    # C = 64
    a = torch.randn(2, 128, 5, 4, generator=gen, dtype=torch.float64)
    w = spade.interleave_gamma_beta(sp.mlp_gamma.weight.detach(), sp.mlp_beta.weight.detach())
    b = spade.interleave_gamma_beta(sp.mlp_gamma.bias.detach(), sp.mlp_beta.bias.detach())
    assert tuple(w.shape) == (128, 128, 3, 3) and tuple(b.shape) == (128,)
    both = F.conv2d(a, w.double(), b.double(), padding=1)
    gamma = F.conv2d(a, sp.mlp_gamma.weight.double(), sp.mlp_gamma.bias.double(), padding=1)
    beta = F.conv2d(a, sp.mlp_beta.weight.double(), sp.mlp_beta.bias.double(), padding=1)
    assert float(gamma.abs().max()) > 0.1 and float((gamma - beta).abs().max()) > 0.1
    assert float((both[:, 0::2] - gamma).abs().max()) <= 1e-13 and float((both[:, 1::2] - beta).abs().max()) <= 1e-13
    assert torch.equal(w[6], sp.mlp_gamma.weight[3]) and torch.equal(w[7], sp.mlp_beta.weight[3])
    with pytest.raises(ValueError):
        spade.interleave_gamma_beta(torch.zeros(4, 2), torch.zeros(5, 2))
    # the concatenated mlp_shared rows: SPADE i owns channels 128 i .. 128 i + 127, in the order of the block's spades()
    spades = dec.up_0.spades()
    assert spades == [dec.up_0.norm_0, dec.up_0.norm_1, dec.up_0.norm_s] and dec.G_middle_2.spades() == [dec.G_middle_2.norm_0, dec.G_middle_2.norm_1]
    wc, bc = spade.concat_shared(spades)
    assert tuple(wc.shape) == (384, 256, 3, 3) and tuple(bc.shape) == (384,)
    seg = torch.randn(1, 256, 4, 3, generator=gen, dtype=torch.float64)
    cat = F.relu(F.conv2d(seg, wc.double(), bc.double(), padding=1))
    for i, s in enumerate(spades):
        conv = s.mlp_shared[0]
        one = F.relu(F.conv2d(seg, conv.weight.double(), conv.bias.double(), padding=1))
        assert float(one.abs().max()) > 0.1 and float((cat[:, 128 * i:128 * (i + 1)] - one).abs().max()) <= 1e-13, i
    stages = dec.stages()
    assert [s for s, _ in stages] == [0, 1, 2] and [len(b) for _, b in stages] == [6, 1, 1]
    assert sum(len(blk.spades()) for _, blk in stages[0][1]) == 12


def test_refusals(g, monkeypatch):
    from e4s_amd import criteria, spade
    dec, _ = _decoder(g)
    assert not dec.training and not dec.G_middle_0.training
    with pytest.raises(RuntimeError, match="train"):
        dec.train()
    assert dec.eval() is dec
    with pytest.raises(NotImplementedError, match="run"):
        dec(torch.zeros(1, 256, 2, 2))
    with pytest.raises(RuntimeError, match="device tensor"):
        dec.run(torch.zeros(1, 256, 2, 2))                                  # no CPU path
    narrow = dict(SMALL_GEN, block_expansion=32, max_features=128, reshape_depth=4,
                  dense_motion_params=dict(SMALL_GEN["dense_motion_params"], reshape_depth=4))
    with pytest.raises(NotImplementedError, match="OcclusionAwareSPADEGenerator.*128.*256"):
        spade.OcclusionAwareSPADEGenerator(**narrow)
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    fresh = spade.SPADEDecoder()
    with pytest.raises(RuntimeError, match="no weights were loaded"):
        fresh.run(torch.zeros(1, 256, 2, 2))
    with pytest.raises(TypeError):
        spade.Reenactor(object(), object())


def test_synthetic_decoder_weights_are_chosen_by_key_and_shape(g):
    dec, sd = _decoder(g)

    class Holder(nn.Module):                                                # another module with the same keys and shapes
        def __init__(self):
            super().__init__()
            for i, (k, shape) in enumerate(zip(g["dec.keys"], g["dec.shapes"])):
                self.register_buffer(f"t{i}", torch.empty(shape, device="meta"), persistent=True)

        def state_dict(self, *a, **kw):
            return {k: getattr(self, f"t{i}") for i, k in enumerate(g["dec.keys"])}

    other = synth.synth_vid2vid_decoder_state_dict(Holder(), seed=g["dec_seed"])
    assert list(other.keys()) == list(sd.keys()) and all(torch.equal(other[k], sd[k]) for k in sd)
    again = synth.synth_vid2vid_decoder_state_dict(dec, seed=g["dec_seed"] + 1)
    assert not torch.equal(again["fc.weight"], sd["fc.weight"])
    for k in sd:
        if k.endswith(("weight_u", "weight_v")):
            assert abs(float(sd[k].double().norm()) - 1.0) <= 1e-6, k
    w = sd["G_middle_1.conv_1.weight_orig"]
    assert abs(float(w.std()) * (512 * 9) ** 0.5 - 1.0) < 0.05             # fan-in scaled
    x = synth.synth_vid2vid_decoder_feature(2, 3, 4, 7)
    assert tuple(x.shape) == (2, 256, 3, 4) and not torch.equal(x[0], x[1]) and torch.equal(x, synth.synth_vid2vid_decoder_feature(2, 3, 4, 7))
