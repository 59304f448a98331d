"""CPU: layer-level checks of the oracle restatement against the REAL reference modules on shapes the golden fixtures of
tests/test_oracle_golden.py do not cover.  The reference's results are recorded in tests/golden/refchecks.pt and
tests/golden/w_norm.pt (tests/golden/make_reference_checks.py, run where the reference tree exists)."""
import pytest
import torch

from e4s_amd import synth
from oracle import e4s_oracle as orc


@pytest.fixture(scope="module")
def refchecks(golden):
    return golden("refchecks.pt")


@pytest.mark.parametrize("cin,cout,up", [(16, 24, False), (16, 8, True)])
@torch.no_grad()
def test_styled_conv_masked_matches_reference_module(refchecks, cin, cout, up):
    case = [c for c in refchecks["styled_conv"] if (c["cin"], c["cout"], c["up"]) == (cin, cout, up)]
    assert len(case) == 1
    c = case[0]
    mask = synth.onehot(synth.synth_labels_blocks(2, 64, 8, seed=1))
    got = orc.styled_conv(c["sd"], "", c["x"], c["style"], mask, c["noise"], up, True)
    assert got.shape == c["want"].shape
    assert float((got - c["want"]).abs().max()) < 1e-5


@torch.no_grad()
def test_torgb_matches_reference_module(refchecks):
    c = refchecks["torgb"]
    mask = synth.onehot(synth.synth_labels_blocks(2, 64, 8, seed=2))
    got = orc.to_rgb(c["sd"], "", c["x"], c["style"], mask, c["skip"], True)
    assert got.shape == c["want"].shape
    assert float((got - c["want"]).abs().max()) < 1e-5


def test_w_norm_loss_matches_reference_class(refchecks, golden):
    """train.w_norm_loss == src/criteria/w_norm.py:WNormLoss, value and gradient."""
    from e4s_amd.train import w_norm_loss
    rec = golden("w_norm.pt")
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(2, 12, 18, 512, generator=g, requires_grad=True)
    avg = torch.randn(18, 512, generator=g)
    # the latent is redrawn from its seed: it must be the one the recorded gradient belongs to
    assert abs(float(lat.detach().double().sum()) - rec["lat_sum"]) < 1e-6 * rec["lat_abs_sum"]
    assert torch.equal(avg, rec["avg"])
    for flag in (True, False):
        a = w_norm_loss(lat, avg, flag)
        b = refchecks["w_norm_value"][flag]
        assert float((a - b).abs()) < 1e-5 * float(b.abs())
    a.backward()
    assert torch.allclose(lat.grad, rec["grad"])


def test_reference_itself_fails_on_the_branches_net3_refuses(refchecks):
    """e4s_amd.networks.Net3.cal_style_codes raises NotImplementedError for start_from_latent_avg=False and learn_in_w=True; so does the
    reference, less politely (networks.py:145-158: `style_codes` is never assigned; a [bs,R,512] tensor is added to [bs,R,K,512] codes)."""
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    assert refchecks["net3_errors"] == {"start_from_latent_avg=False": "UnboundLocalError", "learn_in_w=True": "RuntimeError"}
    sd = synth.synth_state_dict(256, 13)
    lat = synth.synth_latent_avg(256)
    net = Net3(make_opts(out_size=256))
    net.load_state_dict(sd, strict=True)
    net.latent_avg = lat
    sv = torch.randn(1, 12, 1280)
    net.opts.start_from_latent_avg = False
    with pytest.raises(NotImplementedError):
        net.cal_style_codes(sv)
    net.opts.start_from_latent_avg, net.opts.learn_in_w = True, True
    net.latent_avg = lat[:1].repeat(1, 1)                 # coach.py:118-119
    with pytest.raises(NotImplementedError):
        net.cal_style_codes(sv)
