"""StyleLoss off the GPU: the parameter tree, weight loading, the refusals, and the train step's option and term plumbing."""
import os

import pytest
import torch

from e4s_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "style.pt")


@pytest.fixture
def crit(monkeypatch):
    from e4s_amd import criteria
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", True)
    monkeypatch.delenv("E4S_VGG16_WEIGHTS", raising=False)
    return criteria


def test_state_dict_keys_are_the_references(crit):
    rec = torch.load(GOLDEN)
    mod = crit.StyleLoss([3, 8, 15, 22], normalize=True)
    assert list(mod.state_dict()) == rec["state_dict_keys"]
    assert all(not p.requires_grad for p in mod.parameters())


def test_a_torchvision_state_dict_loads_and_unused_entries_are_ignored(crit):
    sd = synth.synth_vgg16_state_dict(seed=3)
    assert all(float(v.abs().max()) > 0 for v in sd.values())                      # the biases too
    tv = dict(sd)
    tv["features.24.weight"] = torch.full((512, 512, 3, 3), 9.0)
    tv["features.24.bias"] = torch.full((512,), 9.0)
    tv["classifier.0.weight"] = torch.zeros(8, 8)
    mod = crit.StyleLoss([3, 8, 15, 22], weights=tv)
    got = mod.state_dict()
    for k, v in sd.items():
        assert torch.equal(got["vgg16_act." + k], v), k
    assert not bool((got["vgg16_act.features.24.weight"] == 9.0).any())
    # a shallower tap list needs fewer entries
    few = {k: v for k, v in sd.items() if int(k.split(".")[1]) < 8}
    crit.StyleLoss([3, 8], weights=few)


def test_a_missing_used_key_is_an_error(crit):
    sd = synth.synth_vgg16_state_dict()
    del sd["features.14.bias"]
    with pytest.raises(KeyError, match="features.14.bias"):
        crit.StyleLoss([3, 8, 15, 22], weights=sd)


def test_no_weights_is_an_error_unless_allowed(monkeypatch):
    from e4s_amd import criteria
    monkeypatch.setattr(criteria, "ALLOW_UNINITIALIZED", False)
    monkeypatch.delenv("E4S_VGG16_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError):
        criteria.StyleLoss([3, 8, 15, 22])


def test_refusals(crit):
    for taps in ([21], [3, 4], [2], [29], [25], []):                   # a conv output (the reference's default), a pool, deeper than 22, none
        with pytest.raises(NotImplementedError):
            crit.StyleLoss(taps)
    with pytest.raises(NotImplementedError, match="l2"):
        crit.StyleLoss([3], distance="l1")
    mod = crit.StyleLoss([3, 8])
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="x_hat"):
        mod(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        mod(x, x, mask_x=torch.ones(1, 1, 8, 8))


class _Fake(torch.nn.Module):
    """a loss module that records the order it is called in"""

    def __init__(self, name, log, value):
        super().__init__()
        self.name, self.log, self.value = name, log, value

    def forward(self, *a, **k):
        self.log.append((self.name, sorted(k)))
        out = torch.tensor(self.value)
        return out if self.name in ("lpips", "style") else (out, None)

    forward_pooled = forward


def _iteration(lo, log, with_style):
    from e4s_amd.train import TrainIteration
    crit = {k: _Fake(k, log, v) for k, v in (("lpips", 0.5), ("id", 0.25), ("parsing", 2.0))}
    if with_style:
        crit["style"] = _Fake("style", log, 4.0)
    return TrainIteration(torch.nn.Linear(2, 2), None, crit, None, None, lo=lo)


def test_loss_opts_and_the_term_list():
    from e4s_amd.train import LossOpts
    lo = LossOpts()
    assert lo.style_lambda == 0 and lo.style_loss_norm == 1
    img, recon = torch.zeros(1, 3, 8, 8), torch.ones(1, 3, 8, 8)
    base_log, log = [], []
    loss0, terms0 = _iteration(LossOpts(), base_log, False).calc_loss(img, recon)
    loss1, terms1 = _iteration(LossOpts(), log, True).calc_loss(img, recon)
    assert list(terms0) == list(terms1) == ["parsing", "id", "l2", "lpips"] and log == base_log      # the default: the same term list as before
    assert torch.equal(loss0, loss1)
    mask = torch.ones(1, 1, 4, 4)
    log = []
    loss2, terms2 = _iteration(LossOpts(style_lambda=2.0), log, True).calc_loss(img, recon, mask=mask)
    assert list(terms2) == ["parsing", "id", "l2", "lpips", "style"] and log[-1] == ("style", ["mask_x", "mask_x_hat"])
    assert float(loss2) == float(loss0) + 2.0 * 4.0
    with pytest.raises(RuntimeError, match="mask"):
        _iteration(LossOpts(style_lambda=2.0), [], True).calc_loss(img, recon)
    assert "style" not in _iteration(LossOpts(style_lambda=2.0), [], False).calc_loss(img, recon)[1]
