"""Host-side checks of the Ranger optimiser (e4s_amd/optim.py:Ranger; no GPU): the pure-Python restatement of the reference's
rectification coefficients against the values recorded from its formulas (tests/golden/make_ranger_golden.py), the row geometry of the
gradient centralisation, the drop-in import path `src.training.ranger`, configure_optimizers, and the constructor's checks."""
import importlib
import importlib.util
import math
import os

import pytest
import torch


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ranger.pt")


def test_radam_coefficients_match_the_recorded_steps(fx):
    from e4s_amd.optim import Ranger
    assert [r[0] for r in fx["radam"]] == list(range(1, 21))
    for step, n_sma, step_size, adaptive in fx["radam"]:
        got = Ranger.radam_coefficients(step, 0.95, 0.999, 5)
        assert abs(got[0] - n_sma) <= 1e-14 * abs(n_sma), step
        assert abs(got[1] - step_size) <= 1e-14 * abs(step_size), step
        assert got[2] is adaptive, step
    # defaults: steps 1-5 take the momentum-only branch, step 6 (N_sma 5.994) is the first adaptive one
    assert [Ranger.radam_coefficients(s, 0.95, 0.999, 5)[2] for s in range(1, 8)] == [False] * 5 + [True] * 2
    assert abs(Ranger.radam_coefficients(6, 0.95, 0.999, 5)[0] - 5.994) < 1e-3
    assert Ranger.radam_coefficients(3, 0.95, 0.999, 5)[1] == 1.0 / (1 - 0.95 ** 3)


def test_gc_rows_on_the_fixture_shapes(fx):
    from e4s_amd.optim import Ranger
    want = {(1, 8, 6, 3, 3): (1, 432), (1, 37, 33, 3, 3): (1, 10989), (5, 7): (5, 7), (9, 4099): (9, 4099), (3, 4096): (3, 4096),
            (513, 27): (513, 27), (6, 1): (6, 1), (1, 3, 1, 1): (1, 3), (3,): None, (1,): None, (4097,): None, (64, 64, 3, 3): (64, 576)}
    assert set(want) == {tuple(s) for s in fx["shapes"]}
    for shape in fx["shapes"]:
        shape = tuple(shape)
        assert Ranger.gc_rows(shape) == want[shape], shape
        assert Ranger.gc_rows(torch.Size(shape), gc_conv_only=True) == (want[shape] if len(shape) > 3 else None), shape
    assert Ranger.gc_rows((0, 4)) is None and Ranger.gc_rows((4, 0, 2)) is None


def test_src_training_ranger_is_the_native_class():
    from e4s_amd import optim
    from src.training.ranger import Ranger
    import src.training
    from src import _overlay
    assert Ranger is optim.Ranger
    assert issubclass(Ranger, torch.optim.Optimizer)
    ref = _overlay.reference_src()
    if ref is not None:                  # with a reference checkout every other module of the package resolves there
        assert os.path.join(ref, "training") in list(src.training.__path__)
        spec = importlib.util.find_spec("src.training.coach")
        assert spec is not None and os.path.dirname(spec.origin) == os.path.join(ref, "training")
    else:
        assert len(list(src.training.__path__)) == 1
    assert os.path.dirname(importlib.import_module("src.training.ranger").__file__) == list(src.training.__path__)[0]


def test_configure_optimizers_mirrors_the_coach():
    from e4s_amd.optim import FusedAdam, Ranger
    from e4s_amd.train import configure_optimizers
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    disc = torch.nn.Linear(5, 1)
    net[1].bias.requires_grad_(False)
    for name, cls in (("adam", FusedAdam), ("ranger", Ranger), ("anything else", Ranger)):
        for d_reg_every, ratio in ((-1, 1.0), (16, 16 / 17)):
            opt, opt_d = configure_optimizers(net, disc, optim_name=name, learning_rate=2e-4, train_D=True, d_reg_every=d_reg_every)
            assert type(opt) is cls and type(opt_d) is cls
            assert opt.capturable and opt_d.capturable
            assert opt.param_groups[0]["lr"] == 2e-4
            assert opt_d.param_groups[0]["lr"] == 2e-4 * ratio
            assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in net.parameters() if p.requires_grad]
            assert len(opt.param_groups[0]["params"]) == 3
            assert [id(p) for p in opt_d.param_groups[0]["params"]] == [id(p) for p in disc.parameters()]
        opt, opt_d = configure_optimizers(net, disc, optim_name=name, train_D=False)
        assert type(opt) is cls and opt_d is None and opt.param_groups[0]["lr"] == 1e-4


def test_constructor_defaults_and_checks():
    from e4s_amd.optim import Ranger
    p = [torch.zeros(2, 3, requires_grad=True)]
    opt = Ranger(p)
    g = opt.param_groups[0]
    assert {k: g[k] for k in ("lr", "alpha", "k", "step_counter", "betas", "N_sma_threshhold", "eps", "weight_decay")} == dict(
        lr=1e-3, alpha=0.5, k=6, step_counter=0, betas=(.95, 0.999), N_sma_threshhold=5, eps=1e-5, weight_decay=0)
    assert (opt.alpha, opt.k, opt.N_sma_threshhold, opt.use_gc, opt.gc_gradient_threshold, opt.capturable) == (0.5, 6, 5, True, 1, True)
    assert Ranger(p, gc_conv_only=True, use_gc=False).gc_gradient_threshold == 3
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(k=0), dict(lr=0.0), dict(lr=-1e-3), dict(eps=0.0), dict(eps=-1e-5)):
        with pytest.raises(ValueError):
            Ranger(p, **bad)
    # the protocol GraphedStep relies on, before any step
    assert opt.hyper_by_value() == (((0.95, 0.999), 1e-5, 0.0, 6), 0.5, 5.0, 1)
    assert opt.captured_state_ptrs() == (0, 0) and opt.written_tensors() == []
    assert math.isfinite(Ranger.radam_coefficients(1, 0.95, 0.999, 5)[0])
