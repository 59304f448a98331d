"""Host-only checks of e4s_amd.invert (scripts/optimization.py natively): the optimiser table of setup_W_optimizer, its refusals,
LatentOptimizer's construction, the names of the script's files, the bytes of a saved image, and the three entry points behind it in the
binding derived from include/e4s_hip.h."""
import os
import types
from functools import partial

import pytest
import torch

from e4s_amd import invert, lib
from e4s_amd.optim import FusedAdam, FusedAdamax, FusedSGD


class _Net(torch.nn.Module):
    """What LatentOptimizer asks of a Net3 before it runs anything."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))

    def get_style_vectors(self, img, mask):
        raise AssertionError("not called on the host")

    gen_img = cal_style_codes = get_style_vectors


def _opts(**kw):
    base = dict(l2_lambda=1.0, lpips_lambda=0.0, id_lambda=0.0, face_parsing_lambda=0.0, opt_name="adam", lr=1e-2, W_steps=4,
                output_dir="out", save_intermediate=False, save_interval=2, device="cpu", num_seg_cls=12, out_size=256, verbose=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


class _Dataset(list):
    imgs = ["/data/CelebA-HQ-img/123.jpg"]


# optimization.py:134-139
TORCH_TABLE = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "sgdm": partial(torch.optim.SGD, momentum=0.9), "adamax": torch.optim.Adamax}
NATIVE_CLASS = {"sgd": FusedSGD, "adam": FusedAdam, "sgdm": FusedSGD, "adamax": FusedAdamax}


@pytest.mark.parametrize("name", ["sgd", "adam", "sgdm", "adamax"])
def test_setup_W_optimizer_builds_the_scripts_optimiser(name):
    w = torch.randn(1, 12, 1280)
    o = invert.Optimizer(_opts(opt_name=name, lr=0.03), dataset=_Dataset(), net=_Net(), crit={})
    opt, latent = o.setup_W_optimizer(w)
    assert type(opt) is NATIVE_CLASS[name] and opt.capturable
    ref = TORCH_TABLE[name]([w.clone().requires_grad_(True)], lr=0.03)
    (g,), (rg,) = opt.param_groups, ref.param_groups
    keys = {"sgd": ("lr", "momentum", "dampening", "weight_decay", "nesterov"), "sgdm": ("lr", "momentum", "dampening", "weight_decay", "nesterov"),
            "adam": ("lr", "betas", "eps", "weight_decay"), "adamax": ("lr", "betas", "eps", "weight_decay")}[name]
    for k in keys:
        assert g[k] == rg[k], (name, k)
    assert all(g[k] == rg[k] for k in g if k != "params" and k in rg)        # and whatever else the two groups share
    if name == "sgdm":
        assert g["momentum"] == 0.9
    # the latent: a detached copy that asks for a gradient, the one parameter of the optimiser
    assert g["params"] == [latent] and g["params"][0] is latent
    assert latent.requires_grad and latent.is_leaf and latent.grad_fn is None
    assert latent.data_ptr() != w.data_ptr() and torch.equal(latent.detach(), w) and not w.requires_grad


def test_refusals():
    o = invert.Optimizer(_opts(), dataset=_Dataset(), net=_Net(), crit={})
    with pytest.raises(NotImplementedError):
        o.setup_W_optimizer(torch.zeros(1, 12, 1280), noise_init=[torch.zeros(1, 1, 4, 4)])
    o.opts.opt_name = "rmsprop"
    with pytest.raises(KeyError):
        o.setup_W_optimizer(torch.zeros(1, 12, 1280))
    with pytest.raises(KeyError):
        invert.LatentOptimizer(_Net(), {}, lpips_lambda=0, id_lambda=0, face_parsing_lambda=0, opt_name="rmsprop")
    with pytest.raises(RuntimeError):                                          # no CPU path
        invert.LatentOptimizer(_Net(), {}, lpips_lambda=0, id_lambda=0, face_parsing_lambda=0).invert(
            torch.zeros(1, 3, 8, 8), torch.zeros(1, 12, 4, 4))


def test_construction_and_names():
    for key, kw in (("lpips", "lpips_lambda"), ("id", "id_lambda"), ("parsing", "face_parsing_lambda")):
        lam = dict(lpips_lambda=0, id_lambda=0, face_parsing_lambda=0)
        lam[kw] = 0.5
        with pytest.raises(ValueError, match=key):
            invert.LatentOptimizer(_Net(), {}, **lam)
        invert.LatentOptimizer(_Net(), {key: object()}, **lam)                 # its network is enough
    with pytest.raises(ValueError):
        invert.LatentOptimizer(_Net(), None)                                   # the defaults need all three
    net = _Net()
    lo = invert.LatentOptimizer(net, {}, lpips_lambda=0, id_lambda=0, face_parsing_lambda=0)
    assert not any(p.requires_grad for p in net.parameters())                  # frozen
    assert (lo.l2_lambda, lo.opt_name, lo.lr, lo.W_steps, lo.graph, lo.noise, lo.lpips_sizes) == (1.0, "adam", 1e-2, 200, True, None, (1024, 512, 256))
    assert invert.TERMS == invert.Inversion.terms == ('loss_id', 'id_improve', 'loss_l2', 'loss_lpips', 'loss_face_parsing',
                                                      'face_parsing_improve', 'loss')
    assert invert.result_names("123") == (os.path.join("123", "123_gt.png"), os.path.join("123", "123_recon.png"))
    assert invert.result_names("123", 200) == (os.path.join("123", "123_0200.png"), os.path.join("123", "123_0200.npy"))
    assert invert.result_names("a", 7)[0].endswith("a_0007.png")


def test_image_bytes_are_ToPILImage_s():
    k = torch.arange(256, dtype=torch.float64)
    ties = (k / 255 * 2 - 1).to(torch.float32)                                 # x whose ((x + 1) / 2) * 255 sits at or next to an integer
    below, above = torch.nextafter(ties, torch.tensor(-2.0)), torch.nextafter(ties, torch.tensor(2.0))
    special = torch.tensor([-1.0, 1.0, -1.5, 1.5, -100.0, 100.0, 0.0, -0.0, 1.0 - 2 ** -24, -1.0 + 2 ** -24])
    g = torch.Generator().manual_seed(3)
    vals = torch.cat([ties, below, above, special, torch.rand(3 * 32 * 32 - 3 * 256 - special.numel(), generator=g) * 2.4 - 1.2])
    x = vals.view(1, 3, 32, 32)
    want = ((x + 1) / 2).clamp(0, 1).mul(255).byte()
    got = invert.to_uint8(x)
    assert got.dtype == torch.uint8 and got.shape == x.shape and torch.equal(got, want)
    assert got.min() == 0 and got.max() == 255 and len(torch.unique(got)) == 256
    # a file written from a host image decodes to the same bytes
    import numpy as np
    from PIL import Image
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        o = invert.Optimizer(_opts(output_dir=d), dataset=_Dataset(), net=_Net(), crit={})
        o.save_W_intermediate_results("n", x, torch.ones(1, 12, 1280), 3)
        png, npy = (os.path.join(d, f) for f in invert.result_names("n", 3))
        assert np.array_equal(np.asarray(Image.open(png)), want[0].permute(1, 2, 0).numpy())
        lat = np.load(npy)
        assert lat.dtype == np.float32 and lat.shape == (1, 12, 1280) and (lat == 1).all()


def test_abi_has_the_three_entry_points():
    assert lib.ABI_VERSION == 31
    p, i, l, d = lib.c_p, lib.c_i, lib.c_l, lib.c_d
    assert lib.SIGNATURES["e4s_sgd_multi_dev_f32"] == [i, p, p, p, p, d, p, d, d, d, p]
    assert lib.SIGNATURES["e4s_adamax_multi_dev_f32"] == [i, p, p, p, p, p, p, d, p, d, d, d, d, p]
    assert lib.SIGNATURES["e4s_scalar_log_f32"] == [i, p, p, p, l, p]
    assert [t for t, _ in lib.FUNCTIONS["e4s_scalar_log_f32"][1]] == ["int", "const float* const*", "const int64_t*", "float*", "int64_t", "void*"]
    assert not {"e4s_sgd_multi_dev_f32", "e4s_adamax_multi_dev_f32", "e4s_scalar_log_f32"} & lib.INT64_RETURN
