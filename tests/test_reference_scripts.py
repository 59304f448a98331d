"""CPU tests of the Python boundary: the reference's scripts import everything through `src.*`; with this
repo first on sys.path the `src` overlay must resolve the hot path to e4s_amd and everything else to the reference checkout at
$E4S_REFERENCE_ROOT.  What the reference's scripts and classes import, build and return is recorded in tests/golden/refchecks.pt
(tests/golden/make_reference_checks.py, run where the reference tree exists); the overlay is exercised here against a stand-in
checkout written into a temporary directory, so no test needs the reference tree."""
import importlib
import inspect
import os
import sys
import types

import pytest
import torch

from e4s_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def refchecks(golden):
    return golden("refchecks.pt")


def _drop_src_modules():
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]


@pytest.fixture
def overlay(monkeypatch):
    """Import `src.*` afresh with $E4S_REFERENCE_ROOT set by the test (the overlay reads it when a package is imported)."""
    def use(reference_root):
        monkeypatch.setenv("E4S_REFERENCE_ROOT", str(reference_root))
        _drop_src_modules()
        if ROOT not in sys.path:
            monkeypatch.syspath_prepend(ROOT)
    yield use
    _drop_src_modules()


def _stub_source(names):
    return "".join(("class %s:\n    pass\n\n\n" if n[:1].isupper() else "def %s(*args, **kwargs):\n    return None\n\n\n") % n
                   for n in names)


def _write_stand_in_checkout(root, script_imports):
    """A checkout with the reference's `src` layout (a namespace package: no __init__.py) whose modules define every name the
    scripts import from them, plus the helpers the overlay executes in place."""
    mods = {"src.models.networks": {"Net3"},
            "src.utils.torch_utils": {"tensor2im", "tensor2map", "labelMap2OneHot", "accumulate"},
            "src.models.encoders.helpers": {"l2_norm", "bottleneck_IR", "get_blocks", "bottleneck_IR_SE", "bottleneck_IR_SE_Ours"}}
    for recs in script_imports.values():
        for mod, names in recs:
            if mod == "src.utils" and names == ["torch_utils"]:
                continue
            mods.setdefault(mod, set()).update(names)
    for mod, names in mods.items():
        path = os.path.join(root, *mod.split(".")) + ".py"
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(_stub_source(sorted(names)))
    return mods


def test_scripts_resolve_hot_path_to_e4s_amd_and_the_rest_to_the_reference(refchecks, overlay, tmp_path):
    import e4s_amd.criteria
    import e4s_amd.encoders
    import e4s_amd.networks
    import e4s_amd.op
    imports = refchecks["script_imports"]
    assert set(imports) == {"face_swap", "optimization"} and all(imports.values())
    ref = tmp_path / "reference"
    _write_stand_in_checkout(str(ref), imports)
    overlay(ref)
    # the loss networks of the optimisation loop (scripts/optimization.py:23-24) are the native ones too
    native = {"Net3": e4s_amd.networks.Net3, "IDLoss": e4s_amd.criteria.IDLoss, "LPIPS": e4s_amd.criteria.LPIPS,
              "FaceParsingLoss": e4s_amd.criteria.FaceParsingLoss}
    seen_native = set()
    for script, recs in imports.items():
        for mod, names in recs:
            m = importlib.import_module(mod)
            for n in names:
                obj = getattr(m, n) if hasattr(m, n) else importlib.import_module(mod + "." + n)
                if n in native:
                    # the hot path: the native implementation, not the checkout's module of the same name
                    assert obj is native[n], (script, mod, n)
                    seen_native.add(n)
                elif isinstance(obj, types.ModuleType):
                    assert obj.__name__ == mod + "." + n
                else:
                    # everything off the hot path is the checkout's own module, imported where it lies
                    assert inspect.getfile(obj).startswith(str(ref) + os.sep), (script, mod, n)
                    assert obj.__module__ == mod
    assert seen_native == set(native)
    # src.utils.torch_utils: the checkout's helpers + the version-bumping accumulate of the overlay
    tu = importlib.import_module("src.utils.torch_utils")
    assert inspect.getfile(tu.tensor2im).startswith(str(ref) + os.sep)
    assert not inspect.getfile(tu.accumulate).startswith(str(ref) + os.sep)
    assert not inspect.getfile(tu.labelMap2OneHot).startswith(str(ref) + os.sep)
    op = importlib.import_module("src.models.stylegan2.op")
    assert op.fused_leaky_relu is e4s_amd.op.fused_leaky_relu and op.upfirdn2d is e4s_amd.op.upfirdn2d
    assert hasattr(op.conv2d_gradfix, "no_weight_gradients")                   # src/criteria/adv_loss.py:34
    helpers = importlib.import_module("src.models.encoders.helpers")
    assert inspect.getfile(helpers.l2_norm).startswith(str(ref) + os.sep)
    assert inspect.getfile(helpers.bottleneck_IR).startswith(str(ref) + os.sep)  # parsing UNet
    assert helpers.bottleneck_IR_SE_Ours is e4s_amd.encoders.bottleneck_IR_SE_Ours
    assert helpers.bottleneck_IR_SE is e4s_amd.criteria.bottleneck_IR_SE


def test_loss_network_state_dicts_match_the_reference_classes(refchecks):
    """IDLoss / LPIPS: same keys and shapes as the reference's own modules, so its checkpoints load unchanged."""
    import e4s_amd.criteria as C
    want = refchecks["loss_shapes"]
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes(C.IDLoss(types.SimpleNamespace())) == want["IDLoss"]
    assert shapes(C.LPIPS()) == want["LPIPS"]
    assert shapes(C.FaceParsingLoss(types.SimpleNamespace())) == want["FaceParsingLoss"]


@pytest.mark.parametrize("case", ["plain", "no_ear", "no_teeth", "below_face"])
def test_swap_comp_style_vector_matches_the_scripts(refchecks, case):
    """scripts/face_swap.py:117-146 (the reference's result, recorded) vs the batched, sync-free e4s_amd version."""
    from e4s_amd.networks import swap_comp_style_vector
    rec = refchecks["swap_comp"]
    t_sv = rec["t_sv"].clone()
    d_sv = rec["d_sv"].clone()
    if case == "no_ear":
        d_sv[:, 7] = 0
    if case == "no_teeth":
        d_sv[:, 9] = 0
    comp = sorted(set(range(12)) - {0, 4, 11, 10})
    assert comp == rec["comp"]
    bf = case == "below_face"
    want = rec["want"][case]
    got = swap_comp_style_vector(t_sv, d_sv, comp, belowFace_interpolation=bf)
    assert torch.equal(want, got)
    # batched: row i of a batch equals the single-sample call
    t2, d2 = torch.cat([t_sv, d_sv.flip(1)]), torch.cat([d_sv, t_sv])
    got2 = swap_comp_style_vector(t2, d2, comp, belowFace_interpolation=bf)
    assert torch.equal(got2[:1], want)


def test_optimizer_setup_against_native_net3(refchecks):
    """scripts/optimization.py:125-161 (the reference's optimizer, recorded) on the latent the native Net3 produces the shape of."""
    from e4s_amd.networks import Net3
    from e4s_amd.options import make_opts
    with torch.device("meta"):
        net = Net3(make_opts(out_size=1024))
    assert set(net.state_dict()) == {k for k, _, _ in synth.net3_param_spec(1024, 13)}
    rec = refchecks["w_optimizer"]
    assert rec["cls"] == "Adam" and rec["group"]["lr"] == 1e-2
    assert rec["requires_grad"] and rec["equal_before"] and not rec["aliases_input"]
    w_init = rec["w_init"]
    assert tuple(w_init.shape) == (1, 12, 1280)
    latent = w_init.clone().detach().requires_grad_(True)
    optimizer = getattr(torch.optim, rec["cls"])([latent], **rec["group"])
    latent.grad = torch.ones_like(latent)
    optimizer.step()
    assert float((latent - w_init).abs().max()) > 0
    assert torch.equal(latent.detach(), rec["after_one_step"])


def test_accumulate_invalidates_weight_packs(overlay, tmp_path):
    """the reference's EMA writes through `.data` (src/utils/torch_utils.py:189-194) which leaves `_version`
    alone; the overlay's accumulate must make every cached weight pack stale."""
    from e4s_amd import packs
    overlay(tmp_path / "no_reference")                  # the overlay alone: no checkout to fall through to
    tu = importlib.import_module("src.utils.torch_utils")
    a, b = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)
    k0 = packs.param_key(a.weight)
    a.weight.data.mul_(0.5)                      # the reference's form: invisible to the version counter ...
    assert packs.param_key(a.weight) == k0
    packs.invalidate_packs()                     # ... hence the explicit invalidation hook
    k1 = packs.param_key(a.weight)
    assert k1 != k0
    before = a.weight.detach().clone()
    tu.accumulate(a, b, decay=0.9)
    assert torch.allclose(a.weight, before * 0.9 + b.weight * 0.1)
    assert packs.param_key(a.weight) != k1
