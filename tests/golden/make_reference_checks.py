"""Generate tests/golden/refchecks.pt and tests/golden/w_norm.pt by running the REAL reference on CPU.

Run where a checkout of the reference exists (oracle/ref_shim.py: $E4S_REFERENCE_ROOT):
    python tests/golden/make_reference_checks.py
The reference is read where it lies; only its recorded results are stored, so that tests/test_oracle_vs_reference.py and
tests/test_reference_scripts.py run without it.

What is pinned:
  refchecks.pt  styled_conv   StyledConv(mask_op=True) at (cin, cout, upsample) = (16, 24, False), (16, 8, True): seeded state
                              dict, inputs and the reference module's output (the test redraws the block masks with e4s_amd.synth)
                torgb         ToRGB(16, 512, mask_op=True): seeded state dict, inputs (with skip) and output
                w_norm_value  src/criteria/w_norm.py:WNormLoss on the seeded latents of w_norm.pt, start_from_latent_avg True / False
                net3_errors   the exception classes the reference's Net3.cal_style_codes raises for start_from_latent_avg=False and
                              learn_in_w=True (networks.py:145-158)
                loss_shapes   {key: shape} of the state dicts of the reference's IDLoss, LPIPS(alex) and FaceParsingLoss
                swap_comp     scripts/face_swap.py:swap_comp_style_vector on seeded [1,12,1280] style vectors, four cases
                w_optimizer   scripts/optimization.py:Optimizer.setup_W_optimizer: optimizer class, its param-group settings and the
                              latent after one step with an all-ones gradient
                script_imports  every `from src.<module> import <names>` of scripts/face_swap.py and scripts/optimization.py
  w_norm.pt     the gradient of WNormLoss(start_from_latent_avg=False) w.r.t. a seeded [2,12,18,512] latent (the test redraws the
                latent from the same seed; a checksum of it is stored beside the gradient)
"""
import os
import re
import sys
import tempfile
import types

os.environ.setdefault("E4S_ALLOW_UNINITIALIZED_LOSS_NETS", "1")

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from e4s_amd import synth  # noqa: E402
from oracle import ref_shim  # noqa: E402


@torch.no_grad()
def styled_conv_case(cin, cout, up):
    ns = ref_shim.reference_modules()
    m = ns.StyledConv(cin, cout, 3, 512, upsample=up, mask_op=True)
    g = torch.Generator().manual_seed(0)
    for p in m.parameters():
        p.copy_(torch.randn(p.shape, generator=g) * 0.5 + (1.0 if p.ndim == 1 and p.numel() == cin else 0.0))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(2, cin, 8, 8, generator=g)
    style = torch.randn(2, 12, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(2, 64, 8, seed=1))
    res = 16 if up else 8
    noise = torch.randn(2, 1, res, res, generator=g)
    return dict(cin=cin, cout=cout, up=up, sd=sd, x=x, style=style, noise=noise, want=m(x, style, mask, noise=noise))


@torch.no_grad()
def torgb_case():
    ns = ref_shim.reference_modules()
    m = ns.ToRGB(16, 512, mask_op=True)
    g = torch.Generator().manual_seed(1)
    for p in m.parameters():
        p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(2, 16, 8, 8, generator=g)
    style = torch.randn(2, 12, 512, generator=g)
    mask = synth.onehot(synth.synth_labels_blocks(2, 64, 8, seed=2))
    skip = torch.randn(2, 3, 4, 4, generator=g)
    return dict(sd=sd, x=x, style=style, skip=skip, want=m(x, style, mask, skip))


def w_norm_inputs():
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(2, 12, 18, 512, generator=g)
    avg = torch.randn(18, 512, generator=g)
    return lat, avg


def w_norm_case():
    import importlib.util
    sp = importlib.util.spec_from_file_location("ref_w_norm", os.path.join(ref_shim.REF_ROOT, "src", "criteria", "w_norm.py"))
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    lat, avg = w_norm_inputs()
    value = {}
    for flag in (True, False):
        x = lat.clone().requires_grad_(True)
        loss = mod.WNormLoss(start_from_latent_avg=flag)(x, avg)
        value[flag] = loss.detach()
    loss.backward()
    return value, dict(lat_sum=float(lat.double().sum()), lat_abs_sum=float(lat.double().abs().sum()), avg=avg, grad=x.grad)


def net3_errors():
    sd = synth.synth_state_dict(256, 13)
    lat = synth.synth_latent_avg(256)
    net = ref_shim.build_reference_net3(sd, lat, 256, 13)
    sv = torch.randn(1, 12, 1280)
    out = {}
    net.opts.start_from_latent_avg = False
    try:
        net.cal_style_codes(sv)
        out["start_from_latent_avg=False"] = None
    except Exception as e:      # noqa: BLE001
        out["start_from_latent_avg=False"] = type(e).__name__
    net.opts.start_from_latent_avg, net.opts.learn_in_w = True, True
    net.latent_avg = lat[:1].repeat(1, 1)                 # coach.py:118-119
    try:
        net.cal_style_codes(sv)
        out["learn_in_w=True"] = None
    except Exception as e:      # noqa: BLE001
        out["learn_in_w=True"] = type(e).__name__
    return out


def loss_shapes():
    import e4s_amd.criteria as C
    ns = ref_shim.reference_criteria(C.alexnet_features)
    tmp = tempfile.mkdtemp()
    mine = C.IDLoss(types.SimpleNamespace())
    torch.save(mine.facenet.state_dict(), tmp + "/irse50.pth")
    minep = C.FaceParsingLoss(types.SimpleNamespace())
    torch.save(minep.G.state_dict(), tmp + "/unet.pth")
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    return {"IDLoss": shapes(ns.IDLoss(types.SimpleNamespace(ir_se50_path=tmp + "/irse50.pth", id_loss_multiscale=True))),
            "LPIPS": shapes(ns.LPIPS(net_type="alex")),
            "FaceParsingLoss": shapes(ns.FaceParsingLoss(types.SimpleNamespace(face_parsing_model_path=tmp + "/unet.pth")))}


def swap_comp_cases(fs):
    g = torch.Generator().manual_seed(3)
    t_sv = torch.randn(1, 12, 1280, generator=g)
    d_sv = torch.randn(1, 12, 1280, generator=g)
    comp = sorted(set(range(12)) - {0, 4, 11, 10})
    out = dict(t_sv=t_sv, d_sv=d_sv, comp=comp, want={})
    for case in ("plain", "no_ear", "no_teeth", "below_face"):
        d = d_sv.clone()
        if case == "no_ear":
            d[:, 7] = 0
        if case == "no_teeth":
            d[:, 9] = 0
        out["want"][case] = fs.swap_comp_style_vector(t_sv, d, comp, belowFace_interpolation=case == "below_face")
    return out


def w_optimizer_case(opt_script):
    fake_self = types.SimpleNamespace(opts=types.SimpleNamespace(opt_name="adam", lr=1e-2))
    w_init = torch.randn(1, 12, 1280, generator=torch.Generator().manual_seed(4))
    optimizer, latent = opt_script.Optimizer.setup_W_optimizer(fake_self, w_init)
    group = {k: v for k, v in optimizer.param_groups[0].items() if k != "params"}
    rec = dict(cls=type(optimizer).__name__, group=group, w_init=w_init, requires_grad=bool(latent.requires_grad),
               aliases_input=latent.data_ptr() == w_init.data_ptr(), equal_before=bool(torch.equal(latent, w_init)))
    latent.grad = torch.ones_like(latent)
    optimizer.step()
    rec["after_one_step"] = latent.detach().clone()
    return rec


def script_imports():
    out = {}
    for name in ("face_swap", "optimization"):
        with open(os.path.join(ref_shim.REF_ROOT, "scripts", name + ".py"), encoding="utf-8") as fh:
            lines = fh.read().splitlines()
        recs = []
        for ln in lines:
            m = re.match(r"^from (src(?:\.\w+)*) import (.+)$", ln.strip())
            if m:
                recs.append((m.group(1), [n.strip() for n in m.group(2).split(",") if n.strip()]))
        out[name] = recs
    return out


def main():
    if not ref_shim.available():
        raise SystemExit("needs the reference tree at %s" % ref_shim.REF_ROOT)
    rec = dict(styled_conv=[styled_conv_case(16, 24, False), styled_conv_case(16, 8, True)], torgb=torgb_case())
    value, grad = w_norm_case()
    rec["w_norm_value"] = value
    rec["net3_errors"] = net3_errors()
    rec["loss_shapes"] = loss_shapes()
    fs = ref_shim.import_reference_script("face_swap")
    opt = ref_shim.import_reference_script("optimization")
    rec["swap_comp"] = swap_comp_cases(fs)
    rec["w_optimizer"] = w_optimizer_case(opt)
    rec["script_imports"] = script_imports()
    torch.save(rec, os.path.join(HERE, "refchecks.pt"))
    torch.save(grad, os.path.join(HERE, "w_norm.pt"))


if __name__ == "__main__":
    main()
