"""Fixture of the BiSeNet face parser (e4s_amd/face_parser.py): the REFERENCE's own modules run on CPU.

Imports src/pretrained/face_parsing/{resnet,model,face_parsing_demo}.py and src/datasets/dataset.py where they lie, with the
absent third-party packages stubbed (oracle/ref_shim.stub_third_party) and `.cuda()` a no-op (model.py:15 calls it at import).
Nothing reaches the network: torch.utils.model_zoo.load_url / torch.hub.load_state_dict_from_url raise, and
Resnet18.init_weight (which fetches the ImageNet ResNet-18, resnet.py:82-89) is a no-op before any BiSeNet is built.
Weights: synth.synth_module_state_dict(model, tag="bisenet."), the same seeded tensors the tests load into e4s_amd's BiSeNet.

Recorded (inputs as seeds, never as tensors):
    keys / shapes         the reference BiSeNet's state_dict
    seg12_of_arange19     __ffhq_masks_to_faceParser_mask_detailed(arange(19))
    taps                  BicubicDownSample(factor=2).k1 (the normalised 8-tap filter)
    small.*               BiSeNet(x) for x = synth_image(2, 128, seed=SMALL_SEED, tag="bisenet.small") (already normalised):
                          the three heads' logits at the rows / columns SAMPLE128 (fp32 forward)
    full.*                for the uint8 image FULL_IMAGE (seed FULL_SEED) parsed with FaceParser's steps: the preprocessed
                          512^2 input at the rows / columns SAMPLE512, the first head's 64^2 logits (NCHW), the 512^2 19-class
                          and seg12 labels (zlib), and the fp64 top-2 margin of the upsampled first-head logits in units of
                          1e-4 x the logit scale, saturated at 255 (uint8, zlib)

Run in the build container:  python tests/golden/make_face_parser_golden.py   (writes tests/golden/face_parser.pt)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SMALL_SEED, FULL_SEED = 11, 12
SAMPLE128 = sorted(set(range(0, 128, 8)) | {127})
SAMPLE512 = sorted(set(range(0, 8)) | set(range(504, 512)) | set(range(0, 512, 11)))


def full_image():
    """The seeded 1024^2 uint8 NHWC image of the full-size check (decoded pixels, as PIL hands them to ToTensor)."""
    from e4s_amd import synth
    x = synth.synth_image(1, 1024, seed=FULL_SEED, tag="bisenet.full")
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def small_input():
    from e4s_amd import synth
    return synth.synth_image(2, 128, seed=SMALL_SEED, tag="bisenet.small")


def reference_parser():
    """(BiSeNet, BicubicDownSample, seg_mean, seg_std, seg19->12 function) of the reference, imported offline on CPU."""
    from oracle import ref_shim
    ref_shim.stub_third_party()
    import torch.hub
    import torch.utils.model_zoo

    def _no_network(*a, **k):
        raise RuntimeError("the face parser fixture must not download anything")

    torch.utils.model_zoo.load_url = _no_network
    torch.hub.load_state_dict_from_url = _no_network
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    saved = list(sys.path)
    sys.path[:] = [ref_shim.REF_ROOT] + [p for p in saved if not os.path.isfile(os.path.join(p or os.getcwd(), "src", "__init__.py"))]
    patched = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        import importlib
        resnet = importlib.import_module("src.pretrained.face_parsing.resnet")
        resnet.Resnet18.init_weight = lambda self: None
        model = importlib.import_module("src.pretrained.face_parsing.model")
        demo = importlib.import_module("src.pretrained.face_parsing.face_parsing_demo")
        dataset = importlib.import_module("src.datasets.dataset")
    finally:
        torch.Tensor.cuda = patched
        sys.path[:] = saved
    to12 = getattr(dataset, "__ffhq_masks_to_faceParser_mask_detailed")
    return model.BiSeNet, demo.BicubicDownSample, model.seg_mean, model.seg_std, to12


def _z(a):
    """uint8 array -> (zlib bytes, shape): keeps the fixture small (committed files stay under 1 MiB)."""
    import zlib
    return zlib.compress(np.ascontiguousarray(a).tobytes(), 9), tuple(a.shape)


def unz(z):
    import zlib
    return torch.from_numpy(np.frombuffer(zlib.decompress(z[0]), dtype=np.uint8).reshape(z[1]).copy())


def main():
    from e4s_amd import synth
    BiSeNet, BicubicDownSample, seg_mean, seg_std, to12 = reference_parser()
    torch.manual_seed(0)
    net = BiSeNet(n_classes=19).eval()
    sd = synth.synth_module_state_dict(net, tag="bisenet.")
    net.load_state_dict(sd, strict=True)
    out = {"keys": list(sd.keys()), "shapes": [tuple(v.shape) for v in sd.values()],
           "seg12_of_arange19": torch.from_numpy(to12(np.arange(19, dtype=np.uint8)).astype(np.uint8)),
           "sample128": SAMPLE128, "sample512": SAMPLE512, "small_seed": SMALL_SEED, "full_seed": FULL_SEED}
    down = BicubicDownSample(factor=2, cuda=False)
    out["taps"] = down.k1.reshape(3, -1)[0].clone()
    with torch.no_grad():
        heads = net(small_input())
        idx = torch.tensor(SAMPLE128)
        out["small.logits"] = [h[:, :, idx][:, :, :, idx].contiguous() for h in heads]
        # FaceParser.preprocess_img (face_parsing_demo.py:152-156): ToTensor (x / 255), bicubic /2, clamp, normalise
        img = full_image().permute(0, 3, 1, 2).float().div(255)
        pre = (down(img).clamp(0, 1) - seg_mean) / seg_std
        s = torch.tensor(SAMPLE512)
        out["full.pre"] = pre[:, :, s][:, :, :, s].contiguous()
        # the first head before its upsampling: hook the main BiSeNetOutput
        low = {}
        hk = net.conv_out.register_forward_hook(lambda m, i, o: low.__setitem__("x", o))
        main, _, _ = net(pre)
        hk.remove()
        out["full.logits64"] = low["x"].contiguous()
        lab19 = torch.argmax(main, dim=1)[0].to(torch.uint8)
        out["full.labels19"] = _z(lab19.numpy())
        out["full.labels12"] = _z(to12(lab19.numpy()).astype(np.uint8))
        # fp64 top-2 margin of the same network in double precision
        net64 = BiSeNet(n_classes=19).eval()
        net64.load_state_dict(sd, strict=True)
        net64.double()
        main64, _, _ = net64(pre.double())
        top2 = torch.topk(main64[0], 2, dim=0).values
        out["full.scale"] = float(main64.abs().max())
        # margin in units of 1e-4 x scale, saturated at 255 (what the test needs is margin > 1e-3 x scale, i.e. > 10 units)
        units = ((top2[0] - top2[1]) / out["full.scale"] * 1e4).round().clamp(0, 255).to(torch.uint8)
        out["full.margin_u8"] = _z(units.numpy())
        out["full.labels19_fp64_agree"] = float((torch.argmax(main64, dim=1)[0].to(torch.uint8) == lab19).double().mean())
    path = os.path.join(HERE, "face_parser.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
