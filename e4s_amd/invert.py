"""Latent optimisation on the device: scripts/optimization.py `Optimizer.invertion`, for one image or a batch.

    reference                                              here
    -----------------------------------------------------  ------------------------------------------------------------------
    optimization.py:125-161  setup_W_optimizer              make_optimizer / Optimizer.setup_W_optimizer on the fused, capturable
                                                            optimisers (optim.FusedSGD / FusedAdam / FusedAdamax)
    optimization.py:88-122   calc_loss + seven float()s     LatentOptimizer's step; the seven numbers go to a device log
                                                            (e4s_scalar_log_f32), captured with the step: no host sync
    optimization.py:164-234  invertion                      LatentOptimizer.invert (B images at once) / Optimizer.invertion
    optimization.py:236-255  save_W_intermediate_results    Optimizer.save_W_intermediate_results

Every term of the script's objective is a batch mean of per-sample terms (id_loss.py:46-55, F.mse_loss, LPIPS,
face_parsing_loss.py), so B x the objective of a batch is the sum of B single-image objectives and its gradient with respect to
sample b's latent is the gradient of sample b's own objective: one step on a batch is the same step on each of its images.  The
step backpropagates B x the batch loss; the log keeps the batch's own numbers, the ones calc_loss would print."""
import os
from functools import partial

import numpy as np
import torch

from . import kernels as K
from . import postproc
from .optim import FusedAdam, FusedAdamax, FusedSGD, GraphedStep, forked_sum

TERMS = ('loss_id', 'id_improve', 'loss_l2', 'loss_lpips', 'loss_face_parsing', 'face_parsing_improve', 'loss')
WARMUP = 2                        # eager steps of a GraphedStep before its capture; they are optimisation steps like the others

# optimization.py:134-139 on the native optimisers (an unknown name is the dict's KeyError, as in the script)
OPTIMIZERS = {
    'sgd': FusedSGD,
    'adam': partial(FusedAdam, capturable=True),
    'sgdm': partial(FusedSGD, momentum=0.9),
    'adamax': FusedAdamax,
}


def make_optimizer(opt_name, params, lr):
    return OPTIMIZERS[opt_name](params, lr=lr)


def to_uint8(x):
    """ToPILImage's arithmetic on ((x + 1) / 2).clamp(0, 1) (optimization.py:238): mul(255).byte().  x fp32 [...,3,H,W] in [-1,1]:
    a device tensor goes through postproc.tensor2im -- the same operations, one rounding each -- and comes back uint8 [...,H,W,3];
    a host tensor is converted by the expression itself, in the layout it has."""
    if x.is_cuda:
        return postproc.tensor2im(x)
    return ((x + 1) / 2).clamp(0, 1).mul(255).byte()


def result_names(name, step=None):
    """File names of optimization.py:204-206,244-245 relative to the output directory: (gt, recon) or, with a step, (png, npy)."""
    if step is None:
        return os.path.join(name, name + "_gt.png"), os.path.join(name, name + "_recon.png")
    return os.path.join(name, f'{name}_{step:04}.png'), os.path.join(name, f'{name}_{step:04}.npy')


class Inversion(object):
    """What LatentOptimizer.invert returns.  latent [B,12,1280] (detached); recon0: the image of the encoder's vectors; recon: the image
    of the last step, generated before its update (what the script saves); history: device fp32 [W_steps, 7], columns `terms`."""
    terms = TERMS

    def __init__(self, latent, recon0, recon, history):
        self.latent, self.recon0, self.recon, self.history = latent, recon0, recon, history

    def loss_dict(self, step):
        """The script's loss_dict of 1-based `step` (one host copy)."""
        return dict(zip(self.terms, self.history[step - 1].tolist()))


class LatentOptimizer(object):
    """net: an e4s_amd.networks.Net3 (frozen here); crit: {'lpips': criteria.LPIPS, 'id': criteria.IDLoss, 'parsing':
    criteria.FaceParsingLoss}, each needed only where its lambda is > 0.  noise=None draws fresh noise in every step, as the script
    does; a list of [1 or B,1,h,w] maps fixes it.  graph=True replays the step as one HIP graph (one capture per invert() call: the
    loss modules cache the target's features per target tensor and a capture bakes them in)."""

    def __init__(self, net, crit, *, l2_lambda=1.0, lpips_lambda=0.8, id_lambda=0.1, face_parsing_lambda=0.1,
                 lpips_sizes=(1024, 512, 256), opt_name='adam', lr=1e-2, W_steps=200, graph=True, noise=None):
        if not hasattr(net, "get_style_vectors") or not hasattr(net, "gen_img"):
            raise TypeError("LatentOptimizer: net is a Net3")
        crit = dict(crit or {})
        for key, lam in (('lpips', lpips_lambda), ('id', id_lambda), ('parsing', face_parsing_lambda)):
            if lam > 0 and crit.get(key) is None:
                raise ValueError(f"LatentOptimizer: the {key} term has lambda {lam} but crit[{key!r}] is missing")
        if opt_name not in OPTIMIZERS:
            raise KeyError(opt_name)
        if int(W_steps) < 1:
            raise ValueError("LatentOptimizer: W_steps >= 1")
        self.net, self.crit = net, crit
        self.l2_lambda, self.lpips_lambda, self.id_lambda = float(l2_lambda), float(lpips_lambda), float(id_lambda)
        self.face_parsing_lambda = float(face_parsing_lambda)
        self.lpips_sizes = tuple(int(s) for s in lpips_sizes)
        self.opt_name, self.lr, self.W_steps, self.graph = opt_name, float(lr), int(W_steps), bool(graph)
        self.noise = None if noise is None else list(noise)
        for p in net.parameters():
            p.requires_grad = False

    def _terms(self, img, target, parts):
        """calc_loss's terms in its order (id, l2, lpips, parsing) as closures for forked_sum, each already times its lambda; what
        the log needs besides goes to `parts`.  -> (closures, index of the identity term or None)."""
        from .train import mse_loss
        fns, id_at = [], None
        main = torch.cuda.current_stream()
        if self.id_lambda > 0:
            def f_id():
                loss_id, improve, _ = self.crit['id'](img, target)
                parts['loss_id'], parts['id_improve'] = loss_id.detach(), improve.detach()
                for t in (parts['loss_id'], parts['id_improve']):      # read by the log on the step's stream
                    t.record_stream(main)
                return loss_id * self.id_lambda
            id_at = len(fns)
            fns.append(f_id)
        if self.l2_lambda > 0:
            def f_l2():
                loss_l2 = mse_loss(img, target)          # (F.mse_loss's semaphore memset must not sit in a captured step)
                parts['loss_l2'] = loss_l2.detach()
                return loss_l2 * self.l2_lambda
            fns.append(f_l2)
        if self.lpips_lambda > 0:
            def f_lpips():
                loss_lpips = self.crit['lpips'].forward_pooled(img, target, self.lpips_sizes)
                parts['loss_lpips'] = loss_lpips.detach()
                return loss_lpips * self.lpips_lambda
            fns.append(f_lpips)
        if self.face_parsing_lambda > 0:
            def f_parsing():
                loss_fp, improve = self.crit['parsing'](img, target)
                parts['loss_face_parsing'], parts['face_parsing_improve'] = loss_fp.detach(), improve.detach()
                return loss_fp * self.face_parsing_lambda
            fns.append(f_parsing)
        return fns, id_at

    def invert(self, img, onehot, init=None, on_snapshot=None, save_interval=None, on_step=None):
        """img fp32 [B,3,S,S] in [-1,1], onehot fp32 [B,12,Hm,Wm] -> Inversion after exactly W_steps steps.  init [B,12,1280]
        replaces the encoder's vectors.  on_snapshot(step, recon_u8 [B,S,S,3], latent) is called after every step that is a
        multiple of save_interval -- the only places where the host loop stops.  on_step(step): a host callback after every step has
        been ENQUEUED (instrumentation: tools/invert_bench.py records a HIP event there); it must not touch the device's results."""
        if not img.is_cuda or not onehot.is_cuda:
            raise RuntimeError("LatentOptimizer.invert: img and onehot must be on the ROCm device (no CPU path)")
        if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32 or onehot.dim() != 4 or onehot.shape[0] != img.shape[0]:
            raise ValueError("LatentOptimizer.invert: img is fp32 [B,3,S,S] and onehot [B,R,Hm,Wm]")
        net, B, steps = self.net, img.shape[0], self.W_steps
        img, onehot = img.contiguous(), onehot.contiguous()
        with torch.no_grad():
            sv, _ = net.get_style_vectors(img, onehot)
            if init is not None:
                if tuple(init.shape) != tuple(sv.shape):
                    raise ValueError(f"LatentOptimizer.invert: init is {list(sv.shape)}, got {list(init.shape)}")
                sv = init.to(device=img.device, dtype=torch.float32)
            recon0, _, _ = net.gen_img(None, net.cal_style_codes(sv), onehot, noise=self.noise)
        latent = sv.detach().clone().contiguous().requires_grad_(True)
        opt = make_optimizer(self.opt_name, [latent], self.lr)
        history = torch.zeros(steps, len(TERMS), device=img.device, dtype=torch.float32)
        count = torch.zeros(1, device=img.device, dtype=torch.int64)       # the step being taken, on the device: the log's row
        zero = torch.zeros(1, device=img.device, dtype=torch.float32)      # the columns of absent terms
        last, host = {}, {"n": 0}
        snap = on_snapshot if (on_snapshot is not None and save_interval) else None

        def snapshot():
            if on_step is not None:
                on_step(host["n"])
            if snap is not None and host["n"] % int(save_interval) == 0:
                with torch.no_grad():
                    snap(host["n"], postproc.tensor2im(last["recon"]), latent.detach())

        def body():
            K.advance_steps(count)
            codes = net.cal_style_codes(latent)
            recon, _, _ = net.gen_img(None, codes, onehot, noise=self.noise)
            parts = {}
            fns, id_at = self._terms(recon, img, parts)
            # the identity network, the longest chain, on the one side branch and the rest on this stream under it (bench.py's placement)
            loss = forked_sum(0.0, fns, inputs=(recon, img), side_terms=[] if id_at is None else [id_at])
            (loss if B == 1 else loss * float(B)).backward()
            opt.step()
            parts['loss'] = loss.detach()
            K.scalar_log([parts.get(k, zero) for k in TERMS], count, history)
            last["recon"] = recon.detach()
            if not torch.cuda.is_current_stream_capturing():       # an eager step (a GraphedStep's warm-ups among them)
                host["n"] += 1
                snapshot()
            return parts['loss']

        if self.graph and steps >= WARMUP + 1:
            gs = GraphedStep(opt, body, warmup=WARMUP)              # WARMUP real steps, then the capture (which executes nothing)
            while host["n"] < steps:
                gs.step()
                host["n"] += 1
                snapshot()
            gs.validate()                                           # one-hot masks, finite loss: one sync per inversion
        else:
            while host["n"] < steps:
                opt.zero_grad(set_to_none=True)
                body()
        return Inversion(latent.detach(), recon0, last["recon"].clone(), history)


class Optimizer:
    """scripts/optimization.py:50-255 with the reference's OptimOptions namespace.  net= / crit= take ready-made models (tests
    inject synthetic weights); otherwise they are built from opts.checkpoint_path and the loss networks' paths in opts.  dataset: any
    sequence with `.imgs` (paths) that yields (img [3,S,S] in [-1,1], mask [1,Hm,Wm] = label / 255, _) like CelebAHQDataset; None
    builds the reference's test split through the `src` overlay, which needs torchvision."""

    def __init__(self, opts, dataset=None, net=None, crit=None):
        self.opts = opts
        dev = torch.device(getattr(opts, "device", "cuda:0"))
        if dataset is None:
            import torchvision.transforms as transforms
            from src.datasets.dataset import CelebAHQDataset, MASK_CONVERT_TF_DETAILED, NORMALIZE, TO_TENSOR
            dataset = CelebAHQDataset(dataset_root=opts.dataset_root, mode="test",
                                      img_transform=transforms.Compose([TO_TENSOR, NORMALIZE]),
                                      label_transform=transforms.Compose([MASK_CONVERT_TF_DETAILED, TO_TENSOR]),
                                      fraction=opts.ds_frac)
        self.test_ds = dataset
        if net is None:
            if getattr(opts, "checkpoint_path", None) is None:
                raise ValueError("please specify the pre-trained weights!")
            from .networks import Net3
            net = Net3(opts).eval().to(dev)
            ckpt = torch.load(opts.checkpoint_path, map_location="cpu")
            net.latent_avg = ckpt["latent_avg"].to(dev) if opts.start_from_latent_avg else None
            sd = ckpt["state_dict_ema"] if getattr(opts, "load_ema", False) else ckpt["state_dict"]
            net.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()})
        self.net = net
        if crit is None:
            from . import criteria
            crit = {}
            if opts.lpips_lambda > 0:
                crit['lpips'] = criteria.LPIPS(net_type='alex').to(dev).eval()
            if opts.id_lambda > 0:
                crit['id'] = criteria.IDLoss(opts).to(dev).eval()
            if opts.face_parsing_lambda > 0:
                crit['parsing'] = criteria.FaceParsingLoss(opts).to(dev).eval()
        self.crit = crit
        # (optimization.py:103-107 pools to 1024 // 2 ** i whatever the image; opts.lpips_sizes: other scales, for smaller generators)
        self.latent_optimizer = LatentOptimizer(
            net, crit, l2_lambda=opts.l2_lambda, lpips_lambda=opts.lpips_lambda, id_lambda=opts.id_lambda,
            face_parsing_lambda=opts.face_parsing_lambda, lpips_sizes=tuple(getattr(opts, "lpips_sizes", (1024, 512, 256))),
            opt_name=opts.opt_name, lr=opts.lr, W_steps=opts.W_steps, graph=getattr(opts, "graph", True))

    def calc_loss(self, img, img_recon, mask):
        """optimization.py:88-122 -> (loss, loss_dict, id_logs); the float()s of the script are host syncs, as there."""
        lo = self.latent_optimizer
        parts = {}
        fns, _ = lo._terms(img_recon, img, parts)
        loss = 0.0
        for fn in fns:
            loss = loss + fn()
        parts['loss'] = loss
        return loss, {k: float(parts[k]) for k in TERMS if k in parts}, None

    def setup_W_optimizer(self, W_init, noise_init=None):
        """optimization.py:125-161 -> (optimizer, latent)."""
        if noise_init is not None:
            raise NotImplementedError("optimising the noise maps: the generator backward has no gradient to them")
        tmp = W_init.clone().detach()
        tmp.requires_grad = True
        return make_optimizer(self.opts.opt_name, [tmp], self.opts.lr), tmp

    def save_W_intermediate_results(self, img_name, gen_im, latent, step, noise=None):
        """optimization.py:236-255.  gen_im: fp32 [B,3,S,S] (its first image is saved) or the uint8 [B,S,S,3] of a snapshot."""
        from PIL import Image
        if noise is not None:
            raise NotImplementedError("optimising the noise maps: the generator backward has no gradient to them")
        if gen_im.dtype == torch.uint8:
            u8 = gen_im
        else:
            u8 = to_uint8(gen_im.detach()[:1])
            u8 = u8 if gen_im.is_cuda else u8.movedim(1, -1)       # (the device conversion already returns HWC)
        png, npy = result_names(img_name, step)
        os.makedirs(os.path.join(self.opts.output_dir, img_name), exist_ok=True)
        Image.fromarray(np.ascontiguousarray(u8[0].cpu().numpy())).save(os.path.join(self.opts.output_dir, png))
        np.save(os.path.join(self.opts.output_dir, npy), latent.detach().cpu().numpy())

    def invert_image(self, img, mask, name):
        """The body of `invertion` for one image [3,S,S] in [-1,1] and its label map [1,Hm,Wm] (labels / 255, as the dataset's
        TO_TENSOR leaves them) -> Inversion; writes NAME/NAME_gt.png, NAME_recon.png, NAME_{step:04}.png / .npy."""
        from PIL import Image
        opts = self.opts
        dev = next(self.net.parameters()).device
        os.makedirs(os.path.join(opts.output_dir, name), exist_ok=True)
        img = img.unsqueeze(0).to(dev).float()
        labels = (mask.unsqueeze(0) * 255).long().to(dev)
        onehot = postproc.labelMap2OneHot(labels, int(opts.num_seg_cls))
        gt_path, recon_path = result_names(name)
        Image.fromarray(postproc.tensor2im(img)[0].cpu().numpy()).save(os.path.join(opts.output_dir, gt_path))

        def on_snapshot(step, recon_u8, latent):
            if step != opts.W_steps:                               # (the last step is saved below, once)
                self.save_W_intermediate_results(name, recon_u8, latent, step)
        save = bool(getattr(opts, "save_intermediate", False))
        res = self.latent_optimizer.invert(img, onehot, on_snapshot=on_snapshot if save else None,
                                           save_interval=int(opts.save_interval) if save else None)
        Image.fromarray(postproc.tensor2im(res.recon0)[0].cpu().numpy()).save(os.path.join(opts.output_dir, recon_path))
        self.save_W_intermediate_results(name, res.recon, res.latent, opts.W_steps)
        if getattr(opts, "verbose", False):
            print("[%s]" % name + "".join(k + " : {:.4f}, ".format(v) for k, v in res.loss_dict(opts.W_steps).items() if k[:4] == "loss"))
        return res

    def invertion(self, sample_idx):
        img_name = os.path.basename(self.test_ds.imgs[sample_idx]).split(".")[0]
        img, mask, _ = self.test_ds[sample_idx]
        return self.invert_image(img, mask, img_name)
