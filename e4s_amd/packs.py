"""Cache keys of the re-packed weight images (tap-packed, polyphase, split-bf16, stacked LocalMLPs).

A pack is valid for one (storage, version) of its source parameters.  `Tensor._version` advances on every in-place
update made THROUGH the tensor (optimizer steps, `load_state_dict`, `p.copy_()` under no_grad) but NOT on updates made
through `p.data` (the reference's EMA, src/utils/torch_utils.py:189-194, writes `p.data.mul_().add_()`).  Code that
mutates weights behind autograd's back must call `invalidate_packs()` afterwards (the overlay's
`src.utils.torch_utils.accumulate` does); it bumps a process-wide generation that is part of every key.  A captured
HIP graph (networks.GraphedFaceSwap) bakes the pack pointers in: re-capture it after any weight change.

A captured TRAIN step (train.graphed_g_step / graphed_d_step) reads the packs of a network that another step trains between
its replays.  A cache hit at capture time would bake in a pack allocated eagerly, which serves the weights of the capture
forever and is freed by the next eager consumer that re-packs.  So the step's body calls `invalidate_module_packs()` on the
modules that own a trained parameter: the capture then records the re-pack kernels, into the graph's own memory pool (or
into the module's lifetime buffers, `_e4s_bufs`, which stay), and every replay re-packs from the weights of the moment."""

_GENERATION = 0

# Every attribute that caches a weight pack on a module (keyed on param_key).  A new cache must be listed here, or a captured
# train step keeps serving it stale (tests/test_host_logic.py checks the package against this list).
PACK_ATTRS = (
    "_e4s_pack", "_e4s_wino", "_e4s_split", "_e4s_frag", "_e4s_wt", "_e4s_wt_fwd",         # encoders / encoder_autograd / stylegan2 ConvLayer
    "_e4s_t", "_e4s_stats", "_e4s_head", "_e4s_small", "_e4s_fold",            # criteria (loss networks)
    "_e4s_dpacks",                                                             # disc_autograd
    "_mlp_pack",                                                               # networks.Net3 (stacked LocalMLPs)
    "_pack",                                                                   # stylegan2.ModulatedConv2d (its data lives in _e4s_bufs)
)


def invalidate_packs():
    """Drop every cached weight pack of every module (they are rebuilt on next use)."""
    global _GENERATION
    _GENERATION += 1


def invalidate_module_packs(modules):
    """Drop the cached weight packs held by each of `modules` (not recursive: pass every module whose packs must go).  The next
    use re-packs from the current weights.  Lifetime buffers (`_e4s_bufs`) stay: a re-pack writes them in place.  Other modules
    keep their packs."""
    for m in modules:
        d = vars(m)
        for name in PACK_ATTRS:
            if d.get(name) is not None:
                d[name] = None


def modules_owning(root, params):
    """The modules of `root` (itself included) that hold one of `params`, directly or through a child: the owners of every cache
    keyed on one of them (Net3 keeps the stacked LocalMLP weights on itself)."""
    ids = {id(p) for p in params}
    return [m for m in root.modules() if any(id(p) in ids for p in m.parameters())]


def param_key(*tensors):
    return (_GENERATION,) + tuple((t.data_ptr(), t._version) for t in tensors)
