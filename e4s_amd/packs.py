"""The re-packed weight images of the modules (tap-packed, polyphase, split-bf16, folded BatchNorm, stacked LocalMLPs) and their keys.

THE RULE: a weight pack is stored on a module through this file or not at all.  All packs of a module live in ONE dict,
`vars(module)["_e4s_packs"]`: slot -> (key, value, {name: derived image}).  `cached()` fills a slot, `derived()` hangs a lazily built
image (split-bf16 operand, backward layout, Winograd transform, ...) on the slot's current value, and `invalidate_module_packs()`
drops the dict.  Nothing else has to know which slots exist, so a new network or a new derived image cannot be forgotten by it.

A pack is valid for one (generation, storage, version) of its source tensors (`param_key`).  `Tensor._version` advances on every
in-place update made THROUGH the tensor (optimizer steps, `load_state_dict`, `p.copy_()` under no_grad) but NOT on updates made
through `p.data` (the reference's EMA, src/utils/torch_utils.py:189-194, writes `p.data.mul_().add_()`).  Code that mutates weights
behind autograd's back must call `invalidate_packs()` afterwards (the overlay's `src.utils.torch_utils.accumulate` does); it bumps a
process-wide generation that is part of every key.  A captured HIP graph (networks.GraphedFaceSwap) bakes the pack pointers in:
re-capture it after any weight change.  `copy.deepcopy(module)` copies the dict with the original's pointers in its keys, so the
twin re-packs on first use.

A captured TRAIN step (train.graphed_g_step / graphed_d_step) reads the packs of a network that another step trains between its
replays.  A cache hit at capture time would bake in a pack allocated eagerly, which serves the weights of the capture forever and
is freed by the next eager consumer that re-packs.  So the step's body calls `invalidate_module_packs()` on the modules that own a
trained parameter: the capture then records the re-pack kernels, into the graph's own memory pool (or into the module's lifetime
buffers, `_e4s_bufs`, which stay), and every replay re-packs from the weights of the moment.  Whatever a captured step re-packs and
something else holds the address of (the style prologue's job tables) belongs in such a lifetime buffer, written with `out=`."""
import torch

_GENERATION = 0


def invalidate_packs():
    """Drop every cached weight pack of every module (they are rebuilt on next use)."""
    global _GENERATION
    _GENERATION += 1


def invalidate_module_packs(modules):
    """Drop the cached weight packs held by each of `modules` (not recursive: pass every module whose packs must go).  The next
    use re-packs from the current weights.  Lifetime buffers (`_e4s_bufs`) and the style plan stay: a re-pack writes them in place.
    Other modules keep their packs."""
    for m in modules:
        vars(m).pop("_e4s_packs", None)


def modules_owning(root, params):
    """The modules of `root` (itself included) that hold one of `params`, directly or through a child: the owners of every cache
    keyed on one of them (Net3 keeps the stacked LocalMLP weights on itself)."""
    ids = {id(p) for p in params}
    return [m for m in root.modules() if any(id(p) in ids for p in m.parameters())]


def param_key(*tensors):
    return (_GENERATION,) + tuple((t.data_ptr(), t._version) for t in tensors)


def cached(owner, slot, tensors, build, extra=()):
    """The value build() made for this (generation, storage, version) of `tensors` (+ extra: whatever else the value depends on);
    rebuilt, and every image derived from it dropped, when the key changes.  build runs under torch.no_grad()."""
    key = (_GENERATION, *[(t.data_ptr(), t._version) for t in tensors], *extra)          # == param_key(*tensors) + extra
    try:
        hit = owner.__dict__["_e4s_packs"][slot]
        if hit[0] == key:
            return hit[1]
    except KeyError:
        pass
    with torch.no_grad():
        value = build()
    owner.__dict__.setdefault("_e4s_packs", {})[slot] = (key, value, {})
    return value


def derived(owner, slot, name, build, key=None):
    """A lazily built image of the CURRENT value of `slot` (split-bf16 operand, backward layout, Winograd transform, ...): build(value)
    runs on first use and the image lives and dies with that value.  The slot must be current: call cached() first (a weight pack is
    read through cached() on every use anyway).  A caller that comes back later than that (an autograd backward) passes the `key` it
    made the slot current with (param_key(*tensors) + extra) and is refused when the slot has been re-keyed or dropped since, instead of being served another weight's image."""
    try:
        have, value, images = owner.__dict__["_e4s_packs"][slot]
    except KeyError:
        raise RuntimeError(f"packs.derived: {type(owner).__name__} has no current pack in slot {slot!r} (dropped since packs.cached "
                           "made it; call cached() first)") from None
    if key is not None and key != have:
        raise RuntimeError(f"packs.derived: slot {slot!r} of {type(owner).__name__} was re-packed for other weights since this handle "
                           "was made (a weight update or invalidate_packs() between a forward and its backward)")
    image = images.get(name)
    if image is None:
        image = images[name] = build(value)
    return image
