"""e4s_amd.packs on the host: the one cache of weight packs per module (cached / derived) and the ways to drop it.  Plain nn.Modules,
CPU tensors, counting builds."""
import copy

import pytest
import torch
from torch import nn

from e4s_amd import packs


class Counter:
    """build() for packs.cached / build(value) for packs.derived: counts its calls and records the grad mode it ran under."""

    def __init__(self, tag="v"):
        self.tag, self.calls, self.grad_modes = tag, 0, []

    def __call__(self, *value):
        self.calls += 1
        self.grad_modes.append(torch.is_grad_enabled())
        return (self.tag, self.calls) + value


def _module():
    return nn.Linear(3, 2)


def test_one_build_per_key_and_build_runs_without_grad():
    m, build = _module(), Counter()
    assert torch.is_grad_enabled()
    first = packs.cached(m, "w", (m.weight, m.bias), build)
    for _ in range(3):
        assert packs.cached(m, "w", (m.weight, m.bias), build) is first
    assert build.calls == 1 and first == ("v", 1)
    assert build.grad_modes == [False] and torch.is_grad_enabled()


def test_rebuild_after_every_change_of_the_key():
    m, build = _module(), Counter()
    get = lambda extra=(): packs.cached(m, "w", (m.weight, m.bias), build, extra)
    get()
    with torch.no_grad():
        m.bias.add_(0)                                       # an in-place update through the tensor (any of the key's tensors)
    assert get() == ("v", 2) and get() == ("v", 2)
    packs.invalidate_packs()
    assert get() == ("v", 3) and get() == ("v", 3)
    packs.invalidate_module_packs([m])
    assert "_e4s_packs" not in vars(m)
    assert get() == ("v", 4) and get() == ("v", 4)
    assert get((True,)) == ("v", 5) and get((True,)) == ("v", 5)            # a change of `extra` (a precision flag, a padded width, ...)
    assert get((False,)) == ("v", 6)
    m.weight = nn.Parameter(m.weight.detach().clone())      # other storage
    assert get((False,)) == ("v", 7) and build.calls == 7


def test_an_update_through_data_is_not_seen():
    """The known blind spot (the reference's EMA writes p.data): what invalidate_packs() exists for."""
    m, build = _module(), Counter()
    get = lambda: packs.cached(m, "w", (m.weight,), build)
    get()
    m.weight.data.mul_(0.5).add_(1.0)
    assert get() == ("v", 1) and build.calls == 1           # stale
    packs.invalidate_packs()
    assert get() == ("v", 2)


def test_a_derived_image_is_built_lazily_once_and_dies_with_its_slot():
    m, build, split, bwd = _module(), Counter(), Counter("split"), Counter("bwd")
    get = lambda: packs.cached(m, "w", (m.weight,), build)
    get()
    assert split.calls == 0 and vars(m)["_e4s_packs"]["w"][2] == {}                      # not built with the base pack
    image = packs.derived(m, "w", "split", split)
    assert image == ("split", 1, ("v", 1))                                                 # build(value of the slot)
    get()
    assert packs.derived(m, "w", "split", split) is image and split.calls == 1
    assert packs.derived(m, "w", "bwd", bwd) == ("bwd", 1, ("v", 1)) and split.calls == 1 # images of one slot do not disturb each other
    with torch.no_grad():
        m.weight.add_(0)
    get()
    assert vars(m)["_e4s_packs"]["w"][2] == {} and split.calls == 1                      # dropped with the value; not rebuilt eagerly
    assert packs.derived(m, "w", "split", split) == ("split", 2, ("v", 2))
    assert bwd.calls == 1
    packs.invalidate_module_packs([m])
    get()
    assert packs.derived(m, "w", "split", split) == ("split", 3, ("v", 3))


def test_a_late_caller_is_refused_once_the_slot_was_rekeyed_or_dropped():
    """An autograd backward comes back to the slot its forward made current: with the key it saw it is never served another weight's image."""
    m, build, img = _module(), Counter(), Counter("img")
    packs.cached(m, "w", (m.weight,), build, (32,))
    key = packs.param_key(m.weight) + (32,)
    assert vars(m)["_e4s_packs"]["w"][0] == key
    assert packs.derived(m, "w", "img", img, key) == ("img", 1, ("v", 1))
    with torch.no_grad():
        m.weight.add_(0)
    packs.cached(m, "w", (m.weight,), build, (32,))
    with pytest.raises(RuntimeError, match="re-packed for other weights"):
        packs.derived(m, "w", "img", img, key)
    packs.invalidate_module_packs([m])
    with pytest.raises(RuntimeError, match="no current pack"):
        packs.derived(m, "w", "img", img, key)
    assert img.calls == 1


def test_two_slots_of_one_owner_do_not_disturb_each_other():
    m, a, b, img = _module(), Counter("a"), Counter("b"), Counter("img")
    get_a = lambda: packs.cached(m, "a", (m.weight,), a, (32,))
    get_b = lambda: packs.cached(m, "b", (m.bias,), b)
    get_a(), get_b()
    packs.derived(m, "a", "img", img)
    with torch.no_grad():
        m.bias.add_(0)
    assert get_a() == ("a", 1, ) and get_b() == ("b", 2)
    assert packs.derived(m, "a", "img", img) == ("img", 1, ("a", 1)) and img.calls == 1
    with torch.no_grad():
        m.weight.add_(0)
    assert get_a() == ("a", 2) and get_b() == ("b", 2)
    assert a.calls == 2 and b.calls == 2


def test_invalidate_module_packs_is_per_module_and_spares_the_survivors():
    root = nn.Sequential(_module(), _module())
    m, sibling = root[0], root[1]
    builds = {x: Counter() for x in (root, m, sibling)}
    get = lambda x: packs.cached(x, "w", tuple(x.parameters()), builds[x])
    for x in builds:
        get(x)
        vars(x)["_e4s_bufs"] = {"w": "lifetime"}
        x._e4s_style_plan = {"key": "addresses"}
        x._e4s_style_ok = True
    packs.invalidate_module_packs([m])
    for x in builds:
        get(x)
        assert vars(x)["_e4s_bufs"] == {"w": "lifetime"} and x._e4s_style_plan == {"key": "addresses"} and x._e4s_style_ok is True
    assert builds[m].calls == 2 and builds[sibling].calls == 1 and builds[root].calls == 1
    packs.invalidate_module_packs([root])                    # not recursive
    for x in builds:
        get(x)
    assert builds[root].calls == 2 and builds[m].calls == 2 and builds[sibling].calls == 1


def test_a_deep_copy_repacks_on_first_use():
    """The EMA twin: its copied keys hold the original's pointers, so nothing of the original's packs is served for the copy's weights."""
    m, build = _module(), Counter()
    packs.cached(m, "w", (m.weight,), build)
    twin = copy.deepcopy(m)
    assert packs.cached(twin, "w", (twin.weight,), build) == ("v", 2)
    assert packs.cached(m, "w", (m.weight,), build) == ("v", 1) and build.calls == 2
