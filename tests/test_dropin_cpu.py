"""The drop-in mechanism shared by log_amd.densify, prepare and decide (log_amd/_dropin.py), on two stand-in classes: no
GPU, no library, no reference."""
import pytest
import torch

from log_amd import _dropin
from log_amd._lib import LograstError


class Tree:
    def grow(self, n, scale=1):
        return ("Tree.grow", n, scale)


class Model:
    def step(self):
        return "Model.step"

    def prune(self, *args, **kwargs):
        return ("Model.prune", args, kwargs)


def make(events=None):
    """A registry over the two classes above; the bodies record whether grad was enabled and do as `events` tells them."""
    d = _dropin.DropIns("standin", lambda: {"grow": (Tree, "grow"), "step": (Model, "step"), "prune": (Model, "prune")})
    events = events if events is not None else {}

    @d.dropin
    def grow(self, n, scale=1):
        """doc of grow"""
        events.setdefault("grad", []).append(torch.is_grad_enabled())
        if "raise" in events:
            raise events["raise"]
        return ("ours", n, scale)

    @d.dropin
    def step(self):
        return "ours"

    @d.dropin
    def prune(self, *args, **kwargs):
        raise _dropin.Fallback(events.get("why", "why"))
    return d, grow, step, prune


@pytest.fixture
def classes():
    saved = (Tree.grow, Model.step, Model.prune)
    yield saved
    Tree.grow, Model.step, Model.prune = saved


def test_install_twice_and_uninstall_by_identity(classes):
    d, grow, step, prune = make()
    assert grow.__name__ == "grow" and grow.__doc__ == "doc of grow"
    targets = d.install()
    assert targets["grow"] == (Tree, "grow") and (Tree.grow, Model.step, Model.prune) == (grow, step, prune)
    assert (d.original("grow"), d.original("step"), d.original("prune")) == classes
    d.install()                                                   # our own functions are not saved as "the originals"
    assert (Tree.grow, Model.step, Model.prune) == (grow, step, prune)
    assert (d.original("grow"), d.original("step"), d.original("prune")) == classes
    assert Tree().grow(3) == ("ours", 3, 1)
    d.uninstall()
    assert (Tree.grow, Model.step, Model.prune) == classes


def test_a_method_replaced_before_the_first_save_is_an_error(classes):
    d, grow, step, prune = make()
    Model.step = step
    with pytest.raises(LograstError, match=r"log_amd\.standin: the reference's step was replaced before install\(\) could save it"):
        d.install()
    assert Tree.grow is classes[0] and Model.prune is classes[2]          # nothing was patched


def test_fallback_calls_the_original_with_the_callers_arguments(classes, caplog):
    events = {}
    d, grow, step, prune = make(events)
    d.install()
    m = Model()
    with caplog.at_level("WARNING", logger="log_amd"):
        for _ in range(3):
            assert m.prune(1, 2, keep=True, other=None) == ("Model.prune", (1, 2), {"keep": True, "other": None})
        assert d.stats() == {"calls": {"prune": 3}, "fallbacks": {("prune", "why"): 3}, "readbacks": {}}
        first = [r.getMessage() for r in caplog.records]
        assert first == ["log_amd.standin.prune: why -- the reference's method runs instead (logged once)"]
        events["why"] = "another reason"
        assert m.prune() == ("Model.prune", (), {}) and m.prune() == ("Model.prune", (), {})
    assert d.stats()["fallbacks"] == {("prune", "why"): 3, ("prune", "another reason"): 2} and d.stats()["calls"] == {"prune": 5}
    assert [r.getMessage() for r in caplog.records] == first + [
        "log_amd.standin.prune: another reason -- the reference's method runs instead (logged once)"]
    with d.substituted(prune=lambda self, *a, **k: "stand-in"):
        assert m.prune(7) == "stand-in"
    assert m.prune(7) == ("Model.prune", (7,), {})


def test_bodies_run_without_grad_and_other_exceptions_propagate(classes):
    events = {}
    d, grow, step, prune = make(events)
    d.install()
    assert torch.is_grad_enabled()
    assert Tree().grow(2, scale=5) == ("ours", 2, 5)
    assert events["grad"] == [False] and torch.is_grad_enabled()
    events["raise"] = ValueError("bad flag")
    with pytest.raises(ValueError, match="bad flag"):
        Tree().grow(2)
    assert torch.is_grad_enabled()
    assert d.stats() == {"calls": {"grow": 2}, "fallbacks": {}, "readbacks": {}}
    events["raise"] = _dropin.Fallback("not covered")
    assert Tree().grow(2, scale=3) == ("Tree.grow", 2, 3)
    assert d.stats()["fallbacks"] == {("grow", "not covered"): 1}


def test_stats_are_copies_and_reset_keeps_the_originals(classes):
    d, grow, step, prune = make()
    d.install()
    Model().prune()
    d.count("readbacks", "grow")
    st = d.stats()
    st["calls"]["prune"] = 99
    st["fallbacks"].clear()
    del st["readbacks"]["grow"]
    assert d.stats() == {"calls": {"prune": 1}, "fallbacks": {("prune", "why"): 1}, "readbacks": {"grow": 1}}
    d.reset_stats()
    assert d.stats() == {"calls": {}, "fallbacks": {}, "readbacks": {}}
    assert (d.original("grow"), d.original("step"), d.original("prune")) == classes
    d.uninstall()
    assert (Tree.grow, Model.step, Model.prune) == classes


def test_the_checks_name_their_reason():
    with pytest.raises(_dropin.Fallback, match="tensors are not on the GPU"):
        _dropin.device_and_rows(torch.zeros(4, 3))
    with pytest.raises(_dropin.Fallback, match="tensors are not on the GPU"):
        _dropin.tensor(None, torch.device("cpu"), torch.float32, (4,), "x")
    cpu = torch.device("cpu")
    with pytest.raises(_dropin.Fallback, match=r"x: torch.int32\(4,\) where torch.float32\(4,\) is needed"):
        _dropin.tensor(torch.zeros(4, dtype=torch.int32), cpu, torch.float32, (4,), "x")
    with pytest.raises(_dropin.Fallback, match=r"x: torch.float32\(5,\)"):
        _dropin.tensor(torch.zeros(5), cpu, torch.float32, (4,), "x")
    strided = torch.zeros(4, 2)[:, 0]
    got = _dropin.tensor(strided, cpu, torch.float32, (4,), "x")
    assert got.is_contiguous() and not got.requires_grad
    assert _dropin.flag_u8(torch.tensor([True, False, True]), cpu, 3).tolist() == [1, 0, 1]
    assert _dropin.flag_u8(torch.tensor([5, 0, -1]), cpu, 3).dtype == torch.uint8
    assert _dropin.flag_u8(torch.tensor([5, 0, -1]), cpu, 3).tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="flag of shape"):
        _dropin.flag_u8(torch.zeros(4, dtype=torch.bool), cpu, 3)
    with pytest.raises(_dropin.Fallback, match="flags are not on the model's device"):
        _dropin.flag_u8([True], cpu, 1)
