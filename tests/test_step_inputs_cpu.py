"""trainer._StepInput: the rule one static input image of GraphedStep lives by (load, snapshot, restore), on CPU tensors.  No GPU, no library."""
import pytest
import torch

# (noun of "modified in place", noun of "replaced since", argument name, whether load checks the shape): the four images of GraphedStep
SLOTS = [("ground-truth tensor", "target", "gt_image", False), ("depth target", "depth target", "gt_depth", False),
         ("weight image", "weight image", "weight", True), ("depth weight image", "depth weight image", "depth_weight", True)]


@pytest.fixture(params=SLOTS, ids=[s[2] for s in SLOTS])
def slot(request):
    from gaussian_lic_amd.trainer import _StepInput
    noun, loaded_noun, arg, check_shape = request.param
    return _StepInput(noun, arg, torch.zeros(2, 3), loaded_noun=loaded_noun, check_shape=check_shape)


def _values(k):
    return torch.arange(6, dtype=torch.float32).reshape(2, 3) + 10.0 * k


def test_a_new_slot_starts_at_serial_zero_on_the_buffer_it_was_given():
    from gaussian_lic_amd.trainer import _StepInput
    buf = _values(1)
    s = _StepInput("weight image", "weight", buf)
    assert s.serial == 0 and s.buffer is buf and s.snapshot(None) == (None, None, 0)


def test_load_of_the_buffers_own_storage_copies_nothing(slot):
    slot.buffer.copy_(_values(1))
    before = slot.buffer._version
    slot.load(slot.buffer.view(6).view(2, 3))          # a view of the same storage, as the step's own buffer handed back
    assert slot.serial == 0 and slot.buffer._version == before and torch.equal(slot.buffer, _values(1))


def test_load_of_another_tensor_copies_and_counts(slot):
    slot.load(_values(1))
    assert slot.serial == 1 and torch.equal(slot.buffer, _values(1))
    slot.load(_values(2))
    assert slot.serial == 2 and torch.equal(slot.buffer, _values(2))


def test_restore_refuses_a_tensor_modified_in_place(slot):
    t = _values(1)
    slot.load(t)
    snap = slot.snapshot(t)
    assert snap[0] is t and snap[1:] == (t._version, 1)
    t.add_(1)
    with pytest.raises(RuntimeError, match=f"the {slot.noun} of a step .* modified in place"):
        slot.restore(snap)
    assert slot.serial == 1 and torch.equal(slot.buffer, _values(1))      # refused before anything was copied


def test_restore_refuses_the_loaded_image_once_it_was_replaced(slot):
    slot.load(_values(1))
    snap = slot.snapshot(None)
    slot.load(_values(2))
    with pytest.raises(RuntimeError, match=f"ran on a {slot.loaded_noun} that has been replaced since .*issued with {slot.arg}=None"):
        slot.restore(snap)
    assert torch.equal(slot.buffer, _values(2))


def test_restore_of_the_loaded_image_is_silent_while_nothing_was_loaded(slot):
    slot.load(_values(1))
    snap = slot.snapshot(None)
    before = slot.buffer._version
    slot.restore(snap)
    assert slot.serial == 1 and slot.buffer._version == before and torch.equal(slot.buffer, _values(1))


def test_restore_puts_the_steps_own_tensor_back(slot):
    t, u = _values(1), _values(2)
    slot.load(t)
    snap = slot.snapshot(t)
    slot.load(u)
    assert torch.equal(slot.buffer, u)
    slot.restore(snap)
    assert torch.equal(slot.buffer, t) and slot.serial == 3 and t._version == snap[1]


@pytest.mark.parametrize("noun,loaded_noun,arg,check_shape", [s for s in SLOTS if s[3]], ids=[s[2] for s in SLOTS if s[3]])
def test_a_wrong_shape_is_refused_where_the_shape_is_checked(noun, loaded_noun, arg, check_shape):
    from gaussian_lic_amd.trainer import _StepInput
    s = _StepInput(noun, arg, _values(1), loaded_noun=loaded_noun, check_shape=check_shape)
    with pytest.raises(ValueError, match=f"{arg} of shape \\(3, 3\\) given to a step built for \\(2, 3\\)"):
        s.load(torch.ones(3, 3))
    with pytest.raises(ValueError, match="shape"):
        s.load(torch.ones(3))                             # (would broadcast: refused all the same)
    assert s.serial == 0 and torch.equal(s.buffer, _values(1))
