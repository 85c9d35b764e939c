"""The poisoned arena of footprint_tools catches what it is meant to catch (CPU tensors, no GPU)."""
import pytest
import torch

from footprint_tools import POISON, Arena


def _setup():
    a = Arena(torch.device("cpu"), 1 << 16)
    x = a.put(torch.arange(15, dtype=torch.float32).view(3, 5), ld=12, name="x")
    y = a.carve(3, 5, 8, torch.float32, writable=True, name="y")
    c = a.carve(3, 20, 48, torch.int8, misalign=4, writable=32, name="codes")
    f = a.carve_flat(7, torch.float32, writable=True, name="flat")
    a.seal()
    return a, x, y, c, f


def test_pattern_and_alignment():
    fresh = Arena(torch.device("cpu"), 4096)
    assert bytes(fresh.buf[:4].tolist()) == bytes(POISON)
    assert torch.isnan(fresh.buf.view(torch.float32)).all()
    assert torch.isnan(fresh.buf.view(torch.float16)).all()
    assert (fresh.buf.view(torch.int8) != 0).all()
    a, x, y, c, f = _setup()
    for v in (x, y, f):
        assert v.data_ptr() % 16 == 0 and v.data_ptr() % 32 == 16
    assert c.data_ptr() % 4 == 0 and c.data_ptr() % 8 == 4
    assert x.stride(0) == 12 and y.stride(0) == 8 and c.stride(0) == 48
    # pad columns and guard rows of an input keep the poison
    full = torch.as_strided(x, (5, 12), (12, 1), x.storage_offset() - 12)
    assert torch.isnan(full[0]).all() and torch.isnan(full[4]).all() and torch.isnan(full[1:4, 5:]).all()
    assert torch.equal(x, torch.arange(15, dtype=torch.float32).view(3, 5))


def test_writes_inside_the_writable_set_pass():
    a, x, y, c, f = _setup()
    y.copy_(x * 2)
    torch.as_strided(c, (3, 32), (48, 1), c.storage_offset()).zero_()   # codes and the zeroed padding up to kpad = 32
    f.fill_(1.0)
    a.assert_untouched()


def _raises(a, *words):
    with pytest.raises(AssertionError) as e:
        a.assert_untouched()
    for w in words:
        assert w in str(e.value), str(e.value)


def test_write_one_past_a_row_end_is_caught():
    a, x, y, c, f = _setup()
    torch.as_strided(y, (1,), (1,), y.storage_offset() + 8 + 5).fill_(0.0)    # row 1, column 5 of 5
    _raises(a, "y row 1 column 5", "pad column")


def test_write_past_kpad_is_caught():
    a, x, y, c, f = _setup()
    torch.as_strided(c, (1,), (1,), c.storage_offset() + 2 * 48 + 32).fill_(0)
    _raises(a, "codes row 2 column 32", "pad column")


def test_write_in_a_tail_guard_row_is_caught():
    a, x, y, c, f = _setup()
    torch.as_strided(y, (1,), (1,), y.storage_offset() + 3 * 8 + 2).fill_(0.0)
    _raises(a, "y row 3 column 2", "tail guard row")


def test_write_in_a_lead_guard_row_is_caught():
    a, x, y, c, f = _setup()
    torch.as_strided(y, (1,), (1,), y.storage_offset() - 8 + 4).fill_(0.0)
    _raises(a, "y row -1 column 4", "lead guard row")


def test_write_in_another_carves_input_is_caught():
    a, x, y, c, f = _setup()
    x[2, 1] = 99.0
    _raises(a, "x row 2 column 1", "input")


def test_write_past_a_flat_carve_is_caught():
    a, x, y, c, f = _setup()
    torch.as_strided(f, (1,), (1,), f.storage_offset() + 7).fill_(0.0)
    _raises(a, "first at arena byte")
