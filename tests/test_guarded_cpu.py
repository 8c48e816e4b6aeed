"""The guard-band net of tests/guarded.py is not vacuous: on CPU tensors, numpy functions stand in for a kernel that gets raw
"pointers" (the whole guarded buffer and the payload's offset in it, so that a stand-in CAN reach past its extent).

The operation is y = 2 x on n doubles (column by column on a strided panel).  A faithful stand-in passes; four mutants must each make
check() fail with a message that names the array and what happened; a sixth stand-in reads one element past its input and adds it
into an output, which must come back NaN and be caught.
"""
import numpy as np
import pytest
import torch

import guarded
from guarded import G, Net


def views(*arrays):
    """(numpy view of the whole buffer, offset of the payload) per array: what a raw pointer gives a kernel"""
    return [(a.buf.numpy(), a.off) for a in arrays]


def faithful(x, y, n):
    (xb, xo), (yb, yo) = views(x, y)
    yb[yo:yo + n] = 2.0 * xb[xo:xo + n]


def writes_one_after(x, y, n):
    faithful(x, y, n)
    (yb, yo), = views(y)
    yb[yo + n] = 1.0


def writes_one_before(x, y, n):
    faithful(x, y, n)
    (yb, yo), = views(y)
    yb[yo - 1] = 1.0


def writes_its_input(x, y, n):
    faithful(x, y, n)
    (xb, xo), = views(x)
    xb[xo + n // 2] = 0.0


def leaves_the_last_unwritten(x, y, n):
    (xb, xo), (yb, yo) = views(x, y)
    yb[yo:yo + n - 1] = 2.0 * xb[xo:xo + n - 1]


def reads_one_past_its_input(x, y, n):
    faithful(x, y, n)
    (xb, xo), (yb, yo) = views(x, y)
    yb[yo + n - 1] += xb[xo + n]


def make(n, shift):
    net = Net("cpu", shift)
    x = net.inp("x", np.arange(1, n + 1, dtype=np.float64))
    y = net.out("y", n)
    return net, x, y


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 7, 64, 129])
def test_faithful_stand_in_passes(n, shift):
    net, x, y = make(n, shift)
    assert y.ptr % 16 == 8 * shift and x.ptr % 16 == 8 * shift
    assert y.buf.numel() == G + shift + n + G
    faithful(x, y, n)
    net.check()
    np.testing.assert_array_equal(y.get(), 2.0 * np.arange(1, n + 1))


MUTANTS = [
    (writes_one_after, r"y: the right guard was written at offset 7 from the payload's start"),
    (writes_one_before, r"y: the left guard was written at offset -1 from the payload's start"),
    (writes_its_input, r"x: an input was written at offset 3"),
    (leaves_the_last_unwritten, r"y: payload element 6 of 7 was not written"),
    (reads_one_past_its_input, r"y: payload element 6 of 7 is NaN"),
]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("mutant,message", MUTANTS, ids=[m.__name__ for m, _ in MUTANTS])
def test_each_mutant_is_caught(mutant, message, shift):
    net, x, y = make(7, shift)
    mutant(x, y, 7)
    with pytest.raises(AssertionError, match=message):
        net.check()


@pytest.mark.parametrize("shift", [0, 1])
def test_no_elements_still_guards_both_sides(shift):
    """n = 0: the pointer points into the middle of the guard and any write is outside"""
    net, x, y = make(0, shift)
    net.check()
    writes_one_after(x, y, 0)
    with pytest.raises(AssertionError, match="y: the right guard was written at offset 0"):
        net.check()


def test_the_sentinel_is_a_nan_that_compares_bitwise():
    y = guarded.guarded(3, torch.float64, "out", 1, "cpu", name="y")
    assert torch.isnan(y.buf).all() and bool((y.bits == guarded.SENTINEL_F64).all())
    p = guarded.guarded(3, torch.int32, "out", 1, "cpu", name="perm")
    assert bool((p.bits == guarded.SENTINEL_I32).all()) and p.ptr % 16 == 4
    y.payload()[:] = float("nan")                           # an ordinary NaN written into the payload is "written", and then "NaN"
    with pytest.raises(AssertionError, match="y: payload element 0 of 3 is NaN"):
        y.check()


def test_declared_untouched_elements_must_keep_the_sentinel():
    net = Net("cpu", 0)
    y = net.out("trace", 6, untouched=np.arange(6) >= 4)
    y.payload()[:4] = 1.0
    net.check()
    y.payload()[5] = 0.0
    with pytest.raises(AssertionError, match="trace: element 5 is documented as not touched and was written"):
        net.check()


# ---- a strided panel: rows < ld ------------------------------------------------------------------------------------------------------

def panel_stand_in(x, y, rows, ncols, extra_row=0, skip_last=False):
    (xb, xo), (yb, yo) = views(x, y)
    for j in range(ncols):
        h = rows + (extra_row if j == 0 else 0)
        if skip_last and j == ncols - 1:
            h = rows - 1
        yb[yo + j * y.ld:yo + j * y.ld + h] = 2.0 * np.nan_to_num(xb[xo + j * x.ld:xo + j * x.ld + h], nan=1.0)


@pytest.mark.parametrize("shift", [0, 1])
def test_strided_panel(shift):
    rows, ncols = 5, 3
    data = np.arange(1.0, rows * ncols + 1).reshape(ncols, rows).T
    for extra, skip, message in ((0, False, None),
                                 (1, False, "qtc: a gap row between the logical height 5 and the leading dimension 9 was written at offset 5"),
                                 (0, True, "qtc: payload element 22 of 23 was not written")):
        net = Net("cpu", shift)
        x = net.panel_in("c", data, 7)
        y = net.panel_out("qtc", rows, ncols, 9)
        assert x.n == 2 * 7 + 5 and y.n == 2 * 9 + 5                 # (ncols - 1) ld + rows, not ncols ld
        panel_stand_in(x, y, rows, ncols, extra, skip)
        if message is None:
            net.check()
            np.testing.assert_array_equal(y.get(), 2.0 * data)
        else:
            with pytest.raises(AssertionError, match=message):
                net.check()
    net = Net("cpu", shift)                                          # no columns: no extent at all
    x, y = net.panel_in("c", np.zeros((rows, 0)), 7), net.panel_out("qtc", rows, 0, 9)
    assert x.n == 0 and y.n == 0 and y.get().shape == (rows, 0)
    net.check()


def test_a_read_of_a_gap_row_of_an_input_comes_back_nan():
    net = Net("cpu", 0)
    x = net.panel_in("c", np.ones((5, 2)), 7)
    y = net.panel_out("qtc", 5, 2, 5)
    (xb, xo), (yb, yo) = views(x, y)
    yb[yo:yo + 10] = 1.0
    yb[yo + 4] += xb[xo + 5]                                         # row 5 of column 0: between rows and ldc
    with pytest.raises(AssertionError, match="qtc: payload element 4 of 10 is NaN"):
        net.check()
