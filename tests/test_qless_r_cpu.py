"""CPU: qrk_dense_qless_r without a device -- the level schedule and the workspace size as the header states them,
the argument refusals that touch no device, and the numpy prototype of the reduced LM chain (tests/angular_lm_reduced_reference.py)
against angular_lmpar_reference.chain_evaluate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import angular_lm_reduced_reference as red
import angular_lmpar_reference as ref

NEW = ("qrk_dense_qless_r_work", "qrk_dense_qless_r", "qrk_dense_qless_r_levels", "qrk_dense_qless_r_kernel_name")
ROWS = [0, 1, 5, 255, 256, 257, 700, 1024, 1025, 4097, 70001, 262144, 262145, 300001, 10 ** 6, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1]
COLS = [1, 2, 6, 8, 9, 16, 17, 31, 32]
CAP = 8


def lib():
    from qrkit_amd import _capi as capi
    return capi.lib()


def levels(rows, cols, cap=CAP):
    lr, lc = (C.c_int64 * max(cap, 1))(*([-7] * max(cap, 1))), (C.c_int64 * max(cap, 1))(*([-7] * max(cap, 1)))
    n = lib().qrk_dense_qless_r_levels(rows, cols, lr, lc, cap)
    return n, list(lr), list(lc)


def test_new_symbols_are_declared_exported_and_bound():
    from qrkit_amd import _capi as capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qrkit_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/qrkit_amd.h"
        assert name in capi.EXPORTS
        assert getattr(lib(), name).argtypes is not None, f"{name} has no ctypes signature"


@pytest.mark.parametrize("cols", COLS)
def test_schedule_holds_its_contract(cols):
    for rows in ROWS:
        n, lr, lc = levels(rows, cols)
        assert 1 <= n <= 3 <= CAP, (rows, cols, n)
        assert lr[0] == rows
        for l in range(n):
            assert lc[l] > 0 and lc[l] % 256 == 0, (rows, cols, lr, lc)
            chunks = -(-lr[l] // lc[l])
            if l + 1 < n:
                assert chunks > 1 and lr[l + 1] == chunks * cols, "a level's triangles are the next level's rows"
                assert lr[l + 1] < lr[l], "a level must shrink"
            else:
                assert chunks <= 1, "the last level is one chunk"
        assert all(v == -7 for v in lr[n:] + lc[n:]), "entries beyond the levels were written"
        # level 1 leaves about 1024 workgroups at most, whatever the size: the grid is a function of the shape alone
        assert -(-rows // lc[0]) <= 1025
        # the workspace as the header lays it out: level 1's triangles, then level 2's
        need = (lr[1] * cols if n >= 2 else 0) + (lr[2] * cols if n >= 3 else 0)
        assert lib().qrk_dense_qless_r_work(rows, cols) == max(need, 1)


def test_schedule_cases_the_gpu_tests_rely_on():
    assert levels(700, 6)[:2] == (2, [700, 18] + [-7] * 6)                 # three level-1 chunks and a second level
    assert levels(700, 6)[2][:2] == [256, 256]
    assert levels(256, 32)[0] == 1 and levels(257, 32)[0] == 2
    n, lr, lc = levels(300001, 6)
    assert n == 3 and lc[0] == 512
    assert levels(70001, 32)[0] == 3


def test_schedule_cap_and_refusals():
    # fewer slots than levels: the count is the schedule's, only `cap` entries are written
    n, lr, lc = levels(300001, 6, cap=2)
    assert n == 3 and lr[:2] == [300001, 3516] and lc[:2] == [512, 1024]
    n, lr, lc = levels(300001, 6, cap=0)
    assert n == 3 and lr == [-7] and lc == [-7]
    L = lib()
    assert L.qrk_dense_qless_r_levels(300001, 6, None, None, 4) == 3
    assert L.qrk_dense_qless_r_levels(100, 0, None, None, 4) == 0
    assert L.qrk_dense_qless_r_levels(-1, 6, None, None, 4) == -1
    assert L.qrk_dense_qless_r_levels(100, -1, None, None, 4) == -1
    assert L.qrk_dense_qless_r_levels(100, 33, None, None, 4) == -1
    assert L.qrk_dense_qless_r_levels(100, 6, None, None, -1) == -1


def test_work_and_chunks_are_monotone():
    L = lib()
    table = np.array([[L.qrk_dense_qless_r_work(r, c) for c in COLS] for r in ROWS], dtype=object)
    assert np.all(table >= 1)
    # more columns never need less; more rows never need less while the level-1 chunk is the same (a larger chunk means fewer
    # triangles: the level-1 chunk itself is monotone in the rows instead)
    assert all(table[i, j] <= table[i, j + 1] for i in range(len(ROWS)) for j in range(len(COLS) - 1))
    for j, c in enumerate(COLS):
        chunks = [levels(r, c)[2][0] for r in ROWS]
        assert all(a <= b for a, b in zip(chunks, chunks[1:]))
        for i in range(len(ROWS) - 1):
            if chunks[i] == chunks[i + 1]:
                assert table[i, j] <= table[i + 1, j], (ROWS[i], c)


def test_null_and_invalid_arguments_are_rejected_without_a_gpu():
    from qrkit_amd import _capi as capi
    L, I = lib(), capi.STATUS_INVALID_ARGUMENT
    assert L.qrk_dense_qless_r(None, None, 0, 0, 0, None, 0, None) == I
    assert L.qrk_dense_qless_r(None, 8, 8, 8, 2, 8, 2, 8) == I
    assert L.qrk_dense_qless_r(None, 8, 8, 8, 33, 8, 33, 8) == I                 # (the NULL handle comes before the column limit)
    assert L.qrk_dense_qless_r_kernel_name(-1, 4) == b"" and L.qrk_dense_qless_r_kernel_name(4, -1) == b""
    assert b"unsupported" in L.qrk_dense_qless_r_kernel_name(100, 33)
    assert L.qrk_dense_qless_r_kernel_name(100, 8) == b"qrk::qless::dense_qless_r_kernel<8>"
    assert L.qrk_dense_qless_r_kernel_name(100, 9) == b"qrk::qless::dense_qless_r_kernel<16>"
    assert L.qrk_dense_qless_r_kernel_name(100, 17) == b"qrk::qless::dense_qless_r_kernel<32>"


# ---- the numpy prototype of the reduced chain ---------------------------------------------------------------------------------------------

def test_prototype_tsqr_r_is_an_r_factor():
    rng = np.random.default_rng(3)
    for rows, cols in ((0, 4), (3, 6), (700, 6), (1000, 25)):
        A = rng.standard_normal((rows, cols))
        for chunk in (7, 64, None):
            R = red.tsqr_r(A, chunk)
            assert R.shape == (cols, cols) and not np.tril(R, -1).any()
            assert np.max(np.abs(R.T @ R - A.T @ A)) <= 1e-12 * max(1.0, np.max(np.abs(A.T @ A)) if rows else 1.0)


@pytest.mark.parametrize("name", sorted(ref.GAUSSIAN))
def test_reduced_prototype_matches_the_stacked_chain(name):
    p = ref.problem(name)
    f = ref.KeptFactors(p)
    worst = 0.0
    for diag in (None, p.norms):
        for par in (0.0, 1e-3, 1.0, 1e3):
            x, s0, s1 = ref.chain_evaluate(f, diag, par)
            for chunk in (7, 64, None):
                rx, rs0, rs1 = red.chain_evaluate_reduced(f, diag, par, chunk)
                err = max(np.max(np.abs(rx - x)) / np.max(np.abs(x)), abs(rs0 - s0) / s0, abs(rs1 - s1) / s1)
                worst = max(worst, float(err))
    print(f"{name}: reduced against stacked chain, x / s0 / s1: worst {worst:.2e}")
    assert worst <= 1e-12
