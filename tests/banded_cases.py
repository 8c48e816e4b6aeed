"""Banded matrices of untruncated dense strips and the table of panel classes of the CSR chain (qrk_bb_*): a plain helper module,
imported like helpers.py by tests/test_banded_layout.py, tests/test_banded_classes_gpu.py and tests/test_guarded_banded_gpu.py.

dense_strips(N, ms, n, s): strip i is ms x n at rows i ms, columns i s; the matrix is N ms x ((N - 1) s + n).  With
suggestedBlockCols = 2 every strip is one block, so the chain's panels are ms x n (the first) and (2 ms - s) x n (every later one:
the ms - s rows carried over, then the strip).  The reference's Q row layout holds for such a matrix when N = 2 or ms - s >= n
(include/qrkit_amd.h, qrk_bb_plan_create).
"""
import functools

import numpy as np
import scipy.sparse as sp


def dense_strips(N, ms, n, s, seed=3):
    """Values U(0.5, 5) as tests/test_banded.py::strip_matrix, CSR with sorted indices."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(ms), np.arange(n), indexing="ij")
    rows = np.concatenate([(r + i * ms).ravel() for i in range(N)])
    cols = np.concatenate([(c + i * s).ravel() for i in range(N)])
    J = sp.csr_matrix((rng.uniform(0.5, 5.0, len(rows)), (rows, cols)), shape=(N * ms, (N - 1) * s + n))
    J.sort_indices()
    return J


def panel_shapes(N, ms, n, s):
    """The panels (act_rows, ncols) of the chain on dense_strips(N, ms, n, s) with suggestedBlockCols = 2"""
    return [(ms, n)] + [(2 * ms - s, n)] * (N - 1)


# ((N, ms, n, s), the name qrk_bb_kernel_name gives for the LAST panel, the class the case is there for).  The thresholds the classes
# sit on are those of bb_qr_class, bb_chain2_smem and bb_t_smem (qrkit_amd/csrc/banded.hip): 32-column blocks while
# 32 (m | 1) + 5120 <= 20204 doubles of LDS, i.e. m <= 471; NR 3 / 4 / 8 row registers for m <= 192 / <= 256 / above; T packed in
# LDS while n (n + 1) / 2 * 8 + 2048 <= 160 KB, i.e. n <= 200; bb_chain_kernel beyond 256 columns or 1 024 rows.
CASES = [
    ((3, 24, 16, 8), "bb_chain2_kernel ob32 nr3 t_lds", "exactly one full 16-column group"),
    ((3, 96, 17, 9), "bb_chain2_kernel ob32 nr3 t_lds", "one partial block of 17, m = 183 odd"),
    ((3, 60, 33, 20), "bb_chain2_kernel ob32 nr3 t_lds", "blocks 32 + 1: a one-column tail block behind a block update"),
    ((3, 64, 40, 24), "bb_chain2_kernel ob32 nr3 t_lds", "blocks 32 + 8; ms - s = n exactly (edge of the valid layout)"),
    ((2, 48, 47, 30), "bb_chain2_kernel ob32 nr3 t_lds", "nearly square first panel: last block with mr = 16, ob = 15"),
    ((3, 120, 40, 24), "bb_chain2_kernel ob32 nr4 t_lds", "NR 4 (192 < m <= 256)"),
    ((2, 130, 129, 65), "bb_chain2_kernel ob32 nr4 t_lds", "NR 3 then NR 4 in one chain; four blocks + one column"),
    ((3, 300, 144, 130), "bb_chain2_kernel ob32 nr8 t_lds", "OB 32 / NR 8, last even m that fits (470)"),
    ((3, 300, 144, 129), "bb_chain2_kernel ob32 nr8 t_lds", "OB 32, the largest m that fits (471, odd)"),
    ((3, 300, 144, 128), "bb_chain2_kernel ob16 nr16 t_lds", "first m on OB 16 (472)"),
    ((3, 400, 50, 30), "bb_chain2_kernel ob16 nr16 t_lds", "OB 16 / NR 16, n = 3 groups + 2 columns"),
    ((2, 210, 200, 100), "bb_chain2_kernel ob32 nr8 t_lds", "largest n with T packed in LDS"),
    ((2, 210, 201, 100), "bb_chain2_kernel ob32 nr8 t_global", "first n on the in-place T recurrence, no switch set"),
    ((2, 260, 256, 128), "bb_chain2_kernel ob32 nr8 t_global", "n = BC_CW, OB 32"),
    ((2, 300, 256, 128), "bb_chain2_kernel ob16 nr16 t_global", "n = BC_CW, OB 16"),
    ((2, 300, 257, 136), "bb_chain_kernel", "first n on bb_chain_kernel, no switch"),
    ((2, 300, 272, 136), "bb_chain_kernel", "bb_chain_kernel, n a multiple of 16"),
    ((2, 532, 48, 40), "bb_chain2_kernel ob16 nr16 t_lds", "tallest panel of chain2 (1024)"),
    ((2, 532, 48, 39), "bb_chain_kernel", "first m on bb_chain_kernel (1025)"),
]
# Every name qrk_bb_kernel_name gives with no environment switch set, over ALL panels of the cases.  T in place needs more than
# 200 columns, so a first panel of more than 200 rows: "ob32 nr3 t_global" cannot occur without QRK_BB_T_GLOBAL, and
# "ob32 nr4 t_global" only as the first panel (210 rows) of the n = 201 case.
CLASSES = sorted(["bb_chain_kernel"] + ["bb_chain2_kernel %s t_%s" % (q, t) for t in ("lds", "global")
                                        for q in ("ob32 nr3", "ob32 nr4", "ob32 nr8", "ob16 nr16") if (q, t) != ("ob32 nr3", "global")])
# the reference's layout cannot express these (ms - s < n with more than two panels): refused by name
REJECTED = [(3, 40, 32, 16), (3, 48, 47, 30), (3, 150, 100, 52)]
# the cases of the guard-band net (tests/test_guarded_banded_gpu.py)
GUARDED = [(3, 96, 17, 9), (3, 60, 33, 20), (2, 130, 129, 65), (2, 210, 201, 100), (2, 300, 257, 136)]


def case_id(case):
    return "x".join(str(v) for v in (case[0] if isinstance(case[0], tuple) else case))


@functools.lru_cache(maxsize=None)
def matrix_and_oracle(key, seed=3):
    """(J, oracle factorisation): computed once per case and shared by the tests that need it; neither is modified."""
    from oracle import oracle as orc
    J = dense_strips(*key, seed=seed)
    return J, orc.bb_factorize(J, 2)
