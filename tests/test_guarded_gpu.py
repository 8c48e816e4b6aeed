"""GPU: every kernel route of the block-diagonal, Levenberg-Marquardt and dense calls through the raw C ABI (qrkit_amd._capi on plans
from qrk_bd_plan_create / qrk_dense_plan_create), with EVERY caller-owned array guard-banded at the extent include/qrkit_amd.h
documents (tests/guarded.py): a store past nnz_r, a read of an element past an input's extent that reaches an output, a write into an
input, an output element left unwritten -- none of which a parity test on tensors from a caching allocator can see.

Each case runs at shift 0 (16-byte aligned arrays) and shift 1 (all floating-point arrays 8 bytes off), on batches that leave a
ragged tail in whatever unit a kernel groups tiles by: B = 5 (one partial workgroup), B = 257 (full groups plus an odd tile), B = 3 for
tiles above 64, and mixed batches.  Batches of 5 tiles and the mixed ones carry trailing identity rows (mat_rows > sum of rows).

The values are judged by the project's own judges at the project's own bounds: the oracle (helpers.oracle_factorize: permutation,
info, rank exact; Q, R, tau, Q^T b, x within RTOL = 1e-12 per tile), lm_reference.py / lm_panel_reference.py at 1e-11 per tile, the
dense calls as tests/test_dense_gpu.py judges them.  So that x = P R^-1 Q^T b meets RTOL as well, the tiles are seeded_tiles(-1, 1)
with 2 + c / 2 added on each tile's diagonal: the random part of a c-column tile has a spectral norm of about 2 sqrt(c / 3), well
below the shift, so the condition number stays in the single digits and the oracle's and the device's rounding of x (a few c eps
times that) stays far below 1e-12.  The LM inputs are the
oracle's R and permutation of those tiles with par = 1: the stack [R; sqrt(par) D] is as well conditioned, which is what lets every
sum be held to 1e-11 as well (the bound tests/test_lm_solve_gpu.py states for x).

test_every_route_has_a_guarded_case pins the set of kernel names the five name functions return over all cases to an explicit list:
a route added later without a guarded case fails it.  The strings that start with "unsupported" name no kernel and have no case.
Where the header promises bit-identical repeat calls, whether shift 0 and shift 1 give the same bits is recorded and printed by the
last test (not asserted: qrk_bd_factorize_rhs on 32 x 32 takes its fallback for arrays that are not 16-byte aligned).
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import lm_panel_reference as panel_judge
import lm_reference as lm_judge
from guarded import Net
from helpers import RTOL, oracle_factorize, per_tile_rel, rel_fro, seeded_tiles, tile_sizes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FULL_Q, BLOCK_DIAGONAL_Q = 0, 1
LM_TOL = 1e-11
SHIFTS = (0, 1)
BITS = {}                # route -> shift 0 and shift 1 gave the same bits in every case of the route
ENV_KEYS = ("QRK_EXACT", "QRK_SMALL", "QRK_QUAD", "QRK_QUAD_MIN_ROWS", "QRK_THIN", "QRK_PAIR_V2", "QRK_K1_FORM", "QRK_PAIR_WGS",
            "QRK_Q32_WGS", "QRK_P4_OWN", "QRK_W64", "QRK_COL_ONCHIP", "QRK_DENSE_PATH", "QRK_DENSE_TWO_STAGE", "QRK_DENSE_PERSISTENT",
            "QRK_DENSE_PERS")


def ids_of(table):
    return [case[0].replace(",", "").replace(" ", "_") for case in table]


def note(route, same):
    BITS[route] = BITS.get(route, True) and bool(same)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.int64 if np.asarray(x).dtype == np.float64 else np.int32),
                              np.asarray(y).view(np.int64 if np.asarray(y).dtype == np.float64 else np.int32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


def context_for(qa, monkeypatch, env):
    """A handle created under exactly these switches (they are read when the handle or the plan is created)"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return qa.Context(0)


def sync():
    """A GPU fault ends the session here: nothing more is started on a device that has faulted"""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, no further case is run: {e}", returncode=3)


# ---- batches and their oracle -----------------------------------------------------------------------------------------------------------

def layout(kind, r, c, B):
    if kind == "u":
        return np.full(B, r, np.int32), np.full(B, c, np.int32)
    if kind == "m32":                                                # every width 1 .. 32 and a ragged rest
        rng = np.random.default_rng(7)
        cols = np.concatenate([np.arange(1, 33), rng.integers(1, 33, B - 32)]).astype(np.int32)
        rng.shuffle(cols)
        return (cols + rng.integers(0, 6, B)).clip(max=32).astype(np.int32), cols
    assert kind == "m256"                                            # above 32: one wave per tile, LDS-resident, on chip (both classes)
    return np.array([40, 96, 200, 64, 80], np.int32), np.array([40, 80, 130, 48, 48], np.int32)


def batch_sizes(kind, r):
    return {"m32": (37,), "m256": (5,)}.get(kind, (3,) if r > 64 else (5, 257))


def tiles_for(rows, cols, seed):
    t = seeded_tiles(seed, -1.0, 1.0, int((rows.astype(np.int64) * cols).sum()))
    off = 0
    for r, c in zip(rows.tolist(), cols.tolist()):
        k = np.arange(min(r, c))
        t[off + k * r + k] += 2.0 + c / 2.0
        off += r * c
    return t


class Ref:
    """Oracle factorisation of one batch, its Q as a sparse matrix, and where every tile's entries of Q^T b sit"""

    def __init__(self, kind, r, c, B, extra, q_format, solver):
        self.rows, self.cols = layout(kind, r, c, B)
        self.uniform = kind == "u"
        self.tiles = tiles_for(self.rows, self.cols, 3 + r + c + B)
        self.sum_rows, self.mat_cols = int(self.rows.sum()), int(self.cols.sum())
        self.mat_rows, self.q_format, self.solver = self.sum_rows + extra, q_format, solver
        self.prob, self.ref = oracle_factorize(self.rows, self.cols, self.tiles, mat_rows=self.mat_rows, q_format=q_format, block_solver=solver)
        self.sq, self.sr, self.sc = tile_sizes(self.rows, self.cols)
        self.nnz_q, self.nnz_r = int(self.sq.sum()) + extra, int(self.sr.sum())
        self.q_vals, self.r_vals = self.ref.Q_vals[:self.nnz_q], self.ref.R_vals[:self.nnz_r]
        self.perm, self.hc = self.ref.perm[:self.mat_cols], self.ref.hcoeffs[:self.mat_cols]
        qp, qi, _, _ = self.prob.pattern()
        self.Q = sp.csr_matrix((self.q_vals, qi, qp), shape=(self.mat_rows, self.mat_rows))
        idx, br, bc = [], 0, 0
        for rr, cc in zip(self.rows.tolist(), self.cols.tolist()):   # FullQ [U.. | N..], BlockDiagonalQ by rows
            k = np.arange(rr)
            idx.append(np.where(k < cc, bc + k, self.mat_cols + (br - bc) + (k - cc)) if q_format == FULL_Q else br + k)
            br += rr; bc += cc
        self.qt_idx = np.concatenate(idx)

    def rng(self, salt):
        return np.random.default_rng(1000 * salt + self.mat_rows)


@functools.lru_cache(maxsize=None)
def ref_for(kind, r, c, B, extra, q_format, solver):
    return Ref(kind, r, c, B, extra, q_format, solver)


def extra_rows(kind, B):
    return 5 if (B <= 5 or kind != "u") else 0


@contextlib.contextmanager
def bd_plan(ctx, ref):
    from qrkit_amd import _capi as capi
    lay = capi.BDLayout()
    lay.num_blocks = len(ref.rows)
    if ref.uniform:
        lay.block_rows, lay.block_cols, lay.rows, lay.cols = int(ref.rows[0]), int(ref.cols[0]), None, None
    else:
        lay.rows, lay.cols = ref.rows.ctypes.data_as(C.POINTER(C.c_int32)), ref.cols.ctypes.data_as(C.POINTER(C.c_int32))
    lay.mat_rows, lay.mat_cols = ref.mat_rows, ref.mat_cols
    plan = C.c_void_p()
    capi.check(capi.lib().qrk_bd_plan_create(ctx.handle, C.byref(lay), ref.q_format, ref.solver, C.byref(plan)), ctx.handle)
    try:
        tl, nq, nr = C.c_int64(), C.c_int64(), C.c_int64()
        capi.check(capi.lib().qrk_bd_plan_sizes(plan, C.byref(tl), C.byref(nq), C.byref(nr)), ctx.handle)
        assert (tl.value, nq.value, nr.value) == (ref.tiles.size, ref.nnz_q, ref.nnz_r)      # the documented extents are the plan's
        ctx.use_current_stream()
        yield plan
    finally:
        sync()
        capi.lib().qrk_bd_plan_destroy(plan)


def lib():
    from qrkit_amd import _capi as capi
    L = capi.lib()
    L.qrk_bd_kernel_name.restype = C.c_char_p
    L.qrk_bd_kernel_name.argtypes = [C.c_void_p, C.c_int]
    return L


def ok(ctx, status):
    from qrkit_amd import _capi as capi
    if status == capi.STATUS_HIP_ERROR:
        pytest.exit(f"HIP error, no further case is run: {capi.lib().qrk_last_error(ctx.handle)}", returncode=3)
    capi.check(status, ctx.handle)


def ptr(a):
    return None if a is None else a.ptr


# ---- judges ---------------------------------------------------------------------------------------------------------------------------

def judge_info(ctx, plan, ref):
    info, rank = C.c_int(), C.c_int64()
    ok(ctx, lib().qrk_bd_info(plan, C.byref(info), C.byref(rank)))
    assert (info.value, rank.value) == (ref.ref.info, ref.ref.rank)


def judge_factors(ref, perm, r, hc=None, q=None, what=""):
    np.testing.assert_array_equal(perm.get(), ref.perm)
    e = {"R": per_tile_rel(r.get(), ref.r_vals, ref.sr)}
    if hc is not None:
        e["tau"] = per_tile_rel(hc.get(), ref.hc, ref.sc)
    if q is not None:
        nt = int(ref.sq.sum())
        e["Q"] = per_tile_rel(q.get()[:nt], ref.q_vals[:nt], ref.sq)
        np.testing.assert_array_equal(q.get()[nt:], ref.q_vals[nt:])            # the trailing identity rows
    print(f"{what}: " + ", ".join(f"{k} per tile {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= RTOL, e


def judge_qt(ref, got, want, src, what):
    """Q^T of a panel: per tile in the plan's Q-format order, the trailing identity rows copied"""
    worst = max((per_tile_rel(got[ref.qt_idx, j], want[ref.qt_idx, j], ref.rows) for j in range(got.shape[1])), default=0.0)
    print(f"{what}: Q^T per tile {worst:.2e} over {got.shape[1]} columns")
    assert worst <= RTOL
    np.testing.assert_array_equal(got[ref.sum_rows:], src[ref.sum_rows:])


def judge_cols(ref, got, want, sizes, what):
    worst = max((per_tile_rel(got[:int(sizes.sum()), j], want[:int(sizes.sum()), j], sizes) for j in range(got.shape[1])), default=0.0)
    print(f"{what}: per tile {worst:.2e} over {got.shape[1]} columns")
    assert worst <= RTOL


# ---- qrk_bd_factorize: one case per kernel qrk_bd_kernel_name can name -------------------------------------------------------------------

FACTORIZE = [
    # label, kind, rows, cols, switches, the kernel
    ("thin 1x1", "u", 1, 1, {}, "qrk::thin::bdqr_thin_kernel"),
    ("thin 7x2", "u", 7, 2, {}, "qrk::thin::bdqr_thin_kernel"),
    ("thin 16x2", "u", 16, 2, {}, "qrk::thin::bdqr_thin_kernel"),
    ("quad 16x16", "u", 16, 16, {}, "qrk::bdqr_quad_kernel"),
    ("quad 8x6", "u", 8, 6, {}, "qrk::bdqr_quad_kernel"),
    ("quad 12x5", "u", 12, 5, {}, "qrk::bdqr_quad_kernel"),
    ("small 4x3", "u", 4, 3, {}, "qrk::bdqr_small_kernel"),
    ("small 8x6", "u", 8, 6, {"QRK_QUAD": "0"}, "qrk::bdqr_small_kernel"),
    ("pair4 32x32", "u", 32, 32, {}, "qrk::bdqr_pair4_kernel"),
    ("pair4 32x32, several rounds", "u", 32, 32, {"QRK_PAIR_WGS": "16"}, "qrk::bdqr_pair4_kernel"),
    ("quad32 32x32", "u", 32, 32, {"QRK_K1_FORM": "quad32"}, "qrk::bdqr_quad32_kernel"),
    ("quad32 32x32, several rounds", "u", 32, 32, {"QRK_K1_FORM": "quad32", "QRK_Q32_WGS": "16"}, "qrk::bdqr_quad32_kernel"),
    ("pair32 32x32", "u", 32, 32, {"QRK_PAIR_V2": "0"}, "qrk::bdqr_pair32_kernel"),
    ("ragged 24x20", "u", 24, 20, {}, "qrk::bdqr_pair_kernel"),
    ("mixed 1..32", "m32", 0, 0, {}, "qrk::bdqr_pair_kernel"),
    ("w64 33x33", "u", 33, 33, {}, "qrk::bdqr_w64_kernel"),
    ("w64 48x48", "u", 48, 48, {}, "qrk::bdqr_w64_kernel"),
    ("w64 64x64", "u", 64, 64, {}, "qrk::bdqr_w64_kernel"),
    ("col 80x48", "u", 80, 48, {}, "qrk::bdqr_col_kernel"),
    ("mixed above 32", "m256", 0, 0, {}, "qrk::bdqr_col_kernel"),
    ("on-chip col 200x200", "u", 200, 200, {}, "qrk::bdqr_col_kernel"),
    ("wg 257x257", "u", 257, 257, {}, "qrk::bdqr_wg_kernel"),
    ("exact 7x2", "u", 7, 2, {"QRK_EXACT": "1"}, "qrk::bdqr_exact_kernel"),
    ("exact 32x32", "u", 32, 32, {"QRK_EXACT": "1"}, "qrk::bdqr_exact_kernel"),
]


def formats_for(B, solver):
    """both Q formats on the small batch; on the large one the format follows the solver (every pair of the two is met)"""
    return (FULL_Q, BLOCK_DIAGONAL_Q) if B <= 5 else (solver,)


def run_factorize(ctx, plan, ref, shift, with_hc, what):
    net = Net(ctx.device, shift)
    t = net.inp("tiles", ref.tiles)
    q, r = net.out("q_vals", ref.nnz_q), net.out("r_vals", ref.nnz_r)
    p = net.out("perm", ref.mat_cols, dtype=_i32())
    hc = net.out("hcoeffs", ref.mat_cols) if with_hc else None
    from qrkit_amd import _capi as capi
    ok(ctx, lib().qrk_bd_factorize(plan, t.ptr, q.ptr, r.ptr, p.ptr, ptr(hc), capi.MEM_DEVICE))
    sync()
    net.check()
    judge_info(ctx, plan, ref)
    judge_factors(ref, p, r, hc, q, f"{what} shift {shift} tau {with_hc}")
    return [q.get(), r.get(), p.get()] + ([hc.get()] if with_hc else [])


def _i32():
    import torch
    return torch.int32


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("case", FACTORIZE, ids=ids_of(FACTORIZE))
def test_factorize(qa, monkeypatch, case, solver):
    label, kind, r, c, env, kernel = case
    ctx = context_for(qa, monkeypatch, env)
    for B in batch_sizes(kind, r):
        for qf in formats_for(B, solver):
            ref = ref_for(kind, r, c, B, extra_rows(kind, B), qf, solver)
            with bd_plan(ctx, ref) as plan:
                name = lib().qrk_bd_kernel_name(plan, 0).decode()
                assert kernel in name, name
                for with_hc in (True, False):
                    runs = [run_factorize(ctx, plan, ref, s, with_hc, f"{label} B {B} format {qf}") for s in SHIFTS]
                    note(f"qrk_bd_factorize {name}", same_bits(*runs))


# ---- qrk_bd_tiles_from_sparse -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,r,c,B", [("u", 7, 2, 5), ("u", 8, 6, 257), ("m32", 0, 0, 37)])
def test_tiles_from_sparse(qa, monkeypatch, kind, r, c, B):
    from qrkit_amd import _capi as capi
    ctx = context_for(qa, monkeypatch, {})
    ref = ref_for(kind, r, c, B, extra_rows(kind, B), FULL_Q, 0)
    blocks, off = [], 0
    for rr, cc in zip(ref.rows.tolist(), ref.cols.tolist()):
        blocks.append(ref.tiles[off:off + rr * cc].reshape(cc, rr).T)
        off += rr * cc
    M = sp.lil_matrix((ref.mat_rows, ref.mat_cols))
    M[:ref.sum_rows] = sp.block_diag(blocks)
    M[ref.mat_rows - 1, 0] = 9.0                                     # entries outside the blocks are ignored
    if ref.mat_cols > int(ref.cols[0]):
        M[0, ref.mat_cols - 1] = 9.0
    with bd_plan(ctx, ref) as plan:
        for row_major in (0, 1):
            m = sp.csr_matrix(M) if row_major else sp.csc_matrix(M)
            m.sort_indices()
            runs = []
            for shift in SHIFTS:
                net = Net(ctx.device, shift)
                outer, inner = net.inp("outer_ptr", m.indptr, dtype=_i32()), net.inp("inner_idx", m.indices, dtype=_i32())
                vals, tiles = net.inp("vals", m.data), net.out("tiles", ref.tiles.size)
                ok(ctx, lib().qrk_bd_tiles_from_sparse(plan, row_major, outer.ptr, inner.ptr, vals.ptr, m.nnz, tiles.ptr, capi.MEM_DEVICE))
                sync()
                net.check()
                np.testing.assert_array_equal(tiles.get(), ref.tiles)
                runs.append([tiles.get()])
            note("qrk_bd_tiles_from_sparse", same_bits(*runs))


# ---- qrk_bd_apply_qt / apply_q / solve / solve_r on explicit factors --------------------------------------------------------------------

APPLY = [("u", 7, 2, 5), ("u", 8, 6, 257), ("u", 32, 32, 5), ("m32", 0, 0, 37), ("u", 33, 33, 3), ("m256", 0, 0, 5), ("u", 7, 2, 257)]


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("kind,r,c,B", APPLY)
def test_apply_and_solve(qa, monkeypatch, kind, r, c, B, nrhs):
    """The factors are the oracle's own, so only the product's rounding enters.  mat_rows is odd: the second and third right-hand
    side are 8-byte aligned only (and the first, at shift 1)."""
    from qrkit_amd import _capi as capi
    ctx = context_for(qa, monkeypatch, {})
    rows, _ = layout(kind, r, c, B)
    extra = 5 if int(rows.sum()) % 2 == 0 else 6
    for qf in (FULL_Q, BLOCK_DIAGONAL_Q):
        ref = ref_for(kind, r, c, B, extra, qf, 0)
        assert ref.mat_rows % 2 == 1
        rng = ref.rng(nrhs)
        b = rng.uniform(-1.0, 1.0, (ref.mat_rows, nrhs))
        yin = rng.uniform(-1.0, 1.0, (ref.mat_cols, nrhs))
        Rs = lm_judge.unpack_r(ref.r_vals, ref.cols)
        want_z, base = np.zeros_like(yin), 0
        for R in (Rs if qf == FULL_Q else ()):                       # (R is triangular in the FullQ format only)
            cc = R.shape[0]
            want_z[base:base + cc] = sl.solve_triangular(R, yin[base:base + cc], lower=False)
            base += cc
        with bd_plan(ctx, ref) as plan:
            runs = {k: [] for k in ("apply_qt", "apply_q", "solve", "solve_r")}
            for shift in SHIFTS:
                what = f"{kind} {r}x{c} B {B} format {qf} nrhs {nrhs} shift {shift}"
                net = Net(ctx.device, shift)
                q, rv, pm = net.inp("q_vals", ref.q_vals), net.inp("r_vals", ref.r_vals), net.inp("perm", ref.perm, dtype=_i32())
                bb, yy = net.panel_in("b", b, ref.mat_rows), net.panel_in("y", yin, ref.mat_cols)
                qtb, qb = net.panel_out("apply_qt.y", ref.mat_rows, nrhs, ref.mat_rows), net.panel_out("apply_q.y", ref.mat_rows, nrhs, ref.mat_rows)
                z = net.panel_out("solve_r.z", ref.mat_cols, nrhs, ref.mat_cols)
                ok(ctx, lib().qrk_bd_apply_qt(plan, q.ptr, bb.ptr, nrhs, qtb.ptr, capi.MEM_DEVICE))
                ok(ctx, lib().qrk_bd_apply_q(plan, q.ptr, bb.ptr, nrhs, qb.ptr, capi.MEM_DEVICE))
                x = None
                if qf == FULL_Q:
                    x = net.panel_out("solve.x", ref.mat_cols, nrhs, ref.mat_cols)
                    ok(ctx, lib().qrk_bd_solve(plan, q.ptr, rv.ptr, pm.ptr, bb.ptr, nrhs, x.ptr, capi.MEM_DEVICE))
                    ok(ctx, lib().qrk_bd_solve_r(plan, rv.ptr, yy.ptr, nrhs, z.ptr, capi.MEM_DEVICE))
                else:
                    z.untouched[:] = True                            # (R is triangular in the FullQ format only: not called)
                sync()
                net.check()
                judge_qt(ref, qtb.get(), ref.Q.T @ b, b, what + " apply_qt")
                want = ref.Q @ b
                judge_cols(ref, qb.get(), want, ref.rows.astype(np.int64), what + " apply_q")
                np.testing.assert_array_equal(qb.get()[ref.sum_rows:], want[ref.sum_rows:])
                runs["apply_qt"].append([qtb.get()]); runs["apply_q"].append([qb.get()])
                if x is not None:
                    judge_cols(ref, x.get(), ref.prob.solve(ref.ref, b).reshape(ref.mat_cols, nrhs), ref.sc, what + " solve")
                    judge_cols(ref, z.get(), want_z, ref.sc, what + " solve_r")
                    runs["solve"].append([x.get()]); runs["solve_r"].append([z.get()])
            for k, v in runs.items():
                if v:
                    note(f"qrk_bd_{k}", same_bits(*v))


# ---- qrk_bd_factorize_rhs ---------------------------------------------------------------------------------------------------------------

RHS = [
    # label, kind, rows, cols, switches, right-hand sides, the kernel by nrhs
    ("thin 7x2", "u", 7, 2, {}, (1, 4, 5), lambda n: "bdqr_thin_rhs_kernel" if n <= 4 else "fallback"),
    ("pair4 32x32", "u", 32, 32, {}, (1, 32, 33), lambda n: "bdqr_pair4_rhs_kernel" if n <= 32 else "fallback"),
    ("pair4 32x32, several rounds", "u", 32, 32, {"QRK_PAIR_WGS": "16"}, (1, 32), lambda n: "bdqr_pair4_rhs_kernel"),
    ("fallback 8x6", "u", 8, 6, {}, (1, 5), lambda n: "fallback"),
    ("fallback mixed 1..32", "m32", 0, 0, {}, (3,), lambda n: "fallback"),
]


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("case", RHS, ids=ids_of(RHS))
def test_factorize_rhs(qa, monkeypatch, case, solver):
    from qrkit_amd import _capi as capi
    label, kind, r, c, env, widths, kernel = case
    ctx = context_for(qa, monkeypatch, env)
    for B in batch_sizes(kind, r):
        # FullQ: Q^T b only, x only, both; BlockDiagonalQ (the other row order of Q^T b): Q^T b only, without tau
        for qf, modes in ((FULL_Q, ((True, False), (False, True), (True, True))), (BLOCK_DIAGONAL_Q, ((True, False),))):
            ref = ref_for(kind, r, c, B, extra_rows(kind, B), qf, solver)
            with bd_plan(ctx, ref) as plan:
                for nrhs in widths:
                    name = lib().qrk_bd_rhs_kernel_name(plan, nrhs).decode()
                    assert kernel(nrhs) in name, name
                    b = ref.rng(nrhs).uniform(-1.0, 1.0, (ref.mat_rows, nrhs))
                    want_x = ref.prob.solve(ref.ref, b).reshape(ref.mat_cols, nrhs) if qf == FULL_Q else None
                    for want_qtb, want_sol in modes:
                        runs = []
                        for shift in SHIFTS:
                            what = f"{label} B {B} format {qf} nrhs {nrhs} qtb {want_qtb} x {want_sol} shift {shift}"
                            net = Net(ctx.device, shift)
                            t, bb = net.inp("tiles", ref.tiles), net.panel_in("b", b, ref.mat_rows)
                            rv, pm = net.out("r_vals", ref.nnz_r), net.out("perm", ref.mat_cols, dtype=_i32())
                            hc = net.out("hcoeffs", ref.mat_cols) if qf == FULL_Q else None
                            y = net.panel_out("qtb", ref.mat_rows, nrhs, ref.mat_rows) if want_qtb else None
                            x = net.panel_out("x", ref.mat_cols, nrhs, ref.mat_cols) if want_sol else None
                            ok(ctx, lib().qrk_bd_factorize_rhs(plan, t.ptr, bb.ptr, nrhs, rv.ptr, pm.ptr, ptr(hc), ptr(y), ptr(x), capi.MEM_DEVICE))
                            sync()
                            net.check()
                            judge_info(ctx, plan, ref)
                            judge_factors(ref, pm, rv, hc, None, what)
                            if y is not None:
                                judge_qt(ref, y.get(), ref.Q.T @ b, b, what)
                            if x is not None:
                                judge_cols(ref, x.get(), want_x, ref.sc, what + " x")
                            runs.append([rv.get(), pm.get()] + [a.get() for a in (hc, y, x) if a is not None])
                        note(f"qrk_bd_factorize_rhs {name}", same_bits(*runs))


# ---- qrk_bd_factorize_apply_qt ----------------------------------------------------------------------------------------------------------

PANEL = [
    ("thin 2x2", "u", 2, 2, "bdqr_thin_panel_kernel<{piv}, 2, 4>"),
    ("thin 3x1", "u", 3, 1, "bdqr_thin_panel_kernel<{piv}, 4, 2>"),
    ("thin 7x2", "u", 7, 2, "bdqr_thin_panel_kernel<{piv}, 8, 2>"),
    ("thin 16x2", "u", 16, 2, "bdqr_thin_panel_kernel<{piv}, 16, 1>"),
    ("fallback 8x6", "u", 8, 6, "fallback"),
]
PANEL_WIDTHS = (0, 1, 6, 33)


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("case", PANEL, ids=ids_of(PANEL))
def test_factorize_apply_qt(qa, monkeypatch, case, solver):
    from qrkit_amd import _capi as capi
    label, kind, r, c, kernel = case
    ctx = context_for(qa, monkeypatch, {})
    for B in batch_sizes(kind, r):
        qf = solver if B > 5 else 1 - solver
        ref = ref_for(kind, r, c, B, extra_rows(kind, B), qf, solver)
        with bd_plan(ctx, ref) as plan:
            for ncols in PANEL_WIDTHS:
                name = lib().qrk_bd_panel_kernel_name(plan, ncols).decode()
                assert kernel.format(piv="true" if solver == 0 else "false") in name, name
                panel = ref.rng(ncols).uniform(-1.0, 1.0, (ref.mat_rows, ncols))
                for ldc, ldq in ((ref.mat_rows, ref.mat_rows), ((ref.mat_rows + 3) | 1, (ref.mat_rows + 5) | 1)):
                    runs = []
                    for shift in SHIFTS:
                        what = f"{label} B {B} format {qf} ncols {ncols} ldc {ldc} ldq {ldq} shift {shift}"
                        net = Net(ctx.device, shift)
                        t, cc = net.inp("tiles", ref.tiles), net.panel_in("c", panel, ldc)
                        rv, pm = net.out("r_vals", ref.nnz_r), net.out("perm", ref.mat_cols, dtype=_i32())
                        hc = net.out("hcoeffs", ref.mat_cols) if ncols != 1 else None
                        y = net.panel_out("qtc", ref.mat_rows, ncols, ldq)
                        ok(ctx, lib().qrk_bd_factorize_apply_qt(plan, t.ptr, cc.ptr, ldc, ncols, rv.ptr, pm.ptr, ptr(hc), y.ptr, ldq, capi.MEM_DEVICE))
                        sync()
                        net.check()
                        judge_info(ctx, plan, ref)
                        judge_factors(ref, pm, rv, hc, None, what)
                        judge_qt(ref, y.get(), ref.Q.T @ panel if ncols else panel, panel, what)
                        runs.append([rv.get(), pm.get(), y.get()])
                    note(f"qrk_bd_factorize_apply_qt {name}", same_bits(*runs))


# ---- the Levenberg-Marquardt calls -------------------------------------------------------------------------------------------------------

LM = [
    # label, kind, rows, cols, the kernel of qrk_bd_lm_solve, the kernel of qrk_bd_lm_panel
    ("7x2", "u", 7, 2, "qrk::lm::bd_lm_thin_kernel", "qrk::lm::bd_lm_panel_thin_kernel"),
    ("9x2", "u", 9, 2, "qrk::lm::bd_lm_thin_kernel", "qrk::lm::bd_lm_panel_thin_kernel"),
    ("8x6", "u", 8, 6, "qrk::lm::bd_lm_group_kernel<8>", "qrk::lm::bd_lm_panel_group_kernel<8>"),
    ("16x12", "u", 16, 12, "qrk::lm::bd_lm_group_kernel<16>", "qrk::lm::bd_lm_panel_group_kernel<16>"),
    ("24x20", "u", 24, 20, "qrk::lm::bd_lm_group_kernel<32>", "qrk::lm::bd_lm_panel_group_kernel<32>"),
    ("mixed 1..32", "m32", 0, 0, "qrk::lm::bd_lm_group_kernel<64>", "qrk::lm::bd_lm_panel_group_kernel<32>"),
    ("32x32", "u", 32, 32, "qrk::lm::bd_lm_group_kernel<64>", "qrk::lm::bd_lm_panel_group_kernel<32>"),
]
PAR = 1.0


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


class LmInputs:
    """The oracle's R and permutation of one batch, y, a seeded diag, and the judge's view of them"""

    def __init__(self, ref):
        rng = ref.rng(77)
        self.y = rng.uniform(-1.0, 1.0, ref.mat_cols)
        self.diag = rng.uniform(0.5, 2.0, ref.mat_cols)
        self.t = lm_judge.Tiles(ref.cols, ref.r_vals, ref.perm, self.y)

    def arrays(self, net, ref, with_diag):
        return (net.inp("r_vals", ref.r_vals), net.inp("perm", ref.perm, dtype=_i32()), net.inp("y", self.y),
                net.inp("diag", self.diag) if with_diag else None)


@functools.lru_cache(maxsize=None)
def lm_inputs(ref):
    return LmInputs(ref)


@pytest.mark.parametrize("case", LM, ids=ids_of(LM))
def test_lm_solve_gradient_and_norms(qa, monkeypatch, case):
    from qrkit_amd import _capi as capi
    label, kind, r, c, kernel, _ = case
    ctx = context_for(qa, monkeypatch, {})
    for B in batch_sizes(kind, r):
        ref = ref_for(kind, r, c, B, extra_rows(kind, B), FULL_Q, 0)
        inp = lm_inputs(ref)
        with bd_plan(ctx, ref) as plan:
            name = lib().qrk_bd_lm_kernel_name(plan).decode()
            assert name == kernel, name
            want_norms = lm_judge.col_norms(inp.t)
            for with_diag in (False, True):
                diag = inp.diag if with_diag else None
                want_x, want_s, _ = lm_judge.solve(inp.t, diag, PAR)
                want_g, want_gn = lm_judge.gradient(inp.t, diag)
                for with_sums in (True, False):            # (the gradient runs "g only" next to the sums, "gnorm2 only" without)
                    runs = []
                    for shift in SHIFTS:
                        what = f"{label} B {B} diag {with_diag} sums {with_sums} shift {shift}"
                        net = Net(ctx.device, shift)
                        rv, pm, y, dg = inp.arrays(net, ref, with_diag)
                        x = net.out("x", ref.mat_cols)
                        sums = net.out("sums", 3) if with_sums else None
                        g = net.out("g", ref.mat_cols) if with_sums else None
                        gn = None if with_sums else net.out("gnorm2", 1)
                        norms = net.out("norms", ref.mat_cols)
                        ok(ctx, lib().qrk_bd_lm_solve(plan, rv.ptr, pm.ptr, y.ptr, ptr(dg), PAR, x.ptr, ptr(sums), capi.MEM_DEVICE))
                        ok(ctx, lib().qrk_bd_lm_gradient(plan, rv.ptr, pm.ptr, y.ptr, ptr(dg), ptr(g), ptr(gn), capi.MEM_DEVICE))
                        ok(ctx, lib().qrk_bd_r_col_norms(plan, rv.ptr, pm.ptr, norms.ptr, capi.MEM_DEVICE))
                        sync()
                        net.check()
                        ex = lm_judge.per_tile_rel(x.get(), want_x, inp.t)
                        en = lm_judge.per_tile_rel(norms.get(), want_norms, inp.t)
                        print(f"{what}: x per tile {ex:.2e}, norms per tile {en:.2e}")
                        assert ex <= LM_TOL and en <= 1e-13
                        if with_sums:
                            s = sums.get()
                            e0, e1, eg = rel(s[0], want_s[0]), rel(s[1], want_s[1]), lm_judge.per_tile_rel(g.get(), want_g, inp.t)
                            print(f"{what}: sums[0] {e0:.2e}, sums[1] {e1:.2e}, g per tile {eg:.2e}")
                            assert e0 <= LM_TOL and e1 <= LM_TOL and s[2] == want_s[2] and eg <= 1e-13
                        else:
                            en2 = rel(gn.get()[0], want_gn)
                            print(f"{what}: gnorm2 {en2:.2e}")
                            assert en2 <= LM_TOL
                        runs.append([a.get() for a in (x, sums, g, gn, norms) if a is not None])
                    note(f"qrk_bd_lm_solve / lm_gradient / r_col_norms {name}", same_bits(*runs))


@pytest.mark.parametrize("case", LM, ids=ids_of(LM))
def test_lmpar_device(qa, monkeypatch, case):
    """delta, par, iters and trace are device arrays of 1, 1, 1 and 33 elements; the trace rows that did not run are written as zero"""
    label, kind, r, c, _, _ = case
    ctx = context_for(qa, monkeypatch, {})
    for B in batch_sizes(kind, r):
        ref = ref_for(kind, r, c, B, extra_rows(kind, B), FULL_Q, 0)
        inp = lm_inputs(ref)
        dx0 = float(np.linalg.norm(inp.diag * lm_judge.solve(inp.t, inp.diag, 0.0)[0]))
        with bd_plan(ctx, ref) as plan:
            for f in (2.0, 0.1):                                     # the Gauss-Newton step accepted at once; a search
                delta = f * dx0
                want_par, _, want_iters, _ = lm_judge.lmpar(inp.t, inp.diag, delta)
                runs = []
                for shift in SHIFTS:
                    what = f"{label} B {B} delta {f} |D x0| shift {shift}"
                    net = Net(ctx.device, shift)
                    rv, pm, y, dg = inp.arrays(net, ref, True)
                    dl, pv = net.inp("delta", [delta]), net.inp("par", [0.0], role="inout")
                    x, it, trace = net.out("x", ref.mat_cols), net.out("iters", 1, dtype=_i32()), net.out("trace", 33)
                    ok(ctx, lib().qrk_bd_lmpar_device(plan, rv.ptr, pm.ptr, y.ptr, dg.ptr, dl.ptr, pv.ptr, x.ptr, it.ptr, trace.ptr))
                    sync()
                    net.check()
                    par, iters, tr = float(pv.get()[0]), int(it.get()[0]), trace.get().reshape(11, 3)
                    print(f"{what}: par {par:.6e} (judge {want_par:.6e}), passes {iters} (judge {want_iters})")
                    assert iters == want_iters and np.all(tr[iters + 1:] == 0.0) and tr[0, 0] == 0.0
                    assert rel(par, want_par) <= 1e-9                # (tests/test_lmpar_gpu.py's bound on par against the judge)
                    assert par == tr[iters, 0] and (iters == 0) == (f == 2.0) and (par == 0.0) == (f == 2.0)
                    for p_k, s0, s1 in tr[:iters + 1]:               # every evaluation, at the par the device used
                        _, s, _ = lm_judge.solve(inp.t, inp.diag, p_k)
                        assert rel(s0, s[0]) <= LM_TOL and rel(s1, s[1]) <= LM_TOL, (p_k, s0, s1, s)
                    ex = lm_judge.per_tile_rel(x.get(), lm_judge.solve(inp.t, inp.diag, par)[0], inp.t)
                    print(f"{what}: x per tile {ex:.2e}")
                    assert ex <= LM_TOL
                    runs.append([pv.get(), x.get(), it.get(), trace.get()])
                note("qrk_bd_lmpar_device", same_bits(*runs))


@pytest.mark.parametrize("case", LM, ids=ids_of(LM))
def test_lm_panel(qa, monkeypatch, case):
    """Judged as tests/test_lm_panel_gpu.py judges: S^T S = R^T R + par Dt^2, top against numpy's Q^T [C; 0] with the rows
    sign-matched to the device's S, top^T top + fill^T fill = C^T C, each per tile"""
    label, kind, r, c, _, kernel = case
    ctx = context_for(qa, monkeypatch, {})
    for B in batch_sizes(kind, r):
        ref = ref_for(kind, r, c, B, extra_rows(kind, B), FULL_Q, 0)
        inp = lm_inputs(ref)
        n = ref.mat_cols
        Rs = panel_judge.unpack_tiles(ref.cols, ref.r_vals)
        base = np.concatenate([[0], np.cumsum(ref.cols)]).astype(np.int64)
        with bd_plan(ctx, ref) as plan:
            for ncols in (0, 1, 5):
                name = lib().qrk_bd_lm_panel_kernel_name(plan, ncols).decode()
                assert name == kernel, name
                for with_idx, pad in ((False, 0), (True, 3)):       # tight, in order; padded leading dimensions and gathered columns
                    nsrc = ncols + 2 if (with_idx and ncols) else ncols
                    colidx = (np.arange(nsrc)[::-1][:ncols] if with_idx else np.arange(ncols)).astype(np.int32)
                    Cmat = ref.rng(ncols + 10 * pad).standard_normal((n, nsrc))
                    diag = inp.diag if with_idx else None
                    D = np.ones(n) if diag is None else diag
                    ldc, ldt, ldf = n + pad, n + 2 * pad + (1 if pad else 0), n + pad
                    runs = []
                    for shift in SHIFTS:
                        what = f"{label} B {B} ncols {ncols} colidx {with_idx} pad {pad} shift {shift}"
                        net = Net(ctx.device, shift)
                        rv, pm = net.inp("r_vals", ref.r_vals), net.inp("perm", ref.perm, dtype=_i32())
                        dg = net.inp("diag", diag) if diag is not None else None
                        cc = net.panel_in("c", Cmat, ldc)
                        ci = net.inp("colidx", colidx, dtype=_i32()) if with_idx else None
                        s, top, fill = net.out("s_vals", ref.nnz_r), net.panel_out("top", n, ncols, ldt), net.panel_out("fill", n, ncols, ldf)
                        ok(ctx, lib().qrk_bd_lm_panel(plan, rv.ptr, pm.ptr, ptr(dg), PAR, cc.ptr, ldc, ncols, ptr(ci), s.ptr, top.ptr, ldt,
                                                      fill.ptr, ldf))
                        sync()
                        net.check()
                        Ss, tp, fl = panel_judge.unpack_tiles(ref.cols, s.get()), top.get(), fill.get()
                        worst = np.zeros(3)
                        for t, (R, S) in enumerate(zip(Rs, Ss)):
                            lo, hi = int(base[t]), int(base[t + 1])
                            dt = D[ref.perm[lo:hi]]
                            worst[0] = max(worst[0], rel_all(S.T @ S, R.T @ R + PAR * np.diag(dt * dt)))
                            if ncols:
                                Ct = Cmat[lo:hi][:, colidx]
                                Sn, topn, _ = panel_judge.tile_step(R, dt, PAR, Ct)
                                _, topn = panel_judge.match_signs(Sn, topn, np.diag(S))
                                worst[1] = max(worst[1], rel_all(tp[lo:hi], topn))
                                worst[2] = max(worst[2], rel_all(tp[lo:hi].T @ tp[lo:hi] + fl[lo:hi].T @ fl[lo:hi], Ct.T @ Ct))
                        print(f"{what}: S^T S {worst[0]:.2e}  top {worst[1]:.2e}  Gram {worst[2]:.2e}")
                        assert worst.max() <= LM_TOL
                        runs.append([s.get(), tp, fl])
                    note(f"qrk_bd_lm_panel {name}", same_bits(*runs))


def rel_all(a, b):
    den = np.linalg.norm(b)
    return np.linalg.norm(a - b) / den if den > 0 else np.linalg.norm(a - b)


@pytest.mark.parametrize("m2", [0, 1, 7])
def test_dense_lm_stack(qa, monkeypatch, m2):
    """rows 0 .. m2 = [triu(qr) | y2], rows m2 + m1 .. = sqrt(par) diag2[perm2] on the diagonal; the m1 rows between are the panel's
    fill and are not touched; ldg larger than the stack.  par = 4: sqrt(par) is exact and the whole result is known to the bit."""
    ctx = context_for(qa, monkeypatch, {})
    ctx.use_current_stream()
    m1, par = 9, 4.0
    rng = np.random.default_rng(m2)
    qr, y2, d2, p2 = rng.standard_normal((m2, m2)), rng.standard_normal(m2), rng.uniform(0.5, 2.0, m2), rng.permutation(m2).astype(np.int32)
    height, ldg, lda = 2 * m2 + m1, 2 * m2 + m1 + 3, m2 + 3
    middle = (np.arange(height) >= m2) & (np.arange(height) < m2 + m1)
    want = np.zeros((height, m2 + 1))
    want[:m2, :m2], want[:m2, m2] = np.triu(qr), y2
    want[m2 + m1 + np.arange(m2), np.arange(m2)] = 2.0 * d2[p2]
    for with_opt in (True, False):
        runs = []
        for shift in SHIFTS:
            net = Net(ctx.device, shift)
            a, yy = net.panel_in("qr", qr, lda), net.inp("y2", y2)
            dd, pp = (net.inp("diag2", d2), net.inp("perm2", p2, dtype=_i32())) if with_opt else (None, None)
            g = net.panel_out("g", height, m2 + 1 if m2 else 0, ldg, untouched_rows=middle)
            ok(ctx, lib().qrk_dense_lm_stack(ctx.handle, a.ptr, lda, m2, yy.ptr, ptr(dd), ptr(pp), par, m1, g.ptr, ldg))
            sync()
            net.check()
            if m2:
                w = want.copy()
                if not with_opt:
                    w[m2 + m1 + np.arange(m2), np.arange(m2)] = 2.0
                np.testing.assert_array_equal(g.get()[~middle], w[~middle])
            runs.append([np.nan_to_num(g.get())])
        note("qrk_dense_lm_stack", same_bits(*runs))


# ---- the dense right-block solver on a window of a taller array ---------------------------------------------------------------------------

DENSE = [
    # label, rows, cols, switches, two-stage format
    ("single workgroup 40x7", 40, 7, {}, False),
    ("column-parallel 300x40", 300, 40, {"QRK_DENSE_PATH": "cols"}, False),
    ("tall (row slabs) 640x48", 640, 48, {"QRK_DENSE_PATH": "slabs"}, False),
    ("persistent kernel 300x256", 300, 256, {"QRK_DENSE_PATH": "cols", "QRK_DENSE_PERS": "1"}, False),
    ("row slabs in one cooperative kernel 3000x150", 3000, 150, {"QRK_DENSE_PATH": "slabs", "QRK_DENSE_PERSISTENT": "1"}, False),
    ("two-stage 640x48", 640, 48, {"QRK_DENSE_TWO_STAGE": "1"}, True),
]


@pytest.mark.parametrize("case", DENSE, ids=ids_of(DENSE))
def test_dense_window(qa, monkeypatch, case):
    """qrk_dense_factorize, qrk_dense_apply_q in both directions and qrk_dense_solve_r with lda > rows and ldb > rows: the rows of the
    parent array above the window, below it and between its columns are guards.  Judged as tests/test_dense_gpu.py judges the route."""
    from qrkit_amd import _capi as capi
    label, rows, cols, env, two_stage = case
    ctx = context_for(qa, monkeypatch, env)
    ctx.use_current_stream()
    rng = np.random.default_rng(rows * 7 + cols)
    A = rng.uniform(-1.0, 1.0, (rows, cols)) * rng.uniform(0.5, 2.0, cols)[None, :]
    ref, hc_ref, perm_ref, _ = orc.colpiv_qr(A)
    Y = rng.uniform(-1.0, 1.0, (cols, 3))
    plan = C.c_void_p()
    ok(ctx, lib().qrk_dense_plan_create(ctx.handle, rows, cols, capi.COLPIV_HOUSEHOLDER, C.byref(plan)))
    try:
        assert bool(lib().qrk_dense_plan_two_stage(plan)) == two_stage
        lda, ldb = (rows + 5) | 1, (rows + 3) | 1
        runs = []
        for shift in SHIFTS:
            net = Net(ctx.device, shift)
            a = net.panel_in("a", A, lda, role="inout")
            hc, pm = net.out("hcoeffs", min(rows, cols)), net.out("perm", cols, dtype=_i32())
            ok(ctx, lib().qrk_dense_factorize(plan, a.ptr, lda, hc.ptr, pm.ptr, capi.MEM_DEVICE))
            sync()
            net.check()
            got, P = a.get(), pm.get()
            np.testing.assert_array_equal(P, perm_ref)
            Rg, Rr = np.triu(got[:cols]), np.triu(ref[:cols])
            if two_stage:      # R equal to Eigen's up to the sign of each row; what lies below are the reflectors of Q0
                sg = np.sign(np.diag(Rg)) * np.sign(np.diag(Rr))
                assert np.all(sg != 0)
                row_err = (np.linalg.norm(Rg * sg[:, None] - Rr, axis=1) / np.linalg.norm(Rr, axis=1)).max()
                print(f"{label} shift {shift}: R per row {row_err:.2e}")
                assert row_err <= 1e-11
            else:
                e = (rel_fro(Rg, Rr), rel_fro(hc.get(), hc_ref), rel_fro(np.tril(got, -1), np.tril(ref, -1)))
                print(f"{label} shift {shift}: R {e[0]:.2e}, tau {e[1]:.2e}, reflectors {e[2]:.2e}")
                assert e[0] <= 1e-11 and e[1] <= 1e-11 and e[2] <= 1e-10
            # Q^T (A P) = R and back, through the implicit Q, on a window of its own; the factors are inputs now
            fixed = Net(ctx.device, shift)
            hin = fixed.inp("hcoeffs", hc.get())
            b = fixed.panel_in("b", A[:, P], ldb, role="inout")
            ok(ctx, lib().qrk_dense_apply_q(plan, a.ptr, lda, hin.ptr, 1, b.ptr, ldb, cols, capi.MEM_DEVICE))
            sync()
            fixed.check()
            a.check()
            assert same_bits([a.get()], [got]), "the factors are an input here"
            Rfull = np.zeros((rows, cols)); Rfull[:cols] = Rg
            qtb = b.get()
            tol = 1e-12 * np.sqrt(cols) if two_stage else 1e-11      # (the bounds of the two tests of tests/test_dense_gpu.py)
            assert np.linalg.norm(qtb - Rfull) <= tol * np.linalg.norm(A)
            ok(ctx, lib().qrk_dense_apply_q(plan, a.ptr, lda, hin.ptr, 0, b.ptr, ldb, cols, capi.MEM_DEVICE))
            sync()
            fixed.check()
            a.check()
            assert same_bits([a.get()], [got]), "the factors are an input here"
            assert rel_fro(b.get(), A[:, P]) <= tol
            # back substitution on the upper triangle: only the first cols rows of b belong to the call
            z = fixed.panel_in("solve_r.b", Y, cols + 3, role="inout")
            ok(ctx, lib().qrk_dense_solve_r(plan, a.ptr, lda, z.ptr, cols + 3, 3, capi.MEM_DEVICE))
            sync()
            fixed.check()
            a.check()
            assert same_bits([a.get()], [got]), "the factors are an input here"
            want = sl.solve_triangular(Rg, Y, lower=False)
            assert rel_fro(z.get(), want) <= 1e-10 * max(1.0, np.linalg.cond(Rg) * 1e-6)
            runs.append([np.triu(got[:cols]), P, qtb, z.get()])
        note(f"qrk_dense_factorize / apply_q / solve_r, {label}", same_bits(*runs))
    finally:
        sync()
        lib().qrk_dense_plan_destroy(plan)


@pytest.mark.parametrize("rows,cols", [(40, 7), (300, 40), (641, 48)])
def test_dense_gemv_sub(qa, monkeypatch, rows, cols):
    """y -= S(:, colidx) z on a window with lds > rows, with and without colidx.  Bound: a sum of cols + 1 terms in any order is
    within (cols + 1) eps (|S| |z| + |y|) of the exact one, entry by entry."""
    ctx = context_for(qa, monkeypatch, {})
    ctx.use_current_stream()
    rng = np.random.default_rng(rows + cols)
    lds = (rows + 3) | 1
    y0, z = rng.uniform(-1.0, 1.0, rows), rng.uniform(-1.0, 1.0, cols)
    for with_idx in (False, True):
        nsrc = cols + 2 if with_idx else cols
        S = rng.uniform(-1.0, 1.0, (rows, nsrc))
        colidx = (rng.permutation(nsrc)[:cols] if with_idx else np.arange(cols)).astype(np.int32)
        if with_idx:
            colidx[0] = nsrc - 1                                     # the last column of S is read
        want = y0 - S[:, colidx] @ z
        bound = (cols + 1) * np.finfo(np.float64).eps * (np.abs(S[:, colidx]) @ np.abs(z) + np.abs(y0))
        runs = []
        for shift in SHIFTS:
            net = Net(ctx.device, shift)
            s, zz, y = net.panel_in("S", S, lds), net.inp("z", z), net.inp("y", y0, role="inout")
            ci = net.inp("colidx", colidx, dtype=_i32()) if with_idx else None
            ok(ctx, lib().qrk_dense_gemv_sub(ctx.handle, s.ptr, lds, rows, cols, ptr(ci), zz.ptr, y.ptr))
            sync()
            net.check()
            assert np.all(np.abs(y.get() - want) <= bound)
            runs.append([y.get()])
        note("qrk_dense_gemv_sub", same_bits(*runs))


# ---- coverage and the table ---------------------------------------------------------------------------------------------------------------

KERNELS = sorted(
    [f"qrk::bdqr_exact_kernel<{p}>" for p in ("true", "false")] + ["qrk::bdqr_wg_kernel", "qrk::bdqr_col_kernel"] +
    [f"qrk::bdqr_w64_kernel<{p}>" for p in ("true", "false")] +
    [f"qrk::thin::bdqr_thin_kernel<{p}, HC>" for p in ("true", "false")] +
    [f"qrk::bdqr_quad_kernel<WR, {p}, HC>" for p in ("true", "false")] +
    [f"qrk::bdqr_small_kernel<G, {p}>" for p in ("true", "false")] +
    [f"qrk::bdqr_quad32_kernel<{p}, false>" for p in ("true", "false")] +
    [f"qrk::bdqr_pair4_kernel<{p}, false, {own}>" for p in ("true", "false") for own in ("true", "false")] +
    [f"qrk::bdqr_pair32_kernel<{p}, false>" for p in ("true", "false")] +
    [f"qrk::bdqr_pair_kernel<false, {p}, true>" for p in ("true", "false")] +
    [f"qrk::thin_rhs::bdqr_thin_rhs_kernel<{p}, HC>" for p in ("true", "false")] +
    [f"qrk::bdqr_pair4_rhs_kernel<{p}, HC, {own}, NR>" for p in ("true", "false") for own in ("true", "false")] +
    ["fallback: qrk_bd_factorize + qrk_bd_apply_qt + qrk_bd_solve through the plan's Q scratch"] +
    [f"qrk::thin_panel::bdqr_thin_panel_kernel<{p}, {rc}>" for p in ("true", "false") for rc in ("2, 4", "4, 2", "8, 2", "16, 1")] +
    ["fallback: qrk_bd_factorize + qrk_bd_apply_qt through the plan's Q scratch"] +
    ["qrk::lm::bd_lm_thin_kernel"] + [f"qrk::lm::bd_lm_group_kernel<{g}>" for g in (8, 16, 32, 64)] +
    ["qrk::lm::bd_lm_panel_thin_kernel"] + [f"qrk::lm::bd_lm_panel_group_kernel<{g}>" for g in (8, 16, 32)])


def test_every_route_has_a_guarded_case(qa, monkeypatch):
    """The names the five name functions return over the cases above -- the same plans, the same switches, no launch -- are exactly
    KERNELS: a route added later without a guarded case fails here, and so does a case that no longer reaches its kernel."""
    hit = set()

    def plans(table, solvers, env_of, formats=(FULL_Q,)):
        for case in table:
            kind, r, c = case[1], case[2], case[3]
            ctx = context_for(qa, monkeypatch, env_of(case))
            for solver in solvers:
                for B in batch_sizes(kind, r):
                    for qf in formats:
                        ref = ref_for(kind, r, c, B, extra_rows(kind, B), qf, solver)
                        with bd_plan(ctx, ref) as plan:
                            yield case, plan

    for case, plan in plans(FACTORIZE, (0, 1), lambda k: k[4]):
        hit.add(lib().qrk_bd_kernel_name(plan, 0).decode())
    for case, plan in plans(RHS, (0, 1), lambda k: k[4]):
        hit.update(lib().qrk_bd_rhs_kernel_name(plan, n).decode() for n in case[5])
    for case, plan in plans(PANEL, (0, 1), lambda k: {}):
        hit.update(lib().qrk_bd_panel_kernel_name(plan, n).decode() for n in PANEL_WIDTHS)
    for case, plan in plans(LM, (0,), lambda k: {}):
        hit.add(lib().qrk_bd_lm_kernel_name(plan).decode())
        hit.update(lib().qrk_bd_lm_panel_kernel_name(plan, n).decode() for n in (0, 1, 5))
    assert sorted(hit) == KERNELS, (sorted(hit - set(KERNELS)), sorted(set(KERNELS) - hit))


def test_zz_print_the_shift_table():
    """Printed, not asserted: whether 8-byte and 16-byte aligned arrays gave the same bits, route by route"""
    print("\nshift 0 and shift 1 give the same bits:")
    for route in sorted(BITS):
        print(f"  {'yes' if BITS[route] else 'NO '}  {route}")
