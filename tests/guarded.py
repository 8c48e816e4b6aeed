"""Guard-banded arrays for calls that take raw pointers (the C ABI of include/qrkit_amd.h): a plain helper module, imported like
helpers.py.

Every kernel here reads and writes caller-owned arrays through raw pointers, and the header documents the extent of each to the
element.  A tensor from torch's caching allocator is rounded up and carved from a pool, so a store one vector past the end lands in
a neighbour and no parity test sees it.  guarded() puts the documented extent, and not one element more, between two guards:

    [ G guard elements | shift | n payload elements | G guard elements ]          G = 64

G = 64 elements is 512 bytes of doubles: wider than any vector access and wider than two 128-byte lines, so a kernel that rounds a
store up to whole lines cannot jump over it.  shift = 0 puts the payload on a 16-byte boundary (torch's allocations are at least
that aligned, which guarded() asserts), shift = 1 one element off it (8 bytes for doubles, 4 for int32).  n = 0 is allowed: the
pointer then points into the middle of the guard.  A strided panel (rows < ld) is one such array of (ncols - 1) ld + rows elements
whose rows between `rows` and `ld` of every column but the last are guards too ("gap").

role "out":   the whole tensor, payload included, holds one fixed quiet-NaN bit pattern (SENTINEL_F64; SENTINEL_I32 for int32),
              written through an integer view.  Every comparison is bitwise on that view: == on NaN is useless.
role "in":    the payload holds the data, the guards an ordinary NaN: an element read past the extent and used turns the result NaN.
              The guards of an int32 input hold 0: a wild index would turn a finding into a fault (see below).
role "inout": the payload holds the data, the guards the sentinel (arrays a call updates in place).

Net.check(), after the call and a synchronisation of the stream, asserts
  1. every guard element of every array is bitwise what it was (the message names the array, the side -- left, right or gap -- and
     the first offending offset, counted from the payload's first element);
  2. every "in" array is bitwise unchanged, payload included;
  3. no payload element of an "out" array still holds the sentinel, except those the case declared `untouched` (a documented
     exception: they must then STILL hold it), and no payload element of an "out" or "inout" array is NaN.
The values themselves are the caller's to judge.

What this net does not see: a read past an extent that does not influence any output, and a read past the extent of an index array
(its guards are valid indices).  Placing an array at the end of an allocation would catch those as a GPU fault, which on a shared
machine is not a test result: not done here, by design.

Works on CPU tensors as on device tensors (tests/test_guarded_cpu.py proves the net on numpy stand-ins).
"""
import numpy as np
import torch

G = 64
SENTINEL_F64 = 0x7FF8_5EA7_BAD0_5EA7          # a quiet NaN with a payload no arithmetic produces
SENTINEL_I32 = -0x5EA7_BAD                    # no index, no count
_INT_VIEW = {torch.float64: torch.int64, torch.int32: torch.int32}
ROLES = ("in", "out", "inout")


def _sentinel(dtype):
    return SENTINEL_F64 if dtype == torch.float64 else SENTINEL_I32


class Guarded:
    """One guarded array; see the module docstring.  `ptr` is what the call gets."""

    def __init__(self, n, dtype, role, shift, device, data=None, name="array", rows=None, ld=None, untouched=None):
        assert dtype in _INT_VIEW and role in ROLES and shift in (0, 1) and n >= 0
        self.n, self.dtype, self.role, self.shift, self.name = int(n), dtype, role, shift, name
        self.off = G + shift
        self.buf = torch.empty(G + shift + self.n + G, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0, "the allocator's alignment is what shift is counted from"
        self.bits = self.buf.view(_INT_VIEW[dtype])
        guard_bits = _sentinel(dtype) if role != "in" else (0 if dtype == torch.int32 else
                                                          int(np.array(np.nan).view(np.int64)))
        self.bits.fill_(guard_bits)
        # which of the n elements are payload (the others: gap rows of a strided panel)
        self.is_payload = torch.ones(self.n, dtype=torch.bool)
        self.rows, self.ld, self.ncols = rows, ld, None
        if rows is not None:
            assert ld >= rows and (self.n == 0 or (self.n - rows) % ld == 0)
            self.ncols = 0 if self.n == 0 else (self.n - rows) // ld + 1
            self.is_payload = (torch.arange(self.n) % ld) < rows
        if role != "out":
            assert data is not None, "in / inout arrays carry data"
            src = torch.as_tensor(np.ascontiguousarray(data)).to(dtype)
            if rows is not None:                                     # data: rows x ncols, column j at j * ld
                assert tuple(src.shape) == (rows, self.ncols), (tuple(src.shape), rows, self.ncols)
                if self.ncols:
                    self.columns().copy_(src.T.to(device))
            else:
                assert src.numel() == self.n, (src.numel(), self.n)
                self.payload().copy_(src.reshape(-1).to(device))
        self.untouched = torch.zeros(self.n, dtype=torch.bool)
        if untouched is not None:
            self.untouched = torch.as_tensor(np.broadcast_to(np.asarray(untouched, dtype=bool), (self.n,)).copy())
        self.before = self.bits.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def payload(self):
        """the n elements at the pointer (a view: gap rows of a panel included)"""
        return self.buf[self.off:self.off + self.n]

    def columns(self):
        """a strided panel as a (ncols, rows) view: row j is column j"""
        return torch.as_strided(self.buf, (self.ncols, self.rows), (self.ld, 1), self.off)

    def get(self):
        """numpy copy of the payload: (rows, ncols) for a panel, else the n elements"""
        if self.rows is not None:
            return self.columns().cpu().numpy().T.copy() if self.ncols else np.zeros((self.rows, 0))
        return self.payload().cpu().numpy().copy()

    def check(self):
        now, was = self.bits.cpu(), self.before.cpu()
        changed = now != was
        lo, hi = self.off, self.off + self.n
        where = {"left": (0, lo), "right": (hi, now.numel())}
        for side, (a, b) in where.items():
            bad = torch.nonzero(changed[a:b])
            assert bad.numel() == 0, (f"{self.name}: the {side} guard was written at offset {int(bad[0]) + a - lo} from the payload's "
                                      f"start (extent {self.n}, shift {self.shift})")
        gap = changed[lo:hi] & ~self.is_payload
        bad = torch.nonzero(gap)
        assert bad.numel() == 0, (f"{self.name}: a gap row between the logical height {self.rows} and the leading dimension {self.ld} "
                                  f"was written at offset {int(bad[0]) if bad.numel() else -1} from the payload's start")
        if self.role == "in":
            bad = torch.nonzero(changed[lo:hi])
            assert bad.numel() == 0, f"{self.name}: an input was written at offset {int(bad[0]) if bad.numel() else -1}"
            return
        sent = now[lo:hi] == _sentinel(self.dtype)
        if self.role == "out":
            bad = torch.nonzero(sent & self.is_payload & ~self.untouched)
            assert bad.numel() == 0, (f"{self.name}: payload element {int(bad[0]) if bad.numel() else -1} of {self.n} was not written "
                                      "(it still holds the sentinel)")
            bad = torch.nonzero(~sent & self.untouched)
            assert bad.numel() == 0, (f"{self.name}: element {int(bad[0]) if bad.numel() else -1} is documented as not touched "
                                      "and was written")
        if self.dtype == torch.float64:
            nan = torch.isnan(self.payload().cpu()) & self.is_payload & ~self.untouched
            bad = torch.nonzero(nan)
            assert bad.numel() == 0, (f"{self.name}: payload element {int(bad[0]) if bad.numel() else -1} of {self.n} is NaN "
                                      "(a guard or a neighbour's NaN was read and used)")


def guarded(n, dtype=torch.float64, role="out", shift=0, device="cpu", **kw):
    return Guarded(n, dtype, role, shift, device, **kw)


class Net:
    """The guarded arrays of one call: make them, pass their .ptr, synchronise, check()."""

    def __init__(self, device="cpu", shift=0):
        self.device, self.shift, self.arrays = device, shift, []

    def _add(self, a):
        self.arrays.append(a)
        return a

    def _shift(self, dtype):
        return self.shift if dtype == torch.float64 else 0       # the shift is that of the floating-point arrays

    def out(self, name, n, dtype=torch.float64, untouched=None):
        return self._add(Guarded(n, dtype, "out", self._shift(dtype), self.device, name=name, untouched=untouched))

    def inp(self, name, data, dtype=torch.float64, role="in"):
        data = np.asarray(data)
        return self._add(Guarded(data.size, dtype, role, self._shift(dtype), self.device, data=data, name=name))

    def panel_out(self, name, rows, ncols, ld, untouched_rows=None):
        """untouched_rows: a mask over the rows of every column that the call is documented not to write"""
        n = (ncols - 1) * ld + rows if ncols > 0 else 0
        mask = None
        if untouched_rows is not None and n:
            per_col = np.zeros(ld, dtype=bool)
            per_col[:rows] = np.asarray(untouched_rows, dtype=bool)
            mask = np.tile(per_col, ncols)[:n]
        return self._add(Guarded(n, torch.float64, "out", self.shift, self.device, name=name, rows=rows, ld=ld, untouched=mask))

    def panel_in(self, name, data, ld, role="in"):
        data = np.asarray(data, dtype=np.float64)
        rows, ncols = data.shape
        n = (ncols - 1) * ld + rows if ncols > 0 else 0
        return self._add(Guarded(n, torch.float64, role, self.shift, self.device, data=data, name=name, rows=rows, ld=ld))

    def check(self):
        for a in self.arrays:
            a.check()
