"""Guarded, poisoned device buffers for the C-ABI entry points (tests/test_buffers_*.py).

Every argument of a call gets ONE allocation laid out as [front guard | payload | back guard].  Each guard is GUARD_BYTES (16 KiB:
wider than one tile row of any kernel, so a wrong stride lands inside it) and the payload starts 256-byte aligned (the alignment the
stem checks) unless the argument is given a `skew`: the payload then starts `skew` ELEMENTS past a 256-byte boundary, the guards
still contiguous around it (tests/test_alignment_gpu.py: "at which address").  Everything a kernel could write lands inside the one
allocation: a stray write is DATA here, never a fault.

The payload is filled by the argument's role, and check() compares bit patterns, not values:

  role "in"       the caller's tensor, unchanged by the call (the const contract); input halos stay zero as the contract requires
  role "out"      MUST be written: the interior is pre-filled with POISON (a quiet NaN with its own payload; int32 -0x5A5A5A5B) of
                  which no element may remain; an output halo (`halo` > 0) is filled with SENTINEL, which must survive bit for bit
                  ("kernels write interiors only", include/s3r.h); with halo_zeros=True, for the kernels s3r.h names as
                  rewriting the halo rows of their interior planes, each halo element is the sentinel or +0.0 (bits 0)
  role "scratch"  contents irrelevant: NaN-filled (fill="nan") or zero-filled (fill="zero"); the test compares the results of the
                  two fillings bit for bit

Guards hold GUARD (fp32 0x7FA5A5A5 / bf16 0x7FA5: signalling-NaN payloads no kernel produces; int32 0xA5A5A5A5).  The int32 guard
and poison are the same bit pattern (two's complement): both are negative, and every int32 output of the library (indices,
counts) is >= 0, so neither can be a legitimate value.

Skews are given per argument (`skew=`), or by argument name for a whole test body: `with skews({"x": 1, "y": 3}):` or
`with skews(lambda name, dtype, role: ...)` — every Guarded built inside takes its skew from there unless it passes one itself.

check() returns None or the FIRST offending place, e.g. "back guard of scratch +1344" (element offset from the start of that
region) or "leftover poison in y +17 (index (0, 1, 2, 3))".
"""
from __future__ import annotations

import contextlib

import torch

GUARD_BYTES = 16384
ALIGN = 256

# dtype -> (bit-view dtype, guard, poison, halo sentinel, scratch NaN), as values of the signed bit view
_BITS = {
    torch.float32: (torch.int32, 0x7FA5A5A5, 0x7FE5A5A5, 0x7FD5A5A5, 0x7FC00000),
    torch.bfloat16: (torch.int16, 0x7FA5, 0x7FE5, 0x7FD5, 0x7FC0),
    torch.int32: (torch.int32, -0x5A5A5A5B, -0x5A5A5A5B, -0x2B2B2B2C, None),
    torch.uint8: (torch.uint8, 0xA5, None, None, None),
}


def _as_bits(t):
    return t.view(_BITS[t.dtype][0])


def interior_mask(shape, halo, spatial):
    """bool mask of a halo-padded buffer's interior: `spatial` lists the dims that carry the halo"""
    m = torch.ones(shape, dtype=torch.bool)
    if halo:
        for d in spatial:
            idx = [slice(None)] * len(shape)
            idx[d] = slice(0, halo)
            m[tuple(idx)] = False
            idx[d] = slice(shape[d] - halo, shape[d])
            m[tuple(idx)] = False
    return m


_SKEWS = [None]          # the innermost `with skews(...)`: a dict name -> elements, or a callable (name, dtype, role) -> elements


@contextlib.contextmanager
def skews(by_name):
    """every Guarded built in the body that passes no skew of its own takes `by_name[name]` (a dict; a missing name is 0) or
    `by_name(name, dtype, role)` (a callable) elements"""
    _SKEWS.append(by_name)
    try:
        yield
    finally:
        _SKEWS.pop()


def _skew_of(name, dtype, role):
    s = _SKEWS[-1]
    if s is None:
        return 0
    return int(s(name, dtype, role) if callable(s) else s.get(name, 0))


class Guarded:
    """One argument of a call.  `.t` is the payload (a view of `shape`), `.ptr` its device address."""

    def __init__(self, name, shape, dtype, device, role, data=None, halo=0, spatial=(), fill="nan", mask=None, halo_zeros=False, skew=None):
        if isinstance(shape, int):
            shape = (shape,)
        self.name, self.shape, self.dtype, self.role = name, tuple(shape), dtype, role
        esz = torch.empty(0, dtype=dtype).element_size()
        self.g = GUARD_BYTES // esz
        n = 1
        for s in self.shape:
            n *= s
        self.n = n
        self.skew = _skew_of(name, dtype, role) if skew is None else int(skew)
        assert self.skew >= 0
        base = torch.empty(2 * self.g + n + self.skew + ALIGN // esz, dtype=dtype, device=device)
        lead = (-base.data_ptr()) % ALIGN // esz + self.skew     # (the device allocator aligns already; the host one may not)
        self.raw = base[lead:lead + 2 * self.g + n]
        bits = _as_bits(self.raw)
        bits.fill_(_BITS[dtype][1])
        self.t = self.raw[self.g:self.g + n].view(self.shape)
        self.ptr = self.raw.data_ptr() + GUARD_BYTES             # (an empty payload has no address of its own)
        assert (self.ptr - self.skew * esz) % ALIGN == 0 and (n == 0 or self.t.data_ptr() == self.ptr), \
            "payload must start skew elements past a 256-byte aligned address (skew 0: 256-byte aligned), guards contiguous around it"
        self.mask = None
        self.halo_zeros = halo_zeros          # the kernel may rewrite the halo with +0.0 (the zeros the contract says it holds)
        if role == "in":
            assert data is not None
            self.t.copy_(data.reshape(self.shape))
            self.snapshot = _as_bits(self.t).clone()
        elif role == "out":
            self.mask = (mask if mask is not None else interior_mask(self.shape, halo, spatial)).to(device)
            b = _as_bits(self.t)
            b.fill_(_BITS[dtype][2])
            if not bool(self.mask.all()):
                b[~self.mask] = _BITS[dtype][3]
        elif role == "scratch":
            if fill == "nan":
                _as_bits(self.t).fill_(_BITS[dtype][4])
            elif fill == "zero":
                self.t.zero_()
            else:
                raise ValueError(fill)
        else:
            raise ValueError(role)

    def _first(self, bad, region, shape=None):
        i = int(bad.reshape(-1).nonzero()[0, 0])
        if shape is None:
            return f"{region} of {self.name} +{i}"
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), shape))
        return f"{region} {self.name} +{i} (index {idx})"

    def check(self):
        """None, or the first offending offset and region"""
        bits = _as_bits(self.raw)
        guard = _BITS[self.dtype][1]
        front, back = bits[:self.g], bits[self.g + self.n:]
        if not bool((front == guard).all()):
            return self._first((front != guard).cpu(), "front guard")
        if not bool((back == guard).all()):
            return self._first((back != guard).cpu(), "back guard")
        pb = _as_bits(self.t)
        if self.role == "in":
            if not torch.equal(pb, self.snapshot):
                return self._first((pb != self.snapshot).cpu(), "change of the input", self.shape)
        elif self.role == "out":
            poison = _BITS[self.dtype][2]
            left = (pb == poison) & self.mask
            if bool(left.any()):
                return self._first(left.cpu(), "leftover poison in", self.shape)
            if not bool(self.mask.all()):
                sent = _BITS[self.dtype][3]
                hit = (pb != sent) & ~self.mask
                if self.halo_zeros:
                    hit &= pb != 0
                if bool(hit.any()):
                    return self._first(hit.cpu(), "write into the halo of", self.shape)
        return None


def check_all(*bufs):
    """assert that no buffer reports a problem; the message names the first one found"""
    for b in bufs:
        where = b.check()
        assert where is None, where
