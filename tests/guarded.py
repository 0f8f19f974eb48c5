"""Guard-banded output planes: what a call stored, and where.

A plane of `rows * W` elements lives inside a larger buffer, with a guard band before and after it.  Payload and guards
are filled with a bit pattern no kernel produces (a quiet NaN with a recognisable payload for the float planes, a fixed
odd constant for iter); after a call the buffer answers
  guards_intact()       every guard byte still holds the pattern;
  unwritten(rows_mask)  how many payload elements of the given rows (default: all) still hold the pattern;
  untouched(rows_mask)  every element of the given rows still holds the pattern (the rows of OTHER parts under
                        FR_LAYOUT_FRAME).
Every comparison is on the integer view of the bytes, never a float ==: a NaN is a value like any other here.

Backends: "device" (torch tensors on cuda:0; the contiguous payload views go through data_ptr(), which Renderer._ptr
accepts) and "host" (numpy arrays, FR_MEM_HOST).  Guarded: one 1-D buffer of any element type (the export kernels'
outputs); GuardedPlanes: the rgba / nu / iter planes of a render, any of them None.
"""
from __future__ import annotations

import numpy as np

F32_PATTERN = 0x7FC5A5A5                 # quiet NaN, payload 0x5A5A5
F64_PATTERN = 0x7FF8A5A5C3C3A5A5         # quiet NaN, payload 0xA5A5C3C3A5A5
I32_PATTERN = 0x5A5A5A5B                 # odd, far above any iteration count, not -1 (Mandelbulb's miss)
MIN_GUARD = 4096

_INT_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def guard_elements(W: int) -> int:
    """elements per guard band of a plane W wide: a whole row of 8 x 8 sub-tiles of overshoot, and at least 4096"""
    return max(8 * ((W + 7) // 8 * 8), MIN_GUARD)


class Guarded:
    """`n` elements of `dtype` between two guard bands of `guard` elements, all filled with the integer `pattern`.
    `offset` moves the payload that many elements into the leading guard's end (a caller's sub-buffer at an odd address):
    the bands are then guard + offset and guard - offset elements long."""

    def __init__(self, n: int, dtype, pattern: int, guard: int, backend: str = "host", offset: int = 0):
        self.dtype = np.dtype(dtype)
        self.int_dtype = np.dtype(_INT_OF[self.dtype.itemsize])
        self.n, self.pattern, self.backend = int(n), int(pattern), backend
        assert guard * self.dtype.itemsize % 16 == 0, "guard bands are multiples of 16 bytes"
        assert 0 <= offset < guard
        self.lo = guard + offset
        self.total = 2 * guard + self.n
        if backend == "host":
            self._buf = np.full(self.total, self.pattern, self.int_dtype)
        elif backend == "device":
            import torch
            # torch has no unsigned arithmetic above 8 bits: the same bits as a signed integer
            tdt, ndt = {1: (torch.uint8, np.uint8), 2: (torch.int16, np.int16), 4: (torch.int32, np.int32),
                        8: (torch.int64, np.int64)}[self.dtype.itemsize]
            as_signed = int(np.array([self.pattern], self.int_dtype).view(ndt)[0])
            self._buf = torch.full((self.total,), as_signed, dtype=tdt, device="cuda:0")
            torch.cuda.synchronize()        # the fill ran on torch's stream; the library renders on its own
        else:
            raise ValueError(backend)

    # -- what the call gets -------------------------------------------------------------------------------------
    def payload(self, shape=None):
        """the payload as an array / tensor of the plane's own type (a contiguous view of the buffer)"""
        if self.backend == "host":
            v = self._buf[self.lo:self.lo + self.n].view(self.dtype)
        else:
            import torch
            tdt = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8,
                   "int16": torch.int16, "uint16": torch.int16}[self.dtype.name]
            v = self._buf[self.lo:self.lo + self.n].view(tdt)
        return v.reshape(shape) if shape is not None else v

    def address(self) -> int:
        return self._buf.ctypes.data + self.lo * self.dtype.itemsize if self.backend == "host" \
            else self._buf.data_ptr() + self.lo * self.dtype.itemsize

    # -- what the call left -------------------------------------------------------------------------------------
    def bits(self) -> np.ndarray:
        """the whole buffer, guards included, as unsigned integers on the host"""
        if self.backend == "host":
            return self._buf
        import torch
        torch.cuda.synchronize()
        return self._buf.cpu().numpy().view(self.int_dtype)

    def payload_bits(self) -> np.ndarray:
        return self.bits()[self.lo:self.lo + self.n]

    def values(self, shape=None) -> np.ndarray:
        v = self.payload_bits().view(self.dtype).copy()
        return v.reshape(shape) if shape is not None else v

    def guard_hits(self) -> int:
        b = self.bits()
        return int((b[:self.lo] != self.pattern).sum()) + int((b[self.lo + self.n:] != self.pattern).sum())

    def guards_intact(self) -> bool:
        return self.guard_hits() == 0

    def still_pattern(self) -> np.ndarray:
        """mask over the payload: True where an element still holds the pattern"""
        return self.payload_bits() == self.pattern


class GuardedPlane(Guarded):
    """one output plane: rows x W pixels of `comps` components"""

    def __init__(self, rows: int, W: int, comps: int, dtype, pattern: int, backend: str):
        self.rows, self.W, self.comps = int(rows), int(W), int(comps)
        super().__init__(self.rows * self.W * self.comps, dtype, pattern, guard_elements(W) * self.comps, backend)
        assert self.address() % 16 == 0 or comps != 4, "the rgba payload stays 16-byte aligned"

    @property
    def shape(self):
        return (self.rows, self.W, self.comps) if self.comps > 1 else (self.rows, self.W)

    def _rows(self, rows_mask) -> np.ndarray:
        m = self.still_pattern().reshape(self.rows, self.W * self.comps)
        return m if rows_mask is None else m[np.asarray(rows_mask)]

    def unwritten(self, rows_mask=None) -> int:
        return int(self._rows(rows_mask).sum())

    def untouched(self, rows_mask) -> bool:
        return bool(self._rows(rows_mask).all())


class GuardedPlanes:
    """The planes of one render of `rows` rows of a frame W wide: rgba (f32 x 4), nu (f32, or f64 with f64=True) and iter
    (i32), each inside its own guarded buffer; planes=("nu",) etc. leaves the others None (the library accepts any
    non-empty subset)."""

    NAMES = ("rgba", "nu", "iter")

    def __init__(self, rows: int, W: int, *, f64: bool, backend: str = "device", planes=NAMES):
        self.rows, self.W, self.backend = int(rows), int(W), backend
        spec = {"rgba": (4, np.float32, F32_PATTERN),
                "nu": (1, np.float64, F64_PATTERN) if f64 else (1, np.float32, F32_PATTERN),
                "iter": (1, np.int32, I32_PATTERN)}
        self.planes = {k: (GuardedPlane(rows, W, *spec[k], backend) if k in planes else None) for k in self.NAMES}
        assert any(p is not None for p in self.planes.values())

    def __getitem__(self, name) -> GuardedPlane:
        return self.planes[name]

    def present(self):
        return [(k, p) for k, p in self.planes.items() if p is not None]

    def kwargs(self) -> dict:
        """rgba= / nu= / iter= for Renderer.render*()"""
        return {k: (None if p is None else p.payload(p.shape)) for k, p in self.planes.items()}

    def output(self, capi, layout: int = 0):
        """the fr_output of the raw C ABI"""
        a = [None if p is None else p.address() for p in self.planes.values()]
        return capi.fr_output(a[0], a[1], a[2], capi.FR_MEM_DEVICE if self.backend == "device" else capi.FR_MEM_HOST, layout)

    def values(self):
        """(rgba, nu, iter) as numpy arrays on the host, None for an absent plane"""
        return tuple(None if p is None else p.values(p.shape) for p in self.planes.values())

    def guard_hits(self) -> dict:
        return {k: p.guard_hits() for k, p in self.present()}

    def guards_intact(self) -> bool:
        return all(p.guards_intact() for _, p in self.present())

    def unwritten(self, rows_mask=None) -> int:
        return sum(p.unwritten(rows_mask) for _, p in self.present())

    def untouched(self, rows_mask) -> bool:
        return all(p.untouched(rows_mask) for _, p in self.present())
