"""The SPIR-V interpreter of spirv_interp.py, extended with what the reference's compiled Mandelbulb shader needs.

TEST INFRASTRUCTURE ONLY.  spirv_interp.py stays as it is (test_spv_golden.py and the committed fixtures depend on
it).  This module loads a private copy of it and adds, with the same numerics (IEEE binary32, one rounding per operation,
numpy's float32 functions for the transcendentals):
  GLSL.std.450  Acos (17), Cross (68), Normalize (69), Reflect (71)
  core          OpTypeMatrix (24), OpSMod (139), OpFMod (141), OpMatrixTimesVector (145), OpIsNan (156), OpIsInf (157)
The core opcodes are rewritten at load time into extended instructions of a private range (>= 0x10000, which no
GLSL.std.450 instruction uses), so the interpreter's own dispatch runs them.  Operation orders:
  cross(a, b)        (a1*b2 - b1*a2, a2*b0 - b2*a0, a0*b1 - b0*a1)
  normalize(v)       v[k] / length(v)
  reflect(I, N)      I - (2 * dot(N, I)) * N
  mod(x, y) float    x - y * floor(x / y);  int: x - y * floor(x / y) exactly (the result takes the divisor's sign)
  M * v              sum over columns in order: ((c0*v0 + c1*v1) + c2*v2)
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_spirv_interp_ext_base",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "spirv_interp.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

F32, Cell, Invocation = base.F32, base.Cell, base.Invocation
_lift1, _lift2 = base._lift1, base._lift2

_SMOD, _FMOD, _MTV, _ISNAN, _ISINF = 0x10000, 0x10001, 0x10002, 0x10003, 0x10004


def _cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def _normalize(v):
    n = base._length(v)
    return [e / n for e in v]


def _reflect(i, n):
    d = n[0] * i[0]
    for k in range(1, len(i)):
        d = d + n[k] * i[k]
    k2 = F32(2.0) * d
    return [i[k] - k2 * n[k] for k in range(len(i))]


def _fmod(x, y):
    return x - y * F32(np.floor(x / y))


def _smod(x, y):
    return base._i32(x - y * (x // y)) if y else 0


def _mat_times_vec(m, v):
    out = [c * v[0] for c in m[0]]
    for j in range(1, len(m)):
        out = [s + c * v[j] for s, c in zip(out, m[j])]
    return out


base._GLSL.update({
    17: _lift1(lambda a: F32(np.arccos(a))),
    68: _cross,
    69: _normalize,
    71: _reflect,
    _SMOD: _lift2(_smod),
    _FMOD: _lift2(_fmod),
    _MTV: _mat_times_vec,
    _ISNAN: _lift1(lambda a: bool(np.isnan(a))),
    _ISINF: _lift1(lambda a: bool(np.isinf(a))),
})

_REWRITE = {139: _SMOD, 141: _FMOD, 145: _MTV, 156: _ISNAN, 157: _ISINF}


class Module(base.Module):
    def __init__(self, path: str):
        super().__init__(path)
        import struct
        raw = open(path, "rb").read()
        w = struct.unpack("<%dI" % (len(raw) // 4), raw)
        i = 5
        while i < len(w):
            op, n = w[i] & 0xFFFF, w[i] >> 16
            if op == 24:                                   # OpTypeMatrix: result, column type, column count
                self.types[w[i + 1]] = ("mat", w[i + 2], w[i + 3])
            i += n
        for f in self.functions.values():
            for label, block in f["blocks"].items():
                for k, (op, a) in enumerate(block):
                    if op in _REWRITE:                     # (result type, result, operands...) -> ExtInst
                        block[k] = (12, (a[0], a[1], 0, _REWRITE[op]) + tuple(a[2:]))

    def default(self, tid):
        t = self.types[tid]
        if t[0] == "mat":
            return [self.default(t[1]) for _ in range(t[2])]
        return super().default(tid)
