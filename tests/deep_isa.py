"""fr_device.hip compiled for gfx950, device side only, once per session: every deep kernel's resource remarks and assembly.
deep_kernel<DeepBlock<F, X, DE, BLA>> is keyed by (formula, X, DE, BLA), parsed from its symbol; the six level kernels by name."""
import collections
import functools
import itertools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Kernel = collections.namedtuple("Kernel", "symbol usage asm")    # usage: remark -> int; asm: the body's lines behind its label
LEVEL_KERNELS = {"deep_bla_level_kernel", "deepx_bla_level_kernel", "deep_ship_bla_level_kernel", "deepx_ship_bla_level_kernel",
                 "deep_julia_bla_level_kernel", "deepx_julia_bla_level_kernel"}
# the blocks' names while each was a struct of its own (DeepArgs .. DeepJuliaXDeBlaArgs; no ship DE): the budgets' keys
OLD_NAMES = {"Deep" + f.replace("Mandel", "") + "X" * x + "De" * de + "Bla" * bla + "Args": (f, x, de, bla)
             for f, x, de, bla in itertools.product(("Mandel", "Ship", "Julia"), (False, True), (False, True), (False, True))
             if not (f == "Ship" and de)}


def by_old_name():
    """kernels() under the blocks' old names and the level kernels' own; None without hipcc"""
    built = kernels()
    return built and {**{name: built[key] for name, key in OLD_NAMES.items()}, **{name: built[name] for name in LEVEL_KERNELS}}


def key_of(symbol):
    """(formula, X, DE, BLA) of a deep_kernel instantiation, the name of a level kernel, None for anything else"""
    m = re.match(r"^_ZN2fr\d+deep_kernelINS_\d+DeepBlockINS_\d+(\w+?)FormulaELb([01])ELb([01])ELb([01])EEEEEvT_$", symbol)
    if m:
        return (m.group(1),) + tuple(b == "1" for b in m.group(2, 3, 4))
    m = re.match(r"^_ZN2fr\d+(deepx?_\w*?level_kernel)E", symbol)
    return m.group(1) if m else None


@functools.lru_cache(maxsize=None)
def kernels():
    """key -> Kernel for every deep_kernel instantiation and level kernel of the file; None without hipcc"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    csrc = os.path.join(ROOT, "fractalrenderer_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fr_device.s")
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                              "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S",
                              os.path.join(csrc, "fr_device.hip"), "-o", path, "-Rpass-analysis=kernel-resource-usage"],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        asm = open(path).read().split("\n")
    found, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur, key = None, key_of(m.group(1))
            if key is not None:
                assert key not in found, m.group(1)
                start, =[i for i, t in enumerate(asm) if t.startswith(m.group(1) + ":")]
                end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
                cur = found[key] = Kernel(m.group(1), {}, asm[start + 1:end])
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur.usage[m.group(1)] = int(m.group(2))
    return found
