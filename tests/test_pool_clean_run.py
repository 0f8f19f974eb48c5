"""The lane pool's clean run: a run of clean unchecked stretches that reach no deadline is a loop of its own inside
pool_kernel's stretch loop, around the 16-update block, and carries nothing but the stretch-start z.

Without a GPU: the compiler's output for gfx950 must show that loop -- the loop immediately around the 16-update block holds
a handful of vector instructions besides the fp64 arithmetic, not the two dozen register copies of the whole stretch state
machine.  On the GPU: the schedule is the one it was, update for update, so every plane of the tile pass + lane pool render
is bit-identical to the single pass (and within the bars of test_gpu_parity.py of the oracle) where runs of clean stretches
start, cross deadlines, end on them and are broken by dirty stretches.
"""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cases import CASES, SEAHORSE
from test_gpu_parity import check_against, gpu_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- without a GPU: the shape of the compiled loop -------------------------------------------------------------------

MAX_OTHER_VALU = 8      # vector instructions that are not fp64 arithmetic, per trip of the clean-run loop (4 as built: the
                        # stretch-start z kept for the deferred-escape ring, and its way back)


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    """fr_device.hip compiled for gfx950 to assembly, with the flags of test_hot_kernels_keep_their_register_budget."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "fractalrenderer_amd", "csrc")
    out = str(tmp_path_factory.mktemp("asm") / "fr_device.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S",
                        os.path.join(csrc, "fr_device.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read().splitlines()


def basic_blocks(asm, kernel):
    """The basic blocks of one function of the compiler's assembly: label, instructions, and what the loop annotations say:
    the header of the innermost loop the block is in (`loop`), whether it is a loop header itself, its enclosing loops."""
    start = next(i for i, l in enumerate(asm) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    blocks, cur = [], None
    for l in asm[start + 1:end]:
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(;.*)?$", l)
        if m:
            cur = {"label": m.group(1) or "bb." + m.group(2), "notes": m.group(3) or "", "ins": []}
            blocks.append(cur)
            continue
        if cur is None:
            continue
        s = l.strip()
        if s.startswith(";"):
            if not cur["ins"]:
                cur["notes"] += " " + s         # the annotations continue on the lines below the label
        elif s and not s.startswith("."):
            cur["ins"].append(s.split(";")[0].strip())
    for b in blocks:
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", b["notes"])
        b["loop"] = m.group(1) if m else None
        b["header"] = "Loop Header" in b["notes"]
        b["parents"] = [(h, int(d)) for h, d in re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", b["notes"])]
    return blocks


def is_f64(ins):
    return re.match(r"v_\w+_f64", ins) is not None


def is_f64_arithmetic(ins):
    return re.match(r"v_(fma|fmac|mul|add)_f64", ins) is not None


def other_valu_around_the_block(asm, kernel):
    """Vector instructions other than *_f64 in the loop immediately around the 16-update block (a basic block of exactly 96
    fp64 arithmetic instructions that branches to itself), that block left out; one figure per such block."""
    blocks = basic_blocks(asm, kernel)
    hot = [b for b in blocks if sum(map(is_f64_arithmetic, b["ins"])) == 96
           and any(re.match(r"s_cbranch\S+\s+\.L%s$" % re.escape(b["label"]), i) for i in b["ins"])]
    assert hot, "no 16-update block (96 fp64 instructions, branching to itself) in " + kernel
    counts = []
    for h in hot:
        assert h["parents"], "the 16-update block %s has no enclosing loop" % h["label"]
        outer = max(h["parents"], key=lambda p: p[1])[0]
        headers = {outer} | {b["label"] for b in blocks if b["header"] and any(p == outer for p, _ in b["parents"])}
        members = [b for b in blocks if b is not h and (b["label"] in headers or b["loop"] in headers)]
        counts.append(sum(1 for b in members for i in b["ins"] if i.startswith("v_") and not is_f64(i)))
    return counts


PLAIN = "_ZN2fr11pool_kernelIdLi0ELb0EEEvNS_10LaunchArgsE"


def test_clean_run_loop_carries_no_lane_state(device_asm):
    """The loop immediately around the 16-update block of pool_kernel<double, 0, false> is the clean run: besides fp64
    arithmetic it holds at most MAX_OTHER_VALU vector instructions.  (Where the clean stretch shares its loop with the dirty
    path, reach_deadline and the tested stretch, that loop is the whole stretch state machine: 25 register copies on the
    clean path alone.)  The kernel that closes cycles keeps the general form and is not held to it."""
    counts = other_valu_around_the_block(device_asm, PLAIN)
    print(PLAIN, "vector instructions other than fp64 around the 16-update block:", counts)
    assert len(counts) == 1 and counts[0] <= MAX_OTHER_VALU, counts


# ---- on the GPU: the same planes, bit for bit -------------------------------------------------------------------------

VIEWS = {   # name: (parameters of the view, W, H)
    # inside the main cardioid: no sample ever escapes -- every stretch is clean, whole refill groups meet one deadline
    "interior": (dict(center_x=-0.2, center_y=0.0, zoom=0.3), 67, 45),
    "default": (dict(), 136, 104),
    # dirty stretches between clean runs, ring replays
    "seahorse": (dict(center_x=SEAHORSE[0], center_y=SEAHORSE[1], zoom=0.008), 101, 77),
}
TILE_BUDGET = 16
# updates left to the lane pool: a deadline inside a block right after the first one (23; the planner stages a forced
# schedule from max_iter >= 2 * stage_first, so no staged frame leaves the pool fewer than 16), whole blocks, 1 and 15 mod
# 16, and runs long enough for the streak to reach 6, whose 64-update stretches cross deadlines and end on them
REMAINING = [23, 32, 97, 111, 400, 1040]


@functools.lru_cache(maxsize=None)
def _oracle_render(oracle, key, W, H):
    return oracle.render(oracle.OracleParams(**dict(key)), W, H)


_single_pass = {}


def single_pass(fr, renderer, key, p, W, H):
    """The staging=1 render of a view, made once per view and max_iter."""
    if (key, W, H) not in _single_pass:
        try:
            renderer.set_option("staging", 1)
            _single_pass[(key, W, H)] = gpu_render(fr, renderer, p, W, H)
            assert renderer.last_stages() == 1
        finally:
            renderer.set_option("staging", 0)
    return _single_pass[(key, W, H)]


def pool_against_single_pass(fr, renderer, oracle, kw, W, H, refill_at=0, periodicity=0):
    key = tuple(sorted(kw.items()))
    p = oracle.OracleParams(**kw)
    ref = _oracle_render(oracle, key, W, H)
    base = single_pass(fr, renderer, key, p, W, H)
    try:
        renderer.set_option("staging", 3)
        renderer.set_option("stage_first", TILE_BUDGET)
        renderer.set_option("pool_refill_at", refill_at)
        renderer.set_option("periodicity", periodicity)
        rgba, nu, it = gpu_render(fr, renderer, p, W, H)
        stages = renderer.last_stages()
    finally:
        for k in ("staging", "stage_first", "pool_refill_at", "periodicity"):
            renderer.set_option(k, 0)
    assert stages == 2
    for a, b in zip(base, (rgba, nu, it)):
        assert np.array_equal(a, b)
    check_against(p, ref.iter, ref.nu, ref.rgba, rgba, nu, it)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("periodicity", [-1, 1])
@pytest.mark.parametrize("refill_at", [1, 16, 64])
@pytest.mark.parametrize("remaining", REMAINING)
@pytest.mark.parametrize("view", sorted(VIEWS))
def test_clean_runs_fp64_mandelbrot(fr, renderer, oracle, view, remaining, refill_at, periodicity):
    kw, W, H = VIEWS[view]
    max_iter = TILE_BUDGET + remaining
    ref = pool_against_single_pass(fr, renderer, oracle, dict(kw, max_iterations=max_iter), W, H, refill_at, periodicity)
    if view == "interior":
        assert np.all(ref.iter == max_iter), "the interior view has escaping samples: it no longer tests what it is for"


@pytest.mark.gpu
def test_clean_runs_fp32_julia(fr, renderer, oracle):
    """pool_kernel<float, 1, false>: the C3 constant."""
    kw = dict(fractal=1, precision=0, center_x=0.0, center_y=0.0, zoom=3.0, max_iterations=272, julia_c_real=-0.8, julia_c_imag=0.156)
    pool_against_single_pass(fr, renderer, oracle, kw, 96, 64, periodicity=-1)
    pool_against_single_pass(fr, renderer, oracle, kw, 96, 64, periodicity=1)


@pytest.mark.gpu
def test_clean_runs_fp64_burning_ship(fr, renderer, oracle):
    """pool_kernel<double, 2, *>."""
    p, W, H = CASES["ship_f64_ragged_mi2048"]
    kw = dict(fractal=2, center_x=p.center_x, center_y=p.center_y, zoom=p.zoom, max_iterations=528,
              color_scale=p.color_scale, palette_mode=p.palette_mode)
    pool_against_single_pass(fr, renderer, oracle, kw, W, H, periodicity=-1)
    pool_against_single_pass(fr, renderer, oracle, kw, W, H, periodicity=1)
