"""The plan flag of the survivor stream's second class ("whole_blocks", fr_plan.h: RenderPlan::whole_blocks_apply), pinned
without a GPU across the three things it depends on: whether the lane pool looks for cycles, stripes, staged or one pass."""
import pytest


def _params(fr, **kw):
    from fractalrenderer_amd import _capi
    p = _capi.fr_params()
    _capi.check(_capi.lib().fr_params_default(p))
    p.precision, p.max_iterations = 1, 1024
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("pool_looks", [False, True])
@pytest.mark.parametrize("stripes", [False, True])
@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("tuning", [0, 1, 2])
def test_flag_follows_pool_stripes_and_staging(fr, pool_looks, stripes, staged, tuning):
    from fractalrenderer_amd import _capi
    p = _params(fr, stripe_enabled=int(stripes))
    tunings = [("staging", 3 if staged else 1), ("whole_blocks", tuning)]
    got = _capi.plan_whole_blocks(p, 4096, 4096, None, 256, tunings, pool_looks)
    assert got == (staged and not stripes and not pool_looks and tuning != 1)      # (automatic: a frame of this size takes it)
    plan = _capi.plan_describe(p, 4096, 4096, None, 256, tunings)
    assert plan["nstages"] == (2 if staged else 1) and plan["family"] == (4 if stripes else 3)


def test_flag_is_the_lean_kernels(fr):
    """"whole_blocks" = 2: the general tile kernel writes one class; a Julia set, fp32 and a row-strip shard take the path; the
    sample grid of a staged SSAA frame is a lean render like any other and takes it too (the sample loop of the general tile
    kernel, "ssaa" = 1, does not); Deep_Zoom has no survivor stream"""
    from fractalrenderer_amd import _capi
    p = _params(fr)
    on = [("staging", 3), ("whole_blocks", 2)]
    assert _capi.plan_whole_blocks(p, 1920, 1080, None, 256, on, False)
    assert not _capi.plan_whole_blocks(p, 1920, 1080, None, 256, on + [("tile_kernel", 1)], False)
    assert _capi.plan_whole_blocks(p, 1920, 1080, _capi.fr_shard(1, 2, 8), 256, on, False)
    assert not _capi.plan_whole_blocks(p, 1920, 1080, _capi.fr_shard(1, 2, 12), 256, on, False)    # strips of no whole sub-tile rows
    assert _capi.plan_whole_blocks(_params(fr, fractal_type=1, precision=0), 1920, 1080, None, 256, on, False)
    ssaa = _params(fr, antialiasing_samples=2)
    assert _capi.plan_describe(ssaa, 520, 504, None, 256, on)["route"] == 3
    assert _capi.plan_whole_blocks(ssaa, 520, 504, None, 256, on, False)
    assert not _capi.plan_whole_blocks(ssaa, 520, 504, None, 256, on, True)
    assert not _capi.plan_whole_blocks(ssaa, 520, 504, None, 256, on + [("ssaa", 1)], False)
    assert _capi.plan_whole_blocks(ssaa, 520, 504, None, 256, on + [("ssaa_band_samples", 200000)], False)     # banded
    assert not _capi.plan_whole_blocks(_params(fr, fractal_type=5), 520, 504, None, 256, on, False)
    with pytest.raises(_capi.FractalRendererError):
        _capi.plan_whole_blocks(p, 64, 64, None, 256, [("whole_blocks", 3)], False)


def test_automatic_rule(fr):
    """"whole_blocks" = 0: fp64 frames with at least 16 blocks of 64 pixels per wave of the lane pool's grid (fr_plan.h,
    kWholeBlocksPerWave; 256 compute units x 6 workgroups x 4 waves = 6144 waves: from 6.3 M pixels)"""
    from fractalrenderer_amd import _capi
    p = _params(fr)
    off = [("periodicity", -1)]
    assert _capi.plan_whole_blocks(p, 4096, 4096, None, 256, off, False)                     # the C2 frame
    assert _capi.plan_whole_blocks(p, 3840, 2160, None, 256, off, False)
    assert not _capi.plan_whole_blocks(p, 1920, 1080, None, 256, off, False)
    assert _capi.plan_whole_blocks(p, 6144 * 16, 64, None, 256, off, False)
    assert not _capi.plan_whole_blocks(p, 6144 * 16 - 1, 64, None, 256, off, False)
    assert not _capi.plan_whole_blocks(p, 4096, 4096, None, 256, [], True)                   # the library's default: the pool looks
    assert not _capi.plan_whole_blocks(_params(fr, precision=0), 4096, 4096, None, 256, off, False)
    assert _capi.plan_whole_blocks(p, 1920, 1080, None, 8, off, False)                       # 8 compute units: 192 waves


def test_two_class_kernels_keep_the_register_budget(fr):
    """The tile pass of a render with two classes is tile_lean_kernel<T, F, false, NP + 2>: the fp64 Mandelbrot instantiation
    is held to the budget tests/test_host.py holds the one-class kernel to (the launcher sizes the grid for 5 workgroups per
    CU), and so is its lane pool, pool_kernel<T, F + 8, false> (6 per CU, no spilled SGPR)."""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(root, "fractalrenderer_amd", "csrc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-I" + os.path.join(root, "include"), "-I" + csrc, "-c", os.path.join(csrc, "fr_device.hip"),
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    budget = {   # mangled name: (max VGPRs, min waves/SIMD, max SGPR spills)
        "_ZN2fr16tile_lean_kernelIdLi0ELb0ELi4EEEvNS_10LaunchArgsE": (96, 5, 20),   # fp64 Mandelbrot, two sub-tiles per trip (C2)
        "_ZN2fr16tile_lean_kernelIdLi0ELb0ELi3EEEvNS_10LaunchArgsE": (96, 5, 20),   # ... one
        "_ZN2fr16tile_lean_kernelIfLi1ELb0ELi4EEEvNS_10LaunchArgsE": (64, 6, 0),    # fp32 Julia
        # the lane pool of a stream in two classes, pool_kernel<T, F + 8, false>: the one-class kernel's budget
        "_ZN2fr11pool_kernelIdLi8ELb0EEEvNS_10LaunchArgsE": (80, 6, 0),             # fp64 Mandelbrot (C2)
        "_ZN2fr11pool_kernelIfLi9ELb0EEEvNS_10LaunchArgsE": (64, 6, 0),             # fp32 Julia
    }
    for name, (vgprs, waves, spills) in budget.items():
        u = usage[name]
        print(name, u)
        assert u["VGPRs"] <= vgprs and u["Occupancy [waves/SIMD]"] >= waves and u["SGPRs Spill"] <= spills, (name, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
