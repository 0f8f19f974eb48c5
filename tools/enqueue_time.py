"""Wall time of fr_render_shard_async alone, us per call (mean of 3000 calls, best of 5 passes), on a 256x256 frame at max_iter 64
and a 1920x1080 frame at max_iter 1024, for the library FR_LIB_PATH names (default: the in-tree build).  A/B use: run it and
bench.py --workload c2 / c3 / stripes alternately with FR_LIB_PATH set to the parent's and the branch's library
(in the manner of profiles/pool_refactor_ab.txt)."""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fractalrenderer_amd as fr
from fractalrenderer_amd import _capi
L = _capi.lib()
res = []
for W, H, mi in ((256, 256, 64), (1920, 1080, 1024)):
    with fr.Renderer(0) as r:
        st = fr.FractalState(max_iterations=mi)
        p = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F32)
        it = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        out = _capi.fr_output(None, None, it.data_ptr(), _capi.FR_MEM_DEVICE, _capi.FR_LAYOUT_PACKED)
        r.reserve(st, W, H, fractal_type=fr.FractalType.Mandelbrot, precision=fr.Precision.F32)
        n = 3000
        best = 1e9
        for rep in range(5):
            for _ in range(200):
                _capi.check(L.fr_render_shard_async(r._ctx, C.byref(p), W, H, None, C.byref(out), None))
            _capi.check(L.fr_ctx_synchronize(r._ctx))
            tot = 0.0
            for k in range(n):
                t0 = time.perf_counter_ns()
                L.fr_render_shard_async(r._ctx, C.byref(p), W, H, None, C.byref(out), None)
                tot += time.perf_counter_ns() - t0
                if k % 64 == 63: _capi.check(L.fr_ctx_synchronize(r._ctx))     # keep the queue short: time the call, not back-pressure
            _capi.check(L.fr_ctx_synchronize(r._ctx))
            best = min(best, tot / n / 1e3)
        res.append(best)
print("ENQUEUE_US %.3f %.3f" % tuple(res))
