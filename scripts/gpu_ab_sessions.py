"""Developer tool: interleaved timing of a session's recompute from TWO builds of the library in one process — each
build drives a session of its own on the same synthetic cube, the two alternate round by round, and the fused launch's
time comes from the library's own hipEvents (THZ_STAGE_PIPELINE).  Unlike gpu_ab_builds.py (thz_pipeline_ex on shared
buffers, which always writes everything) this times what a session does between recomputes: the out-of-band zeros of
the spectrum and the amplitudes stay in place (fft_f.hpp, "keep range").  Also times the FIRST recompute after an
upload, which writes everything.
Usage: scripts/gpu_ab_sessions.py <other libthzgpu.so> [nx ny nt]; the first build is the package's own."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import thz_image_explorer_amd as pkg
from thz_image_explorer_amd import binding, Engine
import synth

other = sys.argv[1]
nx, ny, nt = (int(a) for a in (sys.argv[2:5] if len(sys.argv) > 4 else (1024, 1024, 4096)))
rounds = int(os.environ.get("THZ_AB_ROUNDS", "6"))
a = Engine(0)
lib_b = C.CDLL(other)
for name, res, args in binding.SYMBOLS:
    if hasattr(lib_b, name):
        fn = getattr(lib_b, name); fn.restype = res; fn.argtypes = args
b = Engine.__new__(Engine)
b.lib, b.ctx, b._bufs = lib_b, binding._P(), []
assert lib_b.thz_create(0, C.byref(b.ctx)) == 0
tm = synth.make_time(nt)
npix, nf = nx * ny, nt // 2 + 1
sides = {}
for name, e in (("this", a), ("other", b)):
    e.set_time_axis(tm)
    s = pkg.Session(e, nx, ny, tm)
    d_t = e.to_device(tm)
    e.synth_cube(e.lib.thz_session_buffer(s.h, pkg.BUF_RAW), npix, 0, d_t)
    s.upload(None, subtract_bias=False)
    e.enable_timing(2)
    sides[name] = (e, s)
H = np.zeros((nf, 2), np.float32); H[:, 0] = 0.7; H[:, 1] = 0.3


def timed(e, s, cfg, n):
    for _ in range(n):
        s.recompute(cfg)
    e.sync()
    ns, calls = e.timing_collect(binding.STAGE_PIPELINE)
    e.timing_collect(binding.STAGE_MEAN); e.timing_collect(binding.STAGE_FFT)
    return ns / calls * 1e-6


variants = [("sums", 1, None), ("no sums", 0, None), ("cmask+sums", 1, H)]
only = os.environ.get("THZ_AB_ONLY")
res, first = {}, {}
for vname, means, cm in variants:
    if only and vname not in only.split(","):
        continue
    cfg = pkg.chain_cfg_default(tm)
    cfg.want_means = means
    for name, (e, s) in sides.items():
        s.set_fd_filters(None, cm)
    for r in range(rounds + 1):
        for name, (e, s) in sides.items():
            if r == 0:
                s.upload(None, subtract_bias=False)     # the next recompute writes everything
                first[(vname, name)] = timed(e, s, cfg, 1)
                timed(e, s, cfg, 2)                     # warm-up of the steady state
            else:
                res.setdefault((vname, name), []).append(timed(e, s, cfg, 3))
print(f"{nx}x{ny}x{nt}: fused launch of a session recompute (hipEvents), 'this' = the package's build, 'other' = {other}")
for (vname, name), v in res.items():
    v = np.array(v)
    print(f"{vname:11s} {name:6s} steady: median {np.median(v):7.3f} ms  min {v.min():7.3f}  max {v.max():7.3f}  spread {100 * (v.max() - v.min()) / np.median(v):5.2f} %"
          f"   first recompute after an upload {first[(vname, name)]:7.3f} ms", flush=True)
for vname, _, _ in variants:
    if (vname, "this") in res:
        t, o = np.median(res[(vname, "this")]), np.median(res[(vname, "other")])
        print(f"{vname:11s} this / other = {t / o:.4f}  ({100 * (o - t) / o:+.2f} % faster)")
