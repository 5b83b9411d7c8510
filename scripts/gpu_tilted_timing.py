"""Developer tool: the fused chain (thz_pipeline, all outputs) at the trace lengths of a tilted 1001-sample scan, timed
with hipEvents from TWO builds of the library in one process on the same device buffers, alternating — this build in
family 0 (FBP kernels, fft_fbp.hpp), this build in family 2 (the kernels over the F core: the cross-check that the old
path did not move) and another build (the parent commit).  Every measurement is `calls` launches (>= 0.3 s of timed
work); `rounds` repeats give the run-to-run spread.
Usage: scripts/gpu_tilted_timing.py <other libthzgpu.so> [nx ny] [nt ...]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from thz_image_explorer_amd import binding, Engine
import synth

other = sys.argv[1]
nx, ny = (int(a) for a in sys.argv[2:4]) if len(sys.argv) > 3 else (512, 512)
lengths = [int(a) for a in sys.argv[4:]] or [1041, 1101, 1152, 1153, 1201, 1280]
rounds = int(os.environ.get("THZ_AB_ROUNDS", "5"))
npix = nx * ny

this0, this2 = Engine(0), Engine(0)
this2.set_kernel_family(2)
lib_b = C.CDLL(other)
for name, res, args in binding.SYMBOLS:
    if hasattr(lib_b, name):
        fn = getattr(lib_b, name); fn.restype = res; fn.argtypes = args
parent = Engine.__new__(Engine)
parent.lib, parent.ctx, parent._bufs = lib_b, binding._P(), []
assert lib_b.thz_create(0, C.byref(parent.ctx)) == 0
engines = (("this-fam0", this0), ("this-fam2", this2), ("other", parent))
for _, e in engines:
    e.enable_timing(2)

print(f"fused chain (thz_pipeline, all outputs), {nx} x {ny} traces, hipEvents around the launches; 'other' = {other}")
print("roofline fraction: algorithmic bytes of the chain (16 nt + 20 per trace) over 8 TB/s peak HBM")
for nt in lengths:
    tm = synth.make_time(nt)
    for _, e in engines:
        e.set_time_axis(tm)
    a = this0
    nf = a.nf
    chain = synth.default_chain(tm)
    d_t = a.to_device(tm); d_raw = a.empty((npix, nt)); a.synth_cube(d_raw, npix, 0, d_t)
    d_pre = a.to_device(chain["w_pre"]); d_fd = a.to_device(chain["fd_mask"]); d_post = a.to_device(chain["w_post"])
    bufs = [a.empty((npix, nf, 2)), a.empty((npix, nf)), a.empty((npix, nf)), a.empty((npix, nt)), a.empty((npix,))]
    run = lambda e: e.pipeline(npix, d_raw, d_pre, d_fd, d_post, *bufs)
    res, calls = {}, {}
    for name, e in engines:          # warm, and size every measurement to >= 0.3 s of timed work
        for _ in range(3):
            run(e)
        e.sync()
        e.timing_collect(binding.STAGE_PIPELINE)
        for _ in range(5):
            run(e)
        e.sync()
        ns, c = e.timing_collect(binding.STAGE_PIPELINE)
        calls[name] = max(10, int(np.ceil(0.3e9 / (ns / c))))
    for r in range(rounds):
        for name, e in engines:
            for _ in range(calls[name]):
                run(e)
            e.sync()
            ns, c = e.timing_collect(binding.STAGE_PIPELINE)
            res.setdefault(name, []).append(ns / c * 1e-6)
    print(f"nt={nt}: variants {this0.kernel_variant()} | {this2.kernel_variant()} | {parent.kernel_variant()}")
    byts = npix * (16 * nt + 20)
    for name, _ in engines:
        v = np.array(res[name])
        print(f"  {name:9s} calls/meas {calls[name]:4d}  median {np.median(v):7.3f} ms  min {v.min():7.3f}  max {v.max():7.3f}  "
              f"spread {(v.max() - v.min()) / np.median(v) * 100:5.2f} %  frac-of-roofline {byts / np.median(v) / 1e6 / 8000:.4f}")
    m0, mp = np.median(res["this-fam0"]), np.median(res["other"])
    print(f"  other / this-fam0 = {mp / m0:.3f}x   this-fam2 / other = {np.median(res['this-fam2']) / mp:.3f}", flush=True)
    for b in bufs + [d_t, d_raw, d_pre, d_fd, d_post]:
        b.free()
