"""Developer tool: one whole thz_session_recompute of a TILTED 1001-sample scan, timed on the host clock (the call ends
in a stream synchronise) from TWO builds of the library in one process, alternating — this build (one launch from the
raw cube: thz_pipeline_tilted, fft_fbp.hpp TILT / CM / SUMS) and another build (the parent commit: tilt pass into an
extended cube, stream wait, fused launch, second passes for a complex multiplier and the means).  Two tilts, one per
convolution length (M = 2304 / 2560), four settings each: plain chain, want_means = 1, Wiener multiplier, both.  Every
measurement is `calls` recomputes (>= 0.3 s of timed work); `rounds` repeats give the run-to-run spread.  Also the bare
launch (STAGE_PIPELINE, hipEvents) of the plain chain at both lengths: the un-tilted, un-multiplied kernel must not move.
Usage: scripts/gpu_tilted_session_timing.py <other libthzgpu.so> [nx ny]
       scripts/gpu_tilted_session_timing.py --one      (one tilted recompute with multiplier and means: for a kernel trace)"""
import ctypes as C, os, sys, time as clock
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import thz_image_explorer_amd as pkg
from thz_image_explorer_amd import binding, Engine
import synth

NT, D = 1001, 0.1
TILTS = (((1.0, 0.5), 44, 1089), ((2.0, 1.0), 89, 1179))   # dx = dy = 0.1 mm, 512 x 512: steps, nt_out


def wiener(time, nf):
    z = ((time - time[0] - 11.0) / 0.35).astype(np.float64)
    R = np.fft.rfft(-z * np.exp(-z * z) * pkg.host_fft_window(time, 0, 1.0, 7.0).astype(np.float64))
    H = np.conj(R) / (np.abs(R) ** 2 + 1e-2 * (np.abs(R) ** 2).max())
    return np.ascontiguousarray(np.stack([H.real, H.imag], -1), np.float32)


def other_engine(path):
    lib = C.CDLL(path)
    for name, res, args in binding.SYMBOLS:
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    e = Engine.__new__(Engine)
    e.lib, e.ctx, e._bufs = lib, binding._P(), []
    assert lib.thz_create(0, C.byref(e.ctx)) == 0
    return e


def fill(sess, e, npix, time):
    d_t = e.to_device(time)
    e.synth_cube(e.lib.thz_session_buffer(sess.h, pkg.BUF_RAW), npix, 0, d_t)
    d_t.free()
    sess.upload(None, subtract_bias=False)


if sys.argv[1:2] == ["--one"]:
    nx = ny = 512
    time = synth.make_time(NT)
    e = Engine(0)
    s = pkg.Session(e, nx, ny, time, D, D)
    fill(s, e, nx * ny, time)
    cfg = pkg.chain_cfg_default(time)
    cfg.tilt_x_deg, cfg.tilt_y_deg = TILTS[0][0]
    nto = NT + 2 * TILTS[0][1]
    s.set_fd_filters(None, wiener(synth.make_time(nto), nto // 2 + 1))
    s.recompute(cfg)
    print("one tilted recompute, multiplier + means:", e.kernel_variant(), s.nt_out)
    s.close()
    sys.exit(0)

other = sys.argv[1]
nx, ny = (int(a) for a in sys.argv[2:4]) if len(sys.argv) > 3 else (512, 512)
rounds = int(os.environ.get("THZ_AB_ROUNDS", "5"))
npix = nx * ny
time = synth.make_time(NT)
engines = (("this", Engine(0)), ("other", other_engine(other)))
sessions = {}
for name, e in engines:
    sessions[name] = pkg.Session(e, nx, ny, time, D, D)
    fill(sessions[name], e, npix, time)

print(f"thz_session_recompute of a tilted {nx} x {ny} x {NT} scan (dx = dy = {D} mm), host clock around the call; 'other' = {other}")
print("roofline fraction: algorithmic bytes of the step (4 nt_in + 16 nf + 4 nt_out + 4 per trace) over 8 TB/s peak HBM;")
print("the FBP kernels are LDS-bound (profiles/tilted_lengths_timing.txt), so the gain in time is smaller than the gain in bytes")
spreads = []
for tilt, steps, nto in TILTS:
    got = int(pkg.host_tilt_plan(time, nx, ny, tilt[0], tilt[1], D, D)[0])
    assert got == steps, (tilt, got)
    nf = nto // 2 + 1
    H = wiener(synth.make_time(nto), nf)
    for means, mult in ((0, False), (1, False), (0, True), (1, True)):
        cfg = pkg.chain_cfg_default(time)
        cfg.tilt_x_deg, cfg.tilt_y_deg = tilt
        cfg.want_means = means
        res, calls = {}, {}
        for name, e in engines:
            s = sessions[name]
            s.set_fd_filters(None, H if mult else None)
            for _ in range(3):
                s.recompute(cfg)
            t0 = clock.perf_counter()
            for _ in range(5):
                s.recompute(cfg)
            calls[name] = max(10, int(np.ceil(0.3 / ((clock.perf_counter() - t0) / 5))))
            assert s.nt_out == nto and e.kernel_variant().startswith("fbp-")
        for r in range(rounds):
            for name, e in engines:
                s = sessions[name]
                s.set_fd_filters(None, H if mult else None)
                s.recompute(cfg)
                t0 = clock.perf_counter()
                for _ in range(calls[name]):
                    s.recompute(cfg)
                res.setdefault(name, []).append((clock.perf_counter() - t0) / calls[name] * 1e3)
        byts = npix * (4 * NT + 16 * nf + 4 * nto + 4)
        print(f"tilt {tilt} -> nt_out {nto}, want_means {means}, multiplier {'yes' if mult else 'no '}")
        for name, _ in engines:
            v = np.array(res[name])
            sp = (v.max() - v.min()) / np.median(v) * 100
            spreads.append(sp)
            print(f"  {name:6s} calls/meas {calls[name]:4d}  median {np.median(v):7.3f} ms  min {v.min():7.3f}  max {v.max():7.3f}  "
                  f"spread {sp:5.2f} %  frac-of-roofline {byts / np.median(v) / 1e6 / 8000:.4f}")
        mt, mo = np.median(res["this"]), np.median(res["other"])
        margin = 3 * max((np.max(res[n]) - np.min(res[n])) / np.median(res[n]) for n in res) * 100
        print(f"  other / this = {mo / mt:.3f}x  (this is {(1 - mt / mo) * 100:+.2f} % faster; margin 3 x spread = {margin:.2f} %)", flush=True)

# the bare launch of the plain chain: thz_pipeline on an extended cube, hipEvents
print("bare launch (STAGE_PIPELINE) of the plain un-tilted chain, hipEvents:")
for name, e in engines:
    sessions[name].close()
    e.enable_timing(2)
for _, _, nto in TILTS:
    tm = synth.make_time(nto)
    for _, e in engines:
        e.set_time_axis(tm)
    a = engines[0][1]
    nf = a.nf
    chain = synth.default_chain(tm)
    d_t = a.to_device(tm); d_raw = a.empty((npix, nto)); a.synth_cube(d_raw, npix, 0, d_t)
    d_pre = a.to_device(chain["w_pre"]); d_fd = a.to_device(chain["fd_mask"]); d_post = a.to_device(chain["w_post"])
    bufs = [a.empty((npix, nf, 2)), a.empty((npix, nf)), a.empty((npix, nf)), a.empty((npix, nto)), a.empty((npix,))]
    run = lambda e: e.pipeline(npix, d_raw, d_pre, d_fd, d_post, *bufs)
    res, calls = {}, {}
    for name, e in engines:
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
    for name, _ in engines:
        v = np.array(res[name])
        print(f"  nt={nto} {name:6s} calls/meas {calls[name]:4d}  median {np.median(v):7.3f} ms  min {v.min():7.3f}  max {v.max():7.3f}  "
              f"spread {(v.max() - v.min()) / np.median(v) * 100:5.2f} %")
    print(f"  nt={nto} this / other = {np.median(res['this']) / np.median(res['other']):.4f}", flush=True)
    for b in bufs + [d_t, d_raw, d_pre, d_fd, d_post]:
        b.free()
