"""Developer tool: are the fused nt = 4096 chain's outputs the same BITS in two builds of the library?  Loads another
libthzgpu.so beside the package's own (as gpu_ab_builds.py / gpu_ab_sessions.py do), runs both on the same 19 traces —
one block's rounds of 8, 8 and 3, among them a NaN trace, an Inf trace, an all-zero trace and one with negative zeros —
and compares spectrum, amplitudes, phases, traces, image and sums as 32-bit words:
  thz_pipeline_ex   real / complex multiplier  x  with / without sums  x  the default band / a band from bin 0
  a session         the same, first recompute (writes everything) and the two after it (keep range, pruned build)
Usage: scripts/gpu_ab_bits.py <other libthzgpu.so>; exit status 1 if any word differs."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import thz_image_explorer_amd as pkg
from thz_image_explorer_amd import binding, Engine
import synth

other = sys.argv[1]
NX, NY, NT = 19, 1, 4096
NPIX, NF = NX * NY, NT // 2 + 1
a = Engine(0)
lib_b = C.CDLL(other)
for name, res, args in binding.SYMBOLS:
    if hasattr(lib_b, name):
        fn = getattr(lib_b, name); fn.restype = res; fn.argtypes = args
b = Engine.__new__(Engine)
b.lib, b.ctx, b._bufs = lib_b, binding._P(), []
assert lib_b.thz_create(0, C.byref(b.ctx)) == 0
time, cube = synth.make_cube(NX, NY, NT)
cube = cube.copy()
flat = cube.reshape(NPIX, NT)
flat[3] = 0.0
flat[9, ::7] = -0.0
flat[5, NT // 3] = np.nan
flat[17, 11] = np.inf
chain = synth.default_chain(time)
H = np.empty((NF, 2), np.float32)
H[:, 0] = 0.7 + 0.2 * np.cos(np.arange(NF) * 0.01)
H[:, 1] = 0.3 * np.sin(np.arange(NF) * 0.02)
low = np.zeros(NF, np.float32)
k = np.arange(700)
low[k] = (0.6 + 0.4 * np.cos(k * 0.013)).astype(np.float32)
nz = np.nonzero(chain["fd_mask"])[0]
MASKS = {"default band": (np.ascontiguousarray(chain["fd_mask"], np.float32), (int(nz[0]), int(nz[-1]) + 1)), "band from bin 0": (low, (0, 700))}
bad = 0


def report(what, x, y):
    global bad
    n = 0
    for key in x:
        u, v = np.ascontiguousarray(x[key]).view(np.uint32), np.ascontiguousarray(y[key]).view(np.uint32)
        d = int((u != v).sum())
        if d:
            fu, fv = u.view(np.float32), v.view(np.float32)
            nan_only = bool(np.all(np.isnan(fu[u != v]) & np.isnan(fv[u != v])))
            print(f"{what}: {key}: {d} of {u.size} words differ" + (" (NaNs of another sign or payload on both sides)" if nan_only else ""), flush=True)
        n += d
    bad += n
    if not n:
        print(f"{what}: same bits ({', '.join(x)})", flush=True)


def pipeline(e, mask, band, cm, sums):
    e.set_time_axis(time)
    bufs = [e.to_device(cube), e.to_device(chain["w_pre"]), e.to_device(mask), e.to_device(H) if cm else None, e.to_device(chain["w_post"]),
            e.empty((NPIX, NF, 2)), e.empty((NPIX, NF)), e.empty((NPIX, NF)), e.empty((NPIX, NT)), e.empty((NPIX,)),
            e.empty((2 * NF,)) if sums else None]
    e.pipeline_ex(NPIX, *bufs, band=band)
    out = dict(fft=bufs[5].download((NPIX, NF, 2), np.float32), amp=bufs[6].download((NPIX, NF), np.float32),
               ph=bufs[7].download((NPIX, NF), np.float32), data=bufs[8].download((NPIX, NT), np.float32),
               img=bufs[9].download((NPIX,), np.float32))
    if sums:
        out["sums"] = bufs[10].download((2 * NF,), np.float32)
    for x in bufs:
        if x is not None:
            x.free()
    return out


def session(e, lo, cm, means):
    e.set_time_axis(time)
    s = pkg.Session(e, NX, NY, time)
    outs = []
    try:
        s.upload(cube, subtract_bias=False)
        if cm:
            s.set_fd_filters(None, H)
        cfg = pkg.chain_cfg_default(time)
        cfg.want_means = means
        cfg.fd_low = lo
        for _ in range(3):
            s.recompute(cfg)
            o = dict(fft=s.download(pkg.BUF_FFT), amp=s.download(pkg.BUF_AMPLITUDES), ph=s.download(pkg.BUF_PHASES),
                     data=s.download(pkg.BUF_DATA), img=s.download(pkg.BUF_IMG))
            if means:
                o.update(avg_fft=s.download(pkg.BUF_AVG_FFT), avg_amp=s.download(pkg.BUF_AVG_AMPLITUDES), avg_ph=s.download(pkg.BUF_AVG_PHASES))
            outs.append(o)
    finally:
        s.close()
    return outs


for mname, (mask, band) in MASKS.items():
    for cm in (False, True):
        for sums in (False, True):
            for with_band in (False, True):
                what = f"pipeline_ex, {mname}{', band given' if with_band else ''}, {'complex' if cm else 'real'} multiplier{', sums' if sums else ''}"
                report(what, pipeline(a, mask, band if with_band else None, cm, sums), pipeline(b, mask, band if with_band else None, cm, sums))
for lo, lname in ((0.2, "default band"), (0.0, "band from bin 0")):
    for cm in (False, True):
        for means in (0, 1):
            x, y = session(a, lo, cm, means), session(b, lo, cm, means)
            for i, step in enumerate(("first recompute", "second (keep range)", "third")):
                report(f"session, {lname}, {'complex' if cm else 'real'} multiplier{', means' if means else ''}, {step}", x[i], y[i])
print("ALL THE SAME BITS" if not bad else f"{bad} WORDS DIFFER", flush=True)
sys.exit(1 if bad else 0)
