"""Developer tool: thz_pipeline_ex at the PH lengths (2002 / 2400 / 3000 / 4000; plain, cmask, sums, cmask + sums) from TWO
builds of the library in one process on the same device buffers, as scripts/gpu_ab_builds.py — the other build takes two
slots of the rotation (other, this, other again), so its two medians show the run-to-run spread.  Per call: the hipEvent
time of STAGE_PIPELINE + STAGE_MEAN, i.e. what the call costs with its sums passes.
Usage: scripts/gpu_ph_ab_builds.py <other libthzgpu.so> [output file]; THZ_AB_ROUNDS (8)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from thz_image_explorer_amd import binding, Engine
import synth

other = sys.argv[1]
rounds = int(os.environ.get("THZ_AB_ROUNDS", "8"))
nx = ny = 256
a = Engine(0)
lib_b = C.CDLL(other)
for name, res, args in binding.SYMBOLS:
    if hasattr(lib_b, name):
        fn = getattr(lib_b, name); fn.restype = res; fn.argtypes = args
b = Engine.__new__(Engine)
b.lib, b.ctx, b._bufs = lib_b, binding._P(), []
assert lib_b.thz_create(0, C.byref(b.ctx)) == 0
npix = nx * ny
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n"); out.flush()
say(f"{nx} x {ny} traces, ms per thz_pipeline_ex call (STAGE_PIPELINE + STAGE_MEAN hipEvent time), median of {rounds} rounds of 3 calls")
say("rotation per round: other, this, other again (the other build twice: the run-to-run spread)")
for nt in (2002, 2400, 3000, 4000):
    tm = synth.make_time(nt)
    for e in (a, b):
        e.set_time_axis(tm)
    nf = a.nf
    chain = synth.default_chain(tm)
    d_t = a.to_device(tm); d_raw = a.empty((npix, nt)); a.synth_cube(d_raw, npix, 0, d_t)
    d_pre = a.to_device(chain["w_pre"]); d_fd = a.to_device(chain["fd_mask"]); d_post = a.to_device(chain["w_post"])
    d_fft = a.empty((npix, nf, 2)); d_amp = a.empty((npix, nf)); d_ph = a.empty((npix, nf)); d_out = a.empty((npix, nt)); d_img = a.empty((npix,))
    d_sums = a.empty((2 * nf,))
    H = np.zeros((nf, 2), np.float32); H[:, 0] = 0.7; H[:, 1] = 0.3
    d_H = a.to_device(H)
    variants = {
        "plain": lambda e: e.pipeline_ex(npix, d_raw, d_pre, d_fd, None, d_post, d_fft, d_amp, d_ph, d_out, d_img, None),
        "cmask": lambda e: e.pipeline_ex(npix, d_raw, d_pre, d_fd, d_H, d_post, d_fft, d_amp, d_ph, d_out, d_img, None),
        "sums": lambda e: e.pipeline_ex(npix, d_raw, d_pre, d_fd, None, d_post, d_fft, d_amp, d_ph, d_out, d_img, d_sums),
        "cmask+sums": lambda e: e.pipeline_ex(npix, d_raw, d_pre, d_fd, d_H, d_post, d_fft, d_amp, d_ph, d_out, d_img, d_sums),
    }
    res = {}
    for e in (a, b):
        e.enable_timing(2)
        for st in range(12):
            e.timing_collect(st)
    for r in range(rounds + 1):
        for vname, fn in variants.items():
            for name, e in (("other-A", b), ("this", a), ("other-B", b)):
                for _ in range(3):
                    fn(e)
                e.sync()
                ns, calls = e.timing_collect(binding.STAGE_PIPELINE)
                ns2, calls2 = e.timing_collect(binding.STAGE_MEAN)
                if r:
                    res.setdefault((vname, name), []).append((ns + ns2) / calls * 1e-6)
                    res[(vname, name, "launches")] = (calls + calls2) / calls
    for e in (a, b):
        e.enable_timing(0)
    say(f"nt = {nt} ({a.kernel_variant()})")
    for vname in variants:
        m = {n: float(np.median(res[(vname, n)])) for n in ("other-A", "this", "other-B")}
        spread = abs(m["other-A"] - m["other-B"])
        say(f"  {vname:11s} other {m['other-A']:.4f} / {m['other-B']:.4f} ms (spread {spread:.4f})   this {m['this']:.4f} ms   "
            f"this / other {m['this'] / min(m['other-A'], m['other-B']):.3f}   timed stages per call: other {res[(vname, 'other-A', 'launches')]:.0f}, this {res[(vname, 'this', 'launches')]:.0f}")
    for d in (d_t, d_raw, d_pre, d_fd, d_post, d_fft, d_amp, d_ph, d_out, d_img, d_sums, d_H):
        d.free()
if out:
    out.close()
