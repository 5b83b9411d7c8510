"""Optical-property maps on the device (csrc/optical.hip, optical_api.cpp): the kernel on arrays the test
writes itself — no transform in front, so no 2 pi decision of an unwrap can reach a bar — and the session form on a scan
of delayed pulses.

`want` is the fp64 mean, over a band's nb bins, of the CPU oracle's per-bin f32 values (thz_oracle_optical_properties,
called per pixel on fl32(P - w) with that pixel's thickness).  With eps = 2^-23:
- wraps: bit for bit the model's count (the generator keeps every pixel's b / 2 pi at least 1e-3 from a half-integer).
- slope: within 1 ulp of (float) of the model's fp64 slope; not finite where that is not.
- n:     |got - want| <= mean_k 4 eps (1 + |n_k|) + S
- alpha: <= mean_k (2 / |d|) 8 eps (1 + |L_k|) + S, L_k the logarithm: absolute in L because the logarithm's argument is
         rounded before the logarithm's own <= 1 ulp on either side
- kappa: <= mean_k [that bin's alpha bar times C / (4 pi f_hz) + eps |kappa_k|] + S
- S = (ceil(nb / 64) + 8) eps mean_k |v_k| for the f32 summation: a lane adds at most ceil(nb / 64) values, the lanes take
  six more steps, the mean one: each half an ulp of the partial sum.
- where want is not finite, got is not finite.
Derived, not measured; the test prints the largest error / bar of every output."""
import functools
import math

import numpy as np
import pytest

import optical_map_model as model
import oracle_binding as ob
import thz_image_explorer_amd as pkg
from test_gpu_helper_sizes import Dev

pytestmark = pytest.mark.gpu

NX, NY = 17, 19
NPIX = NX * NY              # 323 pixels: odd, no multiple of the four waves of a block, 81 blocks
NFS = [3, 65, 501, 513, 2049]
EPS = model.EPS
PIX_D0, PIX_NAN, PIX_A0 = 0, 1, 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _anchor_for(nf):
    return (1, 3) if nf == 3 else (nf // 8 + 1, nf // 2)


def _bands_for(nf):
    """every band shape the kernel's loops can meet, as far as nf has room: one bin; 63, 64 and 65 bins (a wave's worth
    of bins minus one, exactly, plus one: the lane loop's second trip); all of [1, nf); one that ends at
    nf; two that overlap; one inside the anchor and one apart from it"""
    a0, a1 = _anchor_for(nf)
    cand = [(min(5, nf - 1), min(5, nf - 1) + 1), (2, 65), (1, 65), (3, 68), (1, nf), (nf - min(7, nf - 1), nf),
            (nf // 4, nf // 4 + 40), (nf // 4 + 20, nf // 4 + 70), (a0 + 1, a1 - 1), (a1 + 1, a1 + 30), (1, 2)]
    out = []
    for k0, k1 in cand:
        if 1 <= k0 < k1 <= nf and (k0, k1) not in out:
            out.append((k0, k1))
    return out


def _configs(nf):
    """(anchor on, thickness image, bands): 8 bands and 1, the anchor on and off, a scalar thickness and an image"""
    bands = _bands_for(nf)
    first = [bands[i % len(bands)] for i in range(8)]      # eight bands also where nf has room for fewer shapes
    rest = bands[8:] or [(1, nf)]
    return [(True, False, first), (False, True, first), (True, True, rest), (False, False, [(1, nf)])]


@functools.lru_cache(maxsize=None)
def _inputs(nf):
    x = model.make_inputs(NPIX, nf, _anchor_for(nf), seed=nf)
    a0, a1 = _anchor_for(nf)
    x["d_img"][PIX_D0] = 0.0                              # a pixel without thickness (where the image is used)
    x["P"][PIX_NAN, (a0 + a1) // 2] = np.nan              # a NaN phase inside the anchor and most bands
    x["A"][PIX_A0] = 0.0                                  # zero amplitudes: the 1e-12 floor
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(nf, anchor_on, image):
    """the oracle's per-bin values, once per (nf, anchor, thickness form) and shared by every band and test"""
    x = _inputs(nf)
    a0, a1 = _anchor_for(nf) if anchor_on else (0, 0)
    m, w, s64, _ = model.anchor(x["P"], x["Pr"], a0, a1)
    d = x["d_img"] if image else np.full(NPIX, x["d"], np.float32)
    n, alpha, kappa = (np.empty((NPIX, nf), np.float32) for _ in range(3))
    for p in range(NPIX):
        n[p], alpha[p], kappa[p] = ob.optical_properties(x["A"][p], (x["P"][p] - w[p]).astype(np.float32), x["Ar"], x["Pr"],
                                                         x["f"], float(d[p]))
    mod = model.per_bin(x["A"], x["P"], w, x["Ar"], x["Pr"], x["f"], d)
    with np.errstate(all="ignore"):
        L = np.log(mod["arg"].astype(np.float64))
    return dict(m=m, s64=s64, d=d, n=n, alpha=alpha, kappa=kappa, L=L, f_hz=mod["f_hz"].astype(np.float64))


def _bars(ref, bands):
    """-> {name: (want (n_bands, npix) f64, bar (n_bands, npix) f64)}"""
    out = {}
    d = np.abs(ref["d"].astype(np.float64))[:, None]
    with np.errstate(all="ignore"):
        per_alpha = (2.0 / d) * 8.0 * EPS * (1.0 + np.abs(ref["L"]))
        per = dict(n=4.0 * EPS * (1.0 + np.abs(ref["n"].astype(np.float64))), alpha=per_alpha,
                   kappa=per_alpha * float(model.C_LIGHT) / (4.0 * np.pi * ref["f_hz"])
                   + EPS * np.abs(ref["kappa"].astype(np.float64)))
        for name in ("n", "alpha", "kappa"):
            v = ref[name].astype(np.float64)
            want, bar = [], []
            for k0, k1 in bands:
                nb = k1 - k0
                S = (math.ceil(nb / 64) + 8) * EPS * np.abs(v[:, k0:k1]).mean(axis=1)
                want.append(v[:, k0:k1].mean(axis=1))
                bar.append(per[name][:, k0:k1].mean(axis=1) + S)
            out[name] = (np.stack(want), np.stack(bar))
    return out


def _check_bands(got, want, bar, tag):
    """-> largest error / bar over the entries whose want is finite"""
    fin = np.isfinite(want)
    assert not np.isfinite(got[~fin]).any(), (tag, "finite where the oracle's mean is not")
    assert np.isfinite(bar[fin]).all(), tag
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    bad = err > bar[fin]
    assert not bad.any(), (tag, np.argwhere(fin)[bad][:8], err[bad][:8], bar[fin][bad][:8])
    return float(np.max(err / bar[fin])) if fin.any() else 0.0


def _check_anchor(wraps, slope, ref, anchor_on, tag):
    assert np.array_equal(wraps, ref["m"]), (tag, np.flatnonzero(wraps != ref["m"])[:8])
    if not anchor_on:
        assert not wraps.any() and np.all(slope == 0.0) and not np.signbit(slope).any(), tag
        return 0.0
    fin = np.isfinite(ref["s64"])
    assert not fin[PIX_NAN] and fin.sum() == NPIX - 1 and not np.isfinite(slope[~fin]).any(), tag
    u = model.ulps(slope[fin], ref["s64"][fin].astype(np.float32))
    assert u.max() <= 1, (tag, u.max())
    return float(u.max())


def _run(engine, d, x, nf, cfg, dA, dP, dD, outs=("n", "alpha", "kappa", "wraps", "slope")):
    nb = int(cfg.n_bands)
    bufs = dict(n=d.new(max(nb, 1) * NPIX), alpha=d.new(max(nb, 1) * NPIX), kappa=d.new(max(nb, 1) * NPIX),
                wraps=d.put(np.full(NPIX, -77, np.int32)), slope=d.new(NPIX))
    engine.optical_maps(NPIX, nf, dA, dP, x["Ar"], x["Pr"], x["f"], cfg, dD, **{k: bufs[k] for k in outs})
    res = {k: d.get(bufs[k], nb * NPIX).reshape(nb, NPIX) for k in ("n", "alpha", "kappa")}
    res["wraps"], res["slope"] = d.get(bufs["wraps"], NPIX, np.int32), d.get(bufs["slope"], NPIX)
    return res


@pytest.mark.parametrize("nf", NFS)
def test_optical_maps(engine, nf):
    x = _inputs(nf)
    worst = dict(n=0.0, alpha=0.0, kappa=0.0, slope=0.0)
    with Dev(engine) as d:
        for off in (0, 4):                                 # ... and both arrays 4 bytes behind a 16-byte boundary
            dA, dP, dD = d.put(x["A"], off), d.put(x["P"], off), d.put(x["d_img"], off)
            for anchor_on, image, bands in _configs(nf):
                cfg = pkg.optical_cfg(x["d"], _anchor_for(nf) if anchor_on else None, bands)
                tag = (nf, off, anchor_on, image, bands)
                got = _run(engine, d, x, nf, cfg, dA, dP, dD if image else None)
                ref = _reference(nf, anchor_on, image)
                worst["slope"] = max(worst["slope"], _check_anchor(got["wraps"], got["slope"], ref, anchor_on, tag))
                for name, (want, bar) in _bars(ref, bands).items():
                    worst[name] = max(worst[name], _check_bands(got[name], want, bar, tag + (name,)))
                if image:                                  # the pixel without thickness: nothing finite, nothing trapped
                    assert not np.isfinite(got["n"][:, PIX_D0]).any()
                # the same call again: the same bits
                again = _run(engine, d, x, nf, cfg, dA, dP, dD if image else None)
                for k in got:
                    assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (tag, k)
    print(f"optical_maps nf={nf}: largest error / bar n {worst['n']:.3f}, alpha {worst['alpha']:.3f}, kappa {worst['kappa']:.3f}; "
          f"slope {worst['slope']:.0f} ulp")


def test_null_outputs_are_skipped_and_empty_calls_are_no_ops(engine):
    nf = 65
    x = _inputs(nf)
    bands = _bands_for(nf)[:3]
    cfg = pkg.optical_cfg(x["d"], _anchor_for(nf), bands)
    ref = _reference(nf, True, False)
    bars = _bars(ref, bands)
    with Dev(engine) as d:
        dA, dP = d.put(x["A"]), d.put(x["P"])
        for outs in (("n",), ("alpha", "slope"), ("kappa",), ("wraps",), ()):
            got = _run(engine, d, x, nf, cfg, dA, dP, None, outs)
            for name in ("n", "alpha", "kappa"):
                if name in outs:
                    _check_bands(got[name], *bars[name], (outs, name))
                else:
                    assert np.isnan(got[name]).all(), (outs, name)       # as the test left it
            if "wraps" in outs:
                assert np.array_equal(got["wraps"], ref["m"])
            else:
                assert np.all(got["wraps"] == -77)
            if "slope" in outs:
                _check_anchor(ref["m"], got["slope"], ref, True, outs)
            else:
                assert np.isnan(got["slope"]).all()
        # no pixels: a no-op
        engine.optical_maps(0, nf, dA, dP, x["Ar"], x["Pr"], x["f"], cfg, None, n=d.new(1))
        # no bands: the anchor alone
        got = _run(engine, d, x, nf, pkg.optical_cfg(x["d"], _anchor_for(nf), []), dA, dP, None)
        assert np.array_equal(got["wraps"], ref["m"])


def test_argument_errors_leave_the_outputs_alone(engine):
    nf = 65
    x = _inputs(nf)
    ok_band, ok_anchor = [(1, nf)], _anchor_for(nf)
    bad = [(ok_anchor, [(0, 5)]),                          # bin 0 has omega = 0
           (ok_anchor, [(7, 7)]), (ok_anchor, [(9, 8)]),   # empty, reversed
           (ok_anchor, [(1, nf + 1)]),                     # beyond the row
           (ok_anchor, ok_band + [(3, 9), (nf, nf + 1)]),  # a bad band behind good ones
           (ok_anchor, [(1, 2)] * 9),                      # more than THZ_OPTICAL_MAX_BANDS
           ((5, 6), ok_band),                              # an anchor of one bin
           ((9, 5), ok_band),                              # reversed
           ((nf - 3, nf + 1), ok_band)]                    # beyond the row
    with Dev(engine) as d:
        dA, dP = d.put(x["A"]), d.put(x["P"])
        for anchor, bands in bad:
            cfg = pkg.optical_cfg(x["d"], anchor, bands)
            with pytest.raises(pkg.ThzError) as e:
                _run(engine, d, x, nf, cfg, dA, dP, None)
            assert e.value.code == -1, (anchor, bands)
        # ... and they were checked before anything was launched: outputs as they were
        outs = dict(n=d.new(9 * NPIX), wraps=d.put(np.full(NPIX, -77, np.int32)), slope=d.new(NPIX))
        for anchor, bands in bad:
            with pytest.raises(pkg.ThzError):
                engine.optical_maps(NPIX, nf, dA, dP, x["Ar"], x["Pr"], x["f"], pkg.optical_cfg(x["d"], anchor, bands), None, **outs)
        assert np.isnan(d.get(outs["n"], 9 * NPIX)).all() and np.isnan(d.get(outs["slope"], NPIX)).all()
        assert np.all(d.get(outs["wraps"], NPIX, np.int32) == -77)
        for missing in ("amp", "phase"):
            with pytest.raises(pkg.ThzError) as e:
                engine.optical_maps(NPIX, nf, None if missing == "amp" else dA, None if missing == "phase" else dP, x["Ar"], x["Pr"],
                                    x["f"], pkg.optical_cfg(x["d"], ok_anchor, ok_band), None, **outs)
            assert e.value.code == -1


def test_more_pixels_than_one_grid_pass_and_stage_time(engine):
    """2048 blocks of four waves cover 8192 pixels: the 8300 here take a second trip of the pixel loop"""
    npix, nf = 8300, 33
    a0, a1 = 4, 20
    bands = [(1, nf), (6, 13)]
    x = model.make_inputs(npix, nf, (a0, a1), seed=5)
    m, w, s64, _ = model.anchor(x["P"], x["Pr"], a0, a1)
    mod = model.per_bin(x["A"], x["P"], w, x["Ar"], x["Pr"], x["f"], x["d_img"])
    with Dev(engine) as d:
        dn, dw, ds = d.new(2 * npix), d.put(np.full(npix, -77, np.int32)), d.new(npix)
        engine.enable_timing(1)
        try:
            engine.optical_maps(npix, nf, d.put(x["A"]), d.put(x["P"]), x["Ar"], x["Pr"], x["f"], pkg.optical_cfg(0.0, (a0, a1), bands),
                                d.put(x["d_img"]), n=dn, wraps=dw, slope=ds)
            assert engine.stage_time_ns(pkg.STAGE_OPTICAL) > 0
        finally:
            engine.enable_timing(0)
        n, wraps, slope = d.get(dn, 2 * npix).reshape(2, npix), d.get(dw, npix, np.int32), d.get(ds, npix)
    assert np.array_equal(wraps, m)
    assert model.ulps(slope, s64.astype(np.float32)).max() <= 1
    # n's operations are IEEE ones on both sides: the model's per-bin values are the kernel's, the bar is n's own
    want = model.band_means(mod["n"], bands)
    for b, (k0, k1) in enumerate(bands):
        v = np.abs(mod["n"][:, k0:k1].astype(np.float64))
        bar = (4.0 * EPS * (1.0 + v)).mean(axis=1) + (math.ceil((k1 - k0) / 64) + 8) * EPS * v.mean(axis=1)
        assert np.all(np.abs(n[b] - want[b]) <= bar)


# ---- the session form -------------------------------------------------------------------------------------------
SNX, SNY, SNT = 16, 12, 1001
# What the CPU oracle's default chain (oracle_binding.run_pipeline) plus the model's anchor over the bins of 0.5 - 1.5 THz
# leave of the planted delays on this very cube: at most 0.626 sample (mean 0.169) — the 1 % noise and the chain's
# windows, which meet every delayed pulse at another place.  The device's chain gets twice that.
DELAY_BAR_SAMPLES = 2 * 0.626


def test_session_maps_a_scan_of_delayed_pulses(engine):
    """(see DELAY_BAR_SAMPLES above for the measured CPU figure the delay's bar is twice of)"""
    time, cube, pulse, delay = model.delayed_pulse_cube(SNX, SNY, SNT)
    npix, nf = SNX * SNY, SNT // 2 + 1
    lib = engine.lib
    opt_bufs = (pkg.BUF_OPT_N, pkg.BUF_OPT_ALPHA, pkg.BUF_OPT_KAPPA, pkg.BUF_OPT_WRAPS, pkg.BUF_OPT_SLOPE)
    _, ref_amp, ref_phase = engine.reference_spectrum(time, time, pulse)
    sess = pkg.Session(engine, SNX, SNY, time)
    try:
        sess.upload(cube, subtract_bias=False)
        f = pkg.host_frequency_axis(time)
        k = np.flatnonzero((f >= 0.5) & (f <= 1.5))
        band = (int(k[0]), int(k[-1]) + 1)
        thickness = np.float32(1e-3)
        on, off = pkg.optical_cfg(thickness, band, [band]), pkg.optical_cfg(thickness, None, [band])
        # nothing resident yet: no spectra, no maps
        with pytest.raises(pkg.ThzError) as e:
            sess.optical_maps(ref_amp, ref_phase, on)
        assert e.value.code == -4
        for b in opt_bufs:
            assert not lib.thz_session_buffer(sess.h, b)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(b, npix=npix)
            assert e.value.code == -4
        sess.recompute(pkg.chain_cfg_default(time))
        assert not any(lib.thz_session_buffer(sess.h, b) for b in opt_bufs)      # a recompute alone makes none
        with pytest.raises(pkg.ThzError) as e:                                   # a reference of another length
            sess.optical_maps(ref_amp[:-1], ref_phase[:-1], on)
        assert e.value.code == -1
        with pytest.raises(pkg.ThzError) as e:
            sess.optical_maps(ref_amp, ref_phase, pkg.optical_cfg(thickness, band, [(0, 4)]))
        assert e.value.code == -1
        assert not any(lib.thz_session_buffer(sess.h, b) for b in opt_bufs)

        n_on, alpha_on, kappa_on, wraps, slope = sess.optical_maps(ref_amp, ref_phase, on)
        assert n_on.shape == (1, SNX, SNY) and wraps.dtype == np.int32 and all(lib.thz_session_buffer(sess.h, b) for b in opt_bufs)
        # against the model on the session's own amplitudes and phases, to the kernel test's bars
        A, P = sess.download(pkg.BUF_AMPLITUDES), sess.download(pkg.BUF_PHASES)
        m, w, s64, b64 = model.anchor(P, ref_phase, *band)
        frac = np.abs(b64 / model.TWO_PI - np.floor(b64 / model.TWO_PI) - 0.5)
        assert frac.min() >= 1e-3                                                # the count is not a coin toss on this cube
        assert np.array_equal(wraps.ravel(), m) and np.any(m != 0)
        assert model.ulps(slope.ravel(), s64.astype(np.float32)).max() <= 1
        d = np.full(npix, thickness, np.float32)
        for cfg_w, got in ((w, (n_on, alpha_on, kappa_on)), (np.zeros(npix, np.float32), sess.optical_maps(ref_amp, ref_phase, off)[:3])):
            ref = dict(d=d, m=m, s64=s64)
            ref["n"], ref["alpha"], ref["kappa"] = (np.empty((npix, nf), np.float32) for _ in range(3))
            for p in range(npix):
                ref["n"][p], ref["alpha"][p], ref["kappa"][p] = ob.optical_properties(A[p], (P[p] - cfg_w[p]).astype(np.float32), ref_amp,
                                                                                      ref_phase, f, float(thickness))
            mod = model.per_bin(A, P, cfg_w, ref_amp, ref_phase, f, d)
            with np.errstate(all="ignore"):
                ref["L"], ref["f_hz"] = np.log(mod["arg"].astype(np.float64)), mod["f_hz"].astype(np.float64)
            for (name, (want, bar)), g in zip(_bars(ref, [band]).items(), got):
                r = _check_bands(g.reshape(1, npix), want, bar, name)
                print(f"session {name}: largest error / bar {r:.3f}")
        n_off = sess.optical_maps(ref_amp, ref_phase, off)[0]
        # the planted delays come back from the slope ...
        err = np.abs(model.delay_samples(slope, SNT) - delay)
        print(f"delay from the slope: largest error {err.max():.3f} samples (mean {err.mean():.3f}); wraps {m.min()} ... {m.max()}, "
              f"{(m != 0).sum()} pixels; spread of n {np.ptp(n_on):.3f} anchored, {np.ptp(n_off):.3f} not")
        assert err.max() <= DELAY_BAR_SAMPLES
        # ... and the anchor takes the unwrap's whole turns out of the map
        assert np.ptp(n_on) <= np.ptp(n_off)
        # the band-major maps are read as one flat (band, pixel) array; nothing beyond it
        two = pkg.optical_cfg(thickness, band, [band, (band[0], band[0] + 5)])
        n2 = sess.optical_maps(ref_amp, ref_phase, two)[0]
        assert n2.shape == (2, SNX, SNY) and np.array_equal(_bits(n2[0]), _bits(n_on[0]))
        assert np.array_equal(_bits(sess.download(pkg.BUF_OPT_N, pix0=npix + 3, npix=5)), _bits(n2[1].ravel()[3:8]))
        for which, total in ((pkg.BUF_OPT_N, 2 * npix), (pkg.BUF_OPT_KAPPA, 2 * npix), (pkg.BUF_OPT_WRAPS, npix), (pkg.BUF_OPT_SLOPE, npix)):
            sess.download(which, npix=total)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(which, pix0=1, npix=total)
            assert e.value.code == -1
        # reading the spectra in place has not cost the next recompute its knowledge of their zeros: same maps after it
        sess.recompute(pkg.chain_cfg_default(time))
        assert np.array_equal(_bits(sess.optical_maps(ref_amp, ref_phase, on)[0]), _bits(n_on))
        # a new upload voids the maps
        sess.upload(cube, subtract_bias=False)
        assert not any(lib.thz_session_buffer(sess.h, b) for b in opt_bufs)
        with pytest.raises(pkg.ThzError) as e:
            sess.optical_maps(ref_amp, ref_phase, on)
        assert e.value.code == -4
    finally:
        sess.close()
