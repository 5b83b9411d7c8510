"""The numpy model of the optical-property maps (optical_map_model.py) against the CPU oracle's
calculate_optical_properties, and the guarantees of the input generator the GPU tests rely on.  No GPU."""
import numpy as np
import pytest

import optical_map_model as model
import oracle_binding as ob
import thz_image_explorer_amd as pkg

NPIX = 41


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nf,anchor", [(3, (1, 3)), (65, (9, 33)), (501, (50, 150)), (2049, (0, 0))])
@pytest.mark.parametrize("image", [False, True])
def test_per_bin_values_are_the_oracles(nf, anchor, image):
    """n bit for bit; alpha within 2 ulp (numpy's log against libm's logf, each within an ulp of the true one); kappa's
    own operations bit for bit: the model's formula on the ORACLE's alpha gives the oracle's kappa"""
    x = model.make_inputs(NPIX, nf, anchor, seed=1)
    x["A"][5] = 0.0                                        # zero amplitudes: the 1e-12 floor
    x["P"][7, nf // 2] = np.nan
    m, w, s, b = model.anchor(x["P"], x["Pr"], *anchor)
    if anchor[0] != anchor[1]:
        assert np.any(m != 0)
    d = x["d_img"] if image else x["d"]
    got = model.per_bin(x["A"], x["P"], w, x["Ar"], x["Pr"], x["f"], d)
    worst = 0.0
    for p in range(NPIX):
        dp = float(d[p]) if image else float(d)
        n, alpha, kappa = ob.optical_properties(x["A"][p], (x["P"][p] - w[p]).astype(np.float32), x["Ar"], x["Pr"], x["f"], dp)
        sl = slice(1, None)                                # bin 0 has omega = 0: no band may hold it
        assert np.array_equal(_bits(got["n"][p, sl]), _bits(n[sl])), p
        u = model.ulps(got["alpha"][p, sl], alpha[sl])
        worst = max(worst, u.max())
        assert u.max() <= 2, (p, u.max())
        assert np.array_equal(_bits(model.kappa_of(alpha[sl], x["f"][sl])), _bits(kappa[sl])), p
        # ... and the library's host loop, which the maps replace, is the oracle's too
        hn, ha, hk = pkg.host_optical_properties(x["A"][p], (x["P"][p] - w[p]).astype(np.float32), x["Ar"], x["Pr"], x["f"], dp)
        assert np.array_equal(_bits(hn[sl]), _bits(n[sl]))
        assert model.ulps(ha[sl], alpha[sl]).max() <= 2
    print(f"nf={nf}: alpha model vs oracle, largest distance {worst:.0f} ulp")


@pytest.mark.parametrize("nf,anchor", [(3, (1, 3)), (65, (1, 3)), (65, (30, 65)), (501, (100, 300)), (2049, (200, 1100))])
def test_anchor_finds_the_planted_multiple(nf, anchor):
    """2 pi m + s k + noise gives back m, the slope s and — with the anchor off — nothing"""
    x = model.make_inputs(323, nf, anchor, seed=2)         # asserts the guarantees (finite b, 1e-3 off a half-integer)
    m, w, s, b = model.anchor(x["P"], x["Pr"], *anchor)
    assert np.array_equal(m, x["m"]) and m.min() == -3 and m.max() == 3
    assert np.array_equal(_bits(w), _bits((m.astype(np.float64) * model.TWO_PI).astype(np.float32)))
    assert np.all((s > 0.0) & (s < 0.4)) if anchor[1] - anchor[0] > 20 else True
    # taken off, the phases' lag is that of a pixel that never wrapped: n comes out the same whatever m was
    got = model.per_bin(x["A"], x["P"], w, x["Ar"], x["Pr"], x["f"], x["d"])["n"]
    flat = model.per_bin(x["A"], (x["P"].astype(np.float64) - model.TWO_PI * x["m"][:, None]).astype(np.float32), np.zeros(323, np.float32),
                         x["Ar"], x["Pr"], x["f"], x["d"])["n"]
    k = slice(max(1, nf // 2), nf)
    assert np.allclose(got[:, k], flat[:, k], rtol=0, atol=2e-3 * np.abs(flat[:, k]).max())
    m0, w0, s0, b0 = model.anchor(x["P"], x["Pr"], 5, 5)
    assert not m0.any() and not w0.any() and not np.signbit(w0).any() and not s0.any()


def test_anchor_corner_cases():
    x = model.make_inputs(8, 65, (8, 40), seed=3)
    P = x["P"].copy()
    P[1, 20] = np.nan
    P[2, 39] = np.inf
    P[3, 7] = np.nan                                       # outside the anchor: no effect on it
    m, w, s, b = model.anchor(P, x["Pr"], 8, 40)
    assert m[1] == 0 and w[1] == 0 and np.isnan(s[1])
    assert m[2] == 0 and w[2] == 0 and not np.isfinite(s[2])
    assert m[3] == x["m"][3]
    assert np.array_equal(m[4:], x["m"][4:])


def test_delay_from_slope():
    nt = 1001
    k = np.arange(nt // 2 + 1)
    for D in (-37, 4, 40):
        P = (-model.TWO_PI * k * D / nt).astype(np.float32)[None, :]
        m, w, s, b = model.anchor(P, np.zeros(k.size, np.float32), 10, 30)
        assert abs(model.delay_samples(s, nt)[0] - D) < 1e-4 and m[0] == 0
