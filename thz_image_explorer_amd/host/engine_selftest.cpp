// engine_selftest.cpp — drives the record-and-flush engine (thz_engine.hpp) through the patched stage walk the way
// the reference's data thread would: filters switched off and on again, one slider per chain position, the
// build-defined Frequency plugins, regions of interest, a scaled chain, and the Deconvolution stage on a group of
// two slabs.  Every scenario dumps the engine's results; tests/test_gpu_engine.py compares them with the oracle
// walking the same chain.  Checks that need no oracle (deferred show_data, group == single) are made here.
//
// usage: engine_selftest <dir>   (dir/cube.bin, dir/psf.bin as written by the test; outputs dir/<scenario>.bin)
#include "thz_engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <cstring>
#include <vector>

using namespace thzhost;

static int g_fail = 0;
#define CHECK(cond, msg)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

struct Cube {
    int nx = 0, ny = 0, nt = 0;
    float dx = 1.0f, dy = 1.0f;
    std::vector<float> time, raw;
};

static Cube read_cube(const std::string &path)
{
    Cube c;
    std::ifstream f(path, std::ios::binary);
    int32_t dims[3] = {0, 0, 0};
    float d[2] = {1.0f, 1.0f};
    f.read(reinterpret_cast<char *>(dims), sizeof dims);
    f.read(reinterpret_cast<char *>(d), sizeof d);
    c.nx = dims[0]; c.ny = dims[1]; c.nt = dims[2]; c.dx = d[0]; c.dy = d[1];
    c.time.resize((size_t)c.nt);
    c.raw.resize((size_t)c.nx * c.ny * c.nt);
    f.read(reinterpret_cast<char *>(c.time.data()), (std::streamsize)(c.time.size() * sizeof(float)));
    f.read(reinterpret_cast<char *>(c.raw.data()), (std::streamsize)(c.raw.size() * sizeof(float)));
    return c;
}

static PsfArrays read_psf(const std::string &path)
{
    PsfArrays p;
    std::ifstream f(path, std::ios::binary);
    float base[4];
    f.read(reinterpret_cast<char *>(base), sizeof base);
    p.wx_a = base[0]; p.wx_b = base[1]; p.wy_a = base[2]; p.wy_b = base[3];
    for (int s = 0; s < 4; ++s)
        for (std::vector<float> *v : {&p.k[s], &p.v[s], &p.a[s], &p.b[s], &p.c[s], &p.d[s]}) {
            int32_t n = 0;
            f.read(reinterpret_cast<char *>(&n), sizeof n);
            v->resize((size_t)n);
            f.read(reinterpret_cast<char *>(v->data()), (std::streamsize)((size_t)n * sizeof(float)));
        }
    return p;
}

// [int32 nt_out, gx, gy, n_rois] [final cube gx*gy*nt_out] [img as the last container holds it] [avg amplitudes nf]
// per region with a polygon, in map order: [roi_signal_fft nf | roi_phase_fft nf | roi_data nt_out]
static void dump(GpuPipeline &p, const std::string &path)
{
    std::vector<float> cube;
    CHECK(p.eng.download_final(cube), "download_final");
    const ScannedImageFilterData &last = p.filter_data.back();
    const int32_t nto = (int32_t)p.eng.nt_out();
    const int32_t gx = (int32_t)last.width, gy = (int32_t)last.height;
    int32_t nroi = 0;
    for (auto &kv : last.roi_signal_fft) { (void)kv; ++nroi; }
    std::ofstream f(path, std::ios::binary);
    const int32_t head[4] = {nto, gx, gy, nroi};
    f.write(reinterpret_cast<const char *>(head), sizeof head);
    auto put = [&](const std::vector<float> &v) { f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(float))); };
    CHECK(cube.size() == (size_t)gx * gy * nto, "final cube size");
    put(cube);
    put(last.img.download());
    put(last.avg_signal_fft);
    for (auto &kv : last.roi_signal_fft) {
        put(kv.second.second);
        put(last.roi_phase_fft.at(kv.first).second);
        put(last.roi_data.at(kv.first).second);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::printf("usage: engine_selftest <dir>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const Cube c = read_cube(dir + "/cube.bin");
    GpuEngine eng({0});
    if (!eng.available()) {
        std::printf("FAIL: no GPU engine\n");
        return 1;
    }
    GpuPipeline p(eng);
    p.gui_settings.psf = read_psf(dir + "/psf.bin");
    p.open(c.raw.data(), (size_t)c.nx, (size_t)c.ny, c.time, c.dx, c.dy);
    p.filter_data[0].pixel_selected = {3, 2};
    const size_t i_tilt = p.index_of("Tilt Compensation"), i_tdb = p.index_of("Band-Pass Filter in Time Domain before the FFT."),
                 i_fd = p.index_of("Frequency Band Pass"), i_water = p.index_of("Water Line Notch"),
                 i_wiener = p.index_of("Reference Wiener Filter"), i_tda = p.index_of("Band-Pass Filter in Time Domain after the FFT."),
                 i_dec = p.index_of("Deconvolution");
    CHECK(i_tilt == 2 && i_tdb == 3 && p.filter_chain[4] == "fft" && i_fd == 5 && i_water == 6 && i_wiener == 7
              && p.filter_chain[8] == "ifft" && i_tda == 9 && i_dec == 10,
          "chain order: initial, scaling, Tilt, Time Band Pass, fft, Frequency plugins, ifft, Time Band Pass, Deconvolution");
    auto active = [&](size_t idx, bool on) { p.filters_active[p.filter_chain[idx]] = on; };

    // ---- 1: OpenFile -> Filter(1), defaults
    p.update_filter(1);
    dump(p, dir + "/default.bin");
    CHECK(eng.dirty_from() > 8, "flush leaves nothing pending");

    // ---- 2: each plugin switched off in turn (UpdateFilter(uuid) -> Filter(idx of the filter), data_thread.rs:907-921);
    //         the reference does not call filter() for an inactive plugin (:1185-1188)
    active(i_fd, false);
    p.update_filter(i_fd);
    CHECK(eng.pending().fd_active == 0, "an inactive Frequency Band Pass is off in the chain");
    dump(p, dir + "/fd_off.bin");
    active(i_fd, true);
    active(i_tdb, false);
    p.update_filter(i_tdb);
    CHECK(eng.pending().fd_active == 1 && eng.pending().td_before_active == 0, "fd on again, Time Band Pass off");
    dump(p, dir + "/tdb_off.bin");
    active(i_tdb, true);
    active(i_tda, false);
    p.update_filter(i_tdb);
    dump(p, dir + "/tda_off.bin");
    active(i_tda, true);
    active(i_tilt, false);
    p.update_filter(i_tilt);
    CHECK(eng.pending().tilt_active == 0 && eng.pending().td_after_active == 1, "tilt off, the others on");
    dump(p, dir + "/tilt_off.bin");
    active(i_tilt, true);
    p.update_filter(1);

    // ---- 3: one slider per chain position, the walk starting where the reference starts it
    auto *fd = dynamic_cast<FrequencyDomainBandPass *>(p.filter_by("Frequency Band Pass"));
    const std::vector<float> fd_plot_before = fd->signal_axis;
    fd->low = 0.4; fd->high = 2.5;
    p.update_filter(i_fd);
    {   // show_data ran AFTER the flush: the filter's plot is the selected pixel's band-passed spectrum of THIS walk
        std::vector<float> amp(eng.nt_out() / 2 + 1);
        thz_plot_out po{};
        po.filtered_signal_fft = amp.data();
        CHECK(eng.plot(3, 2, po), "plot");
        CHECK(fd->signal_axis == amp, "deferred show_data: the Frequency Band Pass plot shows the current results");
        CHECK(fd->signal_axis != fd_plot_before, "... and not the previous walk's");
        size_t zeros = 0;
        for (float v : amp) zeros += v == 0.0f;
        CHECK(zeros > amp.size() / 2, "0.4 - 2.5 THz leaves most bins exactly zero");
    }
    auto *tda = dynamic_cast<TimeDomainBandPassBeforeFFT *>(p.filter_by("Band-Pass Filter in Time Domain after the FFT."));
    tda->high = (double)c.time.back() - 4.0;
    p.update_filter(i_tda);   // chain position 7: only C2R + taper + image are re-run
    p.config.fft_window = {0.5f, 3.0f};
    p.update_filter(p.fft_index);   // SetFFTWindow*: Filter(fft_index), data_thread.rs:813-836
    dump(p, dir + "/sliders.bin");

    // ---- 4: the build-defined Frequency plugins: on, then off again (an inactive plugin must not linger)
    auto *water = dynamic_cast<WaterLineNotch *>(p.filter_by("Water Line Notch"));
    {
        std::ifstream lf(dir + "/water_lines.bin", std::ios::binary);
        int32_t n = 0;
        lf.read(reinterpret_cast<char *>(&n), sizeof n);
        water->lines_thz.resize((size_t)n);
        lf.read(reinterpret_cast<char *>(water->lines_thz.data()), (std::streamsize)((size_t)n * sizeof(float)));
        water->sigma_thz = 0.02f;
    }
    active(i_water, true);
    p.update_filter(i_water);
    dump(p, dir + "/water_on.bin");
    active(i_water, false);
    p.update_filter(i_water);
    dump(p, dir + "/water_off.bin");   // == sliders.bin

    // ---- 5: regions of interest + avg_in_fourier_space through the ifft stage
    p.filter_data[0].rois["roi-a"] = {"ROI 1", Polygon{{1, 1}, {5, 1}, {6, 4}, {3, 6}, {1, 4}}};
    p.filter_data[0].rois["roi-b"] = {"ROI 2", Polygon{{8, 2}, {14, 3}, {12, 12}}};
    p.filter_data[0].rois["roi-none"] = {"no polygon yet", std::nullopt};
    p.update_filter(1);
    dump(p, dir + "/rois.bin");
    p.config.avg_in_fourier_space = true;
    p.update_filter(p.fft_index);   // SetAvgInFourierSpace: Filter(fft_index)
    dump(p, dir + "/rois_fourier.bin");
    CHECK(p.filter_data.back().avg_data.size() == eng.nt_out(), "avg_data of the ifft stage");
    p.config.avg_in_fourier_space = false;

    // ---- 6: scaling (SetDownScaling -> Filter(1)); the image is expanded to the raw grid like data_thread.rs:1243-1285
    p.config.scale_factor = 2;
    p.update_filter(1);
    dump(p, dir + "/scaled.bin");
    CHECK(p.filter_data.back().img.size() == (size_t)(c.nx / 2 * 2) * (size_t)(c.ny / 2 * 2), "scaled image expanded s x s");
    p.config.scale_factor = 1;
    p.update_filter(1);

    // ---- 7: the Deconvolution stage, on one slab and on a group of two: the stage must see the WHOLE image
    auto small_bank = [](Filter *f) {   // a bank whose widest band PSF fits a 36 x 32 image (deconvolution.rs:873-885)
        auto *d = dynamic_cast<Deconvolution *>(f);
        d->n_iterations = 20; d->n_filters = 5; d->start_freq = 0.4f; d->end_freq = 3.0f; d->win_width = 0.5f;
    };
    small_bank(p.filter_by("Deconvolution"));
    active(i_dec, true);
    p.update_filter(i_dec);
    std::vector<float> dec_single;
    CHECK(eng.download_final(dec_single), "download_final");
    dump(p, dir + "/deconv_single.bin");
    {
        GpuEngine eng2({0, 0});
        CHECK(eng2.available(), "two slabs on device 0");
        GpuPipeline q(eng2);
        q.gui_settings.psf = p.gui_settings.psf;
        q.open(c.raw.data(), (size_t)c.nx, (size_t)c.ny, c.time, c.dx, c.dy);
        q.filter_data[0].pixel_selected = {3, 2};
        q.filter_data[0].rois = p.filter_data[0].rois;
        // the arrival plane of the raw cube: two slabs give one session's fit bit for bit, and the plugin's
        // "Estimate" action writes exactly those angles into its fields
        thz_tilt_fit fit1{}, fit2{};
        const int rc1 = eng.estimate_tilt(THZ_BUF_RAW, 1, 0.25f, fit1), rc2 = eng2.estimate_tilt(THZ_BUF_RAW, 1, 0.25f, fit2);
        std::printf("estimate_tilt: %d / %d, %.6f / %.6f degrees over %llu pixels, rms %.4f ps\n", rc1, rc2, fit1.tilt_x_deg, fit1.tilt_y_deg,
                    (unsigned long long)fit1.n_used, fit1.rms_ps);
        CHECK(rc1 == THZ_OK && rc2 == THZ_OK && fit1.n_used > 0, "estimate_tilt on one slab and on two");
        CHECK(std::memcmp(&fit1, &fit2, sizeof fit1) == 0, "estimate_tilt over two slabs == over one");
        GpuTiltCompensation tilt_plugin;
        CHECK(tilt_plugin.estimate(eng2) && tilt_plugin.tilt_x == fit1.tilt_x_deg && tilt_plugin.tilt_y == fit1.tilt_y_deg,
              "the Tilt plugin's Estimate action writes the fitted angles");
        *dynamic_cast<FrequencyDomainBandPass *>(q.filter_by("Frequency Band Pass")) = *fd;
        dynamic_cast<TimeDomainBandPassBeforeFFT *>(q.filter_by("Band-Pass Filter in Time Domain after the FFT."))->high = tda->high;
        q.config = p.config;
        q.update_filter(1);
        // (reset() put the Time Band Pass bounds back to the full range: set the slider again, as the GUI would)
        dynamic_cast<TimeDomainBandPassBeforeFFT *>(q.filter_by("Band-Pass Filter in Time Domain after the FFT."))->high = tda->high;
        q.update_filter(q.index_of("Band-Pass Filter in Time Domain after the FFT."));
        std::vector<float> before;
        CHECK(eng2.download_final(before), "download_final");
        {
            // optical-property maps against the scan's own mean spectrum, on one slab and on two: the slabs' maps are the
            // whole grid's rows (a slab's kernels may pair other traces than one session's, so the last bits may differ)
            std::vector<std::complex<float>> avg_fft;
            std::vector<float> ref_amp, ref_phase, n1, a1, k1, s1, n2, a2, k2, s2;
            std::vector<int32_t> w1, w2;
            CHECK(eng2.averages(avg_fft, ref_amp, ref_phase), "averages");
            const size_t nf = ref_amp.size();
            thz_optical_cfg oc{};
            oc.thickness = 1e-3f;
            oc.anchor_k0 = (uint32_t)(nf / 10 + 1); oc.anchor_k1 = (uint32_t)(nf / 2);
            oc.n_bands = 2;
            oc.band_k0[0] = oc.anchor_k0; oc.band_k1[0] = oc.anchor_k1;
            oc.band_k0[1] = 1; oc.band_k1[1] = (uint32_t)nf;
            size_t gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0;
            CHECK(eng.optical_maps(ref_amp, ref_phase, oc, n1, a1, k1, w1, s1, gx1, gy1), "optical_maps on one slab");
            CHECK(eng2.optical_maps(ref_amp, ref_phase, oc, n2, a2, k2, w2, s2, gx2, gy2), "optical_maps on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1, "optical_maps: the whole grid");
            CHECK(n2.size() == 2 * gx1 * gy1 && k2.size() == n2.size() && w2.size() == gx1 * gy1 && s2.size() == w2.size(), "optical_maps: sizes");
            double worst = 0.0;
            for (size_t i = 0; i < s1.size(); ++i) worst = std::fmax(worst, std::fabs((double)s1[i] - s2[i]));
            std::printf("optical_maps: slope over two slabs against one, largest difference %.3g rad / bin\n", worst);
            CHECK(worst < 1e-4, "optical_maps over two slabs == over one (slope)");
        }
        {
            // echo maps and layer maps of the raw cube, on one slab and on two: every pixel is independent and the
            // winners depend on the data alone, so the slabs' maps are the whole grid's rows bit for bit
            thz_echo_cfg ec{};
            ec.mode = 1; ec.n_echoes = 3; ec.guard = 10; ec.rel_threshold = 0.1f;
            std::vector<int32_t> i1, i2, c1, c2;
            std::vector<float> o1, o2, v1, v2, t1, t2, d1, d2;
            size_t gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0, r1 = 0, r2 = 0;
            CHECK(eng.echo_map(THZ_BUF_RAW, ec, i1, o1, v1, c1, gx1, gy1), "echo_map on one slab");
            CHECK(eng2.echo_map(THZ_BUF_RAW, ec, i2, o2, v2, c2, gx2, gy2), "echo_map on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1, "echo_map: the whole grid");
            CHECK(i1.size() == 3 * gx1 * gy1 && c1.size() == gx1 * gy1, "echo_map: sizes");
            CHECK(i1 == i2 && c1 == c2 && std::memcmp(o1.data(), o2.data(), o1.size() * sizeof(float)) == 0
                      && std::memcmp(v1.data(), v2.data(), v1.size() * sizeof(float)) == 0,
                  "echo_map over two slabs == over one");
            size_t seconds = 0;
            for (int32_t n : c1) seconds += n >= 2;
            std::printf("echo_map: %zu of %zu pixels with a second pulse\n", seconds, c1.size());
            thz_layer_cfg lc{};
            lc.mode = 0;
            lc.scale[0] = lc.scale[1] = 0.01f;
            CHECK(eng.layer_map(lc, t1, d1, r1, gx1, gy1) && eng2.layer_map(lc, t2, d2, r2, gx2, gy2), "layer_map on one slab and on two");
            CHECK(r1 == 2 && r2 == 2 && t1.size() == 2 * gx1 * gy1 && t2.size() == t1.size(), "layer_map: sizes");
            CHECK(std::memcmp(t1.data(), t2.data(), t1.size() * sizeof(float)) == 0
                      && std::memcmp(d1.data(), d2.data(), d1.size() * sizeof(float)) == 0,
                  "layer_map over two slabs == over one");
        }
        {
            // sparse deconvolution of the raw cube, on one slab and on two: every pixel is independent and every sum has
            // one order, so the slabs' spike trains are the whole grid's rows bit for bit — and so are the echo maps taken
            // of them
            std::vector<float> ref((size_t)c.nt), taps(48);
            for (size_t i = 0; i < ref.size(); ++i) ref[i] = c.raw[i];  // pixel (0, 0)'s trace as the reference pulse
            thz_sparse_cfg sc{};
            sc.n_taps = 48; sc.center = 24; sc.n_iter = 25; sc.accelerate = 1; sc.rel_lambda = 0.05f; sc.min_lambda = 0.0f;
            CHECK(thz_host_sparse_kernel(ref.data(), ref.size(), sc.n_taps, sc.center, taps.data(), &sc.step) == THZ_OK, "sparse kernel from a trace");
            std::vector<float> x1, x2, r1, r2;
            std::vector<int32_t> n1, n2;
            size_t gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0, nt1 = 0, nt2 = 0;
            CHECK(eng.sparse_deconv(THZ_BUF_RAW, taps, sc, x1, r1, n1, gx1, gy1, nt1), "sparse_deconv on one slab");
            CHECK(eng2.sparse_deconv(THZ_BUF_RAW, taps, sc, x2, r2, n2, gx2, gy2, nt2), "sparse_deconv on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1 && nt1 == (size_t)c.nt && nt2 == nt1, "sparse_deconv: the whole grid");
            CHECK(x1.size() == gx1 * gy1 * nt1 && r1.size() == gx1 * gy1 && n1.size() == r1.size(), "sparse_deconv: sizes");
            CHECK(x1.size() == x2.size() && std::memcmp(x1.data(), x2.data(), x1.size() * sizeof(float)) == 0 && n1 == n2
                      && std::memcmp(r1.data(), r2.data(), r1.size() * sizeof(float)) == 0,
                  "sparse_deconv over two slabs == over one");
            // the device against the host function on one trace
            std::vector<float> hx(nt1);
            float hr = 0.0f;
            int32_t hn = 0;
            std::vector<float> y5(nt1);
            for (size_t i = 0; i < nt1; ++i) y5[i] = c.raw[5 * nt1 + i] - c.raw[5 * nt1];  // as uploaded: the first sample taken off
            CHECK(thz_host_sparse_trace(y5.data(), nt1, taps.data(), &sc, hx.data(), &hr, &hn) == THZ_OK, "host sparse trace");
            bool same = hn == n1[5];
            for (size_t i = 0; i < nt1; ++i) same = same && hx[i] == x1[5 * nt1 + i];
            CHECK(same, "sparse_deconv == thz_host_sparse_trace on a trace");
            size_t spikes = 0;
            for (int32_t n : n1) spikes += (size_t)n;
            std::printf("sparse_deconv: %.1f spikes per trace of %zu samples\n", (double)spikes / (double)n1.size(), nt1);
            thz_echo_cfg ec{};
            ec.mode = 0; ec.n_echoes = 2; ec.guard = 4; ec.rel_threshold = 0.3f;
            std::vector<int32_t> i1, i2, c1, c2;
            std::vector<float> o1, o2, v1, v2;
            CHECK(eng.echo_map(THZ_BUF_SPARSE, ec, i1, o1, v1, c1, gx1, gy1) && eng2.echo_map(THZ_BUF_SPARSE, ec, i2, o2, v2, c2, gx2, gy2),
                  "echo_map of the spike trains on one slab and on two");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && i1 == i2 && c1 == c2, "echo_map of the spike trains over two slabs == over one");
        }
        {
            // wavelet shrinkage of the raw cube, on one slab and on two: every pixel is independent and every sum has one
            // order, so the slabs' denoised traces are the whole grid's rows bit for bit
            thz_wavelet_cfg wc{};
            wc.n_levels = 4; wc.shrink = 1; wc.noise_mode = 0;
            std::vector<float> hn(8), gn(8), scale(4);
            int n_taps = 0;
            CHECK(thz_host_wavelet_filter(4, hn.data(), gn.data(), &n_taps) == THZ_OK && n_taps == 8, "wavelet filter");
            wc.n_taps = n_taps;
            CHECK(thz_host_wavelet_universal((size_t)c.nt, wc.n_levels, scale.data()) == THZ_OK, "universal thresholds");
            std::vector<float> x1, x2, s1, s2;
            std::vector<int32_t> k1, k2;
            size_t gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0, nt1 = 0, nt2 = 0;
            CHECK(eng.wavelet_denoise(THZ_BUF_RAW, hn, gn, scale, wc, x1, s1, k1, gx1, gy1, nt1), "wavelet_denoise on one slab");
            CHECK(eng2.wavelet_denoise(THZ_BUF_RAW, hn, gn, scale, wc, x2, s2, k2, gx2, gy2, nt2), "wavelet_denoise on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1 && nt1 == (size_t)c.nt && nt2 == nt1, "wavelet_denoise: the whole grid");
            CHECK(x1.size() == gx1 * gy1 * nt1 && s1.size() == gx1 * gy1 && k1.size() == s1.size(), "wavelet_denoise: sizes");
            CHECK(x1.size() == x2.size() && std::memcmp(x1.data(), x2.data(), x1.size() * sizeof(float)) == 0 && k1 == k2
                      && std::memcmp(s1.data(), s2.data(), s1.size() * sizeof(float)) == 0,
                  "wavelet_denoise over two slabs == over one");
            // the device against the host function on one trace
            std::vector<float> hx(nt1), y5(nt1);
            float hs = 0.0f;
            int32_t hk = 0;
            for (size_t i = 0; i < nt1; ++i) y5[i] = c.raw[5 * nt1 + i] - c.raw[5 * nt1];  // as uploaded: the first sample taken off
            CHECK(thz_host_wavelet_trace(y5.data(), nt1, hn.data(), gn.data(), scale.data(), &wc, hx.data(), &hs, &hk) == THZ_OK, "host wavelet trace");
            bool same = hk == k1[5] && hs == s1[5];
            for (size_t i = 0; i < nt1; ++i) same = same && hx[i] == x1[5 * nt1 + i];
            CHECK(same, "wavelet_denoise == thz_host_wavelet_trace on a trace");
            size_t kept = 0;
            for (int32_t n : k1) kept += (size_t)n;
            std::printf("wavelet_denoise: %.1f coefficients kept per trace of %zu samples\n", (double)kept / (double)k1.size(), nt1);
        }
        {
            // principal components of the resident amplitudes, on one slab and on two: the slabs' sums and Gram matrices
            // are added in f64, so the eigenvalues agree far inside the Gram matrix's own f32 error, and the scores to
            // the f32 rounding of the components
            thz_pca_cfg pc{};
            pc.first = 4; pc.count = 40; pc.step = 2; pc.n_components = 2; pc.center = 1;
            std::vector<uint8_t> mask((size_t)c.nx * (size_t)c.ny, 1);
            for (size_t i = 0; i < mask.size(); i += 7) mask[i] = 0;
            thz_pca_out o1{}, o2{};
            std::vector<float> s1, s2, v1, v2, m1, m2;
            size_t gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0;
            CHECK(eng.pca(THZ_BUF_AMPLITUDES, pc, mask, o1, s1, v1, m1, gx1, gy1), "pca on one slab");
            CHECK(eng2.pca(THZ_BUF_AMPLITUDES, pc, mask, o2, s2, v2, m2, gx2, gy2), "pca on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1, "pca: the whole grid");
            CHECK(s1.size() == 2 * gx1 * gy1 && s2.size() == s1.size() && v1.size() == 80 && m1.size() == 40, "pca: sizes");
            CHECK(o1.count == o2.count && o1.count == mask.size() - (mask.size() + 6) / 7, "pca: the unmasked pixels, bit for bit");
            CHECK(o1.eigenvalues[0] >= o1.eigenvalues[1] && o1.eigenvalues[1] > 0.0 && o1.total_variance >= o1.eigenvalues[0] + o1.eigenvalues[1] * 0.999,
                  "pca: eigenvalues in descending order inside the total variance");
            double worst_ev = 0.0, worst_s = 0.0, big_s = 0.0;
            for (int k = 0; k < 2; ++k) worst_ev = std::max(worst_ev, std::fabs(o1.eigenvalues[k] - o2.eigenvalues[k]) / o1.eigenvalues[0]);
            for (size_t i = 0; i < gx1 * gy1; ++i) {  // the leading component's score image
                worst_s = std::max(worst_s, (double)std::fabs(s1[i] - s2[i]));
                big_s = std::max(big_s, (double)std::fabs(s1[i]));
            }
            std::printf("pca: eigenvalues %.6g %.6g of %.6g; two slabs against one: eigenvalues %.3g (relative), scores %.3g of %.3g\n",
                        o1.eigenvalues[0], o1.eigenvalues[1], o1.total_variance, worst_ev, worst_s, big_s);
            CHECK(worst_ev < 1e-5, "pca over two slabs == over one (eigenvalues)");
            CHECK(worst_s < 1e-3 * big_s, "pca over two slabs == over one (leading score image)");
        }
        {
            // k-means of the resident amplitudes, on one slab and on two: the slabs' sums are added in f64 and the
            // farthest pixel is taken over both, so the two runs seed, iterate and label alike
            thz_cluster_cfg cc{};
            cc.first = 4; cc.count = 40; cc.step = 2; cc.n_clusters = 3; cc.init = 1; cc.max_iter = 20;
            std::vector<uint8_t> mask((size_t)c.nx * (size_t)c.ny, 1);
            for (size_t i = 0; i < mask.size(); i += 7) mask[i] = 0;
            thz_cluster_out o1{}, o2{};
            std::vector<int32_t> l1, l2;
            std::vector<float> d1, d2, m1, m2;
            size_t gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0;
            CHECK(eng.cluster(THZ_BUF_AMPLITUDES, cc, mask, o1, l1, d1, m1, gx1, gy1), "cluster on one slab");
            CHECK(eng2.cluster(THZ_BUF_AMPLITUDES, cc, mask, o2, l2, d2, m2, gx2, gy2), "cluster on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1, "cluster: the whole grid");
            CHECK(l1.size() == gx1 * gy1 && l2.size() == l1.size() && d1.size() == l1.size() && m1.size() == 120 && m2.size() == 120, "cluster: sizes");
            CHECK(o1.count == mask.size() - (mask.size() + 6) / 7 && o2.count == o1.count, "cluster: the unmasked pixels, bit for bit");
            CHECK(o1.iterations >= 2 && o1.iterations == o2.iterations && o1.converged == o2.converged, "cluster: the same steps");
            CHECK(o1.counts[0] + o1.counts[1] + o1.counts[2] == o1.count && o1.counts[0] > 0, "cluster: counts add up");
            CHECK(l1 == l2, "cluster over two slabs == over one (labels)");
            double worst_m = 0.0, worst_d = 0.0;
            for (size_t i = 0; i < m1.size(); ++i) worst_m = std::max(worst_m, (double)std::fabs(m1[i] - m2[i]) / std::max((double)std::fabs(m1[i]), 1e-30));
            for (size_t i = 0; i < d1.size(); ++i) worst_d = std::max(worst_d, (double)std::fabs(d1[i] - d2[i]) / std::max((double)d1[i], 1e-30));
            std::printf("cluster: %d steps, converged %d, counts %llu %llu %llu, inertia %.6g; two slabs against one: centroids %.3g, distances %.3g (relative)\n",
                        o1.iterations, o1.converged, (unsigned long long)o1.counts[0], (unsigned long long)o1.counts[1],
                        (unsigned long long)o1.counts[2], o1.inertia, worst_m, worst_d);
            CHECK(worst_m <= 1e-6, "cluster over two slabs == over one (centroids)");
            CHECK(worst_d <= 1e-4, "cluster over two slabs == over one (distances)");
            CHECK(std::fabs(o1.inertia - o2.inertia) <= 1e-5 * o1.inertia, "cluster over two slabs == over one (inertia)");
            // the fractions behind the labels: every pixel is independent, so with the same endmembers two slabs give
            // one slab's bits, and the resident centroids are the ones cluster() returned
            thz_unmix_session_cfg uc{};
            uc.first = cc.first; uc.count = cc.count; uc.step = cc.step; uc.n_endmembers = 3; uc.n_sweeps = 64;
            uc.endmembers = m1.data();
            std::vector<float> a1, a2, a3, r1, r2, r3, k1, k2, k3;
            CHECK(eng.unmix(THZ_BUF_AMPLITUDES, uc, a1, r1, k1, gx1, gy1), "unmix on one slab");
            CHECK(eng2.unmix(THZ_BUF_AMPLITUDES, uc, a2, r2, k2, gx2, gy2), "unmix on two slabs");
            CHECK(gx1 == (size_t)c.nx && gy1 == (size_t)c.ny && gx2 == gx1 && gy2 == gy1, "unmix: the whole grid");
            CHECK(a1.size() == 3 * gx1 * gy1 && r1.size() == gx1 * gy1 && k1.size() == r1.size(), "unmix: sizes");
            CHECK(a1 == a2 && r1 == r2 && k1 == k2, "unmix over two slabs == over one, bit for bit");
            uc.endmembers = nullptr;
            CHECK(eng.unmix(THZ_BUF_AMPLITUDES, uc, a3, r3, k3, gx1, gy1), "unmix with the resident centroids");
            CHECK(a1 == a3 && r1 == r3 && k1 == k3, "unmix: the resident centroids are cluster()'s");
            size_t agree = 0;
            for (size_t p = 0; p < gx1 * gy1; ++p) {
                int top = 0;
                for (int k = 1; k < 3; ++k)
                    if (a1[(size_t)k * gx1 * gy1 + p] > a1[(size_t)top * gx1 * gy1 + p]) top = k;
                agree += top == l1[p];
            }
            std::printf("unmix: the largest abundance names the k-means label at %zu of %zu pixels\n", agree, gx1 * gy1);
        }
        small_bank(q.filter_by("Deconvolution"));
        q.filters_active[q.filter_chain[q.index_of("Deconvolution")]] = true;
        q.update_filter(q.index_of("Deconvolution"));
        std::vector<float> dec_group;
        CHECK(eng2.download_final(dec_group), "download_final");
        CHECK(dec_group.size() == dec_single.size(), "group deconvolution: size");
        double err = 0.0, scale = 0.0, moved = 0.0;
        for (size_t i = 0; i < dec_group.size() && i < dec_single.size(); ++i) {
            err = std::fmax(err, std::fabs((double)dec_group[i] - dec_single[i]));
            scale = std::fmax(scale, std::fabs((double)dec_single[i]));
            moved = std::fmax(moved, std::fabs((double)dec_group[i] - before[i]));
        }
        std::printf("deconvolution, two slabs vs one: max |diff| %.3e of %.3e; the stage moved the cube by %.3e\n", err, scale, moved);
        CHECK(err <= 2e-6 * scale, "Deconvolution over two slabs == over one (the stage sees the whole image)");
        CHECK(moved > 1e-3 * scale, "... and it did run");
        dump(q, dir + "/deconv_group.bin");
        // a walk that starts elsewhere passes the stage's input through again (data_thread.rs:1139-1149)
        q.update_filter(q.index_of("Band-Pass Filter in Time Domain after the FFT."));
        std::vector<float> after;
        CHECK(eng2.download_final(after), "download_final");
        CHECK(after == before, "Deconvolution is a pass-through unless it is the filter being updated");
    }
    // switched off: the stage's input is the chain's output again
    active(i_dec, false);
    p.update_filter(i_dec);
    std::vector<float> undone;
    CHECK(eng.download_final(undone), "download_final");
    CHECK(undone != dec_single, "an inactive Deconvolution hands its input on");
    dump(p, dir + "/deconv_off.bin");

    std::printf(g_fail ? "ENGINE SELFTEST FAILED (%d)\n" : "ENGINE SELFTEST OK\n", g_fail);
    return g_fail ? 1 : 0;
}
