// engine_voxel_selftest.cpp — the 3-D tab's instances of the record-and-flush engine (GpuEngine::voxels) over a group
// of three slabs against one slab: the same cube, the same stage walk on both, and the group's instances must be those
// of the whole cube bit for bit (threshold, count, records, cube dimensions).  A cube of its own (no input files):
// pulses whose position and height change across the grid, some rows dead.  tests/test_gpu_group_voxels.py runs it.
//
// usage: engine_voxel_selftest
#include "thz_engine.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
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

struct Voxels {
    bool ok = false;
    std::vector<thz_voxel_instance> inst;
    float threshold = -1.0f, dims[3] = {0.0f, 0.0f, 0.0f};
};

static Voxels voxels_of(GpuEngine &eng, const thz_voxel_cfg &cfg, uint64_t max_instances, size_t scaling)
{
    Voxels v;
    v.ok = eng.voxels(cfg, max_instances, scaling, eng.nx, eng.ny, eng.nt_out(), v.inst, v.threshold, v.dims);
    return v;
}

static void compare(const Voxels &one, const Voxels &group, const std::string &what)
{
    CHECK(one.ok && group.ok, (what + ": voxels").c_str());
    CHECK(!one.inst.empty(), (what + ": instances exist").c_str());
    CHECK(std::memcmp(&one.threshold, &group.threshold, sizeof(float)) == 0, (what + ": threshold bits").c_str());
    CHECK(one.inst.size() == group.inst.size(), (what + ": count").c_str());
    CHECK(one.inst.size() == group.inst.size()
              && std::memcmp(one.inst.data(), group.inst.data(), one.inst.size() * sizeof(thz_voxel_instance)) == 0,
          (what + ": records").c_str());
    CHECK(std::memcmp(one.dims, group.dims, sizeof one.dims) == 0, (what + ": cube dimensions").c_str());
    std::printf("%s: %zu instances, threshold %.6g\n", what.c_str(), group.inst.size(), (double)group.threshold);
}

int main()
{
    // 20 x 12 x 256: three slabs of 7, 7 and 6 rows; a power-of-two length (no trace pairs across slab edges)
    const size_t nx = 20, ny = 12, nt = 256;
    std::vector<float> time(nt), cube(nx * ny * nt, 0.0f);
    for (size_t k = 0; k < nt; ++k) time[k] = 0.05f * (float)k;
    for (size_t x = 0; x < nx; ++x)
        for (size_t y = 0; y < ny; ++y) {
            if (x == 2 || x == 15) continue;  // dead rows: no instance there
            const double t0 = 3.0 + 0.35 * (double)x + 0.2 * (double)y, amp = 1.0 + 0.1 * (double)((x * 7 + y * 3) % 11);
            for (size_t k = 0; k < nt; ++k) {
                const double u = (double)time[k] - t0;
                cube[(x * ny + y) * nt + k] = (float)(amp * (1.0 - 2.0 * u * u) * std::exp(-u * u) + 0.01 * std::sin(0.7 * (double)k));
            }
        }
    GpuEngine one({0}), three({0, 0, 0});
    if (!one.available() || !three.available()) {
        std::printf("FAIL: no GPU engine\n");
        return 1;
    }
    GpuPipeline p1(one), p3(three);
    p1.open(cube.data(), nx, ny, time, 0.5f, 0.5f);
    p3.open(cube.data(), nx, ny, time, 0.5f, 0.5f);
    thz_voxel_cfg cfg;
    thz_voxel_cfg_default(&cfg);
    cfg.opacity_threshold = 0.0f;  // the band-passed traces are weak: at 0.1 most traces would be dead
    const uint64_t n_total = nx * ny * nt;

    // ---- the default chain: every voxel fits; then a selection (threshold from the whole cube), and a max_instances
    //      that every slab's own voxels fit but the cube's do not
    p1.update_filter(1);
    p3.update_filter(1);
    compare(voxels_of(one, cfg, n_total, 1), voxels_of(three, cfg, n_total, 1), "default chain, no selection");
    compare(voxels_of(one, cfg, 5000, 1), voxels_of(three, cfg, 5000, 1), "default chain, max_instances 5000");
    const uint64_t slab_max = 7 * ny * nt;
    const Voxels sel1 = voxels_of(one, cfg, slab_max, 1), sel3 = voxels_of(three, cfg, slab_max, 1);
    compare(sel1, sel3, "default chain, max_instances = the largest slab");
    CHECK(sel3.threshold > 0.0f, "the whole cube's n exceeds max_instances: a selection took place");

    // ---- scaled (s = 2: 10 x 6 blocks; the block of rows 6-7 lies in two slabs and belongs to the second)
    p1.config.scale_factor = 2;
    p3.config.scale_factor = 2;
    p1.update_filter(1);
    p3.update_filter(1);
    compare(voxels_of(one, cfg, 3000, 2), voxels_of(three, cfg, 3000, 2), "scale 2, max_instances 3000");

    // ---- back to the raw grid, a narrower kernel and more contrast
    p1.config.scale_factor = 1;
    p3.config.scale_factor = 1;
    p1.update_filter(1);
    p3.update_filter(1);
    cfg.radius = 4;
    cfg.contrast = 3.0f;
    compare(voxels_of(one, cfg, 10000, 1), voxels_of(three, cfg, 10000, 1), "radius 4, contrast 3, max_instances 10000");

    std::printf(g_fail ? "ENGINE VOXEL SELFTEST FAILED (%d)\n" : "ENGINE VOXEL SELFTEST OK\n", g_fail);
    return g_fail ? 1 : 0;
}
