// fixed_frame_host_test.cpp -- which frames take the kernels compiled for a fixed frame (pbrt-v1_amd/csrc/hip/rt_fixed_frame.h), on the host: a stand-alone
// program that tests/test_fixed_frame_host.py compiles with -fsanitize=address,undefined and runs.  The predicate is checked on the frame that qualifies
// and on every disqualifier alone; the family's table is checked against the entries of flavour::Mega its kernels are the twins of.
#include "rt_fixed_frame.h"
#include <cstdio>
#include <set>

using namespace rt;
using namespace rt::flavour;

static int g_failed = 0;
static const char *g_what = "";
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what); ++g_failed; } } while (0)

// the headline frame: DirectLighting, stratified, pinhole perspective camera, one shard handed out in 32-pixel blocks, every light with one sample,
// the timed high-occupancy kernel of a large scene without EXT materials and without a medium
static fixed::Facts good() { return fixed::Facts{RT_INTEGRATOR_DIRECT, RT_SAMPLER_STRATIFIED, false, 0.f, RT_CAMERA_PERSPECTIVE, 1, 32, 1, false, false, false, true}; }

// compile time too: the host's choice is a constant expression
static_assert(fixed::qualifies(fixed::Facts{RT_INTEGRATOR_PATH, RT_SAMPLER_STRATIFIED, false, 0.f, RT_CAMERA_ORTHOGRAPHIC, 1, 32, 1, false, false, false, true}), "an orthographic path frame qualifies");
static_assert(fixed::Any::sampler < 0 && !fixed::Any::no_lens && !fixed::Any::no_env_camera && !fixed::Any::tile_order && !fixed::Any::all_n1, "fixed::Any fixes nothing");

int main() {
    int n_cases = 0;
    // ---- the frames that qualify
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ)
    for (int cam : {int(RT_CAMERA_PERSPECTIVE), int(RT_CAMERA_ORTHOGRAPHIC)})
    for (int n : {0, 1})                                  // Whitted asks for no samples at all
    for (int tile : {1, 32, 4096}) {
        g_what = "qualifies";
        fixed::Facts f = good(); f.integrator = integ; f.camera_type = cam; f.dims_max_n = n; f.mega_tile = tile;
        CHECK(fixed::qualifies(f)); ++n_cases;
    }
    // ---- every disqualifier on its own
#define DISQUALIFIES(WHAT, ...) { g_what = WHAT; fixed::Facts f = good(); __VA_ARGS__; CHECK(!fixed::qualifies(f)); ++n_cases; }
    DISQUALIFIES("lowdiscrepancy", f.sampler = RT_SAMPLER_LOWDISCREPANCY)
    DISQUALIFIES("random", f.sampler = RT_SAMPLER_RANDOM)
    DISQUALIFIES("a light with nsamples 4", f.dims_max_n = 4)
    DISQUALIFIES("a light with nsamples 2", f.dims_max_n = 2)
    DISQUALIFIES("lens_radius > 0", f.lens_radius = 0.5f)
    DISQUALIFIES("lens_radius tiny but > 0", f.lens_radius = 1e-30f)
    DISQUALIFIES("environment camera", f.camera_type = RT_CAMERA_ENVIRONMENT)
    DISQUALIFIES("two shards", f.shard_count = 2)
    DISQUALIFIES("scanline order", f.mega_tile = 0)
    DISQUALIFIES("counting", f.counting = true)
    DISQUALIFIES("EXT", f.ext = true)
    DISQUALIFIES("a medium", f.vol = true)
    DISQUALIFIES("a tiny scene: no high-occupancy kernel", f.high_occ = false)
    DISQUALIFIES("weighted", f.weighted = true)
    DISQUALIFIES("bidirectional", f.integrator = RT_INTEGRATOR_BIDIRECTIONAL)
    DISQUALIFIES("debug", f.integrator = RT_INTEGRATOR_DEBUG)
    DISQUALIFIES("integrator below the range", f.integrator = -1)

    // ---- the family: six different kernels, index / request round trips, each the twin of the Mega entry the frame would take otherwise
    g_what = "Fixed";
    std::set<std::pair<int, int>> seen;
    for (int k = 0; k < Fixed::N; ++k) {
        const Flavour f = Fixed::flavour(k);
        seen.insert({Fixed::integrator(k), f.accel});
        CHECK(!f.count && !f.vol && !f.ext && f.high_occ && f.waves == RT_HIGH_OCC_WAVES);
        CHECK(Fixed::integrator(k) >= RT_INTEGRATOR_WHITTED && Fixed::integrator(k) <= RT_INTEGRATOR_PATH);
        const Request r = Fixed::request(k);
        CHECK(Fixed::index(r) == k);
        CHECK(r.integ == Fixed::integrator(k) && r.grid == (f.accel == RT_ACCEL_GRID) && !r.vol && !r.count && !r.ext && r.high_occ);
        const int g = Fixed::generic(k);
        CHECK(g == Mega::index(r) && g >= 8 && g < 12);
        const Flavour m = Mega::flavour(g, Fixed::integrator(k));
        CHECK(m.count == f.count && m.accel == f.accel && m.vol == f.vol && m.ext == f.ext && m.waves == f.waves && m.high_occ == f.high_occ);
    }
    CHECK(int(seen.size()) == Fixed::N && Fixed::N == 6);
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ)
    for (int grid = 0; grid < 2; ++grid) {                // every request a qualifying frame can make has an entry of its own
        const Request r{integ, grid != 0, false, false, false, true};
        const int k = Fixed::index(r);
        CHECK(k >= 0 && k < Fixed::N && Fixed::integrator(k) == integ && Fixed::flavour(k).accel == (grid ? RT_ACCEL_GRID : RT_ACCEL_KDTREE));
    }
    if (g_failed) { std::fprintf(stderr, "fixed_frame_host_test: %d checks failed\n", g_failed); return 1; }
    std::printf("fixed_frame_host_test: ok (%d frames)\n", n_cases);
    return 0;
}
