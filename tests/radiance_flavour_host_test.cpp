// radiance_flavour_host_test.cpp -- the radiance query's kernel family and plan (pbrt-v1_amd/csrc/hip/rt_flavour.h flavour::Rays, rt_fixed_frame.h
// fixed::Rays, rt_frame_plan.h plan_query) on the host: a stand-alone program that tests/test_radiance_host.py compiles with
// -fsanitize=address,undefined and runs.  Which entry a query launches and what its work extent is cannot be seen in its results.
#include "rt_frame_plan.h"
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

using namespace rt;
using namespace rt::flavour;

static int g_failed = 0;
static char g_what[160] = "";
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what); ++g_failed; } } while (0)

static RtRenderDesc frame(int integ, int strategy, int sampler) {
    RtRenderDesc rd; std::memset(&rd, 0, sizeof rd);
    rd.integrator = integ; rd.max_depth = 5; rd.strategy = strategy; rd.sampler = sampler;
    rd.x_samples = 2; rd.y_samples = 2; rd.pixel_samples = 4; rd.jitter = 1;
    rd.x_res = rd.x_pixel_count = 33; rd.y_res = rd.y_pixel_count = 21;
    rd.x_start = -1; rd.x_end = 34; rd.y_start = -1; rd.y_end = 22;                  // 35 x 23 pixels of samples, 4 spp: 3220 camera samples
    rd.filter_x_width = rd.filter_y_width = 2.f;
    rd.shard_index = 0; rd.shard_count = 1; rd.tile_pixels = 64;
    return rd;
}
static const unsigned long long SAMPLES = 35ull * 23ull * 4ull;

// the plan of a query of rays [first, first + n) of the frame rd, as make_frame forms it
static plan::Refusal plan_of(const RtRenderDesc &rd, const plan::SceneFacts &sf, unsigned long long first, unsigned n, plan::Schedule &sc) {
    plan::Extent ext; plan::Requests rq;
    if (plan::Refusal r = plan::plan_extent(rd, ext)) return r;
    if (plan::Refusal r = plan::plan_requests(rd, sf, ext.spp, rq)) return r;
    sc = plan::plan_schedule(rd, sf, ext, rq, plan::FrameKnobs{});
    return plan::plan_query(rd, plan::QueryRange{first, n}, sc);
}

int main() {
    // ---- the traits: the ray source is an axis of its own, off in everything that existed
    static_assert(!fixed::Any::caller_rays && !fixed::Frame::caller_rays && fixed::Rays::caller_rays, "ray-source axis");
    static_assert(fixed::Rays::sampler == -1 && !fixed::Rays::no_lens && !fixed::Rays::no_env_camera && !fixed::Rays::tile_order && !fixed::Rays::all_n1,
                  "a query assumes nothing else of its frame");
    CHECK(fixed::Any::caller_rays == false);

    // ---- the family: 8 entries per integrator, one per (medium, accelerator, counting), all EXT at natural allocation, never high occupancy
    CHECK(Rays::N == 8);
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ) {
        std::set<std::tuple<bool, int, bool>> seen;
        for (int k = 0; k < Rays::N; ++k) {
            std::snprintf(g_what, sizeof g_what, "integ %d entry %d", integ, k);
            const Flavour f = Rays::flavour(k, integ);
            CHECK(Rays::index(f.request()) == k);
            CHECK(f.ext && !f.high_occ && f.waves < RT_HIGH_OCC_WAVES);
            seen.insert(std::make_tuple(f.count, f.accel, f.vol));
            // the Mega entry whose shading code it carries: the same arguments but the ray source
            const Flavour m = Mega::flavour(Rays::generic(k), integ);
            CHECK(m.count == f.count && m.accel == f.accel && m.vol == f.vol && m.ext && !m.high_occ);
        }
        CHECK(int(seen.size()) == Rays::N);
    }
    int n_requests = 0;
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ)
    for (int bits = 0; bits < 32; ++bits, ++n_requests) {
        const bool g = bits & 1, v = bits & 2, c = bits & 4, e = bits & 8, h = bits & 16;
        std::snprintf(g_what, sizeof g_what, "integ %d grid %d vol %d count %d ext %d high_occ %d", integ, g, v, c, e, h);
        const int k = Rays::index(Request{integ, g, v, c, e, h});
        CHECK(k >= 0 && k < Rays::N);
        const Flavour f = Rays::flavour(k, integ);
        CHECK(f.count == c && f.accel == (g ? RT_ACCEL_GRID : RT_ACCEL_KDTREE) && f.vol == v && f.ext);      // whatever the scene's EXT and the frame's occupancy choice
    }

    // ---- the plan: the work extent of a query of n rays is n, always the megakernel, no tile order, no fixed twin
    plan::SceneFacts sf;
    sf.n_nodes = 1u << 20; sf.per_leaf = 1.2; sf.n_lights = 2; sf.light_samples = {1, 4}; sf.counting = false;      // a large tree: the frame itself would take high occupancy
    const int integs[4][2] = {{RT_INTEGRATOR_WHITTED, 0}, {RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL}, {RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE}, {RT_INTEGRATOR_PATH, 0}};
    for (const auto &is : integs)
    for (int sampler = RT_SAMPLER_STRATIFIED; sampler <= RT_SAMPLER_RANDOM; ++sampler)
    for (int medium = 0; medium < 2; ++medium) {
        std::snprintf(g_what, sizeof g_what, "integ %d strategy %d sampler %d medium %d", is[0], is[1], sampler, medium);
        RtRenderDesc rd = frame(is[0], is[1], sampler);
        sf.medium = medium != 0;
        const unsigned ns[] = {0u, 1u, 63u, 64u, 65u, 1000u, unsigned(SAMPLES)};
        for (unsigned n : ns) {
            plan::Schedule sc;
            const plan::Refusal r = plan_of(rd, sf, 0, n, sc);
            CHECK(!r);
            CHECK(sc.extent.total_work == n);
            CHECK(sc.extent.spp == 4 && sc.extent.total_pixels == 35ull * 23ull && sc.extent.shard_count == 1);
            CHECK(sc.pipeline == 0 && sc.mega_tile == 0 && sc.high_occupancy == 0 && !sc.fixed_frame && !sc.by_vertex);
            CHECK(sc.trav_mode == 2 || sc.trav_mode == 3);
        }
        plan::Schedule sc;
        CHECK(!plan_of(rd, sf, SAMPLES - 5, 5, sc) && sc.extent.total_work == 5);
        CHECK(!plan_of(rd, sf, SAMPLES, 0, sc));
        // ... and the same sample requests as the frame's: the sample set is the frame's
        plan::Extent ext; plan::Requests a, b;
        CHECK(!plan::plan_extent(rd, ext) && !plan::plan_requests(rd, sf, ext.spp, a) && !plan::plan_requests(rd, sf, sc.extent.spp, b));
        CHECK(a.lhs_total == b.lhs_total && a.pixgen_draws == b.pixgen_draws && a.table.size() == b.table.size());
    }

    // ---- the refusals, each with its reason
    struct { int integ, strategy, shards; unsigned long long first; unsigned n; const char *word; } bad[] = {
        {RT_INTEGRATOR_DIRECT, RT_STRATEGY_WEIGHTED, 1, 0, 8, "weighted"},
        {RT_INTEGRATOR_BIDIRECTIONAL, 0, 1, 0, 8, "bidirectional"},
        {RT_INTEGRATOR_DEBUG, 0, 1, 0, 8, "debug"},
        {RT_INTEGRATOR_PATH, 0, 2, 0, 8, "shard_count"},
        {RT_INTEGRATOR_PATH, 0, 1, SAMPLES - 4, 5, "beyond"},
        {RT_INTEGRATOR_PATH, 0, 1, SAMPLES + 1, 0, "beyond"},
        {RT_INTEGRATOR_PATH, 0, 1, 1ull << 40, 1, "beyond"},
    };
    sf.medium = false;
    for (const auto &b : bad) {
        std::snprintf(g_what, sizeof g_what, "refusal %s", b.word);
        RtRenderDesc rd = frame(b.integ, b.strategy, RT_SAMPLER_STRATIFIED);
        rd.shard_count = b.shards;
        plan::Schedule sc;
        const plan::Refusal r = plan_of(rd, sf, b.first, b.n, sc);
        CHECK(r.code == RT_EINVAL);
        CHECK(std::strstr(r.msg, b.word) != nullptr && std::strstr(r.msg, "rt_radiance_device") != nullptr);
    }

    if (g_failed) { std::fprintf(stderr, "radiance_flavour_host_test: %d checks failed\n", g_failed); return 1; }
    std::printf("radiance_flavour_host_test: ok (%d requests)\n", n_requests);
    return 0;
}
