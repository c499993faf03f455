// fixed_scene_host_test.cpp -- which scenes take the scene twins of the fixed-frame kernels (pbrt-v1_amd/csrc/hip/rt_fixed_frame.h, flavour::FixedScene), on
// the host: a stand-alone program that tests/test_fixed_scene_host.py compiles with -fsanitize=address,undefined and runs.  scene_qualifies is checked over
// every combination of the scene facts, on every frame disqualifier and integrator; the family's tables are checked against the entries of
// flavour::Fixed its kernels are the twins of; and plan_schedule (rt_frame_plan.h) is checked to let the scene's knob (SceneFacts::scene_twins) turn a
// twin off and never on.
#include "rt_frame_plan.h"
#include <cstdio>
#include <cstring>
#include <set>

using namespace rt;
using namespace rt::flavour;

static int g_failed = 0;
static char g_what[160] = "";
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what); ++g_failed; } } while (0)

// the headline frame (tests/fixed_frame_host_test.cpp): it takes a fixed-frame kernel
static constexpr fixed::Facts good(int integ) { return fixed::Facts{integ, RT_SAMPLER_STRATIFIED, false, 0.f, RT_CAMERA_PERSPECTIVE, 1, 32, 1, false, false, false, true}; }

static_assert(!fixed::AnyScene::one_light && !fixed::AnyScene::no_specular, "fixed::AnyScene fixes nothing");
static_assert(fixed::scene_qualifies(good(RT_INTEGRATOR_DIRECT), fixed::SceneFacts{1u, false}) == (fixed::SCENE_ONE_LIGHT | fixed::SCENE_NO_SPECULAR), "C3's scene: both axes, at compile time");
static_assert(fixed::scene_qualifies(good(RT_INTEGRATOR_PATH), fixed::SceneFacts{1u, true}) == fixed::SCENE_ONE_LIGHT, "C4's scene: one light alone");

static RtRenderDesc desc(int integ, int strategy) {
    RtRenderDesc rd; std::memset(&rd, 0, sizeof rd);
    rd.integrator = integ; rd.strategy = strategy; rd.sampler = RT_SAMPLER_STRATIFIED; rd.x_samples = rd.y_samples = 2; rd.jitter = 1;
    rd.x_start = 0; rd.x_end = 70; rd.y_start = 0; rd.y_end = 45; rd.shard_index = 0; rd.shard_count = 1; rd.tile_pixels = 64; rd.max_depth = 5;
    return rd;
}
static plan::SceneFacts large_scene(unsigned n_lights, bool specular) {      // a timed kd-tree of thin leaves, no EXT code, no medium
    plan::SceneFacts f; f.n_nodes = 100000; f.per_leaf = 1.2; f.counting = false; f.n_lights = n_lights; f.light_samples.assign(n_lights, 1);
    f.specular_materials = specular;
    return f;
}
static plan::Schedule scheduled(const RtRenderDesc &rd, const plan::SceneFacts &sf, const plan::FrameKnobs &kn) {
    plan::Extent e; plan::Requests rq;
    CHECK(!plan::plan_extent(rd, e)); CHECK(!plan::plan_requests(rd, sf, e.spp, rq));
    return plan::plan_schedule(rd, sf, e, rq, kn);
}

int main() {
    int n_cases = 0;
    // ---- scene_qualifies over every combination of the scene facts, for every integrator a fixed frame can have
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ)
    for (unsigned nl : {0u, 1u, 2u, 3u, 65534u})
    for (int spec = 0; spec < 2; ++spec) {
        std::snprintf(g_what, sizeof g_what, "integ %d lights %u specular %d", integ, nl, spec);
        const int axes = fixed::scene_qualifies(good(integ), fixed::SceneFacts{nl, spec != 0});
        const bool twin = FixedScene::has(integ) && nl == 1u;                 // every twin is compiled for one light
        CHECK(axes == (twin ? fixed::SCENE_ONE_LIGHT | (spec ? 0 : fixed::SCENE_NO_SPECULAR) : 0));
        CHECK(!(axes & fixed::SCENE_NO_SPECULAR) || !spec);                   // never "no specular lobe" on a scene that has one
        CHECK(!(axes & fixed::SCENE_ONE_LIGHT) || nl == 1u);
        CHECK(axes == 0 || FixedScene::has_axes(axes));
        ++n_cases;
    }
    // ---- a frame that takes no fixed-frame kernel takes no scene twin, whatever the scene
#define DISQUALIFIES(WHAT, ...) { std::snprintf(g_what, sizeof g_what, "%s", WHAT); fixed::Facts f = good(RT_INTEGRATOR_DIRECT); __VA_ARGS__; \
        CHECK(!fixed::qualifies(f)); CHECK(fixed::scene_qualifies(f, fixed::SceneFacts{1u, false}) == 0); CHECK(fixed::scene_qualifies(f, fixed::SceneFacts{1u, true}) == 0); ++n_cases; }
    DISQUALIFIES("lowdiscrepancy", f.sampler = RT_SAMPLER_LOWDISCREPANCY)
    DISQUALIFIES("random", f.sampler = RT_SAMPLER_RANDOM)
    DISQUALIFIES("a light with nsamples 4", f.dims_max_n = 4)
    DISQUALIFIES("lens_radius > 0", f.lens_radius = 0.5f)
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

    // ---- the family: per integrator four different kernels, index / request round trips, each the twin of the Fixed entry the frame would take otherwise
    std::set<std::pair<int, std::pair<int, int>>> seen;
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ) {
        CHECK(FixedScene::has(integ) == (integ == RT_INTEGRATOR_DIRECT || integ == RT_INTEGRATOR_PATH));
        if (!FixedScene::has(integ)) continue;
        for (int k = 0; k < FixedScene::N; ++k) {
            std::snprintf(g_what, sizeof g_what, "FixedScene integ %d entry %d", integ, k);
            const Flavour f = FixedScene::flavour(k);
            const int axes = FixedScene::axes(k);
            seen.insert({integ, {f.accel, axes}});
            CHECK(!f.count && !f.vol && !f.ext && f.high_occ && f.waves == RT_HIGH_OCC_WAVES);
            CHECK(FixedScene::has_axes(axes) && (axes & fixed::SCENE_ONE_LIGHT));
            const Request r = FixedScene::request(k, integ);
            CHECK(FixedScene::index(r, axes) == k);
            CHECK(r.integ == integ && r.grid == (f.accel == RT_ACCEL_GRID) && !r.vol && !r.count && !r.ext && r.high_occ);
            const int t = FixedScene::fixed_twin(k, integ);
            CHECK(t == Fixed::index(r) && t >= 0 && t < Fixed::N && Fixed::integrator(t) == integ);
            const Flavour m = Fixed::flavour(t);
            CHECK(m.count == f.count && m.accel == f.accel && m.vol == f.vol && m.ext == f.ext && m.waves == f.waves && m.high_occ == f.high_occ);
            ++n_cases;
        }
    }
    std::snprintf(g_what, sizeof g_what, "FixedScene");
    CHECK(int(seen.size()) == 2 * FixedScene::N && 2 * FixedScene::N <= 12);
    CHECK(!FixedScene::has_axes(0) && !FixedScene::has_axes(fixed::SCENE_NO_SPECULAR) && !FixedScene::has_axes(4) && !FixedScene::has_axes(7));

    // ---- plan_schedule: the twin is chosen for the scenes that qualify, the knob at 0 turns it off, and no value of it turns it on
    struct Case { const char *what; int integ, strategy; unsigned nl; bool spec; bool ext, counting, medium; int want; };
    const int BOTH = fixed::SCENE_ONE_LIGHT | fixed::SCENE_NO_SPECULAR, ONE = fixed::SCENE_ONE_LIGHT;
    const Case cases[] = {
        {"direct all, one light, matte", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 1, false, false, false, false, BOTH},
        {"direct one, one light, matte", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE, 1, false, false, false, false, BOTH},
        {"path, one light, matte", RT_INTEGRATOR_PATH, 0, 1, false, false, false, false, BOTH},
        {"path, one light, glass and mirror", RT_INTEGRATOR_PATH, 0, 1, true, false, false, false, ONE},
        {"direct all, one light, a mirror", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 1, true, false, false, false, ONE},
        {"direct all, two lights", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 2, false, false, false, false, 0},
        {"direct all, no light", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 0, false, false, false, false, 0},
        {"path, two lights, a mirror", RT_INTEGRATOR_PATH, 0, 2, true, false, false, false, 0},
        {"whitted, one light", RT_INTEGRATOR_WHITTED, 0, 1, false, false, false, false, 0},
        {"direct weighted", RT_INTEGRATOR_DIRECT, RT_STRATEGY_WEIGHTED, 1, false, false, false, false, 0},
        {"EXT", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 1, false, true, false, false, 0},
        {"counting", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 1, false, false, true, false, 0},
        {"a medium", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, 1, false, false, false, true, 0},
    };
    for (const Case &c : cases) {
        plan::SceneFacts sf = large_scene(c.nl, c.spec); sf.has_ext = c.ext; sf.counting = c.counting; sf.medium = c.medium;
        const RtRenderDesc rd = desc(c.integ, c.strategy);
        for (int twins = 0; twins < 2; ++twins) {                             // SceneFacts::scene_twins: false for a scene created under PBRT_HIP_FIXED_SCENE=0, true for every other value and unset
            std::snprintf(g_what, sizeof g_what, "%s, scene_twins %d", c.what, twins);
            sf.scene_twins = twins != 0;
            plan::FrameKnobs kn;
            if (sf.medium) kn.pipeline = 0;
            const plan::Schedule sc = scheduled(rd, sf, kn);
            CHECK(sc.fixed_scene == (twins ? c.want : 0));                    // allowing the twin never puts one on a scene that does not qualify
            CHECK(sc.fixed_scene == 0 || sc.fixed_frame);                     // a scene twin is a fixed-frame kernel
            CHECK(sc.fixed_scene == 0 || FixedScene::has_axes(sc.fixed_scene));
            ++n_cases;
        }
        {   // the frame's own knob at 0 takes the scene twin with it; at 1 it forces nothing
            std::snprintf(g_what, sizeof g_what, "%s, PBRT_HIP_FIXED_FRAME", c.what);
            sf.scene_twins = true;
            plan::FrameKnobs off; off.fixed_frame = 0; if (sf.medium) off.pipeline = 0;
            const plan::Schedule sc = scheduled(rd, sf, off);
            CHECK(!sc.fixed_frame && sc.fixed_scene == 0);
            plan::FrameKnobs on; on.fixed_frame = 1; if (sf.medium) on.pipeline = 0;
            CHECK(scheduled(rd, sf, on).fixed_scene == c.want);
            ++n_cases;
        }
    }
    {   // a radiance query takes neither
        std::snprintf(g_what, sizeof g_what, "plan_query");
        plan::Schedule sc = scheduled(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL), large_scene(1, false), plan::FrameKnobs{});
        CHECK(sc.fixed_scene == BOTH);
        CHECK(!plan::plan_query(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL), plan::QueryRange{0, 64}, sc));
        CHECK(!sc.fixed_frame && sc.fixed_scene == 0);
        ++n_cases;
    }
    if (g_failed) { std::fprintf(stderr, "fixed_scene_host_test: %d checks failed\n", g_failed); return 1; }
    std::printf("fixed_scene_host_test: ok (%d cases)\n", n_cases);
    return 0;
}
