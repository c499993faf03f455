// frame_plan_host_test.cpp -- what the host plans for a frame (pbrt-v1_amd/csrc/hip/rt_frame_plan.h), on the host: a stand-alone program that
// tests/test_frame_plan_host.py compiles with -fsanitize=address,undefined and runs.  The expectations are written from the reference's rules
// (Sample::Sample sampling.cpp:41-70, LatinHypercube's draw counts sampling.cpp:98-113, stratified.cpp:99-117, random.cpp:88-112,
// lowdiscrepancy.cpp:93-104, Sampler::RoundSize) and from the scheduling policy as DESIGN.md 4.1 states it, not from the planner's output.
#include "rt_frame_plan.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace rt;
using namespace rt::plan;

static int g_failed = 0, g_cases = 0;
static std::string g_what;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what.c_str()); ++g_failed; } } while (0)
#define CASE(what) do { g_what = (what); ++g_cases; } while (0)

// ---- frames and scenes
static RtRenderDesc desc(int integ, int strategy = RT_STRATEGY_ALL, int sampler = RT_SAMPLER_STRATIFIED) {
    RtRenderDesc rd{};
    rd.integrator = integ; rd.strategy = strategy; rd.max_depth = 5; rd.volume_integrator = RT_VOLUME_EMISSION; rd.step_size = 1.f;
    rd.sampler = sampler; rd.x_samples = 2; rd.y_samples = 2; rd.jitter = 1; rd.pixel_samples = 3;
    rd.x_res = rd.x_pixel_count = 16; rd.y_res = rd.y_pixel_count = 16; rd.x_end = 17; rd.y_end = 13;       // a 17 x 13 sample extent
    rd.filter_x_width = rd.filter_y_width = .5f;
    rd.shard_index = 0; rd.shard_count = 1; rd.tile_pixels = 1;
    return rd;
}
static SceneFacts large_scene() {                         // a timed kd-tree of thin leaves, no EXT code, no medium, one light of one sample
    SceneFacts f; f.n_nodes = 100000; f.per_leaf = 1.2; f.counting = false; f.n_lights = 1; f.light_samples = {1};
    const float b[6] = {0, 0, 0, 2, 4, 4}; std::memcpy(f.bounds, b, sizeof b);
    return f;
}
static SceneFacts tiny_fat() { SceneFacts f = large_scene(); f.n_nodes = 4096; f.per_leaf = 1.5; return f; }
static SceneFacts with_lights(std::vector<int> ns) { SceneFacts f = large_scene(); f.n_lights = unsigned(ns.size()); f.light_samples = std::move(ns); return f; }

struct Combo { const char *name; int integ, strategy; std::vector<int> n1, n2; };      // RequestSamples: the integrator's own 1-D and 2-D requests, one light of one sample
static std::vector<Combo> combos() {
    return {{"whitted", RT_INTEGRATOR_WHITTED, 0, {}, {}},                                                   // whitted.cpp requests nothing
            {"direct all", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, {1}, {1, 1}},                              // directlighting.cpp:44-55: per light 2 x 2-D, 1 x 1-D
            {"direct one", RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE, {1, 1}, {1, 1}},                           // :57-65: light sample, light number, BSDF sample, BSDF component
            {"direct weighted", RT_INTEGRATOR_DIRECT, RT_STRATEGY_WEIGHTED, {1, 1}, {1, 1}},
            {"path", RT_INTEGRATOR_PATH, 0, std::vector<int>(9, 1), std::vector<int>(9, 1)},                 // path.cpp:47-57: 3 x 3 of each
            {"bidirectional", RT_INTEGRATOR_BIDIRECTIONAL, 0, std::vector<int>(17, 1), std::vector<int>(18, 1)},     // bidirectional.cpp:65-79
            {"debug", RT_INTEGRATOR_DEBUG, 0, {}, {}}};
}

// Sample::Sample lays out every 1-D request, then every 2-D one; where the sampler's values of request r start in the stream of one camera sample:
//   stratified: LatinHypercube(n values of d dimensions) draws n * d floats, then n * d shuffle numbers (sampling.cpp:98-113)
//   random: one float per value (random.cpp:107-112)
//   lowdiscrepancy: after the image (2 + 2P), lens (2 + 2P) and time (1 + 2P) blocks, a request of n takes d scrambles, n * P values, P shuffles
struct Want { std::vector<DimReq> d1, d2; unsigned lhs_total, pixgen; };
static Want model(int sampler, int jitter, unsigned P, std::vector<int> n1, const std::vector<int> &n2) {
    n1.push_back(1); n1.push_back(1);                     // emission.cpp:42-46 / single.cpp:43-47: tau and scatter offsets, after the surface integrator's
    Want w; unsigned at = sampler == RT_SAMPLER_LOWDISCREPANCY ? 5 + 6 * P : 0;
    for (int d = 1; d <= 2; ++d)
        for (int n : (d == 1 ? n1 : n2)) {
            const unsigned values = unsigned(n) * unsigned(d);
            DimReq r{at, sampler == RT_SAMPLER_STRATIFIED ? at + values : 0u, (unsigned short)n, (unsigned short)d};
            at += sampler == RT_SAMPLER_STRATIFIED ? 2 * values : sampler == RT_SAMPLER_RANDOM ? values : unsigned(d) + unsigned(n) * P + P;
            (d == 1 ? w.d1 : w.d2).push_back(r);
        }
    w.lhs_total = sampler == RT_SAMPLER_LOWDISCREPANCY ? 0 : at;
    // a new pixel: stratified draws 2 P image + 2 P lens + P time jitters and the lens and time shuffles (P each) with jitter, the two shuffles
    // without (stratified.cpp:99-117); random 2 P + 2 P + P floats (random.cpp:88-92); lowdiscrepancy everything, requests included
    w.pixgen = sampler == RT_SAMPLER_STRATIFIED ? (jitter ? 7 * P : 2 * P) : sampler == RT_SAMPLER_RANDOM ? 5 * P : at;
    return w;
}
static bool same(const DimReq &a, const DimReq &b) { return a.f_base == b.f_base && a.u_base == b.u_base && a.n == b.n && a.dims == b.dims; }
static bool is(const DimReq &a, unsigned f, unsigned u, unsigned n, unsigned d) { return same(a, DimReq{f, u, (unsigned short)n, (unsigned short)d}); }

static void test_requests() {
    // ---- every integrator x sampler (x jitter) against the model
    for (const Combo &c : combos())
    for (int sampler : {int(RT_SAMPLER_STRATIFIED), int(RT_SAMPLER_LOWDISCREPANCY), int(RT_SAMPLER_RANDOM)})
    for (int jitter : {1, 0}) {
        CASE(std::string(c.name) + " sampler " + std::to_string(sampler) + " jitter " + std::to_string(jitter));
        RtRenderDesc rd = desc(c.integ, c.strategy, sampler); rd.jitter = jitter;
        Extent e; Requests rq;
        CHECK(!plan_extent(rd, e));
        CHECK(e.spp == 4);                                // 2 x 2 strata; pixelsamples 3 rounds up to 4
        CHECK(!plan_requests(rd, large_scene(), e.spp, rq));
        const Want w = model(sampler, jitter, 4, c.n1, c.n2);
        CHECK(rq.lhs_total == w.lhs_total && rq.pixgen_draws == w.pixgen);
        const bool all = c.integ == RT_INTEGRATOR_DIRECT && c.strategy == RT_STRATEGY_ALL, bidir = c.integ == RT_INTEGRATOR_BIDIRECTIONAL;
        CHECK(rq.dims_max_n == (c.n2.empty() ? 0 : 1));
        if (all || bidir) {                               // the integrator's requests live in the table, the descriptor keeps the volume integrator's two
            CHECK(rq.n1d == 2 && rq.n2d == 0);
            CHECK(same(rq.one_d[0], w.d1[w.d1.size() - 2]) && same(rq.one_d[1], w.d1[w.d1.size() - 1]));
            if (all) {
                CHECK(rq.table.size() == 4);
                if (rq.table.size() == 4) CHECK(same(rq.table[0], w.d2[0]) && same(rq.table[1], w.d2[1]) && same(rq.table[2], w.d1[0]) && is(rq.table[3], 0, 0, 0, 0));
            } else {
                CHECK(rq.table.size() * sizeof(DimReq) >= sizeof(BidirTable) && rq.table.size() == 37);
                BidirTable bt; std::memcpy(&bt, rq.table.data(), sizeof bt);
                for (int i = 0; i < 17; ++i) CHECK(same(bt.one_d[i], w.d1[size_t(i)]));
                for (int i = 0; i < 18; ++i) CHECK(same(bt.two_d[i], w.d2[size_t(i)]));
            }
        } else {
            CHECK(rq.table.empty());
            CHECK(rq.n1d == int(w.d1.size()) && rq.n2d == int(w.d2.size()));
            for (int i = 0; i < rq.n1d; ++i) CHECK(same(rq.one_d[i], w.d1[size_t(i)]));
            for (int i = 0; i < rq.n2d; ++i) CHECK(same(rq.two_d[i], w.d2[size_t(i)]));
        }
        for (int i = rq.n1d; i < RT_MAX_DIM_REQ; ++i) CHECK(is(rq.one_d[i], 0, 0, 0, 0));
        for (int i = rq.n2d; i < RT_MAX_DIM_REQ; ++i) CHECK(is(rq.two_d[i], 0, 0, 0, 0));
    }
    // ---- the anchors, derived by hand
    auto planned = [](RtRenderDesc rd, const SceneFacts &sf, int *spp = nullptr) { Extent e; Requests rq; CHECK(!plan_extent(rd, e)); CHECK(!plan_requests(rd, sf, e.spp, rq)); if (spp) *spp = e.spp; return rq; };
    for (int jitter : {1, 0}) {
        CASE("stratified path"); RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); rd.jitter = jitter; rd.x_samples = 3; rd.y_samples = 2;
        const Requests rq = planned(rd, large_scene());
        CHECK(rq.n1d == 11 && rq.n2d == 9 && rq.lhs_total == 58 && rq.pixgen_draws == (jitter ? 7u * 6u : 2u * 6u));
        for (unsigned i = 0; i < 11; ++i) CHECK(is(rq.one_d[i], 2 * i, 2 * i + 1, 1, 1));
        for (unsigned j = 0; j < 9; ++j) CHECK(is(rq.two_d[j], 22 + 4 * j, 24 + 4 * j, 1, 2));
    }
    { CASE("stratified whitted"); CHECK(planned(desc(RT_INTEGRATOR_WHITTED), large_scene()).lhs_total == 4); }
    { CASE("stratified direct one"); CHECK(planned(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE), large_scene()).lhs_total == 16); }
    {   CASE("stratified bidirectional"); const Requests rq = planned(desc(RT_INTEGRATOR_BIDIRECTIONAL), large_scene());
        CHECK(rq.lhs_total == 110 && rq.n1d == 2 && rq.n2d == 0 && is(rq.one_d[0], 34, 35, 1, 1) && is(rq.one_d[1], 36, 37, 1, 1)); }
    {   CASE("random path"); const Requests rq = planned(desc(RT_INTEGRATOR_PATH, 0, RT_SAMPLER_RANDOM), large_scene());
        CHECK(rq.lhs_total == 29 && rq.pixgen_draws == 5 * 4);
        for (unsigned i = 0; i < 11; ++i) CHECK(is(rq.one_d[i], i, 0, 1, 1));
        for (unsigned j = 0; j < 9; ++j) CHECK(is(rq.two_d[j], 11 + 2 * j, 0, 1, 2)); }
    for (int ps : {3, 4, 16, 1}) {
        CASE("lowdiscrepancy path, pixelsamples " + std::to_string(ps)); RtRenderDesc rd = desc(RT_INTEGRATOR_PATH, 0, RT_SAMPLER_LOWDISCREPANCY); rd.pixel_samples = ps;
        int spp = 0; const Requests rq = planned(rd, large_scene(), &spp);
        const unsigned P = ps == 3 ? 4u : unsigned(ps);
        CHECK(unsigned(spp) == P && rq.lhs_total == 0 && rq.one_d[0].f_base == 5 + 6 * P);
        CHECK(rq.one_d[1].f_base == 5 + 6 * P + (1 + 2 * P));                      // one scramble, P values, P shuffles
        CHECK(rq.pixgen_draws == 5 + 6 * P + 11 * (1 + 2 * P) + 9 * (2 + 2 * P));  // the running total
    }
    {   CASE("direct all, lights of 1, 3 and 16 samples, stratified");
        const Requests rq = planned(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL), with_lights({1, 3, 16}));
        CHECK(rq.table.size() == 10 && rq.dims_max_n == 16 && rq.lhs_total == 204 && rq.n1d == 2 && rq.n2d == 0);
        if (rq.table.size() == 10) {
            // 1-D requests first (bases 0, 2, 8, then the volume integrator's at 40 and 42), then the lights' pairs of 2-D requests from 44
            CHECK(is(rq.table[0], 44, 46, 1, 2) && is(rq.table[1], 48, 50, 1, 2) && is(rq.table[2], 0, 1, 1, 1));
            CHECK(is(rq.table[3], 52, 58, 3, 2) && is(rq.table[4], 64, 70, 3, 2) && is(rq.table[5], 2, 5, 3, 1));
            CHECK(is(rq.table[6], 76, 108, 16, 2) && is(rq.table[7], 140, 172, 16, 2) && is(rq.table[8], 8, 24, 16, 1));
            CHECK(is(rq.table[9], 0, 0, 0, 0));
        }
        CHECK(is(rq.one_d[0], 40, 41, 1, 1) && is(rq.one_d[1], 42, 43, 1, 1));
    }
    {   CASE("direct all, lights of 1, 3 and 16 samples, lowdiscrepancy: RoundSize");
        const Requests rq = planned(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, RT_SAMPLER_LOWDISCREPANCY), with_lights({1, 3, 16}));
        CHECK(rq.table.size() == 10 && rq.dims_max_n == 16);
        if (rq.table.size() == 10) {
            CHECK(rq.table[3].n == 4 && rq.table[4].n == 4 && rq.table[5].n == 4 && rq.table[0].n == 1 && rq.table[6].n == 16);
            for (int i = 0; i < 3; ++i) CHECK(rq.table[3 * i].dims == 2 && rq.table[3 * i + 1].dims == 2 && rq.table[3 * i + 2].dims == 1);
            CHECK(rq.table[2].f_base == 5 + 6 * 4 && rq.table[5].f_base == 29 + (1 + 4 + 4) && rq.table[8].f_base == 38 + (1 + 16 + 4));     // P = 4
        }
    }
    {   CASE("direct all without lights"); const Requests rq = planned(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL), with_lights({}));
        CHECK(rq.table.size() == 1 && rq.dims_max_n == 0 && rq.lhs_total == 4); }
    for (int ns : {65535, 65536}) {
        CASE("a light of " + std::to_string(ns) + " samples"); RtRenderDesc rd = desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL);
        Requests rq; const Refusal r = plan_requests(rd, with_lights({ns}), 4, rq);
        if (ns == 65535) CHECK(!r && rq.dims_max_n == 65535);
        else CHECK(r.code == RT_EINVAL && std::string(r.msg) == "rt_render: more than 65535 samples per light (the sample table holds counts in 16 bits)");
    }
    {   CASE("32769 samples round up to 65536 under lowdiscrepancy"); Requests rq;
        CHECK(plan_requests(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, RT_SAMPLER_LOWDISCREPANCY), with_lights({32769}), 4, rq).code == RT_EINVAL);
        CHECK(!plan_requests(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL, RT_SAMPLER_LOWDISCREPANCY), with_lights({32768}), 4, rq)); }
    // the 2^30 draw limit: a camera sample of P = 1 addresses (P + 1) * (2 * sum n1 + 4 * sum n2) = 2 * (10 S + 4) draws for lights of S samples together;
    // 20 S + 8 > 2^30 - 1 from S = 53 687 091 on: 819 lights of 65535 and one of 13 926 (refused) or 13 925 (accepted)
    for (int last : {13925, 13926}) {
        CASE("the 2^30 draw limit, last light " + std::to_string(last)); RtRenderDesc rd = desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL); rd.x_samples = rd.y_samples = 1;
        std::vector<int> ns(819, 65535); ns.push_back(last);
        Requests rq; const Refusal r = plan_requests(rd, with_lights(ns), 1, rq);
        if (last == 13925) CHECK(!r && rq.table.size() == 3 * 820 + 1);
        else CHECK(r.code == RT_EINVAL && std::string(r.msg) == "rt_render: the lights' sample requests need more than 2^30 random numbers per camera sample");
    }
    {   CASE("unknown integrator"); Requests rq; CHECK(std::string(plan_requests(desc(7), large_scene(), 4, rq).msg) == "unknown integrator"); }
    // ---- the BidirTable's sphere: BBox::BoundingSphere (geometry.cpp:47-50) of [0,0,0] - [2,4,4] is centre (1,2,2), radius |(1,2,2)| = 3
    for (int inverted : {0, 1}) {
        CASE(inverted ? "bidirectional, inverted world bound" : "bidirectional, world sphere"); SceneFacts sf = large_scene();
        if (inverted) { const float b[6] = {2, 4, 4, 0, 0, 0}; std::memcpy(sf.bounds, b, sizeof b); }
        const Requests rq = planned(desc(RT_INTEGRATOR_BIDIRECTIONAL), sf);
        BidirTable bt; std::memset(&bt, 0, sizeof bt);
        if (rq.table.size() * sizeof(DimReq) >= sizeof bt) std::memcpy(&bt, rq.table.data(), sizeof bt);
        CHECK(bt.wc[0] == 1.f && bt.wc[1] == 2.f && bt.wc[2] == 2.f && bt.wr == (inverted ? 0.f : 3.f));
    }
}

// ---------------------------------------------------------------------------------------------- extent
static void test_extent() {
    const int two_d = -(8 | (4 << 16));
    for (int tile : {1, 64, two_d}) {                     // 17 x 13 = 221 pixels of 4 samples
        CASE("shards add up, tile " + std::to_string(tile));
        const unsigned long long n_tiles = tile == 1 ? 221 : tile == 64 ? 4 : 3 * 4, tile_pixels = tile == 1 ? 1 : tile == 64 ? 64 : 32;
        for (int shards : {1, 3, 5}) {
            unsigned long long sum = 0;
            for (int k = 0; k < shards; ++k) {
                RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); rd.tile_pixels = tile; rd.shard_count = shards; rd.shard_index = k;
                Extent e; CHECK(!plan_extent(rd, e));
                CHECK(e.spp == 4 && e.total_pixels == 221 && e.shard_index == k && e.shard_count == shards && (unsigned long long)e.tile_pixels == tile_pixels);
                if (tile < 0) CHECK(e.tile_w == 8 && e.tile_h == 4 && e.tiles_x == 3); else CHECK(e.tile_w == 0 && e.tile_h == 0 && e.tiles_x == 0);
                CHECK(e.total_work % (tile_pixels * 4) == 0);
                sum += e.total_work;
            }
            CHECK(sum == n_tiles * tile_pixels * 4);
        }
    }
    {   CASE("a shard beyond the tiles"); RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); rd.x_end = 2; rd.y_end = 1; rd.tile_pixels = 64; rd.shard_count = 3;
        Extent e; rd.shard_index = 0; CHECK(!plan_extent(rd, e) && e.total_work == 64 * 4);
        rd.shard_index = 1; CHECK(!plan_extent(rd, e) && e.total_work == 0);
        rd.shard_index = 2; CHECK(!plan_extent(rd, e) && e.total_work == 0); }
    {   CASE("shard_count < 1 is one shard, tile_pixels 0 is 1"); RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); rd.shard_count = 0; rd.tile_pixels = 0;
        Extent e; CHECK(!plan_extent(rd, e) && e.shard_count == 1 && e.tile_pixels == 1 && e.total_work == 221 * 4); }
    auto refused = [](const RtRenderDesc &rd, const char *msg) { Extent e; const Refusal r = plan_extent(rd, e); return r.code == RT_EINVAL && std::string(r.msg) == msg; };
    {   CASE("2-D tile bounds"); RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); Extent e;
        rd.tile_pixels = -(4096 | (4096 << 16)); CHECK(!plan_extent(rd, e) && e.tile_w == 4096 && e.tile_h == 4096 && e.tile_pixels == 4096 * 4096 && e.tiles_x == 1);
        rd.tile_pixels = -(4097 | (1 << 16)); CHECK(refused(rd, "bad 2-D tile size"));
        rd.tile_pixels = -(1 | (4097 << 16)); CHECK(refused(rd, "bad 2-D tile size"));
        rd.tile_pixels = -8; CHECK(refused(rd, "bad 2-D tile size"));                       // height 0
        rd.tile_pixels = -(5 << 16); CHECK(refused(rd, "bad 2-D tile size")); }            // width 0
    {   CASE("refusals in order"); RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED);
        rd.sampler = 3; rd.x_end = 0; CHECK(refused(rd, "unknown sampler"));
        rd.sampler = RT_SAMPLER_STRATIFIED; rd.x_samples = 0; CHECK(refused(rd, "bad xsamples/ysamples"));
        rd.sampler = RT_SAMPLER_LOWDISCREPANCY; rd.pixel_samples = 0; CHECK(refused(rd, "bad pixelsamples"));
        rd.pixel_samples = 1; rd.shard_index = 1; CHECK(refused(rd, "empty sample extent"));
        rd.x_end = 17; CHECK(refused(rd, "bad shard index"));
        rd.shard_index = -1; rd.shard_count = 4; CHECK(refused(rd, "bad shard index")); }
    {   // 2^32 - 1 = 65535 * 65537 samples is the last frame accepted, 2^32 = 65536 * 65536 the first refused
        CASE("2^32 camera samples"); RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); rd.x_samples = rd.y_samples = 1; Extent e;
        rd.x_end = 65537; rd.y_end = 65535; CHECK(!plan_extent(rd, e) && e.total_pixels == 0xFFFFFFFFull && e.total_work == 0xFFFFFFFFull);
        rd.x_end = 65536; rd.y_end = 65536; CHECK(refused(rd, "more than 2^32 camera samples per frame"));
        // ... with border tiles: 1 x 1 tiles pad nothing (accepted), 2 x 1 tiles pad the 65537 columns to 65538 (refused)
        rd.x_end = 65537; rd.y_end = 65535;
        rd.tile_pixels = -(1 | (1 << 16)); CHECK(!plan_extent(rd, e) && e.total_work == 0xFFFFFFFFull && e.tiles_x == 65537);
        rd.tile_pixels = -(2 | (1 << 16)); CHECK(refused(rd, "more than 2^32 camera samples per frame (2-D tiles, border tiles included)")); }
}

// ---------------------------------------------------------------------------------------------- schedule
static Schedule scheduled(const RtRenderDesc &rd, const SceneFacts &sf, const FrameKnobs &kn = FrameKnobs{}) {
    Extent e; Requests rq;
    CHECK(!plan_extent(rd, e)); CHECK(!plan_requests(rd, sf, e.spp, rq));
    return plan_schedule(rd, sf, e, rq, kn);
}
static bool same_extent(const Extent &a, const Extent &b) {
    return a.spp == b.spp && a.shard_index == b.shard_index && a.shard_count == b.shard_count && a.tile_pixels == b.tile_pixels && a.tile_w == b.tile_w &&
           a.tile_h == b.tile_h && a.tiles_x == b.tiles_x && a.total_pixels == b.total_pixels && a.total_work == b.total_work;
}
// the fields of `b` that differ from `a`, by name
static std::string moved(const Schedule &a, const Schedule &b) {
    std::string s;
#define FIELD(f) if (a.f != b.f) s += #f " ";
    FIELD(trav_mode) FIELD(exit_thresh) FIELD(high_occupancy) FIELD(leaf_min) FIELD(xcd_bands) FIELD(phase_sync) FIELD(pipeline) FIELD(mega_tile)
    FIELD(dbg_x) FIELD(dbg_y) FIELD(fixed_frame) FIELD(by_vertex)
#undef FIELD
    if (!same_extent(a.extent, b.extent)) s += "extent ";
    return s;
}

// Whitted, DirectLighting "all" / "one" and Path under the stratified sampler: the frames the fixed kernels were compiled for (rt_fixed_frame.h)
static bool headline_frame(int integ, int strategy, int sampler) {
    return sampler == RT_SAMPLER_STRATIFIED && integ >= RT_INTEGRATOR_WHITTED && integ <= RT_INTEGRATOR_PATH && !(integ == RT_INTEGRATOR_DIRECT && strategy == RT_STRATEGY_WEIGHTED);
}

static void test_schedule() {
    const SceneFacts large = large_scene(), tiny = tiny_fat();
    SceneFacts medium = large; medium.medium = true;
    {   CASE("tiny-fat whitted"); const Schedule s = scheduled(desc(RT_INTEGRATOR_WHITTED), tiny);
        CHECK(s.trav_mode == 3 && s.exit_thresh == 0 && s.high_occupancy == 0 && s.leaf_min == 8 && s.phase_sync == 1 && s.xcd_bands == 1 && !s.pipeline && !s.fixed_frame); }
    {   CASE("tiny-fat direct"); const Schedule s = scheduled(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE), tiny);
        CHECK(s.trav_mode == 3 && s.exit_thresh == 0 && s.high_occupancy == 0 && s.leaf_min == 8 && s.phase_sync == 1); }
    {   CASE("tiny path"); SceneFacts ext = tiny; ext.has_ext = true; SceneFacts vol = tiny; vol.medium = true;
        const Schedule byv = scheduled(desc(RT_INTEGRATOR_PATH), tiny), e = scheduled(desc(RT_INTEGRATOR_PATH), ext), v = scheduled(desc(RT_INTEGRATOR_PATH), vol);
        CHECK(byv.trav_mode == 2 && byv.high_occupancy == 1 && byv.exit_thresh == (RT_MEGA_BYV ? 16 : 8) && byv.leaf_min == 8 && byv.phase_sync == 1 && byv.xcd_bands == 0);
        CHECK(e.trav_mode == 2 && e.high_occupancy == 1 && e.exit_thresh == 8);
        CHECK(v.trav_mode == 2 && v.high_occupancy == 1 && v.exit_thresh == 8 && !v.pipeline); }              // a tiny tree stays on the megakernel
    for (int integ : {int(RT_INTEGRATOR_WHITTED), int(RT_INTEGRATOR_DIRECT), int(RT_INTEGRATOR_PATH)}) {
        CASE("large tree, integrator " + std::to_string(integ)); const Schedule s = scheduled(desc(integ), large);
        CHECK(s.trav_mode == 2 && s.exit_thresh == 32 && s.leaf_min == RT_TRACE_LEAF_MIN && s.high_occupancy == 1 && s.phase_sync == 0 && !s.pipeline);
        CHECK(s.xcd_bands == (integ == RT_INTEGRATOR_PATH ? 0 : 1)); }
    {   CASE("tiny needs both: <= 4096 nodes and >= 1.5 per leaf"); SceneFacts thin = tiny; thin.per_leaf = 1.49; SceneFacts big = tiny; big.n_nodes = 4097;
        CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), thin).trav_mode == 2 && scheduled(desc(RT_INTEGRATOR_WHITTED), thin).exit_thresh == 32);
        CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), big).trav_mode == 2 && scheduled(desc(RT_INTEGRATOR_WHITTED), big).leaf_min == RT_TRACE_LEAF_MIN); }
    {   CASE("the pipeline: a large tree with a medium only");
        CHECK(scheduled(desc(RT_INTEGRATOR_PATH), medium).pipeline == 1 && !scheduled(desc(RT_INTEGRATOR_PATH), medium).by_vertex);
        CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), medium).pipeline == 1);
        SceneFacts tv = tiny; tv.medium = true; CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), tv).pipeline == 0);
        CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), large).pipeline == 0); }
    // ---- the one-shard reset
    {   CASE("one shard, megakernel: scanline order in 32-pixel blocks"); RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); rd.tile_pixels = -(8 | (4 << 16));
        const Schedule s = scheduled(rd, large);
        CHECK(s.extent.tile_w == 0 && s.extent.tile_h == 0 && s.extent.tiles_x == 0 && s.extent.tile_pixels == 1 && s.extent.total_work == 221 * 4 && s.mega_tile == 32);
        rd.shard_count = 3; const Schedule t = scheduled(rd, large);                       // three shards keep the caller's tiles
        CHECK(t.extent.tile_w == 8 && t.extent.tile_h == 4 && t.extent.tile_pixels == 32 && t.extent.total_work == 4 * 32 * 4 && t.mega_tile == 0);
        rd.shard_count = 1; const Schedule p = scheduled(rd, medium);                      // ... and so does the queue pipeline
        CHECK(p.pipeline == 1 && p.extent.tile_w == 8 && p.extent.tile_pixels == 32 && p.extent.total_work == 12 * 32 * 4 && p.mega_tile == 0); }
    {   CASE("mega_tile falls to 0 above 4096 and from 2^32 samples on"); FrameKnobs kn;
        kn.mega_tile = 4096; CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), large, kn).mega_tile == 4096);
        kn.mega_tile = 4097; CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), large, kn).mega_tile == 0);
        kn.mega_tile = -5; CHECK(scheduled(desc(RT_INTEGRATOR_WHITTED), large, kn).mega_tile == 0);
        const RtRenderDesc rd = desc(RT_INTEGRATOR_WHITTED); Extent e; Requests rq; CHECK(!plan_extent(rd, e)); CHECK(!plan_requests(rd, large, e.spp, rq));
        e.spp = 1; e.total_pixels = 0xFFFFFFFFull; CHECK(plan_schedule(rd, large, e, rq, FrameKnobs{}).mega_tile == 32);
        e.total_pixels = 0x100000000ull; CHECK(plan_schedule(rd, large, e, rq, FrameKnobs{}).mega_tile == 0); }
    // ---- each knob alone moves its own field and nothing else (counting scene: no frame is a fixed frame unless the case is about that)
    SceneFacts counted = large; counted.counting = true;
    SceneFacts tiny_counted = tiny; tiny_counted.counting = true;
    const RtRenderDesc whitted = desc(RT_INTEGRATOR_WHITTED);
    RtRenderDesc sharded = whitted; sharded.shard_count = 3;
    const Schedule base = scheduled(whitted, counted), base_tiny = scheduled(whitted, tiny), base3 = scheduled(sharded, counted);
#define KNOB(WHAT, RD, SF, BASE, SET, FIELDS, ...) { CASE(WHAT); FrameKnobs kn; SET; const Schedule s = scheduled(RD, SF, kn); CHECK(moved(BASE, s) == FIELDS); CHECK(__VA_ARGS__); }
    KNOB("HIGH_OCC=0", whitted, counted, base, kn.high_occ = 0, "high_occupancy ", s.high_occupancy == 0)
    KNOB("HIGH_OCC=1", whitted, tiny_counted, scheduled(whitted, tiny_counted), kn.high_occ = 1, "trav_mode high_occupancy ", s.high_occupancy == 1 && s.trav_mode == 2)     // (with its rule: no pooled rounds at high occupancy)
    KNOB("LEAF_MIN=5", whitted, counted, base, kn.leaf_min = 5, "leaf_min ", s.leaf_min == 5)
    KNOB("LEAF_MIN=0", whitted, counted, base, kn.leaf_min = 0, "leaf_min ", s.leaf_min == 1)
    KNOB("TRAV_MODE=2", whitted, tiny, base_tiny, kn.trav_mode = 2, "trav_mode ", s.trav_mode == 2)
    KNOB("TRAV_MODE=3, tiny", whitted, tiny, base_tiny, kn.trav_mode = 3, "", s.trav_mode == 3)
    KNOB("XCD_BANDS=0", whitted, counted, base, kn.xcd_bands = 0, "xcd_bands ", s.xcd_bands == 0)
    KNOB("XCD_BANDS=7", desc(RT_INTEGRATOR_PATH), counted, scheduled(desc(RT_INTEGRATOR_PATH), counted), kn.xcd_bands = 7, "xcd_bands ", s.xcd_bands == 1)
    KNOB("EXIT_THRESH=5", whitted, counted, base, kn.exit_thresh = 5, "exit_thresh ", s.exit_thresh == 5)
    KNOB("EXIT_THRESH=0", whitted, counted, base, kn.exit_thresh = 0, "exit_thresh ", s.exit_thresh == 0)
    KNOB("PHASE_SYNC=1", whitted, counted, base, kn.phase_sync = 1, "phase_sync ", s.phase_sync == 1)
    KNOB("PHASE_SYNC=0", whitted, tiny, base_tiny, kn.phase_sync = 0, "phase_sync ", s.phase_sync == 0)
    KNOB("PIPELINE=1", sharded, counted, base3, kn.pipeline = 1, "pipeline ", s.pipeline == 1)
    KNOB("PIPELINE=0", sharded, medium, scheduled(sharded, medium), kn.pipeline = 0, "pipeline ", s.pipeline == 0)
    KNOB("MEGA_TILE=16", whitted, counted, base, kn.mega_tile = 16, "mega_tile ", s.mega_tile == 16)
    KNOB("MEGA_TILE=0", whitted, counted, base, kn.mega_tile = 0, "mega_tile ", s.mega_tile == 0)
    KNOB("DEBUG_PIXEL", whitted, counted, base, (kn.dbg_x = 3, kn.dbg_y = 9), "dbg_x dbg_y ", s.dbg_x == 3 && s.dbg_y == 9)
    KNOB("FIXED_FRAME=0", whitted, large, scheduled(whitted, large), kn.fixed_frame = 0, "fixed_frame ", !s.fixed_frame)
    KNOB("FIXED_FRAME=1 on a qualifying frame", whitted, large, scheduled(whitted, large), kn.fixed_frame = 1, "", s.fixed_frame)
    KNOB("FIXED_FRAME=1 cannot turn it on", whitted, counted, base, kn.fixed_frame = 1, "", !s.fixed_frame)
    {   FrameKnobs piped; piped.pipeline = 1; const RtRenderDesc path = desc(RT_INTEGRATOR_PATH); const Schedule bp = scheduled(path, counted, piped);
        CASE("a path in the pipeline without a medium is by vertex"); CHECK(bp.pipeline == 1 && bp.by_vertex);
        KNOB("PIPE_VERTEX=0", path, counted, bp, (kn.pipeline = 1, kn.pipe_vertex = 0), "by_vertex ", !s.by_vertex)
        KNOB("PIPE_VERTEX=1", path, counted, bp, (kn.pipeline = 1, kn.pipe_vertex = 1), "", s.by_vertex)
        KNOB("PIPE_VERTEX=1 cannot turn it on", path, medium, scheduled(path, medium), kn.pipe_vertex = 1, "", s.pipeline == 1 && !s.by_vertex) }
    KNOB("PIPE_MEM_MB, PIPE_SLOTS, DEBUG_NOFILM are not the schedule's", whitted, counted, base, (kn.pipe_mem_mb = 64, kn.pipe_slots = 1024, kn.debug_nofilm = 1), "", true)
    // ---- the rules that hold whatever the knobs say
    FrameKnobs piped; piped.pipeline = 1;
    for (int depth : {250, 251, -1}) {
        CASE("PIPELINE=1, maxdepth " + std::to_string(depth)); RtRenderDesc rd = sharded; rd.max_depth = depth;
        CHECK(scheduled(rd, counted, piped).pipeline == (depth == 250 ? 1 : 0)); }
    for (int ns : {65534, 65535}) {
        CASE("PIPELINE=1, a light of " + std::to_string(ns) + " samples"); RtRenderDesc rd = desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ALL); rd.shard_count = 3;
        SceneFacts sf = with_lights({ns}); sf.counting = true;
        CHECK(scheduled(rd, sf, piped).pipeline == (ns == 65534 ? 1 : 0)); }
    for (unsigned nl : {65534u, 65535u}) {
        CASE("PIPELINE=1, " + std::to_string(nl) + " lights"); SceneFacts sf = counted; sf.n_lights = nl; sf.light_samples.assign(nl, 1);
        CHECK(scheduled(sharded, sf, piped).pipeline == (nl == 65534u ? 1 : 0)); }
    {   CASE("PIPELINE=1, weighted"); CHECK(scheduled(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_WEIGHTED), medium, piped).pipeline == 0);
        CHECK(scheduled(desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE), medium, piped).pipeline == 1); }
    {   CASE("bidirectional: no pipeline, no bands"); FrameKnobs kn; kn.pipeline = 1; kn.xcd_bands = 1;
        const Schedule s = scheduled(desc(RT_INTEGRATOR_BIDIRECTIONAL), large, kn); CHECK(s.pipeline == 0 && s.xcd_bands == 0 && !s.fixed_frame && !s.by_vertex); }
    {   CASE("debug: no pipeline, natural allocation"); FrameKnobs kn; kn.pipeline = 1; kn.high_occ = 1;
        const Schedule s = scheduled(desc(RT_INTEGRATOR_DEBUG), medium, kn); CHECK(s.pipeline == 0 && s.high_occupancy == 0 && !s.fixed_frame);
        const Schedule t = scheduled(desc(RT_INTEGRATOR_DEBUG), tiny); CHECK(t.trav_mode == 3 && t.high_occupancy == 0); }
    {   CASE("trav_mode 3 at high occupancy falls to 2"); FrameKnobs kn; kn.trav_mode = 3;
        CHECK(scheduled(whitted, large, kn).trav_mode == 2);
        kn.high_occ = 0; CHECK(scheduled(whitted, large, kn).trav_mode == 3);
        FrameKnobs other; other.trav_mode = 1; CHECK(scheduled(whitted, tiny, other).trav_mode == 2); }
    // ---- the fixed frame: fixed::qualifies on the planned frame
    for (const Combo &c : combos())
    for (int sampler : {int(RT_SAMPLER_STRATIFIED), int(RT_SAMPLER_RANDOM)})
    for (int variant = 0; variant < 8; ++variant) {
        CASE(std::string("fixed frame: ") + c.name + " sampler " + std::to_string(sampler) + " variant " + std::to_string(variant));
        SceneFacts sf = variant == 1 ? tiny : large;
        RtRenderDesc rd = desc(c.integ, c.strategy, sampler);
        if (variant == 2) sf.counting = true;
        if (variant == 3) sf.has_ext = true;
        if (variant == 4) sf.lens_radius = .1f;
        if (variant == 5) sf.camera_type = RT_CAMERA_ENVIRONMENT;
        if (variant == 6) rd.shard_count = 2;
        if (variant == 7) { sf.n_lights = 2; sf.light_samples = {1, 4}; }
        const Schedule s = scheduled(rd, sf);
        const bool weighted = c.integ == RT_INTEGRATOR_DIRECT && c.strategy == RT_STRATEGY_WEIGHTED, all = c.integ == RT_INTEGRATOR_DIRECT && c.strategy == RT_STRATEGY_ALL;
        const int max_n = (c.n2.empty() ? 0 : (variant == 7 && all) ? 4 : 1);
        CHECK(s.fixed_frame == fixed::qualifies(fixed::Facts{c.integ, sampler, weighted, sf.lens_radius, sf.camera_type, rd.shard_count, s.mega_tile, max_n,
                                                             sf.counting, sf.has_ext, sf.medium, s.high_occupancy != 0}));
        if (variant == 0) CHECK(s.fixed_frame == headline_frame(c.integ, c.strategy, sampler));
        if (variant == 7 && all) CHECK(!s.fixed_frame);
        if (variant >= 2 && variant <= 6) CHECK(!s.fixed_frame);
        if (variant == 1) CHECK(s.fixed_frame == (headline_frame(c.integ, c.strategy, sampler) && c.integ == RT_INTEGRATOR_PATH));     // a tiny tree: only its path frames run at high occupancy
    }
}

// ---------------------------------------------------------------------------------------------- march bounds
static void test_march() {
    const float below_one = std::nextafter(1.f, 0.f);
    auto refused = [](const RtRenderDesc &rd, const SceneFacts &sf, const char *msg) { March m; const Refusal r = plan_march(rd, sf, m); return r.code == RT_EINVAL && std::string(r.msg) == msg; };
    const char *too_many = "rt_render: stepsize too small for the medium (more than 65536 march steps)";
    const char *too_many_taus = "rt_render: stepsize too small for the density region (an optical-depth march would take more than 2^20 samples)";
    const char *no_advance = "rt_render: stepsize too small for the density region: at the scene's ray parameters t + .5 * stepsize == t, the optical-depth march would not advance";
    SceneFacts homog = large_scene(); homog.medium = true; homog.vol_p1[0] = 65534.f;       // the extent's diagonal is 65534
    {   CASE("no medium"); March m; m.vol_nmax = 7; RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); rd.step_size = -1.f;
        CHECK(!plan_march(rd, large_scene(), m) && m.vol_nmax == 0 && m.dens_cap == 0); }
    {   CASE("65536 march steps"); RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); March m;
        CHECK(!plan_march(rd, homog, m) && m.vol_nmax == 65536 && m.dens_cap == 0);         // ceil(65534 / 1) + 2
        rd.step_size = below_one; CHECK(refused(rd, homog, too_many)); }
    {   CASE("stepsize and volume integrator"); RtRenderDesc rd = desc(RT_INTEGRATOR_PATH);
        rd.step_size = 0.f; CHECK(refused(rd, homog, "rt_render: volume integrator stepsize must be positive"));
        rd.step_size = std::nanf(""); rd.volume_integrator = 9; CHECK(refused(rd, homog, "rt_render: volume integrator stepsize must be positive"));
        rd.step_size = 1.f; CHECK(refused(rd, homog, "rt_render: unknown volume integrator"));
        rd.volume_integrator = RT_VOLUME_SINGLE; March m; CHECK(!plan_march(rd, homog, m)); }
    SceneFacts region = large_scene(); region.medium = true; region.density_kind = RT_DENSITY_EXPONENTIAL; region.vol_p1[0] = 1.f;
    {   CASE("a density region: dens_cap and the world diagonal's march steps"); SceneFacts sf = region; sf.vol_world[3] = 10.; RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); rd.step_size = .5f;
        March m; CHECK(!plan_march(rd, sf, m) && m.dens_cap == 40 + 2 && m.vol_nmax == 20 + 2); }      // 10 / .25 optical-depth samples, 10 / .5 steps (the extent's own: 2 + 2)
    {   // 2^20 optical-depth samples: a world diagonal of 2^19 - 1 at stepsize 1 takes (2^19 - 1) / .5 + 2 = 2^20, which that bound lets pass (the march-step
        // bound then refuses the frame: 2^19 + 1 steps); the next smaller stepsize takes one more
        CASE("2^20 optical-depth samples"); SceneFacts sf = region; sf.vol_world[3] = 524287.; RtRenderDesc rd = desc(RT_INTEGRATOR_PATH);
        CHECK(refused(rd, sf, too_many));
        rd.step_size = below_one; CHECK(refused(rd, sf, too_many_taus)); }
    {   // floats at 2^24 + 2 are 2 apart: adding 1 is a tie that rounds to the even neighbour above, adding less than 1 changes nothing
        CASE("t + .5 * stepsize == t"); SceneFacts sf = region; sf.vol_world[3] = 1.; sf.bounds[3] = 16777216.f; sf.bounds[4] = sf.bounds[5] = 0.f;
        RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); March m;
        rd.step_size = 2.f; CHECK(!plan_march(rd, sf, m) && m.dens_cap == 1 + 2);
        rd.step_size = std::nextafter(2.f, 0.f); CHECK(refused(rd, sf, no_advance));
        // the camera position counts, an inverted (empty) scene bound does not
        SceneFacts cam = region; cam.vol_world[3] = 1.; cam.bounds[3] = cam.bounds[4] = cam.bounds[5] = 0.f; cam.cam_pos[1] = -16777216.;
        CHECK(refused(rd, cam, no_advance));
        SceneFacts inv = cam; inv.cam_pos[1] = 0.; const float b[6] = {16777216.f, 0, 0, -16777216.f, 0, 0}; std::memcpy(inv.bounds, b, sizeof b);
        CHECK(!plan_march(rd, inv, m));
        const float c[6] = {-16777216.f, 0, 0, 16777216.f, 0, 0}; std::memcpy(inv.bounds, c, sizeof c);
        CHECK(refused(rd, inv, no_advance)); }
}

// ---------------------------------------------------------------------------------------------- the launch
// What a frame launches, as a table: the first row whose condition holds names the family (a query runs the radiance kernels; the queue
// pipeline where the schedule says so; the bidirectional integrator, DirectLighting "weighted" and the debug integrator have a family each; a qualifying
// frame takes the scene twin where the integrator has one and the scene has one light, else the fixed-frame twin; everything else the generic megakernel)
struct LaunchCase { RtRenderDesc rd; SceneFacts sf; Schedule sc; bool query; };
static bool lc_weighted(const LaunchCase &c) { return c.rd.integrator == RT_INTEGRATOR_DIRECT && c.rd.strategy == RT_STRATEGY_WEIGHTED; }
static bool lc_scene_twin(const LaunchCase &c) {
    return c.sc.fixed_frame && (c.rd.integrator == RT_INTEGRATOR_DIRECT || c.rd.integrator == RT_INTEGRATOR_PATH) && c.sf.n_lights == 1u && c.sf.scene_twins;
}
struct LaunchRule { Launch::Family family; bool (*holds)(const LaunchCase &); };
static const LaunchRule launch_rules[] = {
    {Launch::Rays, [](const LaunchCase &c) { return c.query; }},
    {Launch::Pipeline, [](const LaunchCase &c) { return c.sc.pipeline != 0; }},
    {Launch::Bidir, [](const LaunchCase &c) { return c.rd.integrator == RT_INTEGRATOR_BIDIRECTIONAL; }},
    {Launch::Weighted, lc_weighted},
    {Launch::Debug, [](const LaunchCase &c) { return c.rd.integrator == RT_INTEGRATOR_DEBUG; }},
    {Launch::FixedScene, lc_scene_twin},
    {Launch::Fixed, [](const LaunchCase &c) { return c.sc.fixed_frame; }},
    {Launch::Mega, [](const LaunchCase &) { return true; }},
};
// the one entry k of a family's N whose flavour (and what else the family's entries differ by) `serves` accepts; -1 when none or several do
template <class Serves> static int only_entry(int n, Serves serves) {
    int found = -1;
    for (int k = 0; k < n; ++k) if (serves(k)) { if (found >= 0) return -1; found = k; }
    return found;
}
// ... for the request of a case: the entry counts exactly when the scene counts, is built for its accelerator and medium, and carries the EXT code when the
// scene needs it.  Mega has more than one such entry: of those, the one with EXT exactly when the frame counts (a counting twin always carries it) or needs
// it, and the high-occupancy flavour exactly when a timed frame without EXT asks for it
static bool serves(const flavour::Flavour &f, const LaunchCase &c, bool has_vol = true) {
    return f.count == c.sf.counting && f.accel == c.sf.accel_kind && (!has_vol || f.vol == c.sf.medium) && (f.ext || !c.sf.has_ext);
}
static int expected_entry(Launch::Family family, const LaunchCase &c, int axes) {
    const int integ = c.rd.integrator;
    const bool want_high = c.sc.high_occupancy != 0 && !c.sf.counting && !c.sf.has_ext;
    switch (family) {
    case Launch::Mega: return only_entry(flavour::Mega::N, [&](int k) { const flavour::Flavour f = flavour::Mega::flavour(k, integ); return serves(f, c) && f.ext == (c.sf.counting || c.sf.has_ext) && f.high_occ == want_high; });
    case Launch::Fixed: return only_entry(flavour::Fixed::N, [&](int k) { return serves(flavour::Fixed::flavour(k), c) && flavour::Fixed::integrator(k) == integ; });
    case Launch::FixedScene: return only_entry(flavour::FixedScene::N, [&](int k) { return serves(flavour::FixedScene::flavour(k), c) && flavour::FixedScene::axes(k) == axes; });
    case Launch::Debug: return only_entry(flavour::Debug::N, [&](int k) { return serves(flavour::Debug::flavour(k), c); });
    case Launch::Weighted: return only_entry(flavour::Weighted::N, [&](int k) { return serves(flavour::Weighted::flavour(k), c); });
    case Launch::Bidir: return only_entry(flavour::Bidir::N, [&](int k) { return serves(flavour::Bidir::flavour(k), c, false); });      // (a medium is refused before the launch)
    case Launch::Rays: return only_entry(flavour::Rays::N, [&](int k) { return serves(flavour::Rays::flavour(k, integ), c); });
    case Launch::Pipeline: return 0;
    }
    return -1;
}
static void check_launch(const LaunchCase &c) {
    const Launch ln = plan_launch(c.rd, c.sf, c.sc, c.query);
    Launch::Family family = Launch::Mega;
    for (const LaunchRule &r : launch_rules) if (r.holds(c)) { family = r.family; break; }
    const int axes = family == Launch::FixedScene ? (fixed::SCENE_ONE_LIGHT | (c.sf.specular_materials ? 0 : fixed::SCENE_NO_SPECULAR)) : 0;
    CHECK(ln.family == family);
    CHECK(ln.integ == c.rd.integrator);
    CHECK(ln.scene_axes == axes);
    const int k = expected_entry(family, c, axes);
    CHECK(k >= 0);
    CHECK(ln.k == k);
    // a fixed-frame kernel is timed, without EXT, without a medium and at high occupancy: plan_schedule admits no other frame to it
    if (family == Launch::Fixed || family == Launch::FixedScene) CHECK(!c.sf.counting && !c.sf.has_ext && !c.sf.medium && c.sc.high_occupancy != 0);
}

static void test_launch() {
    const std::optional<int> unset, off(0), on(1);
    for (const Combo &c : combos())
    for (int scene = 0; scene < 3; ++scene) {
        CASE(std::string("launch: ") + c.name + (scene == 0 ? ", large scene" : scene == 1 ? ", tiny scene" : ", large scene with a medium"));
        const std::string what = g_what;
        const bool weighted = c.integ == RT_INTEGRATOR_DIRECT && c.strategy == RT_STRATEGY_WEIGHTED, bidir = c.integ == RT_INTEGRATOR_BIDIRECTIONAL, debug = c.integ == RT_INTEGRATOR_DEBUG;
        if (bidir && scene == 2) continue;                // rt_render refuses the bidirectional integrator in a medium
        for (int bits = 0; bits < 32; ++bits)             // counting, EXT, three lights (of one sample each), a specular material, a grid
        for (const std::optional<int> &pipeline : {unset, off, on})
        for (const std::optional<int> &fixed_frame : {unset, off, on})
        for (const std::optional<int> &high_occ : {unset, off, on})
        for (int query = 0; query < 2; ++query) {
            if (query && (weighted || bidir || debug)) continue;          // plan_query refuses them
            LaunchCase lc{desc(c.integ, c.strategy), scene == 1 ? tiny_fat() : large_scene(), Schedule{}, query != 0};
            lc.sf.medium = scene == 2; lc.sf.counting = (bits & 1) != 0; lc.sf.has_ext = (bits & 2) != 0;
            if (bits & 4) { lc.sf.n_lights = 3; lc.sf.light_samples = {1, 1, 1}; }
            lc.sf.specular_materials = (bits & 8) != 0;
            if (bits & 16) lc.sf.accel_kind = RT_ACCEL_GRID;
            FrameKnobs kn; kn.pipeline = pipeline; kn.fixed_frame = fixed_frame; kn.high_occ = high_occ;
            g_what = what + " bits " + std::to_string(bits) + " pipeline " + std::to_string(pipeline.value_or(-1)) + " fixed_frame " + std::to_string(fixed_frame.value_or(-1)) +
                     " high_occ " + std::to_string(high_occ.value_or(-1)) + (query ? " query" : "");
            lc.sc = scheduled(lc.rd, lc.sf, kn);
            const Schedule frame = lc.sc;
            if (query) CHECK(!plan_query(lc.rd, QueryRange{3, 8}, lc.sc));
            check_launch(lc);
            const Launch ln = plan_launch(lc.rd, lc.sf, lc.sc, lc.query);
            if (weighted || bidir || debug) CHECK(ln.family != Launch::Pipeline && ln.family != Launch::Fixed && ln.family != Launch::FixedScene);
            if (query) {                                  // ... whatever the frame itself would have taken, and without plan_query's reset of the schedule too
                CHECK(ln.family == Launch::Rays);
                CHECK(plan_launch(lc.rd, lc.sf, frame, true).family == Launch::Rays);
            }
        }
    }
    // ---- what the precedence decides where plan_schedule would not lead: schedules made by hand
    const SceneFacts large = large_scene();
    {   CASE("launch: Whitted has no scene twin"); Schedule sc = scheduled(desc(RT_INTEGRATOR_WHITTED), large); CHECK(sc.fixed_frame && sc.fixed_scene == 0);
        sc.fixed_scene = fixed::SCENE_ONE_LIGHT | fixed::SCENE_NO_SPECULAR;
        const Launch ln = plan_launch(desc(RT_INTEGRATOR_WHITTED), large, sc, false);
        CHECK(ln.family == Launch::Fixed && ln.scene_axes == 0 && ln.k == 2 * RT_INTEGRATOR_WHITTED); }
    {   CASE("launch: axes no twin was compiled for"); const RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); Schedule sc = scheduled(rd, large);
        CHECK(plan_launch(rd, large, sc, false).family == Launch::FixedScene && plan_launch(rd, large, sc, false).scene_axes == (fixed::SCENE_ONE_LIGHT | fixed::SCENE_NO_SPECULAR));
        sc.fixed_scene = fixed::SCENE_NO_SPECULAR;        // every scene twin is compiled for one light
        CHECK(plan_launch(rd, large, sc, false).family == Launch::Fixed && plan_launch(rd, large, sc, false).scene_axes == 0);
        sc.fixed_scene = fixed::SCENE_ONE_LIGHT; sc.fixed_frame = false;      // no scene twin without the fixed frame
        CHECK(plan_launch(rd, large, sc, false).family == Launch::Mega && plan_launch(rd, large, sc, false).scene_axes == 0); }
    {   CASE("launch: a scene that keeps its frames off the scene twins"); SceneFacts sf = large; sf.scene_twins = false; const RtRenderDesc rd = desc(RT_INTEGRATOR_DIRECT, RT_STRATEGY_ONE);
        check_launch(LaunchCase{rd, sf, scheduled(rd, sf), false});
        CHECK(plan_launch(rd, sf, scheduled(rd, sf), false).family == Launch::Fixed); }
    {   CASE("launch: debug ignores the fixed-frame choice"); const RtRenderDesc rd = desc(RT_INTEGRATOR_DEBUG); Schedule sc = scheduled(rd, large);
        sc.fixed_frame = true; sc.fixed_scene = fixed::SCENE_ONE_LIGHT;
        const Launch ln = plan_launch(rd, large, sc, false);
        CHECK(ln.family == Launch::Debug && ln.scene_axes == 0 && ln.k == 0); }
    for (const Combo &c : combos()) {
        if (c.integ != RT_INTEGRATOR_BIDIRECTIONAL && !(c.integ == RT_INTEGRATOR_DIRECT && c.strategy == RT_STRATEGY_WEIGHTED)) continue;
        CASE(std::string("launch: PIPELINE=1, ") + c.name); FrameKnobs kn; kn.pipeline = 1; const RtRenderDesc rd = desc(c.integ, c.strategy);
        CHECK(plan_launch(rd, large, scheduled(rd, large, kn), false).family == (c.integ == RT_INTEGRATOR_BIDIRECTIONAL ? Launch::Bidir : Launch::Weighted)); }
    {   CASE("launch: a query takes neither the pipeline nor a fixed kernel"); const RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); Schedule sc = scheduled(rd, large);
        sc.pipeline = 1; sc.fixed_frame = true; sc.fixed_scene = fixed::SCENE_ONE_LIGHT;
        const Launch ln = plan_launch(rd, large, sc, true);
        CHECK(ln.family == Launch::Rays && ln.scene_axes == 0 && ln.k == 0 && ln.integ == RT_INTEGRATOR_PATH); }
    {   CASE("request: without a frame"); SceneFacts sf = large; sf.accel_kind = RT_ACCEL_GRID; sf.medium = true; sf.has_ext = true; sf.counting = true;
        const flavour::Request r = request(nullptr, sf, nullptr), z = request(nullptr, large, nullptr);
        CHECK(r.integ == 0 && r.grid && r.vol && r.count && r.ext && !r.high_occ);
        CHECK(z.integ == 0 && !z.grid && !z.vol && !z.count && !z.ext && !z.high_occ);
        const RtRenderDesc rd = desc(RT_INTEGRATOR_PATH); Schedule sc = scheduled(rd, large);
        CHECK(sc.high_occupancy == 1 && request(&rd, large, &sc).high_occ && request(&rd, large, &sc).integ == RT_INTEGRATOR_PATH && !request(&rd, large, nullptr).high_occ); }
}

int main() {
    test_requests();
    test_extent();
    test_schedule();
    test_march();
    test_launch();
    if (g_failed) { std::fprintf(stderr, "frame_plan_host_test: %d checks failed\n", g_failed); return 1; }
    std::printf("frame_plan_host_test: ok (%d cases)\n", g_cases);
    return 0;
}
