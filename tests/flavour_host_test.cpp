// flavour_host_test.cpp -- the kernel selection of pbrt-v1_amd/csrc/hip/rt_flavour.h on the host: a stand-alone program that tests/test_flavour_host.py
// compiles with -fsanitize=address,undefined and runs.  No rendering test can see which instantiation a frame ran (the flavours compute the same film),
// so the rules are stated here as predicates on the template arguments of the entry that index() selects, for every request there is.
#include "rt_flavour.h"
#include <cstdio>
#include <set>
#include <tuple>

using namespace rt::flavour;

static int g_failed = 0;
static char g_what[128] = "";        // the family or request under test
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_what); ++g_failed; } } while (0)

// the template arguments alone (not the request they came from)
static std::tuple<bool, int, bool, bool, int> args(const Flavour &f) { return std::make_tuple(f.count, f.accel, f.vol, f.ext, f.waves); }

template <class Family, class... Integ> static void distinct(const char *name, Integ... integ) {
    std::snprintf(g_what, sizeof g_what, "%s", name);
    std::set<std::tuple<bool, int, bool, bool, int>> seen;
    for (int k = 0; k < Family::N; ++k) seen.insert(args(Family::flavour(k, integ...)));
    CHECK(int(seen.size()) == Family::N);
}

int main() {
    // ---- bijection: a family's N entries are N different instantiations
    distinct<Mega>("Mega whitted", int(RT_INTEGRATOR_WHITTED)); distinct<Mega>("Mega direct", int(RT_INTEGRATOR_DIRECT)); distinct<Mega>("Mega path", int(RT_INTEGRATOR_PATH));
    distinct<Weighted>("Weighted"); distinct<Bidir>("Bidir"); distinct<Shade>("Shade"); distinct<Vertex>("Vertex"); distinct<March>("March"); distinct<Trace>("Trace");
    CHECK(3 * Mega::N + Weighted::N + Bidir::N + 3 * Shade::N + Vertex::N + March::N + Trace::N == 95);

    // ---- the rules, over all 96 requests: 3 integrators x grid, medium, counting, EXT, high occupancy
    int n_requests = 0;
    for (int integ = RT_INTEGRATOR_WHITTED; integ <= RT_INTEGRATOR_PATH; ++integ)
    for (int bits = 0; bits < 32; ++bits, ++n_requests) {
        const bool g = bits & 1, v = bits & 2, c = bits & 4, e = bits & 8, h = bits & 16;
        const Request r{integ, g, v, c, e, h};
        const int accel = g ? RT_ACCEL_GRID : RT_ACCEL_KDTREE;
        std::snprintf(g_what, sizeof g_what, "integ %d grid %d vol %d count %d ext %d high_occ %d", integ, g, v, c, e, h);
        {   // megakernel: a counting twin always carries the EXT code and is never register-capped; EXT beats high occupancy
            const int k = Mega::index(r);
            CHECK(k >= 0 && k < Mega::N);
            const Flavour f = Mega::flavour(k, integ);
            CHECK(f.count == c && f.accel == accel && f.vol == v);
            CHECK(f.ext == (c || e));
            CHECK((f.waves == RT_HIGH_OCC_WAVES) == (!c && !e && h));
            const bool natural = !c && !e && !h;
            if (natural) CHECK(f.waves == (integ == RT_INTEGRATOR_DIRECT && !v ? 3 : RT_MIN_WAVES));       // DirectLighting without a medium: held to 3 waves
            if (c || e) CHECK(f.waves == RT_MIN_WAVES);
        }
        {   // weighted: EXT always, 3 waves for the timed kernels without a medium
            const int k = Weighted::index(r);
            CHECK(k >= 0 && k < Weighted::N);
            const Flavour f = Weighted::flavour(k);
            CHECK(f.count == c && f.accel == accel && f.vol == v && f.ext);
            CHECK(f.waves == ((!c && !v) ? 3 : RT_MIN_WAVES));
        }
        {   // bidirectional
            const int k = Bidir::index(r);
            CHECK(k >= 0 && k < Bidir::N);
            const Flavour f = Bidir::flavour(k);
            CHECK(f.count == c && f.accel == accel);
        }
        {   // pipeline shade
            const int k = Shade::index(r);
            CHECK(k >= 0 && k < Shade::N);
            const Flavour f = Shade::flavour(k);
            CHECK(f.count == c && f.vol == v);
            CHECK(f.ext == (c || e));
        }
        {   // by-vertex shade
            const int k = Vertex::index(r);
            CHECK(k >= 0 && k < Vertex::N);
            const Flavour f = Vertex::flavour(k);
            CHECK(f.count == c);
            CHECK(f.ext == (c || e));
        }
        {   // march
            const int k = March::index(r);
            CHECK(k >= 0 && k < March::N);
            const Flavour f = March::flavour(k);
            CHECK(f.count == c && f.accel == accel);
            CHECK(f.ext == (c || e));
        }
        {   // trace: the one family with a counting kernel without EXT (rt_trace_closest / rt_trace_any are the requests with c set)
            const int k = Trace::index(r);
            CHECK(k >= 0 && k < Trace::N);
            const Flavour f = Trace::flavour(k);
            CHECK(f.count == c && f.accel == accel);
            CHECK(f.ext == e);
        }
    }
    CHECK(n_requests == 96);
    if (g_failed) { std::fprintf(stderr, "flavour_host_test: %d checks failed\n", g_failed); return 1; }
    std::printf("flavour_host_test: ok (%d requests)\n", n_requests);
    return 0;
}
