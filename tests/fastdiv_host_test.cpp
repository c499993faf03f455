// fastdiv_host_test.cpp -- rt_fastdiv.h on the host: the quotient of rt::fastdiv against `/` for every divisor from 1 to 4096 and for the divisors
// of the frames bench.py renders (C3, C2, c4full, the multi-rank tilings), as rt::framediv_make derives them.  Dividends per divisor d: k*d - 1, k*d
// and k*d + 1 for k near 0 and for k near 2^32 / d, 0, 2^32 - 1, and one million seeded random 32-bit values.  Stand-alone (tests/test_fastdiv_host.py
// builds it under AddressSanitizer and UndefinedBehaviorSanitizer); no GPU, no HIP header.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "rt_fastdiv.h"

namespace {

std::atomic<unsigned long long> g_checked{0}, g_failed{0};

bool check(uint32_t n, uint32_t d, const rt::FastDiv &f) {
    const uint32_t q = rt::fastdiv(n, f);
    if (q == n / d) return true;
    if (g_failed.fetch_add(1) < 10) std::fprintf(stderr, "CHECK(fastdiv) %u / %u: got %u, expected %u\n", n, d, q, n / d);
    return false;
}

// splitmix64: the seeded dividends
uint64_t mix(uint64_t &x) {
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

void check_divisor(uint32_t d, const std::vector<uint32_t> &random) {
    const rt::FastDiv f = rt::fastdiv_make(d);
    unsigned long long n_checked = 0;
    auto around = [&](uint64_t k) {                                    // k*d - 1, k*d, k*d + 1, where they are 32-bit values
        for (int o = -1; o <= 1; ++o) {
            const int64_t v = int64_t(k * uint64_t(d)) + o;
            if (v >= 0 && v <= int64_t(0xffffffffll)) { check(uint32_t(v), d, f); ++n_checked; }
        }
    };
    const uint64_t top = (uint64_t(1) << 32) / d;
    for (uint64_t k = 0; k <= 4; ++k) around(k);
    for (uint64_t k = top > 4 ? top - 4 : 0; k <= top; ++k) around(k);
    check(0u, d, f); check(0xffffffffu, d, f); n_checked += 2;
    for (uint32_t n : random) check(n, d, f);
    g_checked += n_checked + random.size();
}

// the divisors a frame's work fetch uses, read back from the table make_frame stores (each FastDiv is checked against the divisor it was made from)
void frame_divisors(std::vector<uint32_t> &out, uint32_t spp, uint32_t xs, uint32_t W, uint32_t H, uint32_t T, uint32_t tile_pixels, uint32_t tile_w, uint32_t tiles_x) {
    const uint32_t h_last = H - (H - 1u) / T * T, w_last = W - (W - 1u) / T * T;
    const uint32_t ds[] = {spp, xs, W, W * T, T * T, T * h_last, T, w_last, tile_pixels * spp, tile_w, tiles_x};
    for (uint32_t d : ds) if (d) out.push_back(d);
    // ... and the table itself holds exactly these
    const rt::FrameDiv fd = rt::framediv_make(spp, xs, W, H, T, uint64_t(tile_pixels) * spp, tile_w, tiles_x);
    const struct { rt::FastDiv f; uint32_t d; } pairs[] = {{fd.spp, spp}, {fd.xs, xs}, {fd.width, W}, {fd.row_px, W * T}, {fd.block[0], T * T}, {fd.block[1], T * h_last},
                                                            {fd.block_w[0], T}, {fd.block_w[1], w_last}, {fd.per_tile, tile_pixels * spp}, {fd.tile_w, tile_w}, {fd.tiles_x, tiles_x}};
    for (const auto &p : pairs) {
        const rt::FastDiv want = rt::fastdiv_make(p.d);
        if (p.f.mul != want.mul || p.f.sh1 != want.sh1 || p.f.sh2 != want.sh2) { ++g_failed; std::fprintf(stderr, "CHECK(framediv) divisor %u\n", p.d); }
    }
    if (fd.blocks_x != (W + T - 1u) / T) { ++g_failed; std::fprintf(stderr, "CHECK(framediv) blocks_x %u\n", fd.blocks_x); }
}

}  // namespace

int main() {
    std::vector<uint32_t> divisors;
    for (uint32_t d = 1; d <= 4096; ++d) divisors.push_back(d);
    // sample extents: the image plus the Mitchell filter's 2 pixels on every side; 32 x 32-pixel work blocks on one shard
    frame_divisors(divisors, 16, 4, 1924, 1084, 32, 1, 0, 0);           // C3: 1920 x 1080 @ 16 spp
    frame_divisors(divisors, 64, 8, 1028, 1028, 32, 1, 0, 0);           // C2: 1024 x 1024 @ 64 spp
    frame_divisors(divisors, 256, 16, 2052, 2052, 32, 1, 0, 0);         // c4full on one device
    frame_divisors(divisors, 256, 16, 2052, 2052, 32, 64 * 64, 64, 33); // c4full over 8 ranks: 64 x 64-pixel 2-D tiles
    frame_divisors(divisors, 16, 4, 1028, 1028, 32, 64 * 64, 64, 17);   // C4 / C5 over ranks, 2-D tiles
    frame_divisors(divisors, 16, 4, 1028, 1028, 32, 48, 0, 0);          // ... and in 1-D tiles of 48 consecutive pixels
    frame_divisors(divisors, 64, 8, 1028, 1028, 32, 48, 0, 0);
    for (uint32_t d : {0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu}) divisors.push_back(d);      // the ends of the divisor range
    std::sort(divisors.begin(), divisors.end());
    divisors.erase(std::unique(divisors.begin(), divisors.end()), divisors.end());

    std::vector<uint32_t> random(1000000);
    uint64_t seed = 20240607ull;
    for (uint32_t &n : random) n = uint32_t(mix(seed) >> 16);

    const unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < n_threads; ++t)
        pool.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < divisors.size();) check_divisor(divisors[i], random); });
    for (std::thread &t : pool) t.join();

    if (g_failed.load()) { std::fprintf(stderr, "fastdiv_host_test: %llu failures\n", g_failed.load()); return 1; }
    std::printf("fastdiv_host_test: ok (%zu divisors, %llu quotients)\n", divisors.size(), g_checked.load());
    return 0;
}
