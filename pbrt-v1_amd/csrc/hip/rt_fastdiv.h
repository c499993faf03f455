// rt_fastdiv.h -- exact unsigned 32-bit division by a frame constant without a divide instruction (no HIP header: tests/fastdiv_host_test.cpp
// runs it on the host).  gfx950 has no integer divider: `n / d` with a run-time d expands to ~25 VALU instructions around a float reciprocal, and the
// work fetch of the megakernel divides by frame constants half a dozen times per camera sample.  The host finds, once per frame, a multiplier and two
// shifts per divisor (make_frame's bind_extent, rt_kernels.hip); the device then needs one multiply-high, a subtract, an add and two shifts.
//
// The form is the round-up multiplier with the add-and-shift fix-up (Granlund & Montgomery, "Division by Invariant Integers using Multiplication",
// PLDI 1994, figure 4.1): with l = ceil(log2 d), m = floor(2^32 * (2^l - d) / d) + 1 -- the low 32 bits of the 33-bit multiplier ceil(2^(32+l) / d) --
//     t = mulhi(m, n);  q = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0)
// is floor(n / d) for EVERY 32-bit n and every d in [1, 2^32): the sum t + ((n - t) >> 1) cannot overflow 32 bits, which is what the plain 32-bit
// "magic number" form gives up (it is exact only for divisors whose multiplier happens to fit 32 bits).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_FASTDIV_FN __host__ __device__ inline
#else
#define RT_FASTDIV_FN inline
#endif

namespace rt {

struct FastDiv {
    uint32_t mul, sh1, sh2;      // d == 0 (a divisor a frame does not have) is stored as {0, 0, 0}: never used
};

// host side (make_frame); d >= 1
inline FastDiv fastdiv_make(uint32_t d) {
    FastDiv f = {0u, 0u, 0u};
    if (d == 0u) return f;
    uint32_t l = 0;
    while (l < 32u && (uint64_t(1) << l) < d) ++l;                               // ceil(log2 d)
    f.mul = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1u);
    f.sh1 = l < 1u ? l : 1u;
    f.sh2 = l > 0u ? l - 1u : 0u;
    return f;
}

RT_FASTDIV_FN uint32_t fastdiv_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return uint32_t((uint64_t(a) * uint64_t(b)) >> 32);
#endif
}

// floor(n / d) for the d that `f` was made from
RT_FASTDIV_FN uint32_t fastdiv(uint32_t n, const FastDiv &f) {
    const uint32_t t = fastdiv_mulhi(f.mul, n);
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

// The divisors of the work fetch (rt_integrate.h: tile_order_to_sample, work_to_sample, setup_sample, stratified_camera_sample, sample_write), all of
// them constants of one frame.  The 32 x 32-pixel blocks of tile_order_to_sample are clipped at the extent's right and bottom edge, so the block
// height and width take two values each: index 0 is the full block, index 1 the clipped last row / column of blocks.
struct FrameDiv {
    FastDiv spp;                 // samples per pixel
    FastDiv xs;                  // strata per pixel row (stratified sampler)
    FastDiv width;               // W: pixels per scanline of the sample extent
    FastDiv row_px;              // W * T: pixels per row of blocks
    FastDiv block[2];            // T * h_t: pixels per full-width block in a full / the clipped row of blocks
    FastDiv block_w[2];          // w_t: width of a full / the clipped block
    uint32_t blocks_x;           // blocks per row of blocks, ceil(W / T)
    FastDiv per_tile;            // tile_pixels * spp  (work_to_sample)
    FastDiv tile_w, tiles_x;     // 2-D shard tiles (work_to_sample)
};

// W, H: the sample extent; T: DevFrame::mega_tile (0: none); the rest as in DevFrame
inline FrameDiv framediv_make(uint32_t spp, uint32_t xs, uint32_t W, uint32_t H, uint32_t T, uint64_t per_tile, uint32_t tile_w, uint32_t tiles_x) {
    FrameDiv fd = {};
    fd.spp = fastdiv_make(spp); fd.xs = fastdiv_make(xs); fd.width = fastdiv_make(W);
    if (T > 0u && uint64_t(W) * T <= 0xffffffffull) {
        const uint32_t h_last = H - (H - 1u) / T * T, w_last = W - (W - 1u) / T * T;        // the clipped last row / column of blocks (T when it is whole)
        fd.row_px = fastdiv_make(W * T);
        fd.block[0] = fastdiv_make(T * T); fd.block[1] = fastdiv_make(T * h_last);
        fd.block_w[0] = fastdiv_make(T); fd.block_w[1] = fastdiv_make(w_last);
        fd.blocks_x = (W - 1u) / T + 1u;
    }
    if (per_tile <= 0xffffffffull) fd.per_tile = fastdiv_make(uint32_t(per_tile));
    fd.tile_w = fastdiv_make(tile_w); fd.tiles_x = fastdiv_make(tiles_x);
    return fd;
}

}  // namespace rt
