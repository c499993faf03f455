// rt_film_add.hip -- Film::AddSample for radiances in DEVICE memory (rt_film_add_device, include/pbrt_hip.h) and the image positions of camera samples
// (rt_sample_positions_device): the kernels and their launches.  The entry points themselves (rt_kernels.hip) bind what plan::plan_film_add
// (rt_frame_plan.h) plans.  The frame's own gathers (rt_film.hip) assume whole sample pixels in the sample_slot() layout, all of them taking part; a
// range [first, first + n) of the frame's scanline order can begin and end inside a pixel, so the kernels here are their own.
//
// Kernels
//   sample_positions_kernel   the camera kernel without the camera: setup_sample (rt_integrate.h) for camera sample first + i, imageX / imageY out -- the
//                             values sample_write parks in a frame's records.  For a film add it also runs Scene::Render's radiance check
//                             (scene.cpp:60-74) over the caller's radiances to COUNT the bad ones, once per sample and only when the scene counts.
//   film_add_kernel<PACKED>   ImageFilm::AddSample (film/image.cpp:103-142) as a gather over the film rows the range can reach, the caller's float4
//                             array and the staged positions as record source; two forms of what a staged record carries (see the kernel).
#include "rt_host.h"

namespace rt {

#define RT_ADD_TILE_W 64          // a workgroup's film pixels: 64 columns x RT_ADD_TILE_H rows, one row per wave
#ifndef RT_ADD_TILE_H
#define RT_ADD_TILE_H 8           // measured against 2, 4 and 16 rows: taller = fewer halo rows staged, more waves waiting per sample row
#endif
#ifndef RT_ADD_SLOTS
#define RT_ADD_SLOTS 1280         // records a workgroup stages at a time: 2 x 20 KB of LDS (three workgroups per CU; 1024 slots measured slower)
#endif
#define RT_ADD_BLOCK (RT_ADD_TILE_W * RT_ADD_TILE_H)
#define RT_ADD_PACKED_REACH 5     // 2 * 5 + 1 entries of 5 bits fit a 64-bit word

// Scene::Render's radiance check (scene.cpp:60-74), the expressions of sample_write (rt_integrate.h)
__device__ inline bool radiance_is_bad(float r, float g, float b) {
    const float y = lum_y(mk3(r, g, b));
    if (r != r || g != g || b != b) return true;
    if (y < -1e-5) return true;
    return isinf(y);
}

__global__ __launch_bounds__(RT_ADD_BLOCK) void sample_positions_kernel(DevScene sc, DevFrame fr, unsigned long long first, unsigned count, float2 *__restrict__ xy,
                                                                        const float4 *__restrict__ L, unsigned long long *__restrict__ counters) {
    const unsigned i = blockIdx.x * RT_ADD_BLOCK + threadIdx.x;
    unsigned long long bad = 0;
    if (i < count) {
        const unsigned long long n = first + i;
        Lane ln; Ray r;
        setup_sample(sc, fr, ln, n / fr.spp, int(n % fr.spp), r);
        RT_GPTR(float2, xy)[i] = make_float2(ln.image_x, ln.image_y);
        if (L) { const float4 v = RT_GPTR(const float4, L)[i]; bad = radiance_is_bad(v.x, v.y, v.z) ? 1u : 0u; }
    }
    if (L) {                                                             // (a property of the launch: wave-uniform)
        for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
        if ((threadIdx.x & 63) == 0 && bad) atomicAdd(counters + 6, bad);       // RtCounters::bad_samples, as the render kernels add it (rt_render_body.inc)
    }
}

// What the gather reads of the frame and of the call
struct FilmAddArgs {
    float *accum; const float *filter_table;
    const float4 *L; const float2 *xy;                                   // [n] the caller's {L.rgb, alpha}, [n] imageX, imageY: entry i is camera sample first + i
    unsigned long long first, end;                                       // the range [first, end) in the frame's scanline order (pixel * spp + s)
    int spp, width;                                                      // samples per pixel, sample pixels per row of the sample extent
    int x_start, x_end, y_start, y_end;
    int x_pixel_start, y_pixel_start, x_pixel_count, y_pixel_count;
    int row0, row_end;                                                   // film rows to visit, relative to the crop window (plan::FilmAdd)
    int rx, ry;
    float fxw, fyw, inv_fxw, inv_fyw;
    int ncols, ns;                                                       // a staged chunk: ncols sample pixels x ns samples (ns < spp: one pixel at a time)
};

// One thread per film pixel of a 64 x RT_ADD_TILE_H tile, a wave per pixel row: every lane of a wave is reached by the same sample rows, so a wave either
// works or waits at the barrier as a whole.  For each sample row the tile can reach, the records of the sample pixels that reach it are staged in LDS
// chunk by chunk with the radiance check applied, and every pixel then walks the records of its own columns in ascending sample index: sample rows,
// columns, samples in pixel, the order of the frame's gathers, on top of what the film holds.  A record outside [first, end) is never fetched: its slot
// says "outside" for every pixel, and a pixel outside a record's footprint skips it -- the reference's `continue`, not a weight of zero, so that a
// caller's radiance need not be finite to contribute nothing.  Column blocks are padded by one slot (the 64 lanes of a row read 64 consecutive columns
// at the same sample: different LDS banks).  What sits next to the radiance in a slot comes in two forms:
//   PACKED   (filters reaching up to 5 pixels) the staging thread evaluates image.cpp:108-132 for each of the 2 rx + 1 pixel columns and 2 ry + 1 pixel
//            rows the record's sample pixel can reach -- inside the footprint? which filter-table index? -- and packs them as 5-bit entries into two
//            64-bit words, as film_slot_kernel (rt_film.hip) does for the frame; a pixel then takes its two entries with a shift each and looks the
//            weight up.  The expressions are the reference's own, evaluated once per staged record instead of once per pixel under it.
//   general  (any reach) the position and the footprint as int16 pairs, as film_gather_kernel keeps them; the pixel evaluates its own table index.
template <bool PACKED>
__global__ __launch_bounds__(RT_ADD_BLOCK) void film_add_kernel(const FilmAddArgs a) {
    __shared__ __attribute__((aligned(16))) float4 lds_L[RT_ADD_SLOTS];
    __shared__ __attribute__((aligned(16))) float4 lds_q[RT_ADD_SLOTS];
    __shared__ float ftab[256];                                         // FILTER_TABLE_SIZE^2 (film/image.cpp:53-64)
    const int t = int(threadIdx.x);
    for (int i = t; i < 256; i += RT_ADD_BLOCK) ftab[i] = RT_GPTR(const float, a.filter_table)[i];
    const int nbx = (a.x_pixel_count + RT_ADD_TILE_W - 1) / RT_ADD_TILE_W;
    const int bx = int(blockIdx.x) % nbx, by = int(blockIdx.x) / nbx;
    const int lx = bx * RT_ADD_TILE_W + (t & 63), ly = a.row0 + by * RT_ADD_TILE_H + (t >> 6);
    const bool live = lx < a.x_pixel_count && ly < a.row_end;
    const int x = a.x_pixel_start + lx, y = a.y_pixel_start + ly;
    const size_t plane = size_t(a.x_pixel_count) * a.y_pixel_count, px = size_t(ly) * a.x_pixel_count + lx;
    float RT_G *accum = RT_GPTR(float, a.accum);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
    if (live) { a0 = accum[px]; a1 = accum[plane + px]; a2 = accum[2 * plane + px]; a3 = accum[3 * plane + px]; a4 = accum[4 * plane + px]; }
    // sample pixels whose samples (imageX in [sx, sx+1]) can reach pixel x: |x - (sx + u - .5)| <= width
    const int sx0 = max(int(ceilf(x - a.fxw - 0.5f)), a.x_start), sx1 = min(int(floorf(x + a.fxw + 0.5f)), a.x_end - 1);
    const int sy0 = max(int(ceilf(y - a.fyw - 0.5f)), a.y_start), sy1 = min(int(floorf(y + a.fyw + 0.5f)), a.y_end - 1);
    const int xlo = a.x_pixel_start, xhi = a.x_pixel_start + a.x_pixel_count - 1;
    const int ylo = a.y_pixel_start, yhi = a.y_pixel_start + a.y_pixel_count - 1;
    const int X0 = a.x_pixel_start + bx * RT_ADD_TILE_W, X1 = min(X0 + RT_ADD_TILE_W - 1, xhi);
    const int Y0 = a.y_pixel_start + a.row0 + by * RT_ADD_TILE_H, Y1 = min(Y0 + RT_ADD_TILE_H - 1, a.y_pixel_start + a.row_end - 1);
    const int bsx0 = max(X0 - a.rx, a.x_start), bsx1 = min(X1 + a.rx, a.x_end - 1);
    const int bsy0 = max(Y0 - a.ry, a.y_start), bsy1 = min(Y1 + a.ry, a.y_end - 1);
    const unsigned long long spp = unsigned(a.spp);
    const float inv_fxw = a.inv_fxw, inv_fyw = a.inv_fyw;
    const int rx = a.rx, ry = a.ry;
    // every `continue` below depends on the launch and the workgroup only: the barriers are met by all of its threads
    for (int sy = bsy0; sy <= bsy1; ++sy) {
        const unsigned long long rowpix = (unsigned long long)(sy - a.y_start) * unsigned(a.width);
        if (bsx0 > bsx1) continue;
        if ((rowpix + unsigned(bsx1 - a.x_start) + 1) * spp <= a.first || (rowpix + unsigned(bsx0 - a.x_start)) * spp >= a.end) continue;
        const bool row_mine = live && sy >= sy0 && sy <= sy1;
        const unsigned shy = unsigned(5 * (y - sy + ry));               // PACKED: my row's entry in a record's y word (0 <= y - sy + ry <= 2 ry where row_mine)
        for (int cx = bsx0; cx <= bsx1; cx += a.ncols) {
            const int nc = min(a.ncols, bsx1 - cx + 1);
            const unsigned long long colpix = rowpix + unsigned(cx - a.x_start);
            for (int s0 = 0; s0 < a.spp; s0 += a.ns) {
                const int ns = min(a.ns, a.spp - s0), stride = ns + 1;
                if ((colpix + unsigned(nc - 1)) * spp + unsigned(s0 + ns) <= a.first || colpix * spp + unsigned(s0) >= a.end) continue;
                __syncthreads();                                        // the chunk before this one has been walked
                for (int r = t; r < nc * ns; r += RT_ADD_BLOCK) {
                    const int col = r / ns, sv = r - col * ns;
                    const unsigned long long idx = (colpix + unsigned(col)) * spp + unsigned(s0 + sv);
                    // outside the range: no pixel lies inside (general: x0 = 1 > x1 = 0; PACKED: every "inside" bit clear)
                    float4 L = make_float4(0.f, 0.f, 0.f, 0.f), q = PACKED ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(0.f, 0.f, __uint_as_float(1u), __uint_as_float(1u));
                    if (idx >= a.first && idx < a.end) {
                        const size_t i = size_t(idx - a.first);
                        L = RT_GPTR(const float4, a.L)[i];
                        const float2 p = RT_GPTR(const float2, a.xy)[i];
                        if (radiance_is_bad(L.x, L.y, L.z)) { L.x = 0.f; L.y = 0.f; L.z = 0.f; }      // scene.cpp:60-74: black, and still added
                        // the sample's pixel footprint (film/image.cpp:108-116): once per staged record, not once per pixel under it
                        const float dImageX = p.x - 0.5f, dImageY = p.y - 0.5f;
                        const int x0 = max(int(ceilf(dImageX - a.fxw)), xlo), x1 = min(int(floorf(dImageX + a.fxw)), xhi);
                        const int y0 = max(int(ceilf(dImageY - a.fyw)), ylo), y1 = min(int(floorf(dImageY + a.fyw)), yhi);
                        if (PACKED) {
                            // ... and the filter-table offsets of image.cpp:118-130 for the pixel columns cx + col - rx + e and rows sy - ry + e
                            unsigned long long wx = 0, wy = 0;
                            if (x0 <= x1 && y0 <= y1) {                 // image.cpp:116
                                const int xb = cx + col - rx, yb = sy - ry;
                                for (int e = 0; e <= 2 * rx; ++e) {
                                    const int xi = xb + e;
                                    const float fx = fabsf((xi - dImageX) * inv_fxw * 16);
                                    const unsigned ent = ((xi >= x0 && xi <= x1) ? 16u : 0u) | unsigned(min(int(floorf(fx)), 15));
                                    wx |= (unsigned long long)ent << (5 * e);
                                }
                                for (int e = 0; e <= 2 * ry; ++e) {
                                    const int yi = yb + e;
                                    const float fy = fabsf((yi - dImageY) * inv_fyw * 16);
                                    const unsigned ent = ((yi >= y0 && yi <= y1) ? 16u : 0u) | unsigned(min(int(floorf(fy)), 15));
                                    wy |= (unsigned long long)ent << (5 * e);
                                }
                            }
                            q = make_float4(__uint_as_float(unsigned(wx)), __uint_as_float(unsigned(wx >> 32)), __uint_as_float(unsigned(wy)), __uint_as_float(unsigned(wy >> 32)));
                        } else {
                            q.x = p.x; q.y = p.y;
                            if (x0 <= x1 && y0 <= y1) {                 // image.cpp:116
                                q.z = __uint_as_float((unsigned(x0) & 0xffffu) | (unsigned(x1) << 16));
                                q.w = __uint_as_float((unsigned(y0) & 0xffffu) | (unsigned(y1) << 16));
                            }
                        }
                    }
                    lds_L[col * stride + sv] = L; lds_q[col * stride + sv] = q;
                }
                __syncthreads();
                if (!row_mine) continue;                                // (no barrier below in this trip)
                for (int sx = max(cx, sx0); sx <= min(cx + nc - 1, sx1); ++sx) {
                    const float4 *Lp = lds_L + (sx - cx) * stride, *qp = lds_q + (sx - cx) * stride;
                    const unsigned shx = unsigned(5 * (x - sx + rx));   // PACKED: my column's entry in the x word (sx0 <= sx <= sx1: 0 <= x - sx + rx <= 2 rx)
                    // in? and the weight of record q for my pixel
                    auto weigh = [&](const float4 &q, float &wt) __attribute__((always_inline)) -> bool {
                        if (PACKED) {
                            const unsigned long long wx = (unsigned long long)__float_as_uint(q.x) | ((unsigned long long)__float_as_uint(q.y) << 32);
                            const unsigned long long wy = (unsigned long long)__float_as_uint(q.z) | ((unsigned long long)__float_as_uint(q.w) << 32);
                            const unsigned ex = unsigned(wx >> shx) & 31u, ey = unsigned(wy >> shy) & 31u;
                            wt = ftab[((ey & 15u) << 4) | (ex & 15u)];
                            return (ex & ey & 16u) != 0u;
                        }
                        const int bx_ = __float_as_int(q.z), by_ = __float_as_int(q.w);
                        const int x0 = int(short(bx_ & 0xffff)), x1 = bx_ >> 16, y0 = int(short(by_ & 0xffff)), y1 = by_ >> 16;
                        const float dImageX = q.x - 0.5f, dImageY = q.y - 0.5f;
                        const float fx = fabsf((x - dImageX) * inv_fxw * 16), fy = fabsf((y - dImageY) * inv_fyw * 16);
                        const int ifx = min(int(floorf(fx)), 15), ify = min(int(floorf(fy)), 15);
                        wt = ftab[(ify * 16 + ifx) & 255];
                        return !(x < x0 || x > x1 || y < y0 || y > y1);
                    };
                    // four samples per trip: their records, footprint tests and filter weights are independent; only the five accumulations keep
                    // the reference's sample order
                    int s = 0;
                    for (; s + 4 <= ns; s += 4) {
                        float4 L[4], q[4]; float wt[4]; bool in[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) { L[u] = Lp[s + u]; q[u] = qp[s + u]; }
#pragma unroll
                        for (int u = 0; u < 4; ++u) in[u] = weigh(q[u], wt[u]);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (in[u]) {
                                a0 += wt[u] * L[u].x; a1 += wt[u] * L[u].y; a2 += wt[u] * L[u].z;   // Spectrum::AddWeighted color.h:116-120
                                a3 += L[u].w * wt[u]; a4 += wt[u];
                            }
                    }
                    for (; s < ns; ++s) {
                        float wt;
                        if (!weigh(qp[s], wt)) continue;
                        const float4 L = Lp[s];
                        a0 += wt * L.x; a1 += wt * L.y; a2 += wt * L.z;       // Spectrum::AddWeighted color.h:116-120
                        a3 += L.w * wt; a4 += wt;
                    }
                }
            }
        }
    }
    if (live) { accum[px] = a0; accum[plane + px] = a1; accum[2 * plane + px] = a2; accum[3 * plane + px] = a3; accum[4 * plane + px] = a4; }
}

}  // namespace rt

// ------------------------------------------------------------------------------------------ host side
// imageX, imageY of camera samples first .. first + count - 1 of the frame `fr` (bind_extent's fields) into dev_xy; with dev_L, the bad radiances among
// dev_L[count] are added to RtCounters::bad_samples
int sample_positions_launch(RtScene *s, const DevFrame &fr, unsigned long long first, unsigned count, float *dev_xy, const float *dev_L) {
    if (count == 0) return RT_OK;
    hipLaunchKernelGGL(sample_positions_kernel, dim3((count + RT_ADD_BLOCK - 1) / RT_ADD_BLOCK), dim3(RT_ADD_BLOCK), 0, s->stream, s->dev, fr, first, count,
                       reinterpret_cast<float2 *>(dev_xy), reinterpret_cast<const float4 *>(dev_L), (unsigned long long *)s->counters);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// Which form of the gather a planned add takes (called before anything is launched): the packed one wherever its two 64-bit words hold the filter's
// reach; PBRT_HIP_FILM_ADD=packed|general forces one (tests)
int film_add_form(const plan::FilmAdd &p, bool &packed) {
    const bool packed_ok = p.reach_x <= RT_ADD_PACKED_REACH && p.reach_y <= RT_ADD_PACKED_REACH;
    packed = packed_ok;
    if (const char *e = knob("PBRT_HIP_FILM_ADD")) {
        if (std::strcmp(e, "packed") && std::strcmp(e, "general")) return fail(RT_EINVAL, "PBRT_HIP_FILM_ADD: packed or general");
        packed = !std::strcmp(e, "packed");
        if (packed && !packed_ok) return fail(RT_EINVAL, "PBRT_HIP_FILM_ADD=packed: the filter reaches more than 5 pixels");
    }
    return RT_OK;
}

// ImageFilm::AddSample for the planned range over the film rows it reaches, on the scene's stream
int film_add_launch(RtScene *s, const RtRenderDesc &rd, const plan::FilmAdd &p, bool packed, unsigned long long first, unsigned n, const float *dev_L, const float *dev_xy) {
    const int nrows = p.row_end - p.row0;
    if (n == 0 || nrows <= 0) return RT_OK;
    FilmAddArgs a{};
    a.accum = s->accum; a.filter_table = s->filter_dev;
    a.L = reinterpret_cast<const float4 *>(dev_L); a.xy = reinterpret_cast<const float2 *>(dev_xy);
    a.first = first; a.end = first + n;
    a.spp = p.spp; a.width = rd.x_end - rd.x_start;
    a.x_start = rd.x_start; a.x_end = rd.x_end; a.y_start = rd.y_start; a.y_end = rd.y_end;
    a.x_pixel_start = rd.x_pixel_start; a.y_pixel_start = rd.y_pixel_start; a.x_pixel_count = rd.x_pixel_count; a.y_pixel_count = rd.y_pixel_count;
    a.row0 = p.row0; a.row_end = p.row_end;
    // (a sample pixel further away than the film is wide reaches nothing: the tile's column range is clipped to the sample extent anyway)
    a.rx = std::min(p.reach_x, 65536); a.ry = std::min(p.reach_y, 65536);
    a.fxw = rd.filter_x_width; a.fyw = rd.filter_y_width; a.inv_fxw = 1.f / a.fxw; a.inv_fyw = 1.f / a.fyw;       // bind_extent's expressions
    // whole sample pixels where one fits the staging slots with its pad, as many as fit; else one pixel in pieces
    if (p.spp + 1 <= RT_ADD_SLOTS) { a.ns = p.spp; a.ncols = RT_ADD_SLOTS / (p.spp + 1); }
    else { a.ns = RT_ADD_SLOTS - 1; a.ncols = 1; }
    const unsigned nbx = unsigned((rd.x_pixel_count + RT_ADD_TILE_W - 1) / RT_ADD_TILE_W), nby = unsigned((nrows + RT_ADD_TILE_H - 1) / RT_ADD_TILE_H);
    hipLaunchKernelGGL(packed ? film_add_kernel<true> : film_add_kernel<false>, dim3(nbx * nby), dim3(RT_ADD_BLOCK), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    return RT_OK;
}
