// plm_device_check.hip -- the portable libm functions (rt_libm_portable.h) evaluated ON THE DEVICE over the arguments of a file, results written raw:
// tests/test_gpu_plm.py compares them bit for bit with the host's (oracle/_build/libplm.so).  Stand-alone, compiled with the project's device flags.
//   plm_device_check IN OUT
// IN:  int64 n, then for each of the 7 functions (sinf cosf sincosf acosf atan2f powf expf) float a[n], float b[n].
// OUT: for each function float out[n], float out2[n] (out2: sincosf's cosine, else 0).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define PLM_FN __host__ __device__ inline
#include "rt_libm_portable.h"

#define CHECK(call)                                                                                     \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) { std::fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); std::exit(3); } \
    } while (0)

__global__ void plm_eval_kernel(int fn, const float *a, const float *b, float *out, float *out2, size_t n) {
    for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
        float r = 0.f, r2 = 0.f;
        switch (fn) {
            case 0: r = plm_sinf(a[i]); break;
            case 1: r = plm_cosf(a[i]); break;
            case 2: plm_sincosf(a[i], &r, &r2); break;
            case 3: r = plm_acosf(a[i]); break;
            case 4: r = plm_atan2f(a[i], b[i]); break;
            case 5: r = plm_powf(a[i], b[i]); break;
            default: r = plm_expf(a[i]); break;
        }
        out[i] = r; out2[i] = r2;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: plm_device_check IN OUT\n"); return 2; }
    FILE *in = std::fopen(argv[1], "rb");
    long long n = 0;
    if (!in || std::fread(&n, sizeof n, 1, in) != 1 || n <= 0 || n > (1ll << 24)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const size_t count = size_t(n);
    std::vector<float> a(count), b(count), out(count), out2(count);
    float *da, *db, *dout, *dout2;
    CHECK(hipMalloc(&da, count * sizeof(float))); CHECK(hipMalloc(&db, count * sizeof(float)));
    CHECK(hipMalloc(&dout, count * sizeof(float))); CHECK(hipMalloc(&dout2, count * sizeof(float)));
    FILE *of = std::fopen(argv[2], "wb");
    if (!of) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int fn = 0; fn < 7; ++fn) {
        if (std::fread(a.data(), sizeof(float), count, in) != count || std::fread(b.data(), sizeof(float), count, in) != count) { std::fprintf(stderr, "short input\n"); return 2; }
        CHECK(hipMemcpy(da, a.data(), count * sizeof(float), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(db, b.data(), count * sizeof(float), hipMemcpyHostToDevice));
        plm_eval_kernel<<<1024, 256>>>(fn, da, db, dout, dout2, count);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(out.data(), dout, count * sizeof(float), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(out2.data(), dout2, count * sizeof(float), hipMemcpyDeviceToHost));
        if (std::fwrite(out.data(), sizeof(float), count, of) != count || std::fwrite(out2.data(), sizeof(float), count, of) != count) { std::fprintf(stderr, "short output\n"); return 2; }
    }
    std::fclose(of); std::fclose(in);
    CHECK(hipFree(da)); CHECK(hipFree(db)); CHECK(hipFree(dout)); CHECK(hipFree(dout2));
    std::printf("plm_device_check: ok (%lld arguments per function)\n", n);
    return 0;
}
