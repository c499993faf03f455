// devbuf_host_test.cpp -- rt::DevBuf (pbrt-v1_amd/csrc/hip/rt_devbuf.h) over malloc / free: a stand-alone program that tests/test_devbuf_host.py
// compiles with -fsanitize=address,undefined and runs.  rt::dev_alloc / rt::dev_free are defined here, with a count of live blocks and a switch
// that makes the next allocation fail; a double free, a leak or a use after free is the sanitizers' to report.
#include "rt_devbuf.h"
#include <cstdio>
#include <cstdlib>

static int g_live = 0, g_allocs = 0, g_frees = 0;
static bool g_fail_next = false;
namespace rt {
int dev_alloc(void **p, size_t bytes) {
    if (g_fail_next) { g_fail_next = false; *p = nullptr; return -3; }
    *p = std::malloc(bytes);
    ++g_live; ++g_allocs;
    return 0;
}
void dev_free(void *p) { std::free(p); --g_live; ++g_frees; }
}  // namespace rt
using rt::DevBuf;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); ++g_failed; } } while (0)

static int g_other_released = 0;
static void other_release(void *p) { std::free(p); ++g_other_released; }

struct Several { DevBuf<float> a; DevBuf<unsigned long long> b; DevBuf<char> c[3]; };

int main() {
    {   // growth replaces the block; need <= cap keeps pointer and capacity
        DevBuf<float> b;
        CHECK(b.p == nullptr && b.cap == 0 && b.grow(0) == 0 && b.p == nullptr && g_allocs == 0);
        CHECK(b.grow(100) == 0 && b.p && b.cap == 100 && b.bytes() == 400 && g_live == 1);
        for (size_t i = 0; i < b.cap; ++i) b.p[i] = float(i);      // every element is the buffer's
        float *first = b.p;
        CHECK(b.grow(100) == 0 && b.p == first && b.cap == 100);
        CHECK(b.grow(7) == 0 && b.p == first && b.cap == 100 && g_allocs == 1 && g_frees == 0);
        CHECK(b.grow(101) == 0 && b.cap == 101 && g_allocs == 2 && g_frees == 1 && g_live == 1);   // the old block went, once
        b.p[100] = 1.f;
        float *q = b;                                               // the view the call sites use
        CHECK(q == b.p);
        // a failed growth leaves {nullptr, 0} and has released the old block
        g_fail_next = true;
        CHECK(b.grow(1000) == -3 && b.p == nullptr && b.cap == 0 && g_frees == 2 && g_live == 0);
        CHECK(b.grow(5) == 0 && b.cap == 5 && g_live == 1);         // ... and the buffer is usable again
        b.reset();
        CHECK(b.p == nullptr && b.cap == 0 && g_live == 0);
        b.reset();                                                  // (idempotent)
        CHECK(g_live == 0);
    }
    {   // move construction and assignment leave the source empty and free the target's old block once
        DevBuf<int> a;
        CHECK(a.grow(10) == 0);
        int *pa = a.p;
        DevBuf<int> m(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && m.p == pa && m.cap == 10 && g_live == 1);
        DevBuf<int> t;
        CHECK(t.grow(20) == 0 && g_live == 2);
        const int frees = g_frees;
        t = std::move(m);
        CHECK(m.p == nullptr && m.cap == 0 && t.p == pa && t.cap == 10 && g_frees == frees + 1 && g_live == 1);
        DevBuf<int> &self = t;
        t = std::move(self);                                        // self-assignment keeps the block
        CHECK(t.p == pa && t.cap == 10 && g_live == 1);
        t = DevBuf<int>();                                          // from an empty one: the block goes
        CHECK(t.p == nullptr && g_live == 0);
    }
    {   // destroying a struct of several owners brings the live counter to 0
        {
            Several s;
            CHECK(s.a.grow(3) == 0 && s.b.grow(4) == 0 && s.c[0].grow(1) == 0 && s.c[2].grow(9) == 0 && g_live == 4);
            g_fail_next = true;
            CHECK(s.c[1].grow(2) != 0 && g_live == 4);               // one member's failure leaves the others alone
        }
        CHECK(g_live == 0 && g_allocs == g_frees);
    }
    {   // a second release function: the handle is given to the owner, which releases it through that function only
        const int frees = g_frees;
        {
            DevBuf<char, other_release> h;
            h.p = static_cast<char *>(std::malloc(8));
            DevBuf<char, other_release> h2(std::move(h));
            CHECK(h.p == nullptr && h2.p != nullptr);
        }
        CHECK(g_other_released == 1 && g_frees == frees);
    }
    if (g_failed) return 1;
    std::puts("devbuf_host_test: ok");
    return 0;
}
