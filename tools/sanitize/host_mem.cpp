// ASan + UBSan over wrenc_amd/csrc/host_mem.h: DevBuf against stub definitions of the three HIP calls it uses (malloc and
// free behind them, a count of live allocations, a switch that makes the k-th allocation fail and leaves HIP's error
// pending).  A double free or a leak is the sanitizer's to report.  Stand-alone (tools/sanitize/run.sh builds and runs it,
// no HIP library linked); never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../wrenc_amd/csrc/host_mem.h"

static int g_live = 0, g_allocs = 0, g_fail_at = 0; // g_fail_at: the allocation (1-based, counted from arm()) that fails
static hipError_t g_pending = hipSuccess;

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    ++g_allocs;
    if (g_allocs == g_fail_at) {
        *p = (void*)16; // (a failed call's pointer is not to be kept)
        return g_pending = hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    ++g_live;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
    free(p);
    --g_live;
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) {
    const hipError_t e = g_pending;
    g_pending = hipSuccess;
    return e;
}

static void arm(int fail_at) {
    g_allocs = 0;
    g_fail_at = fail_at;
}

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "host_mem: line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                          \
        }                                                                      \
    } while (0)

using wrenc::DevBuf;

struct Several { // a context in small
    DevBuf<char> a;
    DevBuf<int> b[3];
    DevBuf<double> c;
};
static hipError_t fill(Several& s) {
    if (hipError_t e = s.a.alloc(10)) return e;
    for (DevBuf<int>& b : s.b)
        if (hipError_t e = b.alloc(7)) return e;
    return s.c.alloc(3);
}

// the search scratch of wrenc_gpu_encode: into locals, then both into the holder or neither
struct Pair {
    DevBuf<char> scratch;
    DevBuf<long> map;
};
static hipError_t make_pair(Pair& p) {
    DevBuf<char> scratch;
    DevBuf<long> map;
    if (hipError_t e = scratch.alloc(100)) return e;
    if (hipError_t e = map.alloc(5)) return e;
    map.get()[4] = 0;
    p.scratch = std::move(scratch);
    p.map = std::move(map);
    return hipSuccess;
}

int main() {
    arm(0);
    {
        DevBuf<int> b;
        CHECK(!b && b.get() == nullptr && b.count() == 0);
        CHECK(b.alloc(8) == hipSuccess && b && b.count() == 8 && g_live == 1);
        b.get()[7] = 1;
        CHECK(b.alloc(4) == hipSuccess && b.count() == 4 && g_live == 1); // alloc over a held buffer frees the old one
        // grow: below or at the held count nothing is allocated, above it once
        int* held = b.get();
        arm(0);
        CHECK(b.grow(3) == hipSuccess && b.grow(4) == hipSuccess && g_allocs == 0 && b.get() == held && b.count() == 4);
        CHECK(b.grow(9) == hipSuccess && g_allocs == 1 && b.count() == 9 && g_live == 1);
        b.get()[8] = 2;
        // a failed alloc and a failed grow hold nothing and leave no error pending
        arm(1);
        CHECK(b.alloc(5) == hipErrorOutOfMemory && !b && b.get() == nullptr && b.count() == 0 && g_live == 0 && g_pending == hipSuccess);
        arm(0);
        CHECK(b.grow(2) == hipSuccess && g_live == 1);
        arm(1);
        CHECK(b.grow(6) == hipErrorOutOfMemory && !b && b.count() == 0 && g_live == 0 && g_pending == hipSuccess);
        arm(0);
        CHECK(b.grow(6) == hipSuccess && b.count() == 6); // usable again
        b.reset();
        CHECK(!b && b.count() == 0 && g_live == 0);
        b.reset();
        CHECK(b.alloc(2) == hipSuccess && g_live == 1);
    } // the destructor frees
    CHECK(g_live == 0);
    {
        // moves leave one owner
        DevBuf<int> a;
        CHECK(a.alloc(3) == hipSuccess);
        int* p = a.get();
        DevBuf<int> b(std::move(a));
        CHECK(!a && a.count() == 0 && b.get() == p && b.count() == 3 && g_live == 1);
        DevBuf<int> c;
        CHECK(c.alloc(5) == hipSuccess && g_live == 2);
        c = std::move(b); // what c held is freed
        CHECK(!b && c.get() == p && c.count() == 3 && g_live == 1);
        DevBuf<int>& self = c;
        c = std::move(self);
        CHECK(c.get() == p && g_live == 1);
    }
    CHECK(g_live == 0);
    // several buffers in one holder, the k-th allocation failing: nothing is left once the holder is gone
    for (int k = 1; k <= 6; ++k) {
        arm(k);
        {
            Several s;
            const hipError_t e = fill(s);
            CHECK((e == hipSuccess) == (k == 6) && g_live == (k == 6 ? 5 : k - 1) && g_pending == hipSuccess);
        }
        CHECK(g_live == 0);
    }
    // both or neither
    {
        Pair p;
        for (int k = 1; k <= 2; ++k) {
            arm(k);
            CHECK(make_pair(p) == hipErrorOutOfMemory && !p.scratch && !p.map && g_live == 0 && g_pending == hipSuccess);
        }
        arm(0);
        CHECK(make_pair(p) == hipSuccess && p.scratch && p.map && p.scratch.count() == 100 && p.map.count() == 5 && g_live == 2);
    }
    CHECK(g_live == 0);
    printf("host_mem: DevBuf clean, no live allocation at exit\n");
    return 0;
}
