// ASan + UBSan over wrenc_amd/csrc/host_mem.h: DevBuf, HipStream and HipEvent against stub definitions of the HIP calls they
// use (malloc and free behind them, counts of live allocations and live handles, a switch that makes the k-th allocation
// or creation fail and leaves HIP's error pending).  A double free or a leak is the sanitizer's to report.  Stand-alone
// (tools/sanitize/run.sh builds and runs it, no HIP library linked); never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

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

// streams and events: a handle is a small allocation of its own (a double destroy or a leak is the sanitizer's to report);
// creations count with the allocations, so that arm() makes the k-th creation of any kind fail
static int g_live_handles = 0;
template <class H>
static hipError_t make_handle(H* h) {
    ++g_allocs;
    if (g_allocs == g_fail_at) {
        *h = (H)16;
        return g_pending = hipErrorOutOfMemory;
    }
    *h = (H)malloc(1);
    ++g_live_handles;
    return hipSuccess;
}
template <class H>
static hipError_t drop_handle(H h) {
    free((void*)h);
    --g_live_handles;
    return hipSuccess;
}
extern "C" hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return make_handle(s); }
extern "C" hipError_t hipStreamDestroy(hipStream_t s) { return drop_handle(s); }
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make_handle(e); }
extern "C" hipError_t hipEventDestroy(hipEvent_t e) { return drop_handle(e); }

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

using wrenc::HipEvent;
using wrenc::HipStream;

struct Handles { // the streams and events of a context in small, memory between them
    HipStream stream;
    HipEvent fork;
    std::vector<HipEvent> ring;
    std::vector<HipStream> lanes;
    DevBuf<int> mem;
    HipStream copy;
    HipEvent timing[2];
};
static hipError_t fill(Handles& h) { // 1 + 1 + 3 + 2 + 1 + 1 + 2 = 11 creations
    if (hipError_t e = h.stream.create(hipStreamNonBlocking)) return e;
    if (hipError_t e = h.fork.create()) return e;
    h.ring.resize(3);
    for (HipEvent& ev : h.ring)
        if (hipError_t e = ev.create(hipEventDisableTiming)) return e;
    h.lanes.resize(2);
    for (HipStream& s : h.lanes)
        if (hipError_t e = s.create(hipStreamNonBlocking)) return e;
    if (hipError_t e = h.mem.alloc(4)) return e;
    if (hipError_t e = h.copy.create(hipStreamNonBlocking)) return e;
    for (HipEvent& ev : h.timing)
        if (hipError_t e = ev.create()) return e;
    return hipSuccess;
}

template <class Handle>
static int handle_cases() {
    arm(0);
    {
        Handle a;
        CHECK(!a && a.get() == nullptr && g_live_handles == 0);
        CHECK(a.create() == hipSuccess && a && g_live_handles == 1);
        CHECK(a.create(1) == hipSuccess && a && g_live_handles == 1); // create over a held handle destroys the old one
        // a failed create holds nothing and leaves no error pending
        arm(1);
        CHECK(a.create() == hipErrorOutOfMemory && !a && a.get() == nullptr && g_live_handles == 0 && g_pending == hipSuccess);
        arm(0);
        CHECK(a.create() == hipSuccess && g_live_handles == 1); // usable again
        a.reset();
        CHECK(!a && g_live_handles == 0);
        a.reset();
        CHECK(a.create() == hipSuccess && g_live_handles == 1);
    } // the destructor destroys
    CHECK(g_live_handles == 0);
    {
        // moves leave one owner
        Handle a;
        CHECK(a.create() == hipSuccess);
        const auto h = a.get();
        Handle b(std::move(a));
        CHECK(!a && b.get() == h && g_live_handles == 1);
        Handle c;
        CHECK(c.create() == hipSuccess && g_live_handles == 2);
        c = std::move(b); // what c held is destroyed
        CHECK(!b && c.get() == h && g_live_handles == 1);
        Handle& self = c;
        c = std::move(self);
        CHECK(c.get() == h && g_live_handles == 1);
        // a growing vector moves its handles (the pool of timing events)
        std::vector<Handle> pool;
        for (int i = 0; i < 9; ++i) {
            Handle e;
            CHECK(e.create() == hipSuccess);
            pool.push_back(std::move(e));
        }
        CHECK(g_live_handles == 10);
    }
    CHECK(g_live_handles == 0);
    return 0;
}

int main() {
    if (handle_cases<HipStream>() || handle_cases<HipEvent>()) return 1;
    // the handles of one holder, the k-th creation failing: nothing is left once the holder is gone
    for (int k = 1; k <= 12; ++k) {
        arm(k);
        {
            Handles h;
            const hipError_t e = fill(h);
            CHECK((e == hipSuccess) == (k == 12) && g_live_handles + g_live == (k == 12 ? 11 : k - 1) && g_pending == hipSuccess);
        }
        CHECK(g_live_handles == 0 && g_live == 0);
    }
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
    CHECK(g_live_handles == 0);
    printf("host_mem: DevBuf, HipStream and HipEvent clean, no live allocation or handle at exit\n");
    return 0;
}
