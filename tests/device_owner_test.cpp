// CPU test of csrc/device_owner.h (tests/test_device_owner_cpu.py builds this with g++ -fsanitize=address,undefined and runs it):
// the header the library compiles, instantiated over a backend that keeps a table of live objects, logs every destruction in
// order and fails the k-th malloc / memset on request.  Usage: device_owner_test CASE; exit status 0 and a line "ok CASE" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "device_owner.h"

static std::string g_error;
void ch_set_error(const std::string &msg) { g_error = msg; }

struct Fake {
    using stream_t = int *;
    using event_t = long *;
    std::map<void *, size_t> live;          // device blocks: pointer -> size
    std::set<void *> host, streams, events;
    std::vector<char> log;                  // destruction order: 'e'vent, 's'tream, 'h'ost block, 'm'emory block
    int mallocs = 0, memsets = 0, frees = 0, bad_frees = 0;
    int fail_malloc_at = 0, fail_memset_at = 0;   // 1-based index of the call that fails; 0 = none
} F;

struct FakeApi {
    using stream_t = Fake::stream_t;
    using event_t = Fake::event_t;
    static void *malloc(size_t bytes) {
        if (++F.mallocs == F.fail_malloc_at) return nullptr;
        void *p = ::malloc(bytes ? bytes : 1);
        memset(p, 0xab, bytes);
        F.live[p] = bytes;
        return p;
    }
    static bool free(void *p) {
        F.log.push_back('m');
        if (!F.live.count(p)) {   // double free, or a pointer that was never handed out
            F.bad_frees++;
            return false;
        }
        F.live.erase(p);
        F.frees++;
        ::free(p);
        return true;
    }
    static bool memset_zero(void *p, size_t bytes) {
        if (++F.memsets == F.fail_memset_at) return false;
        memset(p, 0, bytes);
        return true;
    }
    static void *host_malloc(size_t bytes) {
        void *p = ::malloc(bytes);
        F.host.insert(p);
        return p;
    }
    static void host_free(void *p) {
        F.log.push_back('h');
        if (!F.host.erase(p)) F.bad_frees++;
        else ::free(p);
    }
    static stream_t stream_create(unsigned) {
        stream_t s = new int(0);
        F.streams.insert(s);
        return s;
    }
    static void stream_destroy(stream_t s) {
        F.log.push_back('s');
        if (!F.streams.erase(s)) F.bad_frees++;
        else delete s;
    }
    static event_t event_create(unsigned) {
        event_t e = new long(0);
        F.events.insert(e);
        return e;
    }
    static void event_destroy(event_t e) {
        F.log.push_back('e');
        if (!F.events.erase(e)) F.bad_frees++;
        else delete e;
    }
};
using Owner = ChDeviceOwnerT<FakeApi>;
using Temp = ChDeviceTempT<FakeApi>;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static void nothing_left() {
    CHECK(F.live.empty() && F.host.empty() && F.streams.empty() && F.events.empty());
    CHECK(F.bad_frees == 0);
}

static const int N = 7;
static size_t size_of(int i) { return 100 + 24 * (size_t)i; }

static void case_destructor_frees_each_block_once() {
    {
        Owner o;
        size_t sum = 0;
        for (int i = 0; i < N; ++i) {
            char *p = (char *)o.alloc(size_of(i), i % 2 == 1);
            CHECK(p != nullptr);
            if (i % 2 == 1) CHECK(p[0] == 0 && p[size_of(i) - 1] == 0);
            sum += size_of(i);
        }
        CHECK(o.bytes() == sum && F.live.size() == (size_t)N && F.frees == 0);
    }
    CHECK(F.frees == N);
    nothing_left();
}

// the k-th malloc (memset) of N zero-filled allocations fails, for every k
static void case_failure_at_every_k(bool in_memset) {
    for (int k = 1; k <= N; ++k) {
        F = Fake();
        (in_memset ? F.fail_memset_at : F.fail_malloc_at) = k;
        {
            Owner o;
            size_t sum = 0;
            for (int i = 1; i <= N; ++i) {
                g_error.clear();
                void *p = o.alloc(size_of(i), true);
                if (i == k) {
                    CHECK(p == nullptr && !g_error.empty());
                } else {
                    CHECK(p != nullptr && g_error.empty());
                    sum += size_of(i);
                }
                CHECK(o.bytes() == sum);   // the failed block is not counted, before or after
            }
            // a block whose zero-fill failed is still owned: it is live until the owner goes
            CHECK(F.live.size() == (size_t)(in_memset ? N : N - 1));
        }
        CHECK(F.frees == (in_memset ? N : N - 1));
        nothing_left();
    }
}

static void case_release() {
    {
        Owner o;
        void *a = o.alloc(300), *b = o.alloc(500), *c = o.alloc(700);
        CHECK(a && b && c && o.bytes() == 1500);
        CHECK(o.release(b) == 0);
        CHECK(o.bytes() == 1000 && F.frees == 1 && !F.live.count(b) && F.live.size() == 2);
        g_error.clear();
        CHECK(o.release(b) != 0 && !g_error.empty());   // no longer owned: refused, not freed again
        CHECK(F.frees == 1 && F.bad_frees == 0 && o.bytes() == 1000);
    }
    CHECK(F.frees == 3);   // a and c once each; b not again
    nothing_left();
}

static void case_release_foreign_pointer() {
    void *foreign = FakeApi::malloc(64);   // live in the backend, but no block of the owner
    int local = 0;
    {
        Owner o;
        void *a = o.alloc(128);
        CHECK(a != nullptr);
        g_error.clear();
        CHECK(o.release(foreign) != 0 && !g_error.empty());
        CHECK(o.release(&local) != 0 && o.release(nullptr) != 0 && o.release((char *)a + 8) != 0);
        CHECK(F.frees == 0 && F.bad_frees == 0 && F.log.empty() && o.bytes() == 128 && F.live.count(foreign));
    }
    CHECK(F.frees == 1 && F.live.count(foreign));
    CHECK(FakeApi::free(foreign));
    nothing_left();
}

static void case_zero_bytes_count_16() {
    {
        Owner o;
        void *p = o.alloc(0), *q = o.alloc(0, true);
        CHECK(p && q && p != q && o.bytes() == 32 && F.live[p] == 16 && F.live[q] == 16);
        CHECK(o.release(p) == 0 && o.bytes() == 16);
    }
    nothing_left();
}

static void case_streams_and_events_go_before_memory() {
    {
        Owner o;
        CHECK(o.alloc(64) != nullptr);
        Owner::event_t e0 = o.event(2);
        Owner::stream_t s0 = o.stream(1);
        CHECK(o.alloc(64, true) != nullptr);
        CHECK(o.host_alloc(256) != nullptr);
        Owner::event_t e1 = o.event();
        Owner::stream_t s1 = o.stream(1);
        CHECK(o.alloc(64) != nullptr);
        CHECK(e0 && e1 && e0 != e1 && s0 && s1 && s0 != s1);
        CHECK(F.events.size() == 2 && F.streams.size() == 2 && F.host.size() == 1 && F.log.empty());
        CHECK(o.bytes() == 192);   // device blocks only
    }
    CHECK(std::string(F.log.begin(), F.log.end()) == "eesshmmm");   // each once; events, then streams, then memory
    nothing_left();
}

static int temp_user(int leave_at, size_t bytes) {
    Temp a, b;
    if (a.get(bytes)) return 1;
    if (leave_at == 1) return 10;
    if (b.get(bytes)) return 1;   // (a is freed although b could not be had)
    if (leave_at == 2) return 20;
    memset(a.as<char>(), 1, bytes);
    memset(b.as<char>(), 2, bytes);
    return 0;
}
static void case_temp_frees_on_every_path() {
    CHECK(temp_user(0, 96) == 0 && F.frees == 2);
    nothing_left();
    CHECK(temp_user(1, 96) == 10 && F.frees == 3);
    nothing_left();
    CHECK(temp_user(2, 96) == 20 && F.frees == 5);
    nothing_left();
    F = Fake();
    F.fail_malloc_at = 2;
    g_error.clear();
    CHECK(temp_user(0, 96) == 1 && !g_error.empty() && F.frees == 1);
    nothing_left();
    F = Fake();
    F.fail_malloc_at = 1;
    CHECK(temp_user(0, 96) == 1 && F.frees == 0 && F.log.empty());
    nothing_left();
}

// what ensure_bytes (model.hip) does with a staging buffer that has to grow
static void case_regrow() {
    {
        Owner o;
        CHECK(o.alloc(40) != nullptr);
        void *buf = nullptr;
        size_t have = 0;
        CHECK(o.regrow(&buf, &have, 1000) == 0 && buf && have == 1000 && o.bytes() == 1040);
        void *first = buf;
        CHECK(o.regrow(&buf, &have, 4000) == 0 && buf && have == 4000 && o.bytes() == 4040);
        CHECK(!F.live.count(first) || buf == first);   // the old block went back (the allocator may hand the address out again)
        CHECK(F.frees == 1 && F.live.size() == 2);
        F.fail_malloc_at = F.mallocs + 1;              // the next growth: release succeeds, alloc fails
        g_error.clear();
        CHECK(o.regrow(&buf, &have, 9000) != 0 && !g_error.empty());
        CHECK(buf == nullptr && have == 0 && o.bytes() == 40 && F.frees == 2 && F.live.size() == 1);
        // the next call, with a SMALLER need, must allocate: there is no block to mistake for a live one
        CHECK(o.regrow(&buf, &have, 500) == 0 && buf && have == 500 && o.bytes() == 540);
        memset(buf, 3, 500);
    }
    CHECK(F.frees == 4);
    nothing_left();
}

int main(int argc, char **argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "destructor") case_destructor_frees_each_block_once();
    else if (which == "malloc_failure") case_failure_at_every_k(false);
    else if (which == "memset_failure") case_failure_at_every_k(true);
    else if (which == "release") case_release();
    else if (which == "release_foreign") case_release_foreign_pointer();
    else if (which == "zero_bytes") case_zero_bytes_count_16();
    else if (which == "destruction_order") case_streams_and_events_go_before_memory();
    else if (which == "temp") case_temp_frees_on_every_path();
    else if (which == "regrow") case_regrow();
    else {
        printf("unknown case '%s'\n", which.c_str());
        return 2;
    }
    printf("ok %s\n", which.c_str());
    return 0;
}
