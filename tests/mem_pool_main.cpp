// The engines' allocation pool (csrc/vch_mem.h) over a mock runtime built on malloc / free: tests/test_mem_pool_cpu.py compiles
// this with the address and undefined-behaviour sanitizers and runs `mem_pool <case>`.  The mock keeps its own books (what it
// handed out, what came back and in which order, how often it was called) and every check is made on those, not on a leak
// report at exit.
#include "vch_mem.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

struct Block { void *p; bool host; };
static std::vector<Block> g_handed, g_live, g_freed;      // in the order of the calls
static int g_alloc_calls = 0, g_free_calls = 0;
static unsigned g_last_flags = 0;

static int mock_alloc(void **p, size_t bytes, bool host) {
    ++g_alloc_calls;
    *p = malloc(bytes ? bytes : 1);
    CHECK(*p);
    memset(*p, host ? 0x5a : 0xa5, bytes);
    g_handed.push_back(Block{*p, host});
    g_live.push_back(Block{*p, host});
    return 0;
}
static int mock_free(void *p, bool host) {
    ++g_free_calls;
    auto it = std::find_if(g_live.begin(), g_live.end(), [&](const Block &b) { return b.p == p; });
    CHECK(it != g_live.end());            // a pointer the mock handed out and has not seen back yet
    CHECK(it->host == host);              // through the free function of its own kind
    g_freed.push_back(*it);
    g_live.erase(it);
    free(p);
    return 0;
}
static const vch_mem_fns MOCK = {[](void **p, size_t n) { return mock_alloc(p, n, false); }, [](void *p) { return mock_free(p, false); },
                                 [](void **p, size_t n, unsigned f) { g_last_flags = f; return mock_alloc(p, n, true); },
                                 [](void *p) { return mock_free(p, true); }};

static void reset_books() {
    CHECK(g_live.empty());
    g_handed.clear();
    g_freed.clear();
    g_alloc_calls = g_free_calls = 0;
}

// twelve owners of four types, as a context has them; request i is a pinned-host one for i = 3, 7, 8, 11
struct Owners {
    double *a = nullptr, *ring[3] = {nullptr, nullptr, nullptr};
    int *stats = nullptr;
    unsigned long long *cells = nullptr;
    double *h0 = nullptr, *h1 = nullptr;
    int *hstats = nullptr;
    char *mapped = nullptr;
    float *f0 = nullptr, *f1 = nullptr;
    void *at(int i) const {
        void *const all[12] = {a, ring[0], ring[1], h0, ring[2], stats, cells, h1, hstats, f0, f1, mapped};
        return all[i];
    }
};
// the twelve requests, stopping at the first that fails as vchNd_create does: -> its index, or -1
static int twelve(vch_pool &pool, Owners &o) {
    int i = 0;
    if (pool.dev(&o.a, 640)) return i;
    ++i; if (pool.dev(&o.ring[0], 64)) return i;
    ++i; if (pool.dev(&o.ring[1], 64)) return i;
    ++i; if (pool.host(&o.h0, 256)) return i;
    ++i; if (pool.dev(&o.ring[2], 64)) return i;
    ++i; if (pool.dev(&o.stats, 32)) return i;
    ++i; if (pool.dev(&o.cells, 128)) return i;
    ++i; if (pool.host(&o.h1, 8)) return i;
    ++i; if (pool.host(&o.hstats, 32)) return i;
    ++i; if (pool.dev(&o.f0, 4)) return i;
    ++i; if (pool.dev(&o.f1, 12)) return i;
    ++i; if (pool.host(&o.mapped, 64, 6u)) return i;
    return -1;
}
static bool is_host(int i) { return i == 3 || i == 7 || i == 8 || i == 11; }

static void case_release() {
    reset_books();
    vch_pool pool(&MOCK);
    Owners o;
    CHECK(twelve(pool, o) == -1);
    CHECK(g_last_flags == 6u);                            // the flags of a host request reach the runtime
    CHECK(g_alloc_calls == 12 && g_handed.size() == 12 && vch_mem_live() == 12);
    for (int i = 0; i < 12; ++i) CHECK(o.at(i) == g_handed[i].p && g_handed[i].host == is_host(i));
    pool.release();
    CHECK(g_free_calls == 12 && g_freed.size() == 12 && g_live.empty());      // every block once (mock_free checks "once")
    for (int i = 0; i < 12; ++i) CHECK(g_freed[i].p == g_handed[11 - i].p);   // newest first
    for (int i = 0; i < 12; ++i) CHECK(o.at(i) == nullptr);
    CHECK(vch_mem_live() == 0);
    pool.release();                                       // nothing left to do
    CHECK(g_free_calls == 12 && vch_mem_live() == 0);
}

static void case_refused_create() {
    for (int k = 0; k < 12; ++k) {
        reset_books();
        {
            vch_pool pool(&MOCK);
            Owners o;
            vch_mem_refuse_after(k);
            CHECK(twelve(pool, o) == k);
            CHECK(g_alloc_calls == k);                    // the runtime never heard of the refused request
            CHECK(vch_mem_live() == k && (int)g_live.size() == k);
            for (int i = 0; i < 12; ++i) CHECK((o.at(i) != nullptr) == (i < k));
            pool.release();                               // what a failed create does
            CHECK(vch_mem_live() == 0 && g_live.empty() && g_free_calls == k);
            for (int i = 0; i < 12; ++i) CHECK(o.at(i) == nullptr);
            for (int i = 0; i < k; ++i) CHECK(g_freed[i].p == g_handed[k - 1 - i].p);
        }                                                 // and the pool's destructor finds nothing
        CHECK(g_free_calls == k);
    }
}

struct Lazy { double *part = nullptr, *lvl = nullptr, *lvl_host = nullptr; };
// a lazy group as the engines write one
static int ensure_group(vch_pool &pool, Lazy &z) {
    if (z.part) return 0;
    vch_group g(pool);
    if (int e = pool.dev(&z.part, 96)) return e;
    if (int e = pool.dev(&z.lvl, 48)) return e;
    if (int e = pool.host(&z.lvl_host, 48)) return e;
    return g.keep();
}

static void case_group() {
    reset_books();
    vch_pool pool(&MOCK);
    double *early0 = nullptr, *early1 = nullptr;
    CHECK(pool.dev(&early0, 80) == 0 && pool.host(&early1, 80) == 0);
    for (int i = 0; i < 10; ++i) { early0[i] = 1.5 * i; early1[i] = -2.0 * i; }
    double *const keep0 = early0, *const keep1 = early1;
    auto early_intact = [&]() {
        CHECK(early0 == keep0 && early1 == keep1 && g_live.size() >= 2 && g_live[0].p == keep0 && g_live[1].p == keep1);
        for (int i = 0; i < 10; ++i) CHECK(early0[i] == 1.5 * i && early1[i] == -2.0 * i);
    };
    Lazy z;
    for (int j = 0; j < 3; ++j) {
        // by hand with mark() / rollback() ...
        vch_mem_refuse_after(j);
        const size_t m = pool.mark();
        const bool failed = pool.dev(&z.part, 96) || pool.dev(&z.lvl, 48) || pool.host(&z.lvl_host, 48);
        CHECK(failed);
        pool.rollback(m);
        CHECK(!z.part && !z.lvl && !z.lvl_host && vch_mem_live() == 2 && g_live.size() == 2);
        early_intact();
        // ... and through the guard
        vch_mem_refuse_after(j);
        CHECK(ensure_group(pool, z) == VCH_MEM_REFUSED);
        CHECK(!z.part && !z.lvl && !z.lvl_host && vch_mem_live() == 2 && g_live.size() == 2);
        early_intact();
    }
    CHECK(ensure_group(pool, z) == 0);                    // the retry
    CHECK(z.part && z.lvl && z.lvl_host && vch_mem_live() == 5 && g_live.size() == 5);
    const int calls = g_alloc_calls;
    CHECK(ensure_group(pool, z) == 0 && g_alloc_calls == calls);
    early_intact();
    {                                                     // a temporary: a group that is never kept
        double *tmp = nullptr;
        vch_group scope(pool);
        CHECK(pool.dev(&tmp, 1024) == 0 && vch_mem_live() == 6);
    }
    CHECK(vch_mem_live() == 5 && g_live.size() == 5);
    early_intact();
    pool.release();
    CHECK(vch_mem_live() == 0 && g_live.empty() && !early0 && !early1 && !z.part && !z.lvl && !z.lvl_host);
}

static void case_disarm() {
    reset_books();
    vch_pool pool(&MOCK);
    double *p[4] = {nullptr, nullptr, nullptr, nullptr};
    vch_mem_refuse_after(0);
    CHECK(pool.dev(&p[0], 8) == VCH_MEM_REFUSED && !p[0] && g_alloc_calls == 0);
    CHECK(pool.dev(&p[0], 8) == 0 && p[0]);               // the refusal was for one request
    vch_mem_refuse_after(1);
    CHECK(pool.host(&p[1], 8) == 0 && pool.host(&p[2], 8) == VCH_MEM_REFUSED && !p[2]);
    CHECK(pool.host(&p[2], 8) == 0 && pool.dev(&p[3], 8) == 0);
    pool.release();
    vch_mem_refuse_after(2);
    vch_mem_refuse_after(-7);                             // disarmed by hand
    for (double *&q : p) CHECK(pool.dev(&q, 8) == 0);
    CHECK(vch_mem_live() == 4);
    pool.release();
    CHECK(vch_mem_live() == 0 && g_live.empty());
}

int main(int argc, char **argv) {
    const int which = argc > 1 ? atoi(argv[1]) : 0;
    void (*const cases[4])() = {case_release, case_refused_create, case_group, case_disarm};
    CHECK(which >= 1 && which <= 4);
    cases[which - 1]();
    CHECK(vch_mem_live() == 0 && g_live.empty());
    printf("ok %d\n", which);
    return 0;
}
