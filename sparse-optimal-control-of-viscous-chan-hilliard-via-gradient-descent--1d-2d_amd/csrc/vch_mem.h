// vch_mem.h — who owns the engines' device and pinned-host memory (host only: no HIP header, a plain C++ compiler builds
// it for tests/mem_pool_main.cpp).
//
// Every context has one vch_pool.  An allocation is made INTO an owner pointer (a field of the context, as a rule) and the
// pool remembers that owner, so whatever frees a block also sets its owner back to NULL.  release() frees everything the
// pool handed out; mark() / rollback() free what came after a mark, which is how a lazy group of buffers is made
// all-or-nothing (vch_group) and how a call's temporary goes away on every path out of it.
#pragma once
#include <atomic>
#include <stddef.h>
#include <vector>
#include "../../include/vch.h"

// The runtime behind a pool.  Each function returns the runtime's own status, 0 = success.
struct vch_mem_fns {
    int (*dev_alloc)(void **p, size_t bytes);
    int (*dev_free)(void *p);
    int (*host_alloc)(void **p, size_t bytes, unsigned flags);
    int (*host_free)(void *p);
};
constexpr int VCH_MEM_REFUSED = 2;        // what a refused request reports: hipErrorOutOfMemory (asserted beside the HIP table)

// process-wide diagnostics (include/vch.h): blocks owned by pools now, and the countdown to the one refused request
inline std::atomic<int> g_vch_mem_live{0}, g_vch_mem_refuse{-1};
extern "C" __attribute__((used, visibility("default"))) inline int vch_mem_live(void) { return g_vch_mem_live.load(); }
extern "C" __attribute__((used, visibility("default"))) inline void vch_mem_refuse_after(int k) { g_vch_mem_refuse.store(k < 0 ? -1 : k); }

class vch_pool {
    struct rec { void **owner; bool host; };
    const vch_mem_fns *fns;
    std::vector<rec> recs;

    int get(void **owner, size_t bytes, bool host, unsigned flags) {
        *owner = nullptr;
        // the armed request is refused before the runtime hears of it, and the countdown ends at -1: disarmed
        const bool refused = g_vch_mem_refuse.load() >= 0 && g_vch_mem_refuse.fetch_sub(1) == 0;
        const int e = refused ? VCH_MEM_REFUSED : host ? fns->host_alloc(owner, bytes, flags) : fns->dev_alloc(owner, bytes);
        if (e != 0) {
            *owner = nullptr;
            return e;
        }
        recs.push_back(rec{owner, host});
        ++g_vch_mem_live;
        return 0;
    }

public:
    explicit vch_pool(const vch_mem_fns *f) : fns(f) {}
    vch_pool(const vch_pool &) = delete;
    vch_pool &operator=(const vch_pool &) = delete;
    ~vch_pool() { release(); }

    // *owner = a new block (device / pinned host), or NULL and the runtime's status.  The owner must outlive the block.
    template <class T> int dev(T **owner, size_t bytes) { return get((void **)owner, bytes, false, 0); }
    template <class T> int host(T **owner, size_t bytes, unsigned flags = 0) { return get((void **)owner, bytes, true, flags); }

    size_t mark() const { return recs.size(); }
    // free, newest first, what was allocated since mark() returned m, and NULL the owners
    void rollback(size_t m) {
        while (recs.size() > m) {
            const rec r = recs.back();
            recs.pop_back();
            (r.host ? fns->host_free : fns->dev_free)(*r.owner);
            *r.owner = nullptr;
            --g_vch_mem_live;
        }
    }
    void release() { rollback(0); }
    // free the one block made into `owner` (any age) and NULL the owner; not inside a vch_group's scope, whose mark counts
    // the blocks in front of it
    void drop(void **owner) {
        for (size_t i = 0; i < recs.size(); ++i)
            if (recs[i].owner == owner) {
                (recs[i].host ? fns->host_free : fns->dev_free)(*owner);
                *owner = nullptr;
                recs.erase(recs.begin() + (long)i);
                --g_vch_mem_live;
                return;
            }
    }
};

// What a scope allocates goes away with the scope unless keep() is reached: a lazy group whose second member was refused
// leaves every pointer of the group NULL (the next call allocates again), and a temporary never calls keep().
class vch_group {
    vch_pool &pool;
    const size_t m;
    bool kept = false;

public:
    explicit vch_group(vch_pool &p) : pool(p), m(p.mark()) {}
    vch_group(const vch_group &) = delete;
    ~vch_group() { if (!kept) pool.rollback(m); }
    int keep() { kept = true; return 0; }
};
