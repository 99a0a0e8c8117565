// Host check of the resource pool's policy (egobox_amd/csrc/resource_pool.h): keys, least-recently-returned order, slabs-before-
// handles eviction and the per-device bound, with made-up byte sizes and an int for a payload.  Built and run by
// tests/test_tile_tables_cpu.py (g++, no GPU).
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../egobox_amd/csrc/resource_pool.h"

using Pool = egx::ResourcePool<int>;

static int fails = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #cond);             \
            fails++;                                                   \
        }                                                              \
    } while (0)

static egx::PoolKey handle_key(int device, int n_pad, bool member = false, int nws = 1) {
    egx::PoolKey k;
    k.device = device, k.n_pad = n_pad, k.d = 3, k.q = 2, k.hmax = 1, k.nws = nws, k.member = member;
    return k;
}
static egx::PoolKey slabs_key(int device, size_t bM, size_t bD, size_t bI) {
    egx::PoolKey k;
    k.slabs = true, k.device = device, k.bytes_M = bM, k.bytes_D = bD, k.bytes_I = bI;
    return k;
}
static Pool::Entry entry(const egx::PoolKey &k, size_t bytes, int id) {
    Pool::Entry e;
    e.key = k, e.bytes = bytes, e.res = id;
    return e;
}
// the payloads of what a call handed back to be freed, in the order of the list
static std::vector<int> ids(const Pool::List &l) {
    std::vector<int> v;
    for (const auto &e : l) v.push_back(e.res);
    return v;
}
static int64_t cached(Pool &p) {
    int64_t b = 0;
    p.stats(&b, nullptr, nullptr);
    return b;
}
static size_t count(Pool &p) {
    size_t n = 0;
    p.stats(nullptr, nullptr, nullptr, &n);
    return n;
}

int main() {
    const size_t cap = 1000;
    int got = 0;
    {   // keys: a member's entry never serves a lone handle of the same shape, nor the reverse; every shape field and the device count
        Pool p;
        CHECK(p.give(entry(handle_key(0, 1024, true), 10, 1), true, cap).empty());
        CHECK(!p.take(handle_key(0, 1024, false), got));
        CHECK(p.take(handle_key(0, 1024, true), got) && got == 1);
        CHECK(p.give(entry(handle_key(0, 1024, false), 10, 2), true, cap).empty());
        CHECK(!p.take(handle_key(0, 1024, true), got));
        CHECK(!p.take(handle_key(1, 1024, false), got));
        CHECK(!p.take(handle_key(0, 1152, false), got));
        CHECK(!p.take(handle_key(0, 1024, false, 2), got));
        egx::PoolKey gls = handle_key(0, 1024, false);
        gls.gls = true;
        CHECK(!p.take(gls, got));
        CHECK(p.take(handle_key(0, 1024, false), got) && got == 2);
        int64_t hits = 0, misses = 0;
        p.stats(nullptr, &hits, &misses);
        CHECK(hits == 2 && misses == 6 && count(p) == 0);
    }
    {   // a group's slabs match on all three sizes and the device only, and never serve a handle
        Pool p;
        CHECK(p.give(entry(slabs_key(0, 400, 40, 4), 444, 7), true, cap).empty());
        CHECK(!p.take(slabs_key(0, 401, 40, 4), got));
        CHECK(!p.take(slabs_key(0, 400, 41, 4), got));
        CHECK(!p.take(slabs_key(0, 400, 40, 5), got));
        CHECK(!p.take(slabs_key(1, 400, 40, 4), got));
        CHECK(!p.take(handle_key(0, 0), got));
        CHECK(p.take(slabs_key(0, 400, 40, 4), got) && got == 7);
        CHECK(!p.take(slabs_key(0, 400, 40, 4), got));
    }
    {   // least recently returned: of two entries of one key the later one is taken first; eviction takes the earliest first
        Pool p;
        for (int id = 1; id <= 4; id++) CHECK(p.give(entry(handle_key(0, 1024), 300, id), true, cap).size() == (id == 4 ? 1u : 0u));
        CHECK(cached(p) == 900 && count(p) == 3);  // (1 went when 4 came)
        CHECK(p.take(handle_key(0, 1024), got) && got == 4);
        CHECK(p.take(handle_key(0, 1024), got) && got == 3);
        CHECK(p.give(entry(handle_key(0, 2048), 800, 5), true, cap) .size() == 1 && cached(p) == 800);  // 2 went, the newcomer stays
        CHECK(!p.take(handle_key(0, 1024), got));
    }
    {   // bare slabs go before handle entries, whichever kind the newcomer is; within a kind the oldest first
        Pool p;
        p.give(entry(slabs_key(0, 100, 10, 1), 200, 1), true, cap);
        p.give(entry(handle_key(0, 1024), 200, 2), true, cap);
        p.give(entry(slabs_key(0, 200, 10, 1), 200, 3), true, cap);
        p.give(entry(handle_key(0, 2048), 200, 4), true, cap);
        CHECK(ids(p.give(entry(handle_key(0, 4096), 500, 5), true, cap)) == std::vector<int>({3, 1}));  // (1 went first)
        CHECK(cached(p) == 900);
        CHECK(ids(p.give(entry(slabs_key(0, 300, 10, 1), 500, 6), true, cap)) == std::vector<int>({4, 2}));  // the newcomer, a slab, is spared
        CHECK(cached(p) == 1000 && count(p) == 2);
        CHECK(ids(p.give(entry(slabs_key(0, 400, 10, 1), 100, 7), true, cap)) == std::vector<int>({6}));
        CHECK(p.take(handle_key(0, 4096), got) && got == 5);
        CHECK(p.take(slabs_key(0, 400, 10, 1), got) && got == 7);
    }
    {   // the bound is per device: pressure on device 0 leaves device 1 alone
        Pool p;
        p.give(entry(handle_key(1, 1024), 900, 1), true, cap);
        p.give(entry(slabs_key(1, 50, 5, 1), 56, 2), true, cap);
        p.give(entry(handle_key(0, 1024), 900, 3), true, cap);
        CHECK(cached(p) == 1856);
        CHECK(ids(p.give(entry(handle_key(0, 2048), 900, 4), true, cap)) == std::vector<int>({3}));
        CHECK(cached(p) == 1856);
        CHECK(p.take(handle_key(1, 1024), got) && got == 1);
        CHECK(p.take(slabs_key(1, 50, 5, 1), got) && got == 2);
    }
    {   // an entry larger than the bound, an incomplete one, and everything under a bound of 0 come straight back
        Pool p;
        p.give(entry(handle_key(0, 1024), 100, 1), true, cap);
        CHECK(ids(p.give(entry(handle_key(0, 8192), cap + 1, 2), true, cap)) == std::vector<int>({2}));
        CHECK(ids(p.give(entry(handle_key(0, 1024), 100, 3), false, cap)) == std::vector<int>({3}));
        CHECK(cached(p) == 100 && count(p) == 1);  // (and nothing was evicted for them)
        CHECK(p.give(entry(handle_key(0, 8192), cap, 4), true, cap).size() == 1 && cached(p) == (int64_t)cap);  // exactly the bound fits
        Pool z;
        CHECK(ids(z.give(entry(handle_key(0, 1024), 1, 5), true, 0)) == std::vector<int>({5}));
        CHECK(ids(z.give(entry(slabs_key(0, 1, 1, 1), 3, 6), true, 0)) == std::vector<int>({6}));
        CHECK(cached(z) == 0 && count(z) == 0);
    }
    {   // trim: one device, then all of them; the byte totals are what was pooled, the list ends empty
        Pool p;
        p.give(entry(handle_key(0, 1024), 100, 1), true, cap);
        p.give(entry(slabs_key(0, 10, 1, 1), 12, 2), true, cap);
        p.give(entry(handle_key(1, 1024), 300, 3), true, cap);
        p.give(entry(slabs_key(2, 10, 1, 1), 12, 4), true, cap);
        size_t bytes = 0;
        CHECK(p.trim(0, &bytes).size() == 2 && bytes == 112 && cached(p) == 312);
        CHECK(p.trim(0, &bytes).empty() && bytes == 0);
        CHECK(!p.take(handle_key(0, 1024), got));
        CHECK(p.trim(-1, &bytes).size() == 2 && bytes == 312 && cached(p) == 0 && count(p) == 0);
        CHECK(p.trim(-1, &bytes).empty() && bytes == 0);
    }
    if (fails) {
        std::printf("%d pool policy checks failed\n", fails);
        return 1;
    }
    std::printf("pool policy ok\n");
    return 0;
}
