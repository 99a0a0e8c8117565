// The policy of the resource pool (host-testable: no HIP in here; tests/c_host/pool_policy_test.cpp walks it with made-up byte
// sizes).  Destroyed handles and groups leave what they own on the device in ONE least-recently-returned list; gp_host.hip
// supplies the payload (its HandleRes) and frees whatever these functions hand back.
//
//   key      a handle's resources match on the shape of the handle (and never across lone handle / member of a group: a
//            member's entry has no slabs); a group's bare slabs match on their three sizes; both on the device
//   bound    `cap` bytes PER DEVICE.  give() evicts entries of the newcomer's device until the device is within the bound: bare
//            slabs before handle entries, within each kind the least recently returned first, never the newcomer itself.
//            An entry larger than the bound, or an incomplete one (a creation that failed half way), is not pooled at all
//   trim     everything of one device (-1: of every device) leaves the list
#pragma once
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <list>
#include <mutex>
#include <utility>

namespace egx {

struct PoolKey {
    bool slabs = false;  // a group's bare slabs (bytes_M / bytes_D / bytes_I), not a handle's resources (the shape fields)
    int device = 0;
    int n_pad = 0, d = 0, q = 0, hmax = 1, nws = 0;
    bool gls = false;
    bool member = false;  // a member of a group (egx_gp_create_group): everything but the slabs, which belong to the group
    size_t bytes_M = 0, bytes_D = 0, bytes_I = 0;
    bool operator==(const PoolKey &o) const {
        return slabs == o.slabs && device == o.device && n_pad == o.n_pad && d == o.d && q == o.q && hmax == o.hmax && nws == o.nws &&
               gls == o.gls && member == o.member && bytes_M == o.bytes_M && bytes_D == o.bytes_D && bytes_I == o.bytes_I;
    }
};

template <typename Payload>
class ResourcePool {
public:
    struct Entry {
        PoolKey key;
        size_t bytes = 0;
        Payload res;
    };
    using List = std::list<Entry>;

    // the most recently returned entry of this key moves into `out`; counts a hit or a miss
    bool take(const PoolKey &key, Payload &out) {
        std::lock_guard<std::mutex> lock(mu_);
        for (auto it = list_.begin(); it != list_.end(); ++it)
            if (it->key == key) {
                out = std::move(it->res);
                list_.erase(it);
                hits_++;
                return true;
            }
        misses_++;
        return false;
    }
    // returns what the caller has to free: the evicted entries, or the newcomer itself when it cannot be pooled
    List give(Entry e, bool complete, size_t cap) {
        List out;
        const int dev = e.key.device;
        const bool pooled = complete && e.bytes <= cap;
        std::lock_guard<std::mutex> lock(mu_);
        (pooled ? list_ : out).push_front(std::move(e));
        while (pooled && bytes_on(dev) > cap) {
            auto victim = list_.end();
            for (int want_slabs = 1; want_slabs >= 0 && victim == list_.end(); want_slabs--)
                for (auto it = std::next(list_.begin()); it != list_.end(); ++it)
                    if (it->key.device == dev && it->key.slabs == (want_slabs != 0)) victim = it;  // (the last one: the oldest)
            if (victim == list_.end()) break;
            out.splice(out.begin(), list_, victim);
        }
        return out;
    }
    List trim(int device, size_t *bytes) {
        List out;
        *bytes = 0;
        std::lock_guard<std::mutex> lock(mu_);
        for (auto it = list_.begin(); it != list_.end();) {
            auto next = std::next(it);
            if (device < 0 || it->key.device == device) {
                *bytes += it->bytes;
                out.splice(out.end(), list_, it);
            }
            it = next;
        }
        return out;
    }
    void stats(int64_t *cached_bytes, int64_t *hits, int64_t *misses, size_t *entries = nullptr) {
        std::lock_guard<std::mutex> lock(mu_);
        if (cached_bytes) *cached_bytes = (int64_t)bytes_on(-1);
        if (hits) *hits = hits_;
        if (misses) *misses = misses_;
        if (entries) *entries = list_.size();
    }

private:
    size_t bytes_on(int device) const {
        size_t b = 0;
        for (const auto &e : list_)
            if (device < 0 || e.key.device == device) b += e.bytes;
        return b;
    }
    std::mutex mu_;
    List list_;  // front = most recently returned
    int64_t hits_ = 0, misses_ = 0;
};

}  // namespace egx
