// The lock-step path's slot pipeline, kept free of HIP so that the CPU test tests/c_host/slot_pipeline_test.cpp can drive it
// with fake callbacks.  Both batch cores are clients: likelihood_batch_core (gp_host.hip, one phase per slot) and
// likelihood_grad_batch_core (gp_fit.hip, two: the likelihoods, then the gradient stages).
//
// The usable workspaces ws_lo .. ws_lo + nws - 1 of a handle form SLOTS of `width` consecutive ones (the last slot may hold
// fewer: 11 workspaces, width 4 -> 4 + 4 + 3).  The candidates of a slot are factored in lock-step by one launch sequence on
// the streams of the slot's first workspace; different slots run on their own stream sets, so the exposed serial parts of one
// slot overlap the trailing updates of another.  The slots are visited round-robin: a busy slot is advanced one phase, a slot
// that is idle (again) takes the next candidates the source hands out and is enqueued.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace egx {

// Where a batch takes its candidates from: the sequence 0 .. k-1, a rank's static shard or the node-wide counter of a
// dynamic sweep (sweep.hip).  pull() hands out up to `want` candidate indices, 0 = exhausted.
struct CandidateSource {
    virtual int pull(int want, int64_t *out) = 0;
    virtual ~CandidateSource() = default;
};
struct SequentialSource final : CandidateSource {
    int64_t k, next = 0;
    explicit SequentialSource(int64_t k_) : k(k_) {}
    int pull(int want, int64_t *out) override {
        int got = 0;
        while (got < want && next < k) out[got++] = next++;
        return got;
    }
};

struct SlotGeometry {
    int ws_lo = 0, nws = 0, width = 1, nslots = 0;
    int first_ws(int slot) const { return ws_lo + slot * width; }
    int capacity(int slot) const { return std::min(width, nws - slot * width); }
};
// nws >= 1 usable workspaces from ws_lo on, in slots of the handle's lock-step width (at most max_width: what one launch takes)
inline SlotGeometry slot_geometry(int ws_lo, int nws, int lockstep, int max_width) {
    SlotGeometry g;
    g.ws_lo = ws_lo;
    g.nws = nws;
    g.width = std::max(1, std::min(lockstep, std::min(nws, max_width)));
    g.nslots = (nws + g.width - 1) / g.width;
    return g;
}

constexpr int kSlotBadIndex = -1;  // run_slot_pipeline: the source handed out an index outside [0, k) (no egx_rc is negative)

// Runs the candidates of `src` (indices in [0, k)) through the slots of g.  The callbacks return 0 or an error code:
//   admit(slot, j, c, valid)    candidate c would be the slot's j-th: prepare it (valid = true), or answer it at once
//                               (valid = false: a NaN theta) -- it then takes no place in the slot
//   enqueue(slot, count)        enqueue the `count` candidates admitted since the slot was last idle
//   advance(slot, phase, idle)  the slot finished its phase `phase` (1 = what enqueue started): read it back and either enqueue
//                               the next phase (idle = false) or leave the slot idle (idle = true)
//   sync(slot)                  wait for everything the slot has in flight
// Returns 0 when the source is exhausted and every slot is idle; otherwise the FIRST error, after sync() of every slot that
// was busy (also one whose enqueue failed half way): no work is left behind that still writes into the workspaces.
template <class Admit, class Enqueue, class Advance, class Sync>
int run_slot_pipeline(const SlotGeometry &g, CandidateSource &src, int64_t k, Admit &&admit, Enqueue &&enqueue, Advance &&advance,
                      Sync &&sync) {
    std::vector<int> phase((size_t)g.nslots, 0);  // 0 idle, p >= 1: phase p in flight
    bool exhausted = false;
    int busy = 0;
    auto run = [&]() -> int {
        for (int i = 0; g.nslots > 0; i = (i + 1) % g.nslots) {
            if (phase[i] > 0) {
                bool idle = true;
                if (int rc = advance(i, phase[i], idle)) return rc;
                if (!idle) {
                    phase[i]++;
                    continue;
                }
                phase[i] = 0;
                busy--;
            }
            int held = 0;
            while (!exhausted && held < g.capacity(i)) {
                int64_t c;
                if (src.pull(1, &c) == 0) {
                    exhausted = true;
                    break;
                }
                if (c < 0 || c >= k) return kSlotBadIndex;
                bool valid = false;
                if (int rc = admit(i, held, c, valid)) return rc;
                if (valid) held++;
            }
            if (held > 0) {
                phase[i] = 1;
                busy++;
                if (int rc = enqueue(i, held)) return rc;
            }
            if (exhausted && busy == 0) break;
        }
        return 0;
    };
    const int rc = run();
    if (rc)
        for (int i = 0; i < g.nslots; i++)
            if (phase[i] > 0) sync(i);
    return rc;
}

}  // namespace egx
