// Host test of egobox_amd/csrc/slot_pipeline.h (no HIP): the round-robin slot driver of the lock-step path, run with fake
// callbacks that keep the books a GPU client cannot.  Swept: k = 0 .. 40 candidates, 1 .. 20 workspaces, widths 1 .. 16 (and a
// request beyond 16), ws_lo in {0, 1}, one and two phases per slot, the sequential source and one that hands out a shuffled
// subset, invalid candidates at arbitrary positions, an error injected into the callbacks, a source's index out of range.
//   g++ -std=c++17 -Wall -Werror -I egobox_amd/csrc tests/c_host/slot_pipeline_test.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "slot_pipeline.h"

using namespace egx;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

constexpr int kMaxWidth = 16;
constexpr int kInjected = 7;  // the error a callback returns at the chosen step

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

struct ListSource final : CandidateSource {
    std::vector<int64_t> order;
    size_t next = 0;
    int pull(int want, int64_t *out) override {
        int got = 0;
        while (got < want && next < order.size()) out[got++] = order[next++];
        return got;
    }
};

struct Sim {
    SlotGeometry g;
    int phases = 1;
    int64_t k = 0;
    std::vector<char> valid;                   // per candidate
    std::vector<int> enq, fin, answered;       // per candidate: times enqueued / finished / answered as invalid
    std::vector<std::vector<int64_t>> held;    // per slot: admitted since it was last idle
    std::vector<int> in_flight, expect_phase;  // per slot
    std::vector<int> synced;                   // per slot
    std::vector<int> ws_owner;                 // per workspace of the handle: slot that has it in flight, or -1
    long calls = 0, fail_at = -1;              // callbacks so far (sync not counted); the one that fails
    bool failed = false;

    Sim(const SlotGeometry &g_, int phases_, int64_t k_, int n_workspaces) : g(g_), phases(phases_), k(k_) {
        valid.assign((size_t)k, 1);
        enq.assign((size_t)k, 0), fin.assign((size_t)k, 0), answered.assign((size_t)k, 0);
        held.resize((size_t)g.nslots);
        in_flight.assign((size_t)g.nslots, 0), expect_phase.assign((size_t)g.nslots, 0), synced.assign((size_t)g.nslots, 0);
        ws_owner.assign((size_t)n_workspaces, -1);
    }
    int step() {
        CHECK(!failed);  // after the first error nothing but sync is called
        if (++calls == fail_at) {
            failed = true;
            return kInjected;
        }
        return 0;
    }
    int admit(int i, int j, int64_t c, bool &ok) {
        CHECK(i >= 0 && i < g.nslots && !in_flight[i]);
        CHECK(c >= 0 && c < k);
        CHECK(j == (int)held[i].size() && j < g.capacity(i) && j < kMaxWidth);
        if (int rc = step()) return rc;
        ok = valid[(size_t)c] != 0;
        if (ok) held[i].push_back(c);
        else answered[(size_t)c]++;  // takes no place in the slot
        return 0;
    }
    int enqueue(int i, int count) {
        CHECK(i >= 0 && i < g.nslots && !in_flight[i]);
        CHECK(count == (int)held[i].size() && count >= 1 && count <= g.capacity(i) && count <= kMaxWidth);
        in_flight[i] = 1;  // (a launch sequence that fails half way has still put work on the slot's stream)
        expect_phase[i] = 1;
        for (int j = 0; j < count; j++) {
            const int w = g.first_ws(i) + j;
            CHECK(w >= g.ws_lo && w < (int)ws_owner.size() && ws_owner[(size_t)w] == -1);
            ws_owner[(size_t)w] = i;
            enq[(size_t)held[i][(size_t)j]]++;
        }
        return step();
    }
    int advance(int i, int phase, bool &idle) {
        CHECK(i >= 0 && i < g.nslots && in_flight[i] && phase == expect_phase[i] && phase <= phases);
        if (int rc = step()) return rc;
        idle = phase == phases;
        if (!idle) {
            expect_phase[i]++;
            return 0;
        }
        for (size_t j = 0; j < held[i].size(); j++) {
            fin[(size_t)held[i][j]]++;
            ws_owner[(size_t)(g.first_ws(i) + (int)j)] = -1;
        }
        held[i].clear();
        in_flight[i] = 0;
        return 0;
    }
    int run(CandidateSource &src) {
        return run_slot_pipeline(
            g, src, k, [&](int i, int j, int64_t c, bool &ok) { return admit(i, j, c, ok); },
            [&](int i, int count) { return enqueue(i, count); }, [&](int i, int phase, bool &idle) { return advance(i, phase, idle); },
            [&](int i) { synced[(size_t)i]++; });
    }
    // a run that ended in an error: exactly one synchronise per busy slot, none for the others
    void check_drained() const {
        for (int i = 0; i < g.nslots; i++) CHECK(synced[(size_t)i] == (in_flight[i] ? 1 : 0));
    }
};

static void check_geometry(const SlotGeometry &g, int ws_lo, int nws, int want_width) {
    CHECK(g.ws_lo == ws_lo && g.nws == nws);
    CHECK(g.width >= 1 && g.width <= kMaxWidth && g.width <= nws && g.width == (want_width < 1 ? 1 : want_width));
    int next = ws_lo;
    for (int i = 0; i < g.nslots; i++) {  // the slots tile the usable workspaces: consecutive, disjoint, only the last one ragged
        CHECK(g.first_ws(i) == next);
        CHECK(g.capacity(i) >= 1 && g.capacity(i) <= g.width && (i == g.nslots - 1 || g.capacity(i) == g.width));
        next += g.capacity(i);
    }
    CHECK(next == ws_lo + nws);
}

int main() {
    long runs = 0, injected = 0;
    for (int ws_lo = 0; ws_lo <= 1; ws_lo++)
        for (int nws = 1; nws <= 20; nws++)
            for (int width = 1; width <= 17; width++) {  // (17: a request beyond what one launch takes)
                const SlotGeometry g = slot_geometry(ws_lo, nws, width == 17 ? 1000 : width, kMaxWidth);
                check_geometry(g, ws_lo, nws, width == 17 ? (nws < kMaxWidth ? nws : kMaxWidth) : (width < nws ? width : nws));
                for (int phases = 1; phases <= 2; phases++)
                    for (int64_t k = 0; k <= 40; k++) {
                        // which candidates the source hands out and in which order; which of them are invalid
                        const int variant = (int)(rnd() % 3);  // 0 sequential default, 1 shuffled subset, 2 all, shuffled
                        std::vector<char> member((size_t)k, 1), valid((size_t)k, 1);
                        ListSource list;
                        for (int64_t c = 0; c < k; c++) {
                            if (variant == 1 && rnd() % 3 == 0) member[(size_t)c] = 0;
                            if (rnd() % 4 == 0) valid[(size_t)c] = 0;
                            if (member[(size_t)c]) list.order.push_back(c);
                        }
                        if (k > 0 && rnd() % 16 == 0) std::fill(valid.begin(), valid.end(), 0);  // nothing takes a slot
                        for (size_t a = list.order.size(); a > 1; a--) std::swap(list.order[a - 1], list.order[rnd() % a]);
                        SequentialSource seq(k);
                        auto source = [&]() -> CandidateSource & {
                            list.next = 0, seq.next = 0;
                            return variant == 0 ? static_cast<CandidateSource &>(seq) : list;
                        };
                        // the clean run
                        Sim sim(g, phases, k, ws_lo + nws);
                        sim.valid = valid;
                        CHECK(sim.run(source()) == 0);
                        runs++;
                        for (int64_t c = 0; c < k; c++) {
                            const bool handed = variant == 0 || member[(size_t)c];
                            CHECK(sim.enq[(size_t)c] == (handed && valid[(size_t)c] ? 1 : 0));
                            CHECK(sim.fin[(size_t)c] == sim.enq[(size_t)c]);
                            CHECK(sim.answered[(size_t)c] == (handed && !valid[(size_t)c] ? 1 : 0));
                        }
                        for (int i = 0; i < g.nslots; i++) CHECK(!sim.in_flight[i] && sim.held[(size_t)i].empty() && sim.synced[(size_t)i] == 0);
                        for (int w : sim.ws_owner) CHECK(w == -1);
                        // an error at a step: every step on a thinned grid, three random ones elsewhere
                        const long total = sim.calls;
                        const bool every = (k % 8 == 1 || k == 40) && (nws % 6 == 1 || nws == 20) && (width % 5 == 1 || width == 3);
                        for (long t = 1, picks = 0; total > 0 && (every ? t <= total : picks < 3); t++, picks++) {
                            Sim bad(g, phases, k, ws_lo + nws);
                            bad.valid = valid;
                            bad.fail_at = every ? t : 1 + (long)(rnd() % (uint32_t)total);
                            CHECK(bad.run(source()) == kInjected);  // the first error, and nothing called after it
                            CHECK(bad.failed && bad.calls == bad.fail_at);
                            bad.check_drained();
                            for (int64_t c = 0; c < k; c++) CHECK(bad.enq[(size_t)c] <= 1 && bad.fin[(size_t)c] <= bad.enq[(size_t)c]);
                            injected++;
                        }
                        // a source that hands out an index outside [0, k), somewhere along the way
                        if (rnd() % 8 == 0) {
                            ListSource wrong;
                            wrong.order = list.order;
                            const int64_t out_of_range = rnd() % 2 ? k : -1;
                            wrong.order.insert(wrong.order.begin() + (long)(rnd() % (wrong.order.size() + 1)), out_of_range);
                            Sim bad(g, phases, k, ws_lo + nws);
                            bad.valid = valid;
                            CHECK(bad.run(wrong) == kSlotBadIndex);
                            bad.check_drained();
                        }
                    }
            }
    std::printf("slot pipeline ok: %ld clean runs, %ld with an injected error\n", runs, injected);
    return 0;
}
