// The launch ORDER of launch_potrf (kernels_chol.hip) as data: which launch, solve, update, chain / flow launch and which event
// record / wait a factorisation issues, on which of its four streams, in which order.  Host only, no HIP in here, like
// schedule.h: launch_potrf resolves a PotrfPlanInput (what needs the device or the pointers enters as resolved values), calls
// potrf_plan and walks the steps with one switch.  tests/c_host/potrf_plan_test.cpp compares the plans with traces recorded from
// the function this header replaced (tests/golden/potrf_plan/), runs them on a model of four FIFO streams with events -- no
// unordered pair of accesses to a tile, nothing starts before the caller's stream, everything is joined into it at the end --
// and checks the algebra: every tile receives the K ranges [0, its panel) exactly once, before it is factored or solved.
//
// What runs beside what (the comment on launch_potrf says why):
//   right-looking, look-ahead   S : LUd | rec LU | [LUr | rec LUR | signal] | RU | wait PANEL | rider's hand-over
//                               S2: wait LU | chain of the next group (its first solve waits for LUR) | rec PANEL
//                               S3: the rest of the chain's in-group updates (rec A on the chain's stream, rec B here); LUr when
//                                   it goes to the side stream
//   left-looking, look-ahead    S : U_long(J) | wait PANEL (chain J-1) | U_short(J) | rec LU | U_long(J+1) ...
//                               S2: wait LU | chain(J) | rec PANEL
//   the C^-T rider              SW: wait GRP (recorded where a group became final) | the group's solves and updates of W;
//                                   rec DONE at the end, waited for by S in front of the tile inverses
#pragma once

#include <cstddef>
#include <vector>

namespace egx {

constexpr int kPlanPanel = 256;        // kNB (egx_internal.h; kernels_chol.hip asserts that they agree)
constexpr int kLurSideMinCols = 6144;  // LUr on the side stream only while at least this many columns trail the look-ahead group

enum class PotrfChain {
    SEPARATE,    // diagonal blocks, panel solves, in-group updates as launches of their own
    PIPE_GROUP,  // the chain of every group of panels is one chain launch (kernels_pipe.hip)
    PIPE_WHOLE,  // the whole factorisation is one chain launch
    FLOW,        // the whole factorisation is one flow launch (pipe_flow.h)
    FLOW_TAIL    // right-looking by separate launches, the last tail_cols columns as a flow launch
};
struct PotrfPlanInput {
    int n_pad = 0, m_tot = 0;  // multiples of 128, m_tot >= n_pad (rows from n_pad on: right-hand sides)
    int GW = 512;              // columns per group of panels
    bool left = false;         // left-looking group updates of the factorisation ...
    bool w_left = false;       // ... of the rider (resolved: never with n_pad % 256 != 0)
    PotrfChain chain = PotrfChain::SEPARATE;  // resolved: flow_fits / pipe_fits, hand-off words given, one matrix, no rider
    int tail_cols = 0;         // FLOW_TAIL: (n_pad - tail_cols) % GW == 0, 0 < tail_cols < n_pad, never with `left`
    bool lookahead = false;    // the streams S2 and S3 exist (both or none)
    bool rider = false;        // a PotrfInverse is given: W = C^-T rides along on SW
    int seqs = 1;              // launch sequences of the handle in flight: beyond two a look-ahead chain launch waits on the stream
    int look_min = 3072;       // "look_min" at launch time: look-ahead while at least this many columns trail the next group
    int lur_side = 1;          // "lur_side" at launch time
    bool trace = false;        // trace slots are there: the chip-filling updates are marked `timed`
};

enum class PotrfKind { POTF2, TRSM, UPDATE, PIPE, FLOW, SIGNAL, W_TRSM, W_UPDATE, W_LEFT, TILE_INVERSES, RECORD, WAIT };
enum class PotrfStream { S, S2, S3, SW };
enum class PotrfEvent { NONE, LU, LUR, PANEL, A, B, GRP, DONE };
enum { POTRF_UNTIMED = 0, POTRF_TIMED_IF_BIG = 1, POTRF_TIMED = 2 };  // (the second closes its slot only when the update filled the chip)

// kind            fields
// POTF2, TRSM     k0, K (the panel's width): the diagonal block at (k0, k0); the rows below it
// UPDATE          M[r0.. (rows), c0.. (cols)) -= M[r0.., k0..k0+K) M[c0.., k0..k0+K)^T; lower, tag, timed, flops (one matrix')
// PIPE            c0, cols: the group; panel: its first solves wait on the device for SIGNAL(panel) (0: not); high: it shares the chip
// FLOW            r0: the trailing matrix from (r0, r0) on
// SIGNAL          panel
// W_TRSM          k0, K: the rows [0, k0 + K) of W's columns k0..
// W_UPDATE        W[0.. (rows), c0.. (cols)) -= W[0.., k0..k0+K) M[c0.., k0..k0+K)^T
// W_LEFT          W[0..c0, c0..c0+cols) = -W[0..c0, 0..c0) M[c0.., 0..c0)^T
// RECORD, WAIT    ev
struct PotrfStep {
    PotrfKind kind;
    PotrfStream stream;
    PotrfEvent ev;
    int r0, c0, rows, cols, k0, K;
    int lower, tag, timed, panel, high;
    double flops;
};

namespace potrf_plan_detail {
struct Builder {
    const PotrfPlanInput &in;
    std::vector<PotrfStep> &out;
    using St = PotrfStream;
    using Ev = PotrfEvent;

    PotrfStep &add(PotrfKind kind, St st) {
        out.push_back(PotrfStep{kind, st, Ev::NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0});
        return out.back();
    }
    void record(St st, Ev ev) { add(PotrfKind::RECORD, st).ev = ev; }
    void wait(St st, Ev ev) { add(PotrfKind::WAIT, st).ev = ev; }
    void panel(PotrfKind kind, St st, int k0, int nbk) {
        PotrfStep &p = add(kind, st);
        p.k0 = k0, p.K = nbk;
    }
    void update(St st, int r0, int c0, int rows, int cols, int k0, int K, int lower, int tag = 0, int timed = POTRF_UNTIMED,
                double flops = 0.0) {
        PotrfStep &p = add(PotrfKind::UPDATE, st);
        p.r0 = r0, p.c0 = c0, p.rows = rows, p.cols = cols, p.k0 = k0, p.K = K, p.lower = lower, p.tag = tag;
        if (in.trace) p.timed = timed, p.flops = flops;
    }
    void w_update(int rows, int c0, int cols, int k0, int K) {
        PotrfStep &p = add(PotrfKind::W_UPDATE, St::SW);
        p.rows = rows, p.c0 = c0, p.cols = cols, p.k0 = k0, p.K = K;
    }
    int gwidth(int g0) const { return (in.n_pad - g0 < in.GW) ? (in.n_pad - g0) : in.GW; }
    // the trailing update of the lower triangle from column c on by K columns: what the roofline trace counts
    double trailing_flops(int c, int K) const {
        const double nc = (double)(in.n_pad - c);
        return 2.0 * K * nc * (nc + 1.0) / 2.0;
    }

    // panels of one group on stream `st`; `side` splits every in-group update into the next diagonal block (on st) and the
    // rest (on the side stream S3); `first_wait` is waited for before the FIRST panel solve (the rest of the update that brought
    // this group's columns up to date)
    void chain(St st, int g0, int gw, bool side, Ev first_wait) {
        if (in.chain == PotrfChain::PIPE_GROUP) {  // one launch: diagonal blocks, panel solves and in-group updates hand over on the device
            // (first_wait -- the rest of the update that brought this group's columns up to date, on another stream -- is
            //  waited for ON THE DEVICE by the first panel's solve tasks: SIGNAL behind that update.
            //  With more than two launch sequences of the handle in flight the workgroups that spin on that word -- 96 per launch,
            //  one compute unit each -- could leave the update they wait for no unit to run on (3 x 96 > 256): the STREAM waits then.)
            const bool on_device = first_wait != Ev::NONE && in.seqs <= 2;
            if (first_wait != Ev::NONE && !on_device) wait(st, first_wait);
            PotrfStep &p = add(PotrfKind::PIPE, st);
            p.c0 = g0, p.cols = gw, p.panel = on_device ? g0 / kPlanPanel + 1 : 0, p.high = st != St::S;
            // (... and by the stream behind the launch: a matrix that lost a pivot skips its tasks without waiting for anything)
            if (on_device) wait(st, first_wait);
            return;
        }
        Ev pending = first_wait;
        for (int k0 = g0; k0 < g0 + gw; k0 += kPlanPanel) {
            const int nbk = (g0 + gw - k0 < kPlanPanel) ? (g0 + gw - k0) : kPlanPanel;
            panel(PotrfKind::POTF2, st, k0, nbk);
            if (pending != Ev::NONE) {
                wait(st, pending);
                pending = Ev::NONE;
            }
            if (in.m_tot - (k0 + nbk) > 0) panel(PotrfKind::TRSM, st, k0, nbk);
            const int r1 = k0 + nbk;
            if (r1 >= g0 + gw) break;
            const int ncols = g0 + gw - r1;
            const int nb1 = ncols < kPlanPanel ? ncols : kPlanPanel;  // width of the next panel
            const int rest_rows = in.m_tot - r1 - nb1;
            if (side && rest_rows >= 128) {
                update(st, r1, r1, nb1, nb1, k0, nbk, 1);  // the next diagonal block only
                record(st, Ev::A);
                wait(St::S3, Ev::A);
                // everything below it (blocks above the diagonal inside this rectangle are written but never read)
                update(St::S3, r1 + nb1, r1, rest_rows, ncols, k0, nbk, 0);
                record(St::S3, Ev::B);
                pending = Ev::B;
            } else {
                update(st, r1, r1, in.m_tot - r1, ncols, k0, nbk, 1);
            }
        }
        if (pending != Ev::NONE) wait(st, pending);
    }

    // The rows of W = C^-T through the group of panels [g0, g0 + gw), which is final on `sfin` when this is called (PotrfInverse,
    // egx_internal.h): on SW, beside whatever the factorisation does next.  Row i of the identity is zero left of
    // column i, so panel k0 only has the rows [0, k0 + nbk) to solve and the updates as many rows to carry.
    void rider(St sfin, int g0, int gw) {
        if (!in.rider) return;
        record(sfin, Ev::GRP);
        wait(St::SW, Ev::GRP);
        const int gend = g0 + gw;
        for (int k0 = g0; k0 < gend; k0 += kPlanPanel) {
            const int nbk = (gend - k0 < kPlanPanel) ? (gend - k0) : kPlanPanel;
            panel(PotrfKind::W_TRSM, St::SW, k0, nbk);
            const int ncols = gend - (k0 + nbk);
            if (ncols > 0) w_update(k0 + nbk, k0 + nbk, ncols, k0, nbk);
        }
        const int ncols = in.n_pad - gend;
        if (ncols > 0 && in.w_left) {
            // left-looking rider (round 4; w_left_for): the NEXT group's columns of W receive all earlier columns at once,
            //     W[0:gend, next) = -W[0:gend, 0:gend) L[next, 0:gend)^T      (rows below gend: the identity, untouched)
            // by one launch of the stream kernel with per-tile K ranges (row i of W is zero left of column i) and
            // zero-initialised accumulators: a tile of W is written once by a long K loop, then read and written once by
            // its group's own solves -- instead of one read-modify-write pass (K = 1024) per earlier group.  It only reads
            // rows of the factor that are final with THIS group, so it is issued here, ahead of the next group's chain.
            PotrfStep &p = add(PotrfKind::W_LEFT, St::SW);
            p.c0 = gend, p.cols = gwidth(gend);
        } else if (ncols > 0) {
            // (round 6 measured this update SPLIT into the next group's columns on this stream and the rest on a second rider stream
            //  beside the next group's solves -- the timeline shows the rider six groups behind the factorisation with ~0.7 ms of
            //  small launches exposed per group: one candidate 76.5 -> 79.4 ms at n = 16384, 35.3 -> 39.5 at 12288, 12.2 -> 14.2 at 8192
            //  (a third stream competing with the factorisation, two launches' tails for one): profiles/r06_rider_split_ab.txt; gone)
            w_update(gend, gend, ncols, g0, gw);
        }
    }

    // W is complete (its panel solves read the 16 x 16 inverses the last launch overwrites) and every stream has been joined
    // into S: the 64x64 tile inverses of the complete factor(s), one launch
    void finish() {
        if (in.rider) {
            record(St::SW, Ev::DONE);
            wait(St::S, Ev::DONE);
        }
        add(PotrfKind::TILE_INVERSES, St::S);
    }

    void whole() {
        // (decided per HANDLE, never by the number of matrices in a launch: a matrix gets the same bits in any batch -- and with or
        //  without the theta-gradient's rider: its substitution then follows the launch group by group instead of riding along)
        if (in.chain == PotrfChain::FLOW) {
            add(PotrfKind::FLOW, St::S);
        } else {
            PotrfStep &p = add(PotrfKind::PIPE, St::S);
            p.cols = in.n_pad;
        }
        for (int g0 = 0; g0 < in.n_pad; g0 += in.GW) rider(St::S, g0, gwidth(g0));
    }

    void left() {
        // LEFT-looking over the groups of panels (round 4): the columns of group J receive the contributions of ALL earlier
        // columns in two updates -- a LONG one, K = every column before the previous group, and a SHORT one, K = the previous
        // group (1024) -- instead of one read-modify-write pass per earlier group: a tile of the factor is read and written
        // twice in the whole factorisation, by long K loops (what makes the theta-gradient's R^-1 launch run at 0.85 of
        // peak; the long updates of a lock-step group of eight measured 0.82, the right-looking trailing updates 0.72).
        // Look-ahead: the chain of group J (diagonal blocks, panel solves, in-group updates; stream S2) runs beside the
        // long update of group J + 1 (stream S), which only needs the groups before J:
        //     S :  ... U_long(J) | wait C(J-1) | U_short(J) | rec U(J) | U_long(J+1) | wait C(J) | U_short(J+1) ...
        //     S2:                                            wait U(J) | chain(J) | rec C(J)
        // A lone matrix' late long updates have few tiles with very long K loops and leave the chip underfilled: the mode is
        // chosen per HANDLE (n_pad >= 14336 and a lock-step width of at least eight, PotrfBatch::left), never by the number of
        // matrices in a launch, so a candidate's bits do not depend on its companions.
        const bool la = in.lookahead;
        const St sc = la ? St::S2 : St::S;  // the chain's stream
        chain(St::S, 0, gwidth(0), la, Ev::NONE);
        rider(St::S, 0, gwidth(0));
        int gprev = 0;  // start of the previous group
        for (int g0 = gwidth(0); g0 < in.n_pad; g0 += in.GW) {
            const int gw = gwidth(g0);
            if (gprev > 0) {  // U_long: columns [0, gprev), all final (C(J-2) was waited for before U_short(J-1))
                const double nr = (double)(in.n_pad - g0);
                update(St::S, g0, g0, in.m_tot - g0, gw, 0, gprev, 1, 1, POTRF_TIMED, 2.0 * gprev * (nr * gw - 0.5 * gw * (gw - 1.0)));
            }
            if (la && gprev > 0) wait(St::S, Ev::PANEL);                   // C(J-1): the previous group is final
            update(St::S, g0, g0, in.m_tot - g0, gw, gprev, g0 - gprev, 1, 2);  // U_short
            if (la) {
                record(St::S, Ev::LU);
                wait(sc, Ev::LU);
            }
            chain(sc, g0, gw, la, Ev::NONE);
            if (la) record(sc, Ev::PANEL);
            rider(sc, g0, gw);
            gprev = g0;
        }
        if (la && gprev > 0) wait(St::S, Ev::PANEL);
    }

    void right() {
        chain(St::S, 0, gwidth(0), in.lookahead, Ev::NONE);
        rider(St::S, 0, gwidth(0));
        for (int g0 = 0; g0 < in.n_pad; g0 += in.GW) {
            const int gw = gwidth(g0);
            const int r1 = g0 + gw;     // first row/col of the trailing matrix
            if (r1 >= in.n_pad) break;  // (right-hand-side rows below the last block were solved by its panel)
            const int gw1 = gwidth(r1);
            if (in.chain == PotrfChain::FLOW_TAIL && in.n_pad - r1 == in.tail_cols) {
                // the flow tail: ONE update of the whole trailing matrix by this group, then the trailing matrix -- every update of the
                // columns before it applied -- is a factorisation of its own, as one flow launch (pipe_flow.h)
                update(St::S, r1, r1, in.m_tot - r1, in.n_pad - r1, g0, gw, 1);
                add(PotrfKind::FLOW, St::S).r0 = r1;
                for (int t0 = r1; t0 < in.n_pad; t0 += in.GW) rider(St::S, t0, gwidth(t0));
                break;
            }
            // the cross-stream hand-off costs ~2 x 10 us; below ~3k trailing columns RU is shorter than that (and with
            // several fits in flight the extra hand-offs cost more than they hide: profiles/r02_run23_tail_lookahead_ab.txt)
            const bool look = in.lookahead && (in.n_pad - r1 - gw1 >= in.look_min);
            const int r2 = r1 + gw1;
            if (look) {
                // LUd: the next group's first diagonal block; its chain may start.  LUr: the rest of the next group's columns.
                const int nb1 = gw1 < kPlanPanel ? gw1 : kPlanPanel;
                update(St::S, r1, r1, nb1, nb1, g0, gw, 1);
                record(St::S, Ev::LU);
                wait(St::S2, Ev::LU);
                // LUr writes the next group's columns, RU the columns right of them, both only READ this group's panel: LUr goes
                // to the (high-priority) side stream, so that RU fills the CUs LUr's last, partly filled round of tiles leaves idle
                // (+0.8 % on the sweep, +1 % on a lone fit: profiles/r03_run4_lur_side_ab.txt, r03_run8_*).  Round 3 kept a lone
                // matrix' LUr in front of RU because the driver line's roofline timed those RU launches one by one; since round 4
                // that leg switches the side stream off for itself (egx_set_tuning "lur_side" = 0).  From n_pad 14336 on only
                // (n = 16384 lone: 31.5 -> 30.9 ms; n = 8192: one fit 6.24 -> 6.44 ms, twelve in lock-step 260 -> 258 fits/s:
                // profiles/r04_run11_lur_side_lone_ab.txt).  In the last ~6000 columns the chain is what a factorisation waits for and
                // its first panel solve waits for LUr: there LUr runs ALONE in front of RU (250 us instead of 520-770 beside it;
                // n = 16384 lone: 29.85 -> 29.6 ms, profiles/r04_run14_*).  Streams only: the arithmetic is the same either way.
                const St slu = (in.lur_side && in.n_pad >= 14336 && in.n_pad - r2 >= kLurSideMinCols) ? St::S3 : St::S;
                if (slu != St::S) wait(slu, Ev::LU);
                update(slu, r1 + nb1, r1, in.m_tot - r1 - nb1, gw1, g0, gw, 0);
                record(slu, Ev::LUR);
                if (in.chain == PotrfChain::PIPE_GROUP) add(PotrfKind::SIGNAL, slu).panel = r1 / kPlanPanel + 1;
                chain(St::S2, r1, gw1, true, Ev::LUR);
                record(St::S2, Ev::PANEL);
                // RU: the rest of the trailing matrix
                if (r2 < in.n_pad) update(St::S, r2, r2, in.m_tot - r2, in.n_pad - r2, g0, gw, 1, 0, POTRF_TIMED_IF_BIG, trailing_flops(r2, gw));
                wait(St::S, Ev::PANEL);
            } else {
                // no look-ahead (small matrices, the last ~3000 columns): nothing runs beside the trailing update, so the next
                // group's columns and the rest are ONE launch (round 4: one ramp-up and one tail instead of two)
                update(St::S, r1, r1, in.m_tot - r1, in.n_pad - r1, g0, gw, 1, 0, POTRF_TIMED_IF_BIG, trailing_flops(r1, gw));
                chain(St::S, r1, gw1, false, Ev::NONE);
            }
            rider(St::S, r1, gw1);  // the group that has just become final
        }
    }
};
}  // namespace potrf_plan_detail

// upper bound on the steps of a plan (launch_potrf reserves its vector once per call)
inline size_t potrf_plan_max_steps(const PotrfPlanInput &in) {
    const size_t panels = (size_t)(in.n_pad + kPlanPanel - 1) / kPlanPanel, groups = (size_t)(in.n_pad + in.GW - 1) / in.GW;
    return 12 * panels + 16 * groups + 8;  // a panel: diagonal block, wait, solve, split update (6), rider's solve and update
}

// The steps of one factorisation, appended to `out`.  A pure function of `in`: no globals, no environment.
inline void potrf_plan(const PotrfPlanInput &in, std::vector<PotrfStep> &out) {
    potrf_plan_detail::Builder b{in, out};
    if (in.chain == PotrfChain::FLOW || in.chain == PotrfChain::PIPE_WHOLE)
        b.whole();
    else if (in.left)
        b.left();
    else
        b.right();
    b.finish();
}

}  // namespace egx
