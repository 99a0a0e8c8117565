// Host test of egobox_amd/csrc/potrf_plan.h (no HIP): the launch order of launch_potrf as data.
//   (a) every case's plan, printed as the launches and event calls launch_potrf's executor makes of it, is the trace recorded
//       from the function the plan replaced (tests/golden/potrf_plan/<case>.txt.gz unpacked, README there)
//   (b) on a model of four FIFO streams, a WAIT bound to the latest earlier RECORD of its event, no two accesses to a 128 x 128
//       tile of M or W or to a 64-column slot of dinv, one of them a write, are unordered
//   (c) nothing starts before the first step on S, and the last step on S comes after everything
//   (d) every tile receives disjoint K ranges whose union is [0, where its own launch starts), each before that launch; the
//       rider's columns likewise; the flops of the timed updates
// and three broken plans (a dropped WAIT(LUR), a dropped WAIT(B), a dropped UPDATE) are each reported.
// usage: potrf_plan_test <golden dir> | --list | --print <case>
#include "../../egobox_amd/csrc/potrf_plan.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace egx;
using Steps = std::vector<PotrfStep>;

struct Case {
    std::string name;
    PotrfPlanInput in;
    int nz;  // matrices in lock-step: grids and batch descriptors only
};

static std::vector<Case> cases() {
    std::vector<Case> out;
    auto add = [&](const std::string &name, int n_pad, bool rhs, int GW, PotrfChain chain, bool look, bool rider,
                   const PotrfPlanInput &more) {
        Case c;
        c.in = more;
        c.in.n_pad = n_pad, c.in.m_tot = n_pad + (rhs ? 128 : 0), c.in.GW = GW, c.in.chain = chain, c.in.lookahead = look;
        c.in.rider = rider, c.in.trace = true;
        c.nz = (chain == PotrfChain::FLOW || chain == PotrfChain::FLOW_TAIL) ? 1 : 3;
        c.name = name + "_n" + std::to_string(n_pad) + (rhs ? "" : "_square") + (rider ? "_rider" : "");
        out.push_back(c);
    };
    const PotrfPlanInput dflt;
    for (int n : {128, 384, 1024})
        for (bool rhs : {true, false}) add("separate", n, rhs, 512, PotrfChain::SEPARATE, false, false, dflt);
    for (bool rider : {false, true}) {
        add("look", 8192, true, 512, PotrfChain::SEPARATE, true, rider, dflt);
        PotrfPlanInput p;
        p.look_min = 256;
        add("look_min256", 1536, true, 256, PotrfChain::SEPARATE, true, rider, p);
    }
    for (int n : {14336, 16384})
        for (int lur : {1, 0})
            for (int r = 0; r < 3; r++) {  // rider off, right-looking, left-looking
                PotrfPlanInput p;
                p.lur_side = lur, p.w_left = r == 2;
                add(std::string("lur") + (lur ? "_side" : "_front") + (r == 2 ? "_wleft" : ""), n, true, 1024, PotrfChain::SEPARATE, true,
                    r > 0, p);
            }
    for (bool rider : {false, true}) {
        PotrfPlanInput p;
        p.left = true, p.w_left = true;
        add("left", 14336, true, 1024, PotrfChain::SEPARATE, true, rider, p);
    }
    for (int n : {1536, 1408})
        for (bool look : {true, false}) {
            PotrfPlanInput p;
            p.left = true, p.w_left = n % 256 == 0;
            add(std::string("left") + (look ? "_look" : "_inorder"), n, true, 512, PotrfChain::SEPARATE, look, true, p);
        }
    for (int seqs : {1, 3})
        for (bool rider : {false, true}) {
            PotrfPlanInput p;
            p.seqs = seqs;
            add("chain_group_seqs" + std::to_string(seqs), 4096, true, 512, PotrfChain::PIPE_GROUP, true, rider, p);
        }
    for (bool rhs : {true, false})
        for (bool rider : {false, true}) add("chain_whole", 2048, rhs, 512, PotrfChain::PIPE_WHOLE, true, rider, dflt);
    add("flow", 8192, true, 512, PotrfChain::FLOW, true, false, dflt);
    for (int n : {14336, 16384}) {
        PotrfPlanInput p;
        p.tail_cols = 6144;
        add("flow_tail", n, true, 1024, PotrfChain::FLOW_TAIL, true, false, p);
    }
    return out;
}

static int chain_code(PotrfChain c) {
    switch (c) {
    case PotrfChain::SEPARATE: return 0;
    case PotrfChain::PIPE_GROUP: return 1;
    case PotrfChain::PIPE_WHOLE: return 2;
    case PotrfChain::FLOW: return 3;
    default: return 4;
    }
}

// ---- (a) the plan as the calls launch_potrf's executor makes of it ------------------------------------------------
// The recording set-up (README in the golden directory): ld = n_pad + 128, ldw = n_pad + 256, the strides between the matrices of
// a batch sM = 11, sD = 13, sI = 17, sW = 19; pointers as M(row,col) / W(row,col) / d<64-column tile>; a launch as
// "<stream> <kernel> <grid> <block> <dynamic LDS> <arguments>"; an update as "<stream> gemm C ldc A lda B ldb M N K lower ktri info
// {count,sC,sA,sB,sInfo} tag"; every timed update closes its slot (the recording's updates all report a chip-filling launch).
static const char *kStream[] = {"S", "S2", "S3", "SW"};
static const char *kEvent[] = {"-", "LU", "LUR", "PANEL", "A", "B", "GRP", "DONE"};

static std::string print_plan(const Case &c, const Steps &plan) {
    const PotrfPlanInput &in = c.in;
    const long ld = in.n_pad + 128, ldw = in.n_pad + 256;
    const int nz = c.nz, sM = 11, sD = 13, sI = 17, sW = 19;
    std::ostringstream o;
    std::vector<double> flops;
    char b[400];
    if (in.chain != PotrfChain::SEPARATE) o << "S memset\n";
    for (const PotrfStep &p : plan) {
        const char *st = kStream[(int)p.stream];
        b[0] = 0;
        switch (p.kind) {
        case PotrfKind::POTF2:
            snprintf(b, sizeof b, "%s k_potf2_reg<16> 1,1,%d 1024 RB_LDS_BYTES M(%d,%d) %ld %d d%d info %d %d %d %d %d", st, nz, p.k0, p.k0,
                     ld, p.K, p.k0 / 64, p.k0, in.n_pad, sM, sD, sI);
            break;
        case PotrfKind::TRSM: {
            const int below = in.m_tot - (p.k0 + p.K), rt = below >= 4096 ? 2 : 1;
            snprintf(b, sizeof b, "%s k_panel_trsm16<%d,false> %d,1,%d 256 0 M(%d,%d) %ld M(%d,%d) %ld d%d %d info %d %d %d %d 0", st, rt,
                     below / (16 * rt), nz, p.k0 + p.K, p.k0, ld, p.k0, p.k0, ld, p.k0 / 64, p.K, sM, sM, sD, sI);
            break;
        }
        case PotrfKind::W_TRSM: {
            const int rows = p.k0 + p.K, rt = rows >= 4096 ? 2 : 1;
            snprintf(b, sizeof b, "%s k_panel_trsm16<%d,false> %d,1,%d 256 0 W(0,%d) %ld M(%d,%d) %ld d%d %d info %d %d %d %d 0", st, rt,
                     rows / (16 * rt), nz, p.k0, ldw, p.k0, p.k0, ld, p.k0 / 64, p.K, sW, sM, sD, sI);
            break;
        }
        case PotrfKind::UPDATE:
            if (p.timed) o << st << " rec e0[" << flops.size() << "]\n";
            snprintf(b, sizeof b, "%s gemm M(%d,%d) %ld M(%d,%d) %ld M(%d,%d) %ld %d %d %d %d 0 info {%d,%d,%d,%d,%d} %d", st, p.r0, p.c0, ld,
                     p.r0, p.k0, ld, p.c0, p.k0, ld, p.rows, p.cols, p.K, p.lower, nz, sM, sM, sM, sI, p.tag);
            if (p.timed) {
                o << b << "\n";
                snprintf(b, sizeof b, "%s rec e1[%d]", st, (int)flops.size());
                flops.push_back((double)nz * p.flops);
            }
            break;
        case PotrfKind::W_UPDATE:
            snprintf(b, sizeof b, "%s gemm W(0,%d) %ld W(0,%d) %ld M(%d,%d) %ld %d %d %d 0 0 info {%d,%d,%d,%d,%d} 0", st, p.c0, ldw, p.k0,
                     ldw, p.c0, p.k0, ld, p.rows, p.cols, p.K, nz, sW, sW, sM, sI);
            break;
        case PotrfKind::W_LEFT: {
            const int nbx = p.c0 / 128, nby = p.cols / 256, nt = nbx * nby;
            snprintf(b, sizeof b, "%s k_gemm_stream<false,true> %d,1,1 512 ST_LDS_BYTES W(0,%d) %ld W(0,0) %ld M(%d,0) %ld %d %d %d %d info {%d,%d,%d,%d,%d}",
                     st, nt * nz, p.c0, ldw, ldw, p.c0, ld, p.c0, nbx, nby, nt, nz, sW, sW, sM, sI);
            break;
        }
        case PotrfKind::PIPE:
            snprintf(b, sizeof b, "%s pipe M(0,0) %ld %d %d d0 info %d %d %d %d", st, ld, in.n_pad, in.m_tot, p.c0, p.cols, p.panel, p.high);
            break;
        case PotrfKind::FLOW:
            snprintf(b, sizeof b, "%s flow M(%d,%d) %ld %d %d d%d info %d", st, p.r0, p.r0, ld, in.n_pad - p.r0, in.m_tot - p.r0, p.r0 / 64,
                     p.r0);
            break;
        case PotrfKind::SIGNAL: snprintf(b, sizeof b, "%s signal %d", st, p.panel); break;
        case PotrfKind::TILE_INVERSES:
            snprintf(b, sizeof b, "%s k_diag_tile_inverses %d,1,%d 256 0 M(0,0) %ld d0 d%d %d %d", st, in.n_pad / 64, nz, ld, in.n_pad / 64, sM,
                     sD);
            break;
        case PotrfKind::RECORD: snprintf(b, sizeof b, "%s rec %s", st, kEvent[(int)p.ev]); break;
        case PotrfKind::WAIT: snprintf(b, sizeof b, "%s wait %s", st, kEvent[(int)p.ev]); break;
        }
        o << b << "\n";
    }
    for (size_t i = 0; i < flops.size(); i++) {
        snprintf(b, sizeof b, "flops[%d] %.17g", (int)i, flops[i]);
        o << b << "\n";
    }
    return o.str();
}

// ---- (b) (c) (d): the plan on a model -----------------------------------------------------------------------------
struct Report {
    int unbound_waits = 0, conflicts = 0, entry_exit = 0, algebra = 0, flops = 0;
    std::string first;
    bool ok() const { return !(unbound_waits || conflicts || entry_exit || algebra || flops); }
    void note(int &counter, const std::string &what) {
        if (ok()) first = what;
        counter++;
    }
};

struct Node {
    int step;
    int stream, seq;            // position on its stream
    std::array<int, 4> clock;   // per stream: the last position that happens before (or is) this node; -1: none
};
struct Range { int lo, hi, node; };
struct TileState {
    int last_write = -1;
    std::vector<int> reads;     // since the last write
    std::vector<Range> applied; // K ranges of the updates
    int finisher = -1, fin_lo = 0;  // the node that factors / solves the tile, and where its own work starts
};

struct Model {
    const PotrfPlanInput &in;
    const Steps &plan;
    Report &rep;
    std::vector<Node> nodes;
    int T, TR;  // 128-tiles across, rows of M
    std::vector<TileState> m, w, d;

    Model(const PotrfPlanInput &i, const Steps &p, Report &r) : in(i), plan(p), rep(r) {
        T = in.n_pad / 128, TR = in.m_tot / 128;
        m.resize((size_t)TR * T), w.resize((size_t)T * T), d.resize((size_t)in.n_pad / 64);
    }
    bool before(int a, int b) const { return a == b || nodes[b].clock[nodes[a].stream] >= nodes[a].seq; }
    std::string where(int node) const {
        const PotrfStep &p = plan[nodes[node].step];
        char b[96];
        snprintf(b, sizeof b, "step %d (kind %d on %s)", nodes[node].step, (int)p.kind, kStream[(int)p.stream]);
        return b;
    }
    void touch(TileState &t, int node, bool write, const char *what, int i, int j) {
        auto ordered = [&](int earlier) {
            if (before(earlier, node)) return;
            char b[64];
            snprintf(b, sizeof b, "%s(%d,%d): ", what, i, j);
            rep.note(rep.conflicts, std::string(b) + where(earlier) + " and " + where(node) + " are not ordered");
        };
        if (t.last_write >= 0) ordered(t.last_write);
        if (write) {
            for (int r : t.reads) ordered(r);
            t.reads.clear();
            t.last_write = node;
        } else {
            t.reads.push_back(node);
        }
    }
    // rows [r0, r1) x columns [c0, c1) of M in elements; tiles above the diagonal are written by rectangular updates but never read
    void m_rect(int node, int r0, int r1, int c0, int c1, bool write) {
        for (int I = r0 / 128; I < (r1 + 127) / 128; I++)
            for (int J = c0 / 128; J < (c1 + 127) / 128 && J <= I; J++) touch(m[(size_t)I * T + J], node, write, "M", I, J);
    }
    void w_rect(int node, int r1, int c0, int c1, bool write) {  // rows [0, r1)
        for (int I = 0; I < (r1 + 127) / 128; I++)
            for (int J = c0 / 128; J < (c1 + 127) / 128; J++) touch(w[(size_t)I * T + J], node, write, "W", I, J);
    }
    void d_slots(int node, int c0, int c1, bool write) {
        for (int s = c0 / 64; s < (c1 + 63) / 64; s++) touch(d[s], node, write, "dinv", s, 0);
    }
    void m_apply(int node, int r0, int r1, int c0, int c1, int k0, int k1) {
        for (int I = r0 / 128; I < (r1 + 127) / 128; I++)
            for (int J = c0 / 128; J < (c1 + 127) / 128 && J <= I; J++) m[(size_t)I * T + J].applied.push_back({k0, k1, node});
    }
    void m_finish(int node, int r0, int r1, int c0, int c1, int lo) {
        for (int I = r0 / 128; I < (r1 + 127) / 128; I++)
            for (int J = c0 / 128; J < (c1 + 127) / 128 && J <= I; J++) {
                TileState &t = m[(size_t)I * T + J];
                if (t.finisher >= 0) rep.note(rep.algebra, "a tile of M is factored or solved twice: " + where(node));
                t.finisher = node, t.fin_lo = lo;
            }
    }

    int add_node(int step, int stream, int extra_pred) {
        Node n;
        n.step = step, n.stream = stream;
        n.clock = {-1, -1, -1, -1};
        n.seq = 0;
        for (int k = (int)nodes.size() - 1; k >= 0; k--)
            if (nodes[k].stream == stream) {
                n.clock = nodes[k].clock, n.seq = nodes[k].seq + 1;
                break;
            }
        if (extra_pred >= 0)
            for (int s = 0; s < 4; s++) n.clock[s] = std::max(n.clock[s], nodes[extra_pred].clock[s]);
        n.clock[stream] = n.seq;
        nodes.push_back(n);
        return (int)nodes.size() - 1;
    }

    void run() {
        const int n_pad = in.n_pad, m_tot = in.m_tot;
        int last_record[8];
        std::fill(last_record, last_record + 8, -1);
        std::vector<std::pair<int, int>> signals;  // (panel, node)
        for (int s = 0; s < (int)plan.size(); s++) {
            const PotrfStep &p = plan[s];
            const int st = (int)p.stream;
            switch (p.kind) {
            case PotrfKind::RECORD: last_record[(int)p.ev] = add_node(s, st, -1); break;
            case PotrfKind::WAIT: {
                const int r = last_record[(int)p.ev];
                if (r < 0) rep.note(rep.unbound_waits, "WAIT with no earlier RECORD at step " + std::to_string(s));
                add_node(s, st, r);
                break;
            }
            case PotrfKind::SIGNAL: signals.push_back({p.panel, add_node(s, st, -1)}); break;
            case PotrfKind::POTF2: {
                const int n = add_node(s, st, -1);
                m_rect(n, p.k0, p.k0 + p.K, p.k0, p.k0 + p.K, true);
                d_slots(n, p.k0, p.k0 + p.K, true);
                m_finish(n, p.k0, p.k0 + p.K, p.k0, p.k0 + p.K, p.k0);
                break;
            }
            case PotrfKind::TRSM: {
                const int n = add_node(s, st, -1);
                m_rect(n, p.k0, p.k0 + p.K, p.k0, p.k0 + p.K, false);
                d_slots(n, p.k0, p.k0 + p.K, false);
                m_rect(n, p.k0 + p.K, m_tot, p.k0, p.k0 + p.K, true);
                m_finish(n, p.k0 + p.K, m_tot, p.k0, p.k0 + p.K, p.k0);
                break;
            }
            case PotrfKind::UPDATE: {
                const int n = add_node(s, st, -1);
                m_rect(n, p.r0, p.r0 + p.rows, p.k0, p.k0 + p.K, false);
                m_rect(n, p.c0, p.c0 + p.cols, p.k0, p.k0 + p.K, false);
                m_rect(n, p.r0, p.r0 + p.rows, p.c0, p.c0 + p.cols, true);
                m_apply(n, p.r0, p.r0 + p.rows, p.c0, p.c0 + p.cols, p.k0, p.k0 + p.K);
                if (p.lower && p.r0 != p.c0) rep.note(rep.algebra, "a lower update off the diagonal at step " + std::to_string(s));
                break;
            }
            case PotrfKind::PIPE: {
                // the launch's first diagonal block starts with the launch; with a signal panel everything else is ordered behind
                // the SIGNAL of that panel as well (the first panel's solve tasks wait for it on the device)
                const int g0 = p.c0, gend = p.c0 + p.cols, nb = std::min(p.cols, kPlanPanel);
                int n = add_node(s, st, -1);
                if (p.panel) {
                    m_rect(n, g0, g0 + nb, g0, g0 + nb, true);
                    d_slots(n, g0, g0 + nb, true);
                    int sig = -1;
                    for (auto &sg : signals)
                        if (sg.first == p.panel) sig = sg.second;
                    if (sig < 0) rep.note(rep.unbound_waits, "PIPE waits for a SIGNAL that was never issued, step " + std::to_string(s));
                    n = add_node(s, st, sig);
                }
                m_rect(n, g0, m_tot, g0, gend, true);
                d_slots(n, g0, gend, true);
                m_finish(n, g0, m_tot, g0, gend, g0);
                break;
            }
            case PotrfKind::FLOW: {
                const int n = add_node(s, st, -1);
                m_rect(n, p.r0, m_tot, p.r0, n_pad, true);
                d_slots(n, p.r0, n_pad, true);
                m_finish(n, p.r0, m_tot, p.r0, n_pad, p.r0);
                break;
            }
            case PotrfKind::W_TRSM: {
                const int n = add_node(s, st, -1);
                m_rect(n, p.k0, p.k0 + p.K, p.k0, p.k0 + p.K, false);
                d_slots(n, p.k0, p.k0 + p.K, false);
                w_rect(n, p.k0 + p.K, p.k0, p.k0 + p.K, true);
                for (int I = 0; I < (p.k0 + p.K) / 128; I++)
                    for (int J = p.k0 / 128; J < (p.k0 + p.K) / 128; J++) {
                        TileState &t = w[(size_t)I * T + J];
                        if (t.finisher >= 0) rep.note(rep.algebra, "a tile of W is solved twice: " + where(n));
                        t.finisher = n, t.fin_lo = p.k0;
                    }
                break;
            }
            case PotrfKind::W_UPDATE:
            case PotrfKind::W_LEFT: {
                const int n = add_node(s, st, -1);
                const bool lft = p.kind == PotrfKind::W_LEFT;
                const int rows = lft ? p.c0 : p.rows, k0 = lft ? 0 : p.k0, k1 = lft ? p.c0 : p.k0 + p.K;
                w_rect(n, rows, k0, k1, false);
                m_rect(n, p.c0, p.c0 + p.cols, k0, k1, false);
                w_rect(n, rows, p.c0, p.c0 + p.cols, true);
                for (int I = 0; I < (rows + 127) / 128; I++)
                    for (int J = p.c0 / 128; J < (p.c0 + p.cols) / 128; J++) w[(size_t)I * T + J].applied.push_back({k0, k1, n});
                break;
            }
            case PotrfKind::TILE_INVERSES: {
                const int n = add_node(s, st, -1);
                for (int J = 0; J < T; J++) touch(m[(size_t)J * T + J], n, false, "M", J, J);
                d_slots(n, 0, n_pad, true);
                break;
            }
            }
        }
    }

    // (c)
    void entry_exit() {
        int first = -1, last = -1;
        for (int k = 0; k < (int)nodes.size(); k++)
            if (nodes[k].stream == 0) {
                if (first < 0) first = k;
                last = k;
            }
        if (first < 0) {
            rep.note(rep.entry_exit, "no step on S");
            return;
        }
        for (int k = 0; k < (int)nodes.size(); k++) {
            if (!before(first, k)) rep.note(rep.entry_exit, where(k) + " may start before the first step on S");
            if (!before(k, last)) rep.note(rep.entry_exit, where(k) + " is not joined into the last step on S");
        }
    }

    // (d)
    void ranges(TileState &t, int need_lo, const char *what, int I, int J) {
        char tag[64];
        snprintf(tag, sizeof tag, "%s(%d,%d): ", what, I, J);
        if (t.finisher < 0) {
            rep.note(rep.algebra, std::string(tag) + "never factored or solved");
            return;
        }
        std::sort(t.applied.begin(), t.applied.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
        int covered = -1;  // the applied ranges from need_lo on are contiguous up to here
        int prev_hi = 0;
        for (const Range &r : t.applied) {
            if (r.lo < prev_hi) rep.note(rep.algebra, std::string(tag) + "K ranges overlap");
            prev_hi = r.hi;
            if (r.hi > t.fin_lo) rep.note(rep.algebra, std::string(tag) + "a K range beyond the tile's own panel");
            if (!before(r.node, t.finisher)) rep.note(rep.algebra, std::string(tag) + where(r.node) + " is not before " + where(t.finisher));
            if (r.hi <= need_lo) continue;
            if (covered < 0 ? r.lo > need_lo : r.lo != covered) rep.note(rep.algebra, std::string(tag) + "a gap in the K ranges");
            covered = r.hi;
        }
        if (need_lo < t.fin_lo && covered != t.fin_lo) rep.note(rep.algebra, std::string(tag) + "the K ranges do not reach the tile's panel");
    }
    void algebra() {
        for (int I = 0; I < TR; I++)
            for (int J = 0; J < T && J <= I; J++) ranges(m[(size_t)I * T + J], 0, "M", I, J);
        if (!in.rider) return;
        // row tile I of W is zero left of column 128 I: it needs the columns from its own panel on
        for (int J = 0; J < T; J++)
            for (int I = 0; I < T && I * 128 < (J * 128 / kPlanPanel + 1) * kPlanPanel; I++)
                ranges(w[(size_t)I * T + J], I * 128 / kPlanPanel * kPlanPanel, "W", I, J);
    }
    // the flops the roofline trace divides by: the lower triangle of the updated block by 2 K (the left-looking long update)
    void flops() {
        for (const PotrfStep &p : plan) {
            if (p.kind != PotrfKind::UPDATE || !p.timed) continue;
            const double nc = in.n_pad - p.c0;
            const double want = p.tag == 1 ? 2.0 * p.K * (nc * p.cols - 0.5 * p.cols * (p.cols - 1.0)) : p.K * nc * (nc + 1.0);
            if (p.flops != want || !p.lower) rep.note(rep.flops, "flops of a timed update");
        }
    }
};

static Report check(const PotrfPlanInput &in, const Steps &plan) {
    Report rep;
    Model mod(in, plan, rep);
    mod.run();
    mod.entry_exit();
    mod.algebra();
    mod.flops();
    return rep;
}

static int fails = 0;
static void expect(bool ok, const std::string &what) {
    if (!ok) {
        printf("FAIL %s\n", what.c_str());
        fails++;
    }
}

// ---- the checker has teeth: three broken plans derived from a good one (vectors on the host; nothing of the kind is ever run)
static void teeth(const Case &c) {
    Steps good;
    potrf_plan(c.in, good);
    expect(check(c.in, good).ok(), "teeth: the plan to break is good");
    int wait_lur = -1, wait_b = -1, upd = -1;
    for (int s = 0; s < (int)good.size(); s++) {
        const PotrfStep &p = good[s];
        // the WAIT(LUR) in front of a look-ahead group's first solve
        if (wait_lur < 0 && p.kind == PotrfKind::WAIT && p.ev == PotrfEvent::LUR && s + 1 < (int)good.size() && good[s + 1].kind == PotrfKind::TRSM)
            wait_lur = s;
        if (wait_b < 0 && p.kind == PotrfKind::WAIT && p.ev == PotrfEvent::B && p.stream == PotrfStream::S2) wait_b = s;
        if (upd < 0 && p.kind == PotrfKind::UPDATE && p.stream == PotrfStream::S && p.lower && p.rows > kPlanPanel) upd = s;
    }
    expect(wait_lur >= 0 && wait_b >= 0 && upd >= 0, "teeth: the plan has the steps to drop");
    if (wait_lur < 0 || wait_b < 0 || upd < 0) return;
    auto without = [&](int s) {
        Steps p = good;
        p.erase(p.begin() + s);
        return p;
    };
    const Report r1 = check(c.in, without(wait_lur)), r2 = check(c.in, without(wait_b)), r3 = check(c.in, without(upd));
    expect(r1.conflicts > 0, "teeth: a dropped WAIT(LUR) is reported as a conflict");
    expect(r2.conflicts > 0, "teeth: a dropped WAIT(B) is reported as a conflict");
    expect(r3.algebra > 0, "teeth: a dropped UPDATE is reported by the algebra");
    printf("broken plans reported: no WAIT(LUR): %s | no WAIT(B): %s | no UPDATE: %s\n", r1.first.c_str(), r2.first.c_str(), r3.first.c_str());
}

int main(int argc, char **argv) {
    const std::vector<Case> cs = cases();
    if (argc == 2 && !strcmp(argv[1], "--list")) {  // what a recording harness needs (README in the golden directory)
        for (const Case &c : cs)
            printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", c.name.c_str(), c.in.n_pad, c.in.m_tot, c.in.GW, (int)c.in.left,
                   (int)c.in.w_left, chain_code(c.in.chain), c.in.tail_cols, (int)c.in.lookahead, (int)c.in.rider, c.in.seqs, c.in.look_min,
                   c.in.lur_side, (int)c.in.trace, c.nz);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--print")) {
        for (const Case &c : cs)
            if (c.name == argv[2]) {
                Steps plan;
                potrf_plan(c.in, plan);
                fputs(print_plan(c, plan).c_str(), stdout);
                return 0;
            }
        return 2;
    }
    if (argc != 2) {
        printf("usage: potrf_plan_test <golden dir> | --list | --print <case>\n");
        return 2;
    }
    for (const Case &c : cs) {
        Steps plan;
        potrf_plan(c.in, plan);
        expect(plan.size() <= potrf_plan_max_steps(c.in), c.name + ": potrf_plan_max_steps bounds the plan");
        Steps again;
        potrf_plan(c.in, again);
        expect(again.size() == plan.size(), c.name + ": the plan is a function of its input");
        std::ifstream f(std::string(argv[1]) + "/" + c.name + ".txt");
        std::stringstream want;
        want << f.rdbuf();
        const std::string got = print_plan(c, plan);
        expect(f.good() && !want.str().empty(), c.name + ": the recorded trace is there");
        if (got != want.str()) {
            std::istringstream a(got), b(want.str());
            std::string la, lb;
            int line = 1;
            while (std::getline(a, la) && std::getline(b, lb) && la == lb) line++;
            expect(false, c.name + ": (a) differs from the recorded trace at line " + std::to_string(line) + ":\n  plan   " + la + "\n  parent " + lb);
        }
        const Report rep = check(c.in, plan);
        expect(rep.unbound_waits == 0 && rep.conflicts == 0, c.name + ": (b) " + rep.first);
        expect(rep.entry_exit == 0, c.name + ": (c) " + rep.first);
        expect(rep.algebra == 0 && rep.flops == 0, c.name + ": (d) " + rep.first);
        printf("%s %s: %d steps\n", rep.ok() && got == want.str() ? "ok" : "BAD", c.name.c_str(), (int)plan.size());
    }
    for (const Case &c : cs)
        if (c.name == "look_n8192") teeth(c);
    if (fails) {
        printf("%d failures\n", fails);
        return 1;
    }
    printf("potrf plan ok: %d cases\n", (int)cs.size());
    return 0;
}
