// Predictions of a fitted dense GP and their x-gradients (GaussianProcess::predict / predict_var / predict_valvar,
// crates/gp/src/algorithm.rs:253-380; predict_gradients / predict_var_gradients :510-727): batched paths on the
// factorisation's own kernels, and few-query paths for EGO's one-point-at-a-time calls.
#include "gp_handle.h"

using namespace egx;

namespace egx {


// ---- prediction -------------------------------------------------------------------------------
int check_query(const egx_gp *gp, const double *xq, int64_t m) {
    if (!gp->fitted) {
        set_error("model is not fitted (call egx_gp_finalize or egx_gp_fit first)");
        return EGX_ERR_NOT_FITTED;
    }
    if (m < 0 || (m > 0 && !xq)) {
        set_error("bad query array");
        return EGX_ERR_INVALID_VALUE;
    }
    return EGX_SUCCESS;
}

// few queries: split the training range so that ~1024 (mean) / ~512 (x-gradient) workgroups exist
static int even_splits(int slabs, int want) {
    if (want > slabs) want = slabs;
    const int per = (slabs + want - 1) / want;
    return (slabs + per - 1) / per;
}
int mean_splits(int rows, int m_pad) {
    const int wgs = m_pad / 64;
    return even_splits(rows / 64, wgs < 1024 ? (1024 + wgs - 1) / wgs : 1);
}
int xgrad_splits(int rows, int m_pad) {
    const int wgs = m_pad / 128;
    return even_splits((rows + 63) / 64, wgs < 512 ? (512 + wgs - 1) / wgs : 1);
}

// corr (m x n): algorithm.rs:372-380 ; rt = C^-1 corr^T: :337-350 (held transposed, row per query) ; sum rt^2 and ft^T rt
// (:352): the factor and its tile inverses are workspace 0's, the ft^T rows live below the factor
int posterior_solve(egx_gp *gp, hipStream_t st, const double *xqT, int m_pad, double *RT, double *s0, double *sl) {
    return posterior_solve_run(&gp, 1, st, xqT, m_pad, RT, s0, sl);
}
// the members' own pointers of a posterior batch; the strides are the caller's layout
static void posterior_batch(egx_gp *const *gps, int len, PosteriorBatch &pb) {
    pb.count = len;
    for (int j = 0; j < len; j++) {
        const egx_gp *g = gps[j];
        pb.ptrs.par[j] = dev_xnorm(g);
        pb.ptrs.xT[j] = g->d_xT;
        pb.ptrs.coef[j] = g->d_fit_coef;
        pb.ptrs.gamma[j] = g->d_gamma;
        pb.ptrs.ftT[j] = g->ws[0].M + (size_t)g->n_pad * g->ld;
        pb.ptrs.spec[j] = dev_spec(g);
    }
}
// ... of a run of `len` models of one shape whose factors sit at one stride (members of a group in consecutive slots; a lone
// model is a run of one): member j's blocks are xqT + j d m_pad, RT + j m_pad n_pad, s0 + j m_pad, sl + j m_pad p
int posterior_solve_run(egx_gp *const *gps, int len, hipStream_t st, const double *xqT, int m_pad, double *RT, double *s0, double *sl) {
    const egx_gp *lead = gps[0];
    const Workspace &w = lead->ws[0];
    const int n_pad = lead->n_pad;
    PosteriorBatch pb;
    posterior_batch(gps, len, pb);
    pb.sq = (int64_t)lead->d * m_pad, pb.sR = (int64_t)m_pad * n_pad, pb.ss0 = m_pad, pb.ssl = (int64_t)m_pad * lead->p;
    TrsmBatch tb;
    tb.count = len;
    if (len > 1) tb.sM = gps[1]->ws[0].M - w.M, tb.sD = gps[1]->ws[0].dinv - w.dinv;
    tb.sR = pb.sR;
    EGX_RC(launch_cross_corr(st, lead->corr, pb, xqT, m_pad, m_pad, n_pad, n_pad, lead->d, lead->fit_hcols, RT, n_pad));
    EGX_RC(launch_trsm_rows(st, w.M, lead->ld, n_pad, w.dinv, RT, n_pad, m_pad, 0, &tb));
    return launch_row_reduce(st, pb, RT, n_pad, m_pad, lead->n, lead->ld, lead->p, s0, sl);
}
// -Z^T = 0 - C^-T rt as an (n_pad x m_pad) matrix (W upper triangular: K range starts at the row tile)
int posterior_weights(egx_gp *gp, hipStream_t st, const double *RT, int m_pad, double *Wt) {
    return posterior_weights_run(&gp, 1, st, RT, m_pad, Wt);
}
// -(Z + E)^T : Wt -= (-R^-1 F) (-D)^T
int posterior_weights_trend(egx_gp *gp, hipStream_t st, const double *dneg, int m_pad, double *Wt) {
    return posterior_weights_trend_run(&gp, 1, st, dneg, m_pad, Wt);
}
// ... of a run of `len` models of one shape whose C^-T and -R^-1 F sit at one stride (members of a group in consecutive slots:
// the group's slab, ensure_winv; a lone model is a run of one): ONE GEMM launch, the member a grid coordinate.  Member j's blocks
// are RT + j m_pad n_pad, dneg + j m_pad rhs_pad and Wt + j n_pad m_pad.  The GEMM's kernel is chosen by one matrix' shape.
int posterior_weights_run(egx_gp *const *gps, int len, hipStream_t st, const double *RT, int m_pad, double *Wt) {
    const egx_gp *lead = gps[0];
    const int n_pad = lead->n_pad;
    GemmBatch gb;
    gb.count = len;
    gb.sC = (int64_t)n_pad * m_pad, gb.sB = (int64_t)m_pad * n_pad;
    if (len > 1) gb.sA = dev_winv(gps[1]) - dev_winv(lead);
    EGX_HIP_CHECK(hipMemsetAsync(Wt, 0, sizeof(double) * (size_t)n_pad * m_pad * len, st));
    return launch_gemm_nt_sub(st, Wt, m_pad, dev_winv(lead), n_pad, RT, n_pad, n_pad, m_pad, n_pad, 0, 1, nullptr, nullptr, &gb);
}
int posterior_weights_trend_run(egx_gp *const *gps, int len, hipStream_t st, const double *dneg, int m_pad, double *Wt) {
    const egx_gp *lead = gps[0];
    const int rp = lead->rhs_pad;
    GemmBatch gb;
    gb.count = len;
    gb.sC = (int64_t)lead->n_pad * m_pad, gb.sB = (int64_t)m_pad * rp;
    if (len > 1) gb.sA = dev_neg_invkf(gps[1]) - dev_neg_invkf(lead);
    return launch_gemm_nt_sub(st, Wt, m_pad, dev_neg_invkf(lead), rp, dneg, rp, lead->n_pad, m_pad, rp, 0, 0, nullptr, nullptr, &gb);
}

static int predict_var_small(egx_gp *gp, const double *xq, int64_t m, double *vout);
static int small_path_buffers(egx_gp *gp);
static void posterior_batch(egx_gp *const *gps, int len, PosteriorBatch &pb);

int predict_impl(egx_gp *gp, const double *xq, int64_t m, double *yout, double *vout) {
    EGX_RC(check_query(gp, xq, m));
    EGX_RC(set_device(gp));
    if (vout && m > 0 && m <= 8 && gp->winv_fail_epoch != gp->fit_epoch) {
        // a few points at a time: EGO's inner loop (its criteria ask for value AND variance).  The cached C^-T behind
        // this path is an OPTIMISATION (a second n_pad^2 matrix): when it cannot be had -- allocation failure, or less
        // than its size + 25 % free on the device -- the batched path below serves the call, for this fit and all later
        // small calls on it.
        const bool have_w = gp->winv_epoch == gp->fit_epoch && dev_winv(gp) && dev_neg_invkf(gp);
        if (have_w || ++gp->small_var_calls >= 3) {
            int rc = EGX_SUCCESS;
            if (!have_w && !dev_winv(gp)) {  // (a member of a group: the slab of all its members)
                size_t fr = 0, tot = 0;
                const size_t need = sizeof(double) * (size_t)gp->n_pad * gp->n_pad * (gp->group ? gp->group->k : 1);
                if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < need + need / 4) rc = EGX_ERR_HIP;
            }
            if (rc == EGX_SUCCESS) rc = ensure_winv(gp);
            if (rc == EGX_SUCCESS) rc = small_path_buffers(gp);
            if (rc == EGX_SUCCESS) {
                if (yout) EGX_RC(predict_impl(gp, xq, m, yout, nullptr));  // split-range mean kernel
                return predict_var_small(gp, xq, m, vout);
            }
            (void)hipGetLastError();
            if (gp->winv_epoch != gp->fit_epoch && !gp->group) {  // give a half-built cache back (a group keeps its slab)
                gp->d_W.reset();
                gp->d_neg_invkf.reset();
            }
            gp->winv_fail_epoch = gp->fit_epoch;
        }
    }
    return predict_run(&gp, 1, &xq, m, yout ? &yout : nullptr, vout ? &vout : nullptr);
}

// The queries of one chunk of the batched posterior: so many that the (m_tile x n_pad) block of predict_var stays <= 1 GiB
// (kBlockDoubles).  ONE rule for predict_run's chunks and for how many members of a run fit beside each other
// (predict_run_members): the chunks of a run must be the lone call's, or the bits are not.
constexpr int64_t kBlockDoubles = (int64_t)1 << 27;
static int64_t predict_chunk_cap(int n_pad, bool want_var) {
    if (!want_var) return 65536;
    int64_t cap = kBlockDoubles / n_pad / kTile * kTile;
    if (cap < kTile) cap = kTile;
    if (cap > 16384) cap = 16384;
    return cap;
}
// how many members' (m_pad x n_pad) blocks of the largest chunk of m queries stay within kBlockDoubles together (>= 1)
static int predict_run_members(int n_pad, int64_t m, bool want_var, int len) {
    if (!want_var) return len;
    const int64_t m_pad = round_up(std::min(m, predict_chunk_cap(n_pad, true)), kTile);
    return (int)std::max<int64_t>(1, std::min<int64_t>(len, kBlockDoubles / (m_pad * n_pad)));
}

// The batched posterior of a run of `len` fitted models of one shape (one n, d, trend and correlation; fit_hcols equal) whose
// factors sit at one stride -- members of a group in consecutive slots, or ONE model: predict_impl's batched route is this with
// len = 1.  Member j answers its own m queries xq[j] (original units) into yout[j] / vout[j] (either array may be nullptr as a
// whole).  One launch sequence, one upload, one read-back and one host synchronisation per chunk, whatever len is; the
// kernels take the member as a grid coordinate and do a member's arithmetic the same way whatever its companions, and the
// chunks are those of the lone call, so every member's results are the lone call's bits.
int predict_run(egx_gp *const *gps, int len, const double *const *xq, int64_t m, double *const *yout, double *const *vout) {
    egx_gp *lead = gps[0];
    Workspace &w = lead->ws[0];
    const int n_pad = lead->n_pad, d = lead->d, p = lead->p;
    const bool prescaled = predict_mean_prescaled(d, lead->fit_hcols);
    const int64_t cap = predict_chunk_cap(n_pad, vout != nullptr);
    // Two chunks in flight on two streams: while the GPU works on chunk i the host post-processes chunk i - 1 and
    // normalises / uploads chunk i + 1, and the tail of one chunk's solve overlaps the head of the next (the (m x n)
    // block of a chunk is bounded at 1 GiB, so 100 000 query points at n = 8192 are 7 chunks).
    struct Slot {
        DevBuf d_xraw, d_xqT, d_racc, d_RT, d_s0, d_sl;  // sized by the first (largest) chunk, reused by the later ones
        std::vector<double> stage, racc, s0, sl;          // stage: the members' raw rows side by side (len > 1)
        int64_t m0 = 0;
        int mc = 0, m_pad = 0, msplit = 1;
        hipStream_t stream = nullptr;
    } slots[2];
    slots[0].stream = w.stream;
    slots[1].stream = w.lk.s2 ? w.lk.s2 : w.stream;
    PosteriorBatch pb;
    posterior_batch(gps, len, pb);
    auto enqueue = [&](Slot &sl_, int64_t m0) -> int {
        const int mc = (int)((m - m0 < cap) ? (m - m0) : cap);
        const int m_pad = (int)round_up(mc, kTile);
        sl_.m0 = m0;
        sl_.mc = mc;
        sl_.m_pad = m_pad;
        hipStream_t st = sl_.stream;
        // the raw rows as the caller holds them (xq outlives the call, the staging copy the slot), normalised on the device
        // (algorithm.rs:254) with every member's own x_mean | x_std
        const size_t blk = (size_t)mc * d;
        EGX_RC(sl_.d_xraw.alloc(blk * len));
        EGX_RC(sl_.d_xqT.alloc((size_t)d * m_pad * len));
        const double *src = xq[0] + (size_t)m0 * d;
        if (len > 1) {
            sl_.stage.resize(blk * len);
            for (int j = 0; j < len; j++) std::memcpy(&sl_.stage[blk * j], xq[j] + (size_t)m0 * d, sizeof(double) * blk);
            src = sl_.stage.data();
        }
        EGX_HIP_CHECK(hipMemcpyAsync(sl_.d_xraw.p, src, sizeof(double) * blk * len, hipMemcpyHostToDevice, st));
        pb.sq = (int64_t)d * m_pad;
        EGX_RC(launch_normalize_queries(st, pb, sl_.d_xraw.p, (int64_t)blk, mc, d, sl_.d_xqT.p, m_pad, m_pad));
        const int msplit = sl_.msplit = mean_splits(n_pad, m_pad);  // (partial sums added below)
        if (yout) {
            EGX_RC(sl_.d_racc.alloc((size_t)msplit * m_pad * len));
            PosteriorBatch pm = pb;
            pm.sracc = (int64_t)msplit * m_pad;
            if (prescaled)
                for (int j = 0; j < len; j++) pm.ptrs.xT[j] = dev_xs_fit(gps[j]);
            EGX_RC(launch_predict_mean(st, lead->corr, pm, sl_.d_xqT.p, m_pad, m_pad, n_pad, n_pad, d, lead->fit_hcols, sl_.d_racc.p,
                                       msplit, prescaled ? 1 : 0));
        }
        if (vout) {
            EGX_RC(sl_.d_RT.alloc((size_t)m_pad * n_pad * len));
            EGX_RC(sl_.d_s0.alloc((size_t)m_pad * len));
            EGX_RC(sl_.d_sl.alloc((size_t)m_pad * p * len));
            EGX_RC(posterior_solve_run(gps, len, st, sl_.d_xqT.p, m_pad, sl_.d_RT.p, sl_.d_s0.p, sl_.d_sl.p));
        }
        return EGX_SUCCESS;
    };
    std::vector<double> f(p), rhs(p), u(p), xn(d);
    auto finish = [&](Slot &sl_) -> int {
        const int mc = sl_.mc, m_pad = sl_.m_pad, msplit = sl_.msplit;
        const int64_t m0 = sl_.m0;
        EGX_HIP_CHECK(hipStreamSynchronize(sl_.stream));
        // (the copies go to pageable memory: issued after the wait, they cost their transfer time only)
        const size_t nracc = (size_t)msplit * m_pad, ns0 = (size_t)m_pad, nsl = (size_t)m_pad * p;
        if (yout) {
            sl_.racc.resize(nracc * len);
            EGX_HIP_CHECK(hipMemcpy(sl_.racc.data(), sl_.d_racc.p, sizeof(double) * nracc * len, hipMemcpyDeviceToHost));
        }
        if (vout) {
            sl_.s0.resize(ns0 * len);
            sl_.sl.resize(nsl * len);
            EGX_HIP_CHECK(hipMemcpy(sl_.s0.data(), sl_.d_s0.p, sizeof(double) * ns0 * len, hipMemcpyDeviceToHost));
            EGX_HIP_CHECK(hipMemcpy(sl_.sl.data(), sl_.d_sl.p, sizeof(double) * nsl * len, hipMemcpyDeviceToHost));
        }
        for (int j = 0; j < len; j++) {
            const egx_gp *gp = gps[j];
            const double *racc = yout ? &sl_.racc[nracc * j] : nullptr;
            const double *s0 = vout ? &sl_.s0[ns0 * j] : nullptr, *sl = vout ? &sl_.sl[nsl * j] : nullptr;
            const double *raw = xq[j] + (size_t)m0 * d;
            for (int a = 0; a < mc; a++) {
                // the trend needs the normalised coordinates (Linear / Quadratic): the same subtraction and division as the device's
                if (gp->mean >= 1)
                    for (int c = 0; c < d; c++) xn[c] = (query_coord(gp, raw + (size_t)a * d, c) - gp->x_mean[c]) / gp->x_std[c];
                hm::regression_row(gp->mean, gp->mean >= 1 ? xn.data() : nullptr, d, f.data());
                if (yout) {
                    double fb = 0.0, rg = 0.0;
                    for (int l = 0; l < p; l++) fb += f[l] * gp->beta[l];
                    for (int sp = 0; sp < msplit; sp++) rg += racc[(size_t)sp * m_pad + a];
                    yout[j][m0 + a] = (fb + rg) * gp->y_std + gp->y_mean;  // algorithm.rs:260-262
                }
                if (vout) {
                    // u = (Rq^T)^-1 (ft^T rt - f^T)   algorithm.rs:352-367 ; Rq^T lower triangular
                    for (int l = 0; l < p; l++) rhs[l] = sl[(size_t)a * p + l] - f[l];
                    const double usq = hm::trend_forward(gp->ft_qr_r.data(), p, rhs.data(), u.data());
                    double mse = gp->sigma2 * (1.0 - s0[a] + usq);     // algorithm.rs:272-274
                    vout[j][m0 + a] = (mse < 0.0) ? 0.0 : mse;         // :278
                }
            }
        }
        return EGX_SUCCESS;
    };
    int cur = 0, rc = EGX_SUCCESS;
    bool pending = false;
    for (int64_t m0 = 0; m0 < m && !rc; m0 += cap) {
        rc = enqueue(slots[cur], m0);
        if (!rc && pending) rc = finish(slots[cur ^ 1]);
        pending = !rc;
        cur ^= 1;
    }
    if (!rc && pending) rc = finish(slots[cur ^ 1]);
    if (rc) {  // nothing may still run on the buffers the slots are about to free
        (void)hipStreamSynchronize(slots[0].stream);
        (void)hipStreamSynchronize(slots[1].stream);
        (void)hipGetLastError();
    }
    return rc;
}

// d_W <- C^-T (upper triangular, rows of the identity through the forward block substitution) and
// d_neg_invkf <- -C^-T [ft | yt] for the factor resident in workspace 0; cached per fitted state.
int ensure_winv(egx_gp *gp) {
    if (gp->winv_epoch == gp->fit_epoch && dev_winv(gp) && dev_neg_invkf(gp)) return EGX_SUCCESS;
    Workspace &w = gp->ws[0];
    const int n_pad = gp->n_pad;
    const size_t sq = (size_t)n_pad * n_pad;
    if (gp->group) {
        // a member of a group: the two matrices of ALL members in the group's slab, at one stride, allocated by whichever member
        // asks first -- what lets a run of members take its weight GEMMs as one launch (posterior_weights_run); a member's own
        // calls read the same matrix.  Memory per member is what a lone handle holds.
        std::lock_guard<std::mutex> lk(gp->group->winv_mu);
        EGX_RC(gp->group->W.alloc(sq * gp->group->k));
        EGX_RC(gp->group->NK.alloc((size_t)n_pad * gp->rhs_pad * gp->group->k));
    } else {
        EGX_RC(gp->d_W.alloc(sq));
        EGX_RC(gp->d_neg_invkf.alloc((size_t)n_pad * gp->rhs_pad));
    }
    double *const d_W = dev_winv(gp), *const d_neg_invkf = dev_neg_invkf(gp);
    // the rows of the identity, written on the device as far as the solve and the readers of W touch them (everything
    // on and above the diagonal 128-tiles): no host round trip, no 2 GiB memset
    EGX_RC(launch_identity_rows(w.stream, d_W, n_pad, n_pad));
    EGX_RC(launch_trsm_rows(w.stream, w.M, gp->ld, n_pad, w.dinv, d_W, n_pad, n_pad, 1));
    EGX_HIP_CHECK(hipMemsetAsync(d_neg_invkf, 0, sizeof(double) * (size_t)n_pad * gp->rhs_pad, w.stream));
    // 0 - W [ft | yt]: the rows [ft | yt]^T sit below the factor; W upper triangular -> K range starts at the row tile
    EGX_RC(launch_gemm_nt_sub(w.stream, d_neg_invkf, gp->rhs_pad, d_W, n_pad, w.M + (size_t)n_pad * gp->ld,
                              gp->ld, n_pad, gp->rhs_pad, n_pad, 0, 1));
    {
        std::vector<double> tmp((size_t)n_pad * gp->rhs_pad);
        EGX_HIP_CHECK(hipMemcpyAsync(tmp.data(), d_neg_invkf, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, w.stream));
        EGX_HIP_CHECK(hipStreamSynchronize(w.stream));
        gp->h_neg_invkf.resize((size_t)gp->n * gp->p);
        for (int i = 0; i < gp->n; i++)
            for (int l = 0; l < gp->p; l++) gp->h_neg_invkf[(size_t)i * gp->p + l] = tmp[(size_t)i * gp->rhs_pad + l];
    }
    gp->winv_epoch = gp->fit_epoch;
    return EGX_SUCCESS;
}

int ensure_trend_state(egx_gp *gp, hipStream_t st) {
    if (gp->trend_epoch == gp->fit_epoch && gp->d_fidx) return EGX_SUCCESS;
    const int p = gp->p;
    const std::vector<int> idx = hm::regression_index(gp->mean, gp->d);
    std::vector<double> rt((size_t)p * p);
    for (int i = 0; i < p; i++)
        for (int l = 0; l < p; l++) rt[(size_t)i * p + l] = gp->ft_qr_r[(size_t)l * p + i];
    EGX_RC(gp->d_tbeta.alloc(p));
    EGX_RC(gp->d_rq.alloc((size_t)p * p));
    EGX_RC(gp->d_rqT.alloc((size_t)p * p));
    EGX_RC(gp->d_fidx.alloc(idx.size()));
    EGX_HIP_CHECK(hipMemcpyAsync(gp->d_tbeta, gp->beta.data(), sizeof(double) * p, hipMemcpyHostToDevice, st));
    EGX_HIP_CHECK(hipMemcpyAsync(gp->d_rq, gp->ft_qr_r.data(), sizeof(double) * (size_t)p * p, hipMemcpyHostToDevice, st));
    EGX_HIP_CHECK(hipMemcpyAsync(gp->d_rqT, rt.data(), sizeof(double) * (size_t)p * p, hipMemcpyHostToDevice, st));
    EGX_HIP_CHECK(hipMemcpyAsync(gp->d_fidx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice, st));
    EGX_HIP_CHECK(hipStreamSynchronize(st));  // rt and idx are locals; once per fitted state
    gp->trend_epoch = gp->fit_epoch;
    return EGX_SUCCESS;
}

// Small batches (EGO's infill optimiser asks for one point at a time): per query two memory-bound passes over the cached
// W = C^-T instead of the batched block solves, then the x-gradient contraction with a per-training-point weight VECTOR.
static int small_path_buffers(egx_gp *gp) {
    if (gp->sp_xq) return EGX_SUCCESS;  // (the last one allocated)
    const int n = gp->n, n_pad = gp->n_pad, d = gp->d;
    int nsplit = (n + 63) / 64;
    if (nsplit > 512) nsplit = 512;
    const int slabs = (n + 63) / 64, per = (slabs + nsplit - 1) / nsplit;
    gp->sp_nsplit = (slabs + per - 1) / per;
    EGX_RC(gp->sp_R.alloc((size_t)kTile * n_pad));
    EGX_RC(gp->sp_P.alloc((size_t)32 * n_pad));
    EGX_RC(gp->sp_y.alloc((size_t)n_pad));
    EGX_RC(gp->sp_z.alloc((size_t)n_pad));
    EGX_RC(gp->sp_wt.alloc((size_t)n_pad));
    EGX_RC(gp->sp_out.alloc((size_t)gp->sp_nsplit * kTile * d));
    return gp->sp_xq.alloc((size_t)d * kTile);
}

// normalised query a of xq, k-major with the other 127 slots zero, into the cached device slab; xn (d) on the host
static int small_path_query(egx_gp *gp, const double *xq, int64_t a, std::vector<double> &xn, std::vector<double> &slab) {
    const int d = gp->d;
    xn.resize(d);
    slab.assign((size_t)d * kTile, 0.0);
    for (int j = 0; j < d; j++) {
        xn[j] = (query_coord(gp, xq + (size_t)a * d, j) - gp->x_mean[j]) / gp->x_std[j];
        slab[(size_t)j * kTile] = xn[j];
    }
    EGX_HIP_CHECK(hipMemcpyAsync(gp->sp_xq, slab.data(), sizeof(double) * slab.size(), hipMemcpyHostToDevice, gp->ws[0].stream));
    return EGX_SUCCESS;
}

// y = C^-1 r, z = R^-1 r of ONE query (already in sp_xq) on the host; needs ensure_winv
static int small_path_solve(egx_gp *gp, std::vector<double> &y, std::vector<double> &z, bool want_z) {
    Workspace &w = gp->ws[0];
    const int n = gp->n, n_pad = gp->n_pad, d = gp->d;
    EGX_RC(launch_cross_corr(w.stream, gp->corr, gp->sp_xq, kTile, kTile, gp->d_xT, n_pad, n_pad, d, gp->d_fit_coef,
                             gp->fit_hcols, gp->sp_R, n_pad));
    EGX_RC(launch_uptri_solve_pair(w.stream, dev_winv(gp), n_pad, n, n_pad, gp->sp_R, gp->sp_P, gp->sp_y, gp->sp_z));
    y.resize(n_pad);
    EGX_HIP_CHECK(hipMemcpyAsync(y.data(), gp->sp_y, sizeof(double) * n_pad, hipMemcpyDeviceToHost, w.stream));
    if (want_z) {
        z.resize(n_pad);
        EGX_HIP_CHECK(hipMemcpyAsync(z.data(), gp->sp_z, sizeof(double) * n_pad, hipMemcpyDeviceToHost, w.stream));
    }
    EGX_HIP_CHECK(hipStreamSynchronize(w.stream));
    return EGX_SUCCESS;
}

static int xgrad_small(egx_gp *gp, const double *xq, int64_t m, double *gy, double *gv) {
    Workspace &w = gp->ws[0];
    const int n = gp->n, n_pad = gp->n_pad, d = gp->d, p = gp->p;
    if (gv) EGX_RC(ensure_winv(gp));
    EGX_RC(small_path_buffers(gp));
    const int m_pad = kTile;
    const int nblk = (n + 255) / 256;  // k_xgrad_point: one partial row of d sums per 256 training points
    std::vector<double> xn, slab, y, z, wt(n_pad, 0.0), part((size_t)nblk * d), f(p), a_vec(p), u(p), dd(p), df(d);
    auto reduce_out = [&](int k) {
        double sacc = 0.0;
        for (int sidx = 0; sidx < nblk; sidx++) sacc += part[(size_t)sidx * d + k];
        return sacc;
    };
    auto contract = [&](const double *weights) -> int {
        EGX_RC(launch_xgrad_point(w.stream, gp->corr, gp->sp_xq, m_pad, 1, gp->d_xT, n_pad, n, d, gp->d_fit_coef,
                                  gp->fit_hcols, weights, gp->sp_out));
        EGX_HIP_CHECK(hipMemcpyAsync(part.data(), gp->sp_out, sizeof(double) * (size_t)nblk * d, hipMemcpyDeviceToHost,
                                     w.stream));
        EGX_HIP_CHECK(hipStreamSynchronize(w.stream));
        return EGX_SUCCESS;
    };
    for (int64_t a = 0; a < m; a++) {
        EGX_RC(small_path_query(gp, xq, a, xn, slab));
        if (gy) {
            EGX_RC(contract(gp->d_gamma));
            hm::regression_jac_dot(gp->mean, xn.data(), d, gp->beta.data(), df.data());
            for (int k = 0; k < d; k++) gy[(size_t)a * d + k] = (df[k] + reduce_out(k)) * gp->y_std / gp->x_std[k];
        }
        if (gv) {
            EGX_RC(small_path_solve(gp, y, z, true));
            hm::regression_row(gp->mean, xn.data(), d, f.data());
            for (int l = 0; l < p; l++) {  // A = f - ft^T rt
                double sacc = 0.0;
                for (int i = 0; i < n; i++) sacc += gp->ft[(size_t)i * p + l] * y[i];
                a_vec[l] = f[l] - sacc;
            }
            (void)hm::trend_forward(gp->ft_qr_r.data(), p, a_vec.data(), u.data());
            hm::trend_backward(gp->ft_qr_r.data(), p, u.data(), dd.data());
            for (int i = 0; i < n; i++) {  // -(R^-1 r + R^-1 F D)_i
                double e = 0.0;
                for (int l = 0; l < p; l++) e += gp->h_neg_invkf[(size_t)i * p + l] * dd[l];
                wt[i] = -z[i] + e;
            }
            EGX_HIP_CHECK(hipMemcpyAsync(gp->sp_wt, wt.data(), sizeof(double) * n_pad, hipMemcpyHostToDevice, w.stream));
            EGX_RC(contract(gp->sp_wt));
            hm::regression_jac_dot(gp->mean, xn.data(), d, dd.data(), df.data());
            for (int k = 0; k < d; k++) gv[(size_t)a * d + k] = 2.0 * gp->sigma2 * (df[k] + reduce_out(k)) / gp->x_std[k];
        }
    }
    return EGX_SUCCESS;
}

// predict_var of a few points through the cached W (built on the third such call after a fit, or by any gradient call)
static int predict_var_small(egx_gp *gp, const double *xq, int64_t m, double *vout) {
    const int n = gp->n, d = gp->d, p = gp->p;
    EGX_RC(ensure_winv(gp));
    EGX_RC(small_path_buffers(gp));
    std::vector<double> xn, slab, y, z, f(p), rhs(p), u(p);
    for (int64_t a = 0; a < m; a++) {
        EGX_RC(small_path_query(gp, xq, a, xn, slab));
        EGX_RC(small_path_solve(gp, y, z, false));
        double s0 = 0.0;
        for (int i = 0; i < n; i++) s0 += y[i] * y[i];
        hm::regression_row(gp->mean, xn.data(), d, f.data());
        for (int i = 0; i < p; i++) {  // u = (Rq^T)^-1 (ft^T rt - f)   algorithm.rs:352-367
            rhs[i] = -f[i];
            for (int t = 0; t < n; t++) rhs[i] += gp->ft[(size_t)t * p + i] * y[t];
        }
        const double usq = hm::trend_forward(gp->ft_qr_r.data(), p, rhs.data(), u.data());
        const double mse = gp->sigma2 * (1.0 - s0 + usq);
        vout[a] = (mse < 0.0) ? 0.0 : mse;
    }
    return EGX_SUCCESS;
}

// predict_gradients / predict_var_gradients (algorithm.rs:510-549, 555-617, 702-727), batched over the queries:
//   d mean / d x_k = (dF beta + sum_i gamma_i dr_i/dx_k) y_std / x_std_k
//   d var  / d x_k = 2 sigma2 / x_std_k * ( D^T dF_k - sum_i (R^-1 r + R^-1 F D)_i dr_i/dx_k ),  D = B^-1 A^T,
//   A = f(x)^T - r^T R^-1 F = f^T - rt^T ft,  B = F^T R^-1 F = Rq^T Rq   (Rq = ft_qr_r, so D = Rq^-1 Rq^-T A^T)
// The reference redoes R^-1 F and chol(B) for every query point; here they are per-fit state, the per-query
// R^-1 r = C^-T (C^-1 r) is the predict_var solve followed by one GEMM with the cached C^-T.
int xgrad_impl(egx_gp *gp, const double *xq, int64_t m, double *gy, double *gv) {
    EGX_RC(check_query(gp, xq, m));
    EGX_RC(set_device(gp));
    // (the few-query kernel keeps 5 + hcols doubles per input dimension in LDS, the batched one 1 + hcols: very wide
    //  inputs take the batched form whatever m is)
    if (m > 0 && m <= 8 && (int64_t)gp->d * (gp->fit_hcols + 5) <= 20480) return xgrad_small(gp, xq, m, gy, gv);
    return xgrad_run(&gp, 1, &xq, m, gy ? &gy : nullptr, gv ? &gv : nullptr);
}

// The batched x-gradients of a run of `len` fitted models of one shape whose factors -- and, for the variance, whose C^-T and
// -R^-1 F (ensure_winv: the group's slab) -- sit at one stride: members of a group in consecutive slots, or ONE model
// (xgrad_impl's batched route is this with len = 1).  Member j answers its own m queries xq[j] into gy[j] / gv[j] (m x d; either
// array may be nullptr as a whole).  One launch sequence, one upload and one read-back per chunk and half, whatever len is.  The
// kernels take the member as a grid coordinate, the splits of the training range come from one member's shape and the chunks are
// the lone call's, so every member's results are the lone call's bits.
int xgrad_run(egx_gp *const *gps, int len, const double *const *xq, int64_t m, double *const *gy, double *const *gv) {
    egx_gp *lead = gps[0];
    Workspace &w = lead->ws[0];
    const int n = lead->n, n_pad = lead->n_pad, d = lead->d, p = lead->p, rp = lead->rhs_pad;
    if (gv)
        for (int j = 0; j < len; j++) EGX_RC(ensure_winv(gps[j]));
    const int64_t cap = predict_chunk_cap(n_pad, gv != nullptr);
    PosteriorBatch pb;
    posterior_batch(gps, len, pb);
    std::vector<double> stage, xn, part, sl, f(p), a_vec(p), u(p), dd(p), dneg, df(d);
    DevBuf d_xraw, d_xqT, d_out, d_RT, d_s0, d_sl, d_Wt, d_D;  // sized by the first (largest) chunk, reused by the others
    for (int64_t m0 = 0; m0 < m; m0 += cap) {
        const int mc = (int)((m - m0 < cap) ? (m - m0) : cap);
        const int m_pad = (int)round_up(mc, kTile);
        const int nsplit = xgrad_splits(n, m_pad);  // (partial sums added on the host)
        // the members' raw rows side by side, normalised on the device with every member's own x_mean | x_std; the trend needs
        // the normalised coordinates on the host too (Linear / Quadratic; a model with xtypes: the cast ones, as the device's)
        const size_t blk = (size_t)mc * d;
        EGX_RC(d_xraw.alloc(blk * len));
        EGX_RC(d_xqT.alloc((size_t)d * m_pad * len));
        const double *src = xq[0] + (size_t)m0 * d;
        if (len > 1) {
            stage.resize(blk * len);
            for (int j = 0; j < len; j++) std::memcpy(&stage[blk * j], xq[j] + (size_t)m0 * d, sizeof(double) * blk);
            src = stage.data();
        }
        EGX_HIP_CHECK(hipMemcpyAsync(d_xraw.p, src, sizeof(double) * blk * len, hipMemcpyHostToDevice, w.stream));
        pb.sq = (int64_t)d * m_pad;
        EGX_RC(launch_normalize_queries(w.stream, pb, d_xraw.p, (int64_t)blk, mc, d, d_xqT.p, m_pad, m_pad));
        if (lead->mean >= 1) {
            xn.resize(blk * len);
            for (int j = 0; j < len; j++) {
                const egx_gp *gp = gps[j];
                const double *raw = xq[j] + (size_t)m0 * d;
                for (int a = 0; a < mc; a++)
                    for (int c = 0; c < d; c++)
                        xn[blk * j + (size_t)a * d + c] = (query_coord(gp, raw + (size_t)a * d, c) - gp->x_mean[c]) / gp->x_std[c];
            }
        } else {
            xn.clear();
        }
        const size_t out_sz = (size_t)nsplit * m_pad * d;
        pb.sout = (int64_t)out_sz;
        EGX_RC(d_out.alloc(out_sz * len));
        part.resize(out_sz * len);
        auto reduce_out = [&](int j, int a, int k) {
            double sacc = 0.0;
            for (int sidx = 0; sidx < nsplit; sidx++) sacc += part[out_sz * j + ((size_t)sidx * m_pad + a) * d + k];
            return sacc;
        };
        auto xn_row = [&](int j, int a) { return xn.empty() ? nullptr : &xn[blk * j + (size_t)a * d]; };
        if (gy) {
            EGX_RC(launch_xgrad(w.stream, lead->corr, pb, d_xqT.p, m_pad, m_pad, n_pad, n, d, lead->fit_hcols, nullptr, 0, 1, nsplit,
                                d_out.p));
            EGX_HIP_CHECK(hipMemcpyAsync(part.data(), d_out.p, sizeof(double) * out_sz * len, hipMemcpyDeviceToHost, w.stream));
            EGX_HIP_CHECK(hipStreamSynchronize(w.stream));
            for (int j = 0; j < len; j++) {
                const egx_gp *gp = gps[j];
                for (int a = 0; a < mc; a++) {
                    hm::regression_jac_dot(gp->mean, xn_row(j, a), d, gp->beta.data(), df.data());
                    for (int k = 0; k < d; k++)
                        gy[j][(size_t)(m0 + a) * d + k] = (df[k] + reduce_out(j, a, k)) * gp->y_std / gp->x_std[k];
                }
            }
        }
        if (gv) {
            const size_t nsl = (size_t)m_pad * p, nD = (size_t)m_pad * rp;
            sl.resize(nsl * len);
            EGX_RC(d_RT.alloc((size_t)m_pad * n_pad * len));
            EGX_RC(d_s0.alloc((size_t)m_pad * len));
            EGX_RC(d_sl.alloc(nsl * len));
            EGX_RC(d_Wt.alloc((size_t)n_pad * m_pad * len));
            EGX_RC(d_D.alloc(nD * len));
            EGX_RC(posterior_solve_run(gps, len, w.stream, d_xqT.p, m_pad, d_RT.p, d_s0.p, d_sl.p));
            EGX_HIP_CHECK(hipMemcpyAsync(sl.data(), d_sl.p, sizeof(double) * nsl * len, hipMemcpyDeviceToHost, w.stream));
            EGX_RC(posterior_weights_run(gps, len, w.stream, d_RT.p, m_pad, d_Wt.p));
            EGX_HIP_CHECK(hipStreamSynchronize(w.stream));
            // D = B^-1 A^T per query (p x p work on the host), uploaded negated and zero padded to rhs_pad columns
            dneg.assign(nD * len, 0.0);
            for (int j = 0; j < len; j++) {
                const egx_gp *gp = gps[j];
                for (int a = 0; a < mc; a++) {
                    hm::regression_row(gp->mean, xn_row(j, a), d, f.data());
                    for (int l = 0; l < p; l++) a_vec[l] = f[l] - sl[nsl * j + (size_t)a * p + l];
                    (void)hm::trend_forward(gp->ft_qr_r.data(), p, a_vec.data(), u.data());  // Rq^T u = A^T
                    hm::trend_backward(gp->ft_qr_r.data(), p, u.data(), dd.data());          // Rq D = u
                    for (int l = 0; l < p; l++) dneg[nD * j + (size_t)a * rp + l] = -dd[l];
                }
            }
            EGX_HIP_CHECK(hipMemcpyAsync(d_D.p, dneg.data(), sizeof(double) * dneg.size(), hipMemcpyHostToDevice, w.stream));
            EGX_RC(posterior_weights_trend_run(gps, len, w.stream, d_D.p, m_pad, d_Wt.p));
            pb.sW = (int64_t)n_pad * m_pad;
            EGX_RC(launch_xgrad(w.stream, lead->corr, pb, d_xqT.p, m_pad, m_pad, n_pad, n, d, lead->fit_hcols, d_Wt.p, m_pad, 0, nsplit,
                                d_out.p));
            EGX_HIP_CHECK(hipMemcpyAsync(part.data(), d_out.p, sizeof(double) * out_sz * len, hipMemcpyDeviceToHost, w.stream));
            EGX_HIP_CHECK(hipStreamSynchronize(w.stream));
            for (int j = 0; j < len; j++) {
                const egx_gp *gp = gps[j];
                for (int a = 0; a < mc; a++) {
                    for (int l = 0; l < p; l++) dd[l] = -dneg[nD * j + (size_t)a * rp + l];
                    hm::regression_jac_dot(gp->mean, xn_row(j, a), d, dd.data(), df.data());
                    for (int k = 0; k < d; k++)
                        gv[j][(size_t)(m0 + a) * d + k] = 2.0 * gp->sigma2 * (df[k] + reduce_out(j, a, k)) / gp->x_std[k];
                }
            }
        }
    }
    return EGX_SUCCESS;
}
}  // namespace egx

extern "C" {

int32_t egx_gp_predict(egx_gp *gp, const double *xq, int64_t m, double *y) {
    if (!gp || (m > 0 && !y)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return predict_impl(gp, xq, m, y, nullptr);
}
int32_t egx_gp_predict_var(egx_gp *gp, const double *xq, int64_t m, double *var) {
    if (!gp || (m > 0 && !var)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return predict_impl(gp, xq, m, nullptr, var);
}
int32_t egx_gp_predict_valvar(egx_gp *gp, const double *xq, int64_t m, double *y, double *var) {
    if (!gp || (m > 0 && (!y || !var))) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return predict_impl(gp, xq, m, y, var);
}

// Runs of fitted members of one group in consecutive slots (the runs of egx_gp_finalize_multi) answer in lock-step: one
// launch sequence per run and chunk.  A run is cut shorter where its (m_pad x n_pad) blocks would pass the 1 GiB that
// predict_impl allows one handle -- the chunks stay the lone call's, which is what keeps the bits the lone call's.
int32_t egx_gp_predict_valvar_multi(egx_gp *const *gps, int32_t k, const double *xq, int64_t m, double *y, double *var) {
    if (m < 0 || (m > 0 && (!xq || (!y && !var)))) {
        set_error(m > 0 && xq ? "NULL output: y and var" : "bad query array");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<std::unique_lock<std::shared_mutex>> locks;
    EGX_RC(lock_multi(gps, k, locks));
    for (int32_t j = 1; j < k; j++)
        if (gps[j]->d != gps[0]->d) {
            set_error("egx_gp_predict_valvar_multi: the models must have the same input dimension");
            return EGX_ERR_INVALID_VALUE;
        }
    const size_t d = (size_t)gps[0]->d;
    int first_rc = EGX_SUCCESS;
    for (int i = 0; i < k;) {
        egx_gp *g = gps[i];
        int rc = check_query(g, xq, m);
        int len = 1;
        if (rc == EGX_SUCCESS) rc = set_device(g);
        if (rc == EGX_SUCCESS && m > 0) {
            if (g->group && g->fit_hcols == 1) {
                len = run_len_multi(gps, k, i);
                for (int j = 1; j < len; j++)
                    if (!gps[i + j]->fitted || gps[i + j]->fit_hcols != 1 || gps[i + j]->mean != g->mean || gps[i + j]->n != g->n) len = j;
                len = predict_run_members(g->n_pad, m, var != nullptr, len);
                const double *xqs[kLockstepMax];
                double *ys[kLockstepMax], *vs[kLockstepMax];
                for (int j = 0; j < len; j++) {
                    xqs[j] = xq + (size_t)(i + j) * m * d;
                    ys[j] = y ? y + (size_t)(i + j) * m : nullptr;
                    vs[j] = var ? var + (size_t)(i + j) * m : nullptr;
                }
                rc = predict_run(gps + i, len, xqs, m, y ? ys : nullptr, var ? vs : nullptr);
            } else {
                rc = predict_impl(g, xq + (size_t)i * m * d, m, y ? y + (size_t)i * m : nullptr, var ? var + (size_t)i * m : nullptr);
            }
        }
        if (rc != EGX_SUCCESS && first_rc == EGX_SUCCESS) first_rc = rc;  // (the others still finish)
        i += len;
    }
    return first_rc;
}

// The x-gradients of the same runs in lock-step (xgrad_run); the run rule, the byte bound and the chunks are those of
// egx_gp_predict_valvar_multi.  m <= 8: a lone call may take its few-query route, a run never does.
int32_t egx_gp_predict_valvar_gradients_multi(egx_gp *const *gps, int32_t k, const double *xq, int64_t m, double *grad_y,
                                              double *grad_var) {
    if (m < 0 || (m > 0 && (!xq || (!grad_y && !grad_var)))) {
        set_error(m > 0 && xq ? "NULL output: grad_y and grad_var" : "bad query array");
        return EGX_ERR_INVALID_VALUE;
    }
    std::vector<std::unique_lock<std::shared_mutex>> locks;
    EGX_RC(lock_multi(gps, k, locks));
    for (int32_t j = 1; j < k; j++)
        if (gps[j]->d != gps[0]->d) {
            set_error("egx_gp_predict_valvar_gradients_multi: the models must have the same input dimension");
            return EGX_ERR_INVALID_VALUE;
        }
    const size_t d = (size_t)gps[0]->d;
    int first_rc = EGX_SUCCESS;
    for (int i = 0; i < k;) {
        egx_gp *g = gps[i];
        int rc = check_query(g, xq, m);
        int len = 1;
        if (rc == EGX_SUCCESS) rc = set_device(g);
        if (rc == EGX_SUCCESS && m > 0) {
            const size_t blk = (size_t)m * d;
            if (g->group && g->fit_hcols == 1) {
                len = run_len_multi(gps, k, i);
                for (int j = 1; j < len; j++)
                    if (!gps[i + j]->fitted || gps[i + j]->fit_hcols != 1 || gps[i + j]->mean != g->mean || gps[i + j]->n != g->n) len = j;
                len = predict_run_members(g->n_pad, m, grad_var != nullptr, len);
                const double *xqs[kLockstepMax];
                double *gys[kLockstepMax], *gvs[kLockstepMax];
                for (int j = 0; j < len; j++) {
                    xqs[j] = xq + (size_t)(i + j) * blk;
                    gys[j] = grad_y ? grad_y + (size_t)(i + j) * blk : nullptr;
                    gvs[j] = grad_var ? grad_var + (size_t)(i + j) * blk : nullptr;
                }
                rc = xgrad_run(gps + i, len, xqs, m, grad_y ? gys : nullptr, grad_var ? gvs : nullptr);
            } else {
                rc = xgrad_impl(g, xq + (size_t)i * blk, m, grad_y ? grad_y + (size_t)i * blk : nullptr,
                                grad_var ? grad_var + (size_t)i * blk : nullptr);
            }
        }
        if (rc != EGX_SUCCESS && first_rc == EGX_SUCCESS) first_rc = rc;  // (the others still finish)
        i += len;
    }
    return first_rc;
}

int32_t egx_gp_predict_gradients(egx_gp *gp, const double *x, int64_t m, double *grad) {
    if (!gp || (m > 0 && !grad)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return xgrad_impl(gp, x, m, grad, nullptr);
}

int32_t egx_gp_predict_var_gradients(egx_gp *gp, const double *x, int64_t m, double *grad) {
    if (!gp || (m > 0 && !grad)) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return xgrad_impl(gp, x, m, nullptr, grad);
}

int32_t egx_gp_predict_valvar_gradients(egx_gp *gp, const double *x, int64_t m, double *grad_y, double *grad_var) {
    if (!gp || (m > 0 && (!grad_y || !grad_var))) {
        set_error("NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    return xgrad_impl(gp, x, m, grad_y, grad_var);
}
}  // extern "C"
