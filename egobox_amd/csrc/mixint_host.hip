// Mixed-integer design spaces at the C ABI (XType, crates/ego/src/types.rs; MixintContext and the free functions of
// crates/ego/src/gpmix/mixint.rs:38-226): validation of a spec, the six host helpers -- no device needed, the arithmetic is
// mixint.h's -- and the spec of a GP handle, whose queries are then cast on the device by the kernels that read them.
#include "gp_handle.h"

using namespace egx;

namespace egx {

int mixspec_build(const char *who, const egx_xtype *xt, int32_t nx, int64_t d_expect, MixSpec &out) {
    const std::string w(who);
    out = MixSpec();
    if (nx < 1 || !xt) {
        set_error(w + ": need nx >= 1 xtypes");
        return EGX_ERR_INVALID_VALUE;
    }
    int64_t d = 0, nvals = 0;
    for (int32_t j = 0; j < nx; j++) {
        const egx_xtype &t = xt[j];
        const std::string e = w + ": xtype " + std::to_string(j);
        switch (t.kind) {
            case EGX_XTYPE_FLOAT:
            case EGX_XTYPE_INT:
                if (std::isnan(t.lo) || std::isnan(t.hi) || t.lo > t.hi) {
                    set_error(e + ": bounds lo > hi (or NaN)");
                    return EGX_ERR_INVALID_VALUE;
                }
                d += 1;
                break;
            case EGX_XTYPE_ORD:
                if (t.n < 1 || !t.values) {
                    set_error(e + ": Ord needs n >= 1 values");
                    return EGX_ERR_INVALID_VALUE;
                }
                for (int32_t i = 0; i < t.n; i++)
                    if (!std::isfinite(t.values[i])) {
                        set_error(e + ": Ord value " + std::to_string(i) + " is not finite");
                        return EGX_ERR_INVALID_VALUE;
                    }
                d += 1, nvals += t.n;
                break;
            case EGX_XTYPE_ENUM:
                if (t.n < 1) {
                    set_error(e + ": Enum needs n >= 1 levels");
                    return EGX_ERR_INVALID_VALUE;
                }
                d += t.n;
                break;
            default:
                set_error(e + ": unknown kind " + std::to_string(t.kind));
                return EGX_ERR_INVALID_VALUE;
        }
        if (d > (int64_t)1 << 24) {
            set_error(e + ": unfolded dimension beyond 2^24");
            return EGX_ERR_UNSUPPORTED;
        }
    }
    if (d_expect >= 0 && d != d_expect) {
        set_error(w + ": the xtypes unfold to " + std::to_string(d) + " columns, expected " + std::to_string(d_expect));
        return EGX_ERR_INVALID_VALUE;
    }
    if (nvals > EGX_MIXINT_MAX_ORD_VALUES) {
        set_error(w + ": " + std::to_string(nvals) + " Ord values in all, more than EGX_MIXINT_MAX_ORD_VALUES");
        return EGX_ERR_UNSUPPORTED;
    }
    out.xt.assign(xt, xt + nx);
    out.cols.reserve((size_t)d);
    for (int32_t j = 0; j < nx; j++) {
        egx_xtype &t = out.xt[j];
        const int32_t u = (int32_t)out.cols.size();
        if (t.kind == EGX_XTYPE_ENUM) {
            for (int32_t l = 0; l < t.n; l++) out.cols.push_back({mixint::kEnum, u, t.n, 0});
        } else if (t.kind == EGX_XTYPE_ORD) {
            out.cols.push_back({mixint::kOrd, u, t.n, (int32_t)out.vals.size()});
            out.vals.insert(out.vals.end(), t.values, t.values + t.n);
        } else {
            out.cols.push_back({t.kind == EGX_XTYPE_INT ? mixint::kInt : mixint::kFloat, u, 1, 0});
        }
        t.values = nullptr;  // (borrowed during the call only: the copy is in vals)
        if (t.kind != EGX_XTYPE_ORD && t.kind != EGX_XTYPE_ENUM) t.n = 0;
    }
    return EGX_SUCCESS;
}

}  // namespace egx

namespace {

// the common head of the row helpers: the spec, and m rows in / out
int rows_head(const char *who, const egx_xtype *xt, int32_t nx, const double *x, int64_t m, double *out, MixSpec &sp) {
    EGX_RC(mixspec_build(who, xt, nx, -1, sp));
    if (m < 0 || (m > 0 && (!x || !out))) {
        set_error(std::string(who) + ": bad array");
        return EGX_ERR_INVALID_VALUE;
    }
    return EGX_SUCCESS;
}

}  // namespace

extern "C" {

int32_t egx_mixint_unfolded_dim(const egx_xtype *xt, int32_t nx, int64_t *d) {
    MixSpec sp;
    EGX_RC(mixspec_build("egx_mixint_unfolded_dim", xt, nx, -1, sp));
    if (d) *d = (int64_t)sp.cols.size();
    return EGX_SUCCESS;
}

int32_t egx_mixint_continuous_limits(const egx_xtype *xt, int32_t nx, double *xlimits) {
    MixSpec sp;
    EGX_RC(mixspec_build("egx_mixint_continuous_limits", xt, nx, -1, sp));
    if (!xlimits) {
        set_error("egx_mixint_continuous_limits: NULL output");
        return EGX_ERR_INVALID_VALUE;
    }
    size_t u = 0;
    for (int32_t j = 0; j < nx; j++) {  // mixint.rs:38-67
        const egx_xtype &t = xt[j];
        if (t.kind == EGX_XTYPE_ENUM) {
            for (int32_t l = 0; l < t.n; l++, u++) xlimits[2 * u] = 0.0, xlimits[2 * u + 1] = 1.0;
        } else if (t.kind == EGX_XTYPE_ORD) {
            double lo = t.values[0], hi = t.values[0];
            for (int32_t i = 1; i < t.n; i++) lo = std::min(lo, t.values[i]), hi = std::max(hi, t.values[i]);
            xlimits[2 * u] = lo, xlimits[2 * u + 1] = hi, u++;
        } else {
            xlimits[2 * u] = t.lo, xlimits[2 * u + 1] = t.hi, u++;
        }
    }
    return EGX_SUCCESS;
}

int32_t egx_mixint_unfold(const egx_xtype *xt, int32_t nx, const double *x, int64_t m, double *out) {
    MixSpec sp;
    EGX_RC(rows_head("egx_mixint_unfold", xt, nx, x, m, out, sp));
    const int d = (int)sp.cols.size();
    for (int64_t a = 0; a < m; a++) {
        const int bad = mixint::unfold_row(sp.cols.data(), d, x + a * nx, out + a * d);
        if (bad >= 0) {
            set_error("egx_mixint_unfold: row " + std::to_string(a) + ", xtype " + std::to_string(bad) + ": enum index outside [0, " +
                      std::to_string(xt[bad].n) + ") or not finite");
            return EGX_ERR_INVALID_VALUE;
        }
    }
    return EGX_SUCCESS;
}

int32_t egx_mixint_fold(const egx_xtype *xt, int32_t nx, const double *x, int64_t m, double *out) {
    MixSpec sp;
    EGX_RC(rows_head("egx_mixint_fold", xt, nx, x, m, out, sp));
    const int d = (int)sp.cols.size();
    for (int64_t a = 0; a < m; a++) mixint::fold_row(sp.cols.data(), d, x + a * d, out + a * nx);
    return EGX_SUCCESS;
}

int32_t egx_mixint_cast(const egx_xtype *xt, int32_t nx, const double *x, int64_t m, double *out) {
    MixSpec sp;
    EGX_RC(rows_head("egx_mixint_cast", xt, nx, x, m, out, sp));
    const int d = (int)sp.cols.size();
    std::vector<double> row((size_t)d);  // (out may be x)
    for (int64_t a = 0; a < m; a++) {
        mixint::cast_row(sp.cols.data(), sp.vals.data(), d, x + a * d, row.data());
        std::memcpy(out + a * d, row.data(), sizeof(double) * d);
    }
    return EGX_SUCCESS;
}

int32_t egx_mixint_to_discrete(const egx_xtype *xt, int32_t nx, const double *x, int64_t m, double *out) {
    MixSpec sp;
    EGX_RC(rows_head("egx_mixint_to_discrete", xt, nx, x, m, out, sp));
    const int d = (int)sp.cols.size();
    std::vector<double> row((size_t)d);
    for (int64_t a = 0; a < m; a++) {  // mixint.rs:220-226
        mixint::cast_row(sp.cols.data(), sp.vals.data(), d, x + a * d, row.data());
        mixint::fold_row(sp.cols.data(), d, row.data(), out + a * nx);
    }
    return EGX_SUCCESS;
}

int32_t egx_gp_set_xtypes(egx_gp *gp, const egx_xtype *xt, int32_t nx) {
    if (!gp) {
        set_error("NULL handle");
        return EGX_ERR_INVALID_VALUE;
    }
    MixSpec sp;
    if (nx != 0) EGX_RC(mixspec_build("egx_gp_set_xtypes", xt, nx, gp->d, sp));  // before the device is touched
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    if (nx == 0) {
        gp->xspec = MixSpec();
        return EGX_SUCCESS;
    }
    EGX_RC(set_device(gp));
    const std::vector<double> tab = sp.table();
    EGX_RC(gp->d_xspec.alloc(tab.size()));
    hipStream_t st = gp->ws[0].stream;
    EGX_HIP_CHECK(hipStreamSynchronize(st));  // nothing in flight reads the table that is about to change
    EGX_HIP_CHECK(hipMemcpyAsync(gp->d_xspec.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st));
    EGX_HIP_CHECK(hipStreamSynchronize(st));  // tab is a local
    gp->xspec = std::move(sp);
    return EGX_SUCCESS;
}

int32_t egx_gp_get_xtypes(egx_gp *gp, egx_xtype *xt, int32_t cap, int32_t *nx, double *ord_values, int64_t *n_ord_values) {
    if (!gp || cap < 0 || (cap > 0 && !xt)) {
        set_error("egx_gp_get_xtypes: NULL handle or bad capacity");
        return EGX_ERR_INVALID_VALUE;
    }
    std::unique_lock<std::shared_mutex> lock(gp->mu);
    const MixSpec &sp = gp->xspec;
    if (nx) *nx = (int32_t)sp.xt.size();
    if (n_ord_values) *n_ord_values = (int64_t)sp.vals.size();
    if (ord_values && !sp.vals.empty()) std::memcpy(ord_values, sp.vals.data(), sizeof(double) * sp.vals.size());
    size_t off = 0;
    for (size_t j = 0; j < sp.xt.size(); j++) {
        const bool ord = sp.xt[j].kind == EGX_XTYPE_ORD;
        if ((int64_t)j < cap) {
            xt[j] = sp.xt[j];
            xt[j].values = ord && ord_values ? ord_values + off : nullptr;
        }
        if (ord) off += (size_t)sp.xt[j].n;
    }
    return EGX_SUCCESS;
}

}  // extern "C"
