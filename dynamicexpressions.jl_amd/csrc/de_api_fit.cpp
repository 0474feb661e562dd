// de_api_fit.cpp — C ABI (include/de_hip.h): what CONSUMES the gradients and matrices de_api_grad.cpp produces.  de_gn_lm_step /
// de_fit_stats_lm_step (and _wide): one Levenberg-Marquardt step per tree (kernels de_lm.hip, de_gn_wide.hip, de_lm_scaled.hip,
// de_lm_scaled_wide.hip); de_fit_consts_lm(_ex, _wide), de_fit_consts_lm_scaled(_wide) and
// de_fit_consts_bfgs (kernels de_bfgs.hip, §4.4.10), de_fit_consts_lbfgs (kernels de_lbfgs.hip, §4.4.15), de_fit_consts_nm (kernels de_nm.hip, §4.4.13) and the scaled forms of those two
// (de_fit_consts_bfgs_scaled / de_fit_consts_nm_scaled, adapter kernel de_fit_scaled.hip, §4.4.14): fits on the constants that are
// ONE driver — fit_check, stage_fit_inputs, a Workspace in sLm, run_fit, FitOutputs — around their own evaluation and kernels; the _tied forms
// of four of them (de_fit_consts_{bfgs,lbfgs,nm,lm}_tied, §4.4.16: a shared GraphNode constant as one unknown; kernels de_ties.hip, arithmetic
// de_ties.h), which are the same functions with a TiedState; and the host hooks that run the kernels' arithmetic.
#include "de_api_internal.h"
#include "de_lm.h"
#include "de_lm_solve.h"
#include "de_gn_wide.h"
#include "de_lm_solve_wide.h"
#include "de_lm_scaled.h"
#include "de_lm_project.h"
#include "de_lm_project_wide.h"
#include "de_bfgs.h"
#include "de_bfgs_dev.h"
#include "de_lbfgs.h"
#include "de_lbfgs_dev.h"
#include "de_nm.h"
#include "de_nm_dev.h"
#include "de_fit_scaled.h"
#include "de_fit_scaled_dev.h"
#include "de_ties.h"
#include "de_ties_dev.h"

// the tie hooks (de_ties.h): one tree's map on host buffers of the element type.  Each returns U, or -1 with nothing written
template <class Body>
static int ties_hook(int32_t n_slots, const int32_t *tie, const Body &body) {
    const int64_t U = ties_unknowns(n_slots, tie);
    if (U < 0) return -1;
    std::vector<int64_t> off((size_t)U + 1), list((size_t)n_slots);
    ties_csr(n_slots, tie, U, 0, off.data(), list.data());
    body(U, off.data(), list.data());
    return (int)U;
}
static bool ties_hook_args(int dtype, int32_t n_slots, const int32_t *tie, const void *in, const void *out) {
    return (dtype == DE_F32 || dtype == DE_F64) && n_slots >= 0 && tie && in && out;
}
template <typename T>
static int ties_pack_t(int32_t n, const int32_t *tie, const void *slots, void *unique) {
    return ties_hook(n, tie, [&](int64_t U, const int64_t *off, const int64_t *list) {
        for (int64_t u = 0; u < U; u++) std::memcpy(static_cast<T *>(unique) + u, static_cast<const T *>(slots) + list[off[u]], sizeof(T));
    });
}
template <typename T>
static int ties_unpack_t(int32_t n, const int32_t *tie, const void *unique, void *slots) {
    return ties_hook(n, tie, [&](int64_t, const int64_t *, const int64_t *) {
        for (int32_t s = 0; s < n; s++) std::memcpy(static_cast<T *>(slots) + s, static_cast<const T *>(unique) + tie[s], sizeof(T));
    });
}
template <typename T>
static int ties_fold_t(int32_t n, const int32_t *tie, const void *g, void *gu) {
    return ties_hook(n, tie, [&](int64_t U, const int64_t *off, const int64_t *list) {
        for (int64_t u = 0; u < U; u++) static_cast<T *>(gu)[u] = ties_fold<T>(static_cast<const T *>(g), list + off[u], off[u + 1] - off[u]);
    });
}
template <typename T>
static int ties_fold_matrix_t(int32_t n, const int32_t *tie, const void *H, void *Hu) {
    return ties_hook(n, tie, [&](int64_t U, const int64_t *off, const int64_t *list) {
        for (int64_t v = 0; v < U; v++)
            for (int64_t u = 0; u < U; u++)
                static_cast<T *>(Hu)[u + U * v] = ties_fold_matrix<T>(static_cast<const T *>(H), n, 0, list + off[u], off[u + 1] - off[u],
                                                                      list + off[v], off[v + 1] - off[v]);
    });
}

extern "C" {
// ---- the host hooks: the arithmetic of the step, projection and BFGS kernels on host buffers (de_lm_solve.h, de_lm_solve_wide.h,
// de_lm_project.h, de_lm_project_wide.h, de_bfgs.h, de_lbfgs.h) -----------------------------------------------------------------------------------------
int de_lm_solve_host(int G, const double *H, const double *g, double lam, double *step) {
    double x[LM_MAX_ROWS];
    const bool args = G <= 0 || (H && g);
    const int solved = args ? lm_solve8<double>(G, H, g, lam, x) : 0;
    if (step)
        for (int k = 0; k < G; k++) step[k] = solved && k < LM_MAX_ROWS ? x[k] : 0.0;
    return solved;
}
int de_lm_solve_host_wide(int G, const double *H, const double *g, double lam, double *step) {
    if (G <= LM_MAX_ROWS) return de_lm_solve_host(G, H, g, lam, step); // (lm_solve8 itself: the same bits by construction)
    double x[LM_WIDE_MAX_ROWS], work[LMW_WORK];
    const int solved = G <= LM_WIDE_MAX_ROWS && H && g ? lm_solve_wide<double>(G, H, g, lam, x, work) : 0;
    if (step)
        for (int k = 0; k < G; k++) step[k] = solved ? x[k] : 0.0;
    return solved;
}
int de_lm_project_host(int G, const double *stats, const double *ystats, const double *dmom, const double *H, double *sse, double *g, double *Ht) {
    if (stats && ystats && sse) *sse = lm_scaled_sse(stats[1], stats[2], ystats[0], ystats[2]);
    int formed = 0;
    if (stats && ystats && dmom && H && g && Ht && G >= 1 && G <= LM_MAX_ROWS) {
        DE_LM_FOR_G(G, formed = lm_project_mem<GG>(stats, ystats, dmom, H, g, Ht));
        return formed;
    }
    for (int k = 0; g && k < G; k++) g[k] = 0.0;
    for (int64_t k = 0; Ht && k < (int64_t)G * G; k++) Ht[k] = 0.0;
    return 0;
}
int de_lm_project_host_wide(int G, const double *stats, const double *ystats, const double *dmom, const double *H, double *sse, double *g, double *Ht) {
    if (G >= 0 && G <= LM_MAX_ROWS) return de_lm_project_host(G, stats, ystats, dmom, H, sse, g, Ht); // (lm_project itself: the same bits by construction)
    if (stats && ystats && sse) *sse = lm_scaled_sse(stats[1], stats[2], ystats[0], ystats[2]);
    if (G < 0) return 0; // (nothing else is written)
    if (stats && ystats && dmom && H && g && Ht && G <= LM_WIDE_MAX_ROWS) return lm_project_wide(G, stats, ystats, dmom, H, g, Ht);
    for (int k = 0; g && k < G; k++) g[k] = 0.0;
    for (int64_t k = 0; Ht && k < (int64_t)G * G; k++) Ht[k] = 0.0;
    return 0;
}
int de_bfgs_max_rows(void) { return BFGS_MAX_ROWS; }
int de_bfgs_direction_host(int G, double *B, uint8_t *fresh, double *alpha, const double *g, double step0, double *p, double *slope) {
    const bool args = B && fresh && alpha && g && p && slope;
    if (args && G >= 1 && G <= BFGS_MAX_ROWS) return bfgs_direction(G, B, fresh, alpha, g, step0, p, slope);
    for (int k = 0; p && k < G; k++) p[k] = 0.0;
    return 0;
}
int de_bfgs_update_host(int G, double *B, uint8_t *fresh, const double *s, const double *yv, double curv) {
    if (!B || !fresh || !s || !yv) return 0;
    return bfgs_update(G, B, fresh, s, yv, curv);
}
int de_lbfgs_max_rows(void) { return LBFGS_MAX_ROWS; }
int de_lbfgs_max_memory(void) { return LBFGS_MAX_MEMORY; }
static bool lbfgs_hook_args(int G, int memory, const int32_t *count, const int32_t *head) {
    return G >= 1 && G <= LBFGS_MAX_ROWS && memory >= 1 && memory <= LBFGS_MAX_MEMORY && count && head && *count >= 0 && *count <= memory &&
           *head >= 0 && *head < memory;
}
int de_lbfgs_direction_host(int G, int memory, const double *S, const double *Y, const double *rho, int32_t *count, int32_t *head,
                            double *alpha, const double *g, double step0, double *p, double *slope) {
    if (!S || !Y || !rho || !alpha || !g || !p || !slope || !lbfgs_hook_args(G, memory, count, head)) return 0; // (nothing is written)
    LbfgsHostTeam tm;
    const LbfgsDir r = lbfgs_direction(tm, G, memory, S, Y, rho, *count, *head, *alpha, g, step0, p);
    *count = r.count;
    *alpha = r.alpha;
    *slope = r.slope;
    return r.produced;
}
int de_lbfgs_update_host(int G, int memory, double *S, double *Y, double *rho, int32_t *count, int32_t *head, const double *s,
                         const double *yv, double curv) {
    if (!S || !Y || !rho || !s || !yv || !lbfgs_hook_args(G, memory, count, head)) return 0;
    LbfgsHostTeam tm;
    return lbfgs_update(tm, G, memory, S, Y, rho, count, head, s, yv, curv);
}
int de_scaled_objective_host(int G, const double *stats, const double *ystats, const double *dmom, double *sse, double *g) {
    if (stats && ystats && sse) *sse = lm_scaled_sse(stats[1], stats[2], ystats[0], ystats[2]);
    if (stats && ystats && dmom && g && G >= 1 && G <= FIT_SCALED_MAX_ROWS) {
        double e;
        return fit_scaled_objective(G, stats, ystats, dmom, &e, g);
    }
    for (int k = 0; g && k < G; k++) g[k] = 0.0;
    return 0;
}
int de_nm_max_rows(void) { return NM_MAX_ROWS; }
static bool nm_hook_args(int G, int dtype, const int32_t *st) {
    return G >= 1 && G <= NM_MAX_ROWS && (dtype == DE_F32 || dtype == DE_F64) && st && st[0] >= NM_BUILD && st[0] <= NM_DONE &&
           (st[0] == NM_REFLECT || st[0] == NM_DONE || (st[1] >= 0 && st[1] <= G && st[2] >= 0 && st[2] <= G));
}
int de_nm_ask_host(int G, int dtype, const de_nm_opts_t *opts, double *V, const double *f, int32_t *st, double *c, double *xr, void *trial) {
    if (!V || !f || !c || !xr || !trial || !nm_hook_args(G, dtype, st)) return 0;
    const double a = opts ? opts->a : 0.025, b = opts ? opts->b : 0.5, f_tol = opts ? opts->f_tol : 0.0;
    if (dtype == DE_F32) nm_ask_tree<float>(G, 0, G, true, a, b, f_tol, V, f, st, c, xr, static_cast<float *>(trial));
    else nm_ask_tree<double>(G, 0, G, true, a, b, f_tol, V, f, st, c, xr, static_cast<double *>(trial));
    return 1;
}
int de_nm_tell_host(int G, int dtype, double *V, double *f, int32_t *st, const double *c, const double *xr, double *fr, double f_trial,
                    int ok_trial) {
    if (!V || !f || !c || !xr || !fr || !nm_hook_args(G, dtype, st)) return 0;
    const double F = nm_loss(f_trial, ok_trial != 0);
    if (dtype == DE_F32) nm_tell_tree<float>(G, 0, G, true, V, f, st, c, xr, fr, F);
    else nm_tell_tree<double>(G, 0, G, true, V, f, st, c, xr, fr, F);
    return 1;
}
#define DE_TIES_HOOK(NAME, BODY)                                                                         \
    int NAME(int dtype, int32_t n_slots, const int32_t *tie, const void *in, void *out) {                \
        if (!ties_hook_args(dtype, n_slots, tie, in, out)) return -1;                                    \
        try { return dtype == DE_F32 ? BODY<float>(n_slots, tie, in, out) : BODY<double>(n_slots, tie, in, out); }      \
        catch (...) { return -1; }                                                                       \
    }
DE_TIES_HOOK(de_ties_pack_host, ties_pack_t)
DE_TIES_HOOK(de_ties_unpack_host, ties_unpack_t)
DE_TIES_HOOK(de_ties_fold_host, ties_fold_t)
DE_TIES_HOOK(de_ties_fold_matrix_host, ties_fold_matrix_t)
#undef DE_TIES_HOOK

// what the fits refuse about their options: null = good, else the reason
const char *bfgs_opts_problem(const de_bfgs_opts_t *o) {
    if (o->reserved != 0) return "de_bfgs_opts_t: reserved must be 0";
    if (o->iters < 0) return "de_bfgs_opts_t: iters < 0";
    for (const double v : {o->step0, o->c1, o->curv})
        if (!(std::isfinite(v) && v > 0.0)) return "de_bfgs_opts_t: step0, c1 and curv must be finite and positive";
    if (!(o->shrink > 0.0 && o->shrink < 1.0)) return "de_bfgs_opts_t: shrink must lie in (0, 1)";
    return nullptr;
}
// de_lbfgs_opts_t: bfgs_opts_problem's refusals of the fields they share, and of its own two; *o: the shared fields
const char *lbfgs_opts_problem(const de_lbfgs_opts_t *l, de_bfgs_opts_t *o) {
    *o = de_bfgs_opts_t{l->iters, l->reserved, l->step0, l->shrink, l->c1, l->curv};
    if (l->reserved != 0 || l->reserved2 != 0) return "de_lbfgs_opts_t: reserved and reserved2 must be 0";
    if (l->memory < 1 || l->memory > LBFGS_MAX_MEMORY) return "de_lbfgs_opts_t: memory must lie in 1 .. de_lbfgs_max_memory()";
    if (l->iters < 0) return "de_lbfgs_opts_t: iters < 0";
    for (const double v : {l->step0, l->c1, l->curv})
        if (!(std::isfinite(v) && v > 0.0)) return "de_lbfgs_opts_t: step0, c1 and curv must be finite and positive";
    if (!(l->shrink > 0.0 && l->shrink < 1.0)) return "de_lbfgs_opts_t: shrink must lie in (0, 1)";
    return nullptr;
}
static const char *nm_opts_problem(const de_nm_opts_t *o) {
    if (o->reserved != 0) return "de_nm_opts_t: reserved must be 0";
    if (o->iters < 0) return "de_nm_opts_t: iters < 0";
    if (!(std::isfinite(o->a) && std::isfinite(o->b)) || (o->a == 0.0 && o->b == 0.0)) return "de_nm_opts_t: a and b must be finite and not both 0";
    if (!(std::isfinite(o->f_tol) && o->f_tol >= 0.0)) return "de_nm_opts_t: f_tol must be finite and not negative";
    return nullptr;
}
static const char *lm_opts_problem(const de_lm_opts_t *o) {
    if (o->reserved != 0) return "de_lm_opts_t: reserved must be 0";
    if (o->iters < 0) return "de_lm_opts_t: iters < 0";
    for (const double v : {o->lam0, o->up, o->down, o->lam_min})
        if (!(std::isfinite(v) && v > 0.0)) return "de_lm_opts_t: lam0, up, down and lam_min must be finite and positive";
    return nullptr;
}

// ---- the geometry tables -------------------------------------------------------------------------------------------------
// The geometry tables of a step / fit on the device: [dloss offsets | jtj offsets | widths].  Uploaded only when they differ from what the
// device holds, through a pinned image: a call whose buffers are device pointers is stream-ordered and never waits for the stream.
// rows_per_g = 3 (de_fit_stats_lm_step / de_fit_consts_lm_scaled: the offsets are those of dmom, 3 G doubles per tree): the image is
// [dmom offsets | jtj offsets | packed offsets of G entries per tree | widths], soff the third table (else soff = doff).
struct LmTables {
    const int64_t *doff = nullptr, *joff = nullptr, *soff = nullptr;
    const int32_t *ng = nullptr;
    int64_t span = 0, jspan = 0, sspan = 0;
};
// extra (may be null): a table of the caller's own behind them, 8-byte aligned — the tie tables of a tied fit; *extra_dev: where it lies.
static int lm_tables(de_ctx *c, int64_t n, const int32_t *ng, const int64_t *doffs, const int64_t *joffs, LmTables *out, int rows_per_g = 1,
                     const std::vector<unsigned char> *extra = nullptr, const unsigned char **extra_dev = nullptr) {
    const size_t nn = (size_t)n, n_off = rows_per_g > 1 ? 3 : 2;
    const size_t own = nn * (n_off * sizeof(int64_t) + sizeof(int32_t)), extra_at = (own + 7) & ~(size_t)7;
    std::vector<unsigned char> img(extra ? extra_at + extra->size() : own);
    if (extra && !extra->empty()) std::memcpy(img.data() + extra_at, extra->data(), extra->size());
    int64_t *doff = reinterpret_cast<int64_t *>(img.data()), *joff = doff + nn, *soff = n_off > 2 ? joff + nn : nullptr;
    int32_t *w = reinterpret_cast<int32_t *>(doff + n_off * nn);
    int64_t run = 0, jrun = 0, span = 0, jspan = 0, srun = 0;
    for (size_t t = 0; t < nn; t++) {
        const int64_t g = ng[t];
        if (g < 0) return fail(c, DE_ERR_INVALID_ARG, "negative n_grad");
        doff[t] = doffs ? doffs[t] : run;
        joff[t] = joffs ? joffs[t] : jrun;
        if (doff[t] < 0 || joff[t] < 0) return fail(c, DE_ERR_INVALID_ARG, "negative offset");
        if (soff) soff[t] = srun;
        w[t] = (int32_t)g;
        run += rows_per_g * g;
        srun += g;
        jrun += g * g;
        span = std::max(span, doff[t] + rows_per_g * g);
        jspan = std::max(jspan, joff[t] + g * g);
    }
    if (img != c->lm_tab || !c->sLmTab.p) {
        if (c->lm_ev) HIP_TRY(c, hipEventSynchronize(c->lm_ev)); // (the previous upload reads the pinned image)
        else HIP_TRY(c, hipEventCreateWithFlags(&c->lm_ev, hipEventDisableTiming));
        if (c->lm_pin_cap < img.size()) {
            if (c->lm_pin) (void)hipHostFree(c->lm_pin);
            c->lm_pin = nullptr;
            c->lm_pin_cap = 0;
            HIP_TRY(c, hipHostMalloc(&c->lm_pin, img.size(), hipHostMallocDefault));
            c->lm_pin_cap = img.size();
        }
        c->lm_tab.clear();
        if (c->sLmTab.cap < img.size()) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (growing frees the tables queued work may read)
        HIP_TRY(c, c->sLmTab.reserve(img.size()));
        std::memcpy(c->lm_pin, img.data(), img.size());
        HIP_TRY(c, hipMemcpyAsync(c->sLmTab.p, c->lm_pin, img.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->lm_ev, c->stream));
        c->lm_tab = std::move(img);
    }
    out->doff = static_cast<const int64_t *>(c->sLmTab.p);
    out->joff = out->doff + nn;
    out->soff = n_off > 2 ? out->joff + nn : out->doff;
    out->ng = reinterpret_cast<const int32_t *>(out->doff + n_off * nn);
    out->span = span;
    out->jspan = jspan;
    out->sspan = srun;
    if (extra_dev) *extra_dev = static_cast<const unsigned char *>(c->sLmTab.p) + extra_at;
    return DE_OK;
}

// ---- the tie tables ------------------------------------------------------------------------------------------------------
// A tied fit's view of the program: U_t unknowns per tree (what the optimiser kernels take for n_grad) and the device tables of TieArgs as
// one image of int64 words [slot_unk | unk_off | unk_slots | slot_off | unk_tree_off | hoff], uploaded behind the geometry tables.
struct TiePlan {
    std::vector<int32_t> ng;
    std::vector<unsigned char> blob;
    int64_t nu = 0, hspan = 0; // the unknowns of the population; the elements of its packed S x S occurrence blocks
    size_t nc = 0, nt = 0;
    void bind(const unsigned char *dev, const int64_t *huoff, int32_t max_slots, TieArgs *a) const {
        const int64_t *w = reinterpret_cast<const int64_t *>(dev);
        a->n_trees = (int64_t)nt; a->n_slots = (int64_t)nc; a->n_unknowns = nu;
        a->slot_unk = w;
        a->unk_off = a->slot_unk + nc;
        a->unk_slots = a->unk_off + nu + 1;
        a->slot_off = a->unk_slots + nc;
        a->unk_tree_off = a->slot_off + nt + 1;
        a->hoff = a->unk_tree_off + nt + 1;
        a->huoff = huoff;
        a->max_slots = max_slots;
    }
};
// tie: host, one id per constant slot in de_program_set_consts order.  Refused: a negative id, or an id out of first-occurrence order.
static int tie_plan(de_ctx *c, const de_program *p, const char *what, const int32_t *tie, TiePlan *pl) {
    const size_t nt = (size_t)p->n_trees, nc = (size_t)p->const_off[nt];
    pl->nt = nt;
    pl->nc = nc;
    pl->ng.resize(nt);
    int64_t nu = 0;
    for (size_t t = 0; t < nt; t++) {
        const int64_t S = p->const_off[t + 1] - p->const_off[t], U = ties_unknowns(S, tie + p->const_off[t]);
        if (U < 0)
            return fail(c, DE_ERR_INVALID_ARG, "%s: tree %lld: the tie map has a negative id or is not in first-occurrence order", what, (long long)t);
        pl->ng[t] = (int32_t)U;
        nu += U;
    }
    pl->nu = nu;
    pl->blob.assign((2 * nc + (size_t)nu + 1 + 3 * nt + 2) * sizeof(int64_t), 0);
    int64_t *slot_unk = reinterpret_cast<int64_t *>(pl->blob.data()), *unk_off = slot_unk + nc, *unk_slots = unk_off + nu + 1,
            *slot_off = unk_slots + nc, *unk_tree_off = slot_off + nt + 1, *hoff = unk_tree_off + nt + 1;
    int64_t u0 = 0, h = 0;
    for (size_t t = 0; t < nt; t++) {
        const int64_t s0 = p->const_off[t], S = p->const_off[t + 1] - s0, U = pl->ng[t];
        slot_off[t] = s0;
        unk_tree_off[t] = u0;
        hoff[t] = h;
        for (int64_t s = 0; s < S; s++) slot_unk[s0 + s] = u0 + tie[s0 + s];
        // (the tree's CSR offsets count from 0: shifted to its first entry of unk_slots, which is its first slot)
        ties_csr(S, tie + s0, U, s0, unk_off + u0, unk_slots + s0);
        for (int64_t u = 0; u <= U; u++) unk_off[u0 + u] += s0;
        u0 += U;
        h += S * S;
    }
    slot_off[nt] = (int64_t)nc;
    unk_tree_off[nt] = nu;
    pl->hspan = h;
    return DE_OK;
}

// ---- de_gn_lm_step(_wide) (kernels: de_lm.hip, de_gn_wide.hip; arithmetic: de_lm_solve.h, de_lm_solve_wide.h) ----
static int gn_lm_step_impl(de_ctx_t *c, int dtype, int64_t n_trees, const int32_t *n_grad, const void *dloss, const int64_t *dloss_offsets,
                           const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam, double *step, bool wide = false) {
    if (!c) return DE_ERR_INVALID_ARG;
    if (dtype != DE_F32 && dtype != DE_F64) return fail(c, DE_ERR_INVALID_ARG, "de_gn_lm_step: dtype must be DE_F32 or DE_F64");
    if (n_trees < 0) return fail(c, DE_ERR_INVALID_ARG, "n_trees < 0");
    if (n_trees == 0) return DE_OK;
    if (!n_grad || !dloss || !jtj || !has || !lam || !step) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = dtype == DE_F32 ? 4 : 8, nt = (size_t)n_trees;
    // (offsets are checked before anything is written; a growing state buffer is shared with de_fit_consts_lm, which does not run now)
    LmTables tab;
    int rc = lm_tables(c, n_trees, n_grad, dloss_offsets, jtj_offsets, &tab);
    if (rc != DE_OK) return rc;
    const size_t span = (size_t)std::max<int64_t>(tab.span, 1), jspan = (size_t)std::max<int64_t>(tab.jspan, 1);
    const bool h_dl = !is_device_ptr(dloss), h_j = !is_device_ptr(jtj), h_has = !is_device_ptr(has), h_lam = !is_device_ptr(lam), h_step = !is_device_ptr(step);
    Workspace ws; // the staged images of the host buffers
    const auto r_dl = ws.place<char>(span * es, h_dl), r_j = ws.place<char>(jspan * es, h_j);
    const auto r_has = ws.place<uint8_t>(nt, h_has);
    const auto r_lam = ws.place<double>(nt, h_lam), r_step = ws.place<double>(span, h_step);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    LmStepArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = n_trees;
    a.n_grad = tab.ng;
    a.doff = tab.doff;
    a.joff = tab.joff;
    a.dloss = dloss;
    a.jtj = jtj;
    a.has = has;
    a.lam = lam;
    a.step = step;
    if (h_dl) { HIP_TRY(c, hipMemcpyAsync(ws.ptr(r_dl), dloss, span * es, hipMemcpyHostToDevice, c->stream)); a.dloss = ws.ptr(r_dl); }
    if (h_j) { HIP_TRY(c, hipMemcpyAsync(ws.ptr(r_j), jtj, jspan * es, hipMemcpyHostToDevice, c->stream)); a.jtj = ws.ptr(r_j); }
    if (h_has) { HIP_TRY(c, hipMemcpyAsync(ws.ptr(r_has), has, nt, hipMemcpyHostToDevice, c->stream)); a.has = ws.ptr(r_has); }
    if (h_lam) { HIP_TRY(c, hipMemcpyAsync(ws.ptr(r_lam), lam, nt * 8, hipMemcpyHostToDevice, c->stream)); a.lam = ws.ptr(r_lam); }
    if (h_step) { // entries no tree owns keep the caller's values: the staged image starts as a copy
        HIP_TRY(c, hipMemcpyAsync(ws.ptr(r_step), step, span * 8, hipMemcpyHostToDevice, c->stream));
        a.step = ws.ptr(r_step);
    }
    if (!c->nested) HIP_TRY(c, time_begin(c));
    HIP_TRY(c, launch_lm_step(dtype, a, c->stream));
    c->last_kernel = "de_lm_step_kernel";
    if (wide) { // de_gn_lm_step_wide: the trees of 9 .. 32 rows, behind the zero step the kernel above gave them
        HIP_TRY(c, launch_lm_step_wide(dtype, a, c->stream));
        c->last_kernel = "de_lm_step_wide_kernel";
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (h_step) HIP_TRY(c, hipMemcpyAsync(step, ws.ptr(r_step), span * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_dl || h_j || h_has || h_lam || h_step) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DE_OK;
}
int de_gn_lm_step(de_ctx_t *c, int dtype, int64_t n_trees, const int32_t *n_grad, const void *dloss, const int64_t *dloss_offsets,
                  const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam, double *step) {
    DE_NOTHROW(c, gn_lm_step_impl(c, dtype, n_trees, n_grad, dloss, dloss_offsets, jtj, jtj_offsets, has, lam, step));
}
int de_gn_lm_step_wide(de_ctx_t *c, int dtype, int64_t n_trees, const int32_t *n_grad, const void *dloss, const int64_t *dloss_offsets,
                       const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam, double *step) {
    DE_NOTHROW(c, gn_lm_step_impl(c, dtype, n_trees, n_grad, dloss, dloss_offsets, jtj, jtj_offsets, has, lam, step, true));
}

// ---- de_fit_stats_lm_step(_wide) (kernels: de_lm_scaled.hip, de_lm_scaled_wide.hip; arithmetic: de_lm_project.h,
// de_lm_project_wide.h) ------------------------------------------------------------------------------------------------------------------------
static int fit_stats_lm_step_impl(de_ctx_t *c, int dtype, int64_t n_trees, const int32_t *n_grad, const double *stats, const double *ystats,
                                  const double *dmom, const int64_t *dmom_offsets, const void *jtj, const int64_t *jtj_offsets,
                                  const uint8_t *has, const double *lam, double *step, double *sse, bool wide = false) {
    if (!c) return DE_ERR_INVALID_ARG;
    if (dtype != DE_F32 && dtype != DE_F64) return fail(c, DE_ERR_INVALID_ARG, "de_fit_stats_lm_step: dtype must be DE_F32 or DE_F64");
    if (n_trees < 0) return fail(c, DE_ERR_INVALID_ARG, "n_trees < 0");
    if (n_trees == 0) return DE_OK;
    if (!n_grad || !stats || !ystats || !dmom || !jtj || !has || !lam || !step) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = dtype == DE_F32 ? 4 : 8, nt = (size_t)n_trees;
    LmTables tab;
    int rc = lm_tables(c, n_trees, n_grad, dmom_offsets, jtj_offsets, &tab, 3);
    if (rc != DE_OK) return rc;
    const size_t mspan = (size_t)std::max<int64_t>(tab.span, 1), jspan = (size_t)std::max<int64_t>(tab.jspan, 1), sspan = (size_t)tab.sspan;
    const bool h_st = !is_device_ptr(stats), h_ys = !is_device_ptr(ystats), h_dm = !is_device_ptr(dmom), h_j = !is_device_ptr(jtj),
               h_has = !is_device_ptr(has), h_lam = !is_device_ptr(lam), h_step = !is_device_ptr(step), h_sse = sse && !is_device_ptr(sse);
    Workspace ws; // the staged images of the host buffers
    const auto r_st = ws.place<double>(nt * 3, h_st), r_ys = ws.place<double>(3, h_ys), r_dm = ws.place<double>(mspan, h_dm);
    const auto r_j = ws.place<char>(jspan * es, h_j);
    const auto r_has = ws.place<uint8_t>(nt, h_has);
    const auto r_lam = ws.place<double>(nt, h_lam), r_step = ws.place<double>(sspan, h_step), r_sse = ws.place<double>(nt, h_sse);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    LmScaledStepArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = n_trees;
    a.n_grad = tab.ng;
    a.moff = tab.doff;
    a.joff = tab.joff;
    a.soff = tab.soff;
    a.stats = stats; a.ystats = ystats; a.dmom = dmom; a.jtj = jtj; a.has = has; a.lam = lam; a.step = step; a.sse = sse;
    auto up = [&](const void *src, void *dst, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream); };
    if (h_st) { HIP_TRY(c, up(stats, ws.ptr(r_st), nt * 24)); a.stats = ws.ptr(r_st); }
    if (h_ys) { HIP_TRY(c, up(ystats, ws.ptr(r_ys), 24)); a.ystats = ws.ptr(r_ys); }
    if (h_dm) { HIP_TRY(c, up(dmom, ws.ptr(r_dm), mspan * 8)); a.dmom = ws.ptr(r_dm); }
    if (h_j) { HIP_TRY(c, up(jtj, ws.ptr(r_j), jspan * es)); a.jtj = ws.ptr(r_j); }
    if (h_has) { HIP_TRY(c, up(has, ws.ptr(r_has), nt)); a.has = ws.ptr(r_has); }
    if (h_lam) { HIP_TRY(c, up(lam, ws.ptr(r_lam), nt * 8)); a.lam = ws.ptr(r_lam); }
    if (h_step) a.step = ws.ptr(r_step); // (packed: every entry is some tree's)
    if (h_sse) a.sse = ws.ptr(r_sse);
    if (!c->nested) HIP_TRY(c, time_begin(c));
    HIP_TRY(c, launch_lm_step_scaled(dtype, a, c->stream));
    c->last_kernel = "de_lm_step_scaled_kernel";
    if (wide) { // de_fit_stats_lm_step_wide: the trees of 9 .. 32 rows, behind the zero step (and the sse) the kernel above gave them
        HIP_TRY(c, launch_lm_step_scaled_wide(dtype, a, c->stream));
        c->last_kernel = "de_lm_step_scaled_wide_kernel";
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (h_step && sspan) HIP_TRY(c, hipMemcpyAsync(step, ws.ptr(r_step), sspan * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_sse) HIP_TRY(c, hipMemcpyAsync(sse, ws.ptr(r_sse), nt * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_st || h_ys || h_dm || h_j || h_has || h_lam || h_step || h_sse) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DE_OK;
}
int de_fit_stats_lm_step(de_ctx_t *c, int dtype, int64_t n_trees, const int32_t *n_grad, const double *stats, const double *ystats,
                         const double *dmom, const int64_t *dmom_offsets, const void *jtj, const int64_t *jtj_offsets, const uint8_t *has,
                         const double *lam, double *step, double *sse) {
    DE_NOTHROW(c, fit_stats_lm_step_impl(c, dtype, n_trees, n_grad, stats, ystats, dmom, dmom_offsets, jtj, jtj_offsets, has, lam, step, sse));
}
int de_fit_stats_lm_step_wide(de_ctx_t *c, int dtype, int64_t n_trees, const int32_t *n_grad, const double *stats, const double *ystats,
                              const double *dmom, const int64_t *dmom_offsets, const void *jtj, const int64_t *jtj_offsets, const uint8_t *has,
                              const double *lam, double *step, double *sse) {
    DE_NOTHROW(c, fit_stats_lm_step_impl(c, dtype, n_trees, n_grad, stats, ystats, dmom, dmom_offsets, jtj, jtj_offsets, has, lam, step, sse, true));
}

// ---- what the three fits share ---------------------------------------------------------------------------------------------------------------
// The refusals, in their order: the context; the spec (spec_check: the driver's own, empty where the fit takes none); a CSE program
// (fold_hint: what its caller does with the rows of a shared constant); a tree whose constant rows are not its constants; the options
// (opts_why: lm_opts_problem / bfgs_opts_problem); N and the null buffers (`required` must not be null when there is a tree); ldX; the
// parameter arguments.  `what`: the name in the texts (the narrow entry point's, for its _ex and _wide forms too).  gradient_rows = false
// (de_fit_consts_nm: no gradient): the two refusals about constant rows are skipped.  tied (the _tied entry points):
// the occurrence rows are folded on the device, so a CSE program is served.
static int fit_check(de_ctx_t *c, de_program_t *p, const char *what, const char *fold_hint, const std::function<int()> &spec_check,
                     const char *opts_why, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                     std::initializer_list<const void *> required, bool gradient_rows = true, bool tied = false) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    if (spec_check)
        if (const int rc = spec_check()) return rc;
    if (gradient_rows && !tied && !p->in_cse.empty())
        return fail(c, DE_ERR_UNSUPPORTED, "%s: a program made by de_program_create_cse has one gradient row per occurrence of a shared constant "
                                           "(%s); such callers keep the host loop", what, fold_hint);
    for (int64_t t = 0; gradient_rows && t < p->n_trees; t++)
        if (de_program_n_grad(p, t, DE_GRAD_CONSTANT) != p->const_off[(size_t)t + 1] - p->const_off[(size_t)t])
            return fail(c, DE_ERR_UNSUPPORTED, "%s: tree %lld has %lld constant rows for %lld constants", what, (long long)t,
                        (long long)de_program_n_grad(p, t, DE_GRAD_CONSTANT), (long long)(p->const_off[(size_t)t + 1] - p->const_off[(size_t)t]));
    if (opts_why) return fail(c, DE_ERR_INVALID_ARG, "%s", opts_why);
    bool missing = N > 0 && !X;
    for (const void *q : required) missing = missing || !q;
    if (N < 0 || (p->n_trees > 0 && missing)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    if (ldX < p->n_features) return fail(c, DE_ERR_INVALID_ARG, "ldX < n_features");
    return check_param_args(c, p, pa, N);
}

// The loop of a fit, written once.  evaluate(trial): the objective (and what the step needs) at the program's constants, into the accepted
// (false) or the trial (true) state; init: the per-tree state; first_history(row 0) behind it; then, where nothing can move (no sample, no
// constant, no iteration), fill_history for every further row, else `iters` times: propose (the step or direction kernel: trial constants
// from the accepted state), the trial constants installed, evaluate(true), accept(history row).  The program holds the accepted constants
// afterwards; finish (may be empty) runs behind that, where the loop ran; report (may be empty) runs last, whether it ran or not.  The
// inner calls leave the timing events alone: the ring sees one call.
struct FitLoop {
    std::function<int(bool)> evaluate;
    std::function<int()> init, propose, finish, report;
    // a tied fit (both may be empty): prepare runs before the first evaluation where the loop will run — the program takes
    // unpack(pack(its constants)), the accepted unknowns are packed; settle runs before the accepted constants are installed at the end —
    // consts_acc, the slot vector, takes unpack of the accepted unknowns
    std::function<int()> prepare, settle;
    std::function<int(double *)> first_history, fill_history, accept;
    void *consts_acc = nullptr, *consts_trial = nullptr;
    const char *last_kernel = nullptr; // what the context reports behind the loop (null: what the last inner call set)
};
static int run_fit(de_ctx_t *c, de_program_t *p, int32_t iters, bool can_move, double *hist, const FitLoop &f) {
    const size_t nt = (size_t)p->n_trees;
    if (!c->nested) HIP_TRY(c, time_begin(c));
    {
        NestGuard nest(c);
        int rc = can_move && iters > 0 && f.prepare ? f.prepare() : (int)DE_OK;
        if (rc == DE_OK) rc = f.evaluate(false);
        if (rc == DE_OK) rc = f.init();
        if (rc == DE_OK) rc = f.first_history(hist);
        if (rc != DE_OK) return rc;
        if (!(can_move && iters > 0)) { // (nothing can be accepted: every row of the history is the first)
            for (int32_t r = 1; r <= iters && hist; r++)
                if ((rc = f.fill_history(hist + (size_t)r * nt)) != DE_OK) return rc;
        } else {
            rc = de_program_get_consts(p, f.consts_acc); // (device to device behind a device set)
            if (rc != DE_OK) return rc;
            for (int32_t it = 0; it < iters; it++) {
                if ((rc = f.propose()) != DE_OK) return rc;
                rc = set_consts_device_impl(p, f.consts_trial);
                if (rc == DE_OK) rc = f.evaluate(true);
                if (rc != DE_OK) break;
                if ((rc = f.accept(hist ? hist + ((size_t)it + 1) * nt : nullptr)) != DE_OK) return rc;
            }
            if (f.last_kernel) c->last_kernel = f.last_kernel;
            // the program holds the accepted constants afterwards (after a failure too: the last accepted ones)
            int rc2 = f.settle ? f.settle() : (int)DE_OK;
            if (rc2 == DE_OK) rc2 = set_consts_device_impl(p, f.consts_acc);
            if (rc != DE_OK) return rc;
            if (rc2 != DE_OK) return rc2;
            if (f.finish && (rc = f.finish()) != DE_OK) return rc;
        }
        if (f.report && (rc = f.report()) != DE_OK) return rc;
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    return DE_OK;
}

// What a tied fit adds to its driver: the optimiser kernels see U_t unknowns per tree (ng) and vectors of unknowns; the
// program is set from SLOT vectors (sA accepted, sT trial), and an evaluation writes its occurrence rows (gO) and blocks (jO: the
// Levenberg-Marquardt fit alone) into buffers of their own, which fold / fold_matrix reduce into the state the kernels read.
// on = false (tie == NULL: the identity): nothing of this exists and the call runs its untied twin's launches.
struct TiedState {
    bool on = false;
    TiePlan plan;
    TieArgs a;
    const unsigned char *dev = nullptr;
    Workspace::Region<char> sA{0, false}, sT{0, false}, gO{0, false}, jO{0, false};
    int begin(de_ctx *c, const de_program *p, const char *what, const int32_t *tie) {
        std::memset(&a, 0, sizeof a);
        if (!tie) return DE_OK;
        on = true;
        return tie_plan(c, p, what, tie, &plan);
    }
    const int32_t *widths(const de_program *p) const { return on ? plan.ng.data() : p->n_consts_tree.data(); }
    void place(Workspace &ws, size_t es, bool gradient, bool matrix) {
        if (!on) return;
        sA = ws.place<char>(plan.nc * es);
        sT = ws.place<char>(plan.nc * es);
        gO = ws.place<char>(plan.nc * es, gradient);
        jO = ws.place<char>((size_t)std::max<int64_t>(plan.hspan, 1) * es, matrix);
    }
    // FitLoop's slot vectors and hooks: u_acc / u_trial are the kernels' vectors of unknowns
    void hook(de_ctx *c, de_program *p, const Workspace &ws, void *u_acc, void *u_trial, FitLoop *f) {
        if (!on) return;
        void *acc = ws.ptr(sA), *trial = ws.ptr(sT);
        f->consts_acc = acc;
        f->consts_trial = trial;
        const std::function<int()> propose = f->propose;
        f->propose = [=]() -> int {
            const int rc = propose();
            if (rc != DE_OK) return rc;
            HIP_TRY(c, launch_ties_unpack(p->dtype, a, u_trial, trial, c->stream));
            return DE_OK;
        };
        f->prepare = [=]() -> int { // the first occurrence decides: the program starts from unpack(pack(its constants))
            int rc = de_program_get_consts(p, acc);
            if (rc != DE_OK) return rc;
            HIP_TRY(c, launch_ties_pack(p->dtype, a, acc, u_acc, c->stream));
            HIP_TRY(c, launch_ties_unpack(p->dtype, a, u_acc, acc, c->stream));
            return set_consts_device_impl(p, acc);
        };
        f->settle = [=]() -> int {
            HIP_TRY(c, launch_ties_unpack(p->dtype, a, u_acc, acc, c->stream));
            return DE_OK;
        };
    }
};

// ---- de_fit_consts_lm(_ex, _wide) (kernels: de_lm.hip, de_gn_wide.hip) -----------------------------------
// row_limit: the widest tree that is fitted — DE_GN_MAX_ROWS (de_fit_consts_lm: every evaluation is de_eval_loss_gn_ex's) or
// DE_GN_WIDE_MAX_ROWS (de_fit_consts_lm_wide: de_eval_loss_gn_wide's, and the wide trees' steps by de_lm_step_wide_kernel)
static int fit_consts_lm_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                              const void *w, const de_loss_spec_t *spec_in, double e_floor, const de_lm_opts_t *opts, void *loss, uint8_t *ok,
                              double *history, int32_t *n_accept, int row_limit, bool tied = false, const int32_t *tie = nullptr) {
    const char *what = tied ? "de_fit_consts_lm_tied" : "de_fit_consts_lm";
    const de_lm_opts_t defaults{10, 0, 1e-3, 10.0, 0.1, 1e-12};
    const de_lm_opts_t o = opts ? *opts : defaults;
    const auto spec_check = [&]() -> int {
        char why[160];
        int src;
        return gn_spec_problem(spec_in, e_floor, p->dtype, &src, why, sizeof why) ? fail(c, src, "%s", why) : (int)DE_OK;
    };
    int rc = fit_check(c, p, what, "the caller folds them: S H S^T", spec_check, lm_opts_problem(&o), X, N, ldX, pa, {ok, y}, true, tied);
    if (rc != DE_OK || p->n_trees == 0) return rc;
    TiedState ts; // (tied: the gradient and the U x U matrix of the unique constants, folded from the occurrence rows and block)
    if (tied && (rc = ts.begin(c, p, what, tie)) != DE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size(), rows = (size_t)o.iters + 1;
    const size_t nu = ts.on ? (size_t)ts.plan.nu : nc;
    LmTables tab; // packed: the dloss offsets are the constants' offsets
    if ((rc = lm_tables(c, p->n_trees, ts.widths(p), nullptr, nullptr, &tab, 1, ts.on ? &ts.plan.blob : nullptr, &ts.dev)) != DE_OK) return rc;
    const size_t span = (size_t)std::max<int64_t>(tab.span, 1), jspan = (size_t)std::max<int64_t>(tab.jspan, 1);
    FitInputs in;
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    // the state: accepted and trial constants, losses, gradients, matrices and flags; lam and the step; images of a host history / n_accept
    const bool h_hist = FitOutputs::on_host(history), h_acc = FitOutputs::on_host(n_accept);
    Workspace ws;
    const auto cA = ws.place<char>(nu * es), cT = ws.place<char>(nu * es), lA = ws.place<char>(nt * es), lT = ws.place<char>(nt * es),
               dA = ws.place<char>(span * es), dT = ws.place<char>(span * es), jA = ws.place<char>(jspan * es), jT = ws.place<char>(jspan * es);
    ts.place(ws, es, true, true);
    const auto okA = ws.place<uint8_t>(nt), okT = ws.place<uint8_t>(nt);
    const auto lam = ws.place<double>(nt), step = ws.place<double>(span), r_hist = ws.place<double>(rows * nt, h_hist);
    const auto r_acc = ws.place<int32_t>(nt, h_acc);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    if (ts.on) ts.plan.bind(ts.dev, tab.joff, DE_GN_MAX_ROWS, &ts.a);
    FitOutputs out;
    out.from_state(loss, ws.ptr(lA), nt * es);
    out.from_state(ok, ws.ptr(okA), nt);
    double *hist = out.in_place(history, h_hist, ws.ptr(r_hist), rows * nt);
    int32_t *acc = out.in_place(n_accept, h_acc, ws.ptr(r_acc), nt);
    LmStepArgs s;
    std::memset(&s, 0, sizeof s);
    s.n_trees = p->n_trees;
    s.n_grad = tab.ng;
    s.doff = s.coff = tab.doff;
    s.joff = tab.joff;
    s.dloss = ws.ptr(dA); s.jtj = ws.ptr(jA); s.has = ws.ptr(okA);
    s.lam = ws.ptr(lam);
    s.step = ws.ptr(step);
    s.consts = ws.ptr(cA);
    s.trial = ws.ptr(cT);
    LmAcceptArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = p->n_trees;
    a.n_grad = tab.ng;
    a.doff = a.coff = tab.doff;
    a.joff = tab.joff;
    a.consts_acc = ws.ptr(cA); a.loss_acc = ws.ptr(lA); a.dloss_acc = ws.ptr(dA); a.jtj_acc = ws.ptr(jA); a.ok_acc = ws.ptr(okA);
    a.consts_trial = ws.ptr(cT); a.loss_trial = ws.ptr(lT); a.dloss_trial = ws.ptr(dT); a.jtj_trial = ws.ptr(jT); a.ok_trial = ws.ptr(okT);
    a.lam = ws.ptr(lam);
    a.up = o.up; a.down = o.down; a.lam_min = o.lam_min;
    a.n_accept = acc;
    a.row_limit = row_limit;
    const de_loss_spec_t spec = *spec_in;
    const bool wide = row_limit > DE_GN_MAX_ROWS;
    FitLoop f;
    f.consts_acc = ws.ptr(cA);
    f.consts_trial = ws.ptr(cT);
    f.evaluate = [&](bool trial) -> int {
        void *l = ws.ptr(trial ? lT : lA), *d = ws.ptr(trial ? dT : dA), *j = ws.ptr(trial ? jT : jA);
        uint8_t *k = ws.ptr(trial ? okT : okA);
        if (wide) return gn_wide_impl(c, p, in.Xd, N, ldX, in.pa, DE_GRAD_CONSTANT, in.yd, in.wd, &spec, e_floor, l, d, nullptr, j, nullptr, k);
        // (tied: the occurrence rows and packed S x S blocks land in buffers of their own and are folded into d and j)
        const GnPlan gn{ts.on ? ws.ptr(ts.jO) : j, nullptr, e_floor};
        const int rc1 = loss_grad_impl(c, p, in.Xd, N, ldX, in.pa, DE_GRAD_CONSTANT, in.yd, in.wd, &spec, l, ts.on ? ws.ptr(ts.gO) : d, nullptr, k,
                                       nullptr, false, &gn);
        if (rc1 != DE_OK || !ts.on) return rc1;
        HIP_TRY(c, launch_ties_fold(p->dtype, ts.a, ws.ptr(ts.gO), d, c->stream));
        HIP_TRY(c, launch_ties_fold_matrix(p->dtype, ts.a, ws.ptr(ts.jO), j, c->stream));
        return DE_OK;
    };
    f.init = [&]() -> int { HIP_TRY(c, launch_lm_init(p->n_trees, o.lam0, ws.ptr(lam), acc, c->stream)); return DE_OK; };
    f.first_history = f.fill_history = [&](double *row) -> int {
        HIP_TRY(c, launch_lm_history(p->dtype, ws.ptr(lA), p->n_trees, row, c->stream));
        return DE_OK;
    };
    f.propose = [&]() -> int {
        HIP_TRY(c, launch_lm_step(p->dtype, s, c->stream));
        if (wide) HIP_TRY(c, launch_lm_step_wide(p->dtype, s, c->stream)); // (behind it: the narrow kernel gave the wide trees the zero step)
        return DE_OK;
    };
    f.accept = [&](double *row) -> int {
        a.history_row = row;
        HIP_TRY(c, launch_lm_accept(p->dtype, a, c->stream));
        return DE_OK;
    };
    ts.hook(c, p, ws, ws.ptr(cA), ws.ptr(cT), &f);
    if ((rc = run_fit(c, p, o.iters, N > 0 && nc > 0, hist, f)) != DE_OK) return rc;
    return out.finish(c);
}
int de_fit_consts_lm_tied(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                          const void *w, const de_loss_spec_t *spec, double e_floor, const de_lm_opts_t *opts, const int32_t *tie, void *loss,
                          uint8_t *ok, double *history, int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lm_tied");
    DE_NOTHROW(c, fit_consts_lm_impl(c, p, X, N, ldX, pa, y, w, spec, e_floor, opts, loss, ok, history, n_accept, DE_GN_MAX_ROWS, true, tie));
}
int de_fit_consts_lm_ex(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                        const void *w, const de_loss_spec_t *spec, double e_floor, const de_lm_opts_t *opts, void *loss, uint8_t *ok,
                        double *history, int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lm");
    DE_NOTHROW(c, fit_consts_lm_impl(c, p, X, N, ldX, pa, y, w, spec, e_floor, opts, loss, ok, history, n_accept, DE_GN_MAX_ROWS));
}
int de_fit_consts_lm(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                     const void *w, const de_lm_opts_t *opts, void *loss, uint8_t *ok, double *history, int32_t *n_accept) {
    const de_loss_spec_t spec{DE_LOSS_L2, 0, 0.0};
    return de_fit_consts_lm_ex(c, p, X, N, ldX, pa, y, w, &spec, 0.0, opts, loss, ok, history, n_accept);
}
int de_fit_consts_lm_wide(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                          const void *w, const de_loss_spec_t *spec, double e_floor, const de_lm_opts_t *opts, void *loss, uint8_t *ok,
                          double *history, int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lm_wide");
    DE_NOTHROW(c, fit_consts_lm_impl(c, p, X, N, ldX, pa, y, w, spec, e_floor, opts, loss, ok, history, n_accept, DE_GN_WIDE_MAX_ROWS));
}

// ---- de_fit_consts_lm_scaled(_wide) (kernels: de_lm_scaled.hip, de_lm_scaled_wide.hip) ---------------------------
// The fit above with every evaluation de_eval_fit_stats_grad's (a FitPlan into the state) and the objective the scaled sse.
// row_limit: the widest tree that is fitted — DE_GN_MAX_ROWS (de_fit_consts_lm_scaled) or DE_GN_WIDE_MAX_ROWS (de_fit_consts_lm_scaled_wide:
// every evaluation de_eval_fit_stats_grad_wide's, and the wide trees' steps by de_lm_step_scaled_wide_kernel)
static int fit_consts_lm_scaled_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                                     const void *w, const de_lm_opts_t *opts, double *sse, double *stats, double *ystats, uint8_t *ok,
                                     double *history, int32_t *n_accept, int row_limit) {
    const de_lm_opts_t defaults{10, 0, 1e-3, 10.0, 0.1, 1e-12};
    const de_lm_opts_t o = opts ? *opts : defaults;
    int rc = fit_check(c, p, "de_fit_consts_lm_scaled", "the caller folds them: S H S^T", nullptr, lm_opts_problem(&o), X, N, ldX, pa, {ok, sse, y});
    if (rc != DE_OK || p->n_trees == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size(), rows = (size_t)o.iters + 1;
    LmTables tab; // packed: dmom at 3 x the constants' offsets, the step at the constants' offsets
    if ((rc = lm_tables(c, p->n_trees, p->n_consts_tree.data(), nullptr, nullptr, &tab, 3)) != DE_OK) return rc;
    const size_t mspan = (size_t)std::max<int64_t>(tab.span, 1), jspan = (size_t)std::max<int64_t>(tab.jspan, 1), span = std::max<size_t>(nc, 1);
    FitInputs in;
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    // the state: accepted and trial constants, statistics, dmom, matrices and flags; ystats; the accepted sse, lam and the step; the images
    const bool h_hist = FitOutputs::on_host(history), h_acc = FitOutputs::on_host(n_accept);
    Workspace ws;
    const auto cA = ws.place<char>(nc * es), cT = ws.place<char>(nc * es), jA = ws.place<char>(jspan * es), jT = ws.place<char>(jspan * es);
    const auto sA = ws.place<double>(nt * 3), sT = ws.place<double>(nt * 3), ys = ws.place<double>(3), mA = ws.place<double>(mspan),
               mT = ws.place<double>(mspan), sseA = ws.place<double>(nt), lam = ws.place<double>(nt), step = ws.place<double>(span),
               r_hist = ws.place<double>(rows * nt, h_hist);
    const auto okA = ws.place<uint8_t>(nt), okT = ws.place<uint8_t>(nt);
    const auto r_acc = ws.place<int32_t>(nt, h_acc);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    FitOutputs out;
    out.from_state(sse, ws.ptr(sseA), nt * 8);
    out.from_state(stats, ws.ptr(sA), nt * 24);
    out.from_state(ystats, ws.ptr(ys), 24);
    out.from_state(ok, ws.ptr(okA), nt);
    double *hist = out.in_place(history, h_hist, ws.ptr(r_hist), rows * nt);
    int32_t *acc = out.in_place(n_accept, h_acc, ws.ptr(r_acc), nt);
    LmScaledStepArgs s;
    std::memset(&s, 0, sizeof s);
    s.n_trees = p->n_trees;
    s.n_grad = tab.ng;
    s.moff = tab.doff; s.joff = tab.joff; s.soff = tab.soff;
    s.stats = ws.ptr(sA); s.ystats = ws.ptr(ys); s.dmom = ws.ptr(mA); s.jtj = ws.ptr(jA);
    s.has = ws.ptr(okA);
    s.lam = ws.ptr(lam);
    s.step = ws.ptr(step);
    s.consts = ws.ptr(cA);
    s.trial = ws.ptr(cT);
    LmScaledAcceptArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = p->n_trees;
    a.n_grad = tab.ng;
    a.moff = tab.doff; a.joff = tab.joff; a.coff = tab.soff;
    a.ystats = ws.ptr(ys);
    a.consts_acc = ws.ptr(cA); a.jtj_acc = ws.ptr(jA); a.stats_acc = ws.ptr(sA); a.dmom_acc = ws.ptr(mA); a.sse_acc = ws.ptr(sseA); a.ok_acc = ws.ptr(okA);
    a.consts_trial = ws.ptr(cT); a.jtj_trial = ws.ptr(jT); a.stats_trial = ws.ptr(sT); a.dmom_trial = ws.ptr(mT); a.ok_trial = ws.ptr(okT);
    a.lam = ws.ptr(lam);
    a.up = o.up; a.down = o.down; a.lam_min = o.lam_min;
    a.n_accept = acc;
    a.row_limit = row_limit;
    const de_loss_spec_t spec{DE_LOSS_L2, 0, 0.0};
    const bool wide = row_limit > DE_GN_MAX_ROWS;
    FitLoop f;
    f.consts_acc = ws.ptr(cA);
    f.consts_trial = ws.ptr(cT);
    f.last_kernel = "de_lm_accept_scaled_kernel";
    f.evaluate = [&](bool trial) -> int { // (ystats: the same three values every time)
        double *st = ws.ptr(trial ? sT : sA), *m = ws.ptr(trial ? mT : mA);
        void *j = ws.ptr(trial ? jT : jA);
        uint8_t *k = ws.ptr(trial ? okT : okA);
        if (wide) return fit_stats_grad_wide_impl(c, p, in.Xd, N, ldX, in.pa, DE_GRAD_CONSTANT, in.yd, in.wd, st, ws.ptr(ys), m, nullptr, j, nullptr, k);
        const FitPlan fit{st, ws.ptr(ys), j, nullptr};
        return loss_grad_impl(c, p, in.Xd, N, ldX, in.pa, DE_GRAD_CONSTANT, in.yd, in.wd, &spec, nullptr, m, nullptr, k, nullptr, false, nullptr, &fit);
    };
    f.init = [&]() -> int { HIP_TRY(c, launch_lm_init(p->n_trees, o.lam0, ws.ptr(lam), acc, c->stream)); return DE_OK; };
    f.first_history = [&](double *row) -> int { // (the accepted sse itself comes from here)
        HIP_TRY(c, launch_lm_sse_scaled(ws.ptr(sA), ws.ptr(ys), p->n_trees, ws.ptr(sseA), row, c->stream));
        return DE_OK;
    };
    f.fill_history = [&](double *row) -> int {
        HIP_TRY(c, launch_lm_history(DE_F64, ws.ptr(sseA), p->n_trees, row, c->stream));
        return DE_OK;
    };
    f.propose = [&]() -> int {
        HIP_TRY(c, launch_lm_step_scaled(p->dtype, s, c->stream));
        if (wide) HIP_TRY(c, launch_lm_step_scaled_wide(p->dtype, s, c->stream)); // (behind it: the narrow kernel gave the wide trees the zero step)
        return DE_OK;
    };
    f.accept = [&](double *row) -> int {
        a.history_row = row;
        HIP_TRY(c, launch_lm_accept_scaled(p->dtype, a, c->stream));
        return DE_OK;
    };
    if ((rc = run_fit(c, p, o.iters, N > 0 && nc > 0, hist, f)) != DE_OK) return rc;
    return out.finish(c);
}
int de_fit_consts_lm_scaled(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                            const void *w, const de_lm_opts_t *opts, double *sse, double *stats, double *ystats, uint8_t *ok, double *history,
                            int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lm_scaled");
    DE_NOTHROW(c, fit_consts_lm_scaled_impl(c, p, X, N, ldX, pa, y, w, opts, sse, stats, ystats, ok, history, n_accept, DE_GN_MAX_ROWS));
}
int de_fit_consts_lm_scaled_wide(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                                 const void *w, const de_lm_opts_t *opts, double *sse, double *stats, double *ystats, uint8_t *ok, double *history,
                                 int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lm_scaled_wide");
    DE_NOTHROW(c, fit_consts_lm_scaled_impl(c, p, X, N, ldX, pa, y, w, opts, sse, stats, ystats, ok, history, n_accept, DE_GN_WIDE_MAX_ROWS));
}

// ---- de_fit_consts_bfgs (kernels: de_bfgs.hip, arithmetic: de_bfgs.h) and de_fit_consts_lbfgs (§4.4.15; kernels:
// de_lbfgs.hip, arithmetic: de_lbfgs.h) -------------------------------------------------------------------------------------------------------
// The same fit with every evaluation de_eval_loss_grad_ex's (no matrix) and the kernels of de_bfgs.hip (memory = 0) or, with a ring of
// `memory` pairs per tree instead of B, those of de_lbfgs.hip.  o: the options both share; opts_why: what is wrong with the caller's.
// de_fit_consts_lbfgs ends with one de_eval_loss_ex at the accepted constants (FitLoop::report): loss and ok are that call's.
static int fit_consts_qn_impl(de_ctx_t *c, de_program_t *p, const char *what, int memory, const de_bfgs_opts_t &o, const char *opts_why,
                              const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y, const void *w,
                              const de_loss_spec_t *spec_in, void *loss, uint8_t *ok, double *history, int32_t *n_accept,
                              bool tied = false, const int32_t *tie = nullptr) {
    const auto spec_check = [&]() -> int {
        char why[160];
        if (loss_spec_problem(spec_in, 1, why, sizeof why)) return fail(c, DE_ERR_INVALID_ARG, "%s", why);
        if (spec_in->kind == DE_LOSS_PULLBACK) return fail(c, DE_ERR_INVALID_ARG, "%s: DE_LOSS_PULLBACK is no objective", what);
        if (memory > 0 && !p->threaded) // (the loss it reports is de_eval_loss_ex's)
            return fail(c, DE_ERR_UNSUPPORTED, "%s needs the LDS-tiled kernel (feature matrix too wide for this build)", what);
        return DE_OK;
    };
    int rc = fit_check(c, p, what, "the caller sums them", spec_check, opts_why, X, N, ldX, pa, {ok, y}, true, tied);
    if (rc != DE_OK || p->n_trees == 0) return rc;
    TiedState ts; // (tied: the unknowns are the unique constants)
    if (tied && (rc = ts.begin(c, p, what, tie)) != DE_OK) return rc;
    const int32_t *ng = ts.widths(p);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size(), rows = (size_t)o.iters + 1;
    const size_t nu = ts.on ? (size_t)ts.plan.nu : nc;
    QnKernels q;
    std::memset(&q.x, 0, sizeof q.x);
    q.memory = memory;
    std::vector<int64_t> boff(nt); // B: G^2 doubles (the ring: memory x G, twice) of every tree that is fitted, none of the others
    int64_t bspan = 0;
    for (size_t t = 0; t < nt; t++) {
        boff[t] = bspan;
        bspan += q.state_doubles(ng[t]);
    }
    LmTables tab; // packed: the dloss offsets are the constants' offsets; the matrix offsets are B's (the ring's)
    if ((rc = lm_tables(c, p->n_trees, ng, nullptr, boff.data(), &tab, 1, ts.on ? &ts.plan.blob : nullptr, &ts.dev)) != DE_OK) return rc;
    const size_t span = (size_t)std::max<int64_t>(tab.span, 1);
    FitInputs in;
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    // the state: accepted and trial constants, losses, gradients and flags; B (or S, Y, rho, count, head and a scratch vector), alpha, the
    // slope and the direction, two flags per tree; the images
    const bool h_hist = FitOutputs::on_host(history), h_acc = FitOutputs::on_host(n_accept), ring = memory > 0;
    Workspace ws;
    const auto cA = ws.place<char>(nu * es), cT = ws.place<char>(nu * es), lA = ws.place<char>(nt * es), lT = ws.place<char>(nt * es),
               dA = ws.place<char>(span * es), dT = ws.place<char>(span * es);
    ts.place(ws, es, true, false);
    const auto okA = ws.place<uint8_t>(nt), okT = ws.place<uint8_t>(nt), fresh = ws.place<uint8_t>(nt, !ring), produced = ws.place<uint8_t>(nt);
    const auto B = ws.place<double>((size_t)bspan), alpha = ws.place<double>(nt), slope = ws.place<double>(nt), dir = ws.place<double>(span),
               Yr = ws.place<double>((size_t)bspan, ring), rho = ws.place<double>(nt * (size_t)memory, ring), tmp = ws.place<double>(span, ring),
               r_hist = ws.place<double>(rows * nt, h_hist);
    const auto count = ws.place<int32_t>(nt, ring), head = ws.place<int32_t>(nt, ring), r_acc = ws.place<int32_t>(nt, h_acc);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    if (ts.on) ts.plan.bind(ts.dev, tab.joff, 0, &ts.a);
    FitOutputs out;
    out.from_state(loss, ws.ptr(lA), nt * es);
    out.from_state(ok, ws.ptr(okA), nt);
    double *hist = out.in_place(history, h_hist, ws.ptr(r_hist), rows * nt);
    BfgsArgs &a = q.x.b;
    a.n_trees = p->n_trees;
    a.n_grad = tab.ng;
    a.coff = tab.doff;
    a.consts_acc = ws.ptr(cA); a.loss_acc = ws.ptr(lA); a.dloss_acc = ws.ptr(dA); a.ok_acc = ws.ptr(okA);
    a.consts_trial = ws.ptr(cT); a.loss_trial = ws.ptr(lT); a.dloss_trial = ws.ptr(dT); a.ok_trial = ws.ptr(okT);
    a.alpha = ws.ptr(alpha); a.slope = ws.ptr(slope); a.p = ws.ptr(dir);
    a.produced = ws.ptr(produced);
    if (ring) {
        q.x.roff = tab.joff;
        q.x.S = ws.ptr(B); q.x.Y = ws.ptr(Yr); q.x.rho = ws.ptr(rho); q.x.tmp = ws.ptr(tmp);
        q.x.count = ws.ptr(count); q.x.head = ws.ptr(head);
        q.x.memory = memory;
    } else {
        a.boff = tab.joff;
        a.B = ws.ptr(B);
        a.fresh = ws.ptr(fresh);
    }
    a.step0 = o.step0; a.shrink = o.shrink; a.c1 = o.c1; a.curv = o.curv;
    a.n_accept = out.in_place(n_accept, h_acc, ws.ptr(r_acc), nt);
    const de_loss_spec_t spec = *spec_in;
    FitLoop f;
    f.consts_acc = a.consts_acc;
    f.consts_trial = a.consts_trial;
    f.evaluate = [&](bool trial) -> int {
        char *d = ws.ptr(trial ? dT : dA); // (tied: the occurrence rows land in a buffer of their own and are folded into d)
        const int rc1 = loss_grad_impl(c, p, in.Xd, N, ldX, in.pa, DE_GRAD_CONSTANT, in.yd, in.wd, &spec, ws.ptr(trial ? lT : lA),
                                       ts.on ? ws.ptr(ts.gO) : d, nullptr, ws.ptr(trial ? okT : okA), nullptr);
        if (rc1 != DE_OK || !ts.on) return rc1;
        HIP_TRY(c, launch_ties_fold(p->dtype, ts.a, ws.ptr(ts.gO), d, c->stream));
        return DE_OK;
    };
    f.init = [&]() -> int { HIP_TRY(c, q.init(p->dtype, c->stream)); return DE_OK; };
    f.first_history = f.fill_history = [&](double *row) -> int {
        HIP_TRY(c, launch_lm_history(p->dtype, a.loss_acc, p->n_trees, row, c->stream));
        return DE_OK;
    };
    f.propose = [&]() -> int { HIP_TRY(c, q.direction(p->dtype, c->stream)); return DE_OK; };
    f.accept = [&](double *row) -> int {
        a.history_row = row;
        HIP_TRY(c, q.accept(p->dtype, c->stream));
        return DE_OK;
    };
    ts.hook(c, p, ws, a.consts_acc, a.consts_trial, &f);
    if (ring) // de_fit_consts_lbfgs reports the fused loss alone at the accepted constants: what de_eval_loss_ex gives there, bit for bit
        f.report = [&]() -> int { return de_eval_loss_ex(c, p, in.Xd, N, ldX, in.pa, in.yd, in.wd, &spec, ws.ptr(lA), ws.ptr(okA)); };
    if ((rc = run_fit(c, p, o.iters, N > 0 && nc > 0, hist, f)) != DE_OK) return rc;
    return out.finish(c);
}
int de_fit_consts_bfgs_tied(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                            const void *w, const de_loss_spec_t *spec, const de_bfgs_opts_t *opts, const int32_t *tie, void *loss, uint8_t *ok,
                            double *history, int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_bfgs_tied");
    const de_bfgs_opts_t defaults{20, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_bfgs_opts_t o = opts ? *opts : defaults;
    DE_NOTHROW(c, fit_consts_qn_impl(c, p, "de_fit_consts_bfgs_tied", 0, o, bfgs_opts_problem(&o), X, N, ldX, pa, y, w, spec, loss, ok, history,
                                     n_accept, true, tie));
}
int de_fit_consts_lbfgs_tied(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                             const void *w, const de_loss_spec_t *spec, const de_lbfgs_opts_t *opts, const int32_t *tie, void *loss, uint8_t *ok,
                             double *history, int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lbfgs_tied");
    const de_lbfgs_opts_t defaults{20, 0, 8, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_lbfgs_opts_t lo = opts ? *opts : defaults;
    de_bfgs_opts_t o;
    const char *why = lbfgs_opts_problem(&lo, &o);
    char named[200]; // (the text names the call)
    if (why) std::snprintf(named, sizeof named, "de_fit_consts_lbfgs_tied: %s", why);
    DE_NOTHROW(c, fit_consts_qn_impl(c, p, "de_fit_consts_lbfgs_tied", lo.memory, o, why ? named : nullptr, X, N, ldX, pa, y, w, spec, loss, ok,
                                     history, n_accept, true, tie));
}
int de_fit_consts_bfgs(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                       const void *w, const de_loss_spec_t *spec, const de_bfgs_opts_t *opts, void *loss, uint8_t *ok, double *history,
                       int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_bfgs");
    const de_bfgs_opts_t defaults{20, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_bfgs_opts_t o = opts ? *opts : defaults;
    DE_NOTHROW(c, fit_consts_qn_impl(c, p, "de_fit_consts_bfgs", 0, o, bfgs_opts_problem(&o), X, N, ldX, pa, y, w, spec, loss, ok, history, n_accept));
}
int de_fit_consts_lbfgs(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                        const void *w, const de_loss_spec_t *spec, const de_lbfgs_opts_t *opts, void *loss, uint8_t *ok, double *history,
                        int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_lbfgs");
    const de_lbfgs_opts_t defaults{20, 0, 8, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_lbfgs_opts_t lo = opts ? *opts : defaults;
    de_bfgs_opts_t o;
    const char *why = lbfgs_opts_problem(&lo, &o);
    char named[200]; // (the text names the call)
    if (why) std::snprintf(named, sizeof named, "de_fit_consts_lbfgs: %s", why);
    DE_NOTHROW(c, fit_consts_qn_impl(c, p, "de_fit_consts_lbfgs", lo.memory, o, why ? named : nullptr, X, N, ldX, pa, y, w, spec, loss, ok, history,
                                     n_accept));
}

// ---- de_fit_consts_nm (kernels: de_nm.hip, arithmetic: de_nm.h) ----------------------------------------------------------
// The same fit with every evaluation de_eval_loss_ex's — the fused loss alone, no gradient program — and the kernels of de_nm.hip: one
// round is ask, the trial constants installed, one loss launch, tell.  No gradient rows: programs made by de_program_create_cse are served.
static int fit_consts_nm_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                              const void *w, const de_loss_spec_t *spec_in, const de_nm_opts_t *opts, void *loss, uint8_t *ok, double *history,
                              int32_t *n_improve, bool tied = false, const int32_t *tie = nullptr) {
    const char *what = tied ? "de_fit_consts_nm_tied" : "de_fit_consts_nm";
    const de_nm_opts_t defaults{200, 0, 0.025, 0.5, 0.0};
    const de_nm_opts_t o = opts ? *opts : defaults;
    const auto spec_check = [&]() -> int {
        char why[160];
        if (loss_spec_problem(spec_in, 0, why, sizeof why)) return fail(c, DE_ERR_INVALID_ARG, "%s", why);
        if (spec_in->kind == DE_LOSS_PULLBACK) return fail(c, DE_ERR_INVALID_ARG, "%s: DE_LOSS_PULLBACK is no objective", what);
        if (!p->threaded)
            return fail(c, DE_ERR_UNSUPPORTED, "%s needs the LDS-tiled kernel (feature matrix too wide for this build)", what);
        return DE_OK;
    };
    int rc = fit_check(c, p, what, "", spec_check, nm_opts_problem(&o), X, N, ldX, pa, {ok, y}, false);
    if (rc != DE_OK || p->n_trees == 0) return rc;
    TiedState ts; // (tied: ask and tell work on the unique constants)
    if (tied && (rc = ts.begin(c, p, what, tie)) != DE_OK) return rc;
    const int32_t *ng = ts.widths(p);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size(), rows = (size_t)o.iters + 1;
    const size_t nu = ts.on ? (size_t)ts.plan.nu : nc;
    std::vector<int64_t> voff(nt); // the simplex: (G + 1) G vertices and G + 1 losses of every tree that can be fitted, none of the others
    int64_t vspan = 0;
    for (size_t t = 0; t < nt; t++) {
        const int64_t g = ng[t];
        voff[t] = vspan;
        if (g >= 1 && g <= NM_MAX_ROWS) vspan += (g + 1) * (g + 1);
    }
    LmTables tab; // packed: the constants' offsets; the matrix offsets are the simplex's
    if ((rc = lm_tables(c, p->n_trees, ng, nullptr, voff.data(), &tab, 1, ts.on ? &ts.plan.blob : nullptr, &ts.dev)) != DE_OK) return rc;
    const size_t span = (size_t)std::max<int64_t>(tab.span, 1);
    FitInputs in;
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    // the state: accepted and trial constants, losses and flags; the simplex, c, xr, fr and three ints per tree; the images
    const bool h_hist = FitOutputs::on_host(history), h_imp = FitOutputs::on_host(n_improve);
    Workspace ws;
    const auto cA = ws.place<char>(nu * es), cT = ws.place<char>(nu * es), lA = ws.place<char>(nt * es), lT = ws.place<char>(nt * es);
    ts.place(ws, es, false, false);
    const auto okA = ws.place<uint8_t>(nt), okT = ws.place<uint8_t>(nt);
    const auto V = ws.place<double>((size_t)vspan), cen = ws.place<double>(span), xr = ws.place<double>(span), fr = ws.place<double>(nt),
               r_hist = ws.place<double>(rows * nt, h_hist);
    const auto st = ws.place<int32_t>(3 * nt), r_imp = ws.place<int32_t>(nt, h_imp);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    if (ts.on) ts.plan.bind(ts.dev, tab.joff, 0, &ts.a);
    FitOutputs out;
    out.from_state(loss, ws.ptr(lA), nt * es);
    out.from_state(ok, ws.ptr(okA), nt);
    double *hist = out.in_place(history, h_hist, ws.ptr(r_hist), rows * nt);
    NmArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = p->n_trees;
    a.n_grad = tab.ng;
    a.coff = tab.doff;
    a.voff = tab.joff;
    a.consts_acc = ws.ptr(cA); a.loss_acc = ws.ptr(lA); a.ok_acc = ws.ptr(okA);
    a.consts_trial = ws.ptr(cT); a.loss_trial = ws.ptr(lT); a.ok_trial = ws.ptr(okT);
    a.V = ws.ptr(V); a.c = ws.ptr(cen); a.xr = ws.ptr(xr); a.fr = ws.ptr(fr);
    a.st = ws.ptr(st);
    a.a = o.a; a.b = o.b; a.f_tol = o.f_tol;
    a.n_improve = out.in_place(n_improve, h_imp, ws.ptr(r_imp), nt);
    const de_loss_spec_t spec = *spec_in;
    FitLoop f;
    f.consts_acc = a.consts_acc;
    f.consts_trial = a.consts_trial;
    f.last_kernel = "de_nm_tell_kernel";
    f.evaluate = [&](bool trial) -> int {
        return de_eval_loss_ex(c, p, in.Xd, N, ldX, in.pa, in.yd, in.wd, &spec, ws.ptr(trial ? lT : lA), ws.ptr(trial ? okT : okA));
    };
    f.init = [&]() -> int {
        if (nc > 0) { // (the accepted constants are the kernel's V_0: it needs them before run_fit reads them for the loop)
            const int rc1 = de_program_get_consts(p, ts.on ? ws.ptr(ts.sA) : a.consts_acc);
            if (rc1 != DE_OK) return rc1;
            if (ts.on) HIP_TRY(c, launch_ties_pack(p->dtype, ts.a, ws.ptr(ts.sA), a.consts_acc, c->stream));
        }
        HIP_TRY(c, launch_nm_init(p->dtype, a, c->stream));
        return DE_OK;
    };
    f.first_history = f.fill_history = [&](double *row) -> int {
        HIP_TRY(c, launch_lm_history(p->dtype, a.loss_acc, p->n_trees, row, c->stream));
        return DE_OK;
    };
    f.propose = [&]() -> int { HIP_TRY(c, launch_nm_ask(p->dtype, a, c->stream)); return DE_OK; };
    f.accept = [&](double *row) -> int {
        a.history_row = row;
        HIP_TRY(c, launch_nm_tell(p->dtype, a, c->stream));
        return DE_OK;
    };
    ts.hook(c, p, ws, a.consts_acc, a.consts_trial, &f);
    if ((rc = run_fit(c, p, o.iters, N > 0 && nc > 0, hist, f)) != DE_OK) return rc;
    return out.finish(c);
}
int de_fit_consts_nm_tied(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                          const void *w, const de_loss_spec_t *spec, const de_nm_opts_t *opts, const int32_t *tie, void *loss, uint8_t *ok,
                          double *history, int32_t *n_improve) {
    DE_REFUSE_F16("de_fit_consts_nm_tied");
    DE_NOTHROW(c, fit_consts_nm_impl(c, p, X, N, ldX, pa, y, w, spec, opts, loss, ok, history, n_improve, true, tie));
}
int de_fit_consts_nm(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                     const void *w, const de_loss_spec_t *spec, const de_nm_opts_t *opts, void *loss, uint8_t *ok, double *history,
                     int32_t *n_improve) {
    DE_REFUSE_F16("de_fit_consts_nm");
    DE_NOTHROW(c, fit_consts_nm_impl(c, p, X, N, ldX, pa, y, w, spec, opts, loss, ok, history, n_improve));
}

// ---- de_fit_consts_bfgs_scaled / de_fit_consts_nm_scaled (kernels: de_fit_scaled.hip and those of de_bfgs.hip / de_nm.hip
// with a double objective; arithmetic: de_fit_scaled.h) ---------------------------------------------------------------------------------------
// de_fit_consts_bfgs's loop with every evaluation de_eval_fit_stats_grad's without a matrix (a FitPlan into the state) and the adapter kernel
// behind it: the loss slot takes scaled_sse and the gradient slots g, both doubles.  The statistics of the accepted constants are those of
// ONE more evaluation behind the loop (FitLoop::finish): it rewrites the accepted objective, gradient and flag with the same bits.
static int fit_consts_bfgs_scaled_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                                       const void *y, const void *w, const de_bfgs_opts_t *opts, double *sse, double *stats, double *ystats,
                                       uint8_t *ok, double *history, int32_t *n_accept) {
    const de_bfgs_opts_t defaults{20, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_bfgs_opts_t o = opts ? *opts : defaults;
    int rc = fit_check(c, p, "de_fit_consts_bfgs_scaled", "the caller sums them", nullptr, bfgs_opts_problem(&o), X, N, ldX, pa, {ok, sse, y});
    if (rc != DE_OK || p->n_trees == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size(), rows = (size_t)o.iters + 1;
    std::vector<int64_t> boff(nt); // B: G^2 doubles of every tree that is fitted, none of the others
    int64_t bspan = 0;
    for (size_t t = 0; t < nt; t++) {
        const int64_t g = p->n_consts_tree[t];
        boff[t] = bspan;
        if (g >= 1 && g <= BFGS_MAX_ROWS) bspan += g * g;
    }
    LmTables tab; // packed: dmom at 3 x the constants' offsets, the gradients at the constants' offsets; the matrix offsets are B's
    if ((rc = lm_tables(c, p->n_trees, p->n_consts_tree.data(), nullptr, boff.data(), &tab, 3)) != DE_OK) return rc;
    const size_t mspan = (size_t)std::max<int64_t>(tab.span, 1), span = std::max<size_t>(nc, 1);
    FitInputs in;
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    // the state: accepted and trial constants, objectives, gradients (doubles) and flags; the statistics and moments of both evaluations and
    // ystats; B, alpha, the slope and the direction, two flags per tree; the images
    const bool h_hist = FitOutputs::on_host(history), h_acc = FitOutputs::on_host(n_accept);
    Workspace ws;
    const auto cA = ws.place<char>(nc * es), cT = ws.place<char>(nc * es);
    const auto lA = ws.place<double>(nt), lT = ws.place<double>(nt), dA = ws.place<double>(span), dT = ws.place<double>(span),
               sA = ws.place<double>(nt * 3), sT = ws.place<double>(nt * 3), ys = ws.place<double>(3), mom = ws.place<double>(mspan);
    const auto okA = ws.place<uint8_t>(nt), okT = ws.place<uint8_t>(nt), fresh = ws.place<uint8_t>(nt), produced = ws.place<uint8_t>(nt);
    const auto B = ws.place<double>((size_t)bspan), alpha = ws.place<double>(nt), slope = ws.place<double>(nt), dir = ws.place<double>(span),
               r_hist = ws.place<double>(rows * nt, h_hist);
    const auto r_acc = ws.place<int32_t>(nt, h_acc);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    FitOutputs out;
    out.from_state(sse, ws.ptr(lA), nt * 8);
    out.from_state(stats, ws.ptr(sA), nt * 24);
    out.from_state(ystats, ws.ptr(ys), 24);
    out.from_state(ok, ws.ptr(okA), nt);
    double *hist = out.in_place(history, h_hist, ws.ptr(r_hist), rows * nt);
    BfgsArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = p->n_trees;
    a.n_grad = tab.ng;
    a.coff = tab.soff;
    a.boff = tab.joff;
    a.consts_acc = ws.ptr(cA); a.loss_acc = ws.ptr(lA); a.dloss_acc = ws.ptr(dA); a.ok_acc = ws.ptr(okA);
    a.consts_trial = ws.ptr(cT); a.loss_trial = ws.ptr(lT); a.dloss_trial = ws.ptr(dT); a.ok_trial = ws.ptr(okT);
    a.B = ws.ptr(B); a.alpha = ws.ptr(alpha); a.slope = ws.ptr(slope); a.p = ws.ptr(dir);
    a.fresh = ws.ptr(fresh); a.produced = ws.ptr(produced);
    a.step0 = o.step0; a.shrink = o.shrink; a.c1 = o.c1; a.curv = o.curv;
    a.n_accept = out.in_place(n_accept, h_acc, ws.ptr(r_acc), nt);
    FitScaledArgs s;
    std::memset(&s, 0, sizeof s);
    s.n_trees = p->n_trees;
    s.n_grad = tab.ng;
    s.moff = tab.doff;
    s.coff = tab.soff;
    s.ystats = ws.ptr(ys);
    s.dmom = ws.ptr(mom); // (one buffer: the adapter has consumed an evaluation's moments before the next one writes them)
    const de_loss_spec_t spec{DE_LOSS_L2, 0, 0.0};
    FitLoop f;
    f.consts_acc = a.consts_acc;
    f.consts_trial = a.consts_trial;
    f.last_kernel = "de_bfgs_accept_kernel";
    f.evaluate = [&](bool trial) -> int { // (ystats: the same three values every time)
        double *st = ws.ptr(trial ? sT : sA);
        const FitPlan fit{st, ws.ptr(ys), nullptr, nullptr};
        const int rc1 = loss_grad_impl(c, p, in.Xd, N, ldX, in.pa, DE_GRAD_CONSTANT, in.yd, in.wd, &spec, nullptr, ws.ptr(mom), nullptr,
                                       ws.ptr(trial ? okT : okA), nullptr, false, nullptr, &fit);
        if (rc1 != DE_OK) return rc1;
        s.stats = st;
        s.sse = ws.ptr(trial ? lT : lA);
        s.grad = ws.ptr(trial ? dT : dA);
        HIP_TRY(c, launch_fit_scaled_objective(s, c->stream));
        return DE_OK;
    };
    f.init = [&]() -> int { HIP_TRY(c, launch_bfgs_init(p->dtype, a, c->stream, true)); return DE_OK; };
    f.first_history = f.fill_history = [&](double *row) -> int {
        HIP_TRY(c, launch_lm_history(DE_F64, a.loss_acc, p->n_trees, row, c->stream));
        return DE_OK;
    };
    f.propose = [&]() -> int { HIP_TRY(c, launch_bfgs_direction(p->dtype, a, c->stream, true)); return DE_OK; };
    f.accept = [&](double *row) -> int {
        a.history_row = row;
        HIP_TRY(c, launch_bfgs_accept(p->dtype, a, c->stream, true));
        return DE_OK;
    };
    f.finish = [&]() -> int { // the statistics at the accepted constants, which the program holds now
        const int rc1 = f.evaluate(false);
        c->last_kernel = f.last_kernel;
        return rc1;
    };
    if ((rc = run_fit(c, p, o.iters, N > 0 && nc > 0, hist, f)) != DE_OK) return rc;
    return out.finish(c);
}
int de_fit_consts_bfgs_scaled(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                              const void *w, const de_bfgs_opts_t *opts, double *sse, double *stats, double *ystats, uint8_t *ok,
                              double *history, int32_t *n_accept) {
    DE_REFUSE_F16("de_fit_consts_bfgs_scaled");
    DE_NOTHROW(c, fit_consts_bfgs_scaled_impl(c, p, X, N, ldX, pa, y, w, opts, sse, stats, ystats, ok, history, n_accept));
}

// de_fit_consts_nm's loop with every evaluation de_eval_fit_stats's and the adapter kernel behind it (the objective alone: no gradient
// rows, so programs made by de_program_create_cse are served).  The statistics of the accepted constants: as above, one more evaluation.
static int fit_consts_nm_scaled_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                                     const void *y, const void *w, const de_nm_opts_t *opts, double *sse, double *stats, double *ystats,
                                     uint8_t *ok, double *history, int32_t *n_improve) {
    const de_nm_opts_t defaults{200, 0, 0.025, 0.5, 0.0};
    const de_nm_opts_t o = opts ? *opts : defaults;
    const auto spec_check = [&]() -> int {
        if (!p->threaded)
            return fail(c, DE_ERR_UNSUPPORTED, "de_fit_consts_nm_scaled needs the LDS-tiled kernel (feature matrix too wide for this build)");
        return DE_OK;
    };
    int rc = fit_check(c, p, "de_fit_consts_nm_scaled", "", spec_check, nm_opts_problem(&o), X, N, ldX, pa, {ok, sse, y}, false);
    if (rc != DE_OK || p->n_trees == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size(), rows = (size_t)o.iters + 1;
    std::vector<int64_t> voff(nt); // the simplex: (G + 1) G vertices and G + 1 losses of every tree that can be fitted, none of the others
    int64_t vspan = 0;
    for (size_t t = 0; t < nt; t++) {
        const int64_t g = p->n_consts_tree[t];
        voff[t] = vspan;
        if (g >= 1 && g <= NM_MAX_ROWS) vspan += (g + 1) * (g + 1);
    }
    LmTables tab; // packed: the constants' offsets; the matrix offsets are the simplex's
    if ((rc = lm_tables(c, p->n_trees, p->n_consts_tree.data(), nullptr, voff.data(), &tab)) != DE_OK) return rc;
    const size_t span = (size_t)std::max<int64_t>(tab.span, 1);
    FitInputs in;
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    // the state: accepted and trial constants, objectives (doubles) and flags; the statistics of both evaluations and ystats; the simplex, c,
    // xr, fr and three ints per tree; the images
    const bool h_hist = FitOutputs::on_host(history), h_imp = FitOutputs::on_host(n_improve);
    Workspace ws;
    const auto cA = ws.place<char>(nc * es), cT = ws.place<char>(nc * es);
    const auto lA = ws.place<double>(nt), lT = ws.place<double>(nt), sA = ws.place<double>(nt * 3), sT = ws.place<double>(nt * 3),
               ys = ws.place<double>(3);
    const auto okA = ws.place<uint8_t>(nt), okT = ws.place<uint8_t>(nt);
    const auto V = ws.place<double>((size_t)vspan), cen = ws.place<double>(span), xr = ws.place<double>(span), fr = ws.place<double>(nt),
               r_hist = ws.place<double>(rows * nt, h_hist);
    const auto st = ws.place<int32_t>(3 * nt), r_imp = ws.place<int32_t>(nt, h_imp);
    if ((rc = ws.reserve(c, c->sLm)) != DE_OK) return rc;
    FitOutputs out;
    out.from_state(sse, ws.ptr(lA), nt * 8);
    out.from_state(stats, ws.ptr(sA), nt * 24);
    out.from_state(ystats, ws.ptr(ys), 24);
    out.from_state(ok, ws.ptr(okA), nt);
    double *hist = out.in_place(history, h_hist, ws.ptr(r_hist), rows * nt);
    NmArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = p->n_trees;
    a.n_grad = tab.ng;
    a.coff = tab.doff;
    a.voff = tab.joff;
    a.consts_acc = ws.ptr(cA); a.loss_acc = ws.ptr(lA); a.ok_acc = ws.ptr(okA);
    a.consts_trial = ws.ptr(cT); a.loss_trial = ws.ptr(lT); a.ok_trial = ws.ptr(okT);
    a.V = ws.ptr(V); a.c = ws.ptr(cen); a.xr = ws.ptr(xr); a.fr = ws.ptr(fr);
    a.st = ws.ptr(st);
    a.a = o.a; a.b = o.b; a.f_tol = o.f_tol;
    a.n_improve = out.in_place(n_improve, h_imp, ws.ptr(r_imp), nt);
    FitScaledArgs s;
    std::memset(&s, 0, sizeof s);
    s.n_trees = p->n_trees;
    s.n_grad = tab.ng;
    s.ystats = ws.ptr(ys);
    FitLoop f;
    f.consts_acc = a.consts_acc;
    f.consts_trial = a.consts_trial;
    f.last_kernel = "de_nm_tell_kernel";
    f.evaluate = [&](bool trial) -> int { // (ystats: the same three values every time)
        double *sts = ws.ptr(trial ? sT : sA);
        const int rc1 = de_eval_fit_stats(c, p, in.Xd, N, ldX, in.pa, in.yd, in.wd, sts, ws.ptr(ys), ws.ptr(trial ? okT : okA));
        if (rc1 != DE_OK) return rc1;
        s.stats = sts;
        s.sse = ws.ptr(trial ? lT : lA);
        HIP_TRY(c, launch_fit_scaled_objective(s, c->stream));
        return DE_OK;
    };
    f.init = [&]() -> int {
        if (nc > 0) { // (the accepted constants are the kernel's V_0: it needs them before run_fit reads them for the loop)
            const int rc1 = de_program_get_consts(p, a.consts_acc);
            if (rc1 != DE_OK) return rc1;
        }
        HIP_TRY(c, launch_nm_init(p->dtype, a, c->stream, true));
        return DE_OK;
    };
    f.first_history = f.fill_history = [&](double *row) -> int {
        HIP_TRY(c, launch_lm_history(DE_F64, a.loss_acc, p->n_trees, row, c->stream));
        return DE_OK;
    };
    f.propose = [&]() -> int { HIP_TRY(c, launch_nm_ask(p->dtype, a, c->stream, true)); return DE_OK; };
    f.accept = [&](double *row) -> int {
        a.history_row = row;
        HIP_TRY(c, launch_nm_tell(p->dtype, a, c->stream, true));
        return DE_OK;
    };
    f.finish = [&]() -> int { // the statistics at the accepted constants, which the program holds now
        const int rc1 = f.evaluate(false);
        c->last_kernel = f.last_kernel;
        return rc1;
    };
    if ((rc = run_fit(c, p, o.iters, N > 0 && nc > 0, hist, f)) != DE_OK) return rc;
    return out.finish(c);
}
int de_fit_consts_nm_scaled(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, const void *y,
                            const void *w, const de_nm_opts_t *opts, double *sse, double *stats, double *ystats, uint8_t *ok,
                            double *history, int32_t *n_improve) {
    DE_REFUSE_F16("de_fit_consts_nm_scaled");
    DE_NOTHROW(c, fit_consts_nm_scaled_impl(c, p, X, N, ldX, pa, y, w, opts, sse, stats, ystats, ok, history, n_improve));
}

} // extern "C"
