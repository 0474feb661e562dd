// de_api_tree_params.cpp — C ABI (include/de_hip.h): de_tape_params_to_consts, de_eval_tree_params, de_eval_loss_tree_params,
// de_eval_loss_grad_tree_params and the host-only hook de_tree_params_accumulate_host.  A population whose trees
// each own their parameter matrix is an ordinary program in which some constant slots stand for parameters; a call serves it one class
// segment at a time: the class's constant vector is formed and installed on the device (de_program_set_consts_device), the model entry
// point runs on the class's sample range, and the per-tree results are added in double (kernels: de_tree_params.hip, arithmetic:
// de_tree_params.h).  No existing kernel, record format or lowering pass is involved.
// ... and de_fit_tree_params_bfgs with its host-only hooks de_tree_params_pack_host / de_tree_params_unpack_host: BFGS
// over each tree's vcat(constants, parameters[:]) with that class loop as the evaluator (kernels: de_bfgs.hip unchanged on packed
// vectors, the pack / unpack kernels of de_tree_params.hip; index map: de_tree_params_fit.h).
// ... and de_fit_tree_params_lbfgs: the same loop with the kernels of de_lbfgs.hip, for trees of more than 32 unknowns.
#include "de_api_internal.h"
#include "de_tree_params_dev.h"
#include "de_tree_params.h"
#include "de_tree_params_fit.h"
#include "de_bfgs.h"
#include "de_bfgs_dev.h"
#include "de_lbfgs_dev.h"
#include "de_lm.h"

template <typename T>
static void accumulate_host(int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes, const uint8_t *class_used,
                            const T *loss_c, const T *dloss_c, const uint8_t *ok_c, T *loss, T *dloss, T *dparams, uint8_t *ok) {
    // the launches of one call, for one tree: accumulate per used class (ascending), then finish
    double acc_loss = 0.0;
    uint8_t acc_ok = 1;
    std::vector<double> acc_dl((size_t)n_slots, 0.0), acc_dp((size_t)(n_classes * n_params), 0.0);
    for (int64_t c = 0; c < n_classes; c++) {
        if (!class_used[c]) continue;
        acc_loss = tp_add(acc_loss, loss_c[c]);
        acc_ok = (acc_ok && ok_c[c]) ? 1 : 0;
        const T *d = dloss_c + c * n_slots;
        for (int32_t s = 0; s < n_slots; s++) acc_dl[(size_t)s] = tp_add(acc_dl[(size_t)s], d[s]);
        for (int32_t p = 0; p < n_params; p++) acc_dp[(size_t)(c * n_params + p)] = tp_cell(d, slot_param, n_slots, p);
    }
    *ok = acc_ok;
    *loss = tp_finish<T>(acc_loss, acc_ok);
    for (int32_t s = 0; s < n_slots; s++) dloss[s] = tp_finish<T>(acc_dl[(size_t)s], acc_ok);
    for (int64_t j = 0; j < n_classes * n_params; j++) dparams[j] = tp_finish<T>(acc_dp[(size_t)j], acc_ok);
}

// one tree's unknowns gathered from / scattered to (slot values, its parameter block): the table and the copies the kernels run
template <typename T>
static void pack_host(bool unpack, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes, int64_t ld, T *slots,
                      T *cells, T *x) {
    std::vector<int64_t> map((size_t)tpf_unknowns(n_slots, n_params, n_classes));
    const int64_t G = tpf_map_tree(n_slots, slot_param, n_params, n_classes, 0, 0, map.data());
    for (int64_t u = 0; u < G; u++) {
        if (unpack) tpf_store(map[(size_t)u], x[u], slots, cells, n_params, ld);
        else x[u] = tpf_load(map[(size_t)u], static_cast<const T *>(slots), static_cast<const T *>(cells), n_params, ld);
    }
}

// the shared body of de_tree_params_pack_host / de_tree_params_unpack_host: G, or -status with nothing written
static int pack_host_checked(bool unpack, int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes,
                             int64_t ld, void *slots, void *cells, void *x) {
    if ((dtype != DE_F32 && dtype != DE_F64) || n_slots < 0 || n_params < 0 || n_classes < 0 || n_classes > INT32_MAX || ld < n_params)
        return -DE_ERR_INVALID_ARG;
    if (n_slots > 0 && !slot_param) return -DE_ERR_INVALID_ARG;
    int64_t n_real = 0;
    for (int32_t s = 0; s < n_slots; s++) {
        if (slot_param[s] < -1 || slot_param[s] >= n_params) return -DE_ERR_INVALID_ARG;
        n_real += slot_param[s] < 0 ? 1 : 0;
    }
    const int64_t G = tpf_unknowns(n_real, n_params, n_classes);
    if (G > INT32_MAX) return -DE_ERR_INVALID_ARG;
    if ((n_real > 0 && !slots) || ((int64_t)n_params * n_classes > 0 && !cells) || (G > 0 && !x)) return -DE_ERR_INVALID_ARG;
    try {
        if (dtype == DE_F32)
            pack_host<float>(unpack, n_slots, slot_param, n_params, n_classes, ld, static_cast<float *>(slots), static_cast<float *>(cells),
                             static_cast<float *>(x));
        else
            pack_host<double>(unpack, n_slots, slot_param, n_params, n_classes, ld, static_cast<double *>(slots), static_cast<double *>(cells),
                              static_cast<double *>(x));
    } catch (...) { return -DE_ERR_HIP; }
    return (int)G;
}

extern "C" {

int de_tree_params_pack_host(int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes, int64_t ld_params,
                             const void *slot_values, const void *params_tree, void *x) {
    return pack_host_checked(false, dtype, n_slots, slot_param, n_params, n_classes, ld_params, const_cast<void *>(slot_values),
                             const_cast<void *>(params_tree), x);
}
int de_tree_params_unpack_host(int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes, int64_t ld_params,
                               const void *x, void *slot_values, void *params_tree) {
    const int g = pack_host_checked(true, dtype, n_slots, slot_param, n_params, n_classes, ld_params, slot_values, params_tree,
                                    const_cast<void *>(x));
    return g < 0 ? -g : DE_OK;
}

int64_t de_tape_params_to_consts(const de_tape_node_t *nodes, int64_t n_nodes, int32_t n_params, de_tape_node_t *out_nodes,
                                 int32_t *slot_param, int64_t cap) {
    if (n_nodes < 0 || cap < 0 || n_params < 0 || (n_nodes > 0 && (!nodes || !out_nodes))) return -DE_ERR_INVALID_ARG;
    // everything is checked before anything is written: out_nodes may be `nodes`
    int64_t n_slots = 0;
    for (int64_t i = 0; i < n_nodes; i++) {
        const de_tape_node_t &nd = nodes[i];
        if (nd.degree == 0) {
            if (nd.op == DE_LEAF_SHARED) return -DE_ERR_UNSUPPORTED;
            if (nd.op == DE_LEAF_PARAM && (int32_t)nd.arg >= n_params) return -DE_ERR_OUT_OF_RANGE;
            if (nd.op == DE_LEAF_CONST || nd.op == DE_LEAF_PARAM) n_slots++;
        } else if (nd.op == DE_OP_SHARE) return -DE_ERR_UNSUPPORTED;
    }
    if (n_slots > cap || n_slots > 65535 || (n_slots > 0 && !slot_param)) return -DE_ERR_INVALID_ARG;
    int64_t s = 0;
    for (int64_t i = 0; i < n_nodes; i++) {
        de_tape_node_t nd = nodes[i];
        if (nd.degree == 0 && (nd.op == DE_LEAF_CONST || nd.op == DE_LEAF_PARAM)) {
            slot_param[s] = nd.op == DE_LEAF_PARAM ? (int32_t)nd.arg : -1;
            nd.op = DE_LEAF_CONST;
            nd.arg = (uint16_t)s++;
        }
        out_nodes[i] = nd;
    }
    return n_slots;
}

int de_tree_params_accumulate_host(int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes,
                                   const uint8_t *class_used, const void *loss_c, const void *dloss_c, const uint8_t *ok_c,
                                   void *loss, void *dloss, void *dparams, uint8_t *ok) {
    if ((dtype != DE_F32 && dtype != DE_F64) || n_slots < 0 || n_params < 0 || n_classes < 0) return DE_ERR_INVALID_ARG;
    if (!loss || !ok || (n_classes > 0 && (!class_used || !loss_c || !ok_c))) return DE_ERR_INVALID_ARG;
    if (n_slots > 0 && (!slot_param || !dloss || (n_classes > 0 && !dloss_c))) return DE_ERR_INVALID_ARG;
    if (n_classes * n_params > 0 && !dparams) return DE_ERR_INVALID_ARG;
    try {
        if (dtype == DE_F32)
            accumulate_host<float>(n_slots, slot_param, n_params, n_classes, class_used, static_cast<const float *>(loss_c),
                                   static_cast<const float *>(dloss_c), ok_c, static_cast<float *>(loss), static_cast<float *>(dloss),
                                   static_cast<float *>(dparams), ok);
        else
            accumulate_host<double>(n_slots, slot_param, n_params, n_classes, class_used, static_cast<const double *>(loss_c),
                                    static_cast<const double *>(dloss_c), ok_c, static_cast<double *>(loss), static_cast<double *>(dloss),
                                    static_cast<double *>(dparams), ok);
    } catch (...) { return DE_ERR_HIP; }
    return DE_OK;
}

enum TpModel { TP_EVAL, TP_LOSS, TP_LOSS_GRAD };
struct TpOut { // what the model returns
    void *out = nullptr;
    int64_t ld_out = 0;
    const void *y = nullptr, *w = nullptr;
    const de_loss_spec_t *spec = nullptr;
    void *loss = nullptr, *dloss = nullptr, *dparams = nullptr;
    const int64_t *dloss_offsets = nullptr;
    bool fit = false; // de_fit_tree_params_bfgs: loss, dloss, dparams and ok are buffers of the pool, set per evaluation
};
struct TpPlan { // a call that passed every refusal
    size_t nt = 0, nc = 0, es = 4;
    int64_t C = 0, span = 1;
    int32_t P = 0;
    bool any_param = false, grad = false;
    std::vector<int64_t> doff;
};
struct TpDev { // what a call holds on the device: one pooled allocation and the staged inputs
    TreeParamsArgs a;
    char *pool = nullptr;
    void *base = nullptr;  // the base vector (a.base)
    void *lc = nullptr, *dc = nullptr; // one class's loss / dloss
    uint8_t *okc = nullptr;
    size_t o_acc = 0, acc_bytes = 0, o_fit_tab = 0, o_fit = 0;
    Staged sX, sY, sW, sPar;
    bool h_ok = false, h_loss = false, h_dl = false, h_dp = false, h_out = false;
    size_t n_dp = 0;
};

static size_t tp_place(size_t *at, size_t bytes) { // 16-byte aligned pieces of one pooled allocation
    const size_t o = *at;
    *at = o + ((bytes + 15) & ~(size_t)15);
    return o;
}

// every refusal of the three entry points (and the fit's, which adds its own): nothing has been touched when it returns an error
static int tp_check(de_ctx_t *c, de_program_t *p, const char *what, TpModel model, const void *X, int64_t N, int64_t ldX,
                    const de_tree_params_t *tp, const TpOut &o, uint8_t *ok, TpPlan *pl) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    // ---- refusals: before any output or constant is touched ----
    if (p->io == DE_F16 || is_complex_io(p->io))
        return fail(c, DE_ERR_UNSUPPORTED, "%s: DE_F16 and complex programs are not served (DE_F32 / DE_F64 only)", what);
    if (!p->in_cse.empty()) return fail(c, DE_ERR_UNSUPPORTED, "%s: programs made by de_program_create_cse are not served", what);
    if (p->n_params != 0)
        return fail(c, DE_ERR_UNSUPPORTED, "%s: the program has n_params = %d; it takes tapes rewritten by de_tape_params_to_consts (n_params = 0)",
                    what, (int)p->n_params);
    const size_t nt = (size_t)p->n_trees, nc = p->consts.size();
    if (!tp || !tp->class_starts) return fail(c, DE_ERR_INVALID_ARG, "%s: null de_tree_params_t / class_starts", what);
    if (tp->reserved != 0) return fail(c, DE_ERR_INVALID_ARG, "de_tree_params_t: reserved must be 0");
    if (tp->n_params < 0 || tp->n_classes <= 0) return fail(c, DE_ERR_INVALID_ARG, "de_tree_params_t: n_params < 0 or n_classes <= 0");
    if (tp->ld_params < tp->n_params) return fail(c, DE_ERR_INVALID_ARG, "de_tree_params_t: ld_params < n_params");
    if (nc > 0 && !tp->slot_param) return fail(c, DE_ERR_INVALID_ARG, "de_tree_params_t: slot_param is null on a program with constants");
    if (N < 0 || !ok) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    const int64_t C = tp->n_classes;
    const int32_t P = tp->n_params;
    if (tp->class_starts[0] != 0 || tp->class_starts[C] != N) return fail(c, DE_ERR_INVALID_ARG, "class_starts must run from 0 to N");
    for (int64_t k = 0; k < C; k++)
        if (tp->class_starts[k + 1] < tp->class_starts[k]) return fail(c, DE_ERR_INVALID_ARG, "class_starts must be non-decreasing");
    bool any_param = false;
    for (size_t s = 0; s < nc; s++) {
        if (tp->slot_param[s] < -1 || tp->slot_param[s] >= P)
            return fail(c, DE_ERR_INVALID_ARG, "de_tree_params_t: slot_param[%lld] = %d outside [-1, %d)", (long long)s, (int)tp->slot_param[s], (int)P);
        any_param = any_param || tp->slot_param[s] >= 0;
    }
    if (any_param && !tp->params) return fail(c, DE_ERR_INVALID_ARG, "de_tree_params_t: params is null");
    if (ldX < p->n_features) return fail(c, DE_ERR_INVALID_ARG, "ldX < n_features");
    // ... and what the model entry point refuses
    char why[160];
    if (model == TP_EVAL) {
        if (nt > 0 && N > 0 && (!X || !o.out)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
        if (o.ld_out < N) return fail(c, DE_ERR_INVALID_ARG, "ld_out < N");
    } else {
        if (nt > 0 && N > 0 && (!X || !o.y)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
        if (model == TP_LOSS && nt > 0 && !o.loss) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
        if (model == TP_LOSS_GRAD && nt > 0 && !o.fit && (!o.dloss || !o.dparams)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
        if (loss_spec_problem(o.spec, model == TP_LOSS_GRAD ? 1 : 0, why, sizeof why)) return fail(c, DE_ERR_INVALID_ARG, "%s", why);
        if (model == TP_LOSS && !p->threaded)
            return fail(c, DE_ERR_UNSUPPORTED, "de_eval_loss needs the LDS-tiled kernel (feature matrix too wide for this build)");
    }
    const bool grad = model == TP_LOSS_GRAD;
    std::vector<int64_t> doff(nt);
    int64_t span = 0;
    for (size_t t = 0; t < nt; t++) {
        const int64_t g = p->const_off[t + 1] - p->const_off[t];
        if (grad && de_program_n_grad(p, (int64_t)t, DE_GRAD_CONSTANT) != g)
            return fail(c, DE_ERR_UNSUPPORTED, "%s: tree %lld has %lld constant rows for %lld constants", what, (long long)t,
                        (long long)de_program_n_grad(p, (int64_t)t, DE_GRAD_CONSTANT), (long long)g);
        const int64_t off = o.dloss_offsets ? o.dloss_offsets[t] : p->const_off[t];
        if (off < 0) return fail(c, DE_ERR_INVALID_ARG, "negative dloss offset");
        doff[t] = off;
        span = std::max(span, off + g);
    }
    pl->nt = nt; pl->nc = nc; pl->es = p->dtype == DE_F32 ? 4 : 8;
    pl->C = C; pl->P = P; pl->span = std::max<int64_t>(span, 1);
    pl->any_param = any_param; pl->grad = grad;
    pl->doff = std::move(doff);
    return DE_OK;
}

// The pooled allocation, the tables and the staged host inputs of a checked call (n_trees > 0).  `fit_tab` (may be null) is uploaded
// behind the call's own tables, at d->o_fit_tab; `fit_bytes` more bytes of the pool start at d->o_fit.  The stream is idle afterwards.
static int tp_setup(de_ctx_t *c, de_program_t *p, TpModel model, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                    const TpOut &o, uint8_t *ok, const TpPlan &pl, const std::vector<unsigned char> *fit_tab, size_t fit_bytes, TpDev *d) {
    const size_t nt = pl.nt, nc = pl.nc, es = pl.es;
    const int64_t C = pl.C, span = pl.span;
    const int32_t P = pl.P;
    const bool grad = pl.grad, any_param = pl.any_param;
    const std::vector<int64_t> &doff = pl.doff;
    HIP_TRY(c, hipSetDevice(c->device));

    // ---- one pooled allocation: tables, the two constant vectors, one class's results, the accumulators, images of host outputs ----
    const size_t n_dp = grad ? nt * (size_t)C * (size_t)P : 0;
    const bool h_ok = !o.fit && !is_device_ptr(ok), h_loss = o.loss && !is_device_ptr(o.loss), h_dl = grad && !o.fit && !is_device_ptr(o.dloss),
               h_dp = grad && !o.fit && n_dp > 0 && !is_device_ptr(o.dparams), h_out = model == TP_EVAL && N > 0 && !is_device_ptr(o.out);
    size_t at = 0;
    const size_t o_stree = tp_place(&at, nc * 4), o_sparam = tp_place(&at, nc * 4), o_coff = tp_place(&at, (nt + 1) * 8), o_doff = tp_place(&at, nt * 8);
    const size_t o_fit_tab = tp_place(&at, fit_tab ? fit_tab->size() : 0);
    const size_t tab_bytes = at;
    const size_t o_base = tp_place(&at, nc * es), o_cvec = tp_place(&at, nc * es), o_lc = tp_place(&at, nt * es),
                 o_dc = tp_place(&at, grad ? (size_t)span * es : 0), o_okc = tp_place(&at, nt);
    const size_t o_acc = at; // the accumulators are cleared together
    const size_t o_al = tp_place(&at, nt * 8), o_ad = tp_place(&at, grad ? nc * 8 : 0), o_ap = tp_place(&at, n_dp * 8);
    const size_t acc_bytes = at - o_acc;
    const size_t o_aok = tp_place(&at, nt);
    const size_t o_hok = h_ok ? tp_place(&at, nt) : 0, o_hl = h_loss ? tp_place(&at, nt * es) : 0,
                 o_hd = h_dl ? tp_place(&at, (size_t)span * es) : 0, o_hp = h_dp ? tp_place(&at, n_dp * es) : 0;
    const size_t o_fit = tp_place(&at, fit_bytes);
    if (at > c->sTp.cap) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (growing frees what queued work may still use)
    HIP_TRY(c, c->sTp.reserve(at));
    char *base = static_cast<char *>(c->sTp.p);

    std::vector<unsigned char> tab(tab_bytes, 0);
    if (fit_tab && !fit_tab->empty()) std::memcpy(tab.data() + o_fit_tab, fit_tab->data(), fit_tab->size());
    {
        int32_t *st = reinterpret_cast<int32_t *>(tab.data() + o_stree), *sp = reinterpret_cast<int32_t *>(tab.data() + o_sparam);
        int64_t *co = reinterpret_cast<int64_t *>(tab.data() + o_coff), *dof = reinterpret_cast<int64_t *>(tab.data() + o_doff);
        for (size_t t = 0; t < nt; t++) {
            co[t] = p->const_off[t];
            dof[t] = doff[t];
            for (int64_t s = p->const_off[t]; s < p->const_off[t + 1]; s++) st[s] = (int32_t)t;
        }
        co[nt] = p->const_off[nt];
        for (size_t s = 0; s < nc; s++) sp[s] = tp->slot_param[s];
    }
    HIP_TRY(c, hipMemcpyAsync(base, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    // host inputs are staged once for the whole call, into the buffers a single model call would stage them in
    Staged &sX = d->sX, &sY = d->sY, &sW = d->sW, &sPar = d->sPar;
    int rc = DE_OK;
    if (N > 0) {
        if ((rc = stage_in(c, c->sX, X, (size_t)ldX * (size_t)N * es, &sX))) return rc;
        if (o.y && (rc = stage_in(c, c->sY, o.y, (size_t)N * es, &sY))) return rc;
        if (o.w && (rc = stage_in(c, c->sW, o.w, (size_t)N * es, &sW))) return rc;
        // (the fit reads and writes a parameter block of its own in the pool)
        if (any_param && !o.fit && (rc = stage_in(c, c->sParams, tp->params, (size_t)tp->ld_params * (size_t)C * nt * es, &sPar))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the tables and the staged inputs come from pageable memory)

    TreeParamsArgs &a = d->a;
    std::memset(&a, 0, sizeof a);
    a.n_trees = p->n_trees; a.n_consts = (int64_t)nc; a.n_classes = C; a.ld_params = tp->ld_params; a.n_params = P;
    a.slot_tree = reinterpret_cast<const int32_t *>(base + o_stree); a.slot_param = reinterpret_cast<const int32_t *>(base + o_sparam);
    a.coff = reinterpret_cast<const int64_t *>(base + o_coff); a.doff = reinterpret_cast<const int64_t *>(base + o_doff);
    a.base = base + o_base; a.params = sPar.dev; a.cvec = base + o_cvec;
    a.loss_c = model == TP_EVAL ? nullptr : base + o_lc;
    a.dloss_c = grad ? base + o_dc : nullptr;
    a.ok_c = reinterpret_cast<const uint8_t *>(base + o_okc);
    a.acc_loss = reinterpret_cast<double *>(base + o_al); a.acc_dloss = reinterpret_cast<double *>(base + o_ad);
    a.acc_dparams = reinterpret_cast<double *>(base + o_ap); a.acc_ok = reinterpret_cast<uint8_t *>(base + o_aok);
    a.loss = model == TP_EVAL || !o.loss ? nullptr : (h_loss ? static_cast<void *>(base + o_hl) : o.loss);
    a.dloss = grad ? (h_dl ? static_cast<void *>(base + o_hd) : o.dloss) : nullptr;
    a.dparams = grad ? (h_dp ? static_cast<void *>(base + o_hp) : o.dparams) : nullptr;
    a.ok = h_ok ? reinterpret_cast<uint8_t *>(base + o_hok) : ok;
    d->pool = base; d->base = base + o_base; d->lc = base + o_lc; d->dc = base + o_dc; d->okc = reinterpret_cast<uint8_t *>(base + o_okc);
    d->o_acc = o_acc; d->acc_bytes = acc_bytes; d->o_fit_tab = o_fit_tab; d->o_fit = o_fit;
    d->h_ok = h_ok; d->h_loss = h_loss; d->h_dl = h_dl; d->h_dp = h_dp; d->h_out = h_out; d->n_dp = n_dp;
    return DE_OK;
}

// The class loop of one evaluation: the accumulators cleared, then every class with a sample, ascending — scatter (base values in real
// slots, the class's column of a.params in parameter slots), the vector installed, the model entry point on the class's range, the
// accumulate launch.  Everything it reads is on the device already: it queues work on the context's stream and never waits for it, so
// de_fit_tree_params_bfgs runs it once per trial.  *patched: the program no longer holds the base vector (also when the loop fails).  The
// caller sets the program's constants back and launches the finish kernel.
static int tp_run_classes(de_ctx_t *c, de_program_t *p, TpModel model, const TpPlan &pl, TpDev &d, const int64_t *class_starts, int64_t ldX,
                          const TpOut &o, void *out_dev, int64_t ld_dev, bool *patched) {
    TreeParamsArgs &a = d.a;
    const size_t es = pl.es;
    HIP_TRY(c, hipMemsetAsync(d.pool + d.o_acc, 0, d.acc_bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(a.acc_ok, 1, pl.nt, c->stream));
    if (pl.grad) HIP_TRY(c, hipMemsetAsync(d.dc, 0, (size_t)pl.span * es, c->stream)); // (entries no tree owns are never read)
    int rc = DE_OK;
    for (int64_t k = 0; k < pl.C && rc == DE_OK; k++) {
        const int64_t j0 = class_starts[k], n = class_starts[k + 1] - j0;
        if (n <= 0) continue; // a class without samples: its columns are never read
        a.cls = k;
        if (pl.any_param) {
            HIP_TRY(c, launch_tree_params_scatter(p->dtype, a, c->stream));
            *patched = true;
            rc = set_consts_device_impl(p, a.cvec);
            if (rc != DE_OK) break;
        }
        const char *Xk = static_cast<const char *>(d.sX.dev) + (size_t)j0 * (size_t)ldX * es;
        const char *yk = o.y ? static_cast<const char *>(d.sY.dev) + (size_t)j0 * es : nullptr;
        const char *wk = o.w ? static_cast<const char *>(d.sW.dev) + (size_t)j0 * es : nullptr;
        if (model == TP_EVAL) rc = de_eval(c, p, Xk, n, ldX, nullptr, static_cast<char *>(out_dev) + (size_t)j0 * es, ld_dev, d.okc);
        else if (model == TP_LOSS) rc = de_eval_loss_ex(c, p, Xk, n, ldX, nullptr, yk, wk, o.spec, d.lc, d.okc);
        else rc = de_eval_loss_grad_ex(c, p, Xk, n, ldX, nullptr, DE_GRAD_CONSTANT, yk, wk, o.spec, d.lc, d.dc, o.dloss_offsets, d.okc);
        if (rc != DE_OK) break;
        HIP_TRY(c, launch_tree_params_accumulate(p->dtype, a, c->stream));
    }
    return rc;
}

static int tree_params_impl(de_ctx_t *c, de_program_t *p, const char *what, TpModel model, const void *X, int64_t N, int64_t ldX,
                            const de_tree_params_t *tp, const TpOut &o, uint8_t *ok) {
    TpPlan pl;
    int rc = tp_check(c, p, what, model, X, N, ldX, tp, o, ok, &pl);
    if (rc != DE_OK) return rc;
    if (pl.nt == 0) return DE_OK;
    TpDev d;
    rc = tp_setup(c, p, model, X, N, ldX, tp, o, ok, pl, nullptr, 0, &d);
    if (rc != DE_OK) return rc;
    const size_t nt = pl.nt, nc = pl.nc, es = pl.es, n_dp = d.n_dp;
    const std::vector<int64_t> &doff = pl.doff;
    const bool h_ok = d.h_ok, h_loss = d.h_loss, h_dl = d.h_dl, h_dp = d.h_dp, h_out = d.h_out;
    TreeParamsArgs &a = d.a;
    void *out_dev = o.out;
    int64_t ld_dev = o.ld_out;
    if (h_out) {
        HIP_TRY(c, c->sTpOut.reserve(nt * (size_t)N * es));
        out_dev = c->sTpOut.p;
        ld_dev = N;
    }

    if (!c->nested) HIP_TRY(c, time_begin(c));
    {
        NestGuard nest(c);
        if (nc > 0 && (rc = de_program_get_consts(p, d.base)) != DE_OK) return rc; // the base vector
        bool patched = false;
        rc = tp_run_classes(c, p, model, pl, d, tp->class_starts, ldX, o, out_dev, ld_dev, &patched);
        // the program holds its own constants again afterwards (after a failure too)
        const int rc2 = patched ? set_consts_device_impl(p, a.base) : DE_OK;
        if (rc != DE_OK) return rc;
        if (rc2 != DE_OK) return rc2;
        HIP_TRY(c, launch_tree_params_finish(p->dtype, a, c->stream));
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (h_loss) HIP_TRY(c, hipMemcpyAsync(o.loss, a.loss, nt * es, hipMemcpyDeviceToHost, c->stream));
    if (h_dl)
        for (size_t t = 0; t < nt; t++) {
            const size_t g = (size_t)(p->const_off[t + 1] - p->const_off[t]);
            if (g > 0)
                HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(o.dloss) + (size_t)doff[t] * es, static_cast<char *>(a.dloss) + (size_t)doff[t] * es,
                                          g * es, hipMemcpyDeviceToHost, c->stream));
        }
    if (h_dp) HIP_TRY(c, hipMemcpyAsync(o.dparams, a.dparams, n_dp * es, hipMemcpyDeviceToHost, c->stream));
    if (h_ok) HIP_TRY(c, hipMemcpyAsync(ok, a.ok, nt, hipMemcpyDeviceToHost, c->stream));
    if (h_out)
        HIP_TRY(c, hipMemcpy2DAsync(o.out, (size_t)o.ld_out * es, out_dev, (size_t)N * es, (size_t)N * es, nt, hipMemcpyDeviceToHost, c->stream));
    if (h_loss || h_dl || h_dp || h_ok || h_out) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_out) { // rows of incomplete trees are NaN in a host buffer, as de_eval documents
        std::vector<uint8_t> okh(nt);
        if (h_ok) std::memcpy(okh.data(), ok, nt);
        else HIP_TRY(c, hipMemcpy(okh.data(), ok, nt, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < nt; t++)
            if (!okh[t])
                for (int64_t j = 0; j < N; j++) store_elem(p->dtype, static_cast<char *>(o.out) + t * (size_t)o.ld_out * es, (size_t)j, std::nan(""));
    }
    return DE_OK;
}

int de_eval_tree_params(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp, void *out,
                        int64_t ld_out, uint8_t *ok) {
    TpOut o;
    o.out = out;
    o.ld_out = ld_out;
    DE_NOTHROW(c, tree_params_impl(c, p, "de_eval_tree_params", TP_EVAL, X, N, ldX, tp, o, ok));
}
int de_eval_loss_tree_params(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp, const void *y,
                             const void *w, const de_loss_spec_t *spec, void *loss, uint8_t *ok) {
    TpOut o;
    o.y = y; o.w = w; o.spec = spec; o.loss = loss;
    DE_NOTHROW(c, tree_params_impl(c, p, "de_eval_loss_tree_params", TP_LOSS, X, N, ldX, tp, o, ok));
}
int de_eval_loss_grad_tree_params(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                                  const void *y, const void *w, const de_loss_spec_t *spec, void *loss, void *dloss,
                                  const int64_t *dloss_offsets, void *dparams, uint8_t *ok) {
    TpOut o;
    o.y = y; o.w = w; o.spec = spec; o.loss = loss; o.dloss = dloss; o.dloss_offsets = dloss_offsets; o.dparams = dparams;
    DE_NOTHROW(c, tree_params_impl(c, p, "de_eval_loss_grad_tree_params", TP_LOSS_GRAD, X, N, ldX, tp, o, ok));
}

// ---- de_fit_tree_params_bfgs and de_fit_tree_params_lbfgs (§4.4.15): fit_consts_qn_impl's loop over each tree's packed
// vcat(constants, parameters[:]) ----
// Every evaluation is the class loop above followed by the finish kernel — de_eval_loss_grad_tree_params without its staging, its
// synchronisation and its copies — and the kernels of de_bfgs.hip (memory = 0) or de_lbfgs.hip (a ring of `memory` pairs per tree) see
// packed vectors only: pack / unpack (de_tree_params.hip) move the values between them and (the base vector's real slots, the pool's
// parameter block).  bo: the options both kernel sets share; opts_why: what is wrong with the caller's (null: nothing).
static int fit_tree_params_qn_impl(de_ctx_t *c, de_program_t *p, const char *what, int memory, const de_bfgs_opts_t &bo, const char *opts_why,
                                   const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp, const void *y, const void *w,
                                   const de_loss_spec_t *spec_in, void *params_out, void *loss, uint8_t *ok, double *history,
                                   int32_t *n_accept) {
    TpOut o;
    o.y = y; o.w = w; o.spec = spec_in; o.fit = true;
    TpPlan pl;
    int rc = tp_check(c, p, what, TP_LOSS_GRAD, X, N, ldX, tp, o, ok, &pl);
    if (rc != DE_OK) return rc;
    if (spec_in->kind == DE_LOSS_PULLBACK) return fail(c, DE_ERR_INVALID_ARG, "%s: DE_LOSS_PULLBACK is no objective", what);
    if (opts_why) return fail(c, DE_ERR_INVALID_ARG, "%s", opts_why);
    const size_t nt = pl.nt, nc = pl.nc, es = pl.es;
    const int64_t C = pl.C, ld = tp->ld_params;
    const int32_t P = pl.P;
    if (nt > 0 && !y) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    const size_t n_cells = nt * (size_t)C * (size_t)P; // the unknown parameter entries: every one, used by a leaf or not
    if (n_cells > 0 && (!tp->params || !params_out)) return fail(c, DE_ERR_INVALID_ARG, "%s: params / params_out is null", what);
    if (nt == 0) return DE_OK;

    // ---- the geometry of the packed vectors: [widths | packed offsets | B offsets | unknown -> slot or cell] ----
    QnKernels q;
    std::memset(&q.x, 0, sizeof q.x);
    q.memory = memory;
    const bool ring = memory > 0;
    std::vector<int32_t> ng(nt);
    std::vector<int64_t> poff(nt), boff(nt);
    int64_t npk = 0, bspan = 0;
    for (size_t t = 0; t < nt; t++) {
        int64_t n_real = 0;
        for (int64_t s = p->const_off[t]; s < p->const_off[t + 1]; s++) n_real += tp->slot_param[s] < 0 ? 1 : 0;
        const int64_t G = tpf_unknowns(n_real, P, C);
        if (G > INT32_MAX) return fail(c, DE_ERR_INVALID_ARG, "%s: tree %lld has %lld unknowns", what, (long long)t, (long long)G);
        ng[t] = (int32_t)G;
        poff[t] = npk;
        boff[t] = bspan;
        npk += G;
        bspan += q.state_doubles(G); // B, or each of S and Y: of the trees that are fitted
    }
    size_t tat = 0;
    const size_t t_ng = tp_place(&tat, nt * 4), t_poff = tp_place(&tat, nt * 8), t_boff = tp_place(&tat, nt * 8), t_map = tp_place(&tat, (size_t)npk * 8);
    std::vector<unsigned char> ftab(tat, 0);
    std::memcpy(ftab.data() + t_ng, ng.data(), nt * 4);
    std::memcpy(ftab.data() + t_poff, poff.data(), nt * 8);
    std::memcpy(ftab.data() + t_boff, boff.data(), nt * 8);
    {
        int64_t *map = reinterpret_cast<int64_t *>(ftab.data() + t_map);
        for (size_t t = 0; t < nt; t++)
            tpf_map_tree(p->const_off[t + 1] - p->const_off[t], nc > 0 ? tp->slot_param + p->const_off[t] : nullptr, P, C, p->const_off[t],
                         (int64_t)t * C * P, map + poff[t]);
    }

    // ---- the fit's part of the pool ----
    const bool h_hist = FitOutputs::on_host(history), h_acc = FitOutputs::on_host(n_accept), h_par = n_cells > 0 && !is_device_ptr(params_out);
    const size_t rows = (size_t)bo.iters + 1, pk = (size_t)npk, blk = nt * (size_t)C * (size_t)ld;
    size_t at = 0;
    const size_t o_pw = tp_place(&at, blk * es), o_ca = tp_place(&at, pk * es), o_ct = tp_place(&at, pk * es), o_la = tp_place(&at, nt * es),
                 o_lt = tp_place(&at, nt * es), o_da = tp_place(&at, pk * es), o_dt = tp_place(&at, pk * es), o_oka = tp_place(&at, nt),
                 o_okt = tp_place(&at, nt), o_dl = tp_place(&at, (size_t)pl.span * es), o_dp = tp_place(&at, n_cells * es),
                 o_B = tp_place(&at, (size_t)bspan * 8), o_al = tp_place(&at, nt * 8), o_sl = tp_place(&at, nt * 8), o_p = tp_place(&at, pk * 8),
                 o_fr = tp_place(&at, nt), o_pr = tp_place(&at, nt), o_hist = h_hist ? tp_place(&at, rows * nt * 8) : 0,
                 o_acc = h_acc ? tp_place(&at, nt * 4) : 0;
    // (the ring: S in B's place, and Y, rho, a scratch vector, count and head)
    const size_t o_Y = tp_place(&at, ring ? (size_t)bspan * 8 : 0), o_rho = tp_place(&at, ring ? nt * (size_t)memory * 8 : 0),
                 o_tmp = tp_place(&at, ring ? pk * 8 : 0), o_cnt = tp_place(&at, ring ? nt * 4 : 0), o_head = tp_place(&at, ring ? nt * 4 : 0);
    TpDev d;
    rc = tp_setup(c, p, TP_LOSS_GRAD, X, N, ldX, tp, o, ok, pl, &ftab, at, &d);
    if (rc != DE_OK) return rc;
    char *fit = d.pool + d.o_fit;
    const char *tab = d.pool + d.o_fit_tab;
    void *pw = fit + o_pw; // the parameter block the class loop reads: tp's layout, padding included
    if (blk > 0 && tp->params) {
        HIP_TRY(c, hipMemcpyAsync(pw, tp->params, blk * es, is_device_ptr(tp->params) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        if (!is_device_ptr(tp->params)) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (pageable memory)
    }
    TreeParamsArgs &ta = d.a;
    ta.params = pw;
    ta.dloss = fit + o_dl;
    ta.dparams = fit + o_dp;
    FitOutputs out; // (de_api_internal.h: the fits of de_api_fit.cpp resolve and copy theirs the same way)
    out.from_state(loss, fit + o_la, nt * es);
    out.from_state(ok, fit + o_oka, nt);
    double *hist = out.in_place(history, h_hist, reinterpret_cast<double *>(fit + o_hist), rows * nt);
    int32_t *acc = out.in_place(n_accept, h_acc, reinterpret_cast<int32_t *>(fit + o_acc), nt);
    BfgsArgs &a = q.x.b;
    a.n_trees = p->n_trees;
    a.n_grad = reinterpret_cast<const int32_t *>(tab + t_ng);
    a.coff = reinterpret_cast<const int64_t *>(tab + t_poff);
    a.consts_acc = fit + o_ca; a.loss_acc = fit + o_la; a.dloss_acc = fit + o_da; a.ok_acc = reinterpret_cast<uint8_t *>(fit + o_oka);
    void *lT = fit + o_lt, *dT = fit + o_dt;
    uint8_t *okT = reinterpret_cast<uint8_t *>(fit + o_okt);
    a.consts_trial = fit + o_ct; a.loss_trial = lT; a.dloss_trial = dT; a.ok_trial = okT;
    a.alpha = reinterpret_cast<double *>(fit + o_al);
    a.slope = reinterpret_cast<double *>(fit + o_sl); a.p = reinterpret_cast<double *>(fit + o_p);
    a.produced = reinterpret_cast<uint8_t *>(fit + o_pr);
    if (ring) {
        q.x.roff = reinterpret_cast<const int64_t *>(tab + t_boff);
        q.x.S = reinterpret_cast<double *>(fit + o_B); q.x.Y = reinterpret_cast<double *>(fit + o_Y);
        q.x.rho = reinterpret_cast<double *>(fit + o_rho); q.x.tmp = reinterpret_cast<double *>(fit + o_tmp);
        q.x.count = reinterpret_cast<int32_t *>(fit + o_cnt); q.x.head = reinterpret_cast<int32_t *>(fit + o_head);
        q.x.memory = memory;
    } else {
        a.boff = reinterpret_cast<const int64_t *>(tab + t_boff);
        a.B = reinterpret_cast<double *>(fit + o_B);
        a.fresh = reinterpret_cast<uint8_t *>(fit + o_fr);
    }
    a.step0 = bo.step0; a.shrink = bo.shrink; a.c1 = bo.c1; a.curv = bo.curv;
    a.n_accept = acc;
    TreeParamsFitArgs fx; // the unknowns' values: (base vector, parameter block)
    fx.n_unknowns = npk; fx.ld = ld; fx.n_params = P;
    fx.map = reinterpret_cast<const int64_t *>(tab + t_map);
    fx.packed = nullptr; fx.slots = d.base; fx.cells = pw;
    TreeParamsFitArgs fg = fx; // their gradient: (dloss, dparams)
    fg.ld = P; fg.slots = ta.dloss; fg.cells = ta.dparams;

    if (!c->nested) HIP_TRY(c, time_begin(c));
    const de_loss_spec_t spec = *spec_in;
    o.spec = &spec;
    {
        NestGuard nest(c);
        bool patched = false, begun = false;
        // one evaluation at (d.base, pw): de_eval_loss_grad_tree_params' launches, then the gradient packed
        auto evaluate = [&](void *l, void *g, uint8_t *k, bool install) -> int {
            ta.loss = l;
            ta.ok = k;
            if (install && !pl.any_param && nc > 0) { // (no parameter slot: the class loop installs nothing)
                patched = true;
                const int r = set_consts_device_impl(p, d.base);
                if (r != DE_OK) return r;
            }
            const int r = tp_run_classes(c, p, TP_LOSS_GRAD, pl, d, tp->class_starts, ldX, o, nullptr, 0, &patched);
            if (r != DE_OK) return r;
            HIP_TRY(c, launch_tree_params_finish(p->dtype, ta, c->stream));
            fg.packed = g;
            HIP_TRY(c, launch_tree_params_pack(p->dtype, fg, c->stream));
            return DE_OK;
        };
        auto body = [&]() -> int {
            if (nc > 0) {
                const int r = de_program_get_consts(p, d.base); // the base vector: the start of the real constants
                if (r != DE_OK) return r;
            }
            int r = evaluate(a.loss_acc, a.dloss_acc, a.ok_acc, false);
            if (r != DE_OK) return r;
            fx.packed = a.consts_acc;
            HIP_TRY(c, launch_tree_params_pack(p->dtype, fx, c->stream));
            HIP_TRY(c, q.init(p->dtype, c->stream));
            HIP_TRY(c, launch_lm_history(p->dtype, a.loss_acc, p->n_trees, hist, c->stream));
            const bool loop = N > 0 && bo.iters > 0 && npk > 0;
            if (!loop) // (no sample or no unknown: nothing can be accepted, every row of the history is the first)
                for (size_t r2 = 1; r2 < rows && hist; r2++) HIP_TRY(c, launch_lm_history(p->dtype, a.loss_acc, p->n_trees, hist + r2 * nt, c->stream));
            if (!loop) return DE_OK;
            begun = true;
            for (int32_t it = 0; it < bo.iters; it++) {
                HIP_TRY(c, q.direction(p->dtype, c->stream));
                fx.packed = a.consts_trial;
                HIP_TRY(c, launch_tree_params_unpack(p->dtype, fx, c->stream));
                r = evaluate(lT, dT, okT, true);
                if (r != DE_OK) return r;
                a.history_row = hist ? hist + ((size_t)it + 1) * nt : nullptr;
                HIP_TRY(c, q.accept(p->dtype, c->stream));
            }
            return DE_OK;
        };
        rc = body();
        // the program holds the accepted real constants afterwards and its parameter slots their base values (after a failure too: the
        // last accepted ones); the parameter block holds the accepted parameters
        int rc2 = DE_OK;
        if (begun) {
            fx.packed = a.consts_acc;
            if (launch_tree_params_unpack(p->dtype, fx, c->stream) != hipSuccess) rc2 = fail(c, DE_ERR_HIP, "%s: the unpack launch failed", what);
        }
        if (patched && rc2 == DE_OK) rc2 = set_consts_device_impl(p, d.base);
        if (rc != DE_OK) return rc;
        if (rc2 != DE_OK) return rc2;
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (n_cells > 0) { // the accepted parameters in tp's layout; padding entries are not written
        const hipMemcpyKind kind = h_par ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (ld == P) HIP_TRY(c, hipMemcpyAsync(params_out, pw, blk * es, kind, c->stream));
        else HIP_TRY(c, hipMemcpy2DAsync(params_out, (size_t)ld * es, pw, (size_t)ld * es, (size_t)P * es, nt * (size_t)C, kind, c->stream));
    }
    return out.finish(c, h_par);
}
int de_fit_tree_params_bfgs(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp, const void *y,
                            const void *w, const de_loss_spec_t *spec, const de_bfgs_opts_t *opts, void *params_out, void *loss, uint8_t *ok,
                            double *history, int32_t *n_accept) {
    const de_bfgs_opts_t defaults{20, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_bfgs_opts_t o = opts ? *opts : defaults;
    DE_NOTHROW(c, fit_tree_params_qn_impl(c, p, "de_fit_tree_params_bfgs", 0, o, bfgs_opts_problem(&o), X, N, ldX, tp, y, w, spec, params_out, loss,
                                          ok, history, n_accept));
}
int de_fit_tree_params_lbfgs(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp, const void *y,
                             const void *w, const de_loss_spec_t *spec, const de_lbfgs_opts_t *opts, void *params_out, void *loss, uint8_t *ok,
                             double *history, int32_t *n_accept) {
    const de_lbfgs_opts_t defaults{20, 0, 8, 0, 1.0, 0.5, 1e-4, 1e-8};
    const de_lbfgs_opts_t lo = opts ? *opts : defaults;
    de_bfgs_opts_t o;
    const char *why = lbfgs_opts_problem(&lo, &o);
    char named[200]; // (the text names the call)
    if (why) std::snprintf(named, sizeof named, "de_fit_tree_params_lbfgs: %s", why);
    DE_NOTHROW(c, fit_tree_params_qn_impl(c, p, "de_fit_tree_params_lbfgs", lo.memory, o, why ? named : nullptr, X, N, ldX, tp, y, w, spec,
                                          params_out, loss, ok, history, n_accept));
}

} // extern "C"
