// de_api_tree_params.cpp — C ABI (include/de_hip.h): de_tape_params_to_consts, de_eval_tree_params, de_eval_loss_tree_params,
// de_eval_loss_grad_tree_params and the host-only hook de_tree_params_accumulate_host.  A population whose trees
// each own their parameter matrix is an ordinary program in which some constant slots stand for parameters; a call serves it one class
// segment at a time: the class's constant vector is formed and installed on the device (de_program_set_consts_device), the model entry
// point runs on the class's sample range, and the per-tree results are added in double (kernels: de_tree_params.hip, arithmetic:
// de_tree_params.h).  No existing kernel, record format or lowering pass is involved.
#include "de_api_internal.h"
#include "de_tree_params_dev.h"
#include "de_tree_params.h"

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

extern "C" {

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
};

static size_t tp_place(size_t *at, size_t bytes) { // 16-byte aligned pieces of one pooled allocation
    const size_t o = *at;
    *at = o + ((bytes + 15) & ~(size_t)15);
    return o;
}

static int tree_params_impl(de_ctx_t *c, de_program_t *p, const char *what, TpModel model, const void *X, int64_t N, int64_t ldX,
                            const de_tree_params_t *tp, const TpOut &o, uint8_t *ok) {
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
        if (model == TP_LOSS_GRAD && nt > 0 && (!o.dloss || !o.dparams)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
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
    if (nt == 0) return DE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    span = std::max<int64_t>(span, 1);

    // ---- one pooled allocation: tables, the two constant vectors, one class's results, the accumulators, images of host outputs ----
    const size_t n_dp = grad ? nt * (size_t)C * (size_t)P : 0;
    const bool h_ok = !is_device_ptr(ok), h_loss = o.loss && !is_device_ptr(o.loss), h_dl = grad && !is_device_ptr(o.dloss),
               h_dp = grad && n_dp > 0 && !is_device_ptr(o.dparams), h_out = model == TP_EVAL && N > 0 && !is_device_ptr(o.out);
    size_t at = 0;
    const size_t o_stree = tp_place(&at, nc * 4), o_sparam = tp_place(&at, nc * 4), o_coff = tp_place(&at, (nt + 1) * 8), o_doff = tp_place(&at, nt * 8);
    const size_t tab_bytes = at;
    const size_t o_base = tp_place(&at, nc * es), o_cvec = tp_place(&at, nc * es), o_lc = tp_place(&at, nt * es),
                 o_dc = tp_place(&at, grad ? (size_t)span * es : 0), o_okc = tp_place(&at, nt);
    const size_t o_acc = at; // the accumulators are cleared together
    const size_t o_al = tp_place(&at, nt * 8), o_ad = tp_place(&at, grad ? nc * 8 : 0), o_ap = tp_place(&at, n_dp * 8);
    const size_t acc_bytes = at - o_acc;
    const size_t o_aok = tp_place(&at, nt);
    const size_t o_hok = h_ok ? tp_place(&at, nt) : 0, o_hl = h_loss ? tp_place(&at, nt * es) : 0,
                 o_hd = h_dl ? tp_place(&at, (size_t)span * es) : 0, o_hp = h_dp ? tp_place(&at, n_dp * es) : 0;
    if (at > c->sTp.cap) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (growing frees what queued work may still use)
    HIP_TRY(c, c->sTp.reserve(at));
    char *base = static_cast<char *>(c->sTp.p);

    std::vector<unsigned char> tab(tab_bytes, 0);
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
    Staged sX, sY, sW, sPar;
    int rc = DE_OK;
    if (N > 0) {
        if ((rc = stage_in(c, c->sX, X, (size_t)ldX * (size_t)N * es, &sX))) return rc;
        if (o.y && (rc = stage_in(c, c->sY, o.y, (size_t)N * es, &sY))) return rc;
        if (o.w && (rc = stage_in(c, c->sW, o.w, (size_t)N * es, &sW))) return rc;
        if (any_param && (rc = stage_in(c, c->sParams, tp->params, (size_t)tp->ld_params * (size_t)C * nt * es, &sPar))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the tables and the staged inputs come from pageable memory)
    void *out_dev = o.out;
    int64_t ld_dev = o.ld_out;
    if (h_out) {
        HIP_TRY(c, c->sTpOut.reserve(nt * (size_t)N * es));
        out_dev = c->sTpOut.p;
        ld_dev = N;
    }

    TreeParamsArgs a;
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

    if (!c->nested) HIP_TRY(c, time_begin(c));
    struct Nest { // the inner calls leave the timing events alone: the ring sees one call
        de_ctx *c;
        explicit Nest(de_ctx *c_) : c(c_) { c->nested++; }
        ~Nest() { c->nested--; }
    };
    {
        Nest nest(c);
        HIP_TRY(c, hipMemsetAsync(base + o_acc, 0, acc_bytes, c->stream));
        HIP_TRY(c, hipMemsetAsync(a.acc_ok, 1, nt, c->stream));
        if (grad) HIP_TRY(c, hipMemsetAsync(base + o_dc, 0, (size_t)span * es, c->stream)); // (entries no tree owns are never read)
        if (nc > 0 && (rc = de_program_get_consts(p, base + o_base)) != DE_OK) return rc; // the base vector
        bool patched = false;
        for (int64_t k = 0; k < C && rc == DE_OK; k++) {
            const int64_t j0 = tp->class_starts[k], n = tp->class_starts[k + 1] - j0;
            if (n <= 0) continue; // a class without samples: its columns are never read
            a.cls = k;
            if (any_param) {
                HIP_TRY(c, launch_tree_params_scatter(p->dtype, a, c->stream));
                patched = true;
                rc = set_consts_device_impl(p, a.cvec);
                if (rc != DE_OK) break;
            }
            const char *Xk = static_cast<const char *>(sX.dev) + (size_t)j0 * (size_t)ldX * es;
            const char *yk = o.y ? static_cast<const char *>(sY.dev) + (size_t)j0 * es : nullptr;
            const char *wk = o.w ? static_cast<const char *>(sW.dev) + (size_t)j0 * es : nullptr;
            uint8_t *okc = reinterpret_cast<uint8_t *>(base + o_okc);
            if (model == TP_EVAL) rc = de_eval(c, p, Xk, n, ldX, nullptr, static_cast<char *>(out_dev) + (size_t)j0 * es, ld_dev, okc);
            else if (model == TP_LOSS) rc = de_eval_loss_ex(c, p, Xk, n, ldX, nullptr, yk, wk, o.spec, base + o_lc, okc);
            else rc = de_eval_loss_grad_ex(c, p, Xk, n, ldX, nullptr, DE_GRAD_CONSTANT, yk, wk, o.spec, base + o_lc, base + o_dc, o.dloss_offsets, okc);
            if (rc != DE_OK) break;
            HIP_TRY(c, launch_tree_params_accumulate(p->dtype, a, c->stream));
        }
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

} // extern "C"
