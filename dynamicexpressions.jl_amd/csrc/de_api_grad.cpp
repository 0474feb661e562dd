// de_api_grad.cpp — C ABI (include/de_hip.h): what PRODUCES gradients and matrices from X.  de_eval_grad / de_eval_diff /
// de_eval_pullback_dX, de_eval_loss_grad, de_eval_loss_grad_by_class: the generic gradient program, the glue around the host encoders of its
// direct-threaded and reverse-accumulation forms (de_grad_encode.cpp) with their host-only hook de_lower_tape_grad, launch planning of the
// bucketed gradient kernels; de_eval_loss_gn(_ex) and de_eval_fit_stats_grad: the same launch with a GnPlan / FitPlan; their _wide forms
// (kernels de_gn_wide.hip).  The steps and fits that consume all this: de_api_fit.cpp.
#include <functional>

#include "de_api_internal.h"
#include "de_grad_encode.h"
#include "de_gn_wide.h"

// A direct-threaded stream inside one 4 GiB window (the handlers bump the record pointer without a carry), cleared.
static int stream_alloc(de_ctx *c, BoundInstr **d, size_t records, const char *what) {
    const size_t bytes = records * sizeof(BoundInstr);
    const hipError_t ast = prog_malloc(c, reinterpret_cast<void **>(d), bytes);
    if (ast != hipSuccess) return fail(c, DE_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(ast));
    if (!in_one_window(*d, bytes)) return fail(c, DE_ERR_HIP, "%s instruction stream straddles a 4 GiB boundary", what);
    HIP_TRY(c, hipMemset(*d, 0, bytes));
    return DE_OK;
}
// the switches both encoders (and the host hook de_lower_tape_grad) read
static GradEncodeOptions grad_encode_env() {
    GradEncodeOptions opt;
    opt.hot_const_unary = !getenv("DE_NO_CONST_UNARY_HOT"); // unary operators outside the binder's hot set through hot handlers
    opt.rfuse = !getenv("DE_REV_NO_FUSE"); // fused pairs / triples (de_rev_threaded.hip rh_pushload ...): same bits, fewer dispatches
    return opt;
}
template <class T> static hipError_t upload(T *dst, const std::vector<T> &v) {
    return v.empty() ? hipSuccess : hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

extern "C" {
static int ensure_generic_code(de_ctx *c, de_program *p) {
    if (p->gcode_stale || !p->d_gcode) {
        if (const int mrc = consts_materialise(p)) return mrc; // (bound from the host code: its immediates must be current, §3.5)
        // gradients flow through constant subtrees, so this is the UNFOLDED program; every value the
        // reference tests is tested (ee binding) whatever the eval options were
        p->gt_valid = false;
        p->rt_valid = false;
        // bound per worker into a vector of its own, then concatenated (10^4 trees: 3 ms on one thread)
        build_stream_by_trees<BoundInstr>(p->n_trees, &p->gbcode, &p->gbcode_off, [&](int64_t t, std::vector<BoundInstr> *out) {
            const int32_t i0 = p->code_off[(size_t)t], i1 = p->code_off[(size_t)t + 1];
            bind_tree_grad(p->code.data() + i0, (size_t)(i1 - i0), p->n_features, out);
        });
        match_const_sites(p->code, p->code_off, p->gbcode, p->gbcode_off, p->n_trees,
                          [](const BoundInstr &b) { return bop_is_const_source(b.bop); }, &p->gbsite);
        p->gtsite_of_gb.clear();
        p->site_gen++;
    }
    if (!p->d_gcode) {
        HIP_TRY(c, prog_malloc(c, reinterpret_cast<void **>(&p->d_gcode), (p->gbcode.size() + 1) * sizeof(BoundInstr)));
        HIP_TRY(c, hipMemset(p->d_gcode, 0, (p->gbcode.size() + 1) * sizeof(BoundInstr)));
        HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_gcode_off), p->gbcode_off.size() * sizeof(int32_t)));
        HIP_TRY(c, hipMemcpy(p->d_gcode_off, p->gbcode_off.data(), p->gbcode_off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        p->gcode_stale = true;
    }
    if (p->gcode_stale) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!p->gbcode.empty())
            HIP_TRY(c, hipMemcpy(p->d_gcode, p->gbcode.data(), p->gbcode.size() * sizeof(BoundInstr), hipMemcpyHostToDevice));
        p->gcode_stale = false;
    }
    return DE_OK;
}

// Threaded form of the gradient program (de_grad_threaded.hip) for `mode`, encoded by encode_grad_forward (de_grad_encode.cpp: buckets by
// gradient width, one module per window).  Fills g->threaded_code & co. when the program can be expressed this way; otherwise
// leaves them null and the flat-switch kernel runs.  Call after ensure_generic_code().
static int ensure_grad_threaded(de_ctx *c, de_program *p, int mode, const std::vector<int32_t> &ng, int64_t N, GradArgs *g) {
    g->threaded_code = nullptr;
    g->n_buckets = 0;
    g->gt_share = false;
    g->gt_var_stride = 0;
    const char *env = getenv("DE_GRAD_THREADED");
    if (env && *env == '0') return DE_OK;
    // Parameter leaves are LDS rows of their own: the kernel gathers params[:, class] into P rows behind the X rows when it
    // stages a tile (the reference's formulation, src/ParametricExpression.jl:381-389), so every hot handler serves them.
    const int FE = p->n_features + (p->uses_params ? p->n_params : 0);
    GradEncodeOptions opt = grad_encode_env();
    // Two samples per lane double the buckets (launches) and the tile: they pay from ~10^5 samples on (10^4 trees x
    // 10^3 rows: 0.55 ms with them, 0.35 ms without; 10^3 trees x 10^6 rows: 12.1 against 13.4 ms)
    const char *envn = getenv("DE_GRAD_VS2_MIN_N");
    opt.wide = N >= (envn ? atoll(envn) : 65536);
    if (!(p->gt_valid && p->gt_mode == mode && p->gt_wide == opt.wide)) {
        const char *env2 = getenv("DE_GRAD_VS2_ROWS"); // most LDS rows per wave (X + parameters + slots) that still run two samples per lane
        // 15 rows x 512 B x 4 waves = 30.7 KB: 5 workgroups per CU.  Parametric populations (their P parameter rows come on top of X) take 18:
        // measured in round 6 (tools/experiments/sweep_vs2_rows.sh, same box): C5 7.98 / 7.82 / 7.81 / 8.06 / 8.42 ms and C5Ng 7.30 / 7.06 / 7.14 /
        // 7.40 / 7.66 ms at 15 / 18 / 20 / 22 / 24 rows — two samples per lane pay a little further out when most rows are shared inputs
        opt.vs2_rows = env2 ? atoi(env2) : (p->uses_params ? 18 : 15);
        // SHARED LEAF ROWS (GradArgs::gt_share): with many leaf rows most of a wave's LDS is a copy of inputs the other three waves could
        // read as well — the four waves then take different trees on the same samples.  Measured (round 6, constant-mode Jacobians of 1000
        // trees x 10^5 samples, tools/experiments/wide_x_grad.py): F = 5 0.80 -> 0.86 ms (worse: the staging is spread over fewer samples),
        // F = 20 1.14 -> 1.03, F = 40 1.82 -> 1.05, F = 60 2.58 -> 1.18, F = 120 5.82 -> 1.91; 5 features + 8 parameter rows (C5): 7.42 -> 7.35 ms,
        // nothing — those kernels are not short of resident waves.  From 16 leaf rows on; DE_GRAD_SHARE = 0 | 1 overrides.
        const char *envs = getenv("DE_GRAD_SHARE"), *envf = getenv("DE_GRAD_SHARE_MIN_ROWS");
        opt.share = envs ? *envs == '1' : FE >= (envf ? atoi(envf) : 16);
        opt.lap = dbg_lap;
        std::vector<std::array<uint64_t, GOP_MAX>> tables;
        tables.reserve(GRAD_BUCKETS_MAX); // (the encoder keeps pointers into it)
        hipError_t hst = hipSuccess;
        const GradHandlerSource handlers = [&](int GC, int VS, GradHandlers *h) -> int {
            tables.emplace_back();
            hst = grad_handler_table(p->dtype, GC, VS, tables.back().data());
            if (hst != hipSuccess) return -DE_ERR_HIP;
            h->table = tables.back().data();
            return handler_base(h->table, gop_count(GC), &h->base) ? GRAD_ENC_OK : GRAD_ENC_NO_PLAN;
        };
        const GradSource src{p->gbcode, p->gbcode_off, p->n_trees, p->n_features, p->n_params, p->uses_params, p->dtype, mode, ng.data()};
        GradForwardStream r;
        int enc = encode_grad_forward(src, opt, grad_threaded_has, handlers, &r);
        if (hst != hipSuccess) return fail(c, DE_ERR_HIP, "gradient handler table: %s", hipGetErrorString(hst));
        if (enc == GRAD_ENC_NO_PLAN) return DE_OK; // (nothing is kept: a program without a plan asks again at every call)
        if (enc == GRAD_ENC_OK && p->consts_dev_ahead) {
            // a stream that will be kept, encoded from a gbcode whose immediates are behind a device set (§3.5): the host side is
            // brought up first — only now, so that a program without a plan never pays for it — and the stream encoded again
            if (const int mrc = consts_materialise(p)) return mrc;
            tables.clear();
            r = GradForwardStream();
            enc = encode_grad_forward(src, opt, grad_threaded_has, handlers, &r);
            if (hst != hipSuccess) return fail(c, DE_ERR_HIP, "gradient handler table: %s", hipGetErrorString(hst));
            if (enc == GRAD_ENC_NO_PLAN) return DE_OK;
        }
        p->gtsite_of_gb.clear();
        p->site_gen++;
        if (enc < 0) return fail(c, DE_ERR_HIP, "gradient program: the host threads' partitions disagree");
        if (enc != GRAD_ENC_OK) return DE_OK;
        p->gtcode = std::move(r.gtcode);
        p->gtcode_off = std::move(r.gtcode_off);
        p->gtsite_of_gb = std::move(r.gtsite_of_gb);
        p->gt_share = r.share;
        p->gt_stride = r.stride;
        // a unary operator on a constant leaf becomes two instructions: at most twice the bound program
        // ... plus one end record per tree and one of padding (every handler reads the record behind its own)
        const size_t gt_cap = (2 * p->gbcode.size() + (size_t)p->n_trees + 1) * (r.share ? 4 : 1);
        if (p->d_gtcode && p->gt_cap < gt_cap) { // (DE_GRAD_SHARE switched between two encodings of one program: tests)
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            prog_free(c, p->d_gtcode);
            p->d_gtcode = nullptr;
            if (p->d_gtcode_off) { (void)hipFree(p->d_gtcode_off); p->d_gtcode_off = nullptr; }
            if (p->d_gt_ids) { (void)hipFree(p->d_gt_ids); p->d_gt_ids = nullptr; }
        }
        if (!p->d_gtcode) {
            p->gt_cap = gt_cap;
            const int rc = stream_alloc(c, &p->d_gtcode, gt_cap, "gradient");
            if (rc != DE_OK) return rc;
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_gtcode_off), p->gtcode_off.size() * sizeof(int32_t)));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_gt_ids), std::max<size_t>(r.ids.size(), 1) * sizeof(int32_t)));
        }
        dbg_lap("grad threaded: ids, hipMalloc, memset");
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // the previous form may be in use by queued work
        HIP_TRY(c, upload(p->d_gtcode, p->gtcode));
        HIP_TRY(c, upload(p->d_gtcode_off, p->gtcode_off));
        HIP_TRY(c, upload(p->d_gt_ids, r.ids));
        p->gt_n_buckets = r.n_buckets;
        for (int b = 0; b < r.n_buckets; b++) {
            const GradForwardStream::Bucket &rb = r.buckets[b];
            p->gt_buckets[b] = GradArgs::Bucket{rb.GC, rb.VS, rb.windows, rb.max_grad, rb.slots, p->d_gt_ids + rb.start, rb.count, rb.handler_base, rb.param_handler_off};
        }
        dbg_lap("grad threaded: upload");
        p->gt_mode = mode;
        p->gt_wide = opt.wide;
        p->gt_valid = true;
    }
    g->threaded_code = p->d_gtcode;
    g->gt_share = p->gt_share;
    g->gt_var_stride = p->gt_stride;
    g->e.code_off = p->d_gtcode_off;
    g->n_buckets = p->gt_n_buckets;
    for (int b = 0; b < p->gt_n_buckets; b++) g->buckets[b] = p->gt_buckets[b];
    return DE_OK;
}

// Reverse-accumulation form of the gradient program (de_rev_threaded.hip) for `mode`: per tree the forward
// instructions (every operator also stores its partials in LDS rows of its own), then the backward instructions
// in execution order.  Fills g->rev_* when the program can be expressed this way (otherwise leaves rev_code
// null and the forward-dual kernels run).  Call after ensure_generic_code().
static int ensure_rev_threaded(de_ctx *c, de_program *p, int mode, GradArgs *g) {
    g->rev_code = nullptr;
    // Reverse accumulation costs two sweeps whatever the number of gradient rows; forward duals cost one sweep
    // of (1 + rows) values (and one sweep per window of 8 rows).  Measured break-even on MI355X: ~8 rows per tree
    // (20-node trees: 3.5 rows 9.6 ms forward / 17.2 ms reverse; 17 rows 44.6 ms / 30.2 ms).  DE_LOSS_GRAD_REVERSE=1|0 forces.
    const char *env = getenv("DE_LOSS_GRAD_REVERSE");
    if (env && *env == '0') return DE_OK;
    // DE_OPT_FORWARD_GRAD: the caller wants the reference's forward-mode flag semantics exactly (a product chain that overflows in one
    // association only flips `ok` in ~0.03 % of Float32 fuzz cases under reverse accumulation): forward duals whatever the width
    if (p->options & DE_OPT_FORWARD_GRAD) return DE_OK;
    // ABI 3 (round 6): reverse accumulation is an OPT-IN (DE_OPT_REVERSE_GRAD, or DE_LOSS_GRAD_REVERSE=1 for the tests / experiments): the
    // default keeps the reference's forward-mode flag semantics
    if (!(p->options & DE_OPT_REVERSE_GRAD) && !(env && *env == '1')) return DE_OK;
    // a CSE program (GraphNode trees, §3.1) reads a persistent row from several consumers: the backward sweep ACCUMULATES their adjoints
    // into that row (round 4: `acc_use` below); DE_REV_NO_SHARED=1 restores round 3's fall-back to forward duals for such populations
    if (p->cse_generic && getenv("DE_REV_NO_SHARED")) return DE_OK;
    if (!(env && *env == '1')) {
        int64_t total = 0;
        for (int64_t t = 0; t < p->n_trees; t++) total += de_program_n_grad(p, t, mode);
        if (total < 8 * p->n_trees) return DE_OK;
    }
    if (!(p->rt_valid && p->rt_mode == mode)) {
        uint64_t table[ROP_COUNT];
        hipError_t hst = rev_handler_table(p->dtype, table);
        if (hst != hipSuccess) return fail(c, DE_ERR_HIP, "reverse handler table: %s", hipGetErrorString(hst));
        GradHandlers h{table, 0};
        if (!handler_base(table, ROP_COUNT, &h.base)) return DE_OK;
        const GradEncodeOptions opt = grad_encode_env();
        std::vector<int32_t> ng((size_t)p->n_trees);
        for (int64_t t = 0; t < p->n_trees; t++) ng[(size_t)t] = (int32_t)de_program_n_grad(p, t, mode);
        const GradSource src{p->gbcode, p->gbcode_off, p->n_trees, p->n_features, p->n_params, p->uses_params, p->dtype, mode, ng.data()};
        GradReverseStream r;
        int enc = encode_grad_reverse(src, opt, p->n_slots, p->cse_generic, h, &r);
        if (enc == GRAD_ENC_OK && p->consts_dev_ahead) { // (as ensure_grad_threaded: the host side first, then the stream that is kept, §3.5)
            if (const int mrc = consts_materialise(p)) return mrc;
            r = GradReverseStream();
            enc = encode_grad_reverse(src, opt, p->n_slots, p->cse_generic, h, &r);
        }
        p->rtsite_of_gb.clear();
        p->site_gen++;
        if (enc != GRAD_ENC_OK) return DE_OK;
        if (getenv("DE_REV_STATS")) reverse_stream_stats(r, p->n_trees, h);
        p->rtcode = std::move(r.rtcode);
        p->rtcode_off = std::move(r.rtcode_off);
        p->rtcode_mid = std::move(r.rtcode_mid);
        p->rtsite_of_gb = std::move(r.rtsite_of_gb);
        p->rt_n_groups = r.n_groups;
        for (int k = 0; k < r.n_groups; k++) p->rt_groups[k] = GradArgs::RevGroup{r.groups[k].first, r.groups[k].n, r.groups[k].rows};
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // the previous form may be in use by queued work
        if (p->d_rtcode) { // sizes depend on the mode
            prog_free(c, p->d_rtcode);
            p->d_rtcode = nullptr;
        }
        const int rc = stream_alloc(c, &p->d_rtcode, p->rtcode.size() + 1, "reverse");
        if (rc != DE_OK) return rc;
        if (!p->d_rtcode_off) {
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_rtcode_off), p->rtcode_off.size() * sizeof(int32_t)));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_rtcode_mid), std::max<size_t>(p->rtcode_mid.size(), 1) * sizeof(int32_t)));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_rt_ids), std::max<size_t>(r.ids.size(), 1) * sizeof(int32_t)));
        }
        HIP_TRY(c, upload(p->d_rtcode, p->rtcode));
        HIP_TRY(c, upload(p->d_rtcode_off, p->rtcode_off));
        HIP_TRY(c, upload(p->d_rtcode_mid, p->rtcode_mid));
        HIP_TRY(c, upload(p->d_rt_ids, r.ids));
        p->rt_stage_cols = (int)r.stage_cols;
        p->rt_handler_base = h.base;
        p->rt_param_off = (uint32_t)(table[ROP_PARAM] - h.base);
        p->rt_mode = mode;
        p->rt_valid = true;
    }
    g->rev_code = p->d_rtcode;
    g->rev_code_off = p->d_rtcode_off;
    g->rev_code_mid = p->d_rtcode_mid;
    g->rev_ids = p->d_rt_ids;
    g->rev_n_groups = p->rt_n_groups;
    for (int k = 0; k < p->rt_n_groups; k++) g->rev_groups[k] = p->rt_groups[k];
    g->rev_stage_cols = p->rt_stage_cols;
    g->rev_handler_base = p->rt_handler_base;
    g->rev_param_off = p->rt_param_off;
    return DE_OK;
}

// Host-only hook (no HIP call, like de_lower_tape_stage): one tape lowered and bound as ensure_generic_code does (unfolded, early-exit
// binding), then encoded by encode_grad_forward (form 0; 1: `wide`; 2: shared leaf rows, the four variants one behind the other) or
// encode_grad_reverse (form 3) against an identity handler table — a record's handler word is then a plain gop_* / ROP_* id.
// meta[8], forward: GC, VS, windows, slots, records per variant, variants; reverse: mid, need, stage_cols, LDS rows per wave, n_slots;
// both: [6] constants whose site (the record set_consts patches) holds their bits, [7] a hash of the site table.  Returns the words, 0: not expressible, < 0: -status.
int64_t de_lower_tape_grad(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts, int32_t n_features,
                           int32_t n_params, uint32_t options, int mode, int form, uint32_t *words, int64_t cap, int32_t *meta) {
    if (dtype != DE_F32 && dtype != DE_F64) return -DE_ERR_INVALID_ARG;
    if (mode != DE_GRAD_VARIABLE && mode != DE_GRAD_CONSTANT && mode != DE_GRAD_BOTH) return -DE_ERR_INVALID_ARG;
    if (form < 0 || form > 3 || !meta) return -DE_ERR_INVALID_ARG;
    int32_t lmeta[4] = {0, 0, 0, 0};
    int64_t nw = de_lower_tape(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, nullptr, 0, lmeta);
    if (nw < 0) return nw;
    try {
        std::vector<uint32_t> gen((size_t)nw);
        nw = de_lower_tape(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, gen.data(), nw, lmeta);
        if (nw < 0) return nw;
        std::vector<BoundInstr> gb;
        bind_tree_grad(reinterpret_cast<const Instr *>(gen.data()), (size_t)nw / 4, n_features, &gb);
        const std::vector<int32_t> gb_off = {0, (int32_t)gb.size()};
        bool cse = false; // (a CSE tape announces itself by its markers)
        for (int64_t i = 0; i < n_nodes; i++)
            cse = cse || (nodes[i].degree == 1 && nodes[i].op == DE_OP_SHARE) || (nodes[i].degree == 0 && nodes[i].op == DE_LEAF_SHARED);
        const int32_t nv = n_features + n_params;
        const int32_t ng = mode == DE_GRAD_VARIABLE ? nv : (mode == DE_GRAD_CONSTANT ? (int32_t)n_consts : nv + (int32_t)n_consts);
        const GradSource src{gb, gb_off, 1, n_features, n_params, lmeta[3] != 0, dtype, mode, &ng};
        GradEncodeOptions opt = grad_encode_env();
        opt.wide = form == 1;
        opt.share = form == 2;
        opt.vs2_rows = lmeta[3] ? 18 : 15;
        std::vector<uint64_t> identity(std::max<size_t>(GOP_MAX, ROP_COUNT));
        for (size_t i = 0; i < identity.size(); i++) identity[i] = i;
        const std::vector<BoundInstr> *code = nullptr;
        const std::vector<int32_t> *site = nullptr;
        GradForwardStream f;
        GradReverseStream r;
        std::memset(meta, 0, 8 * sizeof(int32_t));
        if (form == 3) {
            const int enc = encode_grad_reverse(src, opt, lmeta[0], cse, GradHandlers{identity.data(), 0}, &r);
            if (enc != GRAD_ENC_OK) return enc < 0 ? -DE_ERR_HIP : 0;
            const int32_t m[5] = {r.rtcode_mid[0], (int32_t)r.need[0], (int32_t)r.stage_cols, r.groups[0].rows, lmeta[0]};
            std::memcpy(meta, m, sizeof m);
            code = &r.rtcode;
            site = &r.rtsite_of_gb;
        } else {
            const GradHandlerSource handlers = [&](int, int, GradHandlers *h) { *h = GradHandlers{identity.data(), 0}; return (int)GRAD_ENC_OK; };
            const int enc = encode_grad_forward(src, opt, grad_threaded_has, handlers, &f);
            if (enc != GRAD_ENC_OK) return enc < 0 ? -DE_ERR_HIP : 0;
            const GradForwardStream::Bucket &bk = f.buckets[0];
            const int32_t m[6] = {bk.GC, bk.VS, bk.windows, bk.slots, f.gtcode_off[1], f.share ? 4 : 1};
            std::memcpy(meta, m, sizeof m);
            code = &f.gtcode;
            site = &f.gtsite_of_gb;
        }
        uint32_t hash = 2166136261u;
        for (size_t i = 0; i < gb.size(); i++) {
            const int32_t at = (*site)[i]; // (where de_program_set_consts would patch this constant: the record must hold its bits)
            if (bop_is_const_source(gb[i].bop) && at >= 0 && (*code)[(size_t)at].lo == gb[i].lo && (*code)[(size_t)at].hi == gb[i].hi) meta[6]++;
            hash = (hash ^ (uint32_t)(*site)[i]) * 16777619u;
        }
        meta[7] = (int32_t)hash;
        const int64_t n = (int64_t)code->size() * 4;
        if (!words || cap < n) return n;
        std::memcpy(words, code->data(), (size_t)n * 4);
        return n;
    } catch (...) {
        return -DE_ERR_HIP;
    }
}

// Shared body of de_eval_grad / de_eval_diff.
static int grad_impl(de_ctx *c, de_program *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                     int mode, int diff_direction, void *out, int64_t ld_out, void *grad,
                     const int64_t *grad_offsets, uint8_t *ok, const void *dY = nullptr) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    const bool diff = diff_direction >= 0;
    if (N < 0 || !ok || (p->n_trees > 0 && N > 0 && (!X || !grad))) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    if (ldX < p->n_features || ((out || diff) && ld_out < N)) return fail(c, DE_ERR_INVALID_ARG, "ldX < n_features or ld_out < N");
    if (!diff && mode != DE_GRAD_VARIABLE && mode != DE_GRAD_CONSTANT && mode != DE_GRAD_BOTH)
        return fail(c, DE_ERR_INVALID_ARG, "bad gradient mode");
    if (diff && diff_direction >= p->n_features) return fail(c, DE_ERR_OUT_OF_RANGE, "direction >= n_features");
    int rc = check_param_args(c, p, pa, N);
    if (rc != DE_OK) return rc;
    if (p->n_trees == 0) return DE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const bool half = p->io == DE_F16; // (a program with DE_OPT_F16_GRAD: de_half_grad.hip, binary16 buffers)
    const size_t es = dtype_bytes(p->io);
    const bool ok_dev = is_device_ptr(ok);
    std::vector<uint8_t> ones;
    if (N == 0 && !diff) { // (the flags alone: from the host side, §3.5)
        rc = consts_materialise(p);
        if (rc != DE_OK) return rc;
    }
    const uint8_t *ok_init = p->host_ok_grad.data();
    if (diff) { // no validity test on this path: always complete (src/EvaluateDerivative.jl:117)
        ones.assign((size_t)p->n_trees, 1);
        ok_init = ones.data();
    }
    if (N == 0) {
        if (ok_dev) {
            HIP_TRY(c, hipMemcpyAsync(ok, ok_init, (size_t)p->n_trees, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        } else std::memcpy(ok, ok_init, (size_t)p->n_trees);
        return DE_OK;
    }
    // per-tree gradient geometry
    std::vector<int32_t> ng((size_t)p->n_trees);
    std::vector<int64_t> goff((size_t)p->n_trees);
    int64_t span = 0, run = 0;
    int32_t maxg = 0;
    for (int64_t t = 0; t < p->n_trees; t++) {
        const int32_t g = diff ? 1 : (int32_t)de_program_n_grad(p, t, mode);
        ng[(size_t)t] = g;
        maxg = std::max(maxg, g);
        const int64_t off = diff ? t * ld_out : (grad_offsets ? grad_offsets[t] : run);
        if (off < 0) return fail(c, DE_ERR_INVALID_ARG, "negative gradient offset");
        goff[(size_t)t] = off;
        run += (int64_t)g * N;
        span = std::max(span, off + (int64_t)g * N);
    }
    rc = ensure_generic_code(c, p);
    if (rc) return rc;

    Staged sX, sOut, sGrad, sOk, sPar, sCls;
    rc = stage_in(c, c->sX, X, (size_t)ldX * (size_t)N * es, &sX);
    if (rc) return rc;
    if (out) {
        rc = stage_out(c, c->sOut, out, ((size_t)(p->n_trees - 1) * (size_t)ld_out + (size_t)N) * es, &sOut);
        if (rc) return rc;
    }
    rc = stage_out(c, diff ? c->sOut2 : c->sGrad, grad, (size_t)span * es, &sGrad);
    if (rc) return rc;
    if (ok_dev) sOk.dev = ok;
    else {
        HIP_TRY(c, c->sOk.reserve((size_t)p->n_trees));
        sOk.dev = c->sOk.p;
        sOk.staged = true;
    }
    // The initial flags, the gradient widths and (packed layout) the offsets depend on the program, the mode and N only:
    // they live on the device and are refreshed when one of those changes — the usual call copies nothing from pageable
    // host memory and does not block.  Caller-supplied offsets and eval_diff take the staged path.
    const bool cached = !diff && !grad_offsets;
    const int64_t *d_goff_use = nullptr;
    const int32_t *d_ng_use = nullptr;
    if (cached) {
        const size_t nt = (size_t)p->n_trees;
        if (!p->d_ok_grad) {
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_ok_grad), nt));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_ng), nt * sizeof(int32_t)));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_goff), nt * sizeof(int64_t)));
            p->tab_ok_stale = true;
            p->tab_mode = -1;
        }
        if (p->tab_ok_stale || p->tab_mode != mode || p->tab_N != N) {
            HIP_TRY(c, hipStreamSynchronize(c->stream)); // earlier calls may still read the tables
            // (behind a device set the flag kernel has written d_ok_grad, and host_ok_grad is not current: §3.5)
            if (!p->consts_dev_ahead) HIP_TRY(c, hipMemcpy(p->d_ok_grad, p->host_ok_grad.data(), nt, hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(p->d_ng, ng.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(p->d_goff, goff.data(), nt * sizeof(int64_t), hipMemcpyHostToDevice));
            p->tab_ok_stale = false;
            p->tab_mode = mode;
            p->tab_N = N;
        }
        HIP_TRY(c, hipMemcpyAsync(sOk.dev, p->d_ok_grad, nt, hipMemcpyDeviceToDevice, c->stream));
        d_goff_use = p->d_goff;
        d_ng_use = p->d_ng;
    } else {
        if (p->consts_dev_ahead && !diff) HIP_TRY(c, hipMemcpyAsync(sOk.dev, p->d_ok_grad, (size_t)p->n_trees, hipMemcpyDeviceToDevice, c->stream));
        else HIP_TRY(c, hipMemcpyAsync(sOk.dev, ok_init, (size_t)p->n_trees, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, c->sGoff.reserve(goff.size() * sizeof(int64_t)));
        HIP_TRY(c, c->sNg.reserve(ng.size() * sizeof(int32_t)));
        HIP_TRY(c, hipMemcpyAsync(c->sGoff.p, goff.data(), goff.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->sNg.p, ng.data(), ng.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        d_goff_use = static_cast<const int64_t *>(c->sGoff.p);
        d_ng_use = static_cast<const int32_t *>(c->sNg.p);
    }
    if (p->uses_params) {
        rc = stage_in(c, c->sParams, pa->params, (size_t)pa->ld_params * (size_t)pa->n_classes * es, &sPar);
        if (rc) return rc;
        rc = stage_in(c, c->sClasses, pa->classes, (size_t)N * (pa->classes_is_i64 ? 8 : 4), &sCls);
        if (rc) return rc;
    }
    // the pageable host vectors of the staged path must outlive their async copies
    if (!cached) HIP_TRY(c, hipStreamSynchronize(c->stream));

    GradArgs g;
    std::memset(&g, 0, sizeof g);
    g.generic_code = p->d_gcode;
    g.e.code_off = nullptr;
    g.e.n_trees = (int32_t)p->n_trees;
    g.e.skip_flagged = !(p->options & DE_OPT_FULL_EVAL) && tree_skip_enabled(); // (the gradient entry points always test validity)
    // (a binary16 program runs neither the priority tiles nor a declared dataset's keys)
    if (!half && c->sPrio.reserve((size_t)3 * DE_PRIO_MAX_F * sizeof(unsigned long long)) == hipSuccess) g.e.prio_keys = c->sPrio.p; // priority tiles (de_kernels.hip)
    g.prio_ready = false;
    g.e.prio_keys_ready = !half && !sX.staged && g.e.prio_keys && dataset_keys(c, p->dtype, X, N, ldX, p->n_features, &g.e.prio_keys);
    g.e.n_slots = p->n_slots;
    g.e.uses_params = p->uses_params;
    g.e.X = sX.dev;
    g.e.N = N;
    g.e.ldX = ldX;
    g.e.F = p->n_features;
    g.e.out = out ? sOut.dev : nullptr;
    g.e.ld_out = ld_out;
    g.e.ok = static_cast<uint8_t *>(sOk.dev);
    if (p->uses_params) {
        g.e.params = sPar.dev;
        g.e.ld_params = pa->ld_params;
        g.e.n_classes = pa->n_classes;
        g.e.classes = sCls.dev;
        g.e.classes_is_i64 = pa->classes_is_i64;
        g.e.class_base = pa->class_base;
    }
    g.mode = diff ? DE_GRAD_VARIABLE : mode;
    g.P = p->n_params;
    g.grad = sGrad.dev;
    g.grad_off = d_goff_use;
    g.n_grad = d_ng_use;
    g.max_grad = maxg;
    g.diff_direction = diff ? diff_direction : -1;
    g.e.code_off = p->d_gcode_off;
    if (!diff && !half) { // (binary16: the flat-switch dual kernel alone)
        rc = ensure_grad_threaded(c, p, mode, ng, N, &g);
        if (rc) return rc;
    }
    // the tape kernel launches (launch_grad / launch_grad_f16): the launch's own window and row size (the binary16 kernel's LDS rows are
    // Float32).  A program the threaded kernels serve has passed their own limit (de_grad_encode.cpp forward_plan).
    if (!g.threaded_code && grad_tape_lds_bytes(p->n_features, p->n_slots, grad_window(maxg), half ? 4 : es) > 160 * 1024)
        return fail(c, DE_ERR_UNSUPPORTED, "gradient kernel: LDS footprint too large for this tree shape");
    Staged sDY;
    if (dY) {
        rc = stage_in(c, c->sY, dY, (size_t)N * es, &sDY);
        if (rc) return rc;
    }
    if (!c->nested) HIP_TRY(c, time_begin(c));
    if (half) HIP_TRY(c, launch_grad_f16(g, c->stream, &c->last_kernel));
    else HIP_TRY(c, launch_grad(p->dtype, g, c->stream, &c->last_kernel));
    if (dY) // the pullback's dX .* dY' (and its NaN fill) on the Jacobians just written
        HIP_TRY(c, launch_pullback_scale(p->dtype, sGrad.dev, g.grad_off, g.n_grad, g.e.ok, sDY.dev, N, p->n_trees, maxg, c->stream));
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (out && sOut.staged)
        for (int64_t t = 0; t < p->n_trees; t++)
            HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(out) + (size_t)t * (size_t)ld_out * es,
                                      static_cast<char *>(sOut.dev) + (size_t)t * (size_t)ld_out * es, (size_t)N * es,
                                      hipMemcpyDeviceToHost, c->stream));
    if (sGrad.staged) {
        if (diff) {
            for (int64_t t = 0; t < p->n_trees; t++)
                HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(grad) + (size_t)t * (size_t)ld_out * es,
                                          static_cast<char *>(sGrad.dev) + (size_t)t * (size_t)ld_out * es, (size_t)N * es,
                                          hipMemcpyDeviceToHost, c->stream));
        } else {
            for (int64_t t = 0; t < p->n_trees; t++)
                if (ng[(size_t)t] > 0)
                    HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(grad) + (size_t)goff[(size_t)t] * es,
                                              static_cast<char *>(sGrad.dev) + (size_t)goff[(size_t)t] * es,
                                              (size_t)ng[(size_t)t] * (size_t)N * es, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (sOk.staged) HIP_TRY(c, hipMemcpyAsync(ok, sOk.dev, (size_t)p->n_trees, hipMemcpyDeviceToHost, c->stream));
    if (sX.staged || sOut.staged || sGrad.staged || sOk.staged || sPar.staged || sCls.staged) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (g.e.skip_flagged && ((out && sOut.staged) || sGrad.staged)) {
        // host buffers: rows / Jacobians of incomplete trees were only partly written into staging buffers every program of the context
        // shares — NaN-fill them (as eval_impl does; src/EvaluationHelpers.jl:56-62 does the same one level up)
        std::vector<uint8_t> okh;
        const uint8_t *okp = ok;
        if (ok_dev) {
            okh.resize((size_t)p->n_trees);
            HIP_TRY(c, hipMemcpy(okh.data(), ok, (size_t)p->n_trees, hipMemcpyDeviceToHost));
            okp = okh.data();
        }
        auto fill = [&](void *base, size_t off, size_t n) {
            if (half) std::fill_n(static_cast<_Float16 *>(base) + off, n, (_Float16)std::nanf(""));
            else if (p->dtype == DE_F32) std::fill_n(static_cast<float *>(base) + off, n, std::nanf(""));
            else std::fill_n(static_cast<double *>(base) + off, n, std::nan(""));
        };
        for (int64_t t = 0; t < p->n_trees; t++) {
            if (okp[t]) continue;
            if (out && sOut.staged) fill(out, (size_t)t * (size_t)ld_out, (size_t)N);
            if (sGrad.staged && diff) fill(grad, (size_t)t * (size_t)ld_out, (size_t)N);
            else if (sGrad.staged && ng[(size_t)t] > 0) fill(grad, (size_t)goff[(size_t)t], (size_t)ng[(size_t)t] * (size_t)N);
        }
    }
    return DE_OK;
}

// By-class reduction in ONE pass (de_eval_loss_grad_by_class): class-aligned tiles, then one pair of finish passes per
// class into loss_c / dloss_c ([C][n_trees] and [C][span], device).  Only the reverse kernel takes a tile table:
// `done` stays false when the population runs forward duals and the caller falls back to one call per class.
struct ByClassPlan {
    const int64_t *class_starts;
    int64_t C, span;
    void *loss_c, *dloss_c;
    bool done;
};
// de_gn_spec_check with its reason (null = good; *rc: DE_ERR_INVALID_ARG or DE_ERR_UNSUPPORTED).  dtype < 0: the element type is not known.
const char *gn_spec_problem(const de_loss_spec_t *spec, double e_floor, int dtype, int *rc, char *buf, size_t cap) {
    *rc = DE_ERR_INVALID_ARG;
    if (loss_spec_problem(spec, 1, buf, cap)) return buf;
    if (spec->kind == DE_LOSS_PULLBACK) { std::snprintf(buf, cap, "DE_LOSS_PULLBACK has no Gauss-Newton matrix"); return buf; }
    if (spec->kind == DE_LOSS_L1_HINGE) {
        *rc = DE_ERR_UNSUPPORTED;
        std::snprintf(buf, cap, "DE_LOSS_L1_HINGE has no curvature, and the IRLS weight of a margin is no majoriser: no Gauss-Newton matrix");
        return buf;
    }
    const bool reads_floor = spec->kind == DE_LOSS_L1 || spec->kind == DE_LOSS_L1_EPS || spec->kind == DE_LOSS_QUANTILE ||
                             (spec->kind == DE_LOSS_LP && spec->param < 2.0);
    if (!reads_floor) return nullptr;
    if (!(std::isfinite(e_floor) && e_floor > 0.0) || (dtype == DE_F32 && !((float)e_floor > 0.0f))) {
        std::snprintf(buf, cap, "loss_kind %d: e_floor %g must be finite and > 0%s", (int)spec->kind, e_floor, dtype == DE_F32 ? " in Float32" : "");
        return buf;
    }
    return nullptr;
}
// DE_F16 programs evaluate only: every gradient / fused-loss entry point refuses them before it touches an output —
// but de_eval_grad and de_eval_diff serve a program created with DE_OPT_F16_GRAD (DE_REFUSE_F16_NO_GRAD).
int refuse_f16(de_ctx_t *c, const de_program_t *p, const char *what) {
    return fail(c, DE_ERR_UNSUPPORTED, "%s: DE_F16 programs evaluate only (de_eval, de_eval_sum_certificate); no binary16 gradients or losses", what);
}
// ... and so do they complex programs
int refuse_complex(de_ctx_t *c, const char *what) {
    return fail(c, DE_ERR_UNSUPPORTED, "%s: complex (DE_CF32 / DE_CF64) programs evaluate only (de_eval, de_eval_sum_certificate); no complex gradients or losses", what);
}

int de_eval_loss_grad(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                      int mode, const void *y, const void *w, int32_t loss_kind, void *loss, void *dloss,
                      const int64_t *dloss_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_loss_grad");
    const de_loss_spec_t spec{loss_kind, 0, 0.0}; // (de_eval_loss_grad_ex, held to the three kinds this entry point has always taken)
    DE_NOTHROW(c, loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, &spec, loss, dloss, dloss_offsets, ok, nullptr, true));
}
int de_eval_loss_grad_ex(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                         int mode, const void *y, const void *w, const de_loss_spec_t *spec, void *loss, void *dloss,
                         const int64_t *dloss_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_loss_grad");
    DE_NOTHROW(c, loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, spec, loss, dloss, dloss_offsets, ok, nullptr));
}
int de_gn_max_rows(void) { return DE_GN_MAX_ROWS; }
int de_gn_spec_check(const de_loss_spec_t *spec, double e_floor) {
    char buf[160];
    int rc;
    return gn_spec_problem(spec, e_floor, -1, &rc, buf, sizeof buf) ? rc : DE_OK;
}
int de_eval_loss_gn_ex(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                       const void *y, const void *w, const de_loss_spec_t *spec, double e_floor, void *loss, void *dloss,
                       const int64_t *dloss_offsets, void *jtj, const int64_t *jtj_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_loss_gn");
    const GnPlan gn{jtj, jtj_offsets, e_floor};
    DE_NOTHROW(c, loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, spec, loss, dloss, dloss_offsets, ok, nullptr, false, &gn));
}
int de_eval_loss_gn(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                    const void *y, const void *w, void *loss, void *dloss, const int64_t *dloss_offsets,
                    void *jtj, const int64_t *jtj_offsets, uint8_t *ok) {
    const de_loss_spec_t spec{DE_LOSS_L2, 0, 0.0};
    return de_eval_loss_gn_ex(c, p, X, N, ldX, pa, mode, y, w, &spec, 0.0, loss, dloss, dloss_offsets, jtj, jtj_offsets, ok);
}
int de_eval_fit_stats_grad(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                           const void *y, const void *w, double *stats, double *ystats, double *dmom, const int64_t *dmom_offsets,
                           void *jtj, const int64_t *jtj_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_fit_stats_grad");
    const de_loss_spec_t spec{DE_LOSS_L2, 0, 0.0};
    const FitPlan fit{stats, ystats, jtj, jtj_offsets};
    DE_NOTHROW(c, loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, &spec, nullptr, dmom, dmom_offsets, ok, nullptr, false, nullptr, &fit));
}
int loss_grad_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode, const void *y,
                   const void *w, const de_loss_spec_t *spec, void *loss, void *dloss, const int64_t *dloss_offsets, uint8_t *ok,
                   ByClassPlan *plan, bool first_kinds_only, const GnPlan *gn, const FitPlan *fit) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    if (N < 0 || !ok || (p->n_trees > 0 && (!dloss || (N > 0 && (!X || !y))))) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    if (gn && p->n_trees > 0 && (!gn->jtj || !y)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    if (fit && p->n_trees > 0 && (!fit->stats || !fit->ystats || !y)) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    if (ldX < p->n_features) return fail(c, DE_ERR_INVALID_ARG, "ldX < n_features");
    if (mode != DE_GRAD_VARIABLE && mode != DE_GRAD_CONSTANT && mode != DE_GRAD_BOTH) return fail(c, DE_ERR_INVALID_ARG, "bad gradient mode");
    if (first_kinds_only && spec->kind != DE_LOSS_L2 && spec->kind != DE_LOSS_L1 && spec->kind != DE_LOSS_PULLBACK)
        return fail(c, DE_ERR_INVALID_ARG, "unknown loss_kind %d", (int)spec->kind);
    char why[160];
    if (loss_spec_problem(spec, 1, why, sizeof why)) return fail(c, DE_ERR_INVALID_ARG, "%s", why);
    int rc = DE_OK;
    if (gn && gn_spec_problem(spec, gn->e_floor, p->dtype, &rc, why, sizeof why)) return fail(c, rc, "%s", why);
    rc = check_param_args(c, p, pa, N);
    if (rc != DE_OK) return rc;
    if (p->n_trees == 0) return DE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    // per-tree geometry: tree t owns reduction columns col_off[t] (loss) .. col_off[t] + n_grad[t]
    std::vector<int32_t> ng((size_t)p->n_trees);
    void *const jtj_out = gn ? gn->jtj : (fit ? fit->jtj : nullptr); // the matrices' buffer and offsets, of either plan
    const int64_t *const jtj_offsets = gn ? gn->jtj_offsets : (fit ? fit->jtj_offsets : nullptr);
    const int rows_per_g = fit ? 3 : 1; // entries of dloss per gradient row (fit: D, P, Q)
    const size_t des = fit ? sizeof(double) : (p->dtype == DE_F32 ? 4 : 8); // element size of dloss
    std::vector<int64_t> coloff((size_t)p->n_trees + 1, 0), doff((size_t)p->n_trees), joff(jtj_out ? (size_t)p->n_trees : 0);
    int64_t span = 0, run = 0, jspan = 0, jrun = 0;
    int32_t maxg = 0;
    for (int64_t t = 0; t < p->n_trees; t++) {
        const int32_t g = (int32_t)de_program_n_grad(p, t, mode);
        ng[(size_t)t] = g;
        maxg = std::max(maxg, g);
        const int64_t off = dloss_offsets ? dloss_offsets[t] : run;
        if (off < 0) return fail(c, DE_ERR_INVALID_ARG, "negative dloss offset");
        doff[(size_t)t] = off;
        run += (int64_t)rows_per_g * g;
        span = std::max(span, off + (int64_t)rows_per_g * g);
        coloff[(size_t)t + 1] = coloff[(size_t)t] + (fit ? FIT_COLS + 3 * g : 1 + g);
        if (jtj_out) { // ... then the lower triangle of its Gauss-Newton matrix, where the tree's rows share a window
            const int64_t jo = jtj_offsets ? jtj_offsets[t] : jrun;
            if (jo < 0) return fail(c, DE_ERR_INVALID_ARG, "negative jtj offset");
            joff[(size_t)t] = jo;
            jrun += (int64_t)g * g;
            jspan = std::max(jspan, jo + (int64_t)g * g);
            if (g <= DE_GN_MAX_ROWS) coloff[(size_t)t + 1] += (int64_t)g * (g + 1) / 2;
        }
    }
    const int64_t n_cols = coloff[(size_t)p->n_trees];
    const bool ok_dev = is_device_ptr(ok);
    if (N == 0 && fit) { // W == 0: the means are NaN, every moment 0; NaN throughout where a constant already fails the flag
        rc = consts_materialise(p); // (from the host's flags: §3.5)
        if (rc != DE_OK) return rc;
        const double nan = std::nan("");
        std::vector<double> zs((size_t)p->n_trees * 3), zd((size_t)std::max<int64_t>(span, 1));
        for (int64_t t = 0; t < p->n_trees; t++) {
            const double v = p->host_ok_grad[(size_t)t] ? 0.0 : nan;
            zs[3 * (size_t)t] = nan;
            zs[3 * (size_t)t + 1] = zs[3 * (size_t)t + 2] = v;
            for (int32_t k = 0; k < 3 * ng[(size_t)t]; k++) zd[(size_t)(doff[(size_t)t] + k)] = v;
        }
        const double ys[3] = {0.0, nan, 0.0};
        HIP_TRY(c, hipMemcpy(fit->stats, zs.data(), zs.size() * sizeof(double), hipMemcpyDefault));
        HIP_TRY(c, hipMemcpy(fit->ystats, ys, sizeof ys, hipMemcpyDefault));
        for (int64_t t = 0; t < p->n_trees; t++)
            if (ng[(size_t)t] > 0)
                HIP_TRY(c, hipMemcpy(static_cast<double *>(dloss) + doff[(size_t)t], zd.data() + doff[(size_t)t], (size_t)3 * (size_t)ng[(size_t)t] * sizeof(double),
                                     hipMemcpyDefault));
        if (jtj_out) {
            std::vector<unsigned char> zj((size_t)std::max<int64_t>(jspan, 1) * es);
            for (int64_t t = 0; t < p->n_trees; t++) {
                const int64_t gg = (int64_t)ng[(size_t)t] * ng[(size_t)t];
                const double v = p->host_ok_grad[(size_t)t] && ng[(size_t)t] <= fit->rows_n0 ? 0.0 : nan;
                for (int64_t e = 0; e < gg; e++) {
                    if (p->dtype == DE_F32) reinterpret_cast<float *>(zj.data())[joff[(size_t)t] + e] = (float)v;
                    else reinterpret_cast<double *>(zj.data())[joff[(size_t)t] + e] = v;
                }
                if (gg > 0) HIP_TRY(c, hipMemcpy(static_cast<char *>(jtj_out) + (size_t)joff[(size_t)t] * es, zj.data() + (size_t)joff[(size_t)t] * es, (size_t)gg * es, hipMemcpyDefault));
            }
        }
        HIP_TRY(c, hipMemcpy(ok, p->host_ok_grad.data(), (size_t)p->n_trees, hipMemcpyDefault));
        return DE_OK;
    }
    if (N == 0) { // empty sums: 0, or NaN where a constant already fails the flag
        rc = consts_materialise(p); // (from the host's flags: §3.5)
        if (rc != DE_OK) return rc;
        std::vector<unsigned char> zl((size_t)p->n_trees * es), zd((size_t)std::max<int64_t>(span, 1) * es);
        auto put = [&](unsigned char *b, int64_t i, double v) {
            if (p->dtype == DE_F32) reinterpret_cast<float *>(b)[i] = (float)v;
            else reinterpret_cast<double *>(b)[i] = v;
        };
        for (int64_t t = 0; t < p->n_trees; t++) {
            const double v = p->host_ok_grad[(size_t)t] ? 0.0 : std::nan("");
            put(zl.data(), t, v);
            for (int32_t k = 0; k < ng[(size_t)t]; k++) put(zd.data(), doff[(size_t)t] + k, v);
        }
        if (gn) { // (a wider tree's block is NaN whatever N is)
            std::vector<unsigned char> zj((size_t)std::max<int64_t>(jspan, 1) * es);
            for (int64_t t = 0; t < p->n_trees; t++) {
                const int64_t gg = (int64_t)ng[(size_t)t] * ng[(size_t)t];
                const double v = p->host_ok_grad[(size_t)t] && ng[(size_t)t] <= gn->rows_n0 ? 0.0 : std::nan("");
                for (int64_t e = 0; e < gg; e++) put(zj.data(), joff[(size_t)t] + e, v);
            }
            for (int64_t t = 0; t < p->n_trees; t++)
                if (ng[(size_t)t] > 0)
                    HIP_TRY(c, hipMemcpy(static_cast<char *>(gn->jtj) + (size_t)joff[(size_t)t] * es, zj.data() + (size_t)joff[(size_t)t] * es,
                                         (size_t)ng[(size_t)t] * (size_t)ng[(size_t)t] * es, hipMemcpyDefault));
        }
        for (int64_t t = 0; t < p->n_trees; t++) // only the entries each tree owns are written
            if (ng[(size_t)t] > 0)
                HIP_TRY(c, hipMemcpy(static_cast<char *>(dloss) + (size_t)doff[(size_t)t] * es, zd.data() + (size_t)doff[(size_t)t] * es,
                                     (size_t)ng[(size_t)t] * es, hipMemcpyDefault));
        if (loss) HIP_TRY(c, hipMemcpy(loss, zl.data(), zl.size(), hipMemcpyDefault));
        HIP_TRY(c, hipMemcpy(ok, p->host_ok_grad.data(), (size_t)p->n_trees, hipMemcpyDefault));
        return DE_OK;
    }
    const bool timing = getenv("DE_DEBUG_TIMING") != nullptr;
    const auto tg0 = std::chrono::steady_clock::now();
    rc = ensure_generic_code(c, p);
    if (rc) return rc;
    const auto tg1 = std::chrono::steady_clock::now();

    Staged sX, sY, sW, sLoss, sDl, sOk, sPar, sCls, sJ, sStats, sYstats;
    rc = stage_in(c, c->sX, X, (size_t)ldX * (size_t)N * es, &sX);
    if (rc) return rc;
    rc = stage_in(c, c->sY, y, (size_t)N * es, &sY);
    if (rc) return rc;
    if (w) {
        rc = stage_in(c, c->sW, w, (size_t)N * es, &sW);
        if (rc) return rc;
    }
    if (loss) {
        rc = stage_out(c, c->sLoss, loss, (size_t)p->n_trees * es, &sLoss);
        if (rc) return rc;
    }
    rc = stage_out(c, c->sDloss, dloss, (size_t)std::max<int64_t>(span, 1) * des, &sDl);
    if (rc) return rc;
    if (jtj_out) {
        rc = stage_out(c, c->sJtj, jtj_out, (size_t)std::max<int64_t>(jspan, 1) * es, &sJ);
        if (rc) return rc;
    }
    if (fit) {
        rc = stage_out(c, c->sStats, fit->stats, (size_t)p->n_trees * 3 * sizeof(double), &sStats);
        if (rc) return rc;
        rc = stage_out(c, c->sYstats, fit->ystats, 3 * sizeof(double), &sYstats);
        if (rc) return rc;
    }
    if (ok_dev) sOk.dev = ok;
    else {
        HIP_TRY(c, c->sOk.reserve((size_t)p->n_trees));
        sOk.dev = c->sOk.p;
        sOk.staged = true;
    }
    int64_t n_tiles = (N + 255) / 256;
    std::vector<int64_t> tile_range, class_tile0; // by-class: (first, last) sample of every class-aligned tile; first tile of every class
    if (plan) {
        class_tile0.assign((size_t)plan->C + 1, 0);
        for (int64_t k = 0; k < plan->C; k++) {
            const int64_t j0 = plan->class_starts[k], j1 = plan->class_starts[k + 1];
            for (int64_t b = j0; b < j1; b += 256) {
                tile_range.push_back(b);
                tile_range.push_back(j1 - 1);
            }
            class_tile0[(size_t)k + 1] = (int64_t)(tile_range.size() / 2);
        }
        n_tiles = (int64_t)(tile_range.size() / 2);
    }
    HIP_TRY(c, c->sPartial.reserve((size_t)n_tiles * (size_t)n_cols * 4 * es));
    // (by class: three regions — the finish passes of the classes run on the caller's stream and two side streams, launch_loss_grad_finish_ranges)
    const size_t seg_region = (size_t)loss_segments(n_tiles) * (size_t)n_cols * 4 * sizeof(double);
    const int seg_regions = plan ? 3 : 1;
    // (fit statistics: the three per-tile arrays of the pre-pass over y / w, then the recombination's segment sums)
    const size_t fit_pre_bytes = (size_t)3 * (size_t)n_tiles * sizeof(double);
    HIP_TRY(c, c->sSeg.reserve(fit ? fit_pre_bytes + fit_grad_seg_bytes(p->n_trees, n_cols, N) : seg_region * (size_t)seg_regions));
    HIP_TRY(c, c->sNg.reserve(ng.size() * sizeof(int32_t)));
    HIP_TRY(c, c->sColOff.reserve(coloff.size() * sizeof(int64_t)));
    HIP_TRY(c, c->sDoff.reserve(doff.size() * sizeof(int64_t)));
    // (behind a device set the initial flags are the device's: §3.5)
    if (p->consts_dev_ahead) HIP_TRY(c, hipMemcpyAsync(sOk.dev, p->d_ok_grad, (size_t)p->n_trees, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(c, hipMemcpyAsync(sOk.dev, p->host_ok_grad.data(), (size_t)p->n_trees, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->sNg.p, ng.data(), ng.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->sColOff.p, coloff.data(), coloff.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->sDoff.p, doff.data(), doff.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (jtj_out) {
        HIP_TRY(c, c->sJoff.reserve(joff.size() * sizeof(int64_t)));
        HIP_TRY(c, hipMemcpyAsync(c->sJoff.p, joff.data(), joff.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    if (p->uses_params) {
        rc = stage_in(c, c->sParams, pa->params, (size_t)pa->ld_params * (size_t)pa->n_classes * es, &sPar);
        if (rc) return rc;
        rc = stage_in(c, c->sClasses, pa->classes, (size_t)N * (pa->classes_is_i64 ? 8 : 4), &sCls);
        if (rc) return rc;
    }
    double ys_host[3] = {0.0, 0.0, 0.0};
    if (fit) { // the pre-pass over y / w: {W, mean_y, M2_y}; the kernels take T(mean_y) by value
        HIP_TRY(c, launch_fit_ystats(p->dtype, sY.dev, w ? sW.dev : nullptr, N, static_cast<double *>(sYstats.dev), c->sSeg.p, c->stream));
        HIP_TRY(c, hipMemcpyAsync(ys_host, sYstats.dev, sizeof ys_host, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the pageable host vectors above must outlive their async copies

    LossArgs la;
    std::memset(&la, 0, sizeof la);
    la.y = sY.dev;
    la.w = w ? sW.dev : nullptr;
    la.kind = spec->kind;
    la.param = spec->param;
    la.e_floor = gn ? gn->e_floor : 0.0;
    la.partial = c->sPartial.p;
    la.seg_sum = c->sSeg.p;
    la.loss = loss ? sLoss.dev : nullptr;
    if (fit) {
        la.kind = (jtj_out ? FIT_MODE_JTJ : FIT_MODE_PLAIN) - 1;
        la.param = ys_host[1];
        la.stats = static_cast<double *>(sStats.dev);
        la.ystats = static_cast<double *>(sYstats.dev);
    }
    GradArgs g;
    std::memset(&g, 0, sizeof g);
    g.generic_code = p->d_gcode;
    g.e.code_off = p->d_gcode_off;
    g.e.n_trees = (int32_t)p->n_trees;
    g.e.skip_flagged = !(p->options & DE_OPT_FULL_EVAL) && tree_skip_enabled(); // (the gradient entry points always test validity)
    if (c->sPrio.reserve((size_t)3 * DE_PRIO_MAX_F * sizeof(unsigned long long)) == hipSuccess) g.e.prio_keys = c->sPrio.p; // priority tiles (de_kernels.hip)
    g.prio_ready = false;
    g.e.prio_keys_ready = !sX.staged && g.e.prio_keys && dataset_keys(c, p->dtype, X, N, ldX, p->n_features, &g.e.prio_keys);
    g.e.n_slots = p->n_slots;
    g.e.uses_params = p->uses_params;
    g.e.X = sX.dev;
    g.e.N = N;
    g.e.ldX = ldX;
    g.e.F = p->n_features;
    g.e.out = nullptr;
    g.e.ld_out = N;
    g.e.ok = static_cast<uint8_t *>(sOk.dev);
    if (p->uses_params) {
        g.e.params = sPar.dev;
        g.e.ld_params = pa->ld_params;
        g.e.n_classes = pa->n_classes;
        g.e.classes = sCls.dev;
        g.e.classes_is_i64 = pa->classes_is_i64;
        g.e.class_base = pa->class_base;
    }
    g.mode = mode;
    g.P = p->n_params;
    g.grad = nullptr;
    g.grad_off = nullptr;
    g.n_grad = static_cast<const int32_t *>(c->sNg.p);
    g.max_grad = maxg;
    g.diff_direction = -1;
    g.loss = &la;
    g.col_off = static_cast<const int64_t *>(c->sColOff.p);
    g.n_cols = n_cols;
    g.dloss = sDl.dev;
    g.dloss_off = static_cast<const int64_t *>(c->sDoff.p);
    if (fit) { // always forward duals as well
        g.fit = true;
        g.fit_jtj = jtj_out != nullptr;
        g.fit_seg = reinterpret_cast<double *>(static_cast<char *>(c->sSeg.p) + fit_pre_bytes);
        if (jtj_out) {
            g.jtj = sJ.dev;
            g.jtj_off = static_cast<const int64_t *>(c->sJoff.p);
        }
    } else if (gn) { // always forward duals: the reverse kernel has no dual rows
        g.gn = true;
        g.jtj = sJ.dev;
        g.jtj_off = static_cast<const int64_t *>(c->sJoff.p);
    } else {
        rc = ensure_rev_threaded(c, p, mode, &g);
        if (rc) return rc;
    }
    if (plan && !g.rev_code) return DE_OK; // forward duals: the caller runs one call per class (plan->done stays false)
    if (plan) {
        HIP_TRY(c, c->sBcTiles.reserve(std::max<size_t>(tile_range.size(), 2) * sizeof(int64_t)));
        if (!tile_range.empty())
            HIP_TRY(c, hipMemcpyAsync(c->sBcTiles.p, tile_range.data(), tile_range.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // tile_range is pageable
        g.rev_tile_range = static_cast<const int64_t *>(c->sBcTiles.p);
        g.rev_n_tiles = n_tiles;
    }
    if (!g.rev_code) {
        rc = ensure_grad_threaded(c, p, mode, ng, N, &g);
        if (rc) return rc;
        if (!g.threaded_code && grad_tape_lds_bytes(p->n_features, p->n_slots, grad_window(maxg), es) > 160 * 1024) // (the tape kernel launches: grad_impl)
            return fail(c, DE_ERR_UNSUPPORTED, "gradient kernel: LDS footprint too large for this tree shape");
    }
    if (timing) {
        const auto tg2 = std::chrono::steady_clock::now();
        fprintf(stderr, "loss_grad host us: generic code %ld, staging + threaded/reverse code %ld\n",
                (long)std::chrono::duration_cast<std::chrono::microseconds>(tg1 - tg0).count(),
                (long)std::chrono::duration_cast<std::chrono::microseconds>(tg2 - tg1).count());
    }
    if (!c->nested) HIP_TRY(c, time_begin(c));
    if (g.rev_code) HIP_TRY(c, launch_rev_threaded(p->dtype, g, c->stream, &c->last_kernel));
    else HIP_TRY(c, launch_grad(p->dtype, g, c->stream, &c->last_kernel));
    if (plan) { // one pair of finish passes per class over its own tiles
        HIP_TRY(c, launch_loss_grad_finish_ranges(p->dtype, g, plan->C, class_tile0.data(), plan->loss_c, (size_t)p->n_trees * es, plan->dloss_c,
                                                  (size_t)plan->span * es, seg_region, seg_regions, c->stream));
        plan->done = true;
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (sLoss.staged) HIP_TRY(c, hipMemcpyAsync(loss, sLoss.dev, (size_t)p->n_trees * es, hipMemcpyDeviceToHost, c->stream));
    if (sDl.staged)
        for (int64_t t = 0; t < p->n_trees; t++)
            if (ng[(size_t)t] > 0)
                HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(dloss) + (size_t)doff[(size_t)t] * des,
                                          static_cast<char *>(sDl.dev) + (size_t)doff[(size_t)t] * des, (size_t)rows_per_g * (size_t)ng[(size_t)t] * des,
                                          hipMemcpyDeviceToHost, c->stream));
    if (sStats.staged) HIP_TRY(c, hipMemcpyAsync(fit->stats, sStats.dev, (size_t)p->n_trees * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (sYstats.staged) HIP_TRY(c, hipMemcpyAsync(fit->ystats, sYstats.dev, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (sJ.staged)
        for (int64_t t = 0; t < p->n_trees; t++)
            if (ng[(size_t)t] > 0)
                HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(jtj_out) + (size_t)joff[(size_t)t] * es,
                                          static_cast<char *>(sJ.dev) + (size_t)joff[(size_t)t] * es,
                                          (size_t)ng[(size_t)t] * (size_t)ng[(size_t)t] * es, hipMemcpyDeviceToHost, c->stream));
    if (sOk.staged) HIP_TRY(c, hipMemcpyAsync(ok, sOk.dev, (size_t)p->n_trees, hipMemcpyDeviceToHost, c->stream));
    if (sX.staged || sY.staged || sW.staged || sLoss.staged || sDl.staged || sJ.staged || sOk.staged || sPar.staged || sCls.staged || sStats.staged || sYstats.staged)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DE_OK;
}

static int by_class_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX,
                               const de_param_args_t *pa, int mode, const void *y, const void *w, const de_loss_spec_t *spec,
                               const int64_t *class_starts, void *loss, void *dloss, const int64_t *dloss_offsets,
                               void *dparams, uint8_t *ok, bool first_kinds_only = false);
int de_eval_loss_grad_by_class(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX,
                               const de_param_args_t *pa, int mode, const void *y, const void *w, int32_t loss_kind,
                               const int64_t *class_starts, void *loss, void *dloss, const int64_t *dloss_offsets,
                               void *dparams, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_loss_grad_by_class");
    const de_loss_spec_t spec{loss_kind, 0, 0.0};
    DE_NOTHROW(c, by_class_impl(c, p, X, N, ldX, pa, mode, y, w, &spec, class_starts, loss, dloss, dloss_offsets, dparams, ok, true));
}
int de_eval_loss_grad_by_class_ex(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX,
                                  const de_param_args_t *pa, int mode, const void *y, const void *w, const de_loss_spec_t *spec,
                                  const int64_t *class_starts, void *loss, void *dloss, const int64_t *dloss_offsets,
                                  void *dparams, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_loss_grad_by_class");
    DE_NOTHROW(c, by_class_impl(c, p, X, N, ldX, pa, mode, y, w, spec, class_starts, loss, dloss, dloss_offsets, dparams, ok));
}
static int by_class_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX,
                               const de_param_args_t *pa, int mode, const void *y, const void *w, const de_loss_spec_t *spec,
                               const int64_t *class_starts, void *loss, void *dloss, const int64_t *dloss_offsets,
                               void *dparams, uint8_t *ok, bool first_kinds_only) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    if (p->n_params <= 0 || !pa) return fail(c, DE_ERR_INVALID_ARG, "not a parametric population (n_params = 0 or no parameter arguments)");
    // the spec first, as loss_grad_impl: before any reservation or copy, and whatever path (one pass, per class, no tree, no sample) follows
    if (first_kinds_only && spec && spec->kind != DE_LOSS_L2 && spec->kind != DE_LOSS_L1 && spec->kind != DE_LOSS_PULLBACK)
        return fail(c, DE_ERR_INVALID_ARG, "unknown loss_kind %d", (int)spec->kind);
    char why[160];
    if (loss_spec_problem(spec, 1, why, sizeof why)) return fail(c, DE_ERR_INVALID_ARG, "%s", why);
    if (mode != DE_GRAD_VARIABLE && mode != DE_GRAD_BOTH)
        return fail(c, DE_ERR_INVALID_ARG, "by-class reduction needs a mode with parameter rows (DE_GRAD_VARIABLE / DE_GRAD_BOTH)");
    if (!pa->params || !pa->classes || pa->ld_params < p->n_params || pa->n_classes <= 0)
        return fail(c, DE_ERR_INVALID_ARG, "bad parameter arguments");
    if (N < 0 || !ok || !class_starts || (p->n_trees > 0 && (!dloss || !dparams))) return fail(c, DE_ERR_INVALID_ARG, "null buffer");
    const int64_t C = pa->n_classes;
    if (class_starts[0] != 0 || class_starts[C] != N) return fail(c, DE_ERR_INVALID_ARG, "class_starts must run from 0 to N");
    for (int64_t k = 0; k < C; k++)
        if (class_starts[k + 1] < class_starts[k]) return fail(c, DE_ERR_INVALID_ARG, "class_starts must be non-decreasing");
    if (p->n_trees == 0) return DE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    const int P = p->n_params;
    std::vector<int32_t> ng((size_t)p->n_trees);
    std::vector<int64_t> doff((size_t)p->n_trees);
    int64_t span = 0, run = 0;
    for (int64_t t = 0; t < p->n_trees; t++) {
        const int32_t g = (int32_t)de_program_n_grad(p, t, mode);
        ng[(size_t)t] = g;
        const int64_t off = dloss_offsets ? dloss_offsets[t] : run;
        if (off < 0) return fail(c, DE_ERR_INVALID_ARG, "negative dloss offset");
        doff[(size_t)t] = off;
        run += g;
        span = std::max(span, off + g);
    }
    span = std::max<int64_t>(span, 1);
    HIP_TRY(c, c->sBcLoss.reserve((size_t)C * (size_t)p->n_trees * es));
    HIP_TRY(c, c->sBcDloss.reserve((size_t)C * (size_t)span * es));
    HIP_TRY(c, c->sBcOk.reserve((size_t)C * (size_t)p->n_trees));
    HIP_TRY(c, c->sBcNg.reserve(ng.size() * sizeof(int32_t)));
    HIP_TRY(c, c->sBcDoff.reserve(doff.size() * sizeof(int64_t)));
    HIP_TRY(c, hipMemcpyAsync(c->sBcNg.p, ng.data(), ng.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->sBcDoff.p, doff.data(), doff.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    // dloss entries no tree owns (caller-chosen offsets) are never read by the combine pass
    HIP_TRY(c, hipMemsetAsync(c->sBcDloss.p, 0, (size_t)C * (size_t)span * es, c->stream));
    HIP_TRY(c, time_begin(c));
    ByClassPlan plan{class_starts, C, span, c->sBcLoss.p, c->sBcDloss.p, false};
    bool shared_ok = false; // one pass: a single flag array instead of one per class
    {
        const char *env1 = getenv("DE_BY_CLASS_ONE_PASS");
        if (!(env1 && *env1 == '0') && N > 0) {
            NestGuard nest(c);
            const int rc1 = loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, spec, c->sBcLoss.p, c->sBcDloss.p, dloss_offsets,
                                           static_cast<uint8_t *>(c->sBcOk.p), &plan, first_kinds_only);
            if (rc1 != DE_OK) return rc1;
            shared_ok = plan.done;
        }
    }
    int rc = DE_OK;
    const size_t cls_es = pa->classes_is_i64 ? 8 : 4;
    {
    NestGuard nest(c);
    for (int64_t k = 0; k < C && rc == DE_OK && !plan.done; k++) {
        const int64_t j0 = class_starts[k], n = class_starts[k + 1] - j0;
        de_param_args_t sub = *pa;
        sub.classes = static_cast<const char *>(pa->classes) + (size_t)j0 * cls_es;
        rc = de_eval_loss_grad_ex(c, p, static_cast<const char *>(X) + (size_t)j0 * (size_t)ldX * es, n, ldX, &sub, mode,
                               y ? static_cast<const char *>(y) + (size_t)j0 * es : nullptr,
                               w ? static_cast<const char *>(w) + (size_t)j0 * es : nullptr, spec,
                               static_cast<char *>(c->sBcLoss.p) + (size_t)k * (size_t)p->n_trees * es,
                               static_cast<char *>(c->sBcDloss.p) + (size_t)k * (size_t)span * es, dloss_offsets,
                               static_cast<uint8_t *>(c->sBcOk.p) + (size_t)k * (size_t)p->n_trees);
    }
    }
    if (rc != DE_OK) return rc;
    Staged sLoss, sDl, sDp, sOk;
    if (loss) {
        rc = stage_out(c, c->sLoss, loss, (size_t)p->n_trees * es, &sLoss);
        if (rc) return rc;
    }
    rc = stage_out(c, c->sDloss, dloss, (size_t)span * es, &sDl);
    if (rc) return rc;
    const size_t dp_bytes = (size_t)p->n_trees * (size_t)C * (size_t)P * es;
    rc = stage_out(c, c->sBcOut, dparams, dp_bytes, &sDp);
    if (rc) return rc;
    rc = stage_out(c, c->sOk, ok, (size_t)p->n_trees, &sOk);
    if (rc) return rc;
    ByClassArgs a;
    a.loss_c = c->sBcLoss.p;
    a.dloss_c = c->sBcDloss.p;
    a.ok_c = static_cast<const uint8_t *>(c->sBcOk.p);
    a.n_classes = (int32_t)C;
    a.ok_stride = shared_ok ? 0 : p->n_trees;
    a.n_params = P;
    a.n_trees = p->n_trees;
    a.span = span;
    a.n_grad = static_cast<const int32_t *>(c->sBcNg.p);
    a.dloss_off = static_cast<const int64_t *>(c->sBcDoff.p);
    a.loss = loss ? sLoss.dev : nullptr;
    a.dloss = sDl.dev;
    a.dparams = sDp.dev;
    a.ok = static_cast<uint8_t *>(sOk.dev);
    HIP_TRY(c, launch_by_class_combine(p->dtype, a, c->stream));
    HIP_TRY(c, time_end(c));
    if (sLoss.staged) HIP_TRY(c, hipMemcpyAsync(loss, sLoss.dev, (size_t)p->n_trees * es, hipMemcpyDeviceToHost, c->stream));
    if (sDl.staged)
        for (int64_t t = 0; t < p->n_trees; t++)
            if (ng[(size_t)t] > 0)
                HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(dloss) + (size_t)doff[(size_t)t] * es,
                                          static_cast<char *>(sDl.dev) + (size_t)doff[(size_t)t] * es, (size_t)ng[(size_t)t] * es,
                                          hipMemcpyDeviceToHost, c->stream));
    if (sDp.staged) HIP_TRY(c, hipMemcpyAsync(dparams, sDp.dev, dp_bytes, hipMemcpyDeviceToHost, c->stream));
    if (sOk.staged) HIP_TRY(c, hipMemcpyAsync(ok, sOk.dev, (size_t)p->n_trees, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // ng/doff (pageable) were copied asynchronously
    return DE_OK;
}

int de_eval_grad(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                 int mode, void *out, int64_t ld_out, void *grad, const int64_t *grad_offsets, uint8_t *ok) {
    DE_REFUSE_F16_NO_GRAD("de_eval_grad");
    DE_NOTHROW(c, grad_impl(c, p, X, N, ldX, pa, mode, -1, out, ld_out, grad, grad_offsets, ok));
}

int de_eval_pullback_dX(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                        const void *dY, void *dX, const int64_t *dX_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_pullback_dX");
    if (c && N > 0 && !dY) return fail(c, DE_ERR_INVALID_ARG, "null cotangent dY");
    DE_NOTHROW(c, grad_impl(c, p, X, N, ldX, pa, DE_GRAD_VARIABLE, -1, nullptr, N, dX, dX_offsets, ok, dY));
}

int de_eval_diff(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, int32_t direction, void *out,
                 void *dout, int64_t ld_out, uint8_t *ok) {
    DE_REFUSE_F16_NO_GRAD("de_eval_diff");
    if (direction < 0) return fail(c, DE_ERR_INVALID_ARG, "direction < 0");
    if (p && p->uses_params) return fail(c, DE_ERR_UNSUPPORTED, "eval_diff on parametric trees");
    DE_NOTHROW(c, grad_impl(c, p, X, N, ldX, nullptr, DE_GRAD_VARIABLE, direction, out, ld_out, dout, nullptr, ok));
}

// ---- de_eval_loss_gn_wide / de_eval_fit_stats_grad_wide (kernels: de_gn_wide.hip) ----
int de_gn_wide_max_rows(void) { return DE_GN_WIDE_MAX_ROWS; }

void gn_wide_release(de_program *p) {
    if (!p || !p->gnw) return;
    GnWideCache *gw = p->gnw;
    p->gnw = nullptr;
    if (gw->sub) de_program_destroy(gw->sub);
    if (gw->d_cidx) (void)hipFree(gw->d_cidx);
    if (gw->d_tab) (void)hipFree(gw->d_tab);
    delete gw;
}

// The hidden sub-program of the wide trees in `mode` (same dtype, features, parameters and options: de_eval_grad's rows of a tree do not
// depend on its neighbours).  Its constants are placeholders until the first mirror (gn_wide_mirror).
static int gn_wide_cache(de_ctx *c, de_program *p, int mode, const std::vector<int32_t> &ng) {
    if (p->gnw && p->gnw->mode == mode) return DE_OK;
    if (p->in_noff.size() != (size_t)p->n_trees + 1)
        return fail(c, DE_ERR_UNSUPPORTED, "de_eval_loss_gn_wide: the program keeps no input to build the wide trees' program from");
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (queued work may still run the sub-program of another mode)
    gn_wide_release(p);
    std::unique_ptr<GnWideCache> gw(new GnWideCache());
    std::vector<de_tape_node_t> nodes;
    std::vector<int64_t> noff{0}, coff{0}, cidx;
    for (int64_t t = 0; t < p->n_trees; t++) {
        const int32_t g = ng[(size_t)t];
        if (g <= DE_GN_MAX_ROWS || g > DE_GN_WIDE_MAX_ROWS) continue;
        gw->trees.push_back((int32_t)t);
        gw->rows.push_back(g);
        nodes.insert(nodes.end(), p->in_nodes.begin() + p->in_noff[(size_t)t], p->in_nodes.begin() + p->in_noff[(size_t)t + 1]);
        noff.push_back((int64_t)nodes.size());
        for (int64_t k = p->const_off[(size_t)t]; k < p->const_off[(size_t)t + 1]; k++) cidx.push_back(k);
        coff.push_back((int64_t)cidx.size());
    }
    gw->n_consts = (int64_t)cidx.size();
    const size_t ies = dtype_bytes(p->io);
    std::vector<unsigned char> ones(std::max<size_t>(cidx.size(), 1) * ies);
    for (size_t k = 0; k < cidx.size(); k++) store_elem(p->io, ones.data(), k, 1.0);
    const int rc = de_program_create(c, p->io, nodes.data(), noff.data(), (int64_t)gw->trees.size(), ones.data(), coff.data(), p->n_features, p->n_params,
                                     p->options, &gw->sub);
    if (rc != DE_OK) return rc;
    if (!cidx.empty()) {
        hipError_t st = hipMalloc(reinterpret_cast<void **>(&gw->d_cidx), cidx.size() * sizeof(int64_t));
        if (st == hipSuccess) st = hipMemcpy(gw->d_cidx, cidx.data(), cidx.size() * sizeof(int64_t), hipMemcpyHostToDevice);
        if (st != hipSuccess) {
            (void)hipGetLastError();
            de_program_destroy(gw->sub);
            if (gw->d_cidx) (void)hipFree(gw->d_cidx);
            return fail(c, DE_ERR_HIP, "de_eval_loss_gn_wide: constant index table: %s", hipGetErrorString(st));
        }
    }
    gw->mode = mode;
    p->gnw = gw.release();
    return DE_OK;
}

// Samples per chunk (de_gn_wide.h): (rows + n_wide) * chunk * es <= 256 MiB, a multiple of 256, or DE_GN_WIDE_CHUNK rounded up to 64
static int64_t gn_wide_chunk(int64_t N, int64_t rows, int64_t n_wide, size_t es) {
    if (const char *env = getenv("DE_GN_WIDE_CHUNK")) {
        const long long v = atoll(env);
        if (v > 0) return std::min<int64_t>((int64_t)((v + 63) / 64 * 64), (N + 63) / 64 * 64);
    }
    const int64_t per = std::max<int64_t>((rows + n_wide) * (int64_t)es, 1);
    int64_t chunk = ((int64_t)256 << 20) / per / 256 * 256;
    chunk = std::max<int64_t>(chunk, 256);
    return std::min<int64_t>(chunk, (N + 255) / 256 * 256);
}

// What a wide call knows of its trees before anything runs: the widths in `mode`, the blocks' offsets, and the trees of 9 .. 32 rows
struct GnWideScan {
    std::vector<int32_t> ng;
    std::vector<int64_t> joff;
    int64_t n_wide = 0, rows = 0, tri = 0, jspan = 0;
    bool mode_ok = false, neg = false; // neg: a negative offset (refused by the narrow call)
};
static GnWideScan gn_wide_scan(const de_program_t *p, int mode, const int64_t *jtj_offsets, const int64_t *dloss_offsets) {
    GnWideScan sc;
    sc.mode_ok = mode == DE_GRAD_VARIABLE || mode == DE_GRAD_CONSTANT || mode == DE_GRAD_BOTH;
    sc.ng.assign((size_t)p->n_trees, 0);
    sc.joff.assign((size_t)p->n_trees, 0);
    int64_t jrun = 0;
    for (int64_t t = 0; t < p->n_trees && sc.mode_ok; t++) {
        const int32_t g = (int32_t)de_program_n_grad(p, t, mode);
        sc.ng[(size_t)t] = g;
        sc.joff[(size_t)t] = jtj_offsets ? jtj_offsets[t] : jrun;
        sc.neg = sc.neg || sc.joff[(size_t)t] < 0 || (dloss_offsets && dloss_offsets[t] < 0);
        jrun += (int64_t)g * g;
        sc.jspan = std::max(sc.jspan, sc.joff[(size_t)t] + (int64_t)g * g);
        if (g > DE_GN_MAX_ROWS && g <= DE_GN_WIDE_MAX_ROWS) { sc.n_wide++; sc.rows += g; sc.tri += (int64_t)g * (g + 1) / 2; }
    }
    return sc;
}

// The wide route behind either narrow call (de_eval_loss_gn_wide: a GnPlan, de_eval_fit_stats_grad_wide: a FitPlan).  The inputs are staged
// once, narrow(Xd, yd, wd, pargs, jtj_d, ok_d) runs the narrow call on them — everything but the wide blocks, into the device images of
// jtj and ok — and then the wide trees' constants, chunks, Gram matrices and folds follow, which do not depend on which plan ran: (spec,
// e_floor) alone select the curvature weight ({DE_LOSS_L2, 0, 0}: c = 1).  sc.n_wide > 0, N > 0, and arguments the narrow call takes.
using GnWideNarrow = std::function<int(const void *Xd, const void *yd, const void *wd, const de_param_args_t *pargs, void *jtj_d, uint8_t *ok_d)>;
static int gn_wide_run(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode, const void *y,
                       const void *w, const de_loss_spec_t *spec, double e_floor, void *jtj, uint8_t *ok, const GnWideScan &sc,
                       const GnWideNarrow &narrow) {
    int rc = check_param_args(c, p, pa, N);
    if (rc != DE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = gn_wide_cache(c, p, mode, sc.ng);
    if (rc != DE_OK) return rc;
    GnWideCache *gw = p->gnw;
    const size_t es = p->dtype == DE_F32 ? 4 : 8, nt = (size_t)p->n_trees, nc = p->consts.size();
    FitInputs in; // (staged once for the narrow call and every chunk, as the fits do)
    if ((rc = stage_fit_inputs(c, p, X, N, ldX, pa, y, w, &in)) != DE_OK) return rc;
    const de_param_args_t *pa_use = in.pa;
    const char *Xd = static_cast<const char *>(in.Xd), *yd = static_cast<const char *>(in.yd), *wd = static_cast<const char *>(in.wd);
    // the pool
    const int64_t chunk = gn_wide_chunk(N, sc.rows, sc.n_wide, es);
    const int64_t n_slices_max = (chunk + GNW_SLICE - 1) / GNW_SLICE;
    const bool h_j = !is_device_ptr(jtj), h_ok = !is_device_ptr(ok);
    Workspace ws;
    const auto jac = ws.place<char>((size_t)sc.rows * (size_t)chunk * es), vals = ws.place<char>((size_t)sc.n_wide * (size_t)chunk * es),
               cf = ws.place<char>(nc * es), cs = ws.place<char>((size_t)gw->n_consts * es), r_j = ws.place<char>((size_t)std::max<int64_t>(sc.jspan, 1) * es, h_j);
    const auto oks = ws.place<uint8_t>((size_t)sc.n_wide), r_ok = ws.place<uint8_t>(nt, h_ok);
    const auto part = ws.place<double>((size_t)n_slices_max * (size_t)sc.tri), tot = ws.place<double>((size_t)sc.tri);
    if ((rc = ws.reserve(c, c->sGnw)) != DE_OK) return rc;
    void *jtj_d = h_j ? static_cast<void *>(ws.ptr(r_j)) : jtj;
    uint8_t *ok_d = h_ok ? ws.ptr(r_ok) : ok;
    // the table of the wide trees, uploaded when the offsets differ from what the device holds
    {
        std::vector<unsigned char> img((size_t)sc.n_wide * sizeof(GnWideTree));
        GnWideTree *tab = reinterpret_cast<GnWideTree *>(img.data());
        int64_t r0 = 0, t0 = 0;
        for (size_t s = 0; s < (size_t)sc.n_wide; s++) {
            std::memset(&tab[s], 0, sizeof tab[s]);
            const int32_t t = gw->trees[s], g = gw->rows[s];
            tab[s].tree = t;
            tab[s].G = g;
            tab[s].row0 = r0;
            tab[s].tri0 = t0;
            tab[s].joff = sc.joff[(size_t)t];
            r0 += g;
            t0 += (int64_t)g * (g + 1) / 2;
        }
        if (!gw->d_tab || img != gw->tab) {
            HIP_TRY(c, hipStreamSynchronize(c->stream)); // (queued work may still read the table)
            if (!gw->d_tab) HIP_TRY(c, hipMalloc(&gw->d_tab, img.size()));
            HIP_TRY(c, hipMemcpy(gw->d_tab, img.data(), img.size(), hipMemcpyHostToDevice));
            gw->tab = std::move(img);
        }
    }
    if (!c->nested) HIP_TRY(c, time_begin(c));
    {
        NestGuard nest(c);
        // 1. everything but the wide blocks, with the narrow call's bits (the wide blocks: NaN for now)
        rc = narrow(Xd, yd, wd, pa_use, jtj_d, ok_d);
        if (rc != DE_OK) return rc;
        // 2. the wide trees' constants, device to device where the program's are on the device
        if (gw->n_consts > 0 && gw->consts_gen != p->consts_gen) {
            rc = de_program_get_consts(p, ws.ptr(cf));
            if (rc != DE_OK) return rc;
            HIP_TRY(c, launch_gnw_gather(p->dtype, ws.ptr(cf), gw->d_cidx, gw->n_consts, ws.ptr(cs), c->stream));
            rc = set_consts_device_impl(gw->sub, ws.ptr(cs));
            if (rc != DE_OK) return rc;
            gw->consts_gen = p->consts_gen;
        }
        // 3. chunk by chunk: the rows and values of the wide trees, their Gram matrices, the running totals; behind the last chunk the blocks
        GnWideGramArgs ga;
        std::memset(&ga, 0, sizeof ga);
        ga.trees = static_cast<const GnWideTree *>(gw->d_tab);
        ga.n_wide = (int32_t)sc.n_wide;
        ga.jac = ws.ptr(jac);
        ga.vals = ws.ptr(vals);
        ga.kind = spec->kind;
        ga.param = spec->param;
        ga.e_floor = e_floor;
        ga.partial = ws.ptr(part);
        ga.tri_total = sc.tri;
        for (int64_t j0 = 0; j0 < N; j0 += chunk) {
            const int64_t n = std::min(chunk, N - j0);
            de_param_args_t pac;
            const de_param_args_t *pa_c = pa_use;
            if (p->uses_params) {
                pac = *pa_use;
                pac.classes = static_cast<const char *>(pa_use->classes) + (size_t)j0 * (pa_use->classes_is_i64 ? 8 : 4);
                pa_c = &pac;
            }
            rc = grad_impl(c, gw->sub, Xd + (size_t)j0 * (size_t)ldX * es, n, ldX, pa_c, mode, -1, ws.ptr(vals), n, ws.ptr(jac), nullptr, ws.ptr(oks));
            if (rc != DE_OK) return rc;
            ga.y = yd + (size_t)j0 * es;
            ga.w = wd ? wd + (size_t)j0 * es : nullptr;
            ga.n = n;
            HIP_TRY(c, launch_gnw_gram(p->dtype, ga, c->stream));
            HIP_TRY(c, launch_gnw_fold(p->dtype, ga.trees, ga.n_wide, ga.partial, (n + GNW_SLICE - 1) / GNW_SLICE, sc.tri, ws.ptr(tot),
                                       j0 == 0, j0 + n >= N, jtj_d, ok_d, c->stream));
        }
        c->last_kernel = "de_gnw_gram_kernel";
    }
    if (!c->nested) HIP_TRY(c, time_end(c));
    if (h_j)
        for (int64_t t = 0; t < p->n_trees; t++)
            if (sc.ng[(size_t)t] > 0)
                HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(jtj) + (size_t)sc.joff[(size_t)t] * es, static_cast<char *>(jtj_d) + (size_t)sc.joff[(size_t)t] * es,
                                          (size_t)sc.ng[(size_t)t] * (size_t)sc.ng[(size_t)t] * es, hipMemcpyDeviceToHost, c->stream));
    if (h_ok) HIP_TRY(c, hipMemcpyAsync(ok, ok_d, nt, hipMemcpyDeviceToHost, c->stream));
    if (h_j || h_ok) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DE_OK;
}
int gn_wide_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode, const void *y,
                 const void *w, const de_loss_spec_t *spec, double e_floor, void *loss, void *dloss, const int64_t *dloss_offsets, void *jtj,
                 const int64_t *jtj_offsets, uint8_t *ok) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    if (!p->in_cse.empty())
        return fail(c, DE_ERR_UNSUPPORTED, "de_eval_loss_gn_wide: a program made by de_program_create_cse has one gradient row per occurrence of a "
                                           "shared constant (the caller folds them: S H S^T); such callers keep the host loop");
    const GnPlan gn{jtj, jtj_offsets, e_floor, DE_GN_WIDE_MAX_ROWS};
    // The wide trees.  None (or no sample, or arguments the narrow call refuses): exactly de_eval_loss_gn_ex's path, no further launch.
    const GnWideScan sc = gn_wide_scan(p, mode, jtj_offsets, dloss_offsets);
    char why[160];
    int src = DE_OK;
    const bool refused = !sc.mode_ok || sc.neg || N < 0 || !ok || !dloss || !jtj || !X || !y || ldX < p->n_features || loss_spec_problem(spec, 1, why, sizeof why) ||
                         gn_spec_problem(spec, e_floor, p->dtype, &src, why, sizeof why);
    if (sc.n_wide == 0 || N <= 0 || refused)
        return loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, spec, loss, dloss, dloss_offsets, ok, nullptr, false, &gn);
    // loss, dloss, ok and the narrow blocks with de_eval_loss_gn_ex's bits
    return gn_wide_run(c, p, X, N, ldX, pa, mode, y, w, spec, e_floor, jtj, ok, sc,
                       [&](const void *Xd, const void *yd, const void *wd, const de_param_args_t *pa_use, void *jtj_d, uint8_t *ok_d) {
                           const GnPlan gnd{jtj_d, jtj_offsets, e_floor, DE_GN_WIDE_MAX_ROWS};
                           return loss_grad_impl(c, p, Xd, N, ldX, pa_use, mode, yd, wd, spec, loss, dloss, dloss_offsets, ok_d, nullptr, false, &gnd);
                       });
}
// de_eval_fit_stats_grad_wide: the same route behind de_eval_fit_stats_grad (a FitPlan), the wide blocks those of {DE_LOSS_L2, 0, 0}
int fit_stats_grad_wide_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                             const void *y, const void *w, double *stats, double *ystats, double *dmom, const int64_t *dmom_offsets, void *jtj,
                             const int64_t *jtj_offsets, uint8_t *ok) {
    if (!c || !p) return DE_ERR_INVALID_ARG;
    if (p->ctx != c) return fail(c, DE_ERR_INVALID_ARG, "program belongs to another context");
    if (!p->in_cse.empty())
        return fail(c, DE_ERR_UNSUPPORTED, "de_eval_fit_stats_grad_wide: a program made by de_program_create_cse has one gradient row per occurrence of a "
                                           "shared constant (the caller folds them: S H S^T); such callers keep the host loop");
    static const de_loss_spec_t spec{DE_LOSS_L2, 0, 0.0};
    const FitPlan fit{stats, ystats, jtj, jtj_offsets, DE_GN_WIDE_MAX_ROWS};
    // No matrix wanted, no wide tree, no sample, or arguments the narrow call refuses: exactly de_eval_fit_stats_grad's path, no further launch.
    const GnWideScan sc = gn_wide_scan(p, mode, jtj_offsets, dmom_offsets);
    const bool refused = !sc.mode_ok || sc.neg || N < 0 || !ok || !dmom || !stats || !ystats || !X || !y || ldX < p->n_features;
    if (!jtj || sc.n_wide == 0 || N <= 0 || refused)
        return loss_grad_impl(c, p, X, N, ldX, pa, mode, y, w, &spec, nullptr, dmom, dmom_offsets, ok, nullptr, false, nullptr, &fit);
    // stats, ystats, dmom, ok and the narrow blocks with de_eval_fit_stats_grad's bits
    return gn_wide_run(c, p, X, N, ldX, pa, mode, y, w, &spec, 0.0, jtj, ok, sc,
                       [&](const void *Xd, const void *yd, const void *wd, const de_param_args_t *pa_use, void *jtj_d, uint8_t *ok_d) {
                           const FitPlan fd{stats, ystats, jtj_d, jtj_offsets, DE_GN_WIDE_MAX_ROWS};
                           return loss_grad_impl(c, p, Xd, N, ldX, pa_use, mode, yd, wd, &spec, nullptr, dmom, dmom_offsets, ok_d, nullptr, false, nullptr, &fd);
                       });
}
int de_eval_loss_gn_wide(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                         const void *y, const void *w, const de_loss_spec_t *spec, double e_floor, void *loss, void *dloss,
                         const int64_t *dloss_offsets, void *jtj, const int64_t *jtj_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_loss_gn_wide");
    DE_NOTHROW(c, gn_wide_impl(c, p, X, N, ldX, pa, mode, y, w, spec, e_floor, loss, dloss, dloss_offsets, jtj, jtj_offsets, ok));
}
int de_eval_fit_stats_grad_wide(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                                const void *y, const void *w, double *stats, double *ystats, double *dmom, const int64_t *dmom_offsets,
                                void *jtj, const int64_t *jtj_offsets, uint8_t *ok) {
    DE_REFUSE_F16("de_eval_fit_stats_grad_wide");
    DE_NOTHROW(c, fit_stats_grad_wide_impl(c, p, X, N, ldX, pa, mode, y, w, stats, ystats, dmom, dmom_offsets, jtj, jtj_offsets, ok));
}

} // extern "C"
