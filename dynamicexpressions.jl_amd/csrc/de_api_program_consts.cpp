// de_api_program_consts.cpp — a program's constants: the folded constant subtrees (host, de_fold_kernel, auxiliary program: refresh_folds),
// the host part of the flags, de_program_set_consts / _get_consts, and de_program_set_consts_device with its device tables.
#include "de_api_program.h"
#include "de_const_patch.h"

// A constant subtree of + - * / on the host, IEEE-exact
// (src/Evaluate.jl:1002-1067: every node's output is validity-tested; the arithmetic goes on, IEEE propagates what it must).
// half: a DE_F16 program (T = float) — every result rounded to binary16, as de_half.hip does (+ - * / in Float32 rounded once more to
// binary16 are the correctly rounded binary16 results: 24 >= 2 * 11 + 2).
template <typename T>
static bool host_fold_eval(const de_tape_node_t *nd, int64_t n, const double *consts, const int64_t *csrc, T *value, bool half = false) {
    T stack_small[32];
    std::vector<T> stack_big;
    T *st = stack_small;
    if (n > 32) { stack_big.resize((size_t)n); st = stack_big.data(); }
    int sp = 0;
    bool ok = true;
    for (int64_t i = 0; i < n; i++) {
        T v;
        if (nd[i].degree == 0) v = (T)consts[csrc[nd[i].arg]];
        else {
            const T b = st[--sp], a = st[--sp];
            switch (nd[i].op) {
            case DE_B_ADD: v = a + b; break;
            case DE_B_SUB: v = a - b; break;
            case DE_B_MUL: v = a * b; break;
            default: v = a / b; break; // DE_B_DIV (host_foldable admits nothing else)
            }
            if (half) v = (T)(_Float16)v;
        }
        ok = ok && std::isfinite(v);
        st[sp++] = v;
    }
    *value = st[0];
    return ok;
}
extern "C" {
// The constants part of a complex program's table (the folded subtrees' entries follow: refresh_folds)
void fill_ctab_consts(de_program *p) {
    p->ctab.resize(2 * (p->consts.size() + p->folds.size()), 0.0);
    for (size_t k = 0; k < p->consts.size(); k++) {
        p->ctab[2 * k] = p->consts[k];
        p->ctab[2 * k + 1] = p->consts_im[k];
    }
}
// The device copy of the table: (re, im) pairs of the component type
int upload_ctab(de_ctx *c, de_program *p) {
    const size_t n = std::max<size_t>(p->ctab.size() / 2, 1), es = p->dtype == DE_F32 ? 4 : 8;
    std::vector<unsigned char> img(2 * n * es, 0);
    for (size_t i = 0; i < p->ctab.size(); i++) store_elem(p->dtype, img.data(), i, p->ctab[i]);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!p->d_ctab) HIP_TRY(c, hipMalloc(&p->d_ctab, img.size()));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (work already queued may read the table)
    HIP_TRY(c, hipMemcpy(p->d_ctab, img.data(), img.size(), hipMemcpyHostToDevice));
    return DE_OK;
}
void recompute_host_ok(de_program *p) {
    const bool ee = (p->options & DE_OPT_EARLY_EXIT) != 0;
    parallel_for_trees(p->n_trees, [&](int64_t t) {
        bool ok_eval = true, ok_grad = true;
        for (int64_t k = p->const_off[t]; k < p->const_off[t + 1]; k++) {
            const bool fin = finite_in(p->dtype, p->consts[k]) && (p->consts_im.empty() || finite_in(p->dtype, p->consts_im[k]));
            const_flags(fin, p->const_checks[k], ee, &ok_eval, &ok_grad);
        }
        p->host_ok_eval[t] = ok_eval;
        p->host_ok_grad[t] = ok_grad;
    }, 1024);
    // a constant subtree that evaluates to a non-finite value clears the flag — with the flag
    // semantics of the program's own options (dispatch_constant_tree tests unconditionally,
    // the Bumper path only under early_exit): that is exactly what `aux` was lowered with
    // — except for a subtree the reference never hands to dispatch_constant_tree (inner branch of a fused
    // 3-node kernel): its non-finite value is only noticed by the early-exit tests
    for (size_t j = 0; j < p->folds.size() && j < p->fold_ok.size(); j++)
        if (!p->fold_ok[j] && (p->folds[j].tested_always || ee)) p->host_ok_eval[(size_t)p->folds[j].tree] = 0;
}
// Device copy of the host part of the eval flag: every de_eval starts from it with one device-to-device copy
// (a pageable host-to-device copy per call costs ~10 us, a fifth of a small-population call).
static int upload_ok_eval(de_ctx *c, de_program *p) {
    p->tab_ok_stale = true; // host_ok_grad moves with the constants too
    if (p->n_trees == 0) return DE_OK;
    if (!p->d_ok_eval) HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_ok_eval), (size_t)std::max<int64_t>(p->n_trees, 1))); // (never taken since round 6: the arena holds it)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(p->d_ok_eval, p->host_ok_eval.data(), (size_t)p->n_trees, hipMemcpyHostToDevice));
    return DE_OK;
}

// (Re-)evaluate the folded constant subtrees — the IEEE-exact ones on the host, the others on the device — and patch their
// values into fcode.
// `aux_current`: the auxiliary program was created with the present constants this very moment (de_program_create: setting them
// again cost 0.9 of the 1.1 ms this step took for 10^4 trees).
int refresh_folds(de_ctx *c, de_program *p, bool aux_current) {
    if (!p->folded || p->folds.empty()) return DE_OK; // (a CSE-only eval program has no constant subtrees to evaluate)
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    const size_t ies = dtype_bytes(p->io); // (the auxiliary program's buffers: a DE_F16 program's auxiliary program is DE_F16 too)
    const size_t nf = p->folds.size();
    p->fold_ok.assign(nf, 0);
    parallel_for_trees((int64_t)nf, [&](int64_t j) {
        if (p->fold_host[(size_t)j] != 1) return;
        const de_tape_node_t *nd = p->fold_nodes.data() + p->fold_noff[(size_t)j];
        const int64_t n = p->fold_noff[(size_t)j + 1] - p->fold_noff[(size_t)j];
        const int64_t *csrc = p->aux_const_src.data() + p->fold_coff[(size_t)j];
        double v;
        bool ok;
        if (p->dtype == DE_F32) { float f; ok = host_fold_eval<float>(nd, n, p->consts.data(), csrc, &f, p->io == DE_F16); v = (double)f; }
        else ok = host_fold_eval<double>(nd, n, p->consts.data(), csrc, &v);
        p->fold_ok[(size_t)j] = ok ? 1 : 0;
        write_imm(p->fcode[(size_t)p->folds[(size_t)j].instr], p->dtype, v);
    }, 256);
    if (!p->kfold.empty()) {
        // the subtrees with other operators: one thread each on the device (de_fold_kernel), the operators' own device code.
        // `aux_current`: the image uploaded at creation already holds these constants.
        const size_t nk = p->kfold.size();
        HIP_TRY(c, hipSetDevice(c->device));
        if (!aux_current) {
            std::vector<unsigned char> cv(std::max<size_t>(p->kf_csrc.size(), 1) * es);
            for (size_t k = 0; k < p->kf_csrc.size(); k++) store_elem(p->dtype, cv.data(), k, p->consts[(size_t)p->kf_csrc[k]]);
            HIP_TRY(c, hipStreamSynchronize(c->stream)); // (an earlier launch may still read the values)
            if (!p->kf_csrc.empty()) HIP_TRY(c, hipMemcpy(p->d_kf + p->kf_o_cvals, cv.data(), p->kf_csrc.size() * es, hipMemcpyHostToDevice));
        }
        HIP_TRY(c, launch_fold(p->dtype, p->d_kf, reinterpret_cast<const int64_t *>(p->d_kf + p->kf_o_noff), reinterpret_cast<const int64_t *>(p->d_kf + p->kf_o_coff),
                               p->d_kf + p->kf_o_cvals, (int64_t)nk, p->d_kf + p->kf_o_out, reinterpret_cast<uint8_t *>(p->d_kf + p->kf_o_ok), c->stream));
        std::vector<unsigned char> res(p->kf_bytes - p->kf_o_out);
        HIP_TRY(c, hipMemcpyAsync(res.data(), p->d_kf + p->kf_o_out, res.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const unsigned char *okb = res.data() + (p->kf_o_ok - p->kf_o_out);
        for (size_t k = 0; k < nk; k++) {
            const size_t j = (size_t)p->kfold[k];
            p->fold_ok[j] = okb[k];
            write_imm(p->fcode[(size_t)p->folds[j].instr], p->dtype, load_elem(p->dtype, res.data(), k));
        }
    }
    if (!p->aux) return DE_OK;
    const size_t na = p->aux_fold.size();
    int rc = DE_OK;
    if (!aux_current) {
        std::vector<unsigned char> ac(std::max<size_t>(p->aux_csrc.size(), 1) * ies);
        for (size_t k = 0; k < p->aux_csrc.size(); k++)
            store_elem(p->io, ac.data(), k, p->consts[(size_t)p->aux_csrc[k]], p->consts_im.empty() ? 0.0 : p->consts_im[(size_t)p->aux_csrc[k]]);
        rc = de_program_set_consts(p->aux, ac.data());
        if (rc != DE_OK) return fail(c, rc, "constant folding: %s", p->aux->ctx->err.c_str());
    }
    std::vector<unsigned char> X(std::max<size_t>((size_t)p->n_features, 1) * ies, 0), out(na * ies);
    std::vector<uint8_t> aok(na, 0);
    rc = de_eval(c, p->aux, X.data(), 1, std::max<int64_t>(p->n_features, 1), nullptr, out.data(), 1, aok.data());
    if (rc != DE_OK) return rc;
    for (size_t a = 0; a < na; a++) {
        const size_t j = (size_t)p->aux_fold[a];
        const double v = load_elem(p->io, out.data(), a);
        p->fold_ok[j] = aok[a];
        if (is_complex_io(p->io)) { // table entry consts.size() + j
            const size_t e = p->consts.size() + j;
            p->ctab[2 * e] = v;
            p->ctab[2 * e + 1] = load_elem_im(p->io, out.data(), a);
            write_cidx(p->fcode[(size_t)p->folds[j].instr], e);
        } else write_imm(p->fcode[(size_t)p->folds[j].instr], p->dtype, v);
    }
    return DE_OK;
}
// The compact site lists (eval_sites / grad_sites) of a threaded, patched-in-place program, rebuilt when site_gen moved: one pass over
// all instructions, afterwards only the immediates are visited.  de_program_set_consts patches by them, and the device tables of
// de_program_set_consts_device are derived from them.
static void refresh_site_lists(de_program *p) {
    if (p->lists_gen == p->site_gen) return;
    const std::vector<Instr> &src = p->folded ? p->fcode : p->code;
    p->eval_sites.clear();
    p->grad_sites.clear();
    for (size_t i = 0; i < src.size(); i++)
        if (p->bsite[i] >= 0) {
            // record of tcode[j] in the chained stream: one end record per preceding tree, behind the head record
            const int32_t j = p->tsite[i];
            const int64_t tree = (std::upper_bound(p->tcode_off.begin(), p->tcode_off.end(), j) - p->tcode_off.begin()) - 1;
            p->eval_sites.push_back({(int32_t)i, p->bsite[i], j, (int32_t)(j + tree + 1)}); // + the head record
        }
    if (!p->gbsite.empty())
        for (size_t i = 0; i < p->code.size(); i++) {
            const int32_t gj = p->gbsite[i];
            if (gj < 0) continue;
            p->grad_sites.push_back({(int32_t)i, gj, p->gtsite_of_gb.empty() ? -1 : p->gtsite_of_gb[(size_t)gj],
                                     p->rtsite_of_gb.empty() ? -1 : p->rtsite_of_gb[(size_t)gj]});
        }
    p->lists_gen = p->site_gen;
}

static int set_consts_impl(de_program_t *p, const void *consts);
static int set_consts_nothrow(de_program_t *p, const void *consts) {
    if (!p) return DE_ERR_INVALID_ARG;
    DE_NOTHROW(p->ctx, set_consts_impl(p, consts));
}
int de_program_set_consts(de_program_t *p, const void *consts) {
    // (every host copy and every device stream is overwritten below: constants a device set left ahead of the host need no materialising)
    if (p && (consts || p->consts.empty())) p->consts_dev_ahead = p->consts_dev_path = false;
    const int rc = set_consts_nothrow(p, consts);
    if (rc == DE_OK && p && getenv("DE_VERIFY") && *getenv("DE_VERIFY") == '1') return de_program_verify(p);
    return rc;
}
static int set_consts_impl(de_program_t *p, const void *consts) {
    if (!p) return DE_ERR_INVALID_ARG;
    de_ctx *ctx = p->ctx;
    if (!consts && !p->consts.empty()) return fail(ctx, DE_ERR_INVALID_ARG, "consts is null");
    p->consts_gen++; // (the cached certificate program belongs to the old constants)
    const bool timing = getenv("DE_DEBUG_TIMING") != nullptr; // stderr: microseconds per phase
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
    const auto t0 = now();
    const bool cplx = is_complex_io(p->io);
    // (every loop of this function over constants, trees or sites writes slots of its own: on the host pool; 10^4 trees: 0.85 -> see DESIGN 9.1)
    try {
        parallel_tree_ranges((int64_t)p->consts.size(), [&](int, int64_t kb, int64_t ke) {
            for (size_t k = (size_t)kb; k < (size_t)ke; k++) {
                const double v = load_elem(p->io, consts, k);
                p->consts[k] = v;
                if (cplx) { p->consts_im[k] = load_elem_im(p->io, consts, k); continue; } // (the immediates are table indices)
                if (p->const_instr[k] >= 0) write_imm(p->code[(size_t)p->const_instr[k]], p->dtype, v);
                if (p->folded && p->fconst_instr[k] >= 0) write_imm(p->fcode[(size_t)p->fconst_instr[k]], p->dtype, v);
            }
        }, 4096);
    } catch (const std::bad_alloc &) { return fail(ctx, DE_ERR_HIP, "out of host memory"); }
    const auto t1 = now();
    if (cplx) fill_ctab_consts(p);
    if (p->folded) {
        int rc = DE_OK;
        try { rc = refresh_folds(ctx, p); } catch (const std::bad_alloc &) { rc = fail(ctx, DE_ERR_HIP, "out of host memory"); }
        if (rc != DE_OK) return rc;
    }
    const auto t2 = now();
    recompute_host_ok(p);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        const int rc = upload_ok_eval(ctx, p);
        if (rc != DE_OK) return rc;
    }
    const auto t3 = now();
    if (cplx) return upload_ctab(ctx, p); // a complex program's stream does not change: its constants and folds are the table
    // Same tree shapes, new immediates: patch the bits where they live (the optimiser calls this once per
    // step — re-binding 10^4 trees costs milliseconds, the kernel it feeds a few hundred microseconds).
    const char *nopatch = getenv("DE_NO_CONST_PATCH");
    if (!(nopatch && *nopatch == '1') && p->threaded && !p->tsite.empty() && !p->bsite.empty()) {
        const std::vector<Instr> &src = p->folded ? p->fcode : p->code;
        const bool gpatch = p->d_gcode && !p->gcode_stale && !p->gbsite.empty();
        const bool tpatch = gpatch && p->gt_valid && !p->gtsite_of_gb.empty();
        const bool rpatch = gpatch && p->rt_valid && !p->rtsite_of_gb.empty();
        refresh_site_lists(p);
        try {
        parallel_tree_ranges((int64_t)p->eval_sites.size(), [&](int, int64_t sb, int64_t se) {
            for (size_t q = (size_t)sb; q < (size_t)se; q++) {
                const de_program::EvalSite &e = p->eval_sites[q];
                const uint32_t lo = src[(size_t)e.src].imm.u32[0], hi = src[(size_t)e.src].imm.u32[1];
                p->bcode[(size_t)e.b].lo = lo;
                p->bcode[(size_t)e.b].hi = hi;
                p->tcode[(size_t)e.t].lo = lo;
                p->tcode[(size_t)e.t].hi = hi;
                p->fbcode[(size_t)e.t].lo = lo; // (the fused form too: de_program_update copies a kept tree's fused code from it)
                p->fbcode[(size_t)e.t].hi = hi;
                patch_chained_imm(p, e.c, lo, hi);
            }
        }, 4096);
        if (gpatch)
            parallel_tree_ranges((int64_t)p->grad_sites.size(), [&](int, int64_t sb, int64_t se) {
                for (size_t q = (size_t)sb; q < (size_t)se; q++) {
                    const de_program::GradSite &g = p->grad_sites[q];
                    const uint32_t lo = p->code[(size_t)g.src].imm.u32[0], hi = p->code[(size_t)g.src].imm.u32[1];
                    p->gbcode[(size_t)g.gb].lo = lo;
                    p->gbcode[(size_t)g.gb].hi = hi;
                    if (tpatch && g.gt >= 0) {
                        for (int64_t w = 0; w < (p->gt_share ? 4 : 1); w++) { // (every stream variant of a shared-leaf-row program)
                            p->gtcode[(size_t)(g.gt + w * p->gt_stride)].lo = lo;
                            p->gtcode[(size_t)(g.gt + w * p->gt_stride)].hi = hi;
                        }
                    }
                    if (rpatch && g.rt >= 0) {
                        p->rtcode[(size_t)g.rt].lo = lo;
                        p->rtcode[(size_t)g.rt].hi = hi;
                    }
                }
            }, 4096);
        } catch (const std::bad_alloc &) { return fail(ctx, DE_ERR_HIP, "out of host memory"); }
        if (gpatch) {
            if (!tpatch) p->gt_valid = false;
            if (!rpatch) p->rt_valid = false;
        } else {
            p->gcode_stale = true;
        }
        if (p->assured) { // new constants, new intervals: the assured handler words of every tree (its immediates were patched above)
            uint64_t table[TOPX_TABLE];
            const hipError_t hs = eval_handler_table(p->dtype, (p->options & DE_OPT_TURBO) != 0, table);
            if (hs != hipSuccess) return fail(ctx, DE_ERR_HIP, "handler table: %s", hipGetErrorString(hs));
            parallel_tree_ranges(p->n_trees, [&](int, int64_t tb, int64_t te) {
                assured_link_trees(p, table, tb, te, true);
                if (p->assured_tiers >= 2) assured_link_trees(p, table, tb, te, true, 2); // (both passes, the touched trees only)
            });
            p->assured_valid = true;
        }
        const auto t4 = now();
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // the program may be in use by work already queued
        if (!p->ccode.empty())
            HIP_TRY(ctx, hipMemcpy(p->d_code, p->ccode.data(), p->ccode.size() * sizeof(BoundInstr), hipMemcpyHostToDevice));
        HIP_TRY(ctx, upload_wave_variants(p));
        if (gpatch) {
            if (!p->gbcode.empty())
                HIP_TRY(ctx, hipMemcpy(p->d_gcode, p->gbcode.data(), p->gbcode.size() * sizeof(BoundInstr), hipMemcpyHostToDevice));
            if (p->gt_valid && !p->gtcode.empty())
                HIP_TRY(ctx, hipMemcpy(p->d_gtcode, p->gtcode.data(), p->gtcode.size() * sizeof(BoundInstr), hipMemcpyHostToDevice));
            if (p->rt_valid && !p->rtcode.empty())
                HIP_TRY(ctx, hipMemcpy(p->d_rtcode, p->rtcode.data(), p->rtcode.size() * sizeof(BoundInstr), hipMemcpyHostToDevice));
        }
        if (timing)
            fprintf(stderr, "set_consts us: write %ld, refresh_folds %ld, flags %ld, patch %ld, upload %ld\n", us(t0, t1), us(t1, t2), us(t2, t3),
                    us(t3, t4), us(t4, now()));
        return DE_OK;
    }
    p->gcode_stale = true;
    try {
        rebind(p); // same shape: only immediates change
    } catch (const std::bad_alloc &) {
        return fail(ctx, DE_ERR_HIP, "out of host memory");
    }
    {
        int rc = DE_OK;
        try { rc = make_threaded(ctx, p); } catch (const std::bad_alloc &) { rc = fail(ctx, DE_ERR_HIP, "out of host memory"); }
        if (rc != DE_OK) return rc;
    }
    // the program may be in use by work already queued on the stream
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!p->bcode.empty())
        HIP_TRY(ctx, hipMemcpy(p->d_code, (p->threaded ? p->ccode : p->bcode).data(),
                               (p->threaded ? p->ccode : p->bcode).size() * sizeof(BoundInstr), hipMemcpyHostToDevice));
    if (p->threaded) HIP_TRY(ctx, upload_wave_variants(p)); // (same shapes: the variants the creation made room for)
    return DE_OK;
}

// ---- de_program_set_consts_device (kernels: de_const_patch.hip) -------------------------------------------------------
// The host side brought up to the device's constants: one device-to-host copy of the owned buffer, then the host function — which
// writes the same bits into every device stream once more and rebuilds every host copy.
int consts_materialise(de_program *p) {
    if (!p || !p->consts_dev_ahead) return DE_OK;
    de_ctx *c = p->ctx;
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    try {
        std::vector<unsigned char> h(std::max<size_t>(p->consts.size(), 1) * es);
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemcpyAsync(h.data(), p->d_cp_vals, p->consts.size() * es, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        p->consts_dev_ahead = false;
        const int rc = set_consts_nothrow(p, h.data());
        if (rc != DE_OK) p->consts_dev_ahead = true;
        return rc;
    } catch (const std::bad_alloc &) { return fail(c, DE_ERR_HIP, "out of host memory"); }
}

// What the program's kind and folds allow, decided once: DE_F32 / DE_F64, threaded, no turbo operators, every fold evaluated by
// de_fold_kernel — its own route, or the host route (+ - * /) where the subtree's evaluation stack fits the kernel's.
static bool const_patch_kind_ok(de_program *p) {
    if (p->cp_eligible >= 0) return p->cp_eligible == 1;
    bool ok = (p->io == DE_F32 || p->io == DE_F64) && p->threaded && !p->aux && p->n_trees > 0 && !(p->options & DE_OPT_TURBO);
    if (!p->folds.empty() && (p->fold_noff.size() != p->folds.size() + 1 || p->fold_coff.size() != p->folds.size() + 1)) ok = false;
    for (size_t j = 0; ok && j < p->folds.size(); j++) {
        if (j >= p->fold_host.size() || p->fold_host[j] == 0) { ok = false; break; }
        if (p->fold_host[j] != 1) continue;
        int depth = 0, worst = 0;
        for (int64_t i = p->fold_noff[j]; i < p->fold_noff[j + 1]; i++) { depth += 1 - (int)p->fold_nodes[(size_t)i].degree; worst = std::max(worst, depth); }
        if (worst > DE_FOLD_STACK) ok = false;
    }
    p->cp_eligible = ok ? 1 : 0;
    return ok;
}

// The device tables of the present streams: 1 built, 0 the program cannot be served (a site without a source: never expected), < 0 -status.
static int build_const_patch_tables(de_ctx *c, de_program *p, const de_program::ConstPatchKey &key, bool gpatch, bool tpatch, bool rpatch) {
    refresh_site_lists(p);
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    const size_t nc = p->consts.size(), nf = p->folds.size(), nt = (size_t)p->n_trees;
    const std::vector<Instr> &src = p->folded ? p->fcode : p->code;
    // sources: constant k = k; fold j = nc + its place among the de_fold_kernel-route folds, or behind them among the host-route ones
    std::vector<uint32_t> pos(nf, 0);
    std::vector<int32_t> hfold;
    for (size_t k = 0; k < p->kfold.size(); k++) pos[(size_t)p->kfold[k]] = (uint32_t)k;
    for (size_t j = 0; j < nf; j++)
        if (p->fold_host[j] == 1) { pos[j] = (uint32_t)(p->kfold.size() + hfold.size()); hfold.push_back((int32_t)j); }
    const size_t nk = p->kfold.size(), nh = hfold.size();
    if (nc + nk + nh > 0xFFFFFFFFull) return 0;
    std::vector<int64_t> src_eval(src.size(), -1), src_code(p->code.size(), -1);
    for (size_t k = 0; k < nc; k++) { // (occurrence slots of a shared constant name one instruction of a CSE program: the last one wins, as on the host)
        const int32_t ie = p->folded ? p->fconst_instr[k] : p->const_instr[k];
        if (ie >= 0) src_eval[(size_t)ie] = (int64_t)k;
        if (p->const_instr[k] >= 0) src_code[(size_t)p->const_instr[k]] = (int64_t)k;
    }
    if (p->folded)
        for (size_t j = 0; j < nf; j++) src_eval[(size_t)p->folds[j].instr] = (int64_t)(nc + pos[j]);
    std::vector<uint64_t> addr;
    std::vector<uint32_t> srcs;
    auto site = [&](const BoundInstr *rec, bool word32, int64_t s) {
        addr.push_back(word32 ? ((uint64_t)(uintptr_t)&rec->arg | CONST_SITE_32) : (uint64_t)(uintptr_t)&rec->lo);
        srcs.push_back((uint32_t)s);
    };
    const size_t nvar = p->var_stride && !p->ccode.empty() ? 1 + p->ccode_w.size() / p->ccode.size() : 1; // (wave groups: every wave's variant)
    if (nvar > 1 && (size_t)p->var_stride < p->ccode.size()) return 0;
    for (const de_program::EvalSite &e : p->eval_sites) {
        const int64_t s = src_eval[(size_t)e.src];
        if (s < 0 || e.c < 0 || (size_t)e.c >= p->ccode.size()) return 0;
        for (size_t w = 0; w < nvar; w++) site(p->d_code + w * (size_t)p->var_stride + (size_t)e.c, p->dtype == DE_F32, s);
    }
    if (gpatch)
        for (const de_program::GradSite &g : p->grad_sites) {
            const int64_t s = src_code[(size_t)g.src];
            if (s < 0 || g.gb < 0 || (size_t)g.gb >= p->gbcode.size()) return 0;
            site(p->d_gcode + g.gb, false, s);
            if (tpatch && g.gt >= 0)
                for (int64_t w = 0; w < (p->gt_share ? 4 : 1); w++) { // (every stream variant of a shared-leaf-row program)
                    const size_t at = (size_t)(g.gt + w * p->gt_stride);
                    if (at >= p->gtcode.size() || at >= p->gt_cap) return 0;
                    site(p->d_gtcode + at, false, s);
                }
            if (rpatch && g.rt >= 0) {
                if ((size_t)g.rt >= p->rtcode.size()) return 0;
                site(p->d_rtcode + g.rt, false, s);
            }
        }
    // the flag kernel's lists: the folds of every tree
    std::vector<int32_t> tfoff(nt + 1, 0);
    std::vector<uint32_t> tfold(std::max<size_t>(nf, 1), 0);
    for (size_t j = 0; j < nf; j++) tfoff[(size_t)p->folds[j].tree + 1]++;
    for (size_t t = 0; t < nt; t++) tfoff[t + 1] += tfoff[t];
    {
        std::vector<int32_t> at(tfoff.begin(), tfoff.end() - 1);
        for (size_t j = 0; j < nf; j++) tfold[(size_t)at[(size_t)p->folds[j].tree]++] = (pos[j] << 1) | (p->folds[j].tested_always ? 1u : 0u);
    }
    // the gather list [de_fold_kernel route | host route] and the host-route folds' image for de_fold_kernel
    std::vector<int64_t> gidx(p->kf_csrc.begin(), p->kf_csrc.end()), hnoff{0}, hcoff{0};
    std::vector<de_tape_node_t> hnodes;
    for (const int32_t j : hfold) {
        hnodes.insert(hnodes.end(), p->fold_nodes.begin() + p->fold_noff[(size_t)j], p->fold_nodes.begin() + p->fold_noff[(size_t)j + 1]);
        gidx.insert(gidx.end(), p->aux_const_src.begin() + p->fold_coff[(size_t)j], p->aux_const_src.begin() + p->fold_coff[(size_t)j + 1]);
        hnoff.push_back((int64_t)hnodes.size());
        hcoff.push_back((int64_t)(gidx.size() - p->kf_csrc.size()));
    }
    for (const int64_t k : gidx)
        if (k < 0 || (size_t)k >= nc) return 0;
    const size_t nkc = p->kf_csrc.size(), nhc = gidx.size() - nkc;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    auto place = [&](size_t bytes) { const size_t at = o; o += al(std::max<size_t>(bytes, 1)); return at; };
    p->cp_o_addr = place(addr.size() * sizeof(uint64_t));
    p->cp_o_src = place(srcs.size() * sizeof(uint32_t));
    p->cp_o_coff = place((nt + 1) * sizeof(int64_t));
    p->cp_o_checks = place(nc);
    p->cp_o_tfoff = place((nt + 1) * sizeof(int32_t));
    p->cp_o_tfold = place(nf * sizeof(uint32_t));
    p->cp_o_gidx = place(gidx.size() * sizeof(int64_t));
    p->cp_o_hnodes = place(hnodes.size() * sizeof(de_tape_node_t));
    p->cp_o_hnoff = place(hnoff.size() * sizeof(int64_t));
    p->cp_o_hcoff = place(hcoff.size() * sizeof(int64_t));
    p->cp_o_hcvals = place(nhc * es);
    std::vector<unsigned char> img(o, 0);
    auto put = [&](size_t at, const void *data, size_t bytes) { if (bytes) std::memcpy(img.data() + at, data, bytes); };
    put(p->cp_o_addr, addr.data(), addr.size() * sizeof(uint64_t));
    put(p->cp_o_src, srcs.data(), srcs.size() * sizeof(uint32_t));
    put(p->cp_o_coff, p->const_off.data(), (nt + 1) * sizeof(int64_t));
    put(p->cp_o_checks, p->const_checks.data(), nc);
    put(p->cp_o_tfoff, tfoff.data(), (nt + 1) * sizeof(int32_t));
    put(p->cp_o_tfold, tfold.data(), nf * sizeof(uint32_t));
    put(p->cp_o_gidx, gidx.data(), gidx.size() * sizeof(int64_t));
    put(p->cp_o_hnodes, hnodes.data(), hnodes.size() * sizeof(de_tape_node_t));
    put(p->cp_o_hnoff, hnoff.data(), hnoff.size() * sizeof(int64_t));
    put(p->cp_o_hcoff, hcoff.data(), hcoff.size() * sizeof(int64_t));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (an earlier device set may still read the old tables)
    prog_free(c, p->d_cp);
    p->d_cp = nullptr;
    p->cp_key = de_program::ConstPatchKey();
    {
        const hipError_t st = prog_malloc(c, reinterpret_cast<void **>(&p->d_cp), o);
        if (st != hipSuccess) return -fail(c, DE_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(st));
    }
    if (!p->d_cp_vals) { // [constants | fold values] in the element type, then the folds' flags: the program's own copy of its constants
        p->cp_o_fok = al((nc + nk + nh) * es);
        const hipError_t st = prog_malloc(c, reinterpret_cast<void **>(&p->d_cp_vals), p->cp_o_fok + al(std::max<size_t>(nk + nh, 1)));
        if (st != hipSuccess) return -fail(c, DE_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(st));
    }
    {
        const hipError_t st = hipMemcpy(p->d_cp, img.data(), img.size(), hipMemcpyHostToDevice);
        if (st != hipSuccess) return -fail(c, DE_ERR_HIP, "constant site tables: upload failed: %s", hipGetErrorString(st));
    }
    p->cp_n_sites = (int64_t)addr.size();
    p->cp_nk = (int64_t)nk;
    p->cp_nh = (int64_t)nh;
    p->cp_nkc = (int64_t)nkc;
    p->cp_nhc = (int64_t)nhc;
    p->cp_key = key;
    return 1;
}

int set_consts_device_impl(de_program_t *p, const void *d_consts) {
    de_ctx *c = p->ctx;
    const size_t nc = p->consts.size();
    if (nc == 0) return DE_OK;
    if (!d_consts) return fail(c, DE_ERR_INVALID_ARG, "d_consts is null");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!is_device_ptr(d_consts))
        return fail(c, DE_ERR_INVALID_ARG, "d_consts is a host pointer: de_program_set_consts takes constants from host memory");
    const char *nopatch = getenv("DE_NO_CONST_PATCH");
    bool device = const_patch_kind_ok(p) && !(nopatch && *nopatch == '1') && !p->tsite.empty() && !p->bsite.empty();
    const size_t es = p->dtype == DE_F32 ? 4 : 8;
    if (device) {
        // which gradient streams are patched and which are dropped: as de_program_set_consts decides it
        const bool gpatch = p->d_gcode && !p->gcode_stale && !p->gbsite.empty();
        const bool tpatch = gpatch && p->gt_valid && !p->gtsite_of_gb.empty();
        const bool rpatch = gpatch && p->rt_valid && !p->rtsite_of_gb.empty();
        if (!p->d_ok_grad) { // (the tables de_eval_grad keeps per program: the flag kernel writes the first of them)
            const size_t nt = (size_t)p->n_trees;
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_ok_grad), nt));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_ng), nt * sizeof(int32_t)));
            HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&p->d_goff), nt * sizeof(int64_t)));
            p->tab_mode = -1;
        }
        de_program::ConstPatchKey key;
        key.site_gen = p->site_gen;
        key.code = p->d_code;
        key.gcode = gpatch ? p->d_gcode : nullptr;
        key.gtcode = tpatch ? p->d_gtcode : nullptr;
        key.rtcode = rpatch ? p->d_rtcode : nullptr;
        key.ok_grad = p->d_ok_grad;
        key.gt_stride = tpatch ? p->gt_stride : 0;
        key.gt_variants = tpatch ? (p->gt_share ? 4 : 1) : 0;
        if (!p->d_cp || !(key == p->cp_key)) {
            const int rc = build_const_patch_tables(c, p, key, gpatch, tpatch, rpatch);
            if (rc < 0) return -rc;
            if (rc == 0) { p->cp_eligible = 0; device = false; }
        }
        if (device) {
            char *vals = p->d_cp_vals;
            uint8_t *fok = reinterpret_cast<uint8_t *>(vals + p->cp_o_fok);
            const int64_t *gidx = reinterpret_cast<const int64_t *>(p->d_cp + p->cp_o_gidx);
            if (!c->nested) HIP_TRY(c, time_begin(c));
            HIP_TRY(c, hipMemcpyAsync(vals, d_consts, nc * es, hipMemcpyDeviceToDevice, c->stream)); // (from here on the caller's buffer is free)
            HIP_TRY(c, launch_const_gather(p->dtype, vals, gidx, p->cp_nkc, p->d_kf ? p->d_kf + p->kf_o_cvals : nullptr, p->cp_nhc,
                                           p->d_cp + p->cp_o_hcvals, c->stream));
            if (p->cp_nk > 0)
                HIP_TRY(c, launch_fold(p->dtype, p->d_kf, reinterpret_cast<const int64_t *>(p->d_kf + p->kf_o_noff),
                                       reinterpret_cast<const int64_t *>(p->d_kf + p->kf_o_coff), p->d_kf + p->kf_o_cvals, p->cp_nk, vals + nc * es, fok,
                                       c->stream));
            if (p->cp_nh > 0)
                HIP_TRY(c, launch_fold(p->dtype, p->d_cp + p->cp_o_hnodes, reinterpret_cast<const int64_t *>(p->d_cp + p->cp_o_hnoff),
                                       reinterpret_cast<const int64_t *>(p->d_cp + p->cp_o_hcoff), p->d_cp + p->cp_o_hcvals, p->cp_nh,
                                       vals + (nc + (size_t)p->cp_nk) * es, fok + p->cp_nk, c->stream));
            HIP_TRY(c, launch_const_scatter(p->dtype, vals, reinterpret_cast<const uint64_t *>(p->d_cp + p->cp_o_addr),
                                            reinterpret_cast<const uint32_t *>(p->d_cp + p->cp_o_src), p->cp_n_sites, c->stream));
            HIP_TRY(c, launch_const_flags(p->dtype, vals, reinterpret_cast<const int64_t *>(p->d_cp + p->cp_o_coff),
                                          reinterpret_cast<const uint8_t *>(p->d_cp + p->cp_o_checks), reinterpret_cast<const int32_t *>(p->d_cp + p->cp_o_tfoff),
                                          reinterpret_cast<const uint32_t *>(p->d_cp + p->cp_o_tfold), fok, p->n_trees, (p->options & DE_OPT_EARLY_EXIT) != 0,
                                          p->d_ok_eval, p->d_ok_grad, c->stream));
            if (!c->nested) HIP_TRY(c, time_end(c));
            p->consts_gen++; // (the cached certificate program belongs to the old constants)
            if (gpatch) {
                if (!tpatch) p->gt_valid = false;
                if (!rpatch) p->rt_valid = false;
            } else {
                p->gcode_stale = true;
            }
            p->tab_ok_stale = false; // (d_ok_grad is current: the flag kernel wrote it)
            p->consts_dev_ahead = true;
            p->consts_dev_path = true;
            p->assured_valid = false; // (the intervals belong to the old constants: the guarded stream until the host sees the new ones)
            return DE_OK;
        }
    }
    // staged: one device-to-host copy, then the host function
    std::vector<unsigned char> h(nc * dtype_bytes(p->io));
    HIP_TRY(c, hipMemcpyAsync(h.data(), d_consts, h.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return de_program_set_consts(p, h.data());
}
int de_program_set_consts_device(de_program_t *p, const void *d_consts) {
    if (!p) return DE_ERR_INVALID_ARG;
    int rc = DE_OK;
    try { rc = set_consts_device_impl(p, d_consts); }
    catch (const std::bad_alloc &) { return fail(p->ctx, DE_ERR_HIP, "out of host memory"); }
    catch (const std::exception &e) { return fail(p->ctx, DE_ERR_HIP, "internal error: %s", e.what()); }
    catch (...) { return fail(p->ctx, DE_ERR_HIP, "internal error (unknown exception)"); }
    if (rc == DE_OK && p->consts_dev_ahead && getenv("DE_VERIFY") && *getenv("DE_VERIFY") == '1') return de_program_verify(p);
    return rc;
}
int de_program_consts_device_path(const de_program_t *p) { return p ? (p->consts_dev_path ? 1 : 0) : -1; }

static int get_consts_impl(de_program_t *p, void *out) {
    de_ctx *c = p->ctx;
    const size_t nc = p->consts.size();
    if (nc == 0) return DE_OK;
    if (!out) return fail(c, DE_ERR_INVALID_ARG, "out is null");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t ies = dtype_bytes(p->io);
    const bool dev = is_device_ptr(out);
    if (dev && p->consts_dev_ahead) { // (a device-path program: io is the compute type)
        HIP_TRY(c, hipMemcpyAsync(out, p->d_cp_vals, nc * ies, hipMemcpyDeviceToDevice, c->stream));
        return DE_OK;
    }
    const int rc = consts_materialise(p);
    if (rc != DE_OK) return rc;
    std::vector<unsigned char> h;
    unsigned char *dst = static_cast<unsigned char *>(out);
    if (dev) { h.resize(nc * ies); dst = h.data(); }
    for (size_t k = 0; k < nc; k++) store_elem(p->io, dst, k, p->consts[k], p->consts_im.empty() ? 0.0 : p->consts_im[k]);
    if (dev) {
        HIP_TRY(c, hipMemcpyAsync(out, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the pageable host vector must outlive its copy)
    }
    return DE_OK;
}
int de_program_get_consts(de_program_t *p, void *out) {
    if (!p) return DE_ERR_INVALID_ARG;
    DE_NOTHROW(p->ctx, get_consts_impl(p, out));
}
} // extern "C"
