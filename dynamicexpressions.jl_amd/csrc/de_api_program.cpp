// de_api_program.cpp — C ABI (include/de_hip.h): de_program_create / _create_cse / _update / _destroy.  A creation lowers every tree into a
// position-independent unit (TreeUnit), links the units into the program's vectors, and runs the program-wide passes (fold evaluation,
// flags, binding, threading, upload) — DESIGN.md §3.2.  An update is a creation whose kept trees' units are views into the old program (§3.4).
#include "de_api_program.h"

static bool host_foldable(const de_tape_node_t *nd, int64_t n) {
    for (int64_t i = 0; i < n; i++) {
        if (nd[i].degree == 0) { if (nd[i].op != DE_LEAF_CONST) return false; }
        else if (nd[i].degree != 2 || nd[i].op < DE_B_ADD || nd[i].op > DE_B_DIV) return false;
    }
    return n > 0;
}

// The environment switches of a creation, read once at its top — at EVERY creation: the tests flip them inside one process
struct CreateEnv {
    bool fold, cse, grad_cse, host_fold, kernel_fold, update_splice, verify, timing;
};
static CreateEnv read_create_env() {
    auto is_1 = [](const char *name) { const char *v = getenv(name); return v && *v == '1'; };
    CreateEnv e;
    e.fold = !is_1("DE_NO_FOLD");
    e.cse = !is_1("DE_NO_CSE");
    e.grad_cse = !getenv("DE_NO_GRAD_CSE"); // (set to anything)
    e.host_fold = !is_1("DE_NO_HOST_FOLD");
    e.kernel_fold = !is_1("DE_NO_KERNEL_FOLD");
    e.update_splice = !is_1("DE_NO_UPDATE_SPLICE");
    e.verify = is_1("DE_VERIFY");
    e.timing = getenv("DE_DEBUG_TIMING") != nullptr; // microseconds per phase of the creation on stderr (tools/bench_create.py)
    return e;
}
struct CreateTimer {
    bool on;
    long long n_trees;
    bool aux;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[de_program_create %lld trees%s] %-28s %9.1f us\n", n_trees, aux ? " (aux)" : "", what,
                std::chrono::duration<double, std::micro>(now - t_last).count());
        t_last = std::chrono::steady_clock::now();
    }
};

// The caller's population.  The eval program of tree t is lowered from its CSE tape when the caller supplied one (a GraphNode tree: shared
// subtrees appear once, de_program_create_cse); everything else — gradients, constant bookkeeping, flags — follows the expanded tape.
struct Population {
    int64_t n_trees;
    const de_tape_node_t *nodes;
    const int64_t *node_offsets;
    const de_tape_node_t *cse_nodes; // null: no CSE tapes
    const int64_t *cse_offsets;
    const void *consts;
    const int64_t *const_offsets;
    const de_tape_node_t *tape(int64_t t) const { return nodes + node_offsets[t]; }
    int64_t n_nodes(int64_t t) const { return node_offsets[t + 1] - node_offsets[t]; }
    int64_t n_consts(int64_t t) const { return const_offsets[t + 1] - const_offsets[t]; }
    bool has_cse(int64_t t) const { return cse_nodes && cse_offsets[t + 1] > cse_offsets[t]; }
    const de_tape_node_t *cse_tape(int64_t t) const { return cse_nodes + cse_offsets[t]; }
    int64_t n_cse_nodes(int64_t t) const { return cse_offsets[t + 1] - cse_offsets[t]; }
};

// ---- per-tree units ------------------------------------------------------------------------------------------------------
// Both lowerings of a tree (plain, and with constant subtrees folded), and the folds of the folded one in the layout a program keeps its
// folds in — so that a unit reads a lowering and a tree of an old program alike
struct Lowered {
    TreeProgram plain, folded;
    int rc = DE_OK, rcf = DE_OK;
    bool cse = false, cse_plain = false;
    std::string why;
    std::vector<de_program::Fold> folds;    // (instr: relative to the tree's first folded instruction)
    std::vector<de_tape_node_t> fold_nodes; // the folds' tape slices, DE_LEAF_CONST arguments renumbered from the fold's first constant
    // [n_folds + 1 offsets into fold_nodes | n_folds + 1 offsets into the sources | the folds' constant sources, relative to the tree's first constant]
    std::vector<int64_t> fold_idx;
};
// Everything the link needs from one tree, position-independent: pointers and lengths into a Lowered or into an old program's vectors (a
// view, never a copy), and the bases that turn what they hold into indices relative to the tree
struct TreeUnit {
    const Instr *code, *fcode;                 // generic code; with folding: the folded code
    int32_t n_code, n_fcode;
    const int32_t *const_instr, *fconst_instr; // per constant slot: its instruction (+ instr_base / finstr_base), or -1
    const uint8_t *const_checks;               // per constant slot: CONST_CHECK_* bits
    int32_t instr_base, finstr_base;
    int32_t n_slots, fn_slots;                 // spill slots of the generic / the folded code
    uint8_t bits;                              // TREE_PARAMS | TREE_CSE_PLAIN | TREE_CSE_FOLDED
    int64_t n_folds;                           // with folding: the tree's folds ...
    const de_program::Fold *folds;             // ... instr (+ finstr_base), tested_always
    const int64_t *fold_noff, *fold_coff;      // ... n_folds + 1 offsets each: tape slices in fold_nodes, constant sources in fold_csrc
    const de_tape_node_t *fold_nodes;
    const int64_t *fold_csrc;                  // ... constant sources (+ const_base)
    int64_t const_base;
    static int32_t rel(int32_t i, int32_t base) { return i >= 0 ? i - base : -1; }
    int32_t const_at(int64_t k) const { return rel(const_instr[k], instr_base); }
    int32_t fconst_at(int64_t k) const { return rel(fconst_instr[k], finstr_base); }
    int64_t n_fold_nodes() const { return fold_noff[n_folds] - fold_noff[0]; }
    int64_t n_fold_consts() const { return fold_coff[n_folds] - fold_coff[0]; }
};
static const int64_t NO_FOLDS[1] = {0};
// Producer 1: a fresh lowering
static TreeUnit unit_of_lowering(const Lowered &L) {
    TreeUnit u{};
    u.code = L.plain.code.data();
    u.n_code = (int32_t)L.plain.code.size();
    u.const_instr = L.plain.const_instr.data();
    u.const_checks = L.plain.const_checks.data();
    u.n_slots = L.plain.n_slots;
    u.bits = (uint8_t)((L.plain.uses_params ? TREE_PARAMS : 0) | (L.cse_plain ? TREE_CSE_PLAIN : 0) | (L.cse ? TREE_CSE_FOLDED : 0));
    u.fcode = L.folded.code.data();
    u.n_fcode = (int32_t)L.folded.code.size();
    u.fconst_instr = L.folded.const_instr.data();
    u.fn_slots = L.folded.n_slots; // (a CSE program keeps one persistent row per shared subtree)
    u.n_folds = (int64_t)L.folds.size();
    u.folds = L.folds.data();
    u.fold_noff = L.folds.empty() ? NO_FOLDS : L.fold_idx.data();
    u.fold_coff = L.folds.empty() ? NO_FOLDS : L.fold_idx.data() + u.n_folds + 1;
    u.fold_nodes = L.fold_nodes.data();
    u.fold_csrc = u.fold_coff + u.n_folds + 1;
    return u;
}
// Producer 2: tree s of an existing program — the old program's absolute indices, rebased when they are read
static TreeUnit unit_of_kept(const Reuse &ru, size_t s) {
    const de_program *o = ru.old;
    TreeUnit u{};
    u.code = o->code.data() + o->code_off[s];
    u.n_code = o->code_off[s + 1] - o->code_off[s];
    u.const_instr = o->const_instr.data() + o->const_off[s];
    u.const_checks = o->const_checks.data() + o->const_off[s];
    u.instr_base = o->code_off[s];
    u.n_slots = u.fn_slots = o->tree_slots[s];
    u.bits = o->tree_bits[s];
    u.fold_noff = u.fold_coff = NO_FOLDS;
    if (!o->folded) return u;
    const int64_t j0 = ru.fold0[s];
    u.fcode = o->fcode.data() + o->fcode_off[s];
    u.n_fcode = o->fcode_off[s + 1] - o->fcode_off[s];
    u.fconst_instr = o->fconst_instr.data() + o->const_off[s];
    u.finstr_base = o->fcode_off[s];
    u.n_folds = ru.fold0[s + 1] - j0;
    u.folds = o->folds.data() + j0;
    u.fold_noff = o->fold_noff.data() + j0;
    u.fold_coff = o->fold_coff.data() + j0;
    u.fold_nodes = o->fold_nodes.data();
    u.fold_csrc = o->aux_const_src.data();
    u.const_base = o->const_off[s];
    return u;
}
// What the link's serial prefix sums need of a unit: one compact array, filled where the units are produced (a unit's own fields lie
// scattered over a Lowered and the heap — a cache miss or two per tree in a serial loop)
struct UnitSize { int rc, rcf; int32_t n_code, n_fcode, n_folds, n_fold_nodes, n_fold_consts; };
// The units of a creation.  kept(t) decides which producer tree t gets — here and nowhere else in this file.
struct Units {
    const Reuse *reuse;
    std::vector<Lowered> low; // (a kept tree's entry stays empty)
    std::vector<UnitSize> size;
    bool kept(int64_t t) const { return reuse && reuse->kept(t); }
    TreeUnit unit(int64_t t) const { return kept(t) ? unit_of_kept(*reuse, (size_t)reuse->src[(size_t)t]) : unit_of_lowering(low[(size_t)t]); }
    // the per-tree lowerings are ~16 small vectors each: released by the thread that merged them (one thread took 5 ms for 10^4 trees)
    void release(int64_t t) { Lowered done; std::swap(done, low[(size_t)t]); }
};

// The folds of a folded lowering as a unit holds them; `tape`: the tape the fold spans index
static void lowered_folds(Lowered &L, const de_tape_node_t *tape, int64_t n_consts) {
    const TreeProgram &tp = L.folded;
    const size_t nf = tp.folds.size();
    if (nf == 0) return;
    size_t nn = 0, nc = 0;
    for (const FoldSpan &sp : tp.folds) { nn += (size_t)(sp.node_end - sp.node_begin); nc += (size_t)(sp.const_end - sp.const_begin); }
    L.folds.resize(nf); // (three allocations per tree with folds, each of its final size)
    L.fold_nodes.resize(nn);
    L.fold_idx.assign(2 * (nf + 1) + nc, 0);
    int64_t *noff = L.fold_idx.data(), *coff = noff + nf + 1, *csrc = coff + nf + 1;
    for (size_t f = 0; f < nf; f++) {
        const FoldSpan &sp = tp.folds[f];
        L.folds[f] = {0, tp.const_instr[(size_t)n_consts + f], sp.tested_always};
        de_tape_node_t *out = L.fold_nodes.data() + noff[f];
        for (int32_t q = sp.node_begin; q < sp.node_end; q++) {
            de_tape_node_t nd = tape[q];
            if (nd.degree == 0 && nd.op == DE_LEAF_CONST) nd.arg = (uint16_t)(nd.arg - sp.const_begin);
            *out++ = nd;
        }
        for (int32_t q = sp.const_begin; q < sp.const_end; q++) csrc[coff[f] + (q - sp.const_begin)] = q;
        noff[f + 1] = noff[f] + (sp.node_end - sp.node_begin);
        coff[f + 1] = coff[f] + (sp.const_end - sp.const_begin);
    }
}
static void lower_one(const Population &in, int64_t t, const LowerOptions &lo, bool allow_fold, bool grad_cse, Lowered &L) {
    const int64_t nc = in.n_consts(t);
    L.rc = lower_tree(in.tape(t), in.n_nodes(t), nc, lo, &L.plain, &L.why);
    if (L.rc != DE_OK) return;
    if (in.has_cse(t) && grad_cse) {
        // GraphNode sharing in the GENERIC program too (round 3; the gradient kernels, eval_diff and the unfolded
        // eval run it): a shared subtree's dual number is computed once into a persistent slot and read by every
        // consumer — the reference evaluates it once per parent with the same arithmetic, so values, Jacobian rows
        // of features / parameters and flags are those of the expansion.  A constant inside a shared subtree keeps
        // the gradient row of its FIRST occurrence, which receives every consumer's contribution; the rows of its
        // later occurrences stay zero (callers sum the occurrence rows: the reference's shared NodeIndex row).
        TreeProgram pc;
        std::string why2;
        LowerOptions loc = lo;
        loc.cse = true;
        if (lower_tree(in.cse_tape(t), in.n_cse_nodes(t), nc, loc, &pc, &why2) == DE_OK) {
            L.plain = std::move(pc);
            L.cse_plain = true;
        }
    }
    if (!allow_fold) return;
    LowerOptions lof = lo;
    lof.fold = true;
    if (in.has_cse(t)) {
        LowerOptions loc = lof;
        loc.cse = true;
        L.rcf = lower_tree(in.cse_tape(t), in.n_cse_nodes(t), nc, loc, &L.folded, &L.why);
        L.cse = L.rcf == DE_OK;
        if (L.rcf == DE_ERR_UNSUPPORTED) {
            // the CSE form does not fit (spill slots + shared rows > 16, a share in an unsupported position): the
            // expanded tape has the same values and flags (the reference evaluates a shared node once per
            // parent), so this tree alone runs expanded instead of failing the whole population
            L.folded = TreeProgram();
            L.why.clear();
            L.rcf = lower_tree(in.tape(t), in.n_nodes(t), nc, lof, &L.folded, &L.why);
        }
    } else L.rcf = lower_tree(in.tape(t), in.n_nodes(t), nc, lof, &L.folded, &L.why);
    if (L.rcf == DE_OK) lowered_folds(L, L.cse ? in.cse_tape(t) : in.tape(t), nc);
}
// Phase 2: the trees that are not kept, lowered on the host threads; every unit's sizes.  false: out of host memory.
static bool lower_units(const Population &in, const LowerOptions &lo, bool allow_fold, const CreateEnv &env, Units *us) {
    us->low.resize((size_t)in.n_trees);
    us->size.resize((size_t)in.n_trees);
    std::atomic<bool> oom{false};
    parallel_for_trees(in.n_trees, [&](int64_t t) {
        Lowered &L = us->low[(size_t)t];
        if (!us->kept(t)) // (de_program_update: a kept tree's unit is a view of the old program)
            try { lower_one(in, t, lo, allow_fold, env.grad_cse, L); } catch (const std::bad_alloc &) { oom = true; }
        const TreeUnit u = us->unit(t);
        us->size[(size_t)t] = {L.rc, L.rcf, u.n_code, u.n_fcode, (int32_t)u.n_folds, (int32_t)u.n_fold_nodes(), (int32_t)u.n_fold_consts()};
    });
    return !oom;
}

// ---- the link: offsets by a serial prefix sum, then one copy per tree on the host threads (every tree writes slices of its own) that rebases
// by the tree's instruction base and constant base and writes the immediates (complex programs: the constant-table indices)
static void write_const(de_program *p, Instr &ins, bool cplx, size_t k) {
    if (cplx) write_cidx(ins, k);
    else write_imm(ins, p->dtype, p->consts[k]);
}
// Phase 3: the generic code, the constants and their bookkeeping, the retained input
static int link_generic(de_ctx *ctx, de_program *p, const Population &in, const Units &us, bool keep_input) {
    const int64_t n_trees = in.n_trees;
    const bool cplx = is_complex_io(p->io);
    uint64_t total = 0;
    for (int64_t t = 0; t < n_trees; t++) {
        const UnitSize &z = us.size[(size_t)t];
        if (z.rc != DE_OK) return fail(ctx, z.rc, "tree %lld: %s", (long long)t, us.low[(size_t)t].why.c_str());
        total += (uint64_t)z.n_code;
        if (total > 0x7fff0000u) return fail(ctx, DE_ERR_UNSUPPORTED, "program too large");
        p->code_off[(size_t)t + 1] = (int32_t)total;
    }
    p->code.resize((size_t)total);
    // the input, retained for de_program_update (copied per tree below; not for an auxiliary program, which is never updated by a
    // caller: an update of its parent rebuilds it from the parent's fold tapes)
    p->in_noff.clear();
    p->in_coff.clear();
    p->in_nodes.clear();
    p->in_cse.clear();
    if (keep_input) {
        p->in_noff.resize((size_t)n_trees + 1);
        p->in_coff.assign((size_t)n_trees + 1, 0);
        for (int64_t t = 0; t <= n_trees; t++) p->in_noff[(size_t)t] = n_trees ? in.node_offsets[t] - in.node_offsets[0] : 0;
        if (in.cse_nodes)
            for (int64_t t = 0; t <= n_trees; t++) p->in_coff[(size_t)t] = n_trees ? in.cse_offsets[t] - in.cse_offsets[0] : 0;
        p->in_nodes.resize((size_t)p->in_noff[(size_t)n_trees]);
        p->in_cse.resize((size_t)p->in_coff[(size_t)n_trees]);
    }
    struct Part { int32_t n_slots = 0; bool cse = false, params = false; int64_t nodes = 0; } part[HOST_RANGES_MAX];
    parallel_tree_ranges(n_trees, [&](int wk, int64_t tb, int64_t te) {
        Part &pt = part[wk];
        for (int64_t t = tb; t < te; t++) {
            if (keep_input) std::copy(in.tape(t), in.tape(t + 1), p->in_nodes.begin() + p->in_noff[(size_t)t]);
            if (keep_input && in.cse_nodes) std::copy(in.cse_tape(t), in.cse_tape(t + 1), p->in_cse.begin() + p->in_coff[(size_t)t]);
            const TreeUnit u = us.unit(t);
            const int64_t c0 = in.const_offsets[t], nc = in.n_consts(t), cb = c0 - in.const_offsets[0];
            const int32_t ib = p->code_off[(size_t)t];
            p->const_off[(size_t)t + 1] = cb + nc; // (entry t is tree t - 1's, entry 0 stays 0)
            p->n_consts_tree[(size_t)t] = (int32_t)nc;
            std::copy(u.code, u.code + u.n_code, p->code.begin() + ib);
            for (int64_t k = 0; k < nc; k++) {
                p->consts[(size_t)(cb + k)] = load_elem(p->io, in.consts, (size_t)(c0 + k));
                if (cplx) p->consts_im[(size_t)(cb + k)] = load_elem_im(p->io, in.consts, (size_t)(c0 + k));
                // (a CSE lowering has no instruction for the later occurrences of a constant inside a shared subtree: -1)
                const int32_t ci = u.const_at(k);
                p->const_instr[(size_t)(cb + k)] = ci >= 0 ? ib + ci : -1;
                p->const_checks[(size_t)(cb + k)] = u.const_checks[k];
                if (ci >= 0) write_const(p, p->code[(size_t)(ib + ci)], cplx, (size_t)(cb + k));
            }
            p->tree_slots[(size_t)t] = u.n_slots;
            p->tree_bits[(size_t)t] = (uint8_t)(u.bits & ~TREE_CSE_FOLDED); // (that bit: link_folded)
            pt.cse = pt.cse || (u.bits & TREE_CSE_PLAIN);
            pt.n_slots = std::max(pt.n_slots, u.n_slots);
            pt.params = pt.params || (u.bits & TREE_PARAMS);
            pt.nodes += in.n_nodes(t);
        }
    });
    for (const Part &pt : part) {
        p->cse_generic = p->cse_generic || pt.cse;
        p->n_slots = std::max(p->n_slots, pt.n_slots);
        p->uses_params = p->uses_params || pt.params;
        p->n_nodes += pt.nodes;
    }
    return DE_OK;
}
// Phase 4: the folded code, the folds and their tape slices (fold_nodes: retained, the host-folded subtrees are re-evaluated from them);
// every tree's lowering is released behind its copy.  *any_cse: some tree's eval program is its CSE lowering.
static int link_folded(de_ctx *ctx, de_program *p, const Population &in, Units *us, bool *any_cse) {
    const int64_t n_trees = in.n_trees;
    const bool cplx = is_complex_io(p->io);
    p->fcode_off.assign((size_t)n_trees + 1, 0);
    p->fconst_instr.assign(p->consts.size(), -1);
    // offsets of every tree's instructions, folds, fold tape nodes and fold constants by a serial prefix sum ...
    std::vector<int64_t> fold0((size_t)n_trees + 1, 0), anode0((size_t)n_trees + 1, 0), acs0((size_t)n_trees + 1, 0);
    uint64_t total = 0;
    for (int64_t t = 0; t < n_trees; t++) {
        const UnitSize &z = us->size[(size_t)t];
        if (z.rcf != DE_OK) return fail(ctx, z.rcf, "tree %lld (folded): %s", (long long)t, us->low[(size_t)t].why.c_str());
        total += (uint64_t)z.n_fcode;
        if (total > 0x7fff0000u) return fail(ctx, DE_ERR_UNSUPPORTED, "program too large");
        p->fcode_off[(size_t)t + 1] = (int32_t)total;
        fold0[(size_t)t + 1] = fold0[(size_t)t] + z.n_folds;
        anode0[(size_t)t + 1] = anode0[(size_t)t] + z.n_fold_nodes;
        acs0[(size_t)t + 1] = acs0[(size_t)t] + z.n_fold_consts;
    }
    p->fcode.resize((size_t)total);
    const size_t n_folds = (size_t)fold0[(size_t)n_trees];
    p->folds.resize(n_folds);
    p->fold_nodes.resize((size_t)anode0[(size_t)n_trees]);
    p->aux_const_src.resize((size_t)acs0[(size_t)n_trees]);
    p->fold_noff.assign(n_folds + 1, 0);
    p->fold_coff.assign(n_folds + 1, 0);
    // ... the copies on the host threads
    struct PartF { int32_t n_slots = 0; bool cse = false; } partf[HOST_RANGES_MAX];
    parallel_tree_ranges(n_trees, [&](int wk, int64_t tb, int64_t te) {
        PartF &pt = partf[wk];
        for (int64_t t = tb; t < te; t++) {
            const TreeUnit u = us->unit(t);
            const int64_t nc = in.n_consts(t), cb = in.const_offsets[t] - in.const_offsets[0];
            const int32_t ib = p->fcode_off[(size_t)t];
            pt.cse = pt.cse || (u.bits & TREE_CSE_FOLDED);
            pt.n_slots = std::max(pt.n_slots, u.fn_slots);
            p->tree_slots[(size_t)t] = std::max(p->tree_slots[(size_t)t], u.fn_slots);
            p->tree_bits[(size_t)t] |= u.bits & TREE_CSE_FOLDED;
            std::copy(u.fcode, u.fcode + u.n_fcode, p->fcode.begin() + ib);
            for (int64_t k = 0; k < nc; k++) {
                const int32_t ci = u.fconst_at(k);
                if (ci < 0) continue; // constant lives inside a folded subtree
                p->fconst_instr[(size_t)(cb + k)] = ib + ci;
                write_const(p, p->fcode[(size_t)(ib + ci)], cplx, (size_t)(cb + k));
            }
            const int64_t an0 = anode0[(size_t)t], ac0 = acs0[(size_t)t];
            std::copy(u.fold_nodes + u.fold_noff[0], u.fold_nodes + u.fold_noff[u.n_folds], p->fold_nodes.begin() + an0);
            for (int64_t q = u.fold_coff[0]; q < u.fold_coff[u.n_folds]; q++)
                p->aux_const_src[(size_t)(ac0 + (q - u.fold_coff[0]))] = u.fold_csrc[q] - u.const_base + cb;
            for (int64_t f = 0; f < u.n_folds; f++) {
                const size_t fi = (size_t)(fold0[(size_t)t] + f);
                p->folds[fi] = {(int32_t)t, ib + (u.folds[f].instr - u.finstr_base), u.folds[f].tested_always};
                p->fold_noff[fi + 1] = an0 + (u.fold_noff[f + 1] - u.fold_noff[0]);
                p->fold_coff[fi + 1] = ac0 + (u.fold_coff[f + 1] - u.fold_coff[0]);
            }
            us->release(t); // both lowerings of the tree are merged
        }
    });
    for (const PartF &pt : partf) {
        *any_cse = *any_cse || pt.cse;
        p->n_slots = std::max(p->n_slots, pt.n_slots);
    }
    return DE_OK;
}

// ---- the folds: who evaluates them ---------------------------------------------------------------------------------------------------------
// Tape slices, offsets and constant sources of a subset of the folds, in fold order (offsets: one leading 0)
struct FoldTapes {
    std::vector<de_tape_node_t> nodes;
    std::vector<int64_t> noff{0}, coff{0};
};
// fold_host: which folds stay on the host — subtrees of + - * / only (the turbo division is not IEEE: such programs fold everything on
// the device, with the operators they evaluate with; DE_NO_HOST_FOLD=1: everything on the device, for A/B tests) — and which go to
// de_fold_kernel: everything else whose evaluation stack fits (a turbo program evaluates with other operators than that kernel has: its
// subtrees stay with the auxiliary program; DE_NO_KERNEL_FOLD=1 for A/B tests)
static void classify_folds(de_program *p, const CreateEnv &env) {
    const bool cplx = is_complex_io(p->io), turbo = (p->options & DE_OPT_TURBO) != 0;
    // (complex programs: every subtree with the auxiliary program, which runs de_complex.hip — the unfolded bits by construction)
    const bool host_fold = env.host_fold && !(p->io != DE_F16 && turbo) && !cplx; // (DE_F16 ignores the turbo bit)
    // (a DE_F16 program's subtrees: de_fold_kernel does not round to binary16 — the auxiliary program, which runs de_half.hip, does)
    const bool kernel_fold = env.kernel_fold && !turbo && p->io != DE_F16 && !cplx;
    p->fold_host.assign(p->folds.size(), 0);
    parallel_for_trees((int64_t)p->folds.size(), [&](int64_t j) {
        const de_tape_node_t *nd = p->fold_nodes.data() + p->fold_noff[(size_t)j];
        const int64_t n = p->fold_noff[(size_t)j + 1] - p->fold_noff[(size_t)j];
        if (host_fold && host_foldable(nd, n)) { p->fold_host[(size_t)j] = 1; return; }
        if (!kernel_fold) return;
        int depth = 0, worst = 0;
        for (int64_t i = 0; i < n; i++) { depth += 1 - (int)nd[i].degree; worst = std::max(worst, depth); }
        if (worst <= DE_FOLD_STACK) p->fold_host[(size_t)j] = 2;
    }, 512);
}
// The kernel's subtrees (kfold, kf_csrc) and the auxiliary population (aux_fold, aux_csrc): positions by one serial prefix sum over the
// folds, the copies on the host threads
static void split_fold_tapes(de_program *p, FoldTapes *k, FoldTapes *x) {
    const size_t n_folds = p->folds.size();
    std::vector<int64_t> pos_n(n_folds), pos_c(n_folds);
    int64_t kn = 0, kc = 0, xn = 0, xc = 0;
    p->kfold.clear();
    p->aux_fold.clear();
    for (size_t j = 0; j < n_folds; j++) {
        const int64_t nn = p->fold_noff[j + 1] - p->fold_noff[j], nc = p->fold_coff[j + 1] - p->fold_coff[j];
        if (p->fold_host[j] == 2) {
            p->kfold.push_back((int32_t)j);
            pos_n[j] = kn; pos_c[j] = kc; kn += nn; kc += nc;
            k->noff.push_back(kn); k->coff.push_back(kc);
        } else if (p->fold_host[j] == 0) {
            p->aux_fold.push_back((int32_t)j);
            pos_n[j] = xn; pos_c[j] = xc; xn += nn; xc += nc;
            x->noff.push_back(xn); x->coff.push_back(xc);
        }
    }
    k->nodes.resize((size_t)kn);
    x->nodes.resize((size_t)xn);
    p->kf_csrc.resize((size_t)kc);
    p->aux_csrc.resize((size_t)xc);
    parallel_for_trees((int64_t)n_folds, [&](int64_t jj) {
        const size_t j = (size_t)jj;
        if (p->fold_host[j] == 1) return;
        const bool kern = p->fold_host[j] == 2;
        std::copy(p->fold_nodes.begin() + p->fold_noff[j], p->fold_nodes.begin() + p->fold_noff[j + 1], (kern ? k : x)->nodes.begin() + pos_n[j]);
        std::copy(p->aux_const_src.begin() + p->fold_coff[j], p->aux_const_src.begin() + p->fold_coff[j + 1], (kern ? p->kf_csrc : p->aux_csrc).begin() + pos_c[j]);
    }, 512);
}
// de_fold_kernel's device image [tape slices | node offsets | constant offsets | constant values | results | flags], with the present constants
static int upload_fold_kernel_image(de_ctx *ctx, de_program *p, const FoldTapes &k) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t nk = p->kfold.size(), es = p->dtype == DE_F32 ? 4 : 8;
    p->kf_o_noff = al(k.nodes.size() * sizeof(de_tape_node_t));
    p->kf_o_coff = p->kf_o_noff + al(k.noff.size() * sizeof(int64_t));
    p->kf_o_cvals = p->kf_o_coff + al(k.coff.size() * sizeof(int64_t));
    p->kf_o_out = p->kf_o_cvals + al(std::max<size_t>(p->kf_csrc.size(), 1) * es);
    p->kf_o_ok = p->kf_o_out + al(nk * es);
    p->kf_bytes = p->kf_o_ok + al(nk);
    std::vector<unsigned char> img(p->kf_o_out, 0);
    std::memcpy(img.data(), k.nodes.data(), k.nodes.size() * sizeof(de_tape_node_t));
    std::memcpy(img.data() + p->kf_o_noff, k.noff.data(), k.noff.size() * sizeof(int64_t));
    std::memcpy(img.data() + p->kf_o_coff, k.coff.data(), k.coff.size() * sizeof(int64_t));
    for (size_t i = 0; i < p->kf_csrc.size(); i++) store_elem(p->dtype, img.data() + p->kf_o_cvals, i, p->consts[(size_t)p->kf_csrc[i]]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipError_t kst = prog_malloc(ctx, reinterpret_cast<void **>(&p->d_kf), p->kf_bytes);
    if (kst != hipSuccess) return fail(ctx, DE_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(kst));
    HIP_TRY(ctx, hipMemcpy(p->d_kf, img.data(), img.size(), hipMemcpyHostToDevice));
    return DE_OK;
}

std::vector<int64_t> first_fold_of_trees(const de_program *p) {
    std::vector<int64_t> fold0((size_t)p->n_trees + 1, 0);
    for (const de_program::Fold &f : p->folds) fold0[(size_t)f.tree + 1]++;
    for (int64_t t = 0; t < p->n_trees; t++) fold0[(size_t)t + 1] += fold0[(size_t)t];
    return fold0;
}

extern "C" {
// The first opcode of a tape a complex program refuses (DE_ERR_UNSUPPORTED_OP), or -1
int complex_refused_op(const de_tape_node_t *nd, int64_t n) {
    for (int64_t i = 0; i < n; i++) {
        if (nd[i].degree == 0 || (nd[i].degree == 1 && nd[i].op == DE_OP_SHARE)) continue;
        if (!complex_opcode_ok(nd[i].degree, nd[i].op)) return nd[i].op;
    }
    return -1;
}
static int fail_complex_op(de_ctx *c, int op) {
    const char *nm = de_opcode_name(op);
    return fail(c, DE_ERR_UNSUPPORTED_OP, "opcode %s (%d) is not supported on complex data (DESIGN.md §14.1)", nm ? nm : "?", op);
}

static int create_impl(de_ctx_t *ctx, int dtype, const Population &in, int32_t n_features, int32_t n_params, uint32_t options, bool allow_fold,
                       const CreateEnv &env, de_program_t **out_program, const Reuse *reuse = nullptr, bool keep_input = true);

// (de_program_update: an auxiliary tree of a kept tree's fold is the old auxiliary program's tree of the same fold)
static void aux_reuse_map(const de_program *p, const Reuse &ru, Reuse *aru) {
    const de_program *o = ru.old;
    const std::vector<int64_t> fold0 = first_fold_of_trees(p);
    std::vector<int32_t> oaux(o->folds.size(), -1);
    for (size_t a = 0; a < o->aux_fold.size(); a++) oaux[(size_t)o->aux_fold[a]] = (int32_t)a;
    aru->old = o->aux;
    aru->src.assign(p->aux_fold.size(), -1);
    for (size_t a = 0; a < p->aux_fold.size(); a++) {
        const size_t j = (size_t)p->aux_fold[a];
        const int64_t t = p->folds[j].tree;
        if (!ru.kept(t)) continue;
        const size_t s = (size_t)ru.src[(size_t)t];
        aru->src[a] = oaux[(size_t)(ru.fold0[s] + ((int64_t)j - fold0[(size_t)t]))];
    }
    aru->fold0 = first_fold_of_trees(o->aux);
}
// Phase 6: the folds no other route takes, as a population of their own (never folded itself, never updated by a caller)
static int create_aux(de_ctx *ctx, de_program *p, const FoldTapes &x, const CreateEnv &env, const Reuse *reuse) {
    const bool cplx = is_complex_io(p->io);
    std::vector<unsigned char> ac(std::max<size_t>(p->aux_csrc.size(), 1) * dtype_bytes(p->io), 0);
    for (size_t k = 0; k < p->aux_csrc.size(); k++)
        store_elem(p->io, ac.data(), k, p->consts[(size_t)p->aux_csrc[k]], cplx ? p->consts_im[(size_t)p->aux_csrc[k]] : 0.0);
    Reuse aru;
    if (reuse && reuse->old->aux) aux_reuse_map(p, *reuse, &aru);
    const Population xin{(int64_t)p->aux_fold.size(), x.nodes.data(), x.noff.data(), nullptr, nullptr, ac.data(), x.coff.data()};
    return create_impl(ctx, p->io, xin, p->n_features, 0, p->options, false, env, &p->aux, aru.old ? &aru : nullptr, false);
}
// Phases 5 - 7: the folds of a linked program classified, their device images and the auxiliary program made, their values evaluated
static int make_folds(de_ctx *ctx, de_program *p, const CreateEnv &env, const Reuse *reuse, CreateTimer &tm) {
    classify_folds(p, env);
    FoldTapes k, x;
    split_fold_tapes(p, &k, &x);
    if (!p->kfold.empty())
        if (const int rc = upload_fold_kernel_image(ctx, p, k)) return rc;
    p->folded = true;
    if (is_complex_io(p->io)) fill_ctab_consts(p);
    tm.lap("folds: classify, kernel image, auxiliary tapes");
    if (!p->aux_fold.empty()) {
        if (const int rc = create_aux(ctx, p, x, env, reuse)) return rc;
        tm.lap("aux program (create)");
    }
    if (const int rc = refresh_folds(ctx, p, true)) return rc;
    tm.lap("folds (evaluate: host + kernel + aux)");
    return DE_OK;
}

// Phase 1: what a creation refuses about its arguments
static int check_create_args(de_ctx *ctx, const DtypeKind &kind, const Population &in, int32_t n_features, int32_t n_params) {
    if (kind.dtype < 0) return fail(ctx, DE_ERR_INVALID_ARG, "dtype must be DE_F32, DE_F64, DE_F16, DE_CF32 or DE_CF64");
    if (kind.cplx && n_params > 0) return fail(ctx, DE_ERR_UNSUPPORTED, "complex programs take no parameters (n_params = %d): parametric complex expressions are not supported", (int)n_params);
    if (in.n_trees < 0 || n_features < 0 || n_params < 0 || n_features > 65535 || n_params > 65535)
        return fail(ctx, DE_ERR_INVALID_ARG, "bad sizes");
    if (in.n_trees > 0 && (!in.nodes || !in.node_offsets || !in.const_offsets))
        return fail(ctx, DE_ERR_INVALID_ARG, "null tape pointers");
    if (in.n_trees > 0x7fffffff) return fail(ctx, DE_ERR_UNSUPPORTED, "too many trees");
    const int64_t total_consts = in.n_trees ? in.const_offsets[in.n_trees] - in.const_offsets[0] : 0;
    if (total_consts < 0) return fail(ctx, DE_ERR_INVALID_ARG, "const_offsets not monotone");
    if (total_consts > 0 && !in.consts) return fail(ctx, DE_ERR_INVALID_ARG, "consts is null");
    for (int64_t t = 0; t < in.n_trees; t++)
        if (in.n_nodes(t) < 0 || in.n_consts(t) < 0) return fail(ctx, DE_ERR_INVALID_ARG, "offsets not monotone at tree %lld", (long long)t);
    if (kind.cplx) // (the expanded tape holds every operator of the CSE one)
        for (int64_t t = 0; t < in.n_trees; t++) {
            const int op = complex_refused_op(in.tape(t), in.n_nodes(t));
            if (op >= 0) return fail_complex_op(ctx, op);
        }
    return DE_OK;
}

// Phase 10: ONE device arena per eval program (round 6): [record stream | its second half for the compacted live trees | tree offsets |
// compaction control ints | initial flags], one allocation from the context's pool; a small program (the one-tree call of
// de_eval_tree_array) goes up in ONE copy from a zero-filled host image, a large one in one memset + three copies.
static int upload_program(de_ctx *ctx, de_program *p, CreateTimer &tm) {
    // one trailing pad instruction: the flat-switch interpreter prefetches code[pc + 1]; the chained form of the
    // threaded kernel has one end record per tree and a head record (and the fused form is never longer than the bound one)
    const size_t cbytes = (p->bcode.size() + (size_t)p->n_trees + 2) * sizeof(BoundInstr); // + head record + one of padding
    // the early-exit walk (h_tree_skip) rebuilds record addresses from their low 32 bits: the stream must lie inside one
    // 4 GiB window.  An allocation that straddles a boundary (once in ~10^4 for a 400 KB stream) is set aside and redone.
    // (a threaded program allocates the stream twice: the second half receives the re-linked stream of the live trees, de_compact_live_kernel)
    // (wave groups: `waves` variants of the stream var_stride = cbytes / 16 records apart, and as much room again for their compacted forms)
    const size_t nvar = p->threaded && p->var_stride ? (p->assured ? 1 + (size_t)p->assured_tiers : (size_t)p->waves) : 1; // (the assured streams: one more variant per tier of a one-wave program)
    if (p->assured) p->assured_tiers_room = p->assured_tiers;
    if (nvar > 1 && (size_t)p->var_stride * sizeof(BoundInstr) != cbytes) return fail(ctx, DE_ERR_HIP, "wave-group stream variants: stride and arena disagree");
    const size_t abytes = p->threaded ? 2 * nvar * cbytes : cbytes;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t off_bytes = p->bcode_off.size() * sizeof(int32_t);
    const size_t ints_bytes = p->threaded ? ((size_t)2 * (size_t)p->n_trees + 5 + (size_t)DE_MEMO_MAX) * sizeof(int32_t) : 0; // (+ the records re-named per memo row)
    const size_t o_off = al(abytes), o_ints = o_off + al(off_bytes), o_ok = o_ints + al(ints_bytes);
    const size_t total = o_ok + al((size_t)std::max<int64_t>(p->n_trees, 1));
    const hipError_t ast = prog_malloc(ctx, reinterpret_cast<void **>(&p->d_code), total); // (one 4 GiB window: prog_malloc's contract)
    if (ast != hipSuccess) return fail(ctx, DE_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(ast));
    if (!in_one_window(p->d_code, abytes)) return fail(ctx, DE_ERR_HIP, "instruction stream straddles a 4 GiB boundary");
    char *base = reinterpret_cast<char *>(p->d_code);
    p->eval_arena = true; // (d_code_off, d_compact_ints, d_ok_eval live inside d_code's allocation: never freed on their own)
    p->d_code_off = reinterpret_cast<int32_t *>(base + o_off);
    p->d_ok_eval = reinterpret_cast<uint8_t *>(base + o_ok);
    if (p->threaded) {
        p->d_compact_code = p->d_code + nvar * cbytes / sizeof(BoundInstr);
        p->d_compact_ints = reinterpret_cast<int32_t *>(base + o_ints);
    }
    tm.lap("hipMalloc (arena)");
    const std::vector<BoundInstr> &stream = p->threaded ? p->ccode : p->bcode;
    const std::vector<int32_t> &offs = p->threaded ? p->ccode_off : p->bcode_off;
    hipError_t st = hipSuccess;
    if (total <= (size_t)(128u << 10)) {
        // (the second half of a threaded stream needs no initial content: de_compact_live_kernel writes what the launch proper reads)
        std::vector<unsigned char> img(total, 0);
        if (!stream.empty()) std::memcpy(img.data(), stream.data(), stream.size() * sizeof(BoundInstr));
        for (size_t w = 1; w < nvar; w++)
            std::memcpy(img.data() + w * cbytes, p->ccode_w.data() + (w - 1) * p->ccode.size(), p->ccode.size() * sizeof(BoundInstr));
        std::memcpy(img.data() + o_off, offs.data(), off_bytes);
        if (p->n_trees > 0) std::memcpy(img.data() + o_ok, p->host_ok_eval.data(), (size_t)p->n_trees);
        st = hipMemcpy(base, img.data(), total, hipMemcpyHostToDevice);
    } else {
        st = hipMemset(p->d_code, 0, nvar * cbytes);
        if (st == hipSuccess && !stream.empty()) st = hipMemcpy(p->d_code, stream.data(), stream.size() * sizeof(BoundInstr), hipMemcpyHostToDevice);
        if (st == hipSuccess) st = upload_wave_variants(p);
        if (st == hipSuccess) st = hipMemcpy(p->d_code_off, offs.data(), off_bytes, hipMemcpyHostToDevice);
        if (st == hipSuccess && p->n_trees > 0) st = hipMemcpy(p->d_ok_eval, p->host_ok_eval.data(), (size_t)p->n_trees, hipMemcpyHostToDevice);
    }
    if (st != hipSuccess) {
        prog_free(ctx, p->d_code);
        p->d_code = nullptr;
        return fail(ctx, DE_ERR_HIP, "program upload failed: %s", hipGetErrorString(st));
    }
    tm.lap("memset + upload (stream, offsets, flags)");
    return DE_OK;
}

// The phases of a creation, in order.  `reuse`: a de_program_update — which trees are kept, and from where.
static int create_phases(de_ctx *ctx, de_program *p, const Population &in, const CreateEnv &env, const Reuse *reuse, bool keep_input) {
    const int64_t n_trees = in.n_trees;
    const bool cplx = is_complex_io(p->io);
    CreateTimer tm{env.timing, (long long)n_trees, !p->allow_fold};
    p->code_off.assign((size_t)n_trees + 1, 0);
    p->const_off.assign((size_t)n_trees + 1, 0);
    p->n_consts_tree.assign((size_t)n_trees, 0);
    p->host_ok_eval.assign((size_t)n_trees, 1);
    p->host_ok_grad.assign((size_t)n_trees, 1);
    p->tree_slots.assign((size_t)n_trees, 0);
    p->tree_bits.assign((size_t)n_trees, 0);
    const size_t total_consts = n_trees ? (size_t)(in.const_offsets[n_trees] - in.const_offsets[0]) : 0;
    p->consts.resize(total_consts);
    p->const_instr.assign(total_consts, -1);
    p->const_checks.assign(total_consts, 0);
    if (cplx) p->consts_im.resize(total_consts);
    Units us{reuse, {}, {}};
    // A DE_F16 program with DE_OPT_F16_GRAD lowers its GENERIC (gradient) program from the expanded tape, as DE_NO_GRAD_CSE=1 does: every
    // occurrence of a shared constant keeps a row that holds its own partial.  The eval program keeps its CSE lowering.
    CreateEnv lenv = env;
    if (p->io == DE_F16 && (p->options & DE_OPT_F16_GRAD)) lenv.grad_cse = false;
    if (!lower_units(in, lower_options(p->options, p->n_features, p->n_params, p->dtype), p->allow_fold, lenv, &us)) return fail(ctx, DE_ERR_HIP, "out of host memory");
    tm.lap("lower (host threads)");
    if (const int rc = link_generic(ctx, p, in, us, keep_input)) return rc;
    tm.lap("merge plain");
    if (p->allow_fold) { // the folded lowering of the eval program + the auxiliary population of constant subtrees
        bool any_cse = false;
        if (const int rc = link_folded(ctx, p, in, &us, &any_cse)) return rc;
        tm.lap("merge folded");
        if (!p->folds.empty()) {
            if (const int rc = make_folds(ctx, p, env, reuse, tm)) return rc;
        } else if (any_cse) {
            p->folded = true; // the eval program is the CSE lowering even without a constant subtree to fold
        } else {
            p->fcode.clear();
            p->fcode_off.clear();
        }
    } else parallel_for_trees(n_trees, [&](int64_t t) { us.release(t); }); // (with folding: released in link_folded)
    tm.lap("release lowerings");
    if (cplx) fill_ctab_consts(p); // (the folds' entries stay: refresh_folds wrote them)
    recompute_host_ok(p);
    rebind(p, reuse);
    tm.lap("bind");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = make_threaded(ctx, p, reuse)) return rc;
    tm.lap("threaded + chained records");
    if (cplx)
        if (const int rc = upload_ctab(ctx, p)) return rc;
    if (const int rc = upload_program(ctx, p, tm)) return rc;
    return env.verify ? de_program_verify(p) : DE_OK;
}
static int create_impl(de_ctx_t *ctx, int dtype, const Population &in, int32_t n_features, int32_t n_params, uint32_t options, bool allow_fold,
                       const CreateEnv &env, de_program_t **out_program, const Reuse *reuse, bool keep_input) {
    if (!ctx) return DE_ERR_INVALID_ARG;
    if (!out_program) return fail(ctx, DE_ERR_INVALID_ARG, "out_program is null");
    *out_program = nullptr;
    const DtypeKind kind = dtype_kind(dtype);
    if (const int rc = check_create_args(ctx, kind, in, n_features, n_params)) return rc;
    std::unique_ptr<de_program> p(new (std::nothrow) de_program());
    if (!p) return fail(ctx, DE_ERR_HIP, "out of host memory");
    adopt_parked(ctx, p.get());
    p->ctx = ctx;
    p->dtype = kind.dtype;
    p->io = kind.io;
    p->options = options;
    p->n_features = n_features;
    p->n_params = n_params;
    p->n_trees = in.n_trees;
    p->allow_fold = allow_fold;
    try {
        if (const int rc = create_phases(ctx, p.get(), in, env, reuse, keep_input)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(ctx, DE_ERR_HIP, "out of host memory");
    }
    *out_program = p.release();
    return DE_OK;
}

int de_program_create(de_ctx_t *ctx, int dtype, const de_tape_node_t *nodes, const int64_t *node_offsets,
                      int64_t n_trees, const void *consts, const int64_t *const_offsets,
                      int32_t n_features, int32_t n_params, uint32_t options, de_program_t **out_program) {
    if (!ctx) return DE_ERR_INVALID_ARG;
    const CreateEnv env = read_create_env();
    const Population in{n_trees, nodes, node_offsets, nullptr, nullptr, consts, const_offsets};
    DE_NOTHROW(ctx, create_impl(ctx, dtype, in, n_features, n_params, options, env.fold, env, out_program));
}

int de_program_create_cse(de_ctx_t *ctx, int dtype, const de_tape_node_t *nodes, const int64_t *node_offsets,
                          const de_tape_node_t *cse_nodes, const int64_t *cse_offsets, int64_t n_trees, const void *consts,
                          const int64_t *const_offsets, int32_t n_features, int32_t n_params, uint32_t options,
                          de_program_t **out_program) {
    if (!ctx) return DE_ERR_INVALID_ARG;
    const CreateEnv env = read_create_env();
    if (n_trees > 0 && cse_nodes && !cse_offsets) return fail(ctx, DE_ERR_INVALID_ARG, "cse_offsets is null");
    const Population in{n_trees, nodes, node_offsets, env.fold && env.cse ? cse_nodes : nullptr, cse_offsets, consts, const_offsets};
    DE_NOTHROW(ctx, create_impl(ctx, dtype, in, n_features, n_params, options, env.fold, env, out_program));
}

// de_program_update: the resulting population's input is spliced from the retained one and the new trees, and a creation
// with a Reuse map builds the program in scratch — only the new trees are lowered, bound and fused; a kept tree's unit is a view of the old
// program's slices (generic and folded code, constant bookkeeping, folds), its auxiliary trees, bound, fused and wave-variant code are
// copied from it, and the program-wide passes (fold evaluation, flags, threaded words, chained records, upload) run as at creation.  On
// success the scratch program takes the old one's place; the old state is destroyed after a stream synchronisation (work already queued
// completes with it).
static int update_impl(de_program_t *p, const int64_t *tree_ids, int64_t n_update, const de_tape_node_t *nodes, const int64_t *node_offsets,
                       const de_tape_node_t *cse_nodes, const int64_t *cse_offsets, const void *consts, const int64_t *const_offsets) {
    de_ctx *ctx = p->ctx;
    if (n_update < 0) return fail(ctx, DE_ERR_INVALID_ARG, "n_update < 0");
    if (n_update == 0) return DE_OK;
    if (const int mrc = consts_materialise(p)) return mrc; // (the kept trees' constants and code are copied from the host side: §3.5)
    if (!tree_ids || !nodes || !node_offsets || !const_offsets) return fail(ctx, DE_ERR_INVALID_ARG, "null tree ids or tape pointers");
    if (cse_nodes && !cse_offsets) return fail(ctx, DE_ERR_INVALID_ARG, "cse_offsets is null");
    const int64_t n = p->n_trees;
    if (p->in_noff.size() != (size_t)n + 1) return fail(ctx, DE_ERR_UNSUPPORTED, "the program keeps no input to update (an auxiliary program)");
    std::vector<int32_t> slot((size_t)n, -1); // tree -> its position in the update, -1: kept
    for (int64_t u = 0; u < n_update; u++) {
        const int64_t t = tree_ids[u];
        if (t < 0 || t >= n) return fail(ctx, DE_ERR_OUT_OF_RANGE, "tree id %lld outside [0, %lld)", (long long)t, (long long)n);
        if (slot[(size_t)t] >= 0) return fail(ctx, DE_ERR_INVALID_ARG, "tree id %lld appears twice", (long long)t);
        slot[(size_t)t] = (int32_t)u;
    }
    for (int64_t u = 0; u < n_update; u++)
        if (node_offsets[u + 1] < node_offsets[u] || const_offsets[u + 1] < const_offsets[u] || (cse_nodes && cse_offsets[u + 1] < cse_offsets[u]))
            return fail(ctx, DE_ERR_INVALID_ARG, "offsets not monotone at new tree %lld", (long long)u);
    if (const_offsets[n_update] > const_offsets[0] && !consts) return fail(ctx, DE_ERR_INVALID_ARG, "consts is null");
    const CreateEnv env = read_create_env();
    // the CSE tapes as de_program_create_cse would take them now
    if (!p->allow_fold || !env.cse) cse_nodes = nullptr;
    // the resulting population's input: tapes, CSE tapes, constants in the caller's element type, offsets
    const size_t es = dtype_bytes(p->io);
    std::vector<de_tape_node_t> nn, cn;
    std::vector<int64_t> noff((size_t)n + 1, 0), coff((size_t)n + 1, 0), koff((size_t)n + 1, 0);
    for (int64_t t = 0; t < n; t++) {
        const int64_t u = slot[(size_t)t];
        noff[(size_t)t + 1] = noff[(size_t)t] + (u >= 0 ? node_offsets[u + 1] - node_offsets[u] : p->in_noff[(size_t)t + 1] - p->in_noff[(size_t)t]);
        coff[(size_t)t + 1] = coff[(size_t)t] + (u >= 0 ? (cse_nodes ? cse_offsets[u + 1] - cse_offsets[u] : 0) : p->in_coff[(size_t)t + 1] - p->in_coff[(size_t)t]);
        koff[(size_t)t + 1] = koff[(size_t)t] + (u >= 0 ? const_offsets[u + 1] - const_offsets[u] : p->const_off[(size_t)t + 1] - p->const_off[(size_t)t]);
    }
    nn.resize((size_t)noff[(size_t)n]);
    cn.resize((size_t)coff[(size_t)n]);
    std::vector<unsigned char> kv(std::max<size_t>((size_t)koff[(size_t)n], 1) * es, 0);
    parallel_tree_ranges(n, [&](int, int64_t tb, int64_t te) {
        for (int64_t t = tb; t < te; t++) {
            const int64_t u = slot[(size_t)t];
            if (u >= 0) {
                std::copy(nodes + node_offsets[u], nodes + node_offsets[u + 1], nn.begin() + noff[(size_t)t]);
                if (cse_nodes) std::copy(cse_nodes + cse_offsets[u], cse_nodes + cse_offsets[u + 1], cn.begin() + coff[(size_t)t]);
                if (koff[(size_t)t + 1] > koff[(size_t)t])
                    std::memcpy(kv.data() + (size_t)koff[(size_t)t] * es, static_cast<const unsigned char *>(consts) + (size_t)const_offsets[u] * es,
                                (size_t)(koff[(size_t)t + 1] - koff[(size_t)t]) * es);
            } else {
                std::copy(p->in_nodes.begin() + p->in_noff[(size_t)t], p->in_nodes.begin() + p->in_noff[(size_t)t + 1], nn.begin() + noff[(size_t)t]);
                std::copy(p->in_cse.begin() + p->in_coff[(size_t)t], p->in_cse.begin() + p->in_coff[(size_t)t + 1], cn.begin() + coff[(size_t)t]);
                for (int64_t k = 0; k < koff[(size_t)t + 1] - koff[(size_t)t]; k++) {
                    const size_t ok = (size_t)(p->const_off[(size_t)t] + k);
                    store_elem(p->io, kv.data(), (size_t)(koff[(size_t)t] + k), p->consts[ok], p->consts_im.empty() ? 0.0 : p->consts_im[ok]);
                }
            }
        }
    }, 256);
    // Float32 / Float64 programs splice; binary16 and complex ones (their constant-table indices and rounding) are rebuilt whole, as is a
    // program whose creation had no folded stream to copy from
    Reuse ru;
    if ((p->io == DE_F32 || p->io == DE_F64) && (!p->allow_fold || p->folded) && env.update_splice) {
        ru.old = p;
        ru.src.resize((size_t)n);
        for (int64_t t = 0; t < n; t++) ru.src[(size_t)t] = slot[(size_t)t] >= 0 ? -1 : (int32_t)t;
        ru.fold0 = first_fold_of_trees(p);
    }
    const bool any_cse = coff[(size_t)n] > 0;
    const Population in{n, nn.data(), noff.data(), any_cse ? cn.data() : nullptr, any_cse ? coff.data() : nullptr, kv.data(), koff.data()};
    de_program_t *q = nullptr;
    const int rc = create_impl(ctx, p->io, in, p->n_features, p->n_params, p->options, p->allow_fold, env, &q, ru.old ? &ru : nullptr);
    if (rc != DE_OK) return rc; // (create_impl released its scratch program: the old one is untouched)
    std::swap(*p, *q);
    return de_program_destroy(q); // (synchronises the stream first)
}

int de_program_update(de_program_t *prog, const int64_t *tree_ids, int64_t n_update, const de_tape_node_t *nodes, const int64_t *node_offsets,
                      const de_tape_node_t *cse_nodes, const int64_t *cse_offsets, const void *consts, const int64_t *const_offsets) {
    if (!prog) return DE_ERR_INVALID_ARG;
    DE_NOTHROW(prog->ctx, update_impl(prog, tree_ids, n_update, nodes, node_offsets, cse_nodes, cse_offsets, consts, const_offsets));
}

int de_program_destroy(de_program_t *p) {
    if (!p) return DE_OK;
    (void)hipSetDevice(p->ctx->device);
    dbg_lap(nullptr);
    (void)hipStreamSynchronize(p->ctx->stream);
    de_ctx *c = p->ctx;
    dbg_lap("destroy: stream sync");
    prog_free(c, p->d_code);
    if (!p->eval_arena) {
        if (p->d_code_off) (void)hipFree(p->d_code_off);
        if (p->d_compact_ints) (void)hipFree(p->d_compact_ints);
    }
    if (p->d_cert_code) (void)hipFree(p->d_cert_code);
    if (p->d_ctab) (void)hipFree(p->d_ctab);
    if (p->d_cert_off) (void)hipFree(p->d_cert_off);
    dbg_lap("destroy: eval streams");
    if (p->aux) de_program_destroy(p->aux);
    gn_wide_release(p);
    prog_free(c, p->d_kf);
    p->d_kf = nullptr;
    prog_free(c, p->d_cp); // (de_program_set_consts_device: site tables, the program's own constants)
    prog_free(c, p->d_cp_vals);
    p->d_cp = p->d_cp_vals = nullptr;
    dbg_lap(nullptr);
    prog_free(c, p->d_gcode);
    if (p->d_gcode_off) (void)hipFree(p->d_gcode_off);
    prog_free(c, p->d_gtcode);
    if (p->d_gtcode_off) (void)hipFree(p->d_gtcode_off);
    if (p->d_gt_ids) (void)hipFree(p->d_gt_ids);
    prog_free(c, p->d_rtcode);
    for (void *q : {(void *)p->d_rtcode_off, (void *)p->d_rtcode_mid, (void *)p->d_rt_ids})
        if (q) (void)hipFree(q);
    if (p->d_ok_eval && !p->eval_arena) (void)hipFree(p->d_ok_eval);
    for (void *q : {(void *)p->d_ok_grad, (void *)p->d_ng, (void *)p->d_goff})
        if (q) (void)hipFree(q);
    dbg_lap("destroy: gradient streams, flags");
    p->aux = nullptr;
    park_program(c, p);
    dbg_lap("destroy: host vectors");
    return DE_OK;
}

int64_t de_program_n_trees(const de_program_t *p) { return p ? p->n_trees : -1; }
int64_t de_program_n_nodes(const de_program_t *p) { return p ? p->n_nodes : -1; }
int64_t de_program_n_grad(const de_program_t *p, int64_t tree, int mode) {
    if (!p || tree < 0 || tree >= p->n_trees) return -1;
    const int64_t nc = p->n_consts_tree[(size_t)tree];
    const int64_t nv = (int64_t)p->n_features + p->n_params;
    switch (mode) {
    case DE_GRAD_VARIABLE: return nv;
    case DE_GRAD_CONSTANT: return nc;
    case DE_GRAD_BOTH: return nv + nc;
    default: return -1;
    }
}

int de_program_last_live_trees(de_program_t *p, int64_t *n_live) {
    if (!p || !n_live) return DE_ERR_INVALID_ARG;
    *n_live = -1;
    if (!p->last_compacted || !p->d_compact_ints) return DE_OK;
    de_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int32_t v = -1;
    HIP_TRY(c, hipMemcpy(&v, p->d_compact_ints + (2 * (size_t)p->n_trees + 1), sizeof v, hipMemcpyDeviceToHost));
    *n_live = v;
    return DE_OK;
}

// The memo rows of the program (de_api_internal.h `memo`): row r remembers operator k[r] (0 cos, 1 exp) of feature feat[r] (0-based), which
// uses[r] instructions of the tightest assured tier evaluate.  Arrays of de_memo_rows_max() entries, any may be null.  Returns the rows.
int32_t de_program_memo_rows(const de_program_t *p, int32_t *k, int32_t *feat, int64_t *uses) {
    if (!p) return -1;
    for (int r = 0; r < p->memo.n; r++) {
        if (k) k[r] = p->memo.k[r];
        if (feat) feat[r] = p->memo.feat[r];
        if (uses) uses[r] = p->memo.uses[r];
    }
    return p->memo.n;
}
// What the most recent eval launch re-named: named[r] = the records of the LAST stream variant handed to memo row r's handlers
// (de_memo_rows_max() entries); all -1 when that launch did not compact its live trees (synchronises the stream like de_program_last_live_trees).
int de_program_last_memo_named(de_program_t *p, int64_t *named) {
    if (!p || !named) return DE_ERR_INVALID_ARG;
    for (int r = 0; r < DE_MEMO_MAX; r++) named[r] = -1;
    if (!p->last_compacted || !p->d_compact_ints) return DE_OK;
    de_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int32_t v[DE_MEMO_MAX];
    HIP_TRY(c, hipMemcpy(v, p->d_compact_ints + (2 * (size_t)p->n_trees + 5), sizeof v, hipMemcpyDeviceToHost));
    for (int r = 0; r < DE_MEMO_MAX; r++) named[r] = v[r];
    return DE_OK;
}

int de_prio_tiles_wanted(int64_t N, int32_t n_features, int64_t n_trees) { return prio_tiles_wanted(N, n_features, n_trees) ? 1 : 0; }
} // extern "C"
