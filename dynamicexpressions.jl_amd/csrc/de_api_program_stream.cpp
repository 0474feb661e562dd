// de_api_program_stream.cpp — the streams the eval kernels execute, derived from a program's generic (or folded) code: the bound stream
// (rebind), the fused and threaded forms, the chained records, the stream variants of a wave group and the assured stream (make_threaded).
// A kept tree of a de_program_update takes its bound, fused and variant code over from the old program (Reuse::kept, de_api_program.h).
#include "de_api_program.h"

extern "C" {
// Early exit at tree granularity (kernels: a workgroup does not evaluate the trees whose flag is already 0).  DE_NO_TREE_SKIP=1
// restores the evaluate-everything behaviour for A/B measurements (the option bit DE_OPT_FULL_EVAL does the same per program).
bool tree_skip_enabled() {
    static const bool on = [] { const char *v = getenv("DE_NO_TREE_SKIP"); return !(v && *v == '1'); }();
    return on;
}
// Parameters as staged rows (round 3): every use of a parameter was a gather of its samples' values through the vector cache (h_param:
// 4 loads per lane and use; per-sample parameters, C = N, ran at 27 % VALU utilisation).  With <= 16 parameters the eval kernels
// instead stage the tile's parameter values once per workgroup, transposed like X, into P more LDS rows behind the spill slots and
// the binder treats a parameter operand as a row operand (every fused form applies).  DE_NO_PARAM_ROWS=1: the gathers.
static bool param_rows_enabled() { // (read at every de_program_create: the tests switch it inside one process)
    const char *v = getenv("DE_NO_PARAM_ROWS");
    return !(v && *v == '1');
}
// `ru` (de_program_update): a kept tree's bound code is copied when the binder's inputs are the old program's — the same source stream
// (folded or not), spill slots and parameter rows; a tree's bound code depends on its own instructions and those only
static bool same_binding(const de_program *p, const de_program *old) {
    return old->folded == p->folded && old->prows == p->prows && old->n_slots == p->n_slots && old->n_features == p->n_features &&
           old->n_params == p->n_params && old->options == p->options && old->dtype == p->dtype;
}
void rebind(de_program *p, const Reuse *ru) {
    const bool ee = (p->options & DE_OPT_EARLY_EXIT) != 0;
    p->prows = p->uses_params && p->n_params > 0 && p->n_params <= 16 && param_rows_enabled() &&
               ((size_t)p->n_features + (size_t)p->n_slots + (size_t)p->n_params) * 257 * 16 <= 150 * 1024;
    const int prb = p->prows ? p->n_features + p->n_slots : -1;
    const std::vector<Instr> &src = p->folded ? p->fcode : p->code;
    const std::vector<int32_t> &off = p->folded ? p->fcode_off : p->code_off;
    const int nf = p->n_features;
    const de_program *old = ru && ru->old && same_binding(p, ru->old) ? ru->old : nullptr;
    build_stream_by_trees<BoundInstr>(p->n_trees, &p->bcode, &p->bcode_off, [&](int64_t t, std::vector<BoundInstr> *out) {
        if (old && ru->kept(t)) {
            const size_t s = (size_t)ru->src[(size_t)t];
            out->insert(out->end(), old->bcode.begin() + old->bcode_off[s], old->bcode.begin() + old->bcode_off[s + 1]);
            return;
        }
        const int32_t i0 = off[(size_t)t], i1 = off[(size_t)t + 1];
        bind_tree(src.data() + i0, (size_t)(i1 - i0), ee, nf, out, prb);
    });
    match_const_sites(src, off, p->bcode, p->bcode_off, p->n_trees, [](const BoundInstr &b) { return bop_is_const_source(b.bop); }, &p->bsite);
    p->tsite.clear();
    p->site_gen++;
}
// (bind_tree / fuse_tree are ~0.3 us per tree — 3 ms each for 10^4 trees on one thread: build_stream_by_trees)

// Threaded-code form of the bound program (de_kernels.hip, de_eval_threaded_kernel): word 0 =
// handler address - handler_base, word 1 = LDS byte offset of the operand row | aux << 24.
// DE_DEBUG_TIMING: microseconds since the previous lap of this thread, on stderr
static void make_chained(de_program *p);
// Waves per workgroup of the threaded eval kernel (de_api_internal.h `waves`).  A one-wave workgroup keeps F rows of X, S spill-slot rows
// and (parametric) P staged parameter rows in LDS: at F = 5, S = 2 that is 21 resident waves per CU (5.25 per SIMD; the kernel's registers
// allow 28) and more buys nothing (measured: W = 2 +1 %, W = 4 +6 % on the headline) — but 8 parameter rows leave 10 waves, 20 features 7, 30
// features 4.  W waves share X and the parameter rows: W is doubled (1 -> 2 -> 4 -> 8) while the workgroup is below 20 resident waves per CU and
// the step raises them by half or more.  Measured, 10^6 samples x 1000 trees: 8 per-sample parameters 1.35 -> 0.92 ms, F = 12 1.29 -> 0.97,
// F = 20 2.06 -> 1.08, F = 30 3.10 -> 1.22 (profiles/r6_wave_groups.txt).  DE_EVAL_WAVES = 1 | 2 | 4 | 8 overrides (1 = the kernel of rounds 1-5).
static int choose_waves(const de_program *p) {
    if (TBLK != 64 || (p->uses_params && !p->prows)) return 1; // (gathered parameters: the class row is per wave)
    if (const char *e = getenv("DE_EVAL_WAVES")) { const int v = atoi(e); return (v == 2 || v == 4 || v == 8) ? v : 1; }
    const size_t rb = trow_bytes(p->dtype), lds_cu = 160u << 10, shared = (size_t)p->n_features + (p->prows ? (size_t)p->n_params : 0);
    auto resident = [&](int W) -> size_t {
        const size_t lds = (shared + (size_t)W * (size_t)p->n_slots) * rb + (size_t)W * 256;
        // (7 waves per SIMD by the kernel's vector registers; a group of W >= 4 waves puts W / 4 on every SIMD)
        const size_t by_regs = W >= 4 ? 7 / ((size_t)W / 4) : 28 / (size_t)W;
        return lds > 150u * 1024 ? 0 : std::min<size_t>(lds_cu / lds, by_regs) * (size_t)W;
    };
    int best = 1;
    size_t have = resident(1);
    for (int W : {2, 4, 8}) {
        const size_t w = resident(W);
        if (have >= 20) break;
        if (w * 2 < have * 3) { // (many slot rows: two waves gain too little — four may still, when the workgroup is below 3 waves per SIMD)
            if (W == 2 && have < 12) continue;
            break;
        }
        best = W;
        have = w;
    }
    return best;
}
static void make_assured(de_program *p, const uint64_t *table);
// DE_ASSURED_XMAX as the pass and the kernel both take it: rounded to Float32 (the kernel compares in Float32), 64 when unset or out of range
double assured_xmax_env() {
    const char *ax = getenv("DE_ASSURED_XMAX");
    const double xm = ax ? (double)(float)atof(ax) : 64.0;
    return (xm >= 0x1p-40 && xm <= 0x1p100) ? xm : 64.0;
}
// DE_ASSURED_PARTS: which tests the pass may elide (de_bind.h ASSURED_PART_*; default: the parts that measured faster)
uint32_t assured_parts_env() {
    const char *ap = getenv("DE_ASSURED_PARTS");
    const int v = ap && *ap ? atoi(ap) : (int)ASSURED_PARTS_SHIPPED;
    return (uint32_t)v & ASSURED_PARTS_ALL;
}
// The tight tier's fact (de_api_internal.h assured_tiers): DE_ASSURED_TIGHT_XMAX / DE_ASSURED_TIGHT_AMIN, rounded to Float32 like the wide
// bound; the defaults when unset or out of range, and never wider than the wide fact [2^-39, xmax] (a tight fact equal to the wide one
// proves nothing more: such a program builds one tier).  DE_ASSURED_TIERS=1: one tier, the behaviour before tiers, for A/B runs.
static void assured_tight_env(double xmax, double *txmax, double *tamin) {
    const char *ax = getenv("DE_ASSURED_TIGHT_XMAX"), *am = getenv("DE_ASSURED_TIGHT_AMIN");
    double tx = ax && *ax ? (double)(float)atof(ax) : ASSURED_TIGHT_XMAX, ta = am && *am ? (double)(float)atof(am) : ASSURED_TIGHT_AMIN;
    if (!(tx >= 0x1p-40 && tx <= 0x1p100)) tx = ASSURED_TIGHT_XMAX;
    if (!(ta >= 0x1p-39 && ta <= 0x1p100)) ta = ASSURED_TIGHT_AMIN;
    tx = std::min(tx, xmax);
    *txmax = tx;
    *tamin = std::min(ta, tx);
}
static int assured_tiers_env() {
    const char *at = getenv("DE_ASSURED_TIERS");
    return at && *at == '1' ? 1 : 2;
}
// DE_ASSURED / DE_ASSURED_XMAX and their kin: read once per program (an update keeps what its program `old` was created with)
static void assured_configure(de_program *p, const de_program *old) {
    if (p->assured_cfg != 0) return;
    if (old && old->assured_cfg != 0) {
        p->assured_cfg = old->assured_cfg;
        p->assured_xmax = old->assured_xmax;
        p->assured_parts = old->assured_parts;
        p->assured_tiers_cfg = old->assured_tiers_cfg;
        p->assured_tight_xmax = old->assured_tight_xmax;
        p->assured_tight_amin = old->assured_tight_amin;
        return;
    }
    const char *as = getenv("DE_ASSURED");
    p->assured_parts = assured_parts_env();
    p->assured_cfg = ((as && *as == '0') || p->assured_parts == 0) ? -1 : 1;
    p->assured_xmax = assured_xmax_env();
    p->assured_tiers_cfg = assured_tiers_env();
    assured_tight_env(p->assured_xmax, &p->assured_tight_xmax, &p->assured_tight_amin);
}
// fused instruction -> threaded words (also what make_wave_variants re-derives the operand words of the other waves' streams with)
struct ThreadedEnc {
    const uint64_t *table; // the device's handler table, and its lowest address
    uint64_t base;
    bool hot_unary;        // unary operators outside the binder's hot set: their own handlers (DE_NO_CONST_UNARY_HOT: the generic one)
    uint32_t row_bytes, class_row; // bytes of an LDS row; byte offset of the class row of a gathered parameter (behind X and the spill slots)
};
static BoundInstr threaded_words(const ThreadedEnc &e, const BoundInstr &b) {
    const uint64_t *table = e.table;
    BoundInstr t = b;
    t.bop = (uint32_t)(table[b.bop] - e.base);
    if (e.hot_unary && (b.bop == BOP_GEN_ROW || b.bop == BOP_GEN_ACC)) {
        const int k = gun_index((int)(b.arg >> 24), DE_U_COS, DE_U_EXP, DE_U_SIN, DE_U_NEG, DE_U_SQUARE, DE_U_CUBE, DE_U_ABS, DE_U_LOG, DE_U_SAFE_LOG,
                                DE_U_SQRT, DE_U_SAFE_SQRT, DE_U_TANH, DE_U_RELU);
        if (k >= 3) t.bop = (uint32_t)(table[TOPX_UN_BASE + (uint32_t)(k - 3) * 2 + (b.bop == BOP_GEN_ACC ? 1 : 0)] - e.base);
    }
    if (e.hot_unary && (b.bop == BOP_GEN_ROW || b.bop == BOP_GEN_CONST) && ((b.arg >> 24) == (uint32_t)DE_B_MAX || (b.arg >> 24) == (uint32_t)DE_B_MIN))
        t.bop = (uint32_t)(table[TOPX_BIN_BASE + ((b.arg >> 24) == (uint32_t)DE_B_MAX ? 0u : 2u) + (b.bop == BOP_GEN_CONST ? 1u : 0u)] - e.base);
    if (b.bop < BOP_COUNT && bop_is_const_source(b.bop)) {
        t.arg = b.arg & 0xFF000000u; // constant ordinal is only for the gradient kernel
    } else if (b.bop == BOP_GEN_PARAM) { // immediate = LDS byte offset of the class row
        t.lo = e.class_row;
        t.hi = 0;
    } else {
        const uint32_t row = b.arg & 0xFFFFFFu, aux = b.arg >> 24;
        t.arg = (row * e.row_bytes) | (aux << 24);
        if (b.bop == BOP_TERN) t.lo = (b.lo - row) * e.row_bytes; // byte distance row B -> row C (mod 2^32)
        if (b.bop >= TOP_BIN2_BASE && b.bop < TOP_COUNT && !(((b.bop - TOP_BIN2_BASE) >> 2) & 1))
            t.lo = (uint32_t)((int32_t)b.lo * (int32_t)e.row_bytes); // row-row: byte distance row A -> row B
    }
    return t;
}
// Wave groups: the stream variants of waves 1 .. W - 1 (de_api_internal.h `waves`) — the chained records of wave 0 with the operand words
// of the tree bound and fused against wave w's slot rows.  `old`: the program a kept tree's variant words are copied from, or null.
static void make_wave_variants(de_program *p, const ThreadedEnc &enc, int W, const FuseRows &rows0, const de_program *old, const Reuse *ru) {
    const bool ee = (p->options & DE_OPT_EARLY_EXIT) != 0, f32 = p->dtype == DE_F32;
    const std::vector<Instr> &src = p->folded ? p->fcode : p->code;
    const std::vector<int32_t> &off = p->folded ? p->fcode_off : p->code_off;
    const int prb = p->prows ? p->n_features + p->n_slots : -1, n_prows = p->prows ? p->n_params : 0;
    const size_t n_rec = p->ccode.size();
    p->ccode_w.resize(n_rec * (size_t)(W - 1));
    std::atomic<bool> same{true};
    const bool wold = old && old->waves == W && old->var_stride != 0 && old->ccode_w.size() == old->ccode.size() * (size_t)(W - 1);
    for (int w = 1; w < W; w++) {
        BoundInstr *cw = p->ccode_w.data() + n_rec * (size_t)(w - 1);
        const int shift = n_prows + w * p->n_slots; // [X | slots of wave 0 | parameter rows | slots of wave 1 | ...]: slot s of wave w = row F + S + P + (w - 1) S + s
        const FuseRows rows_w{(uint32_t)(p->n_features + shift), (uint32_t)(p->n_features + shift + p->n_slots), shift, rows0.headroom};
        parallel_tree_ranges(p->n_trees, [&](int, int64_t tb, int64_t te) {
            std::vector<BoundInstr> b, f;
            // (the records of trees tb .. te - 1 behind the header in front of tree tb, which is tree tb - 1's end record: disjoint ranges)
            const size_t r0 = (size_t)p->ccode_off[(size_t)tb] - 1, r1 = te < p->n_trees ? (size_t)p->ccode_off[(size_t)te] - 1 : n_rec;
            std::copy(p->ccode.begin() + (long)r0, p->ccode.begin() + (long)r1, cw + r0);
            for (int64_t t = tb; t < te; t++) {
                const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1];
                const size_t h = (size_t)p->ccode_off[(size_t)t];
                if (wold && ru->kept(t)) { // the old variant's operand words of the same records
                    const size_t ho = (size_t)old->ccode_off[(size_t)ru->src[(size_t)t]];
                    const BoundInstr *ow = old->ccode_w.data() + old->ccode.size() * (size_t)(w - 1);
                    for (int32_t i = 0; i < i1 - i0; i++) {
                        BoundInstr &r = cw[h + (size_t)i];
                        const BoundInstr &o = ow[ho + (size_t)i];
                        r.bop = o.bop;
                        if (f32) r.arg = o.arg;
                        else { r.lo = o.lo; r.hi = o.hi; }
                    }
                    continue;
                }
                b.clear();
                f.clear();
                bind_tree(src.data() + off[(size_t)t], (size_t)(off[(size_t)t + 1] - off[(size_t)t]), ee, p->n_features, &b, prb, shift);
                fuse_tree(b.data(), b.size(), &f, &rows_w);
                if ((int32_t)f.size() != i1 - i0) { same = false; return; }
                for (int32_t i = i0; i < i1; i++) {
                    if (f[(size_t)(i - i0)].bop != p->fbcode[(size_t)i].bop) { same = false; return; }
                    const BoundInstr tw = threaded_words(enc, f[(size_t)(i - i0)]);
                    BoundInstr &r = cw[h + (size_t)(i - i0)]; // (make_chained `put`: the operand words; the handler words stay)
                    r.bop = tw.arg;
                    if (f32) r.arg = tw.lo;
                    else { r.lo = tw.lo; r.hi = tw.hi; }
                }
            }
        });
    }
    if (same) {
        p->waves = W;
        // (the device keeps a variant in cbytes = (bcode + trees + 2) records: de_program_create)
        p->var_stride = (int64_t)(p->bcode.size() + (size_t)p->n_trees + 2);
    } else p->ccode_w.clear(); // (a fusion decided differently with shifted rows: never seen — rows are < 128 apart — but then one wave)
}
// Whether the program runs the threaded kernel at all (else: a flat-switch kernel, and `direct` says whether that one gathers X)
static bool wants_threaded(de_program *p) {
    // the LDS-staged kernels need (n_features + n_slots) rows of 4112 B; wider X uses the direct variant
    p->direct = (size_t)eval_rows(p) * FLAT_ROW_BYTES > 150 * 1024; // (the flat-switch kernel's geometry: 256 threads x 16 bytes per row; it gathers the features of a wider X from global memory)
    if (p->io == DE_F16) return false; // binary16 programs run de_half.hip's flat-switch kernel only
    if (is_complex_io(p->io)) { // complex programs: de_complex.hip's flat-switch kernel, whose rows are complex_row_bytes
        p->direct = (size_t)eval_rows(p) * complex_row_bytes(p->io) > 64 * 1024;
        return false;
    }
    // the threaded kernel's rows are a quarter of that (one wave's 64 vectors): it stages X up to ~140 rows — and shares them among the
    // waves of a wave group (round 6: F = 36 ... 120 ran the gathering flat-switch kernel, 14 - 20 ms per 10^6 samples x 1000 trees)
    // (a program the flat-switch kernel would gather for takes the threaded kernel while a group of FOUR waves fits: one wave per CU
    // would be no better than the gathers)
    if ((p->direct && ((size_t)eval_rows(p) + 3 * (size_t)p->n_slots) * trow_bytes(p->dtype) + 4 * 256 > 150 * 1024) || !eval_uses_threaded()) return false;
    return eval_rows(p) <= 4000; // row offsets must fit 24 bits
}
int make_threaded(de_ctx *c, de_program *p, const Reuse *ru) {
    p->threaded = false;
    p->waves = 1;
    p->var_stride = 0;
    p->ccode_w.clear();
    p->assured = p->assured_valid = false;
    p->assured_tiers = 0;
    p->aids.clear();
    p->aids2.clear();
    p->memo = MemoAssign{};
    assured_configure(p, ru ? ru->old : nullptr);
    dbg_lap(nullptr);
    if (!wants_threaded(p)) return DE_OK;
    uint64_t table[TOPX_TABLE];
    hipError_t st = eval_handler_table(p->dtype, (p->options & DE_OPT_TURBO) != 0, table);
    if (st != hipSuccess) return fail(c, DE_ERR_HIP, "handler table: %s", hipGetErrorString(st));
    dbg_lap("handler table");
    uint64_t base = table[0];
    for (int i = 0; i < (int)TOPX_TABLE; i++) base = std::min<uint64_t>(base, table[i]);
    for (int i = 0; i < (int)TOPX_TABLE; i++) {
        if (table[i] - base > 0xFFFFFFFFull) return DE_OK; // cannot encode: keep the switch kernel
        // Float64 records carry 32 bits of the next handler's address (the high half is the current pc's)
        if (p->dtype != DE_F32 && (table[i] >> 32) != (table[0] >> 32)) return DE_OK;
    }
    const uint32_t row_bytes = (uint32_t)trow_bytes(p->dtype);
    const ThreadedEnc enc{table, base, !getenv("DE_NO_CONST_UNARY_HOT"), row_bytes, (uint32_t)(p->n_features + p->n_slots) * row_bytes};
    // superinstructions (de_bind.h): fewer dispatches for the same arithmetic
    const char *nf = getenv("DE_NO_FUSE");
    const bool fuse = !(nf && *nf == '1');
    // wave groups: the waves per workgroup, and how far the last variant of the stream moves the slot rows — a fusion must fit all
    if (p->waves_choice == 0) p->waves_choice = choose_waves(p);
    const int W = fuse ? p->waves_choice : 1;
    const FuseRows rows0{(uint32_t)p->n_features, (uint32_t)(p->n_features + p->n_slots), 0, W > 1 ? (p->prows ? p->n_params : 0) + (W - 1) * p->n_slots : 0};
    // (de_program_update: a kept tree's fused code and wave-variant operand words are copied when the old program was threaded with the
    // same binding and the same wave count — fuse_tree reads the tree's bound code and those only)
    const de_program *old = ru && ru->old && ru->old->threaded && ru->old->waves_choice == p->waves_choice && same_binding(p, ru->old) ? ru->old : nullptr;
    build_stream_by_trees<BoundInstr>(p->n_trees, &p->fbcode, &p->tcode_off, [&](int64_t t, std::vector<BoundInstr> *out) {
        if (old && ru->kept(t)) {
            const size_t s = (size_t)ru->src[(size_t)t];
            out->insert(out->end(), old->fbcode.begin() + old->tcode_off[s], old->fbcode.begin() + old->tcode_off[s + 1]);
            return;
        }
        const int32_t b0 = p->bcode_off[(size_t)t], b1 = p->bcode_off[(size_t)t + 1];
        if (fuse) fuse_tree(p->bcode.data() + b0, (size_t)(b1 - b0), out, W > 1 && p->n_slots > 0 ? &rows0 : nullptr);
        else out->insert(out->end(), p->bcode.begin() + b0, p->bcode.begin() + b1);
    });
    dbg_lap("fuse_tree");
    p->tcode.resize(p->fbcode.size());
    parallel_tree_ranges(p->n_trees, [&](int, int64_t tb, int64_t te) {
        for (size_t i = (size_t)p->tcode_off[(size_t)tb]; i < (size_t)p->tcode_off[(size_t)te]; i++) p->tcode[i] = threaded_words(enc, p->fbcode[i]);
    });
    dbg_lap("threaded words");
    match_const_sites(p->folded ? p->fcode : p->code, p->folded ? p->fcode_off : p->code_off, p->fbcode, p->tcode_off, p->n_trees,
                      [](const BoundInstr &b) { return top_carries_const(b.bop); }, &p->tsite);
    p->site_gen++;
    dbg_lap("constant sites");
    p->handler_base = base;
    p->end_handler = table[TOPX_END];
    for (uint32_t k = 0; k < TOPX_ENDV_COUNT; k++) p->endv_handler[k] = table[TOPX_ENDV_BASE + k];
    make_chained(p);
    dbg_lap("chained records");
    p->threaded = true;
    if (W > 1 && p->n_slots > 0 && fuse) {
        make_wave_variants(p, enc, W, rows0, old, ru);
        dbg_lap("wave-group stream variants");
    } else if (W > 1 && fuse) p->waves = W; // no slot: one stream for every wave
    // the assured stream (de_api_internal.h `assured`): Float32 values, no parameters, exact operators, one-wave workgroups
    if (p->assured_cfg > 0 && p->waves == 1 && p->var_stride == 0 && p->io == DE_F32 && p->dtype == DE_F32 && !p->uses_params &&
        !(p->options & DE_OPT_TURBO) && p->n_trees >= 8 && p->allow_fold) { // (not the auxiliary programs of constant subtrees, not a handful of trees: the second stream would cost more than it saves)
        make_assured(p, table);
        dbg_lap("assured stream");
    }
    return DE_OK;
}

// The device layout of the threaded program (see de_kernels.hip): one head record, then per tree one record per instruction
// and an end record.  A record = {its operand word, its immediate, the address of the NEXT record's handler}: the head record
// names the first handler of tree 0, a tree's last instruction names h_tree_end (whose operand word is the tree's index), an
// end record names the first handler of the next tree — a chunk of consecutive trees is ONE chain and a handler knows where
// to jump before the record it has to fetch arrives.  BoundInstr fields by word: Float32 {bop: operand word, arg: imm, lo/hi:
// next handler}; Float64 {bop: operand word, arg: next handler (low half), lo/hi: imm}.
static void make_chained(de_program *p) {
    const bool f32 = p->dtype == DE_F32;
    p->ccode.assign(p->tcode.size() + (size_t)p->n_trees + 1, BoundInstr{0u, 0u, 0u, 0u});
    p->ccode_off.assign((size_t)p->n_trees + 1, 0);
    auto put = [&](BoundInstr &r, uint32_t la, uint32_t lo, uint32_t hi) { // operand words; the handler word is set by the predecessor
        r.bop = la;
        if (f32) r.arg = lo;
        else { r.lo = lo; r.hi = hi; }
    };
    auto name_next = [&](BoundInstr &r, uint64_t handler) {
        if (f32) { r.lo = (uint32_t)handler; r.hi = (uint32_t)(handler >> 32); }
        else r.arg = (uint32_t)handler;
    };
    // (the DE_NO_END_FUSE switch of round 2 measured <= 1 % and is gone)
    // a tree that finishes in a validity-tested hot operator runs that instruction and its end as ONE dispatch (h_chain_end);
    // a one-instruction tree keeps the plain form (the kernel's first call cannot tell the two apart)
    auto ev_of = [&](int64_t t) -> int {
        const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1];
        return i1 - i0 >= 2 ? topx_endv_of(p->fbcode[(size_t)i1 - 1].bop) : -1;
    };
    auto handler_of = [&](int32_t i, int32_t i1, int ev) -> uint64_t {
        return (i == i1 - 1 && ev >= 0) ? p->endv_handler[ev] : p->handler_base + p->tcode[(size_t)i].bop;
    };
    // Pass A, on the host threads: the records a tree OWNS — its instruction records and its end record (h = one end record per
    // preceding tree + the head record).  Pass B, serial (three writes per tree): what a tree writes into its PREDECESSOR's last two
    // records — the handler of its first instruction, and the header words over the end record's.
    parallel_tree_ranges(p->n_trees, [&](int, int64_t tb, int64_t te) {
        for (int64_t t = tb; t < te; t++) {
            const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1];
            const size_t h = (size_t)i0 + (size_t)t + 1;
            p->ccode_off[(size_t)t] = (int32_t)h;
            const int ev = ev_of(t);
            for (int32_t i = i0; i < i1; i++) {
                const BoundInstr &s = p->tcode[(size_t)i];
                put(p->ccode[h + (size_t)(i - i0)], s.arg, s.lo, s.hi);
                if (i > i0) name_next(p->ccode[h + (size_t)(i - i0) - 1], handler_of(i, i1, ev)); // in the record in front
            }
            put(p->ccode[h + (size_t)(i1 - i0)], (uint32_t)t, 0u, 0u); // end record (operand word: the tree's index, informational)
            if (i1 > i0) name_next(p->ccode[h + (size_t)(i1 - i0) - 1], p->end_handler);
        }
    });
    for (int64_t t = 0; t < p->n_trees; t++) {
        const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1];
        const size_t h = (size_t)p->ccode_off[(size_t)t];
        const int ev = ev_of(t);
        if (i1 > i0) {
            const uint64_t first = handler_of(i0, i1, ev);
            name_next(p->ccode[h - 1], first); // in the head record / the previous tree's end record
            // the previous tree finishes in an end-fused handler: ITS last instruction names this tree's first handler, stepping over its end record
            if (t > 0 && ev_of(t - 1) >= 0) name_next(p->ccode[h - 2], first);
        } else name_next(p->ccode[h - 1], p->end_handler);
        // the record in front of the tree (head record / previous tree's end record) is its HEADER: its immediate = the number of
        // instruction records of the tree, which is what h_tree_skip needs to step over a tree that is not evaluated
        // bit 31 = the tree finishes in an end-fused handler (its last instruction record names the next tree's first handler too):
        // what de_compact_live_kernel (de_kernels.hip) needs to re-link a tree behind another one
        put(p->ccode[h - 1], t == 0 ? 0u : (uint32_t)(t - 1), (uint32_t)(i1 - i0) | (ev >= 0 ? DE_HDR_FUSED_END : 0u), 0u);
    }
    if (p->n_trees > 0) name_next(p->ccode.back(), p->end_handler); // never followed: the last tree's end returns (left == 1)
    p->ccode_off[(size_t)p->n_trees] = (int32_t)p->ccode.size();
}
// The assured variant's handler words of trees [tb, te): the interval pass over the fused code (de_bind.h assure_tree; the constants as
// fbcode holds them NOW), then every instruction's handler — its twin's where a test is elided, its own otherwise — named where
// make_chained names it: in the record in front (the first instruction's: in the header record, and in the last instruction record of an
// end-fused predecessor).  A tree writes records no other tree writes: tree ranges may run on the host threads.
// tier 1: the wide fact, variant 1, aids; tier 2: the tight fact, variant 2, aids2 (de_api_internal.h assured_tiers).
void assure_program_tree(const de_program *p, int tier, int32_t i0, int32_t i1, AssuredInstr *info) {
    if (tier == 2) assure_tree_fact(p->fbcode.data() + i0, (size_t)(i1 - i0), p->n_features, p->assured_tight_xmax, p->assured_tight_amin, info, p->assured_parts);
    else assure_tree(p->fbcode.data() + i0, (size_t)(i1 - i0), p->n_features, p->assured_xmax, info, p->assured_parts);
}
void assured_link_trees(de_program *p, const uint64_t *table, int64_t tb, int64_t te, bool touched_only, int tier) {
    BoundInstr *cw = p->ccode_w.data() + (size_t)(tier - 1) * p->ccode.size();
    std::vector<uint32_t> &aids = tier == 2 ? p->aids2 : p->aids;
    std::vector<AssuredInstr> info;
    auto name_next = [](BoundInstr &r, uint64_t handler) { r.lo = (uint32_t)handler; r.hi = (uint32_t)(handler >> 32); }; // (Float32 records)
    auto ev_of = [&](int64_t t) -> int {
        const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1];
        return i1 - i0 >= 2 ? topx_endv_of(p->fbcode[(size_t)i1 - 1].bop) : -1;
    };
    for (int64_t t = tb; t < te; t++) {
        const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1];
        if (i1 <= i0) continue;
        if (touched_only && p->const_off[(size_t)t + 1] == p->const_off[(size_t)t]) continue; // (a set of the constants touches the trees that have some)
        info.resize((size_t)(i1 - i0));
        assure_program_tree(p, tier, i0, i1, info.data());
        const size_t h = (size_t)p->ccode_off[(size_t)t];
        const int ev = ev_of(t);
        for (int32_t i = i0; i < i1; i++) {
            const uint32_t id = info[(size_t)(i - i0)].id;
            aids[(size_t)i] = id;
            // (an end-fused last instruction: the end-fused twin of its assured id, or the end-fused handler of the guarded stream)
            const uint64_t handler = (i == i1 - 1 && ev >= 0) ? (topx_enda_of(id) >= 0 && id != p->fbcode[(size_t)i].bop ? table[TOPX_ENDA_BASE + (uint32_t)topx_enda_of(id)] : p->endv_handler[ev])
                                     : id == p->fbcode[(size_t)i].bop ? p->handler_base + p->tcode[(size_t)i].bop : table[id];
            if (i > i0) name_next(cw[h + (size_t)(i - i0) - 1], handler);
            else {
                name_next(cw[h - 1], handler);
                if (t > 0 && ev_of(t - 1) >= 0) name_next(cw[h - 2], handler);
            }
        }
    }
}
// ccode_w = the guarded stream with the assured handler words; var_stride as a wave group's variants lie (de_program_create sizes the arena by it)
static void make_assured(de_program *p, const uint64_t *table) {
    const bool tight = p->assured_tiers_room ? p->assured_tiers_room >= 2
                                             : p->assured_tiers_cfg >= 2 && (p->assured_tight_xmax < p->assured_xmax || p->assured_tight_amin > assured_wide_amin(p->assured_parts));
    p->ccode_w = p->ccode;
    if (tight) p->ccode_w.insert(p->ccode_w.end(), p->ccode.begin(), p->ccode.end()); // variant 2: the tight tier
    p->aids.assign(p->fbcode.size(), 0u);
    p->aids2.assign(tight ? p->fbcode.size() : 0, 0u);
    parallel_tree_ranges(p->n_trees, [&](int, int64_t tb, int64_t te) {
        assured_link_trees(p, table, tb, te);
        if (tight) assured_link_trees(p, table, tb, te, false, 2);
    });
    // (a tight pass that names no id the wide pass does not name: one tier — no third variant to keep, upload and re-link)
    if (tight && !p->assured_tiers_room && p->aids2 == p->aids) {
        p->ccode_w.resize(p->ccode.size());
        p->aids2.clear();
    }
    p->assured_tiers = p->aids2.empty() ? 1 : 2;
    p->var_stride = (int64_t)(p->bcode.size() + (size_t)p->n_trees + 2);
    p->assured = p->assured_valid = true;
    program_memo_assign(p, &p->memo);
}
// the program's memo rows (de_api_internal.h `memo`): counted over the tightest tier, the stream nearly every tile of bounded data runs
void program_memo_assign(const de_program *p, MemoAssign *out) {
    const std::vector<uint32_t> &ids = p->aids2.empty() ? p->aids : p->aids2;
    *out = MemoAssign{};
    if (!p->assured || ids.size() != p->fbcode.size() || ids.empty()) return;
    *out = memo_assign(ids.data(), 1, &p->fbcode[0].arg, sizeof(BoundInstr) / sizeof(uint32_t), ids.size(), p->n_features, eval_memo_rows());
}
// the stream variants of waves 1 .. (wave groups) to their places behind variant 0
hipError_t upload_wave_variants(de_program *p) {
    for (size_t w = 0; p->var_stride && w * p->ccode.size() < p->ccode_w.size(); w++) {
        const hipError_t st = hipMemcpy(p->d_code + (w + 1) * (size_t)p->var_stride, p->ccode_w.data() + w * p->ccode.size(),
                                        p->ccode.size() * sizeof(BoundInstr), hipMemcpyHostToDevice);
        if (st != hipSuccess) return st;
    }
    return hipSuccess;
}
} // extern "C"
