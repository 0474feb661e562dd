// de_api_program_inspect.cpp — what looks at a program without changing what it computes: de_eval_plan, the test hooks
// de_program_stream_hash / de_program_verify / de_program_dump, and the host-only lowering hooks de_lower_tape*.
#include "de_api_program.h"

extern "C" {
int de_eval_plan(const de_program_t *p, int64_t N, int32_t *plan) {
    if (!p || !plan || N < 0) return DE_ERR_INVALID_ARG;
    eval_plan(p->io, p->n_trees, N, &plan[0], &plan[1], &plan[2], p->threaded ? p->waves : 1);
    return DE_OK;
}

// Test hook: one 64-bit FNV-1a hash over every host-side stream, table and flag de_program_create built (lengths included), and over the
// auxiliary program of constant subtrees — equal for every DE_HOST_THREADS and for a de_program_update against a fresh creation.  The
// gradient streams (gbcode, gtcode, rtcode) are made lazily by the gradient entry points and are not part of it.
uint64_t de_program_stream_hash(const de_program_t *p) {
    if (!p) return 0;
    if (consts_materialise(const_cast<de_program_t *>(p)) != DE_OK) return 0; // (host streams behind a device set: §3.5)
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *data, size_t bytes) {
        const unsigned char *b = static_cast<const unsigned char *>(data);
        for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 1099511628211ull; }
        const uint64_t n = bytes; // (the length too: an empty vector and a missing one differ from a shifted boundary)
        for (int i = 0; i < 8; i++) { h ^= (n >> (8 * i)) & 0xFF; h *= 1099511628211ull; }
    };
    auto vec = [&](const auto &v) { mix(v.data(), v.size() * sizeof(v[0])); };
    vec(p->code); vec(p->code_off); vec(p->fcode); vec(p->fcode_off); vec(p->bcode); vec(p->bcode_off);
    vec(p->fbcode); vec(p->tcode); vec(p->tcode_off); vec(p->ccode); vec(p->ccode_off); vec(p->bsite); vec(p->tsite);
    vec(p->consts); vec(p->const_off); vec(p->const_instr); vec(p->fconst_instr); vec(p->const_checks); vec(p->n_consts_tree);
    vec(p->consts_im); vec(p->ctab); // (complex programs: the imaginary parts and the constant table)
    vec(p->aux_const_src); vec(p->host_ok_eval); vec(p->host_ok_grad); vec(p->fold_ok);
    vec(p->fold_host); vec(p->fold_noff); vec(p->fold_coff); vec(p->aux_fold); vec(p->aux_csrc); vec(p->kfold); vec(p->kf_csrc);
    mix(p->fold_nodes.data(), p->fold_nodes.size() * sizeof(de_tape_node_t));
    for (const auto &f : p->folds) { const int32_t w[3] = {f.tree, f.instr, f.tested_always ? 1 : 0}; mix(w, sizeof w); }
    const int64_t scal[6] = {p->n_trees, p->n_nodes, p->n_slots, p->uses_params ? 1 : 0, p->folded ? 1 : 0, p->threaded ? 1 : 0};
    mix(scal, sizeof scal);
    if (!p->ccode_w.empty()) mix(p->ccode_w.data(), p->ccode_w.size() * sizeof(BoundInstr)); // the stream variants of a wave group
    if (p->aux) { const uint64_t a = de_program_stream_hash(p->aux); mix(&a, sizeof a); }
    return h;
}

static int verify_bad(const de_program *p, const char *what, int64_t tree, int64_t i, uint64_t v) {
    return fail(p->ctx, DE_ERR_BAD_TAPE, "program verify: %s (tree %lld, instruction %lld, value 0x%llx)", what, (long long)tree, (long long)i,
                (unsigned long long)v);
}
// the generic code, plain and folded: opcodes, operand rows, push / pop slots
static int verify_generic(const de_program *p) {
    const int64_t rows = eval_rows(p);
    const std::vector<Instr> *gens[2] = {&p->code, p->folded ? &p->fcode : nullptr};
    const std::vector<int32_t> *goffs[2] = {&p->code_off, p->folded ? &p->fcode_off : nullptr};
    for (int g = 0; g < 2; g++) {
        if (!gens[g]) continue;
        const auto &code = *gens[g];
        const auto &off = *goffs[g];
        if ((int64_t)off.size() != p->n_trees + 1 || off[0] != 0 || off.back() != (int32_t)code.size()) return verify_bad(p, "generic offsets", -1, g, off.size());
        for (int64_t t = 0; t < p->n_trees; t++) {
            if (off[(size_t)t + 1] <= off[(size_t)t]) return verify_bad(p, "empty tree", t, 0, 0);
            for (int32_t i = off[(size_t)t]; i < off[(size_t)t + 1]; i++) {
                const Instr &ins = code[(size_t)i];
                const uint32_t op = ins.hdr & H_OP_MASK, src = (ins.hdr >> H_SRC_SHIFT) & H_SRC_MASK;
                const bool known = op == DOP_LOAD || (op >= DE_U_NEG && op < DE_U_LAST_) || (op >= DE_B_ADD && op < DE_B_LAST_) ||
                                   (op >= DE_T_FMA && op < DE_T_LAST_) || (op >= DOP_RSUB && op <= DOP_RPOW_ABS2);
                if (!known) return verify_bad(p, "unknown opcode", t, i, op);
                if (src == SRC_ROW && (int64_t)(ins.feat & 0xFFFFu) >= rows) return verify_bad(p, "operand row outside X + spill slots", t, i, ins.feat);
                if (src == SRC_PARAM && (int64_t)(ins.feat & 0xFFFFu) >= p->n_params) return verify_bad(p, "parameter row out of range", t, i, ins.feat);
                if (src != SRC_ACC && src != SRC_ROW && src != SRC_CONST && src != SRC_PARAM) return verify_bad(p, "operand kind", t, i, src);
                if ((ins.hdr & H_PUSH) && (int)((ins.hdr >> H_PUSH_SHIFT) & H_SLOT_MASK) >= p->n_slots) return verify_bad(p, "push slot", t, i, ins.hdr);
                if (op >= DE_T_FMA && op < DE_T_LAST_ && (int)((ins.hdr >> H_POPC_SHIFT) & H_SLOT_MASK) >= p->n_slots) return verify_bad(p, "ternary slot", t, i, ins.hdr);
            }
        }
    }
    return DE_OK;
}
// the bound code: handler ids, operand rows; a complex program's table indices and opcodes
static int verify_bound(const de_program *p) {
    const int64_t rows = eval_rows(p);
    for (size_t i = 0; i < p->bcode.size(); i++) {
        const BoundInstr &b = p->bcode[i];
        if (b.bop >= BOP_COUNT) return verify_bad(p, "bound handler id", -1, (int64_t)i, b.bop);
        if (!bop_is_const_source(b.bop) && b.bop != BOP_GEN_PARAM && b.bop != BOP_LOAD_CONST && b.bop != BOP_CHECK_ACC && b.bop != BOP_GEN_ACC &&
            b.bop != BOP_INJ_ACC && !(b.bop >= BOP_UN_BASE && b.bop < BOP_UN_END && !((b.bop - BOP_UN_BASE) & 2)) &&
            (int64_t)(b.arg & 0xFFFFFFu) >= rows)
            return verify_bad(p, "bound operand row", -1, (int64_t)i, b.arg);
    }
    if (is_complex_io(p->io)) { // every constant operand of a complex program indexes the constant table
        const size_t n_entries = p->ctab.size() / 2;
        for (size_t i = 0; i < p->bcode.size(); i++)
            if (bop_is_const_source(p->bcode[i].bop) && p->bcode[i].lo >= n_entries) return verify_bad(p, "constant-table index", -1, (int64_t)i, p->bcode[i].lo);
        for (size_t i = 0; i < p->bcode.size(); i++) {
            const uint32_t bop = p->bcode[i].bop, op = p->bcode[i].arg >> 24;
            const bool gen = bop == BOP_GEN_ROW || bop == BOP_GEN_CONST || bop == BOP_GEN_ACC || bop == BOP_INJ_ACC || bop == BOP_INJ_ROW || bop == BOP_TERN;
            if (bop == BOP_GEN_PARAM) return verify_bad(p, "parameter operand in a complex program", -1, (int64_t)i, bop);
            if (gen && op != DOP_RSUB && op != DOP_RDIV && !complex_opcode_ok(op >= DE_T_FMA ? 3 : op >= DE_B_ADD ? 2 : 1, (int)op))
                return verify_bad(p, "opcode without a complex kernel", -1, (int64_t)i, op);
        }
    }
    return DE_OK;
}
// the chained stream the threaded kernel executes, against the fused and threaded code it was made from
static int verify_chained(const de_program *p, const uint64_t *table) {
    const int64_t rows = eval_rows(p), spill_end = (int64_t)p->n_features + p->n_slots;
    std::vector<uint64_t> valid(table, table + TOPX_TABLE); // (the end-fused variants included)
    std::sort(valid.begin(), valid.end());
    const uint64_t lds_bytes = (uint64_t)(rows + (p->uses_params ? 2 : 0)) * trow_bytes(p->dtype);
    if ((int64_t)p->ccode_off.size() != p->n_trees + 1 || p->ccode.size() != p->tcode.size() + (size_t)p->n_trees + 1) return verify_bad(p, "chained layout", -1, 0, p->ccode.size());
    const bool f32 = p->dtype == DE_F32;
    for (int64_t t = 0; t < p->n_trees; t++) {
        const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1], h = p->ccode_off[(size_t)t];
        if (h != i0 + (int32_t)t + 1) return verify_bad(p, "chained offset", t, h, (uint64_t)i0);
        if (i1 > i0) { // a tree never starts by reading the accumulator: the end of the previous tree leaves it as it is
            const BoundInstr &f0 = p->fbcode[(size_t)i0];
            const uint32_t aux0 = f0.arg >> 24;
            const int deg0 = aux0 == (uint32_t)DOP_LOAD ? 0 : de_opcode_degree((int)aux0);
            if (top_reads_acc(f0.bop, deg0)) return verify_bad(p, "first instruction of a tree reads the accumulator", t, 0, f0.bop);
        }
        { // the header record (in front of the tree) carries the tree's record count: h_tree_skip steps over the tree with it
            const BoundInstr &hd = p->ccode[(size_t)h - 1];
            if (((f32 ? hd.arg : hd.lo) & ~DE_HDR_FUSED_END) != (uint32_t)(i1 - i0)) return verify_bad(p, "tree header does not carry the tree's length", t, 0, f32 ? hd.arg : hd.lo);
        }
        for (int32_t i = i0; i <= i1; i++) {
            const BoundInstr &r = p->ccode[(size_t)(h + (i - i0))];
            const BoundInstr &q = p->ccode[(size_t)(h + (i - i0) - 1)]; // a record's handler is named by the record in front of it
            const uint64_t addr = f32 ? (((uint64_t)q.hi << 32) | q.lo) : ((table[0] & 0xFFFFFFFF00000000ull) | q.arg);
            if (!std::binary_search(valid.begin(), valid.end(), addr)) return verify_bad(p, "handler address not in the device table", t, i - i0, addr);
            // an end-fused last instruction (h_chain_end) steps over the end record: its own record names what the end record names
            const int ev = i1 - i0 >= 2 ? topx_endv_of(p->fbcode[(size_t)i1 - 1].bop) : -1;
            const uint64_t last_plain = p->handler_base + p->tcode[(size_t)i1 - 1].bop;
            const BoundInstr &lastq = p->ccode[(size_t)(h + (i1 - 1 - i0) - 1)];
            const uint64_t last_addr = f32 ? (((uint64_t)lastq.hi << 32) | lastq.lo) : ((table[0] & 0xFFFFFFFF00000000ull) | lastq.arg);
            const bool fused_end = ev >= 0 && last_addr == p->endv_handler[ev] && last_addr != last_plain;
            if (i == i0 && (((f32 ? p->ccode[(size_t)h - 1].arg : p->ccode[(size_t)h - 1].lo) & DE_HDR_FUSED_END) != 0) != fused_end)
                return verify_bad(p, "tree header's end-fused bit", t, 0, (uint64_t)fused_end);
            if (i == i1) {
                const BoundInstr &e = p->ccode[(size_t)(h + (i1 - i0))]; // the end record itself names the next tree's first handler
                const uint64_t after = f32 ? (((uint64_t)e.hi << 32) | e.lo) : ((table[0] & 0xFFFFFFFF00000000ull) | e.arg);
                if (fused_end ? addr != after : addr != p->end_handler) return verify_bad(p, "tree does not end in the end record", t, i - i0, addr);
                if (r.bop != (uint32_t)t) return verify_bad(p, "end record does not name its tree", t, i - i0, r.bop);
                continue;
            }
            const BoundInstr &fb = p->fbcode[(size_t)i];
            if (i == i1 - 1 ? (addr != last_plain && !fused_end) : addr != p->handler_base + p->tcode[(size_t)i].bop)
                return verify_bad(p, "record / threaded code mismatch", t, i - i0, addr);
            if (fb.bop >= TOPX_COUNT) return verify_bad(p, "fused handler id", t, i - i0, fb.bop);
            const bool no_row = top_is_const_source(fb.bop) || fb.bop == BOP_CHECK_ACC || fb.bop == BOP_GEN_ACC || fb.bop == BOP_INJ_ACC ||
                                fb.bop == BOP_GEN_PARAM || (fb.bop >= BOP_UN_BASE && fb.bop < BOP_UN_END && !((fb.bop - BOP_UN_BASE) & 2)) ||
                                (fb.bop >= TOPX_UN_BASE && fb.bop < TOPX_BIN_BASE && ((fb.bop - TOPX_UN_BASE) & 1)) ||
                                (fb.bop >= TOPX_BIN_BASE && ((fb.bop - TOPX_BIN_BASE) & 1));
            if (!no_row) {
                const uint64_t off = r.bop & 0xFFFFFFu;
                if (off % trow_bytes(p->dtype) != 0 || off + trow_bytes(p->dtype) > lds_bytes) return verify_bad(p, "LDS operand offset outside the launch's allocation", t, i - i0, r.bop);
                const bool pushes = (fb.bop >= TOP_LOADROW_BASE && fb.bop < TOP_LOADCONST_PUSH && ((fb.bop - TOP_LOADROW_BASE) & 2)) ||
                                    (fb.bop >= TOP_UNROW_BASE && fb.bop < TOP_BINROWC_BASE && ((fb.bop - TOP_UNROW_BASE) & 2)) ||
                                    (fb.bop >= TOP_BIN2_BASE && fb.bop < TOP_COUNT && ((fb.bop - TOP_BIN2_BASE) & 1));
                if (pushes) {
                    const int64_t prow = (int64_t)(off / trow_bytes(p->dtype)) + (int8_t)(r.bop >> 24);
                    if (prow < p->n_features || prow >= spill_end) return verify_bad(p, "push row of a superinstruction outside the spill slots", t, i - i0, r.bop);
                }
                if (fb.bop >= TOP_BIN2_BASE && fb.bop < TOP_COUNT && !(((fb.bop - TOP_BIN2_BASE) >> 2) & 1)) { // row-row: second row by distance
                    const int64_t second = (int64_t)off + (int32_t)(f32 ? r.arg : r.lo);
                    if (second < 0 || second % (int64_t)trow_bytes(p->dtype) != 0 || (uint64_t)second + trow_bytes(p->dtype) > lds_bytes) return verify_bad(p, "second operand row of a two-operand form", t, i - i0, (uint64_t)second);
                }
            }
            if (fb.bop == BOP_GEN_PARAM && (f32 ? r.arg : r.lo) != (uint32_t)rows * (uint32_t)trow_bytes(p->dtype)) return verify_bad(p, "class-row offset of a parameter operand", t, i - i0, r.arg);
        }
    }
    return DE_OK;
}
static int verify_wave_variants(const de_program *p) {
    const int64_t rows = eval_rows(p), spill_end = (int64_t)p->n_features + p->n_slots;
    const bool f32 = p->dtype == DE_F32;
    // wave groups: variant w of the stream = variant 0 but for the slot rows, which lie `shift` rows further on (behind the staged
    // parameter rows and the slots of the waves before): same handler words, every operand row inside the group's allocation, a row
    // of variant 0's slot area moved by exactly the shift and every other row left where it is
    if (p->waves > 1 && p->ccode_w.size() != (p->var_stride ? p->ccode.size() * (size_t)(p->waves - 1) : 0)) return verify_bad(p, "stream variants of the wave group", -1, p->waves, p->ccode_w.size());
    const uint64_t rb = trow_bytes(p->dtype);
    for (size_t w = 1; p->var_stride && w < (size_t)p->waves; w++) {
        const BoundInstr *cw = p->ccode_w.data() + (w - 1) * p->ccode.size();
        const int64_t shift = (p->prows ? p->n_params : 0) + (int64_t)w * p->n_slots, rows_all = rows + (int64_t)(p->waves - 1) * p->n_slots;
        auto moved = [&](int64_t row0, int64_t roww) { return roww == (row0 >= p->n_features && row0 < spill_end ? row0 + shift : row0) && roww < rows_all; };
        for (int64_t t = 0; t < p->n_trees; t++) {
            const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1], h = p->ccode_off[(size_t)t];
            for (int32_t i = i0 - 1; i <= i1; i++) { // the header in front, the instructions, the end record
                const BoundInstr &r0 = p->ccode[(size_t)(h + (i - i0))], &r = cw[(size_t)(h + (i - i0))];
                const bool same_next = f32 ? (r.lo == r0.lo && r.hi == r0.hi) : r.arg == r0.arg;
                if (!same_next) return verify_bad(p, "stream variant names another handler", t, i - i0, w);
                if (i < i0 || i == i1) { if (std::memcmp(&r, &r0, sizeof r)) return verify_bad(p, "stream variant: header / end record differs", t, i - i0, w); continue; }
                const BoundInstr &fb = p->fbcode[(size_t)i];
                if (fb.bop == BOP_GEN_PARAM) { if (std::memcmp(&r, &r0, sizeof r)) return verify_bad(p, "stream variant: a gathered-parameter record differs", t, i - i0, w); continue; }
                // the operand word: a row offset (a slot row moves by the shift, any other row stays; a record without an LDS operand
                // carries row 0 or no row offset at all: unchanged) | aux << 24
                const uint64_t off0 = r0.bop & 0xFFFFFFu, off = r.bop & 0xFFFFFFu;
                if (off0 % rb != 0 || off % rb != 0) { if (off != off0) return verify_bad(p, "stream variant: operand word", t, i - i0, r.bop); }
                else if (!moved((int64_t)(off0 / rb), (int64_t)(off / rb))) return verify_bad(p, "stream variant: operand row", t, i - i0, r.bop);
                const bool pushes = (fb.bop >= TOP_LOADROW_BASE && fb.bop < TOP_LOADCONST_PUSH && ((fb.bop - TOP_LOADROW_BASE) & 2)) ||
                                    (fb.bop >= TOP_UNROW_BASE && fb.bop < TOP_BINROWC_BASE && ((fb.bop - TOP_UNROW_BASE) & 2)) ||
                                    (fb.bop >= TOP_BIN2_BASE && fb.bop < TOP_COUNT && ((fb.bop - TOP_BIN2_BASE) & 1));
                if (pushes ? !moved((int64_t)(off0 / rb) + (int8_t)(r0.bop >> 24), (int64_t)(off / rb) + (int8_t)(r.bop >> 24)) : (r.bop >> 24) != (r0.bop >> 24))
                    return verify_bad(p, "stream variant: push row / aux byte", t, i - i0, r.bop);
                const bool row_row = fb.bop >= TOP_BIN2_BASE && fb.bop < TOP_COUNT && !(((fb.bop - TOP_BIN2_BASE) >> 2) & 1);
                if (row_row || fb.bop == BOP_TERN) { // the immediate = byte distance to the second / third operand row
                    const int64_t s0 = (int64_t)off0 + (int32_t)(f32 ? r0.arg : r0.lo), s1 = (int64_t)off + (int32_t)(f32 ? r.arg : r.lo);
                    if (s1 < 0 || s1 % (int64_t)rb != 0 || !moved(s0 / (int64_t)rb, s1 / (int64_t)rb)) return verify_bad(p, "stream variant: second operand row", t, i - i0, (uint64_t)s1);
                } else if (f32 ? r.arg != r0.arg : (r.lo != r0.lo || r.hi != r0.hi))
                    return verify_bad(p, "stream variant: immediate differs", t, i - i0, w);
            }
        }
    }
    return DE_OK;
}
// the assured stream: the guarded stream in everything but handler words, and every handler word the one the interval pass over
// the present fused code (its constants) picks — the instruction's own handler or its untested twin's
static int verify_assured(const de_program *p, const uint64_t *table) {
    const bool f32 = p->dtype == DE_F32;
    const size_t tiers = (size_t)p->assured_tiers;
    if (p->waves != 1 || !f32 || tiers < 1 || tiers > 2 || p->ccode_w.size() != tiers * p->ccode.size() || p->aids.size() != p->fbcode.size() ||
        p->aids2.size() != (tiers == 2 ? p->fbcode.size() : 0) || (size_t)p->var_stride < p->ccode.size())
        return verify_bad(p, "assured stream layout", -1, p->waves, p->ccode_w.size());
    for (size_t tier = 1; tier <= tiers; tier++) { // (tier 2: the tight fact's pass, variant 2 — de_api_internal.h assured_tiers)
        const BoundInstr *cw = p->ccode_w.data() + (tier - 1) * p->ccode.size();
        const std::vector<uint32_t> &aids = tier == 2 ? p->aids2 : p->aids;
        std::vector<AssuredInstr> info;
        auto named = [](const BoundInstr &q) { return ((uint64_t)q.hi << 32) | q.lo; };
        for (size_t r = 0; r < p->ccode.size(); r++)
            if (cw[r].bop != p->ccode[r].bop || cw[r].arg != p->ccode[r].arg) return verify_bad(p, "assured stream: operand words differ", -1, (int64_t)r, cw[r].bop);
        for (int64_t t = 0; t < p->n_trees; t++) {
            const int32_t i0 = p->tcode_off[(size_t)t], i1 = p->tcode_off[(size_t)t + 1], h = p->ccode_off[(size_t)t];
            if (i1 <= i0) continue;
            info.resize((size_t)(i1 - i0));
            assure_program_tree(p, (int)tier, i0, i1, info.data());
            const int ev = i1 - i0 >= 2 ? topx_endv_of(p->fbcode[(size_t)i1 - 1].bop) : -1;
            for (int32_t i = i0; i < i1; i++) {
                const uint32_t id = info[(size_t)(i - i0)].id;
                if (p->assured_valid && id != aids[(size_t)i]) return verify_bad(p, "assured stream: stale twin id", t, i - i0, aids[(size_t)i]);
                const uint32_t have = aids[(size_t)i];
                if (have >= TOPX_COUNT) return verify_bad(p, "assured stream: handler id", t, i - i0, have);
                if (tier == 2 && have != p->aids[(size_t)i] && p->aids[(size_t)i] != p->fbcode[(size_t)i].bop && have == p->fbcode[(size_t)i].bop)
                    return verify_bad(p, "assured stream: the tight tier tests what the wide tier elides", t, i - i0, have);
                const uint64_t want = (i == i1 - 1 && ev >= 0) ? (topx_enda_of(have) >= 0 && have != p->fbcode[(size_t)i].bop ? table[TOPX_ENDA_BASE + (uint32_t)topx_enda_of(have)] : p->endv_handler[ev])
                                      : (have == p->fbcode[(size_t)i].bop ? p->handler_base + p->tcode[(size_t)i].bop : table[have]);
                if (named(cw[(size_t)(h + (i - i0) - 1)]) != want) return verify_bad(p, "assured stream: handler word", t, i - i0, named(cw[(size_t)(h + (i - i0) - 1)]));
            }
            // the end record is named as in the guarded stream (by the last instruction, or stepped over by an end-fused one)
            if (ev < 0 && named(cw[(size_t)(h + (i1 - i0) - 1)]) != p->end_handler) return verify_bad(p, "assured stream: tree does not end in the end record", t, i1 - i0, 0);
            if (ev >= 0 && named(cw[(size_t)(h + (i1 - i0) - 1)]) != named(cw[(size_t)(h + (i1 - i0))])) return verify_bad(p, "assured stream: end-fused instruction and end record disagree", t, i1 - i0, 0);
        }
    }
    // the memo rows: what the count over the present ids gives, every row a FEATURE row (a slot row differs from tree to tree), no pair twice
    MemoAssign want;
    program_memo_assign(p, &want);
    if (p->memo.n < 0 || p->memo.n > eval_memo_rows() || (p->assured_valid && p->memo.n != want.n)) return verify_bad(p, "memo rows: count", -1, p->memo.n, (uint64_t)want.n);
    for (int r = 0; r < p->memo.n; r++) {
        if (p->memo.k[r] < 0 || p->memo.k[r] > 1 || p->memo.feat[r] < 0 || p->memo.feat[r] >= p->n_features) return verify_bad(p, "memo rows: not a feature row", -1, r, (uint64_t)p->memo.feat[r]);
        for (int q = 0; q < r; q++)
            if (p->memo.k[q] == p->memo.k[r] && p->memo.feat[q] == p->memo.feat[r]) return verify_bad(p, "memo rows: a pair assigned twice", -1, r, (uint64_t)q);
        if (p->assured_valid && (p->memo.k[r] != want.k[r] || p->memo.feat[r] != want.feat[r] || p->memo.uses[r] != want.uses[r]))
            return verify_bad(p, "memo rows: stale assignment", -1, r, (uint64_t)want.feat[r]);
    }
    for (int k = 0; k < 2; k++) for (int ps = 0; ps < 2; ps++) for (int r = 0; r < DE_MEMO_MAX; r++) // (a row the build lacks keeps the handler it would stand in for)
        if ((r < eval_memo_rows()) == (table[topx_memo(k, ps != 0, r)] == table[topa_unrow_plain(k, ps != 0)])) return verify_bad(p, "memo rows: handler table", -1, r, table[topx_memo(k, ps != 0, r)]);
    return DE_OK;
}
// Program sanitizer (SURVEY.md §5 "sanitizer / bounds-checked debug"): the kernels trust the instruction streams —
// an LDS offset, a spill slot, a handler address are used as they come.  This walks every stream of the program on the
// host and checks each field against the bounds the launch will allocate: generic code (opcodes, operand rows <
// n_features + n_slots, push / pop slots, constant slots), bound and fused code (handler ids, rows, the int8 push
// distance of the superinstructions), and the chained stream the threaded kernel executes (every handler address is an
// entry of the device handler table, LDS byte offsets lie inside the launch's allocation, every tree ends in the end
// record).  DE_VERIFY=1 runs it after every de_program_create / de_program_set_consts.
int de_program_verify(const de_program_t *p) {
    if (!p) return DE_ERR_INVALID_ARG;
    if (const int mrc = consts_materialise(const_cast<de_program_t *>(p))) return mrc; // (host streams behind a device set: §3.5)
    de_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device)); // the handler tables are cached per device: the program's addresses are its OWN device's
    if (const int rc = verify_generic(p)) return rc;
    if (const int rc = verify_bound(p)) return rc;
    if (!p->threaded) return DE_OK;
    uint64_t table[TOPX_TABLE];
    if (eval_handler_table(p->dtype, (p->options & DE_OPT_TURBO) != 0, table) != hipSuccess) return fail(c, DE_ERR_HIP, "handler table");
    if (const int rc = verify_chained(p, table)) return rc;
    if (const int rc = verify_wave_variants(p)) return rc;
    return p->assured ? verify_assured(p, table) : DE_OK;
}

int64_t de_program_dump(const de_program_t *p, int64_t tree, uint32_t *words, int64_t cap, int which) {
    if (!p || tree < 0 || tree >= p->n_trees) return -DE_ERR_INVALID_ARG;
    const bool assured_valid = p->assured && p->assured_valid; // (as the launches see it NOW: materialising the constants below re-runs the pass)
    if (const int mrc = consts_materialise(const_cast<de_program_t *>(p))) return -mrc; // (host streams behind a device set: §3.5)
    if (which == 1) { // metadata: n_slots, host_ok_eval, host_ok_grad, uses_params
        if (cap < 4) return -DE_ERR_INVALID_ARG;
        words[0] = (uint32_t)p->n_slots;
        words[1] = p->host_ok_eval[(size_t)tree];
        words[2] = p->host_ok_grad[(size_t)tree];
        words[3] = p->uses_params;
        if (cap < 5) return 4;
        words[4] = (uint32_t)(p->threaded ? p->waves : 1); // waves per workgroup of the eval kernel (wave groups: 2 / 4 / 8)
        if (cap < 7) return 5;
        words[5] = p->threaded && p->assured ? 1u : 0u; // the program has an assured stream ...
        words[6] = p->threaded && assured_valid ? 1u : 0u; // ... and the launches use it (0 behind de_program_set_consts_device)
        if (cap < 8) return 7;
        words[7] = p->threaded && p->assured ? (uint32_t)p->assured_tiers : 0u; // the assured tiers the program has (0, 1, 2)
        return 8;
    }
    if (which == 4 || which == 5) { // the fused form with the handler ids of the ASSURED stream (5: of its tight tier); empty when the program has none
        if (!p->threaded || !p->assured || (which == 5 && p->assured_tiers < 2)) return 0;
        const std::vector<uint32_t> &aids = which == 5 ? p->aids2 : p->aids;
        const int32_t b0 = p->tcode_off[(size_t)tree], b1 = p->tcode_off[(size_t)tree + 1];
        const int64_t nb = (int64_t)(b1 - b0) * 4;
        if (!words || cap < nb) return nb;
        std::memcpy(words, p->fbcode.data() + b0, (size_t)nb * 4);
        for (int32_t i = b0; i < b1; i++) words[(size_t)(i - b0) * 4] = aids[(size_t)i];
        return nb;
    }
    if (which == 2) { // bound instructions (de_bind.h)
        const int32_t b0 = p->bcode_off[(size_t)tree], b1 = p->bcode_off[(size_t)tree + 1];
        const int64_t nb = (int64_t)(b1 - b0) * 4;
        if (!words || cap < nb) return nb;
        std::memcpy(words, p->bcode.data() + b0, (size_t)nb * 4);
        return nb;
    }
    if (which == 3) { // fused (superinstruction) form of the threaded kernel; empty when that kernel is not in use
        if (!p->threaded) return 0;
        const int32_t b0 = p->tcode_off[(size_t)tree], b1 = p->tcode_off[(size_t)tree + 1];
        const int64_t nb = (int64_t)(b1 - b0) * 4;
        if (!words || cap < nb) return nb;
        std::memcpy(words, p->fbcode.data() + b0, (size_t)nb * 4);
        return nb;
    }
    const int32_t i0 = p->code_off[(size_t)tree], i1 = p->code_off[(size_t)tree + 1];
    const int64_t nw = (int64_t)(i1 - i0) * 4;
    if (!words || cap < nw) return nw;
    std::memcpy(words, p->code.data() + i0, (size_t)nw * 4);
    return nw;
}

// The host lowering hooks: de_lower_tape / de_lower_tape_stage take the real dtypes (DE_F32, DE_F64, DE_F16) — their dtype domain
// is pinned as it was before complex programs existed —, de_lower_tape_complex / de_lower_tape_stage_complex the complex ones; one body.
static int64_t lower_tape_impl(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                               int32_t n_features, int32_t n_params, uint32_t options, uint32_t *words, int64_t cap, int32_t *meta);
static int64_t lower_tape_stage_impl(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                                     int32_t n_features, int32_t n_params, uint32_t options, int stage, uint32_t *words, int64_t cap);
int64_t de_lower_tape(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts,
                      int64_t n_consts, int32_t n_features, int32_t n_params, uint32_t options, uint32_t *words,
                      int64_t cap, int32_t *meta) {
    if (is_complex_io(dtype)) return -DE_ERR_INVALID_ARG;
    return lower_tape_impl(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, words, cap, meta);
}
int64_t de_lower_tape_complex(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts,
                              int64_t n_consts, int32_t n_features, int32_t n_params, uint32_t options, uint32_t *words,
                              int64_t cap, int32_t *meta) {
    if (!is_complex_io(dtype)) return -DE_ERR_INVALID_ARG;
    return lower_tape_impl(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, words, cap, meta);
}
int64_t de_lower_tape_stage(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts,
                            int64_t n_consts, int32_t n_features, int32_t n_params, uint32_t options, int stage,
                            uint32_t *words, int64_t cap) {
    if (is_complex_io(dtype)) return -DE_ERR_INVALID_ARG;
    return lower_tape_stage_impl(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, stage, words, cap);
}
int64_t de_lower_tape_stage_complex(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts,
                                    int64_t n_consts, int32_t n_features, int32_t n_params, uint32_t options, int stage,
                                    uint32_t *words, int64_t cap) {
    if (!is_complex_io(dtype)) return -DE_ERR_INVALID_ARG;
    return lower_tape_stage_impl(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, stage, words, cap);
}
static int64_t lower_tape_impl(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                               int32_t n_features, int32_t n_params, uint32_t options, uint32_t *words, int64_t cap, int32_t *meta) {
    // DE_F16: binary16 constants, lowered like a Float32 tape; complex: the component type's tape, table-index immediates
    const DtypeKind kind = dtype_kind(dtype);
    if (!nodes || kind.dtype < 0 || (n_consts > 0 && !consts)) return -DE_ERR_INVALID_ARG;
    const int io = kind.io;
    const bool cplx = kind.cplx;
    dtype = kind.dtype;
    if (cplx && complex_refused_op(nodes, n_nodes) >= 0) return -DE_ERR_UNSUPPORTED_OP;
    if (cplx && n_params > 0) return -DE_ERR_UNSUPPORTED;
    try {
        LowerOptions lo = lower_options(options, n_features, n_params, dtype);
        for (int64_t i = 0; i < n_nodes; i++) // a CSE tape (GraphNode sharing) announces itself by its markers
            if ((nodes[i].degree == 1 && nodes[i].op == DE_OP_SHARE) || (nodes[i].degree == 0 && nodes[i].op == DE_LEAF_SHARED)) lo.cse = true;
        TreeProgram tp;
        std::string why;
        int rc = lower_tree(nodes, n_nodes, n_consts, lo, &tp, &why);
        if (rc != DE_OK) return -rc;
        bool ok_eval = true, ok_grad = true;
        for (int64_t k = 0; k < n_consts; k++) {
            const double v = load_elem(io, consts, (size_t)k);
            if (tp.const_instr[(size_t)k] >= 0) {
                if (cplx) write_cidx(tp.code[(size_t)tp.const_instr[(size_t)k]], (size_t)k); // (the index of the constant's pair)
                else write_imm(tp.code[(size_t)tp.const_instr[(size_t)k]], dtype, v);
            }
            const bool fin = finite_in(dtype, v) && finite_in(dtype, load_elem_im(io, consts, (size_t)k));
            const_flags(fin, tp.const_checks[(size_t)k], lo.early_exit, &ok_eval, &ok_grad);
        }
        if (meta) {
            meta[0] = tp.n_slots;
            meta[1] = ok_eval;
            meta[2] = ok_grad;
            meta[3] = tp.uses_params;
        }
        const int64_t nw = (int64_t)tp.code.size() * 4;
        if (!words || cap < nw) return nw;
        std::memcpy(words, tp.code.data(), (size_t)nw * 4);
        return nw;
    } catch (...) {
        return -DE_ERR_HIP;
    }
}

// Host-only: the interval pass of the assured stream over ONE Float32 tape (de_bind.h assure_tree) — per fused instruction six doubles
// {lo, hi, amin, proven finite (0 / 1), assured handler id, elision bits (ASSURED_*)}: the accumulator behind it.
int64_t de_lower_tape_assured(const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts, int32_t n_features,
                              uint32_t options, double xmax, double *out, int64_t cap) { // (the first three parts, whatever the environment says)
    return de_lower_tape_assured_parts(nodes, n_nodes, consts, n_consts, n_features, options, xmax, ASSURED_PARTS_CLASSIC, out, cap);
}
// ... with the parts of the pass (ASSURED_PART_*, de_bind.h) given by the caller
int64_t de_lower_tape_assured_parts(const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts, int32_t n_features,
                                    uint32_t options, double xmax, uint32_t parts, double *out, int64_t cap) {
    return de_lower_tape_assured_fact(nodes, n_nodes, consts, n_consts, n_features, options, xmax, assured_wide_amin(parts), parts, out, cap);
}
// ... and with the feature fact amin <= |x| <= xmax given by the caller (de_bind.h assure_tree_fact: the pass of a program's tight tier)
int64_t de_lower_tape_assured_fact(const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts, int32_t n_features,
                                   uint32_t options, double xmax, double amin, uint32_t parts, double *out, int64_t cap) {
    if (parts & ~ASSURED_PARTS_ALL) return -DE_ERR_INVALID_ARG;
    if (!(xmax >= 0x1p-40 && xmax <= 0x1p100)) return -DE_ERR_INVALID_ARG;
    if (!(amin >= 0x1p-40 && amin <= xmax)) return -DE_ERR_INVALID_ARG;
    int64_t nw = lower_tape_stage_impl(DE_F32, nodes, n_nodes, consts, n_consts, n_features, 0, options, 3, nullptr, 0);
    if (nw < 0) return nw;
    try {
        std::vector<BoundInstr> f((size_t)nw / 4);
        nw = lower_tape_stage_impl(DE_F32, nodes, n_nodes, consts, n_consts, n_features, 0, options, 3, reinterpret_cast<uint32_t *>(f.data()), nw);
        if (nw < 0) return nw;
        const int64_t n = (int64_t)f.size() * 6;
        if (!out || cap < n) return n;
        std::vector<AssuredInstr> info(f.size());
        assure_tree_fact(f.data(), f.size(), n_features, xmax, amin, info.data(), parts);
        for (size_t i = 0; i < f.size(); i++) {
            double *o = out + 6 * i;
            o[0] = info[i].acc.lo; o[1] = info[i].acc.hi; o[2] = info[i].acc.amin; o[3] = info[i].acc.fin ? 1.0 : 0.0;
            o[4] = (double)info[i].id; o[5] = (double)info[i].bits;
        }
        return n;
    } catch (...) {
        return -DE_ERR_HIP;
    }
}

// Host-only: which cos / exp of a feature gets which memo row of the eval chain (de_bind.h memo_assign — the function a program calls on
// its tightest assured tier).  words = n_instr instructions of stage-4 words (de_lower_tape_stage: {assured id, operand word, immediate}),
// any number of trees behind each other; n_rows = the rows to give out (de_memo_rows_max() is what the library's kernels have).
int32_t de_memo_rows_max(void) { return eval_memo_rows(); }
int32_t de_memo_rows_assign(const uint32_t *words, int64_t n_instr, int32_t n_features, int32_t n_rows, int32_t *k, int32_t *feat, int64_t *uses) {
    if (n_instr < 0 || (n_instr > 0 && !words) || n_features < 0 || n_rows < 0) return -DE_ERR_INVALID_ARG;
    try {
        const MemoAssign m = memo_assign(words, 4, words ? words + 1 : nullptr, 4, (size_t)n_instr, n_features, n_rows);
        for (int r = 0; r < m.n; r++) {
            if (k) k[r] = m.k[r];
            if (feat) feat[r] = m.feat[r];
            if (uses) uses[r] = m.uses[r];
        }
        return m.n;
    } catch (...) {
        return -DE_ERR_HIP;
    }
}

static int64_t lower_tape_stage_impl(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                                     int32_t n_features, int32_t n_params, uint32_t options, int stage, uint32_t *words, int64_t cap) {
    if (stage != 2 && stage != 3 && stage != 4) return -DE_ERR_INVALID_ARG;
    if (stage == 4 && dtype != DE_F32) return -DE_ERR_INVALID_ARG; // (the assured form exists for Float32 programs only)
    std::vector<uint32_t> g;
    int64_t nw = lower_tape_impl(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, nullptr, 0, nullptr);
    if (nw < 0) return nw;
    try {
        g.resize((size_t)nw);
        nw = lower_tape_impl(dtype, nodes, n_nodes, consts, n_consts, n_features, n_params, options, g.data(), nw, nullptr);
        if (nw < 0) return nw;
        std::vector<BoundInstr> b, f;
        bind_tree(reinterpret_cast<const Instr *>(g.data()), (size_t)nw / 4, (options & DE_OPT_EARLY_EXIT) != 0, n_features, &b);
        if (stage >= 3 && dtype != DE_F16 && !is_complex_io(dtype)) fuse_tree(b.data(), b.size(), &f); // (a DE_F16 program never runs the threaded kernel: no fused form)
        if (stage == 4) { // the fused words with the assured stream's handler ids (de_bind.h assure_tree; DE_ASSURED_XMAX as a program reads it)
            std::vector<AssuredInstr> info(f.size());
            assure_tree(f.data(), f.size(), n_features, assured_xmax_env(), info.data(), assured_parts_env());
            for (size_t i = 0; i < f.size(); i++) f[i].bop = info[i].id;
        }
        const std::vector<BoundInstr> &o = stage >= 3 ? f : b;
        const int64_t n = (int64_t)o.size() * 4;
        if (!words || cap < n) return n;
        std::memcpy(words, o.data(), (size_t)n * 4);
        return n;
    } catch (...) {
        return -DE_ERR_HIP;
    }
}
} // extern "C"
