// de_grad_encode.cpp — the two host encoders of the gradient program (de_grad_encode.h): bound records -> direct-threaded records.
// Both switch over ONE decoded view of a bound record (Rec, below), which holds the promotion rules they share; what a record becomes
// in either stream is in encode_forward_tree / encode_reverse_tree, everything around them (buckets, groups, sites, variants) in
// functions of its own.
#include "de_grad_encode.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../include/de_hip.h"
#include "de_host_par.h"
#include "de_lower.h"

namespace de {

void successor_words(std::vector<BoundInstr> &code, int32_t a0, int32_t b0) {
    if (b0 - a0 < 2) return;
    const uint32_t first = code[(size_t)a0].bop;
    for (int32_t i = a0; i < b0 - 1; i++) code[(size_t)i].bop = code[(size_t)i + 1].bop;
    code[(size_t)b0 - 1].bop = first;
}

bool handler_base(const uint64_t *table, uint32_t n, uint64_t *base) {
    uint64_t lo = table[0];
    for (uint32_t i = 0; i < n; i++) lo = std::min<uint64_t>(lo, table[i]);
    for (uint32_t i = 0; i < n; i++)
        if (table[i] - lo > 0xFFFFFFFFull) return false;
    *base = lo;
    return true;
}

namespace {

void no_lap(const char *) {}
constexpr uint64_t LDS_BYTES = 160 * 1024; // of a CU: four waves' rows must fit

// ---- the decoded view of one bound record -------------------------------------------------------------------------------------------
enum class Cls : uint8_t { CheckRow, Load, Push, CheckAcc, Bin, Un, Gen, Tern, Other }; // Bin / Un: HOT operator `k` (GBIN_K / GUN_K lists)
enum class Opnd : uint8_t { Leaf, Slot, Const, Param, Acc };                            // Leaf: a feature row; Param: parameter row `row`
struct Rec {
    Cls cls;
    Opnd opnd;
    bool checked, generic;  // the hot handler's validity-tested variant | bound as BOP_GEN_*: never checked, lo / hi carry a constant's bits or nothing
    int k;
    uint32_t row, ord, aux; // LDS row (Param: parameter row) | constant ordinal | de_opcode of a generic record
};
int hot_unary(uint32_t op) { // hot unary index of a de_opcode (de_bind.h), or -1
    return gun_index((int)op, DE_U_COS, DE_U_EXP, DE_U_SIN, DE_U_NEG, DE_U_SQUARE, DE_U_CUBE, DE_U_ABS, DE_U_LOG, DE_U_SAFE_LOG, DE_U_SQRT, DE_U_SAFE_SQRT, DE_U_TANH, DE_U_RELU);
}

// `hot`: GradEncodeOptions::hot_const_unary — a generic record whose operator has a hot handler is promoted to it: max / min -> hot
// binary 6 / 7, the GUN_K unary functions -> hot unary k.  A parameter operand (always bound generic) takes every hot handler of a leaf.
Rec decode(const BoundInstr &b, int F, bool hot) {
    Rec d{Cls::Other, Opnd::Acc, false, false, -1, b.arg & 0xFFFFFFu, b.arg & 0xFFFFu, b.arg >> 24};
    const Opnd row_kind = d.row < (uint32_t)F ? Opnd::Leaf : Opnd::Slot;
    const uint32_t bop = b.bop;
    if (bop == BOP_CHECK_ROW) d.cls = Cls::CheckRow;
    else if (bop == BOP_LOAD_ROW) { d.cls = Cls::Load; d.opnd = row_kind; }
    else if (bop == BOP_LOAD_CONST) { d.cls = Cls::Load; d.opnd = Opnd::Const; }
    else if (bop == BOP_PUSH) { d.cls = Cls::Push; d.opnd = Opnd::Slot; }
    else if (bop == BOP_CHECK_ACC) d.cls = Cls::CheckAcc;
    else if (bop == BOP_TERN) { d.cls = Cls::Tern; d.opnd = Opnd::Slot; }
    else if (bop >= BOP_BIN_BASE && bop < BOP_BIN_END) { // base + 4 k + 2 (operand is a constant) + checked
        const uint32_t v = bop - BOP_BIN_BASE;
        d = Rec{Cls::Bin, (v & 2) ? Opnd::Const : row_kind, (v & 1) != 0, false, (int)(v >> 2), d.row, d.ord, d.aux};
    } else if (bop >= BOP_UN_BASE && bop < BOP_UN_END) { // base + 4 k + 2 (operand is a row) + checked
        const uint32_t v = bop - BOP_UN_BASE;
        d = Rec{Cls::Un, (v & 2) ? row_kind : Opnd::Acc, (v & 1) != 0, false, (int)(v >> 2), d.row, d.ord, d.aux};
    } else if (bop == BOP_GEN_ROW || bop == BOP_GEN_CONST || bop == BOP_GEN_ACC || bop == BOP_GEN_PARAM) {
        d.generic = true;
        d.opnd = bop == BOP_GEN_ROW ? row_kind : (bop == BOP_GEN_CONST ? Opnd::Const : (bop == BOP_GEN_ACC ? Opnd::Acc : Opnd::Param));
        if (d.opnd == Opnd::Param) d.row = d.ord;
        int kb = -1;
        if (d.opnd == Opnd::Param)
            kb = d.aux == DE_B_ADD ? 0 : d.aux == DE_B_SUB ? 1 : d.aux == (uint32_t)DOP_RSUB ? 2 : d.aux == DE_B_MUL ? 3 : d.aux == DE_B_DIV ? 4 :
                 d.aux == (uint32_t)DOP_RDIV ? 5 : -1;
        if (kb < 0 && hot && d.opnd != Opnd::Acc && (d.aux == (uint32_t)DE_B_MAX || d.aux == (uint32_t)DE_B_MIN)) kb = d.aux == (uint32_t)DE_B_MAX ? 6 : 7;
        const int ku = kb < 0 && hot ? hot_unary(d.aux) : -1;
        if (d.opnd == Opnd::Param && d.aux == (uint32_t)DOP_LOAD) d.cls = Cls::Load;
        else if (kb >= 0) { d.cls = Cls::Bin; d.k = kb; }
        else if (ku >= 0) { d.cls = Cls::Un; d.k = ku; }
        else d.cls = Cls::Gen;
    } // INJ_*: only bound with early_exit=false, never for gradients
    return d;
}

// Gradient row (0-based, in `mode`) that a leaf operand seeds, or -1: parameters first, then features, then (BOTH) the constants.
int gradient_row(const GradSource &s, const Rec &d) {
    if (d.opnd == Opnd::Const) return s.mode == DE_GRAD_CONSTANT ? (int)d.ord : (s.mode == DE_GRAD_BOTH ? s.n_params + s.n_features + (int)d.ord : -1);
    if (s.mode == DE_GRAD_CONSTANT) return -1;
    return d.opnd == Opnd::Param ? (int)d.row : s.n_params + (int)d.row;
}

// ---- forward duals: buckets ---------------------------------------------------------------------------------------------------------
// bucket of a tree = width index x (samples per lane - 1).  Width index 0..6 = single window of width 1,2,3,4,5,6,8; 7,8,9 = several
// windows of 8,5,6 (the narrowest module that covers the gradient in ceil(G/8) windows: 9-10 rows -> 2x5, 11-12 -> 2x6, 17-18 -> 3x6).
// The two-sample modules exist for Float32 windows <= 6; their rows are twice as long, so they only pay while a workgroup's LDS stays
// small: at most vs2_rows rows per wave.
constexpr int NW = 10, NB = 2 * NW;
static_assert(NB == GRAD_BUCKETS_MAX, "bucket count");
const int WIDTH[NW] = {1, 2, 3, 4, 5, 6, 8, 8, 5, 6};
inline int bucket_gc(int b) { return WIDTH[b % NW]; }
inline int bucket_vs(int b) { return 1 + b / NW; }

struct ForwardPlan {
    std::vector<uint8_t> bucket; // per tree
    int32_t count[NB] = {0}, maxg[NB] = {0}, slots[NB] = {0}; // per bucket: trees, widest gradient, most spill slots
    // one wave's slot area of a bucket, in rows: every slot holds a value and GC gradient rows (at least the accumulator's spill)
    uint64_t slot_rows(int b) const { return std::max<uint64_t>((uint64_t)slots[b] * (1 + bucket_gc(b)), (uint64_t)bucket_gc(b)); }
};

// spill slots of tree t: the rows >= F its code names
int32_t tree_spill_slots(const GradSource &s, int64_t t) {
    const uint32_t F = (uint32_t)s.n_features;
    int32_t need = 0;
    for (int32_t i = s.gbcode_off[(size_t)t]; i < s.gbcode_off[(size_t)t + 1]; i++) {
        const BoundInstr &b = s.gbcode[(size_t)i];
        const uint32_t row = b.arg & 0xFFFFFFu;
        if ((bop_reads_row(b.bop) || b.bop == BOP_PUSH || b.bop == BOP_TERN) && row >= F) need = std::max(need, (int32_t)(row - F) + 1);
        if (b.bop == BOP_TERN && b.lo >= F) need = std::max(need, (int32_t)(b.lo - F) + 1);
    }
    return need;
}

// false: some tree has no bucket (more than 240 gradient rows — they travel in 8 bits —, no module for its window: Float64 states wider
// than 16 dwords would pass through scratch memory) or a bucket's four waves do not fit the LDS
bool plan_forward_buckets(const GradSource &s, const GradEncodeOptions &opt, int FE, bool (*has_module)(int, int, int), ForwardPlan *pl) {
    std::vector<int32_t> tslots((size_t)s.n_trees, 0);
    parallel_for_trees(s.n_trees, [&](int64_t t) { tslots[(size_t)t] = tree_spill_slots(s, t); });
    (opt.lap ? opt.lap : no_lap)("grad threaded: spill slots per tree");
    pl->bucket.assign((size_t)s.n_trees, 0);
    for (int64_t t = 0; t < s.n_trees; t++) {
        const int32_t G = s.ng[(size_t)t];
        if (G > 240) return false;
        int w;
        if (G <= 6) w = G < 1 ? 0 : G - 1;
        else if (G <= 8) w = 6;
        else {
            const int windows = (G + 7) / 8, per = (G + windows - 1) / windows;
            w = per <= 5 ? 8 : (per <= 6 ? 9 : 7);
            if (!has_module(s.dtype, WIDTH[w], 1)) w = 7;
        }
        const int rows2 = FE + std::max(tslots[(size_t)t] * (1 + WIDTH[w]), WIDTH[w]);
        const bool two = opt.wide && s.dtype == DE_F32 && WIDTH[w] <= 6 && rows2 <= opt.vs2_rows && has_module(s.dtype, WIDTH[w], 2);
        const int b = w + (two ? NW : 0);
        if (!has_module(s.dtype, bucket_gc(b), bucket_vs(b))) return false;
        pl->bucket[(size_t)t] = (uint8_t)b;
        pl->count[b]++;
        pl->maxg[b] = std::max(pl->maxg[b], G);
        pl->slots[b] = std::max(pl->slots[b], tslots[(size_t)t]);
    }
    const uint64_t es = s.dtype == DE_F32 ? 4 : 8;
    for (int b = 0; b < NB; b++) {
        if (!pl->count[b]) continue;
        const uint64_t row_bytes = 64ull * bucket_vs(b) * es, srows = pl->slot_rows(b);
        if ((opt.share ? (uint64_t)FE + 4 * srows : 4 * ((uint64_t)FE + srows)) * row_bytes > LDS_BYTES) return false;
    }
    return true;
}

// ---- forward duals: the records of one tree -------------------------------------------------------------------------------------------
struct ForwardTree { // what a tree's records are encoded against: its bucket's module
    const GradSource &s;
    bool hot;
    int FE, GC;
    uint32_t RB;     // bytes of one wave's row
    bool one_window; // then every seed is known here and compiled into the handler choice
    GradHandlers h;
    uint32_t slot_off(uint32_t row) const { return (uint32_t)((FE + (row - (uint32_t)s.n_features) * (1 + GC)) * RB); }
    uint32_t word(uint32_t gop) const { return (uint32_t)(h.table[gop] - h.base); }
};

// Appends tree records [i0, i1) to `out`; site[i] (tree-relative) = the record that carries the bits of bound record i's constant;
// kind[] (per appended record, or null) = what a stream variant of the shared-leaf-row launch adds the wave's slot bytes to: 0 nothing,
// 1 the operand word (a slot operand, a push, the spilled operands of a ternary operator), 2 the immediate (push + load of a leaf: row ->
// slot distance).  false: a record has no threaded form.
bool encode_forward_tree(const ForwardTree &T, int32_t i0, int32_t i1, std::vector<BoundInstr> *out, int32_t *site, uint8_t *kind) {
    const GradSource &s = T.s;
    const int GC = T.GC;
    const size_t first = out->size();
    int src = GSRC_ACC, sv = 0; // operand kind and seed variant (de_bind.h: 0 run-time, 1 none, 2 + k) of the record in hand
    bool ok = true;
    // the operand word of a record (`low`: what else travels in it); rt: the handler reads the seed at run time
    auto operand = [&](const Rec &d, uint32_t low = 0, bool rt = false) -> uint32_t {
        sv = 0;
        if (d.opnd == Opnd::Acc) { src = GSRC_ACC; return 0u; }
        if (d.opnd == Opnd::Slot) { src = GSRC_SLOT; return T.slot_off(d.row); }
        const int g = gradient_row(s, d);
        const uint32_t sd = g < 0 ? 0xFFu : (uint32_t)g;
        if (sd != 0xFFu && sd >= 0xF0u) ok = false;
        src = d.opnd == Opnd::Const ? GSRC_CONST : GSRC_LEAF;
        if (!rt && T.one_window) sv = sd == 0xFFu ? 1 : (sd < (uint32_t)GC ? 2 + (int)sd : 0);
        if (d.opnd != Opnd::Const) low = (d.opnd == Opnd::Param ? (uint32_t)s.n_features + d.row : d.row) * T.RB;
        return low | (sv == 0 ? sd << 24 : 0u); // known seeds are compiled into the handler
    };
    auto emit = [&](const BoundInstr &o, uint32_t gop, int knd) {
        out->push_back(BoundInstr{T.word(gop), o.arg, o.lo, o.hi});
        if (kind) kind[out->size() - 1 - first] = (uint8_t)knd;
    };
    for (int32_t i = i0; i < i1 && ok; i++) {
        const BoundInstr &b = s.gbcode[(size_t)i];
        const Rec d = decode(b, s.n_features, T.hot);
        BoundInstr o = b;
        if (d.generic && d.opnd != Opnd::Const) o.lo = o.hi = 0;
        const int32_t here = (int32_t)(out->size() - first);
        uint32_t gop = 0;
        src = GSRC_ACC;
        switch (d.cls) {
        case Cls::CheckRow: continue; // leaf operands are tested where they are read
        case Cls::Load: o.arg = operand(d); gop = gop_load(GC, src, sv); break;
        case Cls::Push: {
            const Rec d2 = i + 1 < i1 ? decode(s.gbcode[(size_t)i + 1], s.n_features, T.hot) : d;
            if (d2.cls == Cls::Load && !d2.generic && (d2.opnd == Opnd::Const || d2.opnd == Opnd::Leaf)) {
                // PUSH followed by the LOAD that starts the next subtree: one dispatch (g_pushload)
                const BoundInstr &b2 = s.gbcode[(size_t)i + 1];
                const uint32_t slot = T.slot_off(d.row);
                if (d2.opnd == Opnd::Const) {
                    o.arg = operand(d2, slot);
                    o.lo = b2.lo;
                    o.hi = b2.hi;
                    site[i + 1 - i0] = here; // the constant lives in the fused instruction
                } else {
                    o.arg = operand(d2);
                    o.lo = slot - d2.row * T.RB; // byte distance row -> slot
                    o.hi = 0;
                }
                if (ok) emit(o, gop_pushload(GC, src, sv), d2.opnd == Opnd::Const ? 1 : 2);
                i++; // the LOAD is part of this instruction
                continue;
            }
            gop = gop_push(GC);
            o.arg = T.slot_off(d.row);
            break;
        }
        case Cls::CheckAcc: gop = gop_check_acc(GC); o.arg = 0; break;
        case Cls::Bin: o.arg = operand(d); gop = gop_bin(GC, d.k, src, sv, d.checked); break;
        case Cls::Un:
            if (d.opnd == Opnd::Const) {
                // cos / exp / sin of a constant leaf (common: half the leaves are constants and the gradient program
                // is not folded): load the constant, then the hot unary handler on the accumulator — not the generic
                // handler (out-of-line operator switch, OCML functions, scratch traffic of its spills)
                o.arg = operand(d);
                site[i - i0] = here;
                if (ok) emit(o, gop_load(GC, src, sv), 0);
                if (ok) emit(BoundInstr{0u, 0u, 0u, 0u}, gop_un(GC, d.k, GSRC_ACC, 0, false), 0);
                continue;
            }
            o.arg = operand(d);
            gop = gop_un(GC, d.k, src, sv, d.checked);
            break;
        case Cls::Gen:
            o.arg = operand(d, d.aux << 16, true);
            gop = gop_gen(GC, src);
            if (d.opnd != Opnd::Const) o.lo = d.aux;
            break;
        case Cls::Tern:
            if (d.row < (uint32_t)s.n_features || b.lo < (uint32_t)s.n_features) { ok = false; break; } // both operands are spilled duals
            gop = gop_tern(GC);
            o.arg = T.slot_off(d.row) | (d.aux << 24);
            o.lo = T.slot_off(b.lo) - T.slot_off(d.row);
            o.hi = 0;
            break;
        default: ok = false; break;
        }
        if (!ok) break;
        site[i - i0] = here;
        emit(o, gop, (src == GSRC_SLOT || d.cls == Cls::Push || d.cls == Cls::Tern) ? 1 : 0);
    }
    // the end record: every tree's chain finishes in g_end (the table slot of round 1's parameter handler)
    if (ok) emit(BoundInstr{0u, 0u, 0u, 0u}, gop_param(GC), 0);
    return ok;
}

// The stream variants of waves 1 .. 3 of the shared-leaf-row launch: the same records with the wave's slot bytes added where a record
// names a slot.  kinds: per tree t from 2 * gbcode_off[t] + t on.
void add_share_variants(const GradSource &s, const ForwardPlan &pl, const std::vector<uint8_t> &kinds, GradForwardStream *r) {
    const size_t n0 = r->gtcode.size();
    const uint32_t es = s.dtype == DE_F32 ? 4u : 8u;
    r->gtcode.resize(4 * n0);
    parallel_for_trees(s.n_trees, [&](int64_t t) {
        const int b = pl.bucket[(size_t)t];
        const uint32_t sbytes = (uint32_t)pl.slot_rows(b) * 64u * (uint32_t)bucket_vs(b) * es; // one wave's slot area
        const uint8_t *kind = kinds.data() + 2 * (size_t)s.gbcode_off[(size_t)t] + (size_t)t;
        const int32_t i0 = r->gtcode_off[(size_t)t];
        for (int32_t i = i0; i < r->gtcode_off[(size_t)t + 1]; i++)
            for (uint32_t w = 1; w < 4; w++) {
                BoundInstr v = r->gtcode[(size_t)i];
                if (kind[i - i0] == 1) v.arg += w * sbytes; // (the low 24 bits: an LDS offset < 2^18)
                else if (kind[i - i0] == 2) v.lo += w * sbytes;
                r->gtcode[(size_t)w * n0 + (size_t)i] = v;
            }
    });
    r->share = true;
    r->stride = (int64_t)n0;
}

} // namespace

int encode_grad_forward(const GradSource &s, const GradEncodeOptions &opt, bool (*has_module)(int dtype, int GC, int VS),
                        const GradHandlerSource &handlers, GradForwardStream *r) {
    void (*lap)(const char *) = opt.lap ? opt.lap : no_lap;
    const int FE = s.n_features + (s.uses_params ? s.n_params : 0); // parameter leaves are LDS rows of their own behind the X rows
    lap(nullptr);
    ForwardPlan pl;
    if (!plan_forward_buckets(s, opt, FE, has_module, &pl)) return GRAD_ENC_NO_PLAN;
    GradHandlers hs[NB];
    for (int b = 0; b < NB; b++) {
        if (!pl.count[b]) continue;
        const int st = handlers(bucket_gc(b), bucket_vs(b), &hs[b]);
        if (st != GRAD_ENC_OK) return st;
    }
    lap("grad threaded: buckets, handler tables");
    r->gtsite_of_gb.assign(s.gbcode.size(), -1);
    // a tree appends at most two records per bound record and its end record
    std::vector<uint8_t> kinds(opt.share ? 2 * s.gbcode.size() + (size_t)s.n_trees : 0, 0);
    std::atomic<bool> ok{true};
    build_stream_by_trees<BoundInstr>(s.n_trees, &r->gtcode, &r->gtcode_off, [&](int64_t t, std::vector<BoundInstr> *out) {
        if (!ok) return;
        const int b = pl.bucket[(size_t)t];
        const ForwardTree T{s, opt.hot_const_unary, FE, bucket_gc(b), 64u * (uint32_t)bucket_vs(b) * (s.dtype == DE_F32 ? 4u : 8u), b % NW < 7, hs[b]};
        const int32_t i0 = s.gbcode_off[(size_t)t];
        if (!encode_forward_tree(T, i0, s.gbcode_off[(size_t)t + 1], out, r->gtsite_of_gb.data() + i0,
                                 opt.share ? kinds.data() + 2 * (size_t)i0 + (size_t)t : nullptr))
            ok = false;
    });
    lap("grad threaded: encode (host threads)");
    if (!ok) return GRAD_ENC_NO_STREAM;
    parallel_for_trees(s.n_trees, [&](int64_t t) { // sites: tree-relative -> positions in the stream
        const int32_t base = r->gtcode_off[(size_t)t];
        if (base == 0) return;
        for (int32_t i = s.gbcode_off[(size_t)t]; i < s.gbcode_off[(size_t)t + 1]; i++)
            if (r->gtsite_of_gb[(size_t)i] >= 0) r->gtsite_of_gb[(size_t)i] += base;
    });
    lap("grad threaded: concatenate + sites");
    // (a handler knows its successor at entry and jumps without waiting for the record it loads)
    parallel_for_trees(s.n_trees, [&](int64_t t) { successor_words(r->gtcode, r->gtcode_off[(size_t)t], r->gtcode_off[(size_t)t + 1]); });
    lap("grad threaded: successor words");
    r->share = false;
    r->stride = 0;
    if (opt.share) {
        add_share_variants(s, pl, kinds, r);
        lap("grad threaded: stream variants (shared leaf rows)");
    }
    // the trees of a bucket side by side in `ids`, the buckets in order
    r->ids.assign((size_t)s.n_trees, 0);
    int32_t fill[NB], run = 0;
    r->n_buckets = 0;
    for (int b = 0; b < NB; b++) {
        fill[b] = run;
        run += pl.count[b];
        if (!pl.count[b]) continue;
        const int GC = bucket_gc(b);
        r->buckets[r->n_buckets++] = GradForwardStream::Bucket{pl.count[b], pl.maxg[b], pl.slots[b], GC, bucket_vs(b), b % NW >= 7 ? (pl.maxg[b] + GC - 1) / GC : 1,
                                                               fill[b], hs[b].base, (uint32_t)(hs[b].table[gop_param(GC)] - hs[b].base)};
    }
    for (int64_t t = 0; t < s.n_trees; t++) r->ids[(size_t)fill[pl.bucket[(size_t)t]]++] = (int32_t)t;
    return GRAD_ENC_OK;
}

// ---- reverse accumulation ---------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu, ACC = 0x80000000u; // column words of the backward records: no column | accumulated per sample first

// SHARED ROWS.  A slot row is written by a PUSH and normally read once; a GraphNode program reads a persistent row from several
// consumers.  Backwards the consumers run in reverse order and the definition's r_pop last: the consumer that runs FIRST in the
// backward sweep (the last reader in program order) stores its adjoint contribution into the row, every other one adds to it.
// acc_use[i - i0] = instruction i reads a slot row and is NOT that row's last reader before its next PUSH.
void shared_row_accumulators(const GradSource &s, int32_t i0, int32_t i1, std::vector<uint8_t> *acc_use) {
    acc_use->assign((size_t)(i1 - i0), 0);
    std::map<uint32_t, int32_t> last_reader; // slot row -> the last instruction seen reading it since its PUSH
    for (int32_t i = i0; i < i1; i++) {
        const BoundInstr &b = s.gbcode[(size_t)i];
        const uint32_t row = b.arg & 0xFFFFFFu;
        if (b.bop == BOP_PUSH) { last_reader.erase(row); continue; }
        if (!bop_reads_row(b.bop) || row < (uint32_t)s.n_features) continue;
        auto it = last_reader.find(row);
        if (it != last_reader.end()) (*acc_use)[(size_t)(it->second - i0)] = 1; // no longer the last reader: it adds
        last_reader[row] = i;
    }
}

// One tree's records in the making: the forward sweep goes straight into the stream, the backward records are collected in forward
// order (`rv`), then reversed, given their column words and fused.
struct ReverseTree {
    const GradSource &s;
    const GradHandlers &h;
    bool rfuse;
    uint32_t RB, FE, PR0;          // row bytes | leaf rows (features + staged parameters) | first partial row
    std::vector<BoundInstr> &code; // the stream
    uint32_t n_prows = 0, last_f_rop = NONE; // partial rows of this tree so far | rop of its last forward record
    struct Back { BoundInstr o; uint32_t rop; bool has_col; }; // has_col: .lo carries a gradient column word
    std::vector<Back> rv, bw;

    BoundInstr mk(uint32_t rop, uint32_t y, uint32_t z, uint32_t w) const { return BoundInstr{(uint32_t)(h.table[rop] - h.base), y, z, w}; }
    uint32_t alloc(uint32_t n) { const uint32_t r = (PR0 + n_prows) * RB; n_prows += n; return r; }
    uint32_t rowb(uint32_t row) const { return (row < (uint32_t)s.n_features ? row : row + (FE - (uint32_t)s.n_features)) * RB; } // LDS byte offset of a bound row
    // column word of a leaf operand's gradient row, or NONE: column 0 is the value; feature / parameter rows are shared by several leaves
    uint32_t column(const Rec &d) const {
        const int g = gradient_row(s, d);
        return g < 0 ? NONE : (1u + (uint32_t)g) | (d.opnd == Opnd::Const ? 0u : ACC);
    }
    // A forward record; returns its place (the record that carries its immediate: de_program_set_consts patches it there)
    int32_t fwd(uint32_t rop, uint32_t y, uint32_t z, uint32_t w) {
        if (rfuse && last_f_rop == ROP_PUSH) { // PUSH + the load / unary function of a leaf that starts the next subtree: one record
            const uint32_t push_off = code.back().arg;
            const bool un_leaf = rop >= ROP_UN_BASE && rop < ROP_GEN_BASE && (((rop - ROP_UN_BASE) >> 1) & 1u);
            bool fused = true;
            if (rop == rop_load(RSRC_LEAF) && push_off < 65536u && y < 65536u) code.back() = mk(ROP_F_PUSHLOAD_BASE + 0, push_off | (y << 16), 0, 0);
            else if (rop == rop_load(RSRC_CONST) && push_off < 65536u) code.back() = mk(ROP_F_PUSHLOAD_BASE + 1, push_off, z, w);
            else if (un_leaf && push_off < 65536u && y < 65536u) {
                const uint32_t v = rop - ROP_UN_BASE;
                code.back() = mk(rop_pushun((int)(v >> 2), (v & 1u) != 0), push_off | (y << 16), z, 0);
            } else fused = false;
            if (fused) rop = 0xFFFFFFFEu; // (nothing fuses with a fused record)
            else code.push_back(mk(rop, y, z, w));
        } else code.push_back(mk(rop, y, z, w));
        last_f_rop = rop;
        return (int32_t)code.size() - 1;
    }
    void back(uint32_t rop, uint32_t y, uint32_t z, bool has_col = false) { rv.push_back(Back{mk(rop, y, z, 0), rop, has_col}); }
    // backward of "acc' = op(acc, operand)" whose partial rows (d/d acc, d/d operand) start at pr
    void back_binary(int pk, uint32_t pr, bool slot, uint32_t slot_byte, uint32_t col, bool add = false) {
        if (slot && add) back(ROP_R_BINACC_BASE + (uint32_t)pk, pk == 0 ? pr : 0, slot_byte);
        else if (slot) back(rop_rbin(pk, 0), pk == 0 ? pr : 0, slot_byte);
        else if (col != NONE) back(rop_rbin(pk, 1), pk == 0 ? pr : 0, col, true);
        else if (pk == 0) back(ROP_R_UN, pr, 0);
        else if (pk == 3) back(ROP_R_NEG, 0, 0);
    }
    // backward of "acc' = f(leaf)": first the unary partial, then the leaf's row — pushed in reverse
    void back_unary_leaf(uint32_t pr, uint32_t col) {
        if (col != NONE) back(ROP_R_LEAF, 0, col, true);
        back(ROP_R_UN, pr, 0);
    }
    // backward of "acc' = f(shared row)": the unary partial, then the row's adjoint receives the result
    void back_unary_slot(uint32_t pr, uint32_t slot_byte, bool add) {
        back(ROP_R_SLOTACC_BASE + (add ? 1u : 0u), slot_byte, 0);
        back(ROP_R_UN, pr, 0);
    }
};

// Forward sweep of tree records [i0, i1) into the stream, their backward records into T.rv.  false: a record has no form here.
bool encode_reverse_tree(ReverseTree &T, int32_t i0, int32_t i1, bool cse_generic, bool hot, const std::vector<uint8_t> &acc_use, int32_t *site) {
    const GradSource &s = T.s;
    const uint32_t F = (uint32_t)s.n_features;
    for (int32_t i = i0; i < i1; i++) {
        const BoundInstr &b = s.gbcode[(size_t)i];
        Rec d = decode(b, s.n_features, hot);
        // (a generic record of a SHARED row whose operator has a hot unary handler keeps the generic one, as it always has)
        if (d.cls == Cls::Un && d.generic && d.opnd == Opnd::Slot) d.cls = Cls::Gen;
        const bool slot = d.opnd == Opnd::Slot, cst = d.opnd == Opnd::Const;
        const bool add = slot && acc_use[(size_t)(i - i0)] != 0;
        const uint32_t col = slot || d.opnd == Opnd::Acc ? NONE : T.column(d);
        // LDS byte offset of the operand row: a bound row, or parameter row prm = leaf row F + prm
        const uint32_t at = d.opnd == Opnd::Param ? (F + d.row) * T.RB : T.rowb(d.row);
        const int src = slot ? RSRC_SLOT : RSRC_LEAF;
        switch (d.cls) {
        case Cls::CheckRow: break; // leaf operands are tested where they are read
        case Cls::Load:
            if (cst) site[i - i0] = T.fwd(rop_load(RSRC_CONST), 0, b.lo, b.hi);
            else T.fwd(rop_load(src), at, 0, 0);
            if (slot) T.back(ROP_R_SLOTACC_BASE + (add ? 1u : 0u), at, 0); // acc = a shared (persistent) row
            else if (col != NONE) T.back(ROP_R_LEAF, 0, col, true);
            break;
        case Cls::Push: {
            // A spill is followed by the load that starts the next subtree (the accumulator's value is dead: the backward sweep
            // continues with the slot's adjoint).  A SHARED definition that is used at once stays in the accumulator: the next
            // instruction reads it, and backwards BOTH adjoints — the accumulator's and the row's — flow into the definition.
            bool acc_live = false;
            for (int32_t q = i + 1; q < i1; q++) {
                const BoundInstr &nx = s.gbcode[(size_t)q];
                if (nx.bop == BOP_CHECK_ROW || nx.bop == BOP_CHECK_ACC || nx.bop == BOP_PUSH) continue;
                const uint32_t nau = nx.arg >> 24;
                acc_live = top_reads_acc(nx.bop, nau == (uint32_t)DOP_LOAD ? 0 : de_opcode_degree((int)nau));
                break;
            }
            T.fwd(ROP_PUSH, at, 0, 0);
            T.back(acc_live ? (uint32_t)ROP_R_POPADD : (uint32_t)ROP_R_POP, at, 0);
            break;
        }
        case Cls::CheckAcc: T.fwd(ROP_CHECK, 0, 0, 0); break;
        case Cls::Bin: { // + - and the reversed - need no partial rows: PK 1, 2, 3
            const uint32_t pr = d.k >= 3 ? T.alloc(2) : 0;
            const int pk = d.k < 3 ? d.k + 1 : 0;
            if (cst) site[i - i0] = T.fwd(rop_bin(d.k, RSRC_CONST, d.checked), pr, b.lo, b.hi);
            else T.fwd(rop_bin(d.k, src, d.checked), at, pr, 0);
            T.back_binary(pk, pr, slot, at, col, add);
            break;
        }
        case Cls::Un: {
            const uint32_t pr = T.alloc(1);
            if (cst) { // cos / exp / sin of a constant leaf: load + hot unary handler instead of the generic one
                site[i - i0] = T.fwd(rop_load(RSRC_CONST), 0, b.lo, b.hi);
                T.fwd(rop_un(d.k, RSRC_ACC, false), pr, 0, 0);
            } else if (d.opnd == Opnd::Acc) T.fwd(rop_un(d.k, RSRC_ACC, d.checked), pr, 0, 0);
            else T.fwd(slot ? rop_un_slot(d.k, d.checked) : rop_un(d.k, RSRC_LEAF, d.checked), at, pr, 0);
            if (slot) T.back_unary_slot(pr, at, add);
            else if (d.opnd == Opnd::Acc) T.back(ROP_R_UN, pr, 0);
            else T.back_unary_leaf(pr, col);
            break;
        }
        case Cls::Gen: {
            const bool unary = d.opnd == Opnd::Acc || d.aux < (uint32_t)DE_B_ADD;
            const uint32_t pr = T.alloc(unary ? 1 : 2);
            if (cst) site[i - i0] = T.fwd(rop_gen(RSRC_CONST), pr | (d.aux << 24), b.lo, b.hi);
            else if (d.opnd == Opnd::Acc) T.fwd(rop_gen(RSRC_ACC), pr | (d.aux << 24), 0, 0);
            else T.fwd(rop_gen(src), at, pr | (d.aux << 24), 0);
            if (d.opnd == Opnd::Acc) T.back(ROP_R_UN, pr, 0);
            else if (!unary) T.back_binary(0, pr, slot, at, col, add);
            else if (slot) T.back_unary_slot(pr, at, add);
            else T.back_unary_leaf(pr, col);
            break;
        }
        case Cls::Tern: {
            if (d.row < F || b.lo < F || d.row > 0xFFFFu || b.lo > 0xFFFFu) return false;
            if (cse_generic) return false; // (a ternary operator's slot operands may be shared rows: r_tern stores; such populations keep forward duals)
            const uint32_t pr = T.alloc(3);
            const uint32_t rb_ = d.row + (T.FE - F), rc_ = b.lo + (T.FE - F);
            if (rb_ > 0xFFFFu || rc_ > 0xFFFFu) return false;
            T.fwd(ROP_TERN, pr | (d.aux << 24), rb_ | (rc_ << 16), 0);
            T.back(ROP_R_TERN, pr, rb_ | (rc_ << 16));
            break;
        }
        default: return false;
        }
    }
    return true;
}

// T.rv -> T.bw: execution order, with the column words.  Gradient rows several leaves share (features, parameters): the leaves'
// contributions are added per SAMPLE in an LDS row and reduced once, at the last of them — paths that cancel within a sample then
// cancel before the reduction, as they do in the forward Jacobian.
// column word: [15:0] column, [29:16] accumulation row, [31:30] 0 reduce now, 1 first, 2 middle, 3 last
bool order_backward(ReverseTree &T, uint32_t *n_acc) {
    std::map<uint32_t, std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> occ; // column -> (leaves, (seen, row))
    for (const auto &e : T.rv)
        if (e.has_col && (e.o.lo & ACC)) occ[e.o.lo & 0xFFFFu].first++;
    *n_acc = 0;
    T.bw.clear();
    for (size_t k = T.rv.size(); k-- > 0;) {
        ReverseTree::Back e = T.rv[k];
        if (e.has_col) {
            const uint32_t col = e.o.lo & 0xFFFFu;
            if ((e.o.lo & 0x7FFFFFFFu) > 0xFFFFu) return false;
            uint32_t word = col;
            if (e.o.lo & ACC) {
                auto &oc = occ[col];
                if (oc.first > 1) {
                    if (oc.second.first == 0) oc.second.second = (*n_acc)++;
                    const uint32_t nth = ++oc.second.first;
                    const uint32_t md = nth == 1 ? 1u : (nth == oc.first ? 3u : 2u);
                    word = col | ((T.PR0 + T.n_prows + oc.second.second) << 16) | (md << 30);
                }
            }
            e.o.lo = word;
        }
        T.bw.push_back(e);
    }
    return true;
}

// T.bw into the stream, with the fused backward sequences: [r_un] r_leaf [r_pop]  and  r_bin<PK, column> r_leaf [r_pop]
void fuse_backward(ReverseTree &T) {
    const auto &bw = T.bw;
    auto is = [&](size_t q, uint32_t rop) { return q < bw.size() && bw[q].rop == rop; };
    auto small = [&](size_t q) { return q >= bw.size() || bw[q].o.arg < 65536u; };
    for (size_t k = 0; k < bw.size();) {
        const bool pop = is(k + 2, ROP_R_POP);
        const bool bincol = bw[k].rop >= ROP_R_BIN_BASE && bw[k].rop < ROP_R_TERN && ((bw[k].rop - ROP_R_BIN_BASE) & 1u);
        if (T.rfuse && is(k, ROP_R_UN) && is(k + 1, ROP_R_LEAF) && small(k) && (!pop || small(k + 2))) {
            T.code.push_back(T.mk(rop_leafx(true, pop), bw[k].o.arg | (pop ? bw[k + 2].o.arg << 16 : 0u), bw[k + 1].o.lo, 0));
            k += pop ? 3 : 2;
        } else if (T.rfuse && is(k, ROP_R_LEAF) && is(k + 1, ROP_R_POP) && small(k + 1)) {
            T.code.push_back(T.mk(rop_leafx(false, true), bw[k + 1].o.arg << 16, bw[k].o.lo, 0));
            k += 2;
        } else if (T.rfuse && bincol && is(k + 1, ROP_R_LEAF) && small(k) && (!pop || small(k + 2))) {
            T.code.push_back(T.mk(rop_bincolx((int)((bw[k].rop - ROP_R_BIN_BASE) >> 1), pop), bw[k].o.arg | (pop ? bw[k + 2].o.arg << 16 : 0u), bw[k].o.lo, bw[k + 1].o.lo));
            k += pop ? 3 : 2;
        } else {
            T.code.push_back(bw[k].o);
            k += 1;
        }
    }
}

// The kernel is latency-bound and its occupancy is set by the LDS rows of the neediest tree of a launch (5 -> 4 workgroups per CU:
// +17 % time): trees are grouped by the number of workgroups per CU their own need allows and every group is a launch of its own
// (small groups join the next needier one).  fixed_rows: what every tree has (leaf rows, slots, staging).
void plan_reverse_groups(int64_t n_trees, uint64_t fixed_rows, uint32_t RB, GradReverseStream *r) {
    const std::vector<uint32_t> &need = r->need;
    std::vector<int32_t> &ids = r->ids;
    auto wgs_of = [&](uint32_t nd) { return (int)std::min<uint64_t>(8, LDS_BYTES / (4 * (fixed_rows + nd) * RB)); };
    ids.resize((size_t)n_trees);
    for (int64_t t = 0; t < n_trees; t++) ids[(size_t)t] = (int32_t)t;
    std::stable_sort(ids.begin(), ids.end(), [&](int32_t x, int32_t y) { return need[(size_t)x] < need[(size_t)y]; });
    r->n_groups = 0;
    const int64_t fill = std::max<int64_t>(64, n_trees / 16); // fewer trees do not fill the chip
    for (int64_t k = 0; k < n_trees;) {
        int64_t e = k;
        const int w = wgs_of(need[(size_t)ids[(size_t)k]]);
        while (e < n_trees && wgs_of(need[(size_t)ids[(size_t)e]]) == w) e++;
        // a group too small to fill the chip, or the last slot: extend to the end / absorb into the next group
        if (r->n_groups == 7) e = n_trees;
        while (e < n_trees && e - k < fill) e++;
        if (n_trees - e < fill) e = n_trees;
        r->groups[r->n_groups++] = GradReverseStream::Group{(int32_t)k, (int32_t)(e - k), (int32_t)(fixed_rows + need[(size_t)ids[(size_t)e - 1]])};
        std::sort(ids.begin() + k, ids.begin() + e); // tree order inside a group: adjacent trees share staging batches
        k = e;
    }
}

} // namespace

int encode_grad_reverse(const GradSource &s, const GradEncodeOptions &opt, int n_slots, bool cse_generic, const GradHandlers &h,
                        GradReverseStream *r) {
    const uint32_t es = s.dtype == DE_F32 ? 4u : 8u, RB = 64u * es;
    // parameter leaves are LDS rows F .. F+P (gathered by class when the kernel stages a tile), slots follow, then the partial rows
    const uint32_t FE = (uint32_t)s.n_features + (s.uses_params ? (uint32_t)s.n_params : 0u), PR0 = FE + (uint32_t)n_slots;
    r->rtcode.clear();
    r->rtcode_off.assign((size_t)s.n_trees + 1, 0);
    r->rtcode_mid.assign((size_t)s.n_trees, 0);
    r->rtsite_of_gb.assign(s.gbcode.size(), -1);
    r->need.assign((size_t)s.n_trees, 0);
    uint32_t max_prows = 0;
    std::vector<uint8_t> acc_use; // per instruction of the tree: reads a shared row and is not its last reader (adds its adjoint)
    ReverseTree T{s, h, opt.rfuse, RB, FE, PR0, r->rtcode};
    for (int64_t t = 0; t < s.n_trees; t++) {
        const int32_t i0 = s.gbcode_off[(size_t)t], i1 = s.gbcode_off[(size_t)t + 1];
        T.n_prows = 0;
        T.last_f_rop = NONE;
        T.rv.clear();
        shared_row_accumulators(s, i0, i1, &acc_use);
        if (!encode_reverse_tree(T, i0, i1, cse_generic, opt.hot_const_unary, acc_use, r->rtsite_of_gb.data() + i0)) return GRAD_ENC_NO_STREAM;
        // end record of the forward sweep (r_end: the table slot of round 1's parameter handler); the backward sweep's first record follows it
        r->rtcode.push_back(T.mk(ROP_PARAM, 0, 0, 0));
        r->rtcode_mid[(size_t)t] = (int32_t)r->rtcode.size();
        uint32_t n_acc = 0;
        if (!order_backward(T, &n_acc)) return GRAD_ENC_NO_STREAM;
        fuse_backward(T);
        if (PR0 + T.n_prows + n_acc > 0x3FFFu) return GRAD_ENC_NO_STREAM;
        r->rtcode.push_back(T.mk(ROP_PARAM, 0, 0, 0)); // end record of the backward sweep
        r->rtcode_off[(size_t)t + 1] = (int32_t)r->rtcode.size();
        max_prows = std::max(max_prows, T.n_prows + n_acc);
        r->need[(size_t)t] = T.n_prows + n_acc;
    }
    // per-wave staging of the column sums: one LDS row, or the widest tree's columns
    r->stage_cols = 64;
    for (int64_t t = 0; t < s.n_trees; t++) r->stage_cols = std::max<int64_t>(r->stage_cols, 1 + s.ng[(size_t)t]);
    const uint64_t stage_rows = ((uint64_t)r->stage_cols * es + RB - 1) / RB;
    const uint64_t rows = (uint64_t)PR0 + max_prows + stage_rows;
    if (4 * rows * RB > LDS_BYTES || rows * RB >= (1u << 24)) return GRAD_ENC_NO_STREAM;
    plan_reverse_groups(s.n_trees, (uint64_t)PR0 + stage_rows, RB, r);
    for (int64_t t = 0; t < s.n_trees; t++) {
        successor_words(r->rtcode, r->rtcode_off[(size_t)t], r->rtcode_mid[(size_t)t]);
        successor_words(r->rtcode, r->rtcode_mid[(size_t)t], r->rtcode_off[(size_t)t + 1]);
    }
    return GRAD_ENC_OK;
}

void reverse_stream_stats(const GradReverseStream &r, int64_t n_trees, const GradHandlers &h) {
    // the stream as it was before the successor rotation: every record under its own handler word
    std::vector<BoundInstr> code = r.rtcode;
    auto unrotate = [&](int32_t a0, int32_t b0) {
        for (int32_t i = b0 - 1; i > a0; i--) code[(size_t)i].bop = r.rtcode[(size_t)i - 1].bop;
        if (b0 - a0 >= 2) code[(size_t)a0].bop = r.rtcode[(size_t)b0 - 1].bop;
    };
    for (int64_t t = 0; t < n_trees; t++) {
        unrotate(r.rtcode_off[(size_t)t], r.rtcode_mid[(size_t)t]);
        unrotate(r.rtcode_mid[(size_t)t], r.rtcode_off[(size_t)t + 1]);
    }
    std::map<uint32_t, uint32_t> rop_of_off; // handler offset -> rop id
    for (uint32_t rop = 0; rop < ROP_COUNT; rop++) rop_of_off.emplace((uint32_t)(h.table[rop] - h.base), rop); // (an unused id names r_nop)
    auto cls = [&](uint32_t off) -> std::string {
        const uint32_t r = rop_of_off.count(off) ? rop_of_off[off] : 9999u;
        char buf[48];
        if (r < 3) snprintf(buf, sizeof buf, "LOAD%c", "LSC"[r]);
        else if (r == ROP_PUSH) return "PUSH";
        else if (r == ROP_CHECK) return "CHECK";
        else if (r >= ROP_BIN_BASE && r < ROP_UN_BASE) snprintf(buf, sizeof buf, "BIN%c", "LSC"[((r - ROP_BIN_BASE) / 2) % 3]);
        else if (r >= ROP_UN_BASE && r < ROP_GEN_BASE) snprintf(buf, sizeof buf, "UN%c", ((r - ROP_UN_BASE) / 2) % 2 ? 'L' : 'A');
        else if (r >= ROP_GEN_BASE && r < ROP_TERN) return "GEN";
        else if (r == ROP_PARAM) return "END";
        else if (r == ROP_R_UN) return "r_un";
        else if (r == ROP_R_NEG) return "r_neg";
        else if (r == ROP_R_POP) return "r_pop";
        else if (r == ROP_R_LEAF) return "r_leaf";
        else if (r >= ROP_R_BIN_BASE && r < ROP_R_TERN) snprintf(buf, sizeof buf, "r_bin%s", (r - ROP_R_BIN_BASE) % 2 ? "col" : "slot");
        else if (r >= ROP_F_PUSHLOAD_BASE && r < ROP_R_LEAFX_BASE) return "PUSH+";
        else if (r >= ROP_R_LEAFX_BASE && r < ROP_R_BINCOLX_BASE) return "r_leafx";
        else if (r >= ROP_R_BINCOLX_BASE && r < ROP_COUNT) return "r_bincolx";
        else return "other";
        return buf;
    };
    std::map<std::string, int64_t> one, two;
    for (size_t i = 0; i < code.size(); i++) {
        const std::string a = cls(code[i].bop);
        one[a]++;
        if (i + 1 < code.size() && a != "END") two[a + " " + cls(code[i + 1].bop)]++;
    }
    fprintf(stderr, "DE_REV_STATS: %zu records, %lld trees: %.2f dispatches per tree\n", code.size(), (long long)n_trees, (double)code.size() / (double)n_trees);
    for (auto &kv : one) fprintf(stderr, "  %-10s %8.3f per tree\n", kv.first.c_str(), (double)kv.second / (double)n_trees);
    std::vector<std::pair<int64_t, std::string>> v;
    for (auto &kv : two) v.push_back({kv.second, kv.first});
    std::sort(v.rbegin(), v.rend());
    for (size_t i = 0; i < v.size() && i < 24; i++) fprintf(stderr, "  pair %-22s %8.3f per tree\n", v[i].second.c_str(), (double)v[i].first / (double)n_trees);
}

} // namespace de
