// de_bind.cpp — see de_bind.h.
#include "de_bind.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/de_opcodes.h"

namespace de {
namespace {

int hot_binary_index(uint32_t op) {
    switch (op) {
    case DE_B_ADD: return 0;
    case DE_B_SUB: return 1;
    case DOP_RSUB: return 2;
    case DE_B_MUL: return 3;
    case DE_B_DIV: return 4;
    case DOP_RDIV: return 5;
    default: return -1;
    }
}
int hot_unary_index(uint32_t op) {
    switch (op) {
    case DE_U_COS: return 0;
    case DE_U_EXP: return 1;
    case DE_U_SIN: return 2;
    default: return -1;
    }
}
BoundInstr mk(uint32_t bop, uint32_t arg, uint32_t lo = 0, uint32_t hi = 0) {
    BoundInstr b;
    b.bop = bop;
    b.arg = arg;
    b.lo = lo;
    b.hi = hi;
    return b;
}

} // namespace

void bind_tree(const Instr *code, size_t n, bool ee, int n_features, std::vector<BoundInstr> *out, int param_row_base, int slot_shift) {
    const uint32_t slot0 = (uint32_t)n_features + (uint32_t)slot_shift; // row of spill slot 0
    for (size_t i = 0; i < n; i++) {
        const Instr &ins = code[i];
        const uint32_t hdr = ins.hdr;
        const uint32_t op = hdr & H_OP_MASK;
        uint32_t src = (hdr >> H_SRC_SHIFT) & H_SRC_MASK;
        uint32_t row = ins.feat & 0xFFFFu;
        if (src == SRC_PARAM && param_row_base >= 0) { // a parameter = one more staged row
            src = SRC_ROW;
            row += (uint32_t)param_row_base;
        } else if (src == SRC_ROW && row >= (uint32_t)n_features) row += (uint32_t)slot_shift; // a popped / shared slot row
        const uint32_t lo = ins.imm.u32[0], hi = ins.imm.u32[1];
        if (hdr & H_PUSH) out->push_back(mk(BOP_PUSH, slot0 + ((hdr >> H_PUSH_SHIFT) & H_SLOT_MASK)));
        const bool check_b = ee && (hdr & H_CHECK_B);
        if (check_b && src == SRC_ROW) out->push_back(mk(BOP_CHECK_ROW, row));
        const bool check_out = op != DOP_LOAD && (hdr & (ee ? H_CHECK_OUT : H_CHECK_ALWAYS));
        const bool inject = !ee && (hdr & H_INJECT);
        bool check_done = false;
        if (op == DOP_LOAD) {
            if (src == SRC_ROW) out->push_back(mk(BOP_LOAD_ROW, row));
            else if (src == SRC_CONST) out->push_back(mk(BOP_LOAD_CONST, ins.feat >> 16, lo, hi)); // arg = constant ordinal (gradient seed)
            else out->push_back(mk(BOP_GEN_PARAM, row | (check_b ? 1u << 23 : 0u) | (DOP_LOAD << 24)));
        } else if (op >= DE_T_FMA && op < DOP_LOAD) {
            out->push_back(mk(BOP_TERN, row | (op << 24), slot0 + ((hdr >> H_POPC_SHIFT) & H_SLOT_MASK)));
        } else if (inject && (src == SRC_ACC || src == SRC_ROW)) {
            out->push_back(mk(src == SRC_ACC ? BOP_INJ_ACC : BOP_INJ_ROW, row | (op << 24)));
        } else if (src == SRC_PARAM) {
            out->push_back(mk(BOP_GEN_PARAM, row | (check_b ? 1u << 23 : 0u) | (op << 24)));
        } else {
            const int kb = hot_binary_index(op), ku = hot_unary_index(op);
            if (kb >= 0 && (src == SRC_ROW || src == SRC_CONST)) {
                out->push_back(mk(BOP_BIN_BASE + 4 * kb + (src == SRC_CONST ? 2 : 0) + (check_out ? 1 : 0),
                                  src == SRC_CONST ? (ins.feat >> 16) : row, lo, hi));
                check_done = true;
            } else if (ku >= 0 && (src == SRC_ACC || src == SRC_ROW)) {
                out->push_back(mk(BOP_UN_BASE + 4 * ku + (src == SRC_ROW ? 2 : 0) + (check_out ? 1 : 0), row));
                check_done = true;
            } else if (src == SRC_ROW) {
                out->push_back(mk(BOP_GEN_ROW, row | (op << 24)));
            } else if (src == SRC_CONST) {
                out->push_back(mk(BOP_GEN_CONST, ((ins.feat >> 16) & 0xFFFFu) | (op << 24), lo, hi));
            } else {
                out->push_back(mk(BOP_GEN_ACC, op << 24));
            }
        }
        if (check_out && !check_done) out->push_back(mk(BOP_CHECK_ACC, 0));
    }
}

void bind_tree_grad(const Instr *code, size_t n, int n_features, std::vector<BoundInstr> *out) {
    bool any = false;
    for (size_t i = 0; i < n && !any; i++) any = (code[i].hdr & H_SWAPPED) != 0;
    if (!any) return bind_tree(code, n, true, n_features, out);
    std::vector<Instr> named(code, code + n);
    for (Instr &ins : named) {
        const uint32_t op = ins.hdr & H_OP_MASK;
        if ((ins.hdr & H_SWAPPED) && (op == DE_B_MAX || op == DE_B_MIN)) ins.hdr = (ins.hdr & ~H_OP_MASK) | (op == DE_B_MAX ? DOP_RMAX : DOP_RMIN);
    }
    bind_tree(named.data(), n, true, n_features, out);
}

// ---- superinstruction pass ---------------------------------------------------------------------
namespace {
struct HotBin { int k; bool cst, out; };
bool hot_bin_of(const BoundInstr &b, HotBin *h) {
    if (b.bop < BOP_BIN_BASE || b.bop >= BOP_BIN_END) return false;
    const uint32_t v = b.bop - BOP_BIN_BASE;
    h->k = (int)(v >> 2);
    h->cst = (v & 2) != 0;
    h->out = (v & 1) != 0;
    return true;
}
// acc = x op b  ->  the same value written as  b' op' x'  with the operands swapped
int mirrored(int k) {
    switch (k) {
    case 1: return 2; // SUB  -> RSUB
    case 2: return 1;
    case 4: return 5; // DIV  -> RDIV
    case 5: return 4;
    default: return k; // ADD, MUL
    }
}
bool delta_ok(uint32_t a, uint32_t b, const FuseRows *fr = nullptr) {
    int64_t d = (int64_t)b - (int64_t)a, lo = -127, hi = 127;
    if (fr) { // the distance in variant 0, and the range every variant's distance stays in
        const bool sa = a >= fr->slot_lo && a < fr->slot_hi, sb = b >= fr->slot_lo && b < fr->slot_hi;
        d -= (int64_t)fr->shift * ((sb ? 1 : 0) - (sa ? 1 : 0));
        if (sb && !sa) hi -= fr->headroom;
        if (sa && !sb) lo += fr->headroom;
    }
    return d >= lo && d <= hi;
}
uint32_t with_delta(uint32_t rowA, bool push, uint32_t push_row) {
    const int32_t d = push ? (int32_t)push_row - (int32_t)rowA : 0;
    return (rowA & 0xFFFFFFu) | ((uint32_t)(d & 0xFF) << 24);
}
} // namespace

bool top_is_const_source(uint32_t top) {
    if (top < BOP_COUNT) return bop_is_const_source(top);
    return top == TOP_LOADCONST_PUSH; // TOP_BIN2 row-const keeps row A in arg
}

void fuse_tree(const BoundInstr *b, size_t n, std::vector<BoundInstr> *out, const FuseRows *fr) {
    size_t i = 0;
    while (i < n) {
        size_t j = i;
        bool push = false, chk = false;
        uint32_t push_row = 0, chk_row = 0;
        if (b[j].bop == BOP_PUSH) { push = true; push_row = b[j].arg & 0xFFFFFFu; j++; }
        if (j < n && b[j].bop == BOP_CHECK_ROW) { chk = true; chk_row = b[j].arg & 0xFFFFFFu; j++; }
        if (j < n && (push || chk)) {
            const BoundInstr &m = b[j];
            const uint32_t row = m.arg & 0xFFFFFFu;
            HotBin hb;
            if (m.bop == BOP_LOAD_ROW && (!chk || chk_row == row) && (!push || delta_ok(row, push_row, fr))) {
                if (!chk && j + 1 < n && hot_bin_of(b[j + 1], &hb) && (hb.cst || delta_ok(row, b[j + 1].arg & 0xFFFFFFu, fr))) {
                    const BoundInstr &nb = b[j + 1];
                    BoundInstr f = nb;
                    f.bop = top_bin2(hb.k, hb.cst, hb.out, push);
                    f.arg = with_delta(row, push, push_row);
                    if (!hb.cst) { f.lo = (uint32_t)((int32_t)(nb.arg & 0xFFFFFFu) - (int32_t)row); f.hi = 0; }
                    out->push_back(f);
                    i = j + 2;
                    continue;
                }
                BoundInstr f = m;
                f.bop = top_loadrow(push, chk);
                f.arg = with_delta(row, push, push_row);
                out->push_back(f);
                i = j + 1;
                continue;
            }
            if (m.bop == BOP_LOAD_CONST && push && !chk) {
                if (j + 1 < n && hot_bin_of(b[j + 1], &hb) && !hb.cst && delta_ok(b[j + 1].arg & 0xFFFFFFu, push_row, fr)) {
                    const uint32_t rowA = b[j + 1].arg & 0xFFFFFFu;
                    BoundInstr f = m; // keeps the constant's bits
                    f.bop = top_bin2(mirrored(hb.k), true, hb.out, true);
                    f.arg = with_delta(rowA, true, push_row);
                    out->push_back(f);
                    i = j + 2;
                    continue;
                }
                BoundInstr f = m;
                f.bop = TOP_LOADCONST_PUSH;
                f.arg = push_row;
                out->push_back(f);
                i = j + 1;
                continue;
            }
            if (m.bop >= BOP_UN_BASE && m.bop < BOP_UN_END && ((m.bop - BOP_UN_BASE) & 2) && (!chk || chk_row == row) &&
                (!push || delta_ok(row, push_row, fr))) {
                const uint32_t v = m.bop - BOP_UN_BASE;
                BoundInstr f = m;
                f.bop = top_unrow((int)(v >> 2), (v & 1) != 0, push, chk);
                f.arg = with_delta(row, push, push_row);
                out->push_back(f);
                i = j + 1;
                continue;
            }
            if (!push && chk && hot_bin_of(m, &hb) && !hb.cst && chk_row == row) {
                BoundInstr f = m;
                f.bop = top_binrowc(hb.k, hb.out);
                f.arg = row;
                out->push_back(f);
                i = j + 1;
                continue;
            }
        } else if (j < n) { // no PUSH / CHECK_ROW prefix: LOAD + BIN pairs
            const BoundInstr &m = b[j];
            HotBin hb;
            if (j + 1 < n && hot_bin_of(b[j + 1], &hb)) {
                const BoundInstr &nb = b[j + 1];
                if (m.bop == BOP_LOAD_ROW && (hb.cst || delta_ok(m.arg & 0xFFFFFFu, nb.arg & 0xFFFFFFu, fr))) {
                    const uint32_t row = m.arg & 0xFFFFFFu;
                    BoundInstr f = nb;
                    f.bop = top_bin2(hb.k, hb.cst, hb.out, false);
                    f.arg = row;
                    if (!hb.cst) { f.lo = (uint32_t)((int32_t)(nb.arg & 0xFFFFFFu) - (int32_t)row); f.hi = 0; }
                    out->push_back(f);
                    i = j + 2;
                    continue;
                }
                if (m.bop == BOP_LOAD_CONST && !hb.cst) {
                    BoundInstr f = m;
                    f.bop = top_bin2(mirrored(hb.k), true, hb.out, false);
                    f.arg = nb.arg & 0xFFFFFFu;
                    out->push_back(f);
                    i = j + 2;
                    continue;
                }
            }
        }
        out->push_back(b[i]); // unfused: same id as the bound form
        i++;
    }
}

// ---- interval pass over a fused tree (de_bind.h assure_tree) ---------------------------------------------------------------------
namespace {
const double A_INF = std::numeric_limits<double>::infinity();
AssuredVal a_unbounded() { return AssuredVal{-A_INF, A_INF, 0.0, false}; }
// [lo, hi] and |v| >= amin as computed in double from sound operand bounds -> sound bounds of the ROUNDED Float32 result
AssuredVal a_make(double lo, double hi, double amin) {
    // (T covers the rounding of a SUBNORMAL result only because the kernels keep denormals — gradual underflow, the eval modules are built
    // without flush-to-zero; a flushed result would be 0 where amin claims 2^-14x.  With BIG = 2^120 no reciprocal of a value the pass
    // still calls bounded away from 0 can overflow.)
    const double W = 0x1p-20, T = 0x1p-140, BIG = 0x1p120;
    lo -= std::fabs(lo) * W + T;
    hi += std::fabs(hi) * W + T;
    if (!(lo >= -BIG && hi <= BIG && lo <= hi)) return a_unbounded(); // (written so that NaN fails)
    amin = amin * (1.0 - W) - T;
    if (!(amin > 0.0)) amin = 0.0;
    if (lo > 0.0) amin = std::max(amin, lo);
    if (hi < 0.0) amin = std::max(amin, -hi);
    return AssuredVal{lo, hi, amin, true};
}
AssuredVal a_const(uint32_t bits) {
    float c;
    std::memcpy(&c, &bits, 4);
    if (!std::isfinite(c)) return a_unbounded();
    return AssuredVal{(double)c, (double)c, std::fabs((double)c), true};
}
double a_absmax(const AssuredVal &a) { return std::max(std::fabs(a.lo), std::fabs(a.hi)); }
AssuredVal a_div(const AssuredVal &n, const AssuredVal &d) {
    if (!n.fin || !d.fin || !(d.amin > 0.0)) return a_unbounded();
    const double amin = n.amin / a_absmax(d);
    if (d.lo > 0.0 || d.hi < 0.0) { // a denominator of one sign: |d| in [dl, dh]
        const double dl = std::max(d.amin, std::min(std::fabs(d.lo), std::fabs(d.hi))), dh = a_absmax(d), s = d.lo > 0.0 ? 1.0 : -1.0;
        const double q[4] = {s * n.lo / dl, s * n.lo / dh, s * n.hi / dl, s * n.hi / dh};
        return a_make(std::min(std::min(q[0], q[1]), std::min(q[2], q[3])), std::max(std::max(q[0], q[1]), std::max(q[2], q[3])), amin);
    }
    const double m = a_absmax(n) / d.amin;
    return a_make(-m, m, amin);
}
// K: 0 ADD 1 SUB 2 RSUB 3 MUL 4 DIV 5 RDIV — x op b (R*: b op x), as de_kernels.hip bin_apply
AssuredVal a_bin(int k, const AssuredVal &x, const AssuredVal &b) {
    if (!x.fin || !b.fin) return a_unbounded();
    switch (k) {
    case 0: return a_make(x.lo + b.lo, x.hi + b.hi, 0.0);
    case 1: return a_make(x.lo - b.hi, x.hi - b.lo, 0.0);
    case 2: return a_make(b.lo - x.hi, b.hi - x.lo, 0.0);
    case 3: {
        const double q[4] = {x.lo * b.lo, x.lo * b.hi, x.hi * b.lo, x.hi * b.hi};
        return a_make(std::min(std::min(q[0], q[1]), std::min(q[2], q[3])), std::max(std::max(q[0], q[1]), std::max(q[2], q[3])), x.amin * b.amin);
    }
    case 4: return a_div(x, b);
    case 5: return a_div(b, x);
    default: return a_unbounded();
    }
}
// K: 0 COS 1 EXP (2 SIN and everything else: no rule)
AssuredVal a_un(int k, const AssuredVal &x) {
    if (!x.fin) return a_unbounded();
    if (k == 0) return a_make(-1.0, 1.0, 0.0);
    if (k == 1) return a_make(std::exp(x.lo), std::exp(x.hi), 0.0);
    return a_unbounded();
}
} // namespace

void assure_tree(const BoundInstr *f, size_t n, int n_features, double xmax, AssuredInstr *out, uint32_t parts) {
    // (the wide feature bound: what the tile test guarantees, taken only with the new part — the classic parts keep their intervals id for id)
    assure_tree_fact(f, n, n_features, xmax, assured_wide_amin(parts), out, parts);
}

void assure_tree_fact(const BoundInstr *f, size_t n, int n_features, double xmax, double amin, AssuredInstr *out, uint32_t parts) {
    static thread_local std::vector<AssuredVal> slots; // rows >= n_features an instruction of THIS tree has written
    slots.clear();
    const AssuredVal feature{-xmax, xmax, amin, true};
    auto row_val = [&](uint32_t row) -> AssuredVal {
        if (row < (uint32_t)n_features) return feature;
        const size_t s = row - (uint32_t)n_features;
        return s < slots.size() ? slots[s] : a_unbounded();
    };
    auto push = [&](uint32_t row, const AssuredVal &v) {
        if (row < (uint32_t)n_features) return; // (never: de_program_verify)
        const size_t s = row - (uint32_t)n_features;
        if (s >= slots.size()) slots.resize(s + 1, a_unbounded());
        slots[s] = v;
    };
    AssuredVal acc = a_unbounded();
    for (size_t i = 0; i < n; i++) {
        const BoundInstr &b = f[i];
        const uint32_t id = b.bop, row = b.arg & 0xFFFFFFu;
        const uint32_t prow = (uint32_t)((int32_t)row + (int32_t)(int8_t)(b.arg >> 24)); // (superinstructions with a spill)
        uint32_t twin = id, bits = 0;
        AssuredVal un_arg = a_unbounded(), div_acc = a_unbounded(), div_row = a_unbounded(); // operands of a cos / exp, of a division
        const bool validity = (parts & ASSURED_PART_VALIDITY) != 0;
        if (id == BOP_LOAD_ROW) acc = row_val(row);
        else if (id == BOP_LOAD_CONST) acc = a_const(b.lo);
        else if (id == BOP_PUSH) push(row, acc);
        else if (id == BOP_CHECK_ROW || id == BOP_CHECK_ACC) ; // (a test on its own keeps its record: no twin)
        else if (id >= BOP_BIN_BASE && id < BOP_BIN_END) {
            const uint32_t v = id - BOP_BIN_BASE;
            div_acc = acc;
            div_row = (v & 2) ? a_const(b.lo) : row_val(row);
            acc = a_bin((int)(v >> 2), acc, div_row);
            if (validity && (v & 1) && acc.fin) { twin = id - 1; bits |= ASSURED_OUT; }
        } else if (id >= BOP_UN_BASE && id < BOP_UN_END) {
            const uint32_t v = id - BOP_UN_BASE;
            un_arg = (v & 2) ? row_val(row) : acc;
            acc = a_un((int)(v >> 2), un_arg);
            if (validity && (v & 1) && acc.fin) { twin = id - 1; bits |= ASSURED_OUT; }
        } else if (id >= TOP_LOADROW_BASE && id < TOP_LOADCONST_PUSH) {
            const uint32_t v = id - TOP_LOADROW_BASE;
            if (v & 2) push(prow, acc);
            acc = row_val(row);
            if (validity && (v & 1) && acc.fin) { twin = top_loadrow((v & 2) != 0, false); bits |= ASSURED_ROW; }
        } else if (id == TOP_LOADCONST_PUSH) {
            push(b.arg & 0xFFFFFFu, acc);
            acc = a_const(b.lo);
        } else if (id >= TOP_UNROW_BASE && id < TOP_BINROWC_BASE) {
            const uint32_t v = id - TOP_UNROW_BASE;
            bool chk = (v & 1) != 0, outc = ((v >> 2) & 1) != 0;
            const bool psh = ((v >> 1) & 1) != 0;
            if (psh) push(prow, acc);
            const AssuredVal x = row_val(row);
            un_arg = x;
            acc = a_un((int)(v >> 3), x);
            if (validity && chk && x.fin) { chk = false; bits |= ASSURED_ROW; }
            if (validity && outc && acc.fin) { outc = false; bits |= ASSURED_OUT; }
            twin = top_unrow((int)(v >> 3), outc, psh, chk);
        } else if (id >= TOP_BINROWC_BASE && id < TOP_BIN2_BASE) {
            const uint32_t v = id - TOP_BINROWC_BASE;
            const int k = (int)(v >> 1);
            bool outc = (v & 1) != 0;
            const AssuredVal x = row_val(row);
            div_acc = acc;
            div_row = x;
            acc = a_bin(k, acc, x);
            if (validity && outc && acc.fin) { outc = false; bits |= ASSURED_OUT; }
            if (validity && x.fin) { twin = BOP_BIN_BASE + 4 * (uint32_t)k + (outc ? 1u : 0u); bits |= ASSURED_ROW; } // the plain row form: same operand word
            else twin = top_binrowc(k, outc);
        } else if (id >= TOP_BIN2_BASE && id < TOP_COUNT) {
            const uint32_t v = id - TOP_BIN2_BASE;
            const bool psh = (v & 1) != 0, cst = ((v >> 2) & 1) != 0;
            bool outc = ((v >> 1) & 1) != 0;
            if (psh) push(prow, acc);
            const AssuredVal x = row_val(row);
            div_acc = x; // (the two halves of a TOP_BIN2 division: row A, and row B or the constant)
            div_row = cst ? a_const(b.lo) : row_val((uint32_t)((int32_t)row + (int32_t)b.lo));
            acc = a_bin((int)(v >> 3), x, div_row);
            if (validity && outc && acc.fin) { outc = false; bits |= ASSURED_OUT; }
            twin = top_bin2((int)(v >> 3), cst, outc, psh);
        } else if (id == BOP_GEN_CONST && ((b.arg >> 24) == (uint32_t)DE_U_COS || (b.arg >> 24) == (uint32_t)DE_U_EXP)) {
            acc = a_un((b.arg >> 24) == (uint32_t)DE_U_COS ? 0 : 1, a_const(b.lo)); // cos / exp of a constant (an unfolded program)
        } else acc = a_unbounded(); // generic operators, parameters, ternaries, Inf injection: no rule
        // the range guards, on the id the validity part left: cos / exp without the pre-test, a division that tests only the
        // operand halves the intervals do not cover (forms without such a handler keep their id)
        auto pre_idle = [](int k, const AssuredVal &x) { return x.fin && a_absmax(x) <= (k == 0 ? 9.0e4 : 125.0 / 1.4426950408889634); };
        auto half_idle = [](const AssuredVal &x) { return x.fin && x.amin >= 0x1p-39 && a_absmax(x) <= 0x1p39; };
        if ((parts & ASSURED_PART_PRETEST) && twin >= BOP_UN_BASE && twin < BOP_UN_BASE + 8 && pre_idle((int)((twin - BOP_UN_BASE) >> 2), un_arg)) {
            twin = topa_un((int)((twin - BOP_UN_BASE) >> 2), (twin - BOP_UN_BASE) & 3u);
            bits |= ASSURED_PRE;
        } else if ((parts & ASSURED_PART_PRETEST) && twin >= TOP_UNROW_BASE && twin < TOP_UNROW_BASE + 16 && pre_idle((int)((twin - TOP_UNROW_BASE) >> 3), un_arg)) {
            twin = TOPA_UNROW_BASE + (twin - TOP_UNROW_BASE);
            bits |= ASSURED_PRE;
        } else if ((parts & ASSURED_PART_DIVISION) && twin >= BOP_BIN_BASE + 16 && twin < BOP_BIN_END) {
            const uint32_t v = twin - BOP_BIN_BASE, var = v & 3u;
            const bool ia = half_idle(div_acc), ir = (var & 2) ? false : half_idle(div_row); // (a constant operand keeps its scalar test)
            if (ia || ir) {
                twin = topa_div((int)(v >> 2), var, (var & 2) ? 0u : ((ia ? 0u : 1u) | (ir ? 0u : 2u)));
                bits |= (ia ? ASSURED_DIV_ACC : 0u) | (ir ? ASSURED_DIV_ROW : 0u);
            }
        } else if ((parts & ASSURED_PART_FUSED_DIV) && twin >= top_bin2(4, false, false, false) && twin < TOP_COUNT) {
            const uint32_t v = twin - TOP_BIN2_BASE;
            const bool cst = ((v >> 2) & 1) != 0;
            const bool ia = half_idle(div_acc), ib = cst ? false : half_idle(div_row); // (a constant operand keeps its scalar test)
            if (ia && (cst || ib) && topa_div2_has((int)(v >> 3), cst)) { // (the twins test neither row)
                twin = topa_div2((int)(v >> 3), cst, ((v >> 1) & 1) != 0, (v & 1) != 0);
                bits |= ASSURED_DIV_A | (ib ? ASSURED_DIV_B : 0u);
            }
        }
        out[i].acc = acc;
        out[i].id = twin;
        out[i].bits = bits;
    }
    // the end-fused last instruction: its twin's end-fused form (TOPX_ENDA_BASE) with ASSURED_PART_END, the guarded one otherwise
    if (n >= 2 && topx_endv_of(f[n - 1].bop) >= 0 && (!(parts & ASSURED_PART_END) || topx_enda_of(out[n - 1].id) < 0)) {
        out[n - 1].id = f[n - 1].bop;
        out[n - 1].bits = 0;
    }
}

MemoAssign memo_assign(const uint32_t *ids, size_t id_stride, const uint32_t *args, size_t arg_stride, size_t n, int32_t n_features, int32_t n_rows) {
    MemoAssign m;
    if (n_rows > DE_MEMO_MAX) n_rows = DE_MEMO_MAX;
    if (!ids || !args || n_features <= 0 || n_rows <= 0) return m;
    std::vector<int64_t> count((size_t)2 * (size_t)n_features, 0); // [k][feature row]
    for (size_t i = 0; i < n; i++) {
        const uint32_t id = ids[i * id_stride], row = args[i * arg_stride] & 0xFFFFFFu;
        if (row >= (uint32_t)n_features) continue;
        for (int k = 0; k < 2; k++)
            if (id == topa_unrow_plain(k, false) || id == topa_unrow_plain(k, true)) count[(size_t)k * (size_t)n_features + row]++;
    }
    // the n_rows largest counts; `count` is in (k, feature) order, so the first of equal counts is the smaller pair
    for (; m.n < n_rows; m.n++) {
        size_t best = count.size();
        for (size_t j = 0; j < count.size(); j++)
            if (count[j] > 0 && (best == count.size() || count[j] > count[best])) best = j;
        if (best == count.size()) break;
        m.k[m.n] = (int32_t)(best / (size_t)n_features);
        m.feat[m.n] = (int32_t)(best % (size_t)n_features);
        m.uses[m.n] = count[best];
        count[best] = 0;
    }
    return m;
}

} // namespace de
