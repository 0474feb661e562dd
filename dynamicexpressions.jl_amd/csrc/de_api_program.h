// de_api_program.h — what the translation units of the eval program share (only they include it; no .hip file does):
//   de_api_program.cpp          de_program_create / _create_cse / _update / _destroy: per-tree units and the link
//   de_api_program_stream.cpp   the bound, fused, threaded, chained, wave-variant and assured streams (rebind, choose_waves, make_threaded)
//   de_api_program_consts.cpp   constant folds (refresh_folds), the host flags, de_program_set_consts / _get_consts and the device twin
//   de_api_program_inspect.cpp  de_program_verify / _stream_hash / _dump, de_eval_plan, the host lowering hooks de_lower_tape*
#ifndef DE_API_PROGRAM_H
#define DE_API_PROGRAM_H
#include "de_api_internal.h"

static inline void write_imm(Instr &ins, int dtype, double v) {
    if (dtype == DE_F32) {
        ins.imm.u32[1] = 0;
        ins.imm.f32 = (float)v;
    } else ins.imm.f64 = v;
}
// A complex program's constant operand: the immediate is the index of its (re, im) pair in the constant table (de_program::ctab)
static inline void write_cidx(Instr &ins, size_t idx) {
    ins.imm.u32[0] = (uint32_t)idx;
    ins.imm.u32[1] = 0;
}
static inline bool finite_in(int dtype, double v) { return dtype == DE_F32 ? std::isfinite((float)v) : std::isfinite(v); }
// The host part of a tree's flags, one constant at a time: a non-finite constant clears ok_grad always, and ok_eval when its
// CONST_CHECK_* bits say the reference tests it (unconditionally, or under early_exit)
static inline void const_flags(bool finite, uint8_t checks, bool early_exit, bool *ok_eval, bool *ok_grad) {
    *ok_grad = *ok_grad && finite;
    if (!finite && ((checks & CONST_CHECK_ALWAYS) || (early_exit && (checks & CONST_CHECK_EE)))) *ok_eval = false;
}
static inline int64_t eval_rows(const de_program *p) { return (int64_t)p->n_features + p->n_slots + (p->prows ? p->n_params : 0); }
static inline void patch_chained_imm(de_program *p, int32_t c, uint32_t lo, uint32_t hi) {
    if (p->dtype == DE_F32) p->ccode[(size_t)c].arg = lo;
    else { p->ccode[(size_t)c].lo = lo; p->ccode[(size_t)c].hi = hi; }
    for (size_t w = 0; w * p->ccode.size() < p->ccode_w.size(); w++) { // the other waves' variants of the record (wave groups)
        BoundInstr &r = p->ccode_w[w * p->ccode.size() + (size_t)c];
        if (p->dtype == DE_F32) r.arg = lo;
        else { r.lo = lo; r.hi = hi; }
    }
}

// A caller's dtype as a program keeps it.  DE_F16: binary16 buffers, a Float32 program; DE_CF32 / DE_CF64: complex buffers, the
// component type's program (de_api_internal.h de_program::io).  `dtype` < 0: not a dtype.
struct DtypeKind { int io, dtype; bool cplx; };
static inline DtypeKind dtype_kind(int dtype) {
    if (dtype != DE_F32 && dtype != DE_F64 && dtype != DE_F16 && !is_complex_io(dtype)) return {dtype, -1, false};
    return {dtype, (dtype == DE_F16 || dtype == DE_CF32) ? DE_F32 : dtype == DE_CF64 ? DE_F64 : dtype, is_complex_io(dtype)};
}
static inline LowerOptions lower_options(uint32_t options, int32_t n_features, int32_t n_params, int dtype) {
    LowerOptions lo;
    lo.early_exit = (options & DE_OPT_EARLY_EXIT) != 0;
    lo.fuse1 = (options & DE_OPT_FUSE_DEG1) != 0;
    lo.fuse2 = (options & DE_OPT_FUSE_DEG2) != 0;
    lo.bumper = (options & DE_OPT_BUMPER_CHECKS) != 0;
    lo.n_features = n_features;
    lo.n_params = n_params;
    lo.dtype = dtype;
    return lo;
}

// de_program_update: a creation that takes tree t's unit and its bound / fused / wave-variant code from tree src[t] of the
// program `old` (src[t] < 0: lower it) — the same records a lowering of the same tape would produce, read instead of recomputed.
// kept(t) is THE query: de_api_program.cpp asks it where a tree's unit is produced, de_api_program_stream.cpp where a kept tree's
// bound, fused and variant code is taken over.
struct Reuse {
    const de_program *old = nullptr;
    std::vector<int32_t> src;       // per tree of the new population: the old tree it is, or -1
    std::vector<int64_t> fold0;     // per old tree: its first fold (old->folds is ordered by tree), n_trees + 1 entries
    bool kept(int64_t t) const { return old && src[(size_t)t] >= 0; }
};
// A program's first fold per tree (folds are ordered by tree): n_trees + 1 entries
std::vector<int64_t> first_fold_of_trees(const de_program *p);

extern "C" {
// de_api_program.cpp
int complex_refused_op(const de_tape_node_t *nd, int64_t n); // the first opcode of a tape a complex program refuses, or -1
// de_api_program_stream.cpp
void rebind(de_program *p, const Reuse *ru = nullptr);
int make_threaded(de_ctx *c, de_program *p, const Reuse *ru = nullptr);
void assure_program_tree(const de_program *p, int tier, int32_t i0, int32_t i1, AssuredInstr *info);
void assured_link_trees(de_program *p, const uint64_t *table, int64_t tb, int64_t te, bool touched_only = false, int tier = 1);
void program_memo_assign(const de_program *p, MemoAssign *out); // (what make_assured stores in p->memo; de_program_verify re-derives it)
hipError_t upload_wave_variants(de_program *p);
double assured_xmax_env();
uint32_t assured_parts_env();
// de_api_program_consts.cpp
void fill_ctab_consts(de_program *p);
int upload_ctab(de_ctx *c, de_program *p);
void recompute_host_ok(de_program *p);
int refresh_folds(de_ctx *c, de_program *p, bool aux_current = false);
}
#endif
