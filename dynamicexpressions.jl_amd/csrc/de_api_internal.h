// de_api_internal.h — what the translation units of the C ABI share (round 6: de_api.cpp was one 3 900-line file):
//   de_api.cpp          registry, contexts, the pool of host threads, the pools of device buffers and parked programs
//   de_api_program*.cpp de_program_create / _update / _set_consts / _destroy, constant folding, the threaded and chained streams, verify / dump /
//                       hash — four files, de_api_program.h says what lives where
//   de_api_eval.cpp     de_eval, de_eval_loss, de_eval_sum_certificate, de_eval_tree_array (staging, launch planning)
//   de_api_grad.cpp     what PRODUCES gradients and matrices from X: de_eval_grad / _diff / _pullback_dX, de_eval_loss_grad(_by_class),
//                       de_eval_loss_gn(_ex, _wide), de_eval_fit_stats_grad(_wide): the generic gradient program; glue around the
//                       host-only encoders of the threaded and reverse streams (de_grad_encode.cpp), de_lower_tape_grad
//   de_api_fit.cpp      what CONSUMES them: de_gn_lm_step / de_fit_stats_lm_step (and _wide), de_fit_consts_lm(_ex, _wide),
//                       de_fit_consts_lm_scaled(_wide), de_fit_consts_bfgs, de_fit_consts_nm, the _tied fits — one driver (run_fit) — and their host hooks
//   de_api_batch.cpp    de_batch_sample_rows, de_batch_gather and their host-only twins: minibatches (kernels: de_batch.hip)
//   de_api_tree_params.cpp  de_tape_params_to_consts, de_eval*_tree_params: per-tree parameter matrices, class by class around the calls above
// No behaviour changed in the split: de_program_stream_hash and the whole test suite are the check.
#ifndef DE_API_INTERNAL_H
#define DE_API_INTERNAL_H
#include <hip/hip_runtime.h>
#include <pthread.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <memory>
#include <new>
#include <string>
#include <algorithm>
#include <array>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/de_hip.h"
#include "de_kernels.h"
#include "de_lower.h"
#include "de_host_par.h"

using namespace de;

// ---------------------------------------------------------------------------
struct DevBuf { // grow-only device scratch
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t st = hipMalloc(&p, n);
        if (st == hipSuccess) cap = n;
        return st;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct de_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // de_ctx_timing_ring: pairs of events for the last `ring.size() / 2` timed calls, so that a caller can read the device time of EVERY
    // call of a free-running loop afterwards (de_ctx_last_kernel_ms blocks until the call is done)
    std::vector<hipEvent_t> ring;
    uint64_t ring_at = 0;
    std::string err;
    const char *last_kernel = "";
    // Device buffers of destroyed programs, recycled (round 5): a search loop creates and destroys a program per generation, and hipFree
    // of a multi-megabyte buffer takes 0.3 - 0.5 ms (10^4 trees: de_program_destroy 1.9 ms of a 10 ms generation).  Instruction streams
    // of >= PROG_RECYCLE_MIN bytes are allocated in 1 MiB granules through prog_malloc and parked here by prog_free; at most
    // PROG_RECYCLE_MAX of them / PROG_RECYCLE_BYTES in total, the rest is freed.  DE_NO_PROG_RECYCLE=1: plain hipMalloc / hipFree.
    std::vector<std::pair<void *, size_t>> recycled;
    // ... and the SMALL ones (round 6): a one-tree program (de_eval_tree_array: the reference's own call shape) is a few hundred bytes, and
    // its hipMalloc / hipFree pairs were a third of the call.  Power-of-two size classes from 512 B up to PROG_RECYCLE_MIN, at most
    // SMALL_RECYCLE_MAX buffers parked per context.
    std::vector<std::pair<void *, size_t>> small_free;
    std::map<void *, size_t> big_live; // granule-sized allocations in use (their sizes)
    // ... and the HOST side of destroyed programs: `delete` of a 10^4-tree program is 1.5 ms of munmap (its ~40 vectors are tens of
    // megabytes), and the next creation faults the same pages in again.  Up to four destroyed programs are parked with their vectors
    // cleared; a creation takes the vectors' capacity over (park_program / adopt_parked).
    std::vector<struct de_program *> parked;
    DevBuf sX, sOut, sGrad, sOk, sParams, sClasses, sOut2, sGoff, sNg, sY, sW, sLoss, sPartial, sSeg, sDloss, sColOff, sDoff, sPrio, sStats, sYstats, sJtj, sJoff;
    DevBuf sCert; // de_eval_sum_certificate: per-tree maxima
    DevBuf sBcLoss, sBcDloss, sBcOk, sBcNg, sBcDoff, sBcOut, sBcTiles; // de_eval_loss_grad_by_class
    // de_gn_lm_step / de_fit_consts_lm: sLm — the fit's state (accepted and trial constants, two sets of loss / dloss /
    // jtj / ok, lam, the step) or the staged buffers of a host-pointer de_gn_lm_step; sLmTab — the geometry tables [dloss offsets | jtj
    // offsets | widths] of the last call, uploaded through the pinned image lm_pin only when they differ from lm_tab (what the device
    // holds): lm_ev marks the end of that copy, so a call with device pointers never waits for the stream
    DevBuf sLm, sLmTab;
    // de_eval_loss_gn_wide (csrc/de_gn_wide.h): one pool per call — the chunk's rows and values of the wide trees, the
    // mirrored constants, the partial sums and totals, and device images of a host jtj / ok
    DevBuf sGnw;
    // de_eval*_tree_params (de_api_tree_params.cpp): sTp — the tables, the base and the class's constant vector, the
    // class's results and the double accumulators of one call; sTpOut — the device image of a host `out` of de_eval_tree_params
    DevBuf sTp, sTpOut;
    // de_batch_gather (de_api_batch.cpp): the counter of a host n_bad and the device image of a host `rows`
    DevBuf sBatch;
    std::vector<unsigned char> lm_tab;
    void *lm_pin = nullptr;
    size_t lm_pin_cap = 0;
    hipEvent_t lm_ev = nullptr;
    int nested = 0; // > 0 inside a call made of several inner calls: those do not touch the timing events
    // de_ctx_declare_dataset: a device-resident X the caller promises not to modify — its priority-tile keys are computed once
    const void *ds_X = nullptr;
    int64_t ds_N = 0, ds_ldX = 0;
    int32_t ds_F = 0;
    int ds_dtype = -1;
    DevBuf sPrioDs;
};

// de_eval_loss_gn_wide: the hidden sub-program of the trees with DE_GN_MAX_ROWS < n_grad <= DE_GN_WIDE_MAX_ROWS in one
// gradient mode, built lazily from the tapes the program keeps for de_program_update (in_nodes / in_noff).  It belongs to the program:
// de_program_destroy releases it, and de_program_update — which swaps a freshly created program in — leaves the new program without one.
struct GnWideCache {
    struct de_program *sub = nullptr;
    int mode = -1;
    std::vector<int32_t> trees;   // the wide trees, in population order
    std::vector<int32_t> rows;    // their n_grad in `mode`
    int64_t n_consts = 0;         // constants of the sub-program
    int64_t *d_cidx = nullptr;    // device: constant k of the sub-program = constant d_cidx[k] of the program
    uint64_t consts_gen = ~0ull;  // de_program::consts_gen the sub-program's constants mirror (~0: none yet)
    void *d_tab = nullptr;        // device: the GnWideTree table, uploaded when the jtj offsets differ from its host image `tab`
    std::vector<unsigned char> tab;
};

struct de_program {
    de_ctx *ctx = nullptr;
    GnWideCache *gnw = nullptr;
    int dtype = DE_F32; // element type of the COMPUTE (and of every host-side stream): DE_F32 or DE_F64
    // element type of the caller's buffers — X, constants, parameters, outputs: DE_F16 programs compute in Float32
    // (dtype == DE_F32, constants are binary16 values Float32 holds exactly) and run de_half.hip's kernel, which rounds every operator
    // step to binary16; never the threaded kernel, wave groups, priority tiles or compaction
    int io = DE_F32;
    // complex programs (io DE_CF32 / DE_CF64): dtype is the component type; consts[] holds the real parts, consts_im[] the
    // imaginary ones.  A constant operand's immediate is an index into the constant table — (re, im) pairs of the component type: the
    // constants (slot k at k), then the folded subtrees (fold j at consts.size() + j) — host copy ctab (doubles), device copy d_ctab, read by
    // de_complex.hip with scalar loads; set_consts rewrites the table, never the instruction stream
    std::vector<double> consts_im, ctab;
    void *d_ctab = nullptr;
    uint32_t options = 0;
    int32_t n_features = 0, n_params = 0;
    int64_t n_trees = 0, n_nodes = 0;
    int n_slots = 0;
    bool prows = false; // eval kernels: the parameters are staged per tile as LDS rows F + n_slots + p (rebind), operands like features; false: BOP_GEN_PARAM gathers
    bool uses_params = false;
    std::vector<Instr> code;            // host copy (patched by set_consts)
    std::vector<int32_t> code_off;      // n_trees + 1
    std::vector<int64_t> const_off;     // n_trees + 1
    std::vector<int32_t> const_instr;   // per const (global index): global instr index
    std::vector<uint8_t> const_checks;  // per const: CONST_CHECK_* bits
    std::vector<int32_t> n_consts_tree; // per tree
    bool cse_generic = false;           // some tree's GENERIC (gradient) program is the CSE lowering: a persistent row has several consumers (no reverse accumulation)
    std::vector<uint8_t> host_ok_eval;  // per tree: constant part of the eval flag
    std::vector<uint8_t> host_ok_grad;  // per tree: all constants finite
    std::vector<double> consts;         // current constants as double
    // Constant folding on the device (LowerOptions.fold): the eval path runs `fcode`, in which every
    // maximal constant subtree is one constant operand; the subtrees themselves form the `aux`
    // population, evaluated once per constant update by the same kernels (N = 1).
    bool folded = false;
    std::vector<Instr> fcode;
    std::vector<int32_t> fcode_off;
    std::vector<int32_t> fconst_instr;  // per constant: index into fcode, or < 0 if folded away
    struct Fold { int32_t tree, instr; bool tested_always; };
    std::vector<Fold> folds;            // aux tree j -> (owning tree, fcode instruction holding its value)
    std::vector<int64_t> aux_const_src; // constant k of the fold spans (all folds, concatenated) = consts[aux_const_src[k]]
    de_program *aux = nullptr;          // the folds that are evaluated ON THE DEVICE (fold_host[j] == 0), as a population of their own
    std::vector<uint8_t> fold_ok;
    // Round 6: a constant subtree made of IEEE-exact operators only (+ - * /) is folded ON THE HOST — the same bits by construction
    // (the device's + - * / are correctly rounded, tests/test_gpu_eval.py::test_ieee_exact_operators_are_bit_identical, and every
    // translation unit is built with -ffp-contract=off) — and never enters the auxiliary program: about half of the constant subtrees of the
    // benchmark's operator set.  fold_nodes / fold_noff / fold_coff: every fold's tape slice (constant leaves numbered from the span's first
    // slot) and its range in aux_const_src; aux_fold: auxiliary tree -> fold; aux_csrc: the auxiliary program's constants -> consts.
    std::vector<uint8_t> fold_host;     // per fold: 1 = folded on the host, 2 = by de_fold_kernel (one thread per subtree), 0 = through `aux`
    // the subtrees de_fold_kernel evaluates: kfold[k] = fold index; device image [tape slices | node offsets | constant offsets | constant
    // values | values out | flags out] in ONE pooled allocation (uploaded once; the constant values again at every de_program_set_consts)
    std::vector<int32_t> kfold;
    std::vector<int64_t> kf_csrc;       // constant k of the kernel folds = consts[kf_csrc[k]]
    char *d_kf = nullptr;
    size_t kf_o_noff = 0, kf_o_coff = 0, kf_o_cvals = 0, kf_o_out = 0, kf_o_ok = 0, kf_bytes = 0;
    std::vector<de_tape_node_t> fold_nodes;
    std::vector<int64_t> fold_noff, fold_coff;
    std::vector<int32_t> aux_fold;
    std::vector<int64_t> aux_csrc;
    std::vector<BoundInstr> bcode;      // bound form of the eval program (handler ids)
    std::vector<BoundInstr> tcode;      // threaded form: handler address offsets + LDS byte offsets
    std::vector<BoundInstr> fbcode;     // fused (superinstruction) form the threaded code is made from
    std::vector<int32_t> tcode_off;     // n_trees + 1 offsets into tcode / fbcode
    // what the threaded kernel reads (de_kernels.hip "direct-threaded dispatch"): one 16-byte record per instruction
    // {operand word, immediate, address of its handler} and an end record per tree; made from tcode
    std::vector<BoundInstr> ccode;
    std::vector<int32_t> ccode_off;     // n_trees + 1: first record of each tree
    // WAVE GROUPS (round 6; de_kernels.hip KArgs::var_stride; de_api_program_stream.cpp choose_waves): a program whose one-wave workgroup is short of
    // resident waves (staged parameter rows, many features) runs `waves` (2 / 4 / 8) waves per workgroup on one sample tile — X and the
    // parameter rows staged once, every wave a chunk and spill-slot rows of its own.  Slot rows
    // are host data, so the chained stream exists once per wave: ccode_w = variants 1 .. waves - 1 (each ccode.size() records; the same
    // records as ccode but for the operand words that name a slot row), on the device `var_stride` records apart behind variant 0
    // (0: the trees use no slot — one stream serves every wave).  waves == 1: one-wave workgroups, nothing of this exists.
    int waves = 1;
    int waves_choice = 0; // what choose_waves said when the program was created (0: not asked yet): a re-bind (de_program_set_consts under
                          // DE_NO_CONST_PATCH) keeps it — the arena was sized for it
    int64_t var_stride = 0;
    std::vector<BoundInstr> ccode_w;
    // The ASSURED stream (de_bind.h assure_tree): Float32, non-parametric, exact-mode programs with one-wave workgroups
    // keep ONE more variant of the chained stream in ccode_w — the same records, but validity tests that cannot fire on a tile of ordinary
    // feature values (|x| in [2^-39, assured_xmax]) are left out by naming the untested twin handlers (aids: the twin id of every fused
    // instruction).  It lies var_stride records behind the guarded stream like a wave's variant; a workgroup whose tile passes the test
    // runs it.  assured_cfg: 0 not decided yet, 1 wanted, -1 off (DE_ASSURED=0), read once when the program is created.
    // assured_valid: false behind a de_program_set_consts_device (the host cannot see the values: launches use the guarded stream until a
    // host set or an update re-runs the pass).
    bool assured = false, assured_valid = false;
    int assured_cfg = 0;
    double assured_xmax = 64.0;
    uint32_t assured_parts = 0; // ASSURED_PART_* the pass may use (DE_ASSURED_PARTS, read with DE_ASSURED)
    std::vector<uint32_t> aids;
    // TIERS: tier 1 is the stream above (variant 1); tier 2 is ONE more variant (variant 2, the second ccode.size() records of ccode_w) made by
    // the same pass under the TIGHT feature fact |x| in [assured_tight_amin, assured_tight_xmax] (de_bind.h assure_tree_fact; aids2 its twin
    // ids, always a superset of tier 1's elisions).  A tile runs the tightest stream whose fact it passes.  assured_tiers_cfg: what the program
    // may build (DE_ASSURED_TIERS, 1 or 2; read and inherited like assured_cfg); assured_tiers: what it has — 2 only where the tight pass names
    // an id the wide pass does not, else 1 (0: no assured stream).
    // assured_tiers_room: the tiers the device arena was sized for (0: not allocated yet) — a re-bind of the same program keeps that many.
    int assured_tiers_cfg = 2, assured_tiers = 0, assured_tiers_room = 0;
    // MEMO ROWS (de_bind.h memo_assign, de_kernels.hip h_unrow_fast<.., MROW>): which cos / exp of a feature gets which memo row of the eval chain — the
    // most frequent pairs among the tightest assured tier's untested unary(feature row) instructions.  Made with the assured streams
    // (creation, de_program_update); a set of the constants keeps it: a feature leaf has no constant.  n == 0: none.
    MemoAssign memo;
    double assured_tight_xmax = 8.0, assured_tight_amin = 0x1p-19;
    std::vector<uint32_t> aids2;
    uint64_t end_handler = 0;
    uint64_t endv_handler[TOPX_ENDV_COUNT] = {0}; // "last instruction + end of tree" variants (de_bind.h topx_endv_of)
    bool threaded = false;
    bool direct = false;                // X too wide for the LDS tile (decided at creation)
    uint64_t handler_base = 0;
    std::vector<int32_t> bcode_off;     // n_trees + 1
    BoundInstr *d_code = nullptr;
    int32_t *d_code_off = nullptr;
    bool eval_arena = false;            // d_code_off / d_compact_ints / d_ok_eval point into d_code's allocation
    // compaction of the live trees (de_kernels.hip de_compact_live_kernel): the second half of the d_code allocation (same 4 GiB window) and
    // (n_trees + 1) + n_trees + 4 ints; null when the program is not threaded
    BoundInstr *d_compact_code = nullptr;
    int32_t *d_compact_ints = nullptr;
    bool last_compacted = false; // the most recent eval launch compacted its live trees (de_program_last_live_trees)
    // de_eval_sum_certificate: the eval program with EVERY operator result validity-tested (no exact elision), bound for the flat-switch kernel
    BoundInstr *d_cert_code = nullptr;
    int32_t *d_cert_off = nullptr;
    size_t cert_cap = 0;
    uint64_t consts_gen = 0;       // bumped by every de_program_set_consts
    uint64_t cert_gen = ~0ull;     // consts_gen the uploaded certificate program was built for (~0: none)
    std::vector<double> cert_cmax; // per tree: the largest |constant operand| (an array of N copies of it is summed by the reference)
    BoundInstr *d_gcode = nullptr;      // bound UNFOLDED program on the device (gradient kernels), lazily uploaded
    int32_t *d_gcode_off = nullptr;
    std::vector<BoundInstr> gbcode;
    std::vector<int32_t> gbcode_off;
    bool gcode_stale = true;
    // threaded form of the gradient program for one (mode, window width): de_grad_threaded.hip
    std::vector<BoundInstr> gtcode;
    std::vector<int32_t> gtcode_off;
    BoundInstr *d_gtcode = nullptr;
    int32_t *d_gtcode_off = nullptr;
    int32_t *d_gt_ids = nullptr;        // tree indices grouped by bucket
    uint8_t *d_ok_eval = nullptr;       // device copy of host_ok_eval (initial value of the flags of every eval call)
    // device-resident per-call tables of de_eval_grad, so that a call copies nothing from pageable host memory and never
    // blocks the stream: initial flags, gradient widths of the last mode and packed offsets of the last (mode, N)
    uint8_t *d_ok_grad = nullptr;
    int32_t *d_ng = nullptr;
    int64_t *d_goff = nullptr;
    int tab_mode = -1;
    int64_t tab_N = -1;
    bool tab_ok_stale = true;
    // immediate sites (set_consts patches constants in place): for a generic instruction with a constant
    // operand, the index of the instruction carrying its bits in bcode / tcode (eval source program) and in
    // gbcode / gtcode (unfolded program); -1 elsewhere.  Empty = not available (full rebuild instead).
    std::vector<int32_t> bsite, tsite, gbsite, gtsite_of_gb;
    // compact forms for de_program_set_consts (rebuilt when site_gen moves): only the instructions that carry an immediate
    struct EvalSite { int32_t src, b, t, c; };       // source instruction (fcode/code), bcode index, tcode index, ccode index
    struct GradSite { int32_t src, gb, gt, rt; };   // code instruction, gbcode index, gtcode / rtcode index or -1
    std::vector<EvalSite> eval_sites;
    std::vector<GradSite> grad_sites;
    uint64_t site_gen = 1, lists_gen = 0;
    // reverse-accumulation form (de_rev_threaded.hip) for one gradient mode
    std::vector<BoundInstr> rtcode;
    std::vector<int32_t> rtcode_off, rtcode_mid, rtsite_of_gb;
    BoundInstr *d_rtcode = nullptr;
    int32_t *d_rtcode_off = nullptr, *d_rtcode_mid = nullptr, *d_rt_ids = nullptr;
    int rt_mode = -1, rt_stage_cols = 0, rt_n_groups = 0;
    GradArgs::RevGroup rt_groups[8];
    bool rt_valid = false;
    uint64_t rt_handler_base = 0;
    uint32_t rt_param_off = 0;
    int gt_mode = -1;
    bool gt_valid = false, gt_wide = false;
    bool gt_share = false;        // the threaded gradient program exists in four variants (GradArgs::gt_share), gt_stride records apart in gtcode
    int64_t gt_stride = 0;
    size_t gt_cap = 0;            // records d_gtcode has room for
    int gt_n_buckets = 0;
    GradArgs::Bucket gt_buckets[24];
    // de_program_update: the population as it was created — expanded tapes and CSE tapes (in_coff all 0: none), offsets
    // rebased to 0 — and per tree what its lowerings reported, so that an update lowers the new trees only and copies the others' slices
    std::vector<de_tape_node_t> in_nodes, in_cse;
    std::vector<int64_t> in_noff, in_coff;
    std::vector<int32_t> tree_slots;    // per tree: spill slots of its plain and folded lowerings (the larger)
    std::vector<uint8_t> tree_bits;     // per tree: TREE_PARAMS | TREE_CSE_PLAIN | TREE_CSE_FOLDED
    bool allow_fold = true;             // the creation folded constant subtrees (DE_NO_FOLD unset; false for an auxiliary program)
    // de_program_set_consts_device (kernels: de_const_patch.hip).  consts_dev_ahead: the device streams, flags and
    // d_cp_vals hold constants the host copies (consts, code, fcode, bcode ..., host_ok_*, fold_ok) have not seen yet — every reader of
    // host state calls consts_materialise() first.  d_cp_vals: [constants | de_fold_kernel-route fold values | host-route fold values]
    // in the element type, then the folds' flags; d_cp: the tables (sites, per-tree lists, the host-route folds' image), rebuilt when
    // cp_key no longer describes the program's streams.
    bool consts_dev_ahead = false, consts_dev_path = false;
    char *d_cp_vals = nullptr, *d_cp = nullptr;
    struct ConstPatchKey {
        uint64_t site_gen = 0;
        const void *code = nullptr, *gcode = nullptr, *gtcode = nullptr, *rtcode = nullptr, *ok_grad = nullptr;
        int64_t gt_stride = 0;
        int gt_variants = 0;
        bool operator==(const ConstPatchKey &o) const {
            return site_gen == o.site_gen && code == o.code && gcode == o.gcode && gtcode == o.gtcode && rtcode == o.rtcode &&
                   ok_grad == o.ok_grad && gt_stride == o.gt_stride && gt_variants == o.gt_variants;
        }
    } cp_key;
    int cp_eligible = -1; // what the program's folds allow (decided once): 1 device path, 0 staged
    int64_t cp_n_sites = 0, cp_nk = 0, cp_nh = 0, cp_nkc = 0, cp_nhc = 0;
    size_t cp_o_fok = 0, cp_o_addr = 0, cp_o_src = 0, cp_o_coff = 0, cp_o_checks = 0, cp_o_tfoff = 0, cp_o_tfold = 0, cp_o_gidx = 0, cp_o_hnodes = 0,
           cp_o_hnoff = 0, cp_o_hcoff = 0, cp_o_hcvals = 0;
};
enum : uint8_t { TREE_PARAMS = 1, TREE_CSE_PLAIN = 2, TREE_CSE_FOLDED = 4 };

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t st_ = (expr);                                                             \
        if (st_ != hipSuccess) {                                                             \
            (void)hipGetLastError();                                                         \
            return fail((ctx), DE_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(st_)); \
        }                                                                                    \
    } while (0)


extern "C" {  // (the definitions sit inside the translation units' extern "C" blocks)
int fail(de_ctx *c, int code, const char *fmt, ...);
hipError_t time_begin(de_ctx *c);
hipError_t time_end(de_ctx *c);
bool is_device_ptr(const void *p);
hipError_t prog_malloc(de_ctx *c, void **out, size_t bytes);
void prog_free(de_ctx *c, void *ptr);
void park_program(de_ctx *c, de_program *p);
void adopt_parked(de_ctx *c, de_program *fresh);
bool dataset_keys(const de_ctx *c, int dtype, const void *X, int64_t N, int64_t ldX, int32_t F, void **keys);
bool tree_skip_enabled();
void dbg_lap(const char *what);
struct Staged {
    void *dev = nullptr;
    bool staged = false;
};
int stage_in(de_ctx *c, DevBuf &buf, const void *user, size_t bytes, Staged *s);
int stage_out(de_ctx *c, DevBuf &buf, void *user, size_t bytes, Staged *s);
int check_param_args(de_ctx *c, const de_program *p, const de_param_args_t *pa, int64_t N);
// the host copies of a program brought up to its device constants (de_api_program_consts.cpp); DE_OK at once when they are current
int consts_materialise(de_program *p);
// the body of de_program_set_consts_device (de_api_program_consts.cpp): de_fit_consts_lm sets its trial and accepted constants through it
int set_consts_device_impl(de_program *p, const void *d_consts);
// what de_fit_consts_bfgs and de_fit_tree_params_bfgs refuse about their options (de_api_fit.cpp): null = good, else the reason
const char *bfgs_opts_problem(const de_bfgs_opts_t *o);
// ... and de_fit_consts_lbfgs / de_fit_tree_params_lbfgs about theirs; *shared receives the fields de_bfgs_opts_t has too
const char *lbfgs_opts_problem(const de_lbfgs_opts_t *o, de_bfgs_opts_t *shared);
// releases a program's GnWideCache (de_api_grad.cpp); the caller has synchronised the stream
void gn_wide_release(de_program *p);
}

// The host inputs of a fit or of a wide evaluation, staged ONCE for all its inner calls (de_api_eval.cpp) into the buffers a single call would
// stage them in (sX, sY, sW, sParams, sClasses), with one synchronisation if anything was staged; device pointers, and every pointer when
// N == 0, pass through.  `pa` is the caller's or &pad (a FitInputs is not copied).
struct FitInputs {
    const void *Xd = nullptr, *yd = nullptr, *wd = nullptr;
    de_param_args_t pad;
    const de_param_args_t *pa = nullptr;
};
extern "C" int stage_fit_inputs(de_ctx *c, const de_program *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa,
                                const void *y, const void *w, FitInputs *out);

// Inside a call made of several inner calls: those leave the timing events alone (the ring sees one call); restored on every exit path.
struct NestGuard {
    de_ctx *c;
    explicit NestGuard(de_ctx *c_) : c(c_) { c->nested++; }
    ~NestGuard() { c->nested--; }
    NestGuard(const NestGuard &) = delete;
    NestGuard &operator=(const NestGuard &) = delete;
};

// A device buffer laid out in 256-byte granules.  place<T>(count) hands out regions (wanted = false: none, its pointer is null); reserve()
// grows the buffer — behind a synchronisation, for growing frees what queued work may still use — and from then on ptr(region) is typed.
struct Workspace {
    template <class T> struct Region { size_t off; bool wanted; };
    size_t at = 0;
    char *base = nullptr;
    template <class T> Region<T> place(size_t count, bool wanted = true) {
        const Region<T> r{at, wanted};
        if (wanted) at += (std::max<size_t>(count * sizeof(T), 1) + 255) & ~(size_t)255;
        return r;
    }
    int reserve(de_ctx *c, DevBuf &buf) {
        if (at > buf.cap) HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, buf.reserve(at));
        base = static_cast<char *>(buf.p);
        return DE_OK;
    }
    template <class T> T *ptr(Region<T> r) const { return r.wanted ? reinterpret_cast<T *>(base + r.off) : nullptr; }
};

// The outputs of a fit, each resolved once.  An output the kernels write in place (history, n_accept) is the caller's device pointer or a
// device image copied to the host at the end; an output the fit's state holds (loss / sse, stats, ystats, ok) is copied to the caller
// whichever side its pointer is on (null: not wanted).  finish() issues the copies and waits once if any went to the host (or `wait`).
struct FitOutputs {
    struct Copy { void *user; const void *dev; size_t bytes; bool host; };
    Copy q[6];
    int n = 0;
    static bool on_host(const void *user) { return user && !is_device_ptr(user); }
    template <class T> T *in_place(T *user, bool host, T *image, size_t count) {
        if (!host) return user;
        q[n++] = Copy{user, image, count * sizeof(T), true};
        return image;
    }
    void from_state(void *user, const void *dev, size_t bytes) {
        if (user) q[n++] = Copy{user, dev, bytes, !is_device_ptr(user)};
    }
    int finish(de_ctx *c, bool wait = false) {
        for (int k = 0; k < n; k++) {
            HIP_TRY(c, hipMemcpyAsync(q[k].user, q[k].dev, q[k].bytes, q[k].host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
            wait = wait || q[k].host;
        }
        if (wait) HIP_TRY(c, hipStreamSynchronize(c->stream));
        return DE_OK;
    }
};

// What loss_grad_impl adds to its launch (de_api_grad.cpp).  GnPlan — de_eval_loss_gn: the kernels' Gauss-Newton tree end and G (G + 1) / 2
// more reduction columns per tree of at most DE_GN_MAX_ROWS rows; jtj_offsets: host, element offset of every tree's G x G block (null:
// packed); e_floor: the residual floor of the kind's curvature weight (the spec itself is loss_grad_impl's argument)
struct GnPlan {
    void *jtj;
    const int64_t *jtj_offsets;
    double e_floor;
    int rows_n0 = DE_GN_MAX_ROWS; // N == 0: the widest tree whose block is 0 rather than NaN (de_eval_loss_gn_wide: DE_GN_WIDE_MAX_ROWS)
};
// FitPlan — de_eval_fit_stats_grad: the kernels' fit-statistics tree end.  A tree owns FIT_COLS + 3 G reduction columns
// and, where a matrix is wanted and G <= DE_GN_MAX_ROWS, G (G + 1) / 2 more; loss_grad_impl's dloss / dloss_offsets carry dmom and its
// offsets (3 G doubles per tree), its loss is null and its spec L2 (unused).  Always forward duals.
struct FitPlan {
    double *stats, *ystats;
    void *jtj; // may be null: no matrix wanted
    const int64_t *jtj_offsets;
    int rows_n0 = DE_GN_MAX_ROWS; // N == 0: the widest tree whose block is 0 rather than NaN (de_eval_fit_stats_grad_wide: DE_GN_WIDE_MAX_ROWS)
};
struct ByClassPlan;
extern "C" {
// The evaluations the fits of de_api_fit.cpp are made of (de_api_grad.cpp): the bodies of de_eval_loss_grad_ex / de_eval_loss_gn_ex /
// de_eval_fit_stats_grad (a GnPlan / FitPlan), de_eval_loss_gn_wide and de_eval_fit_stats_grad_wide
int loss_grad_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode, const void *y,
                   const void *w, const de_loss_spec_t *spec, void *loss, void *dloss, const int64_t *dloss_offsets, uint8_t *ok,
                   ByClassPlan *plan, bool first_kinds_only = false, const GnPlan *gn = nullptr, const FitPlan *fit = nullptr);
int gn_wide_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode, const void *y,
                 const void *w, const de_loss_spec_t *spec, double e_floor, void *loss, void *dloss, const int64_t *dloss_offsets, void *jtj,
                 const int64_t *jtj_offsets, uint8_t *ok);
int fit_stats_grad_wide_impl(de_ctx_t *c, de_program_t *p, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pa, int mode,
                             const void *y, const void *w, double *stats, double *ystats, double *dmom, const int64_t *dmom_offsets, void *jtj,
                             const int64_t *jtj_offsets, uint8_t *ok);
// de_gn_spec_check with its reason (null = good; *rc: DE_ERR_INVALID_ARG or DE_ERR_UNSUPPORTED).  dtype < 0: the element type is not known.
const char *gn_spec_problem(const de_loss_spec_t *spec, double e_floor, int dtype, int *rc, char *buf, size_t cap);
// DE_F16 and complex programs evaluate only: every gradient / fused-loss / fit entry point refuses them before it
// touches an output (de_api_grad.cpp)
int refuse_f16(de_ctx_t *c, const de_program_t *p, const char *what);
int refuse_complex(de_ctx_t *c, const char *what);
}
#define DE_REFUSE_F16(WHAT)                                                 \
    do {                                                                    \
        if (c && p && p->io == DE_F16) return refuse_f16(c, p, WHAT);      \
        if (c && p && is_complex_io(p->io)) return refuse_complex(c, WHAT); \
    } while (0)
// de_eval_grad and de_eval_diff alone: a DE_F16 program created with DE_OPT_F16_GRAD passes
#define DE_REFUSE_F16_NO_GRAD(WHAT)                                                                                  \
    do {                                                                                                             \
        if (c && p && p->io == DE_F16 && !(p->options & DE_OPT_F16_GRAD)) return refuse_f16(c, p, WHAT);            \
        if (c && p && is_complex_io(p->io)) return refuse_complex(c, WHAT);                                          \
    } while (0)

// de_loss_spec_check with its reason (de_api.cpp): null = the spec is good, else a text that names the kind (`buf` holds it)
const char *loss_spec_problem(const de_loss_spec_t *spec, int with_gradient, char *buf, size_t cap);

// Bytes of one element of a dtype's buffers, and element k of such a buffer as / from double (binary16 rounds to nearest even).
static inline bool is_complex_io(int dtype) { return dtype == DE_CF32 || dtype == DE_CF64; }
static inline size_t dtype_bytes(int dtype) { return dtype == DE_CF64 ? 16 : (dtype == DE_F64 || dtype == DE_CF32) ? 8 : dtype == DE_F16 ? 2 : 4; }
// (a complex dtype: the real part; load_elem_im the imaginary one, 0 for real dtypes)
static inline double load_elem(int dtype, const void *p, size_t k) {
    if (dtype == DE_CF64) return static_cast<const double *>(p)[2 * k];
    if (dtype == DE_CF32) return (double)static_cast<const float *>(p)[2 * k];
    if (dtype == DE_F64) return static_cast<const double *>(p)[k];
    if (dtype == DE_F16) return (double)static_cast<const _Float16 *>(p)[k];
    return (double)static_cast<const float *>(p)[k];
}
static inline double load_elem_im(int dtype, const void *p, size_t k) {
    if (dtype == DE_CF64) return static_cast<const double *>(p)[2 * k + 1];
    if (dtype == DE_CF32) return (double)static_cast<const float *>(p)[2 * k + 1];
    return 0.0;
}
static inline void store_elem(int dtype, void *p, size_t k, double v, double im = 0.0) {
    if (dtype == DE_CF64) { static_cast<double *>(p)[2 * k] = v; static_cast<double *>(p)[2 * k + 1] = im; }
    else if (dtype == DE_CF32) { static_cast<float *>(p)[2 * k] = (float)v; static_cast<float *>(p)[2 * k + 1] = (float)im; }
    else if (dtype == DE_F64) static_cast<double *>(p)[k] = v;
    else if (dtype == DE_F16) static_cast<_Float16 *>(p)[k] = (_Float16)v;
    else static_cast<float *>(p)[k] = (float)v;
}
namespace de {
size_t complex_row_bytes(int io); // bytes of one LDS row (X feature / spill slot) of the complex policy (de_complex.hip)
bool complex_opcode_ok(int degree, int op); // the 19 opcodes with a Complex method and a Complex result
}

static inline bool in_one_window(const void *ptr, size_t bytes) {
    const uint64_t a0 = (uint64_t)(uintptr_t)ptr;
    return bytes == 0 || (a0 >> 32) == ((a0 + bytes - 1) >> 32);
}
// Pair the constant-carrying instructions of a generic program with those of a derived (bound / fused)
// stream, tree by tree, in program order.  Returns false if the counts disagree (never expected).
template <class Derived, class Pred>
static bool match_const_sites(const std::vector<Instr> &src, const std::vector<int32_t> &src_off, const std::vector<Derived> &dst,
                              const std::vector<int32_t> &dst_off, int64_t n_trees, Pred carries, std::vector<int32_t> *site) {
    site->assign(src.size(), -1);
    std::atomic<bool> ok{true};
    parallel_tree_ranges(n_trees, [&](int, int64_t tb, int64_t te) { // a tree writes its own instructions' entries only
        for (int64_t t = tb; t < te && ok; t++) {
            int32_t j = dst_off[(size_t)t];
            const int32_t j1 = dst_off[(size_t)t + 1];
            for (int32_t i = src_off[(size_t)t]; i < src_off[(size_t)t + 1]; i++) {
                if (((src[(size_t)i].hdr >> H_SRC_SHIFT) & H_SRC_MASK) != SRC_CONST) continue;
                while (j < j1 && !carries(dst[(size_t)j])) j++;
                if (j >= j1) { ok = false; break; }
                (*site)[(size_t)i] = j++;
            }
            while (j < j1 && !carries(dst[(size_t)j])) j++;
            if (j != j1) ok = false;
        }
    });
    if (!ok) { site->clear(); return false; }
    return true;
}

// failure as std::bad_alloc) — an allocation failure becomes a status like everywhere else.
#define DE_NOTHROW(CTX, CALL)                                                                   \
    do {                                                                                        \
        try { return (CALL); }                                                                  \
        catch (const std::bad_alloc &) { return fail((CTX), DE_ERR_HIP, "out of host memory"); } \
        catch (const std::exception &e) { return fail((CTX), DE_ERR_HIP, "internal error: %s", e.what()); } \
        catch (...) { return fail((CTX), DE_ERR_HIP, "internal error (unknown exception)"); }  \
    } while (0)

#endif
