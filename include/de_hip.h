/*
 * de_hip.h — C ABI of libde_hip.so: MI355X (gfx950) batched expression-tree
 * evaluation, the drop-in replacement for the hot path of DynamicExpressions.jl
 * (reference v2.9.2).  Everything crossing this boundary is plain C: pointers,
 * sizes, enums.  No C++ exception and no abort crosses it; every entry point
 * returns a de_status_t.  Numeric failure (NaN/Inf) is DATA, reported through
 * the per-tree `ok` bytes exactly like the reference's `complete` flag
 * (reference src/Evaluate.jl:258-262), never through the status code.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   de_eval            <- eval_tree_array(tree, cX, operators; eval_context)
 *                         src/Evaluate.jl:279-309 (+ the Bumper whole-tree override
 *                         _bumper_eval_tree_array(tree,cX,operators,ctx)->(result,ok),
 *                         ext/DynamicExpressionsBumperExt.jl:11-49, dispatched at
 *                         src/Evaluate.jl:300-302 — the plug-in precedent this ABI
 *                         sits behind)
 *   de_eval_grad       <- eval_grad_tree_array(tree, cX, operators; variable)
 *                         src/EvaluateDerivative.jl:193-228
 *   de_eval_diff       <- eval_diff_tree_array(tree, cX, operators, direction)
 *                         src/EvaluateDerivative.jl:40-53
 *   de_eval (n_params>0, params/classes set)
 *                      <- eval_tree_array(ex::ParametricExpression, X, classes, ops)
 *                         src/ParametricExpression.jl:371-390
 *   de_opcode_by_name  <- the OperatorEnum function table, src/OperatorEnum.jl:14-49
 *
 * Layouts (identical to the reference so Julia arrays pass zero-copy):
 *   X    : [n_features, N] column-major, feature index fastest; element (f,j) at
 *          X[f + ldX*j]  (src/Evaluate.jl:251,716-724), ldX >= n_features.
 *   out  : population output, row `t` (tree t) at out + t*ld_out, N contiguous
 *          samples (each row is one reference `Vector{T}(N)`).
 *   grad : per tree an [n_grad, N] column-major matrix (gradient index fastest),
 *          entry (k,j) at k + n_grad*j  (src/EvaluateDerivative.jl:355-361).
 *   ok   : one byte per tree, 1 = complete, 0 = a NaN/Inf was met.
 *
 * Memory: the CALLER allocates every buffer.  X/out/grad/ok/params/classes may be
 * device pointers (hipMalloc / AMDGPU.jl ROCArray / torch) — used in place, the
 * call is asynchronous on the context's stream — or plain host pointers, in
 * which case the library stages them through its own device scratch and the
 * call returns after the results are back in host memory.  The library never
 * frees or retains caller memory.
 *
 * Threading: a de_ctx_t owns one device, one stream and scratch; use one context
 * per calling thread (as the reference is re-entrant and lock-free).
 * Different contexts may be used concurrently.
 */
#ifndef DE_HIP_H
#define DE_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "de_opcodes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (callers compare de_abi_version() with the version they were written for):
 *   1  rounds 1-2.
 *   2  round 3-4.  OBSERVABLE changes against 1, none of them in a signature:
 *      (a) early exit at tree granularity is the default: the out / grad rows of a tree with ok == 0 are PARTIALLY written
 *          (device buffers) or NaN-filled (host buffers: the library fills them after the copy) — only the flag is
 *          contractual, as in the reference; DE_OPT_FULL_EVAL (new option bit 5) restores full rows;
 *      (b) programs made by de_program_create_cse: the gradient row of a shared constant's FIRST occurrence carries the
 *          total over its occurrences, the rows of the later occurrences are 0 (callers sum the occurrence rows);
 *      (c) new exports: de_dist_world_size, de_prio_tiles_wanted, de_program_last_live_trees, de_ctx_declare_dataset;
 *      (d) a process may hold contexts on several devices (the handler caches are per device).
 *   3  round 6.  (a) de_eval_loss_grad / de_eval_loss_grad_by_class run FORWARD duals unless the program carries the new option bit
 *      DE_OPT_REVERSE_GRAD (ABI 2 picked reverse accumulation from 8 gradient rows per tree on; DE_OPT_FORWARD_GRAD asked for what is now
 *      the default): same values to rounding, the reference's flags exactly; (b) new exports, all additive (see below).
 *      Additive since: (c) dtype DE_F16 (IEEE binary16 X / constants / parameters / outputs, every operator rounded to binary16 —
 *      Julia's Float16 arithmetic) for de_program_create(_cse), de_program_set_consts, de_eval, de_eval_sum_certificate,
 *      de_eval_tree_array and the host-only / debug hooks; the gradient, loss and dataset entry points answer DE_ERR_UNSUPPORTED for it.
 *      (d) dtypes DE_CF32 / DE_CF64 (interleaved complex X / constants / outputs, Julia's ComplexF32 / ComplexF64 arithmetic over the
 *      19 opcodes that have a Complex method with a Complex result) for the same calls, except that the host lowering
 *      hooks keep their real dtype domain and complex tapes lower through the new de_lower_tape_complex / de_lower_tape_stage_complex;
 *      the same entry points answer DE_ERR_UNSUPPORTED, and so does de_program_create with n_params > 0.
 *      (e) de_program_update: replace some trees of a program in place, for every dtype.
 *      (f) de_lower_tape_grad: the host-only hook of the two gradient stream encoders, DE_F32 / DE_F64.
 *      (g) de_lower_tape_assured, stage 4 of de_lower_tape_stage and words 5 / 6 and which = 4 of de_program_dump: the assured
 *      stream of Float32 programs.
 *      (h) de_gn_lm_step, de_fit_consts_lm (with de_lm_opts_t) and the host-only hook de_lm_solve_host: Levenberg-Marquardt on the
 *      constants of a population on the device, DE_F32 / DE_F64.
 *      (i) de_gn_spec_check, de_eval_loss_gn_ex, de_fit_consts_lm_ex: the Gauss-Newton matrix and the fit under every loss kind that has a
 *      curvature; de_eval_loss_gn and de_fit_consts_lm forward to them with {DE_LOSS_L2, 0, 0}: the same bits.
 *      (j) de_eval_fit_stats_grad: the fit statistics with their gradient moments and the Gauss-Newton matrix — what a
 *      fit of the constants under linear scaling a + b yhat needs.
 *      (k) de_gn_wide_max_rows, de_eval_loss_gn_wide, de_gn_lm_step_wide, de_fit_consts_lm_wide and the host-only hook
 *      de_lm_solve_host_wide: the Gauss-Newton matrix, the step and the fit for trees of 9 to 32 gradient rows; every
 *      entry point above keeps its bits and de_gn_max_rows() stays 8.
 *      (l) de_fit_stats_lm_step, de_fit_consts_lm_scaled and the host-only hook de_lm_project_host: the Levenberg-Marquardt step and the
 *      whole fit under linear scaling on the device, from what de_eval_fit_stats_grad returns; DE_F32 / DE_F64.
 *      (m) de_eval_fit_stats_grad_wide, de_fit_stats_lm_step_wide, de_fit_consts_lm_scaled_wide and the host-only hook
 *      de_lm_project_host_wide: the same for trees of 9 to 32 gradient rows; every entry point above keeps its bits.
 *      (n) de_bfgs_max_rows, de_fit_consts_bfgs (with de_bfgs_opts_t) and the host-only hooks de_bfgs_direction_host and
 *      de_bfgs_update_host: BFGS on the constants of a population on the device, from the loss and its gradient alone (DESIGN.md
 *      §4.4.10), under every loss kind that has a gradient, for trees of up to 32 constants; DE_F32 / DE_F64.
 *      (o) de_tape_params_to_consts, de_eval_tree_params, de_eval_loss_tree_params, de_eval_loss_grad_tree_params (with de_tree_params_t)
 *      and the host-only hook de_tree_params_accumulate_host: a population whose trees each own their parameter matrix, served one class
 *      segment at a time as a non-parametric program whose parameter slots are patched on the device; DE_F32 / DE_F64.
 *      (p) de_fit_tree_params_bfgs and the host-only hooks de_tree_params_pack_host / de_tree_params_unpack_host: BFGS over each tree's
 *      vcat(constants, parameters[:]) of such a population on the device, up to 32 unknowns per tree; DE_F32 / DE_F64.
 *      (q) de_nm_max_rows, de_fit_consts_nm (with de_nm_opts_t) and the host-only hooks de_nm_ask_host / de_nm_tell_host: Nelder-Mead on
 *      the constants of a population on the device, from the fused loss alone — every kind de_eval_loss_ex takes,
 *      programs made by de_program_create_cse included, trees of up to 32 constants; DE_F32 / DE_F64.
 *      (r) de_fit_consts_bfgs_scaled, de_fit_consts_nm_scaled and the host-only hook de_scaled_objective_host: the two fits above under
 *      linear scaling (the objective scaled_sse, in double); every entry point above keeps its bits.
 *      (s) de_lbfgs_max_rows, de_lbfgs_max_memory, de_fit_consts_lbfgs, de_fit_tree_params_lbfgs (with de_lbfgs_opts_t) and the host-only
 *      hooks de_lbfgs_direction_host / de_lbfgs_update_host: L-BFGS for trees of up to 4096 unknowns, the two BFGS fits' contracts with
 *      a ring of (s, yv) pairs per tree instead of B; every entry point above keeps its bits.
 *      (t) de_fit_consts_bfgs_tied, de_fit_consts_lbfgs_tied, de_fit_consts_nm_tied, de_fit_consts_lm_tied and the host-only hooks
 *      de_ties_pack_host / de_ties_unpack_host / de_ties_fold_host / de_ties_fold_matrix_host: the device fits with a shared GraphNode
 *      constant as ONE unknown, for programs made by de_program_create_cse; every entry point above keeps its bits.
 *      (u) DE_OPT_F16_GRAD (new option bit 8): a DE_F16 program created with it is served by de_eval_grad and de_eval_diff, in binary16
 *      steps; without the bit, and for every other dtype, nothing changes.
 *      (v) DE_OPT_TYPED_LOSS (new option bit 9): a DE_F16 / DE_CF32 / DE_CF64 program created with it is served by de_eval_loss and
 *      de_eval_loss_ex (DE_LOSS_L2 / DE_LOSS_L1; the buffer table at de_eval_loss); without the bit nothing changes for them.  And, with
 *      no bit: de_eval_loss / de_eval_loss_ex serve the DE_F32 / DE_F64 programs that do not run the LDS-tiled kernel (a feature matrix
 *      too wide for its tile, DE_EVAL_THREADED=0), every kind — calls that answered DE_ERR_UNSUPPORTED before.
 *      (w) de_batch_sample_rows, de_batch_gather and the host-only de_batch_rows_host / de_batch_gather_host (with de_batch_mode_t,
 *      de_batch_src_t, de_batch_dst_t): minibatches — a counter-based device row sampler and a gather of the sampled rows of X, y, w
 *      and classes into a dense batch that every entry point above serves unchanged; all five dtypes. */
#define DE_HIP_ABI_VERSION 3

typedef enum de_status {
    DE_OK = 0,
    DE_ERR_INVALID_ARG = 1,    /* null pointer, negative size, bad enum          */
    DE_ERR_BAD_TAPE = 2,       /* tape is not a well-formed post-order tree      */
    DE_ERR_UNSUPPORTED_OP = 3, /* opcode outside de_opcodes.h / wrong degree     */
    DE_ERR_HIP = 4,            /* a HIP runtime call failed (see de_last_error)  */
    DE_ERR_NO_DEVICE = 5,      /* no gfx950 device visible                       */
    DE_ERR_OUT_OF_RANGE = 6,   /* feature/param/const/class index out of range   */
    DE_ERR_UNSUPPORTED = 7,    /* valid request this build cannot serve          */
    DE_ERR_RCCL = 8            /* librccl.so missing or an RCCL call failed (de_dist_last_error) */
} de_status_t;

/* DE_F16: binary16 elements (2 bytes) everywhere the dtype sizes a buffer; computed in Float32 registers and rounded to binary16 after
 * every operator step.  Evaluation only: de_eval_grad / _diff / _pullback_dX, de_eval_loss(_grad, _grad_by_class) and
 * de_ctx_declare_dataset return DE_ERR_UNSUPPORTED for an F16 program or dtype and leave their outputs untouched — except that a program
 * created with DE_OPT_F16_GRAD is served by de_eval_grad and de_eval_diff (binary16 X, constants, parameters, out and grad), and one created
 * with DE_OPT_TYPED_LOSS by de_eval_loss / de_eval_loss_ex (DE_LOSS_L2 / DE_LOSS_L1; binary16 y and w, Float32 losses).  F16 programs never
 * run the threaded kernel (de_eval_plan / de_program_dump report the flat-switch kernel's form); a feature matrix too wide for its LDS
 * tile is gathered from global memory as for Float32.  de_eval_sum_certificate refuses such wide programs for every dtype. */
/* DE_CF32 / DE_CF64: complex elements, (re, im) interleaved — 8 bytes (numpy complex64, Julia ComplexF32) / 16 bytes (complex128,
 * ComplexF64) everywhere the dtype sizes a buffer; a constant is one (re, im) pair.  Opcodes: neg square cube inv sqrt exp log sin cos
 * tan sinh cosh tanh custom_cos + - * / +(x, y, z); every other one fails program creation with DE_ERR_UNSUPPORTED_OP (de_last_error names
 * it).  A value is valid when both components are finite.  Evaluation only, as DE_F16 — with DE_OPT_TYPED_LOSS also de_eval_loss /
 * de_eval_loss_ex (DE_LOSS_L2 / DE_LOSS_L1; complex y, REAL w and losses of the component type) — (parameters included: n_params > 0 is refused);
 * DE_OPT_TURBO is ignored.  de_eval_sum_certificate certifies when N * max(|re|, |im|) * 1.001 stays below the component type's floatmax. */
typedef enum de_dtype { DE_F32 = 0, DE_F64 = 1, DE_F16 = 2, DE_CF32 = 3, DE_CF64 = 4 } de_dtype_t;

/* Gradient modes of eval_grad_tree_array (src/EvaluateDerivative.jl:200-210). */
typedef enum de_grad_mode {
    DE_GRAD_VARIABLE = 0, /* variable=true : n_grad = n_features(+n_params)           */
    DE_GRAD_CONSTANT = 1, /* variable=false: n_grad = count_constant_nodes(tree)     */
    DE_GRAD_BOTH = 2      /* Val(:both)    : features first, then constants (:220)   */
} de_grad_mode_t;

/* Option bits = the reference's EvalContext knobs that change RESULTS
 * (src/Evaluate.jl:156-181).  bumper/buffer are CPU back-end choices and have
 * no meaning here, except DE_OPT_BUMPER_CHECKS below; turbo maps to DE_OPT_TURBO. */
enum de_options {
    /* EvalContext.early_exit (default true).  The bit selects the FLAG semantics:
     * with it, `ok` is false iff any value the reference would have tested is
     * non-finite; without it, only constant folding can clear `ok`
     * (src/Evaluate.jl:305-308,347-354).  And, as in the reference, the exit
     * itself (@return_on_nonfinite_array, src/Evaluate.jl:26-32), at TREE
     * granularity: once a tree's flag is 0, workgroups that start afterwards do
     * not evaluate that tree on their samples, so the out / grad rows of a tree
     * with ok == 0 are PARTIALLY WRITTEN (unspecified, as the reference's
     * buffer after its early return, src/Evaluate.jl:350-351; fused losses of
     * such a tree are NaN).  The flags and every row with ok == 1 do not depend
     * on it — nor on the order in which a launch visits its sample tiles (large
     * launches run the tiles with the features' extreme values first).
     * DE_OPT_FULL_EVAL below turns the exit off. */
    DE_OPT_EARLY_EXIT = 1u << 0,
    /* The reference's fused 2/3-node kernels decide WHICH leaves are validity
     * tested and where `Inf` is substituted (src/Evaluate.jl:488-691).  They are
     * on when use_fused=true and the operator count of that degree is <= 15
     * (OPERATOR_LIMIT_BEFORE_SLOWDOWN, src/Evaluate.jl:14,496,607). */
    DE_OPT_FUSE_DEG1 = 1u << 1,
    DE_OPT_FUSE_DEG2 = 1u << 2,
    /* Flag semantics of the Bumper whole-tree path instead
     * (ext/DynamicExpressionsBumperExt.jl:25-36,63): constant leaves tested,
     * feature leaves never tested, every operator result tested, no folding. */
    DE_OPT_BUMPER_CHECKS = 1u << 3,
    /* EvalContext.turbo (the LoopVectorization path, ext/DynamicExpressionsLoopVectorizationExt.jl:24-278): permission
     * to trade the last bits for speed, as the reference's @turbo loops do with SLEEF (their results drift from
     * Base's, test/test_supposition_consistency.jl:106-108).  Float32 eval_tree_array only: `/` = x * v_rcp_f32(y),
     * exp = v_exp_f32 + one correction FMA, cos/sin = two-term pi + degree-9 polynomial without the exact-extremum
     * select and without the Payne-Hanek path — <= 1e-6 relative on ordinary arguments (north_star: 1e-5), flags
     * identical except through the documented domain edges (csrc/de_device_ops.h).  Float64, the
     * gradient entry points and wide-X programs ignore the bit (they run the exact operators). */
    DE_OPT_TURBO = 1u << 4,
    /* Evaluate every tree on every sample even after it is known to be incomplete (no early exit at tree granularity): the
     * rows of an incomplete tree then hold the values the non-finite intermediates propagate to.  Same flags, same rows where
     * ok == 1; costs the evaluation of trees whose results nobody may read (55 % of the benchmark's random population). */
    DE_OPT_FULL_EVAL = 1u << 5,
    /* Round 5's spelling of what is the DEFAULT since ABI 3 (kept so that callers written for ABI 2 still compile and mean the same):
     * de_eval_loss_grad / de_eval_loss_grad_by_class by forward-mode duals, whatever the gradient width.  Wins over DE_OPT_REVERSE_GRAD. */
    DE_OPT_FORWARD_GRAD = 1u << 6,
    /* PERMISSION to compute de_eval_loss_grad / de_eval_loss_grad_by_class by REVERSE accumulation (two sweeps whatever the number of
     * gradient rows: the library uses it from 8 gradient rows per tree on, where it is faster — C5 pullback 13 ms against 30 ms).  Like
     * DE_OPT_TURBO it trades the letter of the reference for speed, here in the FLAG: the reference is forward-mode
     * (src/EvaluateDerivative.jl:230-243,340-365) and reverse accumulation associates the products of a gradient entry leaf-wards instead of
     * root-wards — entries agree with the forward Jacobian to rounding, but a product chain that overflows in ONE association only flips
     * `ok` (~0.03 % of Float32 fuzz cases, never seen in Float64).  Without the bit (the default since ABI 3, VERDICT r5
     * item 4) every fused loss gradient runs forward duals: the reference's flag semantics exactly. */
    DE_OPT_REVERSE_GRAD = 1u << 7,
    /* Float16 forward-mode gradients.  Means something for dtype == DE_F16 only, every other dtype ignores it.  A
     * DE_F16 program created with it (de_program_create, de_program_create_cse; de_program_update keeps a program's options) is served
     * by de_eval_grad — all three modes, with or without `out`, packed or caller-supplied grad_offsets, host or device pointers — and by
     * de_eval_diff: Julia's Float16 arithmetic through grad_degn_eval, every value, partial and chain-rule operation rounded to binary16.
     * X, the constants, the parameters, out and grad are binary16; offsets and ld_out count binary16 elements.  Every other entry point
     * that refuses DE_F16 keeps refusing it, with the same text.  The gradient program of a de_program_create_cse program with the bit
     * is lowered from the EXPANDED tape: every occurrence of a shared constant has a row of its own that holds its own partial. */
    DE_OPT_F16_GRAD = 1u << 8,
    /* Fused losses of Float16 and complex programs.  Means something for dtype == DE_F16 / DE_CF32 / DE_CF64 only,
     * DE_F32 / DE_F64 ignore it.  A program created with it is served by de_eval_loss and de_eval_loss_ex for DE_LOSS_L2 and DE_LOSS_L1
     * (any other kind: DE_ERR_UNSUPPORTED, de_last_error names the kind and the element type, no output touched); the buffer types are
     * in the table at de_eval_loss.  Every other entry point that refuses these programs keeps refusing them, with the same text. */
    DE_OPT_TYPED_LOSS = 1u << 9,
    DE_OPT_DEFAULT = (1u << 0) | (1u << 1) | (1u << 2)
};

/* One node of a flattened tree.  A tree is the POST-ORDER sequence of its nodes
 * (children left to right, then the node; traversal order of tree_mapreduce,
 * src/base.jl:123-158).  This mirrors Node{T,D}'s fields degree/op/feature
 * (src/Node.jl:74-90) with 0-based indices. */
typedef struct de_tape_node {
    uint8_t degree; /* 0 = leaf, 1..3 = operator arity                               */
    uint8_t op;     /* degree 0: enum de_leaf_kind; degree >= 1: enum de_opcode      */
    uint16_t arg;   /* leaf: const slot / feature row / param row (0-based); op: 0  */
} de_tape_node_t;

typedef struct de_ctx de_ctx_t;
typedef struct de_program de_program_t;

/* ---- library / registry ------------------------------------------------- */
int de_abi_version(void);
int de_opcode_table_version(void);
/* Julia function name + degree -> opcode id, or -1 (=> caller keeps CPU path).
 * Names are the Julia spellings: "cos", "exp", "+", "-", "*", "/", "^", "max",
 * "safe_log", "custom_cos", "pow_abs2", "fma", ...; unary minus is ("-", 1). */
int de_opcode_by_name(const char *name, int degree);
/* Inverse of the above; NULL if `opcode` is not in the table. */
const char *de_opcode_name(int opcode);
int de_opcode_degree(int opcode); /* 1, 2, 3 or -1 */
const char *de_status_string(int status);

/* ---- context -------------------------------------------------------------- */
/* `stream` is a hipStream_t to launch on (caller keeps ownership), DE_STREAM_NULL
 * for HIP's null (legacy default) stream — what torch.cuda.current_stream() is
 * unless the caller switched streams — or NULL to let the context create and own
 * a non-blocking stream.  Work is ordered with the caller's other work only if
 * it is submitted to the same stream. */
#define DE_STREAM_NULL ((void *)(intptr_t)-1)
int de_ctx_create(int device, void *stream, de_ctx_t **out_ctx);
int de_ctx_destroy(de_ctx_t *ctx);
/* Launch on another caller-owned stream (or DE_STREAM_NULL) from now on.  The new stream is ordered behind
 * everything the context queued on the old one (its scratch buffers are shared); a stream the context created
 * itself is drained and destroyed.  Cheap when `stream` is already the current one: shims call it before every
 * de_* call with the caller's current stream (torch.cuda.current_stream(), AMDGPU.stream()). */
int de_ctx_set_stream(de_ctx_t *ctx, void *stream);
int de_ctx_synchronize(de_ctx_t *ctx);
/* Release what the context retains between programs (round 6): a destroyed program parks its host vectors (<= 4 shells, <= 512 MB) and its
 * device streams (<= 12 buffers / 256 MB, + 64 small ones) with the context so that the next de_program_create of a search loop allocates
 * nothing; host-pointer calls keep their staging scratch.  de_ctx_trim synchronises the stream and frees all of it (the context stays
 * usable); de_ctx_destroy does the same.  DE_NO_PROG_RECYCLE=1 in the environment turns the retention off altogether. */
int de_ctx_trim(de_ctx_t *ctx);
/* Declare a DEVICE-resident feature matrix that does not change between calls (the X of a search: thousands of de_eval* calls on one
 * matrix): the library computes its per-dataset statistics — the 3 F priority-tile keys of large early-exit launches, one pass over
 * X — here, once, and every later call on this context with the same (X, N, ldX) skips its own pass.  The caller must re-declare (or
 * pass X = NULL to withdraw) before it modifies X.  Results never depend on it (the keys only decide which sample tiles run first). */
int de_ctx_declare_dataset(de_ctx_t *ctx, int dtype, const void *X, int64_t N, int64_t ldX, int32_t n_features);
void *de_ctx_stream(de_ctx_t *ctx);
int de_ctx_device(de_ctx_t *ctx); /* the device index the context was created on (-1: null) */
const char *de_last_error(de_ctx_t *ctx); /* text of the last failure on this ctx */

/* ---- population program --------------------------------------------------- */
/* Validate and lower a population of `n_trees` tapes into the device program.
 *   nodes         all tapes concatenated; tree t = nodes[node_offsets[t] ..
 *                 node_offsets[t+1])
 *   consts        all constant pools concatenated (dtype elements); tree t's
 *                 slot i = consts[const_offsets[t] + i]; slots are in
 *                 depth-first left-to-right leaf order — the row order of the
 *                 constant gradient (index_constant_nodes,
 *                 src/NodeUtils.jl:184-201)
 *   n_features    rows of X; n_params: rows of the parameter matrix (0 for
 *                 plain Node trees)
 * Host pointers only (tapes are host data structures).  Nothing is retained. */
int de_program_create(de_ctx_t *ctx, int dtype, const de_tape_node_t *nodes,
                      const int64_t *node_offsets, int64_t n_trees, const void *consts,
                      const int64_t *const_offsets, int32_t n_features, int32_t n_params,
                      uint32_t options, de_program_t **out_program);
/* The same with a second, CSE tape per tree for GraphNode expressions (shared subtrees, src/Node.jl:138-166).  The
 * reference evaluates a shared node once PER PARENT (its recursion has no cache); `nodes` is therefore the EXPANDED tape,
 * exactly as for de_program_create — gradients, constants and flags follow it — and `cse_nodes` (tree t =
 * cse_nodes[cse_offsets[t] .. cse_offsets[t+1]); an empty range = no sharing) restates the same tree with every shared,
 * non-constant operator subtree present ONCE: its post-order slice followed by a DE_OP_SHARE marker at the first
 * occurrence, one DE_LEAF_SHARED leaf at every later one (include/de_opcodes.h).  Constant leaves of the CSE tape use
 * the slot numbers of their first occurrence in the expanded tape (the host keeps all occurrence slots of a shared constant
 * equal).  The eval program (de_eval, de_eval_loss) is lowered from the CSE tape: the shared value is computed once per
 * tape into a persistent LDS row and re-read — bit-identical values and flags, fewer dispatches.  So are, since round 3, the
 * programs of de_eval_grad / de_eval_diff / de_eval_loss_grad: values, flags and the Jacobian rows of features and parameters
 * are the expansion's bit for bit; a constant INSIDE a shared subtree gets every consumer's contribution in the gradient row of
 * its FIRST occurrence slot and zeros in the rows of its later occurrence slots (n_grad is unchanged: sum the occurrence rows
 * of a shared constant, as before — the totals are the expansion's to rounding).  Reverse accumulation (de_eval_loss_grad's default
 * from 8 gradient rows per tree on) runs over shared rows too since round 4: the backward sweep accumulates the adjoints of a row's
 * consumers (DE_REV_NO_SHARED=1: forward duals for such programs; ternary operators with shared operands always fall back).  Share ids are 0, 1, ... in order of definition, at most 16 minus the tree's spill slots; a shared subtree must not
 * be the root or a direct child of a ternary operator — a tree whose CSE form does not fit runs from its expanded tape (that
 * tree alone).  DE_NO_CSE=1 ignores the CSE tapes, DE_NO_GRAD_CSE=1 only for the gradient programs. */
int de_program_create_cse(de_ctx_t *ctx, int dtype, const de_tape_node_t *nodes, const int64_t *node_offsets,
                          const de_tape_node_t *cse_nodes, const int64_t *cse_offsets, int64_t n_trees,
                          const void *consts, const int64_t *const_offsets, int32_t n_features,
                          int32_t n_params, uint32_t options, de_program_t **out_program);
/* Replace all constants (same counts, same order) without re-flattening: the
 * optimiser inner loop of get/set_scalar_constants (src/NodeUtils.jl:99-143). */
int de_program_set_consts(de_program_t *prog, const void *consts);
/* The same from a DEVICE buffer: d_consts holds the program's constants in its element type, in
 * de_program_set_consts' order.  It is read in stream order on the context's stream — the first thing queued is a device-to-device
 * copy into a buffer the program owns, so the caller may reuse d_consts once the stream has passed that point.  Afterwards every entry
 * point behaves exactly as if de_program_set_consts had been called with the same values (outputs, flags, de_program_stream_hash,
 * de_program_dump, a later de_program_update: the same bits).
 *   - DE_F32 / DE_F64 programs whose streams are patched in place take the DEVICE PATH: the constants are scattered into every
 *     device stream, the constant subtrees re-evaluated and the per-tree flags recomputed by kernels on the context's stream.  From the
 *     second call on nothing is copied to or from the host and the stream is never synchronised; the host copies follow lazily, when
 *     an entry point needs them (de_program_update, _verify, _dump, _stream_hash, the first gradient call that builds a stream ...).
 *   - Every other program (DE_F16, complex, turbo, a constant subtree deeper than the fold kernel's stack, DE_NO_CONST_PATCH=1) is
 *     STAGED: one device-to-host copy, then de_program_set_consts.  The call never fails for being unsupported;
 *     de_program_consts_device_path tells which path ran.
 *   - DE_ERR_INVALID_ARG: prog is null; d_consts is null while the program has constants; d_consts is a host pointer (the message
 *     names de_program_set_consts).  A program without constants returns DE_OK and launches nothing. */
int de_program_set_consts_device(de_program_t *prog, const void *d_consts);
/* The current constants (de_program_set_consts' layout and element type) to a host or device buffer, from whichever side is current. */
int de_program_get_consts(de_program_t *prog, void *out);
/* 1: the last de_program_set_consts_device ran on the device path; 0: it was staged through the host (or the constants were last set
 * by de_program_create / de_program_set_consts / de_program_update); -1: prog is null. */
int de_program_consts_device_path(const de_program_t *prog);
/* Replace trees tree_ids[0 .. n_update) of `prog` with the n_update trees given in de_program_create's layout
 * (nodes / node_offsets / consts / const_offsets describe the NEW trees only, in the order of tree_ids).
 * cse_nodes / cse_offsets may be NULL (no sharing in the new trees), else as de_program_create_cse.
 * The population keeps its size, its order, dtype, n_features, n_params and options.  Afterwards the program is
 * indistinguishable from a fresh creation of the resulting population: every entry point returns the same bits,
 * de_program_stream_hash is equal, de_program_n_grad / _n_nodes / _dump agree.  On any error the program is unchanged.
 *   - Everything is checked before anything changes: DE_ERR_INVALID_ARG for a duplicate id, a null buffer when n_update > 0
 *     or offsets that are not monotone; DE_ERR_OUT_OF_RANGE for an id outside [0, n_trees) or a feature / parameter index at or
 *     above the counts the program was created with; DE_ERR_BAD_TAPE / DE_ERR_UNSUPPORTED_OP as de_program_create returns them
 *     (a complex program names the refused opcode in de_last_error, as at creation).
 *   - n_update == 0 is a no-op and returns DE_OK.
 *   - A tree's constant count may change: the constant vector is renumbered as a fresh creation numbers it, and
 *     de_program_set_consts afterwards takes the new total.
 *   - Every dtype is accepted.  DE_F32 / DE_F64 programs lower only the new trees and copy every other tree's code; DE_F16 and
 *     complex programs are rebuilt whole from the retained population (same result).
 *   - Stream ordering as de_program_set_consts: work already queued on the context's stream that reads the program completes
 *     with the old trees (the call synchronises the stream before it releases them).
 *   - A hipGraph / torch.cuda.graph that captured a launch of this program names device buffers the update releases: it must
 *     be re-captured after an update, exactly as after de_program_destroy.  Never replay such a graph. */
int de_program_update(de_program_t *prog, const int64_t *tree_ids, int64_t n_update,
                      const de_tape_node_t *nodes, const int64_t *node_offsets,
                      const de_tape_node_t *cse_nodes, const int64_t *cse_offsets,
                      const void *consts, const int64_t *const_offsets);
int de_program_destroy(de_program_t *prog);
int64_t de_program_n_trees(const de_program_t *prog);
/* Sum over trees of count_nodes (src/base.jl:271-280): the node-evals unit. */
int64_t de_program_n_nodes(const de_program_t *prog);
/* n_grad of tree t in `mode` (src/EvaluateDerivative.jl:204-210). */
int64_t de_program_n_grad(const de_program_t *prog, int64_t tree, int mode);
/* Debug/test hook: copy the lowered instruction words of tree t into `words`
 * (capacity `cap` 32-bit words); returns the number of words, or -status.
 * which: 0 generic program, 1 metadata (n_slots, host_ok_eval, host_ok_grad, uses_params and,
 * with cap >= 5, the waves per workgroup the eval kernel runs this program with), 2 bound
 * program, 3 fused (superinstruction) program of the threaded eval kernel (0 words when that
 * kernel is not in use), 4 the fused program with the handler ids of the assured stream (0 words
 * when the program has none), 5 the same with the ids of its TIGHT tier (0 words when the program
 * has one tier).  Metadata with cap >= 7 adds: the program has an assured stream, and the launches
 * use it (0 behind de_program_set_consts_device until the host sees the constants); with cap >= 8:
 * the number of assured tiers (0, 1, 2). */
int64_t de_program_dump(const de_program_t *prog, int64_t tree, uint32_t *words, int64_t cap,
                        int which);

/* Program sanitizer: walk every instruction stream of the program on the host and check each field against the bounds
 * the launches allocate (operand rows, spill slots, LDS byte offsets, handler addresses against the device's handler
 * table, end records).  Returns DE_OK, or DE_ERR_BAD_TAPE with the offending (tree, instruction) in de_last_error.
 * With DE_VERIFY=1 in the environment it runs after every de_program_create / de_program_set_consts (debug builds of a
 * caller, CI).  The kernels themselves clamp class ids and never read outside the caller's X / out extents
 * (samples past N are clamped to N - 1 and not stored). */
int de_program_verify(const de_program_t *prog);

/* Test hook: a 64-bit hash over every host-side stream and table de_program_create built for this program (and its auxiliary
 * program of constant subtrees).  The per-tree passes of a creation run on a pool of host threads (DE_HOST_THREADS caps them,
 * 1 = serial) and must build exactly what one thread builds: equal hashes, whatever the thread count.  0 for a null program. */
uint64_t de_program_stream_hash(const de_program_t *prog);

/* Host-only test hook (no HIP call): runs n items over the pool of host threads the per-tree passes of de_program_create use and
 * returns how many were visited exactly once (== n); *n_ranges (may be NULL) = the ranges they were split into.  The pool is one per
 * process, its threads are detached; a fork()ed child starts a pool of its own. */
int64_t de_host_pool_selftest(int64_t n, int32_t *n_ranges);

/* Host-only hook (makes no HIP call, works without a GPU): lower ONE tape and
 * return its instruction words (4 x uint32 each, csrc/de_program.h) in `words`
 * (capacity `cap` words).  meta[4] = {spill slots, host part of the eval flag,
 * host part of the gradient flag, uses parameters}.  Returns the number of words
 * or -status.  Used by the CPU unit tests of the lowering. */
int64_t de_lower_tape(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts,
                      int64_t n_consts, int32_t n_features, int32_t n_params, uint32_t options,
                      uint32_t *words, int64_t cap, int32_t *meta);
/* Same, for the later host stages of the eval program: stage 2 = bound instructions
 * (csrc/de_bind.h), stage 3 = fused superinstructions of the threaded kernel.  Host-only. */
int64_t de_lower_tape_stage(int dtype, const de_tape_node_t *nodes, int64_t n_nodes,
                            const void *consts, int64_t n_consts, int32_t n_features,
                            int32_t n_params, uint32_t options, int stage, uint32_t *words,
                            int64_t cap);
/* Stage 4 (DE_F32 only): the stage-3 words with the handler ids of the ASSURED stream — the same records, a
 * validity test that cannot fire while every feature value has 2^-39 <= |x| <= DE_ASSURED_XMAX (default 64) left out by naming the
 * untested twin of the instruction's handler.  de_lower_tape_assured returns what decides it: per fused instruction six doubles
 * {lo, hi, amin, finite, id, bits} — the interval [lo, hi] and the lower bound amin of |value| of the accumulator behind the
 * instruction (meaningful when finite == 1), the assured handler id and the elision bits (1: the result's validity test, 2: the row
 * operand's, 4: the cos / exp range pre-test, 8 / 16: the division range test of the accumulator / row operand) with every part of
 * the first three parts of the pass on; stage 4 applies the parts a program would (DE_ASSURED_PARTS, default 31 = every part).
 * Returns the number of doubles or -status.  Host-only. */
int64_t de_lower_tape_assured(const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                              int32_t n_features, uint32_t options, double xmax, double *out, int64_t cap);
/* ... with the parts of the pass named by the caller: a mask of 1 validity tests, 2 cos / exp pre-tests, 4 division halves of the plain
 * forms, 8 the TOP_BIN2 divisions and the feature bound 2^-39, 16 the end-fused last instruction (bits 32 / 64 of the elision bits: the
 * range test of row A / row B of a TOP_BIN2 division).  de_lower_tape_assured is parts = 7. */
int64_t de_lower_tape_assured_parts(const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                                    int32_t n_features, uint32_t options, double xmax, uint32_t parts, double *out, int64_t cap);
/* ... and with the feature fact named by the caller: every feature value finite with amin <= |x| <= xmax (2^-40 <= amin <= xmax).  The pass
 * of a program's TIGHT assured tier (DE_ASSURED_TIGHT_XMAX = 8, DE_ASSURED_TIGHT_AMIN = 2^-19 by default; de_program_dump stage 5), which names
 * the same twin ids and elides a superset of the wide fact's tests.  de_lower_tape_assured_parts is amin = 2^-39 with part 8, 2^-40 without. */
int64_t de_lower_tape_assured_fact(const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                                   int32_t n_features, uint32_t options, double xmax, double amin, uint32_t parts, double *out, int64_t cap);
/* The two hooks above take the real dtypes (DE_F32, DE_F64, DE_F16) and answer -DE_ERR_INVALID_ARG for any other code; complex tapes
 * (DE_CF32 / DE_CF64, interleaved (re, im) constants) lower through these two, which take nothing else.  The generic words carry, for a
 * constant operand, the index of its (re, im) pair in the program's constant table (slot k of the tape: index k) instead of its value. */
int64_t de_lower_tape_complex(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts,
                              int64_t n_consts, int32_t n_features, int32_t n_params, uint32_t options,
                              uint32_t *words, int64_t cap, int32_t *meta);
int64_t de_lower_tape_stage_complex(int dtype, const de_tape_node_t *nodes, int64_t n_nodes,
                                    const void *consts, int64_t n_consts, int32_t n_features,
                                    int32_t n_params, uint32_t options, int stage, uint32_t *words,
                                    int64_t cap);
/* MEMO ROWS.  In a compacted store launch of a Float32 program with assured streams the first tree of a chunk that
 * evaluates cos(x_f) / exp(x_f) leaves the vector in a register row of the chain and the trees behind it copy it: same bits, fewer
 * instructions.  de_memo_rows_max(): the rows the library's eval kernel has (build macro DE_MEMO_ROWS + 2; 0: none).
 * de_memo_rows_assign (host-only): the choice a program makes — over n_instr instructions of stage-4 words (de_lower_tape_stage, any
 * number of trees behind each other) the n_rows (<= 6) most frequent (operator, feature) pairs among the untested cos / exp of a feature
 * row, ties to the smaller (operator, feature); row r: k[r] (0 cos, 1 exp), feat[r] (0-based), uses[r].  Returns the rows given out or
 * -status.  de_program_memo_rows: the same for a program (its tightest assured tier; 0 rows without assured streams).
 * de_program_last_memo_named: named[r] (6 entries) = the records of the tightest tier's compact stream the most recent eval launch handed
 * to row r's memo handlers; -1 everywhere when it did not compact.  DE_MEMO=0 (read at launch): no record is handed over. */
int32_t de_memo_rows_max(void);
int32_t de_memo_rows_assign(const uint32_t *words, int64_t n_instr, int32_t n_features, int32_t n_rows, int32_t *k, int32_t *feat, int64_t *uses);
int32_t de_program_memo_rows(const de_program_t *prog, int32_t *k, int32_t *feat, int64_t *uses);
int de_program_last_memo_named(de_program_t *prog, int64_t *named);
/* Host-only hook of the GRADIENT streams (csrc/de_grad_encode.h; DE_F32 / DE_F64 only): the tape lowered and bound as the gradient entry
 * points do (unfolded, every tested value tested), then encoded for `mode` (DE_GRAD_*) against an identity handler table, so that the
 * handler word of a record is a plain gop_* / ROP_* id of csrc/de_bind.h (successor-rotated, as the kernels read it).
 * form 0: forward duals; 1: the same with two samples per lane allowed; 2: with shared leaf rows (the four stream variants one behind
 * the other); 3: reverse accumulation.  meta[8] — forward: {window width GC, samples per lane, windows, spill slots, records per variant,
 * variants}; reverse: {first backward record, partial + accumulation rows, staged columns, LDS rows per wave, spill slots}; both: meta[6] =
 * constants whose site (the record de_program_set_consts patches) holds their bits, meta[7] = a hash of the constant-site table.  Returns the number of words, 0 when the tree has
 * no such stream (the flat kernel / the forward duals run it), or -status. */
int64_t de_lower_tape_grad(int dtype, const de_tape_node_t *nodes, int64_t n_nodes, const void *consts, int64_t n_consts,
                           int32_t n_features, int32_t n_params, uint32_t options, int mode, int form, uint32_t *words,
                           int64_t cap, int32_t *meta);
/* Host-only hook (no HIP call) of the per-tree parameter entry points below: rewrite ONE post-order tape so that every
 * DE_LEAF_CONST and every DE_LEAF_PARAM leaf becomes a DE_LEAF_CONST whose slot is its ordinal among those leaves in tape order (the
 * depth-first constant order de_program_create requires); every other node is copied.  slot_param[s] = -1 for a real constant, else the
 * 0-based parameter row of slot s; a parameter that occurs twice gets two slots with the same row; a tape without parameters comes back
 * unchanged.  out_nodes has room for n_nodes nodes (it may be `nodes` itself), slot_param for `cap` entries.  Returns the number of
 * slots, or -status: DE_ERR_INVALID_ARG for a null pointer, a negative count or more slots than `cap`; DE_ERR_OUT_OF_RANGE for a
 * parameter row >= n_params; DE_ERR_UNSUPPORTED for a DE_LEAF_SHARED or DE_OP_SHARE node (CSE tapes are not served). */
int64_t de_tape_params_to_consts(const de_tape_node_t *nodes, int64_t n_nodes, int32_t n_params, de_tape_node_t *out_nodes,
                                 int32_t *slot_param, int64_t cap);

/* ---- evaluation ------------------------------------------------------------ */
/* Optional per-call inputs of a parametric population
 * (src/ParametricExpression.jl:371-390): value of PARAM leaf p at sample j is
 * params[p + ld_params*(classes[j]-class_base)].  Every class id must lie in
 * [class_base, class_base + n_classes): the reference asserts this on the host
 * (`@assert maximum(classes) <= size(parameters, 2)`, :378-379) and so must the caller's shim —
 * the kernels index `params` with the ids as given. */
typedef struct de_param_args {
    const void *params;     /* [n_params, n_classes] column-major, dtype elements */
    int64_t ld_params;      /* >= n_params                                          */
    int64_t n_classes;
    const void *classes;    /* N class ids                                           */
    int32_t classes_is_i64; /* 0: int32 ids, 1: int64 ids (Julia Vector{Int})        */
    int32_t class_base;     /* 1 for Julia callers, 0 for C/Python                   */
} de_param_args_t;

/* out[t*ld_out + j] = tree_t(X[:, j]),  ok[t] as described above.
 * `pargs` may be NULL when the program has no PARAM leaves. */
int de_eval(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
            const de_param_args_t *pargs, void *out, int64_t ld_out, uint8_t *ok);

/* The `isfinite(sum(x))` quirk, certified (round 5).  The reference's validity test of an array is isfinite(sum(x))
 * (src/ValueInterface.jl:9); the kernels test every element.  The two agree unless all elements are finite and the SUM overflows — values
 * of ~floatmax / N.  This call evaluates the population once more through a certificate pass (every operator result tested, nothing stored)
 * and reports per tree: ok[t] as de_eval would (host or device array), certified[t] (host) = 1 when the reference's `complete` provably
 * equals ok[t] — some element is non-finite (its sum is too), or N * max|tested value or constant operand| times the summation's rounding
 * margin stays below the largest finite value (1.001 for Float32 / Float64; (1 + 2^-11)^d for DE_F16, d = the depth of Julia's pairwise sum,
 * 1.66 at N = 2049) —, max_abs[t] (host doubles, may be NULL) = that maximum.  Trees with certified[t] == 0 are the only ones whose flag a caller who
 * needs the reference's bit has to re-derive on the CPU.  Programs without DE_OPT_EARLY_EXIT sum nothing: all certified.  Slower than
 * de_eval (the flat-switch kernel): a checker, not the hot path. */
int de_eval_sum_certificate(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                            const de_param_args_t *pargs, uint8_t *ok, uint8_t *certified, double *max_abs);

/* Forward-mode gradient of every tree.  grad holds, for tree t, an
 * [n_grad_t, N] column-major matrix starting at element grad_offsets[t]
 * (host array of n_trees entries), or packed back to back when grad_offsets is
 * NULL.  Row order: VARIABLE: (params,) features; CONSTANT: constant slots;
 * BOTH: (params,) features, then constant slots.  `out` may be NULL. */
int de_eval_grad(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                 const de_param_args_t *pargs, int mode, void *out, int64_t ld_out, void *grad,
                 const int64_t *grad_offsets, uint8_t *ok);

/* Single-direction derivative d tree / d x_direction (0-based feature row):
 * out, dout are [n_trees, N] with row strides ld_out.  `ok` is always 1 as in
 * the reference (no validity test on this path, src/EvaluateDerivative.jl:68-119). */
int de_eval_diff(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                 int32_t direction, void *out, void *dout, int64_t ld_out, uint8_t *ok);

/* ---- fused loss (the consumer either side of the path) --------
 * loss[t] = sum_j w_j * l(tree_t(X[:, j]) - y[j]),  l = abs2 (DE_LOSS_L2) or abs (DE_LOSS_L1) — or, through de_eval_loss_ex, any
 * parameterised kind of the table below;
 * w == NULL means w_j = 1; w_j == 0 excludes sample j.  This is what every consumer of
 * eval_tree_array in the reference's optimisation loop computes right after the call —
 * `sum(abs2, tree(X, operators) .- y)` (test/test_optim.jl:95,99), the objective handed to Optim
 * (ext/DynamicExpressionsOptimExt.jl:86-126) — fused into the evaluation so that the
 * [n_trees, N] output never goes to HBM.  loss[t] is NaN where ok[t] == 0 (the callable sugar
 * NaN-fills incomplete evaluations, src/EvaluationHelpers.jl:29-33).  The reduction order is
 * fixed (per-wavefront partials, then two fixed-order passes in double), so results are
 * reproducible run to run.  `loss` holds n_trees values of the program's dtype.
 *
 * Programs served, and their buffers (y / w hold N elements, loss n_trees):
 *   DE_F32 / DE_F64                        y, w, loss of the dtype; every kind.  The LDS-tiled kernel, or — a feature matrix too wide for
 *                                          its tile, DE_EVAL_THREADED=0 — the flat-switch interpreter's loss variant: the same arithmetic
 *                                          per term, another summation order (each deterministic; the two agree to rounding).
 *   DE_F16 with DE_OPT_TYPED_LOSS          y, w binary16; loss FLOAT32.  Julia's Float16 steps per term: e = r16(yhat - y), L2
 *                                          l = r16(e * e), L1 l = |e|, weighted r16(w * l) (r16: a Float32 result rounded to binary16).
 *                                          The term is the reference's, the SUM is the library's: the binary16 terms are widened exactly
 *                                          and summed in Float32 (a binary16 sum of N terms overflows at 65504) — the stance
 *                                          de_eval_fit_stats takes with its double outputs.  A term that overflows binary16 (|e| >= 256
 *                                          under L2) is +Inf and so is the loss, with ok still 1.
 *   DE_CF32 / DE_CF64 with the option      y interleaved (re, im) pairs; w REAL, loss REAL, both of the component type.  e = yhat - y
 *                                          per component; L2 l = re_e * re_e + im_e * im_e (abs2: two products, one sum, no contraction),
 *                                          L1 l = hypot(re_e, im_e) (abs).
 * DE_F16 / complex programs: DE_LOSS_L2 and DE_LOSS_L1 only (DE_ERR_UNSUPPORTED for another kind); without DE_OPT_TYPED_LOSS they are
 * refused as before.  As for every fused loss, the term claims no bit parity with a CPU library. */
typedef enum de_loss_kind {
    DE_LOSS_L2 = 0,      /* l(e) = e^2,  l'(e) = 2e                                              */
    DE_LOSS_L1 = 1,      /* l(e) = |e|,  l'(e) = sign(e)                                         */
    DE_LOSS_PULLBACK = 2, /* de_eval_loss_grad only: `y` holds a cotangent dY (see there)        */
    /* Parameterised kinds: the *_ex entry points only (de_loss_spec_t below).  e = yhat - y, a = y * yhat (margin kinds; y in
     * {-1, +1} by convention, any real value is accepted), sign(0) = 0, l' = dl/dyhat; every l >= 0.       param            */
    DE_LOSS_HUBER = 16,        /* |e| <= delta ? e^2 / 2 : delta (|e| - delta / 2)                          delta > 0        */
    DE_LOSS_LOGCOSH = 17,      /* log(cosh(e)),  l' = tanh(e)                                               -                */
    DE_LOSS_L1_EPS = 18,       /* max(0, |e| - eps),  l' = |e| > eps ? sign(e) : 0                          eps >= 0         */
    DE_LOSS_L2_EPS = 19,       /* max(0, |e| - eps)^2,  l' = |e| > eps ? 2 sign(e) (|e| - eps) : 0          eps >= 0         */
    DE_LOSS_QUANTILE = 20,     /* e ((e > 0) - tau),  l' = (e > 0) - tau                                    tau in [0, 1]    */
    DE_LOSS_LP = 21,           /* |e|^p,  l' = p sign(e) |e|^(p - 1)                                        p >= 1           */
    DE_LOSS_LOGIT_DIST = 22,   /* 2 log(cosh(e / 2)) = -log(4 exp(e) / (1 + exp(e))^2),  l' = tanh(e / 2)   -                */
    DE_LOSS_LOGIT_MARGIN = 23, /* log(1 + exp(-a)),  l' = -y / (1 + exp(a))                                 -                */
    DE_LOSS_L1_HINGE = 24      /* max(0, 1 - a),  l' = a < 1 ? -y : 0                                       -                */
} de_loss_kind_t;
/* A loss kind and its one scalar parameter.  `param` is converted once, on the host, to the program's element type; the kinds that
 * have no parameter ignore it.  `reserved` must be 0. */
typedef struct de_loss_spec {
    int32_t kind;     /* de_loss_kind_t */
    int32_t reserved;
    double param;
} de_loss_spec_t;
/* DE_OK, or DE_ERR_INVALID_ARG for a null spec, a non-zero `reserved`, an unknown kind, a parameter that is not finite or lies outside the kind's range (see the
 * table), and — with_gradient == 0 — DE_LOSS_PULLBACK, which only the gradient entry points know.  Needs no context and touches no device. */
int de_loss_spec_check(const de_loss_spec_t *spec, int with_gradient);
int de_eval_loss(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                 const de_param_args_t *pargs, const void *y, const void *w, int32_t loss_kind,
                 void *loss, uint8_t *ok);
/* The same with any kind of the enumeration above; de_eval_loss itself accepts DE_LOSS_L2 / DE_LOSS_L1 only and forwards here.  A bad spec is
 * DE_ERR_INVALID_ARG with a de_last_error text that names the kind. */
int de_eval_loss_ex(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                    const de_param_args_t *pargs, const void *y, const void *w, const de_loss_spec_t *spec,
                    void *loss, uint8_t *ok);

/* Per tree, the weighted second-order statistics of its values against y, fused into the evaluation
 * (nothing of size N is written):
 *   W = sum_j w_j     mean_y = sum w y / W        M2_y = sum w (y - mean_y)^2          -> ystats[0..2]
 *   mean_p = sum w yhat / W    M2_p = sum w (yhat - mean_p)^2    C = sum w (yhat - mean_p)(y - mean_y)
 *                                                                                     -> stats[3 t + 0..2]
 * w == NULL: w_j = 1; w_j == 0 excludes sample j (as in de_eval_loss).  stats / ystats are DOUBLE whatever
 * the program's dtype; stats[3t..] is NaN where ok[t] == 0.  W == 0 (N == 0 included): the means are NaN,
 * M2 and C are 0.  Fixed reduction order: reproducible run to run.
 * Pearson's r^2 = C^2 / (M2_p M2_y), the least-squares a + b yhat (b = C / M2_p, a = mean_y - b mean_p) and its
 * residual M2_y - C^2 / M2_p, R^2 and the plain L2 loss are all functions of these.
 * Pointers and parametric populations as for de_eval_loss_ex; DE_F16 / complex programs (with or without DE_OPT_TYPED_LOSS) and
 * programs that do not run the LDS-tiled kernel are DE_ERR_UNSUPPORTED, a null y / stats / ystats / ok DE_ERR_INVALID_ARG, both before
 * any output is touched. */
int de_eval_fit_stats(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                      const de_param_args_t *pargs, const void *y, const void *w,
                      double *stats, double *ystats, uint8_t *ok);

/* Fused loss + its gradient (the pullback of the reduction through eval_grad_tree_array):
 *   loss[t]              = sum_j w_j * l(tree_t(x_j) - y_j)
 *   dloss[off_t + k]     = sum_j w_j * l'(tree_t(x_j) - y_j) * d tree_t(x_j) / d theta_k
 * theta = the gradient rows of `mode` (same order as de_eval_grad).  This is the body of the
 * optimiser callback g!/fg! — `dresult_dy = 2 (yhat - y); G[i] = sum_j dresult_dy[j] * dyhat_dconstants[i, j]`
 * (test/test_optim.jl:42-51,83-96) — and, with DE_LOSS_PULLBACK (`y` = the incoming cotangent dY,
 * l' = dY_j, loss[t] = sum_j w_j dY_j tree_t(x_j)), the `dtree` of the ChainRules pullback
 * (`sum(j -> dconstants_dY[:, j] * dY[j])`, src/ChainRules.jl:56-77) — without materialising the
 * [n_grad, N] Jacobian.  Entries are NaN where ok[t] == 0 (src/ChainRules.jl:62-64).
 * `dloss_offsets` = element offset of each tree's n_grad(t, mode) entries (NULL: packed back to
 * back); `loss` may be NULL.  Same fixed-order reduction as de_eval_loss. */
int de_eval_loss_grad(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                      const de_param_args_t *pargs, int mode, const void *y, const void *w,
                      int32_t loss_kind, void *loss, void *dloss, const int64_t *dloss_offsets,
                      uint8_t *ok);
/* ... with any kind of the enumeration, l' from its table. */
int de_eval_loss_grad_ex(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                         const de_param_args_t *pargs, int mode, const void *y, const void *w,
                         const de_loss_spec_t *spec, void *loss, void *dloss, const int64_t *dloss_offsets,
                         uint8_t *ok);

/* Fused Gauss-Newton normal equations per tree (Levenberg-Marquardt on constants), under L2 (any other kind:
 * de_eval_loss_gn_ex below):
 *   loss[t]                 = sum_j w_j e_j^2,   dloss[off_t + k] = sum_j 2 w_j e_j d_k(j)      (exactly de_eval_loss_grad, DE_LOSS_L2: same bits)
 *   jtj[joff_t + i + G_t k] = sum_j w_j d_i(j) d_k(j)       (G_t x G_t, column-major, BOTH triangles written, exactly symmetric)
 * e_j = tree_t(x_j) - y_j, d_k = d tree_t(x_j) / d theta_k over the gradient rows of `mode`, in de_eval_grad's order,
 * G_t = de_program_n_grad(prog, t, mode).  The Gauss-Newton Hessian of the loss is 2 jtj.  Nothing of size N is written.
 * Pointers, staging and offsets as for de_eval_loss_grad (`loss` may be NULL; offsets are host arrays; jtj_offsets == NULL: packed,
 * G_t^2 entries each; a negative offset is DE_ERR_INVALID_ARG).  w == NULL: weight 1; a weight of 0 excludes the sample.
 * ok[t] is de_eval_loss_grad's forward-dual flag; loss, dloss and jtj of a tree with ok[t] == 0 are NaN.  Always forward duals:
 * DE_OPT_REVERSE_GRAD is ignored by this call.  A tree with G_t > de_gn_max_rows() runs in several windows of dual rows, so its
 * cross-window products exist nowhere: its loss / dloss are filled as usual and its jtj block is NaN — a documented limit, not an
 * error.  DE_F16 / complex programs: DE_ERR_UNSUPPORTED; a null y / dloss / jtj / ok on a non-empty population or a bad mode:
 * DE_ERR_INVALID_ARG; both before any output is touched.  The sums are additive over samples: a caller short of scratch memory
 * (n_tiles x columns x 4 partial sums) may split the samples and add the results. */
int de_eval_loss_gn(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                    const de_param_args_t *pargs, int mode, const void *y, const void *w,
                    void *loss, void *dloss, const int64_t *dloss_offsets,
                    void *jtj, const int64_t *jtj_offsets, uint8_t *ok);
int de_gn_max_rows(void); /* 8 */

/* The fit statistics of de_eval_fit_stats with their gradients: per tree, fused into ONE forward-dual launch,
 *   stats[3 t + 0..2], ystats[0..2]                     de_eval_fit_stats' values, layout and rules (same bounds, not the same bits)
 *   dmom[doff_t + k]           D_k = sum_j w_j d_k(j)                          d mean_p / d theta_k = D_k / W
 *   dmom[doff_t + G_t + k]     P_k = sum_j w_j (yhat_j - mean_p) d_k(j)        d M2_p / d theta_k   = 2 P_k
 *   dmom[doff_t + 2 G_t + k]   Q_k = sum_j w_j (y_j - mean_y) d_k(j)           d C / d theta_k      = Q_k
 *   jtj[joff_t + i + G_t k]    sum_j w_j d_i(j) d_k(j): de_eval_loss_gn's block, bit for bit (jtj == NULL: no matrix wanted)
 * d_k over the gradient rows of `mode` in de_eval_grad's order, G_t = de_program_n_grad(prog, t, mode).  With b = C / M2_p the gradient
 * of the residual of the least-squares a + b yhat is 2 b (b P_k - Q_k), and b^2 (jtj - D D^T / W - P P^T / M2_p) is its Gauss-Newton
 * matrix with (a, b) projected out: the Levenberg-Marquardt step under linear scaling.  stats, ystats and dmom are DOUBLE whatever the
 * dtype; jtj has the program's element type, both triangles written, exactly symmetric.  dmom_offsets == NULL: packed, 3 G_t doubles
 * each; jtj_offsets as for de_eval_loss_gn; a negative offset is DE_ERR_INVALID_ARG.  Pointers may be host or device.  w == NULL:
 * weight 1; a weight of 0 excludes the sample.  ok[t] is de_eval_loss_grad's forward-dual flag (always forward duals:
 * DE_OPT_REVERSE_GRAD is ignored); where ok[t] == 0, stats[3t..], the tree's dmom entries and its jtj block are NaN.  W == 0 (N == 0
 * included): the means are NaN, every second moment, dmom entry and jtj entry 0.  A tree with G_t > de_gn_max_rows() gets stats and dmom
 * as usual and a NaN jtj block.  DE_F16 / complex programs: DE_ERR_UNSUPPORTED; a null y / stats / ystats / dmom / ok on a non-empty
 * population or a bad mode: DE_ERR_INVALID_ARG; both before any output is touched.  Scratch, from the context's pools like the
 * loss: ceil(N / 256) x columns x 4 partial sums of the element type, columns = sum_t [6 + 3 G_t + (jtj && G_t <= 8 ? G_t (G_t + 1) / 2 : 0)],
 * and min(ceil(N / 256), 64) x (n_trees + 4 columns) + 3 ceil(N / 256) + 1 doubles.  Fixed reduction order: reproducible run to run. */
int de_eval_fit_stats_grad(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                           const de_param_args_t *pargs, int mode, const void *y, const void *w,
                           double *stats, double *ystats, double *dmom, const int64_t *dmom_offsets,
                           void *jtj, const int64_t *jtj_offsets, uint8_t *ok);

/* The same under any loss kind that has a curvature: generalised Gauss-Newton / iteratively reweighted least squares.
 *   loss[t], dloss[..]      = de_eval_loss_grad_ex's for the same spec, bit for bit
 *   jtj[joff_t + i + G_t k] = M[i, k] = sum_j w_j c_j d_i(j) d_k(j)
 * c_j >= 0 is the kind's curvature weight of sample j, formed in the element type from e = yhat - y (a = y * yhat for the margin kind),
 * the kind's parameter p and the residual floor f = e_floor, both converted to the element type:
 *   DE_LOSS_L2            1                                          DE_LOSS_L1            1 / (2 max(|e|, f))
 *   DE_LOSS_HUBER         |e| <= delta ? 1/2 : delta / (2 |e|)       DE_LOSS_LOGCOSH       |e| < tau ? 1/2 : tanh(e) / (2 e)
 *   DE_LOSS_L1_EPS        |e| > eps ? 1 / (2 max(|e|, f)) : 0        DE_LOSS_L2_EPS        |e| > eps ? (|e| - eps) / |e| : 0
 *   DE_LOSS_QUANTILE      |(e > 0) - tau_q| / (2 max(|e|, f))        DE_LOSS_LOGIT_DIST    h = e / 2; |h| < tau ? 1/4 : tanh(h) / (4 h)
 *   DE_LOSS_LP            p < 2 ? p max(|e|, f)^(p - 2) / 2 : p |e|^(p - 2) / 2   (exactly 1 at p = 2)
 *   DE_LOSS_LOGIT_MARGIN  y^2 s(a) s(-a) / 2,  s(a) = 1 / (1 + exp(a))
 * (tau = 2^-12 for DE_F32, 2^-27 for DE_F64).  2c is the IRLS weight l'(e) / e of a distance kind and the true l'' of the logistic
 * margin, so (M + lam diag M) delta = -dloss / 2 is the damped step of the kind: for de_gn_lm_step and de_lm_solve_host, H is M.
 * Everything else — offsets, symmetry, NaN fills, zero weights, staging, the refusals for DE_F16 / complex programs — is
 * de_eval_loss_gn's, which is this call with {DE_LOSS_L2, 0, 0} and e_floor = 0.
 *
 * de_gn_spec_check (host only, no context): DE_OK for a spec these calls take; DE_ERR_UNSUPPORTED for DE_LOSS_L1_HINGE (no curvature, and
 * the IRLS weight of a margin is no majoriser); DE_ERR_INVALID_ARG for a null spec, DE_LOSS_PULLBACK, an unknown kind, a parameter
 * outside its range (de_loss_spec_check) and — for DE_LOSS_L1, DE_LOSS_L1_EPS, DE_LOSS_QUANTILE and DE_LOSS_LP with p < 2, the kinds that
 * read the floor — an e_floor that is not finite and > 0.  The other kinds ignore e_floor: any value is accepted.  The entry points
 * apply the same check and, knowing the element type, also refuse a floor that rounds to 0 in it (1e-60 for DE_F32); all of it before
 * any output or constant is touched.  The floor bounds the weight of a sample with a tiny residual; de_fit_consts_lm_ex only takes
 * steps that lower the loss, so it affects how fast a fit proceeds, not what it may return. */
int de_gn_spec_check(const de_loss_spec_t *spec, double e_floor);
int de_eval_loss_gn_ex(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                       const de_param_args_t *pargs, int mode, const void *y, const void *w,
                       const de_loss_spec_t *spec, double e_floor, void *loss, void *dloss, const int64_t *dloss_offsets,
                       void *jtj, const int64_t *jtj_offsets, uint8_t *ok);

/* Levenberg-Marquardt on the constants, on the device.
 *
 * de_gn_lm_step: per tree t with G = n_grad[t] rows the step of Population.fit_constants_lm, all arithmetic in double:
 *   step[off_t .. off_t + G) = delta,  A delta = -g / 2,  A = H + lam[t] diag(diag H)
 * with g = dloss[off_t ..] and H = the G x G block jtj[joff_t ..] (column-major, both triangles present, the lower is read) as
 * de_eval_loss_gn wrote them, solved by a Cholesky factorisation without pivoting (pivot d = A_jj - sum_k L_jk^2).  The step is ZERO
 * where has[t] == 0, G == 0, G > de_gn_max_rows(), lam[t] is not finite, an entry of H, g or delta is not finite, or a pivot has
 * !(d > 0) — a rank-deficient H with lam == 0 gives the zero step (an LU solve may return a huge vector there).  Entries of `step` no
 * tree owns are not written.  n_grad and the offsets are host arrays (NULL offsets: packed, G resp. G^2 entries per tree); dloss / jtj
 * (elements of `dtype`: DE_F32 or DE_F64), has, lam (one double per tree) and step (doubles, dloss layout) are host or device pointers,
 * staged like every other buffer.  With device pointers the call is stream-ordered and does not synchronise.
 *
 * de_lm_solve_host: the same arithmetic for ONE system on the host (no HIP call; H column-major G x G doubles): returns 1 if a step
 * was produced, 0 for the zero step.  The kernel and this hook run one source (csrc/de_lm_solve.h): the same bits.
 *
 * de_fit_consts_lm: the whole loop in one call.  It starts from the constants the program holds (de_program_set_consts[_device]),
 * evaluates as de_eval_loss_gn (mode DE_GRAD_CONSTANT, L2) and then `iters` times: step -> device set of the trial constants
 * T(double(c) + delta) -> evaluation -> per tree  accept = has && has_trial && loss_trial < loss  (has: ok and G <= de_gn_max_rows();
 * a NaN compares false); an accepted tree takes the trial constants, loss, gradient, matrix and flag; lam[t] = accept ?
 * max(lam[t] down, lam_min) : lam[t] up.  It ends with a device set of the accepted constants: the program holds them afterwards,
 * de_program_get_consts returns them and de_eval_loss_grad reproduces loss[t] bit for bit.  loss[t] / ok[t]: the accepted loss and
 * its flag (a tree with ok == 0 at the start, or wider than de_gn_max_rows(), keeps its constants; its loss is de_eval_loss_gn's).
 * history (may be NULL): (iters + 1) x n_trees doubles, row r = the accepted losses after r iterations; n_accept (may be NULL): accepted
 * steps per tree.  X, y, w, loss, ok, history, n_accept: host or device pointers; with device pointers the call synchronises only
 * where de_eval_loss_gn does, and neither a constant nor a gradient nor a matrix reaches the host.  opts == NULL: {10, 0, 1e-3, 10.0,
 * 0.1, 1e-12}.  iters == 0 and N == 0: de_eval_loss_gn's loss and flags, the constants unchanged.
 * Refusals, before any output or constant is touched: DE_ERR_UNSUPPORTED for a DE_F16 / complex program, a program made by
 * de_program_create_cse (its occurrence rows need the S H S^T fold of the caller: the host loop) and a tree whose constant rows differ
 * from its constants; DE_ERR_INVALID_ARG for a null y / ok on a non-empty population, iters < 0, reserved != 0 or a lam0 / up / down /
 * lam_min that is not finite and positive.
 *
 * de_fit_consts_lm_ex: the same loop under any kind de_gn_spec_check admits: every evaluation is de_eval_loss_gn_ex
 * with (spec, e_floor), the step, the accept rule, the trial constants and the history are unchanged, and afterwards
 * de_eval_loss_grad_ex with the same spec reproduces loss[t] bit for bit.  A spec or floor de_gn_spec_check refuses is refused here
 * with the same code, before any output or constant is touched.  de_fit_consts_lm is this call with {DE_LOSS_L2, 0, 0}. */
typedef struct de_lm_opts {
    int32_t iters;
    int32_t reserved; /* 0 */
    double lam0, up, down, lam_min;
} de_lm_opts_t;
int de_gn_lm_step(de_ctx_t *ctx, int dtype, int64_t n_trees, const int32_t *n_grad, const void *dloss, const int64_t *dloss_offsets,
                  const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam, double *step);
int de_fit_consts_lm(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                     const void *y, const void *w, const de_lm_opts_t *opts, void *loss, uint8_t *ok, double *history,
                     int32_t *n_accept);
int de_fit_consts_lm_ex(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                        const void *y, const void *w, const de_loss_spec_t *spec, double e_floor, const de_lm_opts_t *opts,
                        void *loss, uint8_t *ok, double *history, int32_t *n_accept);
int de_lm_solve_host(int G, const double *H, const double *g, double lam, double *step);

/* Gauss-Newton matrices and Levenberg-Marquardt fits for trees of 9 to 32 gradient rows.  Additions: every entry point
 * above keeps its bits, its NaN blocks and de_gn_max_rows() == 8.
 *
 * de_eval_loss_gn_wide: de_eval_loss_gn_ex's arguments, pointers, staging, offsets and stream order.
 *   loss, dloss, ok          de_eval_loss_grad_ex's for the same spec, bit for bit, for every tree
 *   G_t <= 8                 the jtj block of de_eval_loss_gn_ex, bit for bit
 *   8 < G_t <= 32, ok[t]     jtj[joff_t + i + G_t k] = sum_j w_j c_j d_i(j) d_k(j): both triangles written, exactly symmetric, a sample of
 *                            weight zero excluded by a select, the association order ((w c) d_i) d_k (i <= k), c_j the curvature weight of
 *                            de_eval_loss_gn_ex with the same floor rules.  Every product is formed in the element type and summed in
 *                            double in a fixed order (tiles of 64 samples, slices of 1024, chunks): reproducible run to run, and
 *                            |jtj - exact| <= 256 u sum_j |w c d_i d_k| as for the narrow blocks
 *   ok[t] == 0 or G_t > 32   a NaN block; neither is an error
 * The wide trees' rows are formed by de_eval_grad's kernels over chunks of samples in the context's scratch: with R = the sum of their
 * G_t and n_w their number, the default chunk is the largest multiple of 256 with (R + n_w) * chunk * sizeof(element) <= 256 MiB (at
 * least 256 samples); DE_GN_WIDE_CHUNK=<samples> in the environment (rounded up to a multiple of 64) overrides it.  A population without
 * a tree of 9 .. 32 rows, and N == 0 (blocks of 0 for G_t <= 32, NaN where the flag already fails), take de_eval_loss_gn_ex's path with
 * no further launch.  Refusals, before any output is touched: what de_eval_loss_gn_ex refuses, with the same codes, and
 * DE_ERR_UNSUPPORTED for a program made by de_program_create_cse with a shared subtree (one gradient row per occurrence of a shared
 * constant: the caller folds them, S H S^T, and keeps the host loop).
 *
 * de_lm_solve_host_wide: de_lm_solve_host for G in 1 .. 32 — de_lm_solve_host's bits for G <= 8, the same arithmetic without the padding
 * (csrc/de_lm_solve_wide.h: Cholesky in double, every sum over k ascending) for 8 < G <= 32; the zero step and 0 for any other G.
 * de_gn_lm_step_wide: de_gn_lm_step's arguments; a tree with G <= 8 gets de_gn_lm_step's bytes, a tree with 8 < G <= 32 the step of
 * de_lm_solve_host_wide bit for bit (one wave per tree, the matrix in LDS), G > 32 and every other zero-step condition zeros; entries no
 * tree owns are not written.
 * de_fit_consts_lm_wide: de_fit_consts_lm_ex's arguments and loop with has = ok && G <= 32: every evaluation is de_eval_loss_gn_wide, a
 * tree with G <= 8 follows de_fit_consts_lm_ex's trajectory bit for bit (constants, loss, history, n_accept), and afterwards
 * de_eval_loss_grad_ex reproduces loss[t] bit for bit for every tree.  The same refusals; reserved stays 0.
 * Not served: programs with shared subtrees, more than 32 rows.  (de_eval_fit_stats_grad for wide trees: de_eval_fit_stats_grad_wide below.) */
int de_gn_wide_max_rows(void); /* 32 */
int de_eval_loss_gn_wide(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                         const de_param_args_t *pargs, int mode, const void *y, const void *w,
                         const de_loss_spec_t *spec, double e_floor, void *loss, void *dloss, const int64_t *dloss_offsets,
                         void *jtj, const int64_t *jtj_offsets, uint8_t *ok);
int de_lm_solve_host_wide(int G, const double *H, const double *g, double lam, double *step);
int de_gn_lm_step_wide(de_ctx_t *ctx, int dtype, int64_t n_trees, const int32_t *n_grad, const void *dloss, const int64_t *dloss_offsets,
                       const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam, double *step);
int de_fit_consts_lm_wide(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                          const void *y, const void *w, const de_loss_spec_t *spec, double e_floor, const de_lm_opts_t *opts,
                          void *loss, uint8_t *ok, double *history, int32_t *n_accept);

/* Levenberg-Marquardt on the constants under Keijzer's linear scaling a + b * yhat, on the device.  Additions: no
 * entry point above changes what it returns.  The objective is scaled_sse = M2_y - C^2 / M2_p of de_eval_fit_stats, the residual of
 * the best a + b * yhat; (a, b) are projected out of the Gauss-Newton system (variable projection, Kaufman's form).
 *
 * de_lm_project_host: the arithmetic for ONE tree of G rows on the host (no HIP call; csrc/de_lm_project.h, the source the kernel runs:
 * the same bits).  stats = (mean_p, M2_p, C), ystats = (W, mean_y, M2_y), dmom = D | P | Q (3 G doubles) and H (column-major G x G
 * doubles: the block of de_eval_fit_stats_grad converted to double) give, all in double and in this association,
 *   b = C / M2_p,  *sse = M2_y - (C C) / M2_p,  g[k] = (2 b) (b P_k - Q_k),
 *   Ht[i + G k] = (b b) ((H_ik - (D_i D_k) / W) - (P_i P_k) / M2_p)          (the lower triangle computed, mirrored)
 * Returns 1 if the system was formed.  M2_p == 0 or W == 0: g = 0, Ht = 0, *sse = M2_y (NaN where C is NaN), returns 0; NaN
 * statistics propagate (and de_lm_solve_host answers the zero step); a NaN *sse is the quiet NaN 0x7ff8000000000000 on both sides.  G outside 1 .. 8: returns 0, *sse as above, and (G > 8) the G
 * entries of g and G^2 of Ht zero.
 *
 * de_fit_stats_lm_step: per tree t with G = n_grad[t] rows, step[soff_t .. soff_t + G) = de_lm_solve_host(Ht, g, lam[t]) of the
 * projected system above, from the buffers de_eval_fit_stats_grad filled: stats (3 doubles per tree), ystats (3 doubles), dmom (tree t
 * at dmom_offsets[t], 3 G doubles), jtj (elements of `dtype`, the block of tree t at jtj_offsets[t]); NULL offsets: packed.  step is
 * packed (soff_t = the sum of the G before t); sse (may be NULL): one double per tree, its scaled_sse.  The step is ZERO where
 * has[t] == 0, G == 0, G > 8, the system was not formed or de_gn_lm_step's solve answers zero.  n_grad and the offsets are host
 * arrays; every other pointer is host or device, staged as in de_gn_lm_step.  With device pointers the call is stream-ordered and does
 * not synchronise.
 *
 * de_fit_consts_lm_scaled: de_fit_consts_lm's loop with every evaluation de_eval_fit_stats_grad (mode DE_GRAD_CONSTANT, the matrix
 * wanted) and  accept = has && has_trial && sse_trial < sse  on scaled_sse, in double; an accepted tree takes the trial constants,
 * statistics, moments, matrix and flag.  The program holds the accepted constants afterwards.  sse[t] (doubles), stats (may be NULL:
 * 3 doubles per tree — slope C / M2_p and intercept mean_y - slope mean_p without another launch; de_eval_fit_stats_grad at the
 * result reproduces them bit for bit), ystats (may be NULL: 3 doubles), ok, history (may be NULL: (iters + 1) x n_trees doubles of
 * scaled_sse), n_accept (may be NULL): host or device pointers.  opts == NULL: de_fit_consts_lm's defaults.  iters == 0, N == 0 or
 * no constants: the first evaluation's values, every history row equal, the constants untouched.  A tree with ok == 0 at the start or
 * G > 8 keeps its constant bits.  With device pointers it synchronises only where de_eval_fit_stats_grad does.  The refusals are
 * de_fit_consts_lm's (DE_F16 / complex / de_program_create_cse programs, constant rows that differ from the constants:
 * DE_ERR_UNSUPPORTED; a null y / ok / sse on a non-empty population, iters < 0, reserved != 0, a lam0 / up / down / lam_min that is not
 * finite and positive: DE_ERR_INVALID_ARG), before any output or constant is touched.
 * Not served: the scaled fit under non-L2 kinds and for programs made by de_program_create_cse (de_fit_consts_nm_scaled fits those
 * without a gradient; trees of 9 to 32 rows: de_fit_consts_lm_scaled_wide below; these three calls keep their limit of 8); a tree
 * with a constant that is redundant under scaling (an additive or multiplicative constant at the root) has a projected matrix with a
 * zero row: the Cholesky step is zero for every lam and the tree keeps its constants (de_fit_consts_bfgs_scaled and
 * de_fit_consts_nm_scaled, which factor no matrix, fit it). */
int de_lm_project_host(int G, const double *stats, const double *ystats, const double *dmom, const double *H,
                       double *sse, double *g, double *Ht);
int de_fit_stats_lm_step(de_ctx_t *ctx, int dtype, int64_t n_trees, const int32_t *n_grad,
                         const double *stats, const double *ystats, const double *dmom, const int64_t *dmom_offsets,
                         const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam,
                         double *step, double *sse);
int de_fit_consts_lm_scaled(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                            const void *y, const void *w, const de_lm_opts_t *opts,
                            double *sse, double *stats, double *ystats, uint8_t *ok, double *history, int32_t *n_accept);

/* The fit under linear scaling for trees of 9 to 32 gradient rows: the wide route (§4.4.7) and the scaled fit (§4.4.8)
 * joined.  Additions: every entry point above keeps its bits, its NaN blocks, its zero steps and its refusals; de_gn_max_rows() == 8 and
 * de_gn_wide_max_rows() == 32.
 *
 * de_eval_fit_stats_grad_wide: de_eval_fit_stats_grad's arguments, pointers, staging, offsets and stream order.
 *   stats, ystats, dmom, ok  de_eval_fit_stats_grad's, bit for bit, for every tree
 *   G_t <= 8                 the jtj block of de_eval_fit_stats_grad, bit for bit
 *   8 < G_t <= 32, ok[t]     the block de_eval_loss_gn_wide writes for the same population, mode, X, w and {DE_LOSS_L2, 0, 0}, bit for bit:
 *                            the same sub-program, chunk rule (DE_GN_WIDE_CHUNK included), Gram and fold kernels with c = 1, so the same
 *                            bound |jtj - exact| <= 256 u sum_j |w d_i d_k| and the same run-to-run reproducibility
 *   ok[t] == 0 or G_t > 32   a NaN block; neither is an error
 * jtj == NULL (no matrix wanted), a population without a tree of 9 .. 32 rows, and N == 0 (blocks of 0 for G_t <= 32, NaN where the flag
 * already fails) take de_eval_fit_stats_grad's path with no further launch.  Weights that are all zero at N > 0 give wide blocks of exact
 * 0 (the Gram kernel's select excludes every sample).  Refusals, before any output is touched: what de_eval_fit_stats_grad refuses,
 * with the same codes, and DE_ERR_UNSUPPORTED for a program made by de_program_create_cse (one gradient row per occurrence of a shared
 * constant: the caller folds them, S H S^T, and keeps the host loop).  Scratch: de_eval_fit_stats_grad's and de_eval_loss_gn_wide's.
 *
 * de_lm_project_host_wide: de_lm_project_host for G in 1 .. 32 (host only) — de_lm_project_host's bits for G <= 8; for 8 < G <= 32 the
 * same formulas in the same association, in double, with run-time loops (csrc/de_lm_project_wide.h, the source the kernel runs: the same
 * bits), the lower triangle of H read and the result mirrored.  The not-formed rules (M2_p == 0 or W == 0: g = 0, Ht = 0, returns 0),
 * the NaN propagation and the canonical quiet NaN of *sse are de_lm_project_host's.  G > 32: returns 0, *sse as above, the G entries of
 * g and G^2 of Ht zero; G < 1: returns 0.
 *
 * de_fit_stats_lm_step_wide: de_fit_stats_lm_step's arguments.  A tree with G <= 8 gets de_fit_stats_lm_step's bytes, step and sse (that
 * call's kernel runs first).  A tree with 8 < G <= 32 gets, bit for bit, de_lm_solve_host_wide(Ht, g, lam[t]) of
 * de_lm_project_host_wide's system and that hook's sse: one wave per tree, the projection folded into the load of the matrix into LDS,
 * then de_gn_lm_step_wide's Cholesky.  The step is ZERO where has[t] == 0, G == 0, G > 32, the system was not formed or the solve
 * answers zero.  Entries of `step` no tree owns are not written.
 *
 * de_fit_consts_lm_scaled_wide: de_fit_consts_lm_scaled's arguments and loop with has = ok && G <= 32: every evaluation is
 * de_eval_fit_stats_grad_wide, the wide trees' steps are de_fit_stats_lm_step_wide's, a tree with G <= 8 follows
 * de_fit_consts_lm_scaled's trajectory bit for bit (constants, sse, stats, history, n_accept).  Afterwards the program holds the accepted
 * constants and de_eval_fit_stats_grad at the result reproduces stats bit for bit.  Inside the fit no constant, statistic, moment or
 * matrix reaches the host.  The refusals and the iters == 0, N == 0 and no-constants rules are de_fit_consts_lm_scaled's.
 * Not served: the scaled fit under non-L2 kinds, programs made by de_program_create_cse, more than 32 rows. */
int de_eval_fit_stats_grad_wide(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                                const de_param_args_t *pargs, int mode, const void *y, const void *w,
                                double *stats, double *ystats, double *dmom, const int64_t *dmom_offsets,
                                void *jtj, const int64_t *jtj_offsets, uint8_t *ok);
int de_lm_project_host_wide(int G, const double *stats, const double *ystats, const double *dmom, const double *H,
                            double *sse, double *g, double *Ht);
int de_fit_stats_lm_step_wide(de_ctx_t *ctx, int dtype, int64_t n_trees, const int32_t *n_grad,
                              const double *stats, const double *ystats, const double *dmom, const int64_t *dmom_offsets,
                              const void *jtj, const int64_t *jtj_offsets, const uint8_t *has, const double *lam,
                              double *step, double *sse);
int de_fit_consts_lm_scaled_wide(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                                 const void *y, const void *w, const de_lm_opts_t *opts,
                                 double *sse, double *stats, double *ystats, uint8_t *ok, double *history, int32_t *n_accept);

/* BFGS on the constants of a population, on the device — the optimiser the reference tests, optimize(f, g!, tree,
 * BFGS()) of test/test_optim.jl:25,56,104, with de_eval_loss_grad_ex as f and g!.  It needs the loss and its gradient only: no
 * Gauss-Newton matrix, so every kind of de_loss_kind_t that has a gradient is served (DE_LOSS_L1_HINGE included), and every tree of up to
 * de_bfgs_max_rows() = 32 constants through one path.  Per tree, in double, every sum over k ascending, no atomics; B is the tree's
 * approximation of the inverse Hessian (G x G, row-major, exactly symmetric), has = ok && 1 <= G <= 32:
 *   direction  p = -B g, slope = g . p.  !(slope < 0), NaN included: the state is reset — B = I, fresh = 1, p = -g, slope = -g . g and
 *              alpha = a0(g) = |g| > step0 ? step0 / |g| : 1 (the first trial step is no longer than step0).  produced = 0 and p = 0 where
 *              an entry of g or of B (before a reset) is not finite or the slope is still not < 0 (g = 0).
 *   trial      T(double(c_i) + alpha p_i); the bits of c_i where !has or nothing was produced
 *   accept     has && produced && ok_trial && finite(f_trial) && f_trial < f && double(f_trial) <= double(f) + (c1 alpha) slope (Armijo)
 *              accepted: s = double(c_trial) - double(c) (the rounded step actually taken), yv = double(g_trial) - double(g), the update
 *              below, the tree takes the trial constants, loss, gradient and flag, alpha = fresh ? a0(g_trial) : 1, n_accept += 1
 *              rejected: alpha *= shrink, B unchanged
 *   update     sy = s . yv, ss = s . s, yy = yv . yv; only where all three are finite and sy > curv sqrt(ss) sqrt(yy).  From a fresh
 *              state B = (sy / yy) I and fresh = 0 first.  Then u = B yv, yBy = yv . u and
 *              B_ik = B_ik + (((sy + yBy) / (sy sy)) (s_i s_k) - (u_i s_k + s_i u_k) / sy)
 *
 * de_bfgs_direction_host / de_bfgs_update_host: the direction and the update of ONE tree on the host (no HIP call; csrc/de_bfgs.h, the
 * source the kernels run: the same bits).  B: G x G doubles, row-major; fresh, alpha: one entry each, read and (on a reset / an update)
 * written; p: G doubles out, slope: one out.  They return `produced` / `updated`.  G outside 1 .. 32 or a null pointer: 0, the state
 * untouched, the G entries of p zero.
 *
 * de_fit_consts_bfgs: the whole loop in one call.  It starts from the constants the program holds, evaluates de_eval_loss_grad_ex (mode
 * DE_GRAD_CONSTANT, `spec`), then `iters` times: direction, the trial constants set on the device, the evaluation there, accept.
 * Afterwards the program holds the accepted constants and de_eval_loss_grad_ex with the same spec reproduces loss[t] bit for bit.  No
 * constant, gradient or matrix reaches the host; host inputs are staged once; with device pointers the call synchronises only where
 * de_eval_loss_grad_ex does.  X .. w: as de_eval_loss_grad_ex; loss (may be NULL), ok: n_trees entries; history (may be NULL): (iters + 1)
 * x n_trees doubles, row r the accepted losses after r iterations; n_accept (may be NULL): accepted steps per tree; host or device
 * pointers.  opts == NULL: {20, 0, 1.0, 0.5, 1e-4, 1e-8}.  A tree with ok == 0, no constants or more than 32 keeps its constants, its
 * loss is de_eval_loss_grad_ex's.  iters == 0, N == 0 or no constants: nothing is accepted, every history row is the first.
 * Refusals, before any output or constant is touched: DE_ERR_UNSUPPORTED as de_fit_consts_lm (DE_F16 / complex /
 * de_program_create_cse programs, constant rows that differ from the constants); DE_ERR_INVALID_ARG for a spec de_loss_spec_check(spec, 1)
 * refuses, DE_LOSS_PULLBACK (no objective), null y or ok on a non-empty population, iters < 0, reserved != 0, step0 / c1 / curv not
 * finite and positive, shrink outside (0, 1).
 * Not served: programs made by de_program_create_cse, more than 32 constants, parameter rows (the per-tree parameter matrices of
 * §4.4.11 are fitted by de_fit_tree_params_bfgs).  The scaled objective: de_fit_consts_bfgs_scaled below. */
typedef struct de_bfgs_opts {
    int32_t iters;    /* iterations: one direction, one evaluation and one accept each */
    int32_t reserved; /* 0 */
    double step0;     /* the longest first trial step after a reset */
    double shrink;    /* alpha *= shrink on a rejected trial, in (0, 1) */
    double c1;        /* the Armijo constant */
    double curv;      /* the update needs s . yv > curv |s| |yv| */
} de_bfgs_opts_t;
int de_bfgs_max_rows(void);
int de_bfgs_direction_host(int G, double *B, uint8_t *fresh, double *alpha, const double *g, double step0, double *p, double *slope);
int de_bfgs_update_host(int G, double *B, uint8_t *fresh, const double *s, const double *yv, double curv);
int de_fit_consts_bfgs(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                       const void *y, const void *w, const de_loss_spec_t *spec, const de_bfgs_opts_t *opts, void *loss, uint8_t *ok,
                       double *history, int32_t *n_accept);

/* Nelder-Mead on the constants of a population, on the device — what the reference's first tested fit runs:
 * optimize(f, tree) of test/test_optim.jl:6 passes no gradient, so Optim takes its default, NelderMead().  It needs the loss alone
 * (de_eval_loss_ex, the cheapest launch of the library): every kind de_loss_spec_check(spec, 0) admits is served, DE_LOSS_L1_HINGE
 * included; a constant under round / floor / ceil / sign / greater / mod / rem or on the flat side of relu / clamp — whose partial is 0 or
 * NaN almost everywhere — moves; and programs made by de_program_create_cse are served (there are no gradient rows: the constants of tree
 * t are the entries de_program_set_consts takes for it).  The method is a restatement, from the papers, of the steps of Lagarias, Reeds,
 * Wright & Wright (1998) with the adaptive coefficients of Gao & Han (2012) and the affine start simplex; one evaluation per round.
 *
 * State of a tree of G constants, has = ok at the start && 1 <= G <= de_nm_max_rows() = 32, all double: the vertices V[(G + 1) x G]
 * (row-major), f[G + 1], the centroid c[G], the reflected point xr[G], fr, and st[3] = {phase, cursor, l0} (int32).  ROUNDING: every
 * coordinate that is evaluated is first rounded to the program's element type T, and the double of that value is what the state holds;
 * every f is the double of the T loss the evaluation returned, +Inf where it failed (ok == 0 or a loss that is not finite), never NaN.
 * Coefficients: G >= 2: alpha = 1, beta = 1 + 2/G, gamma = 0.75 - 1/(2G), delta = 1 - 1/G; G == 1: 1, 2, 0.5, 0.5.
 * Order: l = argmin f (ties: lowest index), h = argmax f (ties: highest), s = argmax over i != h (ties: highest).
 * A ROUND is one ask (the trial constants), one evaluation, one tell (F = the trial's loss as stored):
 *   phase 0 BUILD(k), k = cursor = 1 .. G   ask: V_k = V_0 but coordinate k - 1 = T((1 + b) V_0[k-1] + a); trial V_k.  tell: f[k] = F;
 *                                           behind k = G: REFLECT.  (V_0: the start constants, f[0] their loss, every other f +Inf.)
 *   phase 1 REFLECT       ask: f_h - f_l <= f_tol |f_l|: DONE.  Else c_j = (sum over i != h, ascending, of V_i[j]) / G and
 *                         xr_j = T(c_j + alpha (c_j - V_h[j])); trial xr.  tell: fr = F; F < f_l: EXPAND; else F < f_s: V_h = xr, f_h = F;
 *                         else F < f_h: CONTRACT_OUT; else CONTRACT_IN.
 *   phase 2 EXPAND        trial T(c + beta (xr - c)).  tell: F < fr: the trial and F go to V_h, f_h; else xr and fr.  REFLECT.
 *   phase 3 CONTRACT_OUT  trial T(c + gamma (xr - c)).  tell: F <= fr: the trial and F go to V_h, f_h, REFLECT; else SHRINK.
 *   phase 4 CONTRACT_IN   trial T(c - gamma (xr - c)).  tell: F < f_h: the trial and F go to V_h, f_h, REFLECT; else SHRINK.
 *   phase 5 SHRINK        l0 = l when the shrink begins; cursor = every i != l0, ascending, one round each:
 *                         ask: V_i[j] = T(V_l0[j] + delta (V_i[j] - V_l0[j])); trial V_i.  tell: f[i] = F; behind the last: REFLECT.
 *   phase 6 DONE          trial: vertex l — the accepted constants.  tell: nothing.
 * After every tell the accepted state of the tree (constants, loss, flag 1) is vertex l of the simplex — where f_l is finite; a tree
 * whose every evaluation failed keeps its start — so the accepted loss never increases; n_improve counts the tells behind which it is
 * strictly smaller.
 *
 * de_nm_ask_host / de_nm_tell_host: one tree's ask / tell on host buffers (no HIP call; csrc/de_nm.h, the source the kernels run: the
 * same bits).  dtype: DE_F32 / DE_F64 (T); opts: a, b and f_tol are read (NULL: the defaults); trial: G elements of T out; f_trial: the
 * double of the loss at the trial, ok_trial its flag.  V (from row 1 on), c, xr and fr need no initial values.  They return 1, or 0 with
 * everything untouched for G outside 1 .. 32, a null pointer, another dtype, or a phase / cursor / l0 outside their ranges.
 *
 * de_fit_consts_nm: the whole loop in one call.  It starts from the constants the program holds, evaluates de_eval_loss_ex (`spec`),
 * then `iters` times: ask, the trial constants set on the device, the evaluation there, tell — `iters` counts rounds behind the first
 * evaluation, BUILD rounds included: a tree of G constants spends its first G rounds on the simplex.  Trees move through the phases at
 * their own pace; every round evaluates exactly one point per tree (a DONE tree and a tree that is not fitted: its accepted constants, bit
 * for bit).  Afterwards the program holds the accepted constants and de_eval_loss_ex with the same spec reproduces loss[t] bit for bit.
 * No constant or loss reaches the host; host inputs are staged once; with device pointers the call synchronises only where
 * de_eval_loss_ex does.  X .. w: as de_eval_loss_ex (pargs: the constants move, the parameters do not); loss (may be NULL), ok: n_trees
 * entries; history (may be NULL): (iters + 1) x n_trees doubles, row r the accepted losses after r rounds, non-increasing; n_improve
 * (may be NULL); host or device pointers.  opts == NULL: {200, 0, 0.025, 0.5, 0.0}.  A tree with ok == 0, no constants or more than 32
 * keeps its constants, its loss is de_eval_loss_ex's.  iters == 0, N == 0 or no constants: nothing moves, every history row is the first.
 * Refusals, before any output or constant is touched: DE_ERR_UNSUPPORTED for DE_F16 / complex programs (and a feature matrix too wide
 * for de_eval_loss_ex); DE_ERR_INVALID_ARG for a spec de_loss_spec_check(spec, 0) refuses, DE_LOSS_PULLBACK, null y or ok on a non-empty
 * population, iters < 0, reserved != 0, a or b not finite or both 0, f_tol negative or not finite.
 * Not served: more than 32 constants per tree, parameter rows.  The scaled objective: de_fit_consts_nm_scaled below. */
typedef struct de_nm_opts {
    int32_t iters;    /* rounds: one ask, one evaluation and one tell each */
    int32_t reserved; /* 0 */
    double a, b;      /* the start simplex: coordinate k - 1 of vertex k is (1 + b) V_0[k-1] + a */
    double f_tol;     /* a tree is DONE where f_h - f_l <= f_tol |f_l| */
} de_nm_opts_t;
int de_nm_max_rows(void);
int de_nm_ask_host(int G, int dtype, const de_nm_opts_t *opts, double *V, const double *f, int32_t *st, double *c, double *xr, void *trial);
int de_nm_tell_host(int G, int dtype, double *V, double *f, int32_t *st, const double *c, const double *xr, double *fr, double f_trial,
                    int ok_trial);
int de_fit_consts_nm(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                     const void *y, const void *w, const de_loss_spec_t *spec, const de_nm_opts_t *opts, void *loss, uint8_t *ok,
                     double *history, int32_t *n_improve);

/* The matrix-free fits under Keijzer's linear scaling a + b yhat: de_fit_consts_bfgs and de_fit_consts_nm with the
 * objective scaled_sse = M2_y - C^2 / M2_p of de_fit_consts_lm_scaled.  Additions: every entry point above keeps its bits, its refusals
 * and its return values.  Objective and gradient stay in double from the statistics to the decision, whatever the program's element type
 * (the constants keep it).
 *
 * de_scaled_objective_host: the objective and its gradient of ONE tree on the host (no HIP call; csrc/de_fit_scaled.h, the source the
 * adapter kernel runs: the same bits).  stats = (mean_p, M2_p, C), ystats = (W, mean_y, M2_y), dmom = D | P | Q (3 G doubles; D is not
 * read).  *sse = de_lm_project_host's (a NaN is the canonical quiet NaN); with b = C / M2_p, g_k = (2 b) (b P_k - Q_k) in that
 * association, de_lm_project_host's g bit for bit.  M2_p == 0 or W == 0: *sse = M2_y (NaN where C is NaN), g = 0, returns 0.  NaN
 * statistics propagate.  It returns 1 where the gradient was formed; G outside 1 .. 32 or a null dmom: 0, the G entries of g zero (G < 1:
 * g is not written); *sse is written whenever stats, ystats and sse are not null.
 *
 * de_fit_consts_bfgs_scaled: de_fit_consts_bfgs's loop — direction, Armijo rule, update of B, alpha rules, options and their defaults —
 * with every evaluation de_eval_fit_stats_grad in mode DE_GRAD_CONSTANT with jtj == NULL (no matrix is formed), f = scaled_sse and g as
 * above, for trees of 1 .. de_bfgs_max_rows() constants through one path.  A tree with a constant that is redundant under scaling (an
 * additive or multiplicative constant at the root), which de_fit_consts_lm_scaled leaves alone, is fitted: B needs no factorisation.
 *
 * de_fit_consts_nm_scaled: de_fit_consts_nm's loop with every evaluation de_eval_fit_stats and f = scaled_sse (the double itself: the
 * state's f is not rounded to the element type).  No gradient rows: programs made by de_program_create_cse are served, and a constant
 * whose partial is zero almost everywhere moves.  It needs the LDS-tiled kernel as de_fit_consts_nm does.
 *
 * Both: sse (doubles), stats (may be NULL: 3 doubles per tree at the returned constants), ystats (may be NULL: 3 doubles), ok, history
 * (may be NULL: (iters + 1) x n_trees doubles of accepted scaled_sse, non-increasing), n_accept / n_improve (may be NULL): host or device
 * pointers.  Where the loop ran, the statistics are those of ONE more evaluation of the fit's own kind behind it, at the accepted
 * constants, which the program holds then: stats equal that evaluation's bit for bit, and sse is their scaled_sse.  iters == 0, N == 0
 * or no constants: the first evaluation's values, every history row equal, the constants untouched.  A tree with ok == 0 at the start,
 * without constants or with more than 32 keeps its constant bits, -0 and NaN payloads included.  With device pointers the calls
 * synchronise only where the evaluation they call does.  Refusals, before any output or constant is touched: de_fit_consts_bfgs_scaled
 * what de_fit_consts_bfgs refuses (DE_F16 / complex / de_program_create_cse programs, constant rows that differ from the constants:
 * DE_ERR_UNSUPPORTED; its options); de_fit_consts_nm_scaled what de_fit_consts_nm refuses (DE_F16 / complex programs, a feature matrix
 * too wide for the LDS-tiled kernel: DE_ERR_UNSUPPORTED; its options); both a null y / ok / sse on a non-empty population
 * (DE_ERR_INVALID_ARG).
 * Not served: non-L2 kinds under scaling, more than 32 constants per tree, parameter rows. */
int de_scaled_objective_host(int G, const double *stats, const double *ystats, const double *dmom, double *sse, double *g);
int de_fit_consts_bfgs_scaled(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                              const void *y, const void *w, const de_bfgs_opts_t *opts,
                              double *sse, double *stats, double *ystats, uint8_t *ok, double *history, int32_t *n_accept);
int de_fit_consts_nm_scaled(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                            const void *y, const void *w, const de_nm_opts_t *opts,
                            double *sse, double *stats, double *ystats, uint8_t *ok, double *history, int32_t *n_improve);

/* Fused loss + gradient of a PARAMETRIC population with the parameter rows reduced BY CLASS:
 *   dparams[(t*n_classes + c)*n_params + p] = sum_{j : class_j = c} w_j l'(e_j) d tree_t(x_j) / d params[p, c]
 * i.e. the gradient w.r.t. the [n_params, n_classes] parameter matrix of tree t (column-major, like
 * `params`) — what Zygote returns for `ex.metadata.parameters` when it differentiates through the
 * reference's gather `parameters[i, classes[j]]` (src/ParametricExpression.jl:381-389; known answer
 * test/test_parametric_expression.jl:326-372; the optimiser's combined vector is
 * vcat(constants, parameters[:]), :260-265).  `mode` is DE_GRAD_VARIABLE or DE_GRAD_BOTH (the modes
 * that have parameter rows); loss / dloss / ok are exactly de_eval_loss_grad's (the parameter rows of
 * dloss hold the sum over all classes).
 *
 * The samples must be GROUPED BY CLASS: class_starts[c] .. class_starts[c+1] (host array of
 * n_classes + 1 sample offsets, class_starts[0] = 0, class_starts[n_classes] = N) holds the samples
 * whose class id is class_base + c.  Classes are part of the dataset, so the shim orders the dataset
 * once (api.py / the Julia extension do).  The call runs one fused pass per class over its sample
 * range — a segmented, fixed-order (reproducible) reduction instead of a scatter with atomics. */
int de_eval_loss_grad_by_class(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                               const de_param_args_t *pargs, int mode, const void *y, const void *w,
                               int32_t loss_kind, const int64_t *class_starts, void *loss, void *dloss,
                               const int64_t *dloss_offsets, void *dparams, uint8_t *ok);
/* ... with any kind of de_loss_kind_t. */
int de_eval_loss_grad_by_class_ex(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                                  const de_param_args_t *pargs, int mode, const void *y, const void *w,
                                  const de_loss_spec_t *spec, const int64_t *class_starts, void *loss, void *dloss,
                                  const int64_t *dloss_offsets, void *dparams, uint8_t *ok);

/* ---- per-tree parameter matrices ---------------------------------------------------------------------------
 * In the reference every ParametricExpression owns its parameter matrix (metadata.parameters, [n_params, n_classes]); the entry points
 * above read ONE matrix for the whole population.  These three serve a population whose trees each carry their own: inside one class
 * segment a parameter is a constant of its tree, so the population is an ORDINARY program (n_params == 0) made from tapes rewritten by
 * de_tape_params_to_consts, in which some constant slots stand for parameters.  The samples are grouped by class (class_starts as for
 * de_eval_loss_grad_by_class).  One call, in stream order on the context's stream:
 *   1. the program's current constants are read into device scratch: the base vector;
 *   2. for every class c with at least one sample, ascending: a kernel forms the class's constant vector (base values in real slots,
 *      params[p, c, tree of the slot] in parameter slots), de_program_set_consts_device installs it, the model entry point (de_eval /
 *      de_eval_loss_ex / de_eval_loss_grad_ex in mode DE_GRAD_CONSTANT) runs on the class's sample range, and a kernel adds the class's
 *      per-tree results into DOUBLE accumulators and ANDs the flags (de_eval_tree_params writes straight into out + class_starts[c]);
 *   3. a last kernel writes the accumulators in the program's element type, NaN where the final ok[t] == 0;
 *   4. the base vector is set back: de_program_get_consts returns the bits it returned before the call.
 * Every returned quantity is a plain sum over samples, so the class segments add.  The order of the additions is fixed (classes
 * ascending, occurrences in slot order, in double): two runs give the same bits.  A class without samples is skipped entirely — its
 * parameter columns are never read (an Inf there clears no flag) and its dparams cells are 0.  ok[t] is the AND over the non-empty
 * classes of the model call's flag.  Host inputs are staged once per call.
 *   de_eval_tree_params            as de_eval: rows of trees with ok[t] == 0 are unspecified (device) / NaN (host buffer)
 *   de_eval_loss_tree_params       as de_eval_loss_ex
 *   de_eval_loss_grad_tree_params  as de_eval_loss_grad_by_class_ex: dloss has the DE_GRAD_CONSTANT layout of the program (every slot;
 *                                  a parameter slot holds its occurrence's sum over all classes), `loss` may be NULL, and
 *                                  dparams[(t*n_classes + c)*n_params + p] = the sum over the occurrences of row p in tree t of that
 *                                  slot's gradient over class c (the layout of de_eval_loss_grad_by_class)
 * Refusals, before any output or constant is touched: DE_ERR_UNSUPPORTED for DE_F16 / complex programs, programs made by
 * de_program_create_cse and programs with n_params != 0; DE_ERR_INVALID_ARG for a null tp / class_starts, a null params or slot_param on
 * a program with constants, reserved != 0, n_params < 0, n_classes <= 0, class_starts not monotone from 0 to N, a slot_param entry
 * outside [-1, n_params), ld_params < n_params and whatever the model entry point refuses (a bad spec, a null y / ok, ...).
 *
 * de_tree_params_accumulate_host: the accumulate-and-finish arithmetic of ONE tree on the host (no HIP call; csrc/de_tree_params.h, the
 * code the kernels run: the same bits).  Inputs in `dtype` (DE_F32 / DE_F64): loss_c[c], dloss_c[c*n_slots + s], ok_c[c] — one model
 * result per class; class_used[c] == 0: class c is skipped, its entries are never read.  Outputs: loss (1), dloss (n_slots),
 * dparams[c*n_params + p], ok (1 byte).  Returns DE_OK or DE_ERR_INVALID_ARG. */
typedef struct de_tree_params {
    const void *params;          /* [n_params, n_classes, n_trees], dtype elements: params[p + ld_params*(c + n_classes*t)]; host or device */
    int64_t ld_params;           /* >= n_params */
    int64_t n_classes;
    int32_t n_params, reserved;  /* reserved = 0 */
    const int64_t *class_starts; /* host, n_classes + 1 sample offsets, as de_eval_loss_grad_by_class */
    const int32_t *slot_param;   /* host, one entry per constant slot of the program in de_program_set_consts' order */
} de_tree_params_t;
int de_eval_tree_params(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                        void *out, int64_t ld_out, uint8_t *ok);
int de_eval_loss_tree_params(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                             const void *y, const void *w, const de_loss_spec_t *spec, void *loss, uint8_t *ok);
int de_eval_loss_grad_tree_params(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                                  const void *y, const void *w, const de_loss_spec_t *spec, void *loss, void *dloss,
                                  const int64_t *dloss_offsets, void *dparams, uint8_t *ok);
int de_tree_params_accumulate_host(int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes,
                                   const uint8_t *class_used, const void *loss_c, const void *dloss_c, const uint8_t *ok_c,
                                   void *loss, void *dloss, void *dparams, uint8_t *ok);

/* ---- BFGS over constants AND parameters of a per-tree parametric population, on the device -------------------
 * The reference fits a ParametricExpression by optimising vcat(constants, parameters[:]) (test/test_parametric_expression.jl:140-199).
 * THE UNKNOWNS of tree t are that vector: its real constant slots (slot_param[s] < 0) in slot order, then all n_params * n_classes
 * entries of its matrix, column-major — unknown n_real + c*n_params + p is params[p, c, t].  Every entry is an unknown, whether a leaf
 * uses it or its class has a sample or not (the gradient of an unused entry is dparams' 0: it never moves).  G_t = n_real_t +
 * n_params*n_classes; a tree is fitted where 1 <= G_t <= de_bfgs_max_rows() and its first evaluation is complete.
 *
 * de_fit_tree_params_bfgs: de_fit_consts_bfgs' loop with de_eval_loss_grad_tree_params as the evaluator.  The real constants start
 * from what the program holds, the parameters from tp->params; the gradient of the vector is double(dloss[real slot]) followed by
 * double(dparams cell); direction, trial T(double(x) + alpha p), Armijo accept, update, has / produced / fresh / alpha / n_accept are
 * those documented at de_fit_consts_bfgs.  Kernels gather the unknowns into packed vectors and scatter the trials back into the base
 * vector and a device-resident parameter block; the tables and host inputs are staged once, the stream is not synchronised inside the
 * iterations and no constant, gradient or parameter reaches the host.  Afterwards:
 *   - the program holds the accepted real constants, its parameter slots their base values again (as de_eval_loss_grad_tree_params
 *     leaves them), after a failure too;
 *   - params_out holds the accepted parameters in tp's layout (ld_params; padding entries are not written); it may be tp->params, a
 *     host or a device pointer, and NULL only when n_params*n_classes*n_trees == 0;
 *   - de_eval_loss_grad_tree_params with params_out reproduces loss[t] bit for bit; a tree that is not fitted keeps every bit of its
 *     constants and parameters;
 *   - loss (may be NULL), ok, history ((iters + 1) x n_trees doubles, may be NULL), n_accept (may be NULL): as de_fit_consts_bfgs.
 * iters == 0, N == 0 or no unknown anywhere: nothing is accepted, every history row is the first.
 * Refusals, before any output, constant or parameter is touched: everything de_eval_loss_grad_tree_params refuses; what
 * de_fit_consts_bfgs refuses about spec and opts (DE_LOSS_PULLBACK, iters < 0, reserved != 0, step0 / c1 / curv not finite and
 * positive, shrink outside (0, 1)); null y or ok on a non-empty population; null tp->params or params_out where a parameter entry exists.
 * Not served: more than 32 unknowns per tree (such a tree keeps every bit here; de_fit_tree_params_lbfgs below fits up to
 * de_lbfgs_max_rows() unknowns), LM / Gauss-Newton over parameters, the scaled objective, per-sample classes.
 *
 * de_tree_params_pack_host / de_tree_params_unpack_host: the index map of ONE tree on the host (no HIP call; csrc/de_tree_params_fit.h,
 * the code the kernels run).  slot_values: n_slots entries (parameter slots are skipped on pack and left untouched on unpack);
 * params_tree: ld_params * n_classes entries (padding is neither read nor written); x: G entries.  pack returns G or -status; unpack
 * returns DE_OK or a status.  A null pointer where one is needed, a negative count, ld_params < n_params or a slot_param entry outside
 * [-1, n_params): DE_ERR_INVALID_ARG, nothing written. */
int de_fit_tree_params_bfgs(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                            const void *y, const void *w, const de_loss_spec_t *spec, const de_bfgs_opts_t *opts, void *params_out,
                            void *loss, uint8_t *ok, double *history, int32_t *n_accept);
int de_tree_params_pack_host(int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes,
                             int64_t ld_params, const void *slot_values, const void *params_tree, void *x);
int de_tree_params_unpack_host(int dtype, int32_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes,
                               int64_t ld_params, const void *x, void *slot_values, void *params_tree);

/* ---- L-BFGS: the two BFGS fits for trees of more than 32 unknowns, on the device -------------------------------
 * B of de_fit_consts_bfgs is G^2 doubles with one lane per row; a member of a parametric population has G = n_real + n_params*n_classes
 * unknowns, which passes 32 with a handful of classes.  Here the curvature of a tree is a ring of up to `memory` pairs (s_j, y_j) with
 * rho_j = 1 / (s_j . y_j) — O(memory * G) — for 1 <= G <= de_lbfgs_max_rows() = 4096, memory in 1 .. de_lbfgs_max_memory() = 16.
 * Per tree, in double, no atomics.  EVERY dot product is 64 partial sums — partial l over k = l, l + 64, ... ascending from 0.0, one
 * product at a time (-ffp-contract=off) — added in the order l = 0 .. 63 from 0.0.  count of the slots are stored, head is the next
 * slot to write; the i-th newest pair is slot (head - 1 - i) mod memory.
 *   direction  q = g; for the stored pairs newest to oldest a_i = rho_i (s_i . q), q -= a_i y_i; r = (s . y / y . y of the newest) q;
 *              oldest to newest b = rho_i (y_i . r), r += (a_i - b) s_i; p = -r, slope = g . p.  count == 0: p = -g.
 *              !(slope < 0): count = 0, p = -g, slope = -g . g, alpha = a0(g).  produced = every entry of g and of the stored pairs
 *              is finite && slope < 0; else p = 0.
 *   trial, accept rule, shrink: those of de_fit_consts_bfgs (trial = T(double(c) + alpha p); Armijo; alpha *= shrink on a reject).
 *   update     on an accepted step s = double(c_trial) - double(c), yv = g_trial - g; only where s . yv > curv |s| |yv| the pair goes to
 *              slot head, rho = 1 / s . yv, head = (head + 1) mod memory, count = min(count + 1, memory); a refused pair leaves every
 *              byte of the state.  Then alpha = count == 0 ? a0(g_new) : 1.
 *
 * de_lbfgs_direction_host / de_lbfgs_update_host: ONE tree on the host (no HIP call; csrc/de_lbfgs.h, the templates the kernels
 * instantiate — the same bits).  S, Y: memory x G doubles, slot j at j*G; rho: memory doubles.  direction returns `produced`, writes p
 * and *slope, and *count / *alpha where the state was reset; update returns `updated`.  G outside 1 .. de_lbfgs_max_rows(), memory
 * outside 1 .. de_lbfgs_max_memory(), *count outside 0 .. memory, *head outside 0 .. memory - 1 or a null pointer: 0, nothing written.
 *
 * de_fit_consts_lbfgs: de_fit_consts_bfgs' contract — arguments, outputs, history, n_accept, where the accepted constants live
 * afterwards, host or device pointers, stream order — with these kernels: a tree is fitted where it has 1 .. de_lbfgs_max_rows()
 * constants and its first evaluation is complete; any other keeps every bit of its constants.  One difference: the call ends with one
 * de_eval_loss_ex at the accepted constants, and loss[t] / ok[t] are that evaluation's — de_eval_loss_ex with the same spec reproduces
 * loss[t] bit for bit.  The history rows stay the losses of the accept rule, de_eval_loss_grad_ex's: that kernel sums a tree's samples
 * in another order, so the last row and loss[t] may differ in the last bits.  (So it also refuses what de_eval_loss_ex refuses: a
 * feature matrix too wide for the LDS-tiled kernel.)
 * de_fit_tree_params_lbfgs: de_fit_tree_params_bfgs' contract likewise (params_out, its padding, the program's constants afterwards).
 * Refusals, before any output, constant or parameter is touched: everything the matching BFGS call refuses (DE_F16 / complex programs,
 * programs made by de_program_create_cse, DE_LOSS_PULLBACK, its option checks, null buffers); memory outside 1 ..
 * de_lbfgs_max_memory(); reserved or reserved2 != 0.  The texts name the call.
 * Not served: the scaled objective, a Wolfe line search, per-sample classes. */
typedef struct de_lbfgs_opts {
    int32_t iters;    /* trial evaluations per tree (>= 0) */
    int32_t reserved; /* 0 */
    int32_t memory;   /* pairs kept per tree, 1 .. de_lbfgs_max_memory() */
    int32_t reserved2; /* 0 */
    double step0, shrink, c1, curv; /* as de_bfgs_opts_t */
} de_lbfgs_opts_t; /* NULL: {20, 0, 8, 0, 1.0, 0.5, 1e-4, 1e-8} */
int de_lbfgs_max_rows(void);
int de_lbfgs_max_memory(void);
int de_lbfgs_direction_host(int G, int memory, const double *S, const double *Y, const double *rho, int32_t *count, int32_t *head,
                            double *alpha, const double *g, double step0, double *p, double *slope);
int de_lbfgs_update_host(int G, int memory, double *S, double *Y, double *rho, int32_t *count, int32_t *head, const double *s,
                         const double *yv, double curv);
int de_fit_consts_lbfgs(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                        const void *y, const void *w, const de_loss_spec_t *spec, const de_lbfgs_opts_t *opts, void *loss, uint8_t *ok,
                        double *history, int32_t *n_accept);
int de_fit_tree_params_lbfgs(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_tree_params_t *tp,
                             const void *y, const void *w, const de_loss_spec_t *spec, const de_lbfgs_opts_t *opts, void *params_out,
                             void *loss, uint8_t *ok, double *history, int32_t *n_accept);

/* ---- tied device fits: a shared GraphNode constant is ONE unknown -------------------------------
 * The library keeps one constant slot and one gradient row per OCCURRENCE of a shared constant (de_program_create_cse), the reference
 * one coordinate per constant (count_constant_nodes and the shared NodeIndex entry, src/NodeUtils.jl:43-51, 184-201).  The calls below
 * are the four device fits with the optimiser kernels running unchanged on vectors of UNIQUE constants; small pack / unpack / fold
 * kernels (csrc/de_ties.hip) sit around every evaluation, whose kernels are unchanged too.
 *
 * tie (host): one int32 per constant slot of the program, in de_program_set_consts order — the 0-based index of the slot's unique
 * constant within its tree, in first-occurrence order (a tree's first slot has id 0, every new id is the largest id before it + 1).
 * U_t = max + 1 unknowns, S_t slots.  NULL: the identity.  In the program's element type T, every sum from +0 in ascending slot order
 * (np.add.at into zeros: a lone -0 row becomes +0):
 *   pack         unique[u] = slots[first slot of u]          (bits: NaN payloads and -0 stay)
 *   unpack       slots[s] = unique[tie[s]]                   (bits)
 *   fold         g_u = sum_{s : tie[s] = u} g_s
 *   fold_matrix  half[u][k] = sum_{s in u} H[s][k], Hu[u][v] = sum_{k in v} half[u][k]      (S H S^T, rows first; column-major blocks)
 * de_ties_*_host: ONE tree on host buffers of `dtype` (no HIP call, no program; csrc/de_ties.h, the code the kernels run — the same
 * bits).  in -> out: pack slots[n_slots] -> unique[U]; unpack unique[U] -> slots[n_slots]; fold g[n_slots] -> g_unique[U]; fold_matrix
 * H[n_slots^2] -> Hu[U^2].  Each returns U; -1 with nothing written for a null pointer, a dtype other than DE_F32 / DE_F64, n_slots < 0
 * or a map that is not in first-occurrence order.
 *
 * de_fit_consts_{bfgs,lbfgs,nm}_tied: the untied twin's signature with `tie` before the outputs; de_fit_consts_lm_tied:
 * de_fit_consts_lm_ex's, serving every kind de_gn_spec_check admits.  The twin's contract, except:
 *   - n_grad, the offsets and the optimiser state are those of the unique constants: BFGS and Nelder-Mead fit a tree with 1 <= U_t <= 32
 *     (S_t may be larger), L-BFGS 1 <= U_t <= de_lbfgs_max_rows(), Levenberg-Marquardt a tree whose occurrence block
 *     de_eval_loss_gn_ex forms (S_t <= de_gn_max_rows()); any other tree keeps its first occurrences' bits.
 *   - the fit starts from pack of the program's constants (the first occurrence decides); where the loop ran, every slot s of every
 *     tree holds the bits of unique[tie[s]] afterwards.  iters == 0, N == 0 or no constants: nothing is written to the program.
 *   - tie == NULL on a program NOT made by de_program_create_cse: the untied twin bit for bit.
 *   - a program made by de_program_create_cse is served; refused in addition, before any output or constant is touched:
 *     DE_ERR_INVALID_ARG (the text names the tree) for a map with a negative id or out of first-occurrence order.
 * Afterwards de_eval_loss_grad_ex (BFGS), de_eval_loss_ex (L-BFGS, Nelder-Mead) or de_eval_loss_gn_ex (LM) reproduces loss[t] bit for bit.
 * Not served: the scaled fits, de_fit_consts_lm_wide and the per-tree parameter fits under ties. */
int de_ties_pack_host(int dtype, int32_t n_slots, const int32_t *tie, const void *slots, void *unique);
int de_ties_unpack_host(int dtype, int32_t n_slots, const int32_t *tie, const void *unique, void *slots);
int de_ties_fold_host(int dtype, int32_t n_slots, const int32_t *tie, const void *g, void *g_unique);
int de_ties_fold_matrix_host(int dtype, int32_t n_slots, const int32_t *tie, const void *H, void *Hu);
int de_fit_consts_bfgs_tied(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                            const void *y, const void *w, const de_loss_spec_t *spec, const de_bfgs_opts_t *opts, const int32_t *tie,
                            void *loss, uint8_t *ok, double *history, int32_t *n_accept);
int de_fit_consts_lbfgs_tied(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                             const void *y, const void *w, const de_loss_spec_t *spec, const de_lbfgs_opts_t *opts, const int32_t *tie,
                             void *loss, uint8_t *ok, double *history, int32_t *n_accept);
int de_fit_consts_nm_tied(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                          const void *y, const void *w, const de_loss_spec_t *spec, const de_nm_opts_t *opts, const int32_t *tie, void *loss,
                          uint8_t *ok, double *history, int32_t *n_improve);
int de_fit_consts_lm_tied(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX, const de_param_args_t *pargs,
                          const void *y, const void *w, const de_loss_spec_t *spec, double e_floor, const de_lm_opts_t *opts,
                          const int32_t *tie, void *loss, uint8_t *ok, double *history, int32_t *n_accept);

/* The `dX` of the ChainRules pullback of eval_tree_array (EvalPullback, src/ChainRules.jl:56-77):
 *   dX_t[f, j] = d tree_t(x_j) / d x_f * dY[j]      (`dX = dX_dY .* reshape(dY, 1, length(dY))`, :74)
 * for every tree: a [n_rows, N] column-major matrix per tree (rows = the VARIABLE-mode rows of de_eval_grad:
 * (params,) features) at element offset dX_offsets[t] (host array; NULL: packed), NaN-filled where
 * ok[t] == 0 (`dX_constants_dY .= NaN`, :62-64).  The other half of the pullback, `dtree` =
 * sum_j dconstants[:, j] * dY[j], is de_eval_loss_grad(DE_LOSS_PULLBACK). */
int de_eval_pullback_dX(de_ctx_t *ctx, de_program_t *prog, const void *X, int64_t N, int64_t ldX,
                        const de_param_args_t *pargs, const void *dY, void *dX,
                        const int64_t *dX_offsets, uint8_t *ok);

/* ---- minibatches: a device row sampler and a batch gather -----------------------------
 * A search on a large dataset scores each step on a random subset of the rows (SymbolicRegression.jl's `batching`).  The two calls below
 * make that subset ON THE DEVICE as a DENSE batch — de_batch_sample_rows draws the row indices, de_batch_gather copies those rows of
 * X, y, w and classes into buffers the caller allocated — and every entry point of this header then serves the batch unchanged, bit for
 * bit what it computes on the same rows gathered by any other means.  Work is queued on the context's stream; nothing synchronises
 * unless a host pointer forces it.
 *
 * THE SAMPLER is counter-based: row j of a batch is a pure function of (mode, N, seed, step, offset + j) — no state, a batch drawn in
 * pieces equals the batch drawn at once, and de_batch_rows_host (no context, no device) restates the kernel bit for bit.  All arithmetic
 * is modulo 2^64:
 *   G      = 0x9E3779B97F4A7C15
 *   fin(z) : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (SplitMix64's output function;
 *            fin(G), fin(2G), fin(3G) = e220a8397b1dcdaf 6e789e6aa1b965f4 06c45d188009454f, the published stream of seed 0)
 *   key    : k = fin(seed ^ fin(step + G))          (`seed` names the run, `step` the batch)
 *   DE_BATCH_REPLACE — sampling WITH replacement, what SymbolicRegression.jl's batching draws:
 *            i = offset + j;  r = fin(k + G * (i + 1));  row = mulhi64(r, N)   (the high 64 bits of the product; bias at most N / 2^64)
 *   DE_BATCH_PERMUTE — the slice [offset, offset + n_rows) of a keyed permutation of [0, N): batches without replacement, epochs that
 *            visit every row exactly once, train / hold-out splits.  b = max(2, bit_length(N - 1)) rounded up to even, h = b / 2,
 *            mask = 2^h - 1;  x = offset + j;  repeat { L = x >> h; R = x & mask;
 *            for r = 0 .. 5: (L, R) = (R, L ^ (fin(k ^ (R + G * (r + 1))) & mask));  x = (L << h) | R } until x < N   (cycle walking: the
 *            domain is smaller than 4 N).  offset + n_rows <= N is required: DE_ERR_OUT_OF_RANGE otherwise.
 * Refusals, before anything is written: DE_ERR_INVALID_ARG for a null context, a null `rows` with n_rows > 0, N <= 0, n_rows < 0,
 * offset < 0 or an unknown mode.  n_rows == 0 is DE_OK and touches nothing.  `rows` may be a device or a host pointer; a host `rows` is
 * filled by de_batch_rows_host with no launch. */
typedef enum de_batch_mode { DE_BATCH_REPLACE = 0, DE_BATCH_PERMUTE = 1 } de_batch_mode_t;
int de_batch_sample_rows(de_ctx_t *ctx, int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows);
int de_batch_rows_host(int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows);
/* THE GATHER: dst.X[f + dst.ldX * j] = src.X[f + src.ldX * rows[j]] for f < n_features and j < n_rows, and likewise y[j] = y[rows[j]],
 * w[j] = w[rows[j]], classes[j] = classes[rows[j]].  It is a copy of bytes and serves every de_dtype_t by element size: X and y 2 / 4 / 8 /
 * 8 / 16 bytes for DE_F16 / DE_F32 / DE_F64 / DE_CF32 / DE_CF64; w the real component type (2 / 4 / 8 / 4 / 8 bytes, the buffer table at
 * de_eval_loss); classes 4 or 8 bytes by classes_is_i64, as in de_param_args_t.  N is the number of source rows; ldX counts elements,
 * >= n_features on both sides.  y, w and classes are optional: a column is gathered where BOTH its src and its dst pointer are given; a
 * dst column without its src column is DE_ERR_INVALID_ARG.  X may be null on both sides when n_features == 0.  Source and destination
 * must not overlap (not checked).  One launch gathers X and the present columns; every address is computed in 64 bits.
 *   de_batch_gather: the data pointers (src and dst X, y, w, classes) are all device pointers — or all host pointers, which are served on
 *   the host by the routine below.  `rows` and `n_bad` may each be on either side.
 * Row indices outside [0, N):
 *   - host `rows`: refused with DE_ERR_OUT_OF_RANGE before anything is written (de_last_error names the first position); *n_bad = 0.
 *   - device `rows` cannot be tested without a synchronisation, so the kernel guards: it reads nothing for such a row and writes a quiet
 *     NaN into that batch row's X, y and w (both components of a complex element) — every tree's loss over the batch comes out NaN, loud
 *     rather than silent — and the class id of source row 0, which keeps the parameter lookup downstream in range.  The row is counted
 *     in *n_bad (int32, may be NULL), which the call zeroes first; a host n_bad makes the call synchronise.
 *   de_batch_gather_host (host pointers only, no context) always pre-checks and refuses; ONE routine serves both and fills and counts
 *   in the same way when de_batch_gather hands it rows it copied from the device (host data with device rows).
 * Other refusals, before anything is written: DE_ERR_INVALID_ARG for a null src / dst / rows (n_rows > 0), an unknown dtype, n_rows < 0,
 * N <= 0, n_features < 0, ldX < n_features, a null X with n_features > 0, and (de_batch_gather) data pointers on both sides of the bus.
 * n_rows == 0 is DE_OK and writes nothing but *n_bad = 0. */
typedef struct de_batch_src {
    const void *X;
    int64_t N;
    int64_t ldX;
    int32_t n_features;
    int32_t classes_is_i64;
    const void *y;
    const void *w;
    const void *classes;
} de_batch_src_t;
typedef struct de_batch_dst {
    void *X;
    int64_t ldX;
    void *y;
    void *w;
    void *classes;
} de_batch_dst_t;
int de_batch_gather(de_ctx_t *ctx, int dtype, const de_batch_src_t *src, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *dst,
                    int32_t *n_bad);
int de_batch_gather_host(int dtype, const de_batch_src_t *src, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *dst, int32_t *n_bad);

/* ---- multi-GPU: one process per GPU, population tree-sharded, RCCL over xGMI -----------------------------
 * The path shards embarrassingly: rank r owns trees {t : t mod world == r} (round-robin balances node
 * counts), X is replicated, every rank evaluates its shard with de_eval* into its own output slab, and the only exchange
 * per evaluation is ONE all-gather of the per-tree completion flags (ceil(n_trees / world) bytes per rank, latency-bound).
 * Outputs are never gathered (400 GB at BASELINE config 4).  Usage (every rank):
 *     char id[DE_DIST_ID_BYTES];  if (rank == 0) de_dist_unique_id(id);   <ship the 128 bytes to the other ranks: MPI,
 *     a file, a socket, Julia's Distributed>;   de_dist_init(ctx, rank, world, id, &comm);
 *     de_dist_broadcast(comm, X_dev, bytes, 0);                     // once per dataset
 *     de_eval(ctx, local_program, X_dev, ..., out_local, ld, ok_local);
 *     de_dist_gather_flags(comm, ok_local, n_trees_global, ok_global);  // ok_global[t] in global tree order, on every rank
 * All calls are asynchronous on the context's stream.  librccl.so is loaded on first use (dlopen); without it the
 * calls return DE_ERR_RCCL and single-GPU use is unaffected.  world == 1 needs no id and no RCCL. */
typedef struct de_comm de_comm_t;
#define DE_DIST_ID_BYTES 128
int de_dist_unique_id(void *id);
int de_dist_init(de_ctx_t *ctx, int rank, int world, const void *id, de_comm_t **out_comm);
int de_dist_destroy(de_comm_t *comm);
/* Bound the collectives of this communicator (round 6).  timeout_ms > 0: de_dist_broadcast / de_dist_gather_flags WAIT for what they
 * queued — polling the stream and ncclCommGetAsyncError — and return DE_ERR_RCCL after timeout_ms with the communicator aborted
 * (ncclCommAbort) and a message naming the rank and the collective (de_dist_last_error): a peer that died, or never entered the same
 * collective, otherwise hangs every other rank for ever.  0 (the default; DE_DIST_TIMEOUT_MS in the environment changes it): the calls stay
 * asynchronous on the context's stream and the caller bounds its own synchronisation.  de_dist_init itself — ncclCommInitRank blocks until
 * every rank has called it — is bounded by DE_DIST_INIT_TIMEOUT_MS (default 120 000 ms; 0 = wait for ever). */
int de_dist_set_timeout(de_comm_t *comm, int64_t timeout_ms);
int de_dist_world_size(de_comm_t *comm); /* ranks of the communicator as RCCL reports them (ncclCommCount); 1 for a one-rank comm; -1 on error */
int64_t de_dist_shard_size(int64_t n_trees, int rank, int world);
int de_dist_broadcast(de_comm_t *comm, void *buf, size_t bytes, int root);
int de_dist_gather_flags(de_comm_t *comm, const uint8_t *ok_local, int64_t n_trees, uint8_t *ok_global);
/* test / measurement hook, no RCCL involved: packs every SIMULATED rank's shard of flags_global (host) the way de_dist_gather_flags
 * does, unpacks the gathered buffer into out (host; must equal flags_global), *ms = one rank's pack + unpack launches (may be NULL) */
int de_dist_reorder_selftest(de_ctx_t *ctx, const uint8_t *flags_global, int64_t n_trees, int world, uint8_t *out, float *ms);
const char *de_dist_last_error(de_comm_t *comm); /* comm may be NULL: errors of de_dist_unique_id / de_dist_init */

/* ---- one-shot convenience with the reference's single-tree signature ------- */
int de_eval_tree_array(de_ctx_t *ctx, int dtype, const de_tape_node_t *nodes, int64_t n_nodes,
                       const void *consts, int64_t n_consts, const void *X, int32_t n_features,
                       int64_t N, uint32_t options, void *out, uint8_t *ok);

/* ---- measurement hooks (bench.py) ------------------------------------------- */
/* Launch plan de_eval would use for N samples: plan[0] = samples per workgroup tile,
 * plan[1] = tree chunks, plan[2] = trees per chunk (the trees that share one staged X
 * tile: the K_eff of the algorithmic-bytes formula).  A program that runs
 * in wave groups (several waves per workgroup on one tile, a chunk each): the workgroups
 * per tile and the trees of one workgroup. */
int de_eval_plan(const de_program_t *prog, int64_t N, int32_t *plan);
/* 1 when an early-exit launch of n_trees trees over X[n_features, N] first runs the PRIORITY TILES (one pass over X, a probe
 * launch on the 3 F tiles with the features' extreme values, then the launch proper over the compacted live trees): the
 * library's own thresholds (sample tiles, trees, features; DE_PRIO_MIN_TILES / DE_PRIO_MIN_TREES / DE_NO_PRIO_TILES). */
int de_prio_tiles_wanted(int64_t N, int32_t n_features, int64_t n_trees);
/* Trees still live (flag 1) behind the probe launch of the priority tiles in the most recent de_eval / de_eval_loss of this
 * program that compacted its live trees: *n_live; -1 when that call did not (small launch, DE_OPT_FULL_EVAL, early_exit off).
 * Blocks until the call has finished.  n_trees - n_live = what the 3 F priority tiles flagged. */
int de_program_last_live_trees(de_program_t *prog, int64_t *n_live);
/* Device time of the kernels launched by the most recent de_eval* call on this
 * context, measured with hipEvents recorded on the context's stream.  Blocks
 * until that work has finished. */
int de_ctx_last_kernel_ms(de_ctx_t *ctx, float *ms);
/* Name of the dominant kernel symbol of the most recent call (for matching the
 * rocprofv3 kernel-trace rows). */
const char *de_ctx_last_kernel_name(de_ctx_t *ctx);
/* Device time of EVERY call of a free-running loop: de_ctx_timing_ring(ctx, n) keeps the event pairs of the last n timed calls
 * (n = 0: back to one pair), de_ctx_timing_read waits for the last call and returns their durations, oldest first (at most cap;
 * *n_out written), then restarts the ring.  (de_ctx_last_kernel_ms blocks per call; round 5.) */
int de_ctx_timing_ring(de_ctx_t *ctx, int32_t n);
int de_ctx_timing_read(de_ctx_t *ctx, float *ms, int32_t cap, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* DE_HIP_H */
