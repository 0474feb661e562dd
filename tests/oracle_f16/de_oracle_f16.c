/*
 * de_oracle_f16.c — the CPU oracle (oracle/de_oracle_ops.h + oracle/de_oracle_impl.h) instantiated a THIRD time, for Julia's Float16:
 * OT = _Float16, OW = float.  TEST INFRASTRUCTURE of tests/test_f16_host.py and tests/test_gpu_f16.py, built by their module-scoped
 * fixtures (tests/f16_oracle.py) with ROCm's clang:
 *
 *     clang -O2 -fPIC -shared -ffp-contract=off -Xclang -ffloat16-excess-precision=none
 *
 * The last flag is what makes this a binary16 oracle: without it clang keeps _Float16 expressions in float and rounds only at
 * assignments (z*z/z at z = 300: inf with the flag, 300 without).  With it every _Float16 operation rounds to binary16 — Julia's
 * Float16 arithmetic: + - * / rounded once; the wide-type transcendentals (WIDE1 / WIDE2: the Float32 libm, rounded
 * once), as Julia's Float16 methods compute; composites step by step in T (square, cube, custom_cos, pow_abs2, +(x, y, z), mod's
 * r + y), which is the step table already — no opcode of the shared headers evaluates a composite in the wide type, so none is
 * overridden here.  The native-T functions the headers call (NF(fn) = fn ## f16) are the shims below: exact operations, or Float32
 * ones whose one rounding to binary16 is the correctly rounded result (sqrt: 24 >= 2 * 11 + 2) or Julia's definition (fma: Float32
 * muladd of binary16 operands, rounded once).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/de_hip.h"

/* Tape parser (the same as oracle/de_oracle.c's: that one is static there) */
typedef struct onode {
    uint8_t degree, op;
    uint16_t arg;
    int child[3];
    int is_const; /* is_constant(subtree): no feature/param leaf below (src/NodeUtils.jl:73) */
} onode;

/* Post-order tape -> indexed tree.  Returns root index or a negative error:
 * -2 malformed tape, -3 unknown opcode, -6 index out of range. */
static int o_parse(const de_tape_node_t *tape, int64_t n, int64_t n_consts, int F, int P,
                   onode **out) {
    if (n <= 0) return -2;
    onode *nodes = (onode *)calloc((size_t)n, sizeof(onode));
    int *stack = (int *)malloc((size_t)n * sizeof(int));
    int sp = 0;
    int err = 0;
    for (int64_t i = 0; i < n && !err; i++) {
        onode *nd = &nodes[i];
        nd->degree = tape[i].degree;
        nd->op = tape[i].op;
        nd->arg = tape[i].arg;
        if (nd->degree == 0) {
            if (nd->op == DE_LEAF_CONST) { nd->is_const = 1; if (nd->arg >= n_consts) err = -6; }
            else if (nd->op == DE_LEAF_FEATURE) { if (nd->arg >= F) err = -6; }
            else if (nd->op == DE_LEAF_PARAM) { if (nd->arg >= P) err = -6; }
            else err = -2;
        } else if (nd->degree <= 3) {
            int lo = nd->degree == 1 ? DE_U_NEG : (nd->degree == 2 ? DE_B_ADD : DE_T_FMA);
            int hi = nd->degree == 1 ? DE_U_LAST_ : (nd->degree == 2 ? DE_B_LAST_ : DE_T_LAST_);
            if (nd->op < lo || nd->op >= hi) { err = -3; break; }
            if (sp < nd->degree) { err = -2; break; }
            nd->is_const = 1;
            for (int k = nd->degree - 1; k >= 0; k--) {
                nd->child[k] = stack[--sp];
                nd->is_const &= nodes[nd->child[k]].is_const;
            }
        } else err = -2;
        stack[sp++] = (int)i;
    }
    if (!err && sp != 1) err = -2;
    int root = err ? err : stack[0];
    free(stack);
    if (err) { free(nodes); return err; }
    *out = nodes;
    return root;
}


/* native-T shims for OT = _Float16 */
static inline _Float16 fabsf16(_Float16 x) { return (_Float16)fabsf((float)x); }
static inline _Float16 sqrtf16(_Float16 x) { return (_Float16)sqrtf((float)x); }
static inline _Float16 rintf16(_Float16 x) { return (_Float16)rintf((float)x); }
static inline _Float16 floorf16(_Float16 x) { return (_Float16)floorf((float)x); }
static inline _Float16 ceilf16(_Float16 x) { return (_Float16)ceilf((float)x); }
static inline _Float16 truncf16(_Float16 x) { return (_Float16)truncf((float)x); }
static inline _Float16 fmodf16(_Float16 x, _Float16 y) { return (_Float16)fmodf((float)x, (float)y); }
static inline _Float16 copysignf16(_Float16 x, _Float16 y) { return (_Float16)copysignf((float)x, (float)y); }
static inline _Float16 fmaf16(_Float16 x, _Float16 y, _Float16 z) { return (_Float16)fmaf((float)x, (float)y, (float)z); }

/* ---- _Float16 instantiation ---- */
#define OT _Float16
#define OW float
#define OSUF f16
#define WSUF f
#define ONAME _f16
#include "../../oracle/de_oracle_ops.h"
#include "../../oracle/de_oracle_impl.h"

/* Scalar probes (float in, float out: every value is a binary16 value) */
float de_oracle_unary_f16(int op, float x) { return (float)o_unary_f16(op, (_Float16)x); }
float de_oracle_binary_f16(int op, float x, float y) { return (float)o_binary_f16(op, (_Float16)x, (_Float16)y); }
float de_oracle_ternary_f16(int op, float x, float y, float z) { return (float)o_ternary_f16(op, (_Float16)x, (_Float16)y, (_Float16)z); }
/* the flag of the excess-precision switch: 1 when z*z/z at z = 300 overflows (binary16 per operation) */
int de_oracle_f16_strict(void) {
    volatile _Float16 z = (_Float16)300.0f;
    _Float16 r = z * z / z;
    return isinf((float)r) ? 1 : 0;
}
int de_oracle_f16_abi(void) { return DE_HIP_ABI_VERSION; }
