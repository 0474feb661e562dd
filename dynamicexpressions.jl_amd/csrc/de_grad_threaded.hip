// de_grad_threaded.hip — forward-mode gradient kernel, threaded-code variant (gfx950).
// Same semantics as de_grad_tape_kernel (de_grad_kernels.hip; reference src/EvaluateDerivative.jl:
// eval_grad_tree_array :193-243, grad_degn_eval :340-365, grad_deg0_eval :367-404): every sample
// carries a dual number (x, d[0..GC)) through the bound UNFOLDED program.  The flat switch of that
// kernel costs ~37 scalar instructions per interpreted instruction and a gradient wave holds ONE
// sample per lane, so scalar issue — not the dual arithmetic — was its limit.  Here every
// (operator, operand kind, check) combination is its own leaf function; operand kinds are resolved on the
// host (leaf row / spill slot / constant), so handlers are straight-line code.  Dispatch is DIRECT-THREADED like the
// eval kernel's (de_kernels.hip): a handler loads the next record first (s_load_dwordx4, overlapping its own LDS reads
// and arithmetic), runs its body and tail-calls the next handler (s_setpc_b64) with that record's operand words in
// SGPRs — knowing its successor since entry, without waiting for that load (round 4) —; the tree's end record (g_end) returns to
// the kernel for the epilogue.  6 scalar + 1 vector instruction per dispatch against 14 + 2 for the call/return loop of round 1.
//
// Instruction word (16 B, built by de_api_grad.cpp ensure_grad_threaded from the bound program):
//   x = handler address - handler base OF THE NEXT RECORD (end record: of the tree's first record); the base travels with the chain
//       in SGPRs: one code object module per window width
//   y = LDS byte offset of the operand (leaf row or spill slot base) | aux << 24
//         aux = gradient row seeded by a leaf/constant operand (0xFF: none in this mode);
//         for GOP_GEN_CONST y[23:16] = de_opcode (no LDS operand), for GOP_TERN aux = de_opcode
//   z,w = constant bits | de_opcode (generic row/acc handlers) | byte distance slot B -> slot C (TERN)
// The window offset g0 travels in the state (a uniform VGPR that never moves): seed = aux - g0.
//
// ONE translation unit (= one code object module) per (element type, window width): for an indirect call
// LLVM sizes the kernel's register file for the most expensive address-taken function of the MODULE,
// so with every instantiation in one module the Float32 GC=5 kernel was allocated the 104 VGPRs of the
// Float64 GC=8 handlers (4 waves/SIMD instead of 8).  build.sh compiles this file with
// -DDE_GT_T=float|double -DDE_GT_TAG=f|d -DDE_GT_GC=1..6,8 -DDE_GT_VS=1|2; de_grad_kernels.hip dispatches.
//
// Samples per lane (DE_GT_VS): Float32 windows of <= 6 rows also exist in a variant that carries TWO
// consecutive samples per lane as float2 — the dense dual update  g1*d1[k] + g2*d2[k]  is all multiplies and
// adds, which gfx950 issues two per lane per instruction (v_pk_mul_f32 / v_pk_add_f32), and a dispatch is
// amortised over twice the samples.  It doubles the LDS rows, so the host uses it for the trees that need at
// most one spill slot (11 rows x 512 B x 4 waves = 22.5 KB: 7 workgroups per CU); with two slots (34.8 KB: 4
// workgroups) the lost occupancy costs more than the packed arithmetic saves (measured).  The state must stay
// within the 16 dwords the calling convention passes in registers (2*(1 + GC) + poison + g0).
#include "de_grad_common.h"

#ifndef DE_GT_T
#error "compile with -DDE_GT_T=<float|double> -DDE_GT_TAG=<f|d> -DDE_GT_GC=<n> -DDE_GT_VS=<1|2>"
#endif
#ifndef DE_GT_VS
#define DE_GT_VS 1
#endif

namespace de {

#define DE_GT_CAT4(a, b, c, d, e) a##b##c##d##e
#define DE_GT_CAT5(a, b, c, d, e) DE_GT_CAT4(a, b, c, d, e)
#define DE_GT_NAME(prefix) DE_GT_CAT5(prefix, DE_GT_TAG, DE_GT_GC, v, DE_GT_VS)
// Every module instantiates the SAME templates with different DE_GT_VS: their host-side kernel stubs are
// linkonce symbols the linker would merge across modules (launching some other module's kernel), so each
// module's templates live in a namespace of their own.
namespace DE_GT_NAME(gtm_) {

template <typename T> struct GImm;
template <> struct GImm<float> { typedef uint32_t type; };
template <> struct GImm<double> { typedef uint64_t type; };
template <typename T> __device__ __forceinline__ T gimm_from(typename GImm<T>::type b);
template <> __device__ __forceinline__ float gimm_from<float>(uint32_t b) { return __uint_as_float(b); }
template <> __device__ __forceinline__ double gimm_from<double>(uint64_t b) { return __longlong_as_double((long long)b); }

constexpr int VS = DE_GT_VS; // samples per lane
template <typename T> struct LaneVec { typedef T type __attribute__((ext_vector_type(DE_GT_VS))); };
#define LV(T) typename LaneVec<T>::type
template <typename T> __device__ __forceinline__ LV(T) lv_splat(T c) {
    LV(T) v;
    DE_UNROLL for (int i = 0; i < VS; i++) v[i] = c;
    return v;
}
template <typename T, int GC> struct GState {
    LV(T) x;
    LV(T) d[GC];
    T poison; // one per lane: fma-accumulated over its samples
    uint32_t g0;
};
template <typename T, int GC> struct GDual {
    LV(T) x;
    LV(T) d[GC];
};
#define GHARGS GState<T, GC> st, uint32_t la, typename GImm<T>::type imm
template <typename T, int GC> using GBodyFn = GState<T, GC> (*)(GState<T, GC>, uint32_t, typename GImm<T>::type);
// what the stream points at: gh_chain<T, GC, &body>.  `code` = the NEXT record; (la, imm) = this instruction's operand words; nx = the
// handler of the NEXT record (address - hbase) — it stands in THIS instruction's record (round 4: x of record k names the handler of
// record k + 1, the end record names the tree's first handler), so a handler knows its successor at entry, loads the next record
// straight into the successor's argument registers (the aligned SGPR quad nx, la, imm) and jumps WITHOUT waiting for the load:
// the callee's entry wait completes it, the jump's instruction fetch overlaps with it.  (Before, the target came out of the loaded
// record: every handler sat out the scalar-cache latency before it could jump — the eval kernel dropped that in round 2.)
// lds0 = the lane's LDS base; hbase = handler base of this module.  csrc/irpatch.py moves code, hbase, nx, la, imm to SGPRs.
#define GCHAIN_ARGS GState<T, GC> st, uint32_t lds0, ConstU4Ptr code, uint64_t hbase, uint32_t nx, uint32_t la, typename GImm<T>::type imm
template <typename T, int GC> using GHandlerFn = GState<T, GC> (*)(GState<T, GC>, uint32_t, ConstU4Ptr, uint64_t, uint32_t, uint32_t, typename GImm<T>::type);
template <typename T> __device__ __forceinline__ typename GImm<T>::type grec_imm(const U32x4 &w);
template <> __device__ __forceinline__ uint32_t grec_imm<float>(const U32x4 &w) { return w.z; }
template <> __device__ __forceinline__ uint64_t grec_imm<double>(const U32x4 &w) { return ((uint64_t)w.w << 32) | w.z; }
// record address + 1 WITHOUT a carry into the high half (the stream lies inside one 4 GiB window: prog_malloc in de_api.cpp guarantees it, the callers check the allocation)
__device__ __forceinline__ ConstU4Ptr gcode_next(ConstU4Ptr c) {
    const uint64_t a = (uint64_t)(uintptr_t)c;
    return (ConstU4Ptr)(uintptr_t)((a & 0xFFFFFFFF00000000ull) | (uint64_t)((uint32_t)a + 16u));
}
#define GCHAIN_NEXT(W) [[clang::musttail]] return reinterpret_cast<GHandlerFn<T, GC>>(hbase + nx)(st, lds0, gcode_next(code), hbase, (W).x, (W).y, grec_imm<T>(W))
#define GH(...) (uint64_t)&gh_chain<T, GC, &__VA_ARGS__>
#define GLDS(T, addr) (reinterpret_cast<__attribute__((address_space(3))) LV(T) *>((uintptr_t)(addr)))
// LDS is laid out wave-major: wave w owns rows [w*R, (w+1)*R), a row = the 64*VS samples of that wave
// (512 B for Float32 x 2) — everything a wave touches is private to it and contiguous, which the epilogue
// uses to turn the [samples, G] gradient block into coalesced 16-byte stores.
template <typename T> constexpr uint32_t grow_bytes() { return (uint32_t)(64 * VS * sizeof(T)); }
template <typename T> __device__ __forceinline__ void gpoison(T &poison, LV(T) v) {
    DE_UNROLL for (int i = 0; i < VS; i++) poison = M<T>::fma(v[i], T(0), poison);
}

// operand kinds (de_bind.h GSRC_*)
enum { GS_LEAF = GSRC_LEAF, GS_SLOT = GSRC_SLOT, GS_CONST = GSRC_CONST, GS_ACC = GSRC_ACC };

// An operand: value + how its gradient is represented.  SV (seed variant, de_bind.h): 0 = the one-hot
// row index is read at run time (aux - g0), 1 = no gradient component in this window, 2 + k = component k.
// For LEAF/CONST operands with SV >= 1 the one-hot vector is never materialised: the reference's dense
//   g * db[k]   is   g * 1 = g  for k = seed  and  g * 0  elsewhere  (g * 0 is still computed once: it is NaN
// for an infinite partial and carries the sign of zero, exactly as in grad_degn_eval :340-365).
template <typename T, int GC, int SRC, int SV> struct GOperand {
    LV(T) x;
    LV(T) d[GC]; // only meaningful for SLOT/ACC operands and run-time seeds
};
template <typename T, int GC, int SRC, int SV> __device__ __forceinline__ GOperand<T, GC, SRC, SV> goperand(GState<T, GC> &st, uint32_t la, typename GImm<T>::type imm) {
    GOperand<T, GC, SRC, SV> b;
    if constexpr (SRC == GS_SLOT) {
        b.x = *GLDS(T, la);
        DE_UNROLL for (int k = 0; k < GC; k++) b.d[k] = *GLDS(T, la + (1 + k) * grow_bytes<T>());
    } else if constexpr (SRC == GS_ACC) {
        b.x = st.x;
        DE_UNROLL for (int k = 0; k < GC; k++) b.d[k] = st.d[k];
    } else {
        if constexpr (SRC == GS_LEAF) {
            b.x = *GLDS(T, SV == 0 ? (la & 0xFFFFFFu) : la); // host leaves aux = 0 for known seeds
            gpoison<T>(st.poison, b.x); // every leaf operand is tested where it is read (:239-242)
        } else b.x = lv_splat<T>(gimm_from<T>(imm));
        if constexpr (SV == 0) {
            const int seed = (int)(la >> 24) - (int)(st.g0 & 0xFFFFu);
            DE_UNROLL for (int k = 0; k < GC; k++) b.d[k] = lv_splat<T>((k == seed) ? T(1) : T(0));
        }
    }
    return b;
}
// g * db[k]
template <typename T, int GC, int SRC, int SV> __device__ __forceinline__ void gscale(LV(T) g, const GOperand<T, GC, SRC, SV> &b, LV(T) (&out)[GC]) {
    if constexpr ((SRC == GS_LEAF || SRC == GS_CONST) && SV >= 1) {
        const LV(T) z = g * lv_splat<T>(T(0));
        DE_UNROLL for (int k = 0; k < GC; k++) out[k] = (k == SV - 2) ? g : z; // g * 1 == g bit for bit
    } else {
        DE_UNROLL for (int k = 0; k < GC; k++) out[k] = g * b.d[k];
    }
}

template <typename T, int GC, int SRC, int SV> __device__ __forceinline__ GState<T, GC> g_load(GHARGS) {
    const GOperand<T, GC, SRC, SV> b = goperand<T, GC, SRC, SV>(st, la, imm);
    st.x = b.x;
    if constexpr ((SRC == GS_LEAF || SRC == GS_CONST) && SV >= 1) { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = lv_splat<T>((k == SV - 2) ? T(1) : T(0)); }
    else { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = b.d[k]; }
    return st;
}
template <typename T, int GC> __device__ __forceinline__ GState<T, GC> g_push(GHARGS) {
    *GLDS(T, la) = st.x;
    DE_UNROLL for (int k = 0; k < GC; k++) *GLDS(T, la + (1 + k) * grow_bytes<T>()) = st.d[k];
    return st;
}
// PUSH + LOAD in one dispatch.  LEAF: la = the row (| run-time seed << 24), imm = byte distance from the row to the slot;
// CONST: la = the slot (| run-time seed << 24), imm = the constant.
template <typename T, int GC, int SRC, int SV> __device__ __forceinline__ GState<T, GC> g_pushload(GHARGS) {
    uint32_t slot = la & 0xFFFFFFu;
    if constexpr (SRC == GS_LEAF) slot += (uint32_t)imm;
    *GLDS(T, slot) = st.x;
    DE_UNROLL for (int k = 0; k < GC; k++) *GLDS(T, slot + (1 + k) * grow_bytes<T>()) = st.d[k];
    const GOperand<T, GC, SRC, SV> b = goperand<T, GC, SRC, SV>(st, la, imm);
    st.x = b.x;
    if constexpr (SV >= 1) { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = lv_splat<T>((k == SV - 2) ? T(1) : T(0)); }
    else { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = b.d[k]; }
    return st;
}
template <typename T, int GC> __device__ __forceinline__ GState<T, GC> g_check_acc(GHARGS) {
    gpoison<T>(st.poison, st.x);
    return st;
}
template <typename T, int GC> __device__ __forceinline__ GState<T, GC> g_nop(GHARGS) { return st; }

// binary hot ops: value v and partials (gl, gr) w.r.t. (left, right); K 2/5 (RSUB/RDIV): left = operand.
// The formulas (and their operation order) are the oracle's / the switch kernel's: d = gl*dl + gr*dr dense.
template <typename T, int GC, int K, int SRC, int SV, bool CHK> __device__ __forceinline__ GState<T, GC> g_bin(GHARGS) {
    const GOperand<T, GC, SRC, SV> b = goperand<T, GC, SRC, SV>(st, la, imm);
    constexpr bool REV = (K == 2 || K == 5);
    const LV(T) lx = REV ? b.x : st.x, ly = REV ? st.x : b.x;
    LV(T) v, gl, gr;
    if constexpr (K == 0) { v = lx + ly; gl = lv_splat<T>(T(1)); gr = lv_splat<T>(T(1)); }
    else if constexpr (K == 1 || K == 2) { v = lx - ly; gl = lv_splat<T>(T(1)); gr = lv_splat<T>(T(-1)); }
    else if constexpr (K == 3) { v = lx * ly; gl = ly; gr = lx; }
    else if constexpr (K == 6 || K == 7) { // max / min: the expressions of binary_vg (ties: the second argument takes the gradient of max)
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const bool gt = lx[i] > ly[i];
            v[i] = K == 6 ? jl_max(lx[i], ly[i]) : jl_min(lx[i], ly[i]);
            gl[i] = (K == 6) == gt ? T(1) : T(0);
            gr[i] = (K == 6) == gt ? T(0) : T(1);
        }
    }
    else { v = lx / ly; gl = lv_splat<T>(T(1)) / ly; gr = -(v / ly); }
    st.x = v;
    LV(T) sb[GC];
    gscale<T, GC, SRC, SV>(REV ? gl : gr, b, sb); // the operand's term
    if constexpr (REV) { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = sb[k] + gr * st.d[k]; }
    else { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = gl * st.d[k] + sb[k]; }
    if constexpr (CHK) gpoison<T>(st.poison, st.x);
    return st;
}
// unary hot ops (K: 0 cos, 1 exp, 2 sin, 3.. see gun_inline)
template <typename T, int GC, int K, int SRC, int SV, bool CHK> __device__ __forceinline__ GState<T, GC> g_un(GHARGS) {
    const GOperand<T, GC, SRC, SV> b = goperand<T, GC, SRC, SV>(st, la, imm);
    LV(T) y, g;
    if constexpr (K >= 3) {
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const UG<T> r = gun_inline<T, K>(b.x[i]);
            y[i] = r.y;
            g[i] = r.g;
        }
    } else if constexpr (sizeof(T) == 4) {
        if constexpr (K == 1) { DE_UNROLL for (int i = 0; i < VS; i++) { y[i] = (T)fast_exp_f32((float)b.x[i]); g[i] = y[i]; } }
        else {
            bool big = false;
            DE_UNROLL for (int i = 0; i < VS; i++) {
                float sn, cs;
                fast_sincos_f32((float)b.x[i], &sn, &cs);
                if constexpr (K == 0) { y[i] = (T)cs; g[i] = (T)-sn; } else { y[i] = (T)sn; g[i] = (T)cs; }
                big |= M<T>::abs(b.x[i]) > T(DE_TRIG_FAST_BOUND);
            }
            // |x| > 1e5: OCML's full-range functions, per ELEMENT — a sample's value must not depend on its wave
            // neighbours (inline: a call would make this handler a non-leaf function)
            if (__ballot(big) != 0ull) {
                DE_UNROLL for (int i = 0; i < VS; i++) {
                    if (M<T>::abs(b.x[i]) > T(DE_TRIG_FAST_BOUND)) {
                        const float sn = sinf((float)b.x[i]), cs = cosf((float)b.x[i]);
                        if constexpr (K == 0) { y[i] = (T)cs; g[i] = (T)-sn; } else { y[i] = (T)sn; g[i] = (T)cs; }
                    }
                }
            }
        }
    } else {
        DE_UNROLL for (int i = 0; i < VS; i++) {
            if constexpr (K == 0) { y[i] = M<T>::cos(b.x[i]); g[i] = -M<T>::sin(b.x[i]); }
            else if constexpr (K == 1) { y[i] = M<T>::exp(b.x[i]); g[i] = y[i]; }
            else { y[i] = M<T>::sin(b.x[i]); g[i] = M<T>::cos(b.x[i]); }
        }
    }
    st.x = y;
    gscale<T, GC, SRC, SV>(g, b, st.d);
    if constexpr (CHK) gpoison<T>(st.poison, st.x);
    return st;
}
// generic (cold) operators through the noinline value+partials functions of de_grad_common.h
template <typename T, int GC> __device__ __noinline__ GState<T, GC> g_gen_apply(GState<T, GC> st, uint32_t gop, GDual<T, GC> b) {
    if (gop < DE_B_ADD) {
        LV(T) g;
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const UG<T> r = unary_vg<T>(gop, b.x[i]);
            st.x[i] = r.y;
            g[i] = r.g;
        }
        DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = g * b.d[k];
    } else {
        uint32_t fop = gop;
        bool rev = false;
        switch (gop) {
        case DOP_RSUB: fop = DE_B_SUB; rev = true; break;
        case DOP_RDIV: fop = DE_B_DIV; rev = true; break;
        case DOP_RPOW: fop = DE_B_POW; rev = true; break;
        case DOP_RMOD: fop = DE_B_MOD; rev = true; break;
        case DOP_RREM: fop = DE_B_REM; rev = true; break;
        case DOP_RGREATER: fop = DE_B_GREATER; rev = true; break;
        case DOP_RPOW_ABS2: fop = DE_B_POW_ABS2; rev = true; break;
    case DOP_RMAX: fop = DE_B_MAX; rev = true; break;
    case DOP_RMIN: fop = DE_B_MIN; rev = true; break;
        default: break;
        }
        LV(T) gx, gy;
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const BG<T> r = rev ? binary_vg<T>(fop, b.x[i], st.x[i]) : binary_vg<T>(fop, st.x[i], b.x[i]);
            st.x[i] = r.v;
            gx[i] = r.gx;
            gy[i] = r.gy;
        }
        if (rev) { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = gx * b.d[k] + gy * st.d[k]; }
        else { DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = gx * st.d[k] + gy * b.d[k]; }
    }
    return st;
}
template <typename T, int GC, int SRC> __device__ __forceinline__ GState<T, GC> g_gen(GHARGS) {
    uint32_t gop;
    if constexpr (SRC == GS_CONST) gop = ((la - (st.g0 & 0xFFFF0000u)) >> 16) & 0xFFu; // no LDS operand: the opcode rides in la[23:16] above the lane's LDS base, whose upper half st.g0 carries
    else gop = (uint32_t)imm;
    const GOperand<T, GC, SRC, 0> o = goperand<T, GC, SRC, 0>(st, la, imm);
    GDual<T, GC> b;
    b.x = o.x;
    DE_UNROLL for (int k = 0; k < GC; k++) b.d[k] = o.d[k];
    return g_gen_apply<T, GC>(st, gop, b);
}
template <typename T, int GC> __device__ __forceinline__ GState<T, GC> g_tern(GHARGS) { // acc = op3(slot B, slot C, acc)
    const uint32_t lb = la & 0xFFFFFFu, lc = lb + (uint32_t)imm;
    const LV(T) xb = *GLDS(T, lb), xc = *GLDS(T, lc);
    LV(T) g0, g1, g2;
    DE_UNROLL for (int i = 0; i < VS; i++) {
        const TG<T> r = ternary_vg<T>(la >> 24, xb[i], xc[i], st.x[i]);
        st.x[i] = r.v;
        g0[i] = r.g0; g1[i] = r.g1; g2[i] = r.g2;
    }
    DE_UNROLL for (int k = 0; k < GC; k++)
        st.d[k] = (g0 * *GLDS(T, lb + (1 + k) * grow_bytes<T>()) + g1 * *GLDS(T, lc + (1 + k) * grow_bytes<T>())) + g2 * st.d[k];
    return st;
}

// ---- direct-threaded dispatch (see the head of the file) ----------------------------------------------------------
template <typename T, int GC, GBodyFn<T, GC> BODY> __device__ __noinline__ GState<T, GC> gh_chain(GCHAIN_ARGS) {
    const U32x4 w = *code;
    st = BODY(st, lds0 + la, imm);
    GCHAIN_NEXT(w);
}
template <typename T, int GC> __device__ __noinline__ GState<T, GC> g_end(GState<T, GC> st, uint32_t, ConstU4Ptr, uint64_t, uint32_t, uint32_t, typename GImm<T>::type) { return st; }

// handler table: seed variants enumerated at compile time
template <typename T, int GC, int SV> __device__ __forceinline__ void fill_seeded(uint64_t *t) {
    if constexpr (SV < GC + 2) {
        t[gop_load(GC, GS_LEAF, SV)] = GH(g_load<T, GC, GS_LEAF, SV>);
        t[gop_load(GC, GS_CONST, SV)] = GH(g_load<T, GC, GS_CONST, SV>);
        t[gop_pushload(GC, GS_LEAF, SV)] = GH(g_pushload<T, GC, GS_LEAF, SV>);
        t[gop_pushload(GC, GS_CONST, SV)] = GH(g_pushload<T, GC, GS_CONST, SV>);
#define GB1(K) t[gop_bin(GC, K, GS_LEAF, SV, false)] = GH(g_bin<T, GC, K, GS_LEAF, SV, false>); \
               t[gop_bin(GC, K, GS_LEAF, SV, true)] = GH(g_bin<T, GC, K, GS_LEAF, SV, true>);    \
               t[gop_bin(GC, K, GS_CONST, SV, false)] = GH(g_bin<T, GC, K, GS_CONST, SV, false>); \
               t[gop_bin(GC, K, GS_CONST, SV, true)] = GH(g_bin<T, GC, K, GS_CONST, SV, true>);
        GB1(0) GB1(1) GB1(2) GB1(3) GB1(4) GB1(5) GB1(6) GB1(7)
#undef GB1
#define GU1(K) t[gop_un(GC, K, GS_LEAF, SV, false)] = GH(g_un<T, GC, K, GS_LEAF, SV, false>); \
               t[gop_un(GC, K, GS_LEAF, SV, true)] = GH(g_un<T, GC, K, GS_LEAF, SV, true>);
        GU1(0) GU1(1) GU1(2) GU1(3) GU1(4) GU1(5) GU1(6) GU1(7) GU1(8) GU1(9) GU1(10) GU1(11) GU1(12)
#undef GU1
        fill_seeded<T, GC, SV + 1>(t);
    }
}
template <typename T, int GC> __global__ void de_grad_fill_handlers(uint64_t *t) {
    fill_seeded<T, GC, 0>(t);
    t[gop_load(GC, GS_SLOT, 0)] = GH(g_load<T, GC, GS_SLOT, 0>);
    t[gop_push(GC)] = GH(g_push<T, GC>);
    t[gop_check_acc(GC)] = GH(g_check_acc<T, GC>);
#define GB2(K) t[gop_bin(GC, K, GS_SLOT, 0, false)] = GH(g_bin<T, GC, K, GS_SLOT, 0, false>); \
               t[gop_bin(GC, K, GS_SLOT, 0, true)] = GH(g_bin<T, GC, K, GS_SLOT, 0, true>);
    GB2(0) GB2(1) GB2(2) GB2(3) GB2(4) GB2(5) GB2(6) GB2(7)
#undef GB2
#define GU2(K, S) t[gop_un(GC, K, S, 0, false)] = GH(g_un<T, GC, K, S, 0, false>); t[gop_un(GC, K, S, 0, true)] = GH(g_un<T, GC, K, S, 0, true>);
#define GU3(K) GU2(K, GS_SLOT) GU2(K, GS_ACC)
    GU3(0) GU3(1) GU3(2) GU3(3) GU3(4) GU3(5) GU3(6) GU3(7) GU3(8) GU3(9) GU3(10) GU3(11) GU3(12)
#undef GU3
#undef GU2
    t[gop_gen(GC, GS_LEAF)] = GH(g_gen<T, GC, GS_LEAF>);
    t[gop_gen(GC, GS_SLOT)] = GH(g_gen<T, GC, GS_SLOT>);
    t[gop_gen(GC, GS_CONST)] = GH(g_gen<T, GC, GS_CONST>);
    t[gop_gen(GC, GS_ACC)] = GH(g_gen<T, GC, GS_ACC>);
    t[gop_param(GC)] = (uint64_t)&g_end<T, GC>; // the end record of every tree (the id is a leftover of round 1's parameter handler)
    t[gop_tern(GC)] = GH(g_tern<T, GC>);
}

// End of a tree: store (or reduce) the wave's results.  Out of line on purpose, and fed with plain values
// (taking the address of the kernel-argument struct would make every load from it look divergent): nothing
// of the epilogue stays live in VGPRs across the handler calls of the interpreter loop.
template <typename T, int GC, bool SHARE>
__device__ __noinline__ void g_epilogue_loss(GState<T, GC> st, const T *y, const T *w, T *pp, int64_t N, int loss_mode, T loss_param, int G, int g0, int64_t tile) {
    // pp = the partial sums of the (tile of 256 x VS samples, tree) pair this wave's samples belong to: [1 + n_grad][4 waves]
    // (shared leaf rows: `tile` counts 64 x VS samples — a quarter of such a tile, entry tile & 3 of its four)
    constexpr int TILE = GBLK * VS, WSAMP = 64 * VS;
    const int tid = threadIdx.x, wave = SHARE ? (int)(tile & 3) : tid >> 6, lane = tid & 63;
    const int64_t jl = SHARE ? tile * WSAMP + (int64_t)lane * VS : tile * TILE + (int64_t)tid * VS, last = N - 1; // this lane's first sample
    T l = T(0);
    LV(T) lp, wv;
    DE_UNROLL for (int i = 0; i < VS; i++) {
        const int64_t j = jl + i;
        const int64_t jj = j < last ? j : last;
        const T yv = y[jj];
        wv[i] = j <= last ? (w ? w[jj] : T(1)) : T(0);
        const LossTerm<T> lt = loss_term<T>(loss_mode, st.x[i], yv, wv[i], loss_param);
        lp[i] = lt.lp;
        l += lt.l;
    }
    pp += wave;
    if (g0 == 0) {
        const T s = wave_sum_to_lane63(l);
        if (lane == 63) pp[0] = s;
    }
    DE_UNROLL for (int k = 0; k < GC; k++) {
        if (g0 + k < G) { // wave-uniform
            T c = T(0);
            DE_UNROLL for (int i = 0; i < VS; i++) c += wv[i] == T(0) ? T(0) : lp[i] * st.d[k][i];
            const T s = wave_sum_to_lane63(c);
            if (lane == 63) pp[(int64_t)(1 + g0 + k) * 4] = s;
        }
    }
}
// Tree end of de_eval_loss_gn under L2 (the other kinds: g_epilogue_gn_kind below): the L2 loss and its gradient as g_epilogue_loss forms them, then the Gauss-Newton products
//   sum_j w_j d_i(j) d_k(j),  i <= k < G,
// of a tree whose rows lie in this one window (g0 == 0 && G <= GC: every tree of at most de_gn_max_rows() rows), into the columns behind the
// gradient's: entry (i, k) at 1 + G + k (k + 1) / 2 + i.  One association order, (w d_i) d_k, everywhere — scaling every weight by a power of
// two scales every sum exactly.  Called by the GN instantiations of the kernel only: the others keep the register budget they had.
template <typename T, int GC, bool SHARE>
__device__ __noinline__ void g_epilogue_gn(GState<T, GC> st, const T *y, const T *w, T *pp, int64_t N, int G, int g0, int64_t tile) {
    constexpr int TILE = GBLK * VS, WSAMP = 64 * VS;
    const int tid = threadIdx.x, wave = SHARE ? (int)(tile & 3) : tid >> 6, lane = tid & 63;
    const int64_t jl = SHARE ? tile * WSAMP + (int64_t)lane * VS : tile * TILE + (int64_t)tid * VS, last = N - 1; // this lane's first sample
    T l = T(0);
    LV(T) lp, wv;
    DE_UNROLL for (int i = 0; i < VS; i++) {
        const int64_t j = jl + i;
        const int64_t jj = j < last ? j : last;
        const T yv = y[jj];
        wv[i] = j <= last ? (w ? w[jj] : T(1)) : T(0);
        const LossTerm<T> lt = loss_term<T>(1 + DE_LOSS_L2, st.x[i], yv, wv[i], T(0));
        lp[i] = lt.lp;
        l += lt.l;
    }
    pp += wave;
    if (g0 == 0) {
        const T s = wave_sum_to_lane63(l);
        if (lane == 63) pp[0] = s;
    }
    DE_UNROLL for (int k = 0; k < GC; k++) {
        if (g0 + k < G) { // wave-uniform
            T c = T(0);
            DE_UNROLL for (int i = 0; i < VS; i++) c += wv[i] == T(0) ? T(0) : lp[i] * st.d[k][i];
            const T s = wave_sum_to_lane63(c);
            if (lane == 63) pp[(int64_t)(1 + g0 + k) * 4] = s;
        }
    }
    if (g0 == 0 && G <= GC) {
        T *__restrict__ pj = pp + (int64_t)(1 + G) * 4;
        DE_UNROLL for (int k = 0; k < GC; k++) {
            if (k < G) { // wave-uniform
                DE_UNROLL for (int i = 0; i <= k; i++) {
                    T c = T(0);
                    DE_UNROLL for (int s = 0; s < VS; s++) c += wv[s] == T(0) ? T(0) : (wv[s] * st.d[i][s]) * st.d[k][s];
                    const T sum = wave_sum_to_lane63(c);
                    if (lane == 63) pj[(k * (k + 1) / 2 + i) * 4] = sum;
                }
            }
        }
    }
}
// The same tree end under any other loss kind, in two functions the kernel calls one after the other: the loss and
// gradient columns as g_epilogue_loss forms them (loss_term with the launch's kind: de_eval_loss_grad_ex's bits), the products
// ((w c) d_i) d_k with the kind's curvature weight c (de_loss_kinds.h loss_kind_curv).  g_gn_terms forms the per-sample terms, which need the
// tree's value alone, and calls both tables out of line.  What it keeps across those calls lives in callee-saved registers — every second
// block of eight from v40 on — and a kernel of this module is allotted the registers of the module's most expensive function, so it
// takes neither the dual rows (they wait in the kernel) nor any wave-uniform argument in a vector register (guni).
// g_epilogue_gn_kind then reduces the terms with the rows: a leaf, like g_epilogue_gn, that takes the rows alone and the terms one by one —
// structs of more than 16 dwords in all leave the argument registers and travel through scratch memory.  L2 never comes here: it keeps
// g_epilogue_gn, instruction for instruction.
template <typename T> struct GnTerms {
    T l;           // the lane's loss terms, summed over its samples
    LV(T) lp, wv;  // w l' and w (0 past N) per sample
    LV(T) wc;      // w c
};
template <typename T, int GC> struct GnRows { LV(T) d[GC]; };
template <typename T, bool SHARE>
__device__ __noinline__ GnTerms<T> g_gn_terms(LV(T) x, const T *y_, const T *w_, int64_t N_, int loss_mode_, T loss_param_, T loss_floor_, int64_t tile_) {
    constexpr int TILE = GBLK * VS, WSAMP = 64 * VS;
    const T *y = guni(y_), *w = guni(w_);
    const int64_t last = guni(N_) - 1, tile = guni(tile_);
    const int loss_mode = guni(loss_mode_);
    const T loss_param = guni(loss_param_), loss_floor = guni(loss_floor_);
    GnTerms<T> r;
    r.l = T(0);
    DE_UNROLL for (int i = 0; i < VS; i++) {
        const int tid = threadIdx.x;
        const int64_t j = (SHARE ? tile * WSAMP + (int64_t)(tid & 63) * VS : tile * TILE + (int64_t)tid * VS) + i;
        const int64_t jj = j < last ? j : last;
        const T yv = y[jj];
        r.wv[i] = j <= last ? (w ? w[jj] : T(1)) : T(0);
        const LossTerm<T> lt = loss_term<T>(loss_mode, x[i], yv, r.wv[i], loss_param);
        r.lp[i] = lt.lp;
        r.l += lt.l;
        r.wc[i] = r.wv[i] * loss_kind_curv_ool<T>(loss_mode - 1, x[i], yv, loss_param, loss_floor);
    }
    return r;
}
template <typename T, int GC, bool SHARE>
__device__ __noinline__ void g_epilogue_gn_kind(GnRows<T, GC> st, T l, LV(T) lp, LV(T) wv, LV(T) wc, T *pp, int G, int g0, int wave_of_tile) {
    const int tid = threadIdx.x, wave = SHARE ? wave_of_tile : tid >> 6, lane = tid & 63;
    pp += wave;
    if (g0 == 0) {
        const T s = wave_sum_to_lane63(l);
        if (lane == 63) pp[0] = s;
    }
    DE_UNROLL for (int k = 0; k < GC; k++) {
        if (g0 + k < G) { // wave-uniform
            T c = T(0);
            DE_UNROLL for (int i = 0; i < VS; i++) c += wv[i] == T(0) ? T(0) : lp[i] * st.d[k][i];
            const T s = wave_sum_to_lane63(c);
            if (lane == 63) pp[(int64_t)(1 + g0 + k) * 4] = s;
        }
    }
    if (g0 == 0 && G <= GC) {
        T *__restrict__ pj = pp + (int64_t)(1 + G) * 4;
        DE_UNROLL for (int k = 0; k < GC; k++) {
            if (k < G) { // wave-uniform
                DE_UNROLL for (int i = 0; i <= k; i++) {
                    T c = T(0);
                    DE_UNROLL for (int s = 0; s < VS; s++) c += wv[s] == T(0) ? T(0) : (wc[s] * st.d[i][s]) * st.d[k][s];
                    const T sum = wave_sum_to_lane63(c);
                    if (lane == 63) pj[(k * (k + 1) / 2 + i) * 4] = sum;
                }
            }
        }
    }
}
// Tree end of de_eval_fit_stats_grad: the fit statistics of h_tree_end_stats (de_kernels.hip) with their gradient
// moments.  ym = T(mean_y) of the pre-pass over y / w; per wave, over the samples that count (weight != 0, inside N — by selects):
//   m = the weighted mean of the tree's values, formed in T (any shift makes the recombination an identity; this one keeps the sums
//       free of cancellation)                                   W_wave = sum w              R_wave = sum w yc,  yc = y - ym
//   S1 = sum w (yhat - m)    B = sum w (yhat - m)^2    Cc = sum w (yhat - m) yc                      (window 0 writes the six)
//   D_k = sum w d_k          P'_k = sum (w d_k) (yhat - m)          Q'_k = sum (w d_k) yc             (every window: its rows)
// and, where the caller wants the matrix (want_j) and the tree's rows lie in this one window, the triangle ((w d_i) d_k) in
// g_epilogue_gn's association and column order, behind the 6 + 3 G columns.  Every product has one factor w: doubling every weight
// doubles every sum exactly and leaves m alone.  Called by the FIT instantiations of the kernel only.
template <typename T, int GC, bool SHARE>
__device__ __noinline__ void g_epilogue_fit(GState<T, GC> st, const T *y_, const T *w_, T *pp_, int64_t N_, T ym_, int G_, int g0_, int64_t tile_, int want_j_) {
    constexpr int TILE = GBLK * VS, WSAMP = 64 * VS;
    const T *y = guni(y_), *w = guni(w_);
    T *pp = const_cast<T *>(guni(static_cast<const T *>(pp_)));
    const int64_t last = guni(N_) - 1, tile = guni(tile_);
    const T ym = guni(ym_);
    const int G = guni(G_), g0 = guni(g0_), want_j = guni(want_j_);
    const int tid = threadIdx.x, wave = SHARE ? (int)(tile & 3) : tid >> 6, lane = tid & 63;
    const int64_t jl = SHARE ? tile * WSAMP + (int64_t)lane * VS : tile * TILE + (int64_t)tid * VS; // this lane's first sample
    LV(T) wv, yc;
    T sw = T(0), sy = T(0);
    DE_UNROLL for (int i = 0; i < VS; i++) {
        const int64_t j = jl + i;
        const int64_t jj = j < last ? j : last;
        yc[i] = y[jj] - ym;
        wv[i] = j <= last ? (w ? w[jj] : T(1)) : T(0);
        sw += wv[i];
        sy += wv[i] != T(0) ? wv[i] * st.x[i] : T(0);
    }
    sw = gwave_lane63(wave_sum_to_lane63(sw));
    sy = gwave_lane63(wave_sum_to_lane63(sy));
    const T m = sw != T(0) ? sy / sw : T(0);
    LV(T) dx;
    DE_UNROLL for (int i = 0; i < VS; i++) dx[i] = st.x[i] - m;
    pp += wave;
    if (g0 == 0) {
        T s1 = T(0), b = T(0), cc = T(0), r = T(0);
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const bool in = wv[i] != T(0);
            const T wd = wv[i] * dx[i];
            s1 += in ? wd : T(0);
            b = in ? M<T>::fma(wd, dx[i], b) : b;
            cc = in ? M<T>::fma(wd, yc[i], cc) : cc;
            r += in ? wv[i] * yc[i] : T(0);
        }
        s1 = wave_sum_to_lane63(s1);
        b = wave_sum_to_lane63(b);
        cc = wave_sum_to_lane63(cc);
        r = wave_sum_to_lane63(r);
        if (lane == 63) { pp[0] = m; pp[4] = s1; pp[8] = b; pp[12] = cc; pp[16] = sw; pp[20] = r; }
    }
    T *__restrict__ pd = pp + FIT_COLS * 4;
    DE_UNROLL for (int k = 0; k < GC; k++) {
        if (g0 + k < G) { // wave-uniform
            T cd = T(0), cp = T(0), cq = T(0);
            DE_UNROLL for (int i = 0; i < VS; i++) {
                const bool in = wv[i] != T(0);
                const T wdk = wv[i] * st.d[k][i];
                cd += in ? wdk : T(0);
                cp = in ? M<T>::fma(wdk, dx[i], cp) : cp;
                cq = in ? M<T>::fma(wdk, yc[i], cq) : cq;
            }
            cd = wave_sum_to_lane63(cd);
            cp = wave_sum_to_lane63(cp);
            cq = wave_sum_to_lane63(cq);
            if (lane == 63) {
                pd[(int64_t)(g0 + k) * 4] = cd;
                pd[(int64_t)(G + g0 + k) * 4] = cp;
                pd[(int64_t)(2 * G + g0 + k) * 4] = cq;
            }
        }
    }
    if (want_j && g0 == 0 && G <= GC) {
        T *__restrict__ pj = pd + (int64_t)(3 * G) * 4;
        DE_UNROLL for (int k = 0; k < GC; k++) {
            if (k < G) { // wave-uniform
                DE_UNROLL for (int i = 0; i <= k; i++) {
                    T c = T(0);
                    DE_UNROLL for (int s = 0; s < VS; s++) c += wv[s] == T(0) ? T(0) : (wv[s] * st.d[i][s]) * st.d[k][s];
                    const T sum = wave_sum_to_lane63(c);
                    if (lane == 63) pj[(k * (k + 1) / 2 + i) * 4] = sum;
                }
            }
        }
    }
}
// The Jacobian block and the values are written once and never read by the kernel: non-temporal stores (round 5: the eval kernel's output
// stream gained 2 % from them; -DDE_GRAD_NT_STORE=0 for the A/B)
#ifndef DE_GRAD_NT_STORE
#define DE_GRAD_NT_STORE 1
#endif
#if DE_GRAD_NT_STORE
#define DE_G_STORE(PTR, VAL) __builtin_nontemporal_store((VAL), (PTR))
#else
#define DE_G_STORE(PTR, VAL) (*(PTR) = (VAL))
#endif
template <typename T, int GC, bool SHARE>
__device__ __noinline__ void g_epilogue_store(GState<T, GC> st, T *out_row, T *grad_tree, int64_t N, int G, int g0, int64_t tile, uint32_t stage0) {
    // stage0 = LDS address of the wave's slot area; `tile` counts 64 x VS samples under shared leaf rows, 256 x VS otherwise
    constexpr int TILE = GBLK * VS, WSAMP = 64 * VS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t jl = SHARE ? tile * WSAMP + (int64_t)lane * VS : tile * TILE + (int64_t)tid * VS, last = N - 1; // this lane's first sample
    if (G <= GC) {
        // One window: the wave's gradient block — WSAMP samples x G rows, gradient index fastest
        // (src/EvaluateDerivative.jl:355-361) — is WSAMP*G contiguous elements in memory.  Transpose it
        // through the wave's (now idle) slot rows and write it with 16-byte stores; per-lane stores
        // would each touch 4 of every 4*G*VS bytes.
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const int64_t j = jl + i;
            if (j <= last && out_row) DE_G_STORE(out_row + j, (T)st.x[i]);
        }
        const int64_t j0 = SHARE ? tile * WSAMP : tile * TILE + (int64_t)wave * WSAMP; // first sample of this wave
        const int64_t n_valid = N - j0 < WSAMP ? N - j0 : WSAMP; // samples of this wave inside N (may be <= 0)
        if (G > 0 && n_valid > 0) {
            DE_UNROLL for (int i = 0; i < VS; i++)
                DE_UNROLL for (int k = 0; k < GC; k++)
                    if (k < G) *reinterpret_cast<__attribute__((address_space(3))) T *>((uintptr_t)(stage0 + (uint32_t)(((lane * VS + i) * G + k) * sizeof(T)))) = st.d[k][i];
            __builtin_amdgcn_wave_barrier(); // LDS is in order within a wave; this only pins the compiler
            constexpr int PER16 = 16 / (int)sizeof(T);
            T *__restrict__ gdst = grad_tree + (int64_t)G * j0;
            const int total = (int)n_valid * G; // elements to write
            const bool aligned = (reinterpret_cast<uintptr_t>(gdst) & 15) == 0;
            for (int e = lane * PER16; e < total; e += 64 * PER16) {
                typedef T V16 __attribute__((ext_vector_type(PER16)));
                const V16 v = *reinterpret_cast<__attribute__((address_space(3))) V16 *>((uintptr_t)(stage0 + (uint32_t)(e * sizeof(T))));
                if (aligned && e + PER16 <= total) DE_G_STORE(reinterpret_cast<V16 *>(gdst + e), v);
                else { DE_UNROLL for (int q = 0; q < PER16; q++) if (e + q < total) gdst[e + q] = v[q]; }
            }
            __builtin_amdgcn_wave_barrier();
        }
    } else { // several windows: every window owns a few rows of the block — direct stores
        DE_UNROLL for (int i = 0; i < VS; i++) {
            const int64_t j = jl + i;
            if (j <= last) {
                if (out_row && g0 == 0) out_row[j] = st.x[i];
                T *__restrict__ gp = grad_tree + (int64_t)G * j + g0;
                DE_UNROLL for (int k = 0; k < GC; k++)
                    if (g0 + k < G) gp[k] = st.d[k][i];
            }
        }
    }
}

// VS consecutive samples per thread; wave-major LDS: per wave, rows [0,F) = its slice of the X tile, then each
// spill slot s owns 1+GC rows (x, d[0..GC)); at least GC rows follow the X rows (output staging).
// GN: the launch of de_eval_loss_gn — the tree end is g_epilogue_gn; FIT: the launch of de_eval_fit_stats_grad — g_epilogue_fit
template <typename T, int GC, bool PARAMS, bool SHARE = false, bool GN = false, bool FIT = false>
__global__ void __launch_bounds__(GBLK) de_grad_threaded_kernel(const GArgs<T> a, const uint64_t hbase, const uint32_t param_off) {
    constexpr int TILE = GBLK * VS, WSAMP = 64 * VS; // samples per workgroup / per wave
    extern __shared__ __align__(16) unsigned char gtsmem[];
    T *__restrict__ rows = reinterpret_cast<T *>(gtsmem);

    const GTileMap tm = gmap_block_prio(a, blockIdx.x);
    if (!tm.valid) return;
    const int flag_protocol = tm.prio ? 1 : a.skip_flagged;
    const int tid = threadIdx.x;
    // SHARED LEAF ROWS (GArgs::share): the tile is one wave's 64 x VS samples, staged once for the four waves — rows [0, F) —, behind them
    // every wave's slot rows; wave w runs trees t0 + w, t0 + w + 4, ... of the chunk through stream variant w
    constexpr bool share = SHARE; // (a template parameter: the per-wave-copy kernel keeps the code it had)
    const int wave = share ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int64_t base = tm.tile * (share ? WSAMP : TILE);
    const int64_t last = a.N - 1;
    const int g0 = (int)blockIdx.y * GC; // first gradient component of this window
    const int F = a.F;
    const int slot_rows = a.n_slots * (1 + GC) > GC ? a.n_slots * (1 + GC) : GC;
    const int R = F + slot_rows; // rows per wave
    if (share) {
        // (stage_x_rows / stage_param_rows of de_grad_common.h with the map (j, f) -> f * WSAMP + j, spelled out: through the helpers this
        // branch alone compiles to other code — same IR, other block order; Float32 +2 instructions, Float64 up to +38 — TUNING_LOG.md)
        const uint32_t Fu = (uint32_t)a.FX, total = (uint32_t)WSAMP * Fu;
        for (uint32_t e = tid; e < total; e += GBLK) {
            const uint32_t j = e / Fu, f = e - j * Fu;
            int64_t jj = base + j;
            jj = jj < last ? jj : last;
            rows[f * WSAMP + j] = a.X[f + a.ldX * jj];
        }
        if (PARAMS) {
            const uint32_t Pu = (uint32_t)(F - a.FX), totalp = (uint32_t)WSAMP * Pu;
            for (uint32_t e = tid; e < totalp; e += GBLK) {
                const uint32_t j = e / Pu, q = e - j * Pu;
                int64_t jj = base + j;
                jj = jj < last ? jj : last;
                const int64_t cl = clamp_class((a.classes_is_i64 ? reinterpret_cast<const int64_t *>(a.classes)[jj] : (int64_t) reinterpret_cast<const int32_t *>(a.classes)[jj]) - a.class_base, a.n_classes);
                rows[((uint32_t)a.FX + q) * WSAMP + j] = a.params[q + a.ld_params * cl];
            }
        }
    } else { // one copy of the leaf rows per wave
        const uint32_t FX = (uint32_t)a.FX, Ru = (uint32_t)R;
        const auto at = [Ru](uint32_t j, uint32_t f) { return ((j / WSAMP) * Ru + f) * WSAMP + (j % WSAMP); };
        stage_x_rows<T>(rows, a.X, a.ldX, FX, TILE, base, last, at);
        if (PARAMS) stage_param_rows<T>(rows, a.params, a.ld_params, a.classes, a.classes_is_i64, a.class_base, a.n_classes, FX, (uint32_t)F - FX, TILE, base, last, at);
    }
    __syncthreads();

    const ConstU4Ptr code = (ConstU4Ptr)(uintptr_t)(a.code + (share ? (int64_t)wave * a.var_stride : (int64_t)0));
    const ConstI32Ptr code_off = (ConstI32Ptr)(uintptr_t)a.code_off;
    const ConstI64Ptr col_off = (ConstI64Ptr)(uintptr_t)a.col_off;
    const ConstI64Ptr grad_off = (ConstI64Ptr)(uintptr_t)a.grad_off;
    const ConstI32Ptr n_grad = (ConstI32Ptr)(uintptr_t)a.n_grad;
    const int t0 = tm.chunk * a.trees_per_chunk;
    const int t1 = (t0 + a.trees_per_chunk < a.n_trees) ? t0 + a.trees_per_chunk : a.n_trees;
    const uint32_t wave_base = (uint32_t)(uintptr_t)gtsmem + (share ? 0u : (uint32_t)(wave * R) * grow_bytes<T>());
    const uint32_t lds0 = wave_base + (uint32_t)(tid & 63) * (uint32_t)(VS * sizeof(T));
    const uint32_t stage0 = wave_base + (uint32_t)(F + (share ? wave * slot_rows : 0)) * grow_bytes<T>(); // the wave's slot area, free between trees
    const int64_t ptile = share ? (int64_t)tm.tile >> 2 : (int64_t)tm.tile; // (the tile of 256 x VS samples the partial sums are kept by)

    const ConstI32Ptr tree_ids = (ConstI32Ptr)(uintptr_t)a.tree_ids;
    const uint64_t skip = gskip_mask(a.ok, tree_ids, t0, t1, flag_protocol, (int64_t)tm.tile);
    for (int ti = share ? t0 + wave : t0; ti < t1; ti += share ? 4 : 1) {
        if ((skip >> (ti - t0)) & 1ull) continue; // already incomplete (early exit)
        const int tree = tree_ids[ti];
        const int G = n_grad[tree];
        if (g0 >= G && g0 > 0) continue; // window without a component of this tree (window 0 always runs: x, flag)
        int pc = code_off[tree];
        const int pe = code_off[tree + 1];
        GState<T, GC> st;
        st.x = lv_splat<T>(T(0));
        DE_UNROLL for (int k = 0; k < GC; k++) st.d[k] = lv_splat<T>(T(0));
        st.poison = T(0);
        st.g0 = (uint32_t)g0 | (lds0 & 0xFFFF0000u); // window offset (< 2^16) | upper half of the lane's LDS base (g_gen)
        {   // one call per tree: the chain ends in the tree's end record (g_end)
            const ConstU4Ptr rec = code + pc;
            const U32x4 hd = *rec;
            const uint32_t first = code[pe - 1].x; // the end record names the tree's first handler (every other record: its successor's)
            st = reinterpret_cast<GHandlerFn<T, GC>>(hbase + first)(st, lds0, rec + 1, hbase, hd.x, hd.y, grec_imm<T>(hd));
        }
        // a non-finite d[k] always survives to the root (every update is linear in it), so the gradient
        // is validity-tested once, here; x was tested where the lowering kept a test (H_CHECK_OUT)
        T poison = st.poison;
        gpoison<T>(poison, st.x);
        // only the components this tree really has: a window is as wide as its bucket, and a column beyond
        // n_grad (the lone column of a tree without constants in constant mode) holds g*0 terms that are NaN
        // for an infinite partial although the reference's gradient matrix has no such row
        DE_UNROLL for (int k = 0; k < GC; k++) gpoison<T>(poison, g0 + k < G ? st.d[k] : lv_splat<T>(T(0)));
        if constexpr (FIT) {
            const int64_t n_cols = col_off[a.n_all_trees];
            g_epilogue_fit<T, GC, SHARE>(st, a.y, a.w, a.partial + (ptile * n_cols + col_off[tree]) * 4, a.N, a.loss_param, G, g0, (int64_t)tm.tile, a.loss_mode == FIT_MODE_JTJ);
        } else if constexpr (GN) {
            const int64_t n_cols = col_off[a.n_all_trees];
            T *pp = a.partial + (ptile * n_cols + col_off[tree]) * 4;
            if (a.loss_mode == 1 + DE_LOSS_L2) g_epilogue_gn<T, GC, SHARE>(st, a.y, a.w, pp, a.N, G, g0, (int64_t)tm.tile);
            else {
                GnRows<T, GC> rows_;
                DE_UNROLL for (int k = 0; k < GC; k++) rows_.d[k] = st.d[k];
                const GnTerms<T> t_ = g_gn_terms<T, SHARE>(st.x, a.y, a.w, a.N, a.loss_mode, a.loss_param, a.loss_floor, (int64_t)tm.tile);
                g_epilogue_gn_kind<T, GC, SHARE>(rows_, t_.l, t_.lp, t_.wv, t_.wc, pp, G, g0, (int)(tm.tile & 3));
            }
        } else if (a.loss_mode) {
            const int64_t n_cols = col_off[a.n_all_trees];
            g_epilogue_loss<T, GC, SHARE>(st, a.y, a.w, a.partial + (ptile * n_cols + col_off[tree]) * 4, a.N, a.loss_mode, a.loss_param, G, g0, (int64_t)tm.tile);
        } else {
            g_epilogue_store<T, GC, SHARE>(st, a.out ? a.out + (int64_t)tree * a.ld_out : nullptr, a.grad + grad_off[tree], a.N, G, g0, (int64_t)tm.tile, stage0);
        }
        if (__ballot(poison != poison) != 0ull) gflag_incomplete(a.ok + tree, flag_protocol == 1);
    }
}

} // module namespace

// ---- host side: what this (type, window, samples per lane) module exports; the launch is de_grad_kernels.hip launch_grad_kernel --------
GradModule DE_GT_NAME(grad_thr_module_)() {
    using namespace DE_GT_NAME(gtm_);
    typedef DE_GT_T T;
    constexpr int GC = DE_GT_GC;
    GradModule m;
    m.fill = reinterpret_cast<const void *>(&de_grad_fill_handlers<T, GC>);
    m.kernel[1][0] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, true, false>);
    m.kernel[0][0] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, false, false>);
    m.kernel[1][1] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, true, true>);
    m.kernel[0][1] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, false, true>);
    m.kernel_gn[1][0] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, true, false, true>);
    m.kernel_gn[0][0] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, false, false, true>);
    m.kernel_gn[1][1] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, true, true, true>);
    m.kernel_gn[0][1] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, false, true, true>);
    m.kernel_fit[1][0] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, true, false, false, true>);
    m.kernel_fit[0][0] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, false, false, false, true>);
    m.kernel_fit[1][1] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, true, true, false, true>);
    m.kernel_fit[0][1] = reinterpret_cast<const void *>(&de_grad_threaded_kernel<T, GC, false, true, false, true>);
    return m;
}

} // namespace de
