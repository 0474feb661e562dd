// de_nm.h — the per-tree arithmetic of the device-side Nelder-Mead fit, one source for both sides: the kernels of
// de_nm.hip and the host-only hooks de_nm_ask_host / de_nm_tell_host (de_api_fit.cpp) run this code, so they give the same bits (every
// translation unit is built with -ffp-contract=off; double division is correctly rounded on both sides).
// The method: the steps of Lagarias, Reeds, Wright & Wright (1998), the dimension-adaptive coefficients of Gao & Han (2012) and the
// affine start simplex V_k = V_0 + (b V_0[k-1] + a) e_k — restated from the papers, one evaluation per round.
//   state of one tree of G constants (1 <= G <= 32), all double: V[(G + 1) x G] row-major, f[G + 1], c[G], xr[G], fr;
//   st[3] = {phase, cursor, l0} (int32)
//   rounding: every evaluated coordinate is T(.) first and enters the state as the double of that; every f is the double of a T loss,
//   +Inf for a failed evaluation, never NaN
//   order: l = argmin f (ties: lowest index), h = argmax f (ties: highest), s = argmax over i != h (ties: highest)
// ask writes the trial of the tree's phase, tell takes its loss F.  A function below serves coordinates [jb, je): the host calls it with
// [0, G), lane j of a wave with [j, j + 1) (lanes >= G with an empty range); `lead` (the host, lane 0) writes the scalars, behind
// DE_NM_SYNC() — every lane has read them by then.  No step reduces across coordinates: the centroid is a sum over vertices.
#ifndef DE_NM_H
#define DE_NM_H
#include <cstdint>
#include "de_lm_solve.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DE_NM_SYNC() __syncthreads()
#else
#define DE_NM_SYNC() ((void)0)
#endif

namespace de {

constexpr int NM_MAX_ROWS = 32; // the widest tree that is fitted
enum : int32_t { NM_BUILD = 0, NM_REFLECT = 1, NM_EXPAND = 2, NM_CONTRACT_OUT = 3, NM_CONTRACT_IN = 4, NM_SHRINK = 5, NM_DONE = 6,
                 NM_OFF = 7 /* the kernels' mark of a tree that is not fitted */ };

DE_LM_HD double nm_inf() { return __builtin_inf(); }
// what a loss call returned, as the state stores it
DE_LM_HD double nm_loss(double f, bool ok) { return ok && lm_finite(f) ? f : nm_inf(); }
template <typename T> DE_LM_HD double nm_round(double v) { return (double)(T)v; }

// G >= 2: Gao & Han; G == 1: the classical values (the adaptive delta would be 0 and collapse the simplex)
struct NmCoef { double alpha, beta, gamma, delta; };
DE_LM_HD NmCoef nm_coef(int G) {
    if (G < 2) return NmCoef{1.0, 2.0, 0.5, 0.5};
    return NmCoef{1.0, 1.0 + 2.0 / (double)G, 0.75 - 1.0 / (2.0 * (double)G), 1.0 - 1.0 / (double)G};
}
struct NmOrder { int l, s, h; };
DE_LM_HD NmOrder nm_order(const double *f, int G) {
    int l = 0, h = 0, s = -1;
    for (int i = 1; i <= G; i++) {
        if (f[i] < f[l]) l = i;
        if (f[i] >= f[h]) h = i;
    }
    for (int i = 0; i <= G; i++)
        if (i != h && (s < 0 || f[i] >= f[s])) s = i;
    return NmOrder{l, s, h};
}

// ---- the coordinate primitives: the only arithmetic on coordinates --------------------------------------------------------------------------
template <typename T> DE_LM_HD double nm_build_coord(double v0, double a, double b) { return nm_round<T>((1.0 + b) * v0 + a); }
// coordinate j of the centroid of every vertex but h, i ascending
DE_LM_HD double nm_centroid_coord(const double *V, int G, int j, int h) {
    double s = 0.0;
    for (int i = 0; i <= G; i++)
        if (i != h) s = s + V[i * G + j];
    return s / (double)G;
}
template <typename T> DE_LM_HD double nm_reflect_coord(double c, double vh, double alpha) { return nm_round<T>(c + alpha * (c - vh)); }
// c + k (xr - c): the expansion (k = beta) and the outside contraction (k = gamma); c - k (xr - c): the inside contraction
template <typename T> DE_LM_HD double nm_out_coord(double c, double xr, double k) { return nm_round<T>(c + k * (xr - c)); }
template <typename T> DE_LM_HD double nm_in_coord(double c, double xr, double k) { return nm_round<T>(c - k * (xr - c)); }
template <typename T> DE_LM_HD double nm_shrink_coord(double vl, double vi, double delta) { return nm_round<T>(vl + delta * (vi - vl)); }
// the trial of the three phases that follow a reflection, from c and xr alone (tell recomputes what ask wrote)
template <typename T> DE_LM_HD double nm_second_coord(int phase, const NmCoef &k, double c, double xr) {
    return phase == NM_EXPAND ? nm_out_coord<T>(c, xr, k.beta) : phase == NM_CONTRACT_OUT ? nm_out_coord<T>(c, xr, k.gamma) : nm_in_coord<T>(c, xr, k.gamma);
}

// ---- ask: the trial of the tree's phase into trial[jb .. je) --------------------------------------------------------------------------------
// BUILD and SHRINK write the vertex they evaluate; REFLECT writes c and xr, or moves to DONE where f_h - f_l <= f_tol |f_l|.  The caller
// has checked 1 <= G <= NM_MAX_ROWS.
template <typename T>
DE_LM_HD void nm_ask_tree(int G, int jb, int je, bool lead, double a, double b, double f_tol, double *V, const double *f, int32_t *st, double *c,
                          double *xr, T *trial) {
    const int32_t phase = st[0], cur = st[1], l0 = st[2];
    const NmCoef k = nm_coef(G);
    if (phase == NM_BUILD) {
        for (int j = jb; j < je; j++) {
            const double v = j == cur - 1 ? nm_build_coord<T>(V[j], a, b) : V[j];
            V[cur * G + j] = v;
            trial[j] = (T)v;
        }
    } else if (phase == NM_REFLECT) {
        const NmOrder o = nm_order(f, G);
        if (f[o.h] - f[o.l] <= f_tol * fabs(f[o.l])) { // (uniform; NaN, from an infinite f, compares false)
            for (int j = jb; j < je; j++) trial[j] = (T)V[o.l * G + j];
            DE_NM_SYNC();
            if (lead) st[0] = NM_DONE;
            return;
        }
        for (int j = jb; j < je; j++) {
            const double cj = nm_centroid_coord(V, G, j, o.h);
            const double x = nm_reflect_coord<T>(cj, V[o.h * G + j], k.alpha);
            c[j] = cj;
            xr[j] = x;
            trial[j] = (T)x;
        }
    } else if (phase == NM_EXPAND || phase == NM_CONTRACT_OUT || phase == NM_CONTRACT_IN) {
        for (int j = jb; j < je; j++) trial[j] = (T)nm_second_coord<T>(phase, k, c[j], xr[j]);
    } else if (phase == NM_SHRINK) {
        for (int j = jb; j < je; j++) {
            const double v = nm_shrink_coord<T>(V[l0 * G + j], V[cur * G + j], k.delta);
            V[cur * G + j] = v;
            trial[j] = (T)v;
        }
    } else { // NM_DONE: the accepted constants
        const NmOrder o = nm_order(f, G);
        for (int j = jb; j < je; j++) trial[j] = (T)V[o.l * G + j];
    }
}

// ---- tell: F = nm_loss(the trial's loss, its flag) ------------------------------------------------------------------------------------------
template <typename T>
DE_LM_HD void nm_tell_tree(int G, int jb, int je, bool lead, double *V, double *f, int32_t *st, const double *c, const double *xr, double *fr,
                           double F) {
    const int32_t phase = st[0], cur = st[1], l0 = st[2];
    if (phase == NM_DONE) return;
    const NmCoef k = nm_coef(G);
    const NmOrder o = nm_order(f, G);
    const double frv = *fr, fl = f[o.l], fs = f[o.s], fh = f[o.h];
    DE_NM_SYNC();
    if (phase == NM_BUILD || phase == NM_SHRINK) { // the vertex is in place: its loss, and the cursor moves on
        if (!lead) return;
        f[cur] = F;
        int next = cur + 1;
        if (phase == NM_SHRINK && next == l0) next++;
        if (next > G) st[0] = NM_REFLECT;
        else st[1] = next;
        return;
    }
    int32_t to = NM_REFLECT;
    bool take_trial = false, take_xr = false, shrink = false;
    if (phase == NM_REFLECT) {
        if (F < fl) to = NM_EXPAND;
        else if (F < fs) take_xr = true;
        else if (F < fh) to = NM_CONTRACT_OUT;
        else to = NM_CONTRACT_IN;
    } else if (phase == NM_EXPAND) {
        take_trial = F < frv;
        take_xr = !take_trial;
    } else if (phase == NM_CONTRACT_OUT) {
        take_trial = F <= frv;
        shrink = !take_trial;
    } else { // NM_CONTRACT_IN
        take_trial = F < fh;
        shrink = !take_trial;
    }
    if (take_trial)
        for (int j = jb; j < je; j++) V[o.h * G + j] = nm_second_coord<T>(phase, k, c[j], xr[j]);
    if (take_xr)
        for (int j = jb; j < je; j++) V[o.h * G + j] = xr[j];
    if (!lead) return;
    if (phase == NM_REFLECT) *fr = F;
    if (take_trial) f[o.h] = F;
    if (take_xr) f[o.h] = phase == NM_REFLECT ? F : frv;
    if (shrink) { // the anchor is fixed for the whole shrink; every other vertex, ascending, one round each
        st[0] = NM_SHRINK;
        st[1] = o.l == 0 ? 1 : 0;
        st[2] = o.l;
    } else {
        st[0] = to;
    }
}

} // namespace de
#endif
