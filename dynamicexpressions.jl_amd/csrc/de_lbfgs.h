// de_lbfgs.h — the per-tree arithmetic of the device-side L-BFGS fit, one source for both sides: the kernels of
// de_lbfgs.hip and the host-only hooks de_lbfgs_direction_host / de_lbfgs_update_host (de_api_fit.cpp) instantiate THE SAME templates, so
// they give the same bits (every translation unit is built with -ffp-contract=off; double division and square root are correctly rounded
// on both sides).  For the trees de_bfgs.h does not reach: 1 <= G <= 4096 unknowns, the state O(m G) instead of G^2.
//   ring       up to m pairs S[j][0 .. G), Y[j][0 .. G), rho[j] = 1 / (s_j . y_j); count in 0 .. m of them are stored, head is the next slot
//              to write: the i-th newest pair is slot (head - 1 - i) mod m
//   direction  the two-loop recursion: q = g; newest to oldest a_i = rho_i (s_i . q), q -= a_i y_i; r = (s . y / y . y of the newest) q;
//              oldest to newest b = rho_i (y_i . r), r += (a_i - b) s_i; p = -r, slope = g . p (count = 0: p = -g).
//              !(slope < 0): count = 0, p = -g, slope = -g . g, alpha = a0(g)
//   update     s = c_trial - c, yv = g_trial - g, stored in slot head only where s . yv > curv |s| |yv| (bfgs_curvature)
// Everything is in double.  EVERY dot product is lbfgs_dot's: 64 partial sums, partial l over k = l, l + 64, ... ascending from 0.0, one
// product at a time, then the partials added in the order l = 0 .. 63 from 0.0 — no lane adds G terms in a row at G = 4096.  The vectors
// are owned the same way: lane l touches the entries k = l mod 64 only, so q and r live in p itself and need no barrier of their own.
// A `Team` is the 64 lanes: LbfgsHostTeam runs them one after the other, the kernels' team (de_lbfgs.hip) is one wave.
#ifndef DE_LBFGS_H
#define DE_LBFGS_H
#include <cstdint>
#include "de_bfgs.h"

namespace de {

constexpr int LBFGS_MAX_ROWS = 4096; // the widest tree that is fitted (P = 8 parameters x 511 classes + 8 constants)
constexpr int LBFGS_MAX_MEMORY = 16; // the longest ring
constexpr int LBFGS_LANES = 64;

// partial l of sum_k p[k] q[k]
template <class A, class B> DE_LM_HD double lbfgs_dot_part(const A *p, const B *q, int n, int l) {
    double s = 0.0;
    for (int k = l; k < n; k += LBFGS_LANES) s = s + (double)p[k] * (double)q[k];
    return s;
}
DE_LM_HD double lbfgs_sum(const double *part) {
    double s = 0.0;
    for (int l = 0; l < LBFGS_LANES; l++) s = s + part[l];
    return s;
}
// the slot of the i-th newest pair (0 <= i < m, 0 <= head < m)
DE_LM_HD int lbfgs_slot(int head, int i, int m) { return (head - 1 - i + m) % m; }

// The lanes on one host thread.  each(f): f(l) for every lane; all(f): the conjunction of f(l); one(f): what one lane does for the tree;
// dot: lbfgs_dot; set_a / a: the a_i of the recursion; sync: between a read of the tree's scalars by every lane and their write by one.
struct LbfgsHostTeam {
    double part[LBFGS_LANES], av[LBFGS_MAX_MEMORY];
    template <class F> void each(F f) {
        for (int l = 0; l < LBFGS_LANES; l++) f(l);
    }
    template <class F> bool all(F f) {
        bool r = true;
        for (int l = 0; l < LBFGS_LANES; l++) r = f(l) && r;
        return r;
    }
    template <class F> void one(F f) { f(); }
    template <class A, class B> double dot(const A *p, const B *q, int n) {
        for (int l = 0; l < LBFGS_LANES; l++) part[l] = lbfgs_dot_part(p, q, n, l);
        return lbfgs_sum(part);
    }
    void set_a(int i, double v) { av[i] = v; }
    double a(int i) const { return av[i]; }
    void sync() {}
};

struct LbfgsDir {
    int produced, count; // count: 0 where the state was reset, else unchanged
    double slope, alpha; // alpha: a0(g) where the state was reset, else unchanged
};
// One tree (1 <= G <= LBFGS_MAX_ROWS, 1 <= m <= LBFGS_MAX_MEMORY, 0 <= count <= m, 0 <= head < m).  g: the gradient in its own element
// type.  p receives the direction (zeros where none is produced: an entry of g or of a stored pair not finite, or no descent).  The ring
// is only read; the caller stores the returned count, slope and alpha.
template <class Team, class GT>
DE_LM_HD LbfgsDir lbfgs_direction(Team &tm, int G, int m, const double *S, const double *Y, const double *rho, int count, int head, double alpha,
                                  const GT *g, double step0, double *p) {
    const bool fin = tm.all([&](int l) {
        bool f = true;
        for (int k = l; k < G; k += LBFGS_LANES) f = f && lm_finite((double)g[k]);
        for (int i = 0; i < count; i++) {
            const double *s = S + (int64_t)lbfgs_slot(head, i, m) * G, *y = Y + (int64_t)lbfgs_slot(head, i, m) * G;
            for (int k = l; k < G; k += LBFGS_LANES) f = f && lm_finite(s[k]) && lm_finite(y[k]);
        }
        return f;
    });
    tm.each([&](int l) {
        for (int k = l; k < G; k += LBFGS_LANES) p[k] = (double)g[k];
    });
    for (int i = 0; i < count; i++) { // newest to oldest
        const int j = lbfgs_slot(head, i, m);
        const double *s = S + (int64_t)j * G, *y = Y + (int64_t)j * G;
        const double a = rho[j] * tm.dot(s, p, G);
        tm.set_a(i, a);
        tm.each([&](int l) {
            for (int k = l; k < G; k += LBFGS_LANES) p[k] = p[k] - a * y[k];
        });
    }
    if (count > 0) {
        const int jn = lbfgs_slot(head, 0, m);
        const double *sn = S + (int64_t)jn * G, *yn = Y + (int64_t)jn * G;
        const double sy = tm.dot(sn, yn, G), yy = tm.dot(yn, yn, G);
        const double gamma = sy / yy;
        tm.each([&](int l) {
            for (int k = l; k < G; k += LBFGS_LANES) p[k] = gamma * p[k];
        });
        for (int i = count - 1; i >= 0; i--) { // oldest to newest
            const int j = lbfgs_slot(head, i, m);
            const double *s = S + (int64_t)j * G, *y = Y + (int64_t)j * G;
            const double b = rho[j] * tm.dot(y, p, G);
            const double d = tm.a(i) - b;
            tm.each([&](int l) {
                for (int k = l; k < G; k += LBFGS_LANES) p[k] = p[k] + d * s[k];
            });
        }
    }
    tm.each([&](int l) {
        for (int k = l; k < G; k += LBFGS_LANES) p[k] = -p[k];
    });
    LbfgsDir r;
    r.count = count;
    r.alpha = alpha;
    r.slope = tm.dot(g, p, G);
    if (!(r.slope < 0.0)) { // no descent direction: the state is reset
        const double gg = tm.dot(g, g, G);
        tm.each([&](int l) {
            for (int k = l; k < G; k += LBFGS_LANES) p[k] = -(double)g[k];
        });
        r.count = 0;
        r.alpha = bfgs_a0(gg, step0);
        r.slope = -gg;
    }
    r.produced = fin && r.slope < 0.0 ? 1 : 0;
    if (!r.produced)
        tm.each([&](int l) {
            for (int k = l; k < G; k += LBFGS_LANES) p[k] = 0.0;
        });
    return r;
}

// Returns `updated`; otherwise no byte of the state changes.  s, yv: G doubles outside the ring.
template <class Team>
DE_LM_HD int lbfgs_update(Team &tm, int G, int m, double *S, double *Y, double *rho, int32_t *count, int32_t *head, const double *s,
                          const double *yv, double curv) {
    const int n = *count, h = *head;
    tm.sync();
    const double sy = tm.dot(s, yv, G), ss = tm.dot(s, s, G), yy = tm.dot(yv, yv, G);
    if (!bfgs_curvature(sy, ss, yy, curv)) return 0;
    double *sd = S + (int64_t)h * G, *yd = Y + (int64_t)h * G;
    tm.each([&](int l) {
        for (int k = l; k < G; k += LBFGS_LANES) {
            sd[k] = s[k];
            yd[k] = yv[k];
        }
    });
    tm.one([&]() {
        rho[h] = 1.0 / sy;
        *head = (h + 1) % m;
        *count = n < m ? n + 1 : m;
    });
    return 1;
}

} // namespace de
#endif
