// de_ties.h — the arithmetic of tied constants, one source for both sides: the kernels of de_ties.hip and the host-only
// hooks de_ties_*_host (de_api_fit.cpp) run this code, so they give the same bits (every translation unit is built with -ffp-contract=off).
// A GraphNode constant that is shared fills several constant slots of its tree; the tied fits treat it as ONE unknown:
//   tie[s]   the 0-based unique constant of slot s within its tree, in first-occurrence order (slot 0 has id 0, a new id is the largest
//            id before it + 1): Population._occ[t], the identity for a tree that shares nothing
//   pack     unique[u] = slots[first slot of u]          (bits: NaN payloads and -0 stay)
//   unpack   slots[s] = unique[tie[s]]                   (bits)
//   fold     g_u = sum over the slots s of u, ascending, from +0      (np.add.at into zeros: a lone -0 row becomes +0)
//   fold_matrix  S H S^T, rows first then columns: half[u][k] = sum_{s in u} H[s][k], Hu[u][v] = sum_{k in v} half[u][k], each from +0
// The slot lists are a CSR table: list[off[u] .. off[u + 1]) = the slots of unknown u, ascending.
#ifndef DE_TIES_H
#define DE_TIES_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define DE_TIES_HD __host__ __device__ inline
#else
#define DE_TIES_HD inline
#endif

namespace de {

// The number of unknowns of a tree's map, or -1: a negative id, or an id that is not (largest id before it) + 1 at its first occurrence.
DE_TIES_HD int64_t ties_unknowns(int64_t n_slots, const int32_t *tie) {
    int64_t U = 0;
    for (int64_t s = 0; s < n_slots; s++) {
        const int64_t id = tie ? tie[s] : s;
        if (id < 0 || id > U) return -1;
        if (id == U) U++;
    }
    return U;
}

// The CSR table of a checked map: off[0 .. U] and list[0 .. n_slots), the slots numbered from `base`.  off doubles as the fill cursor.
DE_TIES_HD void ties_csr(int64_t n_slots, const int32_t *tie, int64_t U, int64_t base, int64_t *off, int64_t *list) {
    for (int64_t u = 0; u <= U; u++) off[u] = 0;
    for (int64_t s = 0; s < n_slots; s++) off[(tie ? tie[s] : s) + 1]++;
    for (int64_t u = 0; u < U; u++) off[u + 1] += off[u];
    for (int64_t s = 0; s < n_slots; s++) list[off[tie ? tie[s] : s]++] = base + s; // (off[u] is now the END of u's list)
    for (int64_t u = U; u > 0; u--) off[u] = off[u - 1];
    off[0] = 0;
}

// g_u: the rows list[0 .. n) of g summed in list order, from +0
template <typename T>
DE_TIES_HD T ties_fold(const T *g, const int64_t *list, int64_t n) {
    T acc = (T)0;
    for (int64_t k = 0; k < n; k++) acc = acc + g[list[k]];
    return acc;
}

// Hu[u][v] of a column-major S x S block H; the lists hold slots numbered from `base` (the tree's first slot)
template <typename T>
DE_TIES_HD T ties_fold_matrix(const T *H, int64_t S, int64_t base, const int64_t *list_u, int64_t n_u, const int64_t *list_v, int64_t n_v) {
    T acc = (T)0;
    for (int64_t j = 0; j < n_v; j++) {
        const T *col = H + S * (list_v[j] - base);
        T half = (T)0;
        for (int64_t i = 0; i < n_u; i++) half = half + col[list_u[i] - base];
        acc = acc + half;
    }
    return acc;
}

} // namespace de
#endif
