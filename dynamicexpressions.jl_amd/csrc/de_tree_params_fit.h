// de_tree_params_fit.h — the index map of de_fit_tree_params_bfgs, one source for both sides: the pack / unpack kernels
// of de_tree_params.hip and the host-only hooks de_tree_params_pack_host / de_tree_params_unpack_host (de_api_tree_params.cpp) run this
// code.  The unknowns of a tree are the reference's vcat(constants, parameters[:]): its real constant slots (slot_param < 0) in slot order,
// then every entry of its [n_params, n_classes] matrix, column-major.  A table entry names where unknown u lives:
//   m >= 0   constant slot m
//   m <  0   parameter cell d = -(m + 1), counted densely (d = p + n_params * (c + n_classes * t)); in a block whose columns are ld apart
//            it is element tpf_cell(d, n_params, ld)
// Values are copied, never converted: every bit of a NaN or a -0 survives a pack and an unpack.
#ifndef DE_TREE_PARAMS_FIT_H
#define DE_TREE_PARAMS_FIT_H
#include <cstdint>

#include "de_lm_solve.h" // DE_LM_HD

namespace de {

// unknowns of a tree with n_real real constants
DE_LM_HD int64_t tpf_unknowns(int64_t n_real, int32_t n_params, int64_t n_classes) { return n_real + (int64_t)n_params * n_classes; }

// the table of ONE tree: `map` takes tpf_unknowns entries; slot0 / cell0: the tree's first constant slot / dense parameter cell.
// Returns the number of entries written.
DE_LM_HD int64_t tpf_map_tree(int64_t n_slots, const int32_t *slot_param, int32_t n_params, int64_t n_classes, int64_t slot0, int64_t cell0,
                              int64_t *map) {
    int64_t u = 0;
    for (int64_t s = 0; s < n_slots; s++)
        if (slot_param[s] < 0) map[u++] = slot0 + s;
    for (int64_t d = 0; d < (int64_t)n_params * n_classes; d++) map[u++] = -(cell0 + d + 1);
    return u;
}

// dense cell d in a block with leading dimension ld (n_params > 0 wherever a cell exists)
DE_LM_HD int64_t tpf_cell(int64_t d, int32_t n_params, int64_t ld) { return d % n_params + ld * (d / n_params); }

template <typename T>
DE_LM_HD T tpf_load(int64_t m, const T *slots, const T *cells, int32_t n_params, int64_t ld) {
    return m >= 0 ? slots[m] : cells[tpf_cell(-(m + 1), n_params, ld)];
}

template <typename T>
DE_LM_HD void tpf_store(int64_t m, T v, T *slots, T *cells, int32_t n_params, int64_t ld) {
    if (m >= 0) slots[m] = v;
    else cells[tpf_cell(-(m + 1), n_params, ld)] = v;
}

} // namespace de
#endif
