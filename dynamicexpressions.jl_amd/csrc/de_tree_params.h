// de_tree_params.h — the arithmetic of the per-tree parameter entry points, one source for both sides: the kernels of
// de_tree_params.hip and the host-only hook de_tree_params_accumulate_host (de_api_tree_params.cpp) run this code, so they give the same
// bits (every translation unit is built with -ffp-contract=off).  Everything is accumulated in double, one addition at a time, classes
// ascending and — inside a dparams cell — occurrences in slot order; the result is rounded once to the element type, NaN where the
// tree's flag is 0.
#ifndef DE_TREE_PARAMS_H
#define DE_TREE_PARAMS_H
#include <cstdint>

#include "de_lm_solve.h" // DE_LM_HD

namespace de {

// acc + one class's entry
template <typename T>
DE_LM_HD double tp_add(double acc, T v) { return acc + (double)v; }

// the dparams cell (p, class) of one tree: the class's gradient entries of the slots that stand for row p, in slot order
template <typename T>
DE_LM_HD double tp_cell(const T *dloss_c, const int32_t *slot_param, int64_t n_slots, int32_t p) {
    double s = 0.0;
    for (int64_t k = 0; k < n_slots; k++)
        if (slot_param[k] == p) s = s + (double)dloss_c[k];
    return s;
}

// an accumulator as the caller sees it
template <typename T>
DE_LM_HD T tp_finish(double acc, uint8_t ok) { return ok ? (T)acc : (T)__builtin_nan(""); }

} // namespace de
#endif
