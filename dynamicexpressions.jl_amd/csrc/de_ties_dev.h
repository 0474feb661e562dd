// de_ties_dev.h — launchers of de_ties.hip: the pack, unpack and fold kernels around every evaluation of a tied fit.
#ifndef DE_TIES_DEV_H
#define DE_TIES_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// The tie tables of a population, on the device (uploaded once per fit call).  Slots and unknowns are numbered over the whole population,
// in de_program_set_consts order: tree t owns the slots slot_off[t] .. slot_off[t + 1) and the unknowns unk_tree_off[t] .. unk_tree_off[t + 1).
struct TieArgs {
    int64_t n_trees, n_slots, n_unknowns;
    const int64_t *slot_unk;     // n_slots: the unknown of every slot
    const int64_t *unk_off;      // n_unknowns + 1: CSR offsets into unk_slots
    const int64_t *unk_slots;    // n_slots: the slots of every unknown, ascending
    const int64_t *slot_off;     // n_trees + 1
    const int64_t *unk_tree_off; // n_trees + 1
    // fold_matrix only: the element offsets of every tree's S x S occurrence block and of its U x U block (both column-major), and the
    // largest S whose occurrence block the evaluation formed — a tree of more slots gets a NaN block where U <= max_slots (no step is
    // solved from it), none else
    const int64_t *hoff, *huoff;
    int32_t max_slots;
};
// unique[u] = slots[first slot of u]: one thread per unknown
hipError_t launch_ties_pack(int dtype, const TieArgs &a, const void *slots, void *unique, hipStream_t stream);
// slots[s] = unique[slot_unk[s]]: one thread per slot
hipError_t launch_ties_unpack(int dtype, const TieArgs &a, const void *unique, void *slots, hipStream_t stream);
// g_unique[u] = the rows of u's slots summed in ascending order from +0: one thread per unknown
hipError_t launch_ties_fold(int dtype, const TieArgs &a, const void *g_slots, void *g_unique, hipStream_t stream);
// Hu = S H S^T per tree: one workgroup per tree, one thread per (u, v) entry
hipError_t launch_ties_fold_matrix(int dtype, const TieArgs &a, const void *H, void *Hu, hipStream_t stream);

} // namespace de
#endif
