// de_tree_params_dev.h — launchers of de_tree_params.hip: the device side of de_eval*_tree_params.
#ifndef DE_TREE_PARAMS_DEV_H
#define DE_TREE_PARAMS_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// Tree t owns the constant slots coff[t] .. coff[t + 1) of the program (n_consts in all) and, in dloss / dloss_c, the entries
// doff[t] .. doff[t] + (coff[t + 1] - coff[t]).  slot_tree[s] / slot_param[s]: the tree of slot s and the parameter row it stands for
// (-1: a real constant).  Element type `dtype` for base, params, cvec, *_c and the outputs; the accumulators are doubles.
struct TreeParamsArgs {
    int64_t n_trees, n_consts, n_classes, ld_params;
    int32_t n_params;
    int64_t cls; // the class the scatter / accumulate launch serves
    const int32_t *slot_tree, *slot_param;
    const int64_t *coff, *doff;
    const void *base, *params;
    void *cvec;
    const void *loss_c, *dloss_c; // one model call's results (null: the call has none — de_eval has neither, de_eval_loss_ex no dloss)
    const uint8_t *ok_c;
    double *acc_loss, *acc_dloss, *acc_dparams; // n_trees, n_consts, n_trees * n_classes * n_params
    uint8_t *acc_ok;                            // n_trees
    void *loss, *dloss, *dparams;               // the caller's (or their staged images); null: not wanted
    uint8_t *ok;
};
// cvec[s] = slot_param[s] < 0 ? base[s] : params[slot_param[s] + ld_params * (cls + n_classes * slot_tree[s])]
hipError_t launch_tree_params_scatter(int dtype, const TreeParamsArgs &a, hipStream_t stream);
// the accumulators take class cls: loss and every slot row added, the (p, cls) cells of dparams formed, the flags ANDed
hipError_t launch_tree_params_accumulate(int dtype, const TreeParamsArgs &a, hipStream_t stream);
// the accumulators rounded to the element type, NaN where the tree's flag is 0; ok = acc_ok
hipError_t launch_tree_params_finish(int dtype, const TreeParamsArgs &a, hipStream_t stream);

// de_fit_tree_params_bfgs: the packed vector of unknowns of every tree, n_unknowns entries in all, and where each
// lives (map: de_tree_params_fit.h).  `slots`: a vector in the program's slot layout; `cells`: parameter cells, columns ld apart.
struct TreeParamsFitArgs {
    int64_t n_unknowns, ld;
    int32_t n_params;
    const int64_t *map;
    void *packed;
    void *slots, *cells;
};
// packed[u] = slots / cells at map[u]: pack_x with (constants, parameter block), pack_g with (dloss, dparams; ld = n_params)
hipError_t launch_tree_params_pack(int dtype, const TreeParamsFitArgs &a, hipStream_t stream);
// slots / cells at map[u] = packed[u]; parameter slots and padding are not written
hipError_t launch_tree_params_unpack(int dtype, const TreeParamsFitArgs &a, hipStream_t stream);

} // namespace de
#endif
