// de_grad_encode.h — third stage of the GRADIENT program, on the host only: the bound program (de_bind.h) -> the direct-threaded stream of
// de_grad_threaded.hip (forward duals: buckets by gradient width) or of de_rev_threaded.hip (reverse accumulation: two sweeps per tree).
// No HIP call, no context, no environment switch: de_api_grad.cpp reads the switches, fetches the handler tables, calls an encoder and
// uploads what it returns; de_lower_tape_grad runs the same encoders against an identity handler table on any machine.
#pragma once
#include <stdint.h>

#include <functional>
#include <vector>

#include "de_bind.h"

namespace de {

// Direct threading: the handler word of a record names the handler of the record BEHIND it, the last record of the chain [a0, b0) — a
// tree, or one sweep of it — names the chain's first handler.
void successor_words(std::vector<BoundInstr> &code, int32_t a0, int32_t b0);
// Smallest address of a handler table; false when some handler lies 4 GiB or more above it (a record holds a 32-bit offset).
bool handler_base(const uint64_t *table, uint32_t n, uint64_t *base);

struct GradSource { // what both encoders read of a population: the bound UNFOLDED program and the gradient geometry of `mode`
    const std::vector<BoundInstr> &gbcode;
    const std::vector<int32_t> &gbcode_off; // n_trees + 1
    int64_t n_trees;
    int n_features, n_params;
    bool uses_params;
    int dtype, mode;   // DE_F32 | DE_F64, DE_GRAD_*
    const int32_t *ng; // per tree: gradient rows in `mode`
};
struct GradEncodeOptions {
    bool hot_const_unary = true; // unary operators outside the binder's hot set (and max / min) through hot handlers
    bool wide = false;           // forward: enough samples for two per lane ...
    int vs2_rows = 15;           // ... for trees of at most so many LDS rows per wave
    bool share = false;          // forward: shared leaf rows — the stream in four variants
    bool rfuse = true;           // reverse: fused pairs / triples
    void (*lap)(const char *) = nullptr; // DE_DEBUG_TIMING laps, or null
};
// 0, or why there is no stream: NO_PLAN before anything was encoded, NO_STREAM when a record has no threaded form.  A handler source may
// return a negative value of its own, which the encoder hands on.
enum { GRAD_ENC_OK = 0, GRAD_ENC_NO_PLAN = 1, GRAD_ENC_NO_STREAM = 2 };
struct GradHandlers { const uint64_t *table; uint64_t base; }; // gop_count(GC) / ROP_COUNT handler addresses, handler_base of them
// The table of module (GC, VS) of the source's dtype: GRAD_ENC_OK, GRAD_ENC_NO_PLAN (its handlers do not fit 32-bit offsets) or < 0.
using GradHandlerSource = std::function<int(int GC, int VS, GradHandlers *h)>;

constexpr int GRAD_BUCKETS_MAX = 20;
struct GradForwardStream {
    std::vector<BoundInstr> gtcode; // `share`: four variants, `stride` records apart
    std::vector<int32_t> gtcode_off, gtsite_of_gb, ids;
    bool share = false;
    int64_t stride = 0;
    struct Bucket { int32_t count, max_grad, slots, GC, VS, windows, start; uint64_t handler_base; uint32_t param_handler_off; }; // start: in `ids`
    int n_buckets = 0;
    Bucket buckets[GRAD_BUCKETS_MAX];
};
int encode_grad_forward(const GradSource &s, const GradEncodeOptions &opt, bool (*has_module)(int dtype, int GC, int VS),
                        const GradHandlerSource &handlers, GradForwardStream *r);

struct GradReverseStream {
    std::vector<BoundInstr> rtcode;
    std::vector<int32_t> rtcode_off, rtcode_mid, rtsite_of_gb, ids;
    std::vector<uint32_t> need; // per tree: partial + accumulation rows
    int64_t stage_cols = 0;
    struct Group { int32_t first, n, rows; }; // ids[first .. first + n), LDS rows per wave
    int n_groups = 0;
    Group groups[8];
};
int encode_grad_reverse(const GradSource &s, const GradEncodeOptions &opt, int n_slots, bool cse_generic, const GradHandlers &h,
                        GradReverseStream *r);
// DE_REV_STATS: dispatch classes and adjacent pairs of the two sweeps of a finished stream (what a fusion would save), on stderr
void reverse_stream_stats(const GradReverseStream &r, int64_t n_trees, const GradHandlers &h);

} // namespace de
