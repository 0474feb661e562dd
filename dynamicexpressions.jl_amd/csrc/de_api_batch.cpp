// de_api_batch.cpp — C ABI (include/de_hip.h): de_batch_sample_rows, de_batch_gather and the host-only de_batch_rows_host /
// de_batch_gather_host: the row sampler and the batch gather of minibatches.  The sampler's arithmetic is de_batch.h's,
// shared with the kernel; the kernels are de_batch.hip's.  Nothing here touches a program: the batch is a dense dataset like any other.
#include "de_api_internal.h"
#include "de_batch.h"

namespace {

// what both samplers refuse: DE_OK, or the status and (why != null) the reason
int sample_args_problem(int mode, int64_t N, int64_t offset, int64_t n_rows, const int64_t *rows, const char **why) {
    const char *w = nullptr;
    int rc = DE_ERR_INVALID_ARG;
    if (mode != DE_BATCH_REPLACE && mode != DE_BATCH_PERMUTE) w = "unknown mode (DE_BATCH_REPLACE or DE_BATCH_PERMUTE)";
    else if (N <= 0) w = "N must be positive";
    else if (n_rows < 0) w = "n_rows is negative";
    else if (offset < 0) w = "offset is negative";
    else if (n_rows > 0 && !rows) w = "rows is null";
    else if (offset > INT64_MAX - n_rows) w = "offset + n_rows overflows";
    else if (mode == DE_BATCH_PERMUTE && offset + n_rows > N) {
        w = "DE_BATCH_PERMUTE: offset + n_rows exceeds N (a permutation of [0, N) has N positions)";
        rc = DE_ERR_OUT_OF_RANGE;
    }
    if (why) *why = w;
    return w ? rc : DE_OK;
}

void rows_host(int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows) {
    const uint64_t k = batch_key(seed, step);
    const int h = batch_half_bits((uint64_t)N);
    for (int64_t j = 0; j < n_rows; j++)
        rows[j] = mode == DE_BATCH_PERMUTE ? batch_row_permute(k, (uint64_t)N, h, (uint64_t)(offset + j))
                                           : batch_row_replace(k, (uint64_t)N, (uint64_t)(offset + j));
}

// bytes of one word of a dtype's buffers (the real component type) and words per element
inline int word_bytes(int dtype) { return dtype == DE_F16 ? 2 : (dtype == DE_F32 || dtype == DE_CF32) ? 4 : 8; }
inline int word_parts(int dtype) { return is_complex_io(dtype) ? 2 : 1; }

// what both gathers refuse about their arguments, rows apart
const char *gather_args_problem(int dtype, const de_batch_src_t *s, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *d) {
    if (dtype < DE_F32 || dtype > DE_CF64) return "unknown dtype";
    if (n_rows < 0) return "n_rows is negative";
    if (!s || !d) return "src or dst is null";
    if (s->N <= 0) return "src.N must be positive";
    if (s->n_features < 0) return "src.n_features is negative";
    if (s->ldX < s->n_features || d->ldX < s->n_features) return "ldX is smaller than n_features";
    if (s->n_features > 0 && (!s->X || !d->X)) return "X is null";
    if ((d->y && !s->y) || (d->w && !s->w) || (d->classes && !s->classes)) return "a dst column (y, w or classes) without its src column";
    if (n_rows > 0 && !rows) return "rows is null";
    return nullptr;
}

// first position of `rows` outside [0, N), or -1
int64_t first_bad_row(const int64_t *rows, int64_t n_rows, int64_t N) {
    for (int64_t j = 0; j < n_rows; j++)
        if (rows[j] < 0 || rows[j] >= N) return j;
    return -1;
}

// THE host gather, for rows the caller pre-checked or not: a row outside [0, N) gets the kernel's fill (quiet NaN words, the class of source
// row 0) and is counted.  Returns the count.
template <typename W>
int32_t gather_host_words(int dtype, const de_batch_src_t *s, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *d) {
    const W nan = sizeof(W) == 2 ? (W)0x7E00u : sizeof(W) == 4 ? (W)0x7FC00000u : (W)0x7FF8000000000000ull;
    const int64_t parts = word_parts(dtype), xw = (int64_t)s->n_features * parts;
    const W *sX = static_cast<const W *>(s->X), *sy = static_cast<const W *>(s->y), *sw = static_cast<const W *>(s->w);
    W *dX = static_cast<W *>(d->X), *dy = s->y ? static_cast<W *>(d->y) : nullptr, *dw = s->w ? static_cast<W *>(d->w) : nullptr;
    int32_t n_bad = 0;
    for (int64_t j = 0; j < n_rows; j++) {
        const int64_t row = rows[j];
        const bool bad = row < 0 || row >= s->N;
        n_bad += bad ? 1 : 0;
        for (int64_t f = 0; f < xw; f++) dX[j * d->ldX * parts + f] = bad ? nan : sX[row * s->ldX * parts + f];
        if (dy)
            for (int64_t p = 0; p < parts; p++) dy[j * parts + p] = bad ? nan : sy[row * parts + p];
        if (dw) dw[j] = bad ? nan : sw[row];
        if (s->classes && d->classes) {
            const int64_t from = bad ? 0 : row;
            if (s->classes_is_i64) static_cast<int64_t *>(d->classes)[j] = static_cast<const int64_t *>(s->classes)[from];
            else static_cast<int32_t *>(d->classes)[j] = static_cast<const int32_t *>(s->classes)[from];
        }
    }
    return n_bad;
}

int32_t gather_host_any(int dtype, const de_batch_src_t *s, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *d) {
    const int wb = word_bytes(dtype);
    return wb == 2 ? gather_host_words<uint16_t>(dtype, s, rows, n_rows, d)
                   : wb == 4 ? gather_host_words<uint32_t>(dtype, s, rows, n_rows, d) : gather_host_words<uint64_t>(dtype, s, rows, n_rows, d);
}

} // namespace

extern "C" {

int de_batch_rows_host(int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows) {
    if (const int rc = sample_args_problem(mode, N, offset, n_rows, rows, nullptr)) return rc;
    rows_host(mode, N, seed, step, offset, n_rows, rows);
    return DE_OK;
}

int de_batch_sample_rows(de_ctx_t *c, int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows) {
    if (!c) return DE_ERR_INVALID_ARG;
    const char *why = nullptr;
    if (const int rc = sample_args_problem(mode, N, offset, n_rows, rows, &why)) return fail(c, rc, "de_batch_sample_rows: %s", why);
    if (n_rows == 0) return DE_OK;
    if (!is_device_ptr(rows)) { // a host buffer: the host function, no launch
        rows_host(mode, N, seed, step, offset, n_rows, rows);
        return DE_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // (not bracketed by the context's timing events: de_ctx_last_kernel_ms describes the last de_eval* call, and two event records cost
    // more device time than the kernel of a 10^3-row batch)
    HIP_TRY(c, launch_batch_sample(mode, N, seed, step, offset, n_rows, rows, c->stream));
    return DE_OK;
}

int de_batch_gather_host(int dtype, const de_batch_src_t *src, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *dst, int32_t *n_bad) {
    if (gather_args_problem(dtype, src, rows, n_rows, dst)) return DE_ERR_INVALID_ARG;
    if (first_bad_row(rows, n_rows, src->N) >= 0) return DE_ERR_OUT_OF_RANGE;
    if (n_bad) *n_bad = 0;
    if (n_rows > 0) (void)gather_host_any(dtype, src, rows, n_rows, dst);
    return DE_OK;
}

static int batch_gather_impl(de_ctx_t *c, int dtype, const de_batch_src_t *src, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *dst,
                             int32_t *n_bad) {
    if (const char *why = gather_args_problem(dtype, src, rows, n_rows, dst)) return fail(c, DE_ERR_INVALID_ARG, "de_batch_gather: %s", why);
    const bool bad_host = n_bad && !is_device_ptr(n_bad);
    if (n_rows == 0) {
        if (bad_host) *n_bad = 0;
        else if (n_bad) HIP_TRY(c, hipMemsetAsync(n_bad, 0, sizeof(int32_t), c->stream));
        return DE_OK;
    }
    // the data pointers: all on the device or all on the host
    const void *data[8] = {src->n_features > 0 ? src->X : nullptr, src->n_features > 0 ? dst->X : nullptr, src->y, dst->y, src->w, dst->w,
                           src->classes, dst->classes};
    int n_dev = 0, n_host = 0;
    for (const void *ptr : data)
        if (ptr) (is_device_ptr(ptr) ? n_dev : n_host)++;
    if (n_dev && n_host)
        return fail(c, DE_ERR_INVALID_ARG, "de_batch_gather: the data pointers (src and dst X, y, w, classes) must all be device or all be host pointers");
    const bool rows_host_side = !is_device_ptr(rows);
    if (rows_host_side) {
        const int64_t at = first_bad_row(rows, n_rows, src->N);
        if (at >= 0)
            return fail(c, DE_ERR_OUT_OF_RANGE, "de_batch_gather: rows[%lld] = %lld is outside [0, %lld)", (long long)at, (long long)rows[at],
                        (long long)src->N);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_host) { // host data: the host routine, with device rows copied over first (and then not pre-checked: it fills and counts)
        std::vector<int64_t> copy;
        if (!rows_host_side) {
            copy.resize((size_t)n_rows);
            HIP_TRY(c, hipMemcpyAsync(copy.data(), rows, (size_t)n_rows * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            rows = copy.data();
        }
        const int32_t nb = gather_host_any(dtype, src, rows, n_rows, dst);
        if (bad_host) *n_bad = nb;
        else if (n_bad) {
            HIP_TRY(c, hipMemcpyAsync(n_bad, &nb, sizeof nb, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream)); // (nb leaves scope)
        }
        return DE_OK;
    }
    // device data.  sBatch: [the counter of a host n_bad | a host `rows` staged]
    const size_t rows_at = 256, need = rows_at + (rows_host_side ? (size_t)n_rows * sizeof(int64_t) : 0);
    if ((bad_host || rows_host_side) && need > c->sBatch.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // (growing frees what queued work may still read)
        HIP_TRY(c, c->sBatch.reserve(need));
    }
    int32_t *d_bad = bad_host ? static_cast<int32_t *>(c->sBatch.p) : n_bad;
    if (rows_host_side) {
        int64_t *staged = reinterpret_cast<int64_t *>(static_cast<char *>(c->sBatch.p) + rows_at);
        HIP_TRY(c, hipMemcpyAsync(staged, rows, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        rows = staged;
    }
    if (d_bad) HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(int32_t), c->stream));
    const int parts = word_parts(dtype);
    BatchGatherArgs a{};
    a.rows = rows;
    a.n_bad = d_bad;
    a.N = src->N;
    a.n_rows = n_rows;
    a.xw = src->n_features * parts;
    a.yw = parts;
    a.cls_bytes = src->classes_is_i64 ? 8 : 4;
    a.s_ld = src->ldX * parts;
    a.d_ld = dst->ldX * parts;
    if (a.xw > 0) {
        a.sX = src->X;
        a.dX = dst->X;
        a.recip = ((uint64_t)1 << 32) / (uint64_t)a.xw + 1;
        a.step_q = 256 / a.xw;
        a.step_r = 256 % a.xw;
    }
    if (src->y && dst->y) a.sy = src->y, a.dy = dst->y;
    if (src->w && dst->w) a.sw = src->w, a.dw = dst->w;
    if (src->classes && dst->classes) a.scls = src->classes, a.dcls = dst->classes;
    // about 2048 words of X to a workgroup, at most 256 rows (one lane reads one row index)
    a.tile_rows = (int32_t)std::min<int64_t>(256, std::max<int64_t>(1, 2048 / std::max(a.xw, 1)));
    HIP_TRY(c, launch_batch_gather(word_bytes(dtype), a, c->stream)); // (no timing events, as the sampler)
    if (bad_host) HIP_TRY(c, hipMemcpyAsync(n_bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (bad_host || rows_host_side) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the staged rows are the caller's pageable memory)
    return DE_OK;
}

int de_batch_gather(de_ctx_t *c, int dtype, const de_batch_src_t *src, const int64_t *rows, int64_t n_rows, const de_batch_dst_t *dst,
                    int32_t *n_bad) {
    if (!c) return DE_ERR_INVALID_ARG;
    DE_NOTHROW(c, batch_gather_impl(c, dtype, src, rows, n_rows, dst, n_bad));
}

} // extern "C"
