// de_flat_real.hip — the Float32 / Float64 value policy of the flat-switch interpreter (de_flat.h): wide X (`direct`), the certificate
// pass and DE_EVAL_THREADED=0.  A lane owns one 16-byte vector (4 Float32 / 2 Float64 consecutive samples), a workgroup a tile of 1024 /
// 512 samples.  The X tile ([F, TILE], feature-fastest in HBM) is read once per workgroup with coalesced loads and transposed into LDS as
// rows of 256 vectors (+ one of padding), so a leaf read is one conflict-free ds_read_b128 per lane.  The operators are those of the
// threaded kernel's handlers (de_real_vec.h): the two kernels agree bit for bit.
#include "de_flat.h"
#include "de_loss_kinds.h"
#include "de_real_vec.h"

namespace de {

template <typename T> __device__ __noinline__ void real_store_ragged(T *o, VG<T, 1> v, int64_t remaining) {
    DE_UNROLL for (int i = 0; i < VecOf<T>::W; i++) if (i < remaining) o[i] = v.v[0][i];
}

// The lane's sum of a PARAMETERISED kind's terms (LOSS launches; de_loss_kinds.h): the threaded kernel's h_tree_end_loss on one vector.
// The kind is wave-uniform: a scalar switch, outside the loop over the samples.
template <typename T> __device__ __noinline__ T real_loss_kind_sum(int kind, T p, VG<T, 1> acc, VG<T, 1> y, VG<T, 1> w) {
    typename VecOf<T>::type l;
    DE_LOSS_KIND_SWITCH(kind, DE_UNROLL for (int i = 0; i < VecOf<T>::W; i++) l[i] = (loss_kind_one<KIND, T>(acc.v[0][i], y.v[0][i], p).l))
    T s = T(0);
    DE_UNROLL for (int i = 0; i < VecOf<T>::W; i++) s += w.v[0][i] != T(0) ? w.v[0][i] * l[i] : T(0);
    return s;
}

template <typename T> struct RealPolicy {
    typedef T Elem;
    typedef T Scalar;
    typedef typename VecOf<T>::type V;
    typedef V LY, LW;
    static constexpr bool LOSS_ALL_KINDS = true;
    static constexpr int VW = VecOf<T>::W, TILE = FLAT_BLK * VW, EPS = 1;
    static constexpr int ROWV = FLAT_BLK + 1; // LDS row stride in vectors (+1: bank spread for the staging writes)
    static constexpr size_t ROW_BYTES = FLAT_ROW_BYTES, STORE_BYTES = 16;
    static_assert(ROWV * 16 == FLAT_ROW_BYTES, "de_kernels.h FLAT_ROW_BYTES");
    static constexpr bool HAS_PARAMS = true;
    static constexpr const char *NAMES[5] = {"de_eval_tape_kernel", "de_eval_tape_kernel<direct>", "de_eval_tape_kernel<cert>",
                                             "de_eval_tape_kernel<loss>", "de_eval_tape_kernel<direct,loss>"};

    // coalesced HBM / L2 read, transposed LDS write: sample j of the tile lives at rows[f * ROWV * VW + j]
    static __device__ __forceinline__ void stage_x(const FlatArgs<T> &a, unsigned char *smem, int64_t base, int tid) {
        T *__restrict__ rows = reinterpret_cast<T *>(smem);
        const uint32_t F = (uint32_t)a.F;
        const uint32_t total = (uint32_t)TILE * F;
        if (a.ldX == (int64_t)F && base + TILE <= a.N) {
            const T *__restrict__ src = a.X + base * (int64_t)F; // contiguous TILE*F elements
            for (uint32_t e = tid; e < total; e += FLAT_BLK) {
                const uint32_t j = e / F, f = e - j * F;
                rows[f * (ROWV * VW) + j] = src[e];
            }
        } else { // ragged tail / strided X: clamp to the last real sample
            const int64_t last = a.N - 1;
            for (uint32_t e = tid; e < total; e += FLAT_BLK) {
                const uint32_t j = e / F, f = e - j * F;
                int64_t jj = base + j;
                jj = jj < last ? jj : last;
                rows[f * (ROWV * VW) + j] = a.X[f + a.ldX * jj];
            }
        }
    }
    static __device__ __forceinline__ V load_row(const unsigned char *smem, uint32_t r, int tid) { return reinterpret_cast<const V *>(smem)[r * ROWV + tid]; }
    static __device__ __forceinline__ void store_row(unsigned char *smem, uint32_t r, int tid, V v) { reinterpret_cast<V *>(smem)[r * ROWV + tid] = v; }
    // (re-read per use by design: the L1 / L2 absorb it)
    static __device__ __forceinline__ V gather(const FlatArgs<T> &a, uint32_t f, int64_t j0) {
        V v;
        DE_UNROLL for (int i = 0; i < VW; i++) {
            const int64_t jj = j0 + i < a.N - 1 ? j0 + i : a.N - 1;
            v[i] = a.X[f + a.ldX * jj];
        }
        return v;
    }
    static __device__ __forceinline__ V splat(T c) {
        V v;
        DE_UNROLL for (int i = 0; i < VW; i++) v[i] = c;
        return v;
    }
    static __device__ __forceinline__ V zero() { return splat(T(0)); }
    static __device__ __forceinline__ V constant(const FlatArgs<T> &, U32x4 w) { return splat(imm_of<T>(w.z, w.w)); }
    static __device__ __forceinline__ V param(const FlatArgs<T> &a, uint32_t idx, const int64_t (&cls)[VW]) {
        V v;
        DE_UNROLL for (int i = 0; i < VW; i++) v[i] = a.params[idx + a.ld_params * cls[i]];
        return v;
    }

    static __device__ __forceinline__ V add(V x, V y) { return x + y; }
    static __device__ __forceinline__ V sub(V x, V y) { return x - y; }
    static __device__ __forceinline__ V rsub(V x, V y) { return y - x; }
    static __device__ __forceinline__ V mul(V x, V y) { return x * y; }
    static __device__ __forceinline__ V div(V x, V y) { return x / y; }
    static __device__ __forceinline__ V rdiv(V x, V y) { return y / x; }
    template <bool SIN> static __device__ __forceinline__ V trig(V x) {
        V in[1] = {x}, out[1];
        vec_trig<T, 1, V, SIN>(out, in);
        return out[0];
    }
    static __device__ __forceinline__ V cos(V x) { return trig<false>(x); }
    static __device__ __forceinline__ V sin(V x) { return trig<true>(x); }
    static __device__ __forceinline__ V exp(V x) {
        V in[1] = {x}, out[1];
        vec_exp<T, 1, V>(out, in);
        return out[0];
    }
    static __device__ __forceinline__ V cold(uint32_t op, V x, V y) { return cold_op<T, 1>(op, VG<T, 1>{{x}}, VG<T, 1>{{y}}).v[0]; } // (a unary operator maps y = x)
    static __device__ __forceinline__ V cold_inj(uint32_t op, V x, V y) { // the operator of a fused deg1 kernel (BOP_INJ_*): cos / sin as BOP_UN computes them
        if constexpr (sizeof(T) == 4) {
            if (op == (uint32_t)DE_U_COS) return cos(y);
            if (op == (uint32_t)DE_U_SIN) return sin(y);
        }
        return cold(op, x, y);
    }
    static __device__ __forceinline__ V cold3(uint32_t op, V x, V y, V z) { return cold_op3<T, 1>(op, VG<T, 1>{{z}}, VG<T, 1>{{x}}, VG<T, 1>{{y}}).v[0]; }

    template <bool CERT> static __device__ __forceinline__ void test(T &poison, T &vmax, V v) {
        const V t[1] = {v};
        test_with<T, 1, V, CERT>(poison, vmax, t);
    }
    static __device__ __forceinline__ V inject(V x, V r) {
        DE_UNROLL for (int i = 0; i < VW; i++) r[i] = M<T>::isfinite(x[i]) ? r[i] : M<T>::inf();
        return r;
    }
    static __device__ __forceinline__ void store_vec(T *o, V v) { *reinterpret_cast<V *>(o) = v; } // one 16-byte store per lane, coalesced over the wave
    static __device__ __forceinline__ void store_ragged(T *o, V v, int64_t remaining) { real_store_ragged<T>(o, VG<T, 1>{{v}}, remaining); }

    // ---- LOSS: the threaded kernel's terms — e = yhat - y in T, L2 e * e, L1 |e|, kinds >= 16 through loss_kind_one
    static __device__ __forceinline__ V load_y(const FlatArgs<T> &a, int64_t j0, bool vec) {
        if (vec) return *reinterpret_cast<const V *>(a.y + j0);
        V v;
        DE_UNROLL for (int i = 0; i < VW; i++) v[i] = a.y[j0 + i < a.N - 1 ? j0 + i : a.N - 1];
        return v;
    }
    static __device__ __forceinline__ V load_w(const FlatArgs<T> &a, int64_t j0, bool vec) {
        if (!a.w) {
            V v;
            DE_UNROLL for (int i = 0; i < VW; i++) v[i] = j0 + i < a.N ? T(1) : T(0);
            return v;
        }
        if (vec) return *reinterpret_cast<const V *>(a.w + j0);
        V v;
        DE_UNROLL for (int i = 0; i < VW; i++) v[i] = j0 + i < a.N ? a.w[j0 + i < a.N - 1 ? j0 + i : a.N - 1] : T(0);
        return v;
    }
    static __device__ __forceinline__ T loss_sum(int kind, T p, V acc, V y, V w) {
        if (kind >= (int)DE_LOSS_HUBER) return real_loss_kind_sum<T>(kind, p, VG<T, 1>{{acc}}, VG<T, 1>{{y}}, VG<T, 1>{{w}});
        const V e = acc - y;
        T s = T(0);
        DE_UNROLL for (int i = 0; i < VW; i++) {
            const T l = kind == (int)DE_LOSS_L1 ? M<T>::abs(e[i]) : e[i] * e[i];
            s += w[i] != T(0) ? w[i] * l : T(0);
        }
        return s;
    }
};
static_assert(RealPolicy<float>::TILE == flat_tile_samples(DE_F32) && RealPolicy<double>::TILE == flat_tile_samples(DE_F64), "de_kernels.h flat_tile_samples");

hipError_t launch_eval_flat(int dtype, const EvalArgs &e, hipStream_t stream, const char **kname) {
    return dtype == DE_F32 ? launch_flat<RealPolicy<float>>(e, nullptr, stream, kname) : launch_flat<RealPolicy<double>>(e, nullptr, stream, kname);
}

} // namespace de
