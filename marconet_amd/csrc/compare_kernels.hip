// mnet_compare_stats — the precision margin guard's comparison (include/marconet_hip.h): one streaming pass over two tensors of the same logical shape
// [n_groups][elems_per_group], each in its own storage, one mnet_cmp_stats record per group.
//
// Values.  Both operands go through the storage's own reader (ldraw / unpackr of common.h): what this kernel compares is what every consumer of the tensor
// reads.  The difference is one fp32 subtraction of those values.
//
// Map.  A thread takes UNITS of 8 consecutive elements: one 16-byte chunk of an 8-wide storage, two of fp32.  The map thread -> unit is linear
// (unit = slice * 256 + trip * slices * 256 + thread), a group is a whole number of 32-element blocks, and every slice / trip starts on a multiple of 4 units:
// the 4 lanes of a quad always hold the 4 chunks of ONE block, which ldraw<hm> needs (its DPP moves hand the block's lo bytes and scale round the quad).
// Past the end of a group a thread keeps loading — from the group's LAST block, chunk (lane & 3) — and its contribution is masked: no lane of a quad leaves
// before the reader has run.
//
// Reduction.  thread (registers, in index order) -> wave (butterfly shuffles) -> workgroup (LDS, wave order) -> one partial record per (group, slice) in the
// caller's workspace; a second launch folds a group's slices in slice order.  No atomics, no arrival counters: every record is a fixed function of its own group's
// bytes — the same on every launch, whatever else is in the batch (the slice count depends on elems_per_group alone).
#include "common.h"

namespace {

constexpr int CMP_THREADS = 256;
constexpr int CMP_UNIT = 8;                                  // elements per thread and trip
static_assert(CMP_THREADS * CMP_UNIT == MNET_CMP_WG_ELEMS, "header macro and launch constants disagree");

// the 8 elements at nominal element index `e` (a multiple of 8) of `base`, as the storage's reader returns them
template <typename T> __device__ __forceinline__ void load_unit(const T* base, long long e, float* o) {
    if constexpr (sizeof(T) == 4 && !is_split4_type<T>) {   // fp32: two chunks of 4
        unpackr(ldraw(base + e), o);
        unpackr(ldraw(base + e + 4), o + 4);
    } else {
        unpackr(ldraw(base + e), o);
    }
}

struct Acc {
    float dmax, rmax, mmax;          // dmax starts at -1: "no finite pair yet" (a difference of 0 is attained by its first pair)
    long long idx;
    double ssd, ssr;
    long long nfm, nfr;
};

__device__ __forceinline__ void acc_init(Acc& a) { a.dmax = -1.f; a.rmax = 0.f; a.mmax = 0.f; a.idx = 0x7fffffffffffffffLL; a.ssd = 0.0; a.ssr = 0.0; a.nfm = 0; a.nfr = 0; }

// b folded into a, b's elements coming AFTER a's in the fixed order (maxima: ties keep the lower index; sums: a + b)
__device__ __forceinline__ void acc_fold(Acc& a, const Acc& b) {
    if (b.dmax > a.dmax || (b.dmax == a.dmax && b.idx < a.idx)) { a.dmax = b.dmax; a.idx = b.idx; }
    a.rmax = fmaxf(a.rmax, b.rmax); a.mmax = fmaxf(a.mmax, b.mmax);
    a.ssd += b.ssd; a.ssr += b.ssr; a.nfm += b.nfm; a.nfr += b.nfr;
}

__device__ __forceinline__ Acc acc_shfl_xor(const Acc& a, int o) {
    Acc b;
    b.dmax = __shfl_xor(a.dmax, o, 64); b.rmax = __shfl_xor(a.rmax, o, 64); b.mmax = __shfl_xor(a.mmax, o, 64);
    b.idx = __shfl_xor(a.idx, o, 64); b.ssd = __shfl_xor(a.ssd, o, 64); b.ssr = __shfl_xor(a.ssr, o, 64);
    b.nfm = __shfl_xor(a.nfm, o, 64); b.nfr = __shfl_xor(a.nfr, o, 64);
    return b;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }      // FLT_MAX: false for inf and NaN

__device__ __forceinline__ void acc_store(mnet_cmp_stats* r, const Acc& a, bool final_form) {
    const bool none = a.idx == 0x7fffffffffffffffLL;
    r->max_abs_diff = final_form && none ? 0.f : a.dmax;      // (a partial record keeps -1 / the sentinel index: the fold must see "no finite pair")
    r->max_abs_ref = a.rmax; r->max_abs_mode = a.mmax; r->reserved = 0;
    r->argmax_index = final_form && none ? -1 : a.idx;
    r->sum_sq_diff = a.ssd; r->sum_sq_ref = a.ssr; r->nonfinite_mode = a.nfm; r->nonfinite_ref = a.nfr;
}
__device__ __forceinline__ void acc_load(Acc& a, const mnet_cmp_stats* r) {
    a.dmax = r->max_abs_diff; a.rmax = r->max_abs_ref; a.mmax = r->max_abs_mode; a.idx = r->argmax_index;
    a.ssd = r->sum_sq_diff; a.ssr = r->sum_sq_ref; a.nfm = r->nonfinite_mode; a.nfr = r->nonfinite_ref;
}

// grid (n_groups, slices): workgroup (g, s) -> partial[g * slices + s]
template <typename TM, typename TR>
__global__ void __launch_bounds__(CMP_THREADS) compare_partial_kernel(const TM* __restrict__ mode, const TR* __restrict__ ref, long long elems,
                                                                      mnet_cmp_stats* __restrict__ partial) {
    const int g = blockIdx.x, s = blockIdx.y, slices = gridDim.y;
    const long long units = elems / CMP_UNIT;                                    // a multiple of 4
    const TM* mg = mode + (long long)g * elems;
    const TR* rg = ref + (long long)g * elems;
    const long long stride = (long long)slices * CMP_THREADS;
    const long long first = (long long)s * CMP_THREADS;
    const long long trips = first < units ? (units - first + stride - 1) / stride : 0;      // uniform over the workgroup
    Acc a;
    acc_init(a);
    for (long long t = 0; t < trips; ++t) {
        const long long u = first + t * stride + threadIdx.x;
        const bool live = u < units;
        const long long uc = live ? u : units - 4 + (threadIdx.x & 3);           // clamped: the group's last block, this lane's own chunk of it
        float m[CMP_UNIT], r[CMP_UNIT];
        load_unit(mg, uc * CMP_UNIT, m);
        load_unit(rg, uc * CMP_UNIT, r);
        if (live) {
#pragma unroll
            for (int j = 0; j < CMP_UNIT; ++j) {
                const bool fm = finite_f(m[j]), fr = finite_f(r[j]);
                a.nfm += fm ? 0 : 1; a.nfr += fr ? 0 : 1;
                if (fm && fr) {
                    const float d = fabsf(m[j] - r[j]);
                    if (d > a.dmax) { a.dmax = d; a.idx = u * CMP_UNIT + j; }     // (indices rise inside a thread: the first to attain the maximum is the lowest)
                    a.rmax = fmaxf(a.rmax, fabsf(r[j])); a.mmax = fmaxf(a.mmax, fabsf(m[j]));
                    a.ssd += (double)d * (double)d; a.ssr += (double)r[j] * (double)r[j];
                }
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const Acc b = acc_shfl_xor(a, o); acc_fold(a, b); }      // (a + b == b + a: every lane ends with the same bits)
    __shared__ mnet_cmp_stats wave_rec[CMP_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) acc_store(&wave_rec[wave], a, false);
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc w;
        for (int k = 1; k < CMP_THREADS / 64; ++k) { acc_load(w, &wave_rec[k]); acc_fold(a, w); }
        acc_store(&partial[(long long)g * slices + s], a, false);
    }
}

// one thread per group: its slices in slice order
__global__ void __launch_bounds__(64) compare_fold_kernel(const mnet_cmp_stats* __restrict__ partial, int n_groups, int slices, mnet_cmp_stats* __restrict__ stats) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n_groups) return;
    Acc a, b;
    acc_load(a, &partial[(long long)g * slices]);
    for (int s = 1; s < slices; ++s) { acc_load(b, &partial[(long long)g * slices + s]); acc_fold(a, b); }
    acc_store(&stats[g], a, true);
}

bool pair_ok(int m, int r) {
    if (r == MNET_F16X2) return m == MNET_F16 || m == MNET_F16M;
    if (r == MNET_F32) return is_storage(m);
    return false;
}
bool base_aligned(const void* p, int dt) { return is_split4(dt) ? aligned128(p) : aligned16(p); }

}  // namespace

extern "C" int mnet_compare_stats(const void* mode, int32_t mode_dtype, const void* ref, int32_t ref_dtype, int32_t n_groups, int64_t elems_per_group,
                                  mnet_cmp_stats* stats, void* workspace, void* stream) {
    MNET_CHECK_ARG(mode && ref && stats && workspace, "compare_stats: null pointer");
    MNET_CHECK_ARG(n_groups > 0 && elems_per_group > 0, "compare_stats: n_groups and elems_per_group must be positive");
    MNET_CHECK_ARG(pair_ok(mode_dtype, ref_dtype), "compare_stats: unsupported (mode, reference) storage pair (%d, %d)", (int)mode_dtype, (int)ref_dtype);
    MNET_CHECK_ARG(elems_per_group % 32 == 0, "compare_stats: elems_per_group must be a multiple of 32 (a group starts on a 32-channel block)");
    MNET_CHECK_ALIGN(base_aligned(mode, mode_dtype) && base_aligned(ref, ref_dtype),
                     "compare_stats: F32 / F16 tensors must be 16-byte aligned, split-half / fp16+8 tensors 128-byte aligned");
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(stats) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
                     "compare_stats: stats and workspace must be 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int slices = (int)MNET_CMP_SLICES(elems_per_group);
    mnet_cmp_stats* partial = reinterpret_cast<mnet_cmp_stats*>(workspace);
    const dim3 grid((unsigned)n_groups, (unsigned)slices);
#define CMP_LAUNCH(TM, TR) hipLaunchKernelGGL((compare_partial_kernel<TM, TR>), grid, dim3(CMP_THREADS), 0, st, (const TM*)mode, (const TR*)ref, \
                                              (long long)elems_per_group, partial)
    if (ref_dtype == MNET_F16X2) {
        if (mode_dtype == MNET_F16) CMP_LAUNCH(f16, hs); else CMP_LAUNCH(hm, hs);
    } else {
        dispatch_storage(mode_dtype, [&](auto tag) { using TM = typename decltype(tag)::type; CMP_LAUNCH(TM, float); });
    }
#undef CMP_LAUNCH
    MNET_LAUNCH_CHECK("compare_stats");
    hipLaunchKernelGGL(compare_fold_kernel, dim3((unsigned)((n_groups + 63) / 64)), dim3(64), 0, st, (const mnet_cmp_stats*)partial, (int)n_groups, slices, stats);
    MNET_LAUNCH_CHECK("compare_stats (fold)");
    return MNET_OK;
}
