// adh_debug_log.hip - test entries: the selection's table-driven log (adh_log_f32.h) evaluated on the device, on
// arguments a test supplies and over whole ranges of float32 bit patterns.
//
// Included by adh_api.hip, so the log is compiled with the product's flags (-ffp-contract=off among them) and is the
// code the two selection kernels inline.  Neither kernel here is on a hot path.
#pragma once
#include "adh_log_f32.h"

namespace dbglog {

constexpr int kBlock = 256;
constexpr uint32_t kFirst = 0x3F800000u;  // 1.0f
constexpr uint32_t kLast = 0x7F7FFFFFu;   // the largest finite float32

// The table the log reads: adh_log_tab itself, or its 256 doubles copied to LDS by the workgroup first, as the smoothing
// kernel of the ion-mobility selection does (adh_select_im.hip).
template <bool LDS>
__device__ __forceinline__ const double *table(double *lds) {
    if (!LDS) return &adh_log_tab[0][0];
    for (int t = threadIdx.x; t < 256; t += blockDim.x) lds[t] = adh_log_tab[t >> 1][t & 1];
    __syncthreads();
    return lds;
}

// out64: the float64 log where it is defined (1 <= x < inf), NaN elsewhere.  out32: what the two call sites store, by
// their own three-way dispatch (adh_select.hip `put`, adh_select_im.hip): 0 for x == 1, the rounded table log inside
// the domain, the library routine outside it.
template <bool LDS>
__global__ void __launch_bounds__(kBlock) eval_kernel(const float *__restrict__ x, int64_t n, double *__restrict__ out64,
                                                      float *__restrict__ out32) {
    __shared__ double lds[256];
    const double *tab = table<LDS>(lds);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float x1 = x[i];
        const bool inside = x1 >= 1.0f && x1 < INFINITY;
        float lg = 0.0f;
        if (x1 != 1.0f) lg = inside ? (float)adh_log_f32(x1, tab) : adh_log_f32_rare(x1);
        out32[i] = lg;
        out64[i] = inside ? adh_log_f32(x1, tab) : __longlong_as_double(0x7FF8000000000000ll);
    }
}

struct SweepBlock {  // one workgroup's largest difference
    double ulps;
    uint32_t bits;
    uint32_t pad;
};

// Every bit pattern first + k, k < count (count <= 2^32), against the device library's log: counts[0] += arguments whose
// float32-rounded logs differ, their patterns into list[0..capacity) in the order the slots are taken, and per
// workgroup the largest |table log - library log| in units of the library value's spacing (ties: the smaller argument).
template <bool LDS>
__global__ void __launch_bounds__(kBlock) sweep_kernel(uint32_t first, uint64_t count, unsigned long long *__restrict__ counts,
                                                       uint32_t *__restrict__ list, uint32_t capacity,
                                                       SweepBlock *__restrict__ per_block) {
    __shared__ double lds[256];
    __shared__ double s_ulps[kBlock];
    __shared__ uint32_t s_bits[kBlock];
    const double *tab = table<LDS>(lds);
    double worst = 0.0;
    uint32_t worst_bits = first;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t bits = first + (uint32_t)k;
        const float x = __uint_as_float(bits);
        const double mine = adh_log_f32(x, tab);
        const double ref = log((double)x);
        if ((float)mine != (float)ref) {
            const unsigned long long slot = atomicAdd(&counts[0], 1ull);
            if (slot < (unsigned long long)capacity) list[slot] = bits;
        }
        const double diff = fabs(mine - ref);
        if (diff > 0.0) {
            // spacing of ref: 2^(exponent - 52); ref is a log of x > 1 here, a normal number far above 2^-970
            const uint64_t rb = (uint64_t)__double_as_longlong(fabs(ref));
            const double ulp = __longlong_as_double((long long)(((rb >> 52) - 52ull) << 52));
            const double u = ref != 0.0 ? diff / ulp : INFINITY;
            if (u > worst) worst = u, worst_bits = bits;
        }
    }
    s_ulps[threadIdx.x] = worst;
    s_bits[threadIdx.x] = worst_bits;
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            const double o = s_ulps[threadIdx.x + half];
            const uint32_t ob = s_bits[threadIdx.x + half];
            if (o > s_ulps[threadIdx.x] || (o == s_ulps[threadIdx.x] && ob < s_bits[threadIdx.x]))
                s_ulps[threadIdx.x] = o, s_bits[threadIdx.x] = ob;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) per_block[blockIdx.x] = SweepBlock{s_ulps[0], s_bits[0], 0u};
}

}  // namespace dbglog

extern "C" {

int adh_debug_log_f32(adh_handle_t *h, const float *x, int64_t n, int32_t lds_table, double *out64, float *out32) {
    using namespace dbglog;
    if (!h || !x || !out64 || !out32) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_debug_log_f32: NULL argument");
    if (n < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_debug_log_f32: negative count");
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    sess::DevBufs B;
    float *d_x = nullptr, *d32 = nullptr;
    double *d64 = nullptr;
    HIP_TRY(B.upload(&d_x, x, (size_t)n, st));
    HIP_TRY(B.alloc(&d64, (size_t)n));
    HIP_TRY(B.alloc(&d32, (size_t)n));
    const dim3 grid(sess::grid_for(n)), block(kBlock);
    if (lds_table) hipLaunchKernelGGL(eval_kernel<true>, grid, block, 0, st, d_x, n, d64, d32);
    else hipLaunchKernelGGL(eval_kernel<false>, grid, block, 0, st, d_x, n, d64, d32);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out64, d64, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out32, d32, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ADH_OK;
}

int adh_debug_log_f32_sweep(adh_handle_t *h, uint32_t first_bits, uint32_t last_bits, int32_t lds_table,
                            int64_t *n_mismatch, uint32_t *mismatch_bits, int64_t capacity, double *max_ulps,
                            uint32_t *max_bits) {
    using namespace dbglog;
    if (!h || !n_mismatch || !max_ulps || !max_bits || (capacity > 0 && !mismatch_bits))
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_debug_log_f32_sweep: NULL argument");
    if (capacity < 0 || capacity > (int64_t)1 << 24)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_debug_log_f32_sweep: capacity outside [0, 2^24]");
    if (first_bits > last_bits) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_debug_log_f32_sweep: first_bits > last_bits");
    if (first_bits < kFirst || last_bits > kLast)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_debug_log_f32_sweep: the table log is defined for 1 <= x < inf only");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const uint64_t count = (uint64_t)last_bits - first_bits + 1;
    const unsigned blocks = (unsigned)std::min<uint64_t>((count + kBlock - 1) / kBlock, 4096);
    sess::DevBufs B;
    unsigned long long *d_count = nullptr;
    uint32_t *d_list = nullptr;
    SweepBlock *d_blocks = nullptr;
    HIP_TRY(B.alloc(&d_count, 1));
    HIP_TRY(B.alloc(&d_list, (size_t)capacity));
    HIP_TRY(B.alloc(&d_blocks, (size_t)blocks));
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
    const dim3 grid(blocks), block(kBlock);
    if (lds_table) hipLaunchKernelGGL(sweep_kernel<true>, grid, block, 0, st, first_bits, count, d_count, d_list, (uint32_t)capacity, d_blocks);
    else hipLaunchKernelGGL(sweep_kernel<false>, grid, block, 0, st, first_bits, count, d_count, d_list, (uint32_t)capacity, d_blocks);
    HIP_TRY(hipGetLastError());
    unsigned long long found = 0;
    std::vector<SweepBlock> per_block((size_t)blocks);
    HIP_TRY(hipMemcpyAsync(&found, d_count, sizeof(found), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(per_block.data(), d_blocks, (size_t)blocks * sizeof(SweepBlock), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the list in ascending order: the slots are taken in the order the workgroups happen to run
    const size_t listed = (size_t)std::min<unsigned long long>(found, (unsigned long long)capacity);
    if (listed > 0) {
        HIP_TRY(hipMemcpy(mismatch_bits, d_list, listed * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::sort(mismatch_bits, mismatch_bits + listed);
    }
    *n_mismatch = (int64_t)found;
    // the second pass of the maximum, over one entry per workgroup
    SweepBlock worst = per_block[0];
    for (const SweepBlock &b : per_block)
        if (b.ulps > worst.ulps || (b.ulps == worst.ulps && b.bits < worst.bits)) worst = b;
    *max_ulps = worst.ulps;
    *max_bits = worst.bits;
    return ADH_OK;
}

}  // extern "C"
