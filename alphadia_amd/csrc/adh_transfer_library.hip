// adh_transfer_library.hip - the transfer-learning library of the output stage (outputtransform/outputaccumulator.py):
// the top-k precursors per peptide across runs with their dense fragment rows, the retention-time normalisation and
// the MS2 quality control.
//
// adh_tl_scatter:  the flat fragment rows of one run go into zero-filled dense matrices (m/z, intensity, correlation)
//                  at (row, column); a bitmap of the cells (integer atomic OR) finds a cell written twice and sets a
//                  flag.  The matrices stay in HBM as the staged run of the next adh_tl_update.
// adh_tl_update:   the key columns of the new run are appended to the consensus' (mod_seq_hash, proba and
//                  precursor_idx as order-preserving uint64 keys: a signed hash with its sign bit flipped, proba as
//                  float64 with -0.0 -> +0.0 and every NaN the largest key).  Three stable LSD radix passes
//                  (precursor_idx, proba, hash) order the rows as pandas' stable multi-key sort does; segment heads,
//                  a running maximum of the head positions and `position - head < keep_top` give the keep mask, a
//                  flagged select the kept rows as indices into "consensus, then the new run".  The kept blocks of
//                  dense rows are ordered by their old start (one more stable pass), an exclusive scan of their
//                  lengths renumbers them, a binary search per new dense row finds its source row and one gather per
//                  matrix moves the rows; the source is the old consensus or the run, never a concatenation.
// adh_tl_qc:       the segmented masked median and the mask-multiply.  One wavefront (a workgroup of 64) per
//                  precursor compacts the correlations of the cells with intensity > 0 into its LDS slice and finds
//                  the middle order statistics by counting ranks (ties broken by the position in the slice); a second
//                  pass over the block multiplies every intensity by (correlation > median * ratio) - the product,
//                  not a select.  A block with more masked cells than the slice holds is listed and a workgroup of
//                  256 selects its order statistics digit by digit (4 bits a pass, counts in LDS) against global
//                  memory: any size.
// adh_tl_rt_norm:  two max reductions (NaN-skipping for pandas' max, NaN-propagating for np.max) and the elementwise
//                  formula, every operation in the reference's order and in the dtype NumPy's promotion gives it.
//
// All global writes are plain vector stores or vector integer atomics.  Included by adh_api.hip behind adh_session.h
// (shares its error helpers, the handle and the session helpers); adh_mbr_library.hip includes this file for the
// block-bookkeeping kernels of namespace tl.
#pragma once

struct adh_tl {
    adh_handle_t *h = nullptr;
    int32_t C = 0, M = 0;
    // the consensus: key columns and dense-row blocks of its precursors, the dense matrices
    int64_t n_prec = 0, n_rows = 0;
    sess::DevArray<uint64_t> hk, pk, ik;
    sess::DevArray<int64_t> start, stop;
    sess::DevArray<float> mat[ADH_TL_MAX_MATRICES];
    int hash_signed = -1;
    // the staged run of adh_tl_scatter
    sess::DevArray<float> staged[ADH_TL_MAX_MATRICES];
    int64_t staged_rows = -1;
    // the kept rows of the last update
    sess::DevArray<uint32_t> kept;
    int64_t n_kept = -1;
    sess::EventPair ev;
    double topk_ms = 0.0, gather_ms = 0.0, scatter_ms = 0.0;
};

namespace tl {

using sess::grid_for;
using sess::kBlock;
constexpr int kWave = 64;
constexpr int kQcSlice = ADH_TL_QC_SLICE;  // floats of LDS per wavefront

// ---- the dense scatter ------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) scatter_kernel(const int64_t *__restrict__ row, const int32_t *__restrict__ col,
                                                         const float *__restrict__ mz, const float *__restrict__ inten,
                                                         const float *__restrict__ corr, int64_t n, int32_t C,
                                                         float *__restrict__ m_mz, float *__restrict__ m_in,
                                                         float *__restrict__ m_co, uint32_t *__restrict__ occupied,
                                                         int32_t *__restrict__ duplicate) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t cell = row[i] * C + col[i];
        const uint32_t bit = 1u << (uint32_t)(cell & 31);
        if (atomicOr(&occupied[cell >> 5], bit) & bit) {
            *duplicate = 1;
        } else {
            m_mz[cell] = mz[i];
            m_in[cell] = inten[i];
            m_co[cell] = corr[i];
        }
    }
}

// ---- top-k per peptide ------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t proba_key(double p) {
    if (p != p) return 0xFFFFFFFFFFFFFFFFull;  // NaN sorts last
    if (p == 0.0) p = 0.0;                     // -0.0 and +0.0 tie
    const uint64_t u = (uint64_t)__double_as_longlong(p);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(kBlock) key_kernel(const uint64_t *__restrict__ hash, int32_t hash_signed,
                                                     const void *__restrict__ proba, int32_t proba_is_f64,
                                                     const int64_t *__restrict__ pidx, const int64_t *__restrict__ start,
                                                     const int64_t *__restrict__ stop, int64_t n, int64_t row0,
                                                     uint64_t *__restrict__ hk, uint64_t *__restrict__ pk,
                                                     uint64_t *__restrict__ ik, int64_t *__restrict__ o_start,
                                                     int64_t *__restrict__ o_stop) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        hk[i] = hash_signed ? (hash[i] ^ 0x8000000000000000ull) : hash[i];
        pk[i] = proba_key(proba_is_f64 ? ((const double *)proba)[i] : (double)((const float *)proba)[i]);
        ik[i] = (uint64_t)pidx[i] ^ 0x8000000000000000ull;
        o_start[i] = start[i] + row0;
        o_stop[i] = stop[i] + row0;
    }
}

__global__ void __launch_bounds__(kBlock) take_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ perm,
                                                      int64_t n, uint64_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = key[perm[i]];
}

// the position of a segment's first row at the head, 0 elsewhere: its running maximum is every row's segment start
__global__ void __launch_bounds__(kBlock) head_kernel(const uint64_t *__restrict__ key, int64_t n, uint32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
        head[k] = (k > 0 && key[k] != key[k - 1]) ? (uint32_t)k : 0u;
}

__global__ void __launch_bounds__(kBlock) keep_kernel(const uint32_t *__restrict__ seg_start, int64_t n, uint32_t keep_top,
                                                      uint8_t *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
        flag[k] = ((uint32_t)k - seg_start[k]) < keep_top ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) kept_start_kernel(const uint32_t *__restrict__ kept, const int64_t *__restrict__ start,
                                                            int64_t K, uint32_t *__restrict__ key, uint32_t *__restrict__ pos) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride) {
        key[j] = (uint32_t)start[kept[j]];
        pos[j] = (uint32_t)j;
    }
}

__global__ void __launch_bounds__(kBlock) block_len_kernel(const uint32_t *__restrict__ kept, const uint32_t *__restrict__ ord,
                                                           const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                           int64_t K, int64_t *__restrict__ len) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += stride) {
        const uint32_t src = kept[ord[i]];
        len[i] = stop[src] - start[src];
    }
}

// i: the kept blocks by ascending old start; j = ord[i]: the kept rows in their sorted order
__global__ void __launch_bounds__(kBlock) renumber_kernel(const uint32_t *__restrict__ kept, const uint32_t *__restrict__ ord,
                                                          const int64_t *__restrict__ new_start, const int64_t *__restrict__ len,
                                                          const uint64_t *__restrict__ hk, const uint64_t *__restrict__ pk,
                                                          const uint64_t *__restrict__ ik, int64_t K, uint64_t *__restrict__ o_hk,
                                                          uint64_t *__restrict__ o_pk, uint64_t *__restrict__ o_ik,
                                                          int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += stride) {
        const uint32_t j = ord[i], src = kept[j];
        o_hk[j] = hk[src];
        o_pk[j] = pk[src];
        o_ik[j] = ik[src];
        o_start[j] = new_start[i];
        o_stop[j] = new_start[i] + len[i];
    }
}

// the source row of every new dense row: the last block whose new start is <= r holds it
__global__ void __launch_bounds__(kBlock) row_map_kernel(const int64_t *__restrict__ new_start, const uint32_t *__restrict__ old_start,
                                                         int64_t K, int64_t R, uint32_t *__restrict__ src_row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += stride) {
        int64_t lo = 0, hi = K;  // first block with new_start > r
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (new_start[mid] <= r) lo = mid + 1;
            else hi = mid;
        }
        const int64_t b = lo - 1;
        src_row[r] = old_start[b] + (uint32_t)(r - new_start[b]);
    }
}

__global__ void __launch_bounds__(kBlock) row_gather_kernel(const float *__restrict__ cons, const float *__restrict__ run,
                                                            const uint32_t *__restrict__ src_row, int64_t rows0, int64_t cells,
                                                            int32_t C, float *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += stride) {
        const int64_t r = e / C, c = e - r * C;
        const int64_t s = src_row[r];
        out[e] = s < rows0 ? cons[s * C + c] : run[(s - rows0) * C + c];
    }
}

// ---- MS2 quality control ----------------------------------------------------------------------------------------

__device__ __forceinline__ float quiet_nan_f32() { return __uint_as_float(0x7FC00000u); }

// one wavefront (the whole workgroup) per precursor
__global__ void __launch_bounds__(kWave) qc_wave_kernel(float *__restrict__ inten, const float *__restrict__ corr,
                                                        const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                        int64_t n_prec, int32_t C, float cutoff, float ratio, int32_t empty_passes,
                                                        uint8_t *__restrict__ use, uint32_t *__restrict__ list,
                                                        uint32_t *__restrict__ n_large) {
    __shared__ float v[kQcSlice];
    __shared__ float s_mid[2];
    const uint32_t lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < n_prec; p += gridDim.x) {
        const int64_t off = start[p] * C;
        const uint32_t n_cell = (uint32_t)((stop[p] - start[p]) * C);
        uint32_t n = 0;
        bool nan = false;
        for (uint32_t base = 0; base < n_cell; base += kWave) {
            const uint32_t j = base + lane;
            const bool m = j < n_cell && inten[off + j] > 0.0f;
            const float c = m ? corr[off + j] : 0.0f;
            const uint64_t mask = __ballot(m);
            const uint32_t pos = n + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (m && pos < (uint32_t)kQcSlice) v[pos] = c;
            nan = nan || (m && c != c);
            n += (uint32_t)__popcll(mask);
        }
        if (n > (uint32_t)kQcSlice) {  // (uniform over the wavefront)
            if (lane == 0) list[atomicAdd(n_large, 1u)] = (uint32_t)p;
            continue;
        }
        nan = __any(nan);
        __syncthreads();
        float med = 0.0f;
        if (n > 0 && nan) {
            med = quiet_nan_f32();
        } else if (n > 0) {
            const uint32_t k1 = (n - 1) / 2, k2 = n / 2;
            for (uint32_t i = lane; i < n; i += kWave) {
                const float vi = v[i];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < n; ++j) {
                    const float vj = v[j];
                    rank += (vj < vi || (vj == vi && j < i)) ? 1u : 0u;
                }
                if (rank == k1) s_mid[0] = vi;
                if (rank == k2) s_mid[1] = vi;
            }
            __syncthreads();
            med = (n & 1u) ? s_mid[0] : (s_mid[0] + s_mid[1]) / 2.0f;
        }
        const float thr = med * ratio;
        if (lane == 0) use[p] = n == 0 ? (uint8_t)(empty_passes != 0) : (uint8_t)(med > cutoff);
        for (uint32_t j = lane; j < n_cell; j += kWave) {
            const float x = inten[off + j];
            inten[off + j] = x * (corr[off + j] > thr ? 1.0f : 0.0f);
        }
        __syncthreads();  // the slice is free for the next precursor
    }
}

__device__ __forceinline__ uint32_t f32_key(float c) {
    const uint32_t u = __float_as_uint(c);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float f32_from_key(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k);
}

// the k-th smallest masked correlation of the block (k from 0), found from the top digit down; all threads call it
__device__ float qc_select(const float *__restrict__ inten, const float *__restrict__ corr, int64_t off, uint32_t n_cell,
                           uint32_t k, uint32_t *hist) {
    uint32_t prefix = 0;
    for (int shift = 28; shift >= 0; shift -= 4) {
        if (threadIdx.x < 16) hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < n_cell; j += kBlock) {
            if (!(inten[off + j] > 0.0f)) continue;
            const uint32_t key = f32_key(corr[off + j]);
            if (((uint64_t)key >> (shift + 4)) == ((uint64_t)prefix >> (shift + 4))) atomicAdd(&hist[(key >> shift) & 15u], 1u);
        }
        __syncthreads();
        uint32_t d = 0;
        for (; d < 15; ++d) {
            const uint32_t c = hist[d];
            if (k < c) break;
            k -= c;
        }
        prefix |= d << shift;
        __syncthreads();  // every thread has read the counts
    }
    return f32_from_key(prefix);
}

// a block whose masked cells do not fit the slice: a workgroup per block
__global__ void __launch_bounds__(kBlock) qc_large_kernel(float *__restrict__ inten, const float *__restrict__ corr,
                                                          const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                          int32_t C, float cutoff, float ratio, uint8_t *__restrict__ use,
                                                          const uint32_t *__restrict__ list) {
    __shared__ uint32_t hist[16];
    __shared__ uint32_t s_n, s_nan;
    const uint32_t p = list[blockIdx.x];
    const int64_t off = start[p] * C;
    const uint32_t n_cell = (uint32_t)((stop[p] - start[p]) * C);
    if (threadIdx.x == 0) s_n = 0, s_nan = 0;
    __syncthreads();
    uint32_t mine = 0, nan = 0;
    for (uint32_t j = threadIdx.x; j < n_cell; j += kBlock) {
        if (!(inten[off + j] > 0.0f)) continue;
        const float c = corr[off + j];
        ++mine;
        nan |= (c != c) ? 1u : 0u;
    }
    atomicAdd(&s_n, mine);
    if (nan) atomicOr(&s_nan, 1u);
    __syncthreads();
    const uint32_t n = s_n;  // (above the slice: never 0)
    float med;
    if (s_nan) {
        med = quiet_nan_f32();
    } else {
        const float a = qc_select(inten, corr, off, n_cell, (n - 1) / 2, hist);
        med = (n & 1u) ? a : (a + qc_select(inten, corr, off, n_cell, n / 2, hist)) / 2.0f;
    }
    const float thr = med * ratio;
    if (threadIdx.x == 0) use[p] = (uint8_t)(med > cutoff);
    for (uint32_t j = threadIdx.x; j < n_cell; j += kBlock) {
        const float x = inten[off + j];
        inten[off + j] = x * (corr[off + j] > thr ? 1.0f : 0.0f);
    }
}

// ---- retention-time normalisation -------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ T quiet_nan();
template <>
__device__ __forceinline__ float quiet_nan<float>() {
    return __uint_as_float(0x7FC00000u);
}
template <>
__device__ __forceinline__ double quiet_nan<double>() {
    return __longlong_as_double(0x7FF8000000000000ll);
}

// SKIP: pandas' max (NaN is "no value"; all NaN gives NaN).  Otherwise np.max: any NaN gives NaN.
template <typename T, bool SKIP>
__device__ __forceinline__ T max_combine(T a, T b) {
    if (a != a) return SKIP ? b : quiet_nan<T>();
    if (b != b) return SKIP ? a : quiet_nan<T>();
    return a > b ? a : b;
}

// out[block] = the maximum of the block's share of x; launched again with one workgroup over the partial maxima
template <typename T, bool SKIP>
__global__ void __launch_bounds__(kBlock) max_kernel(const T *__restrict__ x, int64_t n, T *__restrict__ out) {
    __shared__ T s[kBlock];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // np.max of nothing does not occur (n >= 1); a thread without an element holds what SKIP skips, or x[0]
    T m = SKIP ? quiet_nan<T>() : x[0];
    for (; i < n; i += stride) m = max_combine<T, SKIP>(m, x[i]);
    s[threadIdx.x] = m;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] = max_combine<T, SKIP>(s[threadIdx.x], s[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

template <typename T>
__global__ void __launch_bounds__(kBlock) rt_max_norm_kernel(const T *__restrict__ obs, const T *__restrict__ mx, int64_t n,
                                                             T *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const T m = *mx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = obs[i] / m;
}

// calibrated_norm before its own normalisation: rt_library * (1 + (rt_observed - rt_calibrated) / rt_calibrated)
template <typename TO, typename TC, typename TL, typename TN>
__global__ void __launch_bounds__(kBlock) rt_calibrated_kernel(const TO *__restrict__ obs, const TC *__restrict__ cal,
                                                               const TL *__restrict__ lib, int64_t n, TN *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const auto deviation = (obs[i] - cal[i]) / cal[i];
        const auto one_plus = (decltype(deviation))1 + deviation;
        out[i] = lib[i] * one_plus;
    }
}

// (1 - max_norm) * calibrated_norm + max_norm * max_norm
template <typename TO, typename TN>
__global__ void __launch_bounds__(kBlock) rt_delta_kernel(const TO *__restrict__ obs, const TO *__restrict__ obs_max,
                                                          const TN *__restrict__ cn, const TN *__restrict__ cn_max, int64_t n,
                                                          TN *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const TO om = *obs_max;
    const TN cm = *cn_max;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const TO max_norm = obs[i] / om;
        const TN calibrated = cn[i] / cm;
        const TN left = ((TO)1 - max_norm) * calibrated;
        const TO right = max_norm * max_norm;
        out[i] = left + right;
    }
}

template <typename T, bool SKIP>
int reduce_max(sess::DevBufs &B, const T *x, int64_t n, T **out, hipStream_t st) {
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 1024));
    T *part = nullptr;
    HIP_TRY(B.alloc(&part, (size_t)blocks));
    HIP_TRY(B.alloc(out, 4));
    hipLaunchKernelGGL((max_kernel<T, SKIP>), dim3(blocks), dim3(kBlock), 0, st, x, n, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((max_kernel<T, SKIP>), dim3(1), dim3(kBlock), 0, st, (const T *)part, (int64_t)blocks, *out);
    HIP_TRY(hipGetLastError());
    return ADH_OK;
}

template <typename TO, typename TC, typename TL>
int rt_delta_max(sess::DevBufs &B, const void *d_obs, const void *d_cal, const void *d_lib, int64_t n, void *d_out, hipStream_t st) {
    using TN = decltype(TL() * (TO() - TC()));
    const TO *obs = (const TO *)d_obs;
    TN *cn = nullptr;
    TO *obs_max = nullptr;
    TN *cn_max = nullptr;
    HIP_TRY(B.alloc(&cn, (size_t)n));
    ADH_TRY((reduce_max<TO, false>(B, obs, n, &obs_max, st)));
    hipLaunchKernelGGL((rt_calibrated_kernel<TO, TC, TL, TN>), dim3(grid_for(n)), dim3(kBlock), 0, st, obs, (const TC *)d_cal,
                       (const TL *)d_lib, n, cn);
    HIP_TRY(hipGetLastError());
    ADH_TRY((reduce_max<TN, false>(B, cn, n, &cn_max, st)));
    hipLaunchKernelGGL((rt_delta_kernel<TO, TN>), dim3(grid_for(n)), dim3(kBlock), 0, st, obs, (const TO *)obs_max,
                       (const TN *)cn, (const TN *)cn_max, n, (TN *)d_out);
    HIP_TRY(hipGetLastError());
    return ADH_OK;
}

void release_staged(adh_tl *g) {
    for (int m = 0; m < ADH_TL_MAX_MATRICES; ++m) g->staged[m].release();
    g->staged_rows = -1;
}

}  // namespace tl

extern "C" {

int adh_tl_create(adh_handle_t *h, int32_t n_columns, int32_t n_matrices, adh_tl_t **out) {
    if (!h || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_columns < 1 || n_columns > 4096) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_create: 1 to 4096 fragment columns");
    if (n_matrices < 1 || n_matrices > ADH_TL_MAX_MATRICES)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_create: 1 to " + std::to_string(ADH_TL_MAX_MATRICES) + " dense matrices");
    adh_tl *g = new adh_tl();
    g->h = h;
    g->C = n_columns;
    g->M = n_matrices;
    *out = g;
    return ADH_OK;
}

int adh_tl_destroy(adh_tl_t *g) {
    if (!g) return ADH_OK;
    (void)hipSetDevice(g->h->device);
    (void)hipStreamSynchronize(g->h->stream);
    delete g;  // (the members free their device memory and events)
    return ADH_OK;
}

int adh_tl_scatter(adh_tl_t *g, int64_t n_rows, int64_t n_flat, const int64_t *row, const int32_t *col, const float *mz,
                   const float *intensity, const float *correlation, int32_t *duplicate) {
    if (!g || !duplicate || (n_flat > 0 && (!row || !col || !mz || !intensity || !correlation)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->M != 3) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_scatter: the library holds m/z, intensity and correlation");
    if (n_rows < 0 || n_flat < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_scatter: negative size");
    if (n_rows >= (int64_t)0x7FFFFFF0ll || n_flat >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_tl_scatter: 2^31 rows and more are not supported");
    for (int64_t i = 0; i < n_flat; ++i)
        if (row[i] < 0 || row[i] >= n_rows || col[i] < 0 || col[i] >= g->C)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_scatter: flat row " + std::to_string(i) + " lies outside the matrices");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    tl::release_staged(g);
    const size_t cells = (size_t)n_rows * (size_t)g->C;
    sess::DevBufs B;
    int64_t *d_row = nullptr;
    int32_t *d_col = nullptr, *d_dup = nullptr;
    float *d_mz = nullptr, *d_in = nullptr, *d_co = nullptr;
    uint32_t *occ = nullptr;
    HIP_TRY(B.upload(&d_row, row, (size_t)n_flat, st));
    HIP_TRY(B.upload(&d_col, col, (size_t)n_flat, st));
    HIP_TRY(B.upload(&d_mz, mz, (size_t)n_flat, st));
    HIP_TRY(B.upload(&d_in, intensity, (size_t)n_flat, st));
    HIP_TRY(B.upload(&d_co, correlation, (size_t)n_flat, st));
    HIP_TRY(B.alloc(&d_dup, 4));
    HIP_TRY(B.alloc(&occ, cells / 32 + 1));
    float *m[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) HIP_TRY(B.alloc(&m[k], cells));
    sess::EventPair &t = g->ev;
    g->scatter_ms = 0.0;
    ADH_TRY(t.begin(st));
    HIP_TRY(hipMemsetAsync(d_dup, 0, 4, st));
    HIP_TRY(hipMemsetAsync(occ, 0, (cells / 32 + 1) * 4, st));
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemsetAsync(m[k], 0, std::max<size_t>(cells, 4) * 4, st));
    if (n_flat > 0) {
        hipLaunchKernelGGL(tl::scatter_kernel, dim3(tl::grid_for(n_flat)), dim3(tl::kBlock), 0, st, d_row, d_col, d_mz, d_in, d_co,
                           n_flat, g->C, m[0], m[1], m[2], occ, d_dup);
        HIP_TRY(hipGetLastError());
    }
    ADH_TRY(t.end(st, g->scatter_ms));
    HIP_TRY(hipMemcpyAsync(duplicate, d_dup, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += 4;
    if (*duplicate) return ADH_OK;  // nothing is staged
    for (int k = 0; k < 3; ++k) g->staged[k].adopt(B, m[k], cells);
    g->staged_rows = n_rows;
    return ADH_OK;
}

int adh_tl_update(adh_tl_t *g, int32_t keep_top, int64_t n_new, const void *hash, int32_t hash_is_signed, const void *proba,
                  int32_t proba_is_f64, const int64_t *precursor_idx, const int64_t *frag_start, const int64_t *frag_stop,
                  int64_t n_new_rows, const float *const *matrices, int64_t *n_kept, int64_t *n_kept_rows) {
    if (!g || !n_kept || !n_kept_rows || (n_new > 0 && (!hash || !proba || !precursor_idx || !frag_start || !frag_stop)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (keep_top < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_update: keep_top must be at least 1");
    if (n_new < 0 || n_new_rows < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_update: negative size");
    const int64_t n0 = g->n_prec, n = n0 + n_new, R0 = g->n_rows, R = R0 + n_new_rows;
    if (n < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_update: no precursors");
    if (n >= (int64_t)0x7FFFFFF0ll || R >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_tl_update: 2^31 rows and more are not supported");
    if (g->hash_signed >= 0 && n_new > 0 && g->hash_signed != (hash_is_signed ? 1 : 0))
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_update: mod_seq_hash changed its dtype between runs");
    for (int64_t i = 0; i < n_new; ++i)
        if (frag_start[i] < 0 || frag_stop[i] < frag_start[i] || frag_stop[i] > n_new_rows)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_update: the fragment rows of precursor " + std::to_string(i) +
                                                      " lie outside the run's matrices");
    if (!matrices && g->staged_rows != n_new_rows)
        return fail(ADH_ERR_NOT_STAGED, "adh_tl_update: no staged run of " + std::to_string(n_new_rows) + " dense rows");
    if (matrices)
        for (int m = 0; m < g->M; ++m)
            if (!matrices[m] && n_new_rows > 0) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL matrix");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t C = g->C;
    sess::DevBufs B;

    // the run's matrices
    const float *run[ADH_TL_MAX_MATRICES] = {nullptr, nullptr, nullptr, nullptr};
    if (matrices) {
        for (int m = 0; m < g->M; ++m) {
            float *d = nullptr;
            HIP_TRY(B.upload(&d, matrices[m], (size_t)n_new_rows * C, st));
            run[m] = d;
        }
    } else {
        for (int m = 0; m < g->M; ++m) run[m] = g->staged[m].p;
    }

    // consensus, then the new run
    uint64_t *hk = nullptr, *pk = nullptr, *ik = nullptr, *raw_hash = nullptr, *k_in = nullptr, *k_out = nullptr;
    int64_t *start = nullptr, *stop = nullptr, *raw_idx = nullptr, *raw_start = nullptr, *raw_stop = nullptr;
    unsigned char *raw_proba = nullptr;
    uint32_t *perm_a = nullptr, *perm_b = nullptr, *head = nullptr, *seg_start = nullptr, *kept = nullptr, *n_sel = nullptr;
    uint8_t *flag = nullptr;
    HIP_TRY(B.alloc(&hk, (size_t)n));
    HIP_TRY(B.alloc(&pk, (size_t)n));
    HIP_TRY(B.alloc(&ik, (size_t)n));
    HIP_TRY(B.alloc(&start, (size_t)n));
    HIP_TRY(B.alloc(&stop, (size_t)n));
    HIP_TRY(B.alloc(&k_in, (size_t)n));
    HIP_TRY(B.alloc(&k_out, (size_t)n));
    HIP_TRY(B.alloc(&perm_a, (size_t)n));
    HIP_TRY(B.alloc(&perm_b, (size_t)n));
    HIP_TRY(B.alloc(&head, (size_t)n));
    HIP_TRY(B.alloc(&seg_start, (size_t)n));
    HIP_TRY(B.alloc(&flag, (size_t)n));
    HIP_TRY(B.alloc(&kept, (size_t)n));
    HIP_TRY(B.alloc(&n_sel, 4));
    if (n0 > 0) {
        HIP_TRY(hipMemcpyAsync(hk, g->hk, (size_t)n0 * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(pk, g->pk, (size_t)n0 * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(ik, g->ik, (size_t)n0 * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(start, g->start, (size_t)n0 * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(stop, g->stop, (size_t)n0 * 8, hipMemcpyDeviceToDevice, st));
    }
    if (n_new > 0) {
        const size_t pb = proba_is_f64 ? 8 : 4;
        HIP_TRY(B.upload(&raw_hash, (const uint64_t *)hash, (size_t)n_new, st));
        HIP_TRY(B.upload(&raw_idx, precursor_idx, (size_t)n_new, st));
        HIP_TRY(B.upload(&raw_start, frag_start, (size_t)n_new, st));
        HIP_TRY(B.upload(&raw_stop, frag_stop, (size_t)n_new, st));
        HIP_TRY(B.upload(&raw_proba, proba, (size_t)n_new * pb, st));
    }

    sess::EventPair &t = g->ev;
    g->topk_ms = g->gather_ms = 0.0;
    ADH_TRY(t.begin(st));
    if (n_new > 0) {
        hipLaunchKernelGGL(tl::key_kernel, dim3(tl::grid_for(n_new)), dim3(tl::kBlock), 0, st, raw_hash, hash_is_signed ? 1 : 0,
                           (const void *)raw_proba, proba_is_f64, raw_idx, raw_start, raw_stop, n_new, R0, hk + n0, pk + n0,
                           ik + n0, start + n0, stop + n0);
        HIP_TRY(hipGetLastError());
    }
    // least significant key first: precursor_idx, proba, mod_seq_hash
    hipLaunchKernelGGL(sess::iota_kernel, dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st, perm_a, n);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, ik, k_out, perm_a, perm_b, n, 64, st));
    hipLaunchKernelGGL(tl::take_kernel, dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st, pk, perm_b, n, k_in);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, k_in, k_out, perm_b, perm_a, n, 64, st));
    hipLaunchKernelGGL(tl::take_kernel, dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st, hk, perm_a, n, k_in);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, k_in, k_out, perm_a, perm_b, n, 64, st));
    // heads, rank inside the peptide, keep mask, the kept rows
    hipLaunchKernelGGL(tl::head_kernel, dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st, k_out, n, head);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::cub_call(B, [&](void *tmp, size_t &bytes) {
        return hipcub::DeviceScan::InclusiveScan(tmp, bytes, head, seg_start, hipcub::Max(), (int)n, st);
    }));
    hipLaunchKernelGGL(tl::keep_kernel, dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st, seg_start, n, (uint32_t)keep_top, flag);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::select_flagged(B, perm_b, flag, kept, n_sel, n, st));
    uint32_t K32 = 0;
    HIP_TRY(hipMemcpyAsync(&K32, n_sel, 4, hipMemcpyDeviceToHost, st));
    ADH_TRY(t.end(st, g->topk_ms));
    const int64_t K = K32;
    if (K < 1 || K > n) return fail(ADH_ERR_HIP, "adh_tl_update: inconsistent number of kept rows");

    // the kept blocks by ascending old start, renumbered
    uint32_t *ks_in = nullptr, *ks = nullptr, *pos_in = nullptr, *ord = nullptr;
    int64_t *len = nullptr, *new_start = nullptr, *o_start = nullptr, *o_stop = nullptr;
    uint64_t *o_hk = nullptr, *o_pk = nullptr, *o_ik = nullptr;
    HIP_TRY(B.alloc(&ks_in, (size_t)K));
    HIP_TRY(B.alloc(&ks, (size_t)K));
    HIP_TRY(B.alloc(&pos_in, (size_t)K));
    HIP_TRY(B.alloc(&ord, (size_t)K));
    HIP_TRY(B.alloc(&len, (size_t)K));
    HIP_TRY(B.alloc(&new_start, (size_t)K));
    HIP_TRY(B.alloc(&o_hk, (size_t)K));
    HIP_TRY(B.alloc(&o_pk, (size_t)K));
    HIP_TRY(B.alloc(&o_ik, (size_t)K));
    HIP_TRY(B.alloc(&o_start, (size_t)K));
    HIP_TRY(B.alloc(&o_stop, (size_t)K));
    ADH_TRY(t.begin(st));
    hipLaunchKernelGGL(tl::kept_start_kernel, dim3(tl::grid_for(K)), dim3(tl::kBlock), 0, st, kept, start, K, ks_in, pos_in);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, ks_in, ks, pos_in, ord, K, 32, st));
    hipLaunchKernelGGL(tl::block_len_kernel, dim3(tl::grid_for(K)), dim3(tl::kBlock), 0, st, kept, ord, start, stop, K, len);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::exclusive_sum(B, len, new_start, K, st));
    int64_t last[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&last[0], new_start + (K - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last[1], len + (K - 1), 8, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(tl::renumber_kernel, dim3(tl::grid_for(K)), dim3(tl::kBlock), 0, st, kept, ord, new_start, len, hk, pk, ik, K,
                       o_hk, o_pk, o_ik, o_start, o_stop);
    HIP_TRY(hipGetLastError());
    ADH_TRY(t.end(st, g->gather_ms));
    const int64_t Rn = last[0] + last[1];
    if (Rn < 0 || Rn >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_tl_update: the kept fragment rows number 2^31 or more");

    uint32_t *src_row = nullptr;
    float *out[ADH_TL_MAX_MATRICES] = {nullptr, nullptr, nullptr, nullptr};
    HIP_TRY(B.alloc(&src_row, (size_t)Rn));
    for (int m = 0; m < g->M; ++m) HIP_TRY(B.alloc(&out[m], (size_t)Rn * C));
    if (Rn > 0) {
        ADH_TRY(t.begin(st));
        hipLaunchKernelGGL(tl::row_map_kernel, dim3(tl::grid_for(Rn)), dim3(tl::kBlock), 0, st, new_start, ks, K, Rn, src_row);
        HIP_TRY(hipGetLastError());
        for (int m = 0; m < g->M; ++m) {
            hipLaunchKernelGGL(tl::row_gather_kernel, dim3(tl::grid_for(Rn * C)), dim3(tl::kBlock), 0, st, (const float *)g->mat[m].p,
                               run[m], src_row, R0, Rn * C, C, out[m]);
            HIP_TRY(hipGetLastError());
        }
        ADH_TRY(t.end(st, g->gather_ms));
    }
    HIP_TRY(hipStreamSynchronize(st));

    // the new consensus replaces the old one and the run
    for (int m = 0; m < g->M; ++m) g->mat[m].adopt(B, out[m], (size_t)Rn * C);
    tl::release_staged(g);
    g->hk.adopt(B, o_hk, (size_t)K), g->pk.adopt(B, o_pk, (size_t)K), g->ik.adopt(B, o_ik, (size_t)K);
    g->start.adopt(B, o_start, (size_t)K), g->stop.adopt(B, o_stop, (size_t)K), g->kept.adopt(B, kept, (size_t)n);
    g->n_prec = K, g->n_rows = Rn, g->n_kept = K;
    if (g->hash_signed < 0) g->hash_signed = hash_is_signed ? 1 : 0;
    *n_kept = K;
    *n_kept_rows = Rn;
    return ADH_OK;
}

int adh_tl_read_kept(adh_tl_t *g, int64_t *kept, int64_t *frag_start, int64_t *frag_stop) {
    if (!g || !kept || !frag_start || !frag_stop) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->n_kept < 1) return fail(ADH_ERR_NOT_STAGED, "adh_tl_read_kept: no update");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    const size_t K = (size_t)g->n_kept;
    std::vector<uint32_t> k32(K);
    HIP_TRY(hipMemcpyAsync(k32.data(), g->kept, K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(frag_start, g->start, K * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(frag_stop, g->stop, K * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < K; ++j) kept[j] = (int64_t)k32[j];
    g->h->d2h_bytes += K * 20;
    return ADH_OK;
}

int adh_tl_read_matrix(adh_tl_t *g, int32_t m, float *out) {
    if (!g || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m < 0 || m >= g->M) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_read_matrix: no such matrix");
    if (g->n_kept < 1) return fail(ADH_ERR_NOT_STAGED, "adh_tl_read_matrix: no update");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    const size_t bytes = (size_t)g->n_rows * g->C * 4;
    if (bytes) HIP_TRY(hipMemcpyAsync(out, g->mat[m], bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += bytes;
    return ADH_OK;
}

int adh_tl_time_ms(adh_tl_t *g, double *topk_ms, double *gather_ms, double *scatter_ms) {
    if (!g || !topk_ms || !gather_ms || !scatter_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *topk_ms = g->topk_ms;
    *gather_ms = g->gather_ms;
    *scatter_ms = g->scatter_ms;
    return ADH_OK;
}

int adh_tl_qc(adh_handle_t *h, int64_t n_prec, const int64_t *frag_start, const int64_t *frag_stop, int64_t n_rows,
              int32_t n_columns, float *intensity, const float *correlation, float cutoff, float ratio, int32_t empty_passes,
              uint8_t *use_for_ms2, int64_t *n_large, double *kernel_ms) {
    if (!h || !n_large || !kernel_ms || (n_prec > 0 && (!frag_start || !frag_stop || !use_for_ms2)) ||
        (n_rows > 0 && (!intensity || !correlation)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_prec < 0 || n_rows < 0 || n_columns < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_qc: negative size");
    if (n_prec >= (int64_t)0x7FFFFFF0ll) return fail(ADH_ERR_UNSUPPORTED, "adh_tl_qc: 2^31 precursors and more");
    for (int64_t i = 0; i < n_prec; ++i) {
        if (frag_start[i] < 0 || frag_stop[i] < frag_start[i] || frag_stop[i] > n_rows)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_qc: the fragment rows of precursor " + std::to_string(i) +
                                                      " lie outside the matrices");
        if ((frag_stop[i] - frag_start[i]) * (int64_t)n_columns >= (int64_t)0x7FFFFFF0ll)
            return fail(ADH_ERR_UNSUPPORTED, "adh_tl_qc: a block of 2^31 cells and more");
    }
    *n_large = 0;
    *kernel_ms = 0.0;
    if (n_prec == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t cells = (size_t)n_rows * (size_t)n_columns;
    sess::DevBufs B;
    float *d_in = nullptr, *d_co = nullptr;
    int64_t *d_start = nullptr, *d_stop = nullptr;
    uint8_t *d_use = nullptr;
    uint32_t *list = nullptr, *d_large = nullptr;
    HIP_TRY(B.upload(&d_in, (const float *)intensity, cells, st));
    HIP_TRY(B.upload(&d_co, correlation, cells, st));
    HIP_TRY(B.upload(&d_start, frag_start, (size_t)n_prec, st));
    HIP_TRY(B.upload(&d_stop, frag_stop, (size_t)n_prec, st));
    HIP_TRY(B.alloc(&d_use, (size_t)n_prec));
    HIP_TRY(B.alloc(&list, (size_t)n_prec));
    HIP_TRY(B.alloc(&d_large, 4));
    sess::EventPair t;
    ADH_TRY(t.begin(st));
    HIP_TRY(hipMemsetAsync(d_large, 0, 4, st));
    const unsigned grid = (unsigned)std::min<int64_t>(n_prec, 1 << 16);
    hipLaunchKernelGGL(tl::qc_wave_kernel, dim3(grid), dim3(tl::kWave), 0, st, d_in, (const float *)d_co,
                       (const int64_t *)d_start, (const int64_t *)d_stop, n_prec, n_columns, cutoff, ratio, empty_passes, d_use,
                       list, d_large);
    HIP_TRY(hipGetLastError());
    uint32_t large = 0;
    HIP_TRY(hipMemcpyAsync(&large, d_large, 4, hipMemcpyDeviceToHost, st));
    ADH_TRY(t.end(st, *kernel_ms));
    if ((int64_t)large > n_prec) return fail(ADH_ERR_HIP, "adh_tl_qc: inconsistent number of large blocks");
    *n_large = large;
    if (large > 0) {
        ADH_TRY(t.begin(st));
        hipLaunchKernelGGL(tl::qc_large_kernel, dim3(large), dim3(tl::kBlock), 0, st, d_in, (const float *)d_co,
                           (const int64_t *)d_start, (const int64_t *)d_stop, n_columns, cutoff, ratio, d_use,
                           (const uint32_t *)list);
        HIP_TRY(hipGetLastError());
        ADH_TRY(t.end(st, *kernel_ms));
    }
    if (cells) HIP_TRY(hipMemcpyAsync(intensity, d_in, cells * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(use_for_ms2, d_use, (size_t)n_prec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->d2h_bytes += cells * 4 + (uint64_t)n_prec;
    return ADH_OK;
}

int adh_tl_rt_norm(adh_handle_t *h, int64_t n, int32_t delta_max, const void *rt_observed, int32_t observed_is_f64,
                   const void *rt_calibrated, int32_t calibrated_is_f64, const void *rt_library, int32_t library_is_f64,
                   void *rt_norm, double *kernel_ms) {
    if (!h || !rt_observed || !rt_norm || !kernel_ms || (delta_max && (!rt_calibrated || !rt_library)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_tl_rt_norm: no rows");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    sess::DevBufs B;
    const bool of = observed_is_f64 != 0, cf = calibrated_is_f64 != 0, lf = library_is_f64 != 0;
    const size_t ob = of ? 8 : 4, cb = cf ? 8 : 4, lb = lf ? 8 : 4;
    const size_t outb = delta_max ? ((of || cf || lf) ? 8 : 4) : ob;
    unsigned char *d_obs = nullptr, *d_cal = nullptr, *d_lib = nullptr, *d_out = nullptr;
    HIP_TRY(B.upload(&d_obs, rt_observed, (size_t)n * ob, st));
    HIP_TRY(B.alloc(&d_out, (size_t)n * outb));
    if (delta_max) {
        HIP_TRY(B.upload(&d_cal, rt_calibrated, (size_t)n * cb, st));
        HIP_TRY(B.upload(&d_lib, rt_library, (size_t)n * lb, st));
    }
    sess::EventPair t;
    *kernel_ms = 0.0;
    ADH_TRY(t.begin(st));
    if (!delta_max) {
        if (of) {
            double *mx = nullptr;
            ADH_TRY((tl::reduce_max<double, true>(B, (const double *)d_obs, n, &mx, st)));
            hipLaunchKernelGGL((tl::rt_max_norm_kernel<double>), dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st,
                               (const double *)d_obs, (const double *)mx, n, (double *)d_out);
        } else {
            float *mx = nullptr;
            ADH_TRY((tl::reduce_max<float, true>(B, (const float *)d_obs, n, &mx, st)));
            hipLaunchKernelGGL((tl::rt_max_norm_kernel<float>), dim3(tl::grid_for(n)), dim3(tl::kBlock), 0, st,
                               (const float *)d_obs, (const float *)mx, n, (float *)d_out);
        }
        HIP_TRY(hipGetLastError());
    } else {
        const int which = (of ? 4 : 0) | (cf ? 2 : 0) | (lf ? 1 : 0);
        int r = ADH_OK;
        switch (which) {
            case 0: r = tl::rt_delta_max<float, float, float>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            case 1: r = tl::rt_delta_max<float, float, double>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            case 2: r = tl::rt_delta_max<float, double, float>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            case 3: r = tl::rt_delta_max<float, double, double>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            case 4: r = tl::rt_delta_max<double, float, float>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            case 5: r = tl::rt_delta_max<double, float, double>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            case 6: r = tl::rt_delta_max<double, double, float>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
            default: r = tl::rt_delta_max<double, double, double>(B, d_obs, d_cal, d_lib, n, d_out, st); break;
        }
        ADH_TRY(r);
    }
    ADH_TRY(t.end(st, *kernel_ms));
    HIP_TRY(hipMemcpyAsync(rt_norm, d_out, (size_t)n * outb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->d2h_bytes += (uint64_t)n * outb;
    return ADH_OK;
}

}  // extern "C"
