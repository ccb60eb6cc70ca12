// adh_protein_fdr.hip - protein-group FDR on the device (outputtransform/protein_fdr.py:15-112): the features of
// every (pg, decoy) group, the target/decoy classifier and the way back from the groups to the rows.
//
// adh_pfdr_features: a stable radix sort of the rows by (pg code, decoy) keeps table order inside a group; segment
//                    heads and an inclusive scan number the groups.  Distinct precursors / sequences / runs: sort
//                    (group, value), count the heads (integer atomics).  Best, worst and mean score: the scores are
//                    gathered into sorted order in their own dtype; a group of up to kSeqRows rows is one thread's, a
//                    larger one a workgroup's.  The mean is NumPy's sum: chunks of 8 192 elements (NumPy's buffer
//                    size) added one after the other, and inside a chunk the pairwise sum - sequential below 8
//                    elements, eight strided accumulators per block of up to 128, a split at n/2 rounded down to a
//                    multiple of 8 above that - so it is bit-equal to pandas' in float32 and float64.  The workgroup
//                    gives every chunk to one thread and thread 0 adds the chunk sums in order: the association
//                    never depends on the launch.
// adh_pfdr_epoch:    one launch = one epoch of sklearn's MLPClassifier (float64, 7 -> 100 ReLU -> 1 logistic, Adam,
//                    log-loss + L2) on ONE workgroup that walks the epoch's batches in order.  The 901 parameters and
//                    their two Adam moments live in LDS.  Per batch: a thread per row runs the forward pass (loss
//                    term and output delta to LDS), then a thread per (hidden unit, half of the batch) recomputes its
//                    unit's activation row by row and accumulates the unit's nine gradient entries in registers - no
//                    batch of activations is ever held - the two halves are added in a fixed order and the owner
//                    applies Adam.  The sums over the rows (loss, output delta) and over the weights (L2) are a fifth
//                    wavefront's: strided partial sums and a fixed shuffle tree.  No floating-point atomics: two runs
//                    give the same bits.  The host draws the permutations and applies the stopping rule between
//                    launches.
// adh_pfdr_predict:  a thread per row, the same forward expression: equal rows give equal bits.
// adh_pfdr_gather:   row -> its group's value, NaN for a row of no group.
//
// Included by adh_api.hip behind adh_session.h (shares its error helpers, the handle and the session helpers).

struct adh_pfdr {
    adh_handle_t *h = nullptr;
    sess::DevBufs bufs;  // the device buffers of the last adh_pfdr_features
    int64_t n_rows = 0, n_groups = -1;
    int32_t *row_group = nullptr, *group_pg = nullptr;
    uint8_t *group_decoy = nullptr;
    double *feat = nullptr;
    // the classifier
    sess::DevBufs fit_bufs;
    int64_t n_train = 0;
    double *x = nullptr, *y = nullptr, *params = nullptr, *m = nullptr, *v = nullptr, *lr = nullptr, *loss = nullptr;
    int32_t *order = nullptr;
    int32_t max_steps = 0;
    bool fitted = false;
    sess::EventPair ev;
    double features_ms = 0.0, epochs_ms = 0.0, predict_ms = 0.0, gather_ms = 0.0;
};

namespace pfdr {

constexpr int kBlock = 256;
constexpr int kIn = 7;
constexpr int kHid = 100;
constexpr int kParams = kIn * kHid + kHid + kHid + 1;  // W1 [7][100], b1 [100], W2 [100], b2
constexpr int kB1 = kIn * kHid, kW2 = kB1 + kHid, kB2 = kW2 + kHid;
constexpr int kBatch = 200;
constexpr int kHalf = kBatch / 2;
constexpr int kWave = 64;
constexpr int kEpochBlock = kBlock + kWave;  // four wavefronts of rows / hidden units and one that sums
constexpr uint32_t kLeaf = 128;      // NumPy's PW_BLOCKSIZE
constexpr uint32_t kSeqRows = 1024;  // groups up to this many rows are summed by one thread
constexpr uint32_t kChunk = 8192;    // NumPy's buffer size: a longer vector is summed chunk after chunk

using sess::grid_for;

// ---- group features ---------------------------------------------------------------------------------------------

// rows of no group sort behind every group
__global__ void __launch_bounds__(kBlock) row_key_kernel(const int32_t *__restrict__ pg, const uint8_t *__restrict__ decoy,
                                                         int64_t n, uint32_t *__restrict__ key, uint32_t *__restrict__ row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        key[i] = pg[i] < 0 ? 0xFFFFFFFFu : (((uint32_t)pg[i] << 1) | (decoy[i] ? 1u : 0u));
        row[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(kBlock) head_kernel(const uint32_t *__restrict__ key, int64_t nv, uint32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride)
        head[k] = (k == 0 || key[k] != key[k - 1]) ? 1u : 0u;
}

// seg: the 1-based group of every sorted position (inclusive scan of the heads)
__global__ void __launch_bounds__(kBlock) seg_fill_kernel(const uint32_t *__restrict__ key, const uint32_t *__restrict__ seg,
                                                          const uint32_t *__restrict__ srow, int64_t nv,
                                                          uint32_t *__restrict__ seg_start, int32_t *__restrict__ group_pg,
                                                          uint8_t *__restrict__ group_decoy, int32_t *__restrict__ row_group) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride) {
        const uint32_t s = seg[k] - 1u;
        row_group[srow[k]] = (int32_t)s;
        if (k == 0 || seg[k - 1] != seg[k]) {
            seg_start[s] = (uint32_t)k;
            group_pg[s] = (int32_t)(key[k] >> 1);
            group_decoy[s] = (uint8_t)(key[k] & 1u);
        }
        if (k == nv - 1) seg_start[s + 1] = (uint32_t)nv;
    }
}

__global__ void __launch_bounds__(kBlock) attr_key_kernel(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ srow,
                                                          const int32_t *__restrict__ attr, int64_t nv,
                                                          uint64_t *__restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride)
        key[k] = ((uint64_t)(seg[k] - 1u) << 32) | (uint32_t)attr[srow[k]];
}

__global__ void __launch_bounds__(kBlock) distinct_kernel(const uint64_t *__restrict__ key, int64_t nv,
                                                          uint32_t *__restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride)
        if (k == 0 || key[k] != key[k - 1]) atomicAdd(&count[(uint32_t)(key[k] >> 32)], 1u);
}

// 64-bit values take two stable sorts: by value, then by group
__global__ void __launch_bounds__(kBlock) wide_gather_kernel(const int64_t *__restrict__ value, const uint32_t *__restrict__ srow,
                                                             int64_t nv, int64_t *__restrict__ out, uint32_t *__restrict__ pos) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride) {
        out[k] = value[srow[k]];
        pos[k] = (uint32_t)k;
    }
}

__global__ void __launch_bounds__(kBlock) take_seg_kernel(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ pos,
                                                          int64_t nv, uint32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride) out[k] = seg[pos[k]];
}

__global__ void __launch_bounds__(kBlock) wide_distinct_kernel(const uint32_t *__restrict__ seg, const int64_t *__restrict__ value,
                                                               int64_t nv, uint32_t *__restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride)
        if (k == 0 || seg[k] != seg[k - 1] || value[k] != value[k - 1]) atomicAdd(&count[seg[k] - 1u], 1u);
}

template <typename T>
__global__ void __launch_bounds__(kBlock) score_gather_kernel(const T *__restrict__ proba, const uint32_t *__restrict__ srow,
                                                              int64_t nv, T *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += stride) out[k] = proba[srow[k]];
}

// NumPy's pairwise_sum of up to 128 elements
template <typename T>
__device__ T leaf_sum(const T *__restrict__ a, uint32_t n) {
    if (n < 8) {
        T res = (T)0;
        for (uint32_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    T r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    uint32_t i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += a[i], r1 += a[i + 1], r2 += a[i + 2], r3 += a[i + 3];
        r4 += a[i + 4], r5 += a[i + 5], r6 += a[i + 6], r7 += a[i + 7];
    }
    T res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

__device__ __forceinline__ uint32_t left_half(uint32_t n) {
    const uint32_t h = n / 2;
    return h - (h % 8);
}

// the recursion over up to kChunk elements (six splits) on one thread: a work stack of (offset, length) nodes,
// length 0 = add the two values on top
template <typename T>
__device__ T pairwise_sum(const T *__restrict__ a, uint32_t n) {
    if (n <= kLeaf) return leaf_sum(a, n);
    uint32_t w_off[16], w_len[16];
    T val[8];
    int nw = 0, nv = 0;
    w_off[0] = 0, w_len[0] = n, nw = 1;
    while (nw > 0) {
        --nw;
        const uint32_t o = w_off[nw], l = w_len[nw];
        if (l == 0) {
            const T b = val[--nv];
            val[nv - 1] = val[nv - 1] + b;
        } else if (l <= kLeaf) {
            val[nv++] = leaf_sum(a + o, l);
        } else {
            const uint32_t h = left_half(l);
            w_off[nw] = 0, w_len[nw] = 0, ++nw;
            w_off[nw] = o + h, w_len[nw] = l - h, ++nw;
            w_off[nw] = o, w_len[nw] = h, ++nw;  // the left half is summed first
        }
    }
    return val[0];
}

// np.add.reduce of n elements: 0 + chunk + chunk + ...
template <typename T>
__device__ T numpy_sum(const T *__restrict__ a, uint32_t n) {
    T res = (T)0;
    for (uint32_t o = 0; o < n; o += kChunk) res += pairwise_sum(a + o, n - o < kChunk ? n - o : kChunk);
    return res;
}

template <typename T>
__device__ __forceinline__ void write_stats(double *__restrict__ feat, uint32_t s, uint32_t n, T sum, T lo, T hi) {
    double *f = feat + (size_t)s * kIn;
    f[0] = (double)n;
    f[1] = (double)(sum / (T)n);
    f[5] = (double)lo;
    f[6] = (double)hi;
}

// groups of up to kSeqRows rows: a thread each; the larger ones are listed for the workgroup kernel
template <typename T>
__global__ void __launch_bounds__(kBlock) small_stats_kernel(const T *__restrict__ score, const uint32_t *__restrict__ seg_start,
                                                             int64_t G, double *__restrict__ feat, uint32_t *__restrict__ list,
                                                             uint32_t *__restrict__ n_large) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < G; s += stride) {
        const uint32_t off = seg_start[s], n = seg_start[s + 1] - off;
        if (n > kSeqRows) {
            list[atomicAdd(n_large, 1u)] = (uint32_t)s;
            continue;
        }
        const T *a = score + off;
        T lo = a[0], hi = a[0];
        for (uint32_t i = 1; i < n; ++i) {
            lo = a[i] < lo ? a[i] : lo;
            hi = a[i] > hi ? a[i] : hi;
        }
        write_stats<T>(feat, (uint32_t)s, n, numpy_sum(a, n), lo, hi);
    }
}

// A larger group: kBlock chunks at a time, a thread per chunk; thread 0 adds their sums in order.
template <typename T>
__global__ void __launch_bounds__(kBlock) large_stats_kernel(const T *__restrict__ score, const uint32_t *__restrict__ seg_start,
                                                             const uint32_t *__restrict__ list, double *__restrict__ feat) {
    __shared__ T c_val[kBlock];
    __shared__ T r_lo[kBlock], r_hi[kBlock];
    const uint32_t s = list[blockIdx.x];
    const uint32_t off = seg_start[s], n = seg_start[s + 1] - off;
    const T *a = score + off;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_chunks = (n + kChunk - 1) / kChunk;
    T sum = (T)0;  // (thread 0's)
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += kBlock) {
        const uint32_t c = c0 + tid;
        if (c < n_chunks) {
            const uint32_t o = c * kChunk;
            c_val[tid] = pairwise_sum(a + o, n - o < kChunk ? n - o : kChunk);
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t m = n_chunks - c0 < (uint32_t)kBlock ? n_chunks - c0 : (uint32_t)kBlock;
            for (uint32_t k = 0; k < m; ++k) sum += c_val[k];
        }
        __syncthreads();
    }
    T lo = a[0], hi = a[0];
    for (uint32_t i = tid; i < n; i += kBlock) {
        lo = a[i] < lo ? a[i] : lo;
        hi = a[i] > hi ? a[i] : hi;
    }
    r_lo[tid] = lo, r_hi[tid] = hi;
    __syncthreads();
    for (uint32_t d = kBlock / 2; d > 0; d >>= 1) {
        if (tid < d) {
            r_lo[tid] = r_lo[tid + d] < r_lo[tid] ? r_lo[tid + d] : r_lo[tid];
            r_hi[tid] = r_hi[tid + d] > r_hi[tid] ? r_hi[tid + d] : r_hi[tid];
        }
        __syncthreads();
    }
    if (tid == 0) write_stats<T>(feat, s, n, sum, r_lo[0], r_hi[0]);
}

__global__ void __launch_bounds__(kBlock) counts_kernel(const uint32_t *__restrict__ n_seq, const uint32_t *__restrict__ n_prec,
                                                        const uint32_t *__restrict__ n_run, int64_t G, double *__restrict__ feat) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < G; s += stride) {
        double *f = feat + (size_t)s * kIn;
        f[2] = (double)n_seq[s];
        f[3] = (double)n_prec[s];
        f[4] = (double)n_run[s];
    }
}

__global__ void __launch_bounds__(kBlock) gather_kernel(const int32_t *__restrict__ row_group, const double *__restrict__ value,
                                                        int64_t n, double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int32_t g = row_group[i];
        out[i] = g >= 0 ? value[g] : __longlong_as_double(0x7FF8000000000000ll);
    }
}

template <typename T>
int score_stats(adh_pfdr *g, const void *proba, const uint32_t *srow, int64_t n, int64_t nv, int64_t G,
                const uint32_t *seg_start, uint32_t *list, uint32_t *n_large, hipStream_t st) {
    T *d_p = nullptr, *d_s = nullptr;
    HIP_TRY(g->bufs.upload(&d_p, (const T *)proba, (size_t)n, st));
    HIP_TRY(g->bufs.alloc(&d_s, (size_t)nv));
    hipLaunchKernelGGL((score_gather_kernel<T>), dim3(grid_for(nv)), dim3(kBlock), 0, st, d_p, srow, nv, d_s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(n_large, 0, 4, st));
    hipLaunchKernelGGL((small_stats_kernel<T>), dim3(grid_for(G)), dim3(kBlock), 0, st, d_s, seg_start, G, g->feat, list,
                       n_large);
    HIP_TRY(hipGetLastError());
    uint32_t large = 0;
    HIP_TRY(hipMemcpyAsync(&large, n_large, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((int64_t)large > G) return fail(ADH_ERR_HIP, "adh_pfdr_features: inconsistent group sizes");
    if (large > 0) {
        hipLaunchKernelGGL((large_stats_kernel<T>), dim3(large), dim3(kBlock), 0, st, d_s, seg_start, list, g->feat);
        HIP_TRY(hipGetLastError());
    }
    return ADH_OK;
}

// ---- the classifier ---------------------------------------------------------------------------------------------

// z_j = (sum_i x_i W1[i][j]) + b1_j, the products added in the order of i: the forward pass, the backward pass and
// the prediction all go through this one expression, so a unit is on or off alike in all three
__device__ __forceinline__ double hidden_unit(const double *__restrict__ x, const double *__restrict__ p, int j) {
    double z = x[0] * p[j];
#pragma unroll
    for (int i = 1; i < kIn; ++i) z += x[i] * p[i * kHid + j];
    z += p[kB1 + j];
    return z > 0.0 ? z : 0.0;
}

__device__ __forceinline__ double forward(const double *__restrict__ x, const double *__restrict__ p) {
    double o = hidden_unit(x, p, 0) * p[kW2];
    for (int j = 1; j < kHid; ++j) o += hidden_unit(x, p, j) * p[kW2 + j];
    o += p[kB2];
    return 1.0 / (1.0 + exp(-o));
}

__device__ __forceinline__ void adam(double *p, double *m, double *v, int k, double grad, double lr) {
    constexpr double b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double mk = b1 * m[k] + (1.0 - b1) * grad;
    const double vk = b2 * v[k] + (1.0 - b2) * (grad * grad);
    m[k] = mk, v[k] = vk;
    p[k] = p[k] + (-lr * mk / (sqrt(vk) + eps));
}

// the sum of v over the wavefront in a fixed tree; every lane gets the same bits (a + b == b + a)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// sum of f(k) over k in [0, n): lane l of the wavefront adds up k = l, l + 64, ... in order, then the tree
template <typename F>
__device__ __forceinline__ double strided_sum(int lane, int n, F &&f) {
    double v = 0.0;
    for (int k = lane; k < n; k += kWave) v += f(k);
    return wave_sum(v);
}

// Waves 0 - 3 (threads 0 ... 255) hold the rows and the hidden units; wave 4 adds up what runs over a whole batch or
// over all weights, so that no gradient thread waits for a serial sum in its own wavefront.
__global__ void __launch_bounds__(kEpochBlock) epoch_kernel(const double *__restrict__ x, const double *__restrict__ y, int32_t n,
                                                            const int32_t *__restrict__ order, const double *__restrict__ lr,
                                                            double *__restrict__ params, double *__restrict__ mom1,
                                                            double *__restrict__ mom2, double *__restrict__ loss_out) {
    __shared__ double s_p[kParams], s_m[kParams], s_v[kParams];
    __shared__ double s_x[kBatch * kIn], s_y[kBatch], s_delta[kBatch], s_ll[kBatch];
    __shared__ double s_part[9 * kHid];
    constexpr double alpha = 1e-4;
    constexpr double clip_lo = 2.220446049250313e-16, clip_hi = 1.0 - 2.220446049250313e-16;
    const int tid = threadIdx.x;
    const int lane = tid - kBlock;  // of the summing wavefront
    for (int k = tid; k < kParams; k += kEpochBlock) s_p[k] = params[k], s_m[k] = mom1[k], s_v[k] = mom2[k];
    const int batch = n < kBatch ? n : kBatch;
    double accumulated = 0.0;  // (the summing wavefront's)
    int step = 0;
    for (int start = 0; start < n; start += batch, ++step) {
        const int nb = n - start < batch ? n - start : batch;
        const double dn = (double)nb;
        __syncthreads();  // the parameters of the previous step are in place
        if (tid < nb) {
            const int r = order[start + tid];
#pragma unroll
            for (int i = 0; i < kIn; ++i) s_x[tid * kIn + i] = x[(size_t)r * kIn + i];
            s_y[tid] = y[r];
            const double p = forward(s_x + tid * kIn, s_p);
            const double pc = p < clip_lo ? clip_lo : (p > clip_hi ? clip_hi : p);
            s_ll[tid] = s_y[tid] != 0.0 ? log(pc) : log(1.0 - pc);
            s_delta[tid] = p - s_y[tid];
        }
        __syncthreads();
        // the gradient of hidden unit j over one half of the batch
        double g_w1[kIn], g_b1 = 0.0, g_w2 = 0.0, g_b2 = 0.0;
        const int j = tid % kHid, half = tid / kHid;
        if (tid < 2 * kHid) {
#pragma unroll
            for (int i = 0; i < kIn; ++i) g_w1[i] = 0.0;
            const double w2 = s_p[kW2 + j];
            const int r1 = (half + 1) * kHalf < nb ? (half + 1) * kHalf : nb;
            for (int r = half * kHalf; r < r1; ++r) {
                const double *xr = s_x + r * kIn;
                const double h = hidden_unit(xr, s_p, j);
                const double d = s_delta[r];
                g_w2 += h * d;
                const double d1 = h == 0.0 ? 0.0 : d * w2;
                g_b1 += d1;
#pragma unroll
                for (int i = 0; i < kIn; ++i) g_w1[i] += xr[i] * d1;
            }
            if (half == 1) {
#pragma unroll
                for (int i = 0; i < kIn; ++i) s_part[i * kHid + j] = g_w1[i];
                s_part[7 * kHid + j] = g_b1;
                s_part[8 * kHid + j] = g_w2;
            }
        } else if (lane >= 0) {
            // log-loss of the batch and the L2 term, put together as sklearn does; the output intercept's gradient
            const double ll = strided_sum(lane, nb, [&](int r) { return s_ll[r]; });
            const double sq1 = strided_sum(lane, kB1, [&](int k) { return s_p[k] * s_p[k]; });
            const double sq2 = strided_sum(lane, kHid, [&](int k) { return s_p[kW2 + k] * s_p[kW2 + k]; });
            g_b2 = strided_sum(lane, nb, [&](int r) { return s_delta[r]; });
            double loss = -(ll / dn);
            loss += (0.5 * alpha) * (sq1 + sq2) / dn;
            accumulated += loss * dn;
        }
        __syncthreads();
        const double rate = lr[step];
        if (tid < kHid) {
#pragma unroll
            for (int i = 0; i < kIn; ++i) {
                const int k = i * kHid + j;
                adam(s_p, s_m, s_v, k, ((g_w1[i] + s_part[k]) + alpha * s_p[k]) / dn, rate);
            }
            adam(s_p, s_m, s_v, kB1 + j, (g_b1 + s_part[7 * kHid + j]) / dn, rate);
            adam(s_p, s_m, s_v, kW2 + j, ((g_w2 + s_part[8 * kHid + j]) + alpha * s_p[kW2 + j]) / dn, rate);
        } else if (lane == 0) {
            adam(s_p, s_m, s_v, kB2, g_b2 / dn, rate);
        }
    }
    __syncthreads();
    for (int k = tid; k < kParams; k += kEpochBlock) params[k] = s_p[k], mom1[k] = s_m[k], mom2[k] = s_v[k];
    if (lane == 0) *loss_out = accumulated / (double)n;
}

__global__ void __launch_bounds__(kBlock) predict_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ params,
                                                         double *__restrict__ out) {
    __shared__ double s_p[kParams];
    for (int k = threadIdx.x; k < kParams; k += kBlock) s_p[k] = params[k];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        double xr[kIn];
#pragma unroll
        for (int i = 0; i < kIn; ++i) xr[i] = x[(size_t)r * kIn + i];
        out[r] = forward(xr, s_p);
    }
}

}  // namespace pfdr

extern "C" {

int adh_pfdr_create(adh_handle_t *h, adh_pfdr_t **out) {
    if (!h || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    adh_pfdr *g = new adh_pfdr();
    g->h = h;
    *out = g;
    return ADH_OK;
}

int adh_pfdr_destroy(adh_pfdr_t *g) {
    if (!g) return ADH_OK;
    (void)hipSetDevice(g->h->device);
    (void)hipStreamSynchronize(g->h->stream);
    delete g;  // (the members free their device memory and events)
    return ADH_OK;
}

int adh_pfdr_features(adh_pfdr_t *g, int64_t n_rows, const int32_t *pg, const uint8_t *decoy, const int64_t *precursor_idx,
                      const int32_t *sequence, const int32_t *run, const void *proba, int32_t proba_is_f64,
                      int64_t *n_groups) {
    if (!g || !pg || !decoy || !precursor_idx || !sequence || !run || !proba || !n_groups)
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    const int64_t n = n_rows;
    if (n < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_features: no rows");
    if (n >= (int64_t)0x7FFFFFF0ll) return fail(ADH_ERR_UNSUPPORTED, "adh_pfdr_features: 2^31 rows and more are not supported");
    int64_t nv = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (pg[i] >= (int32_t)0x40000000) return fail(ADH_ERR_UNSUPPORTED, "adh_pfdr_features: 2^30 pg codes and more");
        if (pg[i] < 0) continue;
        ++nv;
        if (decoy[i] > 1)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_features: decoy of row " + std::to_string(i) + " is not 0 or 1");
        const double p = proba_is_f64 ? ((const double *)proba)[i] : (double)((const float *)proba)[i];
        if (!std::isfinite(p))
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_features: proba of row " + std::to_string(i) + " is not finite");
    }
    if (nv < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_features: no row has a pg");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    g->bufs.release();
    g->n_rows = n, g->n_groups = -1;
    g->features_ms = 0.0;
    auto &B = g->bufs;

    int32_t *d_pg = nullptr, *d_seq = nullptr, *d_run = nullptr;
    uint8_t *d_decoy = nullptr;
    int64_t *d_prec = nullptr, *wide_in = nullptr, *wide = nullptr, *wide2 = nullptr;
    uint32_t *key_in = nullptr, *key = nullptr, *row_in = nullptr, *srow = nullptr, *seg = nullptr, *seg_start = nullptr,
             *pos_in = nullptr, *pos = nullptr, *sk_in = nullptr, *sk = nullptr, *counts = nullptr, *list = nullptr,
             *n_large = nullptr;
    uint64_t *akey_in = nullptr, *akey = nullptr;
    HIP_TRY(B.upload(&d_pg, pg, (size_t)n, st));
    HIP_TRY(B.upload(&d_seq, sequence, (size_t)n, st));
    HIP_TRY(B.upload(&d_run, run, (size_t)n, st));
    HIP_TRY(B.upload(&d_decoy, decoy, (size_t)n, st));
    HIP_TRY(B.upload(&d_prec, precursor_idx, (size_t)n, st));
    HIP_TRY(B.alloc(&key_in, (size_t)n));
    HIP_TRY(B.alloc(&key, (size_t)n));
    HIP_TRY(B.alloc(&row_in, (size_t)n));
    HIP_TRY(B.alloc(&srow, (size_t)n));
    HIP_TRY(B.alloc(&seg, (size_t)nv));
    HIP_TRY(B.alloc(&g->row_group, (size_t)n));
    HIP_TRY(B.alloc(&n_large, 4));

    uint32_t G32 = 0;
    int rc = sess::timed(g->ev, st, g->features_ms, [&]() -> int {
        hipLaunchKernelGGL(pfdr::row_key_kernel, dim3(pfdr::grid_for(n)), dim3(pfdr::kBlock), 0, st, d_pg, d_decoy, n, key_in,
                           row_in);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_pairs(B, key_in, key, row_in, srow, n, 32, st));
        hipLaunchKernelGGL(pfdr::head_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, key, nv, seg);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::inclusive_sum(B, seg, seg, nv, st));
        HIP_TRY(hipMemcpyAsync(&G32, seg + (nv - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    const int64_t G = G32;
    if (G < 1 || G > nv) return fail(ADH_ERR_HIP, "adh_pfdr_features: inconsistent group count");

    HIP_TRY(B.alloc(&seg_start, (size_t)G + 1));
    HIP_TRY(B.alloc(&g->group_pg, (size_t)G));
    HIP_TRY(B.alloc(&g->group_decoy, (size_t)G));
    HIP_TRY(B.alloc(&g->feat, (size_t)G * pfdr::kIn));
    HIP_TRY(B.alloc(&counts, (size_t)G * 3));
    HIP_TRY(B.alloc(&list, (size_t)G));
    HIP_TRY(B.alloc(&akey_in, (size_t)nv));
    HIP_TRY(B.alloc(&akey, (size_t)nv));
    HIP_TRY(B.alloc(&wide_in, (size_t)nv));
    HIP_TRY(B.alloc(&wide, (size_t)nv));
    HIP_TRY(B.alloc(&wide2, (size_t)nv));
    HIP_TRY(B.alloc(&pos_in, (size_t)nv));
    HIP_TRY(B.alloc(&pos, (size_t)nv));
    HIP_TRY(B.alloc(&sk_in, (size_t)nv));
    HIP_TRY(B.alloc(&sk, (size_t)nv));
    rc = sess::timed(g->ev, st, g->features_ms, [&]() -> int {
        HIP_TRY(hipMemsetAsync(g->row_group, 0xFF, (size_t)n * 4, st));
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)G * 3 * 4, st));
        hipLaunchKernelGGL(pfdr::seg_fill_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, key, seg, srow, nv,
                           seg_start, g->group_pg, g->group_decoy, g->row_group);
        HIP_TRY(hipGetLastError());
        const int32_t *attr[2] = {d_seq, d_run};
        uint32_t *count[2] = {counts, counts + 2 * G};
        for (int a = 0; a < 2; ++a) {
            hipLaunchKernelGGL(pfdr::attr_key_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, seg, srow, attr[a], nv,
                               akey_in);
            HIP_TRY(hipGetLastError());
            ADH_TRY(sess::sort_keys(B, akey_in, akey, nv, 64, st));
            hipLaunchKernelGGL(pfdr::distinct_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, akey, nv, count[a]);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(pfdr::wide_gather_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, d_prec, srow, nv,
                           wide_in, pos_in);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_pairs(B, wide_in, wide, pos_in, pos, nv, 64, st));
        hipLaunchKernelGGL(pfdr::take_seg_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, seg, pos, nv, sk_in);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_pairs(B, sk_in, sk, wide, wide2, nv, 32, st));
        hipLaunchKernelGGL(pfdr::wide_distinct_kernel, dim3(pfdr::grid_for(nv)), dim3(pfdr::kBlock), 0, st, sk, wide2, nv,
                           counts + G);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pfdr::counts_kernel, dim3(pfdr::grid_for(G)), dim3(pfdr::kBlock), 0, st, counts, counts + G,
                           counts + 2 * G, G, g->feat);
        HIP_TRY(hipGetLastError());
        return proba_is_f64 ? pfdr::score_stats<double>(g, proba, srow, n, nv, G, seg_start, list, n_large, st)
                            : pfdr::score_stats<float>(g, proba, srow, n, nv, G, seg_start, list, n_large, st);
    });
    if (rc != ADH_OK) return rc;
    g->n_groups = G;
    *n_groups = G;
    return ADH_OK;
}

int adh_pfdr_read_features(adh_pfdr_t *g, int32_t *group_pg, uint8_t *group_decoy, double *features, int32_t *row_group) {
    if (!g || !group_pg || !group_decoy || !features) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->n_groups < 1) return fail(ADH_ERR_NOT_STAGED, "adh_pfdr_read_features: no group features");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    const size_t G = (size_t)g->n_groups;
    HIP_TRY(hipMemcpyAsync(group_pg, g->group_pg, G * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(group_decoy, g->group_decoy, G, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(features, g->feat, G * pfdr::kIn * 8, hipMemcpyDeviceToHost, st));
    if (row_group) HIP_TRY(hipMemcpyAsync(row_group, g->row_group, (size_t)g->n_rows * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += G * (5 + pfdr::kIn * 8) + (row_group ? (uint64_t)g->n_rows * 4 : 0);
    return ADH_OK;
}

int adh_pfdr_fit_begin(adh_pfdr_t *g, int64_t n_train, const double *x, const uint8_t *y, const double *params) {
    if (!g || !x || !y || !params) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_train < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_fit_begin: no training rows");
    if (n_train >= (int64_t)0x7FFFFFF0ll / pfdr::kIn) return fail(ADH_ERR_UNSUPPORTED, "adh_pfdr_fit_begin: too many rows");
    std::vector<double> yd((size_t)n_train);
    for (int64_t i = 0; i < n_train; ++i) {
        if (y[i] > 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_fit_begin: label " + std::to_string(i) + " is not 0 or 1");
        yd[(size_t)i] = (double)y[i];
    }
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    g->fit_bufs.release();
    g->fitted = false;
    g->epochs_ms = g->predict_ms = 0.0;
    auto &B = g->fit_bufs;
    const int64_t batch = std::min<int64_t>(n_train, pfdr::kBatch);
    g->max_steps = (int32_t)((n_train + batch - 1) / batch);
    HIP_TRY(B.upload(&g->x, x, (size_t)n_train * pfdr::kIn, st));
    HIP_TRY(B.upload(&g->y, (const double *)yd.data(), (size_t)n_train, st));
    HIP_TRY(B.alloc(&g->order, (size_t)n_train));
    HIP_TRY(B.alloc(&g->lr, (size_t)g->max_steps));
    HIP_TRY(B.upload(&g->params, params, (size_t)pfdr::kParams, st));
    HIP_TRY(B.alloc(&g->m, (size_t)pfdr::kParams));
    HIP_TRY(B.alloc(&g->v, (size_t)pfdr::kParams));
    HIP_TRY(B.alloc(&g->loss, 4));
    HIP_TRY(hipMemsetAsync(g->m, 0, (size_t)pfdr::kParams * 8, st));
    HIP_TRY(hipMemsetAsync(g->v, 0, (size_t)pfdr::kParams * 8, st));
    HIP_TRY(hipStreamSynchronize(st));  // (yd leaves scope)
    g->n_train = n_train;
    g->fitted = true;
    return ADH_OK;
}

int adh_pfdr_epoch(adh_pfdr_t *g, const int32_t *order, int32_t n_steps, const double *step_size, double *loss) {
    if (!g || !order || !step_size || !loss) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!g->fitted) return fail(ADH_ERR_NOT_STAGED, "adh_pfdr_epoch: no adh_pfdr_fit_begin");
    if (n_steps != g->max_steps)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_epoch: an epoch of these rows takes " + std::to_string(g->max_steps) +
                                                  " steps");
    for (int64_t i = 0; i < g->n_train; ++i)
        if (order[i] < 0 || order[i] >= g->n_train)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_epoch: order " + std::to_string(i) + " is out of range");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipMemcpyAsync(g->order, order, (size_t)g->n_train * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g->lr, step_size, (size_t)n_steps * 8, hipMemcpyHostToDevice, st));
    const int rc = sess::timed(g->ev, st, g->epochs_ms, [&]() -> int {  // (adds up over the epochs of one fit)
        hipLaunchKernelGGL(pfdr::epoch_kernel, dim3(1), dim3(pfdr::kEpochBlock), 0, st, g->x, g->y, (int32_t)g->n_train, g->order,
                           g->lr, g->params, g->m, g->v, g->loss);
        HIP_TRY(hipGetLastError());
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(loss, g->loss, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += 8;
    return ADH_OK;
}

int adh_pfdr_predict(adh_pfdr_t *g, int64_t n, const double *x, double *proba) {
    if (!g || !x || !proba) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!g->fitted) return fail(ADH_ERR_NOT_STAGED, "adh_pfdr_predict: no adh_pfdr_fit_begin");
    if (n < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_predict: no rows");
    if (n >= (int64_t)0x7FFFFFF0ll / pfdr::kIn) return fail(ADH_ERR_UNSUPPORTED, "adh_pfdr_predict: too many rows");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    fdr::Scratch s;
    double *d_x = nullptr, *d_p = nullptr;
    HIP_TRY(s.alloc(&d_x, (size_t)n * pfdr::kIn));
    HIP_TRY(s.alloc(&d_p, (size_t)n));
    HIP_TRY(hipMemcpyAsync(d_x, x, (size_t)n * pfdr::kIn * 8, hipMemcpyHostToDevice, st));
    g->predict_ms = 0.0;
    const int rc = sess::timed(g->ev, st, g->predict_ms, [&]() -> int {
        hipLaunchKernelGGL(pfdr::predict_kernel, dim3(pfdr::grid_for(n)), dim3(pfdr::kBlock), 0, st, d_x, n, g->params, d_p);
        HIP_TRY(hipGetLastError());
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(proba, d_p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += (uint64_t)n * 8;
    return ADH_OK;
}

int adh_pfdr_gather(adh_pfdr_t *g, int64_t n_groups, const double *group_value, double *row_value) {
    if (!g || !group_value || !row_value) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->n_groups < 1) return fail(ADH_ERR_NOT_STAGED, "adh_pfdr_gather: no group features");
    if (n_groups != g->n_groups)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pfdr_gather: the table has " + std::to_string(g->n_groups) + " groups");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    fdr::Scratch s;
    double *d_v = nullptr, *d_out = nullptr;
    HIP_TRY(s.alloc(&d_v, (size_t)n_groups));
    HIP_TRY(s.alloc(&d_out, (size_t)g->n_rows));
    HIP_TRY(hipMemcpyAsync(d_v, group_value, (size_t)n_groups * 8, hipMemcpyHostToDevice, st));
    g->gather_ms = 0.0;
    const int rc = sess::timed(g->ev, st, g->gather_ms, [&]() -> int {
        hipLaunchKernelGGL(pfdr::gather_kernel, dim3(pfdr::grid_for(g->n_rows)), dim3(pfdr::kBlock), 0, st, g->row_group, d_v,
                           g->n_rows, d_out);
        HIP_TRY(hipGetLastError());
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(row_value, d_out, (size_t)g->n_rows * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += (uint64_t)g->n_rows * 8;
    return ADH_OK;
}

int adh_pfdr_time_ms(adh_pfdr_t *g, double *features_ms, double *epochs_ms, double *predict_ms, double *gather_ms) {
    if (!g || !features_ms || !epochs_ms || !predict_ms || !gather_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *features_ms = g->features_ms;
    *epochs_ms = g->epochs_ms;
    *predict_ms = g->predict_ms;
    *gather_ms = g->gather_ms;
    return ADH_OK;
}

}  // extern "C"
