// adh_mbr_library.hip - the match-between-runs library of the output stage (libtransform/mbr.py: MbrLibraryBuilder,
// IndexBuilder): the PSM table aggregated per elution group and per precursor hash, the base library cut down to the
// elution groups that passed, and the observed RT / protein group of every remaining precursor.
//
// adh_mbr_aggregate: rows with qval <= fdr are compacted (a flagged select, NaN is false).  For each of the two keys
//                    (elution_group_idx, mod_seq_charge_hash) the survivors are ordered by (key, rt_observed) with
//                    two stable radix passes over order-preserving uint64 keys (a signed key with its sign bit
//                    flipped; the RT as float64 bits, -0.0 -> +0.0, every NaN the largest key).  Segment heads, a
//                    flagged select of the head positions and an inclusive sum give the segments.  One lane per
//                    segment finds where the NaNs begin by binary search and reads the middle one or two values:
//                    the sort has ordered them, so a segment of any size costs the same.  The first non-null pg of a
//                    segment is an integer atomic minimum over the original rows.  The groups that passed are the
//                    distinct elution groups (those with a target row unless decoys are kept).
// adh_mbr_filter:    membership of every library precursor by binary search in the passed groups, the kept rows by a
//                    flagged select (library row order), then the block bookkeeping of adh_tl_update (its kernels are
//                    shared, namespace tl): the kept blocks by ascending old start (stable), an exclusive scan of
//                    their lengths, the source row of every new dense row, one gather per matrix.  The gather moves
//                    16 bytes per lane along the columns, a row per lane group, when the rows are 16-byte multiples.
// adh_mbr_assign:    per precursor two binary searches (elution group: the fallback slot; hash: the specific slot or
//                    a miss) in the tables the aggregate left in HBM.  The tables are 8 bytes per distinct key: a few
//                    MB, which an XCD's 4 MiB L2 holds whole or nearly so - every lane walks the same top levels and
//                    they stay hot without staging them; a merge over sorted queries would need one more sort of the
//                    library for a search that is a small part of the step.
// adh_mbr_index:     IndexBuilder for any two key columns: the lookup keys sorted with their positions, adjacent equal
//                    keys flagged (pandas refuses a duplicate index), a binary search per target.
// adh_mbr_notnull_objects: the null mask of the pg column on the host (no kernel): None and str told apart by pointer.
//
// All global writes are plain vector stores or vector integer atomics.  Included by adh_api.hip behind adh_session.h
// (shares its error helpers, the handle and the session helpers); the block-bookkeeping kernels of namespace tl come
// with the include below.
#include "adh_transfer_library.hip"

struct adh_mbr {
    adh_handle_t *h = nullptr;
    // the aggregate: [0] by elution group, [1] by hash - distinct keys ascending (order-preserving form), median,
    // original row of the first non-null pg (0xFFFFFFFF: none); the groups that passed.  Grow-only.
    sess::DevArray<uint64_t> key[2];
    sess::DevArray<double> med[2];
    sess::DevArray<uint32_t> first[2];
    int64_t n_seg[2] = {-1, -1};
    sess::DevArray<uint64_t> groups;
    int64_t n_groups = -1;
    int rt_is_f64 = 0, hash_signed = 0, eg_is_u32 = 0;
    // the filter: kept library rows, their renumbered blocks, the source row of every kept dense row, the matrices
    sess::DevArray<uint32_t> kept, src_row;
    sess::DevArray<int64_t> start, stop;
    sess::DevArray<float> mat[ADH_TL_MAX_MATRICES];
    int64_t n_kept = -1, n_rows = 0;
    int32_t C = 0, M = 0;
    sess::EventPair ev;
    double aggregate_ms = 0.0, filter_ms = 0.0, gather_ms = 0.0, assign_ms = 0.0;
    uint64_t h2d_bytes = 0, d2h_bytes = 0;
};

namespace mbr {

using sess::grid_for;
using sess::kBlock;

constexpr uint64_t kSign = 0x8000000000000000ull;
constexpr uint64_t kNanKey = 0xFFFFFFFFFFFFFFFFull;
constexpr int kKeyU32 = 0, kKeyI64 = 1, kKeyU64 = 2;

__device__ __forceinline__ uint64_t load_key(const void *__restrict__ col, int32_t kind, int64_t i) {
    if (kind == kKeyU32) return (uint64_t)((const uint32_t *)col)[i] ^ kSign;  // (as the int64 of the same value)
    const uint64_t v = ((const uint64_t *)col)[i];
    return kind == kKeyI64 ? (v ^ kSign) : v;
}

__device__ __forceinline__ uint64_t rt_key(double v) {
    if (v != v) return kNanKey;  // NaN sorts last
    if (v == 0.0) v = 0.0;       // -0.0 counts as +0.0
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | kSign);
}

__device__ __forceinline__ double rt_from_key(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~kSign) : ~k));
}

__global__ void __launch_bounds__(kBlock) pass_kernel(const double *__restrict__ qval, double fdr, int64_t n, uint8_t *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) flag[i] = qval[i] <= fdr ? 1 : 0;
}

// the two sort keys of the survivors, in the order of the compaction
__global__ void __launch_bounds__(kBlock) keys_kernel(const uint32_t *__restrict__ sel, int64_t K, const void *__restrict__ col,
                                                      int32_t kind, const void *__restrict__ rt, int32_t rt_is_f64,
                                                      uint64_t *__restrict__ key, uint64_t *__restrict__ rtk) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += stride) {
        const int64_t i = sel[j];
        key[j] = load_key(col, kind, i);
        rtk[j] = rt_key(rt_is_f64 ? ((const double *)rt)[i] : (double)((const float *)rt)[i]);
    }
}

__global__ void __launch_bounds__(kBlock) head_flag_kernel(const uint64_t *__restrict__ key, int64_t n, uint32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
        head[k] = (k == 0 || key[k] != key[k - 1]) ? 1u : 0u;
}

// seg[k]: 1 + the segment of sorted position k.  The first non-null pg of a segment is the smallest original row
// with one; a segment of the elution groups with a target row is marked.
__global__ void __launch_bounds__(kBlock) segment_rows_kernel(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ perm,
                                                              const uint32_t *__restrict__ sel, const uint8_t *__restrict__ pg_notnull,
                                                              const uint8_t *__restrict__ decoy, int64_t K,
                                                              uint32_t *__restrict__ first, uint8_t *__restrict__ has_target) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const uint32_t s = seg[k] - 1u, row = sel[perm[k]];
        if (pg_notnull[row]) atomicMin(&first[s], row);
        if (has_target && !decoy[row]) has_target[s] = 1;
    }
}

// one lane per segment: the values are in order, the NaNs behind them
__global__ void __launch_bounds__(kBlock) median_kernel(const uint64_t *__restrict__ key, const uint64_t *__restrict__ rtk,
                                                        const uint32_t *__restrict__ seg_start, int64_t S, int64_t K,
                                                        uint64_t *__restrict__ o_key, double *__restrict__ o_med) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride) {
        const int64_t a = seg_start[s], b = s + 1 < S ? (int64_t)seg_start[s + 1] : K;
        int64_t lo = a, hi = b;  // the first NaN of [a, b)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (rtk[mid] != kNanKey) lo = mid + 1;
            else hi = mid;
        }
        const int64_t m = lo - a;
        double v = __longlong_as_double(0x7FF8000000000000ll);
        if (m > 0) {
            const double x = rt_from_key(rtk[a + (m - 1) / 2]);
            v = (m & 1) ? x : (x + rt_from_key(rtk[a + m / 2])) / 2.0;
        }
        o_key[s] = key[a];
        o_med[s] = v;
    }
}

// the position of `k` in the ascending table, or -1
__device__ __forceinline__ int64_t find_key(const uint64_t *__restrict__ table, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (table[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && table[lo] == k) ? lo : -1;
}

__global__ void __launch_bounds__(kBlock) member_kernel(const void *__restrict__ eg, int32_t kind, int64_t n,
                                                        const uint64_t *__restrict__ groups, int64_t G, uint8_t *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        flag[i] = find_key(groups, G, load_key(eg, kind, i)) >= 0 ? 1 : 0;
}

// i: the kept blocks by ascending old start; ord[i]: the kept rows in library order
__global__ void __launch_bounds__(kBlock) renumber_kernel(const uint32_t *__restrict__ ord, const int64_t *__restrict__ new_start,
                                                          const int64_t *__restrict__ len, int64_t K, int64_t *__restrict__ o_start,
                                                          int64_t *__restrict__ o_stop) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += stride) {
        const uint32_t j = ord[i];
        o_start[j] = new_start[i];
        o_stop[j] = new_start[i] + len[i];
    }
}

// rows of Q float4: a group of 1 << lane_shift lanes per row, 16 bytes a lane along the columns; no LDS
__global__ void __launch_bounds__(kBlock) row_gather4_kernel(const float4 *__restrict__ src, const uint32_t *__restrict__ src_row,
                                                             int64_t R, int32_t Q, int32_t lane_shift, float4 *__restrict__ out) {
    const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> lane_shift;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lanes = 1 << lane_shift, c0 = (int32_t)(t & (lanes - 1));
    for (int64_t r = t >> lane_shift; r < R; r += stride) {
        const int64_t s = src_row[r];
        for (int32_t c = c0; c < Q; c += lanes) out[r * Q + c] = src[s * Q + c];
    }
}

__global__ void __launch_bounds__(kBlock) assign_kernel(const void *__restrict__ eg, int32_t eg_kind, const void *__restrict__ hash,
                                                        int32_t hash_kind, int64_t n, const uint64_t *__restrict__ eg_key,
                                                        const double *__restrict__ eg_med, const uint32_t *__restrict__ eg_first,
                                                        int64_t S_eg, const uint64_t *__restrict__ h_key,
                                                        const double *__restrict__ h_med, const uint32_t *__restrict__ h_first,
                                                        int64_t S_h, int32_t rt_is_f64, void *__restrict__ rt, int64_t *__restrict__ pg_row,
                                                        uint32_t *__restrict__ n_missing) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t fb = find_key(eg_key, S_eg, load_key(eg, eg_kind, i));
        const int64_t sp = find_key(h_key, S_h, load_key(hash, hash_kind, i));
        double v = __longlong_as_double(0x7FF8000000000000ll);
        uint32_t row = 0xFFFFFFFFu;
        if (fb < 0) atomicAdd(n_missing, 1u);
        if (sp >= 0) v = h_med[sp], row = h_first[sp];
        else if (fb >= 0) v = eg_med[fb], row = eg_first[fb];
        if (rt_is_f64) ((double *)rt)[i] = v;
        else ((float *)rt)[i] = (float)v;
        pg_row[i] = row == 0xFFFFFFFFu ? -1 : (int64_t)row;
    }
}

__global__ void __launch_bounds__(kBlock) adjacent_equal_kernel(const uint64_t *__restrict__ key, int64_t n, int32_t *__restrict__ dup) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; k < n; k += stride)
        if (key[k] == key[k - 1]) *dup = 1;
}

__global__ void __launch_bounds__(kBlock) index_kernel(const uint64_t *__restrict__ target, int64_t n, const uint64_t *__restrict__ sorted,
                                                       const uint32_t *__restrict__ pos, int64_t L, int64_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t at = find_key(sorted, L, target[i]);
        out[i] = at < 0 ? -1 : (int64_t)pos[at];
    }
}

inline int key_kind(int32_t is_u32) { return is_u32 ? kKeyU32 : kKeyI64; }
inline int hash_kind(int32_t is_signed) { return is_signed ? kKeyI64 : kKeyU64; }

// one key of the aggregate: fills g->key / med / first [w]; w == 0 also the groups that passed
int aggregate_key(adh_mbr *g, sess::DevBufs &B, int w, const uint32_t *sel, int64_t K, const void *col, int32_t kind, const void *rt,
                  int32_t rt_is_f64, const uint8_t *pg_notnull, const uint8_t *decoy, int32_t keep_decoys, const uint32_t *iota,
                  hipStream_t st) {
    uint64_t *key = nullptr, *rtk = nullptr, *k_in = nullptr, *k_s = nullptr, *rtk_s = nullptr;
    uint32_t *p1 = nullptr, *p2 = nullptr, *head = nullptr, *seg = nullptr, *seg_start = nullptr, *n_sel = nullptr;
    uint8_t *has_target = nullptr;
    HIP_TRY(B.alloc(&key, (size_t)K));
    HIP_TRY(B.alloc(&rtk, (size_t)K));
    HIP_TRY(B.alloc(&k_in, (size_t)K));
    HIP_TRY(B.alloc(&k_s, (size_t)K));
    HIP_TRY(B.alloc(&rtk_s, (size_t)K));
    HIP_TRY(B.alloc(&p1, (size_t)K));
    HIP_TRY(B.alloc(&p2, (size_t)K));
    HIP_TRY(B.alloc(&head, (size_t)K));
    HIP_TRY(B.alloc(&seg, (size_t)K));
    HIP_TRY(B.alloc(&seg_start, (size_t)K));
    HIP_TRY(B.alloc(&n_sel, 4));
    if (w == 0) HIP_TRY(B.alloc(&has_target, (size_t)K));
    const dim3 grid(grid_for(K)), block(kBlock);
    hipLaunchKernelGGL(keys_kernel, grid, block, 0, st, sel, K, col, kind, rt, rt_is_f64, key, rtk);
    HIP_TRY(hipGetLastError());
    // least significant key first: the RT, then the group key
    ADH_TRY(sess::sort_pairs(B, rtk, rtk_s, iota, p1, K, 64, st));
    hipLaunchKernelGGL(tl::take_kernel, grid, block, 0, st, (const uint64_t *)key, (const uint32_t *)p1, K, k_in);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, k_in, k_s, p1, p2, K, 64, st));
    hipLaunchKernelGGL(tl::take_kernel, grid, block, 0, st, (const uint64_t *)rtk, (const uint32_t *)p2, K, rtk_s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(head_flag_kernel, grid, block, 0, st, (const uint64_t *)k_s, K, head);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::inclusive_sum(B, head, seg, K, st));
    ADH_TRY(sess::select_flagged(B, iota, (const uint32_t *)head, seg_start, n_sel, K, st));
    uint32_t S32 = 0;
    HIP_TRY(hipMemcpyAsync(&S32, n_sel, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t S = S32;
    if (S < 1 || S > K) return fail(ADH_ERR_HIP, "adh_mbr_aggregate: inconsistent number of segments");
    HIP_TRY(g->key[w].reserve((size_t)S));
    HIP_TRY(g->med[w].reserve((size_t)S));
    HIP_TRY(g->first[w].reserve((size_t)S));
    HIP_TRY(hipMemsetAsync(g->first[w], 0xFF, (size_t)S * 4, st));
    if (has_target) HIP_TRY(hipMemsetAsync(has_target, 0, (size_t)S, st));
    hipLaunchKernelGGL(segment_rows_kernel, grid, block, 0, st, (const uint32_t *)seg, (const uint32_t *)p2, sel, pg_notnull, decoy, K,
                       g->first[w].p, has_target);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(median_kernel, dim3(grid_for(S)), block, 0, st, (const uint64_t *)k_s, (const uint64_t *)rtk_s,
                       (const uint32_t *)seg_start, S, K, g->key[w].p, g->med[w].p);
    HIP_TRY(hipGetLastError());
    g->n_seg[w] = S;
    if (w != 0) return ADH_OK;
    HIP_TRY(g->groups.reserve((size_t)S));
    if (keep_decoys) {
        HIP_TRY(hipMemcpyAsync(g->groups, g->key[0], (size_t)S * 8, hipMemcpyDeviceToDevice, st));
        g->n_groups = S;
    } else {
        ADH_TRY(sess::select_flagged(B, (const uint64_t *)g->key[0].p, (const uint8_t *)has_target, g->groups.p, n_sel, S, st));
        uint32_t G32 = 0;
        HIP_TRY(hipMemcpyAsync(&G32, n_sel, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)G32 > S) return fail(ADH_ERR_HIP, "adh_mbr_aggregate: inconsistent number of groups");
        g->n_groups = G32;
    }
    return ADH_OK;
}

}  // namespace mbr

extern "C" {

int adh_mbr_create(adh_handle_t *h, adh_mbr_t **out) {
    if (!h || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    adh_mbr *g = new adh_mbr();
    g->h = h;
    *out = g;
    return ADH_OK;
}

int adh_mbr_destroy(adh_mbr_t *g) {
    if (!g) return ADH_OK;
    (void)hipSetDevice(g->h->device);
    (void)hipStreamSynchronize(g->h->stream);
    delete g;  // (the members free their device memory and events)
    return ADH_OK;
}

int adh_mbr_aggregate(adh_mbr_t *g, int64_t n, const double *qval, const uint8_t *decoy, const void *elution_group_idx,
                      int32_t group_is_u32, const void *mod_seq_charge_hash, int32_t hash_is_signed, const void *rt_observed,
                      int32_t rt_is_f64, const uint8_t *pg_notnull, double fdr, int32_t keep_decoys, int64_t *n_passed,
                      int64_t *n_by_group, int64_t *n_by_hash, int64_t *n_groups) {
    if (!g || !n_passed || !n_by_group || !n_by_hash || !n_groups ||
        (n > 0 && (!qval || !decoy || !elution_group_idx || !mod_seq_charge_hash || !rt_observed || !pg_notnull)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_aggregate: negative size");
    if (n >= (int64_t)0x7FFFFFF0ll) return fail(ADH_ERR_UNSUPPORTED, "adh_mbr_aggregate: 2^31 rows and more are not supported");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    g->n_seg[0] = g->n_seg[1] = 0;
    g->n_groups = 0;
    g->rt_is_f64 = rt_is_f64 ? 1 : 0;
    g->hash_signed = hash_is_signed ? 1 : 0;
    g->eg_is_u32 = group_is_u32 ? 1 : 0;
    g->aggregate_ms = 0.0;
    *n_passed = *n_by_group = *n_by_hash = *n_groups = 0;
    if (n == 0) return ADH_OK;
    const size_t gb = group_is_u32 ? 4 : 8, rb = rt_is_f64 ? 8 : 4;
    sess::DevBufs B;
    double *d_q = nullptr;
    uint8_t *d_decoy = nullptr, *d_pg = nullptr, *flag = nullptr;
    unsigned char *d_eg = nullptr, *d_hash = nullptr, *d_rt = nullptr;
    uint32_t *iota = nullptr, *sel = nullptr, *n_sel = nullptr;
    HIP_TRY(B.upload(&d_q, qval, (size_t)n, st));
    HIP_TRY(B.upload(&d_decoy, decoy, (size_t)n, st));
    HIP_TRY(B.upload(&d_pg, pg_notnull, (size_t)n, st));
    HIP_TRY(B.alloc(&flag, (size_t)n));
    HIP_TRY(B.upload(&d_eg, elution_group_idx, (size_t)n * gb, st));
    HIP_TRY(B.upload(&d_hash, mod_seq_charge_hash, (size_t)n * 8, st));
    HIP_TRY(B.upload(&d_rt, rt_observed, (size_t)n * rb, st));
    HIP_TRY(B.alloc(&iota, (size_t)n));
    HIP_TRY(B.alloc(&sel, (size_t)n));
    HIP_TRY(B.alloc(&n_sel, 4));
    g->h2d_bytes += (uint64_t)n * (8 + 1 + 1 + gb + 8 + rb);
    sess::EventPair &t = g->ev;
    ADH_TRY(t.begin(st));
    hipLaunchKernelGGL(mbr::pass_kernel, dim3(mbr::grid_for(n)), dim3(mbr::kBlock), 0, st, (const double *)d_q, fdr, n, flag);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sess::iota_kernel, dim3(mbr::grid_for(n)), dim3(mbr::kBlock), 0, st, iota, n);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::select_flagged(B, (const uint32_t *)iota, (const uint8_t *)flag, sel, n_sel, n, st));
    uint32_t K32 = 0;
    HIP_TRY(hipMemcpyAsync(&K32, n_sel, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t K = K32;
    if (K > n) return fail(ADH_ERR_HIP, "adh_mbr_aggregate: inconsistent number of passing rows");
    if (K > 0) {
        ADH_TRY(mbr::aggregate_key(g, B, 0, sel, K, d_eg, mbr::key_kind(group_is_u32), d_rt, rt_is_f64, d_pg, d_decoy, keep_decoys,
                                  iota, st));
        ADH_TRY(mbr::aggregate_key(g, B, 1, sel, K, d_hash, mbr::hash_kind(hash_is_signed), d_rt, rt_is_f64, d_pg, d_decoy, 1, iota,
                                  st));
    }
    ADH_TRY(t.end(st, g->aggregate_ms));
    g->d2h_bytes += 16;
    *n_passed = K;
    *n_by_group = g->n_seg[0];
    *n_by_hash = g->n_seg[1];
    *n_groups = g->n_groups;
    return ADH_OK;
}

int adh_mbr_read_table(adh_mbr_t *g, int32_t which, void *keys, void *median, int64_t *first_row) {
    if (!g || !keys || (which != 2 && (!median || !first_row))) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (which < 0 || which > 2) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_read_table: 0 by group, 1 by hash, 2 the groups that passed");
    if (g->n_groups < 0) return fail(ADH_ERR_NOT_STAGED, "adh_mbr_read_table: no aggregate");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    const size_t S = (size_t)(which == 2 ? g->n_groups : g->n_seg[which]);
    if (S == 0) return ADH_OK;
    uint64_t *k = (uint64_t *)keys;
    HIP_TRY(hipMemcpyAsync(k, which == 2 ? g->groups.p : g->key[which].p, S * 8, hipMemcpyDeviceToHost, st));
    std::vector<double> med;
    std::vector<uint32_t> first;
    if (which != 2) {
        med.resize(S), first.resize(S);
        HIP_TRY(hipMemcpyAsync(med.data(), g->med[which], S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(first.data(), g->first[which], S * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // back from the order-preserving form: the groups as int64 values, the hash in the bits it came in
    if (which != 1 || g->hash_signed)
        for (size_t s = 0; s < S; ++s) k[s] ^= mbr::kSign;
    if (which != 2) {
        for (size_t s = 0; s < S; ++s) {
            if (g->rt_is_f64) ((double *)median)[s] = med[s];
            else ((float *)median)[s] = (float)med[s];
            first_row[s] = first[s] == 0xFFFFFFFFu ? -1 : (int64_t)first[s];
        }
    }
    g->d2h_bytes += S * (which == 2 ? 8 : 20);
    return ADH_OK;
}

int adh_mbr_filter(adh_mbr_t *g, int64_t n_lib, const void *elution_group_idx, int32_t group_is_u32, const int64_t *frag_start,
                   const int64_t *frag_stop, int64_t n_rows, int32_t n_columns, int32_t n_matrices, const float *const *matrices,
                   int64_t *n_kept, int64_t *n_kept_rows) {
    if (!g || !n_kept || !n_kept_rows || (n_lib > 0 && (!elution_group_idx || !frag_start || !frag_stop)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->n_groups < 0) return fail(ADH_ERR_NOT_STAGED, "adh_mbr_filter: no aggregate");
    if (n_lib < 0 || n_rows < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_filter: negative size");
    if (n_lib >= (int64_t)0x7FFFFFF0ll || n_rows >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_mbr_filter: 2^31 rows and more are not supported");
    const int32_t M = matrices ? n_matrices : 0;
    if (matrices && (n_matrices < 1 || n_matrices > ADH_TL_MAX_MATRICES))
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_filter: 1 to " + std::to_string(ADH_TL_MAX_MATRICES) + " dense matrices");
    if (matrices && (n_columns < 1 || n_columns > 4096)) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_filter: 1 to 4096 fragment columns");
    for (int m = 0; m < M; ++m)
        if (!matrices[m] && n_rows > 0) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL matrix");
    for (int64_t i = 0; i < n_lib; ++i)
        if (frag_start[i] < 0 || frag_stop[i] < frag_start[i] || frag_stop[i] > n_rows)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_filter: the fragment rows of precursor " + std::to_string(i) +
                                                      " lie outside the library's matrices");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    g->n_kept = -1, g->n_rows = 0, g->C = n_columns, g->M = M;
    g->filter_ms = g->gather_ms = 0.0;
    *n_kept = *n_kept_rows = 0;
    if (n_lib == 0 || g->n_groups == 0) {
        g->n_kept = 0;
        return ADH_OK;
    }
    const int32_t C = n_columns;
    const size_t gb = group_is_u32 ? 4 : 8;
    sess::DevBufs B;
    unsigned char *d_eg = nullptr;
    int64_t *start = nullptr, *stop = nullptr;
    uint8_t *flag = nullptr;
    uint32_t *iota = nullptr, *n_sel = nullptr;
    const float *src[ADH_TL_MAX_MATRICES] = {nullptr, nullptr, nullptr, nullptr};
    HIP_TRY(B.upload(&d_eg, elution_group_idx, (size_t)n_lib * gb, st));
    HIP_TRY(B.upload(&start, frag_start, (size_t)n_lib, st));
    HIP_TRY(B.upload(&stop, frag_stop, (size_t)n_lib, st));
    HIP_TRY(B.alloc(&flag, (size_t)n_lib));
    HIP_TRY(B.alloc(&iota, (size_t)n_lib));
    HIP_TRY(B.alloc(&n_sel, 4));
    HIP_TRY(g->kept.reserve((size_t)n_lib));
    g->h2d_bytes += (uint64_t)n_lib * (gb + 16);
    {
        // the matrices are the bytes of this step: from the caller's pageable arrays through the handle's page-locked lanes
        std::vector<UpJob> jobs;
        for (int m = 0; m < M; ++m) {
            float *d = nullptr;
            HIP_TRY(B.alloc(&d, (size_t)n_rows * C));
            jobs.push_back(UpJob{d, matrices[m], (size_t)n_rows * C * 4});
            g->h2d_bytes += (uint64_t)n_rows * C * 4;
            src[m] = d;
        }
        if (M > 0 && n_rows > 0) ADH_TRY(upload_staged(g->h, jobs));
    }
    sess::EventPair &t = g->ev;
    ADH_TRY(t.begin(st));
    hipLaunchKernelGGL(mbr::member_kernel, dim3(mbr::grid_for(n_lib)), dim3(mbr::kBlock), 0, st, (const void *)d_eg,
                       mbr::key_kind(group_is_u32), n_lib, (const uint64_t *)g->groups.p, g->n_groups, flag);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sess::iota_kernel, dim3(mbr::grid_for(n_lib)), dim3(mbr::kBlock), 0, st, iota, n_lib);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::select_flagged(B, (const uint32_t *)iota, (const uint8_t *)flag, g->kept.p, n_sel, n_lib, st));
    uint32_t K32 = 0;
    HIP_TRY(hipMemcpyAsync(&K32, n_sel, 4, hipMemcpyDeviceToHost, st));
    ADH_TRY(t.end(st, g->filter_ms));
    const int64_t K = K32;
    if (K > n_lib) return fail(ADH_ERR_HIP, "adh_mbr_filter: inconsistent number of kept precursors");
    if (K == 0) {
        g->n_kept = 0;
        return ADH_OK;
    }

    // the kept blocks by ascending old start, renumbered (as adh_tl_update does)
    uint32_t *ks_in = nullptr, *ks = nullptr, *pos_in = nullptr, *ord = nullptr;
    int64_t *len = nullptr, *new_start = nullptr;
    HIP_TRY(B.alloc(&ks_in, (size_t)K));
    HIP_TRY(B.alloc(&ks, (size_t)K));
    HIP_TRY(B.alloc(&pos_in, (size_t)K));
    HIP_TRY(B.alloc(&ord, (size_t)K));
    HIP_TRY(B.alloc(&len, (size_t)K));
    HIP_TRY(B.alloc(&new_start, (size_t)K));
    HIP_TRY(g->start.reserve((size_t)K));
    HIP_TRY(g->stop.reserve((size_t)K));
    ADH_TRY(t.begin(st));
    hipLaunchKernelGGL(tl::kept_start_kernel, dim3(mbr::grid_for(K)), dim3(mbr::kBlock), 0, st, (const uint32_t *)g->kept.p,
                       (const int64_t *)start, K, ks_in, pos_in);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, ks_in, ks, pos_in, ord, K, 32, st));
    hipLaunchKernelGGL(tl::block_len_kernel, dim3(mbr::grid_for(K)), dim3(mbr::kBlock), 0, st, (const uint32_t *)g->kept.p,
                       (const uint32_t *)ord, (const int64_t *)start, (const int64_t *)stop, K, len);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::exclusive_sum(B, len, new_start, K, st));
    int64_t last[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&last[0], new_start + (K - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last[1], len + (K - 1), 8, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(mbr::renumber_kernel, dim3(mbr::grid_for(K)), dim3(mbr::kBlock), 0, st, (const uint32_t *)ord,
                       (const int64_t *)new_start, (const int64_t *)len, K, g->start.p, g->stop.p);
    HIP_TRY(hipGetLastError());
    ADH_TRY(t.end(st, g->filter_ms));
    g->d2h_bytes += 20;
    const int64_t Rn = last[0] + last[1];
    if (Rn < 0 || Rn >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_mbr_filter: the kept fragment rows number 2^31 or more");
    HIP_TRY(g->src_row.reserve((size_t)Rn));
    for (int m = 0; m < M; ++m) HIP_TRY(g->mat[m].reserve((size_t)Rn * C));
    if (Rn > 0) {
        ADH_TRY(t.begin(st));
        hipLaunchKernelGGL(tl::row_map_kernel, dim3(mbr::grid_for(Rn)), dim3(mbr::kBlock), 0, st, (const int64_t *)new_start,
                           (const uint32_t *)ks, K, Rn, g->src_row.p);
        HIP_TRY(hipGetLastError());
        for (int m = 0; m < M; ++m) {
            if (C % 4 == 0) {
                const int32_t Q = C / 4;
                int32_t shift = 0;
                while ((1 << shift) < Q && shift < 6) ++shift;
                hipLaunchKernelGGL(mbr::row_gather4_kernel, dim3(mbr::grid_for(Rn << shift)), dim3(mbr::kBlock), 0, st,
                                   (const float4 *)src[m], (const uint32_t *)g->src_row.p, Rn, Q, shift, (float4 *)g->mat[m].p);
            } else {  // rows that are no multiple of 16 bytes: adh_tl_update's gather, all rows from one source
                hipLaunchKernelGGL(tl::row_gather_kernel, dim3(mbr::grid_for(Rn * C)), dim3(mbr::kBlock), 0, st, src[m],
                                   (const float *)nullptr, (const uint32_t *)g->src_row.p, (int64_t)0x7FFFFFFFFFFFFFFFll, Rn * C, C,
                                   g->mat[m].p);
            }
            HIP_TRY(hipGetLastError());
        }
        ADH_TRY(t.end(st, g->gather_ms));
    }
    HIP_TRY(hipStreamSynchronize(st));
    g->n_kept = K, g->n_rows = Rn;
    *n_kept = K;
    *n_kept_rows = Rn;
    return ADH_OK;
}

int adh_mbr_read_filter(adh_mbr_t *g, int64_t *kept, int64_t *frag_start, int64_t *frag_stop, int64_t *source_row) {
    if (!g || !kept || !frag_start || !frag_stop) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->n_kept < 1) return fail(ADH_ERR_NOT_STAGED, "adh_mbr_read_filter: no kept precursors");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    const size_t K = (size_t)g->n_kept, R = source_row ? (size_t)g->n_rows : 0;
    std::vector<uint32_t> k32(K), r32(R);
    HIP_TRY(hipMemcpyAsync(k32.data(), g->kept, K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(frag_start, g->start, K * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(frag_stop, g->stop, K * 8, hipMemcpyDeviceToHost, st));
    if (R) HIP_TRY(hipMemcpyAsync(r32.data(), g->src_row, R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < K; ++j) kept[j] = (int64_t)k32[j];
    for (size_t r = 0; r < R; ++r) source_row[r] = (int64_t)r32[r];
    g->d2h_bytes += K * 20 + R * 4;
    return ADH_OK;
}

int adh_mbr_read_matrix(adh_mbr_t *g, int32_t m, float *out) {
    if (!g || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m < 0 || m >= g->M) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_read_matrix: no such matrix");
    if (g->n_kept < 1) return fail(ADH_ERR_NOT_STAGED, "adh_mbr_read_matrix: no kept precursors");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    const size_t bytes = (size_t)g->n_rows * g->C * 4;
    if (bytes) HIP_TRY(hipMemcpyAsync(out, g->mat[m], bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->d2h_bytes += bytes;
    return ADH_OK;
}

int adh_mbr_assign(adh_mbr_t *g, int64_t n, const void *elution_group_idx, int32_t group_is_u32, const void *mod_seq_charge_hash,
                   int32_t hash_is_signed, void *rt, int64_t *pg_row, int64_t *n_missing) {
    if (!g || !n_missing || (n > 0 && (!elution_group_idx || !mod_seq_charge_hash || !rt || !pg_row)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (g->n_groups < 0) return fail(ADH_ERR_NOT_STAGED, "adh_mbr_assign: no aggregate");
    if (n < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_assign: negative size");
    if (n >= (int64_t)0x7FFFFFF0ll) return fail(ADH_ERR_UNSUPPORTED, "adh_mbr_assign: 2^31 rows and more are not supported");
    if ((hash_is_signed ? 1 : 0) != g->hash_signed)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_assign: mod_seq_charge_hash differs in dtype from the aggregate's");
    g->assign_ms = 0.0;
    *n_missing = 0;
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    const size_t gb = group_is_u32 ? 4 : 8, rb = g->rt_is_f64 ? 8 : 4;
    sess::DevBufs B;
    unsigned char *d_eg = nullptr, *d_hash = nullptr, *d_rt = nullptr;
    int64_t *d_row = nullptr;
    uint32_t *d_missing = nullptr;
    HIP_TRY(B.upload(&d_eg, elution_group_idx, (size_t)n * gb, st));
    HIP_TRY(B.upload(&d_hash, mod_seq_charge_hash, (size_t)n * 8, st));
    HIP_TRY(B.alloc(&d_rt, (size_t)n * rb));
    HIP_TRY(B.alloc(&d_row, (size_t)n));
    HIP_TRY(B.alloc(&d_missing, 4));
    g->h2d_bytes += (uint64_t)n * (gb + 8);
    sess::EventPair &t = g->ev;
    ADH_TRY(t.begin(st));
    HIP_TRY(hipMemsetAsync(d_missing, 0, 4, st));
    hipLaunchKernelGGL(mbr::assign_kernel, dim3(mbr::grid_for(n)), dim3(mbr::kBlock), 0, st, (const void *)d_eg,
                       mbr::key_kind(group_is_u32), (const void *)d_hash, mbr::hash_kind(hash_is_signed), n,
                       (const uint64_t *)g->key[0].p, (const double *)g->med[0].p, (const uint32_t *)g->first[0].p, g->n_seg[0],
                       (const uint64_t *)g->key[1].p, (const double *)g->med[1].p, (const uint32_t *)g->first[1].p, g->n_seg[1],
                       g->rt_is_f64, (void *)d_rt, d_row, d_missing);
    HIP_TRY(hipGetLastError());
    ADH_TRY(t.end(st, g->assign_ms));
    uint32_t missing = 0;
    HIP_TRY(hipMemcpyAsync(rt, d_rt, (size_t)n * rb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pg_row, d_row, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&missing, d_missing, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->d2h_bytes += (uint64_t)n * (rb + 8) + 4;
    *n_missing = missing;
    return ADH_OK;
}

int adh_mbr_index(adh_mbr_t *g, int64_t n_targets, const uint64_t *target_keys, int64_t n_lookup, const uint64_t *lookup_keys,
                  int64_t *index, int32_t *duplicate) {
    if (!g || !duplicate || (n_targets > 0 && (!target_keys || !index)) || (n_lookup > 0 && !lookup_keys))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_targets < 0 || n_lookup < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_index: negative size");
    if (n_targets >= (int64_t)0x7FFFFFF0ll || n_lookup >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_mbr_index: 2^31 keys and more are not supported");
    *duplicate = 0;
    if (n_lookup == 0 || n_targets == 0) {
        for (int64_t i = 0; i < n_targets; ++i) index[i] = -1;
        if (n_lookup == 0) return ADH_OK;
    }
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    sess::DevBufs B;
    uint64_t *d_t = nullptr, *d_l = nullptr, *sorted = nullptr;
    uint32_t *iota = nullptr, *pos = nullptr;
    int64_t *d_out = nullptr;
    int32_t *d_dup = nullptr;
    HIP_TRY(B.upload(&d_t, target_keys, (size_t)n_targets, st));
    HIP_TRY(B.upload(&d_l, lookup_keys, (size_t)n_lookup, st));
    HIP_TRY(B.alloc(&sorted, (size_t)n_lookup));
    HIP_TRY(B.alloc(&iota, (size_t)n_lookup));
    HIP_TRY(B.alloc(&pos, (size_t)n_lookup));
    HIP_TRY(B.alloc(&d_out, (size_t)n_targets));
    HIP_TRY(B.alloc(&d_dup, 4));
    g->h2d_bytes += (uint64_t)(n_targets + n_lookup) * 8;
    HIP_TRY(hipMemsetAsync(d_dup, 0, 4, st));
    hipLaunchKernelGGL(sess::iota_kernel, dim3(mbr::grid_for(n_lookup)), dim3(mbr::kBlock), 0, st, iota, n_lookup);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::sort_pairs(B, (const uint64_t *)d_l, sorted, (const uint32_t *)iota, pos, n_lookup, 64, st));
    hipLaunchKernelGGL(mbr::adjacent_equal_kernel, dim3(mbr::grid_for(n_lookup)), dim3(mbr::kBlock), 0, st, (const uint64_t *)sorted,
                       n_lookup, d_dup);
    HIP_TRY(hipGetLastError());
    if (n_targets > 0) {
        hipLaunchKernelGGL(mbr::index_kernel, dim3(mbr::grid_for(n_targets)), dim3(mbr::kBlock), 0, st, (const uint64_t *)d_t, n_targets,
                           (const uint64_t *)sorted, (const uint32_t *)pos, n_lookup, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(index, d_out, (size_t)n_targets * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(duplicate, d_dup, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->d2h_bytes += (uint64_t)n_targets * 8 + 4;
    return ADH_OK;
}

// host only, no Python call per element: 0 where an entry of a 1-d object array is `none`, 1 where its type is
// `str_type`, 2 elsewhere (*n_other of them: the caller asks pandas about those).  Reads the type word behind the
// reference count - the object layout runtime.py probes before it calls this.
int adh_mbr_notnull_objects(void *const *items, int64_t n, const void *none, const void *str_type, uint8_t *out, int64_t *n_other) {
    if (!n_other || (n > 0 && (!items || !out)) || !none || !str_type) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    int64_t other = 0;
    for (int64_t i = 0; i < n; ++i) {
        const void *p = items[i];
        if (!p) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_mbr_notnull_objects: an empty slot");
        if (p == none) {
            out[i] = 0;
        } else if (static_cast<const void *const *>(p)[1] == str_type) {
            out[i] = 1;
        } else {
            out[i] = 2;
            ++other;
        }
    }
    *n_other = other;
    return ADH_OK;
}

int adh_mbr_stats(adh_mbr_t *g, double *aggregate_ms, double *filter_ms, double *gather_ms, double *assign_ms, uint64_t *h2d_bytes,
                  uint64_t *d2h_bytes) {
    if (!g || !aggregate_ms || !filter_ms || !gather_ms || !assign_ms || !h2d_bytes || !d2h_bytes)
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *aggregate_ms = g->aggregate_ms;
    *filter_ms = g->filter_ms;
    *gather_ms = g->gather_ms;
    *assign_ms = g->assign_ms;
    *h2d_bytes = g->h2d_bytes;
    *d2h_bytes = g->d2h_bytes;
    return ADH_OK;
}

}  // extern "C"
