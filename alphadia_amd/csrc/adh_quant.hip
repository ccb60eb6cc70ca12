// adh_quant.hip - the cross-run fragment quantity matrices of label-free quantification on the device.
//
// After the last raw file the reference builds, per quantity column, one frame over all runs
// (FragmentQuantLoader.accumulate, outputtransform/quantification/fragment_accumulator.py:51-101): per run the frag
// rows of PSM precursors get an ion key (quant_builder.py:52-81), an outer merge on (ion, precursor_idx) adds the
// run as a column, fillna(0) fills the gaps.  QuantBuilder.filter_frag_df (quant_builder.py:132-182) then keeps, per
// group, the top-N fragments by their mean correlation over the runs plus those above a threshold.
//
// Here the kept rows of every run are appended in HBM (adh_quant_add_run), one stable radix sort of the ion keys
// gives the union and each row's place in it, and the quantity columns are scattered into zero-filled column-major
// n_keys x n_runs matrices (adh_quant_build).  The matrices stay on the device: the host copies the ones it needs
// (adh_quant_matrix), and every filter call (adh_quant_filter) reads the quality matrix in place - a row mean in the
// order NumPy takes it, a radix sort by (group, mean descending, row), a rank per group, the mask.
// Included by adh_api.hip behind adh_session.h (shares its error helpers, the handle and the session helpers).

struct adh_quant {
    // scratch that grows with the largest run or filter seen: sized in bytes with an eighth of slack
    using Scratch = sess::DevArray<unsigned char, sess::eighth_slack>;
    adh_handle_t *h = nullptr;
    int32_t n_cols = 0;
    sess::DevArray<uint32_t, sess::as_asked> psm;  // sorted distinct precursor_idx of the PSMs
    int64_t n_psm = 0;
    // kept rows of all runs in run order: ion key, precursor_idx, run, then n_cols value columns of cap rows each
    int64_t n_rows = 0, cap = 0;
    sess::DevArray<int64_t> ion;
    sess::DevArray<uint32_t> pidx, run;
    sess::DevArray<float> val;
    int32_t n_runs = 0;
    // one run's input columns and its row flags / offsets (u32)
    Scratch in, off;
    // the built union: keys, matrices (n_cols x n_runs columns of n_keys), filter scratch
    bool built = false, duplicate = false;
    int64_t n_keys = 0;
    sess::DevArray<int64_t, sess::as_asked> key_ion;  // (built once, with at least one key: the exact size)
    sess::DevArray<uint32_t, sess::as_asked> key_pidx;
    sess::DevArray<float, sess::as_asked> mat;
    Scratch work, tmp;  // tmp: hipCUB temporary storage
    sess::DevArray<uint32_t> flag;  // one u32 on the device: a run holds a key twice
    sess::EventPair ev;
    double build_ms = 0.0, filter_ms = 0.0;
    std::shared_ptr<void> lfq;  // the state of label-free quantification over these matrices (adh_lfq.hip)
};

namespace quant {

using sess::grid_for;
using sess::kBlock;
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;

__host__ __device__ inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// the ion key (quant_builder.py:52-81) in int64: precursor_idx + number << 32 + type << 40 + charge << 48 +
// loss_type << 56, wrapping as Numba's int64 arithmetic does
__device__ __forceinline__ int64_t ion_key(uint32_t p, uint8_t number, uint8_t type, uint8_t charge, uint8_t loss) {
    return (int64_t)((uint64_t)p + ((uint64_t)number << 32) + ((uint64_t)type << 40) + ((uint64_t)charge << 48) +
                     ((uint64_t)loss << 56));
}

__device__ __forceinline__ bool is_psm(const uint32_t *__restrict__ psm, int64_t n_psm, uint32_t p) {
    int64_t lo = 0, hi = n_psm;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (psm[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_psm && psm[lo] == p;
}

// flag[i] = row i's precursor is among the PSMs; flag[n] = 0 (an exclusive scan turns this into offsets and a count)
__global__ void __launch_bounds__(kBlock) member_kernel(const uint32_t *__restrict__ pidx, int64_t n,
                                                        const uint32_t *__restrict__ psm, int64_t n_psm,
                                                        uint32_t *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride)
        flag[i] = i < n ? (uint32_t)is_psm(psm, n_psm, pidx[i]) : 0u;
}

// the kept rows of one run appended at `base`: key, precursor, run, values (NaN kept: the duplicate-key path on the
// host needs the rows as they came)
__global__ void __launch_bounds__(kBlock) append_kernel(const unsigned char *__restrict__ in, int64_t n, int n_cols,
                                                        const uint32_t *__restrict__ off, int64_t base, uint32_t run_id,
                                                        int64_t *__restrict__ ion, uint32_t *__restrict__ pidx_out,
                                                        uint32_t *__restrict__ run, float *__restrict__ val, int64_t cap) {
    const size_t b4 = align16((size_t)n * 4), b1 = align16((size_t)n);
    const uint32_t *p = reinterpret_cast<const uint32_t *>(in);
    const uint8_t *number = in + b4, *type = number + b1, *charge = type + b1, *loss = charge + b1;
    const float *cols = reinterpret_cast<const float *>(loss + b1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t o = off[i];
        if (off[i + 1] == o) continue;
        const int64_t j = base + (int64_t)o;
        const uint32_t pi = p[i];
        ion[j] = ion_key(pi, number[i], type[i], charge[i], loss[i]);
        pidx_out[j] = pi;
        run[j] = run_id;
        for (int c = 0; c < n_cols; ++c) val[(size_t)c * (size_t)cap + (size_t)j] = cols[(size_t)c * b4 / 4 + (size_t)i];
    }
}

// head[i] = the sorted key at i starts a new key; a key repeated inside one run raises the flag (the reference's
// merge makes a cartesian product of it; the host takes that case)
__global__ void __launch_bounds__(kBlock) head_kernel(const int64_t *__restrict__ key, const uint32_t *__restrict__ perm,
                                                      const uint32_t *__restrict__ run, int64_t n,
                                                      uint32_t *__restrict__ head, uint32_t *__restrict__ dup) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const bool h = i == 0 || key[i] != key[i - 1];
        head[i] = h;
        if (!h && run[perm[i]] == run[perm[i - 1]]) *dup = 1u;
    }
}

// keys of the union (kid: inclusive scan of the heads, 1-based) and every row's values into the matrices
__global__ void __launch_bounds__(kBlock) scatter_kernel(const int64_t *__restrict__ key, const uint32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ kid, int64_t n,
                                                         const uint32_t *__restrict__ pidx, const uint32_t *__restrict__ run,
                                                         const float *__restrict__ val, int64_t cap, int n_cols,
                                                         int64_t n_keys, int n_runs, int64_t *__restrict__ key_ion,
                                                         uint32_t *__restrict__ key_pidx, float *__restrict__ mat) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const size_t plane = (size_t)n_keys * (size_t)n_runs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t row = perm[i];
        const int64_t k = (int64_t)kid[i] - 1;
        if (i == 0 || kid[i - 1] != kid[i]) {
            key_ion[k] = key[i];
            key_pidx[k] = pidx[row];
        }
        const size_t at = (size_t)run[row] * (size_t)n_keys + (size_t)k;
        for (int c = 0; c < n_cols; ++c) {
            const float v = val[(size_t)c * (size_t)cap + row];
            mat[(size_t)c * plane + at] = v != v ? 0.0f : v;  // fillna(0)
        }
    }
}

// one run: the frame is the run's kept rows in their order (no merge takes place)
__global__ void __launch_bounds__(kBlock) single_kernel(const int64_t *__restrict__ ion, const uint32_t *__restrict__ pidx,
                                                        const float *__restrict__ val, int64_t cap, int64_t n, int n_cols,
                                                        int64_t *__restrict__ key_ion, uint32_t *__restrict__ key_pidx,
                                                        float *__restrict__ mat) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        key_ion[i] = ion[i];
        key_pidx[i] = pidx[i];
        for (int c = 0; c < n_cols; ++c) {
            const float v = val[(size_t)c * (size_t)cap + (size_t)i];
            mat[(size_t)c * (size_t)n + (size_t)i] = v != v ? 0.0f : v;
        }
    }
}

// total = np.mean(quality_df[run_columns].values, axis=1): the frame's values are an F-ordered float32 array, which
// NumPy reduces along the strided axis one column after the other into a float32 accumulator that starts as the
// first column, then divides by the run count in float32.  The sort key: group in the high half, the total mapped so
// that ascending order is descending total (NaN last, -0 as +0) in the low half.
__global__ void __launch_bounds__(kBlock) total_kernel(const float *__restrict__ m, int64_t n_keys, int n_runs,
                                                       const int32_t *__restrict__ group, float *__restrict__ total,
                                                       uint64_t *__restrict__ sort_key, uint32_t *__restrict__ sort_row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride) {
        float s = m[i];
        for (int r = 1; r < n_runs; ++r) s += m[(size_t)r * (size_t)n_keys + (size_t)i];
        const float t = s / (float)n_runs;
        total[i] = t;
        uint32_t d;
        if (t != t) {
            d = 0xFFFFFFFFu;
        } else {
            const uint32_t u = __float_as_uint(t == 0.0f ? 0.0f : t);
            d = ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
        }
        const int32_t g = group[i];
        sort_key[i] = ((uint64_t)(g < 0 ? kNoGroup : (uint32_t)g) << 32) | d;
        sort_row[i] = (uint32_t)i;
    }
}

// first sorted position of every group
__global__ void __launch_bounds__(kBlock) first_kernel(const uint64_t *__restrict__ key, int64_t n,
                                                       uint32_t *__restrict__ first) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint32_t g = (uint32_t)(key[p] >> 32);
        if (g != kNoGroup && (p == 0 || (uint32_t)(key[p - 1] >> 32) != g)) first[g] = (uint32_t)p;
    }
}

// rank(ascending=False, method="first") inside the group - NaN for a NaN total or a missing group, as pandas leaves
// them - and the mask rank <= top_n | total > threshold
__global__ void __launch_bounds__(kBlock) rank_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ row,
                                                      int64_t n, const uint32_t *__restrict__ first,
                                                      const float *__restrict__ total, double top_n, double threshold,
                                                      double *__restrict__ rank, uint8_t *__restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint64_t k = key[p];
        const uint32_t g = (uint32_t)(k >> 32), i = row[p];
        const float t = total[i];
        const double r = (g == kNoGroup || t != t) ? __longlong_as_double(0x7FF8000000000000ll)
                                                   : (double)((uint32_t)p - first[g] + 1u);
        rank[i] = r;
        mask[i] = (uint8_t)((r <= top_n) || ((double)t > threshold));
    }
}

// the appended row buffers grown to hold `need` rows, the rows so far kept
int grow_rows(adh_quant *q, int64_t need) {
    if (need <= q->cap) return ADH_OK;
    const int64_t cap = std::max<int64_t>(need, q->cap + q->cap / 2 + 4096);
    hipStream_t st = q->h->stream;
    sess::DevArray<int64_t> ion;
    sess::DevArray<uint32_t> pidx, run;
    sess::DevArray<float> val;
    hipError_t e = ion.reserve((size_t)cap);
    if (e == hipSuccess) e = pidx.reserve((size_t)cap);
    if (e == hipSuccess) e = run.reserve((size_t)cap);
    if (e == hipSuccess) e = val.reserve((size_t)cap * (size_t)std::max(q->n_cols, 1));
    if (e == hipSuccess && q->n_rows > 0) {
        const size_t r = (size_t)q->n_rows;
        e = hipMemcpyAsync(ion.p, q->ion.p, r * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pidx.p, q->pidx.p, r * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(run.p, q->run.p, r * 4, hipMemcpyDeviceToDevice, st);
        for (int c = 0; c < q->n_cols && e == hipSuccess; ++c)
            e = hipMemcpyAsync(val.p + (size_t)c * (size_t)cap, q->val.p + (size_t)c * (size_t)q->cap, r * 4,
                               hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? ADH_ERR_OUT_OF_MEMORY : ADH_ERR_HIP,
                    std::string("adh_quant_add_run: row buffers: ") + hipGetErrorString(e));
    }
    // (the old buffers leave with the locals)
    q->ion.swap(ion), q->pidx.swap(pidx), q->run.swap(run), q->val.swap(val), q->cap = cap;
    return ADH_OK;
}

}  // namespace quant

extern "C" {

int adh_quant_create(adh_handle_t *h, int32_t n_columns, const uint32_t *psm_precursor_idx, int64_t n_psm,
                     adh_quant_t **out) {
    if (!h || !out || (n_psm > 0 && !psm_precursor_idx)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_columns < 1 || n_columns > ADH_QUANT_MAX_COLUMNS || n_psm < 0)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_create: 1 .. ADH_QUANT_MAX_COLUMNS quantity columns");
    for (int64_t i = 1; i < n_psm; ++i)
        if (psm_precursor_idx[i] <= psm_precursor_idx[i - 1])
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_create: PSM precursors must be sorted and distinct");
    HIP_TRY(hipSetDevice(h->device));
    adh_quant *q = new adh_quant();
    q->h = h;
    q->n_cols = n_columns;
    q->n_psm = n_psm;
    hipError_t e = q->psm.reserve((size_t)std::max<int64_t>(n_psm, 1));
    if (e == hipSuccess && n_psm > 0)
        e = hipMemcpyAsync(q->psm.p, psm_precursor_idx, (size_t)n_psm * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = q->flag.reserve(4);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        adh_quant_destroy(q);
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? ADH_ERR_OUT_OF_MEMORY : ADH_ERR_HIP,
                    std::string("adh_quant_create: ") + hipGetErrorString(e));
    }
    *out = q;
    return ADH_OK;
}

int adh_quant_destroy(adh_quant_t *q) {
    if (!q) return ADH_OK;
    (void)hipSetDevice(q->h->device);
    (void)hipStreamSynchronize(q->h->stream);
    delete q;  // (the members free their device memory and events)
    return ADH_OK;
}

int adh_quant_add_run(adh_quant_t *q, int64_t n, const uint32_t *precursor_idx, const uint8_t *number,
                      const uint8_t *type, const uint8_t *charge, const uint8_t *loss_type, const float *const *columns,
                      int64_t *n_kept) {
    if (!q || !n_kept || (n > 0 && (!precursor_idx || !number || !type || !charge || !loss_type || !columns)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_add_run: negative row count");
    if (q->built) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_add_run: the matrices are already built");
    if (q->n_runs >= 0xFFFFFF) return fail(ADH_ERR_UNSUPPORTED, "adh_quant_add_run: too many runs");
    for (int c = 0; c < q->n_cols && n > 0; ++c)
        if (!columns[c]) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_add_run: a quantity column is NULL");
    if (q->n_rows + n >= (int64_t)0xFFFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_quant_add_run: more than 2^32 fragment rows over all runs");
    *n_kept = 0;
    const uint32_t run_id = (uint32_t)q->n_runs++;
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    using quant::align16;
    const size_t b4 = align16((size_t)n * 4), b1 = align16((size_t)n);
    HIP_TRY(q->in.reserve(b4 + 4 * b1 + (size_t)q->n_cols * b4));
    HIP_TRY(q->off.reserve((size_t)(n + 1) * 4));
    unsigned char *in = q->in.p;
    uint32_t *off = reinterpret_cast<uint32_t *>(q->off.p);
    HIP_TRY(hipMemcpyAsync(in, precursor_idx, (size_t)n * 4, hipMemcpyHostToDevice, st));
    const uint8_t *bytes[4] = {number, type, charge, loss_type};
    for (int j = 0; j < 4; ++j)
        HIP_TRY(hipMemcpyAsync(in + b4 + (size_t)j * b1, bytes[j], (size_t)n, hipMemcpyHostToDevice, st));
    for (int c = 0; c < q->n_cols; ++c)
        HIP_TRY(hipMemcpyAsync(in + b4 + 4 * b1 + (size_t)c * b4, columns[c], (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(quant::member_kernel, dim3(quant::grid_for(n + 1)), dim3(quant::kBlock), 0, st,
                       reinterpret_cast<const uint32_t *>(in), n, q->psm.p, q->n_psm, off);
    HIP_TRY(hipGetLastError());
    ADH_TRY(sess::exclusive_sum(q->tmp, off, off, n + 1, st));
    uint32_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, off + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int rc = quant::grow_rows(q, q->n_rows + (int64_t)kept);
    if (rc != ADH_OK) return rc;
    if (kept > 0) {
        hipLaunchKernelGGL(quant::append_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, in, n, q->n_cols,
                           off, q->n_rows, run_id, q->ion.p, q->pidx.p, q->run.p, q->val.p, q->cap);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));  // (the next run reuses the input buffer)
    }
    q->n_rows += kept;
    *n_kept = kept;
    return ADH_OK;
}

int adh_quant_build(adh_quant_t *q, int64_t *n_keys, int32_t *duplicate) {
    if (!q || !n_keys || !duplicate) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (q->built) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_build: already built");
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    const int64_t n = q->n_rows;
    const int R = q->n_runs;
    int64_t keys = 0;
    bool dup = false;
    q->build_ms = 0.0;
    const int rc = sess::timed(q->ev, st, q->build_ms, [&]() -> int {
        if (n == 0) return ADH_OK;
        if (R == 1) {
            keys = n;
        } else {
            // work: sorted keys [n] i64 | perm in [n] u32 | perm [n] u32 | key id [n] u32
            const size_t wb = quant::align16((size_t)n * 8) + 3 * quant::align16((size_t)n * 4);
            HIP_TRY(q->work.reserve(wb));
            unsigned char *w = q->work.p;
            int64_t *skey = reinterpret_cast<int64_t *>(w);
            uint32_t *perm_in = reinterpret_cast<uint32_t *>(w + quant::align16((size_t)n * 8));
            uint32_t *perm = perm_in + quant::align16((size_t)n * 4) / 4;
            uint32_t *kid = perm + quant::align16((size_t)n * 4) / 4;
            hipLaunchKernelGGL(sess::iota_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, perm_in, n);
            HIP_TRY(hipGetLastError());
            // one block for the sort and the scan
            sess::TmpSize both;
            ADH_TRY(sess::sort_pairs(both, q->ion.p, skey, perm_in, perm, n, 64, st));
            ADH_TRY(sess::inclusive_sum(both, kid, kid, n, st));
            HIP_TRY(q->tmp.reserve(both.bytes));
            // stable: rows of one key stay in run order
            ADH_TRY(sess::sort_pairs(q->tmp, q->ion.p, skey, perm_in, perm, n, 64, st));
            HIP_TRY(hipMemsetAsync(q->flag, 0, 4, st));
            hipLaunchKernelGGL(quant::head_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, skey, perm, q->run.p,
                               n, kid, q->flag.p);
            HIP_TRY(hipGetLastError());
            ADH_TRY(sess::inclusive_sum(q->tmp, kid, kid, n, st));
            uint32_t hk[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(&hk[0], kid + n - 1, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&hk[1], q->flag, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            keys = hk[0];
            dup = hk[1] != 0;
            if (dup) return ADH_OK;  // (the host merges these rows itself)
        }
        const size_t plane = (size_t)keys * (size_t)R * (size_t)q->n_cols;
        HIP_TRY(q->key_ion.reserve((size_t)keys));
        HIP_TRY(q->key_pidx.reserve((size_t)keys));
        HIP_TRY(q->mat.reserve(plane));
        if (R == 1) {
            hipLaunchKernelGGL(quant::single_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, q->ion.p, q->pidx.p,
                               q->val.p, q->cap, n, q->n_cols, q->key_ion.p, q->key_pidx.p, q->mat.p);
        } else {
            HIP_TRY(hipMemsetAsync(q->mat, 0, plane * 4, st));
            unsigned char *w = q->work.p;
            const int64_t *skey = reinterpret_cast<const int64_t *>(w);
            const uint32_t *perm = reinterpret_cast<const uint32_t *>(w + quant::align16((size_t)n * 8)) +
                                   quant::align16((size_t)n * 4) / 4;
            const uint32_t *kid = perm + quant::align16((size_t)n * 4) / 4;
            hipLaunchKernelGGL(quant::scatter_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, skey, perm, kid,
                               n, q->pidx.p, q->run.p, q->val.p, q->cap, q->n_cols, keys, R, q->key_ion.p, q->key_pidx.p,
                               q->mat.p);
        }
        HIP_TRY(hipGetLastError());
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    q->built = true;
    q->duplicate = dup;
    q->n_keys = dup ? 0 : keys;
    *n_keys = q->n_keys;
    *duplicate = dup;
    return ADH_OK;
}

int adh_quant_keys(adh_quant_t *q, int64_t *ion, uint32_t *precursor_idx) {
    if (!q || (q->n_keys > 0 && (!ion || !precursor_idx))) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!q->built) return fail(ADH_ERR_NOT_STAGED, "adh_quant_keys: no built matrices");
    if (q->n_keys == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    HIP_TRY(hipMemcpyAsync(ion, q->key_ion.p, (size_t)q->n_keys * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(precursor_idx, q->key_pidx.p, (size_t)q->n_keys * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    q->h->d2h_bytes += (uint64_t)q->n_keys * 12;
    return ADH_OK;
}

int adh_quant_matrix(adh_quant_t *q, int32_t column, float *out) {
    if (!q || (q->n_keys > 0 && !out)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!q->built) return fail(ADH_ERR_NOT_STAGED, "adh_quant_matrix: no built matrices");
    if (column < 0 || column >= q->n_cols) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_matrix: column out of range");
    if (q->n_keys == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(q->h->device));
    const size_t plane = (size_t)q->n_keys * (size_t)q->n_runs;
    HIP_TRY(hipMemcpyAsync(out, q->mat.p + (size_t)column * plane, plane * 4, hipMemcpyDeviceToHost, q->h->stream));
    HIP_TRY(hipStreamSynchronize(q->h->stream));
    q->h->d2h_bytes += plane * 4;
    return ADH_OK;
}

int adh_quant_rows(adh_quant_t *q, int64_t *ion, uint32_t *precursor_idx, uint32_t *run, float *const *columns) {
    if (!q || (q->n_rows > 0 && (!ion || !precursor_idx || !run || !columns)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (q->n_rows == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    const size_t r = (size_t)q->n_rows;
    HIP_TRY(hipMemcpyAsync(ion, q->ion.p, r * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(precursor_idx, q->pidx.p, r * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(run, q->run.p, r * 4, hipMemcpyDeviceToHost, st));
    for (int c = 0; c < q->n_cols; ++c) {
        if (!columns[c]) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_rows: a quantity column is NULL");
        HIP_TRY(hipMemcpyAsync(columns[c], q->val.p + (size_t)c * (size_t)q->cap, r * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    q->h->d2h_bytes += r * (16 + 4 * (size_t)q->n_cols);
    return ADH_OK;
}

int adh_quant_set_matrix(adh_quant_t *q, int64_t n_keys, int32_t n_runs, const float *const *run_columns) {
    if (!q || (n_keys > 0 && n_runs > 0 && !run_columns)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (q->built || q->n_rows > 0 || q->n_cols != 1)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_set_matrix: needs a fresh object of one column");
    if (n_keys < 0 || n_runs < 1 || n_keys >= (int64_t)0xFFFFFFF0ll)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_set_matrix: 0 .. 2^32 rows and at least one run column");
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    q->n_runs = n_runs;
    q->n_keys = n_keys;
    if (n_keys > 0) {
        HIP_TRY(q->mat.reserve((size_t)n_keys * (size_t)n_runs));
        for (int r = 0; r < n_runs; ++r) {
            if (!run_columns[r]) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_set_matrix: a run column is NULL");
            HIP_TRY(hipMemcpyAsync(q->mat.p + (size_t)r * (size_t)n_keys, run_columns[r], (size_t)n_keys * 4,
                                   hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    q->built = true;
    return ADH_OK;
}

int adh_quant_filter(adh_quant_t *q, int32_t column, const int32_t *group, int32_t n_groups, double top_n,
                     double threshold, float *total, double *rank, uint8_t *mask) {
    if (!q || (q->n_keys > 0 && (!group || !total || !rank || !mask))) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!q->built || q->duplicate) return fail(ADH_ERR_NOT_STAGED, "adh_quant_filter: no built matrices");
    if (column < 0 || column >= q->n_cols) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_filter: column out of range");
    if (n_groups < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_filter: negative group count");
    const int64_t n = q->n_keys;
    for (int64_t i = 0; i < n; ++i)
        if (group[i] >= n_groups) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_quant_filter: group code >= n_groups");
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    using quant::align16;
    // work: group [n] i32 | total [n] f32 | key in / out [n] u64 | row in / out [n] u32 | first [n_groups] u32 |
    //       rank [n] f64 | mask [n] u8
    const size_t o_total = align16((size_t)n * 4), o_kin = o_total + align16((size_t)n * 4),
                 o_kout = o_kin + align16((size_t)n * 8), o_rin = o_kout + align16((size_t)n * 8),
                 o_rout = o_rin + align16((size_t)n * 4), o_first = o_rout + align16((size_t)n * 4),
                 o_rank = o_first + align16((size_t)std::max(n_groups, 1) * 4), o_mask = o_rank + align16((size_t)n * 8),
                 wb = o_mask + align16((size_t)n);
    HIP_TRY(q->work.reserve(wb));
    unsigned char *w = q->work.p;
    int32_t *d_group = reinterpret_cast<int32_t *>(w);
    float *d_total = reinterpret_cast<float *>(w + o_total);
    uint64_t *kin = reinterpret_cast<uint64_t *>(w + o_kin), *kout = reinterpret_cast<uint64_t *>(w + o_kout);
    uint32_t *rin = reinterpret_cast<uint32_t *>(w + o_rin), *rout = reinterpret_cast<uint32_t *>(w + o_rout);
    uint32_t *first = reinterpret_cast<uint32_t *>(w + o_first);
    double *d_rank = reinterpret_cast<double *>(w + o_rank);
    uint8_t *d_mask = w + o_mask;
    // (the sort's temporary storage is in place before the timed part)
    sess::TmpSize sort;
    ADH_TRY(sess::sort_pairs(sort, kin, kout, rin, rout, n, 64, st));
    HIP_TRY(q->tmp.reserve(sort.bytes));
    HIP_TRY(hipMemcpyAsync(d_group, group, (size_t)n * 4, hipMemcpyHostToDevice, st));
    const int32_t R = q->n_runs;
    const float *m = q->mat.p + (size_t)column * (size_t)n * (size_t)R;
    q->filter_ms = 0.0;
    int rc = sess::timed(q->ev, st, q->filter_ms, [&]() -> int {
        hipLaunchKernelGGL(quant::total_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, m, n, R, d_group,
                           d_total, kin, rin);
        HIP_TRY(hipGetLastError());
        // stable: ties keep the row order (method="first")
        ADH_TRY(sess::sort_pairs(q->tmp, kin, kout, rin, rout, n, 64, st));
        hipLaunchKernelGGL(quant::first_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, kout, n, first);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(quant::rank_kernel, dim3(quant::grid_for(n)), dim3(quant::kBlock), 0, st, kout, rout, n, first,
                           d_total, top_n, threshold, d_rank, d_mask);
        HIP_TRY(hipGetLastError());
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(total, d_total, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rank, d_rank, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mask, d_mask, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    q->h->d2h_bytes += (uint64_t)n * 13;
    return ADH_OK;
}

int adh_quant_time_ms(adh_quant_t *q, double *build_ms, double *filter_ms) {
    if (!q || !build_ms || !filter_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *build_ms = q->build_ms;
    *filter_ms = q->filter_ms;
    return ADH_OK;
}

}  // extern "C"
