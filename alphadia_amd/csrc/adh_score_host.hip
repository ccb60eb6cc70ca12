// adh_score_host.hip - host side of the scoring entry points (included by adh_api.hip inside
// its extern "C" block): candidate upload, the device-built plan (adh_plan.hip), kernel
// launches and the chunked host -> host pipeline of adh_score_candidates.
//
// Replaces the harness around the reference's pjit loop:
//   CandidateScoring.__call__            alphadia/search/scoring/scoring.py:582-661
//   assemble_score_group_container       alphadia/search/scoring/scoring.py:273-353
//   _process_score_groups                alphadia/search/scoring/scoring.py:114-137
// Timeline of one adh_score_candidates call (three HIP streams, two plan slots):
//   copy-in : H2D columns(c+1) | plan(c+1)                    (while the kernels of chunk c run)
//   compute : zero tables | gather(c) features(c) | gather(c+1) ...
//   copy-out:                  D2H tables(c) | D2H tables(c+1) ...
// The host only waits for the 128-byte plan record of a chunk (class sizes, LDS capacities,
// validation result) before it launches that chunk's kernels.

namespace {

// adh_comm.hip
int comm_wait_slot(adh_handle *h, int slot);
int comm_gather_slot(adh_handle *h, int slot);

struct OutFieldDesc {
    const char *name;  // the OutputPsmDF column (adh_table_layout)
    size_t member;   // offsetof the pointer inside adh_output_t
    int per_row;     // 1, ADH_NUM_FEATURES, or -1 = top_k
    int elem;        // bytes per element
    bool wire;       // travels in the all-gather and over PCIe (computed tables); the others are rebuilt locally
    bool optional;   // the caller's host pointer may be NULL
};
// The columns that are not `wire` are copies of the candidate table (precursor_idx, rank) and of the library
// (per fragment slot): adh_score_candidates does not copy them back, it rebuilds them in the caller's host
// buffers from fragment_lib_slot with host threads while the D2H copies of later chunks are in flight
// (216 of the 646 bytes per candidate; the link is what bounds the host -> host step).
// stat_matched_peaks is the exception: computed, optional, copied when asked for.

// computed tables first: they form the contiguous "wire" prefix of the packed device buffer
const OutFieldDesc kOutFields[] = {
    {"valid", offsetof(adh_output_t, valid), 1, 1, true, false},
    {"features", offsetof(adh_output_t, features), ADH_NUM_FEATURES, 4, true, false},
    {"fragment_mz_observed", offsetof(adh_output_t, fragment_mz_observed), -1, 4, true, false},
    {"fragment_height", offsetof(adh_output_t, fragment_height), -1, 4, true, false},
    {"fragment_intensity", offsetof(adh_output_t, fragment_intensity), -1, 4, true, false},
    {"fragment_mass_error", offsetof(adh_output_t, fragment_mass_error), -1, 4, true, false},
    {"fragment_correlation", offsetof(adh_output_t, fragment_correlation), -1, 4, true, false},
    {"fragment_lib_slot", offsetof(adh_output_t, fragment_lib_slot), -1, 2, true, true},
    {"precursor_idx", offsetof(adh_output_t, precursor_idx), 1, 4, false, false},
    {"rank", offsetof(adh_output_t, rank), 1, 1, false, false},
    {"fragment_precursor_idx", offsetof(adh_output_t, fragment_precursor_idx), -1, 4, false, false},
    {"fragment_rank", offsetof(adh_output_t, fragment_rank), -1, 1, false, false},
    {"fragment_mz_library", offsetof(adh_output_t, fragment_mz_library), -1, 4, false, false},
    {"fragment_mz", offsetof(adh_output_t, fragment_mz), -1, 4, false, false},
    {"fragment_position", offsetof(adh_output_t, fragment_position), -1, 1, false, false},
    {"fragment_number", offsetof(adh_output_t, fragment_number), -1, 1, false, false},
    {"fragment_type", offsetof(adh_output_t, fragment_type), -1, 1, false, false},
    {"fragment_charge", offsetof(adh_output_t, fragment_charge), -1, 1, false, false},
    {"fragment_loss_type", offsetof(adh_output_t, fragment_loss_type), -1, 1, false, false},
    {"stat_matched_peaks", offsetof(adh_output_t, stat_matched_peaks), 1, 4, false, true},
};
constexpr int kNumOutFields = (int)(sizeof(kOutFields) / sizeof(kOutFields[0]));

inline void **out_member(adh_output_t *o, const OutFieldDesc &f) {
    return reinterpret_cast<void **>(reinterpret_cast<unsigned char *>(o) + f.member);
}
inline size_t out_row_bytes(const OutFieldDesc &f, int top_k) {
    return (size_t)(f.per_row < 0 ? top_k : f.per_row) * (size_t)f.elem;
}

// layout of the packed device tables for `rows` rows: view->... = base + offset; returns total bytes
size_t layout_tables(unsigned char *base, int64_t rows, int top_k, adh_output_t *view, size_t *wire_bytes) {
    size_t off = 0, wire = 0;
    for (int i = 0; i < kNumOutFields; ++i) {
        const OutFieldDesc &f = kOutFields[i];
        if (view) *out_member(view, f) = base ? (void *)(base + off) : nullptr;
        off += ((size_t)rows * out_row_bytes(f, top_k) + 255) / 256 * 256;
        if (f.wire) wire = off;
    }
    if (wire_bytes) *wire_bytes = wire;
    if (view) {
        view->n = rows;
        view->top_k = top_k;
    }
    return std::max<size_t>(off, 256);
}

int ensure_tables_in(DevTables &t, int64_t rows, int top_k) {
    const size_t need = layout_tables(nullptr, rows, top_k, nullptr, nullptr);
    if (t.bytes < need) {
        if (t.base) (void)hipFree(t.base);
        t.base = nullptr;
        t.bytes = 0;
        hipError_t e = hipMalloc(&t.base, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ADH_ERR_OUT_OF_MEMORY, std::string("hipMalloc(output tables): ") + hipGetErrorString(e));
        }
        t.bytes = need;
    }
    t.used = layout_tables(static_cast<unsigned char *>(t.base), rows, top_k, &t.view, &t.wire_bytes);
    t.rows = rows;
    t.top_k = top_k;
    return ADH_OK;
}

int ensure_tables(adh_handle *h, int slot, int64_t rows, int top_k) { return ensure_tables_in(h->tables[slot], rows, top_k); }

// ---------------------------------------------------------------- candidate columns in HBM
struct CandColumn {
    const void *host;
    void **dev;
    size_t elem;
};

int cand_reserve(adh_handle *h, int64_t n, int32_t n_iso) {
    CandSlab &s = h->cs;
    const int64_t rows = std::max<int64_t>(n, 1);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t need = 3 * al((size_t)rows * 4) + 3 * al((size_t)rows) + 6 * al((size_t)rows * 8) +
                        al((size_t)rows * 4) + al((size_t)rows * (size_t)n_iso * 4);
    if (s.bytes < need) {
        HIP_TRY(hipDeviceSynchronize());  // nothing may still read the old slab
        if (s.base) (void)hipFree(s.base);
        s.base = nullptr;
        s.bytes = 0;
        HIP_TRY(hipMalloc(&s.base, need + need / 8));
        s.bytes = need + need / 8;
    }
    unsigned char *p = static_cast<unsigned char *>(s.base);
    auto take = [&](size_t b) {
        unsigned char *q = p;
        p += al(b);
        return q;
    };
    s.d.precursor_idx = (const uint32_t *)take((size_t)rows * 4);
    s.d.frag_start = (const uint32_t *)take((size_t)rows * 4);
    s.d.frag_stop = (const uint32_t *)take((size_t)rows * 4);
    s.d.rank = (const uint8_t *)take((size_t)rows);
    s.flags = (uint8_t *)take((size_t)rows);
    s.d.charge = (const uint8_t *)take((size_t)rows);
    s.d.scan_start = (const int64_t *)take((size_t)rows * 8);
    s.d.scan_stop = (const int64_t *)take((size_t)rows * 8);
    s.d.scan_center = (const int64_t *)take((size_t)rows * 8);
    s.d.frame_start = (const int64_t *)take((size_t)rows * 8);
    s.d.frame_stop = (const int64_t *)take((size_t)rows * 8);
    s.d.frame_center = (const int64_t *)take((size_t)rows * 8);
    s.d.precursor_mz = (const float *)take((size_t)rows * 4);
    s.iso = (float *)take((size_t)rows * (size_t)n_iso * 4);
    s.d.flags = nullptr;
    s.n = n;
    s.n_iso_cols = n_iso;
    return ADH_OK;
}

// H2D of rows [a, b) of every candidate column, asynchronous on `st`
// Copy jobs done by a kernel: the candidate columns of a SMALL range (<= 131 072 rows: the batches of the
// optimisation loop, the short first chunk of a large call) when they sit in page-locked host memory - one
// launch that reads the 14 host columns over PCIe instead of 14 DMA copies.  Measured: 5-10 % on small
// batches (8 000 precursors host -> host 1.45 -> 1.33 ms: fewer driver calls).  Large ranges stay with the
// DMA engine: a copy kernel sits on the CUs for the 4-5 ms the 0.2 GB of a 3 M-candidate step take over PCIe
// and the gather kernel next to it ran 7 % slower, with nothing gained on the step (the host-bound stream
// is the limit either way; round 4 again, for the burst behind the plan of chunk 1 and for per-chunk uploads: the
// scoring kernels 14.8 -> 17.7 ... 18.4 ms, the step 33 -> 37 ms).  ADH_H2D_KERNEL=0 switches the kernel off; pageable columns always use
// hipMemcpyAsync.
struct CopyJobs {
    const unsigned char *src[16];
    unsigned char *dst[16];
    uint64_t bytes[16];
    int n;
};
__global__ __launch_bounds__(256) void adh_copy_jobs_kernel(CopyJobs jobs) {
    const int j = blockIdx.y;
    if (j >= jobs.n) return;
    const unsigned char *src = jobs.src[j];
    unsigned char *dst = jobs.dst[j];
    const uint64_t bytes = jobs.bytes[j];
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        const uint64_t words = bytes / 16;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (uint64_t w = tid; w < words; w += stride) d4[w] = s4[w];
        for (uint64_t q = words * 16 + tid; q < bytes; q += stride) dst[q] = src[q];
    } else {
        for (uint64_t q = tid; q < bytes; q += stride) dst[q] = src[q];
    }
}

int cand_upload_range(adh_handle *h, const adh_candidates_t *c, int64_t a, int64_t b, hipStream_t st) {
    CandSlab &s = h->cs;
    if (b <= a) return ADH_OK;
    s.d.flags = c->flags ? s.flags : nullptr;
    const size_t iso_w = (size_t)c->n_isotope_cols * 4;
    const CandColumn cols[] = {
        {c->precursor_idx, (void **)&s.d.precursor_idx, 4}, {c->frag_start_idx, (void **)&s.d.frag_start, 4},
        {c->frag_stop_idx, (void **)&s.d.frag_stop, 4},     {c->rank, (void **)&s.d.rank, 1},
        {c->flags, (void **)&s.flags, 1},                   {c->charge, (void **)&s.d.charge, 1},
        {c->scan_start, (void **)&s.d.scan_start, 8},       {c->scan_stop, (void **)&s.d.scan_stop, 8},
        {c->scan_center, (void **)&s.d.scan_center, 8},     {c->frame_start, (void **)&s.d.frame_start, 8},
        {c->frame_stop, (void **)&s.d.frame_stop, 8},       {c->frame_center, (void **)&s.d.frame_center, 8},
        {c->precursor_mz, (void **)&s.d.precursor_mz, 4},   {c->isotope_intensity, (void **)&s.iso, iso_w},
    };
    // page-locked columns are read by a kernel, pageable ones go through hipMemcpyAsync
    static const bool by_kernel = [] {
        const char *env = getenv("ADH_H2D_KERNEL");
        return !(env && atoi(env) == 0);
    }();
    CopyJobs jobs;
    jobs.n = 0;
    uint64_t most = 0;
    for (const CandColumn &col : cols) {
        if (!col.host) continue;
        unsigned char *dst = static_cast<unsigned char *>(*col.dev) + (size_t)a * col.elem;
        const unsigned char *src = static_cast<const unsigned char *>(col.host) + (size_t)a * col.elem;
        const size_t bytes = (size_t)(b - a) * col.elem;
        void *dev_view = nullptr;
        if (by_kernel && b - a <= 131072) {  // (small ranges only: see above)
            hipPointerAttribute_t attr;
            if (hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost &&
                hipHostGetDevicePointer(&dev_view, const_cast<unsigned char *>(src), 0) == hipSuccess && dev_view) {
                jobs.src[jobs.n] = static_cast<const unsigned char *>(dev_view);
                jobs.dst[jobs.n] = dst;
                jobs.bytes[jobs.n] = bytes;
                most = std::max<uint64_t>(most, bytes);
                ++jobs.n;
                continue;
            }
            (void)hipGetLastError();
        }
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    }
    if (jobs.n > 0) {
        const unsigned blocks = (unsigned)std::min<uint64_t>(std::max<uint64_t>(most / 16 / 256, 1), 64);
        hipLaunchKernelGGL(adh_copy_jobs_kernel, dim3(blocks, (unsigned)jobs.n), dim3(256), 0, st, jobs);
        HIP_TRY(hipGetLastError());
    }
    return ADH_OK;
}

int check_candidate_args(adh_handle *h, const adh_candidates_t *c) {
    if (!(h->run_staged || h->tims_staged) || !h->lib_staged)
        return fail(ADH_ERR_NOT_STAGED, "stage the run and the fragment library first");
    if (c->n < 0 || c->n_isotope_cols < 1)
        return fail(ADH_ERR_INVALID_ARGUMENT, "invalid candidate table dimensions");
    if (c->n > 0x7FFFFFFFll) return fail(ADH_ERR_UNSUPPORTED, "more than 2^31 candidates in one batch");
    if (c->n > 0 && (!c->precursor_idx || !c->rank || !c->frag_start_idx || !c->frag_stop_idx || !c->scan_start ||
                     !c->scan_stop || !c->scan_center || !c->frame_start || !c->frame_stop || !c->frame_center ||
                     !c->charge || !c->precursor_mz || !c->isotope_intensity))
        return fail(ADH_ERR_INVALID_ARGUMENT, "candidate column is NULL");
    return ADH_OK;
}

// ---------------------------------------------------------------- the plan (adh_plan.hip)
__global__ void adh_plan_init_kernel(PlanMeta *meta, int32_t I) {
    // a word per lane into the record itself (a private copy of the record is scratch memory): the ten maxima
    // all_k ... gen_n_lib start at 1, everything else at 0
    static_assert(offsetof(PlanMeta, class_first) - offsetof(PlanMeta, all_k) == 10 * sizeof(int32_t) && sizeof(PlanMeta) % 4 == 0,
                  "PlanMeta: the maxima are ten consecutive words");
    constexpr unsigned w0 = offsetof(PlanMeta, all_k) / 4, w1 = offsetof(PlanMeta, class_first) / 4;
    int32_t *const words = reinterpret_cast<int32_t *>(meta);
    for (unsigned w = threadIdx.x; w < sizeof(PlanMeta) / 4; w += blockDim.x) words[w] = (w >= w0 && w < w1) ? 1 : 0;
    (void)I;
}

int plan_reserve(adh_handle *h, PlanSlot &s, int64_t n, bool im) {
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (!s.h_meta) HIP_TRY(hipHostMalloc((void **)&s.h_meta, sizeof(PlanMeta), hipHostMallocDefault));
    const size_t rec = im ? sizeof(CandRecIM) : sizeof(CandRec);
    if (s.cap >= n && s.rec_bytes >= rec) return ADH_OK;
    HIP_TRY(hipDeviceSynchronize());
    s.buf.release();
    s.cap = 0;
    const int64_t cap = n + n / 8 + 64;
    auto dev_alloc = [&](void **p, size_t bytes) -> int {
        HIP_TRY(hipMalloc(p, std::max<size_t>(bytes, 256)));
        s.buf.ptrs.push_back(*p);
        return ADH_OK;
    };
    int rc;
    if ((rc = dev_alloc(&s.recs, (size_t)cap * rec)) != ADH_OK) return rc;
    if ((rc = dev_alloc(&s.ordered, (size_t)cap * rec)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.keys_in, (size_t)cap * 4)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.keys_out, (size_t)cap * 4)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.idx_in, (size_t)cap * 4)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.idx_out, (size_t)cap * 4)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.bytes, (size_t)cap * 8)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.sorted_bytes, (size_t)cap * 8)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.offs, (size_t)cap * 8)) != ADH_OK) return rc;
    if ((rc = dev_alloc((void **)&s.d_meta, sizeof(PlanMeta))) != ADH_OK) return rc;
    size_t b_sort = 0, b_scan = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, s.keys_in, s.keys_out, s.idx_in, s.idx_out, (int)cap, 0, 32,
                                               h->stream));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan, s.sorted_bytes, s.offs, (int)cap, h->stream));
    s.cub_bytes = std::max(b_sort, b_scan);
    if ((rc = dev_alloc(&s.cub_tmp, s.cub_bytes)) != ADH_OK) return rc;
    s.cap = cap;
    s.rec_bytes = rec;
    return ADH_OK;
}

struct PlanKey {
    uint32_t top_k_fragments, top_k_isotopes;
    bool fast_cfg, quant_all, fused_cfg, wide_cfg, spill_all, im_spill_all;
};

PlanKey plan_key(const adh_scoring_config_t *cfg) {
    const bool fast = cfg->experimental_xic != 0 && !getenv("ADH_DEBUG_NO_FAST");
    return PlanKey{cfg->top_k_fragments, cfg->top_k_isotopes, fast, cfg->quant_all != 0,
                   fast && !getenv("ADH_DEBUG_NO_FUSED"),   // developer switches: two-kernel path only
                   fast && !getenv("ADH_DEBUG_NO_WIDE"),    // ... more than 16 kept fragments through the generic kernel
                   getenv("ADH_DEBUG_GENERIC_SPILL") != nullptr,   // ... every generic candidate through the spill instantiation
                   getenv("ADH_DEBUG_IM_SPILL") != nullptr};       // ... every ion-mobility candidate of the dynamic route likewise
}

// enqueue the plan of rows [row0, row0 + n) on `st`; plan_finish() waits for it
int plan_enqueue(adh_handle *h, PlanSlot &s, const adh_scoring_config_t *cfg, int64_t row0, int64_t n, hipStream_t st) {
    const bool im = h->tims_staged;
    int rc = plan_reserve(h, s, n, im);
    if (rc != ADH_OK) return rc;
    const PlanKey key = plan_key(cfg);
    PlanArgs p{};
    p.row0 = row0;
    p.n = n;
    p.n_lib = h->n_lib;
    p.I = (int32_t)std::min<uint32_t>(cfg->top_k_isotopes, (uint32_t)h->cs.n_iso_cols);
    p.top_k = cfg->top_k_fragments;
    p.fast_cfg = (key.fast_cfg ? 1 : 0) | (key.wide_cfg ? 2 : 0);
    p.quant_all = key.quant_all ? 1 : 0;
    p.spill_all = (im ? key.im_spill_all : key.spill_all) ? 1 : 0;
    p.fused_cfg = (key.fused_cfg && !im && h->run.n_ms1_obs == 1 && p.I <= 4) ? (getenv("ADH_DEBUG_NO_FUSED2") ? 1 : 3) : 0;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(adh_plan_init_kernel, dim3(1), dim3(128), 0, st, s.d_meta, p.I);
    const int64_t n_frames = im ? h->tims.n_frames : h->run.n_spectra;
    const int L = im ? h->tims.cycle_len : h->run.cycle_len;
    p.L = L;
    p.n_frames = n_frames;
    p.n_cyc_bins = (int32_t)std::min<int64_t>(n_frames / L + 2, 1 << 26);
    // counting sort when the key space is small next to the batch (the usual case: the sort classes x
    // cycles of the run); a stable radix sort otherwise
    const int64_t n_keys = (int64_t)ADH_N_SORT_CLASSES * p.n_cyc_bins;
    const bool counting = n_keys <= (1 << 22) && !getenv("ADH_DEBUG_PLAN_RADIX");
    if (counting) {
        if (s.hist_cap < n_keys + 1) {
            HIP_TRY(hipDeviceSynchronize());
            if (s.hist) (void)hipFree(s.hist);
            s.hist = nullptr;
            s.hist_cap = 0;
            HIP_TRY(hipMalloc((void **)&s.hist, (size_t)(n_keys + 1) * 4));
            s.hist_cap = n_keys + 1;
            size_t b = 0;
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, s.hist, s.hist, (int)(n_keys + 1), st));
            if (b > s.cub_bytes) {  // (the scratch was sized for the per-candidate scans)
                void *tmp = nullptr;
                HIP_TRY(hipMalloc(&tmp, b));
                s.buf.ptrs.push_back(tmp);
                s.cub_tmp = tmp;
                s.cub_bytes = b;
            }
        }
        HIP_TRY(hipMemsetAsync(s.hist, 0, (size_t)(n_keys + 1) * 4, st));
    }
    uint32_t *hist = counting ? s.hist : nullptr;
    if (im) {
        p.rows = h->tims.cycle_len;
        p.scan_max = h->tims.scan_max;
        p.zeroth = h->tims.zeroth;
        hipLaunchKernelGGL(adh_plan_rec_im_kernel, dim3(blocks), dim3(256), 0, st, h->cs.d, h->tims.cycle, h->tims.dpc, p,
                           static_cast<CandRecIM *>(s.recs), s.keys_in, s.idx_in, s.bytes, hist, s.d_meta);
    } else {
        p.rows = h->run.cycle_len * h->run.cycle_scans;
        hipLaunchKernelGGL(adh_plan_rec_kernel, dim3(blocks), dim3(256), 0, st, h->cs.d, h->run.cycle, p,
                           static_cast<CandRec *>(s.recs), s.keys_in, s.idx_in, s.bytes, hist, s.d_meta);
    }
    HIP_TRY(hipGetLastError());
    size_t tb = s.cub_bytes;
    if (counting) {
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.cub_tmp, tb, s.hist, s.hist, (int)(n_keys + 1), st));
        hipLaunchKernelGGL(adh_plan_scatter_kernel, dim3(blocks), dim3(256), 0, st, s.keys_in, s.bytes, n, s.hist, s.keys_out,
                           s.idx_out, s.sorted_bytes);
    } else {
        int end_bit = 1;
        while (end_bit < 32 && (1ull << end_bit) < (uint64_t)n_keys) ++end_bit;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(s.cub_tmp, tb, s.keys_in, s.keys_out, s.idx_in, s.idx_out, (int)n, 0,
                                                   end_bit, st));
        hipLaunchKernelGGL(adh_plan_take_bytes_kernel, dim3(blocks), dim3(256), 0, st, s.bytes, s.idx_out, n, s.sorted_bytes);
    }
    tb = s.cub_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.cub_tmp, tb, s.sorted_bytes, s.offs, (int)n, st));
    if (im)
        hipLaunchKernelGGL((adh_plan_order_kernel<CandRecIM>), dim3(blocks), dim3(256), 0, st,
                           static_cast<const CandRecIM *>(s.recs), s.keys_out, s.idx_out, s.offs, s.sorted_bytes, n,
                           (uint32_t)p.n_cyc_bins, static_cast<CandRecIM *>(s.ordered), s.d_meta);
    else
        hipLaunchKernelGGL((adh_plan_order_kernel<CandRec>), dim3(blocks), dim3(256), 0, st,
                           static_cast<const CandRec *>(s.recs), s.keys_out, s.idx_out, s.offs, s.sorted_bytes, n,
                           (uint32_t)p.n_cyc_bins, static_cast<CandRec *>(s.ordered), s.d_meta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s.h_meta, s.d_meta, sizeof(PlanMeta), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s.done, st));
    return ADH_OK;
}

int plan_finish(adh_handle *h, PlanSlot &s, const adh_scoring_config_t *cfg, int64_t row0, int64_t n, Plan &p) {
    HIP_TRY(hipEventSynchronize(s.done));
    const PlanMeta &m = *s.h_meta;
    switch (m.err) {
        case ADH_PLAN_OK: break;
        case ADH_PLAN_ERR_FRAG_SLICE: return fail(ADH_ERR_INVALID_ARGUMENT, "fragment slice outside the staged library");
        case ADH_PLAN_ERR_FRAME_LIMITS: return fail(ADH_ERR_INVALID_ARGUMENT, "frame limits outside the staged run");
        case ADH_PLAN_ERR_CYCLE_BOUNDARY: return fail(ADH_ERR_INVALID_ARGUMENT, "frame_start must sit on a cycle boundary");
        case ADH_PLAN_ERR_SCAN_LIMITS: return fail(ADH_ERR_INVALID_ARGUMENT, "scan limits outside the staged run");
        case ADH_PLAN_ERR_ALPHARAW_SCANS:
            return fail(ADH_ERR_UNSUPPORTED, "AlphaRaw candidates must have scan_start=0, scan_stop=1, scan_center=0");
        case ADH_PLAN_ERR_CHARGE: return fail(ADH_ERR_INVALID_ARGUMENT, "precursor charge is 0");
        case ADH_PLAN_ERR_TOO_MANY_OBS:
            return fail(ADH_ERR_UNSUPPORTED, h->tims_staged ? "a precursor overlaps more than 8 cycle rows"
                                                            : "a precursor overlaps more than 8 isolation windows");
        default: return fail(ADH_ERR_UNSUPPORTED, "more than 16 unfragmented cycle rows in the scan range");
    }
    const PlanKey key = plan_key(cfg);
    const int I = (int)std::min<uint32_t>(cfg->top_k_isotopes, (uint32_t)h->cs.n_iso_cols);
    p = Plan();
    p.row0 = row0;
    p.n = n;
    p.d_recs = h->tims_staged ? nullptr : static_cast<CandRec *>(s.ordered);
    p.d_recs_im = h->tims_staged ? static_cast<CandRecIM *>(s.ordered) : nullptr;
    for (int c = 0; c < ADH_N_CLASSES; ++c) p.n_class[c] = (int64_t)m.class_first[c + 1] - (int64_t)m.class_first[c];
    // the launch groups of the generic class are consecutive sort classes: one class to everything outside the plan
    p.n_class[ADH_CLASS_GENERIC] = (int64_t)m.class_first[ADH_N_SORT_CLASSES] - (int64_t)m.class_first[ADH_CLASS_GENERIC];
    for (int g = 0; g < ADH_GENERIC_GROUPS; ++g) {
        p.n_generic[g] = (int64_t)m.class_first[ADH_CLASS_GENERIC + g + 1] - (int64_t)m.class_first[ADH_CLASS_GENERIC + g];
        p.lds_generic[g] = m.gen_lds[g];
    }
    p.generic_over = m.gen_over;
    p.spill_all = key.spill_all;
    p.im_spill_all = key.im_spill_all;
    if (h->tims_staged) {
        // the launch groups of a class are consecutive sort classes (3 * slot + group): one class to everything outside the plan
        static const int slot_class[ADH_IM_CLASS_SLOTS] = {0, 1, ADH_CLASS_IM_SMALL, ADH_CLASS_GENERIC};
        for (int c = 0; c < ADH_N_CLASSES; ++c) p.n_class[c] = 0;
        for (int sl = 0; sl < ADH_IM_CLASS_SLOTS; ++sl)
            for (int g = 0; g < ADH_IM_GROUPS; ++g) {
                const int sc = sl * ADH_IM_GROUPS + g;
                p.n_im[sl][g] = (int64_t)m.class_first[sc + 1] - (int64_t)m.class_first[sc];
                p.lds_im[sl][g] = m.im_lds[sl][g];
                p.n_class[slot_class[sl]] += p.n_im[sl][g];
            }
        p.im_over = m.im_over;
        if (m.im_over != 0) {  // (a refusal: the record of the largest candidate, for the message)
            CandRecIM rec;
            const uint32_t j = 0xFFFFFFFFu - (uint32_t)(m.im_over & 0xFFFFFFFFu);
            HIP_TRY(hipMemcpy(&rec, static_cast<const CandRecIM *>(s.recs) + j, sizeof(rec), hipMemcpyDeviceToHost));
            const int L = h->tims.cycle_len, z = h->tims.zeroth;
            p.im_over_shape[0] = rec.k_cap;
            p.im_over_shape[1] = std::max<int>(rec.n_obs, 1);
            p.im_over_shape[2] = std::max(rec.scan_stop - rec.scan_start, 0);
            p.im_over_shape[3] = std::max((rec.frame_stop - z) / L - (rec.frame_start - z) / L, 0);
        }
    }
    p.caps_all = Caps{m.all_k, m.all_o, m.all_f, std::max(I, 1), m.all_n_lib, 0, m.all_s, m.all_op};
    p.scratch_bytes = std::max<uint64_t>(m.scratch_bytes, 32);
    p.top_k_fragments = key.top_k_fragments;
    p.top_k_isotopes = key.top_k_isotopes;
    p.fast_ok = key.fast_cfg;
    p.fused_ok = key.fused_cfg;
    p.wide_ok = key.wide_cfg;
    p.quant_all = key.quant_all;
    p.ready = true;
    return ADH_OK;
}

// the scratch slab is grow-only and shared by all chunks (their kernels are serialised on one stream)
// (see DevBlockCache in adh_api.hip)
void settle_copy_path(adh_handle *h) {
    // Only on request (ADH_COPY_PATH_RESET=1) and only after a block of 1 GB or more really went back to the runtime
    // (DevBlockCache in adh_api.hip parks them, so that needs a cache overflow or adh_trim_device_cache): page-locking
    // 2 GB of host memory once brings the DMA copies back to the full link rate on this ROCm (tools/probes/d2h_pattern.hip)
    (void)h;
    static const bool on = [] {
        const char *env = getenv("ADH_COPY_PATH_RESET");
        return env && atoi(env) != 0;
    }();
    if (!on || !g_big_free.exchange(false)) return;
    void *p = nullptr;
    if (hipHostMalloc(&p, (size_t)2 << 30, hipHostMallocPortable) == hipSuccess && p) (void)hipHostFree(p);
    (void)hipGetLastError();  // (no room for it: the copies stay slow, nothing else changes)
}

// The grow-only buffers of a handle: `*p` holds at least `need` bytes afterwards (`*bytes` says how many); a block that
// has to grow is replaced by one of need + slack bytes.  Device memory goes back only once the device is idle
// (whatever was enqueued may still read the old block).
int grow_device(void **p, size_t *bytes, size_t need, size_t slack) {
    if (*bytes >= need) return ADH_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (*p) (void)hipFree(*p);
    *p = nullptr, *bytes = 0;
    HIP_TRY(hipMalloc(p, need + slack));
    *bytes = need + slack;
    return ADH_OK;
}
// ... and page-locked host memory
int grow_pinned(void **p, size_t *bytes, size_t need, size_t slack) {
    if (*bytes >= need) return ADH_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr, *bytes = 0;
    HIP_TRY(hipHostMalloc(p, need + slack, hipHostMallocDefault));
    *bytes = need + slack;
    return ADH_OK;
}
int ensure_scratch(adh_handle *h, uint64_t bytes) { return grow_device(&h->scratch_slab, &h->scratch_slab_bytes, bytes, bytes / 4); }

// fold finished timing triples into the running sums so that the event list stays short
void fold_timed(adh_handle *h, bool wait) {
    size_t keep = 0;
    for (size_t i = 0; i < h->timed.size(); ++i) {
        adh_handle::Timed &t = h->timed[i];
        bool done = wait ? (hipEventSynchronize(t.e2) == hipSuccess) : (hipEventQuery(t.e2) == hipSuccess);
        float a = 0, b = 0;
        if (done && hipEventElapsedTime(&a, t.e0, t.e1) == hipSuccess && hipEventElapsedTime(&b, t.e1, t.e2) == hipSuccess) {
            h->sum_gather_ms += a;
            h->sum_feature_ms += b;
            ++h->n_timed;
            h->free_events.push_back(t.e0);
            h->free_events.push_back(t.e1);
            h->free_events.push_back(t.e2);
        } else {
            h->timed[keep++] = t;
        }
    }
    (void)hipGetLastError();
    h->timed.resize(keep);
}

// The developer switches of an ion-mobility launch (ADH_DEBUG_IM*), read from the environment here and nowhere else,
// once per call of launch_scoring: the tests flip them between calls on one handle.  (plan_key reads the plan's own.)
struct ImSwitches {
    int32_t stop_phase, drop_dense, stop4;
    size_t gather_pad, feature_pad, tile4_two_pad;
    bool dynamic_layout, no_split, no_split2, tile1, tile1_two, no_fuse4, no_tiles;
};

ImSwitches im_switches_from_env() {
    auto number = [](const char *name) { const char *v = getenv(name); return v ? atoi(v) : 0; };
    auto is_set = [](const char *name) { return getenv(name) != nullptr; };
    ImSwitches sw{};
    sw.stop_phase = number("ADH_DEBUG_IM");  // ablation stops of the gather and the one-kernel path (8: dense tiles only)
    sw.drop_dense = number("ADH_DEBUG_IM_DROP_DENSE");
    // extra LDS per block, to see what occupancy is worth: the gather, every feature launch, the two-observation tile4 launch alone
    sw.gather_pad = (size_t)number("ADH_DEBUG_IM_GATHER_LDS_PAD");
    sw.feature_pad = (size_t)number("ADH_DEBUG_IM_FEATURE_LDS_PAD");
    sw.tile4_two_pad = (size_t)number("ADH_DEBUG_IM_TILE4_TWO_LDS_PAD");
    sw.dynamic_layout = is_set("ADH_DEBUG_IM_DYNAMIC_LAYOUT");  // no fixed layout
    sw.no_split = is_set("ADH_DEBUG_IM_NO_SPLIT");              // the one-kernel path for everything
    sw.no_split2 = is_set("ADH_DEBUG_IM_NO_SPLIT2");            // ... for the two-observation class
    sw.tile1 = is_set("ADH_DEBUG_IM_TILE1");                    // the one-candidate-per-wavefront tile kernel everywhere
    sw.tile1_two = is_set("ADH_DEBUG_IM_TILE1_TWO");            // ... for the two-observation class
    sw.no_fuse4 = is_set("ADH_DEBUG_IM_NO_FUSE4");              // tile and profile phase in two kernels
    sw.stop4 = number("ADH_DEBUG_IM4");                         // ablation stops of the tile4 kernel (tile4_phase); not fused then
    sw.no_tiles = is_set("ADH_DEBUG_IM_NO_TILES");  // A/B: the gather without the (window, TOF bin) ranges of the TOF-major events
    return sw;
}

// What an ion-mobility plan is still refused for, before anything is launched or counted.  No candidate is refused for
// the product of the call's maxima: every block of the dynamic route asks for its candidate's own layout.
int refuse_im(const Plan &p, const ImSwitches &sw) {
    char buf[256];
    if (p.im_over != 0) {
        // even the spill path keeps everything indexed by K * O and K, the template and the scan tables in LDS
        // (featim::LayoutSpill)
        snprintf(buf, sizeof(buf),
                 "candidate needs %llu bytes of LDS on the spill path of the ion-mobility feature kernel (K=%lld O=%lld S=%lld F=%lld): "
                 "exceeds the bound of %d bytes",
                 (unsigned long long)(p.im_over >> 32), (long long)p.im_over_shape[0], (long long)p.im_over_shape[1],
                 (long long)p.im_over_shape[2], (long long)p.im_over_shape[3], (int)ADH_IM_LDS_LIMIT);
        return fail(ADH_ERR_UNSUPPORTED, buf);
    }
    const size_t g_lds = adh_gather_im_lds_bytes(p.caps_all) + sw.gather_pad;
    if (g_lds > 160 * 1024) {
        snprintf(buf, sizeof(buf),
                 "library slice of %d fragments needs %zu bytes of LDS in the ion-mobility gather kernel: exceeds 160 KiB",
                 p.caps_all.n_lib, g_lds);
        return fail(ADH_ERR_UNSUPPORTED, buf);
    }
    return ADH_OK;
}

// ---- the route of every plan class of an ion-mobility launch: im_launch_routes decides, launch_scoring_im follows
struct ImRoute {
    int32_t layout, launch;  // ADH_IM_LAYOUT_*, ADH_IM_LAUNCH_* (include/alphadia_hip.h: adh_im_launch_routes); 0: the class is empty
    uint64_t prof_off;  // split launches: the class's profile records (ImProfRec) in the scratch slab
    uint64_t side_off;  // fused4 / tile4: its side list (featim4::side_bytes: a counter and the plan positions)
};
struct ImRoutes {
    ImRoute of[ADH_N_CLASSES];
    uint64_t scratch_bytes;  // the plan's blocks, the profile records and the side lists behind them
};

// the maxima of the launch of plan class `c` (one launch per observation class: 1, 2, more; adh_plan_rec_im_kernel)
Caps im_class_caps(Caps cc, int c) {
    if (c == 0 || c == ADH_CLASS_IM_SMALL) cc.o = 1;
    if (c == 1) cc.o = std::min(cc.o, 2);
    if (c == ADH_CLASS_IM_SMALL) {  // (what the plan admitted to the class)
        cc.k = std::min(cc.k, ADH_IM_SMALL_K);
        cc.s = std::min(cc.s, ADH_IM_SMALL_S);
        cc.f = std::min(cc.f, ADH_IM_SMALL_F);
    }
    return cc;
}

// The rule, and nothing else: no HIP call, no handle.  `caps`: the launch maxima (k, o, s, f and the isotopes i of the
// call); `scratch_bytes`: the plan's blocks in the scratch slab.
//  * Split feature path (adh_features_im2.hip): a one- or two-observation class whose maxima a fixed layout holds leaves
//    a profile record per candidate behind the scratch blocks, and a second kernel with four candidates per wavefront
//    finishes them.  Not with four isotopes, without experimental_xic or under a stop of the one-kernel path (8 is the
//    gather's dense-tiles switch, no feature-kernel stop): the one-kernel path then, on a fixed layout where one holds
//    the class (capacities fixed at compile time: adh_features_im.hip, DimsFix).
//  * The tile part of a split class takes four candidates per wavefront (tile4, adh_features_im4.hip); the candidates
//    it leaves aside (materialised tiles) are on the class's side list and taken by the first blocks of the same grid
//    with the one-candidate body.  With one observation the profile phase runs in the same kernel (fused4).
//    split1: the one-candidate-per-wavefront tile kernel, then the profile kernel.
//  * Everything else: the dynamic route, every block with its candidate's own layout.
ImRoutes im_launch_routes(const Caps &caps, const int64_t *n_class, const adh_scoring_config_t *cfg, const ImSwitches &sw,
                          uint64_t scratch_bytes) {
    using namespace featim;
    const bool fixed = !sw.dynamic_layout;
    const bool split_cfg = fixed && cfg->experimental_xic && (sw.stop_phase == 0 || sw.stop_phase == 8) && !sw.no_split && caps.i <= 3;
    const bool tile4 = !sw.tile1;
    const bool fuse4 = tile4 && !sw.no_fuse4 && sw.stop4 == 0;
    const int32_t one_obs = fuse4 ? ADH_IM_LAUNCH_FUSED4 : tile4 ? ADH_IM_LAUNCH_TILE4 : ADH_IM_LAUNCH_SPLIT1;
    const int32_t two_obs = tile4 && !sw.tile1_two ? ADH_IM_LAUNCH_TILE4 : ADH_IM_LAUNCH_SPLIT1;
    ImRoutes r{};
    for (int c = 0; c < ADH_N_CLASSES; ++c) {
        if (n_class[c] <= 0) continue;
        const Caps cc = im_class_caps(caps, c);
        // (the small class was admitted candidate by candidate, plane size included: its axes alone are asked, and
        // not the f >= 3 of the split path of the common shapes)
        if (c == ADH_CLASS_IM_SMALL && fixed && DimsSmall::holds_axes(cc))
            r.of[c] = {ADH_IM_LAYOUT_SMALL, split_cfg ? one_obs : ADH_IM_LAUNCH_ONE};
        else if (c == 1 && split_cfg && DimsCommon2::holds(cc) && cc.f >= 3 && !sw.no_split2)
            r.of[c] = {ADH_IM_LAYOUT_COMMON2, two_obs};
        else if (fixed && DimsCommon::holds(cc))
            r.of[c] = {ADH_IM_LAYOUT_COMMON, c == 0 && split_cfg && cc.f >= 3 ? one_obs : ADH_IM_LAUNCH_ONE};
        else
            r.of[c] = {ADH_IM_LAYOUT_DYNAMIC, ADH_IM_LAUNCH_ONE};
    }
    // behind the plan's blocks: the profile records of the split classes, then the side lists
    static const int split_classes[3] = {0, ADH_CLASS_IM_SMALL, 1};
    uint64_t at = (scratch_bytes + 255) / 256 * 256;
    for (int c : split_classes) {
        ImRoute &rt = r.of[c];
        if (rt.launch == ADH_IM_LAUNCH_NONE || rt.launch == ADH_IM_LAUNCH_ONE) continue;
        rt.prof_off = at;
        at += (uint64_t)n_class[c] * (rt.layout == ADH_IM_LAYOUT_SMALL    ? sizeof(ImProfRec<DimsSmall::Fc, DimsSmall::Sc, 1>)
                                      : rt.layout == ADH_IM_LAYOUT_COMMON ? sizeof(ImProfRec<DimsCommon::Fc, DimsCommon::Sc, 1>)
                                                                          : sizeof(ImProfRec<DimsCommon2::Fc, DimsCommon2::Sc, 2>));
    }
    at = (at + 255) / 256 * 256;
    for (int c : split_classes) {
        ImRoute &rt = r.of[c];
        if (rt.launch != ADH_IM_LAUNCH_FUSED4 && rt.launch != ADH_IM_LAUNCH_TILE4) continue;
        rt.side_off = at;
        at += featim4::side_bytes(n_class[c]);
    }
    r.scratch_bytes = at;
    return r;
}

// The launches of `cnt` candidates of one plan class, from plan position `first`, on a fixed layout with NO observations.
extern "C++" template <class Dims, class Layout, int NO>
int launch_im_fixed(adh_handle *h, const Plan &p, const adh_scoring_config_t *cfg, adh_output_t *out, hipStream_t st,
                    const ImSwitches &sw, const ImRoute &rt, const Caps &cc, int64_t first, int64_t cnt) {
    constexpr int Fc = Dims::Fc, Sc = Dims::Sc;
    const int32_t n_iso = h->cs.n_iso_cols;
    const CandRecIM *recs = p.d_recs_im + first;
    unsigned char *d_scratch = static_cast<unsigned char *>(h->scratch_slab);
    unsigned char *prof = d_scratch + rt.prof_off;
    uint32_t *side = reinterpret_cast<uint32_t *>(d_scratch + rt.side_off);
    const size_t lay_lds = Layout(cc).bytes() + sw.feature_pad;
    const unsigned groups = (unsigned)((cnt + ADH_WAVE / 16 - 1) / (ADH_WAVE / 16));
    const unsigned list_blocks = (unsigned)std::min<int64_t>(cnt, 1024);  // (blocks that take the materialised tiles in turn)
    if (rt.launch == ADH_IM_LAUNCH_FUSED4 || rt.launch == ADH_IM_LAUNCH_TILE4) {
        const unsigned ob = (unsigned)((cnt + 255) / 256);
        HIP_TRY(hipMemsetAsync(side, 0, featim4::SIDE_HEAD * 4, st));
        hipLaunchKernelGGL(adh_im_order_hist_kernel, dim3(ob), dim3(256), 0, st, recs, (int32_t)cnt, d_scratch, side);
        hipLaunchKernelGGL(adh_im_order_scatter_kernel, dim3(ob), dim3(256), 0, st, recs, (int32_t)cnt, d_scratch, side);
    }
    // (the kernels that take a whole class in one launch exist for one observation only)
    const char *no_kernel = "ion-mobility launch: no kernel for this layout and launch kind";
    switch (rt.launch) {
        case ADH_IM_LAUNCH_FUSED4:
            if constexpr (NO == 1) {
                const size_t f4_lds = std::max({sizeof(featim4::WaveTile<Fc, Sc, 1>), sizeof(featim2::GroupLds<Fc, Sc, 1>) * (ADH_WAVE / 16),
                                                lay_lds + ADH_IM_STATIC_LDS + 16});
                hipLaunchKernelGGL((adh_feature_im_fused4_kernel<Fc, Sc, Layout>), dim3(groups + list_blocks), dim3(ADH_WAVE), f4_lds,
                                   st, h->tims, recs, (int32_t)cnt, h->cs.iso, n_iso, *cfg, d_scratch, *out, side, cc,
                                   (int32_t)list_blocks);
                HIP_TRY(hipGetLastError());
                return ADH_OK;
            }
            return fail(ADH_ERR_UNSUPPORTED, no_kernel);
        case ADH_IM_LAUNCH_TILE4: {
            const size_t t4_lds = std::max(sizeof(featim4::WaveTile<Fc, Sc, NO>), lay_lds + ADH_IM_STATIC_LDS + 16) +
                                  (NO == 2 ? sw.tile4_two_pad : 0);
            hipLaunchKernelGGL((adh_feature_im_tile4_kernel<Fc, Sc, NO, Layout>), dim3(groups + list_blocks), dim3(ADH_WAVE), t4_lds,
                               st, h->tims, recs, (int32_t)cnt, h->cs.iso, n_iso, *cfg, d_scratch, *out, prof, side, cc,
                               (int32_t)list_blocks, sw.stop4);
            break;
        }
        case ADH_IM_LAUNCH_SPLIT1:
            hipLaunchKernelGGL((adh_feature_im_kernel<Layout, true>), dim3((unsigned)cnt), dim3(ADH_WAVE), lay_lds, st, h->tims, recs,
                               h->cs.iso, n_iso, *cfg, d_scratch, *out, cc, prof);
            break;
        case ADH_IM_LAUNCH_ONE:
            if constexpr (NO == 1) {
                hipLaunchKernelGGL(adh_feature_im_kernel<Layout>, dim3((unsigned)cnt), dim3(ADH_WAVE), lay_lds, st, h->tims, recs,
                                   h->cs.iso, n_iso, *cfg, d_scratch, *out, cc);
                HIP_TRY(hipGetLastError());
                return ADH_OK;
            }
            return fail(ADH_ERR_UNSUPPORTED, no_kernel);
        default: return fail(ADH_ERR_UNSUPPORTED, no_kernel);
    }
    hipLaunchKernelGGL((adh_feature_im_profiles_kernel<Fc, Sc, NO>), dim3(groups), dim3(ADH_WAVE), 0, st, h->tims, recs,
                       (int32_t)cnt, *cfg, n_iso, d_scratch, prof, *out);
    HIP_TRY(hipGetLastError());
    return ADH_OK;
}

int launch_scoring_im(adh_handle *h, Plan &p, const adh_scoring_config_t *cfg, adh_output_t *out, hipStream_t st,
                      const ImSwitches &sw) {
    if (cfg->collect_fragments && p.caps_all.k > out->top_k)
        return fail(ADH_ERR_INVALID_ARGUMENT, "output top_k smaller than config.top_k_fragments");
    p.caps_all.stop_phase = sw.stop_phase;
    p.caps_all.dbg_drop_dense = sw.drop_dense;
    const size_t g_lds = adh_gather_im_lds_bytes(p.caps_all) + sw.gather_pad;  // (within the LDS of a CU: refuse_im)
    const int32_t n_iso = h->cs.n_iso_cols;
    const ImRoutes routes = im_launch_routes(p.caps_all, p.n_class, cfg, sw, p.scratch_bytes);
    int rc = ensure_scratch(h, routes.scratch_bytes);
    if (rc != ADH_OK) return rc;
    unsigned char *d_scratch = static_cast<unsigned char *>(h->scratch_slab);
    adh_handle::Timed t;
    rc = get_event(h, &t.e0);
    if (rc == ADH_OK) rc = get_event(h, &t.e1);
    if (rc == ADH_OK) rc = get_event(h, &t.e2);
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipEventRecord(t.e0, st));
    DevTims run_view = h->tims;
    if (sw.no_tiles) run_view.tile_ev = nullptr;
    hipLaunchKernelGGL(adh_gather_im_kernel, dim3((unsigned)p.n), dim3(ADH_WAVE), g_lds, st, run_view, h->d_lib,
                       p.d_recs_im, *cfg, n_iso, d_scratch, *out, p.caps_all);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t.e1, st));
    int64_t first = 0;
    for (int c = 0; c < ADH_N_CLASSES; first += p.n_class[c], ++c) {
        const int64_t cnt = p.n_class[c];
        if (cnt <= 0) continue;
        const ImRoute &rt = routes.of[c];
        const Caps cc = im_class_caps(p.caps_all, c);
        if (rt.layout == ADH_IM_LAYOUT_SMALL)
            rc = launch_im_fixed<featim::DimsSmall, featim::LayoutSmall, 1>(h, p, cfg, out, st, sw, rt, cc, first, cnt);
        else if (rt.layout == ADH_IM_LAYOUT_COMMON2)
            rc = launch_im_fixed<featim::DimsCommon2, featim::LayoutCommon2, 2>(h, p, cfg, out, st, sw, rt, cc, first, cnt);
        else if (rt.layout == ADH_IM_LAYOUT_COMMON)
            rc = launch_im_fixed<featim::DimsCommon, featim::LayoutCommon, 1>(h, p, cfg, out, st, sw, rt, cc, first, cnt);
        else {
            // the dynamic route: one launch per group of own layouts, each with the LDS of its largest candidate
            // (the plan sorted the class by group); the last group keeps its profile regions in the spill blocks
            // of the scratch slab
            const int sl = c == ADH_CLASS_GENERIC ? ADH_IM_CLASS_SLOTS - 1 : c;
            int64_t at = 0;
            for (int g = 0; g < ADH_IM_GROUPS; ++g) {
                const int64_t ng = p.n_im[sl][g];
                if (ng == 0) continue;
                const size_t lds = (size_t)p.lds_im[sl][g];
                const size_t lds_pad = std::min<size_t>(lds + sw.feature_pad, ADH_IM_LDS_LIMIT);
                if (g == ADH_IM_GROUP_SPILL)
                    hipLaunchKernelGGL(adh_feature_im_own_kernel<true>, dim3((unsigned)ng), dim3(ADH_WAVE), lds_pad, st, h->tims,
                                       p.d_recs_im + first + at, h->cs.iso, n_iso, *cfg, d_scratch, d_scratch, *out, cc);
                else
                    hipLaunchKernelGGL(adh_feature_im_own_kernel<false>, dim3((unsigned)ng), dim3(ADH_WAVE), lds_pad, st, h->tims,
                                       p.d_recs_im + first + at, h->cs.iso, n_iso, *cfg, d_scratch, (unsigned char *)nullptr,
                                       *out, cc);
                HIP_TRY(hipGetLastError());
                h->im_stats[g] += ng;
                h->im_stats[ADH_IM_GROUPS + g] = std::max<int64_t>(h->im_stats[ADH_IM_GROUPS + g], (int64_t)lds);
                at += ng;
            }
        }
        if (rc != ADH_OK) return rc;
    }
    HIP_TRY(hipEventRecord(t.e2, st));
    h->timed.push_back(t);
    return ADH_OK;
}

// enqueue gather + feature kernels of one planned batch on `st`
int launch_scoring(adh_handle *h, Plan &p, const adh_scoring_config_t *cfg, adh_output_t *out, hipStream_t st) {
    if (h->timed.size() > 48) fold_timed(h, false);
    if (p.n == 0) return ADH_OK;
    if (!h->tims_staged && p.generic_over != 0) {
        // even the spill path keeps everything indexed by K * O and K in LDS (feat::Layout with spill = true): refused
        // before anything is launched or counted
        char buf[256];
        snprintf(buf, sizeof(buf),
                 "candidate needs %llu bytes of LDS on the spill path of the generic kernel (K=%llu O=%llu): exceeds the bound of %d bytes",
                 (unsigned long long)(p.generic_over >> 32), (unsigned long long)((p.generic_over >> 8) & 0xFFFFFFu),
                 (unsigned long long)(p.generic_over & 0xFFu), (int)ADH_GENERIC_LDS_LIMIT);
        return fail(ADH_ERR_UNSUPPORTED, buf);
    }
    const ImSwitches im_sw = h->tims_staged ? im_switches_from_env() : ImSwitches{};
    if (h->tims_staged) {
        const int rc = refuse_im(p, im_sw);
        if (rc != ADH_OK) return rc;
    }
    for (int c = 0; c < ADH_N_CLASSES; ++c) h->class_counts[c] += p.n_class[c];
    if (h->tims_staged) return launch_scoring_im(h, p, cfg, out, st, im_sw);
    if (cfg->collect_fragments && p.caps_all.k > out->top_k)
        return fail(ADH_ERR_INVALID_ARGUMENT, "output top_k smaller than config.top_k_fragments");
    int stop_phase = 0;
    if (const char *dbg = getenv("ADH_DEBUG_STOP_PHASE")) stop_phase = atoi(dbg);  // developer switch

    Caps gcaps = p.caps_all;
    if (const char *dbg = getenv("ADH_DEBUG_GATHER")) gcaps.stop_phase = atoi(dbg);
    const size_t g_lds = adh_gather_lds_bytes(gcaps, h->run.n_ms1_obs);
    if (g_lds > 160 * 1024) return fail(ADH_ERR_UNSUPPORTED, "library slice / MS1 tile too large for the gather kernel");
    int rc = ensure_scratch(h, p.scratch_bytes);
    if (rc != ADH_OK) return rc;
    unsigned char *d_scratch = static_cast<unsigned char *>(h->scratch_slab);

    adh_handle::Timed t;
    rc = get_event(h, &t.e0);
    if (rc == ADH_OK) rc = get_event(h, &t.e1);
    if (rc == ADH_OK) rc = get_event(h, &t.e2);
    if (rc != ADH_OK) return rc;
    const int32_t n_iso = h->cs.n_iso_cols;
    int64_t n_fused = 0;  // classes of the fused kernel come first in processing order
    for (int c = ADH_CLASS_FUSED0; c < ADH_CLASS_FAST2; ++c) n_fused += p.n_class[c];
    const char *only = getenv("ADH_DEBUG_ONLY");  // developer switch: "fast" / "generic" / "u" = fused kernels only
    const bool run_generic = !(only && (only[0] == 'f' || only[0] == 'u')), run_fast = !(only && only[0] == 'g');
    const bool fused_only = only && only[0] == 'u';
    HIP_TRY(hipEventRecord(t.e0, st));
    if (p.n > n_fused) {
        hipLaunchKernelGGL(adh_gather_kernel, dim3((unsigned)(p.n - n_fused)), dim3(ADH_WAVE), g_lds, st, h->run, h->d_lib,
                           p.d_recs + n_fused, *cfg, n_iso, d_scratch, *out, gcaps);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(t.e1, st));
    const unsigned per_block = ADH_WAVE / ADH_GS;
    if (n_fused > 0 && run_fast) {
        // per observation count: the shorter rows in one launch, the longest (more LDS; with one observation also
        // more registers than three wavefronts per SIMD leave: adh_fused.hip) in a second one
        FusedClasses fcs[4] = {};  // [2 * (observations - 1) + (long rows)]
        int64_t fblocks[4] = {0, 0, 0, 0};
        int64_t first = 0;
        for (int c = ADH_CLASS_FUSED0; c < ADH_CLASS_FAST2; ++c) {
            const int64_t nc = p.n_class[c];
            const int obs = (c - ADH_CLASS_FUSED0) / 7, fm = 8 + 4 * ((c - ADH_CLASS_FUSED0) % 7);
            // one observation: rows up to ADH_FUSED_FM3 cycles at three wavefronts per SIMD, longer ones at two;
            // two observations: ONE launch (round 5: rows of 32 cycles used to have their own - 190 wavefronts per
            // 47 000-row chunk that kept the GPU for a whole wavefront lifetime, 73 us; at two wavefronts per SIMD
            // the larger LDS block of FM = 32 costs no occupancy)
            const int which = obs == 0 ? (fm > ADH_FUSED_FM3 ? 1 : 0) : 2;
            FusedClasses &fc = fcs[which];
            if (nc > 0) {
                fc.first_block[fc.n] = (int32_t)fblocks[which];
                fc.first_cand[fc.n] = (int32_t)first;
                fc.n_cand[fc.n] = (int32_t)nc;
                fc.kind[fc.n] = c - ADH_CLASS_FUSED0;
                ++fc.n;
                fblocks[which] += (nc + per_block - 1) / per_block;
                fc.first_block[fc.n] = (int32_t)fblocks[which];
            }
            first += nc;
        }
        // tile width: 15 columns while lane 15 carries no isotope, 16 with four isotopes (adh_fused.hip)
        const bool wide = std::min<uint32_t>(cfg->top_k_isotopes, (uint32_t)n_iso) > 3;
        // (the launches of a chunk stay on ONE stream: side streams were measured and bring nothing)
#define ADH_LAUNCH_FUSED_TW(W, FM_MIN, FM_MAX, NO, TW)                                                                   \
    hipLaunchKernelGGL((adh_fused_kernel<FM_MIN, FM_MAX, NO, TW>), dim3((unsigned)fblocks[W]), dim3(ADH_WAVE), 0, st,    \
                       (FusedArgs{h->run, h->d_lib, p.d_recs, fcs[W], h->cs.iso, (int32_t)n_iso, *cfg, h->d_wtp, *out, (int32_t)stop_phase}))
#define ADH_LAUNCH_FUSED(W, FM_MIN, FM_MAX, NO)                                                 \
    if (fblocks[W] > 0) {                                                                       \
        if (wide) ADH_LAUNCH_FUSED_TW(W, FM_MIN, FM_MAX, NO, 16);                               \
        else ADH_LAUNCH_FUSED_TW(W, FM_MIN, FM_MAX, NO, ADH_FUSED_TW3);                         \
        HIP_TRY(hipGetLastError());                                                             \
    }
        ADH_LAUNCH_FUSED(0, 8, ADH_FUSED_FM3, 1)
        ADH_LAUNCH_FUSED(1, ADH_FUSED_FM3 + 4, 32, 1)
        ADH_LAUNCH_FUSED(2, 8, 32, 2)
#undef ADH_LAUNCH_FUSED
#undef ADH_LAUNCH_FUSED_TW
    }
    if (stop_phase != 2 && !fused_only) {
        int64_t first = n_fused;
        for (int c = ADH_CLASS_FAST2; c <= ADH_CLASS_GENERIC; ++c) {
            const bool wide_class = c >= ADH_CLASS_WIDE2 && c < ADH_CLASS_GENERIC;
            if (wide_class && run_fast && c == ADH_CLASS_WIDE2) {
                // the wide classes in two launches (adh_features_fast.hip): classes WIDE2 .. WIDE2 + 2 / WIDE1 .. WIDE1 + 2
                // (one candidate per wavefront) and their 32-lane twins MID2 .. / MID1 .., which follow each other in
                // the plan's order: the heavy bodies first, then the ones that fit three wavefronts per SIMD
                int64_t class_first[ADH_N_CLASSES];
                {
                    int64_t at = first;
                    for (int q = c; q < ADH_CLASS_GENERIC; ++q) class_first[q] = at, at += p.n_class[q];
                }
                for (int part = 0; part < 2; ++part) {
                    const int kinds = part == 0 ? ADH_WIDE_HEAVY : ADH_WIDE_LIGHT;
                    WideClasses wcs{};
                    int64_t blocks = 0;
                    for (int kind = 0; kind < 12; ++kind) {
                        const int j = kind % 6, two = kind / 6;
                        const int q = (j < 3 ? (two ? ADH_CLASS_WIDE2 : ADH_CLASS_WIDE1) : (two ? ADH_CLASS_MID2 : ADH_CLASS_MID1)) + j % 3;
                        const int64_t nq = p.n_class[q];
                        if (nq > 0 && ((kinds >> kind) & 1)) {
                            const int per = j < 3 ? 1 : 2;
                            wcs.first_block[wcs.n] = (int32_t)blocks;
                            wcs.first_cand[wcs.n] = (int32_t)(class_first[q] - n_fused);
                            wcs.n_cand[wcs.n] = (int32_t)nq;
                            wcs.kind[wcs.n] = kind;
                            ++wcs.n;
                            blocks += (nq + per - 1) / per;
                        }
                    }
                    wcs.first_block[wcs.n] = (int32_t)blocks;
                    if (blocks == 0) continue;
                    const CandRec *base = p.d_recs + n_fused;
                    const WideArgs wa{h->run, base, wcs, h->cs.iso, n_iso, *cfg, d_scratch, h->d_wtp, *out, (int32_t)stop_phase};
                    const dim3 grid((unsigned)blocks), wave(ADH_WAVE);
                    if (part == 0) hipLaunchKernelGGL((adh_feature_wide_kernel<ADH_WIDE_HEAVY>), grid, wave, 0, st, wa);
                    else hipLaunchKernelGGL((adh_feature_wide_kernel<ADH_WIDE_LIGHT>), grid, wave, 0, st, wa);
                    HIP_TRY(hipGetLastError());
                }
            }
            if (!wide_class && p.n_class[c] > 0 && (c == ADH_CLASS_GENERIC ? run_generic : run_fast)) {
                const CandRec *recs = p.d_recs + first;
                if (c == ADH_CLASS_GENERIC) {
                    // one launch per group of own layouts, each with the LDS of its largest candidate; the last group
                    // keeps its tile planes in the spill blocks of the scratch slab
                    int64_t at = 0;
                    for (int g = 0; g < ADH_GENERIC_GROUPS; ++g) {
                        const int64_t ng = p.n_generic[g];
                        if (ng == 0) continue;
                        const size_t lds = (size_t)p.lds_generic[g];
                        if (g == ADH_GENERIC_GROUP_SPILL)
                            hipLaunchKernelGGL(adh_feature_kernel<true>, dim3((unsigned)ng), dim3(ADH_WAVE), lds, st, h->run,
                                               recs + at, h->cs.iso, n_iso, *cfg, d_scratch, d_scratch, *out, (int32_t)stop_phase);
                        else
                            hipLaunchKernelGGL(adh_feature_kernel<false>, dim3((unsigned)ng), dim3(ADH_WAVE), lds, st, h->run,
                                               recs + at, h->cs.iso, n_iso, *cfg, d_scratch, (unsigned char *)nullptr, *out,
                                               (int32_t)stop_phase);
                        HIP_TRY(hipGetLastError());
                        h->generic_stats[g] += ng;
                        h->generic_stats[ADH_GENERIC_GROUPS + g] = std::max<int64_t>(h->generic_stats[ADH_GENERIC_GROUPS + g], (int64_t)lds);
                        at += ng;
                    }
                } else {
                    const unsigned blocks = (unsigned)((p.n_class[c] + per_block - 1) / per_block);
                    const int32_t nc = (int32_t)p.n_class[c];
#define ADH_LAUNCH_FAST(FM, NO)                                                                              \
    hipLaunchKernelGGL((adh_feature_fast_kernel<FM, NO>), dim3(blocks), dim3(ADH_WAVE), 0, st, h->run, recs, \
                       nc, h->cs.iso, n_iso, *cfg, d_scratch, h->d_wtp, *out, (int32_t)stop_phase)
                    switch (c) {
                        case ADH_CLASS_FAST2 + 0: ADH_LAUNCH_FAST(16, 2); break;
                        case ADH_CLASS_FAST2 + 1: ADH_LAUNCH_FAST(24, 2); break;
                        case ADH_CLASS_FAST2 + 2: ADH_LAUNCH_FAST(32, 2); break;
                        case ADH_CLASS_FAST1 + 0: ADH_LAUNCH_FAST(8, 1); break;
                        case ADH_CLASS_FAST1 + 1: ADH_LAUNCH_FAST(12, 1); break;
                        case ADH_CLASS_FAST1 + 2: ADH_LAUNCH_FAST(16, 1); break;
                        case ADH_CLASS_FAST1 + 3: ADH_LAUNCH_FAST(20, 1); break;
                        case ADH_CLASS_FAST1 + 4: ADH_LAUNCH_FAST(24, 1); break;
                        case ADH_CLASS_FAST1 + 5: ADH_LAUNCH_FAST(28, 1); break;
                        default: ADH_LAUNCH_FAST(32, 1); break;
                    }
#undef ADH_LAUNCH_FAST
                }
                HIP_TRY(hipGetLastError());
            }
            first += p.n_class[c];
        }
    }
    HIP_TRY(hipEventRecord(t.e2, st));
    h->timed.push_back(t);
    return ADH_OK;
}

int check_score_args(adh_handle *h, const adh_scoring_config_t *cfg, const adh_output_t *out) {
    if (cfg->top_k_fragments == 0 || cfg->top_k_isotopes == 0)
        return fail(ADH_ERR_INVALID_ARGUMENT, "top_k_fragments / top_k_isotopes must be > 0");
    if (out->top_k <= 0) return fail(ADH_ERR_INVALID_ARGUMENT, "output top_k must be > 0");
    if (h->tims_staged && h->tims.cycle_len > 1024)
        return fail(ADH_ERR_UNSUPPORTED, "ion-mobility cycles of more than 1024 frames are not supported");
    return ADH_OK;
}

int64_t pick_chunk(int64_t n, bool fine) {
    // rows per pipeline chunk.  Two regimes (round 5):
    //  * tables of >= 2 M rows (the one-GPU headline): chunks of 524288 rows - fewer, larger launches suit the fused
    //    kernel, and the un-overlapped first H2D / last D2H are a small share of the call.  3 M candidates, host -> host /
    //    kernels (round 3, two sweeps on one box): 196608 rows 37.9, 36.6 / 16.9 ms, 262144 35.0, 36.0 / 16.1, 393216
    //    36.7, 35.9 / 15.2, 524288 35.5, 36.0 / 14.7; 1048576 cost 2 ms of host -> host time (first and last copies)
    //  * smaller tables (the 375 000-row shards of an eight-GPU run, the batches of the optimisation loop): the copy-out
    //    is the longest stage (8.3 ns per row at 54 GB/s against 0.18 ms + 4.7 ns per row of kernels per chunk), so the call
    //    is as long as the wait for the FIRST copy-out plus every gap of the copy-out stream: about five chunks (sweeps of
    //    round 5, 375 000 rows: 3 chunks 5.1-5.5 ms, 4 parts 4.68, 5 4.57, 6 4.62, 7 4.76, 8 4.88, 10 5.36; 750 000 rows: 9.4 / 8.11 /
    //    8.11 / 8.4 / 8.9), none below ADH_CHUNK_MIN rows (below ~50 000 rows a chunk's kernels take longer than its copy-out and the stream
    //    waits for them).  Round 4 cut such a table in two or three (one short first chunk): the 375 000-row shard took
    //    5.1 ms = 0.65 ramp + 3.25 copies + 0.63 gap + 0.55 tail; see tools/bench_shard.py
    const int64_t big = 524288;
    if (const char *env = getenv("ADH_CHUNK")) {
        const int64_t target = std::max<int64_t>(atoll(env), 1024);
        const int64_t parts = (n + target - 1) / target;
        if (parts <= 1) return std::max<int64_t>(n, 1);
        return (n + parts - 1) / parts;
    }
    if (n >= 4 * big) {
        const int64_t parts = (n + big - 1) / big;
        return (n + parts - 1) / parts;
    }
    if (!fine) {
        // ion-mobility tables: a chunk is ~7 launches and the gather's pair lists, so fewer chunks win (configs[3],
        // 600 000 candidates: 18.4 ms host -> host in 3 chunks, 21.3 in 7): the rule of round 4 - chunks of 524288
        // rows, a table of 196608 rows and more in two at least
        int64_t parts = (n + big - 1) / big;
        if (parts < 2 && n >= 196608) parts = 2;
        if (parts <= 1) return std::max<int64_t>(n, 1);
        return (n + parts - 1) / parts;
    }
    int64_t want_parts = 5, min_rows = 40960;
    if (const char *env = getenv("ADH_CHUNK_PARTS")) want_parts = std::max<int64_t>(atoll(env), 1);
    if (const char *env = getenv("ADH_CHUNK_MIN")) min_rows = std::max<int64_t>(atoll(env), 1024);
    int64_t c = std::max(min_rows, (n + want_parts - 1) / want_parts);
    c = std::min(c, big);
    const int64_t parts = (n + c - 1) / c;
    if (parts <= 1) return std::max<int64_t>(n, 1);
    return (n + parts - 1) / parts;
}

}  // namespace

}  // extern "C"

namespace {
// The chunk boundaries of a host -> host call over n > 0 rows: chunk ci is rows [cut[ci], cut[ci + 1]).  A short first
// chunk (its H2D, plan and kernels are the un-overlapped ramp of the D2H-bound pipeline), then equal chunks of
// pick_chunk's length - of at most max_rows rows, where the caller sets a bound (> 0: the ion-mobility scratch fit,
// the 32-bit offsets of the compacted copy-outs) - and, for the packed mode (`packed`), a short last one.  Reads
// ADH_CHUNK, ADH_CHUNK_PARTS, ADH_CHUNK_MIN (pick_chunk), ADH_FIRST_CHUNK_DIV and ADH_LAST_CHUNK_DIV; no GPU.
std::vector<int64_t> chunk_cuts(int64_t n, bool ion_mobility, int64_t max_rows, bool packed) {
    int64_t chunk = pick_chunk(n, !ion_mobility);
    if (max_rows > 0 && max_rows < chunk) {  // (as many equal parts as the bound asks for)
        const int64_t parts = (n + max_rows - 1) / max_rows;
        chunk = (n + parts - 1) / parts;
    }
    std::vector<int64_t> cut{0};
    // a short first chunk: its copy-out starts early.  A quarter of a chunk - or half of one for a table of many
    // chunks, where the copy-out is what the call waits for and the first copy-out should cover the kernels of the
    // (full) second chunk: 3 M candidates 29.3 -> 28.6 ms; tables of two or three chunks lose with it
    // (ADH_FIRST_CHUNK_DIV fixes the divisor)
    const char *first_div_str = getenv("ADH_FIRST_CHUNK_DIV");
    const int first_div_env = first_div_str && atoi(first_div_str) > 0 ? atoi(first_div_str) : 0;
    // (tables of up to three chunks: no short first chunk - 48 000 rows 1.45 against 1.65 ms, 96 000 1.93 against 2.02)
    const int first_div = first_div_env ? first_div_env : (n >= 4 * chunk ? 2 : ((n > 3 * chunk || ion_mobility) ? 4 : 1));
    if (n > chunk) cut.push_back(std::max<int64_t>(chunk / first_div, 1));
    while (cut.back() < n) cut.push_back(std::min(n, cut.back() + chunk));
    if (packed && cut.size() >= 4) {
        // a short last chunk: the host team expands a block only once it has landed, so the team's work on the last
        // block comes after the last copy (ADH_LAST_CHUNK_DIV: the last chunk's share, 1 = no split)
        int last_div = 4;
        if (const char *env = getenv("ADH_LAST_CHUNK_DIV")) last_div = std::max(atoi(env), 1);
        const int64_t last = cut.back() - cut[cut.size() - 2];
        if (last_div > 1 && last / last_div >= 256) cut.insert(cut.end() - 1, n - last / last_div);
    }
    return cut;
}

}  // namespace

// The columns of the device tables that repeat the candidate table (precursor_idx, rank) or the library (per
// fragment slot) from fragment_lib_slot: the device-side twin of rebuild_host_rows, one thread per slot.
__global__ void adh_rebuild_columns_kernel(DevCands c, const LibRec *__restrict__ lib, DevOut out, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int top_k = out.top_k;
    if (t >= n * top_k) return;
    const int64_t i = t / top_k;
    const int j = (int)(t - i * top_k);
    const bool skip = c.flags && (c.flags[i] & ADH_FLAG_SKIP);
    const uint32_t p = skip ? 0u : c.precursor_idx[i];
    const uint8_t r = skip ? (uint8_t)0 : c.rank[i];
    if (j == 0) {
        out.precursor_idx[i] = p;
        out.rank[i] = r;
    }
    const uint16_t s = out.fragment_lib_slot[t];
    if (!s) return;  // (the tables were zeroed before the kernels ran)
    const LibRec l = lib[c.frag_start[i] + s - 1];
    out.fragment_precursor_idx[t] = p;
    out.fragment_rank[t] = r;
    out.fragment_mz_library[t] = l.mz_library;
    out.fragment_mz[t] = l.mz;
    out.fragment_position[t] = l.position;
    out.fragment_number[t] = l.number;
    out.fragment_type[t] = l.type;
    out.fragment_charge[t] = l.charge;
    out.fragment_loss_type[t] = l.loss_type;
}

#include "adh_copyout.hip"

extern "C" {

namespace {

// fill in what a host -> host call left out of the device tables (DevTables::partial) before somebody reads them
int materialise_tables(adh_handle *h) {
    if (h->last_tables < 0) return ADH_OK;
    DevTables &t = h->tables[h->last_tables];
    if (!t.partial) return ADH_OK;
    const int64_t n = h->last_rows;
    if (n > h->cs.n || !h->lib_staged)  // cannot happen through the ABI (replacing either settles the tables first)
        return fail(ADH_ERR_NOT_STAGED, "the candidate table / library the device tables were scored from is gone");
    if (n > 0) {
        HIP_TRY(hipSetDevice(h->device));
        adh_output_t view = t.view;
        view.n = n;
        const int64_t threads = n * (int64_t)view.top_k;
        hipLaunchKernelGGL(adh_rebuild_columns_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, h->cs.d,
                           h->d_lib, view, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    t.partial = false;
    return ADH_OK;
}

}  // namespace

int adh_upload_candidates(adh_handle_t *h, const adh_candidates_t *c) {
    if (!h || !c) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = check_candidate_args(h, c);
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = materialise_tables(h);  // the last call's tables are rebuilt from the candidate columns that go away now
    if (rc != ADH_OK) return rc;
    h->plan = Plan();
    h->cands_uploaded = false;
    h->sel.stage = std::min(h->sel.stage, 1);  // (a table assembled from a selection is replaced)
    rc = cand_reserve(h, c->n, c->n_isotope_cols);
    if (rc != ADH_OK) return rc;
    rc = cand_upload_range(h, c, 0, c->n, h->stream);
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cands_uploaded = true;
    return ADH_OK;
}

int adh_score_uploaded(adh_handle_t *h, const adh_scoring_config_t *cfg, adh_output_t *out, void *hip_stream) {
    if (!h || !cfg || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!h->cands_uploaded) return fail(ADH_ERR_NOT_STAGED, "no candidate table uploaded");
    if (out->n != h->cs.n) return fail(ADH_ERR_INVALID_ARGUMENT, "output rows != candidates");
    int rc = check_score_args(h, cfg, out);
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (h->cs.n == 0) return ADH_OK;
    hipStream_t st = (hipStream_t)hip_stream;  // NULL is HIP's default stream, taken literally
    // the plan of the uploaded table is kept until the table or the plan-relevant settings change
    Plan &p = h->plan;
    const PlanKey key = plan_key(cfg);
    if (!(p.ready && p.top_k_fragments == key.top_k_fragments && p.top_k_isotopes == key.top_k_isotopes &&
          p.fast_ok == key.fast_cfg && p.fused_ok == key.fused_cfg && p.wide_ok == key.wide_cfg && p.quant_all == key.quant_all &&
          p.spill_all == key.spill_all && p.im_spill_all == key.im_spill_all)) {
        p = Plan();
        rc = plan_enqueue(h, h->slots[0], cfg, 0, h->cs.n, st);
        if (rc == ADH_OK) rc = plan_finish(h, h->slots[0], cfg, 0, h->cs.n, p);
        if (rc != ADH_OK) return rc;
    }
    return launch_scoring(h, p, cfg, out, st);
}

int adh_get_stream(adh_handle_t *h, void **hip_stream) {
    if (!h || !hip_stream) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *hip_stream = (void *)h->stream;
    return ADH_OK;
}

int adh_synchronize(adh_handle_t *h) {
    if (!h) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ADH_OK;
}

int adh_kernel_time_ms(adh_handle_t *h, double *gather_ms, double *feature_ms, int64_t *launches, int reset) {
    if (!h || !gather_ms || !feature_ms || !launches) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    fold_timed(h, true);
    const int64_t n = h->n_timed;
    *gather_ms = n ? h->sum_gather_ms / (double)n : 0.0;
    *feature_ms = n ? h->sum_feature_ms / (double)n : 0.0;
    *launches = n;
    if (reset) {
        h->sum_gather_ms = h->sum_feature_ms = 0.0;
        h->n_timed = 0;
    }
    return ADH_OK;
}

int adh_plan_class_counts(adh_handle_t *h, int64_t *counts, int32_t reset) {
    if (!h || !counts) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int c = 0; c < ADH_N_CLASSES; ++c) {
        counts[c] = h->class_counts[c];
        if (reset) h->class_counts[c] = 0;
    }
    return ADH_OK;
}

int adh_generic_launch_stats(adh_handle_t *h, int64_t *stats, int32_t reset) {
    if (!h || !stats) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int i = 0; i < 2 * ADH_GENERIC_GROUPS; ++i) {
        stats[i] = h->generic_stats[i];
        if (reset) h->generic_stats[i] = 0;
    }
    return ADH_OK;
}

int adh_im_launch_stats(adh_handle_t *h, int64_t *stats, int32_t reset) {
    if (!h || !stats) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int i = 0; i < 2 * ADH_IM_GROUPS; ++i) {
        stats[i] = h->im_stats[i];
        if (reset) h->im_stats[i] = 0;
    }
    return ADH_OK;
}

int adh_im_launch_routes(int32_t k, int32_t o, int32_t s, int32_t f, int32_t i, const int64_t *n_class,
                         const adh_scoring_config_t *config, int32_t *layout, int32_t *launch) {
    if (!n_class || !config || !layout || !launch) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    Caps caps{};
    caps.k = k, caps.o = o, caps.s = s, caps.f = f, caps.i = i;
    const ImRoutes routes = im_launch_routes(caps, n_class, config, im_switches_from_env(), 0);
    for (int c = 0; c < ADH_N_CLASSES; ++c) layout[c] = routes.of[c].layout, launch[c] = routes.of[c].launch;
    return ADH_OK;
}

namespace {

// ion-mobility candidates reserve a scratch block sized for their dense tiles (116 KB at 38 scans x 29 cycles,
// although ~1 % of it is touched): *max_rows bounds a chunk so that the slab stays within a third of the free device
// memory (0: no bound).  Tile sizes from the host columns; K <= top_k fragments, 3 observations assumed.
// (`cells_known` > 0: the largest tile of a table assembled on the device, whose columns the host does not hold)
int im_chunk_bound(adh_handle *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg, int64_t *max_rows,
                   int64_t cells_known = 0) {
    *max_rows = 0;
    int64_t cells = std::max<int64_t>(cells_known, 1);
    for (int64_t i = 0; i < c->n && cells_known <= 0; ++i) {
        const int64_t S = std::max<int64_t>(c->scan_stop[i] - c->scan_start[i], 1);
        const int64_t F = std::max<int64_t>((c->frame_stop[i] - c->frame_start[i]) / std::max(h->tims.cycle_len, 1) + 1, 1);
        cells = std::max(cells, S * F);
    }
    const int64_t k_max = std::max<int64_t>(std::min<int64_t>(cfg->top_k_fragments, 64), 1);
    const uint64_t block = (uint64_t)cells * 8 * (uint64_t)(k_max * 3 + 4) + 4096;
    if (h->im_scratch_budget == 0) {  // (asked once per staged run: hipMemGetInfo takes ~2 ms)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            h->im_scratch_budget = std::max<uint64_t>((free_b + h->scratch_slab_bytes) / 3, 1ull << 30);
    }
    if (h->im_scratch_budget) {
        const uint64_t budget = h->im_scratch_budget;
        if (block > budget)
            return fail(ADH_ERR_UNSUPPORTED, "one ion-mobility candidate's tiles exceed a third of the free device memory");
        *max_rows = (int64_t)std::max<uint64_t>(budget / block, 64);  // (the budget holds, down to 64 rows per chunk)
    }
    return ADH_OK;
}

// a call that fails half way leaves no tables behind (a reader would rebuild columns of a half-filled table), and its
// events go back to the pool.  The one place that synchronises the device and clears the error after a failure: the
// copy-out mode is declared behind it, so its team is stopped and joined first.
struct PipelineUnwind {
    adh_handle *h;
    DevTables &tab;
    std::vector<hipEvent_t> &events;
    std::vector<hipEvent_t> &aux;
    bool ok = false;
    ~PipelineUnwind() {
        for (std::vector<hipEvent_t> *list : {&events, &aux}) {
            h->free_events.insert(h->free_events.end(), list->begin(), list->end());
            list->clear();
        }
        if (!ok) {
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            h->last_tables = -1;
            h->last_rows = 0;
            tab.partial = false;
        }
    }
};

// the host -> host pipeline behind adh_score_candidates (padded tables into `out`) and adh_score_candidates_compact
// (`cop` set: `out` only carries n and top_k, the compacted columns go to `cop`) and adh_score_candidates_resident
// (`resident`: `out` only carries n and top_k, nothing is copied back).  This is the schedule of the three streams;
// how the results leave the device is the copy-out mode's part (adh_copyout.hip).  `device_cands`
// (adh_score_selected_resident): the candidate columns are in the handle's slab already (adh_assemble_selected wrote
// them there), `c` only carries n and n_isotope_cols, and nothing is uploaded.
int score_pipeline(adh_handle_t *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg, adh_output_t *out,
                   adh_compact_output_t *cop, bool resident = false, bool device_cands = false) {
    if (!h || !c || !cfg || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (out->n != c->n) return fail(ADH_ERR_INVALID_ARGUMENT, "output rows != candidates");
    adh_candidates_t shape_only = *c;  // (what check_candidate_args looks at when the columns are on the device)
    shape_only.n = 0;
    int rc = check_candidate_args(h, device_cands ? &shape_only : c);
    if (rc == ADH_OK && c->n > 0x7FFFFFFFll) rc = fail(ADH_ERR_UNSUPPORTED, "more than 2^31 candidates in one batch");
    if (rc == ADH_OK) rc = check_score_args(h, cfg, out);
    if (rc != ADH_OK) return rc;
    for (int i = 0; i < kNumOutFields && !cop && !resident; ++i)
        if (!kOutFields[i].optional && *out_member(out, kOutFields[i]) == nullptr)
            return fail(ADH_ERR_INVALID_ARGUMENT, "output buffer is NULL");
    HIP_TRY(hipSetDevice(h->device));
    PipelineTrace trace;  // developer switch ADH_DEBUG_TIMING: stage times to stderr
    const int64_t n = c->n;
    const int top_k = out->top_k;
    h->plan = Plan();            // the resident table (adh_upload_candidates) is replaced
    h->cands_uploaded = false;
    h->acc_live = false;         // ... and so are accumulated tables (adh_score_candidates_resident_append)
    h->acc_rows = 0;
    if (device_cands && (h->sel.stage != 2 || h->cs.n != n || h->cs.n_iso_cols != c->n_isotope_cols))
        return fail(ADH_ERR_NOT_STAGED, "no table assembled from a selection in the candidate slab");
    if (!device_cands) h->sel.stage = std::min(h->sel.stage, 1);  // (the slab's columns are replaced)
    rc = cand_reserve(h, n, c->n_isotope_cols);  // (the same rows and isotope columns: the same layout, nothing moves)
    if (rc != ADH_OK) return rc;
    if (device_cands) h->cs.d.flags = h->cs.flags;
    auto cand_upload = [&](int64_t a, int64_t b, hipStream_t st) {
        return device_cands ? (int)ADH_OK : cand_upload_range(h, c, a, b, st);
    };
    // device tables: with a communicator attached the layout is padded to the largest shard and
    // double-buffered (the all-gather of call i overlaps call i + 1)
    if (h->comm_attached() && n > h->comm_rows)
        return fail(ADH_ERR_INVALID_ARGUMENT,
                    "more candidates than max_rows_per_rank of adh_comm_init: the ranks would disagree on the table layout");
    const int slot = h->comm_attached() ? (h->table_slot ^= 1) : 0;
    rc = comm_wait_slot(h, slot);
    if (rc != ADH_OK) return rc;
    rc = ensure_tables(h, slot, std::max<int64_t>(n, h->comm_attached() ? h->comm_rows : 0), top_k);
    if (rc != ADH_OK) return rc;
    DevTables &tab = h->tables[slot];
    h->last_tables = slot;
    h->last_rows = n;
    {
        const double t_s = trace.now();
        const bool was = g_big_free.load();
        settle_copy_path(h);
        if (trace.timing && was) fprintf(stderr, "[adh] copy path settled in %.1f ms\n", trace.now() - t_s);
    }
    if (cop) cop->n_rows = cop->n_slots = 0;
    h->tables_current = false;
    if (n == 0) {
        rc = comm_gather_slot(h, slot);
        h->tables_current = rc == ADH_OK;
        return rc;
    }
    std::vector<hipEvent_t> chunk_done, tot_ready;  // (events of the copy-out mode, per chunk)
    PipelineUnwind unwind{h, tab, chunk_done, tot_ready};
    adh_output_t dev = tab.view;
    dev.n = n;
    hipStream_t sk = h->stream, si = h->stream_in;
    HIP_TRY(hipMemsetAsync(tab.base, 0, tab.used, sk));
    tab.partial = false;

    // rebuildable columns: not copied back, rebuilt on the host from fragment_lib_slot (see kOutFields)
    const bool rebuild = !cop && !resident && h->h_lib.size() == (size_t)h->n_lib && !getenv("ADH_DEBUG_COPY_ALL") && host_rebuild_pays();
    // compacted copy-out of the fragment tables (see adh_pack_rows_kernel, compact_copy_out_pays)
    const bool compact_wanted = rebuild && top_k <= 65535 && compact_copy_out_pays(n);
    // chunk boundaries: at most max_rows rows per chunk
    int64_t max_rows = 0;
    if (h->tims_staged) {
        rc = im_chunk_bound(h, c, cfg, &max_rows, device_cands ? h->sel.im_cells : 0);
        if (rc != ADH_OK) return rc;
    }
    if (cop || compact_wanted) {  // (a chunk's slot offsets are 32-bit words of the packed count)
        const int64_t fits_32 = std::max<int64_t>((int64_t)(0xFFFFFFFFull / (uint64_t)top_k) - 1, 1);
        max_rows = max_rows ? std::min(max_rows, fits_32) : fits_32;
    }
    const std::vector<int64_t> cut = chunk_cuts(n, h->tims_staged, max_rows, compact_wanted);
    const int64_t n_chunks = (int64_t)cut.size() - 1;
    const bool compact = compact_wanted && n_chunks <= 4096;
    adh_output_t dev_k = dev;  // what the kernels write
    if ((rebuild || cop || resident) && !getenv("ADH_DEBUG_WRITE_ALL")) {
        // ... and the kernels need not write them either: nobody on the host waits for them, and a reader of the
        // device tables (adh_get_device_tables, the resident FDR stage) gets them filled in on demand
        for (int i = 0; i < kNumOutFields; ++i) {
            const OutFieldDesc &f = kOutFields[i];
            if (!f.wire && f.member != offsetof(adh_output_t, stat_matched_peaks)) *out_member(&dev_k, f) = nullptr;
        }
        tab.partial = true;
    }
    const CopyOut call(h, c, dev, cut, chunk_done, tot_ready, trace);
    std::unique_ptr<CopyOut> copy_out;  // (behind `unwind`: a failed call joins its team before the device is synchronised)
    if (resident) copy_out.reset(new CopyOut(call));
    else if (cop) copy_out.reset(new OperatorCopyOut(call, cop));
    else if (compact) copy_out.reset(new PackedCopyOut(call, out));
    else copy_out.reset(new PlainCopyOut(call, out, rebuild));
    rc = copy_out->prepare();
    if (rc != ADH_OK) return rc;
    trace.t_1 = trace.now();
    // The copy-in stream, in order: columns(0) plan(0) | columns(1) plan(1) | columns(2) | plan(2) | columns(3 .. last)
    // | plan(3) ...: every chunk up to 2 goes up just ahead of its plan, ALL later rows in one burst behind the plan of
    // chunk 2 (one H2D per column).  One burst, because uploads of every chunk beside the copy-outs slowed those down
    // four-fold (round 3; the copy engines are shared); behind plan(2), because a plan queued behind the burst waits
    // for all of it: with the burst behind plan(1) the kernels of chunk 2 started 1.4 - 1.7 ms after those of chunk 1
    // had ended and the copy-out had a hole of 1.15 ms (profiles/headline_pipeline.json, `before`).  The burst
    // overlaps the copy-out of chunks 0 and 1 in both orders: that copy runs at 47 - 49 instead of 56 GB/s.
    // plan(3) is such a plan, too: on the headline the burst (2.25 M rows, 2.8 ms) ends and plan(3) (0.3 ms) starts as
    // the kernels of chunk 2 end, and in most calls the scoring stream then idles 0.5 - 0.8 ms in front of chunk 3.
    // Measured and dropped: only the columns of chunk 3 in front of plan(3) and the rows of chunks 4 .. last on a
    // stream of their own, behind plan(2).  The scoring stream's hole closes (span 14.4 - 14.5 ms instead of 14.4 -
    // 15.0), but the block of chunk 1 then waits for that upload on the copy engines - its copy starts 1.5 ms later -
    // and the step takes 18.8 - 21.5 ms instead of 18.3 - 19.6 (profiles/scoring_stream_chunks.json, `split_burst`).
    trace.mark_start(si);
    rc = cand_upload(0, cut[1], si);
    trace.mark_plan(si);
    if (rc == ADH_OK) rc = plan_enqueue(h, h->slots[0], cfg, 0, cut[1], si);
    trace.mark_plan(si);
    if (rc == ADH_OK && n_chunks > 1) rc = cand_upload(cut[1], cut[2], si);
    if (rc != ADH_OK) return rc;
    // the host teams start now that the device has work: started in front of the first copy-in, the 16 threads made
    // the call's set-up 0.4 - 0.5 ms instead of 0.07 - 0.10 (profiles/headline_pipeline.json, `setup_ms`)
    copy_out->start_team();
    for (int64_t ci = 0; ci < n_chunks; ++ci) {
        const int64_t a = cut[(size_t)ci], b = cut[(size_t)ci + 1];
        const int ps = (int)(ci & 1);
        if (ci + 1 < n_chunks) {
            // plan of the next chunk: the other plan slot is free once the kernels of chunk ci - 1 are done
            const int64_t a2 = b, b2 = cut[(size_t)ci + 2];
            if (ci >= 1) HIP_TRY(hipStreamWaitEvent(si, h->ev_k[ps ^ 1], 0));
            trace.mark_plan(si);  // (behind the wait: the plan's own time)
            rc = plan_enqueue(h, h->slots[ps ^ 1], cfg, a2, b2 - a2, si);
            trace.mark_plan(si);
            // (the rows of chunk 2 behind the plan of chunk 1, ALL later rows behind the plan of chunk 2: see above)
            if (rc == ADH_OK && ci == 0 && n_chunks > 2) rc = cand_upload(cut[2], cut[3], si);
            if (rc == ADH_OK && ci == 1 && n_chunks > 3) rc = cand_upload(cut[3], n, si);
            if (rc != ADH_OK) return rc;
        }
        Plan p;
        rc = plan_finish(h, h->slots[ps], cfg, a, b - a, p);
        trace.plan_read();
        trace.mark(sk);
        if (rc == ADH_OK) rc = launch_scoring(h, p, cfg, &dev_k, sk);
        trace.mark(sk);
        if (rc == ADH_OK) rc = copy_out->pack(ci);
        if (rc != ADH_OK) return rc;
        trace.mark(sk);
        trace.chunk_enqueued();
        HIP_TRY(hipEventRecord(h->ev_k[ps], sk));
        rc = copy_out->copy_out(ci);
        if (rc != ADH_OK) return rc;
    }
    rc = copy_out->flush();
    if (rc != ADH_OK) return rc;
    trace.t_2 = trace.now();
    rc = comm_gather_slot(h, slot);  // after the last chunk's kernels; overlaps the remaining D2H
    if (rc == ADH_OK) rc = copy_out->finish();
    if (rc != ADH_OK) {
        unwind.ok = h->tables_current = copy_out->tables_stand;  // (the operator mode's overflow: the device tables are complete)
        return rc;
    }
    hipError_t e = hipStreamSynchronize(sk);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream_out);
    if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("scoring pipeline: ") + hipGetErrorString(e));
    trace.report(cut, chunk_done, compact);
    unwind.ok = true;
    h->tables_current = true;
    return ADH_OK;
}
}  // namespace

int adh_score_candidates(adh_handle_t *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg,
                         adh_output_t *out) {
    return score_pipeline(h, c, cfg, out, nullptr);
}

int adh_score_candidates_compact(adh_handle_t *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg,
                                 adh_compact_output_t *cop) {
    if (!h || !c || !cfg || !cop) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (cop->top_k <= 0 || cop->rows_capacity < 0 || cop->slots_capacity < 0)
        return fail(ADH_ERR_INVALID_ARGUMENT, "compact output: top_k / capacities");
    if (cop->top_k > 255)  // (a row's number of filled slots travels as one byte)
        return fail(ADH_ERR_INVALID_ARGUMENT, "compact output: top_k above 255");
    if (h->h_lib.size() != (size_t)h->n_lib)  // (the team reads the library columns from the host copy)
        return fail(ADH_ERR_NOT_STAGED, "compact output: no host copy of the staged library");
    adh_output_t shape{};
    shape.n = c->n;
    shape.top_k = cop->top_k;
    return score_pipeline(h, c, cfg, &shape, cop);
}

int adh_table_layout(int64_t rows, int32_t top_k, int32_t capacity, adh_table_field_t *fields, int32_t *n_fields,
                     uint64_t *total_bytes, uint64_t *wire_bytes) {
    if (rows < 0 || top_k <= 0 || !n_fields) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_table_layout: bad argument");
    *n_fields = kNumOutFields;
    size_t wire = 0;
    const size_t total = layout_tables(nullptr, rows, top_k, nullptr, &wire);
    if (total_bytes) *total_bytes = total;
    if (wire_bytes) *wire_bytes = wire;
    if (!fields) return ADH_OK;
    if (capacity < kNumOutFields) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_table_layout: field array too short");
    size_t off = 0;
    for (int i = 0; i < kNumOutFields; ++i) {
        const OutFieldDesc &f = kOutFields[i];
        adh_table_field_t &o = fields[i];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", f.name);
        o.offset = off;
        o.row_elems = (uint32_t)(f.per_row < 0 ? top_k : f.per_row);
        o.elem_bytes = (uint32_t)f.elem;
        o.wire = f.wire ? 1 : 0;
        off += ((size_t)rows * out_row_bytes(f, top_k) + 255) / 256 * 256;
    }
    return ADH_OK;
}

int adh_get_device_tables(adh_handle_t *h, adh_output_t *device_view) {
    if (!h || !device_view) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h->last_tables < 0) return fail(ADH_ERR_NOT_STAGED, "no adh_score_candidates call has filled the device tables");
    const int rc = materialise_tables(h);
    if (rc != ADH_OK) return rc;
    *device_view = h->tables[h->last_tables].view;
    device_view->n = h->last_rows;
    return ADH_OK;
}

int adh_debug_get_dense(adh_handle_t *h, int64_t frame_start, int64_t frame_stop, int64_t scan_start, int64_t scan_stop,
                        const float *mz_query, int32_t n_query, float mass_tolerance, float quad_lo, float quad_hi,
                        float *dense, int64_t dense_capacity, int32_t *obs_out, int32_t *n_obs, int32_t *n_scans,
                        int32_t *n_cycles) {
    if (!h || !mz_query || !dense || !obs_out || !n_obs || !n_scans || !n_cycles)
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!h->run_staged && !h->tims_staged) return fail(ADH_ERR_NOT_STAGED, "no run staged");
    if (n_query < 1 || n_query > 4096) return fail(ADH_ERR_INVALID_ARGUMENT, "n_query must be in 1..4096");
    // The kernels sort a candidate's fragments by m/z before they build the windows, as scoring and selection do in
    // the reference; get_dense itself walks the list as given and never steps back.  The two agree on ascending
    // lists only, and no caller of the gather produces another one: refuse it instead of answering for another order.
    for (int k = 1; k < n_query; ++k)
        if (!(mz_query[k] >= mz_query[k - 1])) return fail(ADH_ERR_INVALID_ARGUMENT, "mz_query must ascend");
    HIP_TRY(hipSetDevice(h->device));
    const bool im = h->tims_staged;
    const int L = im ? h->tims.cycle_len : h->run.cycle_len;
    const int z = im ? h->tims.zeroth : 0;
    const int64_t n_fr = im ? h->tims.n_frames : h->run.n_spectra;
    if (frame_start < z || frame_stop < frame_start || frame_stop > n_fr || (frame_start - z) % L != 0)
        return fail(ADH_ERR_INVALID_ARGUMENT, "frame limits outside the staged run / not on a cycle boundary");
    const int K = n_query;
    const int F = (int)((frame_stop - z) / L - (frame_start - z) / L);
    const int S = im ? (int)(scan_stop - scan_start) : 1;
    if (im && (scan_start < 0 || scan_stop < scan_start || scan_stop > h->tims.scan_max))
        return fail(ADH_ERR_INVALID_ARGUMENT, "scan limits outside the staged run");
    // observations: the quadrupole test of get_dense (alpharaw_jit.py:19-50 / bruker_jit.py:315-350)
    const double *cyc = h->h_cycle.data();
    std::vector<uint16_t> obs;
    if (!im) {
        for (int row = 0; row < L; ++row)
            if ((double)quad_lo <= cyc[2 * row + 1] && (double)quad_hi >= cyc[2 * row]) obs.push_back((uint16_t)row);
    } else {
        std::vector<uint8_t> seen((size_t)L, 0);
        for (int fr = 0; fr < L; ++fr)
            for (int64_t sc = scan_start; sc < scan_stop; ++sc) {
                const int64_t rowi = (int64_t)fr * h->tims.scan_max + sc;
                if ((double)quad_lo <= cyc[2 * rowi + 1] && (double)quad_hi >= cyc[2 * rowi]) seen[(size_t)h->h_dpc[(size_t)rowi]] = 1;
            }
        for (int v = 0; v < L; ++v)
            if (seen[(size_t)v]) obs.push_back((uint16_t)v);
    }
    const int O = (int)obs.size();
    if (O > ADH_MAX_OBS) return fail(ADH_ERR_UNSUPPORTED, "the query overlaps more than 8 cycle rows");
    *n_obs = O;
    *n_scans = S;
    *n_cycles = std::max(F, 0);
    for (int o = 0; o < O; ++o) obs_out[o] = obs[(size_t)o];
    const int64_t need = 2ll * K * O * S * std::max(F, 0);
    if (need > dense_capacity) return fail(ADH_ERR_INVALID_ARGUMENT, "dense buffer too small");
    for (int64_t i = 0; i < need; ++i) dense[i] = 0.0f;
    if (O == 0 || F <= 0 || S <= 0) return ADH_OK;

    // a one-precursor library whose fragments are the query (all kept: distinct descending intensities)
    std::vector<LibRec> lib((size_t)K);
    for (int k = 0; k < K; ++k) {
        memset(&lib[(size_t)k], 0, sizeof(LibRec));
        lib[(size_t)k].mz_library = lib[(size_t)k].mz = mz_query[k];
        lib[(size_t)k].intensity = (float)(K - k);
        lib[(size_t)k].cardinality = 1;
    }
    adh_scoring_config_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.collect_fragments = 1;
    cfg.top_k_fragments = (uint32_t)K;
    cfg.top_k_isotopes = 1;
    cfg.reference_channel = -1;
    cfg.quant_window = 3;
    cfg.precursor_mz_tolerance = 10.0f;
    cfg.fragment_mz_tolerance = mass_tolerance;
    Caps caps{K, O, F, 1, K, ADH_DEBUG_DENSE, S, 0, quad_lo, quad_hi};
    const uint64_t sbytes = im ? adh_im_scratch_bytes((uint32_t)K, O, S, F, 1, 0) : adh_scratch_bytes((uint32_t)K, O, F, 1);
    DeviceBuffers tmp;
    const LibRec *d_lib = nullptr;
    int rc = upload(tmp, lib.data(), (int64_t)K, &d_lib, h->stream);
    unsigned char *d_scr = nullptr;
    uint32_t *d_small = nullptr;  // precursor_idx[1] + rank[1] of the kernel's bookkeeping writes
    if (rc == ADH_OK) {
        hipError_t e = hipMalloc((void **)&d_scr, sbytes);
        if (e == hipSuccess) tmp.ptrs.push_back(d_scr);
        if (e == hipSuccess) e = hipMalloc((void **)&d_small, 64);
        if (e == hipSuccess) tmp.ptrs.push_back(d_small);
        if (e != hipSuccess) rc = fail(ADH_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    adh_output_t out;
    memset(&out, 0, sizeof(out));
    out.n = 1;
    out.top_k = K;
    out.precursor_idx = d_small;
    out.rank = reinterpret_cast<uint8_t *>(d_small + 4);
    hipError_t e = hipSuccess;
    if (rc == ADH_OK && !im) {
        CandRec r;
        memset(&r, 0, sizeof(r));
        r.frag_stop = (uint32_t)K;
        r.frame_start = (int32_t)frame_start;
        r.frame_stop = (int32_t)frame_stop;
        r.frame_center = (int32_t)frame_start;
        r.scan_stop = 1;
        r.precursor_mz = 500.0f;
        r.charge = 1;
        r.n_obs = (uint8_t)O;
        for (int o = 0; o < O; ++o) r.obs[o] = obs[(size_t)o];
        r.k_cap = (uint32_t)K;
        const CandRec *d_rec = nullptr;
        rc = upload(tmp, &r, 1, &d_rec, h->stream);
        const size_t lds = adh_gather_lds_bytes(caps, h->run.n_ms1_obs);
        if (rc == ADH_OK && lds > 160 * 1024) rc = fail(ADH_ERR_UNSUPPORTED, "query too large for the gather kernel's LDS");
        if (rc == ADH_OK) {
            hipLaunchKernelGGL(adh_gather_kernel, dim3(1), dim3(ADH_WAVE), lds, h->stream, h->run, d_lib, d_rec, cfg, 1,
                               d_scr, out, caps);
            e = hipGetLastError();
        }
    } else if (rc == ADH_OK) {
        CandRecIM r;
        memset(&r, 0, sizeof(r));
        r.frag_stop = (uint32_t)K;
        r.frame_start = (int32_t)frame_start;
        r.frame_stop = (int32_t)frame_stop;
        r.frame_center = (int32_t)frame_start;
        r.scan_start = (int32_t)scan_start;
        r.scan_stop = (int32_t)scan_stop;
        r.scan_center = (int32_t)scan_start;
        r.precursor_mz = 500.0f;
        r.charge = 1;
        r.n_obs = (uint8_t)O;
        for (int o = 0; o < O; ++o) r.obs[o] = obs[(size_t)o];
        r.k_cap = (uint32_t)K;
        const CandRecIM *d_rec = nullptr;
        rc = upload(tmp, &r, 1, &d_rec, h->stream);
        const size_t lds = adh_gather_im_lds_bytes(caps);
        if (rc == ADH_OK && lds > 160 * 1024) rc = fail(ADH_ERR_UNSUPPORTED, "query too large for the gather kernel's LDS");
        if (rc == ADH_OK) {
            hipLaunchKernelGGL(adh_gather_im_kernel, dim3(1), dim3(ADH_WAVE), lds, h->stream, h->tims, d_lib, d_rec, cfg, 1,
                               d_scr, out, caps);
            e = hipGetLastError();
        }
    }
    std::vector<unsigned char> host((size_t)sbytes);
    if (rc == ADH_OK && e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (rc == ADH_OK && e == hipSuccess) e = hipMemcpy(host.data(), d_scr, sbytes, hipMemcpyDeviceToHost);
    tmp.release();
    if (rc != ADH_OK) return rc;
    if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("adh_debug_get_dense: ") + hipGetErrorString(e));
    const uint32_t k_sel = *reinterpret_cast<const uint32_t *>(host.data());
    if ((int)k_sel != K) return fail(ADH_ERR_HIP, "gather kernel did not keep every query fragment");
    const float2 *cells = reinterpret_cast<const float2 *>(host.data() + adh_scratch_frag_off((uint32_t)K));
    const int64_t plane = (int64_t)K * O * S * F;
    for (int k = 0; k < K; ++k)
        for (int o = 0; o < O; ++o)
            for (int sc = 0; sc < S; ++sc)
                for (int f = 0; f < F; ++f) {
                    const float2 v = im ? cells[(((int64_t)k * O + o) * S + sc) * F + f] : cells[((int64_t)o * F + f) * K + k];
                    const int64_t at = (((int64_t)k * O + o) * S + sc) * F + f;
                    dense[at] = v.x;
                    dense[plane + at] = v.y;
                }
    return ADH_OK;
}

int adh_zero_device_tables(adh_handle_t *h, void *hip_stream) {
    if (!h) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL handle");
    if (h->last_tables < 0) return fail(ADH_ERR_NOT_STAGED, "no device tables yet");
    HIP_TRY(hipSetDevice(h->device));
    DevTables &t = h->tables[h->last_tables];
    HIP_TRY(hipMemsetAsync(t.base, 0, t.used, (hipStream_t)hip_stream));
    return ADH_OK;
}

int adh_copy_to_host(adh_handle_t *h, void *dst, const void *src_device, uint64_t bytes) {
    if (!h || (bytes > 0 && (!dst || !src_device))) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (bytes > 0) HIP_TRY(hipMemcpy(dst, src_device, (size_t)bytes, hipMemcpyDeviceToHost));
    h->d2h_bytes += bytes;
    return ADH_OK;
}

int adh_transfer_counters(adh_handle_t *h, uint64_t *d2h_bytes, int reset) {
    if (!h || !d2h_bytes) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *d2h_bytes = h->d2h_bytes;
    if (reset) h->d2h_bytes = 0;
    return ADH_OK;
}

int adh_host_alloc(void **ptr, uint64_t bytes) {
    if (!ptr) return fail(ADH_ERR_INVALID_ARGUMENT, "ptr is NULL");
    *ptr = nullptr;
    HIP_TRY(hipHostMalloc(ptr, std::max<size_t>((size_t)bytes, 64), hipHostMallocPortable));
    return ADH_OK;
}

int adh_trim_device_cache(void) {
    const hipError_t e = adh_dev_trim();
    if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("adh_trim_device_cache: ") + hipGetErrorString(e));
    return ADH_OK;
}

int adh_host_threads(int64_t n_rows, int32_t *threads, int32_t *cpu_budget) {
    if (threads) *threads = host_threads_for(n_rows);
    if (cpu_budget) *cpu_budget = host_cpu_budget();
    return ADH_OK;
}

int adh_chunk_cuts(int64_t n_rows, int32_t ion_mobility, int64_t max_rows, int32_t packed, int64_t *cuts, int64_t capacity,
                   int64_t *n_cuts) {
    if (n_rows <= 0 || !n_cuts || capacity < 0 || (capacity > 0 && !cuts))
        return fail(ADH_ERR_INVALID_ARGUMENT, "adh_chunk_cuts: bad argument");
    const std::vector<int64_t> cut = chunk_cuts(n_rows, ion_mobility != 0, max_rows, packed != 0);
    *n_cuts = (int64_t)cut.size();  // (what the caller needs, should the array be too short)
    if (*n_cuts > capacity) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_chunk_cuts: capacity too small (n_cuts says what is needed)");
    std::copy(cut.begin(), cut.end(), cuts);
    return ADH_OK;
}

int adh_host_free(void *ptr) {
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return ADH_OK;
}

// dst[i] = src[idx[i]] for arrays of reference-counted CPython object pointers (NumPy dtype=object), on several
// threads: the precursor-side string columns of the features frame (proteins, genes, sequence, mods, mod_sites) are
// 13.5 M such pointers per 3 M candidates and NumPy gathers them on one thread.  The CALLER HOLDS THE GIL for the
// whole call (ctypes.PyDLL): nothing else can touch a reference count meanwhile, the threads here only add to them,
// atomically (ob_refcnt is the first word of an object in CPython <= 3.11; alphadia_amd/runtime.py checks that on a
// probe object before it uses this).  dst must be fresh: every entry NULL or `fill` (np.empty gives an object array
// filled with references to None), whose reference count gives back what the gathered pointers replace.
int adh_host_take_objects(void **dst, void *const *src, const int64_t *idx, int64_t n, int64_t n_src, void *fill,
                          int32_t threads) {
    if ((!dst || !src || !idx) && n > 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_host_take_objects: NULL argument");
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n / 65536));
    std::atomic<int> bad{0};
    auto work = [&](int w) {
        const int64_t a = n * w / T, b = n * (w + 1) / T;
        intptr_t replaced = 0;
        // runs of one object (the candidates of a precursor follow each other; a column of empty strings is ONE
        // interned object) are counted and added once: sixteen threads adding to one reference count one by one spend
        // their time passing its cache line around (measured: the gather of five columns slower than NumPy's)
        void *run = nullptr;
        intptr_t run_len = 0;
        for (int64_t i = a; i < b; ++i) {
            const int64_t k = idx[i];
            void *const old = dst[i];
            if ((uint64_t)k >= (uint64_t)n_src || (old != nullptr && old != fill)) {
                bad.store(1, std::memory_order_relaxed);
                continue;
            }
            void *o = src[k];
            if (o != run) {
                if (run && run_len) __atomic_fetch_add(reinterpret_cast<intptr_t *>(run), run_len, __ATOMIC_RELAXED);
                run = o;
                run_len = 0;
            }
            ++run_len;
            dst[i] = o;
            replaced += old != nullptr;
        }
        if (run && run_len) __atomic_fetch_add(reinterpret_cast<intptr_t *>(run), run_len, __ATOMIC_RELAXED);
        if (replaced) __atomic_fetch_sub(reinterpret_cast<intptr_t *>(fill), replaced, __ATOMIC_RELAXED);
    };
    std::vector<std::thread> team;
    for (int w = 1; w < T; ++w) {
        try {
            team.emplace_back(work, w);
        } catch (const std::system_error &) {
            for (int v = w; v < T; ++v) work(v);
            break;
        }
    }
    work(0);
    for (std::thread &t : team) t.join();
    if (bad.load()) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_host_take_objects: index out of range or dst not fresh");
    return ADH_OK;
}
