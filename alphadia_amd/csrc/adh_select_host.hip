// adh_select_host.hip - host side of candidate selection: adh_select_candidates, adh_select_time_ms and the driver
// that adh_select_candidates_resident (adh_select_handover.hip) shares with them.  One driver per run layout
// (AlphaRaw: adh_select.hip, ion mobility: adh_select_im.hip) around one description of the selection slab, one set
// of switches, one stage timer and one end of a call; what is a decision and not plumbing is adh_select_rules.h.
// Included by adh_api.hip behind adh_session.h (shares its error helpers, the handle, grow_device and the event pair).
#include "adh_select_rules.h"

namespace {

// a refusal of adh_select_rules.h as this library returns it
int refused(const selrules::Refusal &r) { return r.msg ? fail(r.code, r.msg) : ADH_OK; }

// the per-precursor id columns of adh_select_candidates_resident (host)
struct SelIds {
    const uint32_t *elution_group_idx;
    const uint8_t *decoy, *channel;
};

// The switches of a selection call, read from the environment when a call begins: the
// tests flip them between calls on one handle.
struct SelSwitches {
    static int32_t number(const char *name) { const char *env = getenv(name); return env ? atoi(env) : 0; }
    const bool timing = getenv("ADH_DEBUG_SELECT_TIMING") || getenv("ADH_DEBUG_TIMING");  // a line per stage on stderr
    const char *const scratch_mb = getenv("ADH_SELECT_SCRATCH_MB");  // set by hand: wins over a larger slab already held
    const uint64_t scratch_bytes = scratch_mb ? (uint64_t)atoll(scratch_mb) << 20 : 0;
    const int32_t im_dense = number("ADH_DEBUG_SELECT_IM_DENSE"), im_abl = number("ADH_DEBUG_SELECT_IM_ABL");
    const int32_t stop = number("ADH_DEBUG_SELECT_STOP");                // sel::SelCaps::stop
    const bool lds_taps = getenv("ADH_DEBUG_SELECT_LDS_TAPS") != nullptr;  // A/B: the generic smoothing loop
};

// the stage timer of both drivers (host clock)
struct SelStages {
    const bool on;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[select] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// the nine columns of adh_candidate_table_t / DevCandTable in their order, and their widths: 33 bytes per row
constexpr int kCandCols = 9;
constexpr size_t kCandWidth[kCandCols] = {4, 1, 4, 4, 4, 4, 4, 4, 4};
std::array<void *, kCandCols> cand_columns(const adh_candidate_table_t *t) {
    return {t->precursor_idx, t->rank, t->score, t->scan_center, t->scan_start, t->scan_stop, t->frame_center, t->frame_start, t->frame_stop};
}

// A grow-only block of the handle at exactly `need` bytes (grow_device's slack is for scoring batches that grow from
// call to call; the old block goes only after the device is idle).
int grow_exact(void **p, size_t *bytes, size_t need, const char *what) {
    if (grow_device(p, bytes, need, 0) == ADH_OK) return ADH_OK;
    return fail(ADH_ERR_OUT_OF_MEMORY, std::string("hipMalloc(") + what + "): " + g_last_error);
}

// What the handle's selection slab holds in a call, every offset a multiple of 256 bytes.  A driver lays it out in
// the order of its calls: shared(), the columns and regions of its own (column(), carve()), isotopes() and ids()
// where the layout holds them, table().  The candidate table comes LAST: upload() zeroes it with one memset from its
// first column to the end of the slab (rows without a candidate stay zero).
struct SelSlab {
    struct Put { size_t at; const void *src; size_t bytes; };
    const int64_t n;        // precursors
    int64_t rows = 0;       // of the candidate table
    size_t end = 0;
    std::vector<Put> puts;  // the host columns, in upload order
    size_t precursor_idx = 0, frag_start = 0, frag_stop = 0, charge = 0, rt = 0, mz = 0, mobility = 0, iso = 0;
    size_t elution_group = 0, decoy = 0, channel = 0, out[kCandCols] = {0};
    unsigned char *base = nullptr;
    size_t carve(size_t bytes) {
        const size_t at = end;
        end += (bytes + 255) / 256 * 256;
        return at;
    }
    size_t column(const void *src, size_t bytes) {
        const size_t at = carve(bytes);
        puts.push_back(Put{at, src, bytes});
        return at;
    }
    void shared(const adh_precursors_t *pc, bool with_mobility) {
        precursor_idx = column(pc->precursor_idx, (size_t)n * 4);
        frag_start = column(pc->frag_start_idx, (size_t)n * 4);
        frag_stop = column(pc->frag_stop_idx, (size_t)n * 4);
        charge = column(pc->charge, (size_t)n);
        rt = column(pc->rt, (size_t)n * 4);
        if (with_mobility) mobility = column(pc->mobility, (size_t)n * 4);
        mz = column(pc->mz, (size_t)n * 4);
    }
    void isotopes(const adh_precursors_t *pc) { iso = column(pc->isotope_intensity, (size_t)n * pc->n_isotope_cols * 4); }
    void ids(const SelIds *i) {
        elution_group = column(i->elution_group_idx, (size_t)n * 4);
        decoy = column(i->decoy, (size_t)n);
        channel = column(i->channel, (size_t)n);
    }
    void table(int64_t n_rows) {
        rows = n_rows;
        for (int f = 0; f < kCandCols; ++f) out[f] = carve((size_t)rows * kCandWidth[f]);
    }
    int reserve(adh_handle *h) {
        ADH_TRY(grow_exact(&h->sel_slab, &h->sel_slab_bytes, end, "selection slab"));
        base = static_cast<unsigned char *>(h->sel_slab);
        return ADH_OK;
    }
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    // the host columns up, the driver's reduction words and the candidate table zeroed
    int upload(hipStream_t st, size_t red, size_t red_bytes) const {
        hipError_t e = hipSuccess;
        for (const Put &p : puts)
            if (e == hipSuccess && p.bytes) e = hipMemcpyAsync(base + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(base + red, 0, red_bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(base + out[0], 0, end - out[0], st);
        if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("selection upload: ") + hipGetErrorString(e));
        return ADH_OK;
    }
    DevCandTable table_view() const {
        return DevCandTable{at<uint32_t>(out[0]), at<uint8_t>(out[1]), at<float>(out[2]), at<uint32_t>(out[3]), at<uint32_t>(out[4]),
                            at<uint32_t>(out[5]), at<uint32_t>(out[6]), at<uint32_t>(out[7]), at<uint32_t>(out[8])};
    }
    // what a resident selection left in the slab, for adh_assemble_selected
    void note_selected(adh_handle *h, const adh_precursors_t *pc, const adh_selection_config_t *cfg) const {
        adh_handle::Selected &s = h->sel;
        s = adh_handle::Selected();
        s.n_prec = pc->n, s.cand_count = cfg->candidate_count, s.n_iso_cols = pc->n_isotope_cols;
        s.precursor_idx = at<const uint32_t>(precursor_idx);
        s.frag_start = at<const uint32_t>(frag_start);
        s.frag_stop = at<const uint32_t>(frag_stop);
        s.charge = at<const uint8_t>(charge);
        s.mz = at<const float>(mz);
        s.iso = at<const float>(iso);
        s.elution_group = at<const uint32_t>(elution_group);
        s.decoy = at<const uint8_t>(decoy);
        s.channel = at<const uint8_t>(channel);
        s.table = table_view();
        s.stage = 1;
    }
    // The end of a call, `e` being what the launches returned: the second event behind the last kernel, then the
    // copy-out (33 bytes per row; none for a resident selection, which is noted on the handle instead), then the one
    // stream synchronisation, then the kernels' event time.  A failed call leaves the handle's time as it was.
    int finish(adh_handle *h, const sess::EventPair &ev, hipError_t e, const adh_precursors_t *pc, const adh_selection_config_t *cfg,
               const adh_candidate_table_t *host, const SelIds *ids, const char *what) const {
        if (e == hipSuccess) e = hipEventRecord(ev.e1, h->stream);
        const auto to = cand_columns(host);
        for (int f = 0; f < kCandCols && e == hipSuccess && !ids; ++f)
            e = hipMemcpyAsync(to[f], base + out[f], (size_t)rows * kCandWidth[f], hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        if (ids) note_selected(h, pc, cfg);
        else h->d2h_bytes += (uint64_t)rows * 33;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.e0, ev.e1) == hipSuccess) h->last_select_ms = ms;
        return ADH_OK;
    }
};

// Candidate selection on the staged ion-mobility run (see adh_select_im.hip); the caller has
// validated the arguments and zero-filled the host table.  `ids` (adh_select_candidates_resident): the table stays in
// the slab, with the id columns and the isotope columns beside it, and nothing is copied out.
int select_candidates_im(adh_handle *h, const adh_precursors_t *pc, const adh_selection_config_t *cfg, const float *kernel, int32_t k0,
                         int32_t k1, adh_candidate_table_t *out, const SelIds *ids, const SelSwitches &sw, SelStages &stages) {
    const int64_t n = pc->n;
    const DevTims &T = h->tims;
    hipStream_t st = h->stream;
    if (!pc->mobility) return fail(ADH_ERR_INVALID_ARGUMENT, "precursor mobility column is NULL");
    std::vector<double> ku, kv;
    ADH_TRY(refused(selrules::rank1_factors(kernel, k0, k1, ku, kv)));
    const int n_iso = (int)std::min<int64_t>(cfg->top_k_precursors, pc->n_isotope_cols);
    // Beside the columns: plan records, their scratch sizes and prefix sums, the reduction words, the kernel's
    // factors, the batches and the scan's temporary storage.  The plan (limits, validity, empty-query test) is a
    // kernel (adh_select_plan_im_kernel); the host only cuts the batches.
    SelSlab s{n};
    s.shared(pc, true);
    const size_t o_recs = s.carve((size_t)n * sizeof(selim::PrecRec)), o_need = s.carve((size_t)n * 8), o_cum = s.carve((size_t)n * 8),
                 o_red = s.carve(64), o_ku = s.column(ku.data(), (size_t)k0 * 8), o_kv = s.column(kv.data(), (size_t)k1 * 8),
                 o_first = s.carve((size_t)(n + 2) * 8);
    size_t scan_bytes = 0;
    HIP_TRY(select_need_sums(nullptr, scan_bytes, nullptr, nullptr, n, st));
    const size_t o_tmp = s.carve(scan_bytes);
    if (ids) s.isotopes(pc), s.ids(ids);  // (the kernels of this layout read neither)
    s.table(out->n);
    ADH_TRY(s.reserve(h));
    ADH_TRY(s.upload(st, o_red, 64));
    const SelPlanIn pin{s.at<const uint32_t>(s.precursor_idx), s.at<const uint32_t>(s.frag_start), s.at<const uint32_t>(s.frag_stop),
                        s.at<const uint8_t>(s.charge), s.at<const float>(s.rt), s.at<const float>(s.mobility), s.at<const float>(s.mz)};
    selim::PrecRec *d_recs = s.at<selim::PrecRec>(o_recs);
    unsigned long long *d_need = s.at<unsigned long long>(o_need), *d_cum = s.at<unsigned long long>(o_cum);
    int32_t *d_red = s.at<int32_t>(o_red);
    unsigned long long *d_biggest = s.at<unsigned long long>(o_red + 32);
    hipLaunchKernelGGL(adh_select_plan_im_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, pin, n, h->n_lib, n_iso,
                       cfg->rt_tolerance, cfg->mobility_tolerance, cfg->kernel_size, (int)k0, (int)k1, d_recs, d_need, d_red, d_biggest);
    hipError_t e = hipGetLastError();
    size_t tb = scan_bytes;
    if (e == hipSuccess) e = select_need_sums(s.base + o_tmp, tb, d_need, d_cum, n, st);
    struct {
        int32_t red[8];
        unsigned long long biggest, pad;
    } meta;
    unsigned long long all = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&meta, d_red, 48, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&all, d_cum + (n - 1), 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("selection plan: ") + hipGetErrorString(e));
    if (meta.red[0] & 1) return fail(ADH_ERR_INVALID_ARGUMENT, "fragment slice outside the staged library");
    if (meta.red[0] & 2) return fail(ADH_ERR_INVALID_ARGUMENT, "precursor charge must be > 0");
    if (meta.red[0] & 4) return fail(ADH_ERR_UNSUPPORTED, "more than 64 m/z windows per precursor");
    int32_t cap_cells = std::max(meta.red[1], 1), cap_s = std::max(meta.red[2], 1), cap_f = std::max(meta.red[3], 1);
    cap_cells = (cap_cells + 1) & ~1;  // the float64 kernel factors follow the float tiles in LDS
    const int tap_budget = adh_select_tap_budget(cap_cells, cap_s, k0, k1);
    const size_t lds_smooth = adh_select_smooth_im_lds_bytes(cap_cells, cap_s, k0, k1, tap_budget);
    const size_t lds_score = adh_select_score_im_lds_bytes(cap_cells, cap_s, cap_f);
    const size_t lds = std::max(lds_smooth, lds_score);
    if (lds > 150 * 1024 || cap_f > selim::SCORE_THREADS) {
        char buf[200];
        snprintf(buf, sizeof(buf), "selection tile of %d cells (scans x cycles, %d cycles) needs %zu bytes of LDS: exceeds 150 KiB",
                 cap_cells, cap_f, lds);
        return fail(ADH_ERR_UNSUPPORTED, buf);
    }
    // batches of precursors whose tiles fit a bounded scratch slab: the scratch slab of the handle is used (kept
    // between calls; only reserved memory: a precursor's tiles are normally kept in sparse form and touch a few KB of
    // their block); batches follow each other on the stream, so a batch may reuse the slab of the one before without
    // the host waiting
    const uint64_t budget = selrules::selection_budget(all, meta.biggest, h->scratch_slab_bytes, sw.scratch_mb ? &sw.scratch_bytes : nullptr);
    stages.lap("upload + plan");
    std::vector<int64_t> first{0, n};  // first precursor of every batch, then n
    if (all > budget) {
        // the longest prefixes that fit: the inclusive sums come back and are cut on the host
        std::vector<unsigned long long> cum((size_t)n);
        HIP_TRY(hipMemcpy(cum.data(), d_cum, (size_t)n * 8, hipMemcpyDeviceToHost));
        ADH_TRY(refused(selrules::cut_batches(cum.data(), n, budget, first)));
    }
    const int n_batches = (int)first.size() - 1;
    int64_t *d_first = s.at<int64_t>(o_first);
    HIP_TRY(hipMemcpyAsync(d_first, first.data(), first.size() * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(adh_select_offsets_im_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_recs, d_cum, d_need, n, d_first,
                       n_batches);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // (first lives on this stack frame)
    const double *d_ku = s.at<const double>(o_ku), *d_kv = s.at<const double>(o_kv);
    const DevCandTable dt = s.table_view();
    ADH_TRY(grow_exact(&h->scratch_slab, &h->scratch_slab_bytes, budget, "selection scratch"));
    unsigned char *d_scratch = static_cast<unsigned char *>(h->scratch_slab);
    stages.lap("batches");
    select_im_raise_lds_limit();
    sess::EventPair ev;
    ADH_TRY(ev.begin(st));
    for (int b = 0; b < n_batches && e == hipSuccess; ++b) {
        const int64_t b0 = first[(size_t)b];
        const int32_t cnt = (int32_t)(first[(size_t)b + 1] - b0);
        hipLaunchKernelGGL(adh_select_gather_im_kernel, dim3((unsigned)cnt), dim3(ADH_WAVE), 0, st, T, h->d_lib, d_recs + b0, cnt, *cfg,
                           (int32_t)n_iso, d_scratch, sw.im_dense);
        if (sw.im_abl != 0)
            hipLaunchKernelGGL(adh_select_smooth_im_kernel<true>, dim3((unsigned)cnt), dim3(selim::SMOOTH_THREADS), lds_smooth, st,
                               d_recs + b0, cnt, d_ku, d_kv, k0, k1, cap_cells, cap_s, d_scratch, sw.im_abl, (int32_t)tap_budget);
        else
            hipLaunchKernelGGL(adh_select_smooth_im_kernel<false>, dim3((unsigned)cnt), dim3(selim::SMOOTH_THREADS), lds_smooth, st,
                               d_recs + b0, cnt, d_ku, d_kv, k0, k1, cap_cells, cap_s, d_scratch, sw.im_abl, (int32_t)tap_budget);
        hipLaunchKernelGGL(adh_select_score_im_kernel, dim3((unsigned)cnt), dim3(selim::SCORE_THREADS), lds_score, st, T, d_recs + b0, cnt,
                           b0, *cfg, cap_cells, cap_s, cap_f, d_scratch, dt);
        e = hipGetLastError();
    }
    const int rc = s.finish(h, ev, e, pc, cfg, out, ids, "ion-mobility selection kernels");
    stages.lap("kernels + copy-out");
    return rc;
}

// adh_select_candidates (`ids` NULL: the table is copied into `out`) and adh_select_candidates_resident (`ids` set:
// `out` only carries the row count; the table, the precursor columns and the id columns stay in the slab)
int select_candidates_run(adh_handle_t *h, const adh_precursors_t *pc, const adh_selection_config_t *cfg, const float *kernel,
                          int32_t k_rows, int32_t k_cols, adh_candidate_table_t *out, const SelIds *ids) {
    if (!h || !pc || !cfg || !kernel || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    h->sel.stage = 0;  // (the slab is rewritten)
    if (!h->run_staged && !h->tims_staged) return fail(ADH_ERR_NOT_STAGED, "no run staged");
    if (!h->d_lib) return fail(ADH_ERR_NOT_STAGED, "no fragment library staged");
    if (pc->n < 0 || cfg->candidate_count <= 0 || cfg->candidate_count > sel::MAX_CAND)
        return fail(ADH_ERR_INVALID_ARGUMENT, "candidate_count must be in 1..16");
    if (out->n != pc->n * cfg->candidate_count)
        return fail(ADH_ERR_INVALID_ARGUMENT, "candidate table rows != precursors x candidate_count");
    if (k_rows <= 0 || k_cols <= 0 || cfg->top_k_precursors <= 0 || pc->n_isotope_cols <= 0)
        return fail(ADH_ERR_INVALID_ARGUMENT, "kernel / isotope dimensions must be positive");
    HIP_TRY(hipSetDevice(h->device));
    const SelSwitches sw;
    SelStages stages{sw.timing};
    const int64_t n = pc->n;
    const auto host = cand_columns(out);
    for (int f = 0; f < kCandCols && !ids; ++f) {
        if (!host[f]) return fail(ADH_ERR_INVALID_ARGUMENT, "candidate table buffer is NULL");
        memset(host[f], 0, (size_t)out->n * kCandWidth[f]);
    }
    stages.lap("memset");
    if (n == 0) {
        if (ids) {  // (an empty selection: nothing in the slab is read)
            h->sel = adh_handle::Selected();
            h->sel.cand_count = cfg->candidate_count;
            h->sel.n_iso_cols = pc->n_isotope_cols;
            h->sel.stage = 1;
        }
        return ADH_OK;
    }
    if (h->tims_staged) return select_candidates_im(h, pc, cfg, kernel, k_rows, k_cols, out, ids, sw, stages);
    // One grow-only slab of the handle holds the precursor columns, the tile limits and the candidate table of a
    // call (19 allocations and as many frees cost more than the kernel).  The per-precursor limits - two searches
    // over the retention times of 3e5 spectra each: 17 ms per 100 000 precursors on one host core - and the checks
    // of the fragment slices are a kernel of their own; three words come back to size the LDS.
    sel::SelCaps caps{};
    caps.n_iso = (int32_t)std::min<int64_t>(cfg->top_k_precursors, pc->n_isotope_cols);
    caps.k_rows = k_rows, caps.k_cols = k_cols, caps.stop = sw.stop;
    const int L = h->run.cycle_len;
    hipStream_t st = h->stream;
    ADH_TRY(refused(selrules::cycle_rows_refusal(h->h_cycle.data(), L, h->run.n_ms1_obs, pc->mz, pc->charge, n, caps.n_iso, sel::MAX_ROWS)));
    SelSlab s{n};
    s.shared(pc, false);
    s.isotopes(pc);
    const size_t o_cs = s.carve((size_t)n * 4), o_cc = s.carve((size_t)n * 4), o_red = s.carve(16),
                 o_kern = s.column(kernel, (size_t)k_rows * k_cols * 4);
    if (ids) s.ids(ids);
    s.table(out->n);
    ADH_TRY(s.reserve(h));
    ADH_TRY(s.upload(st, o_red, 16));
    const DevPrecursors dp{s.at<const uint32_t>(s.precursor_idx), s.at<const uint32_t>(s.frag_start), s.at<const uint32_t>(s.frag_stop),
                           s.at<const uint8_t>(s.charge), s.at<const float>(s.rt), s.at<const float>(s.mz), s.at<const float>(s.iso),
                           s.at<const int32_t>(o_cs), s.at<const int32_t>(o_cc), pc->n_isotope_cols};
    int32_t *d_red = s.at<int32_t>(o_red);
    hipLaunchKernelGGL(adh_select_limits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->run.rt, h->run.n_spectra, L, dp, n,
                       h->n_lib, cfg->rt_tolerance, cfg->kernel_size, s.at<int32_t>(o_cs), s.at<int32_t>(o_cc), d_red);
    hipError_t e = hipGetLastError();
    int32_t red[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(red, d_red, sizeof(red), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("selection limits: ") + hipGetErrorString(e));
    stages.lap("uploads + limits");
    if (red[2] & 1) return fail(ADH_ERR_INVALID_ARGUMENT, "fragment slice outside the staged library");
    if (red[2] & 2) return fail(ADH_ERR_INVALID_ARGUMENT, "precursor charge must be > 0");
    caps.n_lib = std::max(red[0], 1);
    caps.f = std::max(red[1], 1);
    const size_t lds = sel::lds_bytes(caps);
    if (lds > 150 * 1024) {
        char buf[200];
        snprintf(buf, sizeof(buf), "selection tile needs %zu bytes of LDS (%d cycles, %d fragments): exceeds 150 KiB", lds, caps.f, caps.n_lib);
        return fail(ADH_ERR_UNSUPPORTED, buf);
    }
    sel::Taps taps = selrules::two_row_taps<sel::Taps>(kernel, k_rows, k_cols);
    if (sw.lds_taps) taps.cols = 0;
    (void)hipFuncSetAttribute((const void *)adh_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    (void)hipGetLastError();
    sess::EventPair ev;
    ADH_TRY(ev.begin(st));
    hipLaunchKernelGGL(adh_select_kernel, dim3((unsigned)n), dim3(ADH_WAVE), lds, st,
                       (SelectArgs{h->run, h->d_lib, dp, (int64_t)n, *cfg, s.at<const float>(o_kern), taps, caps, s.table_view()}));
    const int rc = s.finish(h, ev, hipGetLastError(), pc, cfg, out, ids, "selection kernel");
    stages.lap("kernel + copy-out");
    return rc;
}

}  // namespace

int adh_select_candidates(adh_handle_t *h, const adh_precursors_t *pc, const adh_selection_config_t *cfg,
                          const float *kernel, int32_t k_rows, int32_t k_cols, adh_candidate_table_t *out) {
    return select_candidates_run(h, pc, cfg, kernel, k_rows, k_cols, out, nullptr);
}

int adh_select_time_ms(adh_handle_t *h, double *kernel_ms) {
    if (!h || !kernel_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *kernel_ms = h->last_select_ms;
    return ADH_OK;
}
