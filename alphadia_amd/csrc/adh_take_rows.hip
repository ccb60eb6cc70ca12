// adh_take_rows.hip - resident extraction: score into the handle's tables without a copy-out
// (adh_score_candidates_resident), then copy back only the rows a later stage keeps (adh_take_rows).
//
// The per-file extraction (alphadia/workflow/peptidecentric/peptidecentric.py:183-263) scores every candidate, runs the
// FDR stage over them and keeps the survivors at 1 % FDR with their fragment rows - about one row in eight.  With the
// tables left in HBM the FDR stage runs on them in place (adh_fdr_resident), and what the host needs afterwards is the
// survivors' rows in the compact layout of adh_score_candidates_compact.  adh_take_rows is that copy-out for a list of
// rows: the pattern of the compact path (adh_cop_count_kernel / adh_cop_pack_kernel) over the listed rows instead of
// a chunk - a count per row (valid flag, leading filled slots), an exclusive scan, a pack kernel that writes one dense
// block, ONE copy of its used bytes into page-locked memory, host threads moving the columns into the caller's arrays.
// Unlike the compact path every column travels (ids and library columns too, 42 bytes per slot and 193 per row): the
// candidate table the host would rebuild them from is not kept once the scoring call has returned.
// Included by adh_api.hip (shares its error helpers and the handle).

namespace take {

// a block of R rows and S slots: [row u32 | precursor_idx u32 | rank u8 | features f32 [46][R]] then
// [fragment_row u32 | fragment_precursor_idx u32 | fragment_rank u8 | 7 f32 columns | 5 u8 columns]; every column
// starts on a multiple of 16 bytes
struct Block {
    size_t row, pidx, rank, feat, s_row, s_pidx, s_rank, s_f[7], s_b[5], total;
    __host__ __device__ Block(uint64_t R, uint64_t S) {
        size_t o = 0;
        auto col = [&](size_t bytes) {
            const size_t at = o;
            o += (bytes + 15) & ~(size_t)15;
            return at;
        };
        row = col(R * 4), pidx = col(R * 4), rank = col(R), feat = col(R * 4 * ADH_NUM_FEATURES);
        s_row = col(S * 4), s_pidx = col(S * 4), s_rank = col(S);
        for (int j = 0; j < 7; ++j) s_f[j] = col(S * 4);
        for (int j = 0; j < 5; ++j) s_b[j] = col(S);
        total = o;
    }
};

// cnt[i] = (valid << 32) | leading filled slots of listed row rows[i]; cnt[n] = 0 (the scan's last entry is the total)
__global__ void __launch_bounds__(256) count_kernel(const uint8_t *__restrict__ valid, const uint16_t *__restrict__ lib_slot,
                                                    const int64_t *__restrict__ rows, int64_t n, int top_k,
                                                    uint64_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint64_t v = 0;
    if (i < n) {
        const int64_t r = rows[i];
        if (valid[r]) {
            const uint16_t *s = lib_slot + r * (int64_t)top_k;
            uint32_t k = 0;
            while (k < (uint32_t)top_k && s[k]) ++k;  // (filled slots are the leading ones: candidate.py:403-442)
            v = (1ull << 32) | k;
        }
    }
    cnt[i] = v;
}

// every column of the listed valid rows and their filled slots into the dense block (off: the scanned counts)
__global__ void __launch_bounds__(256) pack_kernel(DevOut t, const int64_t *__restrict__ rows, int64_t n, int top_k,
                                                   const uint64_t *__restrict__ off, unsigned char *__restrict__ block) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t tot = off[n];
    const uint64_t R = tot >> 32;
    const Block L(R, tot & 0xFFFFFFFFull);
    uint32_t *const o_row = reinterpret_cast<uint32_t *>(block + L.row);
    uint32_t *const o_pidx = reinterpret_cast<uint32_t *>(block + L.pidx);
    uint8_t *const o_rank = block + L.rank;
    float *const o_feat = reinterpret_cast<float *>(block + L.feat);
    for (int64_t i = tid; i < n; i += stride) {
        const uint64_t o = off[i], o1 = off[i + 1];
        if ((o1 >> 32) == (o >> 32)) continue;
        const int64_t j = (int64_t)(o >> 32), r = rows[i];
        o_row[j] = (uint32_t)r;
        o_pidx[j] = t.precursor_idx[r];
        o_rank[j] = t.rank[r];
        const float *f = t.features + r * ADH_NUM_FEATURES;
#pragma unroll
        for (int k = 0; k < ADH_NUM_FEATURES; ++k) o_feat[(size_t)k * R + (size_t)j] = f[k];
    }
    uint32_t *const s_row = reinterpret_cast<uint32_t *>(block + L.s_row);
    uint32_t *const s_pidx = reinterpret_cast<uint32_t *>(block + L.s_pidx);
    uint8_t *const s_rank = block + L.s_rank;
    const float *const src_f[7] = {t.fragment_mz_library, t.fragment_mz, t.fragment_mz_observed, t.fragment_height,
                                   t.fragment_intensity, t.fragment_mass_error, t.fragment_correlation};
    const uint8_t *const src_b[5] = {t.fragment_position, t.fragment_number, t.fragment_type, t.fragment_charge,
                                     t.fragment_loss_type};
    const int64_t n_slots = n * (int64_t)top_k;
    for (int64_t id = tid; id < n_slots; id += stride) {
        const int64_t i = id / top_k;
        const int s = (int)(id - i * top_k);
        const uint64_t o = off[i], o1 = off[i + 1];
        const uint32_t a = (uint32_t)o, k = (uint32_t)o1 - a;
        if ((uint32_t)s >= k) continue;
        const int64_t r = rows[i], src = r * (int64_t)top_k + s;
        const size_t dst = (size_t)a + (size_t)s;
        s_row[dst] = (uint32_t)r;
        s_pidx[dst] = t.fragment_precursor_idx[src];
        s_rank[dst] = t.fragment_rank[src];
#pragma unroll
        for (int j = 0; j < 7; ++j) reinterpret_cast<float *>(block + L.s_f[j])[dst] = src_f[j][src];
#pragma unroll
        for (int j = 0; j < 5; ++j) (block + L.s_b[j])[dst] = src_b[j][src];
    }
}

// the checks of a resident scoring call and the shape of its tables (rows, width) in `shape`
int resident_shape(adh_handle_t *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg, adh_output_t &shape) {
    if (!h || !c || !cfg) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h->comm_attached())
        return fail(ADH_ERR_UNSUPPORTED, "resident scoring with a communicator attached (the tables are a shard plus a gather)");
    if (c->n < 0 || (c->n > 0 && (!c->frag_start_idx || !c->frag_stop_idx)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "candidate table: row count / fragment slices");
    // the width of the padded tables, as the callers of adh_score_candidates pick it (alphadia_amd/_abi.py:
    // output_width): top_k_fragments clamped to the longest library slice (unsigned: a slice with stop < start wraps
    // to a huge length, the clamp makes that top_k and the pipeline rejects the table)
    uint32_t longest = 0;
    for (int64_t i = 0; i < c->n; ++i) longest = std::max<uint32_t>(longest, c->frag_stop_idx[i] - c->frag_start_idx[i]);
    shape = adh_output_t{};
    shape.n = c->n;
    shape.top_k = c->n == 0 ? 1 : (int32_t)std::max<uint32_t>(1u, std::min<uint32_t>(cfg->top_k_fragments, std::max<uint32_t>(longest, 1u)));
    return ADH_OK;
}

}  // namespace take

extern "C" {

int adh_score_candidates_resident(adh_handle_t *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg) {
    adh_output_t shape{};
    const int rc = take::resident_shape(h, c, cfg, shape);
    if (rc != ADH_OK) return rc;
    return score_pipeline(h, c, cfg, &shape, nullptr, true);
}

int adh_take_rows(adh_handle_t *h, const int64_t *rows, int64_t n, adh_compact_output_t *out) {
    if (!h || !out || (n > 0 && !rows)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 0 || out->rows_capacity < 0 || out->slots_capacity < 0)
        return fail(ADH_ERR_INVALID_ARGUMENT, "take_rows: negative row count / capacities");
    if (h->last_tables < 0 || !h->tables_current)
        return fail(ADH_ERR_NOT_STAGED, "no scored tables of the staged run and library on the device");
    const int64_t n_table = h->last_rows;
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= n_table) return fail(ADH_ERR_INVALID_ARGUMENT, "take_rows: row outside the device tables");
    const adh_output_t &tab = h->tables[h->last_tables].view;
    const int top_k = tab.top_k;
    if (out->top_k != top_k) return fail(ADH_ERR_INVALID_ARGUMENT, "take_rows: top_k differs from the device tables'");
    if (n > 0 && (uint64_t)n * (uint64_t)top_k >= 0xFFFFFFFFull)
        return fail(ADH_ERR_UNSUPPORTED, "take_rows: more than 2^32 fragment slots");
    out->n_rows = out->n_slots = 0;
    if (n == 0) return ADH_OK;
    if (!compact_output_complete(out)) return fail(ADH_ERR_INVALID_ARGUMENT, "compact output buffer is NULL");
    HIP_TRY(hipSetDevice(h->device));
    int rc = materialise_tables(h);  // (ids and library columns of a resident or compact scoring call)
    if (rc != ADH_OK) return rc;
    hipStream_t st = h->stream;
    // device scratch (grow-only, shared with the compact path - both are synchronous): counts [n + 1] then rows [n]
    const size_t cnt_bytes = (size_t)(2 * n + 1) * 8;
    rc = grow_device(&h->cop_cnt, &h->cop_cnt_bytes, cnt_bytes, cnt_bytes / 8);
    if (rc != ADH_OK) return rc;
    uint64_t *const d_cnt = static_cast<uint64_t *>(h->cop_cnt);
    int64_t *const d_rows = reinterpret_cast<int64_t *>(d_cnt + n + 1);
    rc = grow_scan_scratch<uint64_t>(&h->cop_scan, &h->cop_scan_bytes, n + 1, st);
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(take::count_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, tab.valid,
                       tab.fragment_lib_slot, d_rows, n, top_k, d_cnt);
    HIP_TRY(hipGetLastError());
    size_t scan_bytes = h->cop_scan_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->cop_scan, scan_bytes, d_cnt, d_cnt, (int)(n + 1), st));
    uint64_t tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, d_cnt + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->d2h_bytes += 8;
    const int64_t R = (int64_t)(tot >> 32), S = (int64_t)(tot & 0xFFFFFFFFull);
    out->n_rows = R;
    out->n_slots = S;
    if (R > out->rows_capacity || S > out->slots_capacity)
        return fail(ADH_ERR_INVALID_ARGUMENT, "take_rows: rows_capacity / slots_capacity too small (n_rows / n_slots say what is needed)");
    if (R == 0) return ADH_OK;
    const take::Block L((uint64_t)R, (uint64_t)S);
    rc = grow_device(&h->cop_dev, &h->cop_dev_bytes, L.total, L.total / 8 + 4096);
    if (rc == ADH_OK) rc = grow_pinned(&h->cop_stage, &h->cop_stage_bytes, L.total, L.total / 8);
    if (rc != ADH_OK) return rc;
    unsigned char *const d_block = static_cast<unsigned char *>(h->cop_dev);
    unsigned char *const block = static_cast<unsigned char *>(h->cop_stage);
    const int64_t work = std::max<int64_t>(n * (int64_t)top_k, n);
    hipLaunchKernelGGL(take::pack_kernel, dim3((unsigned)std::min<int64_t>((work + 255) / 256, 8192)), dim3(256), 0, st, tab,
                       d_rows, n, top_k, d_cnt, d_block);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(block, d_block, L.total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->d2h_bytes += L.total;
    // the columns into the caller's arrays (which may be pageable): one job per column, on a few host threads
    struct Job {
        void *dst;
        const void *src;
        size_t bytes;
    };
    std::vector<Job> jobs;
    jobs.push_back({out->row, block + L.row, (size_t)R * 4});
    jobs.push_back({out->precursor_idx, block + L.pidx, (size_t)R * 4});
    jobs.push_back({out->rank, block + L.rank, (size_t)R});
    for (int k = 0; k < ADH_NUM_FEATURES; ++k)
        jobs.push_back({out->features + (size_t)k * (size_t)out->rows_capacity, block + L.feat + (size_t)k * (size_t)R * 4,
                        (size_t)R * 4});
    if (S > 0) {
        jobs.push_back({out->fragment_row, block + L.s_row, (size_t)S * 4});
        jobs.push_back({out->fragment_precursor_idx, block + L.s_pidx, (size_t)S * 4});
        jobs.push_back({out->fragment_rank, block + L.s_rank, (size_t)S});
        float *const f[7] = {out->fragment_mz_library, out->fragment_mz, out->fragment_mz_observed, out->fragment_height,
                             out->fragment_intensity, out->fragment_mass_error, out->fragment_correlation};
        uint8_t *const b[5] = {out->fragment_position, out->fragment_number, out->fragment_type, out->fragment_charge,
                               out->fragment_loss_type};
        for (int j = 0; j < 7; ++j) jobs.push_back({f[j], block + L.s_f[j], (size_t)S * 4});
        for (int j = 0; j < 5; ++j) jobs.push_back({b[j], block + L.s_b[j], (size_t)S});
    }
    const int T = std::max(1, std::min<int>(host_threads_for(R + S), (int)jobs.size()));
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < jobs.size();) memcpy(jobs[i].dst, jobs[i].src, jobs[i].bytes);
    };
    std::vector<std::thread> team;
    for (int w = 1; w < T; ++w) {
        try {
            team.emplace_back(worker);
        } catch (const std::system_error &) {
            break;  // (the calling thread takes what the others leave)
        }
    }
    worker();
    for (std::thread &t : team) t.join();
    return ADH_OK;
}

}  // extern "C"
