// adh_select_handover.hip - the candidate table from selection to scoring without leaving HBM.
//
// adh_select_candidates_resident runs the selection kernels of adh_select_candidates and leaves the table - n_precursors
// x candidate_count rows, row p * candidate_count + slot - in the handle's selection slab, next to the precursor columns
// the kernels read and the three id columns scoring orders by (elution_group_idx, decoy, channel).  A candidate's
// precursor row is table_row / candidate_count, so what the host does with a merge and seven searchsorted lookups
// (HipCandidateSelection.__call__, "filter 1" of the extraction handler, scoring.assemble_candidates) is here
//   flag     score > 0 [and score > cutoff]                                  one kernel, a scan for the positions
//   select   the kept rows, in (precursor, slot) order                      sess::select_flagged
//   check    are they in (elution_group_idx, decoy, rank, precursor_idx) order already?
//   sort     if not: two stable LSD passes, (precursor_idx | rank | decoy) then elution_group_idx = np.lexsort
//   groups   score_group_idx = row, or head flags + inclusive scan; duplicates; reference-channel flags
//   gather   the candidate SoA of adh_upload_candidates into the handle's candidate slab
// and adh_score_selected_resident is adh_score_candidates_resident on that slab.  The host gets two id columns per kept
// row (adh_selected_ids: 5 bytes) and later the candidate columns of the rows it lists (adh_take_selected).
// Included by adh_api.hip behind adh_session.h (shares its error helpers, the handle and the sort / scan helpers).

namespace hov {

constexpr int kBlock = sess::kBlock;
using sess::grid_for;

// reductions of a call, one block of words on the device
enum { M_UNSORTED = 0, M_DUP = 1, M_LONGEST = 2, M_CELLS = 3, M_SKIP = 4, M_WORDS = 8 };

struct Table {
    const uint32_t *precursor_idx;
    const uint8_t *rank;
    const float *score;
    const uint32_t *scan_center, *scan_start, *scan_stop, *frame_center, *frame_start, *frame_stop;
};

struct Prec {
    const uint32_t *frag_start, *frag_stop, *elution_group;
    const uint8_t *charge, *decoy, *channel;
    const float *mz, *iso;
    int32_t n_iso_cols;
    uint32_t cand_count;
};

Table table_of(const adh_handle::Selected &s) {
    const DevCandTable &t = s.table;
    return Table{t.precursor_idx, t.rank, t.score, t.scan_center, t.scan_start, t.scan_stop, t.frame_center, t.frame_start, t.frame_stop};
}

Prec prec_of(const adh_handle::Selected &s) {
    return Prec{s.frag_start, s.frag_stop, s.elution_group, s.charge, s.decoy, s.channel, s.mz, s.iso, s.n_iso_cols,
                (uint32_t)s.cand_count};
}

// selected[i] = score > 0 (candidate_container_to_df), keep[i] = selected and, with `apply`, score > cutoff in float64
// (the caller rounded the cutoff to the dtype NumPy compares a float32 column with it in); selected[n] = 0, so that
// the exclusive scan over n + 1 entries ends with the count
__global__ void __launch_bounds__(kBlock) flag_kernel(const float *__restrict__ score, int64_t n, int apply, double cutoff,
                                                      uint32_t *__restrict__ selected, uint8_t *__restrict__ keep) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
        if (i == n) {
            selected[i] = 0;
            continue;
        }
        const float s = score[i];
        const bool sel = s > 0.0f;
        selected[i] = sel ? 1u : 0u;
        keep[i] = (sel && (!apply || (double)s > cutoff)) ? 1 : 0;
    }
}

// (elution_group_idx, decoy, rank, precursor_idx) of table row t, as two words that compare like the tuple
__device__ __forceinline__ void order_key(const Table &t, const Prec &p, uint32_t row, uint64_t &hi, uint64_t &lo) {
    const uint32_t pr = row / p.cand_count;
    hi = ((uint64_t)p.elution_group[pr] << 8) | (uint64_t)p.decoy[pr];
    lo = ((uint64_t)t.rank[row] << 32) | (uint64_t)t.precursor_idx[row];
}

// meta[M_UNSORTED] |= rows[i - 1] orders behind rows[i]
__global__ void __launch_bounds__(kBlock) check_kernel(Table t, Prec p, const uint32_t *__restrict__ rows, int64_t k,
                                                       uint32_t *__restrict__ meta) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < k; i += stride) {
        uint64_t ah, al, bh, bl;
        order_key(t, p, rows[i - 1], ah, al);
        order_key(t, p, rows[i], bh, bl);
        bad |= ah > bh || (ah == bh && al > bl);
    }
    if (bad) atomicOr(&meta[M_UNSORTED], 1u);
}

// the keys of the first sort pass: precursor_idx, then rank, then decoy (48 bits)
__global__ void __launch_bounds__(kBlock) low_key_kernel(Table t, Prec p, const uint32_t *__restrict__ rows, int64_t k,
                                                         uint64_t *__restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
        const uint32_t r = rows[i];
        key[i] = (uint64_t)t.precursor_idx[r] | ((uint64_t)t.rank[r] << 32) | ((uint64_t)p.decoy[r / p.cand_count] << 40);
    }
}

// ... and of the second: elution_group_idx
__global__ void __launch_bounds__(kBlock) high_key_kernel(Prec p, const uint32_t *__restrict__ rows, int64_t k,
                                                          uint32_t *__restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride)
        key[i] = p.elution_group[rows[i] / p.cand_count];
}

// head[i] = 1 where a score group starts: (elution_group_idx, decoy, rank) differ from the row before
__global__ void __launch_bounds__(kBlock) head_kernel(Table t, Prec p, const uint32_t *__restrict__ rows, int64_t k,
                                                      uint32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
        uint32_t h = 1;
        if (i > 0) {
            uint64_t ah, al, bh, bl;
            order_key(t, p, rows[i - 1], ah, al);
            order_key(t, p, rows[i], bh, bl);
            h = (ah != bh || (al >> 32) != (bl >> 32)) ? 1u : 0u;
        }
        head[i] = h;
    }
}

// group[i]: inclusive scan of the head flags (score_group_idx + 1), or NULL when every row is its own group.
// A precursor_idx twice in a row of one group sets meta[M_DUP]; has_ref[group] = 1 where a row of the reference
// channel is in the group (has_ref NULL: no reference channel).
__global__ void __launch_bounds__(kBlock) group_kernel(Table t, Prec p, const uint32_t *__restrict__ rows, int64_t k,
                                                       const uint32_t *__restrict__ group, int32_t reference_channel,
                                                       uint8_t *__restrict__ has_ref, uint32_t *__restrict__ meta) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
        const uint32_t r = rows[i];
        if (group && i > 0 && group[i] == group[i - 1] && t.precursor_idx[r] == t.precursor_idx[rows[i - 1]])
            atomicOr(&meta[M_DUP], 1u);
        if (has_ref && (int32_t)p.channel[r / p.cand_count] == reference_channel) has_ref[group ? group[i] - 1 : (uint32_t)i] = 1;
    }
}

struct Soa {
    uint32_t *precursor_idx, *frag_start, *frag_stop;
    uint8_t *rank, *flags, *charge;
    int64_t *scan_start, *scan_stop, *scan_center, *frame_start, *frame_stop, *frame_center;
    float *precursor_mz, *iso;
};

// The candidate SoA in processing order, the position of every row among the score > 0 rows, and the maxima the
// scoring call sizes its tables and chunks with: the longest library slice and the largest scans x cycles tile.
__global__ void __launch_bounds__(kBlock) gather_kernel(Table t, Prec p, const uint32_t *__restrict__ rows, int64_t k,
                                                        const uint32_t *__restrict__ group, const uint8_t *__restrict__ has_ref,
                                                        const uint32_t *__restrict__ pos, int32_t cycle_len, Soa o,
                                                        uint32_t *__restrict__ sel_pos, uint32_t *__restrict__ meta) {
    __shared__ uint32_t s_longest, s_cells, s_skip;
    if (threadIdx.x == 0) s_longest = s_cells = s_skip = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t longest = 0, cells = 0, skip = 0;
    for (int64_t i = tid; i < k; i += stride) {
        const uint32_t r = rows[i], pr = r / p.cand_count;
        const uint32_t fs = p.frag_start[pr], fe = p.frag_stop[pr];
        o.precursor_idx[i] = t.precursor_idx[r];
        o.rank[i] = t.rank[r];
        o.frag_start[i] = fs;
        o.frag_stop[i] = fe;
        o.charge[i] = p.charge[pr];
        o.precursor_mz[i] = p.mz[pr];
        const int64_t s0 = t.scan_start[r], s1 = t.scan_stop[r], f0 = t.frame_start[r], f1 = t.frame_stop[r];
        o.scan_start[i] = s0;
        o.scan_stop[i] = s1;
        o.scan_center[i] = t.scan_center[r];
        o.frame_start[i] = f0;
        o.frame_stop[i] = f1;
        o.frame_center[i] = t.frame_center[r];
        uint8_t flag = 0;
        if (has_ref && !has_ref[group ? group[i] - 1 : (uint32_t)i]) flag = ADH_FLAG_SKIP, ++skip;
        o.flags[i] = flag;
        sel_pos[i] = pos[r];
        longest = max(longest, fe - fs);  // (unsigned: a slice with stop < start wraps, as on the host)
        const int64_t S = max(s1 - s0, (int64_t)1), F = max((f1 - f0) / max(cycle_len, 1) + 1, (int64_t)1);
        cells = max(cells, (uint32_t)min(S * F, (int64_t)0xFFFFFFFFll));
    }
    const int64_t n_iso = (int64_t)k * p.n_iso_cols;
    for (int64_t id = tid; id < n_iso; id += stride) {
        const int64_t i = id / p.n_iso_cols;
        const int j = (int)(id - i * p.n_iso_cols);
        o.iso[id] = p.iso[(int64_t)(rows[i] / p.cand_count) * p.n_iso_cols + j];
    }
    atomicMax(&s_longest, longest);
    atomicMax(&s_cells, cells);
    atomicAdd(&s_skip, skip);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(&meta[M_LONGEST], s_longest);
        atomicMax(&meta[M_CELLS], s_cells);
        if (s_skip) atomicAdd(&meta[M_SKIP], s_skip);
    }
}

// the nine candidate columns (block: u32 columns [8][n] in table order without rank, then rank [n]) and the position
// among the score > 0 rows of the listed rows of the assembled table
__global__ void __launch_bounds__(kBlock) take_kernel(Table t, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ sel_pos,
                                                      const int64_t *__restrict__ list, int64_t n, uint32_t *__restrict__ words,
                                                      uint8_t *__restrict__ rank) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t a = list[i];
        const uint32_t r = rows[a];
        words[0 * n + i] = t.precursor_idx[r];
        words[1 * n + i] = __float_as_uint(t.score[r]);
        words[2 * n + i] = t.scan_center[r];
        words[3 * n + i] = t.scan_start[r];
        words[4 * n + i] = t.scan_stop[r];
        words[5 * n + i] = t.frame_center[r];
        words[6 * n + i] = t.frame_start[r];
        words[7 * n + i] = t.frame_stop[r];
        words[8 * n + i] = sel_pos[a];
        rank[i] = t.rank[r];
    }
}

int need_assembled(adh_handle_t *h, const char *what) {
    if (!h) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL handle");
    if (h->sel.stage != 2)
        return fail(ADH_ERR_NOT_STAGED, std::string(what) + ": no table assembled from a resident selection of the staged run and library");
    return ADH_OK;
}

int assemble(adh_handle_t *h, int32_t apply_cutoff, double score_cutoff, int32_t score_grouped, int32_t reference_channel) {
    adh_handle::Selected &s = h->sel;
    hipStream_t st = h->stream;
    const int64_t N = s.n_prec * s.cand_count;
    if (N >= 0x7FFFFFFFll) return fail(ADH_ERR_UNSUPPORTED, "more than 2^31 rows in the selection table");
    const Table t = table_of(s);
    const Prec p = prec_of(s);
    s.n_kept = s.n_selected = 0;
    s.longest = 0;
    s.im_cells = 1;
    s.assemble_ms = 0.0;
    for (int32_t &v : s.stats) v = 0;
    s.stats[0] = 1;
    // the candidate slab is rewritten: what the last scoring call's tables still need of it is filled in first
    ADH_TRY(materialise_tables(h));
    h->plan = Plan();
    h->cands_uploaded = false;
    sess::DevBufs B;
    sess::EventPair ev;
    uint32_t *meta = nullptr;
    HIP_TRY(B.alloc(&meta, (size_t)M_WORDS));
    HIP_TRY(hipMemsetAsync(meta, 0, M_WORDS * 4, st));
    ADH_TRY(ev.begin(st));
    int64_t K = 0;
    uint32_t *rows_a = nullptr, *pos = nullptr;
    if (N > 0) {
        uint32_t *selected = nullptr, *iota = nullptr, *n_sel = nullptr;
        uint8_t *keep = nullptr;
        HIP_TRY(B.alloc(&selected, (size_t)N + 1));
        HIP_TRY(B.alloc(&pos, (size_t)N + 1));
        HIP_TRY(B.alloc(&keep, (size_t)N));
        HIP_TRY(B.alloc(&iota, (size_t)N));
        HIP_TRY(B.alloc(&rows_a, (size_t)N));
        HIP_TRY(B.alloc(&n_sel, (size_t)1));
        hipLaunchKernelGGL(flag_kernel, dim3(grid_for(N + 1)), dim3(kBlock), 0, st, t.score, N, (int)(apply_cutoff != 0), score_cutoff,
                           selected, keep);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::exclusive_sum(B, (const uint32_t *)selected, pos, N + 1, st));
        hipLaunchKernelGGL(sess::iota_kernel, dim3(grid_for(N)), dim3(kBlock), 0, st, iota, N);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::select_flagged(B, (const uint32_t *)iota, (const uint8_t *)keep, rows_a, n_sel, N, st));
        uint32_t counts[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&counts[0], n_sel, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&counts[1], pos + N, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h->d2h_bytes += 8;
        K = counts[0];
        s.n_selected = counts[1];
    }
    s.n_kept = K;
    ADH_TRY(cand_reserve(h, K, s.n_iso_cols));
    h->cs.d.flags = h->cs.flags;
    ADH_TRY(grow_device(&h->sel_rows, &h->sel_rows_bytes, (size_t)std::max<int64_t>(K, 1) * 8, (size_t)K + 256));
    uint32_t *const trow = static_cast<uint32_t *>(h->sel_rows), *const sel_pos = trow + std::max<int64_t>(K, 1);
    if (K > 0) {
        hipLaunchKernelGGL(check_kernel, dim3(grid_for(K)), dim3(kBlock), 0, st, t, p, (const uint32_t *)rows_a, K, meta);
        HIP_TRY(hipGetLastError());
        uint32_t unsorted = 0;
        HIP_TRY(hipMemcpyAsync(&unsorted, meta + M_UNSORTED, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h->d2h_bytes += 4;
        if (unsorted) {
            // np.lexsort((precursor_idx, rank, decoy, elution_group_idx)): stable passes, least significant key first
            uint64_t *k1 = nullptr, *k1s = nullptr;
            uint32_t *rows_b = nullptr, *k2 = nullptr, *k2s = nullptr;
            HIP_TRY(B.alloc(&k1, (size_t)K));
            HIP_TRY(B.alloc(&k1s, (size_t)K));
            HIP_TRY(B.alloc(&rows_b, (size_t)K));
            HIP_TRY(B.alloc(&k2, (size_t)K));
            HIP_TRY(B.alloc(&k2s, (size_t)K));
            hipLaunchKernelGGL(low_key_kernel, dim3(grid_for(K)), dim3(kBlock), 0, st, t, p, (const uint32_t *)rows_a, K, k1);
            HIP_TRY(hipGetLastError());
            ADH_TRY(sess::sort_pairs(B, (const uint64_t *)k1, k1s, (const uint32_t *)rows_a, rows_b, K, 48, st));
            hipLaunchKernelGGL(high_key_kernel, dim3(grid_for(K)), dim3(kBlock), 0, st, p, (const uint32_t *)rows_b, K, k2);
            HIP_TRY(hipGetLastError());
            ADH_TRY(sess::sort_pairs(B, (const uint32_t *)k2, k2s, (const uint32_t *)rows_b, trow, K, 32, st));
            s.stats[0] = 0;
            s.stats[1] = 2;
        } else {
            HIP_TRY(hipMemcpyAsync(trow, rows_a, (size_t)K * 4, hipMemcpyDeviceToDevice, st));
        }
        uint32_t *group = nullptr;
        uint8_t *has_ref = nullptr;
        if (score_grouped) {
            uint32_t *head = nullptr;
            HIP_TRY(B.alloc(&head, (size_t)K));
            HIP_TRY(B.alloc(&group, (size_t)K));
            hipLaunchKernelGGL(head_kernel, dim3(grid_for(K)), dim3(kBlock), 0, st, t, p, (const uint32_t *)trow, K, head);
            HIP_TRY(hipGetLastError());
            ADH_TRY(sess::inclusive_sum(B, (const uint32_t *)head, group, K, st));
            s.stats[2] = 1;
        }
        if (reference_channel >= 0) {
            HIP_TRY(B.alloc(&has_ref, (size_t)K));
            HIP_TRY(hipMemsetAsync(has_ref, 0, (size_t)K, st));
        }
        if (group || has_ref) {
            hipLaunchKernelGGL(group_kernel, dim3(grid_for(K)), dim3(kBlock), 0, st, t, p, (const uint32_t *)trow, K,
                               (const uint32_t *)group, reference_channel, has_ref, meta);
            HIP_TRY(hipGetLastError());
        }
        const CandSlab &c = h->cs;
        const Soa o{const_cast<uint32_t *>(c.d.precursor_idx), const_cast<uint32_t *>(c.d.frag_start), const_cast<uint32_t *>(c.d.frag_stop),
                    const_cast<uint8_t *>(c.d.rank), c.flags, const_cast<uint8_t *>(c.d.charge),
                    const_cast<int64_t *>(c.d.scan_start), const_cast<int64_t *>(c.d.scan_stop), const_cast<int64_t *>(c.d.scan_center),
                    const_cast<int64_t *>(c.d.frame_start), const_cast<int64_t *>(c.d.frame_stop), const_cast<int64_t *>(c.d.frame_center),
                    const_cast<float *>(c.d.precursor_mz), c.iso};
        const int32_t cycle_len = h->tims_staged ? h->tims.cycle_len : 1;
        const int64_t work = std::max<int64_t>(K * (int64_t)std::max(s.n_iso_cols, 1), K);
        hipLaunchKernelGGL(gather_kernel, dim3(grid_for(work)), dim3(kBlock), 0, st, t, p, (const uint32_t *)trow, K,
                           (const uint32_t *)group, (const uint8_t *)has_ref, (const uint32_t *)pos, cycle_len, o, sel_pos, meta);
        HIP_TRY(hipGetLastError());
    }
    uint32_t m[M_WORDS] = {0};
    HIP_TRY(hipMemcpyAsync(m, meta, M_WORDS * 4, hipMemcpyDeviceToHost, st));
    ADH_TRY(ev.end(st, s.assemble_ms));
    HIP_TRY(hipStreamSynchronize(st));
    h->d2h_bytes += M_WORDS * 4;
    if (m[M_DUP]) return fail(ADH_ERR_INVALID_ARGUMENT, "precursor_idx must be unique within a score group");
    s.longest = m[M_LONGEST];
    s.im_cells = std::max<int64_t>(m[M_CELLS], 1);
    s.stats[3] = (int32_t)m[M_SKIP];
    s.stage = 2;
    return ADH_OK;
}

}  // namespace hov

int adh_select_candidates_resident(adh_handle_t *h, const adh_precursors_t *pc, const adh_selection_config_t *cfg,
                                   const float *kernel, int32_t k_rows, int32_t k_cols, const uint32_t *elution_group_idx,
                                   const uint8_t *decoy, const uint8_t *channel) {
    if (!h || !pc || !cfg) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h->comm_attached())
        return fail(ADH_ERR_UNSUPPORTED, "resident selection with a communicator attached (the table is a shard plus a gather)");
    if (pc->n > 0 && (!elution_group_idx || !decoy || !channel))
        return fail(ADH_ERR_INVALID_ARGUMENT, "elution_group_idx / decoy / channel column is NULL");
    if (pc->n > 0 && !pc->isotope_intensity) return fail(ADH_ERR_INVALID_ARGUMENT, "isotope_intensity is NULL");
    adh_candidate_table_t shape{};
    shape.n = pc->n * cfg->candidate_count;
    const SelIds ids{elution_group_idx, decoy, channel};
    return select_candidates_run(h, pc, cfg, kernel, k_rows, k_cols, &shape, &ids);
}

int adh_assemble_selected(adh_handle_t *h, int32_t apply_cutoff, double score_cutoff, int32_t score_grouped,
                          int32_t reference_channel, int64_t *n_selected, int64_t *n_kept, int32_t *was_sorted) {
    if (!h || !n_selected || !n_kept || !was_sorted) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h->sel.stage < 1) return fail(ADH_ERR_NOT_STAGED, "no resident selection of the staged run and library in the slab");
    HIP_TRY(hipSetDevice(h->device));
    h->sel.stage = 1;
    const int rc = hov::assemble(h, apply_cutoff, score_cutoff, score_grouped, reference_channel);
    if (rc != ADH_OK) {
        (void)hipStreamSynchronize(h->stream);  // (nothing of the call's temporaries is still read when they are freed)
        return rc;
    }
    *n_selected = h->sel.n_selected;
    *n_kept = h->sel.n_kept;
    *was_sorted = h->sel.stats[0];
    return ADH_OK;
}

int adh_select_handover_stats(adh_handle_t *h, int32_t *stats, double *assemble_ms) {
    if (!h || !stats) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int i = 0; i < 4; ++i) stats[i] = h->sel.stats[i];
    if (assemble_ms) *assemble_ms = h->sel.assemble_ms;
    return ADH_OK;
}

int adh_score_selected_resident(adh_handle_t *h, const adh_scoring_config_t *cfg) {
    if (!h || !cfg) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h->comm_attached())
        return fail(ADH_ERR_UNSUPPORTED, "resident scoring with a communicator attached (the tables are a shard plus a gather)");
    int rc = hov::need_assembled(h, "adh_score_selected_resident");
    if (rc != ADH_OK) return rc;
    adh_candidates_t c{};
    c.n = h->sel.n_kept;
    c.n_isotope_cols = h->sel.n_iso_cols;
    adh_output_t shape{};
    shape.n = c.n;
    // (the width take::resident_shape picks from the host columns)
    shape.top_k = c.n == 0 ? 1 : (int32_t)std::max<uint32_t>(1u, std::min<uint32_t>(cfg->top_k_fragments, std::max<uint32_t>(h->sel.longest, 1u)));
    return score_pipeline(h, &c, cfg, &shape, nullptr, true, true);
}

int adh_selected_ids(adh_handle_t *h, uint32_t *table_row, uint8_t *rank, int64_t n) {
    int rc = hov::need_assembled(h, "adh_selected_ids");
    if (rc != ADH_OK) return rc;
    if (n != h->sel.n_kept) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_selected_ids: n differs from the rows of the assembled table");
    if (n == 0) return ADH_OK;
    if (!table_row || !rank) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(table_row, h->sel_rows, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(rank, h->cs.d.rank, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->d2h_bytes += (uint64_t)n * 5;
    return ADH_OK;
}

int adh_take_selected(adh_handle_t *h, const int64_t *rows, int64_t n, adh_candidate_table_t *out, uint32_t *selected_pos) {
    if (!h || !out || (n > 0 && !rows)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 0 || out->n != n) return fail(ADH_ERR_INVALID_ARGUMENT, "take_selected: row count");
    int rc = hov::need_assembled(h, "adh_take_selected");
    if (rc != ADH_OK) return rc;
    const int64_t K = h->sel.n_kept;
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= K) return fail(ADH_ERR_INVALID_ARGUMENT, "take_selected: row outside the assembled table");
    if (n == 0) return ADH_OK;
    void *const host_u32[8] = {out->precursor_idx, out->score, out->scan_center, out->scan_start, out->scan_stop,
                               out->frame_center, out->frame_start, out->frame_stop};
    for (void *p : host_u32)
        if (!p) return fail(ADH_ERR_INVALID_ARGUMENT, "candidate table buffer is NULL");
    if (!out->rank) return fail(ADH_ERR_INVALID_ARGUMENT, "candidate table buffer is NULL");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    sess::DevBufs B;
    int64_t *d_list = nullptr;
    uint32_t *words = nullptr;
    uint8_t *d_rank = nullptr;
    HIP_TRY(B.upload(&d_list, rows, (size_t)n, st));
    HIP_TRY(B.alloc(&words, (size_t)n * 9));
    HIP_TRY(B.alloc(&d_rank, (size_t)n));
    const uint32_t *trow = static_cast<const uint32_t *>(h->sel_rows);
    hipLaunchKernelGGL(hov::take_kernel, dim3(hov::grid_for(n)), dim3(hov::kBlock), 0, st, hov::table_of(h->sel), trow,
                       trow + std::max<int64_t>(K, 1), (const int64_t *)d_list, n, words, d_rank);
    hipError_t e = hipGetLastError();
    for (int f = 0; f < 8 && e == hipSuccess; ++f)
        e = hipMemcpyAsync(host_u32[f], words + (size_t)f * n, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && selected_pos) e = hipMemcpyAsync(selected_pos, words + (size_t)8 * n, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out->rank, d_rank, (size_t)n, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);  // (before the temporaries go, whatever happened)
    if (e != hipSuccess || e2 != hipSuccess)
        return fail(ADH_ERR_HIP, std::string("take_selected: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    h->d2h_bytes += (uint64_t)n * (selected_pos ? 37 : 33);
    return ADH_OK;
}
