// adh_resident_append.hip - accumulated resident tables for the optimisation loop
// (alphadia/workflow/peptidecentric/optimization_handler.py:220-456): every step scores one more batch of elution
// groups and runs the FDR stage over ALL rows scored since the last reset (OptimizationLock.features_df).
//
// adh_score_candidates_resident_append scores a batch into a scratch table (tables[0], as adh_score_candidates_resident
// does), fills in its id and library columns from the candidate table and library of this call (materialise_tables:
// the rows keep the library values of the time they were scored, whatever is staged later), and moves its rows behind
// the accumulated ones.  The accumulated tables are laid out for a row capacity and a slot width (layout_tables); a
// batch that needs more rows, or wider slots because its longest library slice is longer, first moves the live rows
// into a new layout in HBM (relayout_kernel, zero-filling the new slots).  Capacity grows geometrically, so the
// doubling batch plan of the lock moves O(n) bytes in all.  Afterwards the accumulated buffer is swapped into
// tables[0]: adh_get_device_tables, adh_fdr_resident and adh_take_rows see rows [0, n) of every batch.
// Included by adh_api.hip (shares its error helpers and the handle).

namespace acc {

// dst rows [row0, row0 + n) of a per-row table of width wd from src rows [0, n) of width ws (<= wd), slots j >= ws
// zeroed: the slots a wider layout adds (an empty slot is all zeros, as the scoring call's memset leaves it)
template <typename T>
__global__ void __launch_bounds__(256) relayout_kernel(const T *__restrict__ src, int ws, T *__restrict__ dst, int wd,
                                                       int64_t n, int64_t row0) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = n * (int64_t)wd;
    T *const out = dst + row0 * (int64_t)wd;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / wd;
        const int j = (int)(e - r * wd);
        out[e] = j < ws ? src[r * (int64_t)ws + j] : T(0);
    }
}

// valid rows and their leading filled fragment slots among rows [0, n): a wavefront sum, one atomic per wavefront
__global__ void __launch_bounds__(256) count_kernel(const uint8_t *__restrict__ valid, const uint16_t *__restrict__ lib_slot,
                                                    int64_t n, int top_k, unsigned long long *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long rows = 0, slots = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        if (!valid[r]) continue;
        const uint16_t *s = lib_slot + r * (int64_t)top_k;
        int k = 0;
        while (k < top_k && s[k]) ++k;  // (filled slots are the leading ones: candidate.py:403-442)
        rows += 1;
        slots += (unsigned long long)k;
    }
    for (int off = warpSize / 2; off > 0; off /= 2) {
        rows += __shfl_down(rows, off);
        slots += __shfl_down(slots, off);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0 && (rows | slots)) {
        atomicAdd(out, rows);
        atomicAdd(out + 1, slots);
    }
}

// the accumulated geometry for `live` rows in a (cap, w) layout plus a batch of n rows of width wb: the new capacity
// and width, and whether the live rows move (tests/test_optimization_resident.py mirrors this rule)
struct Geometry {
    int64_t cap;
    int top_k;
    bool relayout;
};
inline Geometry grow(int64_t live, int64_t cap, int w, int64_t n, int wb) {
    if (live == 0) return {std::max<int64_t>(n, 1), wb, false};  // (nothing to move: the batch sets the layout)
    const int64_t need = live + n;
    Geometry g{need > cap ? std::max(need, 2 * cap) : cap, std::max(w, wb), false};
    g.relayout = g.cap != cap || g.top_k != w;
    return g;
}

// rows [0, n) of the tables `src` (width ws) into rows [row0, row0 + n) of `dst` (width wd >= ws), field by field:
// a field whose width does not change is one contiguous run of bytes on both sides (a DMA copy), the fragment tables
// of a wider layout go through relayout_kernel
int move_rows(adh_handle *h, const adh_output_t &src, int ws, adh_output_t &dst, int wd, int64_t n, int64_t row0) {
    if (n == 0) return ADH_OK;
    hipStream_t st = h->stream;
    for (int i = 0; i < kNumOutFields; ++i) {
        const OutFieldDesc &f = kOutFields[i];
        const unsigned char *s = static_cast<const unsigned char *>(*out_member(const_cast<adh_output_t *>(&src), f));
        unsigned char *d = static_cast<unsigned char *>(*out_member(&dst, f));
        if (f.per_row >= 0 || ws == wd) {
            const size_t row_bytes = out_row_bytes(f, wd);
            HIP_TRY(hipMemcpyAsync(d + (size_t)row0 * row_bytes, s, (size_t)n * row_bytes, hipMemcpyDeviceToDevice, st));
            continue;
        }
        const int64_t total = n * (int64_t)wd;
        const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), block(256);
        switch (f.elem) {
        case 1:
            hipLaunchKernelGGL(relayout_kernel<uint8_t>, grid, block, 0, st, s, ws, d, wd, n, row0);
            break;
        case 2:
            hipLaunchKernelGGL(relayout_kernel<uint16_t>, grid, block, 0, st, reinterpret_cast<const uint16_t *>(s), ws,
                               reinterpret_cast<uint16_t *>(d), wd, n, row0);
            break;
        case 4:
            hipLaunchKernelGGL(relayout_kernel<uint32_t>, grid, block, 0, st, reinterpret_cast<const uint32_t *>(s), ws,
                               reinterpret_cast<uint32_t *>(d), wd, n, row0);
            break;
        default:
            return fail(ADH_ERR_HIP, "relayout: unexpected element size");
        }
        HIP_TRY(hipGetLastError());
    }
    return ADH_OK;
}

}  // namespace acc

extern "C" {

int adh_score_candidates_resident_append(adh_handle_t *h, const adh_candidates_t *c, const adh_scoring_config_t *cfg,
                                         int64_t *first_row) {
    if (!first_row) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    adh_output_t shape{};
    int rc = take::resident_shape(h, c, cfg, shape);
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const bool had = h->acc_live;
    const int64_t live = had ? h->acc_rows : 0, cap = had ? h->acc_cap : 0;
    const int w = had ? h->acc_top_k : 0;
    // tables[0] becomes the scratch table of this batch, acc_spare holds the accumulated rows
    if (had) std::swap(h->tables[0], h->acc_spare);
    auto abandon = [h](int code) {  // a failed append ends the accumulation (what is left is one batch's scratch)
        h->acc_live = false;
        h->acc_rows = 0;
        h->tables_current = false;
        return code;
    };
    rc = score_pipeline(h, c, cfg, &shape, nullptr, true);  // (ends the accumulation too: restored below)
    if (rc == ADH_OK && h->last_tables != 0) rc = fail(ADH_ERR_HIP, "resident scoring did not use table slot 0");
    if (rc == ADH_OK) rc = materialise_tables(h);  // the batch's ids and library columns, as staged now
    if (rc != ADH_OK) return abandon(rc);
    const int64_t n = c->n;
    const int wb = shape.top_k;
    const acc::Geometry g = acc::grow(live, cap, w, n, wb);
    DevTables &acc_t = h->acc_spare;
    if (g.relayout) {
        DevTables fresh;
        rc = ensure_tables_in(fresh, g.cap, g.top_k);
        if (rc != ADH_OK) return abandon(rc);
        rc = acc::move_rows(h, acc_t.view, w, fresh.view, g.top_k, live, 0);
        if (rc == ADH_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(ADH_ERR_HIP, "relayout failed");
        if (rc != ADH_OK) {
            (void)hipFree(fresh.base);
            return abandon(rc);
        }
        if (acc_t.base) (void)hipFree(acc_t.base);
        acc_t = fresh;
    } else if (live == 0) {
        rc = ensure_tables_in(acc_t, g.cap, g.top_k);  // (reuses the spare buffer when it is large enough)
        if (rc != ADH_OK) return abandon(rc);
    }
    if (live + n > acc_t.rows || wb > acc_t.top_k) return abandon(fail(ADH_ERR_HIP, "accumulated tables too small"));
    rc = acc::move_rows(h, h->tables[0].view, wb, acc_t.view, acc_t.top_k, n, live);
    if (rc == ADH_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(ADH_ERR_HIP, "append copy failed");
    if (rc != ADH_OK) return abandon(rc);
    std::swap(h->tables[0], h->acc_spare);  // (acc_t now names the scratch table)
    h->tables[0].partial = false;
    h->last_tables = 0;
    h->last_rows = live + n;
    h->acc_rows = live + n;
    h->acc_cap = h->tables[0].rows;
    h->acc_top_k = h->tables[0].top_k;
    h->acc_live = true;
    h->tables_current = true;
    *first_row = live;
    return ADH_OK;
}

int adh_resident_reset(adh_handle_t *h) {
    if (!h) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL handle");
    h->acc_live = false;
    h->acc_rows = 0;
    if (h->last_tables >= 0) {
        h->last_rows = 0;
        h->tables_current = true;  // (empty tables: nothing in them refers to a staged run or library)
    }
    return ADH_OK;
}

int adh_resident_counts(adh_handle_t *h, int64_t *valid_rows, int64_t *filled_slots) {
    if (!h || !valid_rows || !filled_slots) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h->last_tables < 0 || !h->tables_current)
        return fail(ADH_ERR_NOT_STAGED, "no scored tables of the staged run and library on the device");
    *valid_rows = *filled_slots = 0;
    const int64_t n = h->last_rows;
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (!h->acc_counts) HIP_TRY(hipMalloc(&h->acc_counts, 256));
    unsigned long long *const d = static_cast<unsigned long long *>(h->acc_counts);
    const adh_output_t &tab = h->tables[h->last_tables].view;
    hipStream_t st = h->stream;
    HIP_TRY(hipMemsetAsync(d, 0, 16, st));
    hipLaunchKernelGGL(acc::count_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, st,
                       tab.valid, tab.fragment_lib_slot, n, tab.top_k, d);
    HIP_TRY(hipGetLastError());
    unsigned long long got[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(got, d, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->d2h_bytes += 16;
    *valid_rows = (int64_t)got[0];
    *filled_slots = (int64_t)got[1];
    return ADH_OK;
}

}  // extern "C"
