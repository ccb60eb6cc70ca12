// adh_candidate_library.hip - the candidate library of transfer-library requantification built where it is used:
// adh_stage_candidate_library takes the identified precursors as sequence bytes and modification lists (a few dozen
// bytes each) and a kernel writes the 32-byte LibRec records of ALL their b/y-type ions at every fragment charge into
// HBM, calibrating the m/z on the way when a model is given (calib::predict_row, as the pack kernel of adh_stage_lib.hip).
// What the reference builds on the host (_build_candidate_speclib_flat, transfer_library_requantification_handler.py
// :140-240: calc_fragment_mz_df + parse_base_library, 13-20 M rows for 300 000 PSMs) and this package would upload
// column by column never crosses the link: only mz_library (4 bytes per row) and the predictions (8) come back.
//
// The masses (a restatement of alphabase's rules, see alphadia_amd/transfer_requantification.py: host_candidate_library):
//   m[j] = aa_mass[residue j] (+ the masses of its modifications, in list order; site 0 -> residue 0, -1 -> L-1,
//   s >= 1 -> s-1);  B[i] = m[0] + ... + m[i] summed left to right in float64;  pep = B[L-1] + mass_h2o;
//   Y[i] = pep - B[i];  row i * n_series + s of the precursor: float32((from_nterm ? B[i] : Y[i]) / charge_s + mass_proton).
// The build keeps -ffp-contract=off and no fast-math: add, subtract and divide are the IEEE operations of NumPy, on
// the device and in the host team that rebuilds the mirror of the records from the same sums in the same order.
//
// Kernel shape: a block owns ROWS consecutive rows of the library (the scan of the row counts tells which precursors
// they belong to: the one that holds its first row up to the one that holds its last).  The residue masses of those
// precursors go into LDS side by side, one thread per precursor adds its modifications and runs the prefix chain in
// place - at most 255 dependent adds, in sequence order, no cross-lane scan - and then every thread produces records,
// one per row, as two 16-byte stores.  A precursor cut by a block edge has its chain run by both blocks.
// A pipeline chunk (ADH_CALIBRATION_CHUNK_ROWS rows, a whole number of blocks) runs on one of the two slots of
// adh_stage_fragments_columns, which carry mz_library and the predictions of the chunk back.
// Included by adh_api.hip after adh_stage_lib.hip.

namespace candlib {

constexpr int ROWS = 1024;  // rows per block
constexpr int MAX_L = 255;  // number and position are uint8
static_assert(stagelib::C % ROWS == 0, "a pipeline chunk is a whole number of blocks");
// Precursors of a block: the one holding its first row, those wholly inside (each has a row: at most ROWS), the one
// holding its last row.  Their residues: the inner ones have sum (L - 1) <= ROWS, so sum L <= 2 * ROWS; the outer
// two at most MAX_L each.
constexpr int LDS_PRECURSORS = ROWS + 2;
constexpr int LDS_RESIDUES = 2 * ROWS + 2 * MAX_L;

struct Series {
    int32_t n;
    uint8_t type[ADH_CANDIDATE_LIBRARY_MAX_SERIES], from_nterm[ADH_CANDIDATE_LIBRARY_MAX_SERIES],
        charge[ADH_CANDIDATE_LIBRARY_MAX_SERIES];
};

// the device copies of the inputs; residues / mod_* start at the first precursor's entries (res0 / mod0)
struct Tables {
    const uint8_t *residues;
    const int64_t *seq_offset, *mod_offset;  // [n + 1]
    const int32_t *mod_site;
    const double *mod_mass;
    const double *aa_mass;  // [128]
    const uint32_t *start;  // [n + 1]: exclusive scan of the row counts, start[n] = total
    int64_t n, res0, mod0;
    double mass_proton, mass_h2o;
};

// residue a modification site names, or -1
__host__ __device__ inline int site_residue(int32_t site, int L) {
    const int j = site == 0 ? 0 : site == -1 ? L - 1 : site - 1;
    return j >= 0 && j < L ? j : -1;
}

// mz_library of a row from the prefix of its position and of the whole peptide
__host__ __device__ inline float row_mz_library(double b_i, double b_last, int from_nterm, uint32_t charge, double mass_proton,
                                                double mass_h2o) {
    const double pep = b_last + mass_h2o;
    const double v = from_nterm ? b_i : pep - b_i;
    return (float)(v / (double)charge + mass_proton);
}

// largest k in [0, n) with a[k] <= v (a ascending, a[0] <= v)
template <typename A>
__host__ __device__ inline int64_t holder(const A *a, int64_t n, uint32_t v) {
    int64_t lo = 0, hi = n;  // a[lo] <= v < a[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Rows [row0 + blockIdx.x * ROWS, ...) of the library, at most ROWS of them and none at or past row0 + rows.
// out, mzl and y are the chunk's: row r of the library is element r - row0.
__global__ void __launch_bounds__(256) build_kernel(calib::Model m, int calibrate, Tables t, Series ser, int64_t row0,
                                                    int64_t rows, LibRec *__restrict__ out, float *__restrict__ mzl,
                                                    double *__restrict__ y) {
    __shared__ double B[LDS_RESIDUES];
    __shared__ uint32_t s_start[LDS_PRECURSORS + 1];  // first row of the block's precursors and of the one after them
    __shared__ uint32_t s_off[LDS_PRECURSORS + 1];    // their first residue in B, likewise
    __shared__ int64_t s_p[2];
    __shared__ uint8_t s_type[ADH_CANDIDATE_LIBRARY_MAX_SERIES], s_from[ADH_CANDIDATE_LIBRARY_MAX_SERIES],
        s_charge[ADH_CANDIDATE_LIBRARY_MAX_SERIES];  // (indexed per row: not from the kernel arguments)
    const int tid = threadIdx.x;
    const int64_t g0 = row0 + (int64_t)blockIdx.x * ROWS, g1 = g0 + ROWS < row0 + rows ? g0 + ROWS : row0 + rows;
    if (g0 >= g1) return;
    if (tid < 2) s_p[tid] = holder(t.start, t.n, (uint32_t)(tid == 0 ? g0 : g1 - 1));
    if (tid < ser.n) {
        s_type[tid] = ser.type[tid];
        s_from[tid] = ser.from_nterm[tid];
        s_charge[tid] = ser.charge[tid];
    }
    __syncthreads();
    const int64_t p_first = s_p[0];
    const int np = (int)(s_p[1] - p_first) + 1;
    const int64_t seq0 = t.seq_offset[p_first];
    const int n_res = (int)(t.seq_offset[p_first + np] - seq0);
    if (np > LDS_PRECURSORS || n_res > LDS_RESIDUES) return;  // (not reached: the entry checks every length)
    for (int k = tid; k <= np; k += blockDim.x) {
        s_start[k] = t.start[p_first + k];
        s_off[k] = (uint32_t)(t.seq_offset[p_first + k] - seq0);
    }
    for (int k = tid; k < n_res; k += blockDim.x) B[k] = t.aa_mass[t.residues[seq0 - t.res0 + k] & 127];
    __syncthreads();
    // one thread per precursor: its modifications in list order, then the chain in sequence order
    for (int q = tid; q < np; q += blockDim.x) {
        const int base = (int)s_off[q], L = (int)s_off[q + 1] - base;
        const int64_t k1 = t.mod_offset[p_first + q + 1] - t.mod0;
        for (int64_t k = t.mod_offset[p_first + q] - t.mod0; k < k1; ++k) {
            const int j = site_residue(t.mod_site[k], L);
            if (j >= 0) B[base + j] = B[base + j] + t.mod_mass[k];
        }
        double acc = B[base];
        for (int i = 1; i < L; ++i) {
            acc = acc + B[base + i];
            B[base + i] = acc;
        }
    }
    __syncthreads();
    const uint32_t S = (uint32_t)ser.n;
    for (int64_t r = g0 + tid; r < g1; r += blockDim.x) {
        const int q = (int)holder(s_start, np, (uint32_t)r);
        const uint32_t rel = (uint32_t)r - s_start[q];
        const uint32_t i = rel / S, s = rel - i * S;
        const int base = (int)s_off[q], L = (int)s_off[q + 1] - base;
        const int from = s_from[s];
        const uint32_t charge = s_charge[s];
        const float xl = row_mz_library(B[base + i], B[base + L - 1], from, charge, t.mass_proton, t.mass_h2o);
        float v = xl;
        if (calibrate) {
            const double p = calib::predict_row<float>(m, xl);
            y[r - row0] = p;
            v = calib::staged_f32(p);
        }
        mzl[r - row0] = xl;
        uint32_t w[8];
        stagelib::record_words(xl, v, 1.0f, s_type[s], 0, charge, from ? i + 1 : (uint32_t)L - 1 - i, i, 0, w);
        uint4 *o = reinterpret_cast<uint4 *>(out + (r - row0));  // (LibRec is 16-byte aligned)
        o[0] = make_uint4(w[0], w[1], w[2], w[3]);
        o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}

}  // namespace candlib

int adh_stage_candidate_library(adh_handle_t *h, const adh_candidate_library_t *c, const adh_loess_model_t *model,
                                uint32_t *flat_frag_start_idx, uint32_t *flat_frag_stop_idx, float *mz_library_out,
                                double *mz_out) {
    using namespace candlib;
    constexpr int64_t C = stagelib::C;
    if (!h || !c) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c->n < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "negative precursor count");
    if (c->n_series <= 0) return fail(ADH_ERR_INVALID_ARGUMENT, "no fragment series");
    if (c->n_series > ADH_CANDIDATE_LIBRARY_MAX_SERIES)
        return fail(ADH_ERR_UNSUPPORTED, "more than " + std::to_string(ADH_CANDIDATE_LIBRARY_MAX_SERIES) + " fragment series");
    if (!c->aa_mass || !c->series_type || !c->series_from_nterm || !c->series_charge)
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL mass table or series column");
    const int64_t n = c->n;
    if (n > 0 && (!c->seq_offset || !c->mod_offset || !c->residues || !flat_frag_start_idx || !flat_frag_stop_idx))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL precursor column");
    // every precursor is checked, and the scan taken, before anything of the handle is touched
    const int S = c->n_series;
    std::vector<uint32_t> start((size_t)n + 1, 0u);
    int64_t res0 = 0, res1 = 0, mod0 = 0, mod1 = 0;
    if (n > 0) {
        res0 = c->seq_offset[0], res1 = c->seq_offset[n], mod0 = c->mod_offset[0], mod1 = c->mod_offset[n];
        if (res0 < 0 || mod0 < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "negative offset");
        uint64_t total = 0;
        for (int64_t p = 0; p < n; ++p) {
            const int64_t L = c->seq_offset[p + 1] - c->seq_offset[p];
            const int64_t k0 = c->mod_offset[p], k1 = c->mod_offset[p + 1];
            if (L < 2 || L > MAX_L)
                return fail(ADH_ERR_INVALID_ARGUMENT, "precursor " + std::to_string(p) + ": " + std::to_string(L) +
                                                          " residues (2 .. 255 are supported)");
            if (k1 < k0) return fail(ADH_ERR_INVALID_ARGUMENT, "mod_offset decreases at precursor " + std::to_string(p));
            if (k1 > k0 && (!c->mod_site || !c->mod_mass)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL modification column");
            for (int64_t k = k0; k < k1; ++k)
                if (c->mod_site[k] < -1 || c->mod_site[k] > L)
                    return fail(ADH_ERR_INVALID_ARGUMENT, "precursor " + std::to_string(p) + ": modification site " +
                                                              std::to_string(c->mod_site[k]) + " outside [-1, nAA]");
            start[(size_t)p] = (uint32_t)total;
            total += (uint64_t)(L - 1) * (uint64_t)S;
            if (total >= 0xFFFFFFFFull) return fail(ADH_ERR_INVALID_ARGUMENT, "the library would have 2^32 rows or more");
        }
        start[(size_t)n] = (uint32_t)total;
        uint8_t high = 0;
        for (int64_t k = res0; k < res1; ++k) high |= c->residues[k];
        if (high & 0x80) return fail(ADH_ERR_INVALID_ARGUMENT, "a residue byte is 128 or above");
    }
    const int64_t total = (int64_t)start[(size_t)n];
    calib::Model m{};
    if (model) {
        const int rc_m = calib::load_model(model, m);
        if (rc_m != ADH_OK) return rc_m;
    }
    Series ser{};
    ser.n = S;
    for (int s = 0; s < S; ++s) {
        ser.type[s] = c->series_type[s];
        ser.from_nterm[s] = c->series_from_nterm[s] ? 1 : 0;
        ser.charge[s] = c->series_charge[s];
    }
    h->calib_kernel_ms = 0.0;
    HIP_TRY(hipSetDevice(h->device));
    {
        const int rc_l = calib::library_changes(h);
        if (rc_l != ADH_OK) return rc_l;
    }
    h->lib_buf.release();
    h->lib_staged = false;
    h->d_lib = nullptr;
    h->n_lib = 0;
    LibRec *lib = nullptr;
    HIP_TRY(hipMalloc(&lib, (size_t)std::max<int64_t>(total, 1) * sizeof(LibRec)));
    h->lib_buf.ptrs.push_back(lib);
    std::vector<double> own;  // the mirror takes the float32 of the predictions: without mz_out they land here
    if (model && !mz_out && total > 0) {
        own.resize((size_t)total);
        mz_out = own.data();
    }
    struct Inputs {  // the device copies of the precursors live for this call
        DeviceBuffers b;
        ~Inputs() { b.release(); }
    } in;
    Tables t{};
    if (total > 0) {
        const int rc_s = calib::ensure_slots(h->lib_slots, stagelib::SLOT_BYTES);
        if (rc_s != ADH_OK) return rc_s;
        const int32_t no_site = 0;
        const double no_mass = 0.0;
        const int64_t n_mod = mod1 - mod0;
        int rc_u = upload(in.b, c->residues + res0, res1 - res0, &t.residues, h->stream);
        if (rc_u == ADH_OK) rc_u = upload(in.b, c->seq_offset, n + 1, &t.seq_offset, h->stream);
        if (rc_u == ADH_OK) rc_u = upload(in.b, c->mod_offset, n + 1, &t.mod_offset, h->stream);
        if (rc_u == ADH_OK) rc_u = upload(in.b, n_mod ? c->mod_site + mod0 : &no_site, n_mod, &t.mod_site, h->stream);
        if (rc_u == ADH_OK) rc_u = upload(in.b, n_mod ? c->mod_mass + mod0 : &no_mass, n_mod, &t.mod_mass, h->stream);
        if (rc_u == ADH_OK) rc_u = upload(in.b, c->aa_mass, (int64_t)128, &t.aa_mass, h->stream);
        if (rc_u == ADH_OK) rc_u = upload(in.b, start.data(), n + 1, &t.start, h->stream);
        if (rc_u != ADH_OK) return rc_u;
        t.n = n, t.res0 = res0, t.mod0 = mod0;
        t.mass_proton = c->mass_proton, t.mass_h2o = c->mass_h2o;
    }
    hipStream_t streams[2] = {h->stream, h->stream_out};
    const int64_t n_chunks = (total + C - 1) / C;
    auto finish = [&](int64_t ch) -> int {
        adh_handle::CalibSlot &s = h->lib_slots[ch & 1];
        HIP_TRY(hipEventSynchronize(s.done));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
        h->calib_kernel_ms += ms;
        const int64_t r0 = ch * C, rows = std::min(C, total - r0);
        const char *hs = static_cast<const char *>(s.host);
        if (model) memcpy(mz_out + r0, hs + stagelib::OFF_Y, (size_t)rows * sizeof(double));
        if (mz_library_out) memcpy(mz_library_out + r0, hs + stagelib::OFF_MZL, (size_t)rows * sizeof(float));
        return ADH_OK;
    };
    auto pipeline = [&]() -> int {
        for (int64_t ch = 0; ch < n_chunks; ++ch) {
            if (ch >= 2) {
                const int rc = finish(ch - 2);
                if (rc != ADH_OK) return rc;
            }
            adh_handle::CalibSlot &s = h->lib_slots[ch & 1];
            hipStream_t st = streams[ch & 1];
            const int64_t r0 = ch * C, rows = std::min(C, total - r0);
            char *hs = static_cast<char *>(s.host), *ds = static_cast<char *>(s.dev);
            const int blocks = (int)((rows + ROWS - 1) / ROWS);
            HIP_TRY(hipEventRecord(s.k0, st));
            hipLaunchKernelGGL(build_kernel, dim3(blocks), dim3(256), 0, st, m, model ? 1 : 0, t, ser, r0, rows, lib + r0,
                               reinterpret_cast<float *>(ds + stagelib::OFF_MZL), reinterpret_cast<double *>(ds + stagelib::OFF_Y));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s.k1, st));
            if (model) {
                HIP_TRY(hipMemcpyAsync(hs + stagelib::OFF_Y, ds + stagelib::OFF_Y, (size_t)rows * sizeof(double),
                                       hipMemcpyDeviceToHost, st));
                h->d2h_bytes += (uint64_t)rows * sizeof(double);
            }
            if (mz_library_out) {
                HIP_TRY(hipMemcpyAsync(hs + stagelib::OFF_MZL, ds + stagelib::OFF_MZL, (size_t)rows * sizeof(float),
                                       hipMemcpyDeviceToHost, st));
                h->d2h_bytes += (uint64_t)rows * sizeof(float);
            }
            HIP_TRY(hipEventRecord(s.done, st));
        }
        for (int64_t ch = std::max<int64_t>(n_chunks - 2, 0); ch < n_chunks; ++ch) {
            const int rc = finish(ch);
            if (rc != ADH_OK) return rc;
        }
        return ADH_OK;
    };
    const int rc = pipeline();
    if (rc != ADH_OK) {  // nothing of this call may still use the slots or the inputs when they go
        (void)hipStreamSynchronize(streams[0]);
        (void)hipStreamSynchronize(streams[1]);
        (void)hipGetLastError();
        return rc;
    }
    // the mirror: the same sums in the same order on the host team, the float32 of the predictions that came back
    if (h->h_lib.size() != (size_t)total) {  // (not grown in place: that would copy the records that go away)
        std::vector<LibRec>().swap(h->h_lib);
        h->h_lib.resize((size_t)total);
    }
    LibRec *mirror = h->h_lib.data();
    const double *pred = model ? mz_out : nullptr;
    const uint32_t *st0 = start.data();
    calib::team_rows(n, [=, &ser](int64_t lo, int64_t hi) {
        double Bh[MAX_L];
        for (int64_t p = lo; p < hi; ++p) {
            const int L = (int)(c->seq_offset[p + 1] - c->seq_offset[p]);
            const uint8_t *res = c->residues + c->seq_offset[p];
            for (int j = 0; j < L; ++j) Bh[j] = c->aa_mass[res[j]];
            for (int64_t k = c->mod_offset[p]; k < c->mod_offset[p + 1]; ++k) {
                const int j = site_residue(c->mod_site[k], L);
                if (j >= 0) Bh[j] = Bh[j] + c->mod_mass[k];
            }
            for (int i = 1; i < L; ++i) Bh[i] = Bh[i - 1] + Bh[i];
            int64_t r = (int64_t)st0[p];
            for (int i = 0; i < L - 1; ++i)
                for (int s = 0; s < S; ++s, ++r) {
                    const int from = ser.from_nterm[s];
                    const float xl = row_mz_library(Bh[i], Bh[L - 1], from, ser.charge[s], c->mass_proton, c->mass_h2o);
                    uint32_t w[8];
                    stagelib::record_words(xl, pred ? calib::staged_f32(pred[r]) : xl, 1.0f, ser.type[s], 0, ser.charge[s],
                                           from ? (uint32_t)i + 1 : (uint32_t)(L - 1 - i), (uint32_t)i, 0, w);
                    memcpy(&mirror[r], w, sizeof(LibRec));
                }
        }
    });
    for (int64_t p = 0; p < n; ++p) {
        flat_frag_start_idx[p] = start[(size_t)p];
        flat_frag_stop_idx[p] = start[(size_t)p + 1];
    }
    h->d_lib = lib;
    h->n_lib = total;
    h->lib_staged = true;
    note_staged(h, (uint64_t)total * 32);
    return ADH_OK;
}
