// adh_stage_lib.hip - the fragment library staged from its nine columns: adh_stage_fragments_columns uploads the
// columns as columns (14 bytes per row with a model, 18 without) and a kernel packs the 32-byte LibRec records in HBM,
// calibrating the m/z on the way when a model is given (calib::predict_row, the evaluation of adh_calibration_predict);
// adh_staged_fragments_read hands the raw records of the device or of the host mirror to tests and tools.
//
// Chunks of ADH_CALIBRATION_CHUNK_ROWS rows alternate between two slots of the handle, each a page-locked block and a
// device block of the same layout, on two streams:
//   [mz_library f32 | mz f32 | intensity f32 | type, loss_type, charge, number, position, cardinality u8 | y f64]
// every column at a fixed offset (a multiple of the chunk rows).  The host mirror is not copied back: once the
// predictions are on the host (8 bytes per row instead of 32) the host team packs the same records from the same
// columns - the float32 of a prediction is calib::staged_f32 on both sides.
// Included by adh_api.hip after adh_calibration.hip.

namespace stagelib {

constexpr int64_t C = ADH_CALIBRATION_CHUNK_ROWS;
constexpr size_t OFF_MZL = 0, OFF_MZ = (size_t)C * 4, OFF_INT = (size_t)C * 8, OFF_U8 = (size_t)C * 12,
                 OFF_Y = (size_t)C * 18, SLOT_BYTES = (size_t)C * 26;
static_assert(OFF_Y % sizeof(double) == 0, "the predictions of a slot must be 8-byte aligned");

__host__ __device__ inline uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// the two 16-byte halves of a record; every pad byte is zero
__host__ __device__ inline void record_words(float mz_library, float mz, float intensity, uint32_t type, uint32_t loss_type,
                                             uint32_t charge, uint32_t number, uint32_t position, uint32_t cardinality,
                                             uint32_t (&w)[8]) {
    w[0] = bits_of(mz_library);
    w[1] = bits_of(mz);
    w[2] = bits_of(intensity);
    w[3] = type | loss_type << 8 | charge << 16 | number << 24;
    w[4] = position | cardinality << 8;
    w[5] = w[6] = w[7] = 0;
}
static_assert(offsetof(LibRec, type) == 12 && offsetof(LibRec, number) == 15 && offsetof(LibRec, position) == 16 &&
                  offsetof(LibRec, cardinality) == 17,
              "record_words packs the byte fields of LibRec");

// One record per lane, written as two 16-byte stores.  u8: the six byte columns, u8_stride apart.  calibrate: mz is
// the model over mz_library and y takes the float64 prediction; otherwise the mz column is copied.
__global__ void __launch_bounds__(256) pack_kernel(calib::Model m, int calibrate, const float *__restrict__ mz_library,
                                                   const float *__restrict__ mz, const float *__restrict__ intensity,
                                                   const uint8_t *__restrict__ u8, int64_t u8_stride, int64_t n,
                                                   LibRec *__restrict__ out, double *__restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xl = mz_library[i];
        float v;
        if (calibrate) {
            const double p = calib::predict_row<float>(m, xl);
            y[i] = p;
            v = calib::staged_f32(p);
        } else {
            v = mz[i];
        }
        uint32_t w[8];
        record_words(xl, v, intensity[i], u8[i], u8[u8_stride + i], u8[2 * u8_stride + i], u8[3 * u8_stride + i],
                     u8[4 * u8_stride + i], u8[5 * u8_stride + i], w);
        uint4 *o = reinterpret_cast<uint4 *>(out + i);  // (LibRec is 16-byte aligned)
        o[0] = make_uint4(w[0], w[1], w[2], w[3]);
        o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}

}  // namespace stagelib

int adh_stage_fragments_columns(adh_handle_t *h, const adh_fragments_t *f, const adh_loess_model_t *model, double *mz_out) {
    using namespace stagelib;
    if (!h || !f) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (f->n < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "negative fragment count");
    if (f->n >= (int64_t)0xFFFFFFFFll) return fail(ADH_ERR_UNSUPPORTED, "too many fragments");
    const int64_t n = f->n;
    const uint8_t *const bytes_in[6] = {f->type, f->loss_type, f->charge, f->number, f->position, f->cardinality};
    if (n > 0) {
        bool missing = !f->mz_library || !f->intensity || (!model && !f->mz);
        for (const uint8_t *p : bytes_in) missing = missing || !p;
        if (missing) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL fragment column");
    }
    calib::Model m{};
    if (model) {
        const int rc_m = calib::load_model(model, m);
        if (rc_m != ADH_OK) return rc_m;
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
    HIP_TRY(hipMalloc(&lib, (size_t)std::max<int64_t>(n, 1) * sizeof(LibRec)));
    h->lib_buf.ptrs.push_back(lib);
    std::vector<double> own;  // the mirror takes the float32 of the predictions: without mz_out they land here
    if (model && !mz_out && n > 0) {
        own.resize((size_t)n);
        mz_out = own.data();
    }
    if (n > 0) {
        const int rc_s = calib::ensure_slots(h->lib_slots, SLOT_BYTES);
        if (rc_s != ADH_OK) return rc_s;
    }
    hipStream_t streams[2] = {h->stream, h->stream_out};
    const int64_t n_chunks = (n + C - 1) / C;
    auto finish = [&](int64_t c) -> int {
        adh_handle::CalibSlot &s = h->lib_slots[c & 1];
        HIP_TRY(hipEventSynchronize(s.done));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
        h->calib_kernel_ms += ms;
        const int64_t r0 = c * C, rows = std::min(C, n - r0);
        if (model) memcpy(mz_out + r0, static_cast<const char *>(s.host) + OFF_Y, (size_t)rows * sizeof(double));
        return ADH_OK;
    };
    auto pipeline = [&]() -> int {
        for (int64_t c = 0; c < n_chunks; ++c) {
            if (c >= 2) {
                const int rc = finish(c - 2);
                if (rc != ADH_OK) return rc;
            }
            adh_handle::CalibSlot &s = h->lib_slots[c & 1];
            hipStream_t st = streams[c & 1];
            const int64_t r0 = c * C, rows = std::min(C, n - r0);
            char *hs = static_cast<char *>(s.host), *ds = static_cast<char *>(s.dev);
            auto up = [&](size_t off, const void *src, size_t elem) -> hipError_t {
                memcpy(hs + off, static_cast<const char *>(src) + (size_t)r0 * elem, (size_t)rows * elem);
                return hipMemcpyAsync(ds + off, hs + off, (size_t)rows * elem, hipMemcpyHostToDevice, st);
            };
            HIP_TRY(up(OFF_MZL, f->mz_library, 4));
            if (!model) HIP_TRY(up(OFF_MZ, f->mz, 4));
            HIP_TRY(up(OFF_INT, f->intensity, 4));
            for (int j = 0; j < 6; ++j) HIP_TRY(up(OFF_U8 + (size_t)j * C, bytes_in[j], 1));
            const int blocks = (int)std::min<int64_t>((rows + 255) / 256, 4096);
            HIP_TRY(hipEventRecord(s.k0, st));
            hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(256), 0, st, m, model ? 1 : 0,
                               reinterpret_cast<const float *>(ds + OFF_MZL), reinterpret_cast<const float *>(ds + OFF_MZ),
                               reinterpret_cast<const float *>(ds + OFF_INT), reinterpret_cast<const uint8_t *>(ds + OFF_U8),
                               C, rows, lib + r0, reinterpret_cast<double *>(ds + OFF_Y));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s.k1, st));
            if (model) {
                HIP_TRY(hipMemcpyAsync(hs + OFF_Y, ds + OFF_Y, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
                h->d2h_bytes += (uint64_t)rows * sizeof(double);
            }
            HIP_TRY(hipEventRecord(s.done, st));
        }
        for (int64_t c = std::max<int64_t>(n_chunks - 2, 0); c < n_chunks; ++c) {
            const int rc = finish(c);
            if (rc != ADH_OK) return rc;
        }
        return ADH_OK;
    };
    const int rc = pipeline();
    if (rc != ADH_OK) {  // nothing of this call may still use the slots when the next one fills them
        (void)hipStreamSynchronize(streams[0]);
        (void)hipStreamSynchronize(streams[1]);
        (void)hipGetLastError();
        return rc;
    }
    // the mirror: the same records from the same columns (a vector that already has the room is not cleared first -
    // every byte of every record is written)
    if (h->h_lib.size() != (size_t)n) {  // (not grown in place: that would copy the records that go away)
        std::vector<LibRec>().swap(h->h_lib);
        h->h_lib.resize((size_t)n);
    }
    LibRec *mirror = h->h_lib.data();
    const double *pred = model ? mz_out : nullptr;
    calib::team_rows(n, [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            uint32_t w[8];
            record_words(f->mz_library[i], pred ? calib::staged_f32(pred[i]) : f->mz[i], f->intensity[i], bytes_in[0][i],
                         bytes_in[1][i], bytes_in[2][i], bytes_in[3][i], bytes_in[4][i], bytes_in[5][i], w);
            memcpy(&mirror[i], w, sizeof(LibRec));
        }
    });
    h->d_lib = lib;
    h->n_lib = n;
    h->lib_staged = true;
    note_staged(h, (uint64_t)n * 32);
    return ADH_OK;
}

int adh_staged_fragments_read(adh_handle_t *h, int32_t host_mirror, void *records, int64_t n) {
    if (!h || n < 0 || (n > 0 && !records)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument or negative n");
    if (!h->lib_staged || !h->d_lib) return fail(ADH_ERR_NOT_STAGED, "no fragment library staged");
    if (n != h->n_lib) return fail(ADH_ERR_INVALID_ARGUMENT, "n is not the staged library's fragment count");
    if (n == 0) return ADH_OK;
    if (host_mirror) {
        if (h->h_lib.size() != (size_t)n) return fail(ADH_ERR_NOT_STAGED, "no host copy of the staged library");
        memcpy(records, h->h_lib.data(), (size_t)n * sizeof(LibRec));
        return ADH_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(records, h->d_lib, (size_t)n * sizeof(LibRec), hipMemcpyDeviceToHost));
    h->d2h_bytes += (uint64_t)n * sizeof(LibRec);
    return ADH_OK;
}
