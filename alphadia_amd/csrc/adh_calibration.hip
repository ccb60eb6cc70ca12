// adh_calibration.hip - prediction of a fitted LOESS calibration model (LOESSRegression.predict,
// alphadia/calibration/models.py:276-366) over a library column, host -> host.
//
// Per row: w_k = (x - scale_mean[k]) / scale_max[k]; tricubic weights (1 - |w|^3)^3 + 1e-6, 0 where |w| > 1,
// the first kernel left-open (1 for w < 0), the last right-open (1 for w > 0), one kernel = weight 1; weights
// normalised by their sum; y = sum_k w_k * sum_d x^d beta[d][k].  Everything as NumPy evaluates it:
//   - the design row x^d is built in the input's dtype (sklearn's PolynomialFeatures multiplies column by column
//     in the dtype of X), then promoted: a float32 column has x^2 rounded to float32;
//   - the weights are float64 (the fitted scales are float64 arrays, so NumPy promotes the column);
//   - `mask * (...)` is a product, not a select: NaN inputs, and an infinite |w|^3, give NaN as in NumPy; a row
//     whose weights sum to 0 gives NaN.  No guard.
// The build keeps -ffp-contract=off: no mul+add is fused.  The kernel is not the cost of this entry (12 bytes per
// float32 row cross PCIe); it is one grid-stride loop that evaluates every weight twice instead of keeping K of them.
// adh_calibrate_staged_fragments runs the same evaluation over the library that is already staged and rewrites its mz
// field where it lies; adh_stage_lib.hip runs it while it packs a library from its columns.
// Included by adh_api.hip (shares its error helpers and the handle).

namespace calib {

struct Model {
    int32_t n_kernels, degree;
    double scale_mean[ADH_LOESS_MAX_KERNELS];
    double scale_max[ADH_LOESS_MAX_KERNELS];
    double beta[(ADH_LOESS_MAX_DEGREE + 1) * ADH_LOESS_MAX_KERNELS];  // beta[d * n_kernels + k]
};

// _tricubic / _left_open_tricubic / _right_open_tricubic (models.py:345-366)
__device__ __forceinline__ double weight(const Model &m, int k, double x) {
    if (m.n_kernels == 1) return 1.0;
    const double v = (x - m.scale_mean[k]) / m.scale_max[k];
    const double a = fabs(v);
    const double u = 1.0 - a * a * a;
    double t = (a <= 1.0 ? 1.0 : 0.0) * (u * u * u + 1e-6);
    if (k == 0 && v < 0.0) t = 1.0;
    if (k == m.n_kernels - 1 && v > 0.0) t = 1.0;
    return t;
}

// One row of the prediction: every kernel that calibrates (predict_kernel, calibrate_lib_kernel below, the pack kernel
// of adh_stage_lib.hip) evaluates a row here, so a row's value does not depend on the path that produced it.
template <typename X>
__device__ __forceinline__ double predict_row(const Model &m, const X xv) {
    double p[ADH_LOESS_MAX_DEGREE + 1];
    X pw = (X)1;
    p[0] = 1.0;
#pragma unroll
    for (int d = 1; d <= ADH_LOESS_MAX_DEGREE; ++d) {
        pw = d == 1 ? xv : pw * xv;
        p[d] = (double)pw;
    }
    const double xd = (double)xv;
    double wsum = 0.0;
    for (int k = 0; k < m.n_kernels; ++k) wsum += weight(m, k, xd);
    double acc = 0.0;
    for (int k = 0; k < m.n_kernels; ++k) {
        double poly = 0.0;
        for (int d = 0; d <= m.degree; ++d) poly += p[d] * m.beta[d * m.n_kernels + k];
        acc += poly * (weight(m, k, xd) / wsum);
    }
    return acc;
}

template <typename X>
__global__ void __launch_bounds__(256) predict_kernel(Model m, const X *__restrict__ x, int64_t n,
                                                      double *__restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = predict_row<X>(m, x[i]);
}

// The float32 a calibrated m/z is staged as: round to nearest even, what NumPy's astype(float32) makes of the float64
// column on the host.  A NaN keeps its sign and the top 22 bits of its payload and is made quiet (the host's
// conversion instruction), so that the device records, their host mirror and a column converted on the host agree
// bit for bit whatever NaN the evaluation left.
__host__ __device__ inline float staged_f32(double y) {
    if (y != y) {
        uint64_t b;
        memcpy(&b, &y, 8);
        const uint32_t u = (uint32_t)(b >> 63) << 31 | 0x7FC00000u | ((uint32_t)(b >> 29) & 0x003FFFFFu);
        float f;
        memcpy(&f, &u, 4);
        return f;
    }
    return (float)y;
}

// In-place calibration of the staged library: lib[i].mz = float32 of the model over lib[i].mz_library (a float32
// column), nothing else of the record is written; y (may be NULL) takes the float64 predictions.
__global__ void __launch_bounds__(256) calibrate_lib_kernel(Model m, LibRec *__restrict__ lib, int64_t n,
                                                            double *__restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v = predict_row<float>(m, lib[i].mz_library);
        lib[i].mz = staged_f32(v);
        if (y) y[i] = v;
    }
}

}  // namespace calib

namespace calib {

// the limits of adh_loess_model_t, and its parameters as the kernels take them
int load_model(const adh_loess_model_t *model, Model &m) {
    const int K = model->n_kernels, D = model->degree;
    if (K < 1 || K > ADH_LOESS_MAX_KERNELS)
        return fail(ADH_ERR_UNSUPPORTED, "n_kernels must be in 1.." + std::to_string(ADH_LOESS_MAX_KERNELS));
    if (D < 0 || D > ADH_LOESS_MAX_DEGREE)
        return fail(ADH_ERR_UNSUPPORTED, "degree must be in 0.." + std::to_string(ADH_LOESS_MAX_DEGREE));
    m = Model{};
    m.n_kernels = K;
    m.degree = D;
    for (int k = 0; k < K; ++k) {
        m.scale_mean[k] = model->scale_mean[k];
        m.scale_max[k] = model->scale_max[k];
    }
    for (int i = 0; i < (D + 1) * K; ++i) m.beta[i] = model->beta[i];
    return ADH_OK;
}

// a pair of pipeline slots of slot_bytes each: page-locked and device staging, their events (allocated on first use)
int ensure_slots(adh_handle::CalibSlot (&slots)[2], size_t slot_bytes) {
    for (adh_handle::CalibSlot &s : slots) {
        if (!s.host) HIP_TRY(hipHostMalloc(&s.host, slot_bytes, hipHostMallocDefault));
        if (!s.dev) HIP_TRY(hipMalloc(&s.dev, slot_bytes));
        if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        if (!s.k0) HIP_TRY(hipEventCreate(&s.k0));
        if (!s.k1) HIP_TRY(hipEventCreate(&s.k1));
    }
    return ADH_OK;
}

constexpr size_t kSlotBytes = (size_t)ADH_CALIBRATION_CHUNK_ROWS * 2 * sizeof(double);

// fn(lo, hi) over [0, n) on the host team (adh_host_threads)
template <typename F>
void team_rows(int64_t n, F fn) {
    const int T = host_threads_for(n);
    std::vector<std::thread> team;
    int w = 1;
    for (; w < T; ++w) {
        try {
            team.emplace_back(fn, n * w / T, n * (w + 1) / T);
        } catch (const std::system_error &) {
            break;
        }
    }
    fn(0, n / T);
    if (w < T) fn(n * w / T, n);  // (threads that could not be started: their rows run here)
    for (std::thread &t : team) t.join();
}

}  // namespace calib

int adh_calibration_predict(adh_handle_t *h, const adh_loess_model_t *model, const void *x, int32_t x_is_f64,
                            int64_t n, double *y) {
    if (!h || !model || n < 0 || (n > 0 && (!x || !y))) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument or negative n");
    calib::Model m;
    {
        const int rc_m = calib::load_model(model, m);
        if (rc_m != ADH_OK) return rc_m;
    }
    h->calib_kernel_ms = 0.0;
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t xb = x_is_f64 ? sizeof(double) : sizeof(float);
    // two slots, each: page-locked [chunk inputs | chunk outputs], the same on the device, its stream and events
    constexpr int64_t C = ADH_CALIBRATION_CHUNK_ROWS;
    hipStream_t streams[2] = {h->stream, h->stream_out};
    {
        const int rc_s = calib::ensure_slots(h->calib, calib::kSlotBytes);
        if (rc_s != ADH_OK) return rc_s;
    }
    const int64_t n_chunks = (n + C - 1) / C;
    // chunk c runs on slot c & 1: its inputs are copied into the slot's page-locked block on the host while the other
    // slot's copies and kernel run; the outputs of chunk c - 2 leave the slot before its inputs overwrite it
    auto finish = [&](int64_t c) -> int {
        adh_handle::CalibSlot &s = h->calib[c & 1];
        HIP_TRY(hipEventSynchronize(s.done));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
        h->calib_kernel_ms += ms;
        const int64_t r0 = c * C, rows = std::min(C, n - r0);
        memcpy(y + r0, static_cast<const char *>(s.host) + (size_t)C * sizeof(double), (size_t)rows * sizeof(double));
        return ADH_OK;
    };
    auto pipeline = [&]() -> int {
        for (int64_t c = 0; c < n_chunks; ++c) {
            if (c >= 2) {
                const int rc = finish(c - 2);
                if (rc != ADH_OK) return rc;
            }
            adh_handle::CalibSlot &s = h->calib[c & 1];
            hipStream_t st = streams[c & 1];
            const int64_t r0 = c * C, rows = std::min(C, n - r0);
            char *hin = static_cast<char *>(s.host), *din = static_cast<char *>(s.dev);
            double *hout = reinterpret_cast<double *>(hin + (size_t)C * sizeof(double));
            double *dout = reinterpret_cast<double *>(din + (size_t)C * sizeof(double));
            memcpy(hin, static_cast<const char *>(x) + (size_t)r0 * xb, (size_t)rows * xb);
            HIP_TRY(hipMemcpyAsync(din, hin, (size_t)rows * xb, hipMemcpyHostToDevice, st));
            const int blocks = (int)std::min<int64_t>((rows + 255) / 256, 4096);
            HIP_TRY(hipEventRecord(s.k0, st));
            if (x_is_f64)
                hipLaunchKernelGGL(calib::predict_kernel<double>, dim3(blocks), dim3(256), 0, st, m,
                                   reinterpret_cast<const double *>(din), rows, dout);
            else
                hipLaunchKernelGGL(calib::predict_kernel<float>, dim3(blocks), dim3(256), 0, st, m,
                                   reinterpret_cast<const float *>(din), rows, dout);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s.k1, st));
            HIP_TRY(hipMemcpyAsync(hout, dout, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(s.done, st));
            h->d2h_bytes += (uint64_t)rows * sizeof(double);
        }
        for (int64_t c = std::max<int64_t>(n_chunks - 2, 0); c < n_chunks; ++c) {
            const int rc = finish(c);
            if (rc != ADH_OK) return rc;
        }
        return ADH_OK;
    };
    const int rc = pipeline();
    if (rc != ADH_OK) {  // nothing of this call may still read or write the slots when the next one fills them
        (void)hipStreamSynchronize(streams[0]);
        (void)hipStreamSynchronize(streams[1]);
        (void)hipGetLastError();
    }
    return rc;
}

namespace calib {

// What adh_stage_fragments settles because the library changes: the last call's tables are completed from the library
// they were scored with and stop being current (accumulated tables hold every column themselves), the resident
// candidate table and its plan go, nothing in flight reads the records any more.
int library_changes(adh_handle *h) {
    const int rc_m = materialise_tables(h);
    if (rc_m != ADH_OK) return rc_m;
    h->tables_current = h->tables_current && h->acc_live;
    HIP_TRY(hipDeviceSynchronize());
    h->plan = Plan();
    h->cands_uploaded = false;
    h->sel.stage = 0;
    return ADH_OK;
}

}  // namespace calib

int adh_calibrate_staged_fragments(adh_handle_t *h, const adh_loess_model_t *model, double *mz_out) {
    if (!h || !model) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!h->lib_staged || !h->d_lib || h->h_lib.size() != (size_t)h->n_lib)
        return fail(ADH_ERR_NOT_STAGED, "no fragment library staged");
    calib::Model m;
    {
        const int rc_m = calib::load_model(model, m);
        if (rc_m != ADH_OK) return rc_m;
    }
    h->calib_kernel_ms = 0.0;
    HIP_TRY(hipSetDevice(h->device));
    {
        const int rc_l = calib::library_changes(h);
        if (rc_l != ADH_OK) return rc_l;
    }
    const int64_t n = h->n_lib;
    if (n == 0) return ADH_OK;
    // the mirror takes the float32 of the predictions that come back: without mz_out they land in a block of our own
    std::vector<double> own;
    if (!mz_out) {
        own.resize((size_t)n);
        mz_out = own.data();
    }
    constexpr int64_t C = ADH_CALIBRATION_CHUNK_ROWS;
    {
        const int rc_s = calib::ensure_slots(h->calib, calib::kSlotBytes);
        if (rc_s != ADH_OK) return rc_s;
    }
    LibRec *lib = const_cast<LibRec *>(h->d_lib);
    hipStream_t streams[2] = {h->stream, h->stream_out};
    const int64_t n_chunks = (n + C - 1) / C;
    // chunk c on slot c & 1, as in adh_calibration_predict; nothing goes up, the slot only carries the predictions back
    auto finish = [&](int64_t c) -> int {
        adh_handle::CalibSlot &s = h->calib[c & 1];
        HIP_TRY(hipEventSynchronize(s.done));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.k0, s.k1));
        h->calib_kernel_ms += ms;
        const int64_t r0 = c * C, rows = std::min(C, n - r0);
        memcpy(mz_out + r0, s.host, (size_t)rows * sizeof(double));
        return ADH_OK;
    };
    auto pipeline = [&]() -> int {
        for (int64_t c = 0; c < n_chunks; ++c) {
            if (c >= 2) {
                const int rc = finish(c - 2);
                if (rc != ADH_OK) return rc;
            }
            adh_handle::CalibSlot &s = h->calib[c & 1];
            hipStream_t st = streams[c & 1];
            const int64_t r0 = c * C, rows = std::min(C, n - r0);
            const int blocks = (int)std::min<int64_t>((rows + 255) / 256, 4096);
            HIP_TRY(hipEventRecord(s.k0, st));
            hipLaunchKernelGGL(calib::calibrate_lib_kernel, dim3(blocks), dim3(256), 0, st, m, lib + r0, rows,
                               static_cast<double *>(s.dev));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s.k1, st));
            HIP_TRY(hipMemcpyAsync(s.host, s.dev, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(s.done, st));
            h->d2h_bytes += (uint64_t)rows * sizeof(double);
        }
        for (int64_t c = std::max<int64_t>(n_chunks - 2, 0); c < n_chunks; ++c) {
            const int rc = finish(c);
            if (rc != ADH_OK) return rc;
        }
        return ADH_OK;
    };
    const int rc = pipeline();
    if (rc != ADH_OK) {
        (void)hipStreamSynchronize(streams[0]);
        (void)hipStreamSynchronize(streams[1]);
        (void)hipGetLastError();
        h->lib_staged = false;  // (records and mirror may differ now)
        return rc;
    }
    LibRec *mirror = h->h_lib.data();
    calib::team_rows(n, [mirror, mz_out](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) mirror[i].mz = calib::staged_f32(mz_out[i]);
    });
    return ADH_OK;
}

int adh_calibration_time_ms(adh_handle_t *h, double *kernel_ms) {
    if (!h || !kernel_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *kernel_ms = h->calib_kernel_ms;
    return ADH_OK;
}
