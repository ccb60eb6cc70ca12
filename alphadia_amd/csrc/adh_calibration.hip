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

template <typename X>
__global__ void __launch_bounds__(256) predict_kernel(Model m, const X *__restrict__ x, int64_t n,
                                                      double *__restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const X xv = x[i];
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
        y[i] = acc;
    }
}

}  // namespace calib

int adh_calibration_predict(adh_handle_t *h, const adh_loess_model_t *model, const void *x, int32_t x_is_f64,
                            int64_t n, double *y) {
    if (!h || !model || n < 0 || (n > 0 && (!x || !y))) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument or negative n");
    const int K = model->n_kernels, D = model->degree;
    if (K < 1 || K > ADH_LOESS_MAX_KERNELS)
        return fail(ADH_ERR_UNSUPPORTED, "n_kernels must be in 1.." + std::to_string(ADH_LOESS_MAX_KERNELS));
    if (D < 0 || D > ADH_LOESS_MAX_DEGREE)
        return fail(ADH_ERR_UNSUPPORTED, "degree must be in 0.." + std::to_string(ADH_LOESS_MAX_DEGREE));
    h->calib_kernel_ms = 0.0;
    if (n == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(h->device));
    calib::Model m{};
    m.n_kernels = K;
    m.degree = D;
    for (int k = 0; k < K; ++k) {
        m.scale_mean[k] = model->scale_mean[k];
        m.scale_max[k] = model->scale_max[k];
    }
    for (int i = 0; i < (D + 1) * K; ++i) m.beta[i] = model->beta[i];
    const size_t xb = x_is_f64 ? sizeof(double) : sizeof(float);
    // two slots, each: page-locked [chunk inputs | chunk outputs], the same on the device, its stream and events
    constexpr int64_t C = ADH_CALIBRATION_CHUNK_ROWS;
    constexpr size_t slot_bytes = (size_t)C * 2 * sizeof(double);
    hipStream_t streams[2] = {h->stream, h->stream_out};
    for (adh_handle::CalibSlot &s : h->calib) {
        if (!s.host) HIP_TRY(hipHostMalloc(&s.host, slot_bytes, hipHostMallocDefault));
        if (!s.dev) HIP_TRY(hipMalloc(&s.dev, slot_bytes));
        if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        if (!s.k0) HIP_TRY(hipEventCreate(&s.k0));
        if (!s.k1) HIP_TRY(hipEventCreate(&s.k1));
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

int adh_calibration_time_ms(adh_handle_t *h, double *kernel_ms) {
    if (!h || !kernel_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *kernel_ms = h->calib_kernel_ms;
    return ADH_OK;
}
