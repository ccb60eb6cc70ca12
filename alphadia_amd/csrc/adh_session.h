// adh_session.h - the host plumbing that the device-session modules share (adh_quant, adh_grouping, adh_protein_fdr,
// adh_transfer_library, adh_mbr_library): the launch grid, owned device allocations, grow-only device arrays, an
// event-pair timer and the two-call pattern of hipCUB.
//
// Included by adh_api.hip behind `fail`, HIP_TRY and the hipMalloc / hipFree macros, so every allocation made here
// goes through adh_dev_malloc / adh_dev_free like the rest of the translation unit (DESIGN.md sections 3 and 8).
#pragma once

// returns a code other than ADH_OK to the caller
#define ADH_TRY(expr)                  \
    do {                               \
        const int _rc = (expr);        \
        if (_rc != ADH_OK) return _rc; \
    } while (0)

namespace sess {

constexpr int kBlock = 256;

inline unsigned grid_for(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 16384));
}

__global__ void __launch_bounds__(kBlock) iota_kernel(uint32_t *__restrict__ v, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) v[i] = (uint32_t)i;
}

// A list of owned device blocks, freed together: a local of one call (an early HIP_TRY return frees them) or the
// member of a session that holds the buffers of its last call.
struct DevBufs {
    std::vector<void *> ptrs;
    DevBufs() = default;
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs() { release(); }
    void release() {
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
        ptrs.clear();
    }
    // at least 4 elements, so that no caller has to think about an empty column
    template <typename T>
    hipError_t alloc(T **p, size_t n) {
        void *v = nullptr;
        hipError_t e = hipMalloc(&v, std::max<size_t>(n, 4) * sizeof(T));
        if (e != hipSuccess) return e;
        ptrs.push_back(v);
        *p = static_cast<T *>(v);
        return hipSuccess;
    }
    // the caller keeps p
    void keep(void *p) {
        for (void *&q : ptrs)
            if (q == p) q = nullptr;
    }
    // a host column of n elements into a block of its own (nothing is copied for n == 0)
    template <typename T>
    hipError_t upload(T **p, const T *host, size_t n, hipStream_t st) {
        hipError_t e = alloc(p, n);
        if (e == hipSuccess && n > 0) e = hipMemcpyAsync(*p, host, n * sizeof(T), hipMemcpyHostToDevice, st);
        return e;
    }
    // the same for a column whose element size is known at run time
    hipError_t upload(unsigned char **p, const void *host, size_t bytes, hipStream_t st) {
        hipError_t e = alloc(p, bytes);
        if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(*p, host, bytes, hipMemcpyHostToDevice, st);
        return e;
    }
};

// what a DevArray asks the allocator for when it has to hold n elements
inline size_t exact_size(size_t n) { return std::max<size_t>(n, 4); }
inline size_t as_asked(size_t n) { return n; }  // (for a caller that never asks for 0)
inline size_t eighth_slack(size_t n) { return n + n / 8 + 256; }

// A grow-only device array that frees itself; growing does not keep the contents.  No synchronisation of its own
// before the old block goes: hipFree waits for the device, and a block that adh_dev_free parks instead keeps that
// wait (hipDeviceSynchronize in adh_dev_free), so kernels still reading the old block finish first.
template <typename T, size_t (*Size)(size_t) = exact_size>
struct DevArray {
    T *p = nullptr;
    size_t cap = 0;  // elements
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    ~DevArray() { release(); }
    operator T *() const { return p; }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t n) {
        if (p && n <= cap) return hipSuccess;
        release();
        void *v = nullptr;
        hipError_t e = hipMalloc(&v, Size(n) * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T *>(v);
        cap = Size(n);
        return hipSuccess;
    }
    // takes over the block q of n elements that B allocated
    void adopt(DevBufs &B, T *q, size_t n) {
        release();
        B.keep(q);
        p = q;
        cap = exact_size(n);
    }
    void swap(DevArray &o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};

// Two events, created at the first use: end() adds the time since begin() to ms and waits for it.  A caller that
// reports its last call zeroes the field first.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int begin(hipStream_t st) {
        if (!e0) HIP_TRY(hipEventCreate(&e0));
        if (!e1) HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        return ADH_OK;
    }
    int end(hipStream_t st, double &ms) {
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        float f = 0.0f;
        HIP_TRY(hipEventElapsedTime(&f, e0, e1));
        ms += f;
        return ADH_OK;
    }
};

// body() between the two events; a failing body leaves ms as it is - which is 0 for a caller that zeroed the field
// to report its last call: after a failed call no time of an earlier call is reported
template <typename F>
int timed(EventPair &ev, hipStream_t st, double &ms, F &&body) {
    ADH_TRY(ev.begin(st));
    ADH_TRY(body());
    return ev.end(st, ms);
}

// ---- hipCUB: ask for the size of the temporary storage, get it, call again ---------------------------------------
// The temporary storage comes from one of four sources:
//   DevBufs   a fresh block of the size asked for, freed with the rest of the list
//   DevArray  one reused grow-only block; the call is told the whole remembered size
//   TmpSize   none: a dry run that records the largest size asked for, to reserve a block outside a timed region
//   BufsTmp  one reused block of a DevBufs: a call that asks for more gets a larger block of the same list, and the
//             smaller one stays there, so nothing is freed (no device wait) while the list lives

struct TmpSize {
    size_t bytes = 0;
};

struct BufsTmp {
    DevBufs &B;
    unsigned char *p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        const hipError_t e = B.alloc(&p, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
};

inline hipError_t cub_tmp(BufsTmp &t, size_t &bytes, void *&tmp) {
    const hipError_t e = t.reserve(bytes);
    tmp = t.p;
    bytes = t.bytes;
    return e;
}

inline hipError_t cub_tmp(DevBufs &B, size_t &bytes, void *&tmp) {
    unsigned char *t = nullptr;
    const hipError_t e = B.alloc(&t, bytes);
    tmp = t;
    return e;
}

template <size_t (*Size)(size_t)>
hipError_t cub_tmp(DevArray<unsigned char, Size> &A, size_t &bytes, void *&tmp) {
    const hipError_t e = A.reserve(bytes);
    tmp = A.p;
    bytes = A.cap;
    return e;
}

inline hipError_t cub_tmp(TmpSize &s, size_t &bytes, void *&tmp) {
    s.bytes = std::max(s.bytes, bytes);
    tmp = nullptr;  // (the second call asks for the size again)
    return hipSuccess;
}

// call: (void *tmp, size_t &bytes) -> hipError_t
template <typename Tmp, typename Call>
int cub_call(Tmp &src, Call &&call) {
    size_t bytes = 0;
    HIP_TRY(call(nullptr, bytes));
    void *tmp = nullptr;
    HIP_TRY(cub_tmp(src, bytes, tmp));
    HIP_TRY(call(tmp, bytes));
    return ADH_OK;
}

// The iterator arguments reach hipCUB in the types the caller passes them in.

// stable, bits [0, end_bit) of the key
template <typename Tmp, typename K, typename V>
int sort_pairs(Tmp &src, const K *k_in, K *k_out, const V *v_in, V *v_out, int64_t n, int end_bit, hipStream_t st) {
    return cub_call(src, [&](void *t, size_t &b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, k_in, k_out, v_in, v_out, (int)n, 0, end_bit, st);
    });
}

template <typename Tmp, typename K>
int sort_keys(Tmp &src, const K *in, K *out, int64_t n, int end_bit, hipStream_t st) {
    return cub_call(src, [&](void *t, size_t &b) {
        return hipcub::DeviceRadixSort::SortKeys(t, b, in, out, (int)n, 0, end_bit, st);
    });
}

template <typename Tmp, typename In, typename Out>
int exclusive_sum(Tmp &src, In in, Out out, int64_t n, hipStream_t st) {
    return cub_call(src, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, (int)n, st); });
}

template <typename Tmp, typename In, typename Out>
int inclusive_sum(Tmp &src, In in, Out out, int64_t n, hipStream_t st) {
    return cub_call(src, [&](void *t, size_t &b) { return hipcub::DeviceScan::InclusiveSum(t, b, in, out, (int)n, st); });
}

template <typename Tmp, typename In, typename Flag, typename Out>
int select_flagged(Tmp &src, In in, Flag flag, Out out, uint32_t *n_sel, int64_t n, hipStream_t st) {
    return cub_call(src, [&](void *t, size_t &b) {
        return hipcub::DeviceSelect::Flagged(t, b, in, flag, out, n_sel, (int)n, st);
    });
}

}  // namespace sess
