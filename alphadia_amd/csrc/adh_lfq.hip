// adh_lfq.hip - label-free quantification (directLFQ) on the resident fragment matrices of an adh_quant object.
//
// The procedure is the one alphadia_amd/lfq.py states (host_direct_lfq): float64 over
// x = log2(v) of the float32 intensities, v <= 0 and NaN missing.
//
//   prepare   the kept rows of one matrix ordered by (group, row) with one stable radix sort, the group offsets as a
//             CSR, the float64 log2 traces row-major (n_rows x n_runs) and every row's valid count
//   sample    one shift per run: the runs are traces as long as the row count.  The pair matrices and the merge
//             loop's control run on the host over R x R doubles; every median / variance of differences is a device
//             pass (differences as sortable keys, one radix sort, block partial sums in a fixed order that the host
//             adds in order), every merge one pass over the anchor's merged trace
//   groups    the hot path: one kernel instance per group does the whole per-group procedure - summed intensity,
//             the quadratic subset, pair matrices, merge loop, linear remainder, per-run medians, scale.
//             Groups of up to 16 ions get one wavefront (four per block), larger ones a workgroup of four; the
//             traces and the two matrices live in LDS where they fit and in a global slab per block where not.
//
// Every quantity is computed by one lane or by one wavefront in a fixed order (rank counting for the medians, a
// butterfly for the sums), so the routes give the same bits and two calls give the same bits.  A workgroup's
// wavefronts share work by index; no kernel waits for another workgroup.
// Included by adh_api.hip behind adh_quant.hip (uses the session helpers and the adh_quant object's matrices).

#include "../../include/alphadia_hip_lfq.h"

struct adlfq_state {
    using Bytes = sess::DevArray<unsigned char, sess::eighth_slack>;
    Bytes work, tmp, slab, small;
    sess::DevArray<double, sess::eighth_slack> X, out;
    sess::DevArray<int32_t, sess::eighth_slack> cnt;
    sess::DevArray<uint32_t, sess::eighth_slack> ord, off;
    sess::DevArray<uint64_t, sess::eighth_slack> keys;
    sess::DevArray<double> part;
    std::vector<int32_t> groups;  // the last result: kept group codes and their rows of n_runs doubles
    std::vector<double> table;
    sess::EventPair ev;
    double prepare_ms = 0.0, sample_ms = 0.0, group_ms = 0.0;
};

namespace lfq {

using sess::grid_for;
using sess::kBlock;
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;
constexpr int kWave = 64;
constexpr int kWaveIons = 16;               // groups of up to this many ions run on one wavefront
constexpr size_t kWaveBudget = 24 * 1024;   // LDS bytes of one wavefront's group (four per block)
constexpr size_t kBlockBudget = 144 * 1024; // LDS bytes of a workgroup's group
constexpr int kScratchBlocks = 128;         // workgroups (and slabs) of the scratch route
constexpr int kParts = 256;                 // blocks of a sample-normalisation reduction

__host__ __device__ inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7FF0000000000000ll); }

// ---- prepare -------------------------------------------------------------------------------------------------------

// sort key of every matrix row: its group code, or kNoGroup for a row that is masked out, has no group or no value
__global__ void __launch_bounds__(kBlock) key_kernel(const float *__restrict__ m, int64_t n_keys, int n_runs,
                                                     const uint8_t *__restrict__ keep, const int32_t *__restrict__ group,
                                                     int32_t n_groups, uint32_t *__restrict__ key, uint32_t *__restrict__ row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride) {
        const int32_t g = group[i];
        bool ok = g >= 0 && g < n_groups && (!keep || keep[i]);
        if (ok) {
            bool any = false;
            for (int r = 0; r < n_runs && !any; ++r) any = m[(size_t)r * (size_t)n_keys + (size_t)i] > 0.0f;
            ok = any;
        }
        key[i] = ok ? (uint32_t)g : kNoGroup;
        row[i] = (uint32_t)i;
    }
}

// off[g] = first sorted position of group g, off[n_groups] = the kept rows (a CSR; empty groups included)
__global__ void __launch_bounds__(kBlock) offsets_kernel(const uint32_t *__restrict__ key, int64_t n, uint32_t n_groups,
                                                         uint32_t *__restrict__ off) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint32_t k = min(key[p], n_groups);
        const uint32_t lo = p == 0 ? 0u : min(key[p - 1], n_groups) + 1u;
        for (uint32_t g = lo; g <= k; ++g) off[g] = (uint32_t)p;
        if (p == n - 1)
            for (uint32_t g = k + 1; g <= n_groups; ++g) off[g] = (uint32_t)n;
    }
}

// the log2 traces of the kept rows, row-major, and their valid counts
__global__ void __launch_bounds__(kBlock) trace_kernel(const float *__restrict__ m, int64_t n_keys, int n_runs,
                                                       const uint32_t *__restrict__ row, int64_t n_rows,
                                                       double *__restrict__ X, int32_t *__restrict__ cnt) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_rows; p += stride) {
        const size_t i = row[p];
        int32_t c = 0;
        for (int r = 0; r < n_runs; ++r) {
            const float v = m[(size_t)r * (size_t)n_keys + i];
            const bool ok = v > 0.0f;
            X[(size_t)p * (size_t)n_runs + (size_t)r] = ok ? log2((double)v) : nan64();
            c += ok;
        }
        cnt[p] = c;
    }
}

// ---- sample normalisation: device passes over traces as long as the row count --------------------------------------

__device__ __forceinline__ uint64_t sortable(double d) {
    const uint64_t u = (uint64_t)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double unsortable(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// a block's sum in a fixed order: thread partials, then a tree over LDS
__device__ __forceinline__ double block_sum(double v, double *s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// key[k] = a[k] - b[k] as a sortable key (all ones where either is missing); part[blk] = valid count of the block's
// positions, part[kParts + blk] = their sum
__global__ void __launch_bounds__(kBlock) diff_kernel(const double *__restrict__ a, int64_t sa, const double *__restrict__ b,
                                                      int64_t sb, int64_t L, uint64_t *__restrict__ key,
                                                      double *__restrict__ part) {
    __shared__ double s[kBlock];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double c = 0.0, sum = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += stride) {
        const double d = a[(size_t)k * (size_t)sa] - b[(size_t)k * (size_t)sb];
        const bool ok = d == d;
        key[k] = ok ? sortable(d) : ~0ull;
        if (ok) c += 1.0, sum += d;
    }
    c = block_sum(c, s);
    sum = block_sum(sum, s);
    if (threadIdx.x == 0) part[blockIdx.x] = c, part[kParts + blockIdx.x] = sum;
}

// part[blk] = the block's sum of squared deviations of the differences from `mean`
__global__ void __launch_bounds__(kBlock) dev_kernel(const uint64_t *__restrict__ key, int64_t L, double mean,
                                                     double *__restrict__ part) {
    __shared__ double s[kBlock];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double sq = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += stride) {
        const uint64_t u = key[k];
        if (u != ~0ull) {
            const double e = unsortable(u) - mean;
            sq += e * e;
        }
    }
    sq = block_sum(sq, s);
    if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

__global__ void __launch_bounds__(kBlock) column_kernel(const double *__restrict__ X, int n_runs, int run, int64_t L,
                                                        double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += stride)
        out[k] = X[(size_t)k * (size_t)n_runs + (size_t)run];
}

// merged[k] takes the original trace t (stride st) shifted by sh, weighted by the counts
__global__ void __launch_bounds__(kBlock) merge_kernel(double *__restrict__ merged, const double *__restrict__ t, int64_t st,
                                                       double sh, double ca, double cs, int64_t L) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += stride) {
        const double m = merged[k], x = t[(size_t)k * (size_t)st] + sh;
        if (m != m) merged[k] = x;
        else if (x == x) merged[k] = (m * ca + x * cs) / (ca + cs);
    }
}

// valid values per run: one block per run
__global__ void __launch_bounds__(kBlock) run_count_kernel(const double *__restrict__ X, int n_runs, int64_t L,
                                                           double *__restrict__ count) {
    __shared__ double s[kBlock];
    double c = 0.0;
    for (int64_t k = threadIdx.x; k < L; k += kBlock) {
        const double x = X[(size_t)k * (size_t)n_runs + blockIdx.x];
        c += x == x;
    }
    c = block_sum(c, s);  // (whole numbers below 2^53: exact in any order)
    if (threadIdx.x == 0) count[blockIdx.x] = c;
}

// ref[k] = the median over the q normalised traces X[k][sel[j]] + tot[j] that are valid at position k
__global__ void __launch_bounds__(kBlock) ref_kernel(const double *__restrict__ X, int n_runs, int64_t L,
                                                     const int32_t *__restrict__ sel, const double *__restrict__ tot, int q,
                                                     double *__restrict__ ref) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += stride) {
        const double *x = X + (size_t)k * (size_t)n_runs;
        int c = 0;
        for (int j = 0; j < q; ++j) c += x[sel[j]] == x[sel[j]];
        double m1 = 0.0, m2 = 0.0;
        for (int j = 0; j < q && c > 0; ++j) {
            const double v = x[sel[j]] + tot[j];
            if (v != v) continue;
            int rank = 0;
            for (int i = 0; i < q; ++i) {
                const double w = x[sel[i]] + tot[i];
                rank += (w < v) || (w == v && i < j);
            }
            if (rank == (c - 1) / 2) m1 = v;
            if (rank == c / 2) m2 = v;
        }
        ref[k] = c > 0 ? (m1 + m2) / 2 : nan64();
    }
}

__global__ void __launch_bounds__(kBlock) shift_kernel(double *__restrict__ X, int n_runs, int64_t total,
                                                       const double *__restrict__ shift) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) X[e] += shift[e % n_runs];
}

// ---- the group kernel ----------------------------------------------------------------------------------------------

struct GroupArgs {
    double *X;                 // log2 traces of the kept rows, row-major
    const int32_t *cnt;        // valid count of every kept row
    const uint32_t *off;       // group offsets
    uint32_t *ord;             // per kept row: the group's trace order (fullest first) on the linear path
    const int32_t *list;       // the groups of this launch
    int32_t n_list, n_runs, q, min_nonan;
    double *out;               // n_groups x n_runs
    uint8_t *keep;             // n_groups
    unsigned char *slab;       // scratch route: one slab of slab_bytes per block
    size_t slab_bytes;         // wave route: the LDS bytes of one wavefront's slice
};

// what one team (W wavefronts) needs for a group of mq quadratic traces over R runs
struct TeamMem {
    double *merged, *dist, *var, *dbuf, *ref, *mid, *shift, *tot, *bc_d;
    int32_t *cntr, *anchor, *counts, *bc_i;
    __host__ __device__ static size_t bytes(size_t mq, size_t R, size_t W) {
        return align16(8 * (mq * R + 2 * mq * mq + W * R + 3 * R + 2 * mq + 2) + 4 * (R + 2 * mq + 4));
    }
    __device__ TeamMem(unsigned char *mem, size_t mq, size_t R, size_t W) {
        double *d = reinterpret_cast<double *>(mem);
        merged = d, d += mq * R;
        dist = d, d += mq * mq;
        var = d, d += mq * mq;
        dbuf = d, d += W * R;
        ref = d, d += R;
        mid = d, d += 2 * R;
        shift = d, d += mq;
        tot = d, d += mq;
        bc_d = d, d += 2;
        int32_t *i = reinterpret_cast<int32_t *>(d);
        cntr = i, i += R;
        anchor = i, i += mq;
        counts = i, i += mq;
        bc_i = i;
    }
};

// a wavefront's lanes see each other's LDS and global writes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int W>
__device__ __forceinline__ void team_sync() {
    if constexpr (W == 1) wave_sync();
    else __syncthreads();
}

// butterfly sums: every lane gets the same bits
__device__ __forceinline__ double wave_sum(double v) {
    for (int w = kWave / 2; w > 0; w >>= 1) v += __shfl_xor(v, w, kWave);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int w = kWave / 2; w > 0; w >>= 1) v += __shfl_xor(v, w, kWave);
    return v;
}

// One wavefront: median (mean of the two middle values of an even count, by rank counting) and population variance
// of a - b over the positions where both are valid; +inf in both without one.  dbuf: R doubles of this wavefront.
__device__ void pair_stats(const double *a, const double *b, int R, double *dbuf, int lane, double &med, double &var) {
    int c = 0;
    double sum = 0.0;
    for (int r = lane; r < R; r += kWave) {
        const double d = a[r] - b[r];
        dbuf[r] = d;
        if (d == d) ++c, sum += d;
    }
    c = wave_sum(c);
    sum = wave_sum(sum);
    wave_sync();
    if (c == 0) {
        med = var = inf64();
        return;
    }
    const double mean = sum / (double)c;
    const int k1 = (c - 1) / 2, k2 = c / 2;
    double sq = 0.0, m1 = 0.0, m2 = 0.0;
    for (int r = lane; r < R; r += kWave) {
        const double d = dbuf[r];
        if (d != d) continue;
        const double e = d - mean;
        sq += e * e;
        int rank = 0;
        for (int s = 0; s < R; ++s) {
            const double o = dbuf[s];
            rank += (o < d) || (o == d && s < r);
        }
        if (rank == k1) m1 = d;
        if (rank == k2) m2 = d;
    }
    // (one lane holds each middle value, the others add zeros)
    med = (wave_sum(m1) + wave_sum(m2)) / 2;
    var = wave_sum(sq) / (double)c;
    wave_sync();  // dbuf is free again
}

// normalize(X, q) over the n > 1 traces of one group, in place
template <int W>
__device__ void normalize_group(const GroupArgs &A, double *Xg, uint32_t row0, int n, const TeamMem &M, int tid) {
    constexpr int T = kWave * W;
    const int wave = tid / kWave, lane = tid % kWave, R = A.n_runs;
    const int mq = min(n, A.q);
    const bool linear = n > A.q;
    uint32_t *ord = A.ord + row0;
    if (linear) {  // traces by valid count, fullest first, stable
        for (int i = tid; i < n; i += T) {
            const int32_t ci = A.cnt[row0 + i];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const int32_t cj = A.cnt[row0 + j];
                rank += (cj > ci) || (cj == ci && j < i);
            }
            ord[rank] = (uint32_t)i;
        }
        team_sync<W>();
    }
    auto sel = [&](int k) -> size_t { return linear ? (size_t)ord[k] : (size_t)k; };
    for (int e = tid; e < mq * R; e += T) M.merged[e] = Xg[sel(e / R) * (size_t)R + (size_t)(e % R)];
    for (int e = tid; e < mq * mq; e += T) M.dist[e] = M.var[e] = inf64();
    for (int k = tid; k < mq; k += T) M.shift[k] = 0.0, M.anchor[k] = -1, M.counts[k] = 1;
    team_sync<W>();
    double *dbuf = M.dbuf + (size_t)wave * (size_t)R;
    for (int e = wave; e < mq * mq; e += W) {
        const int i = e / mq, j = e % mq;
        if (i >= j) continue;
        double med, var;
        pair_stats(M.merged + (size_t)i * R, M.merged + (size_t)j * R, R, dbuf, lane, med, var);
        if (lane == 0) M.dist[e] = med, M.var[e] = var;
    }
    team_sync<W>();
    for (int step = 0; step + 1 < mq; ++step) {
        if (wave == 0) {  // the first minimum of var in row-major order
            double bv = inf64();
            int bi = 0x7FFFFFFF;
            for (int e = lane; e < mq * mq; e += kWave)
                if (bi == 0x7FFFFFFF || M.var[e] < bv) bv = M.var[e], bi = e;
            for (int w = kWave / 2; w > 0; w >>= 1) {
                const double ov = __shfl_xor(bv, w, kWave);
                const int oi = __shfl_xor(bi, w, kWave);
                if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
            }
            if (lane == 0) M.bc_i[0] = bi;
        }
        team_sync<W>();
        const int best = M.bc_i[0], i = best / mq, j = best % mq;
        const double dij = M.dist[best];
        if (dij == inf64()) break;  // (the same for every thread of the team)
        const int ci = M.counts[i], cj = M.counts[j];
        const bool by_i = ci >= cj;
        const int a = by_i ? i : j, s = by_i ? j : i, ca = by_i ? ci : cj, cs = by_i ? cj : ci;
        const double sh = by_i ? dij : -dij;
        team_sync<W>();
        const double *ts = Xg + sel(s) * (size_t)R;  // the original trace
        for (int r = tid; r < R; r += T) {
            const double m = M.merged[(size_t)a * R + r], x = ts[r] + sh;
            if (m != m) M.merged[(size_t)a * R + r] = x;
            else if (x == x) M.merged[(size_t)a * R + r] = (m * (double)ca + x * (double)cs) / ((double)ca + (double)cs);
        }
        if (tid == 0) M.anchor[s] = a, M.shift[s] = sh, M.counts[a] = ca + 1;
        team_sync<W>();
        for (int k = wave; k < mq; k += W) {
            if (k == a || k == s) continue;
            const int lo = min(a, k), hi = max(a, k), e = lo * mq + hi;
            if (M.dist[e] == inf64()) continue;
            double med, var;
            pair_stats(M.merged + (size_t)lo * R, M.merged + (size_t)hi * R, R, dbuf, lane, med, var);
            if (lane == 0) M.dist[e] = med, M.var[e] = var;
        }
        team_sync<W>();
        for (int k = tid; k < mq; k += T)
            M.dist[s * mq + k] = M.dist[k * mq + s] = M.var[s * mq + k] = M.var[k * mq + s] = inf64();
        team_sync<W>();
    }
    team_sync<W>();
    for (int k = tid; k < mq; k += T) {  // own shift plus the anchors' along the chain
        double t = M.shift[k];
        for (int a = M.anchor[k]; a >= 0; a = M.anchor[a]) t += M.shift[a];
        M.tot[k] = t;
    }
    team_sync<W>();
    for (int e = tid; e < mq * R; e += T) {
        const size_t at = sel(e / R) * (size_t)R + (size_t)(e % R);
        const double v = Xg[at] + M.tot[e / R];
        Xg[at] = v;
        M.merged[e] = v;  // the normalised traces, for the linear path's reference
    }
    team_sync<W>();
    if (!linear) return;
    for (int r = tid; r < R; r += T) {  // the median trace of the normalised ones
        int c = 0;
        for (int k = 0; k < mq; ++k) c += M.merged[(size_t)k * R + r] == M.merged[(size_t)k * R + r];
        double m1 = 0.0, m2 = 0.0;
        for (int k = 0; k < mq && c > 0; ++k) {
            const double v = M.merged[(size_t)k * R + r];
            if (v != v) continue;
            int rank = 0;
            for (int o = 0; o < mq; ++o) {
                const double w = M.merged[(size_t)o * R + r];
                rank += (w < v) || (w == v && o < k);
            }
            if (rank == (c - 1) / 2) m1 = v;
            if (rank == c / 2) m2 = v;
        }
        M.ref[r] = c > 0 ? (m1 + m2) / 2 : nan64();
    }
    team_sync<W>();
    for (int t = A.q + wave; t < n; t += W) {  // every other trace onto it
        double *trace = Xg + (size_t)ord[t] * (size_t)R;
        double med, var;
        pair_stats(M.ref, trace, R, dbuf, lane, med, var);
        if (med != inf64())
            for (int r = lane; r < R; r += kWave) trace[r] += med;
    }
    team_sync<W>();
}

// one group on a team of W wavefronts; mem: the team's LDS or slab
template <int W>
__device__ void group_body(const GroupArgs &A, int g, unsigned char *mem, int tid) {
    constexpr int T = kWave * W;
    const int wave = tid / kWave, lane = tid % kWave, R = A.n_runs;
    const uint32_t row0 = A.off[g];
    const int n = (int)(A.off[g + 1] - row0);
    if (n <= 0) return;
    double *Xg = A.X + (size_t)row0 * (size_t)R;
    const TeamMem M(mem, (size_t)min(n, A.q), (size_t)R, (size_t)W);
    const int64_t cells = (int64_t)n * R;
    if (wave == 0) {  // the group's summed intensity
        double s = 0.0;
        for (int64_t e = lane; e < cells; e += kWave) {
            const double x = Xg[e];
            if (x == x) s += exp2(x);
        }
        s = wave_sum(s);
        if (lane == 0) M.bc_d[0] = s;
    }
    team_sync<W>();
    if (n > 1) normalize_group<W>(A, Xg, row0, n, M, tid);
    const int need = max(A.min_nonan, 1);
    for (int r = tid; r < R; r += T) {
        int c = 0;
        for (int i = 0; i < n; ++i) c += Xg[(size_t)i * R + r] == Xg[(size_t)i * R + r];
        M.cntr[r] = c;
        M.mid[2 * r] = M.mid[2 * r + 1] = 0.0;
    }
    team_sync<W>();
    for (int64_t e = tid; e < cells; e += T) {  // per-run medians by rank counting: one cell each
        const int i = (int)(e / R), r = (int)(e % R);
        const double x = Xg[e];
        const int c = M.cntr[r];
        if (x != x || c < need) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double y = Xg[(size_t)j * R + r];
            rank += (y < x) || (y == x && j < i);
        }
        if (rank == (c - 1) / 2) M.mid[2 * r] = x;
        if (rank == c / 2) M.mid[2 * r + 1] = x;
    }
    team_sync<W>();
    if (tid == 0) {
        double s = 0.0;
        bool any = false;
        for (int r = 0; r < R; ++r)
            if (M.cntr[r] >= need) s += exp2((M.mid[2 * r] + M.mid[2 * r + 1]) / 2), any = true;
        M.bc_d[1] = any ? log2(M.bc_d[0] / s) : 0.0;
        A.keep[g] = (uint8_t)any;
    }
    team_sync<W>();
    const double lg = M.bc_d[1];
    for (int r = tid; r < R; r += T)
        A.out[(size_t)g * R + r] = M.cntr[r] >= need ? exp2((M.mid[2 * r] + M.mid[2 * r + 1]) / 2 + lg) : 0.0;
    team_sync<W>();
}

extern __shared__ __align__(16) unsigned char adlfq_lds[];

// groups of up to kWaveIons ions: one wavefront each, four per block
__global__ void __launch_bounds__(4 * kWave) adlfq_wave_kernel(GroupArgs A) {
    const int wave = threadIdx.x / kWave;
    const int64_t it = (int64_t)blockIdx.x * 4 + wave;
    if (it >= A.n_list) return;
    group_body<1>(A, A.list[it], adlfq_lds + (size_t)wave * A.slab_bytes, threadIdx.x % kWave);
}

// larger groups: one workgroup each, the team's memory in LDS or in the block's slab
template <bool kScratch>
__global__ void __launch_bounds__(4 * kWave) adlfq_block_kernel(GroupArgs A) {
    unsigned char *mem = kScratch ? A.slab + (size_t)blockIdx.x * A.slab_bytes : adlfq_lds;
    for (int it = blockIdx.x; it < A.n_list; it += gridDim.x) {
        group_body<4>(A, A.list[it], mem, threadIdx.x);
        __syncthreads();
    }
}

// ---- host: sample normalisation ------------------------------------------------------------------------------------

struct Trace {
    const double *p;
    int64_t stride;
};

struct SampleNorm {
    adlfq_state *s;
    hipStream_t st;
    double *X;
    int64_t L;
    int R;
    sess::DevBufs bufs;
    uint64_t *sorted = nullptr;
    std::vector<double> part = std::vector<double>(2 * kParts);

    // median and variance of a - b over the common valid positions (+inf without one)
    int pair(Trace a, Trace b, double &med, double &var) {
        hipLaunchKernelGGL(diff_kernel, dim3(kParts), dim3(kBlock), 0, st, a.p, a.stride, b.p, b.stride, L, s->keys.p,
                           s->part.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(part.data(), s->part.p, 2 * kParts * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        double c = 0.0, sum = 0.0;
        for (int b2 = 0; b2 < kParts; ++b2) c += part[b2], sum += part[kParts + b2];
        if (c == 0.0) {
            med = var = INFINITY;
            return ADH_OK;
        }
        const double mean = sum / c;
        hipLaunchKernelGGL(dev_kernel, dim3(kParts), dim3(kBlock), 0, st, s->keys.p, L, mean, s->part.p);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_keys(s->tmp, s->keys.p, sorted, L, 64, st));
        const int64_t n = (int64_t)c;
        uint64_t mid[2];
        HIP_TRY(hipMemcpyAsync(part.data(), s->part.p, kParts * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&mid[0], sorted + (n - 1) / 2, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&mid[1], sorted + n / 2, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        double sq = 0.0;
        for (int b2 = 0; b2 < kParts; ++b2) sq += part[b2];
        med = (unsortable(mid[0]) + unsortable(mid[1])) / 2;
        var = sq / c;
        return ADH_OK;
    }

    // normfacts over the runs `runs` as traces: one total shift each
    int normfacts(const std::vector<int> &runs, std::vector<double> &total) {
        const int m = (int)runs.size();
        const double inf = INFINITY;
        std::vector<double> dist((size_t)m * m, inf), var((size_t)m * m, inf), shift(m, 0.0);
        std::vector<int> counts(m, 1), anchor(m, -1);
        std::vector<double *> merged(m, nullptr);  // contiguous, once a trace has been an anchor
        auto orig = [&](int i) { return Trace{X + runs[i], (int64_t)R}; };
        auto cur = [&](int i) { return merged[i] ? Trace{merged[i], 1} : orig(i); };
        for (int i = 0; i < m; ++i)
            for (int j = i + 1; j < m; ++j) ADH_TRY(pair(orig(i), orig(j), dist[(size_t)i * m + j], var[(size_t)i * m + j]));
        for (int step = 0; step + 1 < m; ++step) {
            size_t best = 0;
            for (size_t e = 1; e < (size_t)m * m; ++e)
                if (var[e] < var[best]) best = e;
            const int i = (int)(best / m), j = (int)(best % m);
            if (dist[best] == inf) break;
            const bool by_i = counts[i] >= counts[j];
            const int a = by_i ? i : j, sft = by_i ? j : i;
            const double sh = by_i ? dist[best] : -dist[best];
            anchor[sft] = a, shift[sft] = sh;
            if (!merged[a]) {
                HIP_TRY(bufs.alloc(&merged[a], (size_t)L));
                hipLaunchKernelGGL(column_kernel, dim3(grid_for(L)), dim3(kBlock), 0, st, X, R, runs[a], L, merged[a]);
                HIP_TRY(hipGetLastError());
            }
            const Trace t = orig(sft);
            hipLaunchKernelGGL(merge_kernel, dim3(grid_for(L)), dim3(kBlock), 0, st, merged[a], t.p, t.stride, sh,
                               (double)counts[a], (double)counts[sft], L);
            HIP_TRY(hipGetLastError());
            for (int k = 0; k < m; ++k) {
                const int lo = std::min(a, k), hi = std::max(a, k);
                const size_t e = (size_t)lo * m + hi;
                if (k == a || k == sft || dist[e] == inf) continue;
                ADH_TRY(pair(cur(lo), cur(hi), dist[e], var[e]));
            }
            for (int k = 0; k < m; ++k) {
                dist[(size_t)sft * m + k] = dist[(size_t)k * m + sft] = inf;
                var[(size_t)sft * m + k] = var[(size_t)k * m + sft] = inf;
            }
            counts[a] += 1;
        }
        total.assign(m, 0.0);
        for (int k = 0; k < m; ++k) {
            double t = shift[k];
            for (int a = anchor[k]; a >= 0; a = anchor[a]) t += shift[a];
            total[k] = t;
        }
        return ADH_OK;
    }

    // normalize(T, q) with the runs as traces: shift[r] per run, added to X
    int run(int q) {
        HIP_TRY(s->keys.reserve((size_t)L));
        HIP_TRY(s->part.reserve(2 * kParts));
        HIP_TRY(bufs.alloc(&sorted, (size_t)L));
        std::vector<double> shift(R, 0.0);
        if (R <= q) {
            std::vector<int> runs(R);
            for (int r = 0; r < R; ++r) runs[r] = r;
            ADH_TRY(normfacts(runs, shift));
        } else {
            double *d_count = nullptr, *d_tot = nullptr, *d_ref = nullptr;
            int32_t *d_sel = nullptr;
            HIP_TRY(bufs.alloc(&d_count, (size_t)R));
            hipLaunchKernelGGL(run_count_kernel, dim3(R), dim3(kBlock), 0, st, X, R, L, d_count);
            HIP_TRY(hipGetLastError());
            std::vector<double> count(R);
            HIP_TRY(hipMemcpyAsync(count.data(), d_count, (size_t)R * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            std::vector<int> order(R);
            for (int r = 0; r < R; ++r) order[r] = r;
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return count[x] > count[y]; });
            std::vector<int> runs(order.begin(), order.begin() + q);
            std::vector<double> tot;
            ADH_TRY(normfacts(runs, tot));
            for (int k = 0; k < q; ++k) shift[runs[k]] = tot[k];
            HIP_TRY(bufs.upload(&d_sel, runs.data(), (size_t)q, st));
            HIP_TRY(bufs.upload(&d_tot, tot.data(), (size_t)q, st));
            HIP_TRY(bufs.alloc(&d_ref, (size_t)L));
            hipLaunchKernelGGL(ref_kernel, dim3(grid_for(L)), dim3(kBlock), 0, st, X, R, L, d_sel, d_tot, q, d_ref);
            HIP_TRY(hipGetLastError());
            for (int k = q; k < R; ++k) {
                double med, var;
                ADH_TRY(pair(Trace{d_ref, 1}, Trace{X + order[k], (int64_t)R}, med, var));
                if (med != INFINITY) shift[order[k]] = med;  // (no overlap: the run stays where it is)
            }
        }
        double *d_shift = nullptr;
        HIP_TRY(bufs.upload(&d_shift, shift.data(), (size_t)R, st));
        hipLaunchKernelGGL(shift_kernel, dim3(grid_for(L * R)), dim3(kBlock), 0, st, X, R, L * (int64_t)R, d_shift);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));  // (shift and the buffers leave with this object)
        return ADH_OK;
    }
};

inline adlfq_state *state_of(adh_quant *q) {
    if (!q->lfq) q->lfq = std::make_shared<adlfq_state>();
    return static_cast<adlfq_state *>(q->lfq.get());
}

}  // namespace lfq

extern "C" {

int adlfq_run(adh_quant_t *q, int32_t column, const uint8_t *keep, const int32_t *group, int32_t n_groups,
              int32_t min_nonan, int32_t num_samples_quadratic, int32_t normalize, int64_t *n_kept) {
    if (!q || !n_kept || (q->n_keys > 0 && !group)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!q->built || q->duplicate) return fail(ADH_ERR_NOT_STAGED, "adlfq_run: no built matrices");
    if (column < 0 || column >= q->n_cols) return fail(ADH_ERR_INVALID_ARGUMENT, "adlfq_run: column out of range");
    if (n_groups < 0 || num_samples_quadratic < 2 || num_samples_quadratic > 4096)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adlfq_run: n_groups >= 0 and 2 .. 4096 quadratic samples expected");
    const int64_t n = q->n_keys;
    const int R = q->n_runs;
    if (n >= (int64_t)0x7FFFFFF0ll || R < 1 || R > (1 << 16))
        return fail(ADH_ERR_UNSUPPORTED, "adlfq_run: up to 2^31 rows and 2^16 runs");
    using namespace lfq;
    adlfq_state *s = state_of(q);
    s->groups.clear();
    s->table.clear();
    s->prepare_ms = s->sample_ms = s->group_ms = 0.0;
    *n_kept = 0;
    if (n == 0 || n_groups == 0) return ADH_OK;
    HIP_TRY(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    const int Q = num_samples_quadratic;

    // ---- prepare: work = group [n] i32 | keep [n] u8 | key in / out [n] u32 | row in / out [n] u32
    const size_t o_keep = align16((size_t)n * 4), o_kin = o_keep + align16((size_t)n), o_kout = o_kin + align16((size_t)n * 4),
                 o_rin = o_kout + align16((size_t)n * 4), o_rout = o_rin + align16((size_t)n * 4),
                 wb = o_rout + align16((size_t)n * 4);
    HIP_TRY(s->work.reserve(wb));
    HIP_TRY(s->off.reserve((size_t)n_groups + 1));
    unsigned char *w = s->work.p;
    int32_t *d_group = reinterpret_cast<int32_t *>(w);
    uint8_t *d_keep = keep ? w + o_keep : nullptr;
    uint32_t *kin = reinterpret_cast<uint32_t *>(w + o_kin), *kout = reinterpret_cast<uint32_t *>(w + o_kout);
    uint32_t *rin = reinterpret_cast<uint32_t *>(w + o_rin), *rout = reinterpret_cast<uint32_t *>(w + o_rout);
    sess::TmpSize sort;
    ADH_TRY(sess::sort_pairs(sort, kin, kout, rin, rout, n, 32, st));
    HIP_TRY(s->tmp.reserve(sort.bytes));
    HIP_TRY(hipMemcpyAsync(d_group, group, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (keep) HIP_TRY(hipMemcpyAsync(d_keep, keep, (size_t)n, hipMemcpyHostToDevice, st));
    const float *m = q->mat.p + (size_t)column * (size_t)n * (size_t)R;
    std::vector<uint32_t> off((size_t)n_groups + 1);
    int rc = sess::timed(s->ev, st, s->prepare_ms, [&]() -> int {
        hipLaunchKernelGGL(key_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, m, n, R, d_keep, d_group, n_groups, kin, rin);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_pairs(s->tmp, kin, kout, rin, rout, n, 32, st));  // stable: (group, row)
        hipLaunchKernelGGL(offsets_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, kout, n, (uint32_t)n_groups, s->off.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(off.data(), s->off.p, off.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int64_t L = off[n_groups];
        if (L == 0) return ADH_OK;
        HIP_TRY(s->X.reserve((size_t)L * (size_t)R));
        HIP_TRY(s->cnt.reserve((size_t)L));
        HIP_TRY(s->ord.reserve((size_t)L));
        hipLaunchKernelGGL(trace_kernel, dim3(grid_for(L)), dim3(kBlock), 0, st, m, n, R, rout, L, s->X.p, s->cnt.p);
        HIP_TRY(hipGetLastError());
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    const int64_t L = off[n_groups];
    if (L == 0) return ADH_OK;

    // ---- sample normalisation
    if (normalize) {
        SampleNorm sn{s, st, s->X.p, L, R};
        rc = sess::timed(s->ev, st, s->sample_ms, [&]() -> int { return sn.run(Q); });
        if (rc != ADH_OK) return rc;
    }

    // ---- the groups by route
    const char *route = getenv("ADH_DEBUG_LFQ_ROUTE");  // developer switch: "scratch" sends every group to the slab route
    const bool force_scratch = route && std::string(route) == "scratch";
    std::vector<int32_t> list[3];  // wavefront | workgroup in LDS | workgroup in a slab
    size_t mq_max[3] = {0, 0, 0};
    for (int32_t g = 0; g < n_groups; ++g) {
        const size_t ng = off[g + 1] - off[g], mq = std::min<size_t>(ng, (size_t)Q);
        if (ng == 0) continue;
        int to = 2;
        if (!force_scratch) {
            if (ng <= (size_t)kWaveIons && TeamMem::bytes(mq, R, 1) <= kWaveBudget) to = 0;
            else if (TeamMem::bytes(mq, R, 4) <= kBlockBudget) to = 1;
        }
        list[to].push_back(g);
        mq_max[to] = std::max(mq_max[to], mq);
    }
    const size_t n_list = list[0].size() + list[1].size() + list[2].size();
    HIP_TRY(s->small.reserve(align16(n_list * 4) + align16((size_t)n_groups)));
    int32_t *d_list = reinterpret_cast<int32_t *>(s->small.p);
    uint8_t *d_flag = s->small.p + align16(n_list * 4);
    HIP_TRY(s->out.reserve((size_t)n_groups * (size_t)R));
    {
        size_t at = 0;
        for (auto &l : list) {
            if (!l.empty()) HIP_TRY(hipMemcpyAsync(d_list + at, l.data(), l.size() * 4, hipMemcpyHostToDevice, st));
            at += l.size();
        }
    }
    HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)n_groups, st));
    static bool lds_set = false;
    if (!lds_set) {
        (void)hipFuncSetAttribute((const void *)adlfq_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void *)adlfq_block_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        lds_set = true;
    }
    GroupArgs A{};
    A.X = s->X.p, A.cnt = s->cnt.p, A.off = s->off.p, A.ord = s->ord.p;
    A.n_runs = R, A.q = Q, A.min_nonan = min_nonan;
    A.out = s->out.p, A.keep = d_flag;
    const int n_scratch = (int)std::min<size_t>(list[2].size(), kScratchBlocks);
    const size_t slab_bytes = TeamMem::bytes(mq_max[2], R, 4);
    if (n_scratch > 0) HIP_TRY(s->slab.reserve(slab_bytes * (size_t)n_scratch));
    rc = sess::timed(s->ev, st, s->group_ms, [&]() -> int {
        if (!list[0].empty()) {
            GroupArgs a = A;
            a.list = d_list, a.n_list = (int32_t)list[0].size();
            a.slab_bytes = TeamMem::bytes(mq_max[0], R, 1);
            hipLaunchKernelGGL(adlfq_wave_kernel, dim3((unsigned)((list[0].size() + 3) / 4)), dim3(4 * kWave),
                               4 * a.slab_bytes, st, a);
            HIP_TRY(hipGetLastError());
        }
        if (!list[1].empty()) {
            GroupArgs a = A;
            a.list = d_list + list[0].size(), a.n_list = (int32_t)list[1].size();
            hipLaunchKernelGGL(adlfq_block_kernel<false>, dim3((unsigned)list[1].size()), dim3(4 * kWave),
                               TeamMem::bytes(mq_max[1], R, 4), st, a);
            HIP_TRY(hipGetLastError());
        }
        if (n_scratch > 0) {
            GroupArgs a = A;
            a.list = d_list + list[0].size() + list[1].size(), a.n_list = (int32_t)list[2].size();
            a.slab = s->slab.p, a.slab_bytes = slab_bytes;
            hipLaunchKernelGGL(adlfq_block_kernel<true>, dim3((unsigned)n_scratch), dim3(4 * kWave), 0, st, a);
            HIP_TRY(hipGetLastError());
        }
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;

    // ---- the result: the kept groups' rows
    std::vector<uint8_t> flag((size_t)n_groups);
    std::vector<double> full((size_t)n_groups * (size_t)R);
    HIP_TRY(hipMemcpyAsync(flag.data(), d_flag, flag.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(full.data(), s->out.p, full.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    q->h->d2h_bytes += flag.size() + full.size() * 8 + off.size() * 4;
    for (int32_t g = 0; g < n_groups; ++g) {
        if (!flag[g]) continue;
        s->groups.push_back(g);
        s->table.insert(s->table.end(), full.begin() + (size_t)g * R, full.begin() + (size_t)(g + 1) * R);
    }
    *n_kept = (int64_t)s->groups.size();
    return ADH_OK;
}

int adlfq_result(adh_quant_t *q, int32_t *group, double *table) {
    if (!q) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    adlfq_state *s = lfq::state_of(q);
    if (!s->groups.empty() && (!group || !table)) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    std::copy(s->groups.begin(), s->groups.end(), group);
    std::copy(s->table.begin(), s->table.end(), table);
    return ADH_OK;
}

int adlfq_time_ms(adh_quant_t *q, double *prepare_ms, double *sample_ms, double *group_ms) {
    if (!q || !prepare_ms || !sample_ms || !group_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    adlfq_state *s = lfq::state_of(q);
    *prepare_ms = s->prepare_ms;
    *sample_ms = s->sample_ms;
    *group_ms = s->group_ms;
    return ADH_OK;
}

}  // extern "C"
