// adh_flatten.hip - the dense library flattened on the device (include/alphadia_hip_flatten.h): fragment cardinality
// across an elution group, intensity threshold and top-k per precursor, compaction into the flat fragment table with
// renumbered flat_frag_start_idx / flat_frag_stop_idx, and - when asked - the LibRec records left staged on the
// handle as adh_stage_fragments_columns would have staged the returned columns.
//
// The rules are those of alphadia_amd/flatten.py: host_flatten_library (this repository's restatement of alphabase's
// calc_fragment_cardinality + SpecLibFlat.parse_base_library), bit for bit.
//
//   upload    the two matrices through the handle's page-locked lanes (upload_staged), the precursor columns as they are
//   order     one stable radix sort by (decoy, elution group) -> group segments; one by (start, row count) -> block
//             order, on which neighbours are checked for overlap
//   card      per group: a wavefront (up to card_wave_max members) or a workgroup; lanes stride over the block's
//             cells, the loop over the other members is the inner one (their blocks come from L2); uint8 per cell
//   select    per block: a wavefront (up to ADFL_SELECT_WAVE_MAX_CELLS cells) or a workgroup; the order keys of the
//             block's intensities in LDS, rank of a cell = cells with a larger (key, flat index); a keep byte per cell
//             and the kept count per block
//   scan      exclusive sum of the counts in block order
//   emit      a wavefront per block compacts the kept cells in flat order, ballot / popcount prefix per 64 cells,
//             into the eight columns and, when staging, the records (stagelib::record_words, two 16-byte stores)
//
// Every number comes out of integer counting and copies, so the routes agree bit for bit.
// Included by adh_api.hip behind adh_stage_lib.hip and adh_session.h.

#include "../../include/alphadia_hip_flatten.h"

namespace flat {

constexpr int kWave = 64, kBlock = 256, kWaves = kBlock / kWave;
constexpr int kMaxCells = ADFL_MAX_ROWS * ADFL_MAX_COLUMNS;
static_assert(ADFL_CARD_WAVE_MAX_MEMBERS <= ADFL_CARD_WAVE_DEBUG_MEMBERS && ADFL_CARD_WAVE_DEBUG_MEMBERS <= kWave,
              "a wavefront's slice of the member table holds kWave entries");
static_assert(ADFL_MAX_GROUP <= kBlock, "the workgroup's member table holds kBlock entries");
static_assert(ADFL_SELECT_WAVE_MAX_CELLS <= kMaxCells, "the wavefront's tile is the smaller one");

// a wavefront's lanes see each other's LDS writes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The unit of work is a wavefront (WAVE) or the workgroup: its index, how many there are, the lane in it, its lanes.
template <bool WAVE>
struct Team {
    static constexpr int lanes = WAVE ? kWave : kBlock;
    __device__ static int64_t index() { return WAVE ? (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave : (int64_t)blockIdx.x; }
    __device__ static int64_t count() { return WAVE ? (int64_t)gridDim.x * kWaves : (int64_t)gridDim.x; }
    __device__ static int lane() { return WAVE ? (int)(threadIdx.x % kWave) : (int)threadIdx.x; }
    __device__ static int wave() { return WAVE ? (int)(threadIdx.x / kWave) : 0; }
    __device__ static void sync() {
        if constexpr (WAVE) wave_sync();
        else __syncthreads();
    }
};

// float32 intensity -> uint32 whose order is the ranking's: NaN below every number, -0 with +0
__host__ __device__ inline uint32_t order_key(float x) {
    if (x != x) return 0u;
    if (x == 0.0f) x = 0.0f;
    const uint32_t u = stagelib::bits_of(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the two sort keys of every precursor: (start, row count) and (decoy, elution group)
__global__ void __launch_bounds__(kBlock) keys_kernel(const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                      const int64_t *__restrict__ eg, const uint8_t *__restrict__ decoy,
                                                      int64_t n, uint64_t *__restrict__ block_key,
                                                      uint64_t *__restrict__ group_key, uint32_t *__restrict__ iota) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        block_key[i] = (uint64_t)start[i] << 8 | (uint64_t)(stop[i] - start[i]);
        group_key[i] = (uint64_t)eg[i] | (uint64_t)(decoy ? decoy[i] : 0) << 56;
        iota[i] = (uint32_t)i;
    }
}

// head[j]: position j of the group order opens a group
__global__ void __launch_bounds__(kBlock) heads_kernel(const uint64_t *__restrict__ key, int64_t n, uint8_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
        head[j] = j == 0 || key[j] != key[j - 1];
}

// err[0]: the first position of the block order whose block starts before its predecessor's ends
__global__ void __launch_bounds__(kBlock) overlap_kernel(const uint32_t *__restrict__ ord, const int64_t *__restrict__ start,
                                                         const int64_t *__restrict__ stop, int64_t n, uint32_t *__restrict__ err) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; j < n; j += stride)
        if (start[ord[j]] < stop[ord[j - 1]]) atomicMin(&err[0], (uint32_t)j);
}

// Cardinalities of the groups this route takes (members <= wave_max: the wavefronts, else the workgroups).
// gorder: the precursors in group order, gstart[*n_groups]: where every group begins in it.  err[1]: the first
// position of the group order of a group with more than ADFL_MAX_GROUP members (nothing of it is written).
template <bool WAVE>
__global__ void __launch_bounds__(kBlock) card_kernel(const uint32_t *__restrict__ gorder, const uint32_t *__restrict__ gstart,
                                                      const uint32_t *__restrict__ n_groups, int64_t n_prec,
                                                      const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                      const float *__restrict__ mz, int32_t C, int32_t wave_max,
                                                      uint8_t *__restrict__ card, uint32_t *__restrict__ err,
                                                      unsigned long long *__restrict__ stats) {
    using T = Team<WAVE>;
    __shared__ int64_t s_base[kBlock];  // first cell of every member's block
    int64_t *base = s_base + T::wave() * kWave;
    const int lane = T::lane();
    const int64_t ng = *n_groups;
    unsigned long long done = 0;
    for (int64_t g = T::index(); g < ng; g += T::count()) {
        const int64_t a = gstart[g], b = g + 1 < ng ? (int64_t)gstart[g + 1] : n_prec;
        const int64_t m = b - a;
        if (m > ADFL_MAX_GROUP) {
            if (!WAVE && lane == 0) atomicMin(&err[1], (uint32_t)a);
            continue;
        }
        if ((m <= wave_max) != WAVE) continue;
        ++done;
        T::sync();  // (the last group's readers are through with the table)
        bool uniform = true;
        const int64_t rows0 = stop[gorder[a]] - start[gorder[a]];
        for (int64_t t = lane; t < m; t += T::lanes) {
            const uint32_t p = gorder[a + t];
            base[t] = start[p] * C;
        }
        for (int64_t t = 1; t < m; ++t) {  // (every lane the same loop: the verdict is the team's without a vote)
            const uint32_t p = gorder[a + t];
            uniform = uniform && stop[p] - start[p] == rows0;
        }
        T::sync();
        if (!uniform || m == 1) {
            for (int64_t t = 0; t < m; ++t) {
                const uint32_t p = gorder[a + t];
                const int64_t first = start[p] * C, cells = (stop[p] - start[p]) * C;
                for (int64_t c = lane; c < cells; c += T::lanes) card[first + c] = 1;
            }
            continue;
        }
        const int64_t cells = rows0 * C;
        for (int64_t t = 0; t < m; ++t) {
            const int64_t first = base[t];
            for (int64_t c = lane; c < cells; c += T::lanes) {
                const float x = mz[first + c];
                uint32_t count = 1;
                for (int64_t u = 0; u < m; ++u) {
                    if (u == t) continue;
                    const float d = fabsf(mz[base[u] + c] - x);  // (float32 difference, compared as float64; NaN: false)
                    count += (double)d < 0.00001 ? 1u : 0u;
                }
                card[first + c] = (uint8_t)count;
            }
        }
    }
    if (lane == 0 && done) atomicAdd(&stats[WAVE ? 0 : 1], done);
}

// Keep bytes and kept counts of the blocks this route takes (cells <= wave_max: the wavefronts, else the workgroups),
// over the positions of the block order.  tile: the order keys of the block's intensities.
template <bool WAVE>
__global__ void __launch_bounds__(kBlock) select_kernel(const uint32_t *__restrict__ ord, int64_t n_prec,
                                                        const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                        const float *__restrict__ intensity, int32_t C, int32_t wave_max,
                                                        int32_t top_k, float min_intensity, uint8_t *__restrict__ keep,
                                                        uint64_t *__restrict__ kept, unsigned long long *__restrict__ stats) {
    using T = Team<WAVE>;
    constexpr int kTile = WAVE ? ADFL_SELECT_WAVE_MAX_CELLS : kMaxCells;
    __shared__ uint32_t s_tile[WAVE ? kWaves * kTile : kTile];
    __shared__ uint32_t s_sum[kWaves];
    uint32_t *tile = s_tile + T::wave() * kTile;
    const int lane = T::lane();
    unsigned long long done = 0;
    for (int64_t j = T::index(); j < n_prec; j += T::count()) {
        const uint32_t p = ord[j];
        const int64_t first = start[p] * C;
        const int N = (int)((stop[p] - start[p]) * C);  // (<= kMaxCells: the caller checked rows and columns)
        if ((N <= wave_max) != WAVE) continue;
        ++done;
        T::sync();  // (the last block's readers are through with the tile)
        for (int c = lane; c < N; c += T::lanes) tile[c] = order_key(intensity[first + c]);
        T::sync();
        uint32_t mine = 0;
        for (int c = lane; c < N; c += T::lanes) {
            const uint32_t o = tile[c];
            int rank = 0;
#pragma unroll 4
            for (int l = 0; l < N; ++l) {
                const uint32_t q = tile[l];
                rank += (q > o || (q == o && l > c)) ? 1 : 0;
            }
            const bool k = rank < top_k && intensity[first + c] > min_intensity;
            keep[first + c] = k ? 1 : 0;
            mine += k ? 1u : 0u;
        }
        for (int w = kWave / 2; w > 0; w >>= 1) mine += __shfl_xor(mine, w, kWave);
        if constexpr (WAVE) {
            if (lane == 0) kept[j] = mine;
        } else {
            if (threadIdx.x % kWave == 0) s_sum[threadIdx.x / kWave] = mine;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t all = 0;
                for (int w = 0; w < kWaves; ++w) all += s_sum[w];
                kept[j] = all;
            }
        }
    }
    if (lane == 0 && done) atomicAdd(&stats[WAVE ? 2 : 3], done);
}

// One wavefront per position of the block order: its kept cells, in flat order, become rows offset[j] ... of the
// eight columns (the six byte columns n_flat apart) and, when records is given, of the staged library.
// codes[4 x C]: type, loss_type, charge, counts-from-the-N-terminus of every column.
__global__ void __launch_bounds__(kBlock) emit_kernel(const uint32_t *__restrict__ ord, int64_t n_prec,
                                                      const int64_t *__restrict__ start, const int64_t *__restrict__ stop,
                                                      const float *__restrict__ mz, const float *__restrict__ intensity,
                                                      const uint8_t *__restrict__ card, const uint8_t *__restrict__ keep,
                                                      const uint64_t *__restrict__ offset, const uint64_t *__restrict__ kept,
                                                      const uint8_t *__restrict__ codes, int32_t C, int64_t n_flat,
                                                      uint32_t *__restrict__ flat_start, uint32_t *__restrict__ flat_stop,
                                                      float *__restrict__ out_mz, float *__restrict__ out_intensity,
                                                      uint8_t *__restrict__ out_bytes, LibRec *__restrict__ records) {
    using T = Team<true>;
    const int lane = T::lane();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t j = T::index(); j < n_prec; j += T::count()) {
        const uint32_t p = ord[j];
        const int64_t first = start[p] * C;
        const int rows = (int)(stop[p] - start[p]), N = rows * C;
        const uint64_t row0 = offset[j];
        if (lane == 0) {
            flat_start[p] = (uint32_t)row0;
            flat_stop[p] = (uint32_t)(row0 + kept[j]);
        }
        uint64_t run = 0;
        for (int c0 = 0; c0 < N; c0 += kWave) {
            const int c = c0 + lane;
            const bool k = c < N && keep[first + c] != 0;
            const unsigned long long mask = __ballot(k);
            if (k) {
                const uint64_t o = row0 + run + (uint64_t)__popcll(mask & below);  // (< n_flat: the scan of the same bytes)
                const int i = c / C, col = c % C;
                const float x = mz[first + c], v = intensity[first + c];
                const uint32_t type = codes[col], loss = codes[C + col], charge = codes[2 * C + col];
                const uint32_t number = codes[3 * C + col] ? (uint32_t)i + 1u : (uint32_t)(rows - i);
                const uint32_t cd = card[first + c];
                out_mz[o] = x;
                out_intensity[o] = v;
                out_bytes[o] = (uint8_t)type;
                out_bytes[n_flat + o] = (uint8_t)loss;
                out_bytes[2 * n_flat + o] = (uint8_t)charge;
                out_bytes[3 * n_flat + o] = (uint8_t)number;
                out_bytes[4 * n_flat + o] = (uint8_t)i;
                out_bytes[5 * n_flat + o] = (uint8_t)cd;
                if (records) {
                    uint32_t w[8];
                    stagelib::record_words(x, x, v, type, loss, charge, number, (uint32_t)i, cd, w);
                    uint4 *r = reinterpret_cast<uint4 *>(records + o);  // (LibRec is 16-byte aligned)
                    r[0] = make_uint4(w[0], w[1], w[2], w[3]);
                    r[1] = make_uint4(w[4], w[5], w[6], w[7]);
                }
            }
            run += (uint64_t)__popcll(mask);
        }
    }
}

inline unsigned wave_grid(int64_t units) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + kWaves - 1) / kWaves, 8192));
}
inline unsigned block_grid(int64_t units) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(units, 2048)); }

inline int bits_for(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

}  // namespace flat

extern "C" {

int adfl_flatten(adh_handle_t *h, int64_t n_prec, const int64_t *frag_start, const int64_t *frag_stop,
                 const int64_t *elution_group, const uint8_t *decoy, int64_t n_rows, int32_t n_cols, const float *mz,
                 const float *intensity, const uint8_t *column_codes, int32_t top_k, float min_intensity, int32_t stage,
                 int64_t capacity, uint32_t *flat_start, uint32_t *flat_stop, float *out_mz, float *out_intensity,
                 uint8_t *out_bytes, int64_t *n_flat, int64_t *routes, double *kernel_ms, uint64_t *link_bytes) {
    using namespace flat;
    if (!h || !n_flat || !routes || !kernel_ms || !link_bytes) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_prec < 0 || n_rows < 0 || capacity < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "negative count");
    if (n_prec >= (int64_t)0x7FFFFFFFll) return fail(ADH_ERR_UNSUPPORTED, "too many precursors");
    if (n_cols < 1 || n_cols > ADFL_MAX_COLUMNS)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: " + std::to_string(n_cols) + " columns (1 .. " +
                                                  std::to_string(ADFL_MAX_COLUMNS) + " are supported)");
    if (n_rows >= ((int64_t)1 << 40)) return fail(ADH_ERR_UNSUPPORTED, "too many dense rows");
    if (top_k < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: top_k must be at least 1");
    if (!column_codes || (n_prec > 0 && (!frag_start || !frag_stop || !elution_group || !flat_start || !flat_stop)) ||
        (n_rows > 0 && (!mz || !intensity)) || (capacity > 0 && (!out_mz || !out_intensity || !out_bytes)))
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL column");
    const int32_t C = n_cols;
    uint64_t eg_max = 0, bound = 0;
    bool any_decoy = false;
    for (int64_t p = 0; p < n_prec; ++p) {
        const int64_t a = frag_start[p], b = frag_stop[p];
        if (a < 0 || b < a || b > n_rows)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: the fragment rows of precursor " + std::to_string(p) +
                                                      " lie outside the library's matrices");
        if (b - a > ADFL_MAX_ROWS)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: precursor " + std::to_string(p) + " has " +
                                                      std::to_string(b - a) + " fragment rows (0 .. " +
                                                      std::to_string(ADFL_MAX_ROWS) + " are supported)");
        if (elution_group[p] < 0 || elution_group[p] >= ((int64_t)1 << 56))
            return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: elution_group_idx of precursor " + std::to_string(p) +
                                                      " is outside [0, 2^56)");
        eg_max = std::max<uint64_t>(eg_max, (uint64_t)elution_group[p]);
        any_decoy = any_decoy || (decoy && decoy[p]);
        bound += (uint64_t)std::min<int64_t>((b - a) * C, top_k);
    }
    routes[0] = routes[1] = routes[2] = routes[3] = 0;
    *kernel_ms = 0.0;
    link_bytes[0] = link_bytes[1] = 0;
    *n_flat = 0;

    int32_t card_wave_max = ADFL_CARD_WAVE_MAX_MEMBERS, select_wave_max = ADFL_SELECT_WAVE_MAX_CELLS;
    if (const char *env = getenv("ADFL_DEBUG_ROUTE")) {  // developer switch: one route for everything it can take
        if (!strcmp(env, "block")) card_wave_max = 0, select_wave_max = -1;
        else if (!strcmp(env, "wave")) card_wave_max = ADFL_CARD_WAVE_DEBUG_MEMBERS;
        else return fail(ADH_ERR_INVALID_ARGUMENT, "ADFL_DEBUG_ROUTE is neither 'wave' nor 'block'");
    }

    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    sess::DevBufs B;
    sess::EventPair ev;
    int64_t total = 0;
    const int64_t n = n_prec;
    int64_t *d_start = nullptr, *d_stop = nullptr;
    uint32_t *ord = nullptr;
    uint64_t *kept = nullptr, *offset = nullptr;
    float *d_mz = nullptr, *d_int = nullptr;
    uint8_t *card = nullptr, *keep = nullptr, *codes = nullptr;
    const size_t cells = (size_t)n_rows * (size_t)C;

    if (n > 0) {
        int64_t *d_eg = nullptr;
        uint8_t *d_decoy = nullptr, *head = nullptr;
        uint64_t *bkey = nullptr, *bkey_s = nullptr, *gkey = nullptr, *gkey_s = nullptr;
        uint32_t *iota = nullptr, *gorder = nullptr, *gstart = nullptr, *n_groups = nullptr, *err = nullptr;
        unsigned long long *stats = nullptr;
        HIP_TRY(B.upload(&d_start, frag_start, (size_t)n, st));
        HIP_TRY(B.upload(&d_stop, frag_stop, (size_t)n, st));
        HIP_TRY(B.upload(&d_eg, elution_group, (size_t)n, st));
        if (decoy) HIP_TRY(B.upload(&d_decoy, decoy, (size_t)n, st));
        HIP_TRY(B.upload(&codes, column_codes, (size_t)4 * C, st));
        link_bytes[0] += (uint64_t)n * (decoy ? 25 : 24) + 4 * (uint64_t)C;
        HIP_TRY(B.alloc(&d_mz, cells));
        HIP_TRY(B.alloc(&d_int, cells));
        if (cells > 0) {
            // the matrices are the bytes of this step: from the caller's pageable arrays through the page-locked lanes
            std::vector<UpJob> jobs{UpJob{d_mz, mz, cells * 4}, UpJob{d_int, intensity, cells * 4}};
            ADH_TRY(upload_staged(h, jobs));
            link_bytes[0] += (uint64_t)cells * 8;
        }
        HIP_TRY(B.alloc(&card, cells));
        HIP_TRY(B.alloc(&keep, cells));
        HIP_TRY(B.alloc(&bkey, (size_t)n));
        HIP_TRY(B.alloc(&bkey_s, (size_t)n));
        HIP_TRY(B.alloc(&gkey, (size_t)n));
        HIP_TRY(B.alloc(&gkey_s, (size_t)n));
        HIP_TRY(B.alloc(&iota, (size_t)n));
        HIP_TRY(B.alloc(&ord, (size_t)n));
        HIP_TRY(B.alloc(&gorder, (size_t)n));
        HIP_TRY(B.alloc(&gstart, (size_t)n));
        HIP_TRY(B.alloc(&head, (size_t)n));
        HIP_TRY(B.alloc(&kept, (size_t)n));
        HIP_TRY(B.alloc(&offset, (size_t)n));
        HIP_TRY(B.alloc(&n_groups, 4));
        HIP_TRY(B.alloc(&err, 4));
        HIP_TRY(B.alloc(&stats, 4));
        HIP_TRY(hipMemsetAsync(err, 0xFF, 16, st));
        HIP_TRY(hipMemsetAsync(stats, 0, 32, st));

        ADH_TRY(ev.begin(st));
        const unsigned grid = sess::grid_for(n);
        hipLaunchKernelGGL(keys_kernel, dim3(grid), dim3(kBlock), 0, st, (const int64_t *)d_start, (const int64_t *)d_stop,
                           (const int64_t *)d_eg, (const uint8_t *)d_decoy, n, bkey, gkey, iota);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_pairs(B, (const uint64_t *)bkey, bkey_s, (const uint32_t *)iota, ord, n,
                                 std::min(64, 8 + bits_for((uint64_t)n_rows)), st));
        ADH_TRY(sess::sort_pairs(B, (const uint64_t *)gkey, gkey_s, (const uint32_t *)iota, gorder, n,
                                 any_decoy ? 64 : bits_for(eg_max), st));
        hipLaunchKernelGGL(heads_kernel, dim3(grid), dim3(kBlock), 0, st, (const uint64_t *)gkey_s, n, head);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::select_flagged(B, (const uint32_t *)iota, (const uint8_t *)head, gstart, n_groups, n, st));
        hipLaunchKernelGGL(overlap_kernel, dim3(grid), dim3(kBlock), 0, st, (const uint32_t *)ord, (const int64_t *)d_start,
                           (const int64_t *)d_stop, n, err);
        HIP_TRY(hipGetLastError());
        // (blocks that overlap still lie inside the matrices: the kernels below write nothing out of bounds, and the
        // call is refused once the flag is on the host)
        hipLaunchKernelGGL(card_kernel<true>, dim3(wave_grid(n)), dim3(kBlock), 0, st, (const uint32_t *)gorder,
                           (const uint32_t *)gstart, (const uint32_t *)n_groups, n, (const int64_t *)d_start,
                           (const int64_t *)d_stop, (const float *)d_mz, C, card_wave_max, card, err, stats);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(card_kernel<false>, dim3(block_grid(n)), dim3(kBlock), 0, st, (const uint32_t *)gorder,
                           (const uint32_t *)gstart, (const uint32_t *)n_groups, n, (const int64_t *)d_start,
                           (const int64_t *)d_stop, (const float *)d_mz, C, card_wave_max, card, err, stats);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(select_kernel<true>, dim3(wave_grid(n)), dim3(kBlock), 0, st, (const uint32_t *)ord, n,
                           (const int64_t *)d_start, (const int64_t *)d_stop, (const float *)d_int, C, select_wave_max, top_k,
                           min_intensity, keep, kept, stats);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(select_kernel<false>, dim3(block_grid(n)), dim3(kBlock), 0, st, (const uint32_t *)ord, n,
                           (const int64_t *)d_start, (const int64_t *)d_stop, (const float *)d_int, C, select_wave_max, top_k,
                           min_intensity, keep, kept, stats);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::exclusive_sum(B, (const uint64_t *)kept, offset, n, st));
        uint32_t h_err[4];
        unsigned long long h_stats[4];
        uint64_t last[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h_err, err, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_stats, stats, 32, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&last[0], offset + (n - 1), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&last[1], kept + (n - 1), 8, hipMemcpyDeviceToHost, st));
        ADH_TRY(ev.end(st, *kernel_ms));
        link_bytes[1] += 64;
        if (h_err[0] != 0xFFFFFFFFu) {
            uint32_t pair[2] = {0, 0};
            HIP_TRY(hipMemcpy(pair, ord + (h_err[0] - 1), 8, hipMemcpyDeviceToHost));
            return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: the fragment rows of precursors " + std::to_string(pair[0]) +
                                                      " and " + std::to_string(pair[1]) + " overlap");
        }
        if (h_err[1] != 0xFFFFFFFFu) {
            uint32_t member = 0;
            HIP_TRY(hipMemcpy(&member, gorder + h_err[1], 4, hipMemcpyDeviceToHost));
            return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: the elution group of precursor " + std::to_string(member) +
                                                      " has more than " + std::to_string(ADFL_MAX_GROUP) +
                                                      " precursors (the cardinality is a uint8)");
        }
        for (int r = 0; r < 4; ++r) routes[r] = (int64_t)h_stats[r];
        if (last[0] + last[1] > bound) return fail(ADH_ERR_HIP, "adfl_flatten: inconsistent number of kept rows");
        if (last[0] + last[1] >= 0xFFFFFFFFull)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: the flat library would have 2^32 rows or more");
        total = (int64_t)(last[0] + last[1]);
    }
    if (total > capacity)
        return fail(ADH_ERR_INVALID_ARGUMENT, "adfl_flatten: " + std::to_string(total) + " kept rows for a capacity of " +
                                                  std::to_string(capacity));

    float *o_mz = nullptr, *o_int = nullptr;
    uint8_t *o_bytes = nullptr;
    uint32_t *o_start = nullptr, *o_stop = nullptr;
    LibRec *lib = nullptr;
    if (stage) {
        // nothing refuses the input from here on: the staged library goes before its successor is allocated, as in
        // adh_stage_fragments_columns (the block it gives up is the one the new records take)
        h->calib_kernel_ms = 0.0;
        ADH_TRY(calib::library_changes(h));
        h->lib_buf.release();
        h->lib_staged = false;
        h->d_lib = nullptr;
        h->n_lib = 0;
        HIP_TRY(hipMalloc(&lib, (size_t)std::max<int64_t>(total, 1) * sizeof(LibRec)));
        h->lib_buf.ptrs.push_back(lib);
    }
    if (n > 0) {
        HIP_TRY(B.alloc(&o_mz, (size_t)total));
        HIP_TRY(B.alloc(&o_int, (size_t)total));
        HIP_TRY(B.alloc(&o_bytes, (size_t)total * 6));
        HIP_TRY(B.alloc(&o_start, (size_t)n));
        HIP_TRY(B.alloc(&o_stop, (size_t)n));
        ADH_TRY(ev.begin(st));
        hipLaunchKernelGGL(emit_kernel, dim3(wave_grid(n)), dim3(kBlock), 0, st, (const uint32_t *)ord, n,
                           (const int64_t *)d_start, (const int64_t *)d_stop, (const float *)d_mz, (const float *)d_int,
                           (const uint8_t *)card, (const uint8_t *)keep, (const uint64_t *)offset, (const uint64_t *)kept,
                           (const uint8_t *)codes, C, total, o_start, o_stop, o_mz, o_int, o_bytes, lib);
        HIP_TRY(hipGetLastError());
        ADH_TRY(ev.end(st, *kernel_ms));
        // back: 14 bytes per kept row, 8 per precursor
        HIP_TRY(hipMemcpy(flat_start, o_start, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(flat_stop, o_stop, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (total > 0) {
            HIP_TRY(hipMemcpy(out_mz, o_mz, (size_t)total * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(out_intensity, o_int, (size_t)total * 4, hipMemcpyDeviceToHost));
            for (int k = 0; k < 6; ++k)
                HIP_TRY(hipMemcpy(out_bytes + (size_t)k * capacity, o_bytes + (size_t)k * total, (size_t)total,
                                  hipMemcpyDeviceToHost));
        }
        const uint64_t back = (uint64_t)n * 8 + (uint64_t)total * 14;
        link_bytes[1] += back;
        h->d2h_bytes += back + 64;
    }
    *n_flat = total;
    if (!stage) return ADH_OK;

    // the mirror: the same records from the columns that came back (a vector that already has the room is not
    // cleared first - every byte of every record is written)
    if (h->h_lib.size() != (size_t)total) {  // (not grown in place: that would copy the records that go away)
        std::vector<LibRec>().swap(h->h_lib);
        h->h_lib.resize((size_t)total);
    }
    LibRec *mirror = h->h_lib.data();
    const size_t cap = (size_t)capacity;
    calib::team_rows(total, [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            uint32_t w[8];
            stagelib::record_words(out_mz[i], out_mz[i], out_intensity[i], out_bytes[i], out_bytes[cap + i],
                                   out_bytes[2 * cap + i], out_bytes[3 * cap + i], out_bytes[4 * cap + i],
                                   out_bytes[5 * cap + i], w);
            memcpy(&mirror[i], w, sizeof(LibRec));
        }
    });
    h->d_lib = lib;
    h->n_lib = total;
    h->lib_staged = true;
    note_staged(h, (uint64_t)total * 32);
    return ADH_OK;
}

}  // extern "C"
