// adh_grouping.hip - protein inference on the device: the greedy set cover of perform_grouping
// (outputtransform/grouping.py:8-194), one independent cover per connected component of the id - precursor graph.
//
// The reference keeps one set of precursors per protein id and repeats: take the id with the largest set (the first
// one that appeared on a tie), make it the master of those precursors, remove them from every other set.  Precursors
// with the same id string behave alike, so the host sends distinct id strings ("patterns") weighted by their number of
// precursors, and the bipartite edge list (pattern, id code); id codes count ids in their order of first appearance.
// Strings never reach the device.
//
// adh_pg_solve:  both CSR directions of the edge list (radix sort by (id, pattern) and by (pattern, id), degree
//                counts, exclusive scans); component labels by hooking (atomicMin of the smaller parent onto the
//                larger one's parent) and pointer jumping in repeated launches until a round changes nothing; the ids
//                sorted by (component, id code); then one cover per component: a wavefront for components of up to
//                64 ids, a workgroup for larger ones (set sizes in LDS up to kLdsIds ids, in global memory beyond).
//                Per iteration: argmax over (set size descending, id code ascending), the winner claims its
//                uncovered patterns and the weight of each leaves the set size of the pattern's other ids; the
//                subtraction that brings an id to zero records the master that emptied it.  All of it is integer
//                arithmetic, so the order of the atomics does not matter.
// adh_pg_filter: the heuristic: strings of masters are allowed (in either decoy class), the edges whose id is allowed
//                are sorted once by (pattern, rank) and come back as a CSR of id codes per pattern.
//
// No kernel here waits for another workgroup: kernel boundaries are the only global synchronisation, and the round
// loop of the labelling is bounded (kMaxRounds).  Included by adh_api.hip behind adh_session.h (shares its error
// helpers, the handle and the session helpers).

struct adh_pg {
    adh_handle_t *h = nullptr;
    sess::DevBufs bufs;  // the device buffers of the last solve and of the filters since
    bool solved = false;
    int32_t P = 0, I = 0;
    int64_t E = 0;
    uint64_t *pkey = nullptr;       // the edges as pattern << 32 | id, ascending
    uint32_t *is_master = nullptr;  // [I]
    int32_t n_comp = 0, n_large = 0, rounds = 0;
    sess::EventPair ev;
    double label_ms = 0.0, cover_ms = 0.0, filter_ms = 0.0;
};

namespace pg {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kSmallWaves = kBlock / kWave;  // components per block of the wavefront kernel
constexpr int kCoverBlock = 1024;
constexpr int kLdsIds = 8192;   // set sizes of a larger component live in global memory
constexpr int kJump = 32;       // pointer-jumping steps of one launch
constexpr int kMaxRounds = 256;
using sess::grid_for;

// both sort keys of every edge and the degree of its two ends
__global__ void __launch_bounds__(kBlock) keys_kernel(const int32_t *__restrict__ ep, const int32_t *__restrict__ ei,
                                                      int64_t E, uint64_t *__restrict__ ikey, uint64_t *__restrict__ pkey,
                                                      uint32_t *__restrict__ ideg, uint32_t *__restrict__ pdeg) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        const uint32_t p = (uint32_t)ep[e], i = (uint32_t)ei[e];
        ikey[e] = ((uint64_t)i << 32) | p;
        pkey[e] = ((uint64_t)p << 32) | i;
        atomicAdd(&ideg[i], 1u);
        atomicAdd(&pdeg[p], 1u);
    }
}

// Hooking.  Node i < I is id i, node I + p is pattern p.  A parent is always a node of the same component with an
// index no larger than the node's own, and parents only decrease, so a value read while another workgroup lowers it
// is still a valid ancestor.  The edge's larger parent gets the smaller one as its parent (atomicMin).
__global__ void __launch_bounds__(kBlock) hook_kernel(const int32_t *__restrict__ ep, const int32_t *__restrict__ ei,
                                                      int64_t E, uint32_t I, uint32_t *parent, uint32_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        const uint32_t ru = parent[(uint32_t)ei[e]], rv = parent[I + (uint32_t)ep[e]];
        if (ru != rv) {
            atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
            *flag = 1u;
        }
    }
}

// Pointer jumping: every node moves up to kJump ancestors towards its root (the chain strictly decreases, so the walk
// ends whatever other workgroups write meanwhile); a node still below its root asks for another round.
__global__ void __launch_bounds__(kBlock) jump_kernel(uint32_t *parent, int64_t N, uint32_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += stride) {
        const uint32_t p0 = parent[v];
        uint32_t p = p0;
        bool root = false;
        for (int k = 0; k < kJump; ++k) {
            const uint32_t gp = parent[p];
            if (gp >= p) {  // (gp > p cannot happen)
                root = true;
                break;
            }
            p = gp;
        }
        if (p != p0) parent[v] = p;
        if (!root) *flag = 1u;
    }
}

__global__ void __launch_bounds__(kBlock) comp_key_kernel(const uint32_t *__restrict__ parent, int64_t I,
                                                          uint64_t *__restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += stride)
        key[i] = ((uint64_t)parent[i] << 32) | (uint32_t)i;
}

__global__ void __launch_bounds__(kBlock) comp_head_kernel(const uint64_t *__restrict__ key, int64_t I,
                                                           uint32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < I; k += stride)
        head[k] = (k == 0 || (key[k] >> 32) != (key[k - 1] >> 32)) ? 1u : 0u;
}

// cid: inclusive scan of the heads (1-based component of every sorted position).  Writes the sorted id list, every
// id's sorted position, the first position of every component (comp_off[n_comp] = I) and the id's initial set size.
__global__ void __launch_bounds__(kBlock) comp_fill_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ cid,
                                                           int64_t I, const uint32_t *__restrict__ ioff,
                                                           const uint64_t *__restrict__ ikey,
                                                           const int32_t *__restrict__ weight,
                                                           uint32_t *__restrict__ sorted_id, uint32_t *__restrict__ pos,
                                                           uint32_t *__restrict__ comp_off, int32_t *__restrict__ size) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < I; k += stride) {
        const uint32_t id = (uint32_t)key[k];
        sorted_id[k] = id;
        pos[id] = (uint32_t)k;
        const uint32_t c = cid[k];
        if (k == 0 || cid[k - 1] != c) comp_off[c - 1] = (uint32_t)k;
        if (k == I - 1) comp_off[c] = (uint32_t)I;
        int32_t s = 0;
        for (uint32_t q = ioff[id]; q < ioff[id + 1]; ++q) s += weight[(uint32_t)ikey[q]];
        size[k] = s;
    }
}

__global__ void __launch_bounds__(kBlock) large_kernel(const uint32_t *__restrict__ comp_off, int32_t n_comp,
                                                       uint32_t *__restrict__ list, uint32_t *__restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_comp; c += stride)
        if (comp_off[c + 1] - comp_off[c] > (uint32_t)kWave) list[atomicAdd(count, 1u)] = (uint32_t)c;
}

// the state the threads of one wavefront / workgroup hand to each other goes through workgroup-scope atomics
__device__ __forceinline__ int32_t ld_wg(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_wg(int32_t *p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct Graph {
    const uint32_t *ioff;   // [I + 1] patterns of id i: ikey[ioff[i] .. ioff[i + 1]) (low half)
    const uint64_t *ikey;
    const uint32_t *poff;   // [P + 1] ids of pattern p: pkey[poff[p] .. poff[p + 1]) (low half)
    const uint64_t *pkey;
    const int32_t *weight;  // [P]
    const uint32_t *pos;    // [I] sorted position of an id
    int32_t *master;        // [P] -1: uncovered
    int32_t *emptied;       // [I] the master whose claim emptied the id's set, -1: none
    uint32_t *is_master;    // [I]
};

// Winner m claims pattern edge k of its list: an uncovered pattern gets m as master and its weight leaves the set
// size of every id of the pattern (m's own included, which ends at zero).  size: the component's set sizes, indexed
// by sorted position - off; n: its id count.
__device__ __forceinline__ void claim(const Graph &g, uint32_t k, uint32_t m, int32_t *size, uint32_t off, uint32_t n) {
    const uint32_t p = (uint32_t)g.ikey[k];
    if (ld_wg(g.master + p) >= 0) return;
    st_wg(g.master + p, (int32_t)m);
    const int32_t w = g.weight[p];
    if (w <= 0) return;
    for (uint32_t q = g.poff[p]; q < g.poff[p + 1]; ++q) {
        const uint32_t j = (uint32_t)g.pkey[q];
        const uint32_t lj = g.pos[j] - off;
        if (lj >= n) continue;  // (an id of another component: cannot happen)
        const int32_t old = __hip_atomic_fetch_sub(size + lj, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == w && j != m) g.emptied[j] = (int32_t)m;
    }
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// components of up to 64 ids: one wavefront each, lane l owns the component's l-th id, set sizes in LDS
__global__ void __launch_bounds__(kBlock) cover_small_kernel(Graph g, const uint32_t *__restrict__ comp_off,
                                                             const uint32_t *__restrict__ sorted_id,
                                                             const int32_t *__restrict__ size0, int32_t n_comp) {
    __shared__ int32_t s_size[kSmallWaves][kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int64_t c = (int64_t)blockIdx.x * kSmallWaves + wave;
    if (c >= n_comp) return;
    const uint32_t off = comp_off[c], n = comp_off[c + 1] - off;
    if (n > (uint32_t)kWave) return;
    int32_t *size = s_size[wave];
    const uint32_t my = (uint32_t)lane < n ? sorted_id[off + lane] : 0u;
    size[lane] = (uint32_t)lane < n ? size0[off + lane] : 0;
    wave_sync();
    for (uint32_t it = 0; it < n; ++it) {
        const int32_t s = ld_wg(size + lane);
        const uint64_t best = wave_max(((uint64_t)(uint32_t)(s > 0 ? s : 0) << 32) | (uint32_t)(kWave - 1 - lane));
        if ((best >> 32) == 0) break;
        const int wl = kWave - 1 - (int)(best & (kWave - 1));
        const uint32_t m = (uint32_t)__shfl((int)my, wl, kWave);
        if (lane == wl) g.is_master[m] = 1u;
        for (uint32_t k = g.ioff[m] + lane; k < g.ioff[m + 1]; k += kWave) claim(g, k, m, size, off, n);
        wave_sync();
    }
}

// larger components: one workgroup each, its threads stride over the ids
__global__ void __launch_bounds__(kCoverBlock) cover_large_kernel(Graph g, const uint32_t *__restrict__ comp_off,
                                                                  const uint32_t *__restrict__ sorted_id,
                                                                  int32_t *__restrict__ size0,
                                                                  const uint32_t *__restrict__ list) {
    __shared__ int32_t s_size[kLdsIds];
    __shared__ uint64_t s_red[kCoverBlock / kWave];
    __shared__ uint64_t s_best;
    const uint32_t c = list[blockIdx.x];
    const uint32_t off = comp_off[c], n = comp_off[c + 1] - off;
    const uint32_t tid = threadIdx.x;
    int32_t *size = n <= (uint32_t)kLdsIds ? s_size : size0 + off;
    if (n <= (uint32_t)kLdsIds)
        for (uint32_t i = tid; i < n; i += kCoverBlock) s_size[i] = size0[off + i];
    __syncthreads();
    for (uint32_t it = 0; it < n; ++it) {
        uint64_t best = 0;
        for (uint32_t i = tid; i < n; i += kCoverBlock) {
            const int32_t s = ld_wg(size + i);
            const uint64_t key = ((uint64_t)(uint32_t)(s > 0 ? s : 0) << 32) | (0xFFFFFFFFu - i);
            best = key > best ? key : best;
        }
        best = wave_max(best);
        if (tid % kWave == 0) s_red[tid / kWave] = best;
        __syncthreads();
        if (tid < (uint32_t)kWave) {
            best = wave_max(tid < (uint32_t)(kCoverBlock / kWave) ? s_red[tid] : 0);
            if (tid == 0) s_best = best;
        }
        __syncthreads();
        best = s_best;
        if ((best >> 32) == 0) break;
        const uint32_t m = sorted_id[off + (0xFFFFFFFFu - (uint32_t)best)];
        if (tid == 0) g.is_master[m] = 1u;
        for (uint32_t k = g.ioff[m] + tid; k < g.ioff[m + 1]; k += kCoverBlock) claim(g, k, m, size, off, n);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) allow_kernel(const uint32_t *__restrict__ is_master,
                                                       const int32_t *__restrict__ id_string, int64_t I,
                                                       uint32_t *__restrict__ allowed) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += stride)
        if (is_master[i]) allowed[id_string[i]] = 1u;
}

// the kept edges get (pattern, rank) as key, the others sort behind them
__global__ void __launch_bounds__(kBlock) filter_key_kernel(const uint64_t *__restrict__ pkey, int64_t E,
                                                            const int32_t *__restrict__ id_string,
                                                            const int32_t *__restrict__ id_rank,
                                                            const uint32_t *__restrict__ allowed, uint64_t *__restrict__ key,
                                                            uint32_t *__restrict__ val, uint32_t *__restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        const uint32_t p = (uint32_t)(pkey[e] >> 32), i = (uint32_t)pkey[e];
        const bool keep = allowed[id_string[i]] != 0u;
        key[e] = keep ? (((uint64_t)p << 32) | (uint32_t)id_rank[i]) : ~(uint64_t)0;
        val[e] = i;
        if (keep) atomicAdd(&count[p], 1u);
    }
}

}  // namespace pg

extern "C" {

int adh_pg_create(adh_handle_t *h, adh_pg_t **out) {
    if (!h || !out) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    adh_pg *g = new adh_pg();
    g->h = h;
    *out = g;
    return ADH_OK;
}

int adh_pg_destroy(adh_pg_t *g) {
    if (!g) return ADH_OK;
    (void)hipSetDevice(g->h->device);
    (void)hipStreamSynchronize(g->h->stream);
    delete g;  // (the members free their device memory and events)
    return ADH_OK;
}

int adh_pg_solve(adh_pg_t *g, int32_t n_patterns, int32_t n_ids, int64_t n_edges, const int32_t *edge_pattern,
                 const int32_t *edge_id, const int32_t *weight, int32_t *pattern_master, int32_t *id_emptied_by) {
    if (!g || !edge_pattern || !edge_id || !weight || !pattern_master || !id_emptied_by)
        return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    const int64_t P = n_patterns, I = n_ids, E = n_edges;
    if (P < 1 || I < 1 || E < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pg_solve: no patterns, ids or edges");
    if (P + I >= (int64_t)0x7FFFFFF0ll || E >= (int64_t)0x7FFFFFF0ll)
        return fail(ADH_ERR_UNSUPPORTED, "adh_pg_solve: 2^31 nodes or edges and more are not supported");
    if (E > P * I) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pg_solve: more edges than patterns x ids");
    int64_t total = 0;
    for (int64_t p = 0; p < P; ++p) {
        if (weight[p] < 0) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pg_solve: negative pattern weight");
        total += weight[p];
    }
    if (total > (int64_t)0x7FFFFFFFll) return fail(ADH_ERR_UNSUPPORTED, "adh_pg_solve: the weights sum to 2^31 or more");
    for (int64_t e = 0; e < E; ++e)
        if (edge_pattern[e] < 0 || edge_pattern[e] >= P || edge_id[e] < 0 || edge_id[e] >= I)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pg_solve: edge " + std::to_string(e) + " is out of range");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    HIP_TRY(hipStreamSynchronize(st));
    g->bufs.release();
    g->pkey = nullptr, g->is_master = nullptr, g->solved = false;
    g->P = n_patterns, g->I = n_ids, g->E = E;
    g->label_ms = g->cover_ms = g->filter_ms = 0.0;
    g->n_comp = g->n_large = g->rounds = 0;

    const int64_t N = I + P;
    int32_t *d_ep = nullptr, *d_ei = nullptr, *d_w = nullptr, *d_master = nullptr, *d_emptied = nullptr, *d_size = nullptr;
    uint64_t *ikey_in = nullptr, *pkey_in = nullptr, *ikey = nullptr, *pkey = nullptr, *ckey_in = nullptr, *ckey = nullptr;
    uint32_t *ioff = nullptr, *poff = nullptr, *parent = nullptr, *flag = nullptr, *head = nullptr, *sorted_id = nullptr,
             *pos = nullptr, *comp_off = nullptr, *list = nullptr, *is_master = nullptr;
    auto &B = g->bufs;
    HIP_TRY(B.upload(&d_ep, edge_pattern, (size_t)E, st));
    HIP_TRY(B.upload(&d_ei, edge_id, (size_t)E, st));
    HIP_TRY(B.upload(&d_w, weight, (size_t)P, st));
    HIP_TRY(B.alloc(&d_master, (size_t)P));
    HIP_TRY(B.alloc(&d_emptied, (size_t)I));
    HIP_TRY(B.alloc(&d_size, (size_t)I));
    HIP_TRY(B.alloc(&ikey_in, (size_t)E));
    HIP_TRY(B.alloc(&pkey_in, (size_t)E));
    HIP_TRY(B.alloc(&ikey, (size_t)E));
    HIP_TRY(B.alloc(&pkey, (size_t)E));
    HIP_TRY(B.alloc(&ckey_in, (size_t)I));
    HIP_TRY(B.alloc(&ckey, (size_t)I));
    HIP_TRY(B.alloc(&ioff, (size_t)I + 1));
    HIP_TRY(B.alloc(&poff, (size_t)P + 1));
    HIP_TRY(B.alloc(&parent, (size_t)N));
    HIP_TRY(B.alloc(&flag, 4));  // [0] a round changed something, [1] number of large components
    HIP_TRY(B.alloc(&head, (size_t)I));
    HIP_TRY(B.alloc(&sorted_id, (size_t)I));
    HIP_TRY(B.alloc(&pos, (size_t)I));
    HIP_TRY(B.alloc(&comp_off, (size_t)I + 1));
    HIP_TRY(B.alloc(&list, (size_t)I));
    HIP_TRY(B.alloc(&is_master, (size_t)I));
    sess::BufsTmp tmp{B};  // hipCUB temporary storage: a superseded block stays in bufs, no free inside the call

    uint32_t n_comp = 0;
    int rounds = 0;
    bool converged = false;
    int rc = sess::timed(g->ev, st, g->label_ms, [&]() -> int {
        HIP_TRY(hipMemsetAsync(ioff, 0, ((size_t)I + 1) * 4, st));
        HIP_TRY(hipMemsetAsync(poff, 0, ((size_t)P + 1) * 4, st));
        hipLaunchKernelGGL(pg::keys_kernel, dim3(pg::grid_for(E)), dim3(pg::kBlock), 0, st, d_ep, d_ei, E, ikey_in, pkey_in,
                           ioff, poff);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::exclusive_sum(tmp, ioff, ioff, I + 1, st));
        ADH_TRY(sess::exclusive_sum(tmp, poff, poff, P + 1, st));
        ADH_TRY(sess::sort_keys(tmp, ikey_in, ikey, E, 64, st));
        ADH_TRY(sess::sort_keys(tmp, pkey_in, pkey, E, 64, st));
        hipLaunchKernelGGL(sess::iota_kernel, dim3(pg::grid_for(N)), dim3(pg::kBlock), 0, st, parent, N);
        HIP_TRY(hipGetLastError());
        while (rounds < pg::kMaxRounds) {
            ++rounds;
            HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
            hipLaunchKernelGGL(pg::hook_kernel, dim3(pg::grid_for(E)), dim3(pg::kBlock), 0, st, d_ep, d_ei, E, (uint32_t)I,
                               parent, flag);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pg::jump_kernel, dim3(pg::grid_for(N)), dim3(pg::kBlock), 0, st, parent, N, flag);
            HIP_TRY(hipGetLastError());
            uint32_t changed = 1;
            HIP_TRY(hipMemcpyAsync(&changed, flag, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (!changed) {
                converged = true;
                break;
            }
        }
        if (!converged) return ADH_OK;
        // the ids by (component, id code); a component's label is its smallest node, an id
        hipLaunchKernelGGL(pg::comp_key_kernel, dim3(pg::grid_for(I)), dim3(pg::kBlock), 0, st, parent, I, ckey_in);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::sort_keys(tmp, ckey_in, ckey, I, 64, st));
        hipLaunchKernelGGL(pg::comp_head_kernel, dim3(pg::grid_for(I)), dim3(pg::kBlock), 0, st, ckey, I, head);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::inclusive_sum(tmp, head, head, I, st));
        HIP_TRY(hipMemcpyAsync(&n_comp, head + (I - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ADH_OK;
    });
    g->rounds = rounds;
    if (rc != ADH_OK) return rc;
    if (!converged)
        return fail(ADH_ERR_HIP, "adh_pg_solve: the component labelling did not converge in " +
                                     std::to_string(pg::kMaxRounds) + " rounds");
    if (n_comp < 1 || (int64_t)n_comp > I) return fail(ADH_ERR_HIP, "adh_pg_solve: inconsistent component count");

    uint32_t n_large = 0;
    pg::Graph gr{ioff, ikey, poff, pkey, d_w, pos, d_master, d_emptied, is_master};
    rc = sess::timed(g->ev, st, g->cover_ms, [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_master, 0xFF, (size_t)P * 4, st));
        HIP_TRY(hipMemsetAsync(d_emptied, 0xFF, (size_t)I * 4, st));
        HIP_TRY(hipMemsetAsync(is_master, 0, (size_t)I * 4, st));
        HIP_TRY(hipMemsetAsync(flag, 0, 16, st));
        hipLaunchKernelGGL(pg::comp_fill_kernel, dim3(pg::grid_for(I)), dim3(pg::kBlock), 0, st, ckey, head, I, ioff, ikey,
                           d_w, sorted_id, pos, comp_off, d_size);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pg::large_kernel, dim3(pg::grid_for(n_comp)), dim3(pg::kBlock), 0, st, comp_off, (int32_t)n_comp,
                           list, flag + 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n_large, flag + 1, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)n_large > I) return fail(ADH_ERR_HIP, "adh_pg_solve: inconsistent component sizes");
        const unsigned small_blocks = (unsigned)(((int64_t)n_comp + pg::kSmallWaves - 1) / pg::kSmallWaves);
        hipLaunchKernelGGL(pg::cover_small_kernel, dim3(small_blocks), dim3(pg::kBlock), 0, st, gr, comp_off, sorted_id,
                           d_size, (int32_t)n_comp);
        HIP_TRY(hipGetLastError());
        if (n_large > 0) {
            hipLaunchKernelGGL(pg::cover_large_kernel, dim3(n_large), dim3(pg::kCoverBlock), 0, st, gr, comp_off, sorted_id,
                               d_size, list);
            HIP_TRY(hipGetLastError());
        }
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pattern_master, d_master, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(id_emptied_by, d_emptied, (size_t)I * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += (uint64_t)(P + I) * 4;
    g->pkey = pkey;
    g->is_master = is_master;
    g->n_comp = (int32_t)n_comp;
    g->n_large = (int32_t)n_large;
    g->solved = true;
    return ADH_OK;
}

int adh_pg_filter(adh_pg_t *g, int32_t n_strings, const int32_t *id_string, const int32_t *id_rank, int32_t *offsets,
                  int32_t *ids, int64_t *n_kept) {
    if (!g || !id_string || !id_rank || !offsets || !ids || !n_kept) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!g->solved) return fail(ADH_ERR_NOT_STAGED, "adh_pg_filter: no solved cover");
    const int64_t P = g->P, I = g->I, E = g->E, S = n_strings;
    if (S < 1) return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pg_filter: no strings");
    for (int64_t i = 0; i < I; ++i)
        if (id_string[i] < 0 || id_string[i] >= S || id_rank[i] < 0)
            return fail(ADH_ERR_INVALID_ARGUMENT, "adh_pg_filter: string code or rank of id " + std::to_string(i) +
                                                      " is out of range");
    HIP_TRY(hipSetDevice(g->h->device));
    hipStream_t st = g->h->stream;
    int32_t *d_str = nullptr, *d_rank = nullptr;
    uint32_t *allowed = nullptr, *count = nullptr, *val_in = nullptr, *val = nullptr;
    uint64_t *key_in = nullptr, *key = nullptr;
    auto &B = g->bufs;
    HIP_TRY(B.upload(&d_str, id_string, (size_t)I, st));
    HIP_TRY(B.upload(&d_rank, id_rank, (size_t)I, st));
    HIP_TRY(B.alloc(&allowed, (size_t)S));
    HIP_TRY(B.alloc(&count, (size_t)P + 1));
    HIP_TRY(B.alloc(&val_in, (size_t)E));
    HIP_TRY(B.alloc(&val, (size_t)E));
    HIP_TRY(B.alloc(&key_in, (size_t)E));
    HIP_TRY(B.alloc(&key, (size_t)E));
    // (the sort's temporary storage is in place before the timed part)
    sess::TmpSize sort;
    ADH_TRY(sess::sort_pairs(sort, key_in, key, val_in, val, E, 64, st));
    sess::BufsTmp sort_tmp{B}, scan_tmp{B};
    HIP_TRY(sort_tmp.reserve(sort.bytes));
    uint32_t kept = 0;
    g->filter_ms = 0.0;
    int rc = sess::timed(g->ev, st, g->filter_ms, [&]() -> int {
        HIP_TRY(hipMemsetAsync(allowed, 0, (size_t)S * 4, st));
        HIP_TRY(hipMemsetAsync(count, 0, ((size_t)P + 1) * 4, st));
        hipLaunchKernelGGL(pg::allow_kernel, dim3(pg::grid_for(I)), dim3(pg::kBlock), 0, st, g->is_master, d_str, I, allowed);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pg::filter_key_kernel, dim3(pg::grid_for(E)), dim3(pg::kBlock), 0, st, g->pkey, E, d_str, d_rank,
                           allowed, key_in, val_in, count);
        HIP_TRY(hipGetLastError());
        ADH_TRY(sess::exclusive_sum(scan_tmp, count, count, P + 1, st));
        ADH_TRY(sess::sort_pairs(sort_tmp, key_in, key, val_in, val, E, 64, st));
        HIP_TRY(hipMemcpyAsync(&kept, count + P, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ADH_OK;
    });
    if (rc != ADH_OK) return rc;
    if ((int64_t)kept > E) return fail(ADH_ERR_HIP, "adh_pg_filter: inconsistent edge count");
    HIP_TRY(hipMemcpyAsync(offsets, count, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, st));
    if (kept > 0) HIP_TRY(hipMemcpyAsync(ids, val, (size_t)kept * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->h->d2h_bytes += ((uint64_t)P + 1 + kept) * 4;
    *n_kept = kept;
    return ADH_OK;
}

int adh_pg_stats(adh_pg_t *g, int32_t *n_components, int32_t *n_large, int32_t *rounds) {
    if (!g || !n_components || !n_large || !rounds) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_components = g->n_comp;
    *n_large = g->n_large;
    *rounds = g->rounds;
    return ADH_OK;
}

int adh_pg_time_ms(adh_pg_t *g, double *label_ms, double *cover_ms, double *filter_ms) {
    if (!g || !label_ms || !cover_ms || !filter_ms) return fail(ADH_ERR_INVALID_ARGUMENT, "NULL argument");
    *label_ms = g->label_ms;
    *cover_ms = g->cover_ms;
    *filter_ms = g->filter_ms;
    return ADH_OK;
}

}  // extern "C"
