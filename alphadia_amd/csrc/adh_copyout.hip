// adh_copyout.hip - how the results of a host -> host scoring call leave the device (included by adh_score_host.hip,
// in front of the pipeline's driver, score_pipeline): the pack kernels and block layouts of the two compacted
// copy-outs, the host code that expands their blocks, the hand-off of landed blocks to a host team, the four
// copy-out modes the driver chooses from, and the ADH_DEBUG_TIMING trace of a call.

// ---- compacted copy-out of the fragment tables of the padded path.  A candidate fills the first K of its top_k fragment
// slots (K = fragments with signal: 4.6 of 12 on the headline) and 58 % of the 264 bytes per candidate that the five
// computed fragment tables + fragment_lib_slot put on PCIe are zeros.  Per chunk of the pipeline, behind its scoring
// kernels, two launches (adh_pack_count_kernel, adh_pack_rows_kernel) write the filled slots of the six columns into ONE
// block (PadBlock) and store the chunk's total straight into page-locked memory - the host sizes the block's single
// copy from it without a round trip behind the copy-out backlog (see adh_cop_pack_kernel for why no copy fetches it).
// The host team expands the block into the caller's padded tables and fills the library / id columns in the same pass
// (fill_host_rows).
#include "adh_fill_host.h"  // PadBlock, SparseBlock, fill_host_rows

// where the block of the chunk that starts at row a sits in the staging buffers (device and host alike): room for every
// slot filled - with every flag set a sparse block is a dense one plus its header and anchors, 8 bytes per anchored row
// (at most R / kAnchorRows + 1 of a chunk's R rows), so a block's place moves by 8 bytes per kAnchorRows rows in front
// of it on either wire - and 64 bytes of slack behind the last block (the host reads a row's 12 floats unmasked)
struct PadLayout {
    size_t per_row, total;
    PadLayout(int64_t n, int top_k, int64_t n_chunks)
        : per_row(4 + (size_t)top_k * 22), total(base(n, n_chunks + 1, 4 + (size_t)top_k * 22) + 64) {}
    size_t base(int64_t a, int64_t ci) const { return base(a, ci, per_row); }
    static size_t base(int64_t a, int64_t ci, size_t per_row_) {
        return ((size_t)a * per_row_ + ((size_t)(a / kAnchorRows) + (size_t)ci) * 8 + (size_t)ci * 1024 + 255) & ~(size_t)255;
    }
};

// ---- the sparse-slot wire of the same block (SparseBlock, adh_fill_host.h): fragment_intensity and
// fragment_correlation travel as streams of their non-zero words, so a row has four counts: its filled slots, the
// non-zero words of either stream among them, and the slot values that leave no room for the flags.
struct alignas(16) SlotCnt {
    uint32_t s, i, c, big;  // filled slots, non-zero intensity words, non-zero correlation words, slot values >= big_from
    __device__ SlotCnt &operator+=(const SlotCnt &b) {
        s += b.s, i += b.i, c += b.c, big += b.big;
        return *this;
    }
};

// ---- count and pack, two launches of kPackRows-thread workgroups, one workgroup per kPackRows rows of the chunk, on
// either wire (kSparseWire: SparseBlock, else PadBlock, which only uses the count of filled slots).  No workgroup waits
// for another: what a workgroup of the second launch needs of the others - the counts of the rows in front of its own
// and the chunk's totals - it sums itself from the per-workgroup totals the first launch left (a 524 288-row chunk has
// 2048 of them, 32 KB).  Before: a count kernel, hipcub::DeviceScan (its own launches) and a pack kernel per chunk.
constexpr int kPackRows = 256;

// the sum of v over the workgroup, in every thread (`lds`: one SlotCnt per wavefront)
__device__ inline SlotCnt pack_wg_sum(SlotCnt v, SlotCnt *lds) {
    for (int d = ADH_WAVE / 2; d > 0; d >>= 1) {
        v.s += __shfl_xor(v.s, d), v.i += __shfl_xor(v.i, d), v.c += __shfl_xor(v.c, d), v.big += __shfl_xor(v.big, d);
    }
    const int lane = (int)(threadIdx.x & (ADH_WAVE - 1)), wave = (int)(threadIdx.x / ADH_WAVE);
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    SlotCnt sum{0, 0, 0, 0};
    for (int w = 0; w < kPackRows / ADH_WAVE; ++w) sum += lds[w];
    __syncthreads();  // (lds may be written again)
    return sum;
}

// (A) one thread per row: cnt[i] for the chunk's n rows, wg_tot[w] for its (n + kPackRows - 1) / kPackRows workgroups.
// One thread per row walks three columns at 24- and 48-byte strides.  Measured and dropped: one thread per slot with
// the lanes of a row voting and the lane of slot 0 counting the votes - coalesced loads, but of all 12 slots of a row
// where 4.6 are filled: 0.069 - 0.071 ms per 500 000-row chunk against 0.048 - 0.052 (profiles/sparse_slots.json,
// `count_by_votes`).
template <bool kSparseWire>
__global__ __launch_bounds__(kPackRows) void adh_pack_count_kernel(const uint16_t *__restrict__ lib_slot,
                                                                   const uint32_t *__restrict__ intensity,
                                                                   const uint32_t *__restrict__ correlation, int64_t row0,
                                                                   int64_t n, int top_k, uint32_t big_from,
                                                                   SlotCnt *__restrict__ cnt, SlotCnt *__restrict__ wg_tot) {
    __shared__ SlotCnt s_sum[kPackRows / ADH_WAVE];
    const int64_t i = (int64_t)blockIdx.x * kPackRows + threadIdx.x;
    SlotCnt v{0, 0, 0, 0};
    if (i < n) {
        const int64_t r0 = (row0 + i) * (int64_t)top_k;
        const uint16_t *s = lib_slot + r0;
        for (; v.s < (uint32_t)top_k && s[v.s]; ++v.s) {  // (filled slots are the leading ones: candidate.py:403-442)
            if (kSparseWire) {
                v.i += intensity[r0 + v.s] != 0u;
                v.c += correlation[r0 + v.s] != 0u;
                v.big += s[v.s] >= big_from;
            }
        }
        cnt[i] = v;
    }
    const SlotCnt sum = pack_wg_sum(v, s_sum);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = sum;
}

// (B) the workgroup of rows [w * kPackRows, (w + 1) * kPackRows) of the chunk: the counts in front of its rows and the
// chunk's totals from wg_tot, an exclusive scan of its rows' counts in LDS, then every thread writes its row's offset
// (and anchor), and the threads share the rows' filled slots - consecutive threads take consecutive slots of a row, of
// as many slots per row as the fullest row of the workgroup has.  The last workgroup stores the totals into page-locked
// memory (`totals`: one word on the dense wire; format, S, NI, NC on the sparse one, as in the block's header).  On the
// sparse wire a slot's place in a stream comes from the votes of the lanes below it: 0.054 - 0.060 ms per 500 000-row
// chunk with one thread per slot, against 0.066 - 0.068 with every thread reading the row's slots in front of its own
// (profiles/sparse_slots.json, `pack_by_loop`).
template <bool kSparseWire>
__global__ __launch_bounds__(kPackRows) void adh_pack_rows_kernel(DevOut t, int64_t row0, int64_t n, int top_k,
                                                                  const SlotCnt *__restrict__ cnt,
                                                                  const SlotCnt *__restrict__ wg_tot,
                                                                  unsigned char *__restrict__ block, uint32_t *__restrict__ totals) {
    __shared__ SlotCnt s_sum[kPackRows / ADH_WAVE];
    __shared__ SlotCnt s_at[kPackRows + 1];  // where the workgroup's rows start in the slot columns and the streams
    __shared__ uint32_t s_kmax;
    const int tid = (int)threadIdx.x, lane = tid & (ADH_WAVE - 1), wave = tid / ADH_WAVE;
    const int64_t wg = blockIdx.x, n_wg = gridDim.x;
    if (tid == 0) s_kmax = 0;
    SlotCnt before{0, 0, 0, 0}, tot{0, 0, 0, 0};
    for (int64_t q = tid; q < n_wg; q += kPackRows) {
        const SlotCnt r = wg_tot[q];
        tot += r;
        if (q < wg) before += r;
    }
    before = pack_wg_sum(before, s_sum);
    tot = pack_wg_sum(tot, s_sum);
    // the rows' counts, scanned: in the wavefront, then over the wavefronts in front
    const int64_t i = wg * kPackRows + tid;
    SlotCnt v{0, 0, 0, 0};
    if (i < n) v = cnt[i];
    SlotCnt at = v;  // (inclusive)
    for (int d = 1; d < ADH_WAVE; d <<= 1) {
        const uint32_t ps = __shfl_up(at.s, d), pi = __shfl_up(at.i, d), pc = __shfl_up(at.c, d);
        if (lane >= d) at.s += ps, at.i += pi, at.c += pc;
    }
    if (lane == ADH_WAVE - 1) s_sum[wave] = at;
    if (v.s) atomicMax(&s_kmax, v.s);
    __syncthreads();
    for (int w = 0; w < wave; ++w) at.s += s_sum[w].s, at.i += s_sum[w].i, at.c += s_sum[w].c;
    at.s += before.s, at.i += before.i, at.c += before.c;
    s_at[tid + 1] = at;
    at.s -= v.s, at.i -= v.i, at.c -= v.c;  // (exclusive)
    if (tid == 0) s_at[0] = at;
    __syncthreads();

    const bool sparse = kSparseWire && tot.big == 0;
    const SparseBlock LS((uint64_t)row0, (uint64_t)n, tot.s, tot.i, tot.c, sparse);
    const PadBlock LP((uint64_t)n, tot.s);
    uint32_t *const off = reinterpret_cast<uint32_t *>(block + (kSparseWire ? LS.off : 0));
    const size_t o_slot = kSparseWire ? LS.slot : LP.slot;
    size_t o_f[5];
    for (int q = 0; q < 5; ++q) o_f[q] = kSparseWire ? LS.f[q] : LP.f[q];
    if (wg == n_wg - 1 && tid == 0) {
        if (kSparseWire) {
            const uint32_t head[4] = {sparse ? kWireSparse : kWireDense, tot.s, tot.i, tot.c};
            for (int q = 0; q < 4; ++q) reinterpret_cast<uint32_t *>(block)[q] = head[q], totals[q] = head[q];  // (totals: page-locked host memory)
        } else {
            totals[0] = tot.s;  // (page-locked host memory)
        }
        off[n] = tot.s;
    }
    if (i < n) {
        off[i] = at.s;
        if (sparse && (row0 + i) % kAnchorRows == 0) {  // (anchors sit on the table's row numbers)
            uint32_t *anchor = reinterpret_cast<uint32_t *>(block + LS.anchor) +
                               2 * ((row0 + i) / kAnchorRows - (int64_t)SparseBlock::anchor_row0((uint64_t)row0));
            anchor[0] = at.i, anchor[1] = at.c;
        }
    }
    const uint32_t *const intensity = reinterpret_cast<const uint32_t *>(t.fragment_intensity);
    const uint32_t *const correlation = reinterpret_cast<const uint32_t *>(t.fragment_correlation);
    const int64_t kmax = s_kmax;
    const int64_t span = std::min<int64_t>(kPackRows, n - wg * kPackRows) * kmax;  // (the same for every thread)
    for (int64_t first = 0; first < span; first += kPackRows) {
        const int64_t id = first + tid;
        const bool in_rows = id < span;
        const int r = in_rows ? (int)(id / kmax) : 0;
        const int j = in_rows ? (int)(id - (int64_t)r * kmax) : 0;
        const SlotCnt a = s_at[r];
        const bool filled = in_rows && (uint32_t)j < s_at[r + 1].s - a.s;
        const int64_t src = (row0 + wg * kPackRows + r) * (int64_t)top_k + j;
        const uint32_t vi = filled ? intensity[src] : 0u, vc = filled ? correlation[src] : 0u;
        // (every lane of the wavefront votes: a row's slots sit in consecutive lanes)
        const uint64_t nz_i = __ballot(vi != 0u), nz_c = __ballot(vc != 0u);
        if (filled) {
            const size_t dst = (size_t)a.s + (size_t)j;
            uint16_t word = t.fragment_lib_slot[src];
            size_t di = dst, dc = dst;
            if (sparse) {
                // the slot's place in a stream: the row's, plus the non-zero words of the row's j slots in front of this
                // one - the votes of the j lanes below this one, or, where the row began in the wavefront before, the
                // words themselves
                uint32_t pi = a.i, pc = a.c;
                if (j <= lane) {
                    const uint64_t below = ((1ull << j) - 1ull) << (lane - j);
                    pi += (uint32_t)__popcll(nz_i & below), pc += (uint32_t)__popcll(nz_c & below);
                } else {
                    for (int q = 0; q < j; ++q) pi += intensity[src - j + q] != 0u, pc += correlation[src - j + q] != 0u;
                }
                di = pi, dc = pc;
                word |= (vi ? kHasIntensity : 0u) | (vc ? kHasCorrelation : 0u);
            }
            reinterpret_cast<uint16_t *>(block + o_slot)[dst] = word;
            reinterpret_cast<float *>(block + o_f[0])[dst] = t.fragment_mz_observed[src];
            reinterpret_cast<float *>(block + o_f[1])[dst] = t.fragment_height[src];
            reinterpret_cast<float *>(block + o_f[3])[dst] = t.fragment_mass_error[src];
            if (!sparse || vi) reinterpret_cast<uint32_t *>(block + o_f[2])[di] = vi;
            if (!sparse || vc) reinterpret_cast<uint32_t *>(block + o_f[4])[dc] = vc;
        }
    }
}

// ---- compacted, column-major copy-out of the operator path (round 5, adh_score_candidates_compact).  What the
// DataFrames of collect_candidates / collect_fragments keep of the padded tables is 91 % of the rows and 38 % of the
// fragment slots (headline).  Per chunk, behind its scoring kernels: (valid, filled slots) per row as one 64-bit count,
// an exclusive scan, and a pack kernel that writes every column of the chunk's valid rows and filled slots - features
// transposed to [feature][row], the library columns of a slot read from the staged library, ids from the candidate
// table - DENSELY into the chunk's block of a device staging buffer (CopBlock: where a column starts follows from the
// chunk's two totals).  The totals reach the host first (8 bytes, stored by the pack kernel straight into page-locked
// memory); the host then moves the block with ONE DMA copy of exactly its used bytes into a page-locked twin, and host
// threads unpack finished blocks into the caller's arrays while later chunks are scored.
// (Measured and dropped: the pack kernel storing through PCIe straight into host memory.  Kernel stores reach the link
// rate - tools/probes/kcopy_probe.hip: 54-55 GB/s from 64 workgroups - but a copy-out kernel does not run BESIDE the
// scoring kernels: on a stream of its own its workgroups wait until the scoring stream's backlog has drained (first
// chunk on the host 15.7 ms into a 36 ms call), on a high-priority stream the launches of the scoring stream stall
// instead (52 ms), and a compute unit backed up with PCIe stores stalls every wavefront on it: scoring kernels of a step
// 14.5 ms alone, 16.8 beside 32 copying workgroups, 23.5 beside 64, 27.2 beside 128.  An 8-byte hipMemcpyAsync is such
// a kernel, too: with the totals fetched that way the first block arrived 57 ms into the call.)
__global__ void adh_cop_count_kernel(const uint8_t *__restrict__ valid, const uint16_t *__restrict__ lib_slot, int64_t row0,
                                     int64_t n, int top_k, uint64_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint64_t v = 0;
    if (i < n && valid[row0 + i]) {
        const uint16_t *s = lib_slot + (row0 + i) * (int64_t)top_k;
        uint32_t k = 0;
        while (k < (uint32_t)top_k && s[k]) ++k;  // (filled slots are the leading ones: candidate.py:403-442)
        v = (1ull << 32) | k;
    }
    cnt[i] = v;  // (entry n: 0, so that the scan's last entry is the total)
}

// a chunk's block, dense: [row u32 | filled slots u8 | features f32 [46][R]] for its R valid rows, then
// [fragment_lib_slot u16 | 5 computed float columns] for its S filled slots; every column starts on a multiple of 16
// bytes.  Round 6: what repeats the candidate table (precursor_idx, rank, and fragment_row = the row of a slot's
// candidate) and the seven library columns of a slot stay off the wire - 26 instead of 42 bytes per slot, 188 instead of
// 193 per row - and are rebuilt by the unpack team from the caller's candidate columns and the host copy of the
// library, as the padded path does (rebuild_host_rows).
struct CopBlock {
    size_t row, cnt, feat, s_slot, s_f[5], total;
    __host__ __device__ CopBlock(uint64_t R, uint64_t S) {
        size_t o = 0;
        row = o, o += (R * 4 + 15) & ~(size_t)15;
        cnt = o, o += (R + 15) & ~(size_t)15;
        feat = o, o += (R * 4 * ADH_NUM_FEATURES + 15) & ~(size_t)15;
        s_slot = o, o += (S * 2 + 15) & ~(size_t)15;
        for (int j = 0; j < 5; ++j) s_f[j] = o, o += (S * 4 + 15) & ~(size_t)15;
        total = o;
    }
};
// where the block of the chunk that starts at row a sits in the staging buffers (device and host alike): room for
// every row valid and every slot filled
struct CopLayout {
    size_t per_row, total;
    CopLayout(int64_t n, int top_k, int64_t n_chunks)
        : per_row(5 + 4 * ADH_NUM_FEATURES + (size_t)top_k * 22), total((size_t)n * per_row + (size_t)(n_chunks + 1) * 1024) {}
    size_t base(int64_t a, int64_t ci) const { return ((size_t)a * per_row + (size_t)ci * 1024 + 255) & ~(size_t)255; }
};

__global__ void adh_cop_pack_kernel(DevOut t, DevCands c, const LibRec *__restrict__ lib, int64_t row0, int64_t n, int top_k,
                                    const uint64_t *__restrict__ off, unsigned char *__restrict__ block,
                                    uint64_t *__restrict__ totals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t tot = off[n];
    const uint64_t R = tot >> 32, S = tot & 0xFFFFFFFFull;
    if (tid == 0) totals[0] = tot;  // (page-locked host memory)
    const CopBlock L(R, S);
    uint32_t *const o_row = reinterpret_cast<uint32_t *>(block + L.row);
    uint8_t *const o_cnt = block + L.cnt;
    float *const o_feat = reinterpret_cast<float *>(block + L.feat);
    // valid rows: row id, number of filled slots, the feature row transposed (consecutive lanes = consecutive output
    // rows of one column)
    for (int64_t i = tid; i < n; i += stride) {
        const uint64_t o = off[i], o1 = off[i + 1];
        if ((o1 >> 32) == (o >> 32)) continue;
        const int64_t j = (int64_t)(o >> 32), r = row0 + i;
        o_row[j] = (uint32_t)r;
        o_cnt[j] = (uint8_t)((uint32_t)o1 - (uint32_t)o);
        const float *f = t.features + r * ADH_NUM_FEATURES;
#pragma unroll
        for (int k = 0; k < ADH_NUM_FEATURES; ++k) o_feat[(size_t)k * R + (size_t)j] = f[k];
    }
    // filled slots
    uint16_t *const s_slot = reinterpret_cast<uint16_t *>(block + L.s_slot);
    const int64_t n_slots = n * (int64_t)top_k;
    for (int64_t id = tid; id < n_slots; id += stride) {
        const int64_t i = id / top_k;
        const int s = (int)(id - i * top_k);
        const uint64_t o = off[i], o1 = off[i + 1];
        const uint32_t a = (uint32_t)o, k = (uint32_t)o1 - a;
        if ((uint32_t)s >= k) continue;
        const int64_t r = row0 + i, src = r * (int64_t)top_k + s;
        const size_t dst = (size_t)a + (size_t)s;
        s_slot[dst] = t.fragment_lib_slot[src];
        reinterpret_cast<float *>(block + L.s_f[0])[dst] = t.fragment_mz_observed[src];
        reinterpret_cast<float *>(block + L.s_f[1])[dst] = t.fragment_height[src];
        reinterpret_cast<float *>(block + L.s_f[2])[dst] = t.fragment_intensity[src];
        reinterpret_cast<float *>(block + L.s_f[3])[dst] = t.fragment_mass_error[src];
        reinterpret_cast<float *>(block + L.s_f[4])[dst] = t.fragment_correlation[src];
    }
}

namespace {
// stripe w of T of a finished block (page-locked host copy) -> the caller's arrays (rows at base_r, slots at base_s): the
// stripe is a range of the block's valid rows together with their slots; what the block leaves out - ids, the row of a
// slot's candidate, the library columns - comes from the candidate columns `c` and the library `lib`
void cop_copy_stripe(const unsigned char *block, int64_t cnt_r, int64_t cnt_s, int64_t base_r, int64_t base_s,
                     adh_compact_output_t *out, int w, int T, const adh_candidates_t *c, const LibRec *lib) {
    const CopBlock L((uint64_t)cnt_r, (uint64_t)cnt_s);
    const int64_t lo = cnt_r * w / T, hi = cnt_r * (w + 1) / T;
    if (hi <= lo) return;
    const uint32_t *rows = reinterpret_cast<const uint32_t *>(block + L.row);
    const uint8_t *cnt = block + L.cnt;
    int64_t s_lo = 0;  // slots of the rows before the stripe
    for (int64_t j = 0; j < lo; ++j) s_lo += cnt[j];
    memcpy(out->row + base_r + lo, rows + lo, (size_t)(hi - lo) * 4);
    const float *fb = reinterpret_cast<const float *>(block + L.feat);
    for (int k = 0; k < ADH_NUM_FEATURES; ++k)
        memcpy(out->features + (size_t)k * (size_t)out->rows_capacity + (size_t)(base_r + lo),
               fb + (size_t)k * (size_t)cnt_r + (size_t)lo, (size_t)(hi - lo) * 4);
    const uint16_t *slot = reinterpret_cast<const uint16_t *>(block + L.s_slot);
    int64_t d = base_s + s_lo, at = s_lo;
    for (int64_t j = lo; j < hi; ++j) {
        const uint32_t r = rows[j];
        const uint32_t p = c->precursor_idx[r];
        const uint8_t rk = c->rank ? c->rank[r] : (uint8_t)0;
        out->precursor_idx[base_r + j] = p;
        out->rank[base_r + j] = rk;
        const LibRec *base = lib + c->frag_start_idx[r];
        const int k = (int)cnt[j];
        for (int q = 0; q < k; ++q, ++d, ++at) {
            const LibRec &l = base[slot[at] - 1];
            out->fragment_row[d] = r;
            out->fragment_precursor_idx[d] = p;
            out->fragment_rank[d] = rk;
            out->fragment_mz_library[d] = l.mz_library;
            out->fragment_mz[d] = l.mz;
            out->fragment_position[d] = l.position;
            out->fragment_number[d] = l.number;
            out->fragment_type[d] = l.type;
            out->fragment_charge[d] = l.charge;
            out->fragment_loss_type[d] = l.loss_type;
        }
    }
    const size_t m = (size_t)(at - s_lo);
    if (m) {
        float *const fcol[5] = {out->fragment_mz_observed, out->fragment_height, out->fragment_intensity, out->fragment_mass_error,
                                out->fragment_correlation};
        for (int j = 0; j < 5; ++j) memcpy(fcol[j] + base_s + s_lo, block + L.s_f[j] + (size_t)s_lo * 4, m * 4);
    }
}

// rows [a, b) of the rebuildable host columns (OutputPsmDF columns that repeat the candidate table / the library,
// alphadia/search/scoring/output.py:17-97; written by the kernels as candidate.py:175-176, 403-481)
void rebuild_host_rows(const adh_handle *h, const adh_candidates_t *c, adh_output_t *out, const uint16_t *slots,
                       int64_t a, int64_t b) {
    const int top_k = out->top_k;
    const LibRec *lib = h->h_lib.data();
    for (int64_t i = a; i < b; ++i) {
        const bool skip = c->flags && (c->flags[i] & ADH_FLAG_SKIP);
        const uint32_t p = skip ? 0u : c->precursor_idx[i];
        const uint8_t r = skip ? (uint8_t)0 : c->rank[i];
        out->precursor_idx[i] = p;
        out->rank[i] = r;
        const LibRec *base = lib + c->frag_start_idx[i];
        for (int j = 0; j < top_k; ++j) {
            const size_t o = (size_t)i * (size_t)top_k + (size_t)j;
            const uint16_t s = slots[o];
            if (s) {
                const LibRec &l = base[s - 1];
                out->fragment_precursor_idx[o] = p;
                out->fragment_rank[o] = r;
                out->fragment_mz_library[o] = l.mz_library;
                out->fragment_mz[o] = l.mz;
                out->fragment_position[o] = l.position;
                out->fragment_number[o] = l.number;
                out->fragment_type[o] = l.type;
                out->fragment_charge[o] = l.charge;
                out->fragment_loss_type[o] = l.loss_type;
            } else {
                out->fragment_precursor_idx[o] = 0;
                out->fragment_rank[o] = 0;
                out->fragment_mz_library[o] = 0.0f;
                out->fragment_mz[o] = 0.0f;
                out->fragment_position[o] = 0;
                out->fragment_number[o] = 0;
                out->fragment_type[o] = 0;
                out->fragment_charge[o] = 0;
                out->fragment_loss_type[o] = 0;
            }
        }
    }
}

// this rank's share of the host: at most 16 threads, and of the cores this process may use (host_cpu_budget: quota,
// affinity, hardware) only the LOCAL_WORLD_SIZE-th part - the ranks of a node run side by side under ONE quota
int host_thread_share() {
    int t = 16;
    if (const char *env = getenv("ADH_HOST_THREADS")) t = atoi(env);
    else {
        int ranks = 1;
        if (const char *lw = getenv("LOCAL_WORLD_SIZE")) ranks = std::max(atoi(lw), 1);
        t = std::min<int>(t, std::max<int>(host_cpu_budget() / ranks, 1));
    }
    return std::max(t, 1);
}

int host_threads_for(int64_t n) {
    // the team that rebuilds the id / library columns behind the copy-out (or unpacks the compact blocks)
    const int t = (int)std::min<int64_t>(host_thread_share(), n / 16384);  // (a thread per 16 k rows at least: starting one costs ~20 us)
    return std::max(t, 1);
}

// Does the host rebuild the id / library columns of the padded tables (197 of 646 bytes per candidate stay off PCIe),
// or does the device write them and the link carry everything?  A thread rebuilds ~23 000 rows per ms, the link delivers
// 122 000 rows per ms of wire tables: below ~6 threads the team is what the call waits for (measured with 2 threads -
// the eighth part of the pool's 16-core quota: a 375 000-row shard takes 8.9 ms against 4.6), and the 44 % more bytes
// cost less (every GPU of a node has its own link, the ranks share the CPU quota).  ADH_REBUILD_MIN_THREADS moves the
// threshold (0: always rebuild).
bool host_rebuild_pays() {
    int least = 6;
    if (const char *env = getenv("ADH_REBUILD_MIN_THREADS")) least = atoi(env);
    return host_thread_share() >= least;
}

// Does the padded path copy the fragment tables out compacted (adh_pad_pack_kernel, fill_host_rows)?  The wire drops from
// 449 to ~290 bytes per candidate, and the host team writes the 5 computed columns it no longer gets by DMA.  That pays
// where the call waits for the link and the team keeps pace with it: a large table (ADH_COMPACT_MIN_ROWS, default
// 1 000 000 rows) and at least 12 threads of host.  ADH_COMPACT_COPY_OUT=1 / =0 forces it on / off.
bool compact_copy_out_pays(int64_t n) {
    if (const char *env = getenv("ADH_COMPACT_COPY_OUT")) return atoi(env) != 0;
    int64_t least_rows = 1000000;
    if (const char *env = getenv("ADH_COMPACT_MIN_ROWS")) least_rows = atoll(env);
    return host_thread_share() >= 12 && n >= least_rows;
}

// Do the packed blocks of that copy-out carry fragment_intensity and fragment_correlation as streams of their non-zero
// words (the sparse-slot wire: SparseBlock)?  1.47 of the 5 float words of a filled slot are zeros on the headline, 9 %
// of the call's bytes on the link; the host team reads fewer bytes and writes the same ones.  That pays where the call
// waits for the link: tables of ADH_SPARSE_SLOTS_MIN_ROWS rows (default 1 000 000) and more.  ADH_SPARSE_SLOTS=1 / =0
// forces it on / off; it only ever applies to a call that takes the compacted copy-out.
bool sparse_slots_pay(int64_t n) {
    if (const char *env = getenv("ADH_SPARSE_SLOTS")) return atoi(env) != 0;
    int64_t least_rows = 1000000;
    if (const char *env = getenv("ADH_SPARSE_SLOTS_MIN_ROWS")) least_rows = atoll(env);
    return n >= least_rows;
}

// The hand-off of landed blocks to a host team (the compacted copy-outs).  The enqueue thread only appends the event
// that follows a block's copy (append).  Whichever thread of the team runs out of work first becomes the watcher: it
// waits on the oldest event nobody has waited for, runs `landed` for that chunk and publishes it.  So a block reaches
// the team when its copy ends, wherever the enqueue thread happens to be (it sleeps a chunk long waiting for the next
// pack total; a poll from there found a block either at once or one chunk - 2.6 ms - late).  Nobody spins: the watcher
// sits in hipEventSynchronize, the others back off to short sleeps (a team that spins burns the CPU quota the busy
// ones need; a team woken all at once from a condition variable took 3 - 8 ms over a 500 000-row block instead of
// 1.5 - 2.5 and ended 3 - 17 ms behind the last copy: profiles/headline_pipeline.json, `condition_variable`).
// The events live in an array sized for every chunk
// before a thread starts: the enqueue thread writes entry `appended` and then raises the count, the watcher - one at
// a time, the role is claimed with `watching` - reads entries below it; what `landed` writes is published with `ready`.
struct BlockHandoff {
    std::vector<hipEvent_t> events;
    std::atomic<int64_t> appended{0}, ready{0};
    std::atomic<bool> watching{false}, abort{false};
    hipError_t error = hipSuccess;  // (written by a watcher before it raises `abort`)
    int device = 0;
    std::function<void(int64_t)> landed;  // once per chunk, in order, before the chunk is published

    BlockHandoff(int64_t n_chunks, int device_) : events((size_t)std::max<int64_t>(n_chunks, 0), nullptr), device(device_) {}
    int append(hipEvent_t ev) {  // (the enqueue thread only)
        const int64_t k = appended.load(std::memory_order_relaxed);
        if (k >= (int64_t)events.size())  // (an event nobody would ever wait for: a waiter of its chunk would hang)
            return fail(ADH_ERR_INVALID_ARGUMENT, "scoring pipeline: more copy-out events than chunks");
        events[(size_t)k] = ev;
        appended.store(k + 1, std::memory_order_release);
        return ADH_OK;
    }
    void stop() { abort.store(true, std::memory_order_release); }  // (an early return: whoever still waits gives up)
    // true once chunk ci has landed; false when the call is given up or a wait has failed (`error`)
    bool wait_for(int64_t ci) {
        for (int spin = 0;; ++spin) {
            if (ready.load(std::memory_order_acquire) > ci) return true;
            if (abort.load(std::memory_order_acquire)) return false;
            if (appended.load(std::memory_order_acquire) > ready.load(std::memory_order_relaxed) &&
                !watching.exchange(true, std::memory_order_acq_rel)) {
                const int64_t k = ready.load(std::memory_order_acquire);  // (nobody else moves it while the role is held)
                if (k < appended.load(std::memory_order_acquire)) {
                    hipError_t q = hipSetDevice(device);
                    if (q == hipSuccess) q = hipEventSynchronize(events[(size_t)k]);
                    if (q == hipSuccess && landed) landed(k);
                    if (q == hipSuccess) {
                        ready.store(k + 1, std::memory_order_release);
                    } else {
                        error = q;
                        abort.store(true, std::memory_order_release);
                    }
                }
                watching.store(false, std::memory_order_release);
                spin = 0;
                continue;
            }
            if (spin < 64) std::this_thread::yield();
            else std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
};

// the threads that follow a BlockHandoff (declared behind what they read: it is destroyed - joined - first)
struct HandoffTeam {
    BlockHandoff &handoff;
    std::vector<std::thread> threads;
    explicit HandoffTeam(BlockHandoff &handoff_) : handoff(handoff_) {}
    void join_all() {
        for (std::thread &t : threads)
            if (t.joinable()) t.join();
    }
    ~HandoffTeam() {
        handoff.stop();
        join_all();
    }
};

// the scratch of hipcub's exclusive scan over `items` entries of type Word (a grow-only buffer of the handle)
template <typename Word>
int grow_scan_scratch(void **p, size_t *bytes, int64_t items, hipStream_t st) {
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (Word *)nullptr, (Word *)nullptr, (int)items, st));
    return grow_device(p, bytes, need, 256);
}
// has the caller passed every array of a compact output?
bool compact_output_complete(const adh_compact_output_t *o) {
    return o->row && o->precursor_idx && o->rank && o->features && o->fragment_row && o->fragment_precursor_idx &&
           o->fragment_rank && o->fragment_mz_library && o->fragment_mz && o->fragment_mz_observed && o->fragment_height &&
           o->fragment_intensity && o->fragment_mass_error && o->fragment_correlation && o->fragment_position &&
           o->fragment_number && o->fragment_type && o->fragment_charge && o->fragment_loss_type;
}

// starts up to T threads that follow the team's hand-off: thread w runs stripe(ci, w) for every chunk, in order, as the
// chunks land.  Returns how many threads could be started.
template <typename Stripe>
int start_handoff_team(HandoffTeam &team, int T, int64_t n_chunks, Stripe stripe) {
    BlockHandoff &handoff = team.handoff;
    auto worker = [&handoff, n_chunks, stripe](int w) {
        for (int64_t ci = 0; ci < n_chunks; ++ci) {
            // (waiting threads sleep: a team that spins burns the CPU quota the busy ones need)
            if (!handoff.wait_for(ci)) return;
            stripe(ci, w);
        }
    };
    int started = 0;
    for (int w = 0; w < T; ++w) {
        try {
            team.threads.emplace_back(worker, w);
            ++started;
        } catch (const std::system_error &) {
            break;  // (the threads there are - at the end the calling thread too - take the rest)
        }
    }
    return started;
}

// ---- ADH_DEBUG_TIMING (developer switch): =1 the stage times of a call to stderr, =2 also per-chunk D2H spans, the
// hand-off of every packed block and the time line of the scoring stream.  With the switch off every method returns
// at once.
struct PipelineTrace {
    const bool timing = getenv("ADH_DEBUG_TIMING") != nullptr;
    const bool events = timing && atoi(getenv("ADH_DEBUG_TIMING")) >= 2;
    const double t_0 = now();
    double t_1 = 0.0, t_2 = 0.0;       // set-up done, everything enqueued
    std::vector<hipEvent_t> spans;     // copy-out stream, per chunk: before and behind the copies of its tables
    std::vector<uint64_t> span_bytes;  // copy-out bytes of every chunk
    hipEvent_t start = nullptr;        // on the copy-in stream, before the first column goes up
    double start_host = 0.0;           // the host's clock when `start` was recorded
    std::vector<hipEvent_t> marks;     // scoring stream, per chunk: before its kernels, behind them, behind its helpers
    std::vector<hipEvent_t> plans;     // copy-in stream, per chunk: before and behind its plan
    std::vector<double> plan_seen, enqueued;  // the host's clock, per chunk: its plan read, its kernels and helpers enqueued
    // the hand-off of every packed block on the host's clock (ms after the call began): its total seen by the enqueue
    // thread, the team told that it has landed, every thread of the team done with its stripe (one entry per chunk
    // and thread: each thread writes its own)
    int T = 0;
    std::vector<double> tot_seen, told, stripe_done, stripe_took;
    std::vector<uint64_t> blk_bytes, blk_dense_bytes;  // a block's copy, and what the dense block (PadBlock) of the chunk holds

    static double now() {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    double since() const { return now() - t_0; }  // ms after the call began
    ~PipelineTrace() {  // (the events go on every way out of the call)
        for (hipEvent_t e : spans) (void)hipEventDestroy(e);
        for (hipEvent_t e : marks) (void)hipEventDestroy(e);
        for (hipEvent_t e : plans) (void)hipEventDestroy(e);
        if (start) (void)hipEventDestroy(start);
    }
    void expect_blocks(int64_t n_chunks, int threads) {
        if (!events) return;
        T = threads;
        tot_seen.assign((size_t)n_chunks, 0.0), told.assign((size_t)n_chunks, 0.0);
        blk_bytes.assign((size_t)n_chunks, 0), blk_dense_bytes.assign((size_t)n_chunks, 0);
        stripe_done.assign((size_t)n_chunks * (size_t)T, 0.0), stripe_took.assign((size_t)n_chunks * (size_t)T, 0.0);
    }
    hipEvent_t stamp(hipStream_t st) const {  // (a time stamp on a stream; NULL with the switch off)
        hipEvent_t e = nullptr;
        if (events && hipEventCreate(&e) == hipSuccess) (void)hipEventRecord(e, st);
        return e;
    }
    void mark_start(hipStream_t si) { start = stamp(si), start_host = since(); }
    void mark(hipStream_t sk) { if (events) marks.push_back(stamp(sk)); }
    void mark_plan(hipStream_t si) { if (events) plans.push_back(stamp(si)); }
    void plan_read() { if (events) plan_seen.push_back(since()); }
    void chunk_enqueued() { if (events) enqueued.push_back(since()); }
    void span_begin(hipStream_t so, uint64_t d2h_bytes) { if (events) spans.push_back(stamp(so)), span_bytes.push_back(d2h_bytes); }
    void span_end(hipStream_t so, uint64_t d2h_bytes) {
        if (events) spans.push_back(stamp(so)), span_bytes.back() = d2h_bytes - span_bytes.back();
    }
    void total_seen(int64_t ci) { if (events) tot_seen[(size_t)ci] = since(); }
    void block_sent(int64_t ci, uint64_t bytes, uint64_t dense) {
        if (events && (size_t)ci < blk_bytes.size()) blk_bytes[(size_t)ci] = bytes, blk_dense_bytes[(size_t)ci] = dense;
    }
    void team_told(int64_t ci) { if (events) told[(size_t)ci] = since(); }
    double stripe_begin() const { return events ? now() : 0.0; }
    void stripe_end(int64_t ci, int w, double t_in) {
        if (events && w < T) {
            stripe_done[(size_t)ci * (size_t)T + (size_t)w] = since();
            stripe_took[(size_t)ci * (size_t)T + (size_t)w] = now() - t_in;
        }
    }
    // at the end of a call that succeeded; `packed`: chunk_done holds the events behind the packed blocks
    void report(const std::vector<int64_t> &cut, const std::vector<hipEvent_t> &chunk_done, bool packed) const {
        if (timing)
            fprintf(stderr, "[adh] score_candidates n=%lld in %lld chunks: setup %.2f ms, enqueue %.2f, drain %.2f\n",
                    (long long)cut.back(), (long long)cut.size() - 1, t_1 - t_0, t_2 - t_1, now() - t_2);
        if (!events) return;
        for (size_t i = 0; i + 1 < spans.size(); i += 2) {
            float ms = 0.f, since_first = 0.f;
            (void)hipEventElapsedTime(&ms, spans[i], spans[i + 1]);
            (void)hipEventElapsedTime(&since_first, spans[0], spans[i]);
            float from_start = 0.f;
            if (start) (void)hipEventElapsedTime(&from_start, start, spans[i]);
            fprintf(stderr, "[adh]   chunk %zu (%lld rows): D2H starts %.2f ms after the first (%.2f ms after the call's first copy-in), "
                            "lasts %.2f ms for %.1f MB = %.1f GB/s\n",
                    i / 2, (long long)(cut[i / 2 + 1] - cut[i / 2]), since_first, from_start, ms, (double)span_bytes[i / 2] / 1e6,
                    (double)span_bytes[i / 2] / 1e6 / std::max(ms, 1e-3f));
        }
        // the hand-off of the packed blocks; a copy's end is its event's time behind `start`, put on the host's clock
        // at the moment `start` was recorded (the copy-in stream is idle then)
        const double t_ret = now() - t_0;
        double last_landed = 0.0;
        for (size_t ci = 0; packed && start && ci < chunk_done.size() && ci < told.size(); ++ci) {
            float landed = 0.f;
            (void)hipEventElapsedTime(&landed, start, chunk_done[ci]);
            last_landed = start_host + landed;
            double team_done = 0.0, took_lo = 1e30, took_hi = 0.0;
            for (int w = 0; w < T; ++w) {
                team_done = std::max(team_done, stripe_done[ci * (size_t)T + (size_t)w]);
                took_lo = std::min(took_lo, stripe_took[ci * (size_t)T + (size_t)w]);
                took_hi = std::max(took_hi, stripe_took[ci * (size_t)T + (size_t)w]);
            }
            fprintf(stderr, "[adh]   block %zu: total seen %.2f ms after the call began, copy ended %.2f, team told %.2f (lag %.2f), "
                            "last thread done %.2f (a stripe took %.2f - %.2f ms)",
                    ci, tot_seen[ci], last_landed, told[ci], told[ci] - last_landed, team_done, took_lo, took_hi);
            if (ci < blk_bytes.size() && blk_bytes[ci])
                fprintf(stderr, "; %.2f MB copied, %.2f MB as a dense block", (double)blk_bytes[ci] / 1e6, (double)blk_dense_bytes[ci] / 1e6);
            fprintf(stderr, "\n");
        }
        if (packed && start)
            fprintf(stderr, "[adh]   tail: the call returns %.2f ms after it began, %.2f ms after the last copy ended\n", t_ret,
                    t_ret - last_landed);
        // the scoring stream: a chunk's kernels, its helpers (count, scan, pack), the idle time in front of it
        double k_sum = 0.0;
        for (size_t i = 0; i + 2 < marks.size(); i += 3) {
            float k_ms = 0.f, help_ms = 0.f, idle_ms = 0.f, at = 0.f;
            (void)hipEventElapsedTime(&k_ms, marks[i], marks[i + 1]);
            (void)hipEventElapsedTime(&help_ms, marks[i + 1], marks[i + 2]);
            if (i >= 3) (void)hipEventElapsedTime(&idle_ms, marks[i - 1], marks[i]);
            if (start) (void)hipEventElapsedTime(&at, start, marks[i]);
            k_sum += (double)k_ms + (double)help_ms;
            fprintf(stderr, "[adh]   chunk %zu: kernels start %.2f ms after the call's first copy-in, last %.2f ms, helpers %.3f ms, "
                            "scoring stream idle before them %.2f ms\n", i / 3, at, k_ms, help_ms, idle_ms);
            // what the kernels waited for: the chunk's plan on the copy-in stream, and the host that reads it and
            // enqueues the kernels (the host's clock, put on the copy-in stream's as `start` was recorded)
            const size_t ci = i / 3;
            if (start && 2 * ci + 1 < plans.size() && ci < plan_seen.size() && ci < enqueued.size()) {
                float p0 = 0.f, p1 = 0.f;
                (void)hipEventElapsedTime(&p0, start, plans[2 * ci]);
                (void)hipEventElapsedTime(&p1, start, plans[2 * ci + 1]);
                fprintf(stderr, "[adh]   chunk %zu: plan runs %.2f - %.2f ms after the call's first copy-in, read by the host at %.2f, "
                                "kernels and helpers enqueued by %.2f\n", ci, p0, p1, plan_seen[ci] - start_host,
                        enqueued[ci] - start_host);
            }
        }
        if (marks.size() >= 3) {
            float span = 0.f;
            (void)hipEventElapsedTime(&span, marks.front(), marks.back());
            fprintf(stderr, "[adh]   scoring stream: %.2f ms from the first kernel to the last helper, %.2f ms of them busy\n", span, k_sum);
        }
    }
};

// ---- the copy-out modes of the host -> host pipeline.  A mode offers the driver (score_pipeline) these steps:
// prepare() before the loop, start_team() once the device has work; per chunk pack(ci) on the scoring stream behind the
// kernels of chunk ci and copy_out(ci) once the event of those kernels is recorded; behind the loop flush() - what is
// still to be enqueued - and finish(), which waits for the copies and the team.  A mode that fails returns at once: its
// destructor stops and joins its team before the buffers the team reads go away, the driver synchronises the device
// after that.  The base class is the resident mode - nothing is copied back - and what every mode sees of the call
// (the driver owns all of it; the events of both lists go back to the handle's pool when the call ends).
struct CopyOut {
    adh_handle *const h;
    const adh_candidates_t *const c;
    adh_output_t &dev;                // the device tables
    const std::vector<int64_t> &cut;  // chunk ci is rows [cut[ci], cut[ci + 1])
    std::vector<hipEvent_t> &chunk_done;  // copy-out stream, per chunk: what the host works on has landed
    std::vector<hipEvent_t> &tot_ready;   // scoring stream, per chunk: its pack kernel is done, its total on the host
    PipelineTrace &trace;
    const int64_t n = cut.back(), n_chunks = (int64_t)cut.size() - 1;
    const int top_k = dev.top_k;
    bool tables_stand = false;  // set by a finish() that fails although the device tables are complete
    CopyOut(adh_handle *h_, const adh_candidates_t *c_, adh_output_t &dev_, const std::vector<int64_t> &cut_,
            std::vector<hipEvent_t> &chunk_done_, std::vector<hipEvent_t> &tot_ready_, PipelineTrace &trace_)
        : h(h_), c(c_), dev(dev_), cut(cut_), chunk_done(chunk_done_), tot_ready(tot_ready_), trace(trace_) {}
    virtual ~CopyOut() = default;
    virtual int prepare() { return ADH_OK; }
    virtual void start_team() {}
    virtual int pack(int64_t) { return ADH_OK; }
    virtual int copy_out(int64_t) { return ADH_OK; }
    virtual int flush() { return ADH_OK; }
    virtual int finish() { return ADH_OK; }

    int64_t longest_chunk() const {
        int64_t longest = 0;
        for (size_t i = 1; i < cut.size(); ++i) longest = std::max(longest, cut[i] - cut[i - 1]);
        return longest;
    }
    // an event on stream st, appended to `list`
    int record(hipStream_t st, std::vector<hipEvent_t> &list) {
        hipEvent_t ev = nullptr;
        const int rc = get_event(h, &ev);
        if (rc != ADH_OK) return rc;
        list.push_back(ev);  // (first: it returns to the pool whatever happens next)
        HIP_TRY(hipEventRecord(ev, st));
        return ADH_OK;
    }
    // the enqueue side of a packed block whose length the host has just learnt: ONE copy of its used bytes, the event
    // behind it, and that event to the team
    int send_block(BlockHandoff &handoff, void *host, const void *device, size_t bytes) {
        if (bytes > 0) HIP_TRY(hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, h->stream_out));
        const int rc = record(h->stream_out, chunk_done);
        return rc != ADH_OK ? rc : handoff.append(chunk_done.back());
    }
};

// The padded tables, row range by row range as they are; with `rebuild` only the wire columns, and a host team
// rebuilds the id / library columns from fragment_lib_slot (rebuild_host_rows) behind the copies.
struct PlainCopyOut : CopyOut {
    adh_output_t *const out;
    const bool rebuild;
    uint16_t *slot_host = nullptr;  // where fragment_lib_slot lands: the caller's column or the handle's staging buffer
    PlainCopyOut(const CopyOut &call, adh_output_t *out_, bool rebuild_) : CopyOut(call), out(out_), rebuild(rebuild_) {}

    int prepare() override {
        slot_host = out->fragment_lib_slot;
        if (rebuild && !slot_host) {
            const size_t need = (size_t)n * (size_t)top_k * sizeof(uint16_t);
            const int rc = grow_pinned(&h->slot_stage, &h->slot_stage_bytes, need, need / 8);
            if (rc != ADH_OK) return rc;
            slot_host = static_cast<uint16_t *>(h->slot_stage);
        }
        return ADH_OK;
    }
    // the tables of chunk ci that travel as they are (all of them, the wire columns, or - `fragment_tables` false - valid
    // + features beside the packed block), row range by row range
    // (A chunk is up to nine copies and the engine idles ~10 us between two of them - a 47 000-row chunk, 21 MB, takes
    // 0.46 ms = 46 GB/s where each copy runs at 55, `rocprofv3 --memory-copy-trace` - but a second copy-out stream for
    // the feature table does not fill the gaps: measured in round 5, same times to the 0.01 ms, and taken out again.)
    int copy_tables(int64_t ci, bool fragment_tables) {
        const int64_t a = cut[(size_t)ci], b = cut[(size_t)ci + 1];
        hipStream_t so = h->stream_out;
        trace.span_begin(so, h->d2h_bytes);
        for (int i = 0; i < kNumOutFields; ++i) {
            const OutFieldDesc &f = kOutFields[i];
            void *host = *out_member(out, f);
            const bool is_slot = f.member == offsetof(adh_output_t, fragment_lib_slot);
            const bool is_stat = f.member == offsetof(adh_output_t, stat_matched_peaks);
            if (is_slot && !host && rebuild) host = slot_host;
            if (!host) continue;
            if (rebuild && !f.wire && !is_stat) continue;      // rebuilt on the host (finish)
            if (!fragment_tables && f.per_row < 0) continue;  // the fragment tables travel packed
            const size_t rb = out_row_bytes(f, top_k);
            hipError_t e = hipMemcpyAsync(static_cast<unsigned char *>(host) + (size_t)a * rb,
                                          static_cast<unsigned char *>(*out_member(&dev, f)) + (size_t)a * rb,
                                          (size_t)(b - a) * rb, hipMemcpyDeviceToHost, so);
            if (e != hipSuccess) return fail(ADH_ERR_HIP, std::string("hipMemcpyAsync D2H: ") + hipGetErrorString(e));
            h->d2h_bytes += (uint64_t)(b - a) * rb;
        }
        trace.span_end(so, h->d2h_bytes);
        return ADH_OK;
    }
    int copy_out(int64_t ci) override {
        HIP_TRY(hipStreamWaitEvent(h->stream_out, h->ev_k[ci & 1], 0));
        const int rc = copy_tables(ci, true);
        if (rc != ADH_OK || !rebuild) return rc;
        return record(h->stream_out, chunk_done);
    }
    int finish() override {
        if (!rebuild) return ADH_OK;
        // host threads follow the copy-out stream chunk by chunk: thread w takes the w-th stripe of every chunk
        const int T = host_threads_for(n);
        std::atomic<int64_t> ready{0};
        std::atomic<bool> abort{false};
        auto stripe = [&](int64_t ci, int w) {
            const int64_t a = cut[(size_t)ci], b = cut[(size_t)ci + 1];
            const int64_t lo = a + (b - a) * w / T, hi = a + (b - a) * (w + 1) / T;
            rebuild_host_rows(h, c, out, slot_host, lo, hi);
        };
        auto worker = [&](int w) {
            for (int64_t ci = 0; ci < n_chunks; ++ci) {
                while (ready.load(std::memory_order_acquire) <= ci) {
                    if (abort.load(std::memory_order_relaxed)) return;
                    std::this_thread::yield();
                }
                stripe(ci, w);
            }
        };
        std::vector<std::thread> team;
        for (int w = 1; w < T; ++w) {
            try {
                team.emplace_back(worker, w);
            } catch (const std::system_error &) {
                break;  // (the calling thread takes the stripes that have no thread)
            }
        }
        const int started = (int)team.size() + 1;
        hipError_t ee = hipSuccess;
        for (int64_t ci = 0; ci < n_chunks && ee == hipSuccess; ++ci) {
            ee = hipEventSynchronize(chunk_done[(size_t)ci]);
            if (ee != hipSuccess) break;
            ready.store(ci + 1, std::memory_order_release);
            stripe(ci, 0);
            for (int w = started; w < T; ++w) stripe(ci, w);
        }
        if (ee != hipSuccess) abort.store(true);
        for (std::thread &t : team) t.join();
        if (ee != hipSuccess) return fail(ADH_ERR_HIP, std::string("scoring pipeline (copy-out): ") + hipGetErrorString(ee));
        return ADH_OK;
    }
};

// The compacted copy-out of the padded path (adh_slot_count_kernel, adh_pad_pack_kernel, fill_host_rows): the fragment
// tables of a chunk travel as one packed block, valid / features as they are.
// The host team expands landed blocks WHILE the later chunks are enqueued and scored - the enqueue loop waits for
// every chunk's pack kernel, so it lasts as long as the kernels, and a team started behind it (as the padded path's
// rebuild team is) had all blocks but none done at that point: 3 M candidates 25 - 30 ms, the team finishing 6 ms
// after the last copy.  The team takes the chunks as their copies complete (BlockHandoff; send() appends the events).
struct PackedCopyOut : PlainCopyOut {
    const PadLayout lay;
    const int T;
    const bool sparse;  // the sparse-slot wire (sparse_slots_pay): blocks are SparseBlocks, four totals per chunk
    // the smallest slot value that leaves no room for the flags (ADH_DEBUG_SPARSE_BIG_FROM, developer switch: a
    // smaller one, so that a test reaches the dense block of such a chunk)
    uint32_t big_from = kSlotFlagFrom;
    uint64_t wire_slots = 0, wire_nz_i = 0, wire_nz_c = 0;  // (the call's totals, for the ADH_DEBUG_TIMING line)
    unsigned char *dev_blocks = nullptr, *host_blocks = nullptr;
    // A chunk is handed out in tiles of kFillTile rows (on multiples of it: fill_host_rows works in aligned groups of 16
    // rows), claimed one by one.  With one fixed stripe per thread a chunk took as long as its slowest thread: of the 16
    // stripes of a 500 000-row block the quickest took 1.1 ms and the slowest 1.7 - 2.4 (team and enqueue thread are 17
    // on a quota of 16 cores), and the team was 0.5 - 1.2 ms behind the last copy (profiles/headline_pipeline.json,
    // `fixed_stripes`).
    static constexpr int64_t kFillTile = 2048;
    std::vector<std::atomic<int64_t>> next_tile;
    BlockHandoff handoff;
    HandoffTeam team{handoff};
    PackedCopyOut(const CopyOut &call, adh_output_t *out_)
        : PlainCopyOut(call, out_, true), lay(n, top_k, n_chunks), T(host_threads_for(n)), sparse(sparse_slots_pay(n)),
          next_tile((size_t)n_chunks), handoff(n_chunks, h->device) {}

    int prepare() override {
        int rc = PlainCopyOut::prepare();
        if (rc == ADH_OK) rc = grow_device(&h->cmp_dev, &h->cmp_dev_bytes, lay.total, lay.total / 8);
        if (rc == ADH_OK) rc = grow_pinned(&h->cmp_host, &h->cmp_host_bytes, lay.total, lay.total / 8);
        if (rc != ADH_OK) return rc;
        if (!h->cmp_tot_pinned) HIP_TRY(hipHostMalloc((void **)&h->cmp_tot_pinned, 4096 * 16, hipHostMallocDefault));
        if (sparse) {
            if (const char *env = getenv("ADH_DEBUG_SPARSE_BIG_FROM")) {  // (anything but a number in 1 .. 0x4000 is ignored)
                char *end = nullptr;
                const long v = strtol(env, &end, 0);
                if (end != env && *end == '\0' && v >= 1 && v <= (long)kSlotFlagFrom) big_from = (uint32_t)v;
            }
        }
        // a chunk's per-row counts and, behind them, its per-workgroup totals
        const size_t cnt_bytes = (size_t)(longest_chunk() + longest_chunk() / kPackRows + 1) * sizeof(SlotCnt);
        rc = grow_device(&h->cmp_cnt, &h->cmp_cnt_bytes, cnt_bytes, cnt_bytes / 8);
        if (rc != ADH_OK) return rc;
        dev_blocks = static_cast<unsigned char *>(h->cmp_dev), host_blocks = static_cast<unsigned char *>(h->cmp_host);
        for (std::atomic<int64_t> &next : next_tile) next.store(0, std::memory_order_relaxed);
        trace.expect_blocks(n_chunks, T);
        if (trace.events) handoff.landed = [this](int64_t ci) { trace.team_told(ci); };
        return ADH_OK;
    }
    void stripe(int64_t ci, int w) {  // (thread w's share of chunk ci; w only names it in the debug times)
        const int64_t a = cut[(size_t)ci], b = cut[(size_t)ci + 1];
        const double t_in = trace.stripe_begin();
        for (;;) {
            const int64_t t = a / kFillTile + next_tile[(size_t)ci].fetch_add(1, std::memory_order_relaxed);
            const int64_t lo = std::max(a, t * kFillTile), hi = std::min(b, (t + 1) * kFillTile);
            if (lo >= b) break;
            fill_host_rows(h->h_lib.data(), c, out, host_blocks + lay.base(a, ci), b - a, a, lo, hi, sparse);
        }
        trace.stripe_end(ci, w, t_in);
    }
    void start_team() override {
        (void)start_handoff_team(team, T, n_chunks, [this](int64_t ci, int w) { stripe(ci, w); });
    }
    // the rows' counts, then offsets and the packed block (adh_pack_count_kernel, adh_pack_rows_kernel): behind the
    // chunk's kernels, on the scoring stream.  (Measured and dropped: both launches on a stream of their own that waits
    // for the chunk's kernels, so that the next chunk's kernels follow directly.  They then run beside those kernels
    // and slow them: the scoring stream's span went from 14.3 - 15.4 ms to 16.2 - 16.7, and to 17.4 - 17.6 on a stream
    // of the highest priority - profiles/scoring_stream_chunks.json, `pack_stream`.)
    template <bool kSparseWire>
    void launch_pack(int64_t ci) {
        const int64_t a = cut[(size_t)ci], nr = cut[(size_t)ci + 1] - a;
        const dim3 grid((unsigned)((nr + kPackRows - 1) / kPackRows)), wg(kPackRows);
        SlotCnt *cnt = static_cast<SlotCnt *>(h->cmp_cnt), *wg_tot = cnt + longest_chunk();
        hipLaunchKernelGGL(adh_pack_count_kernel<kSparseWire>, grid, wg, 0, h->stream, dev.fragment_lib_slot,
                           reinterpret_cast<const uint32_t *>(dev.fragment_intensity),
                           reinterpret_cast<const uint32_t *>(dev.fragment_correlation), a, nr, top_k, big_from, cnt, wg_tot);
        hipLaunchKernelGGL(adh_pack_rows_kernel<kSparseWire>, grid, wg, 0, h->stream, dev, a, nr, top_k, cnt, wg_tot,
                           dev_blocks + lay.base(a, ci), h->cmp_tot_pinned + (kSparseWire ? 4 : 1) * ci);
    }
    int pack(int64_t ci) override {
        if (sparse) launch_pack<true>(ci);
        else launch_pack<false>(ci);
        HIP_TRY(hipGetLastError());
        return record(h->stream, tot_ready);  // (when the totals can be read)
    }
    // the packed block of chunk ci: wait for its pack kernel (an event on the scoring stream - the next chunk's kernels
    // are already queued; never a copy behind the copy-out backlog), ONE copy of its used bytes, then the event behind
    // it to the host team
    int send(int64_t ci) {
        const int64_t a = cut[(size_t)ci], b = cut[(size_t)ci + 1];
        HIP_TRY(hipEventSynchronize(tot_ready[(size_t)ci]));
        trace.total_seen(ci);
        const size_t base = lay.base(a, ci);
        size_t bytes = 0;
        if (sparse) {
            const uint32_t *tot = h->cmp_tot_pinned + 4 * ci;  // (format, slots, non-zero intensity / correlation words)
            bytes = SparseBlock((uint64_t)a, (uint64_t)(b - a), tot[1], tot[2], tot[3], tot[0] == kWireSparse).total;
            wire_slots += tot[1], wire_nz_i += tot[0] == kWireSparse ? tot[2] : tot[1], wire_nz_c += tot[0] == kWireSparse ? tot[3] : tot[1];
        } else {
            bytes = PadBlock((uint64_t)(b - a), (uint64_t)h->cmp_tot_pinned[ci]).total;
        }
        h->d2h_bytes += bytes;
        trace.block_sent(ci, bytes, PadBlock((uint64_t)(b - a), sparse ? h->cmp_tot_pinned[4 * ci + 1] : h->cmp_tot_pinned[ci]).total);
        return send_block(handoff, host_blocks + base, dev_blocks + base, bytes);
    }
    // The packed block of a chunk goes AHEAD of its valid / features rows (from chunk 1 on: the link is busy with chunk
    // ci - 1 when the kernels of chunk ci end, so that the host enqueues both only once it knows the block's length
    // costs nothing).  The team expands a block while the rows that need no work follow it on the link - with the rows
    // first, the blocks of the last three chunks landed within the last 1.4 ms of the copy-out and the team ended
    // 1.0 - 1.3 ms after the last copy (profiles/headline_pipeline.json, `before`, `handoff_ms`).  Chunk 0 keeps its
    // rows first: they leave the moment its kernels end.
    int copy_out(int64_t ci) override {
        if (ci == 0) {
            HIP_TRY(hipStreamWaitEvent(h->stream_out, h->ev_k[0], 0));
            return copy_tables(0, false);
        }
        int rc = send(ci - 1);  // (waits for the pack kernel of chunk ci - 1: its kernels are done)
        if (rc == ADH_OK && ci > 1) rc = copy_tables(ci - 1, false);
        return rc;
    }
    int flush() override { return copy_out(n_chunks); }  // (the last chunk's block and rows)
    int finish() override {
        // the blocks still on their way, then the team (it has been expanding since the first block landed)
        if (!handoff.wait_for(n_chunks - 1))
            return fail(ADH_ERR_HIP, std::string("scoring pipeline (compacted copy-out): ") + hipGetErrorString(handoff.error));
        for (int64_t ci = 0; ci < n_chunks; ++ci) stripe(ci, T);  // (this thread takes what is left)
        team.join_all();
        if (trace.timing)
            fprintf(stderr, "[adh]   compacted copy-out: host team done %.2f ms after the call began (%d threads)\n", trace.since(), T);
        if (trace.timing && sparse)
            fprintf(stderr, "[adh]   sparse-slot wire: %llu filled slots, %llu intensity words and %llu correlation words sent\n",
                    (unsigned long long)wire_slots, (unsigned long long)wire_nz_i, (unsigned long long)wire_nz_c);
        return ADH_OK;
    }
};

// The operator path (adh_score_candidates_compact; adh_cop_count_kernel, adh_cop_pack_kernel, cop_copy_stripe): valid
// rows and filled slots of a chunk travel as one dense block.
// Host threads unpack finished blocks into the caller's arrays WHILE the later chunks are enqueued and scored (the
// enqueue loop waits for every chunk's totals, so it takes as long as the kernels: with the team started behind it
// the unpacking - 2 ms per 450 000-row block - came on top: 32 ms per 3 M candidates).  The team takes the blocks
// as their copies complete (BlockHandoff; send() appends the events), thread w takes stripe w of T of every block.
struct OperatorCopyOut : CopyOut {
    adh_compact_output_t *const cop;
    const CopLayout lay;
    const int T;
    int started = 0;
    unsigned char *dev_blocks = nullptr, *stage = nullptr;
    // base[ci] / cnt[ci] are written once, by the watcher of chunk ci before it publishes the chunk, and never again:
    // a worker reads only its own chunk's pair (a chunk that does not fit - and every one behind it - is published
    // with a count of 0).
    std::vector<int64_t> base_r, base_s, cnt_r, cnt_s;
    bool overflow = false;
    BlockHandoff handoff;
    HandoffTeam team{handoff};
    OperatorCopyOut(const CopyOut &call, adh_compact_output_t *cop_)
        : CopyOut(call), cop(cop_), lay(n, top_k, n_chunks), T(host_threads_for(n)), base_r((size_t)n_chunks + 1, 0),
          base_s((size_t)n_chunks + 1, 0), cnt_r((size_t)n_chunks, 0), cnt_s((size_t)n_chunks, 0),
          handoff(n_chunks, h->device) {}

    // the caller's arrays are usually fresh allocations: ask for huge pages where the kernel gives them on request
    // (270 000 first-touch faults of 4 KiB pages per 3 M candidates otherwise, taken by the copying threads)
    void advise_huge_pages() const {
        auto advise = [](void *p, size_t bytes) {
            const uintptr_t lo = ((uintptr_t)p + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
            const uintptr_t hi = ((uintptr_t)p + bytes) & ~(uintptr_t)((2u << 20) - 1);
            if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
        };
        const size_t rc_ = (size_t)cop->rows_capacity, sc_ = (size_t)cop->slots_capacity;
        advise(cop->features, rc_ * ADH_NUM_FEATURES * 4);
        advise(cop->row, rc_ * 4), advise(cop->precursor_idx, rc_ * 4);
        void *const s4[] = {cop->fragment_row, cop->fragment_precursor_idx, cop->fragment_mz_library, cop->fragment_mz,
                            cop->fragment_mz_observed, cop->fragment_height, cop->fragment_intensity,
                            cop->fragment_mass_error, cop->fragment_correlation};
        for (void *p4 : s4) advise(p4, sc_ * 4);
        void *const s1[] = {cop->fragment_rank, cop->fragment_position, cop->fragment_number, cop->fragment_type,
                            cop->fragment_charge, cop->fragment_loss_type};
        for (void *p1 : s1) advise(p1, sc_);
    }
    // counts / offsets of every chunk (one uint64 per row + one per chunk), scan scratch, staging block
    int prepare() override {
        if (!compact_output_complete(cop)) return fail(ADH_ERR_INVALID_ARGUMENT, "compact output buffer is NULL");
        advise_huge_pages();
        const size_t cnt_bytes = (size_t)(n + n_chunks) * 8;
        int rc = grow_device(&h->cop_cnt, &h->cop_cnt_bytes, cnt_bytes, cnt_bytes / 8);
        if (rc == ADH_OK) rc = grow_scan_scratch<uint64_t>(&h->cop_scan, &h->cop_scan_bytes, longest_chunk() + 1, h->stream);
        if (rc == ADH_OK) rc = grow_pinned(&h->cop_stage, &h->cop_stage_bytes, lay.total, lay.total / 8);
        if (rc != ADH_OK) return rc;
        if (n_chunks > 4096) return fail(ADH_ERR_UNSUPPORTED, "compact output: more than 4096 chunks");
        if (!h->cop_tot_pinned) HIP_TRY(hipHostMalloc((void **)&h->cop_tot_pinned, 4096 * 8, hipHostMallocDefault));
        rc = grow_device(&h->cop_dev, &h->cop_dev_bytes, lay.total, lay.total / 8 + 4096);
        if (rc != ADH_OK) return rc;
        stage = static_cast<unsigned char *>(h->cop_stage), dev_blocks = static_cast<unsigned char *>(h->cop_dev);
        handoff.landed = [this](int64_t ci) {
            const uint64_t tot = h->cop_tot_pinned[ci];  // (valid rows << 32 | filled slots; final since the block's event)
            base_r[(size_t)ci + 1] = base_r[(size_t)ci] + (int64_t)(tot >> 32);
            base_s[(size_t)ci + 1] = base_s[(size_t)ci] + (int64_t)(tot & 0xFFFFFFFFull);
            if (base_r[(size_t)ci + 1] > cop->rows_capacity || base_s[(size_t)ci + 1] > cop->slots_capacity)
                overflow = true;
            // count on (the caller learns what it needs); an overflowing chunk and all behind it copy nothing
            cnt_r[(size_t)ci] = overflow ? 0 : (int64_t)(tot >> 32);
            cnt_s[(size_t)ci] = overflow ? 0 : (int64_t)(tot & 0xFFFFFFFFull);
            if (trace.timing)
                fprintf(stderr, "[adh]   compact chunk %lld: %lld rows, %lld slots on the host %.2f ms after the call began\n",
                        (long long)ci, (long long)(tot >> 32), (long long)(tot & 0xFFFFFFFFull), trace.since());
        };
        return ADH_OK;
    }
    void stripe(int64_t ci, int w) {
        if (cnt_r[(size_t)ci] == 0 && cnt_s[(size_t)ci] == 0) return;
        cop_copy_stripe(stage + lay.base(cut[(size_t)ci], ci), cnt_r[(size_t)ci], cnt_s[(size_t)ci], base_r[(size_t)ci],
                        base_s[(size_t)ci], cop, w, T, c, h->h_lib.data());
    }
    void start_team() override {
        started = start_handoff_team(team, T, n_chunks, [this](int64_t ci, int w) { stripe(ci, w); });
    }
    int pack(int64_t ci) override {
        const int64_t a = cut[(size_t)ci], nr = cut[(size_t)ci + 1] - a;
        hipStream_t sk = h->stream;
        uint64_t *off = static_cast<uint64_t *>(h->cop_cnt) + a + ci;
        hipLaunchKernelGGL(adh_cop_count_kernel, dim3((unsigned)((nr + 256) / 256)), dim3(256), 0, sk, dev.valid,
                           dev.fragment_lib_slot, a, nr, top_k, off);
        size_t scan_bytes = h->cop_scan_bytes;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->cop_scan, scan_bytes, off, off, (int)(nr + 1), sk));
        hipLaunchKernelGGL(adh_cop_pack_kernel, dim3((unsigned)std::min<int64_t>((nr * top_k + 255) / 256, 8192)), dim3(256), 0,
                           sk, dev, h->cs.d, h->d_lib, a, nr, top_k, off, dev_blocks + lay.base(a, ci), h->cop_tot_pinned + ci);
        HIP_TRY(hipGetLastError());
        return record(sk, tot_ready);  // (when the totals can be read)
    }
    // the block of chunk ci: wait for its totals (its kernels are done then), ONE copy of the used bytes
    int send(int64_t ci) {
        HIP_TRY(hipEventSynchronize(tot_ready[(size_t)ci]));
        const uint64_t tot = h->cop_tot_pinned[ci];
        const CopBlock L(tot >> 32, tot & 0xFFFFFFFFull);
        const size_t base = lay.base(cut[(size_t)ci], ci);
        h->d2h_bytes += L.total + 8;
        return send_block(handoff, stage + base, dev_blocks + base, L.total);
    }
    int copy_out(int64_t ci) override {  // the block of the previous chunk, now that the host can know its size
        return ci > 0 ? send(ci - 1) : ADH_OK;
    }
    int flush() override { return send(n_chunks - 1); }
    int finish() override {
        // the blocks still on their way, then the threads (they have been unpacking since the first block landed)
        // (the calling thread joins the watch: a team of no threads still gets every block published)
        if (!handoff.wait_for(n_chunks - 1))
            return fail(ADH_ERR_HIP, std::string("scoring pipeline (compact copy-out): ") + hipGetErrorString(handoff.error));
        team.join_all();
        for (int64_t ci = 0; ci < n_chunks; ++ci)  // (stripes of threads that could not be started)
            for (int w = started; w < T; ++w) stripe(ci, w);
        if (trace.timing)
            fprintf(stderr, "[adh]   compact: host team done %.2f ms after the call began (%d threads)\n", trace.since(), T);
        cop->n_rows = base_r[(size_t)n_chunks];
        cop->n_slots = base_s[(size_t)n_chunks];
        if (overflow) {
            (void)hipStreamSynchronize(h->stream);
            (void)hipStreamSynchronize(h->stream_out);
            tables_stand = true;
            return fail(ADH_ERR_INVALID_ARGUMENT, "compact output: rows_capacity / slots_capacity too small (n_rows / n_slots say what is needed)");
        }
        return ADH_OK;
    }
};

}  // namespace
