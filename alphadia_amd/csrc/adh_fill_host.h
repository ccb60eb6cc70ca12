// adh_fill_host.h - the packed fragment blocks of the padded path's compacted copy-out and the host code that expands
// them into the caller's padded tables (included by adh_copyout.hip; no handle and no device call in here, so that
// tools/probes/sparse_block_probe.hip can run fill_host_rows on hand-made blocks under the host sanitizers).
#pragma once
#include <immintrin.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "adh_device.h"

namespace {

// a chunk's block of R rows and S filled slots: [offsets u32 x (R + 1) | fragment_lib_slot u16 x S | mz_observed, height,
// intensity, mass_error, correlation f32 x S]; every column starts on a multiple of 16 bytes
struct PadBlock {
    size_t slot, f[5], total;
    __host__ __device__ PadBlock(uint64_t R, uint64_t S) {
        size_t o = ((R + 1) * 4 + 15) & ~(size_t)15;
        slot = o, o += (S * 2 + 15) & ~(size_t)15;
        for (int j = 0; j < 5; ++j) f[j] = o, o += (S * 4 + 15) & ~(size_t)15;
        total = o;
    }
};

// ---- the sparse-slot wire (ADH_SPARSE_SLOTS).  66.7 % of the fragment_intensity words and 80.6 % of the
// fragment_correlation words of filled slots are 0x00000000 (the 3 M-row headline table: profiles/sparse_slots.json,
// `table`), so these two columns travel as dense streams of
// their NON-ZERO words (any bit pattern but 0x00000000: -0.0 and NaN travel), in slot order.  Which slots have a word in
// a stream say the top two bits of the slot's u16 word (kHasIntensity, kHasCorrelation); where each stream stands at
// every row of the chunk whose number IN THE TABLE is a multiple of kAnchorRows say the anchors - the team's tiles start
// on such rows or at the chunk's first row, where both streams stand at 0, so that a tile is expanded without walking
// any flags in front of it (fill_host_rows walks them for any other start).  A block with a header:
//   [format, S, NI, NC u32 | offsets u32 x (R + 1) | anchors (u32, u32) x (multiples of kAnchorRows among the chunk's
//    rows) | slot u16 x S | mz_observed, height, mass_error f32 x S | intensity f32 x NI | correlation f32 x NC]
// every column on a multiple of 16 bytes.  A chunk that holds a slot value >= kSlotFlagFrom (a precursor with 16 384
// fragments and more) has no room for the flags: its block has format kWireDense - no anchors, no flags, all five float
// columns S long, in the same order.
constexpr uint32_t kWireDense = 0, kWireSparse = 1;
constexpr uint32_t kSlotFlagFrom = 0x4000, kHasIntensity = 0x8000, kHasCorrelation = 0x4000;
constexpr int64_t kAnchorRows = 64;  // (8 bytes per 64 rows; divides the team's tile of 2048 rows)
struct SparseBlock {
    size_t off, anchor, slot, f[5], total;  // (f[] in table order: f[2] / f[4] are the streams of a sparse block)
    // the first anchored row of a chunk that starts at row a0 of the table is anchor_row0(a0) * kAnchorRows
    __host__ __device__ static uint64_t anchor_row0(uint64_t a0) { return (a0 + kAnchorRows - 1) / kAnchorRows; }
    __host__ __device__ static uint64_t anchors(uint64_t a0, uint64_t R) {
        if (!R) return 0;
        const uint64_t first = anchor_row0(a0), behind = (a0 + R - 1) / kAnchorRows + 1;
        return behind > first ? behind - first : 0;
    }
    __host__ __device__ SparseBlock(uint64_t a0, uint64_t R, uint64_t S, uint64_t NI, uint64_t NC, bool sparse) {
        size_t o = 16;
        off = o, o += ((R + 1) * 4 + 15) & ~(size_t)15;
        anchor = o;
        if (sparse) o += (anchors(a0, R) * 8 + 15) & ~(size_t)15;
        slot = o, o += (S * 2 + 15) & ~(size_t)15;
        const int dense[3] = {0, 1, 3};
        for (int j = 0; j < 3; ++j) f[dense[j]] = o, o += (S * 4 + 15) & ~(size_t)15;
        f[2] = o, o += ((sparse ? NI : S) * 4 + 15) & ~(size_t)15;
        f[4] = o, o += ((sparse ? NC : S) * 4 + 15) & ~(size_t)15;
        total = o;
    }
};

// rows [lo, hi) of the chunk that starts at row a0 and has R rows, from its packed block (host copy; `headed`: a block
// of the sparse-slot wire, SparseBlock, else a PadBlock): ONE pass that writes every host column of a row -
// precursor_idx and rank, the five computed fragment columns and fragment_lib_slot (when the caller asked for it) from
// the block, the library / id columns of the row's K filled slots from the host copy of the library `lib` - with zeros
// behind the K filled slots.  Byte for byte what the copy of the padded tables plus rebuild_host_rows write (skipped
// rows have no filled slot: zeros everywhere).  The block is read up to 64 bytes behind its end.
void fill_host_rows(const LibRec *lib, const adh_candidates_t *c, adh_output_t *out, const unsigned char *blk, int64_t R,
                    int64_t a0, int64_t lo, int64_t hi, bool headed) {
    const int top_k = out->top_k;
    const uint32_t *head = reinterpret_cast<const uint32_t *>(blk);
    const bool sparse = headed && head[0] == kWireSparse;
    const uint32_t *off = reinterpret_cast<const uint32_t *>(blk);
    const uint16_t *src_s;
    const float *src[5];
    if (headed) {
        const SparseBlock L((uint64_t)a0, (uint64_t)R, head[1], head[2], head[3], sparse);
        off = reinterpret_cast<const uint32_t *>(blk + L.off);
        src_s = reinterpret_cast<const uint16_t *>(blk + L.slot);
        for (int j = 0; j < 5; ++j) src[j] = reinterpret_cast<const float *>(blk + L.f[j]);
    } else {
        const PadBlock L((uint64_t)R, (uint64_t)off[R]);
        src_s = reinterpret_cast<const uint16_t *>(blk + L.slot);
        for (int j = 0; j < 5; ++j) src[j] = reinterpret_cast<const float *>(blk + L.f[j]);
    }
    // where the two streams stand at row lo: at the last anchored row up to it (or 0 at the chunk's first row), plus the
    // flags of the rows between - none where lo is a tile boundary of the team
    size_t pi = 0, pc = 0;
    if (sparse && lo < hi) {
        int64_t from = a0;
        const int64_t g = lo / kAnchorRows;
        if (g * kAnchorRows >= a0) {
            const uint32_t *anchor = reinterpret_cast<const uint32_t *>(blk + SparseBlock((uint64_t)a0, (uint64_t)R, 0, 0, 0, true).anchor) +
                                     2 * (g - (int64_t)SparseBlock::anchor_row0((uint64_t)a0));
            pi = anchor[0], pc = anchor[1], from = g * kAnchorRows;
        }
        for (uint32_t s = off[from - a0]; s < off[lo - a0]; ++s) pi += src_s[s] >> 15, pc += (src_s[s] >> 14) & 1u;
    }
    const uint16_t slot_mask = sparse ? (uint16_t)(kSlotFlagFrom - 1) : (uint16_t)0xFFFF;
    const float *const si = src[2], *const sc = src[4];
    float *const dst[5] = {out->fragment_mz_observed, out->fragment_height, out->fragment_intensity, out->fragment_mass_error,
                           out->fragment_correlation};
    uint16_t *const slot_out = out->fragment_lib_slot;  // (NULL: the caller did not ask for the slots)
    uint8_t *const u8col[6] = {out->fragment_rank, out->fragment_position, out->fragment_number, out->fragment_type,
                               out->fragment_charge, out->fragment_loss_type};
    if (top_k == 12) {
        // the usual width (default.yaml:185), in tiles of 16 rows.  A tile's rows of every column are assembled in local
        // buffers first, then each column's part of the tile leaves as one run of streaming stores (768 bytes of a 4-byte
        // column, 192 of a byte column: whole cache lines, as tiles start on multiples of 16 rows) - one column after the
        // other.  (Storing a row's 14 columns side by side with streaming stores left the core's write-combining buffers
        // to be flushed half-filled: the host team took 2x as long as the copies it replaces.)  The packed source is
        // read unmasked (a column has slack behind its last entry, the buffer behind its last block) and cut to the
        // row's k entries with a mask.
        alignas(16) static const uint32_t kMask[13][12] = {
#define ADH_M(k) {k > 0 ? ~0u : 0u, k > 1 ? ~0u : 0u, k > 2 ? ~0u : 0u, k > 3 ? ~0u : 0u, k > 4 ? ~0u : 0u, k > 5 ? ~0u : 0u, \
                  k > 6 ? ~0u : 0u, k > 7 ? ~0u : 0u, k > 8 ? ~0u : 0u, k > 9 ? ~0u : 0u, k > 10 ? ~0u : 0u, k > 11 ? ~0u : 0u}
            ADH_M(0), ADH_M(1), ADH_M(2), ADH_M(3), ADH_M(4), ADH_M(5), ADH_M(6), ADH_M(7), ADH_M(8), ADH_M(9), ADH_M(10), ADH_M(11), ADH_M(12)
#undef ADH_M
        };
        constexpr int TR = 16;
        alignas(64) float tf[8][TR * 12];    // 5 computed columns, mz_library, mz, fragment_precursor_idx (as bits)
        alignas(64) uint8_t tb[6][TR * 12];  // fragment_rank, position, number, type, charge, loss_type
        alignas(64) uint16_t ts[TR * 12];
        alignas(64) uint32_t tp[TR];
        alignas(64) uint8_t tr[TR];
        float *const dstf[8] = {dst[0], dst[1], dst[2], dst[3], dst[4], out->fragment_mz_library, out->fragment_mz,
                                reinterpret_cast<float *>(out->fragment_precursor_idx)};
        auto put = [](void *d, const void *src_, size_t bytes, bool nt) {
            if (nt && (reinterpret_cast<uintptr_t>(d) & 15u) == 0 && bytes % 16 == 0) {
                for (size_t q = 0; q < bytes; q += 16)
                    _mm_stream_si128(reinterpret_cast<__m128i *>(static_cast<char *>(d) + q),
                                     _mm_load_si128(reinterpret_cast<const __m128i *>(static_cast<const char *>(src_) + q)));
            } else {
                memcpy(d, src_, bytes);
            }
        };
        for (int64_t t0 = lo; t0 < hi;) {
            const int64_t t1 = std::min<int64_t>(hi, (t0 / TR + 1) * TR);
            const int m = (int)(t1 - t0);
            const bool full = m == TR;
            memset(tf[5], 0, sizeof(tf[5]) * 2);
            memset(tb, 0, sizeof(tb));
            memset(ts, 0, sizeof(ts));
            if (sparse) memset(tf[2], 0, sizeof(tf[2])), memset(tf[4], 0, sizeof(tf[4]));  // (filled slot by slot)
            for (int q = 0; q < m; ++q) {
                const int64_t i = t0 + q;
                const bool skip = c->flags && (c->flags[i] & ADH_FLAG_SKIP);
                const uint32_t p = skip ? 0u : c->precursor_idx[i];
                const uint8_t r = skip ? (uint8_t)0 : c->rank[i];
                tp[q] = p;
                tr[q] = r;
                const uint32_t o = off[i - a0];
                const uint32_t k = std::min<uint32_t>(off[i - a0 + 1] - o, 12u);
                const __m128 m0 = _mm_load_ps(reinterpret_cast<const float *>(kMask[k]));
                const __m128 m1 = _mm_load_ps(reinterpret_cast<const float *>(kMask[k] + 4));
                const __m128 m2 = _mm_load_ps(reinterpret_cast<const float *>(kMask[k] + 8));
                for (int j = 0; j < 5; ++j) {
                    if (sparse && (j == 2 || j == 4)) continue;
                    const float *sp = src[j] + o;
                    float *row = tf[j] + q * 12;
                    _mm_store_ps(row, _mm_and_ps(_mm_loadu_ps(sp), m0));
                    _mm_store_ps(row + 4, _mm_and_ps(_mm_loadu_ps(sp + 4), m1));
                    _mm_store_ps(row + 8, _mm_and_ps(_mm_loadu_ps(sp + 8), m2));
                }
                const __m128 pv = _mm_castsi128_ps(_mm_set1_epi32((int)p));
                _mm_store_ps(tf[7] + q * 12, _mm_and_ps(pv, m0));
                _mm_store_ps(tf[7] + q * 12 + 4, _mm_and_ps(pv, m1));
                _mm_store_ps(tf[7] + q * 12 + 8, _mm_and_ps(pv, m2));
                // the library columns of the k filled slots (zeros behind: the buffers were cleared)
                const LibRec *base = lib + c->frag_start_idx[i];
                for (uint32_t u = 0; u < k; ++u) {
                    const int e = q * 12 + (int)u;
                    const uint16_t word = src_s[o + u];
                    const uint16_t sl = word & slot_mask;
                    if (sparse) {
                        // (the next word of a stream is read whether the slot has one or not: see the slack above)
                        const bool has_i = (word & kHasIntensity) != 0, has_c = (word & kHasCorrelation) != 0;
                        const float vi = si[pi], vc = sc[pc];
                        tf[2][e] = has_i ? vi : 0.0f;
                        tf[4][e] = has_c ? vc : 0.0f;
                        pi += has_i, pc += has_c;
                    }
                    const LibRec &l = base[sl - 1];
                    ts[e] = sl;
                    tf[5][e] = l.mz_library;
                    tf[6][e] = l.mz;
                    tb[0][e] = r;
                    tb[1][e] = l.position;
                    tb[2][e] = l.number;
                    tb[3][e] = l.type;
                    tb[4][e] = l.charge;
                    tb[5][e] = l.loss_type;
                }
            }
            const size_t r0 = (size_t)t0 * 12;
            for (int j = 0; j < 8; ++j) put(dstf[j] + r0, tf[j], (size_t)m * 48, full);
            for (int j = 0; j < 6; ++j) put(u8col[j] + r0, tb[j], (size_t)m * 12, full);
            if (slot_out) put(slot_out + r0, ts, (size_t)m * 24, full);
            put(out->precursor_idx + t0, tp, (size_t)m * 4, full);
            put(out->rank + t0, tr, (size_t)m, false);  // (16 bytes: a quarter of a line)
            t0 = t1;
        }
        _mm_sfence();
        return;
    }
    // any other width: plain loops
    for (int64_t i = lo; i < hi; ++i) {
        const bool skip = c->flags && (c->flags[i] & ADH_FLAG_SKIP);
        const uint32_t p = skip ? 0u : c->precursor_idx[i];
        const uint8_t r = skip ? (uint8_t)0 : c->rank[i];
        out->precursor_idx[i] = p;
        out->rank[i] = r;
        const uint32_t o = off[i - a0];
        const int k = (int)std::min<uint32_t>(off[i - a0 + 1] - o, (uint32_t)top_k);
        const size_t r0 = (size_t)i * (size_t)top_k;
        const LibRec *base = lib + c->frag_start_idx[i];
        int t = 0;
        for (; t < k; ++t) {
            const size_t d = r0 + (size_t)t;
            const uint16_t word = src_s[o + t];
            const uint16_t s = word & slot_mask;
            const LibRec &l = base[s - 1];
            if (sparse) {
                const bool has_i = (word & kHasIntensity) != 0, has_c = (word & kHasCorrelation) != 0;
                dst[0][d] = src[0][o + t], dst[1][d] = src[1][o + t], dst[3][d] = src[3][o + t];
                dst[2][d] = has_i ? si[pi] : 0.0f;
                dst[4][d] = has_c ? sc[pc] : 0.0f;
                pi += has_i, pc += has_c;
            } else {
                for (int j = 0; j < 5; ++j) dst[j][d] = src[j][o + t];
            }
            if (slot_out) slot_out[d] = s;
            out->fragment_precursor_idx[d] = p;
            out->fragment_rank[d] = r;
            out->fragment_mz_library[d] = l.mz_library;
            out->fragment_mz[d] = l.mz;
            out->fragment_position[d] = l.position;
            out->fragment_number[d] = l.number;
            out->fragment_type[d] = l.type;
            out->fragment_charge[d] = l.charge;
            out->fragment_loss_type[d] = l.loss_type;
        }
        const size_t rest = (size_t)(top_k - t);
        if (!rest) continue;
        const size_t d = r0 + (size_t)t;
        for (int j = 0; j < 5; ++j) memset(dst[j] + d, 0, rest * 4);
        if (slot_out) memset(slot_out + d, 0, rest * 2);
        memset(out->fragment_precursor_idx + d, 0, rest * 4);
        memset(out->fragment_mz_library + d, 0, rest * 4);
        memset(out->fragment_mz + d, 0, rest * 4);
        for (int j = 0; j < 6; ++j) memset(u8col[j] + d, 0, rest);
    }
}

}  // namespace
