// Probe / host check of the packed fragment blocks of the compacted copy-out (alphadia_amd/csrc/adh_fill_host.h): builds
// blocks by a plain restatement of the wire formats - the dense block (PadBlock), the sparse-slot block, the dense block with
// a header that a chunk with a slot value >= 0x4000 falls back to - expands them with the product's fill_host_rows and
// compares every column with padded tables written directly.  Host code only, nothing is launched:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -o tools/probes/sparse_block_probe tools/probes/sparse_block_probe.hip && tools/probes/sparse_block_probe
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "../../alphadia_amd/csrc/adh_fill_host.h"

namespace {

struct Tables {
    int64_t n;
    int top_k;
    std::vector<uint32_t> precursor_idx, fragment_precursor_idx;
    std::vector<uint8_t> rank, b[6];  // fragment_rank, position, number, type, charge, loss_type
    std::vector<float> f[7];          // mz_library, mz, mz_observed, height, intensity, mass_error, correlation
    std::vector<uint16_t> slot;
    Tables(int64_t n_, int top_k_, uint8_t fill) : n(n_), top_k(top_k_) {
        const size_t s = (size_t)n * (size_t)top_k;
        uint32_t w;
        memset(&w, fill, 4);
        float fw;
        memcpy(&fw, &w, 4);
        precursor_idx.assign((size_t)n, w), fragment_precursor_idx.assign(s, w), rank.assign((size_t)n, fill);
        for (auto &v : b) v.assign(s, fill);
        for (auto &v : f) v.assign(s, fw);
        slot.assign(s, (uint16_t)w);
    }
    adh_output_t view(bool with_slot) {
        adh_output_t o{};
        o.n = n, o.top_k = top_k;
        o.precursor_idx = precursor_idx.data(), o.rank = rank.data();
        o.fragment_precursor_idx = fragment_precursor_idx.data();
        o.fragment_rank = b[0].data(), o.fragment_position = b[1].data(), o.fragment_number = b[2].data();
        o.fragment_type = b[3].data(), o.fragment_charge = b[4].data(), o.fragment_loss_type = b[5].data();
        o.fragment_mz_library = f[0].data(), o.fragment_mz = f[1].data(), o.fragment_mz_observed = f[2].data();
        o.fragment_height = f[3].data(), o.fragment_intensity = f[4].data(), o.fragment_mass_error = f[5].data();
        o.fragment_correlation = f[6].data();
        o.fragment_lib_slot = with_slot ? slot.data() : nullptr;
        return o;
    }
};

template <typename V>
bool same_rows(const V &a, const V &b, int64_t row0, int64_t rows, size_t per_row) {
    return memcmp(a.data() + (size_t)row0 * per_row, b.data() + (size_t)row0 * per_row,
                  (size_t)rows * per_row * sizeof(a[0])) == 0;
}

float from_bits(uint32_t w) {
    float v;
    memcpy(&v, &w, 4);
    return v;
}
uint32_t bits_of(float v) {
    uint32_t w;
    memcpy(&w, &v, 4);
    return w;
}
size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

enum Fill { kAllZero, kAllSet, kMixed };
enum Wire { kDense, kSparse };

struct Case {
    const char *name;
    int64_t a0, R;  // the chunk is rows [a0, a0 + R) of the tables
    int top_k;
    Fill fill;
    int fixed_k;    // -1: random per row, else every row has this many filled slots
    bool big_slot;  // one slot value >= 0x4000 in the chunk
    Wire wire;
};

int run(const Case &cs, uint32_t seed) {
    std::mt19937 rng(seed);
    const int64_t n = cs.a0 + cs.R + 5;  // (rows behind the chunk: must stay untouched)
    const int top_k = cs.top_k;
    // library: a slice of top_k + 3 records per row, and one of 0x4100 records for the row with the big slot value
    const uint32_t per = (uint32_t)top_k + 3, big_len = 0x4100;
    std::vector<LibRec> lib((size_t)n * per + big_len);
    for (size_t i = 0; i < lib.size(); ++i) {
        LibRec &l = lib[i];
        memset(&l, 0, sizeof(l));
        l.mz_library = 200.f + (float)(i % 977), l.mz = l.mz_library + 0.25f;
        l.type = (uint8_t)(98 + (i & 1) * 23), l.charge = (uint8_t)(1 + i % 3), l.number = (uint8_t)(i % 29);
        l.position = (uint8_t)(i % 7), l.loss_type = (uint8_t)(i % 5);
    }
    std::vector<uint32_t> pidx((size_t)n), frag_start((size_t)n);
    std::vector<uint8_t> rank((size_t)n), flags((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        pidx[(size_t)i] = 7u + (uint32_t)i * 3u, rank[(size_t)i] = (uint8_t)(i % 3), frag_start[(size_t)i] = (uint32_t)i * per;
        if (i % 13 == 5) flags[(size_t)i] = ADH_FLAG_SKIP;
    }
    const int64_t big_row = cs.big_slot ? cs.a0 + cs.R / 2 : -1;
    if (big_row >= 0) frag_start[(size_t)big_row] = (uint32_t)n * per, flags[(size_t)big_row] = 0;
    adh_candidates_t c{};
    c.n = n, c.precursor_idx = pidx.data(), c.rank = rank.data(), c.flags = flags.data(), c.frag_start_idx = frag_start.data();

    // the chunk's device tables, restated: per row k filled leading slots
    std::vector<int> k_of((size_t)cs.R);
    std::vector<uint16_t> d_slot((size_t)cs.R * top_k, 0);
    std::vector<float> d_f[5];  // mz_observed, height, intensity, mass_error, correlation
    for (auto &v : d_f) v.assign((size_t)cs.R * top_k, 0.0f);
    const uint32_t odd[4] = {0x80000000u /* -0.0f */, 0x7FC00001u /* a NaN */, 0x00000001u, 0xFFC12345u /* a negative NaN */};
    // the first two words of either stream are -0.0 and a NaN (the other stream: the NaN first), later ones now and then
    size_t odd_i = 0, odd_c = 3, placed_i = 0, placed_c = 0;
    int minus_zero[2] = {0, 0}, nans[2] = {0, 0};  // placed per stream
    for (int64_t r = 0; r < cs.R; ++r) {
        const int64_t i = cs.a0 + r;
        int k = cs.fixed_k >= 0 ? cs.fixed_k : (int)(rng() % (uint32_t)(top_k + 1));
        if (cs.fixed_k < 0 && rng() % 7 == 0) k = rng() % 2 ? 0 : top_k;
        if (flags[(size_t)i] & ADH_FLAG_SKIP) k = 0;  // (skipped rows have no filled slot)
        if (i == big_row) k = std::max(k, 1);
        k_of[(size_t)r] = k;
        for (int j = 0; j < k; ++j) {
            const size_t e = (size_t)r * top_k + (size_t)j;
            d_slot[e] = (uint16_t)(1 + rng() % per);
            if (i == big_row && j == 0) d_slot[e] = (uint16_t)(0x4000 + rng() % 0x100);
            d_f[0][e] = 300.f + (float)(rng() % 100000) / 64.f;
            d_f[1][e] = 1.f + (float)(rng() % 5000);
            d_f[3][e] = rng() % 50 == 0 ? 0.0f : ((float)(rng() % 4001) - 2000.f) / 100.f;
            auto value = [&](size_t &next_odd, size_t &placed, int stream) {
                if (cs.fill == kAllZero) return 0.0f;
                if (cs.fill == kMixed && placed >= 2 && rng() % 3 != 0) return 0.0f;
                if (placed++ < 2 || rng() % 5 == 0) {
                    const uint32_t w = odd[next_odd++ % 4];
                    minus_zero[stream] += w == 0x80000000u, nans[stream] += (w & 0x7FC00000u) == 0x7FC00000u;
                    return from_bits(w);
                }
                return (float)(rng() % 100000) / 7.f + 1.f;
            };
            d_f[2][e] = value(odd_i, placed_i, 0);
            d_f[4][e] = value(odd_c, placed_c, 1);
        }
    }

    // expected: the padded tables written directly
    Tables exp(n, top_k, 0xA5), got(n, top_k, 0xA5);
    for (int64_t r = 0; r < cs.R; ++r) {
        const int64_t i = cs.a0 + r;
        const bool skip = (flags[(size_t)i] & ADH_FLAG_SKIP) != 0;
        exp.precursor_idx[(size_t)i] = skip ? 0u : pidx[(size_t)i];
        exp.rank[(size_t)i] = skip ? (uint8_t)0 : rank[(size_t)i];
        for (int j = 0; j < top_k; ++j) {
            const size_t e = (size_t)r * top_k + (size_t)j, d = (size_t)i * top_k + (size_t)j;
            const uint16_t s = d_slot[e];
            const LibRec zero{};
            const LibRec &l = s ? lib[frag_start[(size_t)i] + s - 1] : zero;
            exp.slot[d] = s;
            exp.fragment_precursor_idx[d] = s ? exp.precursor_idx[(size_t)i] : 0u;
            exp.b[0][d] = s ? exp.rank[(size_t)i] : (uint8_t)0;
            exp.b[1][d] = s ? l.position : (uint8_t)0, exp.b[2][d] = s ? l.number : (uint8_t)0;
            exp.b[3][d] = s ? l.type : (uint8_t)0, exp.b[4][d] = s ? l.charge : (uint8_t)0, exp.b[5][d] = s ? l.loss_type : (uint8_t)0;
            exp.f[0][d] = s ? l.mz_library : 0.0f, exp.f[1][d] = s ? l.mz : 0.0f;
            for (int q = 0; q < 5; ++q) exp.f[2 + q][d] = s ? d_f[q][e] : 0.0f;
        }
    }

    // the block, by the format's description
    uint64_t S = 0, NI = 0, NC = 0;
    bool big = false;
    for (int64_t r = 0; r < cs.R; ++r)
        for (int j = 0; j < k_of[(size_t)r]; ++j) {
            const size_t e = (size_t)r * top_k + (size_t)j;
            ++S, NI += bits_of(d_f[2][e]) != 0, NC += bits_of(d_f[4][e]) != 0, big |= d_slot[e] >= 0x4000;
        }
    // the values the format must carry bit for bit are really in both streams
    if (cs.fill != kAllZero && S >= 2 && !(minus_zero[0] && minus_zero[1] && nans[0] && nans[1]))
        return printf("%s: a stream without a -0.0 or without a NaN\n", cs.name), 1;
    const bool headed = cs.wire == kSparse, sparse = headed && !big;
    // anchors: one for every row of the chunk whose number in the table is a multiple of 64
    uint64_t strides = 0;
    for (int64_t r = 0; r < cs.R; ++r) strides += (cs.a0 + r) % 64 == 0;
    const int64_t first_anchor = (cs.a0 + 63) / 64;
    size_t o = headed ? 16 : 0;
    const size_t at_off = o;
    o += a16((size_t)(cs.R + 1) * 4);
    const size_t at_anchor = o;
    if (sparse) o += a16(strides * 8);
    const size_t at_slot = o;
    o += a16(S * 2);
    size_t at_f[5];
    if (headed) {
        at_f[0] = o, o += a16(S * 4), at_f[1] = o, o += a16(S * 4), at_f[3] = o, o += a16(S * 4);
        at_f[2] = o, o += a16((sparse ? NI : S) * 4), at_f[4] = o, o += a16((sparse ? NC : S) * 4);
    } else {
        for (int q = 0; q < 5; ++q) at_f[q] = o, o += a16(S * 4);
    }
    const size_t total = o;
    if (headed && total != SparseBlock((uint64_t)cs.a0, (uint64_t)cs.R, S, NI, NC, sparse).total) return printf("%s: SparseBlock total\n", cs.name), 1;
    if (!headed && total != PadBlock((uint64_t)cs.R, S).total) return printf("%s: PadBlock total\n", cs.name), 1;
    std::vector<unsigned char> blk(total + 64, 0xEE);  // (the 64 bytes of slack the expansion may read)
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t *>(blk.data() + at); };
    if (headed) u32(0)[0] = sparse ? 1u : 0u, u32(0)[1] = (uint32_t)S, u32(0)[2] = (uint32_t)NI, u32(0)[3] = (uint32_t)NC;
    {
        uint32_t s = 0, pi = 0, pc = 0;
        for (int64_t r = 0; r < cs.R; ++r) {
            u32(at_off)[r] = s;
            if (sparse && (cs.a0 + r) % 64 == 0) {
                const int64_t g = (cs.a0 + r) / 64 - first_anchor;
                u32(at_anchor)[2 * g] = pi, u32(at_anchor)[2 * g + 1] = pc;
            }
            for (int j = 0; j < k_of[(size_t)r]; ++j, ++s) {
                const size_t e = (size_t)r * top_k + (size_t)j;
                const uint32_t wi = bits_of(d_f[2][e]), wc = bits_of(d_f[4][e]);
                uint16_t word = d_slot[e];
                if (sparse) word |= (wi ? 0x8000u : 0u) | (wc ? 0x4000u : 0u);
                reinterpret_cast<uint16_t *>(blk.data() + at_slot)[s] = word;
                u32(at_f[0])[s] = bits_of(d_f[0][e]), u32(at_f[1])[s] = bits_of(d_f[1][e]), u32(at_f[3])[s] = bits_of(d_f[3][e]);
                if (!sparse) u32(at_f[2])[s] = wi, u32(at_f[4])[s] = wc;
                if (sparse && wi) u32(at_f[2])[pi++] = wi;
                if (sparse && wc) u32(at_f[4])[pc++] = wc;
            }
        }
        u32(at_off)[cs.R] = s;
        if (sparse && (pi != NI || pc != NC)) return printf("%s: stream lengths\n", cs.name), 1;
    }

    // expansion: the team's tiles of 2048 rows (on multiples of it), then tiles of 48 rows (starts that are no anchored
    // rows: the flags in front are walked), with and without a slot table
    int bad = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t tile = pass == 0 ? 2048 : 48;
        got = Tables(n, top_k, 0xA5);
        adh_output_t out = got.view(pass == 0);
        for (int64_t t = cs.a0 / tile; t * tile < cs.a0 + cs.R; ++t) {
            const int64_t lo = std::max(cs.a0, t * tile), hi = std::min(cs.a0 + cs.R, (t + 1) * tile);
            fill_host_rows(lib.data(), &c, &out, blk.data(), cs.R, cs.a0, lo, hi, headed);
        }
        // every column over ALL rows: the rows around the chunk keep their garbage in both
        const size_t K = (size_t)top_k;
        bool ok = same_rows(got.precursor_idx, exp.precursor_idx, 0, n, 1) && same_rows(got.rank, exp.rank, 0, n, 1) &&
                  same_rows(got.fragment_precursor_idx, exp.fragment_precursor_idx, 0, n, K);
        for (int q = 0; q < 6; ++q) ok = ok && same_rows(got.b[q], exp.b[q], 0, n, K);
        for (int q = 0; q < 7; ++q) ok = ok && same_rows(got.f[q], exp.f[q], 0, n, K);
        if (pass == 0) ok = ok && same_rows(got.slot, exp.slot, 0, n, K);
        if (!ok) printf("%s (tiles of %lld rows): tables differ\n", cs.name, (long long)tile), ++bad;
    }
    if (!bad)
        printf("ok   %-44s R %6lld  S %7llu  NI %7llu  NC %7llu  %s, %zu bytes\n", cs.name, (long long)cs.R, (unsigned long long)S,
               (unsigned long long)NI, (unsigned long long)NC, !headed ? "dense" : sparse ? "sparse" : "dense, headed", total);
    return bad;
}

}  // namespace

int main() {
    const Case cases[] = {
        {"streams empty", 0, 500, 12, kAllZero, -1, false, kSparse},
        {"every flag set", 0, 500, 12, kAllSet, -1, false, kSparse},
        {"every row K = 0", 32, 100, 12, kMixed, 0, false, kSparse},
        {"every row K = top_k", 32, 100, 12, kMixed, 12, false, kSparse},
        {"every row K = top_k, every flag set", 0, 4100, 12, kAllSet, 12, false, kSparse},
        {"R = 1", 0, 1, 12, kMixed, 3, false, kSparse},
        {"R = 1 behind row 37", 37, 1, 12, kMixed, 12, false, kSparse},
        {"R = 63 (one below the anchor stride)", 0, 63, 12, kMixed, -1, false, kSparse},
        {"R = 64 (the anchor stride)", 0, 64, 12, kMixed, -1, false, kSparse},
        {"R = 65 (one above the anchor stride)", 0, 65, 12, kMixed, -1, false, kSparse},
        {"R = 63 behind row 1 (no anchored row)", 1, 63, 12, kMixed, -1, false, kSparse},
        {"R = 64 behind row 1 (one anchored row, the last)", 1, 64, 12, kMixed, -1, false, kSparse},
        {"last tile of 7 rows", 0, 2048 + 64 + 7, 12, kMixed, -1, false, kSparse},
        {"chunk at row 1777, 1777 rows", 1777, 1777, 12, kMixed, -1, false, kSparse},
        {"chunk at row 1500, 3000 rows", 1500, 3000, 12, kMixed, -1, false, kSparse},
        {"width 17", 1500, 300, 17, kMixed, -1, false, kSparse},
        {"width 17, every flag set", 5, 129, 17, kAllSet, -1, false, kSparse},
        {"width 5, streams empty", 5, 129, 5, kAllZero, -1, false, kSparse},
        {"slot value >= 0x4000 (falls back)", 100, 300, 12, kMixed, -1, true, kSparse},
        {"slot value >= 0x4000, width 17", 100, 300, 17, kMixed, -1, true, kSparse},
        {"the dense block", 1777, 1777, 12, kMixed, -1, false, kDense},
        {"the dense block, slot value >= 0x4000", 3, 77, 12, kMixed, -1, true, kDense},
        {"the dense block, width 17", 3, 77, 17, kMixed, -1, false, kDense},
    };
    int bad = 0;
    uint32_t seed = 1;
    for (const Case &cs : cases) bad += run(cs, seed++);
    printf(bad ? "FAILED: %d\n" : "all blocks expand to the padded tables\n", bad);
    return bad ? 1 : 0;
}
