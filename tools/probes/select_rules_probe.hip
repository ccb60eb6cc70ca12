// Host check of the rules of candidate selection's host code (alphadia_amd/csrc/adh_select_rules.h): the rank-1
// factors of a smoothing kernel and their two refusals, the two-row tap table, the refusal of cycles with more than 16
// rows per group, the scratch budget and the cutting of batches - the last against a plain restatement of "the longest
// prefix that fits".  Host code only, nothing is launched:
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined \
//       -o tools/probes/select_rules_probe tools/probes/select_rules_probe.hip && tools/probes/select_rules_probe
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../alphadia_amd/csrc/adh_select_rules.h"

namespace {

using selrules::Refusal;

int g_bad = 0;

void check(bool ok, const char *what) {
    if (!ok) printf("FAILED %s\n", what), ++g_bad;
}

bool fine(const Refusal &r) { return r.code == ADH_OK && r.msg == nullptr; }
bool refuses(const Refusal &r, int code, const char *words) { return r.code == code && r.msg && strstr(r.msg, words); }

// sel::Taps (adh_select.hip)
struct Taps {
    double v[2 * 16];
    int32_t col0, cols;
};

std::vector<float> gaussian(int k0, int k1) {
    std::vector<float> k((size_t)k0 * k1);
    for (int a = 0; a < k0; ++a)
        for (int b = 0; b < k1; ++b) {
            const double x = (a - k0 / 2) / 1.5, y = (b - k1 / 2) / 4.0;
            k[(size_t)a * k1 + b] = (float)(exp(-0.5 * x * x) * exp(-0.5 * y * y));
        }
    return k;
}

void rank1() {
    const int k0 = 6, k1 = 20;
    std::vector<float> k = gaussian(k0, k1);
    std::vector<double> ku, kv;
    check(fine(selrules::rank1_factors(k.data(), k0, k1, ku, kv)), "rank1: a Gaussian kernel is taken");
    bool ok = ku.size() == (size_t)k0 && kv.size() == (size_t)k1 && ku[k0 / 2] == 1.0;
    const double c = k[(size_t)(k0 / 2) * k1 + k1 / 2];
    for (int a = 0; a < k0 && ok; ++a)
        for (int b = 0; b < k1 && ok; ++b) ok = fabs(ku[(size_t)a] * kv[(size_t)b] - (double)k[(size_t)a * k1 + b]) <= 1e-5 * c;
    check(ok, "rank1: ku x kv is the kernel, ku = 1 at the centre row");
    std::vector<float> bent = k;
    bent[(size_t)(k0 / 2 + 1) * k1 + k1 / 2 + 1] *= 1.01f;
    check(refuses(selrules::rank1_factors(bent.data(), k0, k1, ku, kv), ADH_ERR_UNSUPPORTED, "not separable"),
          "rank1: one entry off by 1 % is refused");
    std::vector<float> hollow = k;
    hollow[(size_t)(k0 / 2) * k1 + k1 / 2] = 0.0f;
    check(refuses(selrules::rank1_factors(hollow.data(), k0, k1, ku, kv), ADH_ERR_UNSUPPORTED, "without a positive centre"),
          "rank1: a centre of 0 is refused");
}

// (k_rows, k1) with `count` unequal positive taps from column `first` on, the rest zero
std::vector<float> hand_kernel(int k_rows, int k1, int first, int count) {
    std::vector<float> k((size_t)k_rows * k1, 0.0f);
    for (int a = 0; a < k_rows; ++a)
        for (int b = 0; b < count; ++b) k[(size_t)a * k1 + first + b] = 0.05f + 0.01f * (float)(a * 31 + b * 7 % 13);
    return k;
}

void taps_case(const char *what, int k_rows, int k1, int first, int count, int exp_cols, int exp_col0) {
    const std::vector<float> k = hand_kernel(k_rows, k1, first, count);
    const Taps t = selrules::two_row_taps<Taps>(k.data(), k_rows, k1);
    bool ok = t.cols == exp_cols && (exp_cols == 0 || t.col0 == exp_col0);
    for (int a = 0; a < 2 && ok && exp_cols; ++a)
        for (int b = 0; b < 16 && ok; ++b) {
            const int col = exp_col0 + b;
            ok = t.v[a * 16 + b] == (b < count && col < k1 ? (double)k[(size_t)a * k1 + col] : 0.0);
        }
    check(ok, what);
}

void taps() {
    taps_case("taps: 16 columns from 0", 2, 30, 0, 16, 16, 0);
    taps_case("taps: 16 columns to the end", 2, 30, 14, 16, 16, 14);
    taps_case("taps: 13 columns of 31", 2, 31, 9, 13, 16, 9);
    taps_case("taps: 17 columns do not fit", 2, 30, 6, 17, 0, 0);
    taps_case("taps: an all-zero kernel", 2, 30, 0, 0, 16, 0);
    taps_case("taps: three rows", 3, 30, 0, 16, 0, 0);
    taps_case("taps: one row", 1, 30, 0, 16, 0, 0);
}

struct Cycle {
    std::vector<double> rows;  // (lower, upper)
    void add(double lo, double hi) { rows.push_back(lo), rows.push_back(hi); }
    int L() const { return (int)rows.size() / 2; }
};

Refusal cycle_rows(const Cycle &c, int n_ms1, const std::vector<float> &mz, const std::vector<uint8_t> &charge, int n_iso = 4) {
    return selrules::cycle_rows_refusal(c.rows.data(), c.L(), n_ms1, mz.data(), charge.data(), (int64_t)mz.size(), n_iso, 16);
}

void cycle() {
    const char *over = "isotope range overlaps more than 16 cycle rows";
    Cycle c16, c17;
    c16.add(-1, -1), c17.add(-1, -1);
    for (int r = 0; r < 16; ++r) c16.add(400, 500);
    for (int r = 0; r < 17; ++r) c17.add(400, 500);
    check(fine(cycle_rows(c16, 1, {450.0f}, {2})), "cycle: 16 overlapping rows and an MS1 row are taken");
    check(refuses(cycle_rows(c17, 1, {450.0f}, {2}), ADH_ERR_UNSUPPORTED, over), "cycle: 17 overlapping rows are refused");
    check(fine(cycle_rows(c17, 1, {900.0f, 450.0f, 399.0f}, {2, 0, 0})), "cycle: a precursor of charge 0 is skipped");
    check(fine(cycle_rows(c17, 1, {900.0f, 390.0f}, {2, 1})), "cycle: 17 overlapping rows that no precursor reaches are taken");
    check(fine(cycle_rows(c17, 1, {}, {})), "cycle: no precursors");
    Cycle ms1;
    for (int r = 0; r < 16; ++r) ms1.add(-1, -1);
    ms1.add(400, 500);
    check(fine(cycle_rows(ms1, 16, {450.0f}, {2})), "cycle: 16 MS1 rows (they do not count as overlapping an isotope range)");
    ms1.add(-1, -1);
    check(refuses(cycle_rows(ms1, 17, {450.0f}, {2}), ADH_ERR_UNSUPPORTED, "more than 16 cycle rows are MS1 rows"), "cycle: 17 MS1 rows");
    Cycle bad = c16;
    bad.add(500, 400);
    check(refuses(cycle_rows(bad, 1, {450.0f}, {2}), ADH_ERR_INVALID_ARGUMENT, "lower > upper"), "cycle: a row with lower > upper");
    // 17 narrow rows within 2.98 Th: the widest isotope range (charge 1, four isotopes: 3.02 Th) overlaps them all, so
    // the cycle fails the bound - a doubly charged precursor reaches nine of them, a singly charged one all
    Cycle narrow;
    narrow.add(-1, -1);
    for (int r = 0; r < 17; ++r) narrow.add(400 + 0.18 * r, 400 + 0.18 * r + 0.1);
    check(fine(cycle_rows(narrow, 1, {400.05f, 400.05f}, {2, 3})), "cycle: the bound fails and no precursor does");
    check(refuses(cycle_rows(narrow, 1, {400.05f, 400.05f}, {2, 1}), ADH_ERR_UNSUPPORTED, over), "cycle: ... and one that does");
    check(fine(cycle_rows(narrow, 1, {400.05f}, {1}, 1)), "cycle: ... with one isotope it reaches one row");
}

void budget() {
    const uint64_t MiB = (uint64_t)1 << 20, GiB = (uint64_t)1 << 30;
    check(selrules::selection_budget(100 * MiB, 5 * MiB, 0, nullptr) == 100 * MiB, "budget: what the call needs");
    check(selrules::selection_budget(20 * GiB, 5 * MiB, 0, nullptr) == 8 * GiB, "budget: 8 GiB by default");
    check(selrules::selection_budget(20 * GiB, 9 * GiB, 0, nullptr) == 9 * GiB, "budget: never below the largest block");
    check(selrules::selection_budget(100 * MiB, 5 * MiB, GiB, nullptr) == GiB, "budget: a larger slab at hand is used");
    uint64_t hand = MiB;
    check(selrules::selection_budget(100 * MiB, 5 * MiB, GiB, &hand) == 5 * MiB, "budget: by hand below the largest block, slab at hand ignored");
    hand = 10 * MiB;
    check(selrules::selection_budget(100 * MiB, 5 * MiB, GiB, &hand) == 10 * MiB, "budget: by hand wins over the slab at hand");
    hand = GiB;
    check(selrules::selection_budget(100 * MiB, 5 * MiB, 0, &hand) == 100 * MiB, "budget: by hand above what the call needs");
    hand = 0;
    check(selrules::selection_budget(100 * MiB, 5 * MiB, 0, &hand) == 5 * MiB, "budget: 0 by hand");
}

void batches() {
    std::mt19937_64 rng(7);
    bool ok = true, refused = true;
    for (int round = 0; round < 200 && ok; ++round) {
        const int64_t n = 1 + (int64_t)(rng() % 300);
        std::vector<unsigned long long> need((size_t)n), cum((size_t)n);
        unsigned long long sum = 0, biggest = 0;
        for (int64_t i = 0; i < n; ++i) {
            need[(size_t)i] = 256ull * (1 + rng() % (round % 3 == 0 ? 4 : 4000));
            biggest = std::max(biggest, need[(size_t)i]);
            cum[(size_t)i] = sum += need[(size_t)i];
        }
        const uint64_t budgets[] = {biggest, biggest + 256, biggest * 3, sum / 2 + biggest, sum - 1 > biggest ? sum - 1 : biggest, sum, sum + 1};
        for (const uint64_t budget : budgets) {
            // the rule restated: a batch takes precursors while they fit together
            std::vector<int64_t> exp{0};
            unsigned long long in_batch = 0;
            for (int64_t i = 0; i < n; ++i) {
                if (in_batch + need[(size_t)i] > budget) exp.push_back(i), in_batch = 0;
                in_batch += need[(size_t)i];
            }
            exp.push_back(n);
            std::vector<int64_t> first{77};
            ok = ok && fine(selrules::cut_batches(cum.data(), n, budget, first)) && first == exp;
        }
        std::vector<int64_t> first;
        refused = refused && refuses(selrules::cut_batches(cum.data(), n, biggest - 1, first), ADH_ERR_UNSUPPORTED,
                                     "one precursor's tiles exceed the selection scratch budget");
    }
    check(ok, "batches: the longest prefixes that fit, on random block sizes");
    check(refused, "batches: a budget below the largest block is refused");
}

}  // namespace

int main() {
    rank1();
    taps();
    cycle();
    budget();
    batches();
    printf(g_bad ? "FAILED: %d\n" : "all selection rules hold\n", g_bad);
    return g_bad ? 1 : 0;
}
