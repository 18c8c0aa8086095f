// select_batch_plan_check.cpp -- the plan of score_select_batch_plan.hpp against tables written by hand, stand-alone
// (tests/test_selection_batch_host.py builds it plain and with the host sanitizers and runs it as a child process; it is never
// loaded into Python and needs no GPU).  Cases: the candidate counts [37, 0, 9, 260, 1] with k = [12, 0, 9, 32, 1] of the
// tests' group A..E, the counts [0, 1, 32, 33, 260] whose tile tables are written out below, an all-empty group, every argument
// error with its message, and the 2^28 cap at its edge.  It exits non-zero on the first difference, and unless the cases reach
// every branch of the plan.
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "score_select_batch_plan.hpp"

using namespace score;

namespace {

int failures = 0;
// branches: [0] a member without candidates, [1] one with; [2] a single-tile member, [3] a member with a partly filled last
// tile, [4] an all-empty group; [5..] the errors, in the order of main
bool reached[5 + 12] = {};

void expect(bool ok, const char* what, long long a = -1, long long b = -1) {
    if (ok) return;
    std::fprintf(stderr, "%s (%lld, %lld)\n", what, a, b);
    ++failures;
}

std::vector<int32_t> prefix(const std::vector<int32_t>& counts) {
    std::vector<int32_t> ptr{0};
    for (int32_t c : counts) ptr.push_back(ptr.back() + c);
    return ptr;
}

std::vector<double> weights(size_t n) {
    std::vector<double> w(n);
    for (size_t c = 0; c < n; ++c) w[c] = 4.0 + (double)(c % 7);
    return w;
}

const std::string who = "score_refine_batch_select_ranges: ";

// the offsets by their definitions, the tile table entry by entry
void walk(const GbSelPlan& p, const std::vector<int32_t>& counts, const std::vector<int32_t>& k) {
    int64_t mat = 0, l = 0;
    int32_t pick = 0, wg = 0, n_active = 0;
    expect(p.G == (int)counts.size() && p.mat0.size() == counts.size() + 1 && p.l0.size() == counts.size() + 1 &&
               p.pick0.size() == counts.size() + 1 && p.wg0.size() == counts.size() + 1, "sizes");
    for (int g = 0; g < p.G; ++g) {
        const int32_t C = counts[(size_t)g];
        expect(p.count[(size_t)g] == C && p.k[(size_t)g] == k[(size_t)g], "count and k", g);
        expect(p.mat0[(size_t)g] == mat && p.l0[(size_t)g] == l && p.pick0[(size_t)g] == pick && p.wg0[(size_t)g] == wg, "offsets", g);
        const int T = (C + 31) / 32;
        expect(p.tiles(g) == T, "tiles", g, T);
        for (int i = 0; i < T; ++i)
            for (int j = i; j < T; ++j, ++wg) {
                const bool in = (size_t)wg < p.tile.size();
                expect(in && p.tile[(size_t)wg].member == g && p.tile[(size_t)wg].i == i && p.tile[(size_t)wg].j == j, "tile pair", g, wg);
            }
        if (C > 0) {
            expect((size_t)n_active < p.active.size() && p.active[(size_t)n_active] == g, "active member", g);
            ++n_active;
        }
        reached[C ? 1 : 0] = true;
        if (T == 1) reached[2] = true;
        if (C % 32 && T > 1) reached[3] = true;
        mat += (int64_t)C * C; l += (int64_t)C * k[(size_t)g]; pick += k[(size_t)g];
    }
    expect(p.mat0.back() == mat && p.entries == mat && p.l0.back() == l && p.l_entries == l && p.pick0.back() == pick && p.picks == pick,
           "totals");
    expect(p.wg0.back() == wg && (int32_t)p.tile.size() == wg && (int32_t)p.active.size() == n_active, "table sizes", wg, n_active);
}

int n_errors = 0;
void refuses(const char* words, const std::vector<int32_t>& counts, const double* w, const int32_t* k, double min_gain) {
    const int at = 5 + n_errors++;
    try {
        gbsel_plan(who, (int)counts.size(), prefix(counts), w, k, min_gain);
        expect(false, words);
    } catch (const std::runtime_error& e) {
        const bool ok = std::string(e.what()) == who + words;
        if (!ok) std::fprintf(stderr, "got: %s\n", e.what());
        expect(ok, words);
        reached[at] = ok;
    }
}

}  // namespace

int main() {
    {   // the tests' group A..E
        const std::vector<int32_t> counts{37, 0, 9, 260, 1}, k{12, 0, 9, 32, 1};
        const std::vector<double> w = weights(307);
        const GbSelPlan p = gbsel_plan(who, 5, prefix(counts), w.data(), k.data(), 0.0);
        walk(p, counts, k);
        expect(p.pairs == 307 && p.entries == 37 * 37 + 81 + 260 * 260 + 1 && p.l_entries == 37 * 12 + 81 + 260 * 32 + 1 && p.picks == 54, "A..E totals");
        expect(p.mat0 == std::vector<int64_t>({0, 1369, 1369, 1450, 69050, 69051}), "A..E mat0");
        expect(p.l0 == std::vector<int64_t>({0, 444, 444, 525, 8845, 8846}), "A..E l0");
        expect(p.pick0 == std::vector<int32_t>({0, 12, 12, 21, 53, 54}), "A..E pick0");
        expect(p.wg0 == std::vector<int32_t>({0, 3, 3, 4, 49, 50}), "A..E wg0");   // T = 2, 0, 1, 9, 1: 3, 0, 1, 45, 1 pairs
        expect(p.active == std::vector<int32_t>({0, 2, 3, 4}), "A..E active");
    }
    {   // members of 0, 1, 32, 33 and 260 candidates: the table written out
        const std::vector<int32_t> counts{0, 1, 32, 33, 260}, k{0, 1, 32, 5, 256};
        const std::vector<double> w = weights(326);
        const GbSelPlan p = gbsel_plan(who, 5, prefix(counts), w.data(), k.data(), 0.5);
        walk(p, counts, k);
        expect(p.wg0 == std::vector<int32_t>({0, 0, 1, 2, 5, 50}), "wg0");
        const int want[5][3] = {{1, 0, 0}, {2, 0, 0}, {3, 0, 0}, {3, 0, 1}, {3, 1, 1}};
        for (int b = 0; b < 5; ++b)
            expect(p.tile[(size_t)b].member == want[b][0] && p.tile[(size_t)b].i == want[b][1] && p.tile[(size_t)b].j == want[b][2], "table", b);
        // member 4, T = 9: row i starts after 9 + 8 + .. + (10 - i) pairs
        int at = 5;
        for (int i = 0; i < 9; ++i) {
            expect(p.tile[(size_t)at].member == 4 && p.tile[(size_t)at].i == i && p.tile[(size_t)at].j == i, "row start", i, at);
            expect(p.tile[(size_t)(at + 8 - i)].i == i && p.tile[(size_t)(at + 8 - i)].j == 8, "row end", i);
            at += 9 - i;
        }
        expect(at == 50 && p.tiles(4) == 9 && p.tiles(3) == 2 && p.tiles(2) == 1 && p.tiles(1) == 1 && p.tiles(0) == 0, "tiles a side");
        expect(p.active == std::vector<int32_t>({1, 2, 3, 4}), "active");
        expect(p.l0.back() == 1 + 32 * 32 + 33 * 5 + 260 * 256, "l0");
    }
    {   // nobody lists a pair: no k, no precisions needed
        const std::vector<int32_t> counts{0, 0, 0}, zeros{0, 0, 0};
        const GbSelPlan p = gbsel_plan(who, 3, prefix(counts), nullptr, nullptr, 0.0);
        walk(p, counts, zeros);
        expect(p.pairs == 0 && p.entries == 0 && p.tile.empty() && p.active.empty(), "an empty group");
        const GbSelPlan q = gbsel_plan(who, 3, prefix(counts), nullptr, zeros.data(), 0.0);
        expect(q.picks == 0, "an empty group with k");
        reached[4] = true;
    }
    {   // every argument error
        const std::vector<int32_t> counts{3, 0, 2};
        const std::vector<double> w = weights(5);
        const std::vector<int32_t> k{2, 0, 2};
        refuses("no members", {}, w.data(), k.data(), 0.0);
        refuses("min_gain must be >= 0", counts, w.data(), k.data(), -1e-300);
        refuses("min_gain must be >= 0", counts, w.data(), k.data(), std::nan(""));
        refuses("k is missing", counts, w.data(), nullptr, 0.0);
        refuses("the precisions are missing", counts, nullptr, k.data(), 0.0);
        const std::vector<int32_t> k_zero{2, 0, 0}, k_many{4, 0, 2}, k_empty{2, 1, 2};
        refuses("member 2: k must be 1..min(candidates, 256)", counts, w.data(), k_zero.data(), 0.0);
        refuses("member 0: k must be 1..min(candidates, 256)", counts, w.data(), k_many.data(), 0.0);
        refuses("member 1: k must be 0 for a member without candidates", counts, w.data(), k_empty.data(), 0.0);
        std::vector<double> bad = w;
        bad[3] = 0.0;
        refuses("member 2: a precision must be finite and positive", counts, bad.data(), k.data(), 0.0);
        bad[3] = 4.0; bad[1] = std::numeric_limits<double>::infinity();
        refuses("member 0: a precision must be finite and positive", counts, bad.data(), k.data(), 0.0);
        const std::vector<double> many = weights(4097 + 300);
        const std::vector<int32_t> k_big{1, 257};
        refuses("member 0: the number of candidates must be at most 4096", {4097, 300}, many.data(), k_big.data(), 0.0);
        const std::vector<int32_t> k_257{257, 1};
        refuses("member 0: k must be 1..min(candidates, 256)", {300, 4097}, many.data(), k_257.data(), 0.0);
    }
    {   // the cap: 16 members of 4096 candidates are 2^28 entries exactly; one candidate more is refused with the figure
        std::vector<int32_t> counts(16, 4096), k(16, 1);
        std::vector<double> w = weights(16 * 4096 + 1);
        const GbSelPlan p = gbsel_plan(who, 16, prefix(counts), w.data(), k.data(), 0.0);
        expect(p.entries == ((int64_t)1 << 28) && p.tile.size() == (size_t)16 * 128 * 129 / 2, "the cap's edge");
        counts.push_back(1); k.push_back(1);
        try {
            gbsel_plan(who, 17, prefix(counts), w.data(), k.data(), 0.0);
            expect(false, "the cap");
        } catch (const std::runtime_error& e) {
            expect(std::string(e.what()) == who + "the members' matrices take 268435457 entries: at most 268435456 (2^28, 2 GiB) in one call", "the cap's message");
        }
    }
    expect(n_errors == 12, "errors", n_errors);
    for (size_t b = 0; b < sizeof reached / sizeof reached[0]; ++b)
        if (!reached[b]) {
            std::fprintf(stderr, "branch %zu was not reached\n", b);
            ++failures;
        }
    if (failures) return 1;
    std::printf("every branch reached\n");
    return 0;
}
