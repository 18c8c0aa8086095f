// leverage_batch_plan_check.cpp -- the plan of score_leverage_batch_plan.hpp against tables written by hand, stand-alone
// (tests/test_leverage_batch_host.py builds it with the host sanitizers and runs it as a child process; it is never loaded
// into Python and needs no GPU).  Cases: the draw counts [17, 5, 0, 16, 1] at width 4 with the pair counts [5, 0, 0, 260, 1]
// (a member without draws lists none), the pair counts [5, 0, 3, 260, 1] of the range variances at widths 4 and 16, an
// all-empty list, no list at all, every argument error.  It checks where the members' sums and pairs start, the member, pass
// and slot of every listed pair, the live slots and NV of every pair pass; it exits non-zero on the first difference, and
// unless the cases reach every branch of the plan.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "score_leverage_batch_plan.hpp"

using namespace score;

namespace {

int failures = 0;
// branches of the plan: [0] a member that takes part, [1] one that does not; [2] no list at all, [3] an empty member list,
// [4] a member with pairs; [5] a pair pass a member has dropped out of, [6] a partly filled one, [7] a full one; [8] a slot
// without a pair, [9] a slot with one; [10..19] the errors, in the order of `errors` in main
bool reached[20] = {};

void expect(bool ok, const char* what, int a = -1, int b = -1, int c = -1) {
    if (ok) return;
    std::fprintf(stderr, "%s (%d, %d, %d)\n", what, a, b, c);
    ++failures;
}

template <class T>
bool same(const std::vector<T>& got, std::initializer_list<T> want) { return got == std::vector<T>(want); }

// the five members of the tests: variables, measurements (those of A..E)
const std::vector<GblShape> kShapes = {{40, 306}, {20, 119}, {9, 27}, {60, 461}, {30, 113}};
const int32_t kDraws[5] = {17, 5, 0, 16, 1};

// pair c of a member with `vars` variables: two different ids in range
void fill(std::vector<int32_t>& a, std::vector<int32_t>& b, int count, int vars) {
    for (int c = 0; c < count; ++c) {
        a.push_back(c % vars);
        b.push_back((c + 1) % vars);
    }
}

struct Lists {
    std::vector<int32_t> ptr{0}, a, b;
    explicit Lists(std::initializer_list<int> counts) {
        int g = 0;
        for (int c : counts) {
            fill(a, b, c, (int)kShapes[(size_t)g++].vars);
            ptr.push_back((int32_t)a.size());
        }
    }
};

// live[k][g] and nv[k] by hand; every (member, slot, pass) and every pair against them
void walk(const GblPlan& p, const std::vector<int>& counts, int passes, const std::vector<std::vector<int>>& live, const std::vector<int>& nv) {
    expect(p.passes == passes && (int)live.size() == passes && (int)nv.size() == passes, "passes", p.passes, passes);
    int64_t total = 0;
    for (int g = 0; g < p.G; ++g) {
        expect(p.count(g) == counts[(size_t)g], "pairs of a member", g, p.count(g));
        expect(p.pair_ptr[(size_t)g] == total, "pair_ptr", g);
        for (int c = 0; c < counts[(size_t)g]; ++c) {
            const int64_t pair = total + c;
            expect(p.pair_member[(size_t)pair] == g, "member of a pair", g, c);
            expect(p.pass_of(pair) == c / p.W && p.slot_of(pair) == c % p.W, "pass and slot of a pair", g, c);
            expect(p.pair_at(g, p.slot_of(pair), p.pass_of(pair)) == pair, "the pair of its pass and slot", g, c);
        }
        total += counts[(size_t)g];
        reached[counts[(size_t)g] ? 4 : 3] = true;
    }
    expect(p.pairs == total && (int64_t)p.pair_member.size() == total && p.pair_ptr.back() == total, "all pairs");
    for (int k = 0; k < passes && k < p.passes; ++k) {
        expect(p.nv(k) == nv[(size_t)k], "NV of a pass", k, p.nv(k), nv[(size_t)k]);
        for (int g = 0; g < p.G; ++g) {
            const int want = live[(size_t)k][(size_t)g];
            expect(p.live(g, k) == want, "live slots", g, k, p.live(g, k));
            reached[want == 0 ? 5 : want < p.W ? 6 : 7] = true;
            expect(want <= p.nv(k), "NV holds the live slots", g, k);
            for (int c = -1; c <= kGbsMaxWidth; ++c) {
                const bool on = c >= 0 && c < want;
                expect(p.pair_at(g, c, k) == (on ? (int64_t)p.pair_ptr[(size_t)g] + k * p.W + c : -1), "pair of a slot", g, c, k);
                reached[on ? 9 : 8] = true;
            }
        }
    }
    // every pair of every member is carried exactly once
    std::vector<int> seen((size_t)total, 0);
    for (int g = 0; g < p.G; ++g)
        for (int k = 0; k < p.passes; ++k)
            for (int c = 0; c < p.W; ++c)
                if (p.pair_at(g, c, k) >= 0) ++seen[(size_t)p.pair_at(g, c, k)];
    for (int s : seen) expect(s == 1, "a pair is carried once");
}

struct Bad {
    const char* words;  // of the message
    int G; int width; const int32_t* draws; const int32_t* ptr; const int32_t* a; const int32_t* b;
};

}  // namespace

int main() {
    // the leverage: draws [17, 5, 0, 16, 1] at width 4; member 2 takes no part, has room on the device and none in the outputs
    {
        const Lists l({5, 0, 0, 260, 1});
        const GblPlan p = gbl_plan("check: ", 5, 4, kDraws, kShapes, l.ptr.data(), l.a.data(), l.b.data());
        expect(p.G == 5 && p.W == 4 && p.meas == 1026 && p.most == 260 && p.pairs == 266, "members, measurements, pairs");
        expect(same<int64_t>(p.meas0, {0, 306, 425, 452, 913}), "meas0");
        expect(same<int64_t>(p.meas_off, {0, 306, 425, 425, 886, 999}), "meas_off");
        expect(same<int32_t>(p.pair_ptr, {0, 5, 5, 5, 265, 266}), "pair_ptr");
        std::vector<std::vector<int>> live;
        for (int k = 0; k < 65; ++k) live.push_back({k == 0 ? 4 : k == 1 ? 1 : 0, 0, 0, 4, k == 0 ? 1 : 0});
        walk(p, {5, 0, 0, 260, 1}, 65, live, std::vector<int>(65, 4));
        reached[0] = reached[1] = true;  // (meas_off above: members 0, 1, 3, 4 take part, member 2 does not)
    }
    // the range variances: pair counts [5, 0, 3, 260, 1], everyone takes part; the first 256 pairs end inside member 3's list
    for (int width : {4, 16}) {
        const Lists l({5, 0, 3, 260, 1});
        const GblPlan p = gbl_plan("check: ", 5, width, nullptr, kShapes, l.ptr.data(), l.a.data(), l.b.data());
        expect(same<int64_t>(p.meas_off, {0, 306, 425, 452, 913, 1026}), "meas_off with everyone");
        expect(same<int32_t>(p.pair_ptr, {0, 5, 5, 8, 268, 269}) && p.pairs == 269, "pair_ptr");
        expect(p.pair_member[255] == 3 && p.pair_member[4] == 0 && p.pair_member[5] == 2 && p.pair_member[8] == 3 && p.pair_member[268] == 4,
               "the members of the first workgroup's pairs");
        std::vector<std::vector<int>> live;
        std::vector<int> nv;
        if (width == 4) {
            for (int k = 0; k < 65; ++k) live.push_back({k == 0 ? 4 : k == 1 ? 1 : 0, 0, k == 0 ? 3 : 0, 4, k == 0 ? 1 : 0});
            nv.assign(65, 4);
        } else {
            for (int k = 0; k < 17; ++k) live.push_back({k == 0 ? 5 : 0, 0, k == 0 ? 3 : 0, k < 16 ? 16 : 4, k == 0 ? 1 : 0});
            nv.assign(17, 16);
            nv[16] = 4;
        }
        walk(p, {5, 0, 3, 260, 1}, width == 4 ? 65 : 17, live, nv);
    }
    // an all-empty list and no list at all: no pairs, no passes
    {
        const int32_t zeros[6] = {0, 0, 0, 0, 0, 0};
        GblPlan p = gbl_plan("check: ", 5, 16, nullptr, kShapes, zeros, nullptr, nullptr);
        walk(p, {0, 0, 0, 0, 0}, 0, {}, {});
        expect(p.pairs == 0 && p.most == 0 && p.passes == 0, "an all-empty list");
        p = gbl_plan("check: ", 5, 16, kDraws, kShapes, nullptr, nullptr, nullptr);
        walk(p, {0, 0, 0, 0, 0}, 0, {}, {});
        expect(p.pairs == 0 && p.passes == 0 && same<int32_t>(p.pair_ptr, {0, 0, 0, 0, 0, 0}), "no list at all");
        expect(same<int64_t>(p.meas_off, {0, 306, 425, 425, 886, 999}), "meas_off without lists");
        reached[2] = true;
    }
    // every argument error, by its words
    {
        const int32_t ptr[6] = {0, 1, 1, 2, 3, 4}, late[6] = {1, 1, 1, 2, 3, 4}, back[6] = {0, 2, 1, 2, 3, 4};
        const int32_t a[4] = {0, 1, 2, 3}, b[4] = {1, 2, 3, 4}, self[4] = {0, 2, 2, 3}, high[4] = {1, 2, 60, 4}, low[4] = {-1, 1, 2, 3};
        const int32_t all_draw[5] = {1, 1, 1, 1, 1};
        const Bad errors[] = {
            {"no members", 0, 16, all_draw, ptr, a, b},
            {"block_width", 5, 0, all_draw, ptr, a, b},
            {"block_width", 5, 17, all_draw, ptr, a, b},
            {"must start at 0", 5, 16, all_draw, late, a, b},
            {"must not decrease", 5, 16, all_draw, back, a, b},
            {"pairs without their lists", 5, 16, all_draw, ptr, a, nullptr},
            {"member 2: pairs listed for a member without draws", 5, 16, kDraws, ptr, a, b},
            {"member 2: a pair joins a variable to itself", 5, 16, all_draw, ptr, self, b},
            {"member 3: a pair's variable is out of range", 5, 16, all_draw, ptr, a, high},
            {"member 0: a pair's variable is out of range", 5, 16, nullptr, ptr, low, b},
        };
        int e = 0;
        for (const Bad& bad : errors) {
            try {
                (void)gbl_plan("check: ", bad.G, bad.width, bad.draws, kShapes, bad.ptr, bad.a, bad.b);
                expect(false, "no error", e);
            } catch (const std::runtime_error& err) {
                const bool ok = std::strstr(err.what(), bad.words) != nullptr && std::strncmp(err.what(), "check: ", 7) == 0;
                expect(ok, err.what(), e);
                if (ok) reached[10 + e] = true;
            }
            ++e;
        }
        // ... and the same lists are a plan where nothing is wrong with them
        const GblPlan p = gbl_plan("check: ", 5, 16, all_draw, kShapes, ptr, a, b);
        walk(p, {1, 0, 1, 1, 1}, 1, {{1, 0, 1, 1, 1}}, {1});
    }
    for (int e = 0; e < 20; ++e)
        if (!reached[e]) { std::fprintf(stderr, "branch %d of the plan was not reached\n", e); ++failures; }
    if (failures) return 1;
    std::printf("every branch reached\n");
    return 0;
}
