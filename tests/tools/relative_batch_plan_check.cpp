// relative_batch_plan_check.cpp -- the plan of score_relative_batch_plan.hpp against tables written by hand, stand-alone
// (tests/test_relative_batch_host.py builds it plain and with the host sanitizers and runs it as a child process; it is never
// loaded into Python and needs no GPU).  Cases, for DP = 3 and DP = 6: the pair counts [6, 0, 1, 11, 2] of the tests' group
// A..E at widths 16, 5 and 1 -- a member without pairs, members that drop out mid-way, pairs that straddle two passes --, an
// all-empty list, no list at all, every argument error.  It checks the column offsets, the member of every listed pair, the
// live slots and NV of every pass, the pair and error coordinate of every (member, slot, pass); it exits non-zero on the first
// difference, and unless the cases reach every branch of the plan.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "score_relative_batch_plan.hpp"

using namespace score;

namespace {

int failures = 0;
// branches of the plan: [0] no list at all, [1] an empty member list, [2] a member with pairs; [3] a pass a member has dropped
// out of, [4] a partly filled one, [5] a full one; [6] a slot without a column, [7] a slot with one; [8] a pair whose columns
// straddle two passes; [9..18] the errors, in the order of `errors` in main
bool reached[19] = {};

void expect(bool ok, const char* what, int a = -1, int b = -1, int c = -1) {
    if (ok) return;
    std::fprintf(stderr, "%s (%d, %d, %d)\n", what, a, b, c);
    ++failures;
}

template <class T>
bool same(const std::vector<T>& got, std::initializer_list<T> want) { return got == std::vector<T>(want); }

// the poses of the five members of the tests (those of A..E)
const std::vector<int64_t> kPoses = {40, 20, 9, 60, 30};

struct Lists {
    std::vector<int32_t> ptr{0}, a, b;
    explicit Lists(std::initializer_list<int> counts) {
        int g = 0;
        for (int n : counts) {
            const int np = (int)kPoses[(size_t)g++];
            for (int c = 0; c < n; ++c) {  // two different pose ids in range, pose 0 among them
                a.push_back(c % np);
                b.push_back((c + 1) % np);
            }
            ptr.push_back((int32_t)a.size());
        }
    }
};

// live[k][g] and nv[k] by hand; every (member, slot, pass) and every column against them
void walk(const GrpPlan& p, const std::vector<int>& counts, int passes, const std::vector<std::vector<int>>& live, const std::vector<int>& nv) {
    expect(p.passes == passes && (int)live.size() == passes && (int)nv.size() == passes, "passes", p.passes, passes);
    int64_t total = 0;
    for (int g = 0; g < p.G; ++g) {
        expect(p.count(g) == (int64_t)p.DP * counts[(size_t)g], "columns of a member", g, (int)p.count(g));
        expect(p.pair_ptr[(size_t)g] == total && p.col_ptr[(size_t)g] == p.DP * total, "pair_ptr and col_ptr", g);
        for (int c = 0; c < counts[(size_t)g]; ++c) {
            expect(p.pair_member[(size_t)(total + c)] == g, "member of a pair", g, c);
            for (int q = 0; q < p.DP; ++q) {  // local column c DP + q: pass and slot by division, and back
                const int j = c * p.DP + q;
                const GrpColumn col = p.column_at(g, j % p.W, j / p.W);
                expect(col.pair == total + c && col.q == q, "the pair and coordinate of a column's pass and slot", g, c, q);
            }
            if ((c * p.DP) / p.W != (c * p.DP + p.DP - 1) / p.W) reached[8] = true;
        }
        total += counts[(size_t)g];
        reached[counts[(size_t)g] ? 2 : 1] = true;
    }
    expect(p.pairs == total && (int64_t)p.pair_member.size() == total && p.pair_ptr.back() == total && p.columns == p.DP * total &&
           p.col_ptr.back() == p.DP * total, "all pairs and columns");
    for (int k = 0; k < passes && k < p.passes; ++k) {
        expect(p.nv(k) == nv[(size_t)k], "NV of a pass", k, p.nv(k), nv[(size_t)k]);
        for (int g = 0; g < p.G; ++g) {
            const int want = live[(size_t)k][(size_t)g];
            expect(p.live(g, k) == want, "live slots", g, k, p.live(g, k));
            reached[want == 0 ? 3 : want < p.W ? 4 : 5] = true;
            expect(want <= p.nv(k), "NV holds the live slots", g, k);
            for (int s = -1; s <= kGbsMaxWidth; ++s) {
                const bool on = s >= 0 && s < want;
                const GrpColumn col = p.column_at(g, s, k);
                const int64_t j = (int64_t)p.col_ptr[(size_t)g] + (int64_t)k * p.W + s;
                expect(on ? (col.pair == j / p.DP && col.q == (int)(j % p.DP)) : col.pair == -1, "column of a slot", g, s, k);
                reached[on ? 7 : 6] = true;
            }
        }
    }
    // every column of every member is carried exactly once
    std::vector<int> seen((size_t)(p.DP * total), 0);
    for (int g = 0; g < p.G; ++g)
        for (int k = 0; k < p.passes; ++k)
            for (int s = 0; s < p.W; ++s) {
                const GrpColumn col = p.column_at(g, s, k);
                if (col.pair >= 0) ++seen[(size_t)(col.pair * p.DP + col.q)];
            }
    for (int s : seen) expect(s == 1, "a column is carried once");
}

struct Spot { int g, s, k; int64_t pair; int q; };
void spots(const GrpPlan& p, std::initializer_list<Spot> want) {
    for (const Spot& w : want) {
        const GrpColumn col = p.column_at(w.g, w.s, w.k);
        expect(col.pair == w.pair && col.q == w.q, "a column written by hand", w.g, w.s, w.k);
    }
}

struct Bad {
    const char* words;  // of the message
    int G; int width; const int32_t* ptr; const int32_t* a; const int32_t* b;
};

}  // namespace

int main() {
    const std::vector<int> counts = {6, 0, 1, 11, 2};
    const Lists l({6, 0, 1, 11, 2});
    // DP = 3: columns 18, 0, 3, 33, 6
    {
        GrpPlan p = grp_plan("check: ", 5, 3, 16, kPoses, l.ptr.data(), l.a.data(), l.b.data());
        expect(same<int32_t>(p.pair_ptr, {0, 6, 6, 7, 18, 20}) && same<int32_t>(p.col_ptr, {0, 18, 18, 21, 54, 60}), "offsets, DP 3");
        expect(p.pairs == 20 && p.columns == 60 && p.most == 33 && p.W == 16 && p.G == 5 && p.DP == 3, "totals, DP 3");
        expect(same<int32_t>(p.pair_member, {0, 0, 0, 0, 0, 0, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4}), "pair_member");
        walk(p, counts, 3, {{16, 0, 3, 16, 6}, {2, 0, 0, 16, 0}, {0, 0, 0, 1, 0}}, {16, 16, 1});
        // A's pair 5 is its columns 15..17, D's pair 5 (pair 12 of the group) its 15..17, D's pair 10 (17) its 30..32
        spots(p, {{0, 15, 0, 5, 0}, {0, 0, 1, 5, 1}, {0, 1, 1, 5, 2}, {0, 2, 1, -1, 0}, {3, 15, 0, 12, 0}, {3, 0, 1, 12, 1}, {3, 1, 1, 12, 2},
                  {3, 14, 1, 17, 0}, {3, 15, 1, 17, 1}, {3, 0, 2, 17, 2}, {3, 1, 2, -1, 0}, {2, 0, 0, 6, 0}, {2, 2, 0, 6, 2}, {2, 3, 0, -1, 0},
                  {4, 5, 0, 19, 2}, {4, 6, 0, -1, 0}, {1, 0, 0, -1, 0}, {0, 0, 0, 0, 0}, {0, 3, 0, 1, 0}});
        p = grp_plan("check: ", 5, 3, 5, kPoses, l.ptr.data(), l.a.data(), l.b.data());
        walk(p, counts, 7, {{5, 0, 3, 5, 5}, {5, 0, 0, 5, 1}, {5, 0, 0, 5, 0}, {3, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 3, 0}},
             {8, 8, 8, 8, 8, 8, 4});
        // width 5: A's pair 1 is its columns 3..5 and straddles passes 0 and 1; E's column 5 is alone in pass 1
        spots(p, {{0, 3, 0, 1, 0}, {0, 4, 0, 1, 1}, {0, 0, 1, 1, 2}, {4, 0, 1, 19, 2}, {4, 1, 1, -1, 0}, {3, 2, 6, 17, 2}, {3, 3, 6, -1, 0}});
        p = grp_plan("check: ", 5, 3, 1, kPoses, l.ptr.data(), l.a.data(), l.b.data());
        std::vector<std::vector<int>> live;
        for (int k = 0; k < 33; ++k) live.push_back({k < 18 ? 1 : 0, 0, k < 3 ? 1 : 0, 1, k < 6 ? 1 : 0});
        walk(p, counts, 33, live, std::vector<int>(33, 1));
        spots(p, {{0, 0, 17, 5, 2}, {0, 0, 18, -1, 0}, {3, 0, 32, 17, 2}, {3, 0, 4, 8, 1}});
    }
    // DP = 6: columns 36, 0, 6, 66, 12
    {
        GrpPlan p = grp_plan("check: ", 5, 6, 16, kPoses, l.ptr.data(), l.a.data(), l.b.data());
        expect(same<int32_t>(p.pair_ptr, {0, 6, 6, 7, 18, 20}) && same<int32_t>(p.col_ptr, {0, 36, 36, 42, 108, 120}), "offsets, DP 6");
        expect(p.pairs == 20 && p.columns == 120 && p.most == 66, "totals, DP 6");
        walk(p, counts, 5, {{16, 0, 6, 16, 12}, {16, 0, 0, 16, 0}, {4, 0, 0, 16, 0}, {0, 0, 0, 16, 0}, {0, 0, 0, 2, 0}}, {16, 16, 16, 16, 2});
        // A's pair 2 is its columns 12..17 and straddles passes 0 and 1; D's last pair (17) its 60..65: passes 3 and 4
        spots(p, {{0, 12, 0, 2, 0}, {0, 15, 0, 2, 3}, {0, 0, 1, 2, 4}, {0, 1, 1, 2, 5}, {0, 2, 1, 3, 0}, {3, 12, 3, 17, 0}, {3, 15, 3, 17, 3},
                  {3, 0, 4, 17, 4}, {3, 1, 4, 17, 5}, {3, 2, 4, -1, 0}, {4, 11, 0, 19, 5}, {4, 12, 0, -1, 0}});
        p = grp_plan("check: ", 5, 6, 5, kPoses, l.ptr.data(), l.a.data(), l.b.data());
        walk(p, counts, 14,
             {{5, 0, 5, 5, 5}, {5, 0, 1, 5, 5}, {5, 0, 0, 5, 2}, {5, 0, 0, 5, 0}, {5, 0, 0, 5, 0}, {5, 0, 0, 5, 0}, {5, 0, 0, 5, 0},
              {1, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 5, 0}, {0, 0, 0, 1, 0}},
             {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1});
        spots(p, {{2, 0, 1, 6, 5}, {2, 1, 1, -1, 0}, {0, 0, 7, 5, 5}, {3, 0, 13, 17, 5}});
        p = grp_plan("check: ", 5, 6, 1, kPoses, l.ptr.data(), l.a.data(), l.b.data());
        std::vector<std::vector<int>> live;
        for (int k = 0; k < 66; ++k) live.push_back({k < 36 ? 1 : 0, 0, k < 6 ? 1 : 0, 1, k < 12 ? 1 : 0});
        walk(p, counts, 66, live, std::vector<int>(66, 1));
    }
    // an all-empty list and no list at all: no pairs, no passes
    for (int dp : {3, 6}) {
        const int32_t zeros[6] = {0, 0, 0, 0, 0, 0};
        GrpPlan p = grp_plan("check: ", 5, dp, 16, kPoses, zeros, nullptr, nullptr);
        walk(p, {0, 0, 0, 0, 0}, 0, {}, {});
        expect(p.pairs == 0 && p.columns == 0 && p.most == 0 && p.passes == 0, "an all-empty list");
        p = grp_plan("check: ", 5, dp, 16, kPoses, nullptr, nullptr, nullptr);
        walk(p, {0, 0, 0, 0, 0}, 0, {}, {});
        expect(p.pairs == 0 && p.passes == 0 && same<int32_t>(p.col_ptr, {0, 0, 0, 0, 0, 0}), "no list at all");
        reached[0] = true;
    }
    // every argument error, by its words
    {
        const int32_t ptr[6] = {0, 1, 1, 2, 3, 4}, late[6] = {1, 1, 1, 2, 3, 4}, back[6] = {0, 2, 1, 2, 3, 4};
        const int32_t many[6] = {0, 1, 1, 2, 3, 59652324};  // (36 times the total is 17 past INT32_MAX)
        const int32_t a[4] = {0, 1, 2, 3}, b[4] = {1, 2, 3, 0}, self[4] = {0, 2, 2, 3}, landmark[4] = {1, 2, 60, 4}, low[4] = {-1, 1, 2, 3};
        const Bad errors[] = {
            {"no members", 0, 16, ptr, a, b},
            {"block_width", 5, 0, ptr, a, b},
            {"block_width", 5, 17, ptr, a, b},
            {"must start at 0", 5, 16, late, a, b},
            {"must not decrease", 5, 16, back, a, b},
            {"too many pairs for one call", 5, 16, many, a, b},
            {"pairs without their lists", 5, 16, ptr, a, nullptr},
            {"member 2: a pair joins a pose to itself", 5, 16, ptr, self, b},
            {"member 3: a pair's pose is out of range (a landmark has no relative pose)", 5, 16, ptr, a, landmark},
            {"member 0: a pair's pose is out of range", 5, 16, ptr, low, b},
        };
        int e = 0;
        for (const Bad& bad : errors) {
            try {
                (void)grp_plan("check: ", bad.G, 3, bad.width, kPoses, bad.ptr, bad.a, bad.b);
                expect(false, "no error", e);
            } catch (const std::runtime_error& err) {
                const bool ok = std::strstr(err.what(), bad.words) != nullptr && std::strncmp(err.what(), "check: ", 7) == 0;
                expect(ok, err.what(), e);
                if (ok) reached[9 + e] = true;
            }
            ++e;
        }
        // ... and the same lists are a plan where nothing is wrong with them (pose 0 as a and as b)
        const GrpPlan p = grp_plan("check: ", 5, 3, 16, kPoses, ptr, a, b);
        walk(p, {1, 0, 1, 1, 1}, 1, {{3, 0, 3, 3, 3}}, {4});
    }
    for (int e = 0; e < 19; ++e)
        if (!reached[e]) { std::fprintf(stderr, "branch %d of the plan was not reached\n", e); ++failures; }
    if (failures) return 1;
    std::printf("every branch reached\n");
    return 0;
}
