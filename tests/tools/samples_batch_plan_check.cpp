// samples_batch_plan_check.cpp -- the plan of score_samples_batch_plan.hpp against tables written by hand, stand-alone
// (tests/test_samples_batch_host.py builds it with the host sanitizers and runs it as a child process; it is never loaded
// into Python and needs no GPU).  Cases: the counts [17, 5, 0, 16, 1] at widths 1, 4 and 16, single members, every argument
// error.  It checks the output offsets, the passes, NV per pass and the draw of every (member, slot, pass); it exits
// non-zero on the first difference, and unless the cases reach every branch of the plan.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "score_samples_batch_plan.hpp"

using namespace score;

namespace {

int failures = 0;
// branches of the plan: [0..4] gbs_slots gives 1, 2, 4, 8, 16; [5] a member that has dropped out, [6] a partly filled pass,
// [7] a full pass; [8] a slot without a draw, [9] a slot with one; [10..21] the errors, in the order of `errors` in main
bool reached[22] = {};

void expect(bool ok, const char* what, int a = -1, int b = -1, int c = -1) {
    if (ok) return;
    std::fprintf(stderr, "%s (%d, %d, %d)\n", what, a, b, c);
    ++failures;
}

template <class T>
bool same(const std::vector<T>& got, std::initializer_list<T> want) { return got == std::vector<T>(want); }

// the five members of the tests: unknowns, noise rows, packed moments, selected unknowns
const std::vector<GbsShape> kShapes = {{10, 6, 30, 3}, {4, 2, 8, 0}, {7, 9, 21, 2}, {3, 4, 9, 3}, {5, 1, 25, 1}};
const int32_t kCounts[5] = {17, 5, 0, 16, 1};
const uint64_t kSeeds[5] = {1, 2, 3, 4, 5};
const int32_t kVarPtr[6] = {0, 1, 1, 2, 3, 4};

// live[k][g] and nv[k] by hand; every (member, slot, pass) against them
void walk(const GbsPlan& p, int passes, const std::vector<std::vector<int>>& live, const std::vector<int>& nv, int64_t first) {
    expect(p.passes == passes && (int)live.size() == passes && (int)nv.size() == passes, "passes", p.passes, passes);
    for (int k = 0; k < passes && k < p.passes; ++k) {
        expect(p.nv(k) == nv[(size_t)k], "NV of a pass", k, p.nv(k), nv[(size_t)k]);
        const int slots = p.nv(k);
        reached[slots == 1 ? 0 : slots == 2 ? 1 : slots == 4 ? 2 : slots == 8 ? 3 : 4] = true;
        for (int g = 0; g < p.G; ++g) {
            const int want = live[(size_t)k][(size_t)g];
            expect(p.live(g, k) == want, "live slots", g, k, p.live(g, k));
            if (want == 0) reached[5] = true;
            else if (want < p.W) reached[6] = true;
            else reached[7] = true;
            expect(want <= slots, "NV holds the live slots", g, k);
            for (int c = -1; c <= kGbsMaxWidth; ++c) {
                const bool on = c >= 0 && c < want;
                expect(p.local_draw(g, c, k) == (on ? k * p.W + c : -1), "member-local draw", g, c, k);
                expect(p.draw(g, c, k) == (on ? first + (int64_t)k * p.W + c : -1), "draw index", g, c, k);
                reached[on ? 9 : 8] = true;
            }
        }
    }
    // every draw of every member is carried exactly once
    for (int g = 0; g < p.G; ++g) {
        std::vector<int> seen((size_t)p.count[(size_t)g], 0);
        for (int k = 0; k < p.passes; ++k)
            for (int c = 0; c < p.W; ++c)
                if (p.local_draw(g, c, k) >= 0) ++seen[(size_t)p.local_draw(g, c, k)];
        for (int s : seen) expect(s == 1, "a draw is carried once", g);
    }
}

void offsets_of_the_five(const GbsPlan& p) {
    expect(p.G == 5 && p.most == 17 && p.samples == 39, "members, most, samples");
    expect(same<int32_t>(p.count, {17, 5, 0, 16, 1}), "count");
    expect(same<int32_t>(p.cnt_ptr, {0, 17, 22, 22, 38, 39}), "cnt_ptr");
    expect(same<int32_t>(p.probe_ptr, {0, 1, 2, 2, 3, 4}), "probe_ptr");
    expect(same<int64_t>(p.draw_off, {0, 17, 22, 22, 38, 39}), "draw_off");
    expect(same<int64_t>(p.moments_off, {0, 30, 38, 38, 47, 72}), "moments_off");   // (member 2 takes no room)
    expect(same<int64_t>(p.means_off, {0, 10, 14, 14, 17, 22}), "means_off");
    expect(same<int64_t>(p.steps_off, {0, 51, 51, 51, 99, 100}), "steps_off");      // 17 x 3, 5 x 0, -, 16 x 3, 1 x 1
    expect(same<int64_t>(p.rhs_off, {0, 170, 190, 190, 238, 243}), "rhs_off");      // 17 x 10, 5 x 4, -, 16 x 3, 1 x 5
    expect(same<int64_t>(p.noise_off, {0, 102, 112, 112, 176, 177}), "noise_off");  // 17 x 6, 5 x 2, -, 16 x 4, 1 x 1
}

GbsPlan checked(int G, const int32_t* counts, int64_t first, int width, const std::vector<GbsShape>& shapes) {
    std::vector<int32_t> var_ptr((size_t)G + 1, 0);
    std::vector<uint64_t> seeds((size_t)G, 7);
    gbs_check("check: ", G, counts, seeds.data(), var_ptr.data(), first, width);
    return gbs_plan(G, counts, first, width, shapes);
}

struct Bad {
    const char* words;  // of the message
    int G; const int32_t* counts; const uint64_t* seeds; const int32_t* var_ptr; int64_t first; int width;
};

}  // namespace

int main() {
    const int64_t first = 100;
    // width 16: two passes, the second with one live slot of member 0 alone
    {
        GbsPlan p = checked(5, kCounts, first, 16, kShapes);
        offsets_of_the_five(p);
        walk(p, 2, {{16, 5, 0, 16, 1}, {1, 0, 0, 0, 0}}, {16, 1}, first);
    }
    // width 4: the members drop out at different passes
    {
        GbsPlan p = checked(5, kCounts, first, 4, kShapes);
        offsets_of_the_five(p);
        walk(p, 5, {{4, 4, 0, 4, 1}, {4, 1, 0, 4, 0}, {4, 0, 0, 4, 0}, {4, 0, 0, 4, 0}, {1, 0, 0, 0, 0}}, {4, 4, 4, 4, 1}, first);
    }
    // width 1: one draw of every member that still has one per pass
    {
        GbsPlan p = checked(5, kCounts, first, 1, kShapes);
        offsets_of_the_five(p);
        std::vector<std::vector<int>> live;
        for (int k = 0; k < 17; ++k) live.push_back({1, k < 5 ? 1 : 0, 0, k < 16 ? 1 : 0, k < 1 ? 1 : 0});
        walk(p, 17, live, std::vector<int>(17, 1), first);
    }
    // single members: 2 draws (NV = 2), 7 draws at width 8 (NV = 8) and at width 3 (4, 4, 1), the last draw index there is
    {
        const std::vector<GbsShape> one = {{10, 6, 30, 3}};
        int32_t c2 = 2, c7 = 7, c17 = 17;
        GbsPlan p = checked(1, &c2, 0, 16, one);
        walk(p, 1, {{2}}, {2}, 0);
        expect(same<int64_t>(p.steps_off, {0, 6}) && same<int64_t>(p.rhs_off, {0, 20}) && same<int64_t>(p.moments_off, {0, 30}), "one member: offsets");
        p = checked(1, &c7, 5, 8, one);
        walk(p, 1, {{7}}, {8}, 5);
        p = checked(1, &c7, 5, 3, one);
        walk(p, 3, {{3}, {3}, {1}}, {4, 4, 1}, 5);
        const int64_t top = ((int64_t)1 << 32) - 17;
        p = checked(1, &c17, top, 16, one);
        walk(p, 2, {{16}, {1}}, {16, 1}, top);
        expect(p.draw(0, 0, 1) == ((int64_t)1 << 32) - 1, "the last draw index");
    }
    // every argument error, by its words
    {
        const int32_t negative[5] = {17, 5, -1, 16, 1}, none[5] = {0, 0, 0, 0, 0}, huge[2] = {INT32_MAX, 1};
        const int32_t late[6] = {1, 1, 1, 2, 3, 4}, back[6] = {0, 2, 1, 2, 3, 4};
        const Bad errors[] = {
            {"no members", 0, kCounts, kSeeds, kVarPtr, 0, 16},
            {"seeds is null", 5, kCounts, nullptr, kVarPtr, 0, 16},
            {"n_samples is null", 5, nullptr, kSeeds, kVarPtr, 0, 16},
            {"var_ptr is null", 5, kCounts, kSeeds, nullptr, 0, 16},
            {"block_width", 5, kCounts, kSeeds, kVarPtr, 0, 0},
            {"block_width", 5, kCounts, kSeeds, kVarPtr, 0, 17},
            {"must start at 0", 5, kCounts, kSeeds, late, 0, 16},
            {"must not decrease", 5, kCounts, kSeeds, back, 0, 16},
            {"member 2: n_samples is negative", 5, negative, kSeeds, kVarPtr, 0, 16},
            {"zero for every member", 5, none, kSeeds, kVarPtr, 0, 16},
            {"first_sample", 5, kCounts, kSeeds, kVarPtr, -1, 16},
            {"first_sample", 5, kCounts, kSeeds, kVarPtr, ((int64_t)1 << 32) - 16, 16},
        };
        int e = 0;
        for (const Bad& b : errors) {
            try {
                gbs_check("check: ", b.G, b.counts, b.seeds, b.var_ptr, b.first, b.width);
                expect(false, "no error", e);
            } catch (const std::runtime_error& err) {
                const bool ok = std::strstr(err.what(), b.words) != nullptr && std::strncmp(err.what(), "check: ", 7) == 0;
                expect(ok, err.what(), e);
                if (ok) reached[10 + e] = true;
            }
            ++e;
        }
        // more draws than a 32-bit prefix holds: the plan's own error
        try {
            const int32_t two_ptr[3] = {0, 0, 0};
            const uint64_t two_seeds[2] = {1, 2};
            gbs_check("check: ", 2, huge, two_seeds, two_ptr, 0, 16);
            (void)gbs_plan(2, huge, 0, 16, {{10, 6, 30, 3}, {10, 6, 30, 3}});
            expect(false, "no error for 2^31 draws");
        } catch (const std::runtime_error& err) {
            expect(std::strstr(err.what(), "too many draws") != nullptr, err.what());
        }
    }
    expect(gbs_slots(0) == 1 && gbs_slots(1) == 1 && gbs_slots(2) == 2 && gbs_slots(3) == 4 && gbs_slots(5) == 8 && gbs_slots(9) == 16 &&
               gbs_slots(16) == 16, "gbs_slots");
    for (int e = 0; e < 22; ++e)
        if (!reached[e]) { std::fprintf(stderr, "branch %d of the plan was not reached\n", e); ++failures; }
    if (failures) return 1;
    std::printf("every branch reached\n");
    return 0;
}
