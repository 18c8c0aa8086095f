// score_samples_batch.hpp -- posterior samples of every member of a refinement group (include/score_samples_batch.h):
// perturb-and-solve (score_samples.hpp) crossed with the per-member control of the group's gated
// conjugate-gradient iteration (score_group_pcg.hpp, section 12).
//
// In pass k of width W, slot c of member g carries that member's draw first_sample + k W + c; a slot beyond the member's
// count gets r = 0 and done word 1 from the start (k_gbs_begin).  The plan -- offsets, passes, NV per pass, the draw of a
// (member, slot) -- is score_samples_batch_plan.hpp's (HIP-free).
//
// What exists already and is used as it is: ps_measurement<DIM> on the member's gb_view<DIM> (the Jacobian and the noise,
// stated once), group_pcg with a right-hand-side callback, gbm_product for the true residuals, the blocks / gather of H /
// chain factorisation of the group as gbm_solve runs them, GbmWork (B.mvb) for the iteration's vectors -- the marginals and
// the samples share one allocation --, ps_accumulate for the order of the running sums, ps_gather_tile<NV> for the gather
// of one tile, ps_probe_value for the probe, MvTiles and mv_report of score_marginals.hpp.  New here:
//   k_gbs_blocks<DIM>   grid over mblk_member, one lane per measurement of the workgroup's member: J once, then per live
//                       draw of THAT member z and J'z into slot c's slice of a block buffer laid out as the union gblk
//   k_gbs_gather<NV>    b_c[col0 + i] = the contributions of unknown i in gc_ptr / gc_slot order; tiles cut per member from
//                       the union gc_ptr (member in .w); the tile itself is ps_gather_tile with the member's live slots
//   k_gbs_begin         x = 0, r = b_c on the slots that carry a draw; the others r = 0 and done word 1
//   k_gbs_probe_begin   the probe's xi_g into slot 0 of every member with draws
//   k_gbs_residual      per-workgroup partials of |b_c - w_c|^2 on the live slots
//   k_gbs_moments<DIM>  grid over sblk_member, one lane per variable: the running sums over the member's taken draws
//   k_gbs_select        the selected rows of every live (member, slot) into a staging buffer
// No atomics; every sum has a fixed order; every workgroup belongs to one member and returns at once where that member has
// no live slot, so a member's numbers are those of a group that holds it alone.
// What is done with a solved pass is a consumer's, as in ps_solve: GbsMoments (the moments and the selected steps) here,
// GblMeasure (the per-measurement sums of score_leverage_batch.hpp) there.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_samples_batch.h"
#include "score_group_pcg.hpp"
#include "score_marginals_batch.hpp"
#include "score_samples.hpp"
#include "score_samples_batch_plan.hpp"

namespace score {

static_assert(kGbsMaxWidth == kMvMaxWidth, "the plan's widest pass is the block iteration's");

struct GbsArgs {
    GbDev d;
    const double* X;             // the members' points (the group's state)
    const uint64_t* seeds;       // [g]
    const int32_t* cnt_ptr;      // [g + 1] prefix sums of the members' counts (the probe: of S_g > 0)
    int k0, width;               // the pass: slot c carries the member's draw k0 + c, c < width
    long long s0;                // first_sample + k0: the noise index of slot 0
    double* blk; long long gsz;  // [c * gsz + union slot]: J'z of slot c, laid out as the union gblk
    double* noise;               // [c * rows + row0[g] + row] or null
    const long long* row0; long long rows;
    const int32_t* gc_ptr; const int32_t* gc_slot;
    const int4* tiles;           // of the gather: {first unknown, end unknown, long list?, member}
    double* b; long long n;      // [c * n + col0 + i]
    const uint32_t* take;        // [g] moments: bit c set -- the member's draw in slot c enters its sums
    double* mom; double* mean;   // the running sums: member g's moments from mom0[g], its means from col0
    const long long* mom0;
    const int32_t* sel; const int32_t* sel_member;  // [selected row] its member-local unknown, its member
    int n_sel;
    double* steps;               // [c * n_sel + selected row]
};

// live slots of member g in the pass
__device__ __forceinline__ int gbs_live(const GbsArgs& a, int g) {
    const int left = a.cnt_ptr[g + 1] - a.cnt_ptr[g] - a.k0;
    return left <= 0 ? 0 : (left < a.width ? left : a.width);
}

// one measurement of the workgroup's member per lane (ps_measurement on the member's view)
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbs_blocks(GbsArgs a) {
    const int g = a.d.mblk_member[blockIdx.x];
    const int live = gbs_live(a, g);
    if (live == 0) return;
    const GbMember M = a.d.members[g];
    const long long m = (long long)((int)blockIdx.x - M.mblk0) * kThreads + threadIdx.x;
    ps_measurement<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), (int64_t)m, a.seeds[g], (int64_t)a.s0, live, a.blk + M.gblk0,
                        (int64_t)a.gsz, a.noise ? a.noise + a.row0[g] : nullptr, (int64_t)a.rows);
}

// one tile of one member's unknowns per workgroup: ps_gather_tile with the member's live slots
template <int NV>
__global__ __launch_bounds__(kThreads) void k_gbs_gather(GbsArgs a) {
    static_assert(kThreads == kMvThreads, "the gather's tile is the block iteration's workgroup");
    __shared__ double red[(kThreads / 64) * NV];
    const int4 tile = a.tiles[blockIdx.x];
    const int live = gbs_live(a, tile.w);
    if (live == 0) return;
    ps_gather_tile<NV>(a.gc_ptr, a.gc_slot, tile, a.blk, a.gsz, a.b, a.n, live, red);
}

// grid (unknown workgroups, NV): x = 0, r = b_c on the slots that carry a draw (the others: r = 0, done from the start)
__global__ __launch_bounds__(kThreads) void k_gbs_begin(GbmArgs p, GbsArgs a) {
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const GbMember M = a.d.members[g];
    const bool on = c < gbs_live(a, g);
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * p.n + M.col0 + li;
        p.x[e] = 0.0;
        p.r[e] = on ? a.b[e] : 0.0;
    }
    if ((int)blockIdx.x == M.ublk0 && t == 0) {
        p.done[g * p.NV + c] = on ? 0 : 1;
        p.iters[g * p.NV + c] = 0;
        p.ref[g * p.NV + c] = 0.0;
    }
}

// grid (unknown workgroups, NV): the probe -- x = 0, r = b = one standard normal per member-local unknown in slot 0 of
// every member with draws, everything else done
__global__ __launch_bounds__(kThreads) void k_gbs_probe_begin(GbmArgs p, GbsArgs a) {
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const GbMember M = a.d.members[g];
    const bool on = c < gbs_live(a, g);
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const double n0 = on ? ps_probe_value(a.seeds[g], li) : 0.0;
        const long long e = c * p.n + M.col0 + li;
        p.x[e] = 0.0;
        p.r[e] = n0;
        a.b[e] = n0;
    }
    if ((int)blockIdx.x == M.ublk0 && t == 0) {
        p.done[g * p.NV + c] = on ? 0 : 1;
        p.iters[g * p.NV + c] = 0;
        p.ref[g * p.NV + c] = 0.0;
    }
}

// grid (unknown workgroups, NV): partials of |b_c - w_c|^2 on the live slots
__global__ __launch_bounds__(kThreads) void k_gbs_residual(GbmArgs p, GbsArgs a, const double* __restrict__ w) {
    __shared__ double red[4];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    if (c >= gbs_live(a, g)) return;
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    double dv = 0.0;
    if (li < M.n) {
        const long long e = c * p.n + M.col0 + li;
        dv = a.b[e] - w[e];
    }
    const double s = block_sum(dv * dv, red);
    if (t == 0) p.res_part[(size_t)c * p.n_ublocks + blockIdx.x] = s;
}

// one variable of the workgroup's member per lane (pose 0 has no unknowns): ps_accumulate over the member's taken draws
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbs_moments(GbsArgs a, const double* __restrict__ x) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const int g = a.d.sblk_member[blockIdx.x];
    const int live = gbs_live(a, g);
    const unsigned take = a.take[g];
    if (live == 0 || take == 0u) return;
    const GbMember M = a.d.members[g];
    const long long i = (long long)((int)blockIdx.x - M.sblk0) * kThreads + threadIdx.x, np = M.Np - 1;
    PsArgs q{};
    q.live = live; q.take = take; q.x = x + M.col0; q.n = a.n;
    double* mom = a.mom + a.mom0[g];
    double* mean = a.mean + M.col0;
    if (i >= 1 && i < M.Np) {
        const long long j = i - 1;
        ps_accumulate<DP>(q, DP * j, mom + DP * DP * j, mean + DP * j);
    } else if (i >= M.Np && i < M.Np + M.Nl) {
        const long long l = i - M.Np;
        ps_accumulate<DIM>(q, DP * np + DIM * l, mom + DP * DP * np + DIM * DIM * l, mean + DP * np + DIM * l);
    }
}

// grid (blocks over all selected rows, NV): steps[c, row] = x_c[col0_g + sel[row]] on the live slots
__global__ __launch_bounds__(kThreads) void k_gbs_select(GbsArgs a, const double* __restrict__ x) {
    const int c = blockIdx.y;
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= a.n_sel) return;
    const int g = a.sel_member[row];
    if (c >= gbs_live(a, g)) return;
    a.steps[(long long)c * a.n_sel + row] = x[c * a.n + a.d.members[g].col0 + a.sel[row]];
}

// The draws' buffers: device allocations of their own (not the handle's arena); they and the gather's tiles come with the
// first samples call -- score_refine_batch_create costs what it did -- and go with the handle.
struct GbsWork {
    DevBuf<double> blk, b, mom, mean, noise;
    MvTiles tiles;  // of the gather: {first unknown, end unknown, long list?, member}
    DevBuf<long long> row0, mom0;
    std::vector<long long> row0_host, mom0_host;
    long long rows = 0, mom_size = 0;
    template <class Batch>
    void reserve(Batch& B, const std::vector<GbsShape>& shapes, bool with_noise, hipStream_t st) {
        NoArena no_arena;
        const GbUnion& U = B.U;
        if (!blk.d) {
            // the union's contribution lists live on the device (the host's copy went after the create): read the offsets
            // back once and cut every member's tiles from its own lists
            std::vector<int32_t> ptr((size_t)U.n + 1);
            staged_d2h(ptr.data(), B.gc_ptr.d, ptr.size() * sizeof(int32_t), st);
            std::vector<int32_t> own;
            std::vector<long long>& r0 = row0_host;
            rows = 0; mom_size = 0;
            r0.clear(); mom0_host.clear();
            for (int g = 0; g < U.count; ++g) {
                const GbMember& M = U.members[(size_t)g];
                own.assign(ptr.begin() + (std::ptrdiff_t)M.col0, ptr.begin() + (std::ptrdiff_t)(M.col0 + M.n + 1));
                tiles.add(own, M.n, M.col0, g);
                r0.push_back(rows); mom0_host.push_back(mom_size);
                rows += shapes[(size_t)g].rows; mom_size += shapes[(size_t)g].moments;
            }
            tiles.send(st);
            row0.alloc(r0.size()); mom0.alloc(mom0_host.size());
            staged_h2d(row0.d, r0.data(), r0.size() * sizeof(long long), st);
            staged_h2d(mom0.d, mom0_host.data(), mom0_host.size() * sizeof(long long), st);
            const size_t nv = (size_t)kMvMaxWidth;
            b.alloc(nv * (size_t)U.n); b.zero(st);
            mom.alloc((size_t)std::max<long long>(1, mom_size));
            mean.alloc((size_t)U.n);
            blk.alloc(nv * (size_t)std::max<long long>(1, U.gblk_size)); blk.zero(st);
        }
        if (with_noise && !noise.d) { noise.alloc((size_t)kMvMaxWidth * (size_t)std::max<long long>(1, rows)); noise.zero(st); }
    }
};

// what the plan needs of every member (C: the scalar unknowns of its selected variables)
template <class Columns>
inline std::vector<GbsShape> gbs_shapes(const GbUnion& U, Columns columns) {
    std::vector<GbsShape> shapes;
    const int64_t dp = U.dp(), d = U.dim;
    for (int g = 0; g < U.count; ++g) {
        const GbMember& M = U.members[(size_t)g];
        const int64_t rows = gn_dim(U.dim, [&](auto dim) { return ps_rows<decltype(dim)::value>(M.n_rel, M.n_rng, M.n_pri); });
        shapes.push_back(GbsShape{M.n, rows, dp * dp * (M.Np - 1) + d * d * M.Nl, (int64_t)columns(g)});
    }
    return shapes;
}

// A pass of gbs_solve as its consumer sees it: the plan and the members' shapes, the pass, its slots, the most live slots of
// any member, whether any draw of the pass converged (then q.take holds the members' masks on the device), the pass's
// solutions (slot c from x + c * n) and a host buffer for copies back.
struct GbsPass {
    const GbsPlan& plan;
    const std::vector<GbsShape>& shapes;
    int k, NV, most_live;
    bool any;
    const double* x;
    std::vector<double>& host;
};

// one read of the pass's `slots` slices of `stride` doubles, then member g's part of slot c (from first(g), len(g) doubles) to
// where draw k W + c of the member belongs in the caller's array
template <class First, class Len>
inline void gbs_copy_out(const GbsPlan& plan, std::vector<double>& host, hipStream_t st, double* out, const std::vector<int64_t>& off,
                         const double* src, size_t stride, int slots, int k, First first, Len len) {
    host.resize((size_t)slots * stride);
    staged_d2h(host.data(), src, host.size() * sizeof(double), st);
    for (int g = 0; g < plan.G; ++g)
        for (int c = 0; c < plan.live(g, k); ++c) {
            const double* from = host.data() + (size_t)c * stride + (size_t)first(g);
            std::copy(from, from + len(g), out + off[(size_t)g] + (int64_t)plan.local_draw(g, c, k) * (int64_t)len(g));
        }
}

// What score_refine_batch_samples does with a solved pass -- the consumer gbs_solve is given (as PsMoments is ps_solve's): the
// per-variable moments of every member's converged draws and the selected variables' steps.
struct GbsMoments {
    const int32_t* var_ptr; const int32_t* vars;
    double* moments; double* means; double* steps;
    std::vector<int32_t> sel_ptr, sel, sel_member;
    int n_sel = 0;
    DevBuf<int32_t> d_sel, d_sel_member;
    DevBuf<double> d_steps;
    GbsWork* Q = nullptr;
    const GbUnion* U = nullptr;
    const int32_t* offsets(int) { return var_ptr; }
    void check(const GbUnion& Un, const std::string& who, const int32_t*) {
        U = &Un;
        sel_ptr.assign(1, 0);
        for (int g = 0; g < Un.count; ++g) {
            const GbMember& M = Un.members[(size_t)g];
            const int32_t cnt = var_ptr[g + 1] - var_ptr[g];
            if (cnt > 0 && !vars) throw std::runtime_error(who + "vars is null");
            if (cnt > 0)
                mv_variable_unknowns(M.Np, M.Nl, Un.dp(), Un.dim, vars + var_ptr[g], cnt, who + "member " + std::to_string(g) + ": ", sel);
            if (sel.size() >= ((size_t)1 << 27)) throw std::runtime_error(who + "too many selected unknowns");
            sel_ptr.push_back((int32_t)sel.size());
        }
        n_sel = (int)sel.size();
        sel_member.assign((size_t)n_sel, 0);
        for (int g = 0; g < Un.count; ++g) std::fill(sel_member.begin() + sel_ptr[(size_t)g], sel_member.begin() + sel_ptr[(size_t)g + 1], g);
    }
    int64_t columns(int g) const { return sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g]; }
    template <class Batch>
    void begin(Batch& B, GbsArgs& q, const GbsPlan&, const std::vector<GbsShape>&, int widest, hipStream_t st) {
        Q = &B.gbs;
        Q->mom.zero(st); Q->mean.zero(st);
        {
            NoArena no_arena;
            d_sel.alloc((size_t)n_sel); d_sel_member.alloc((size_t)n_sel);
            d_steps.alloc((size_t)widest * (size_t)std::max(1, n_sel));
        }
        staged_h2d(d_sel.d, sel.data(), (size_t)n_sel * sizeof(int32_t), st);
        staged_h2d(d_sel_member.d, sel_member.data(), (size_t)n_sel * sizeof(int32_t), st);
        q.mom = Q->mom.d; q.mean = Q->mean.d; q.mom0 = Q->mom0.d;
        q.sel = d_sel.d; q.sel_member = d_sel_member.d; q.n_sel = n_sel; q.steps = d_steps.d;
    }
    template <class Batch>
    void pass(Batch& B, const GbsArgs& q, const GbsPass& p, hipStream_t st) {
        const dim3 bt(kThreads);
        if (p.any) {
            gn_dim(U->dim, [&](auto dim) { hipLaunchKernelGGL(k_gbs_moments<decltype(dim)::value>, dim3((unsigned)B.n_sblocks), bt, 0, st, q, p.x); });
        }
        if (n_sel && steps) {
            hipLaunchKernelGGL(k_gbs_select, dim3((unsigned)((n_sel + kThreads - 1) / kThreads), (unsigned)p.NV), bt, 0, st, q, p.x);
            HIP_CHECK(hipGetLastError());
            gbs_copy_out(p.plan, p.host, st, steps, p.plan.steps_off, d_steps.d, (size_t)n_sel, p.most_live, p.k,
                         [&](int g) { return sel_ptr[(size_t)g]; }, [&](int g) { return p.shapes[(size_t)g].C; });
        }
    }
    // the running sums of the members that took part, member after member
    void end(const GbsPlan& plan, const std::vector<GbsShape>& shapes, std::vector<double>& host, hipStream_t st) {
        const int G = U->count;
        if (moments) {
            host.resize((size_t)Q->mom_size);
            staged_d2h(host.data(), Q->mom.d, host.size() * sizeof(double), st);
            for (int g = 0; g < G; ++g)
                if (plan.count[(size_t)g] > 0)
                    std::copy(host.begin() + (std::ptrdiff_t)Q->mom0_host[(size_t)g], host.begin() + (std::ptrdiff_t)(Q->mom0_host[(size_t)g] + shapes[(size_t)g].moments),
                              moments + plan.moments_off[(size_t)g]);
        }
        if (means) {
            host.resize((size_t)U->n);
            staged_d2h(host.data(), Q->mean.d, host.size() * sizeof(double), st);
            for (int g = 0; g < G; ++g)
                if (plan.count[(size_t)g] > 0) {
                    const GbMember& M = U->members[(size_t)g];
                    std::copy(host.begin() + (std::ptrdiff_t)M.col0, host.begin() + (std::ptrdiff_t)(M.col0 + M.n), means + plan.means_off[(size_t)g]);
                }
        }
    }
};

// The draws of a call: per member the probe, then pass after pass the noise, J'z, the lock-step solve, the true residuals
// and the verdict of every (member, draw).  Batch: score_refine_batch (its union, point, blocks and gather, its linear-mode
// handle, its GbmWork and GbsWork).  What is done with a solved pass is the caller's (use): offsets(G) -- the per-member
// offsets gbs_check holds to "start at 0, do not decrease" --, check(U, who, n_samples) before any device work,
// columns(g) for the plan, begin(B, q, plan, shapes, widest, st) once the buffers stand, pass(B, q, GbsPass, st) after the
// pass's verdicts and end(plan, shapes, host, st) before the clock stops.  score_refine_batch_samples passes GbsMoments,
// score_refine_batch_leverage (score_leverage_batch.hpp) its per-measurement sums.
template <class Batch, class Use>
int gbs_solve(Batch& B, const std::string& who, const double* poses, const double* landmarks, const uint64_t* seeds, int64_t first_sample,
              const int32_t* n_samples, double rel_tol, int32_t max_iters, int32_t block_width, double* rhs, double* noise,
              double* residuals, int32_t* iters, int32_t* determined, score_samples_batch_info* info, Use& use) {
    const GbUnion& U = B.U;
    const int G = U.count, W = block_width;
    gbs_check(who, G, n_samples, seeds, use.offsets(G), first_sample, block_width);
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    use.check(U, who, n_samples);
    const std::vector<GbsShape> shapes = gbs_shapes(U, [&](int g) { return use.columns(g); });
    const GbsPlan plan = gbs_plan(G, n_samples, first_sample, block_width, shapes);
    HipBackend& be = B.be();
    hipStream_t st = B.stream();
    const long long n = U.n;
    const double t0 = now_ms();
    // H of every member at its point, on the union pattern, lambda = 0; the chains of all members factored once: as gbm_solve
    B.set_point(poses, landmarks);
    B.eval(std::vector<char>((size_t)G, 1), false, true, nullptr);
    const std::vector<double> no_damping((size_t)G, 0.0);
    B.gather_h(no_damping.data());
    be.derive_rho_data(false);
    auto& K = B.mvb;
    auto& Q = B.gbs;
    const int widest = gbs_slots(std::min(W, plan.most));
    const size_t zb_per_vector = (size_t)be.H->bs * (size_t)be.n_join_seps;
    K.reserve(widest, (size_t)G, (size_t)n, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec, zb_per_vector, st);
    Q.reserve(B, shapes, noise != nullptr, st);
    DevBuf<int32_t> d_cnt_ptr, d_probe_ptr;
    DevBuf<uint64_t> d_seeds;
    DevBuf<uint32_t> d_take;
    {
        NoArena no_arena;
        d_cnt_ptr.alloc((size_t)G + 1); d_probe_ptr.alloc((size_t)G + 1);
        d_seeds.alloc((size_t)G); d_take.alloc((size_t)G);
    }
    staged_h2d(d_cnt_ptr.d, plan.cnt_ptr.data(), ((size_t)G + 1) * sizeof(int32_t), st);
    staged_h2d(d_probe_ptr.d, plan.probe_ptr.data(), ((size_t)G + 1) * sizeof(int32_t), st);
    staged_h2d(d_seeds.d, seeds, (size_t)G * sizeof(uint64_t), st);
    GbmArgs a = B.pcg_args();
    a.tol2 = rel_tol * rel_tol;
    a.res_part = K.res_part.d;
    GbsArgs q{};
    q.d = B.dev(); q.X = B.X.d; q.seeds = d_seeds.d;
    q.blk = Q.blk.d; q.gsz = U.gblk_size; q.noise = noise ? Q.noise.d : nullptr; q.row0 = Q.row0.d; q.rows = Q.rows;
    q.gc_ptr = B.gc_ptr.d; q.gc_slot = B.gc_slot.d; q.tiles = Q.tiles.dev.d; q.b = Q.b.d; q.n = n;
    q.take = d_take.d;
    use.begin(B, q, plan, shapes, widest, st);
    const dim3 bt(kThreads);
    const size_t nub = (size_t)B.n_ublocks;
    std::vector<int32_t> words;
    std::vector<double> part, xi_part(nub);
    // the sum of member g's partials of slot c in workgroup order
    auto member_sum = [&](const std::vector<double>& v, int g, int c) {
        const GbMember& M = U.members[(size_t)g];
        double s = 0.0;
        for (int blk = M.ublk0; blk < M.ublk1; ++blk) s += v[(size_t)c * nub + (size_t)blk];
        return s;
    };
    // Is H_g singular?  One probe column per member with draws, in ONE slot of the group's iteration (see ps_solve for why
    // the draws cannot tell and why the true residual decides): slot 0 of member g carries "draw" 0 of a count of one.
    a.sel_ptr = d_probe_ptr.d; a.k0 = 0; a.width = 1;
    q.cnt_ptr = d_probe_ptr.d; q.k0 = 0; q.width = 1; q.s0 = 0;
    group_pcg(be, a, K.pcg, 1, kPsProbeIters, K.zb.d, [&](const GbmArgs& p) {
        const dim3 gu((unsigned)B.n_ublocks, 1u);
        hipLaunchKernelGGL(k_gbs_probe_begin, gu, bt, 0, st, p, q);
        hipLaunchKernelGGL(k_gbs_residual, gu, bt, 0, st, p, q, (const double*)p.x);  // (x = 0: |xi|^2)
        HIP_CHECK(hipGetLastError());
        staged_d2h(xi_part.data(), K.res_part.d, nub * sizeof(double), st);
    }, words);
    a.all_slots = 1; a.p_in = K.pcg.x.d;
    gbm_product(a, st);
    hipLaunchKernelGGL(k_gbs_residual, dim3((unsigned)B.n_ublocks, 1u), bt, 0, st, a, q, (const double*)a.w);
    HIP_CHECK(hipGetLastError());
    part.resize(nub);
    staged_d2h(part.data(), K.res_part.d, nub * sizeof(double), st);
    std::vector<int32_t> det((size_t)G, -1);
    int singular = 0;
    for (int g = 0; g < G; ++g) {
        if (plan.count[(size_t)g] == 0) continue;
        const double xi2 = member_sum(xi_part, g, 0), probe2 = member_sum(part, g, 0);
        det[(size_t)g] = (words[(size_t)g] == 1 && std::isfinite(probe2) && probe2 <= rel_tol * xi2) ? 1 : 0;
        if (!det[(size_t)g]) ++singular;
    }
    HIP_CHECK(sync_stream(st));
    const double t1 = now_ms();
    const size_t total = (size_t)plan.samples;
    std::vector<int32_t> s_done(total, 0), s_iters(total, 0);
    std::vector<double> s_res(total, 0.0), host;
    std::vector<uint32_t> take((size_t)G, 0u);
    int pcg_iters = 0;
    double rhs_ms = 0.0;
    a.sel_ptr = d_cnt_ptr.d; a.width = W;
    q.cnt_ptr = d_cnt_ptr.d; q.width = W;
    for (int k = 0; k < plan.passes; ++k) {
        const int NV = plan.nv(k);
        int most_live = 0;
        for (int g = 0; g < G; ++g) most_live = std::max(most_live, plan.live(g, k));
        a.k0 = k * W;
        q.k0 = k * W; q.s0 = first_sample + (int64_t)k * W;
        // the pass's noise and right-hand sides
        const double tb = now_ms();
        gn_dim(U.dim, [&](auto dim) { hipLaunchKernelGGL(k_gbs_blocks<decltype(dim)::value>, dim3((unsigned)B.n_mblocks), bt, 0, st, q); });
        mv_with_slots(NV, [&](auto nv) {
            hipLaunchKernelGGL(k_gbs_gather<decltype(nv)::value>, dim3((unsigned)Q.tiles.n), bt, 0, st, q);
        });
        HIP_CHECK(hipGetLastError());
        if (noise)
            gbs_copy_out(plan, host, st, noise, plan.noise_off, Q.noise.d, (size_t)Q.rows, most_live, k,
                         [&](int g) { return Q.row0_host[(size_t)g]; }, [&](int g) { return shapes[(size_t)g].rows; });
        if (rhs)
            gbs_copy_out(plan, host, st, rhs, plan.rhs_off, Q.b.d, (size_t)n, most_live, k,
                         [&](int g) { return U.members[(size_t)g].col0; }, [&](int g) { return shapes[(size_t)g].n; });
        HIP_CHECK(sync_stream(st));
        rhs_ms += now_ms() - tb;
        const dim3 gu((unsigned)B.n_ublocks, (unsigned)NV);
        group_pcg(be, a, K.pcg, NV, max_iters, K.zb.d, [&](const GbmArgs& p) { hipLaunchKernelGGL(k_gbs_begin, gu, bt, 0, st, p, q); }, words);
        // the true residual of every draw of the pass (one more product, w = H x)
        a.all_slots = 1; a.p_in = K.pcg.x.d;
        gbm_product(a, st);
        hipLaunchKernelGGL(k_gbs_residual, gu, bt, 0, st, a, q, (const double*)a.w);
        HIP_CHECK(hipGetLastError());
        part.resize((size_t)NV * nub);
        staged_d2h(part.data(), K.res_part.d, part.size() * sizeof(double), st);
        int most_steps = 0;
        bool any = false;
        for (int g = 0; g < G; ++g) {
            take[(size_t)g] = 0u;
            for (int c = 0; c < plan.live(g, k); ++c) {
                const double rho = std::sqrt(member_sum(part, g, c));
                const size_t at = (size_t)plan.draw_off[(size_t)g] + (size_t)plan.local_draw(g, c, k), word = (size_t)g * (size_t)NV + (size_t)c;
                const bool ok = det[(size_t)g] == 1 && words[word] == 1 && std::isfinite(rho);
                s_res[at] = rho;
                s_done[at] = ok ? 1 : 0;
                s_iters[at] = words[(size_t)G * (size_t)NV + word];
                most_steps = std::max(most_steps, s_iters[at]);
                if (ok) take[(size_t)g] |= 1u << c;
            }
            any = any || take[(size_t)g] != 0u;
        }
        pcg_iters += most_steps;
        if (any) staged_h2d(d_take.d, take.data(), (size_t)G * sizeof(uint32_t), st);
        use.pass(B, q, GbsPass{plan, shapes, k, NV, most_live, any, (const double*)K.pcg.x.d, host}, st);
        HIP_CHECK(hipGetLastError());
    }
    use.end(plan, shapes, host, st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(s_done, s_iters, s_res, residuals, iters, worst);
    for (int g = 0; determined && g < G; ++g) determined[g] = det[(size_t)g];
    if (info) {
        info->members = G; info->samples = (int32_t)plan.samples; info->passes = plan.passes; info->pcg_iters = pcg_iters;
        info->unconverged = unconverged; info->singular = singular;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->rhs_ms = rhs_ms; info->solve_ms = t2 - t1 - rhs_ms;
    }
    return unconverged ? 1 : 0;
}

}  // namespace score

