// score_refine_handles.hpp -- the two refinement handles of the HIP library: score_refine (one graph, score_gn.hpp) and
// score_refine_batch (a group in lock-step, score_gn_batch.hpp), and what they share (RefineBase).
//
// Part of score_hip.hip's translation unit, included there once after score_abi.hpp: it uses the backend (HipBackend, DevBuf,
// the arena and the staged copies) and the boundary's g_err.  The analyses are templates over a handle, so all of them come
// first; the entry points of both handles are score_refine_abi.hpp.
#pragma once

#include "score_marginals.hpp"
#include "score_spectrum.hpp"
#include "score_curvature.hpp"
#include "score_samples.hpp"
#include "score_leverage.hpp"
#include "score_relative.hpp"
#include "score_select.hpp"
#include "score_select_poses.hpp"
#include "score_gn_robust.hpp"
#include "score_gn_batch.hpp"
#include "score_gn_robust_batch.hpp"
#include "score_group_pcg.hpp"
#include "score_marginals_batch.hpp"
#include "score_samples_batch.hpp"
#include "score_leverage_batch.hpp"
#include "score_relative_batch.hpp"
#include "score_select_batch.hpp"
#include "score_spectrum_batch.hpp"
#include "score_curvature_batch.hpp"

// the measurement arrays (score_gn.hpp) on the device
struct GnMeasDev : score::GnMeasT<DevBuf> {
    void upload(const score::GnMeas& h) {
        score::gn_meas_each(*this, h, [](auto& dst, const auto& src, int, int) { dst.upload(src); });
    }
    score::GnMeasPtr ptrs() const {
        score::GnMeasPtr p;
        score::gn_meas_each(p, *this, [](auto& dst, const auto& src, int, int) { dst = src.d; });
        return p;
    }
};

// What a refinement handle is made of, one graph or a group: the linear-mode handle `lin` on the pattern of H (its K0 values
// are written in place by the gather kernels), the measurement arrays, the contribution lists, the block storage, the
// per-workgroup partials, and the buffers of the robust refinement.
struct RefineBase {
    score_handle* lin = nullptr;
    int device = 0;
    double setup_ms = 0;
    GnMeasDev meas;
    DevBuf<int32_t> hc_ptr, hc_slot, gc_ptr, gc_slot;
    DevBuf<double> hblk, gblk, rhs, cost_part, gmax_part;
    int n_mblocks = 0, n_ublocks = 0, n_hblocks = 0, n_sblocks = 0;
    std::vector<double> part_host;
    // robust refinement (score_gn_robust.hpp, score_gn_robust_batch.hpp): the measured precisions beside rng_prec / rel_kappa /
    // rel_tau (which hold a robust run's weighted ones while it lasts, and after a group's run with keep_weights), residuals,
    // weights (ranges, then loop closures), per-workgroup partials; they come with the first robust call
    DevBuf<double> rb_prec0, rb_kappa0, rb_tau0, rb_r_rng, rb_r_lc, rb_w_rng, rb_w_lc, rb_part;
    bool rb_ready = false;

    ~RefineBase() { if (lin) score_destroy(lin); }
    HipBackend& be() { return lin->solver.be; }
    hipStream_t stream() { return lin->solver.be.stream; }
    // the linear-mode handle on the pattern given (gn_linear_pattern); the handle's device is its device
    void open_linear(int64_t n, const std::vector<int32_t>& hptr, const std::vector<int32_t>& hcol, const std::vector<int32_t>& chain_ptr,
                     const std::vector<int32_t>& node_first_col, const score_settings* s) {
        const score_problem pat = score::gn_linear_pattern(n, hptr, hcol, chain_ptr, node_first_col);
        if (score_linear_create(&pat, s, &lin) != 0) throw std::runtime_error(g_err);
        device = lin->solver.st.device;
    }
    // the first n partials of buf on the host (part_host), the stream waited for
    const std::vector<double>& read_partials(const DevBuf<double>& buf, size_t n) {
        part_host.resize(n);
        HIP_CHECK(hipMemcpyAsync(part_host.data(), buf.d, n * sizeof(double), hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(sync_stream(stream()));
        return part_host;
    }
    score::GnRobustArrays robust_arrays() const {
        return score::GnRobustArrays{rb_prec0.d, rb_kappa0.d, rb_tau0.d, meas.rng_prec.d, meas.rel_kappa.d, meas.rel_tau.d,
                                     rb_r_rng.d, rb_r_lc.d, rb_w_rng.d, rb_w_lc.d};
    }
    // Residuals and weights of a robust refinement as they are on the device, into the caller's arrays (null: not wanted);
    // hw / hwl: the weights
    void robust_read(double* w, double* r, double* wl, double* rl, std::vector<double>& hw, std::vector<double>& hwl) {
        const size_t nr = rb_r_rng.n, nc = rb_r_lc.n, f8 = sizeof(double);
        hw.resize(nr); hwl.resize(nc);
        if (nr) staged_d2h(hw.data(), rb_w_rng.d, nr * f8, stream());
        if (nc) staged_d2h(hwl.data(), rb_w_lc.d, nc * f8, stream());
        if (r && nr) staged_d2h(r, rb_r_rng.d, nr * f8, stream());
        if (rl && nc) staged_d2h(rl, rb_r_lc.d, nc * f8, stream());
        HIP_CHECK(sync_stream(stream()));
        if (w) std::copy(hw.begin(), hw.end(), w);
        if (wl) std::copy(hwl.begin(), hwl.end(), wl);
    }
};

// Local refinement after SCORE on the device (score_gn.hpp): state, blocks and gathers here, the damped
// normal equations through the linear-mode handle `lin` (its right-hand side is written in place by the gather kernel; the
// step is read from its solution vector).
struct score_refine : RefineBase {
    score::GnProblem P;
    DevBuf<int32_t> is_diag;
    DevBuf<double> u, ut;
    score::MvTiles h_tiles;  // the product's tiles of H's rows: product_tiles()
    score::MvWork mv;  // marginal covariances (score_marginals.hpp)
    score::SpWork sp;  // lowest eigenpairs of H (score_spectrum.hpp)
    score::CvWork cv;  // half the Hessian of the cost: product and lowest eigenpairs (score_curvature.hpp)
    score::PsWork ps;  // posterior samples (score_samples.hpp)
    score::LvWork lv;  // range leverage and predicted range variances (score_leverage.hpp)
    score::RpWork rp;  // predicted relative poses and their covariances (score_relative.hpp)
    score::SelWork sel;  // greedy selection of candidate ranges (score_select.hpp)
    score::SelpWork selp;  // and of candidate loop closures: what the blocks add (score_select_poses.hpp)
    int64_t rb_n_lc = 0;
    const score_refine_robust_settings* rb_settings = nullptr;  // of the robust run under way

    bool has_landmarks() const { return P.Nl != 0; }  // (a point then has a landmark array)
    score::GnView view(const double* where) const {  // the graph on the device, at the point `where`
        return score::GnView{P.Np, P.Nl, P.n_rel(), P.n_rng(), P.n_pri(), meas.ptrs(), where, hblk.d, gblk.d};
    }
    void create(const score_graph& g, const score_settings* s) {
        const double t0 = score::now_ms();
        score::PhaseTimer pt(s && s->verbose != 0);
        score::gn_build(g, P);
        pt.mark("refine: pattern + contribution lists");
        open_linear(P.n, P.hptr, P.hcol, P.chain_ptr, P.node_first_col, s);
        pt.mark("refine: linear-mode handle");
        tl_copy_stream = stream();
        ArenaScope arena_scope(&be().arena);  // the refinement's buffers come from (and go back with) the handle's arena
        meas.upload(P);
        hc_ptr.upload(P.hc_ptr); hc_slot.upload(P.hc_slot); gc_ptr.upload(P.gc_ptr); gc_slot.upload(P.gc_slot);
        std::vector<int32_t> dg(P.hcol.size(), 0);
        for (int64_t i = 0; i < P.n; ++i) dg[(size_t)P.diag_pos[(size_t)i]] = 1;
        is_diag.upload(dg);
        // state: every pose (2-D [theta, x, y], 3-D [R | t]), then the landmarks -- the caller's layout
        u.alloc((size_t)P.state_size()); ut.alloc((size_t)P.state_size()); rhs.alloc((size_t)P.n);
        hblk.alloc((size_t)std::max<int64_t>(1, P.hblk_size())); gblk.alloc((size_t)std::max<int64_t>(1, P.gblk_size()));
        n_mblocks = (int)std::max<int64_t>(1, (P.n_meas() + kThreads - 1) / kThreads);
        n_ublocks = (int)std::max<int64_t>(1, (P.n + kThreads - 1) / kThreads);
        n_sblocks = (int)std::max<int64_t>(1, (P.Np + P.Nl + kThreads - 1) / kThreads);
        n_hblocks = (int)std::max<int64_t>(1, ((int64_t)P.hcol.size() + kThreads - 1) / kThreads);
        cost_part.alloc((size_t)n_mblocks); gmax_part.alloc((size_t)n_ublocks);
        be().linear_buffers(lin->solver.H);
        pt.mark("refine: uploads + buffers");
        setup_ms = score::now_ms() - t0;
    }

    // ---- the backend concept of gn_lm_run ----
    double eval_at(const double* where, bool with_blocks) {
        score::gn_dim(P.dim, [&](auto dim) {
            hipLaunchKernelGGL(score::k_gn_blocks<decltype(dim)::value>, dim3(n_mblocks), dim3(kThreads), 0, stream(), view(where), cost_part.d,
                               with_blocks ? 1 : 0);
        });
        double f = 0.0;
        for (double v : read_partials(cost_part, (size_t)n_mblocks)) f += v;
        return f;
    }
    double eval_current(bool with_blocks) { return eval_at(u.d, with_blocks); }
    double eval_trial() {
        score::gn_dim(P.dim, [&](auto dim) {  // (3-D: the retraction R <- R Exp(omega), t <- t + v)
            hipLaunchKernelGGL(score::k_gn_trial<decltype(dim)::value>, dim3(n_sblocks), dim3(kThreads), 0, stream(), (const double*)u.d,
                               (const double*)be().xtu.d, ut.d, (int64_t)P.Np, (int64_t)P.Nl);
        });
        return eval_at(ut.d, false);
    }
    void accept() { std::swap(u.d, ut.d); }
    double assemble() {  // g = J'r (rhs = -g) from the blocks of the current point; returns |g|_inf
        hipLaunchKernelGGL(score::k_gn_gather_g, dim3(n_ublocks), dim3(kThreads), 0, stream(), (const int32_t*)gc_ptr.d,
                           (const int32_t*)gc_slot.d, (const double*)gblk.d, rhs.d, gmax_part.d, (int64_t)P.n);
        double m = 0.0;
        for (double v : read_partials(gmax_part, (size_t)n_ublocks)) m = std::max(m, v);
        return m;
    }
    void gather_h(double lambda) {  // J'J + lambda I from the blocks of the last evaluation, into the handle's K0
        hipLaunchKernelGGL(score::k_gn_gather_h, dim3(n_hblocks), dim3(kThreads), 0, stream(), (const int32_t*)hc_ptr.d,
                           (const int32_t*)hc_slot.d, (const double*)hblk.d, (const int32_t*)is_diag.d, lambda, be().K0d.d,
                           (int64_t)P.hcol.size());
    }
    bool solve(double lambda, double rel_tol, int* used) {  // (J'J + lambda I) step = -g, step left in the handle's xtu
        gather_h(lambda);
        return be().linear_solve_core(lin->solver.H, rhs.d, rel_tol, 4000, used);
    }
    // the caller's point becomes the current one (u); returns the state as uploaded.  The state is the input layout: the poses
    // (pose 0 included), then the landmarks
    std::vector<double> set_point(const double* poses_in, const double* lms_in) {
        const int64_t np = P.state_size() - P.dim * P.Nl;
        std::vector<double> u0((size_t)P.state_size());
        std::copy(poses_in, poses_in + np, u0.begin());
        if (P.Nl) std::copy(lms_in, lms_in + P.dim * P.Nl, u0.begin() + (std::ptrdiff_t)np);
        staged_h2d(u.d, u0.data(), u0.size() * sizeof(double), stream());
        HIP_CHECK(sync_stream(stream()));
        return u0;
    }
    // The head of an analysis at a point (marginals, weakest modes, posterior samples): the point, its blocks, H on the handle's
    // pattern (lambda = 0).  who: the entry point's words in front of a message; block_needs: what a block of vectors asks of
    // the chain kernel in those words (null: a call that runs the single solves, which refuse nothing here).
    void h_at_point(const double* poses_in, const double* lms_in, const std::string& who, const char* block_needs) {
        (void)set_point(poses_in, lms_in);
        (void)eval_at(u.d, true);
        gather_h(0.0);
        if (!block_needs) return;
        if (be().split.active) throw std::runtime_error(who + block_needs + " the unsplit chain kernel (chain_split = 0)");
        if (be().n_prec == 0) throw std::runtime_error(who + "the handle has no preconditioner work (no unknowns?)");
    }
    // the product's tiles of H's rows: they come with the first analysis that multiplies by H, once for all of them
    const score::MvTiles& product_tiles() {
        if (!h_tiles.dev.d) {
            NoArena no_arena;
            h_tiles.add(P.hptr, P.n);
            h_tiles.send(stream());
        }
        return h_tiles;
    }
    score::LmState run(const double* poses_in, const double* lms_in, int max_iters, double tol, double* poses_out, double* lms_out) {
        std::vector<double> u0 = set_point(poses_in, lms_in);
        const score::LmState s = score::gn_lm_run(*this, max_iters, tol, 1e-9);
        read_point(u0, poses_out, lms_out);
        return s;
    }
    // the current point (u) in the caller's layout; u0: scratch of the state's size
    void read_point(std::vector<double>& u0, double* poses_out, double* lms_out) {
        const std::ptrdiff_t np = (std::ptrdiff_t)(P.state_size() - P.dim * P.Nl);
        staged_d2h(u0.data(), u.d, u0.size() * sizeof(double), stream());
        HIP_CHECK(sync_stream(stream()));
        std::copy(u0.begin(), u0.begin() + np, poses_out);
        if (P.Nl) std::copy(u0.begin() + np, u0.end(), lms_out);
    }

    // ---- robust refinement: the hooks of gn_robust_refine (score_gn_robust.hpp) ----
    void robust_reserve() {  // the buffers, from the handle's arena; the measured precisions are what the block kernels' arrays hold now
        if (rb_ready) return;
        rb_n_lc = score::gn_n_loop_closures(P);
        if (rb_n_lc < 0) throw std::runtime_error("score_refine: fewer relative-pose entries than odometry steps");
        ArenaScope arena_scope(&be().arena);
        const size_t nr = (size_t)P.n_rng(), nc = (size_t)rb_n_lc, first = (size_t)P.n_rel() - nc;
        rb_prec0.alloc(nr); rb_r_rng.alloc(nr); rb_w_rng.alloc(nr);
        rb_kappa0.alloc(nc); rb_tau0.alloc(nc); rb_r_lc.alloc(nc); rb_w_lc.alloc(nc);
        rb_part.alloc((size_t)score::kGnRobustPart * ((nr + nc + kThreads - 1) / kThreads));
        const size_t f8 = sizeof(double);
        if (nr) HIP_CHECK(hipMemcpyAsync(rb_prec0.d, meas.rng_prec.d, nr * f8, hipMemcpyDeviceToDevice, stream()));
        if (nc) HIP_CHECK(hipMemcpyAsync(rb_kappa0.d, meas.rel_kappa.d + first, nc * f8, hipMemcpyDeviceToDevice, stream()));
        if (nc) HIP_CHECK(hipMemcpyAsync(rb_tau0.d, meas.rel_tau.d + first, nc * f8, hipMemcpyDeviceToDevice, stream()));
        HIP_CHECK(sync_stream(stream()));
        rb_ready = true;
    }
    void robust_restore() noexcept {  // the block kernels' arrays hold the measured precisions again
        if (!rb_ready) return;
        const size_t nr = (size_t)P.n_rng(), nc = (size_t)rb_n_lc, first = (size_t)P.n_rel() - nc, f8 = sizeof(double);
        if (nr) (void)hipMemcpyAsync(meas.rng_prec.d, rb_prec0.d, nr * f8, hipMemcpyDeviceToDevice, stream());
        if (nc) (void)hipMemcpyAsync(meas.rel_kappa.d + first, rb_kappa0.d, nc * f8, hipMemcpyDeviceToDevice, stream());
        if (nc) (void)hipMemcpyAsync(meas.rel_tau.d + first, rb_tau0.d, nc * f8, hipMemcpyDeviceToDevice, stream());
        (void)sync_stream(stream());
    }
    score::GnRobustDev robust_dev(int families) const {
        score::GnRobustDev a{};
        a.g = view(u.d);
        a.n_a = (families & score::kGnRobustRanges) ? P.n_rng() : 0;
        a.n_b = (families & score::kGnRobustClosures) ? rb_n_lc : 0;
        a.first_lc = P.n_rel() - rb_n_lc;
        a.a = robust_arrays();
        return a;
    }
    void robust_weights(int families, double mu, double c, double c_rel, double min_weight, bool apply) {
        const score::GnRobustDev a = robust_dev(families);
        const int64_t lanes = a.n_a + a.n_b;
        if (lanes == 0) return;  // (an enabled family without measurements launches nothing)
        hipLaunchKernelGGL(score::k_gn_robust_weight, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream(), a, mu,
                           c, c_rel, min_weight, (int32_t)(apply ? score::kGbrNext : score::kGbrInspect));
    }
    void robust_weights(int families, double mu) {
        robust_weights(families, mu, rb_settings->inlier_threshold, rb_settings->rel_threshold, rb_settings->min_weight, true);
    }
    void robust_begin() { robust_weights(score::kGnRobustRanges | score::kGnRobustClosures, 0.0, 1.0, 1.0, 1.0, true); }
    void robust_residuals(int families, score::RobustSeen* seen) {  // seen[0]: the ranges, seen[1]: the loop closures
        const score::GnRobustDev a = robust_dev(families);
        const int64_t lanes = a.n_a + a.n_b;
        const int nb = (int)((lanes + kThreads - 1) / kThreads);
        double r2[2] = {0.0, 0.0}, nonbin[2] = {0.0, 0.0};
        if (nb > 0) {
            score::gn_dim(P.dim, [&](auto dim) {
                hipLaunchKernelGGL(score::k_gn_robust_resid<decltype(dim)::value>, dim3(nb), dim3(kThreads), 0, stream(), a, rb_part.d);
            });
            score::gn_robust_fold(read_partials(rb_part, (size_t)score::kGnRobustPart * (size_t)nb).data(), 0, nb, r2, nonbin);
        }
        seen[0] = score::RobustSeen{P.n_rng(), r2[0], 0.0, (int32_t)nonbin[0]};
        seen[1] = score::RobustSeen{rb_n_lc, r2[1], 0.0, (int32_t)nonbin[1]};
    }
    void robust_run(const score_refine_robust_settings& s, const double* poses_in, const double* lms_in, double* poses_out, double* lms_out,
                    double* w, double* r, double* wl, double* rl, int32_t* outliers, int32_t* rel_outliers, score::GnRobustResult& R) {
        score::gn_robust_check(s, P);
        robust_reserve();
        struct Restore {  // whatever happens, the handle ends with the measured precisions
            score_refine& h;
            ~Restore() { h.robust_restore(); h.rb_settings = nullptr; }
        } restore{*this};
        rb_settings = &s;
        std::vector<double> u0 = set_point(poses_in, lms_in);
        score::gn_robust_refine(*this, s, 1e-9, R);
        score::RobustSeen seen[2];
        robust_residuals(score::kGnRobustRanges | score::kGnRobustClosures, seen);  // every family's r at the final estimate
        std::vector<double> hw, hwl;
        robust_read(w, r, wl, rl, hw, hwl);
        if (outliers) { *outliers = 0; for (double v : hw) *outliers += v < 0.5 ? 1 : 0; }
        if (rel_outliers) { *rel_outliers = 0; for (double v : hwl) *rel_outliers += v < 0.5 ? 1 : 0; }
        if (!(s.families & score::kGnRobustClosures) && rel_outliers) *rel_outliers = 0;
        if (poses_out) read_point(u0, poses_out, lms_out);
    }
    void robust_inspect(const double* poses, const double* lms, double mu, double c, double c_rel, double* r, double* rl, double* w, double* wl) {
        if (!(mu >= 0.0) || !std::isfinite(mu)) throw std::runtime_error("score_refine_residuals: mu must be finite and >= 0");
        if (mu > 0.0 && !(std::isfinite(c) && c > 0.0 && std::isfinite(c_rel) && c_rel > 0.0))
            throw std::runtime_error("score_refine_residuals: c and c_rel must be positive and finite when mu > 0");
        const int both = score::kGnRobustRanges | score::kGnRobustClosures;
        robust_reserve();
        (void)set_point(poses, lms);
        robust_begin();
        score::RobustSeen seen[2];
        robust_residuals(both, seen);
        robust_weights(both, mu, c, c_rel, 1.0, false);
        std::vector<double> hw, hwl;
        robust_read(w, r, wl, rl, hw, hwl);
    }
};

// Local refinement of a group of graphs in lock-step (score_gn_batch.hpp): the union state, blocks and gathers here, the
// chain factorisation and M^-1 through the linear-mode handle `lin` on the union pattern, the per-member conjugate-gradient
// iteration in score_group_pcg.hpp.  This struct is the backend of gb_lock_step.
struct score_refine_batch : RefineBase {
    score::GbUnion U;
    int rounds = 0;  // of the last run
    DevBuf<score::GbMember> members;
    DevBuf<int4> tiles;
    DevBuf<int32_t> mblk_member, ublk_member, sblk_member, rblk_member, diag_member;
    DevBuf<int32_t> mask;
    DevBuf<double> X, Xt, lambda;
    score::GroupPcgWork pcg;  // the damped step: one slot of the group's iteration, its solution in pcg.x
    int n_tiles = 0;
    long long nnz = 0;
    std::vector<int32_t> word_host;
    score::GbmWork mvb;  // marginal covariances of the members (score_marginals_batch.hpp)
    score::GspWork spb;  // lowest eigenpairs of the members (score_spectrum_batch.hpp)
    score::GbcWork gbc;  // half the Hessian of the members' costs: product and lowest eigenpairs (score_curvature_batch.hpp)
    score::GbsWork gbs;  // posterior samples of the members (score_samples_batch.hpp)
    score::GblWork gbl;  // range leverage and predicted range variances of the members (score_leverage_batch.hpp)
    score::GrpWork grp;  // predicted relative poses of the members and their covariances (score_relative_batch.hpp)
    score::GbSelWork gbsel;  // greedy selection of the members' candidate ranges (score_select_batch.hpp)
    // robust refinement: the members' parameters beside the base's buffers.  U keeps rng_prec / rel_kappa / rel_tau on the host
    // for its checks.
    DevBuf<score::GbrParam> rb_params;
    std::vector<double> rb_kappa0_host, rb_tau0_host;   // loop-closure order
    int robust_rounds = 0, stage_rounds = 0;  // of the last robust run: its rounds, the passes in which some member changed stage

    int count() const { return U.count; }
    bool has_landmarks() const { return U.lms_size != 0; }  // (some member's point then has a landmark array)
    score::GbDev dev() const {
        return score::GbDev{members.d, mblk_member.d, ublk_member.d, sblk_member.d, rblk_member.d, meas.ptrs()};
    }
    void create(const score_graph* graphs, int32_t n_graphs, const score_settings* s) {
        const double t0 = score::now_ms();
        score::PhaseTimer pt(s && s->verbose != 0);
        score::gb_build(graphs, n_graphs, U);
        pt.mark("refine batch: union pattern + contribution lists");
        open_linear(U.n, U.hptr, U.hcol, U.chain_ptr, U.node_first_col, s);
        pt.mark("refine batch: linear-mode handle");
        if (be().split.active) throw std::runtime_error("score_refine_batch: the group needs the unsplit chain kernel (chain_split = 0)");
        if (be().n_prec == 0) throw std::runtime_error("score_refine_batch: the handle has no preconditioner work (no pose chains?)");
        tl_copy_stream = stream();
        ArenaScope arena_scope(&be().arena);  // the group's buffers come from (and go back with) the handle's arena
        members.upload(U.members); tiles.upload(U.tiles);
        mblk_member.upload(U.mblk_member); ublk_member.upload(U.ublk_member); sblk_member.upload(U.sblk_member);
        rblk_member.upload(U.rblk_member);
        meas.upload(U);
        hc_ptr.upload(U.hc_ptr); hc_slot.upload(U.hc_slot); gc_ptr.upload(U.gc_ptr); gc_slot.upload(U.gc_slot);
        diag_member.upload(U.diag_member);
        n_mblocks = (int)U.mblk_member.size(); n_ublocks = (int)U.ublk_member.size(); n_sblocks = (int)U.sblk_member.size();
        n_tiles = (int)U.tiles.size();
        nnz = (long long)U.hcol.size();
        n_hblocks = (int)std::max<long long>(1, (nnz + kThreads - 1) / kThreads);
        const size_t G = (size_t)U.count, n = (size_t)U.n;
        X.alloc((size_t)U.state_size); Xt.alloc((size_t)U.state_size);
        hblk.alloc((size_t)std::max<long long>(1, U.hblk_size)); gblk.alloc((size_t)std::max<long long>(1, U.gblk_size));
        cost_part.alloc((size_t)n_mblocks); gmax_part.alloc((size_t)n_ublocks); lambda.alloc(G);
        mask.alloc(G);
        rhs.alloc(n); rhs.zero(stream());
        pcg.reserve(1, 1, G, n, (size_t)n_tiles, (size_t)n_ublocks, (size_t)be().n_prec, stream());
        be().linear_buffers(lin->solver.H);
        HIP_CHECK(sync_stream(stream()));
        // the lists live on the device now (the precisions a robust run re-weights stay: its checks and prec0 read them)
        for (std::vector<int32_t>* v : {&U.hptr, &U.hcol, &U.hc_ptr, &U.hc_slot, &U.gc_ptr, &U.gc_slot, &U.diag_member, &U.rel_i, &U.rel_j,
                                        &U.rng_a, &U.rng_b, &U.pri_l, &U.chain_ptr, &U.node_first_col})
            std::vector<int32_t>().swap(*v);
        for (std::vector<double>* v : {&U.rel_t, &U.rel_R, &U.rng_dist, &U.pri_t, &U.pri_prec})
            std::vector<double>().swap(*v);
        pt.mark("refine batch: uploads + buffers");
        setup_ms = score::now_ms() - t0;
    }

    void set_mask(const std::vector<char>& m) {
        word_host.assign(m.begin(), m.end());
        HIP_CHECK(hipMemcpyAsync(mask.d, word_host.data(), word_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream()));
        HIP_CHECK(sync_stream(stream()));
    }
    // ---- the backend concept of gb_lock_step ----
    void eval(const std::vector<char>& m, bool trial, bool with_blocks, double* cost) {
        set_mask(m);
        const double* where = trial ? Xt.d : X.d;
        score::gn_dim(U.dim, [&](auto dim) {
            hipLaunchKernelGGL(score::k_gb_blocks<decltype(dim)::value>, dim3(n_mblocks), dim3(kThreads), 0, stream(), dev(), where, hblk.d,
                               gblk.d, cost_part.d, (const int32_t*)mask.d, with_blocks ? 1 : 0);
        });
        HIP_CHECK(hipGetLastError());
        if (!cost) return;
        read_partials(cost_part, (size_t)n_mblocks);
        for (int g = 0; g < U.count; ++g) {
            if (!m[(size_t)g]) continue;
            double f = 0.0;  // the member's partials in workgroup order: the sum a handle on it alone forms
            for (int b = U.members[(size_t)g].mblk0; b < U.members[(size_t)g].mblk1; ++b) f += part_host[(size_t)b];
            cost[g] = f;
        }
    }
    void gradient(const std::vector<char>& m, double* gnorm) {
        set_mask(m);
        hipLaunchKernelGGL(score::k_gb_gather_g, dim3(n_ublocks), dim3(kThreads), 0, stream(), dev(), (const int32_t*)gc_ptr.d,
                           (const int32_t*)gc_slot.d, (const double*)gblk.d, rhs.d, gmax_part.d, (const int32_t*)mask.d);
        HIP_CHECK(hipGetLastError());
        read_partials(gmax_part, (size_t)n_ublocks);
        for (int g = 0; g < U.count; ++g) {
            if (!m[(size_t)g]) continue;
            double mx = 0.0;
            for (int b = U.members[(size_t)g].ublk0; b < U.members[(size_t)g].ublk1; ++b) mx = std::max(mx, part_host[(size_t)b]);
            gnorm[g] = mx;
        }
    }
    // dst = retract(src, step) on the masked members' variables (step null: the copy)
    void retract(const std::vector<char>& m, const double* src, const double* step, double* dst) {
        set_mask(m);
        score::gn_dim(U.dim, [&](auto dim) {
            hipLaunchKernelGGL(score::k_gb_trial<decltype(dim)::value>, dim3(n_sblocks), dim3(kThreads), 0, stream(), dev(), src, step, dst,
                               (const int32_t*)mask.d);
        });
    }
    void trial(const std::vector<char>& m) { retract(m, X.d, pcg.x.d, Xt.d); }
    void accept(const std::vector<char>& m) { retract(m, Xt.d, nullptr, X.d); }  // the trial point of the masked members becomes their current one
    // J'J + lambda_g I of every member from the blocks of the last evaluation, into the handle's K0 (lam: one per member; read
    // by the time the stream is next waited for)
    void gather_h(const double* lam) {
        hipStream_t st = stream();
        HIP_CHECK(hipMemcpyAsync(lambda.d, lam, (size_t)U.count * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(score::k_gb_gather_h, dim3(n_hblocks), dim3(kThreads), 0, st, (const int32_t*)hc_ptr.d, (const int32_t*)hc_slot.d,
                           (const double*)hblk.d, (const int32_t*)diag_member.d, (const double*)lambda.d, be().K0d.d, nnz);
    }
    // the union, its matrix and its tiles as the kernels of score_group_pcg.hpp see them
    score::GbmArgs pcg_args() {
        score::GbmArgs a{};
        a.d = dev();
        a.ptr = be().Kset.mat.ptr.d; a.col = be().Kset.mat.col.d; a.val = be().Kset.mat.val.d;
        a.tiles = tiles.d; a.n_tiles = n_tiles; a.n_ublocks = n_ublocks; a.n = U.n;
        return a;
    }
    // (J'J + lambda_g I) step = -g on the masked members, the steps left in pcg.x; ok / used per masked member
    void solve(const std::vector<char>& m, const double* lam, double rel_tol, char* ok, int32_t* used) {
        const int G = U.count;
        hipStream_t st = stream();
        gather_h(lam);
        be().derive_rho_data(false);  // K = K0, its chain factors and Jacobi inverses, for the whole group
        word_host.assign((size_t)(2 * G + 1), 0);  // (steps and the chain kernel's done word: zero)
        for (int g = 0; g < G; ++g) word_host[(size_t)g] = m[(size_t)g] ? 0 : 1;
        HIP_CHECK(hipMemcpyAsync(pcg.flags.d, word_host.data(), word_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_CHECK(sync_stream(st));
        score::GbmArgs a = pcg_args();
        a.tol2 = rel_tol * rel_tol;
        auto begin = [&](const score::GbmArgs& b) {
            hipLaunchKernelGGL(score::k_gb_pcg_begin, dim3((unsigned)n_ublocks), dim3(kThreads), 0, st, b, (const double*)rhs.d);
        };
        score::group_pcg(be(), a, pcg, 1, 4000, nullptr, begin, word_host);
        for (int g = 0; g < G; ++g) {
            if (!m[(size_t)g]) continue;
            ok[g] = word_host[(size_t)g] == 1 ? 1 : 0;
            used[g] = word_host[(size_t)(G + g)];
        }
    }
    // the caller's points become the members' current ones (X); returns the state as uploaded
    std::vector<double> set_point(const double* poses_in, const double* lms_in) {
        const int ps = U.pose_scalars(), d = U.dim;
        std::vector<double> h((size_t)U.state_size);
        for (const score::GbMember& M : U.members) {
            std::copy(poses_in + M.pose0, poses_in + M.pose0 + ps * M.Np, h.begin() + (std::ptrdiff_t)M.state0);
            if (M.Nl) std::copy(lms_in + M.lm0, lms_in + M.lm0 + d * M.Nl, h.begin() + (std::ptrdiff_t)(M.state0 + ps * M.Np));
        }
        staged_h2d(X.d, h.data(), h.size() * sizeof(double), stream());
        HIP_CHECK(sync_stream(stream()));
        return h;
    }
    void run(const double* poses_in, const double* lms_in, int max_iters, double tol, double* poses_out, double* lms_out,
             std::vector<score::LmState>& S) {
        std::vector<double> h = set_point(poses_in, lms_in);
        rounds = score::gb_lock_step(*this, U.count, max_iters, tol, 1e-9, S);
        read_points(h, poses_out, lms_out);
    }
    // the members' current points (X) in the caller's layout; h: scratch of the state's size
    void read_points(std::vector<double>& h, double* poses_out, double* lms_out) {
        const int ps = U.pose_scalars(), d = U.dim;
        staged_d2h(h.data(), X.d, h.size() * sizeof(double), stream());
        HIP_CHECK(sync_stream(stream()));
        for (const score::GbMember& M : U.members) {
            std::copy(h.begin() + (std::ptrdiff_t)M.state0, h.begin() + (std::ptrdiff_t)(M.state0 + ps * M.Np), poses_out + M.pose0);
            if (M.Nl) std::copy(h.begin() + (std::ptrdiff_t)(M.state0 + ps * M.Np), h.begin() + (std::ptrdiff_t)(M.state0 + ps * M.Np + d * M.Nl), lms_out + M.lm0);
        }
    }

    // ---- robust refinement: the hooks of gbr_lock_step (score_gn_robust_batch.hpp) ----
    // the measured precisions of member g's loop closures on the host (before robust_reserve: from U)
    void robust_host_precisions() {
        if (!rb_kappa0_host.empty() || U.lcs_size == 0) return;
        rb_kappa0_host.reserve((size_t)U.lcs_size); rb_tau0_host.reserve((size_t)U.lcs_size);
        for (const score::GbMember& M : U.members)
            for (long long q = 0; q < M.n_lc; ++q) {
                const size_t m = (size_t)(M.rel0 + (M.n_rel - M.n_lc) + q);
                rb_kappa0_host.push_back(U.rel_kappa[m]); rb_tau0_host.push_back(U.rel_tau[m]);
            }
    }
    void robust_check(const score_refine_robust_settings* rs, int n_settings) {
        if (n_settings != 1 && n_settings != U.count)
            throw std::runtime_error("score_refine_batch_robust_run: n_settings must be 1 or the number of members");
        robust_host_precisions();
        for (int g = 0; g < U.count; ++g) {
            const score::GbMember& M = U.members[(size_t)g];
            if ((rs[n_settings == 1 ? 0 : g].families & score::kGnRobustClosures) && U.lc_short[(size_t)g])
                throw std::runtime_error("score_refine_batch_robust_run: member " + std::to_string(g) +
                                         ": fewer relative-pose entries than odometry steps");
            score::gbr_check(rs[n_settings == 1 ? 0 : g], g, U.rng_prec.data() + M.rng0, M.n_rng, rb_kappa0_host.data() + M.lc0,
                             rb_tau0_host.data() + M.lc0, M.n_lc);
        }
    }
    void robust_reserve() {  // the buffers, from the handle's arena
        if (rb_ready) return;
        robust_host_precisions();
        ArenaScope arena_scope(&be().arena);
        tl_copy_stream = stream();
        const size_t nr = U.rng_prec.size(), nc = (size_t)U.lcs_size;
        rb_prec0.upload(U.rng_prec); rb_kappa0.upload(rb_kappa0_host); rb_tau0.upload(rb_tau0_host);
        rb_r_rng.alloc(nr); rb_w_rng.alloc(nr); rb_r_lc.alloc(nc); rb_w_lc.alloc(nc);
        rb_part.alloc((size_t)score::kGnRobustPart * U.rblk_member.size());
        rb_params.alloc((size_t)U.count);
        if (nr) rb_w_rng.zero(stream());  // (k_gbr_resid counts the non-binary weights of whatever was last written)
        if (nc) rb_w_lc.zero(stream());
        HIP_CHECK(sync_stream(stream()));
        rb_ready = true;
    }
    score::GbrDev robust_dev() const {
        score::GbrDev a{};
        a.d = dev();
        a.a = robust_arrays();
        a.params = rb_params.d;
        return a;
    }
    void robust_weights(const std::vector<char>& m, const score::GbrParam* params) {
        set_mask(m);
        HIP_CHECK(hipMemcpyAsync(rb_params.d, params, (size_t)U.count * sizeof(score::GbrParam), hipMemcpyHostToDevice, stream()));
        hipLaunchKernelGGL(score::k_gbr_weight, dim3((unsigned)U.rblk_member.size()), dim3(kThreads), 0, stream(), robust_dev(),
                           (const int32_t*)mask.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(sync_stream(stream()));  // (params is the caller's)
    }
    void robust_all(double mu, double min_weight, int32_t mode) {  // every member, both families
        const int both = score::kGnRobustRanges | score::kGnRobustClosures;
        std::vector<score::GbrParam> params((size_t)U.count, score::GbrParam{mu, 1.0, 1.0, min_weight, both, mode});
        robust_weights(std::vector<char>((size_t)U.count, 1), params.data());
    }
    void robust_begin() { robust_all(0.0, 1.0, score::kGbrNext); }
    void robust_restore() noexcept {
        if (!rb_ready) return;
        try { robust_all(0.0, 1.0, score::kGbrRestore); } catch (...) {}
    }
    void robust_residuals(const std::vector<char>& m, score::GncSeen* seen) {
        set_mask(m);
        const unsigned nb = (unsigned)U.rblk_member.size();
        score::gn_dim(U.dim, [&](auto dim) {
            hipLaunchKernelGGL(score::k_gbr_resid<decltype(dim)::value>, dim3(nb), dim3(kThreads), 0, stream(), robust_dev(), (const double*)X.d,
                               rb_part.d, (const int32_t*)mask.d);
        });
        HIP_CHECK(hipGetLastError());
        read_partials(rb_part, (size_t)score::kGnRobustPart * nb);
        for (int g = 0; g < U.count; ++g) {
            if (!m[(size_t)g]) continue;
            const score::GbMember& M = U.members[(size_t)g];
            double r2[2], nonbin[2];
            score::gn_robust_fold(part_host.data(), M.rblk0, M.rblk1, r2, nonbin);  // the member's partials in workgroup order
            seen[g].f[0] = score::RobustSeen{(int64_t)M.n_rng, r2[0], 0.0, (int32_t)nonbin[0]};
            seen[g].f[1] = score::RobustSeen{(int64_t)M.n_lc, r2[1], 0.0, (int32_t)nonbin[1]};
        }
    }
    // rs: one record per member
    void robust_run(const score_refine_robust_settings* rs, const double* poses_in, const double* lms_in, double* poses_out, double* lms_out,
                    double* w, double* r, double* wl, double* rl, bool keep, std::vector<score::LmState>& S, std::vector<score::GncState>& R,
                    std::vector<int32_t>& outliers, std::vector<int32_t>& rel_outliers) {
        robust_reserve();
        struct Restore {  // unless the weights are kept, the handle ends with the measured precisions
            score_refine_batch& h;
            bool armed = true;
            ~Restore() { if (armed) h.robust_restore(); }
        } restore{*this};
        std::vector<double> h = set_point(poses_in, lms_in);
        rounds = robust_rounds = score::gbr_lock_step(*this, U.count, rs, 1e-9, S, R, &stage_rounds);
        const std::vector<char> all((size_t)U.count, 1);
        std::vector<score::GncSeen> seen((size_t)U.count);
        robust_residuals(all, seen.data());  // every family's r at the final estimates
        std::vector<double> hw, hwl;
        robust_read(w, r, wl, rl, hw, hwl);
        outliers.assign((size_t)U.count, 0); rel_outliers.assign((size_t)U.count, 0);
        for (int g = 0; g < U.count; ++g) {
            const score::GbMember& M = U.members[(size_t)g];
            for (long long e = M.rng0; e < M.rng0 + M.n_rng; ++e) outliers[(size_t)g] += hw[(size_t)e] < 0.5 ? 1 : 0;
            if (rs[g].families & score::kGnRobustClosures)
                for (long long e = M.lc0; e < M.lc0 + M.n_lc; ++e) rel_outliers[(size_t)g] += hwl[(size_t)e] < 0.5 ? 1 : 0;
        }
        if (poses_out) read_points(h, poses_out, lms_out);
        if (keep) {
            robust_all(0.0, 1.0, score::kGbrKeep);
            restore.armed = false;
        }
    }
    void robust_inspect(const double* poses, const double* lms, const double* mu, const double* c, const double* c_rel, double* r, double* rl,
                        double* w, double* wl) {
        const int both = score::kGnRobustRanges | score::kGnRobustClosures;
        std::vector<score::GbrParam> params((size_t)U.count);
        for (int g = 0; g < U.count; ++g) {
            const std::string who = "score_refine_batch_residuals: member " + std::to_string(g);
            if (!(mu[g] >= 0.0) || !std::isfinite(mu[g])) throw std::runtime_error(who + ": mu must be finite and >= 0");
            if (mu[g] > 0.0 && !(std::isfinite(c[g]) && c[g] > 0.0 && std::isfinite(c_rel[g]) && c_rel[g] > 0.0))
                throw std::runtime_error(who + ": c and c_rel must be positive and finite when mu > 0");
            params[(size_t)g] = score::GbrParam{mu[g], c[g], c_rel[g], 1.0, both, score::kGbrInspect};
        }
        robust_reserve();
        (void)set_point(poses, lms);
        const std::vector<char> all((size_t)U.count, 1);
        std::vector<score::GncSeen> seen((size_t)U.count);
        robust_residuals(all, seen.data());
        robust_weights(all, params.data());
        std::vector<double> hw, hwl;
        robust_read(w, r, wl, rl, hw, hwl);
    }
};
