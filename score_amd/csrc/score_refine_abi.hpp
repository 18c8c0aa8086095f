// score_refine_abi.hpp -- the entry points of the two refinement handles (score_refine_handles.hpp): include/score_hip.h's
// score_refine_*, and score_refine_robust.h, score_marginals.h, score_spectrum.h, score_curvature.h, score_samples.h,
// score_leverage.h with their *_batch.h forms, score_relative.h with score_relative_batch.h, score_select.h with
// score_select_batch.h, and score_select_poses.h.  Part of score_hip.hip's translation unit, included there once after the
// handles: every entry point goes through the frame of score_abi.hpp (abi_call, require, publish_new).
#pragma once

namespace {

const char kNullArgument[] = "null argument";

// The frame of a call on a refinement handle: the handle stands (no_handle: the message when it does not), `refused` is null
// (an entry point's own refusal that comes before the points), the point is given -- poses, and landmarks where the handle
// has any (no_points: the message; null: the entry point checks its arguments itself, under the scope) -- then f() with the
// handle's device current.
template <class Handle, class F>
int refine_call(Handle* h, const char* no_handle, const double* poses, const double* landmarks, const char* no_points, F&& f,
                const char* refused = nullptr) {
    return abi_call([&] {
        require(h != nullptr, no_handle);
        require(refused == nullptr, refused);
        if (no_points) require(poses && (!h->has_landmarks() || landmarks), no_points);
        AbiEnv::Scope scope(h->device, false);
        return f();
    });
}
// a single handle's calls say "null argument" for everything
template <class F>
int refine_call(score_refine* r, const double* poses, const double* landmarks, F&& f) {
    return refine_call(r, kNullArgument, poses, landmarks, kNullArgument, f);
}

// the handle goes with its device current (its buffers and its linear-mode handle live there); then the caller's again
template <class Handle>
void destroy_on_device(Handle* h) {
    if (!h) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(h->device);
    delete h;
    if (prev >= 0) (void)hipSetDevice(prev);
}

// the info records of a refinement, from the states of score_refine_rule.hpp: a single handle's and a group member's alike
void fill_refine_info(score_refine_info& info, const score::LmState& run, double setup_ms, double solve_ms) {
    info.cost_initial = run.cost_initial; info.cost_final = run.f; info.grad_inf = run.gnorm;
    info.iterations = run.iterations; info.linear_solves = run.linear_solves; info.pcg_iters = run.pcg_iters;
    info.setup_ms = setup_ms; info.solve_ms = solve_ms;
}
void fill_refine_robust_info(score_refine_robust_info& info, const score::GncState& loop, const score::LmState& last_run,
                             int32_t outliers, int32_t rel_outliers, double setup_ms, double solve_ms) {
    info.outer_iterations = loop.k; info.converged = loop.converged ? 1 : 0;
    info.outliers = outliers; info.rel_outliers = rel_outliers; info.mu = loop.mu;
    info.lm_iterations = loop.lm_iterations; info.linear_solves = loop.linear_solves; info.pcg_iters = loop.pcg_iters;
    info.cost_initial = loop.cost_initial; info.cost_final = last_run.f; info.grad_inf = last_run.gnorm;
    info.setup_ms = setup_ms; info.solve_ms = solve_ms;
}

}  // namespace

extern "C" {

// ---- one graph ----
int score_refine_create(const score_graph* g, const score_settings* s, score_refine** out) {
    return abi_call([&] {
        require(g && out);
        const score_settings st = resolve_settings(s);
        AbiEnv::require_device(st.device);
        AbiEnv::Scope scope(st.device, false);  // the refinement's own buffers live on the handle's device too
        publish_new(out, [&](score_refine& r) { r.create(*g, s); });
        return 0;
    });
}
int score_refine_run(score_refine* r, const double* poses_in, const double* landmarks_in, int32_t max_iters, double tol,
                     double* poses_out, double* landmarks_out, score_refine_info* info) {
    return refine_call(r, poses_in, landmarks_in, [&] {
        require(poses_out && (!r->has_landmarks() || landmarks_out));
        const double t0 = score::now_ms();
        const score::LmState run = r->run(poses_in, landmarks_in, max_iters, tol, poses_out, landmarks_out);
        if (info) fill_refine_info(*info, run, r->setup_ms, score::now_ms() - t0);
        return 0;
    });
}
int score_refine_marginals(score_refine* r, const double* poses, const double* landmarks, const int32_t* vars, int32_t n_vars,
                           double rel_tol, int32_t max_iters, int32_t block_width, double* joint, double* residuals, int32_t* iters,
                           score_marginals_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        return score::mv_solve(*r, poses, landmarks, vars, n_vars, rel_tol, max_iters, block_width, joint, residuals, iters, info);
    });
}
int score_refine_samples(score_refine* r, const double* poses, const double* landmarks, uint64_t seed, int64_t first_sample,
                         int32_t n_samples, const int32_t* vars, int32_t n_vars, double rel_tol, int32_t max_iters, int32_t block_width,
                         double* moments, double* means, double* steps, double* rhs, double* noise, double* residuals, int32_t* iters,
                         score_samples_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        score::PsMoments use{vars, n_vars, moments, means, steps};
        return score::ps_solve(*r, "score_refine_samples: ", poses, landmarks, seed, first_sample, n_samples, rel_tol, max_iters, block_width,
                               rhs, noise, residuals, iters, info, use);
    });
}
int score_refine_leverage(score_refine* r, const double* poses, const double* landmarks, uint64_t seed, int64_t first_sample,
                          int32_t n_samples, const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, double rel_tol,
                          int32_t max_iters, int32_t block_width, double* lev_sum, double* lev_sq, double* red_sum, double* red_sq,
                          double* pair_sum, double* pair_sq, double* residuals, int32_t* iters, score_samples_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        score::LvMeasure use{pair_a, pair_b, n_pairs, lev_sum, lev_sq, red_sum, red_sq, pair_sum, pair_sq};
        return score::ps_solve(*r, "score_refine_leverage: ", poses, landmarks, seed, first_sample, n_samples, rel_tol, max_iters, block_width,
                               nullptr, nullptr, residuals, iters, info, use);
    });
}
int score_refine_range_variances(score_refine* r, const double* poses, const double* landmarks, const int32_t* pair_a,
                                 const int32_t* pair_b, int32_t n_pairs, double rel_tol, int32_t max_iters, int32_t block_width,
                                 double* variances, double* distances, double* residuals, int32_t* iters, double* solutions,
                                 score_marginals_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        score::LvPairOnly use;
        return score::lv_pair_solve(*r, "score_refine_range_variances: ", poses, landmarks, pair_a, pair_b, n_pairs, rel_tol, max_iters,
                                    block_width, variances, distances, residuals, iters, solutions, info, use);
    });
}
int score_refine_select_ranges(score_refine* r, const double* poses, const double* landmarks, const int32_t* pair_a, const int32_t* pair_b,
                               const double* precisions, int32_t n_pairs, int32_t k, double min_gain, double rel_tol, int32_t max_iters,
                               int32_t block_width, int32_t* order, double* gains, double* pick_variances, double* variances,
                               double* distances, double* remaining, double* residuals, int32_t* iters, double* matrix,
                               score_select_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        score::SelCross use{precisions, k, min_gain, score::SelOutputs{order, gains, pick_variances, remaining}, matrix, info};
        return score::lv_pair_solve(*r, "score_refine_select_ranges: ", poses, landmarks, pair_a, pair_b, n_pairs, rel_tol, max_iters,
                                    block_width, variances, distances, residuals, iters, nullptr, info ? &info->solve : nullptr, use);
    });
}
int score_select_greedy(const double* matrix, const double* precisions, const int32_t* excluded, int32_t n, int32_t k, double min_gain,
                        int32_t* order, double* gains, double* pick_variances, double* remaining, int32_t* picked, double* asymmetry) {
    return abi_call([&] {
        AbiEnv::require_device(0);
        AbiEnv::Scope scope(0, false);
        score::sel_greedy_alone(matrix, precisions, excluded, n, k, min_gain, score::SelOutputs{order, gains, pick_variances, remaining},
                                picked, asymmetry);
        return 0;
    });
}
int score_refine_relative_covariances(score_refine* r, const double* poses, const double* landmarks, const int32_t* pair_a,
                                      const int32_t* pair_b, int32_t n_pairs, double rel_tol, int32_t max_iters, int32_t block_width,
                                      double* rotations, double* translations, double* covariances, double* residuals, int32_t* iters,
                                      double* solutions, score_marginals_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        score::RpOnly use;
        return score::rp_solve(*r, "score_refine_relative_covariances: ", poses, landmarks, pair_a, pair_b, n_pairs, rel_tol, max_iters,
                               block_width, rotations, translations, covariances, residuals, iters, solutions, info, use);
    });
}
int score_refine_select_relative_poses(score_refine* r, const double* poses, const double* landmarks, const int32_t* pair_a,
                                       const int32_t* pair_b, const double* translation_precisions, const double* rotation_precisions,
                                       int32_t n_pairs, int32_t k, double min_gain, double rel_tol, int32_t max_iters, int32_t block_width,
                                       int32_t* order, double* gains, double* pick_covariances, double* rotations, double* translations,
                                       double* covariances, double* remaining, double* residuals, int32_t* iters, double* matrix,
                                       score_select_poses_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        score::SelpCross use{translation_precisions, rotation_precisions, k, min_gain,
                             score::SelpOutputs{order, gains, pick_covariances, remaining}, matrix, info, r->P.dim};
        return score::rp_solve(*r, "score_refine_select_relative_poses: ", poses, landmarks, pair_a, pair_b, n_pairs, rel_tol, max_iters,
                               block_width, rotations, translations, covariances, residuals, iters, nullptr, info ? &info->solve : nullptr,
                               use);
    });
}
int score_select_block_greedy(const double* matrix, const double* translation_precisions, const double* rotation_precisions,
                              const int32_t* excluded, int32_t n_candidates, int32_t dim, int32_t k, double min_gain, int32_t* order,
                              double* gains, double* pick_covariances, double* remaining, int32_t* picked, double* asymmetry) {
    return abi_call([&] {
        AbiEnv::require_device(0);
        AbiEnv::Scope scope(0, false);
        score::selp_greedy_alone(matrix, translation_precisions, rotation_precisions, excluded, n_candidates, dim, k, min_gain,
                                 score::SelpOutputs{order, gains, pick_covariances, remaining}, picked, asymmetry);
        return 0;
    });
}
int score_refine_spectrum(score_refine* r, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters,
                          double shift_rel, double* values, double* vectors, double* residuals, score_spectrum_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        return score::sp_solve(*r, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, info);
    });
}
int score_refine_hessian_product(score_refine* r, const double* poses, const double* landmarks, int32_t exact, const double* V,
                                 int32_t n_cols, double* out) {
    return refine_call(r, poses, landmarks, [&] {
        require(V && out);
        return score::cv_product(*r, poses, landmarks, exact, V, n_cols, out);
    });
}
int score_refine_curvature(score_refine* r, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters,
                           double shift_rel, double* values, double* vectors, double* residuals, double* gn_quotients,
                           score_curvature_info* info) {
    return refine_call(r, poses, landmarks, [&] {
        return score::cv_solve(*r, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, gn_quotients, info);
    });
}
void score_refine_robust_default_settings(score_refine_robust_settings* rs) {
    if (!rs) return;
    rs->inlier_threshold = 3.0; rs->rel_threshold = 3.0; rs->mu_step = 1.4; rs->min_weight = 1e-6;
    rs->families = 1; rs->max_outer = 50; rs->inner_iters = 5; rs->max_iters = 50; rs->tol = 1e-10;
}
int score_refine_robust_run(score_refine* r, const score_refine_robust_settings* rs, const double* poses_in, const double* landmarks_in,
                            double* poses_out, double* landmarks_out, double* weights, double* residuals, double* rel_weights,
                            double* rel_residuals, score_refine_robust_info* info) {
    return refine_call(r, poses_in, landmarks_in, [&] {
        require(!poses_out || !r->has_landmarks() || landmarks_out);
        const double t0 = score::now_ms();
        score_refine_robust_settings s;
        score_refine_robust_default_settings(&s);
        if (rs) s = *rs;
        score::GnRobustResult R;
        int32_t outliers = 0, rel_outliers = 0;
        r->robust_run(s, poses_in, landmarks_in, poses_out, landmarks_out, weights, residuals, rel_weights, rel_residuals, &outliers,
                      &rel_outliers, R);
        if (info) fill_refine_robust_info(*info, R.loop, R.run, outliers, rel_outliers, r->setup_ms, score::now_ms() - t0);
        return 0;
    });
}
int score_refine_residuals(score_refine* r, const double* poses, const double* landmarks, double mu, double c, double c_rel,
                           double* residuals, double* rel_residuals, double* weights, double* rel_weights) {
    return refine_call(r, poses, landmarks, [&] {
        r->robust_inspect(poses, landmarks, mu, c, c_rel, residuals, rel_residuals, weights, rel_weights);
        return 0;
    });
}
void score_refine_destroy(score_refine* r) { destroy_on_device(r); }

// ---- a group ----
int score_refine_batch_create(const score_graph* graphs, int32_t count, const score_settings* s, score_refine_batch** out) {
    return abi_call([&] {
        require(graphs && out);
        require(count > 0, "score_refine_batch_create: count must be positive");
        for (int32_t i = 1; i < count; ++i)
            require(graphs[i].dim == graphs[0].dim, "score_refine_batch_create: the graphs of a group must share dim");
        const score_settings st = resolve_settings(s);
        AbiEnv::require_device(st.device);
        AbiEnv::Scope scope(st.device, false);
        publish_new(out, [&](score_refine_batch& b) { b.create(graphs, count, s); });
        return 0;
    });
}
int score_refine_batch_run(score_refine_batch* b, const double* poses_in, const double* landmarks_in, int32_t max_iters, double tol,
                           double* poses_out, double* landmarks_out, score_refine_info* infos) {
    return refine_call(b, kNullArgument, poses_in, landmarks_in, kNullArgument, [&] {
        require(poses_out && (!b->has_landmarks() || landmarks_out));
        const double t0 = score::now_ms();
        std::vector<score::LmState> S;
        b->run(poses_in, landmarks_in, max_iters, tol, poses_out, landmarks_out, S);
        const double ms = score::now_ms() - t0;
        for (int g = 0; infos && g < b->U.count; ++g) fill_refine_info(infos[g], S[(size_t)g], b->setup_ms, ms);
        return 0;
    });
}
int score_refine_batch_marginals(score_refine_batch* b, const double* poses, const double* landmarks, const int32_t* var_ptr,
                                 const int32_t* vars, double rel_tol, int32_t max_iters, int32_t block_width, double* joint,
                                 double* residuals, int32_t* iters, score_marginals_batch_info* info) {
    return refine_call(b, "score_refine_batch_marginals: null handle", poses, landmarks, "score_refine_batch_marginals: the points are missing", [&] {
        return score::gbm_solve(*b, poses, landmarks, var_ptr, vars, rel_tol, max_iters, block_width, joint, residuals, iters, info);
    }, var_ptr ? nullptr : "score_refine_batch_marginals: var_ptr is null");
}
int score_refine_batch_samples(score_refine_batch* b, const double* poses, const double* landmarks, const uint64_t* seeds,
                               int64_t first_sample, const int32_t* n_samples, const int32_t* var_ptr, const int32_t* vars, double rel_tol,
                               int32_t max_iters, int32_t block_width, double* moments, double* means, double* steps, double* rhs,
                               double* noise, double* residuals, int32_t* iters, int32_t* determined, score_samples_batch_info* info) {
    return refine_call(b, "score_refine_batch_samples: null handle", poses, landmarks, "score_refine_batch_samples: the points are missing", [&] {
        score::GbsMoments use{var_ptr, vars, moments, means, steps};
        return score::gbs_solve(*b, "score_refine_batch_samples: ", poses, landmarks, seeds, first_sample, n_samples, rel_tol, max_iters,
                                block_width, rhs, noise, residuals, iters, determined, info, use);
    });
}
int score_refine_batch_leverage(score_refine_batch* b, const double* poses, const double* landmarks, const uint64_t* seeds,
                                int64_t first_sample, const int32_t* n_samples, const int32_t* pair_ptr, const int32_t* pair_a,
                                const int32_t* pair_b, double rel_tol, int32_t max_iters, int32_t block_width, double* lev_sum,
                                double* lev_sq, double* red_sum, double* red_sq, double* pair_sum, double* pair_sq, double* residuals,
                                int32_t* iters, int32_t* determined, score_samples_batch_info* info) {
    return refine_call(b, "score_refine_batch_leverage: null handle", poses, landmarks, "score_refine_batch_leverage: the points are missing", [&] {
        score::GblMeasure use{pair_ptr, pair_a, pair_b, lev_sum, lev_sq, red_sum, red_sq, pair_sum, pair_sq};
        return score::gbs_solve(*b, "score_refine_batch_leverage: ", poses, landmarks, seeds, first_sample, n_samples, rel_tol, max_iters,
                                block_width, nullptr, nullptr, residuals, iters, determined, info, use);
    });
}
int score_refine_batch_range_variances(score_refine_batch* b, const double* poses, const double* landmarks, const int32_t* pair_ptr,
                                       const int32_t* pair_a, const int32_t* pair_b, double rel_tol, int32_t max_iters,
                                       int32_t block_width, double* variances, double* distances, double* residuals, int32_t* iters,
                                       score_marginals_batch_info* info) {
    return refine_call(b, "score_refine_batch_range_variances: null handle", poses, landmarks,
                       "score_refine_batch_range_variances: the points are missing", [&] {
        score::GblPairOnly use;
        return score::gbl_pair_solve(*b, "score_refine_batch_range_variances: ", poses, landmarks, pair_ptr, pair_a, pair_b, rel_tol, max_iters,
                                     block_width, variances, distances, residuals, iters, info, use);
    });
}
int score_refine_batch_select_ranges(score_refine_batch* b, const double* poses, const double* landmarks, const int32_t* pair_ptr,
                                     const int32_t* pair_a, const int32_t* pair_b, const double* precisions, const int32_t* k,
                                     double min_gain, double rel_tol, int32_t max_iters, int32_t block_width, int32_t* order, double* gains,
                                     double* pick_variances, int32_t* picked, double* total_gains, double* variances, double* distances,
                                     double* remaining, double* residuals, int32_t* iters, double* matrix, score_select_batch_info* info) {
    return refine_call(b, "score_refine_batch_select_ranges: null handle", poses, landmarks,
                       "score_refine_batch_select_ranges: the points are missing", [&] {
        score::GbSelCross use{precisions, k, min_gain, score::GbSelOutputs{order, gains, pick_variances, remaining, picked, total_gains},
                              matrix, info};
        return score::gbl_pair_solve(*b, "score_refine_batch_select_ranges: ", poses, landmarks, pair_ptr, pair_a, pair_b, rel_tol, max_iters,
                                     block_width, variances, distances, residuals, iters, info ? &info->solve : nullptr, use);
    });
}
int score_refine_batch_relative_covariances(score_refine_batch* b, const double* poses, const double* landmarks, const int32_t* pair_ptr,
                                            const int32_t* pair_a, const int32_t* pair_b, double rel_tol, int32_t max_iters,
                                            int32_t block_width, double* rotations, double* translations, double* covariances,
                                            double* residuals, int32_t* iters, score_marginals_batch_info* info) {
    return refine_call(b, "score_refine_batch_relative_covariances: null handle", poses, landmarks,
                       "score_refine_batch_relative_covariances: the points are missing", [&] {
        return score::grp_solve(*b, poses, landmarks, pair_ptr, pair_a, pair_b, rel_tol, max_iters, block_width, rotations, translations,
                                covariances, residuals, iters, info);
    });
}
int score_refine_batch_spectrum(score_refine_batch* b, const double* poses, const double* landmarks, int32_t k, double rel_tol,
                                int32_t max_iters, double shift_rel, double* values, double* vectors, double* residuals,
                                int32_t* iterations, double* h_max, score_spectrum_batch_info* info) {
    return refine_call(b, "score_refine_batch_spectrum: null handle", poses, landmarks, "score_refine_batch_spectrum: the points are missing", [&] {
        return score::gsp_solve(*b, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, iterations, h_max, info);
    });
}
int score_spectrum_ritz(int32_t count, const double* GA, const double* GB, double* theta, double* coef, int32_t* status, int32_t* kept) {
    return abi_call([&] {
        AbiEnv::require_device(0);
        AbiEnv::Scope scope(0, false);
        score::gsp_ritz_alone(count, GA, GB, theta, coef, status, kept);
        return 0;
    });
}
int score_refine_batch_hessian_product(score_refine_batch* b, const double* poses, const double* landmarks, int32_t exact, const double* V,
                                       int32_t n_cols, double* out) {
    return refine_call(b, "score_refine_batch_hessian_product: null handle", poses, landmarks,
                       "score_refine_batch_hessian_product: the points are missing", [&] {
        require(V && out, "score_refine_batch_hessian_product: V and out are missing");
        return score::gbc_product(*b, poses, landmarks, exact, V, n_cols, out);
    });
}
int score_refine_batch_curvature(score_refine_batch* b, const double* poses, const double* landmarks, int32_t k, double rel_tol,
                                 int32_t max_iters, double shift_rel, double* values, double* vectors, double* residuals,
                                 double* gn_quotients, int32_t* iterations, double* h_max, double* c_max,
                                 score_curvature_batch_info* info) {
    return refine_call(b, "score_refine_batch_curvature: null handle", poses, landmarks, "score_refine_batch_curvature: the points are missing", [&] {
        return score::gbc_solve(*b, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, gn_quotients, iterations,
                                h_max, c_max, info);
    });
}
int score_curvature_ritz(int32_t count, const double* GA, const double* GB, double* theta, double* coef, int32_t* status, int32_t* kept) {
    return abi_call([&] {
        AbiEnv::require_device(0);
        AbiEnv::Scope scope(0, false);
        score::gsp_ritz_alone(count, GA, GB, theta, coef, status, kept, true, "score_curvature_ritz: ");
        return 0;
    });
}
int score_refine_batch_robust_run(score_refine_batch* b, const score_refine_robust_settings* rs, int32_t n_settings, const double* poses_in,
                                  const double* landmarks_in, double* poses_out, double* landmarks_out, double* weights, double* residuals,
                                  double* rel_weights, double* rel_residuals, int32_t keep_weights, score_refine_robust_info* infos) {
    return refine_call(b, "score_refine_batch_robust_run: null handle", nullptr, nullptr, nullptr, [&] {
        try {   // (host only: nothing on the device is touched before the arguments and the settings stand)
            require(rs != nullptr, "score_refine_batch_robust_run: the settings are missing");
            require(poses_in && (!b->has_landmarks() || landmarks_in), "score_refine_batch_robust_run: the points are missing");
            require(!poses_out || !b->has_landmarks() || landmarks_out, "score_refine_batch_robust_run: landmarks_out is missing");
            b->robust_check(rs, n_settings);
        } catch (...) {
            b->robust_restore();               // (weights a previous call kept do not survive an error return)
            throw;
        }
        const double t0 = score::now_ms();
        std::vector<score_refine_robust_settings> per((size_t)b->U.count);
        for (int g = 0; g < b->U.count; ++g) per[(size_t)g] = rs[n_settings == 1 ? 0 : g];
        std::vector<score::LmState> S;
        std::vector<score::GncState> R;
        std::vector<int32_t> outliers, rel_outliers;
        b->robust_run(per.data(), poses_in, landmarks_in, poses_out, landmarks_out, weights, residuals, rel_weights, rel_residuals,
                      keep_weights != 0, S, R, outliers, rel_outliers);
        const double ms = score::now_ms() - t0;
        for (int g = 0; infos && g < b->U.count; ++g)
            fill_refine_robust_info(infos[g], R[(size_t)g], S[(size_t)g], outliers[(size_t)g], rel_outliers[(size_t)g], b->setup_ms, ms);
        return 0;
    });
}
int score_refine_batch_residuals(score_refine_batch* b, const double* poses, const double* landmarks, const double* mu, const double* c,
                                 const double* c_rel, double* residuals, double* rel_residuals, double* weights, double* rel_weights) {
    return refine_call(b, "score_refine_batch_residuals: null handle", poses, landmarks, "score_refine_batch_residuals: the points are missing", [&] {
        require(mu && c && c_rel, "score_refine_batch_residuals: mu, c and c_rel take one entry per member");
        b->robust_inspect(poses, landmarks, mu, c, c_rel, residuals, rel_residuals, weights, rel_weights);
        return 0;
    });
}
int score_refine_batch_restore(score_refine_batch* b) {
    return refine_call(b, "score_refine_batch_restore: null handle", nullptr, nullptr, nullptr, [&] {
        if (b->rb_ready) b->robust_all(0.0, 1.0, score::kGbrRestore);
        return 0;
    });
}
int score_refine_batch_robust_rounds(score_refine_batch* b, int32_t* rounds, int32_t* stage_rounds) {
    return abi_call([&] {
        require(b != nullptr, "score_refine_batch_robust_rounds: null handle");
        if (rounds) *rounds = b->robust_rounds;
        if (stage_rounds) *stage_rounds = b->stage_rounds;
        return 0;
    });
}
void score_refine_batch_destroy(score_refine_batch* b) { destroy_on_device(b); }

}  // extern "C"
