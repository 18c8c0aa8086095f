// score_robust_driver.hpp -- the host half of score_robust_solve_rel (include/score_robust.h): the GNC-TLS outer loop.  The graphs'
// measurement arrays go up once ("home" arrays, graph after graph); every outer solve's handle is built from compact copies of
// the running members' arrays through the generator's path (GenSource), with the weighted precisions the weight kernels wrote
// (score_robust.hpp).  The create path's host fallback (the host assembler) reads the precisions from the views: they point at
// host mirrors of the same values.  A re-weighted family is one RobustFamilyHost record; the loop runs over the records.
// Included by score_hip.hip where score_create_from_graphs_impl and the abi frame are complete.
#pragma once

#include "score_slab.hpp"  // Slab, Region: one allocation cut into typed regions (256-byte aligned, 8 bytes at least)

struct RobustHandle { score_handle* h = nullptr; ~RobustHandle() { if (h) score_destroy(h); } };  // (an outer solve's handle goes whatever happens)
struct StreamBack { int dev; hipStream_t s; ~StreamBack() { (void)sync_stream(s); stream_pool().give(dev, s); } };
struct PinBack { char* p; size_t n; int dev; ~PinBack() { block_cache().give(p, n, dev, true); } };

struct MeasRegions {  // the measurement arrays of score_graph: home (graph after graph) and compact (the running members)
    Region<int32_t> rel_base, rel_to, rng_a, rng_b; Region<double> rel_t, rel_R, rel_kappa, rel_tau, rng_dist, prec;
    void declare(Slab& s, size_t n_rel, size_t n_rng, size_t d) {
        rel_base = s.add<int32_t>(n_rel); rel_to = s.add<int32_t>(n_rel); rel_t = s.add<double>(n_rel * d); rel_R = s.add<double>(n_rel * d * d);
        rel_kappa = s.add<double>(n_rel); rel_tau = s.add<double>(n_rel);
        rng_a = s.add<int32_t>(n_rng); rng_b = s.add<int32_t>(n_rng); rng_dist = s.add<double>(n_rng); prec = s.add<double>(n_rng);
    }
    void put(char* base, const score_graph& g, size_t eo, size_t ro, size_t d) const {  // graph g at entries eo / ro
        const size_t ne = (size_t)g.n_rel, nr = (size_t)g.n_rng;
        auto cp = [](auto* dst, const auto* src, size_t n) { if (n) std::memcpy(dst, src, n * sizeof(*dst)); };
        cp(rel_base.in(base) + eo, g.rel_base, ne); cp(rel_to.in(base) + eo, g.rel_to, ne);
        cp(rel_t.in(base) + eo * d, g.rel_t, ne * d); cp(rel_R.in(base) + eo * d * d, g.rel_R, ne * d * d);
        cp(rel_kappa.in(base) + eo, g.rel_kappa, ne); cp(rel_tau.in(base) + eo, g.rel_tau, ne);
        cp(rng_a.in(base) + ro, g.rng_a, nr); cp(rng_b.in(base) + ro, g.rng_b, nr); cp(rng_dist.in(base) + ro, g.rng_dist, nr); cp(prec.in(base) + ro, g.rng_prec, nr);
    }
    HipBackend::GenSource source(char* base) const {
        return HipBackend::GenSource{rel_base.in(base), rel_to.in(base), rel_t.in(base), rel_R.in(base), rel_kappa.in(base), rel_tau.in(base),
                                     rng_a.in(base), rng_b.in(base), rng_dist.in(base), prec.in(base)};
    }
};

struct RobustFamilyKind {  // what a family is, whoever calls
    int slot;               // its control records: [slot * count, (slot + 1) * count) of RobustRun::ctl
    // the precisions its weight scales are n_prec arrays of score_graph, mirrored whole on the host (the views of the next
    // handle point into the mirrors); the family's items are the trailing entries of every graph's part of them
    int n_prec; const double* score_graph::* measured[2];
    int32_t score_robust_info::* outliers;   // the counter it fills
    const char* api; const char* item;       // for its error texts
};
static const RobustFamilyKind kRobustRanges = {0, 1, {&score_graph::rng_prec, nullptr}, &score_robust_info::outliers, "score_robust_solve", "range"};
static const RobustFamilyKind kRobustClosures = {1, 2, {&score_graph::rel_kappa, &score_graph::rel_tau}, &score_robust_info::rel_outliers, "score_robust_solve_rel", "loop closure"};

struct RobustFamilyHost : RobustFamilyKind {  // one re-weighted family of measurements in one call
    explicit RobustFamilyHost(const RobustFamilyKind& kind) : RobustFamilyKind(kind) {}
    bool present = false;   // it has regions, its residual kernel runs and its residuals are reported (the ranges: always)
    bool reweigh = false;   // its bit of `families`: its weight kernel runs, its weights are carried, it takes part in the stop rule
    double c = 0.0;         // inlier threshold
    std::vector<double> mirror[2], w_host;   // the host's precisions (whole arrays) and weights of the solve under way
    std::vector<int64_t> off, arr_off;       // count + 1: the graphs' first items; the graphs' first entries of the mirrored arrays
    double* weights_out = nullptr; double* resid_out = nullptr;   // the caller's (null: not wanted)
    int64_t n_compact = 0;                   // items of the running members
    Region<double> w, w_next, resid, next[2]; Region<int32_t> home_off, tab_off;   // w, home_off: home; tab_off: tables; the rest: read-back

    int64_t total() const { return off.back(); }
    int64_t items(int m) const { return off[(size_t)m + 1] - off[(size_t)m]; }
    int64_t mirror_at(int m) const { return arr_off[(size_t)m + 1] - items(m); }
};

struct RobustRun {  // one score_robust_solve_rel call: the arguments, the layout, the memory, the host's state; the phases in order
    const score_graph* graphs; int count; const score_robust_settings* rs; score_settings st;
    double* poses; double* relaxed; double* landmarks; double* ranges; int32_t* degenerate; score_info* infos;
    int d = 0, qdirs = 0;
    std::vector<int64_t> rel_off, pose_off, lm_off;   // count + 1
    RobustFamilyHost fam[2] = {RobustFamilyHost(kRobustRanges), RobustFamilyHost(kRobustClosures)};
    RobustFamilyHost &rng = fam[0], &lc = fam[1];
    Slab home_s, work_s, back_s, tab_s;               // home arrays (up once), compact work arrays, the read-back block, per-iteration tables
    MeasRegions hm, wm;                               // home, compact
    Region<double> mu_in, mu_out; Region<int32_t> home_rel_off, t_member, t_rel;   // home | read-back | home, tables
    Region<RobustCtl> ctl;                            // read-back: count records per present family
    size_t n_ctl() const { return (size_t)rng.present + (size_t)lc.present; }
    char *home = nullptr, *work = nullptr, *back = nullptr, *back_h = nullptr, *tab = nullptr;   // back_h: the pinned copy of back
    EstProb* d_probs = nullptr; double* d_D = nullptr; size_t d_D_cap = 0;   // (d_D: a handle whose scales live on the host: SCORE_HOST_SETUP and friends)
    DevArena ar; hipStream_t rsm = nullptr;
    std::vector<double> mu_host; std::vector<score_robust_info> rec; std::vector<int> active; double t0 = 0.0;

    // ---- 1. the arguments: settings, the families, the graphs' layout, the slabs ----
    void validate(const score_settings* s, int32_t families, double rel_threshold) {
        if (!graphs || !rs || count <= 0) throw std::runtime_error("score_robust_solve: null argument or count < 1");
        if (families < 1 || families > 3) throw std::runtime_error("score_robust_solve_rel: families must be 1 (ranges), 2 (loop closures) or 3 (both)");
        rng.present = true; rng.reweigh = (families & 1) != 0; lc.present = lc.reweigh = (families & 2) != 0;
        rng.c = rs->inlier_threshold; lc.c = lc.reweigh ? rel_threshold : 0.0;
        if (lc.reweigh && (!(lc.c > 0.0) || !std::isfinite(lc.c))) throw std::runtime_error("score_robust_solve_rel: rel_threshold must be positive and finite");
        if (!(rng.c > 0.0) || !std::isfinite(rng.c)) throw std::runtime_error("score_robust_solve: inlier_threshold must be positive and finite");
        if (!(rs->mu_step > 1.0) || !std::isfinite(rs->mu_step)) throw std::runtime_error("score_robust_solve: mu_step must be finite and > 1");
        if (!(rs->min_weight > 0.0 && rs->min_weight <= 1.0)) throw std::runtime_error("score_robust_solve: min_weight must lie in (0, 1]");
        if (rs->max_outer < 1) throw std::runtime_error("score_robust_solve: max_outer must be >= 1");
        st = resolve_settings(s); d = graphs[0].dim;
        if (d != 2 && d != 3) throw std::runtime_error("score_robust_solve: dim must be 2 or 3");
    }
    void layout() {
        const size_t c = (size_t)count;
        qdirs = rs->qcqp_directions ? 1 : 0;
        rel_off.assign(c + 1, 0); pose_off.assign(c + 1, 0); lm_off.assign(c + 1, 0);
        for (RobustFamilyHost& F : fam) { F.off.assign(c + 1, 0); F.arr_off.assign(c + 1, 0); }
        for (size_t p = 0; p < c; ++p) {
            const score_graph& g = graphs[p];
            if (g.dim != d) throw std::runtime_error("score_robust_solve: graphs of one dimension only");
            if (g.relaxation == 1) qdirs = 1;
            else if (g.relaxation != 0) throw std::runtime_error("score_robust_solve: relaxation must be 0 (SOCP) or 1 (QCQP)");
            int64_t Np = 0;
            for (int ch = 0; ch < g.n_chains; ++ch) Np += g.chain_len[ch];
            // a family's items: the entries of its arrays behind a fixed head (the loop closures: behind the odometry steps)
            const int64_t n_arr[2] = {g.n_rng, g.n_rel}, head[2] = {0, Np - g.n_chains};
            for (int f = 0; f < 2; ++f) {
                RobustFamilyHost& F = fam[f];
                const int64_t n = F.present ? n_arr[f] - head[f] : 0;
                if (n < 0) throw std::runtime_error("score_robust_solve_rel: graph " + std::to_string(p) + " has fewer relative-pose entries than odometry steps");
                for (int64_t e = 0; e < n; ++e)
                    for (int k = 0; k < F.n_prec; ++k) {
                        const double v = (g.*F.measured[k])[n_arr[f] - n + e];
                        if (!(v > 0.0) || !std::isfinite(v))
                            throw std::runtime_error(std::string(F.api) + ": graph " + std::to_string(p) + ": " + F.item + " " + std::to_string(e) +
                                                     " has a precision that is not positive and finite");
                    }
                F.off[p + 1] = F.off[p] + n; F.arr_off[p + 1] = F.arr_off[p] + n_arr[f];
            }
            rel_off[p + 1] = rel_off[p] + g.n_rel; pose_off[p + 1] = pose_off[p] + Np; lm_off[p + 1] = lm_off[p] + g.n_landmarks;
        }
        if (rel_off[c] >= ((int64_t)1 << 31) || rng.total() >= ((int64_t)1 << 31)) throw std::runtime_error("score_robust_solve: too many measurements");
        hm.declare(home_s, (size_t)rel_off[c], (size_t)rng.total(), (size_t)d);
        wm.declare(work_s, (size_t)rel_off[c], (size_t)rng.total(), (size_t)d);
        mu_in = home_s.add<double>(c); home_rel_off = home_s.add<int32_t>(c + 1);
        mu_out = back_s.add<double>(c); ctl = back_s.add<RobustCtl>(c * n_ctl());
        t_member = tab_s.add<int32_t>(c); t_rel = tab_s.add<int32_t>(c + 1);
        for (RobustFamilyHost& F : fam) {
            if (!F.present) continue;   // (an absent family has no region: with the ranges alone the read-back block is the ranges')
            const size_t n = (size_t)F.total();
            F.w = home_s.add<double>(n); F.home_off = home_s.add<int32_t>(c + 1); F.tab_off = tab_s.add<int32_t>(c + 1);
            F.w_next = back_s.add<double>(n); F.resid = back_s.add<double>(n);
            for (int k = 0; k < F.n_prec; ++k) F.next[k] = back_s.add<double>(n);
        }
    }

    // ---- 2. the home arrays go up; the host's weights, precision mirrors, mu and records start ----
    void upload_home() {
        std::vector<char> hp(home_s.bytes, 0);
        for (int p = 0; p < count; ++p) hm.put(hp.data(), graphs[p], (size_t)rel_off[(size_t)p], (size_t)rng.off[(size_t)p], (size_t)d);
        for (int p = 0; p <= count; ++p) home_rel_off.in(hp.data())[p] = (int32_t)rel_off[(size_t)p];
        for (RobustFamilyHost& F : fam) {
            if (!F.present) continue;
            std::fill(F.w.in(hp.data()), F.w.in(hp.data()) + F.total(), 1.0);
            for (int p = 0; p <= count; ++p) F.home_off.in(hp.data())[p] = (int32_t)F.off[(size_t)p];
            F.w_host.assign((size_t)F.total(), 1.0);
            for (int k = 0; k < F.n_prec; ++k) {
                F.mirror[k].resize((size_t)F.arr_off.back());
                for (int p = 0; p < count; ++p)
                    if (const int64_t n = F.arr_off[(size_t)p + 1] - F.arr_off[(size_t)p])
                        std::memcpy(F.mirror[k].data() + F.arr_off[(size_t)p], graphs[p].*F.measured[k], (size_t)n * sizeof(double));
            }
        }
        home = (char*)ar.take(home_s.bytes);
        staged_h2d(home, hp.data(), home_s.bytes, rsm);
        work = (char*)ar.take(work_s.bytes); back = (char*)ar.take(back_s.bytes); tab = (char*)ar.take(tab_s.bytes);
        d_probs = (EstProb*)ar.take((size_t)count * sizeof(EstProb));
        mu_host.assign((size_t)count, 0.0); rec.assign((size_t)count, score_robust_info{});
        for (int p = 0; p < count; ++p) active.push_back(p);
    }

    // ---- 3.1 the running members: their views, their tables, and (after a member left, or before the first solve) their
    //          arrays compacted: k == 1: the measured precisions; later: those the last weight kernels wrote ----
    std::vector<score_graph> compact(int k, bool changed) {
        const int na = (int)active.size();
        std::vector<score_graph> views((size_t)na);
        std::vector<char> tb(tab_s.bytes, 0);
        int64_t nrel_c = 0;
        for (RobustFamilyHost& F : fam) F.n_compact = 0;
        for (int j = 0; j < na; ++j) {
            const int m = active[(size_t)j];
            score_graph& v = views[(size_t)j] = graphs[m]; v.relaxation = 0;
            t_member.in(tb.data())[j] = m; t_rel.in(tb.data())[j] = (int32_t)nrel_c;
            nrel_c += graphs[m].n_rel;
            for (RobustFamilyHost& F : fam) {
                if (!F.present) continue;
                for (int q = 0; q < F.n_prec; ++q) v.*F.measured[q] = F.mirror[q].data() + F.arr_off[(size_t)m];
                F.tab_off.in(tb.data())[j] = (int32_t)F.n_compact;
                F.n_compact += F.items(m);
            }
        }
        t_rel.in(tb.data())[na] = (int32_t)nrel_c;
        for (RobustFamilyHost& F : fam)
            if (F.present) F.tab_off.in(tb.data())[na] = (int32_t)F.n_compact;
        if (changed) {
            staged_h2d(tab, tb.data(), tab_s.bytes, rsm);
            const HipBackend::GenSource h = hm.source(home);
            RobustGatherArgs ga{};
            ga.d = d; ga.count = na; ga.with_static = 1;
            ga.member = t_member.in(tab); ga.rel_off = t_rel.in(tab); ga.rng_off = rng.tab_off.in(tab);
            ga.home_rel_off = home_rel_off.in(home); ga.home_rng_off = rng.home_off.in(home);
            ga.n_rel = nrel_c; ga.n_rng = rng.n_compact;
            ga.h_rel_base = h.rel_base; ga.h_rel_to = h.rel_to; ga.h_rel_t = h.rel_t; ga.h_rel_R = h.rel_R; ga.h_rel_kappa = h.rel_kappa; ga.h_rel_tau = h.rel_tau;
            ga.h_rng_a = h.rng_a; ga.h_rng_b = h.rng_b; ga.h_rng_dist = h.rng_dist;
            ga.h_prec = k > 1 && rng.reweigh ? rng.next[0].in(back) : h.rng_prec;
            if (k > 1 && lc.reweigh) { ga.home_lc_off = lc.home_off.in(home); ga.h_kappa_next = lc.next[0].in(back); ga.h_tau_next = lc.next[1].in(back); }
            ga.rel_base = wm.rel_base.in(work); ga.rel_to = wm.rel_to.in(work); ga.rel_t = wm.rel_t.in(work); ga.rel_R = wm.rel_R.in(work);
            ga.rel_kappa = wm.rel_kappa.in(work); ga.rel_tau = wm.rel_tau.in(work);
            ga.rng_a = wm.rng_a.in(work); ga.rng_b = wm.rng_b.in(work); ga.rng_dist = wm.rng_dist.in(work); ga.prec = wm.prec.in(work);
            const int64_t nmax = std::max(nrel_c, rng.n_compact);
            if (nmax > 0) hipLaunchKernelGGL(k_robust_gather, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, rsm, ga);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(sync_stream(rsm));   // (unchanged members: the weight kernels wrote the compact precisions already)
        return views;
    }

    // ---- 3.2 the outer solve ----
    std::vector<score_info> create_and_solve(const std::vector<score_graph>& views, RobustHandle& rh) {
        const HipBackend::GenSource src = wm.source(work);
        if (score_create_from_graphs_impl(views.data(), (int)views.size(), &st, &rh.h, &src) != 0) throw std::runtime_error(std::string(g_err));
        std::vector<score_info> inf(views.size());
        if (score_solve(rh.h, nullptr, nullptr, nullptr, inf.data()) < 0) throw std::runtime_error(std::string(g_err));
        if (rh.h->solver.est.probs.size() != views.size()) throw std::runtime_error("score_robust_solve: handle layout does not match the members");
        return inf;
    }

    // ---- 3.3 residuals, weights and control records from the solution on the device; one read ----
    void reweigh(int k, score_handle* h) {
        auto& S = h->solver; hipStream_t hs = S.be.stream;
        staged_h2d(d_probs, S.est.probs.data(), active.size() * sizeof(EstProb), hs);
        RobustShared s{};
        s.d = d; s.count = (int)active.size(); s.first = k == 1 ? 1 : 0;
        s.probs = d_probs; s.member = t_member.in(tab); s.x = S.be.xy.d; s.D = S.be.Dd.d;
        if (!S.H.device_setup) {
            const size_t need = (size_t)S.H.n_tot;
            if (need > d_D_cap) { d_D = (double*)ar.take(need * sizeof(double)); d_D_cap = need; }
            staged_h2d(d_D, S.H.D.data(), need * sizeof(double), hs);
            s.D = d_D;
        }
        s.mu_in = mu_in.in(home); s.mu_out = mu_out.in(back); s.mu_step = rs->mu_step; s.min_weight = rs->min_weight;
        auto common = [&](RobustFamily& f, const RobustFamilyHost& F, const RobustFamilyHost& other) {
            f.off = F.tab_off.in(tab); f.home_off = F.home_off.in(home); f.n = F.n_compact;
            f.w = F.w.in(home); f.resid = F.resid.in(back); f.w_next = F.w_next.in(back);
            f.ctl = ctl.in(back) + (size_t)F.slot * count; f.ctl_other = other.reweigh ? ctl.in(back) + (size_t)other.slot * count : nullptr;
            f.c = F.c; f.c_other = other.c;
        };
        RobustRanges fr{}; common(fr, rng, lc);
        fr.a = wm.rng_a.in(work); fr.b = wm.rng_b.in(work); fr.dist = wm.rng_dist.in(work);
        fr.prec = hm.prec.in(home); fr.prec_next = rng.next[0].in(back); fr.prec_work = wm.prec.in(work);
        RobustClosures fc{}; common(fc, lc, rng);   // (an absent family: n = 0, never launched)
        fc.rel_off = t_rel.in(tab); fc.home_rel_off = home_rel_off.in(home);
        fc.rel_base = wm.rel_base.in(work); fc.rel_to = wm.rel_to.in(work); fc.rel_t = wm.rel_t.in(work); fc.rel_R = wm.rel_R.in(work);
        fc.kappa = hm.rel_kappa.in(home); fc.tau = hm.rel_tau.in(home); fc.kappa_next = lc.next[0].in(back); fc.tau_next = lc.next[1].in(back);
        fc.kappa_work = wm.rel_kappa.in(work); fc.tau_work = wm.rel_tau.in(work);
        HIP_CHECK(hipMemsetAsync(ctl.in(back), 0, (size_t)count * sizeof(RobustCtl) * n_ctl(), hs));
        // every family's residuals before any family's weights: the first mu needs all the maxima.  A family that is present
        // but not re-weighted has its residuals reported all the same
        auto launch = [&](auto kernel, const auto& f, bool runs) {
            if (runs && f.n > 0) hipLaunchKernelGGL(kernel, dim3((unsigned)((f.n + 255) / 256)), dim3(256), 0, hs, RobustArgs<std::decay_t<decltype(f)>>{s, f});
        };
        launch(k_robust_resid<RobustRanges>, fr, rng.present); launch(k_robust_resid<RobustClosures>, fc, lc.present);
        launch(k_robust_weight<RobustRanges>, fr, rng.reweigh); launch(k_robust_weight<RobustClosures>, fc, lc.reweigh);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(back_h, back, back_s.bytes, hipMemcpyDeviceToHost, hs));
        HIP_CHECK(sync_stream(hs));
    }

    // ---- 3.4 + 3.5 per running member: go on (the host's weights, mirrors and mu follow the device) or stop (its record, its
    //          weights and residuals to the caller); returns the handle positions of the members that stopped ----
    std::vector<int> sort_members(int k, const std::vector<score_info>& inf, std::vector<int>& next) {
        std::vector<int> stop_j;
        for (int j = 0; j < (int)active.size(); ++j) {
            const int m = active[(size_t)j];
            RobustSeen seen[2]; int n_seen = 0;
            for (const RobustFamilyHost& F : fam) {
                if (!F.reweigh) continue;
                const RobustCtl& C = ctl.in(back_h)[(size_t)F.slot * count + m];
                RobustSeen& s = seen[n_seen++] = RobustSeen{F.items(m), 0.0, F.c, C.nonbinary};
                std::memcpy(&s.r2max, &C.r2max, sizeof(double));
            }
            const RobustNext what = robust_decide(k, rs->max_outer, seen, n_seen);
            score_robust_info& I = rec[(size_t)m];
            I.setup_ms += inf[(size_t)j].setup_ms; I.solve_ms += inf[(size_t)j].solve_ms;
            for (RobustFamilyHost& F : fam) {
                const int64_t i0 = F.off[(size_t)m], n = F.items(m);
                if (what == RobustNext::go && F.reweigh && n) {
                    std::memcpy(F.w_host.data() + i0, F.w_next.in(back_h) + i0, (size_t)n * sizeof(double));
                    for (int q = 0; q < F.n_prec; ++q) std::memcpy(F.mirror[q].data() + F.mirror_at(m), F.next[q].in(back_h) + i0, (size_t)n * sizeof(double));
                }
                if (what == RobustNext::go) continue;
                I.*F.outliers = 0;
                for (int64_t e = 0; e < n; ++e) I.*F.outliers += F.w_host[(size_t)(i0 + e)] < 0.5 ? 1 : 0;
                if (F.weights_out && n) std::memcpy(F.weights_out + i0, F.w_host.data() + i0, (size_t)n * sizeof(double));
                if (F.resid_out && n) std::memcpy(F.resid_out + i0, F.resid.in(back_h) + i0, (size_t)n * sizeof(double));
            }
            if (what == RobustNext::go) { next.push_back(m); mu_host[(size_t)m] = mu_out.in(back_h)[m]; continue; }
            stop_j.push_back(j);
            I.outer_iterations = k; I.converged = what == RobustNext::converged ? 1 : 0; I.mu = mu_host[(size_t)m];
            I.total_ms = score::now_ms() - t0;
            if (infos) infos[m] = inf[(size_t)j];
        }
        return stop_j;
    }

    // ---- 3.5 the estimates of the members that stopped ----
    void copy_estimates(const std::vector<int>& stop_j, score_handle* h) {
        if (stop_j.empty() || !(poses || relaxed || landmarks || ranges || degenerate)) return;
        auto& S = h->solver;
        const EstLayout& L = S.est;
        const int D1 = d + 1, rw = qdirs ? d : 1;
        const size_t f8 = sizeof(double);
        std::vector<double> T((size_t)L.n_pose * D1 * D1), B((size_t)L.n_pose * d * D1), Lm((size_t)std::max<int64_t>(1, L.n_lm) * d),
            Rg((size_t)std::max<int64_t>(1, L.n_rng) * rw);
        std::vector<int32_t> F((size_t)L.n_pose);
        {
            ActiveSolve act;
            S.be.read_estimates(S.H, L, qdirs, T.data(), B.data(), Lm.data(), Rg.data(), F.data());
        }
        for (int j : stop_j) {
            const int m = active[(size_t)j];
            const EstProb& P = L.probs[(size_t)j];
            const size_t po = (size_t)pose_off[(size_t)m], lo = (size_t)lm_off[(size_t)m], ro = (size_t)rng.off[(size_t)m];
            if (poses) std::memcpy(poses + po * D1 * D1, T.data() + (size_t)P.pose_off * D1 * D1, (size_t)P.Np * D1 * D1 * f8);
            if (relaxed) std::memcpy(relaxed + po * d * D1, B.data() + (size_t)P.pose_off * d * D1, (size_t)P.Np * d * D1 * f8);
            if (landmarks && P.Nl) std::memcpy(landmarks + lo * d, Lm.data() + (size_t)P.lm_off * d, (size_t)P.Nl * d * f8);
            if (ranges && P.Nr) std::memcpy(ranges + ro * rw, Rg.data() + (size_t)P.rng_off * rw, (size_t)P.Nr * rw * f8);
            if (degenerate) std::memcpy(degenerate + po, F.data() + P.pose_off, (size_t)P.Np * sizeof(int32_t));
        }
    }

    // ---- 3.6 the next solve's weights and mu on the device (members that stopped are not read again) ----
    void carry(hipStream_t hs) {
        for (const RobustFamilyHost& F : fam)
            if (F.reweigh && F.total())
                HIP_CHECK(hipMemcpyAsync(F.w.in(home), F.w_next.in(back), (size_t)F.total() * sizeof(double), hipMemcpyDeviceToDevice, hs));
        HIP_CHECK(hipMemcpyAsync(mu_in.in(home), mu_out.in(back), (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, hs));
        HIP_CHECK(sync_stream(hs));
    }

    int solve(const score_settings* s, int32_t families, double rel_threshold, score_robust_info* rinfos) {
        validate(s, families, rel_threshold);
        layout();
        AbiEnv::require_device(st.device);
        DeviceGuard guard(st.device);
        t0 = score::now_ms();
        ar.dev = st.device; rsm = stream_pool().take(st.device);
        StreamBack sback{st.device, rsm};
        upload_home();
        size_t got = std::max<size_t>(back_s.bytes, 256);
        back_h = (char*)block_cache().take(got, st.device, true);
        PinBack pinback{back_h, got, st.device};
        bool changed = true;
        for (int k = 1; !active.empty(); ++k) {
            const std::vector<score_graph> views = compact(k, changed);
            RobustHandle rh;   // (goes before the pooled stream is given back)
            const std::vector<score_info> inf = create_and_solve(views, rh);
            std::vector<int> next;
            reweigh(k, rh.h);
            copy_estimates(sort_members(k, inf, next), rh.h);
            if (!next.empty()) carry(rh.h->solver.be.stream);
            changed = next.size() != active.size();
            active.swap(next);
        }
        if (rinfos) std::memcpy(rinfos, rec.data(), (size_t)count * sizeof(score_robust_info));
        return 0;
    }
};
