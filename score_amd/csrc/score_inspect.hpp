// The handle's inspection surface: what score_debug_get, score_debug_time, score_time_kkt_apply and score_time_iteration read
// and measure, and the probe of the Newton PCG's launches.  Tests, bench.py and the profile scripts come through here; the
// solver itself calls only the three probe_* functions (declared in front of HipBackend).  Included by score_hip.hip where
// HipBackend is complete.
#pragma once

// ---- probe of the Newton PCG's launches (score_debug_get "newton_probe_arm" / "newton_probe"): the next polish
//      binds start / stop events to its chain-kernel STEPs and H products (as score_time_iteration does for the ADMM
//      loop) and reports the mean dispatch duration of those that did work (launches queued beyond a solve's
//      convergence are no-ops and are left out) ----
struct NewtonProbe {
    static constexpr int kCap = 1024;
    bool armed = false;
    std::vector<hipEvent_t> ev;
    struct Slot { int kind, step; bool real; };
    std::vector<Slot> slots;
    size_t marked = 0;  // slots [0, marked): of Newton iterations that have been marked
    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
int probe_slot(HipBackend& be, int kind, int step) {
    NewtonProbe* np = be.probe.get();
    if (!np || !np->armed || (int)np->slots.size() >= NewtonProbe::kCap) return -1;
    np->slots.push_back(NewtonProbe::Slot{kind, step, false});
    be.tev = np->ev.data();
    return (int)np->slots.size() - 1;
}
void probe_mark(HipBackend& be, int used) {  // the PCG steps of the current Newton iteration that did work
    NewtonProbe* np = be.probe.get();
    if (!np) return;
    for (; np->marked < np->slots.size(); ++np->marked)
        if (np->slots[np->marked].step < used) np->slots[np->marked].real = true;
}
void probe_collect(HipBackend& be) {
    NewtonProbe* np = be.probe.get();
    if (!np || !np->armed) return;
    double sum[2] = {0, 0};
    int cnt[2] = {0, 0};
    for (size_t i = 0; i < np->slots.size(); ++i) {
        if (!np->slots[i].real) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, np->ev[2 * i], np->ev[2 * i + 1]) != hipSuccess) continue;
        sum[np->slots[i].kind] += 1e3 * (double)ms;
        cnt[np->slots[i].kind] += 1;
    }
    const HostSystem& h = *be.H;
    // algorithmic bytes: H product (KPB: + p, z, w_old in, p out), chain STEP of the Newton set (every chain its own factors)
    double hbytes = 0.0;
    if (be.Hb.on) { for (double b : be.Hb.L.bytes) hbytes += b; }
    else hbytes = 12.0 * (double)be.hm_nnz + 4.0 * (double)(h.n_tot + 1);
    hbytes += 40.0 * (double)h.n_tot;
    const double fbytes = (be.Hset.use_fac32 ? 4.0 : 8.0) * (double)be.Hset.fac_doubles;
    double* o = np->out;
    o[0] = cnt[0]; o[1] = cnt[0] ? sum[0] / cnt[0] : 0.0; o[2] = hbytes;
    o[3] = cnt[1]; o[4] = cnt[1] ? sum[1] / cnt[1] : 0.0; o[5] = fbytes;
    o[6] = (double)be.Hset.blocks(); o[7] = (double)be.n_prec;
    for (hipEvent_t e : np->ev) (void)hipEventDestroy(e);
    np->ev.clear(); np->slots.clear(); np->marked = 0;
    np->armed = false;
}
// the next polish times its PCG launches
int64_t probe_arm(HipBackend& be, double* out, int64_t len) {
    if (!be.Q.available) return -1;
    if (out && len > 0) {
        if (!be.probe) be.probe = std::make_shared<NewtonProbe>();
        NewtonProbe& np = *be.probe;
        for (hipEvent_t e : np.ev) (void)hipEventDestroy(e);
        np.ev.assign((size_t)2 * NewtonProbe::kCap, nullptr);
        for (auto& e : np.ev)
            if (hipEventCreate(&e) != hipSuccess) return -2;
        np.slots.clear(); np.marked = 0;
        np.armed = true;
        out[0] = 1.0;
    }
    return 1;
}

// ---------------------------------------------------------------------------
// score_debug_get: a named array or record of the handle, as doubles.  out == nullptr or len == 0: the size only.
// -1: unknown name / not available on this handle, -2: the device failed.
// ---------------------------------------------------------------------------
std::vector<int32_t> down_i32(HipBackend& be, const int32_t* d, size_t cnt) {
    std::vector<int32_t> v(cnt);
    HIP_CHECK(sync_stream(be.stream));
    if (cnt) staged_d2h(v.data(), d, cnt * sizeof(int32_t), be.stream);
    HIP_CHECK(sync_stream(be.stream));
    return v;
}
std::vector<double> down_f64(HipBackend& be, const double* d, size_t cnt) {
    std::vector<double> v(cnt);
    if (cnt) staged_d2h(v.data(), d, cnt * sizeof(double), be.stream);
    HIP_CHECK(sync_stream(be.stream));
    return v;
}
// the tail of every entry: min(len, sz) values out, sz back
template <class T>
int64_t copy_out_min(const T* src, int64_t sz, double* out, int64_t len) {
    if (out && len > 0) std::copy(src, src + std::min(len, sz), out);
    return sz;
}

// a plain array of the handle: where it lives, how long it is, whether this handle has it
struct DebugRow {
    enum Where { DevF64, DevI32, HostF64, HostI32 };
    const char* name; Where where; const void* ptr; int64_t len; bool ok = true;
};
int64_t read_row(HipBackend& be, const DebugRow& r, double* out, int64_t len) {
    if (!r.ok) return -1;
    if (!out || len <= 0) return r.len;
    const int64_t cnt = std::min(len, r.len);
    switch (r.where) {
        case DebugRow::HostF64: copy_out_min((const double*)r.ptr, cnt, out, cnt); break;
        case DebugRow::HostI32: copy_out_min((const int32_t*)r.ptr, cnt, out, cnt); break;
        case DebugRow::DevI32: copy_out_min(down_i32(be, (const int32_t*)r.ptr, (size_t)cnt).data(), cnt, out, cnt); break;
        case DebugRow::DevF64:
            HIP_CHECK(sync_stream(be.stream));
            if (cnt) staged_d2h(out, r.ptr, sizeof(double) * (size_t)cnt, be.stream);
            break;
    }
    return r.len;
}

// ---- the computed entries ----
int64_t get_setup_scalars(HipBackend& be, double* out, int64_t len) {  // per problem: |q|_inf, |b|_inf unscaled and scaled, kkt_bytes
    const HostSystem& h = *be.H;
    const int64_t sz = 5 * (int64_t)h.count;
    if (out && len >= sz)
        for (int p = 0; p < h.count; ++p) {
            out[5 * p] = h.qnorm_u[(size_t)p]; out[5 * p + 1] = h.qnorm_s[(size_t)p]; out[5 * p + 2] = h.bnorm_u[(size_t)p];
            out[5 * p + 3] = h.bnorm_s[(size_t)p]; out[5 * p + 4] = h.kkt_bytes[(size_t)p];
        }
    return sz;
}
int64_t get_device_setup(HipBackend& be, double* out, int64_t len) {
    const double v = be.H->device_setup ? 1.0 : 0.0;
    return copy_out_min(&v, 1, out, len);
}
int64_t get_matrix_source(HipBackend& be, double* out, int64_t len) {  // 0: built on the device, 1: host system with A, G1, G2 derived on the device, 2: uploaded
    const double v = (double)(int)be.source;
    return copy_out_min(&v, 1, out, len);
}
int64_t get_rep(HipBackend& be, double* out, int64_t len) {  // [replicas the kernels run with (1 = general problem), nnz of the stored K, of the stored A']
    const HostSystem& h = *be.H;
    const double v[3] = {(double)h.rep, (double)h.K.col.size(), (double)(h.device_setup ? (size_t)be.g1_nnz : h.G1.col.size())};
    return copy_out_min(v, 3, out, len);
}
int64_t get_links(HipBackend& be, double* out, int64_t len) {  // [node pairs outside the chains, pairs inside the preconditioner, unknowns, affected chains, rounds, problems whose capacitance matrix was singular]
    double v[6] = {(double)be.link_plan.pairs_total, (double)be.link_plan.pairs_used, (double)be.n_link_u, (double)be.n_link_items, (double)be.link_rounds, 0.0};
    if (be.n_link_probs && out) {
        std::vector<int32_t> stt((size_t)be.n_link_probs);
        HIP_CHECK(sync_stream(be.stream));
        for (int set = 0; set < 2; ++set) {
            if (!be.pset[set].link_on) continue;
            HIP_CHECK(hipMemcpy(stt.data(), be.pset[set].link_status.d, sizeof(int32_t) * (size_t)be.n_link_probs, hipMemcpyDeviceToHost));
            for (int32_t x : stt) v[5] += x;
        }
    }
    return copy_out_min(v, 6, out, len);
}
int64_t get_newton_probe(HipBackend& be, double* out, int64_t len) {
    // [H products timed, mean us, bytes per launch, chain STEPs timed, mean us, factor bytes per launch, H tiles, prec work items]
    static const double none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return copy_out_min(be.probe ? be.probe->out : none, 8, out, len);
}
// the device-against-host checks ("ag_device_check", "polish_build_check"): a device array on the host; entries that
// differ (+ the difference in length); largest difference (1e300 when the lengths differ)
double mismatches(const std::vector<int32_t>& x, const std::vector<int32_t>& y) {
    double c = (double)(x.size() > y.size() ? x.size() - y.size() : y.size() - x.size());
    for (size_t i = 0; i < std::min(x.size(), y.size()); ++i) c += x[i] != y[i];
    return c;
}
double max_diff(const std::vector<double>& x, const std::vector<double>& y) {
    double c = x.size() == y.size() ? 0.0 : 1e300;
    for (size_t i = 0; i < std::min(x.size(), y.size()); ++i) c = std::max(c, std::fabs(x[i] - y[i]));
    return c;
}
int64_t get_ag_device_check(HipBackend& be, double* out, int64_t len) {
    // the equilibrated A, G1, G2 on the device against the host arrays: [derived on the device (0/1), mismatching
    // columns of A, max |A value difference|, the same for G1, for G2]
    const HostSystem& h = *be.H;
    if (h.device_setup) return -1;  // (no host matrices to compare with: SCORE_HOST_SETUP=1)
    if (out && len >= 7) {
        out[0] = be.derive_ag ? 1.0 : 0.0;
        out[1] = mismatches(down_i32(be, be.A_col.d, h.A.col.size()), h.A.col); out[2] = max_diff(down_f64(be, be.A_val.d, h.A.val.size()), h.A.val);
        out[3] = mismatches(down_i32(be, be.G1.col.d, h.G1.col.size()), h.G1.col); out[4] = max_diff(down_f64(be, be.G1.val.d, h.G1.val.size()), h.G1.val);
        out[5] = mismatches(down_i32(be, be.G2.col.d, h.G2.col.size()), h.G2.col); out[6] = max_diff(down_f64(be, be.G2.val.d, h.G2.val.size()), h.G2.val);
    }
    return 7;
}
int64_t get_polish_build_check(HipBackend& be, double* out, int64_t len) {
    // the Newton matrix built on the device against the host loop's (score_polish_host.hpp): [built on the device (0/1),
    // entries device, entries host, mismatching row pointers, columns, max |P-on-pattern difference|, mismatching
    // list pointers, cones, block indices, max |coefficient difference|, mismatching chain positions (diagonal,
    // sub-diagonal), Jacobi positions, long entries]
    const HostSystem& h = *be.H;
    if (h.device_setup) return -1;  // (no host matrices to compare with: SCORE_HOST_SETUP=1)
    if (!be.Q.available) return -1;
    if (out && len >= 14) {
        PolishData R;
        build_polish(h, R, false);
        const size_t nz = (size_t)be.hm_nnz, nc = R.ccone.size();
        out[0] = be.polish_on_device ? 1.0 : 0.0;
        out[1] = (double)be.hm_nnz; out[2] = (double)R.Hm.col.size();
        out[3] = mismatches(down_i32(be, be.Hm.ptr.d, (size_t)h.n_tot + 1), R.Hm.ptr);
        out[4] = mismatches(down_i32(be, be.Hm.col.d, nz), R.Hm.col);
        out[5] = max_diff(down_f64(be, be.q_Pon.d, nz), R.Pon);
        out[6] = mismatches(down_i32(be, be.q_cptr.d, nz + 1), R.cptr);
        out[7] = mismatches(down_i32(be, be.q_ccone.d, nc), R.ccone);
        out[8] = mismatches(down_i32(be, be.q_cab.d, nc), R.cab);
        out[9] = max_diff(down_f64(be, be.q_ccoef.d, nc), R.ccoef);
        out[10] = mismatches(down_i32(be, be.Hset.posd.d, R.pos_diag.size()), R.pos_diag);
        out[11] = mismatches(down_i32(be, be.Hset.poss.d, R.pos_sub.size()), R.pos_sub);
        out[12] = mismatches(down_i32(be, be.Hset.diagpos.d, R.diag_pos.size()), R.diag_pos);
        out[13] = mismatches(be.Q.long_ent, R.long_ent) + mismatches(be.Q.long_prob, R.long_prob);
    }
    return 14;
}
// ---- kernel-level checks of the Newton polish (tests/test_gpu_parity.py) ----
int64_t get_polish_assemble_at_x(HipBackend& be, double* out, int64_t len) {
    // evaluate F, gradient, generalised Hessian and its chain factors at the current ADMM
    // iterate x (what the first Newton iteration does); returns F
    const HostSystem& h = *be.H;
    if (!be.Q.available) return -1;
    if (out && len > 0) {
        try {
            be.c_step.assign(h.count, 1.0); be.c_tol2.assign(h.count, 0.0); be.c_skip.assign(h.count, 0);
            std::vector<char> all(h.count, 1);
            NewtonVecArgs va{};
            va.n = h.n_tot; va.is_head = be.q_ishead.d; va.g = be.q_g.d; va.part = be.q_gd.d;
            HIP_CHECK(hipMemsetAsync(be.q_g.d, 0, be.q_g.n * sizeof(double), be.stream));
            va.u = be.xy.d; va.delta = be.xy.d; va.step = 0.0; va.out = be.q_X0.d;
            hipLaunchKernelGGL(k_newton_trial, dim3((unsigned)((h.n_tot + kThreads - 1) / kThreads)), dim3(kThreads), 0, be.stream, va);
            be.upload_skip(all);
            std::vector<double> F(h.count), gn(h.count);
            be.newton_eval_batch(be.q_X0.d, all, F, gn);
            be.newton_hessian(be.q_skip.d);
            HIP_CHECK(sync_stream(be.stream));
            out[0] = F[0];
        } catch (const std::exception&) { return -2; }
    }
    return 1;
}
int64_t get_polish_prec_of_negg(HipBackend& be, double* out, int64_t len) {
    // z = M^-1 (-g) with the Newton preconditioner as factored on the device (k_factor), applied by
    // the chain kernel the PCG uses
    if (!be.Q.available) return -1;
    if (out && len > 0) {
        PrecArgs pa = be.prec_args(be.Hset);
        pa.done = be.q_skip.d;
        be.prec_vectors(pa, be.r.d, be.q_negg.d, be.z.d, be.p.d, be.w.d, be.q_delta.d, be.q_dummy.d, be.q_pw.d);
        pa.rz_in = nullptr; pa.rz_out = be.rz_part0.d;
        be.launch_prec<PREC_INIT>(be.Hset, pa);
    }
    return read_row(be, DebugRow{"z", DebugRow::DevF64, be.z.d, be.H->n_tot}, out, len);
}
// per column: chain node index (global numbering over all chains; by_chain: the chain's index) or -1
int64_t chain_map(HipBackend& be, bool by_chain, double* out, int64_t len) {
    const HostSystem& h = *be.H;
    std::vector<double> tmp(h.n_tot, -1.0);
    for (size_t ci = 0; ci < h.chains.size(); ++ci)
        for (int i = 0; i < h.chains[ci].N; ++i)
            for (int c = 0; c < h.bs; ++c) tmp[h.node_col[h.chains[ci].node_begin + i] + c] = by_chain ? (double)ci : (double)(h.chains[ci].node_begin + i);
    return copy_out_min(tmp.data(), (int64_t)tmp.size(), out, len);
}
int64_t get_chain_of_col(HipBackend& be, double* out, int64_t len) { return be.Q.available ? chain_map(be, false, out, len) : -1; }
int64_t get_chain_id_of_col(HipBackend& be, double* out, int64_t len) { return chain_map(be, true, out, len); }
int64_t get_graph_launches(HipBackend& be, double* out, int64_t len) {  // captured ADMM blocks replayed on this handle (HipBackend::run)
    const double v = (double)be.graph_launches;
    return copy_out_min(&v, 1, out, len);
}
// how the ADMM loop ends a PCG sweep: {HipBackend::sweep_help(), update helpers per launch, entries per helper, cones per cone workgroup, helpers of the cone launch}
int64_t get_sweep_help(HipBackend& be, double* out, int64_t len) {
    const double v[5] = {be.sweep_help() ? 1.0 : 0.0, (double)be.n_help, (double)HipBackend::kHelpEntries, (double)(be.H->count == 1 ? HipBackend::kLoopConesPerWg : kConesPerBlock),
                         (double)(be.sweep_help() ? be.n_cone_help() : 0)};
    return copy_out_min(v, 5, out, len);
}

// ---- read-outs of the Newton polish (tests/test_polish_model_gpu.py): plain reads of buffers and host values that exist ----
int64_t get_polish_eval(HipBackend& be, double* out, int64_t len) {
    // per problem [F, max |g_i| / D_i, act_flips] as the last evaluation collected them (newton_eval_collect)
    const int64_t cnt = be.H->count, sz = 3 * cnt;
    if (!be.Q.available || (int64_t)be.dbg_eval_F.size() != cnt || (int64_t)be.act_flips.size() != cnt) return -1;
    if (out && len >= sz)
        for (int64_t p = 0; p < cnt; ++p) {
            out[3 * p] = be.dbg_eval_F[(size_t)p]; out[3 * p + 1] = be.dbg_eval_gn[(size_t)p]; out[3 * p + 2] = be.act_flips[(size_t)p];
        }
    return sz;
}
int64_t get_polish_trace(HipBackend& be, double* out, int64_t len) {
    // HipBackend::kTraceFields values per Newton iteration and problem of the last polish_lockstep call, iteration by iteration:
    // [live, reref, eta, pcg_used, gate fired, F, gn, gd, trial steps taken, accepted step, F_new, gn_new, stalled, tolerance]
    // (gn: max |g_i| / D_i; gd = g'delta; a problem that is not live in an iteration holds zeros from pcg_used to stalled)
    if (!be.Q.available) return -1;
    return copy_out_min(be.polish_trace.data(), (int64_t)be.polish_trace.size(), out, len);
}
int64_t get_polish_pcg(HipBackend& be, double* out, int64_t len) {
    // the gate words of the last Newton PCG as the device holds them: [fired per problem | STEPs executed per problem]
    if (!be.Q.available) return -1;
    const int64_t sz = 2 * (int64_t)be.H->count;
    if (out && len >= sz) copy_out_min(down_i32(be, be.q_pcgdone.d, (size_t)sz).data(), sz, out, sz);
    return sz;
}
int64_t get_polish_gate(HipBackend& be, double* out, int64_t len) {
    // what pcg_gate read in the last Newton PCG: [(relative tolerance)^2 per problem | threshold tol2 * r0'z0 per problem]
    if (!be.Q.available) return -1;
    const int64_t cnt = be.H->count;
    if (out && len >= 2 * cnt) {
        HIP_CHECK(sync_stream(be.stream));
        const std::vector<double> t = down_f64(be, be.q_gate_tol2.d, (size_t)cnt), r = down_f64(be, be.q_gate_ref.d, (size_t)cnt);
        std::copy(t.begin(), t.end(), out);
        std::copy(r.begin(), r.end(), out + cnt);
    }
    return 2 * cnt;
}
int64_t get_polish_blocks(HipBackend& be, double* out, int64_t len) {
    // how the polish splits its work: per problem [cone blocks, row blocks of the gradient product, row blocks of H] (the host
    // adds one partial per block: F and g'delta), then the entries of H that take the long path of k_hassemble (positions in Hval)
    const HostSystem& h = *be.H;
    if (!be.Q.available) return -1;
    const int64_t sz = 3 * (int64_t)h.count + (int64_t)be.Q.long_ent.size();
    if (out && len >= sz) {
        for (int p = 0; p < h.count; ++p) {
            out[3 * p] = h.cone_part_ptr[p + 1] - h.cone_part_ptr[p];
            out[3 * p + 1] = h.rbG2.part_ptr[p + 1] - h.rbG2.part_ptr[p];
            out[3 * p + 2] = be.Q.rbH.part_ptr[p + 1] - be.Q.rbH.part_ptr[p];
        }
        std::copy(be.Q.long_ent.begin(), be.Q.long_ent.end(), out + 3 * h.count);
    }
    return sz;
}
int64_t get_polish_p(HipBackend& be, double* out, int64_t len) {
    // the direction of the last product of the last Newton PCG (w = H p for it: "w"), problem by problem.  The products write
    // p and p2 in turn, and a problem's launches are no-ops once its gate has fired: after `used` executed STEPs the
    // direction of its last product is in p2 when `used` is odd and in p when it is even (HipBackend::pcg_step).
    const HostSystem& h = *be.H;
    if (!be.Q.available) return -1;
    if (out && len >= h.n_tot) {
        const std::vector<int32_t> g = down_i32(be, be.q_pcgdone.d, (size_t)2 * h.count);
        const std::vector<double> a = down_f64(be, be.p.d, (size_t)h.n_tot), b = down_f64(be, be.p2.d, (size_t)h.n_tot);
        for (int p = 0; p < h.count; ++p) {
            const std::vector<double>& src = (g[(size_t)h.count + p] & 1) ? b : a;
            std::copy(src.begin() + h.xoff[p], src.begin() + h.xoff[p + 1], out + h.xoff[p]);
        }
    }
    return h.n_tot;
}

int64_t get_vec(HipBackend& be, const char* name, double* out, int64_t len) {
    const HostSystem& h = *be.H;
    const std::string nm(name);
    using R = DebugRow;
    const bool ds = h.device_setup, polish = be.Q.available;
    // the setup's value and pattern arrays as the kernels read them (tests: device setup against host setup, bit for bit)
    const int64_t n = h.n_tot, m = h.m_tot, nk = (int64_t)h.K.col.size(), na = h.A.ptr.empty() ? 0 : (int64_t)h.A.ptr[(size_t)m];
    const int64_t n1 = ds ? be.g1_nnz : (int64_t)h.G1.col.size(), n2 = h.G2.ptr.empty() ? 0 : (int64_t)h.G2.ptr[(size_t)n];
    const PolishData& Q = be.Q;
    const R rows[] = {
        {"xt", R::DevF64, be.xtu.d, n}, {"u", R::DevF64, be.xtu.d + n, m},
        {"x", R::DevF64, be.xy.d, n}, {"y", R::DevF64, be.xy.d + n, m}, {"s", R::DevF64, be.s.d, m},
        {"r", R::DevF64, be.r.d, n}, {"z", R::DevF64, be.z.d, n},
        {"p", R::DevF64, be.dbg_p ? be.dbg_p : ((be.cg_iters % 2 == 1) ? be.p.d : be.p2.d), n},  // last PCG direction
        {"w", R::DevF64, be.w.d, n}, {"kx", R::DevF64, be.kx.d, n},
        {"rho", R::DevF64, be.rho.d, h.count},  // the per-problem penalties as the kernels read them
        {"D", ds ? R::DevF64 : R::HostF64, ds ? (const void*)be.Dd.d : h.D.data(), n},
        {"E", ds ? R::DevF64 : R::HostF64, ds ? (const void*)be.Ed.d : h.E.data(), m},
        {"K0", R::DevF64, be.K0d.d, nk}, {"K1", R::DevF64, be.K1d.d, nk}, {"Kval", R::DevF64, be.K.val.d, nk},
        {"Aval", R::DevF64, be.A_val.d, na}, {"G1val", R::DevF64, be.G1.val.d, n1}, {"G2val", R::DevF64, be.G2.val.d, n2},
        {"qs", R::DevF64, be.q.d, n}, {"bs", R::DevF64, be.b.d, m},
        {"invD", R::DevF64, be.invD.d, n}, {"invE", R::DevF64, be.invE.d, m},
        {"fac", R::DevF64, be.Kset.fac.d, (int64_t)be.Kset.fac_doubles},
        {"polish_g", R::DevF64, be.q_g.d, polish ? n : 0}, {"Hval", R::DevF64, be.Hm.val.d, polish ? be.hm_nnz : 0},
        // the last evaluation's point [u | nu], cone blocks and activity words; the step of the last Newton PCG
        {"polish_u", R::DevF64, be.dbg_eval_x, n, polish && be.dbg_eval_x}, {"polish_nu", R::DevF64, be.dbg_eval_x ? be.dbg_eval_x + n : nullptr, m, polish && be.dbg_eval_x},
        {"polish_B", R::DevF64, be.q_Bbuf.d, polish ? (int64_t)h.cone_row.size() * Q.T * Q.T : 0, polish},
        {"polish_act", R::DevI32, be.q_act.d, polish ? (int64_t)h.cone_row.size() : 0, polish},
        {"polish_delta", R::DevF64, be.q_delta.d, polish ? n : 0, polish},
        {"polish_Pon", R::DevF64, be.q_Pon.d, polish ? be.hm_nnz : 0, polish},  // P (+ the regularisation) on the pattern of H: what k_hassemble starts every entry from
        {"Acol", R::DevI32, be.A_col.d, na}, {"Aptr", R::DevI32, be.A_ptr.d, m + 1},
        {"G1col", R::DevI32, be.G1.col.d, n1}, {"G1ptr", R::DevI32, be.G1.ptr.d, n + 1},
        {"G2col", R::DevI32, be.G2.col.d, n2}, {"G2ptr", R::DevI32, be.G2.ptr.d, n + 1}, {"G2split", R::DevI32, be.G2.split.d, n},
        {"Kcol_dev", R::DevI32, be.K.col.d, nk}, {"Kptr_dev", R::DevI32, be.K.ptr.d, n + 1},
        // (pattern of the K the kernels stream -- a replicated problem: replica 0 + tail rows)
        {"Kcol", R::HostI32, h.K.col.data(), nk}, {"Kptr", R::HostI32, h.K.ptr.data(), (int64_t)h.K.ptr.size()},
        // (made / built on the device: the host never held it)
        {"is_head", ds ? R::DevI32 : R::HostI32, ds ? (const void*)be.q_ishead.d : Q.is_head.data(), ds ? n : (int64_t)Q.is_head.size(), polish},
        {"Hcol", be.polish_on_device ? R::DevI32 : R::HostI32, be.polish_on_device ? (const void*)be.Hm.col.d : Q.Hm.col.data(),
         be.polish_on_device ? be.hm_nnz : (int64_t)Q.Hm.col.size(), polish},
        {"Hptr", R::HostI32, Q.Hm.ptr.data(), (int64_t)Q.Hm.ptr.size(), polish},
        // first columns of the node pairs inside the Newton preconditioner (two per pair)
        {"link_pairs", R::HostI32, be.link_plan.pair_cols.data(), be.n_link_items ? (int64_t)be.link_plan.pair_cols.size() : 0},
    };
    for (const R& r : rows)
        if (nm == r.name) return read_row(be, r, out, len);
    struct Computed { const char* name; int64_t (*fn)(HipBackend&, double*, int64_t); };
    static const Computed computed[] = {
        {"setup_scalars", get_setup_scalars}, {"device_setup", get_device_setup}, {"rep", get_rep}, {"links", get_links},
        {"newton_probe_arm", probe_arm}, {"newton_probe", get_newton_probe}, {"ag_device_check", get_ag_device_check},
        {"polish_build_check", get_polish_build_check}, {"polish_assemble_at_x", get_polish_assemble_at_x},
        {"polish_prec_of_negg", get_polish_prec_of_negg},
        {"chain_of_col", get_chain_of_col}, {"chain_id_of_col", get_chain_id_of_col}, {"matrix_source", get_matrix_source},
        {"graph_launches", get_graph_launches}, {"sweep_help", get_sweep_help},
        {"polish_eval", get_polish_eval}, {"polish_trace", get_polish_trace}, {"polish_pcg", get_polish_pcg}, {"polish_p", get_polish_p}, {"polish_gate", get_polish_gate}, {"polish_blocks", get_polish_blocks},
    };
    for (const Computed& c : computed)
        if (nm == c.name) return c.fn(be, out, len);
    return -1;
}

// ---------------------------------------------------------------------------
// timing: score_debug_time, score_time_kkt_apply, score_time_iteration
// ---------------------------------------------------------------------------
// problems that have converged are skipped by every kernel: time them as active (the done words zeroed for the scope)
struct TimeAllActive {
    HipBackend& be;
    std::vector<int32_t> keep;
    explicit TimeAllActive(HipBackend& b) : be(b), keep((size_t)b.H->count) {
        const std::vector<int32_t> zero(keep.size(), 0);
        HIP_CHECK(sync_stream(be.stream));
        HIP_CHECK(hipMemcpyAsync(keep.data(), be.done.d, keep.size() * sizeof(int32_t), hipMemcpyDeviceToHost, be.stream));
        HIP_CHECK(sync_stream(be.stream));
        HIP_CHECK(hipMemcpyAsync(be.done.d, zero.data(), zero.size() * sizeof(int32_t), hipMemcpyHostToDevice, be.stream));
        HIP_CHECK(sync_stream(be.stream));
    }
    ~TimeAllActive() {
        (void)hipMemcpyAsync(be.done.d, keep.data(), keep.size() * sizeof(int32_t), hipMemcpyHostToDevice, be.stream);
        (void)sync_stream(be.stream);
    }
};
// mean duration of `launch()` in ms: HIP events on the stream the solver launches on
template <class F>
double time_launches(HipBackend& be, int warmup, int reps, F&& launch) {
    for (int i = 0; i < warmup; ++i) launch();
    HIP_CHECK(sync_stream(be.stream));
    HIP_CHECK(hipEventRecord(be.ev0, be.stream));
    for (int i = 0; i < reps; ++i) launch();
    HIP_CHECK(hipEventRecord(be.ev1, be.stream));
    HIP_CHECK(hipEventSynchronize(be.ev1));
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, be.ev0, be.ev1));
    return (double)t / std::max(1, reps);
}

void time_kernel(HipBackend& be, const std::string& which, int reps, double* ms) {
    PrecArgs pa = be.prec_args(be.Kset);
    pa.done = be.done.d;
    be.prec_vectors(pa, be.r.d, be.r.d, be.z.d, be.p.d, be.w.d, be.xtu.d, be.kx.d, be.pw_part.d);
    pa.rz_in = be.rz_part0.d; pa.rz_out = be.rz_part1.d;
    const VecArgs va = be.xupdate_args(be.p.d, be.rz_part0.d, 1);
    const dim3 blk(kThreads);
    auto once = [&]() {
        // (the loop's forms: with HipBackend::sweep_help() the right-hand-side kernel applies no pending update and the cone launch
        //  carries the update helpers)
        if (which == "rhs") { SpmvArgs ra = be.spmv_args(be.G1, be.xtu.d); ra.apply_update = be.sweep_help() ? 0 : 1; be.launch_spmv<MODE_RHS>(be.G1, ra); }
        else if (which.rfind("prec_init:", 0) == 0) { pa.debug_skip = std::atoi(which.c_str() + 10); be.launch_prec<PREC_INIT>(be.Kset, pa); }
        else if (which == "prec_init") be.launch_prec<PREC_INIT>(be.Kset, pa);
        else if (which.rfind("prec_step:", 0) == 0) { pa.debug_skip = std::atoi(which.c_str() + 10); be.launch_prec<PREC_STEP>(be.Kset, pa); }
        else if (which == "prec_step") be.launch_prec<PREC_STEP>(be.Kset, pa);
        // (segmented long chains: the chain kernel alone / the second level alone -- k_join_solve + k_join_apply)
        else if (which == "prec_init_chain") be.launch_prec<PREC_INIT>(be.Kset, pa, -1, HipBackend::PrecDepth::chain);
        else if (which == "prec_step_chain") be.launch_prec<PREC_STEP>(be.Kset, pa, -1, HipBackend::PrecDepth::chain);
        else if (which == "join_init") { if (be.n_join_items) be.join_apply<PREC_INIT>(be.Kset, pa); }
        else if (which == "join_step") { if (be.n_join_items) be.join_apply<PREC_STEP>(be.Kset, pa); }
        else if (which == "kp") be.launch_kp(be.p.d);
        else if (which == "kpb") be.launch_kpb(be.p.d, be.p2.d, be.rz_part1.d, be.rz_part0.d);
        else if (which == "xupdate") hipLaunchKernelGGL(k_xupdate, dim3(be.n_vblocks), blk, 0, be.stream, va);
        // (the plain grid, not the XCD order the loop's cone launch takes -- HipBackend::xcd_grid_of: the measurement the
        //  profile scripts were calibrated with)
        else if (which == "cone") { if (be.n_cone_blocks) { ConeArgs ca = be.cone_args(be.xtu.d); ca.apply_alpha = 1; const unsigned nb = (unsigned)be.loop_cone_blocks(ca); const unsigned cg = be.sweep_help() ? be.cone_helpers(ca, nb) : nb; hipLaunchKernelGGL(k_cone, dim3(cg), blk, 0, be.stream, ca); } }
        else if (which == "nop") hipLaunchKernelGGL(k_nop, dim3(be.K.nblocks), blk, 0, be.stream, (int*)nullptr);
        else if (which == "nop1") hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, be.stream, (int*)nullptr);
        else if (which == "nop_load") hipLaunchKernelGGL(k_nop_load, dim3(be.K.nblocks), blk, 0, be.stream, be.K.blk_prob.d, be.done.d, (int*)nullptr);
        else throw std::runtime_error("unknown kernel name");
    };
    TimeAllActive all_active(be);
    *ms = time_launches(be, 5, reps, once);
}

// roofline probe: average launch duration of the KKT SpMV (w = K p)
void time_kkt(HipBackend& be, int reps, double* ms, double* bytes) {
    const HostSystem& h = *be.H;
    std::vector<double> hp(h.n_tot);
    for (int64_t i = 0; i < h.n_tot; ++i) hp[i] = 1.0 + 1e-3 * (double)(i % 7);
    HIP_CHECK(sync_stream(be.stream));
    staged_h2d(be.p.d, hp.data(), hp.size() * sizeof(double), be.stream);
    TimeAllActive all_active(be);
    *ms = time_launches(be, 10, reps, [&] { be.launch_kp(be.p.d); });
    double bsum = 0;
    for (double v : h.kkt_bytes) bsum += v;
    *bytes = bsum;
}

// in-loop duration of the six kernels of an iteration (see score_time_iteration):
//   us[0..5]   device wall clock, first workgroup in -> last workgroup out
//   us[6..11]  begin -> end of the dispatch as the runtime records it (start/stop events bound to
//              the launch itself: the interval rocprofv3 --kernel-trace reports); 0 when with_events == 0
// The two are taken in separate passes over the same iterations (the per-launch events make
// the runtime wait for each dispatch's completion signal, which the plain pass does not).
void time_iteration(HipBackend& be, int warmup, int iters, double* us, int with_events) {
    if (be.cg_iters != 2) throw std::runtime_error("score_time_iteration: needs cg_iters == 2");
    iters = std::max(1, iters);
    int khz = 0;
    HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, be.st.device));
    if (khz <= 0) throw std::runtime_error("score_time_iteration: no wall clock rate");
    for (int k = 0; k < 12; ++k) us[k] = 0.0;
    const int maxb = std::max(std::max(be.G1.nblocks, be.Kset.blocks()) + 8, std::max(be.n_prec + be.n_help, (be.H->count == 1 ? ((int)be.H->cone_row.size() + HipBackend::kLoopConesPerWg - 1) / HipBackend::kLoopConesPerWg : be.n_cone_blocks) + 8 + be.n_cone_help()));  // (grids: XCD rounding, update helpers)
    be.ts_stride = (size_t)2 * maxb;
    const size_t per_iter = 6 * be.ts_stride, nslot = per_iter * iters;
    {
        std::vector<unsigned long long> hts(nslot);
        for (size_t i = 0; i < nslot; i += 2) { hts[i] = ~0ull; hts[i + 1] = 0ull; }
        DevBuf<unsigned long long> dts;  // (tl_arena is null outside init: a plain hipMalloc on the handle's device)
        dts.alloc(nslot);
        HIP_CHECK(hipMemcpyAsync(dts.d, hts.data(), nslot * sizeof(unsigned long long), hipMemcpyHostToDevice, be.stream));
        HIP_CHECK(sync_stream(be.stream));
        for (int i = 0; i < warmup; ++i) be.enqueue_iteration(false, i == 0);
        for (int i = 0; i < iters; ++i) be.enqueue_iteration(false, warmup == 0 && i == 0, dts.d + per_iter * i);
        HIP_CHECK(hipMemcpyAsync(hts.data(), dts.d, nslot * sizeof(unsigned long long), hipMemcpyDeviceToHost, be.stream));
        HIP_CHECK(sync_stream(be.stream));
        HIP_CHECK(hipGetLastError());
        for (int i = 0; i < iters; ++i)
            for (int k = 0; k < 6; ++k) {
                const unsigned long long* p = &hts[per_iter * i + be.ts_stride * k];
                unsigned long long t0 = ~0ull, t1 = 0ull;
                for (int b = 0; b < maxb; ++b) { t0 = std::min(t0, p[2 * b]); t1 = std::max(t1, p[2 * b + 1]); }
                if (t1 > t0) us[k] += (double)(t1 - t0) * 1e3 / (double)khz / iters;
            }
        if (trace_on("stamps")) {
            // per-workgroup timeline of the last timed iteration: kernel, workgroup, entry and exit in us after the
            // iteration's first entry (stdout; profiles/scripts/r04_timeline.py draws it)
            const unsigned long long* base = &hts[per_iter * (size_t)(iters - 1)];
            unsigned long long t00 = ~0ull;
            for (size_t j = 0; j < per_iter; j += 2) t00 = std::min(t00, base[j]);
            for (int k = 0; k < 6; ++k)
                for (int b = 0; b < maxb; ++b) {
                    const unsigned long long a0 = base[be.ts_stride * k + 2 * (size_t)b], a1 = base[be.ts_stride * k + 2 * (size_t)b + 1];
                    if (a0 == ~0ull || a1 == 0ull) continue;
                    std::printf("STAMP %d %d %.3f %.3f\n", k, b, (double)(a0 - t00) * 1e3 / (double)khz, (double)(a1 - t00) * 1e3 / (double)khz);
                }
        }
    }
    if (!with_events) return;
    std::vector<hipEvent_t> evs((size_t)12 * iters, nullptr);
    struct EvFree {
        std::vector<hipEvent_t>& v;
        ~EvFree() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
    } ev_free{evs};
    for (auto& e : evs) HIP_CHECK(hipEventCreate(&e));
    for (int i = 0; i < warmup; ++i) be.enqueue_iteration(false, false);
    for (int i = 0; i < iters; ++i) {
        be.tev = evs.data() + (size_t)12 * i;
        be.enqueue_iteration(false, false);
    }
    be.tev = nullptr;
    HIP_CHECK(sync_stream(be.stream));
    HIP_CHECK(hipGetLastError());
    for (int i = 0; i < iters; ++i)
        for (int k = 0; k < 6; ++k) {
            if (k == 5 && !be.n_cone_blocks) continue;
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, evs[(size_t)12 * i + 2 * k], evs[(size_t)12 * i + 2 * k + 1]));
            us[6 + k] += 1e3 * (double)ms / iters;
        }
}
