// The C ABI of include/score_hip.h, written once for the HIP library and its CPU twin.
//
// Each library is one translation unit.  It includes this header after it has defined
//   struct score_handle    { score::Solver<Backend> solver; };
//   struct score_generated { score::GeneratedBatch B; ... };
//   struct AbiEnv -- what differs between the two libraries at the boundary:
//       struct Scope { Scope(int device, bool solving); };  // what a call on a handle holds while it runs
//       static void before_create();                         // once-only process setup of the create paths
//       static void require_device(int device);              // throws unless settings may name `device`
// and gets the thread's error string, the call frame every entry point goes through, the helpers of the create paths and
// the entry points that read the same in both libraries.  What only one backend can say (the device assembler against the
// host assembler, the kernels' timers, the resident generator arrays) stays in the library's own file, written with the
// same frame.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

struct score_assembled {
    score::AssembledQP qp;
};

namespace {

thread_local std::string g_err;

// The frame of an entry point: the callable's value, or -- on an exception -- its message in g_err and `fail`.
template <class F>
auto abi_call(F&& f, decltype(f()) fail = -1) -> decltype(f()) {
    try {
        return f();
    } catch (const std::exception& e) {
        g_err = e.what();
        return fail;
    }
}

inline void require(bool ok, const char* msg = "null argument") {
    if (!ok) throw std::runtime_error(msg);
}

// the caller's settings or the defaults
inline score_settings resolve_settings(const score_settings* s) {
    score_settings st;
    if (s) st = *s; else score::default_settings(&st);
    return st;
}

// new object, build it, publish it to *out; a build that throws leaves nothing behind
template <class T, class Build>
void publish_new(T** out, Build&& build) {
    auto obj = std::make_unique<T>();
    build(*obj);
    *out = obj.release();
}

// the scope of a call on a handle; `solving`: create, solve, the step calls, score_read_estimates
inline AbiEnv::Scope handle_scope(const score_handle* h, bool solving = false) {
    require(h != nullptr, "null handle");
    return AbiEnv::Scope(h->solver.st.device, solving);
}

inline score::GenSpec gen_spec(const score_manhattan_spec& m) {
    return score::GenSpec{m.n_robots, m.n_poses, m.n_beacons, m.side, m.p_range, m.sigma_t, m.sigma_theta, m.sigma_range, m.seed, m.dim == 0 ? 2 : m.dim};
}

// the worlds [first, first + count) of a generated batch as graphs (score_create_from_generated)
inline std::vector<score_graph> generated_views(const score_generated* g, int32_t first, int32_t count, int32_t relaxation, score_handle** out) {
    require(g && out);
    require(first >= 0 && count > 0 && first + count <= g->B.count, "score_create_from_generated: worlds out of range");
    require(relaxation == 0 || relaxation == 1, "score_create_from_generated: relaxation must be 0 (SOCP) or 1 (QCQP)");
    std::vector<score_graph> views((size_t)count);
    for (int i = 0; i < count; ++i) { g->B.view(first + i, &views[(size_t)i]); views[(size_t)i].relaxation = relaxation; }
    return views;
}

}  // namespace

extern "C" {

void score_default_settings(score_settings* s) { score::default_settings(s); }

int score_create_batch(const score_problem* p, int32_t count, const score_settings* s, score_handle** out) {
    return abi_call([&] {
        AbiEnv::before_create();
        require(p && out);
        const score_settings st = resolve_settings(s);
        AbiEnv::require_device(st.device);
        AbiEnv::Scope scope(st.device, true);
        publish_new(out, [&](score_handle& h) { h.solver.create(p, count, st); });
        return 0;
    });
}
int score_create(const score_problem* p, const score_settings* s, score_handle** out) {
    return score_create_batch(p, 1, s, out);
}
int score_graphs_connected(const score_graph* graphs, int32_t count) {
    if (!graphs || count < 0) { g_err = "null argument"; return -1; }
    for (int32_t i = 0; i < count; ++i)
        if (!score::graph_connected(graphs[i])) return i + 1;
    return 0;
}
int score_dims(const score_handle* h, int64_t* n_total, int64_t* m_total, int32_t* count) {
    if (!h) { g_err = "null handle"; return -1; }
    if (n_total) *n_total = h->solver.user_n();  // (the programs as given: score_headform.hpp)
    if (m_total) *m_total = h->solver.user_m();
    if (count) *count = h->solver.H.count;
    return 0;
}
int score_solve(score_handle* h, double* x, double* y, double* s, score_info* infos) {
    return abi_call([&] { auto scope = handle_scope(h, true); return h->solver.solve(x, y, s, infos); });
}
int score_reset(score_handle* h) {
    return abi_call([&] { auto scope = handle_scope(h); h->solver.reset(); return 0; });
}
int score_solve_steps(score_handle* h, int32_t iters, double* x, double* y, double* s, score_info* infos) {
    return abi_call([&] { auto scope = handle_scope(h, true); return h->solver.steps(iters, x, y, s, infos); });
}
int score_newton_steps(score_handle* h, int32_t iters, double* x, double* y, double* s, score_info* infos) {
    return abi_call([&] { auto scope = handle_scope(h, true); return h->solver.newton_steps(iters, x, y, s, infos); });
}
int score_linear_create(const score_problem* pattern, const score_settings* s, score_handle** out) {
    return abi_call([&] {
        require(pattern && out);
        score::LinearPattern L;
        score::make_linear_pattern(*pattern, s, L);
        score_handle* h = nullptr;
        if (score_create_batch(&L.prob, 1, &L.st, &h) != 0) return -1;
        auto& S = h->solver;
        if ((int64_t)S.H.K0.size() != (int64_t)pattern->P_rowptr[pattern->n]) {
            score_destroy(h);
            throw std::runtime_error("score_linear_create: internal pattern differs from the given one");
        }
        S.linear_mode = true;
        S.linear_nnz = (int64_t)S.H.K0.size();
        *out = h;
        return 0;
    });
}
int score_linear_solve(score_handle* h, const double* values, const double* rhs, double* x, double rel_tol,
                       int32_t max_iters, int32_t* iters_used, double* rel_residual) {
    return abi_call([&] {
        auto scope = handle_scope(h);
        int used = 0;
        const int rc = h->solver.linear_solve(values, rhs, x, rel_tol, max_iters, &used, rel_residual);
        if (iters_used) *iters_used = used;
        return rc;
    });
}
// (time_kkt, get_vec: the backend's inspection surface -- score_inspect.hpp in the product, loops in the CPU twin)
int score_time_kkt_apply(score_handle* h, int32_t reps, double* ms, double* bytes) {
    return abi_call([&] { auto scope = handle_scope(h); time_kkt(h->solver.be, reps, ms, bytes); return 0; });
}
int64_t score_debug_get(score_handle* h, const char* name, double* out, int64_t len) {
    if (!h || !name) return -1;
    return abi_call([&] { auto scope = handle_scope(h); return get_vec(h->solver.be, name, out, len); }, (int64_t)-2);
}
int score_assemble(const score_graph* g, score_assembled** out) {
    return abi_call([&] {
        require(g && out);
        publish_new(out, [&](score_assembled& a) { score::assemble_graph(*g, a.qp); });
        return 0;
    });
}
int score_assemble_batch(const score_graph* graphs, int32_t count, score_assembled** out) {
    return abi_call([&] {
        require(graphs && out && count > 0);
        std::vector<std::unique_ptr<score_assembled>> made((size_t)count);
        std::vector<score::AssembledQP*> qps((size_t)count, nullptr);
        for (int i = 0; i < count; ++i) { made[(size_t)i] = std::make_unique<score_assembled>(); qps[(size_t)i] = &made[(size_t)i]->qp; }
        score::assemble_graphs(graphs, count, qps.data());
        for (int i = 0; i < count; ++i) out[i] = made[(size_t)i].release();
        return 0;
    });
}
int score_assembled_view(const score_assembled* a, score_problem* view) {
    if (!a || !view) { g_err = "null argument"; return -1; }
    a->qp.view(view);
    return 0;
}
void score_assembled_free(score_assembled* a) { delete a; }
int score_generated_graph(const score_generated* g, int32_t index, score_graph* view) {
    return abi_call([&] { require(g && view); g->B.view(index, view); return 0; });
}
int score_generated_truth(const score_generated* g, int32_t index, double* poses, double* beacons) {
    return abi_call([&] { require(g != nullptr); g->B.truth(index, poses, beacons); return 0; });
}
void score_generated_free(score_generated* g) { delete g; }
const char* score_last_error(void) { return g_err.c_str(); }
int32_t score_abi_version(void) { return SCORE_ABI_VERSION * 1000 + (int32_t)sizeof(score_problem); }

}  // extern "C"
