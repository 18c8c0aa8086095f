// refine_view_check.cpp -- a member of a group sees the measurements that a handle on it alone sees: no device, no library.
//
// The group's kernels read a member's measurements through gn_meas_from (score_gn.hpp): the union's pointer table advanced by
// the member's rel0 / rng0 / pri0, with dim scalars per entry in rel_t and pri_t and dim * dim in rel_R.  Here two groups of
// three small graphs, one 2-D and one 3-D, are laid out as gb_build lays them (GnMeas::append member after member; a member's
// offsets are the families' counts before it is appended).  In each group one member has landmarks, ranges and priors, one has
// no landmarks (so no ranges and no priors), one has ranges and no priors.  For every member and every measurement index the
// group's view must give exactly the integers and doubles (==) that gn_build of the member alone gives through
// GnProblem::view.  Only one member of a group carries priors and its pri0 is 0, so the values cannot show a lost pri0: the
// members' views must also follow each other without a gap, from the union's first entry to its last.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I score_amd/csrc refine_view_check.cpp
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "score_gn.hpp"

using namespace score;

namespace {

int failures = 0;
void fail(const std::string& where, const std::string& what) {
    std::fprintf(stderr, "FAIL %s: %s\n", where.c_str(), what.c_str());
    ++failures;
}

// a graph's arrays and the score_graph over them; every value written is different from every other (next())
struct Graph {
    std::vector<int32_t> chain_len, rel_base, rel_to, rng_a, rng_b, pri_l;
    std::vector<double> rel_t, rel_R, rel_kappa, rel_tau, rng_dist, rng_prec, pri_t, pri_prec;
    score_graph g{};
};
double next() {
    static double v = 1.0;
    return v += 0.03125;
}
// chains: poses per chain; odometry along every chain, then one loop closure from the last pose to pose 1; n_rng ranges from
// pose r to landmark r % n_landmarks; n_pri priors on the first landmarks
template <int DIM>
void make_graph(Graph& G, std::vector<int32_t> chains, int n_landmarks, int n_rng, int n_pri) {
    G.chain_len = chains;
    int32_t p0 = 0;
    for (int32_t len : chains) {
        for (int32_t i = 0; i + 1 < len; ++i) { G.rel_base.push_back(p0 + i); G.rel_to.push_back(p0 + i + 1); }
        p0 += len;
    }
    G.rel_base.push_back(p0 - 1); G.rel_to.push_back(1);
    const size_t n_rel = G.rel_base.size();
    for (size_t k = 0; k < DIM * n_rel; ++k) G.rel_t.push_back(next());
    for (size_t k = 0; k < DIM * DIM * n_rel; ++k) G.rel_R.push_back(next());
    for (size_t k = 0; k < n_rel; ++k) { G.rel_kappa.push_back(next()); G.rel_tau.push_back(next()); }
    for (int r = 0; r < n_rng; ++r) {
        G.rng_a.push_back(r); G.rng_b.push_back(p0 + r % n_landmarks);
        G.rng_dist.push_back(next()); G.rng_prec.push_back(next());
    }
    for (int e = 0; e < n_pri; ++e) {
        G.pri_l.push_back(e); G.pri_prec.push_back(next());
        for (int k = 0; k < DIM; ++k) G.pri_t.push_back(next());
    }
    score_graph& g = G.g;
    g.dim = DIM; g.n_chains = (int32_t)chains.size(); g.chain_len = G.chain_len.data(); g.n_landmarks = n_landmarks;
    g.n_rel = (int64_t)n_rel; g.rel_base = G.rel_base.data(); g.rel_to = G.rel_to.data(); g.rel_t = G.rel_t.data();
    g.rel_R = G.rel_R.data(); g.rel_kappa = G.rel_kappa.data(); g.rel_tau = G.rel_tau.data();
    g.n_rng = n_rng; g.rng_a = G.rng_a.data(); g.rng_b = G.rng_b.data(); g.rng_dist = G.rng_dist.data(); g.rng_prec = G.rng_prec.data();
    g.n_lprior = n_pri; g.lprior_lm = G.pri_l.data(); g.lprior_t = G.pri_t.data(); g.lprior_prec = G.pri_prec.data();
}

template <class T>
void same(const std::string& where, const char* array, const T* group, const T* alone, int64_t count) {
    for (int64_t k = 0; k < count; ++k)
        if (!(group[k] == alone[k])) fail(where, std::string(array) + "[" + std::to_string(k) + "] differs");
}

template <int DIM>
void check_group() {
    const std::string dims = std::to_string(DIM) + "-D";
    Graph graphs[3];
    make_graph<DIM>(graphs[0], {3, 2}, 2, 3, 2);   // landmarks, ranges and priors
    make_graph<DIM>(graphs[1], {4}, 0, 0, 0);      // no landmarks: no ranges, no priors
    make_graph<DIM>(graphs[2], {3, 3}, 1, 2, 0);   // ranges, no priors
    GnProblem P[3];
    GnMeas U;
    long long rel0[3], rng0[3], pri0[3];
    for (int g = 0; g < 3; ++g) {
        gn_build(graphs[g].g, P[g]);
        rel0[g] = U.n_rel(); rng0[g] = U.n_rng(); pri0[g] = U.n_pri();
        U.append(P[g]);
    }
    const GnMeasPtr table = U.ptrs();
    GnMeasPtr at = table;  // where the next member's view must start
    for (int g = 0; g < 3; ++g) {
        const std::string where = dims + " member " + std::to_string(g);
        const GnMeasPtr m = gn_meas_from<DIM>(table, rel0[g], rng0[g], pri0[g]);
        const GnView v = P[g].view(nullptr, nullptr, nullptr);
        const GnMeasPtr& a = v.meas;
        if (v.n_rel != graphs[g].g.n_rel || v.n_rng != graphs[g].g.n_rng || v.n_pri != graphs[g].g.n_lprior) fail(where, "counts");
        same(where, "rel_i", m.rel_i, a.rel_i, v.n_rel); same(where, "rel_j", m.rel_j, a.rel_j, v.n_rel);
        same(where, "rel_t", m.rel_t, a.rel_t, DIM * v.n_rel); same(where, "rel_R", m.rel_R, a.rel_R, DIM * DIM * v.n_rel);
        same(where, "rel_kappa", m.rel_kappa, a.rel_kappa, v.n_rel); same(where, "rel_tau", m.rel_tau, a.rel_tau, v.n_rel);
        same(where, "rng_a", m.rng_a, a.rng_a, v.n_rng); same(where, "rng_b", m.rng_b, a.rng_b, v.n_rng);
        same(where, "rng_dist", m.rng_dist, a.rng_dist, v.n_rng); same(where, "rng_prec", m.rng_prec, a.rng_prec, v.n_rng);
        same(where, "pri_l", m.pri_l, a.pri_l, v.n_pri); same(where, "pri_t", m.pri_t, a.pri_t, DIM * v.n_pri);
        same(where, "pri_prec", m.pri_prec, a.pri_prec, v.n_pri);
        // no gap: this member's view starts where the one before it ended
        const bool joined = m.rel_i == at.rel_i && m.rel_j == at.rel_j && m.rel_t == at.rel_t && m.rel_R == at.rel_R &&
                            m.rel_kappa == at.rel_kappa && m.rel_tau == at.rel_tau && m.rng_a == at.rng_a && m.rng_b == at.rng_b &&
                            m.rng_dist == at.rng_dist && m.rng_prec == at.rng_prec && m.pri_l == at.pri_l && m.pri_t == at.pri_t &&
                            m.pri_prec == at.pri_prec;
        if (!joined) fail(where, "its view does not start where the previous member's ends");
        at = gn_meas_from<DIM>(m, v.n_rel, v.n_rng, v.n_pri);
    }
    const bool whole = at.rel_i == table.rel_i + U.rel_i.size() && at.rel_t == table.rel_t + U.rel_t.size() &&
                       at.rel_R == table.rel_R + U.rel_R.size() && at.rel_tau == table.rel_tau + U.rel_tau.size() &&
                       at.rng_b == table.rng_b + U.rng_b.size() && at.rng_prec == table.rng_prec + U.rng_prec.size() &&
                       at.pri_l == table.pri_l + U.pri_l.size() && at.pri_t == table.pri_t + U.pri_t.size() &&
                       at.pri_prec == table.pri_prec + U.pri_prec.size();
    if (!whole) fail(dims, "the members' views do not end at the union's last entry");
}

}  // namespace

int main() {
    check_group<2>();
    check_group<3>();
    if (failures) return 1;
    std::printf("every member's view equals its own\n");
    return 0;
}
