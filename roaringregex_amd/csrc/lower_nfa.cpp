// lower_nfa.cpp — the shift-and program: positions along a maximum path cover (see lower.hpp).
#include "lower_internal.hpp"

#include <queue>

namespace rrx {

namespace {

// Maximum bipartite matching (Hopcroft-Karp) between "u as source" and "v as target" over the edges
// u -> v, v != u.  match_succ[u] = v uses edge u->v as a "next bit" edge.
void path_cover(const std::vector<Node> &nodes, std::vector<int64_t> &succ, std::vector<int64_t> &pred) {
    const uint32_t n = (uint32_t)nodes.size();
    succ.assign(n, -1); pred.assign(n, -1);
    std::vector<std::vector<uint32_t>> adj(n);
    for (uint32_t u = 0; u < n; u++) for (uint32_t v : nodes[u].follow) if (v != u) adj[u].push_back(v);
    // greedy seed: prefer targets with a single predecessor candidate (typical chains)
    for (uint32_t u = 0; u < n; u++)
        for (uint32_t v : adj[u]) if (pred[v] < 0) { succ[u] = v; pred[v] = u; break; }
    std::vector<int32_t> dist(n);
    const int32_t INF = 1 << 30;
    auto bfs = [&]() {
        std::queue<uint32_t> q;
        bool found = false;
        for (uint32_t u = 0; u < n; u++) { if (succ[u] < 0) { dist[u] = 0; q.push(u); } else dist[u] = INF; }
        while (!q.empty()) {
            uint32_t u = q.front(); q.pop();
            for (uint32_t v : adj[u]) {
                int64_t w = pred[v];
                if (w < 0) found = true;
                else if (dist[(size_t)w] == INF) { dist[(size_t)w] = dist[u] + 1; q.push((uint32_t)w); }
            }
        }
        return found;
    };
    // iterative DFS to avoid deep recursion on long chains
    std::vector<uint32_t> it(n);
    auto try_augment = [&](uint32_t root) {
        std::vector<uint32_t> path{root};
        while (!path.empty()) {
            uint32_t u = path.back();
            if (it[u] >= adj[u].size()) { dist[u] = INF; path.pop_back(); continue; }
            uint32_t v = adj[u][it[u]++];
            int64_t w = pred[v];
            if (w < 0) {
                // augment along path: each path[i] takes the target it was exploring
                uint32_t tv = v;
                for (size_t i = path.size(); i-- > 0;) {
                    uint32_t pu = path[i];
                    int64_t old = succ[pu];
                    succ[pu] = tv; pred[tv] = pu;
                    if (old < 0) break;
                    tv = (uint32_t)old;
                }
                return true;
            }
            if (dist[(size_t)w] == dist[u] + 1) path.push_back((uint32_t)w);
        }
        return false;
    };
    while (bfs()) {
        std::fill(it.begin(), it.end(), 0);
        for (uint32_t u = 0; u < n; u++) if (succ[u] < 0) try_augment(u);
    }
}

}  // namespace

bool lower_nfa(const Reduced &red, uint32_t max_bits, NfaProgram &p, bool allow_carry, bool gaps) {
    p = NfaProgram();
    if (red.nodes.empty()) {                 // empty language: one dead position
        p.W = 1; p.nbits = 1;
        p.init = {0}; p.fin = {0}; p.chain = {0}; p.self = {0}; p.excm = {0}; p.cgrp = {0}; p.ctgt = {0};
        p.X.assign(1, 0); p.B.assign(256, 0);
        return true;
    }
    const std::vector<Node> &nodes = red.nodes;
    const uint32_t n = (uint32_t)nodes.size();
    if (n > max_bits) return false;
    // ---- layout along a path cover
    std::vector<int64_t> succ, pred;
    path_cover(nodes, succ, pred);
    // `gaps`: one never-entered position in front of every path head but the first, so that the bit shifted out of the
    // end of one path dies there instead of entering the next path: the line-mode lane kernel then needs no CHAIN mask
    // (the gap is in no B row).  order[q] = node at position q, or kGap.
    constexpr uint32_t kGap = UINT32_MAX;
    std::vector<uint32_t> pos(n, UINT32_MAX), order;
    std::vector<uint8_t> placed(n, 0);
    auto lay = [&](uint32_t head) {
        if (gaps && !order.empty()) order.push_back(kGap);
        for (int64_t u = head; u >= 0 && !placed[(size_t)u]; u = succ[(size_t)u]) {
            placed[(size_t)u] = 1; pos[(size_t)u] = (uint32_t)order.size(); order.push_back((uint32_t)u);
        }
    };
    lay(0);                                               // node 0 (entered by nothing) heads a path: position 0
    for (uint32_t u = 0; u < n; u++) if (pred[u] < 0 && !placed[u]) lay(u);
    for (uint32_t u = 0; u < n; u++) if (!placed[u]) {   // a cycle: cut it in front of u
        succ[(size_t)pred[u]] = -1; pred[u] = -1; lay(u);
    }
    const uint32_t N = (uint32_t)order.size();            // positions, gaps included
    if (N > max_bits) return false;
    p.nbits = N;
    p.W = (N + 31) / 32;
    const uint32_t W = p.W;
    p.init.assign(W, 0); p.fin.assign(W, 0); p.chain.assign(W, 0); p.self.assign(W, 0); p.excm.assign(W, 0);
    p.cgrp.assign(W, 0); p.ctgt.assign(W, 0);
    const bool dense_x = N <= kDenseExceptionBits;         // beyond: the CSR form only (N * W words would be GiBs)
    p.X.assign(dense_x ? (size_t)N * W : 0, 0);
    p.B.assign((size_t)256 * W, 0);
    auto setbit = [&](std::vector<uint32_t> &v, size_t base, uint32_t b) { v[base + (b >> 5)] |= 1u << (b & 31); };
    setbit(p.init, 0, pos[0]);
    p.accepts_empty = nodes[0].fin;
    // follow sets by position
    std::vector<std::vector<uint32_t>> fpos(N);
    std::vector<uint8_t> has_self(N, 0);
    for (uint32_t u = 0; u < n; u++)
        for (uint32_t v : nodes[u].follow) {
            if (v == u) has_self[pos[u]] = 1;
            else fpos[pos[u]].push_back(pos[v]);
        }
    for (auto &f : fpos) sort_unique(f);
    // carry groups: target t with a maximal run [lo, t-1] of positions that all lead to t
    std::vector<uint8_t> is_target(N, 0), in_group(N, 0);
    std::vector<int64_t> group_target(N, -1);
    for (uint32_t t = 1; allow_carry && t < N; t++) {
        auto leads = [&](uint32_t q) { return std::binary_search(fpos[q].begin(), fpos[q].end(), t); };
        if (!leads(t - 1)) continue;
        uint32_t lo = t - 1;
        while (lo > 0 && leads(lo - 1) && !is_target[lo - 1] && !in_group[lo - 1]) lo--;
        if (is_target[t - 1] || in_group[t - 1]) continue;
        if (lo + 1 == t) continue;                               // a run of one is just the shift edge
        for (uint32_t q = lo; q < t; q++) { in_group[q] = 1; group_target[q] = t; setbit(p.cgrp, 0, q); }
        is_target[t] = 1;
        setbit(p.ctgt, 0, t);
        p.n_carry++;
    }
    for (uint32_t u = 0; u < n; u++) {
        const uint32_t pu = pos[u];
        if (nodes[u].fin) setbit(p.fin, 0, pu);
        if (pred[u] >= 0) setbit(p.chain, 0, pu);          // entered by the shift from position pu-1
        if (has_self[pu]) setbit(p.self, 0, pu);
        for (unsigned c = 1; c < 128; c++) if (nodes[u].label.has(c)) setbit(p.B, (size_t)c * W, pu);
    }
    p.xoff.assign(N + 1, 0);
    for (uint32_t q = 0; q < N; q++) {
        uint32_t extra = 0;
        for (uint32_t tv : fpos[q]) {
            if (tv == q + 1 && ((p.chain[tv >> 5] >> (tv & 31)) & 1u)) continue;     // the shift edge
            if (group_target[q] == (int64_t)tv) continue;                              // covered by the add-carry
            if (dense_x) setbit(p.X, (size_t)q * W, tv);
            p.xtgt.push_back(tv); extra++;
            p.max_exc_row_words = std::max(p.max_exc_row_words, (tv >> 5) + 1);
        }
        p.xoff[q + 1] = (uint32_t)p.xtgt.size();
        if (extra) { setbit(p.excm, 0, q); p.n_exc++; }
    }
    return true;
}

}  // namespace rrx
