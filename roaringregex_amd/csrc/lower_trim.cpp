// lower_trim.cpp — the useful part of the reference automaton (see lower.hpp).
#include "lower_internal.hpp"


namespace rrx {

// ------------------------------------------------------------------------------------------ trim
// The useful part of the reference automaton, taken from its UNEXPANDED rows (frontend.hpp: a row is a DAG of shared pieces).
// Reachability and co-reachability are exact and cost the pieces, not the edges.  The rows that come out are the explicit
// rows minus DOMINATED edges: u->w goes when a sibling u->v stays with label(w) a subset of label(v) and L(v) a superset of
// L(w) (the words accepted from it) - then u->w adds no word to L(u), so every state keeps its language whatever else has been
// dropped before.  L(v) >= L(w) is known when w is final only if v is and
//   * row(w) is empty, or the head piece of w is one of the pieces row(v) is made of (v took a copy of w's row: the skipped
//     tail of every nullable fold - x{1,n} leaves n^2/2 such edges, Parser.cpp:123-141), or
//   * to a small depth: every kept edge of w has a kept edge of v with a label above it into the same state or one that
//     dominates it by these same rules ((ab){1,n}: the state after `a` of copy i over that of copy i+1).
// The pruned row of a piece is made from its own edges and the PRUNED rows of its children, children and target rows first
// (explicit stack: chains are tens of thousands deep), so x{1,n} costs O(n) here too.
namespace {

struct PieceTrimmer {
    const RefAutomaton &a;
    const std::vector<uint8_t> &useful;
    std::vector<uint8_t> st;                       // 0 = not visited, 1 = on the stack, 2 = done
    std::vector<std::vector<Edge>> pe;             // pruned expansion per piece (targets: useful reference states, no NUL)
    std::vector<CharSet> first;                    // the characters pe[piece] moves on
    uint64_t pair_tests = 0;
    std::vector<uint32_t> desc_stack;

    PieceTrimmer(const RefAutomaton &a_, const std::vector<uint8_t> &u) : a(a_), useful(u), st(a_.pieces.size(), 0), pe(a_.pieces.size()), first(a_.pieces.size()) {}

    static CharSet strip(CharSet on) { on.w[0] &= ~1ULL; return on; }           // NUL never occurs inside a string (regex.h:157)

    // "piece `what` is one of the pieces `from` is made of": exact along a spanning forest of the child links (pre / post
    // numbers: what chains of nullable copies give), then a short search for pieces with several parents.  A miss only
    // keeps an edge.
    std::vector<uint32_t> pre, post;
    void number_forest() {
        const uint32_t P = (uint32_t)a.pieces.size();
        pre.assign(P, UINT32_MAX); post.assign(P, 0);
        std::vector<uint8_t> has_parent(P, 0);
        for (uint32_t p = 0; p < P; p++) for (uint32_t c : a.pieces[p].children) has_parent[c] = 1;
        uint32_t clock = 0;
        std::vector<std::pair<uint32_t, uint32_t>> stack;          // (piece, next child)
        for (uint32_t r = 0; r < P; r++) {
            if (has_parent[r] || pre[r] != UINT32_MAX) continue;
            pre[r] = clock++;
            stack.emplace_back(r, 0);
            while (!stack.empty()) {
                const uint32_t p = stack.back().first;
                if (stack.back().second < a.pieces[p].children.size()) {
                    const uint32_t c = a.pieces[p].children[stack.back().second++];
                    if (pre[c] == UINT32_MAX) { pre[c] = clock++; stack.emplace_back(c, 0); }
                } else { post[p] = clock; stack.pop_back(); }
            }
        }
    }
    bool is_descendant(uint32_t from, uint32_t what) {
        if (pre[from] < pre[what] && pre[what] < post[from]) return true;
        if (!a.pieces[what].shared) return false;
        desc_stack.assign(1, from);
        int budget = 12;
        while (!desc_stack.empty() && budget-- > 0) {
            const uint32_t p = desc_stack.back(); desc_stack.pop_back();
            for (uint32_t c : a.pieces[p].children) {
                if (c == what || (pre[c] < pre[what] && pre[what] < post[c])) return true;
                desc_stack.push_back(c);
            }
        }
        return false;
    }
    // The recursive rule is COINDUCTIVE: a pair met again while it is being proven counts as holding (loops inside the
    // repeated operand: (a+b+){1,n} needs "the a-loop of copy i over the a-loop of copy j" to prove itself).  A success that
    // leans on a pair still in progress further up is only as good as that pair: it is handed up (`leans`), never cached;
    // successes that lean on nothing outside their own proof, and all failures (an assumption can only help), are cached.
    std::unordered_map<uint64_t, uint8_t> memo;                 // (v, w) -> 2 yes / 1 no / 16 + d: no within depth d
    std::vector<std::pair<uint32_t, uint32_t>> in_progress;
    static constexpr int kProofDepth = 48;                      // (abcdefghij){1,n}: one level per state of the operand
    // `cut`: set when a limit (depth, an unfinished row, the size caps) stood in for a real "no" somewhere in the proof
    bool dominates(uint32_t v, uint32_t w, int depth, uint32_t &leans, bool &cut) {       // L(v) >= L(w), proven
        leans = UINT32_MAX;
        if (a.is_final[w] && !a.is_final[v]) return false;
        const uint32_t hw = a.head[w], hv = a.head[v];
        if (hw == kNoPiece) return true;
        if (st[hw] == 2 && pe[hw].empty()) return true;
        if (hv == kNoPiece) return false;
        if (is_descendant(hv, hw)) return true;
        if (depth == 0 || st[hv] != 2 || st[hw] != 2 || pair_tests > kTrimPairTests) { cut = true; return false; }
        if (!subset(first[hw], first[hv])) return false;           // w can start with a character v cannot
        for (uint32_t i = 0; i < in_progress.size(); i++) if (in_progress[i].first == v && in_progress[i].second == w) { leans = i; return true; }
        const std::vector<Edge> &rv = pe[hv], &rw = pe[hw];
        if (rw.size() * rv.size() > 1024) { cut = true; return false; }
        const uint64_t key = ((uint64_t)v << 32) | w;
        auto it = memo.find(key);
        if (it != memo.end()) {
            if (it->second == 2) return true;
            if (it->second == 1) return false;
            if (it->second - 16 >= depth) { cut = true; return false; }
        }
        pair_tests += rw.size() * rv.size();
        const uint32_t me = (uint32_t)in_progress.size();
        in_progress.emplace_back(v, w);
        bool all = true, my_cut = false;
        uint32_t lowest = UINT32_MAX;
        for (const Edge &e : rw) {
            bool found = false;
            for (const Edge &f : rv) {
                if (!subset(e.on, f.on)) continue;
                if (f.to == e.to) { found = true; break; }
                uint32_t l;
                if (dominates(f.to, e.to, depth - 1, l, my_cut)) { lowest = std::min(lowest, l); found = true; break; }
            }
            if (!found) { all = false; break; }
        }
        in_progress.pop_back();
        if (!all) {
            memo[key] = my_cut ? (uint8_t)(16 + depth) : (uint8_t)1;
            cut = cut || my_cut;
            return false;
        }
        if (lowest >= me) memo[key] = 2;                        // leans on itself at most
        else leans = lowest;
        return true;
    }
    void raw_expand(uint32_t root, std::vector<Edge> &out) {                    // a child that is still on the stack (a cycle)
        std::vector<uint32_t> stack{root}, seen{root};
        while (!stack.empty()) {
            const uint32_t p = stack.back(); stack.pop_back();
            for (const Edge &e : a.pieces[p].direct) { const CharSet on = strip(e.on); if (useful[e.to] && !on.empty()) out.push_back(Edge{e.to, on}); }
            for (uint32_t c : a.pieces[p].children) if (std::find(seen.begin(), seen.end(), c) == seen.end()) { seen.push_back(c); stack.push_back(c); }
        }
    }
    std::vector<uint32_t> n_parents;               // pieces that list it as a child
    std::vector<uint8_t> heads_useful;             // it is the head piece of a useful state
    uint64_t visited_edges = 0, live_edges = 0;
    void build(uint32_t p) {
        // candidates with their origin: 0 = the piece's own edges, k = its k-th child (whose row is pruned within itself
        // already: only pairs of different origin are compared - an alternation of 1000 keywords is a chain of 1000 pieces,
        // each adding one edge to a row of hundreds)
        std::vector<Edge> cand;
        std::vector<uint16_t> origin;
        for (const Edge &e : a.pieces[p].direct) { const CharSet on = strip(e.on); if (useful[e.to] && !on.empty()) cand.push_back(Edge{e.to, on}); }
        origin.assign(cand.size(), 0);
        uint32_t k = 0;
        for (uint32_t c : a.pieces[p].children) {
            k++;
            if (st[c] == 2) {
                cand.insert(cand.end(), pe[c].begin(), pe[c].end());
                if (n_parents[c] == 1 && !heads_useful[c]) { live_edges -= pe[c].size(); std::vector<Edge>().swap(pe[c]); }    // nobody else reads it
            } else raw_expand(c, cand);
            origin.resize(cand.size(), (uint16_t)std::min<uint32_t>(k, 0xfffe));
        }
        visited_edges += cand.size();
        std::vector<uint32_t> idx(cand.size());
        for (uint32_t i = 0; i < idx.size(); i++) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cand[x].to < cand[y].to; });
        std::vector<Edge> merged;
        std::vector<uint16_t> from;                 // 0xffff: the target came from several origins
        for (uint32_t i : idx) {
            if (!merged.empty() && merged.back().to == cand[i].to) { merged.back().on |= cand[i].on; if (from.back() != origin[i]) from.back() = 0xffff; }
            else { merged.push_back(cand[i]); from.push_back(origin[i]); }
        }
        const size_t n = merged.size();
        std::vector<uint8_t> dropped(n, 0);
        if (n > 1) {
            // dominators are tried in this order: the piece's own edges first (the copy taken, not the tail skipped to)
            std::vector<uint32_t> order, order_own;
            for (uint32_t i = 0; i < n; i++) if (from[i] == 0 || from[i] == 0xffff) order.push_back(i);
            order_own = order;
            for (uint32_t i = 0; i < n; i++) if (from[i] != 0 && from[i] != 0xffff) order.push_back(i);
            const size_t per_edge = n <= 64 ? n : std::max<size_t>(8, 4096 / n);
            for (uint32_t w = 0; w < n; w++) {
                size_t tried = 0;
                // an edge that came from the only child has been compared with its fellows there: the own edges are left
                const bool own_only = k == 1 && from[w] == 1;
                for (uint32_t v : own_only ? order_own : order) {
                    if (v == w || dropped[v] || !subset(merged[w].on, merged[v].on)) continue;
                    if (from[v] == from[w] && from[v] != 0 && from[v] != 0xffff) continue;      // compared when that child was built
                    if (++tried > per_edge) break;
                    uint32_t leans;
                    bool cut = false;
                    if (dominates(merged[v].to, merged[w].to, kProofDepth, leans, cut)) { dropped[w] = 1; break; }
                }
            }
        }
        std::vector<Edge> &out = pe[p];
        for (uint32_t i = 0; i < n; i++) if (!dropped[i]) out.push_back(merged[i]);
        live_edges += out.size();
        for (const Edge &e : out) first[p] |= e.on;
        if (live_edges > kTrimBudget || visited_edges > 32 * kTrimBudget)
            throw BudgetError("pattern too large: the automaton's rows exceed the host pipeline's work budget");
    }
    void run(uint32_t root) {
        if (st[root]) return;
        std::vector<uint32_t> stack{root};
        while (!stack.empty()) {
            const uint32_t p = stack.back();
            if (st[p] == 2) { stack.pop_back(); continue; }
            st[p] = 1;
            bool pushed = false;
            for (uint32_t c : a.pieces[p].children) if (st[c] == 0) { stack.push_back(c); pushed = true; }
            for (const Edge &e : a.pieces[p].direct) {
                if (!useful[e.to] || strip(e.on).empty()) continue;
                const uint32_t h = a.head[e.to];
                if (h != kNoPiece && st[h] == 0) { stack.push_back(h); pushed = true; }
            }
            if (pushed) continue;
            build(p);
            st[p] = 2;
            stack.pop_back();
        }
    }
};

}  // namespace

Trimmed trim(const RefAutomaton &a) {
    Trimmed t;
    std::memset(t.cls, 0, sizeof t.cls);
    t.cls_rep.assign(1, 0);
    const uint32_t N = a.states_n, P = (uint32_t)a.pieces.size();
    auto live_edge = [&](const Edge &e) { CharSet on = e.on; on.w[0] &= ~1ULL; return !on.empty() && e.to < N; };
    // ---- reachable from the initial state: every piece is walked once
    std::vector<uint8_t> fwd(N, 0), bwd(N, 0), seen(P, 0);
    std::vector<uint32_t> stack, pstack;
    if (a.initial < N) { fwd[a.initial] = 1; stack.push_back(a.initial); }
    while (!stack.empty()) {
        const uint32_t s = stack.back(); stack.pop_back();
        if (a.head[s] == kNoPiece || seen[a.head[s]]) continue;
        seen[a.head[s]] = 1; pstack.push_back(a.head[s]);
        while (!pstack.empty()) {
            const uint32_t p = pstack.back(); pstack.pop_back();
            for (const Edge &e : a.pieces[p].direct) if (live_edge(e) && !fwd[e.to]) { fwd[e.to] = 1; stack.push_back(e.to); }
            for (uint32_t c : a.pieces[p].children) if (!seen[c]) { seen[c] = 1; pstack.push_back(c); }
        }
    }
    // ---- able to reach a final state: backwards over (target -> pieces that hold it -> pieces that include those -> owners)
    {
        std::vector<std::vector<uint32_t>> holders(N), parents(P), owners(P);
        for (uint32_t p = 0; p < P; p++) {
            for (const Edge &e : a.pieces[p].direct) if (live_edge(e)) holders[e.to].push_back(p);
            for (uint32_t c : a.pieces[p].children) parents[c].push_back(p);
        }
        for (uint32_t s = 0; s < N; s++) if (a.head[s] != kNoPiece) owners[a.head[s]].push_back(s);
        std::vector<uint8_t> live(P, 0);
        for (uint32_t s = 0; s < N; s++) if (a.is_final[s]) { bwd[s] = 1; stack.push_back(s); }
        while (!stack.empty()) {
            const uint32_t s = stack.back(); stack.pop_back();
            for (uint32_t h : holders[s]) {
                if (live[h]) continue;
                live[h] = 1; pstack.push_back(h);
                while (!pstack.empty()) {
                    const uint32_t p = pstack.back(); pstack.pop_back();
                    for (uint32_t o : owners[p]) if (!bwd[o]) { bwd[o] = 1; stack.push_back(o); }
                    for (uint32_t q : parents[p]) if (!live[q]) { live[q] = 1; pstack.push_back(q); }
                }
            }
        }
    }
    if (a.initial >= N || !(fwd[a.initial] && bwd[a.initial])) return t;   // empty language
    std::vector<uint8_t> useful(N, 0);
    std::vector<int64_t> newid(N, -1);
    for (uint32_t s = 0; s < N; s++) if (fwd[s] && bwd[s]) { useful[s] = 1; newid[s] = (int64_t)t.ref_id.size(); t.ref_id.push_back(s); }
    t.n = (uint32_t)t.ref_id.size();
    t.initial = (uint32_t)newid[a.initial];
    t.is_final.assign(t.n, 0);
    t.out.assign(t.n, {});
    PieceTrimmer pt(a, useful);
    pt.number_forest();
    pt.n_parents.assign(P, 0);
    pt.heads_useful.assign(P, 0);
    for (uint32_t p = 0; p < P; p++) for (uint32_t c : a.pieces[p].children) pt.n_parents[c]++;
    for (uint32_t s = 0; s < N; s++) if (useful[s] && a.head[s] != kNoPiece) pt.heads_useful[a.head[s]] = 1;
    if (a.head[a.initial] != kNoPiece) pt.run(a.head[a.initial]);
    for (uint32_t k = 0; k < t.n; k++) {
        const uint32_t s = t.ref_id[k];
        t.is_final[k] = a.is_final[s];
        if (a.head[s] == kNoPiece) continue;
        pt.run(a.head[s]);
        for (const Edge &e : pt.pe[a.head[s]]) t.out[k].push_back(Edge{(uint32_t)newid[e.to], e.on});
    }
    // byte classes = atoms of the boolean algebra generated by the edge labels
    std::vector<CharSet> labels;
    for (auto &v : t.out) for (const Edge &e : v) labels.push_back(e.on);
    std::sort(labels.begin(), labels.end());
    labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
    std::vector<std::vector<bool>> held(128);            // per char: which labels hold it (NUL: none)
    for (unsigned c = 0; c < 128; c++) for (const CharSet &L : labels) held[c].push_back(L.has(c));
    for (unsigned c = 1; c < 128; c++) {
        if (held[c] == held[0]) continue;                // in no label: class 0
        uint32_t k = 1;                                  // the class of the first char held by the same labels, else a new one
        while (k < t.cls_rep.size() && held[c] != held[t.cls_rep[k]]) k++;
        if (k == t.cls_rep.size()) t.cls_rep.push_back((uint8_t)c);
        t.cls[c] = (uint8_t)k;
    }
    t.ncls = (uint32_t)t.cls_rep.size();
    return t;
}

}  // namespace rrx
