// lower_reduce.cpp — the position graph both device programs are lowered from, and its reductions (see lower.hpp).
#include "lower_internal.hpp"

#include <map>
#include <tuple>

namespace rrx {

namespace {

// Keeps the nodes that node 0 reaches, renumbered breadth first (node 0 stays node 0).  only_if_fewer: leaves the graph as it is
// where every node is reached.
void keep_reachable(std::vector<Node> &nodes, bool only_if_fewer = false) {
    const uint32_t n = (uint32_t)nodes.size();
    std::vector<int64_t> id(n, -1);
    std::vector<uint32_t> reach{0};
    id[0] = 0;
    for (size_t k = 0; k < reach.size(); k++)
        for (uint32_t v : nodes[reach[k]].follow) if (id[v] < 0) { id[v] = (int64_t)reach.size(); reach.push_back(v); }
    if (only_if_fewer && reach.size() == n) return;
    std::vector<Node> kept(reach.size());
    for (size_t k = 0; k < reach.size(); k++) {
        kept[k] = std::move(nodes[reach[k]]);
        for (uint32_t &v : kept[k].follow) v = (uint32_t)id[v];
        sort_unique(kept[k].follow);
    }
    nodes.swap(kept);
}

// One bisimulation quotient.  forward: merge nodes with equal (label, fin, successor blocks);
// backward: merge nodes with equal (label, is-initial, predecessor blocks).  Both keep the language.
// Node 0 is the initial node and stays node 0.  Returns true if anything merged.
bool quotient(std::vector<Node> &nodes, bool forward) {
    const uint32_t n = (uint32_t)nodes.size();
    std::vector<std::vector<uint32_t>> nb(n);
    if (forward) for (uint32_t u = 0; u < n; u++) nb[u] = nodes[u].follow;
    else for (uint32_t u = 0; u < n; u++) for (uint32_t v : nodes[u].follow) nb[v].push_back(u);
    std::vector<uint32_t> block(n);
    uint32_t count = 0;
    {
        std::map<std::tuple<uint64_t, uint64_t, bool>, uint32_t> keys;
        for (uint32_t u = 0; u < n; u++) {
            bool flag = forward ? nodes[u].fin : (u == 0);
            auto key = std::make_tuple(nodes[u].label.w[0], nodes[u].label.w[1], flag);
            auto it = keys.find(key);
            if (it == keys.end()) it = keys.emplace(key, (uint32_t)keys.size()).first;
            block[u] = it->second;
        }
        count = (uint32_t)keys.size();
    }
    // Partition refinement with a worklist: a round only looks at the DIRTY nodes (those with a neighbour that changed
    // block in the round before); the others still carry their block's signature (the set of their neighbours' blocks).
    // The plain "recompute every signature until nothing splits" form took one round per node on a chain of equal labels
    // (x{17000}: 154 s); recomputing only dirty signatures still cost a node of in-degree d its d neighbours in every
    // round it was dirty ((ab?){1,n}: one round per copy, the last node entered from all of them: n^2).  So the signature
    // is kept incrementally: per node a sorted list (neighbour block, how many neighbours in it) and a 64-bit sum of
    // mix(block) over the blocks present; a neighbour's move updates two entries.  Nodes are grouped by (block, sum); the
    // partition that comes out is then CHECKED against the real signatures (below), so a collision cannot merge what must
    // stay apart.  The result is the coarsest stable refinement (unique).
    std::vector<std::vector<uint32_t>> dep(n);             // dep[v]: the nodes whose signature mentions v
    for (uint32_t u = 0; u < n; u++) for (uint32_t v : nb[u]) dep[v].push_back(u);
    std::vector<std::vector<uint32_t>> members(count);
    std::vector<uint32_t> where(n);
    for (uint32_t u = 0; u < n; u++) { where[u] = (uint32_t)members[block[u]].size(); members[block[u]].push_back(u); }
    auto mix = [](uint32_t b) { uint64_t z = (uint64_t)b + 0x9e3779b97f4a7c15ULL; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); };
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> cnt(n);       // sorted by block
    std::vector<uint64_t> sum(n, 0);
    for (uint32_t u = 0; u < n; u++) {
        std::vector<uint32_t> bl;
        bl.reserve(nb[u].size());
        for (uint32_t v : nb[u]) bl.push_back(block[v]);
        std::sort(bl.begin(), bl.end());
        for (size_t i = 0; i < bl.size();) {
            size_t j = i;
            while (j < bl.size() && bl[j] == bl[i]) j++;
            cnt[u].emplace_back(bl[i], (uint32_t)(j - i));
            sum[u] += mix(bl[i]);
            i = j;
        }
    }
    auto bump = [&](uint32_t u, uint32_t b, int by) {
        auto &c = cnt[u];
        auto it = std::lower_bound(c.begin(), c.end(), std::make_pair(b, 0u));
        if (it != c.end() && it->first == b) {
            it->second = (uint32_t)((int64_t)it->second + by);
            if (!it->second) { c.erase(it); sum[u] -= mix(b); }
        } else { c.insert(it, std::make_pair(b, 1u)); sum[u] += mix(b); }      // (by = +1)
    };
    std::vector<uint8_t> is_dirty(n, 1), queued(n, 0);
    std::vector<uint32_t> dirty(n), next_dirty, moved, moved_from, moved_to;
    for (uint32_t u = 0; u < n; u++) dirty[u] = u;
    while (!dirty.empty()) {
        std::sort(dirty.begin(), dirty.end(), [&](uint32_t x, uint32_t y) {
            return block[x] != block[y] ? block[x] < block[y] : sum[x] != sum[y] ? sum[x] < sum[y] : x < y; });
        next_dirty.clear();
        for (size_t i = 0; i < dirty.size();) {
            const uint32_t B = block[dirty[i]];
            size_t end = i;
            while (end < dirty.size() && block[dirty[end]] == B) end++;
            // which group keeps the id B: the one that agrees with the clean members (they all carry one signature: none of
            // their neighbours moved), or, if every member is dirty, the largest group
            int64_t keep_from = -1;
            if (end - i < members[B].size()) {
                uint32_t clean = UINT32_MAX;
                for (uint32_t u : members[B]) if (!is_dirty[u]) { clean = u; break; }
                keep_from = (int64_t)end;                           // (no dirty group stays, unless one matches)
                for (size_t g = i; g < end; g++) if (sum[dirty[g]] == sum[clean]) { keep_from = (int64_t)g; break; }
            } else {
                size_t best = 0;
                for (size_t g = i; g < end;) {
                    size_t g2 = g + 1;
                    while (g2 < end && sum[dirty[g2]] == sum[dirty[g]]) g2++;
                    if (g2 - g > best) { best = g2 - g; keep_from = (int64_t)g; }
                    g = g2;
                }
            }
            for (size_t g = i; g < end;) {
                size_t g2 = g + 1;
                while (g2 < end && sum[dirty[g2]] == sum[dirty[g]]) g2++;
                if ((int64_t)g != keep_from) {
                    const uint32_t nbk = count++;
                    members.emplace_back();
                    for (size_t q = g; q < g2; q++) {
                        const uint32_t u = dirty[q];
                        std::vector<uint32_t> &mb = members[B];
                        const uint32_t last = mb.back();
                        mb[where[u]] = last; where[last] = where[u]; mb.pop_back();
                        where[u] = (uint32_t)members[nbk].size(); members[nbk].push_back(u);
                        moved.push_back(u); moved_from.push_back(B); moved_to.push_back(nbk);
                    }
                }
                g = g2;
            }
            i = end;
        }
        // the moves take effect together, after every group of the round has been formed on the old partition
        for (size_t q = 0; q < moved.size(); q++) {
            block[moved[q]] = moved_to[q];
            for (uint32_t d : dep[moved[q]]) {
                bump(d, moved_from[q], -1);
                bump(d, moved_to[q], +1);
                if (!queued[d]) { queued[d] = 1; next_dirty.push_back(d); }
            }
        }
        moved.clear(); moved_from.clear(); moved_to.clear();
        for (uint32_t u : dirty) is_dirty[u] = 0;
        dirty.swap(next_dirty);
        for (uint32_t u : dirty) { is_dirty[u] = 1; queued[u] = 0; }
    }
    // the check: within a block every member must carry the same SET of neighbour blocks (the sums only said so)
    for (uint32_t b = 0; b < count; b++) {
        const std::vector<uint32_t> &mb = members[b];
        for (size_t k = 1; k < mb.size(); k++) {
            const auto &x = cnt[mb[0]], &y = cnt[mb[k]];
            bool same = x.size() == y.size();
            for (size_t q = 0; same && q < x.size(); q++) same = x[q].first == y[q].first;
            if (!same) return false;                               // a 64-bit collision: merge nothing (sound, and never seen)
        }
    }
    if (count == n) return false;
    // renumber so that node 0's block is 0 and the rest keep first-occurrence order
    std::vector<int64_t> id(count, -1);
    uint32_t next = 0;
    for (uint32_t u = 0; u < n; u++) if (id[block[u]] < 0) id[block[u]] = next++;
    std::vector<Node> merged(count);
    for (uint32_t u = 0; u < n; u++) {
        Node &m = merged[(size_t)id[block[u]]];
        m.label = nodes[u].label;
        m.fin = m.fin || nodes[u].fin;
        for (uint32_t v : nodes[u].follow) m.follow.push_back((uint32_t)id[block[v]]);
    }
    for (Node &m : merged) sort_unique(m.follow);
    nodes.swap(merged);
    return true;
}

// Removes edges u->w that are covered by a sibling edge u->v whose target simulates w ("little brother"
// pruning): v simulates w iff (fin(w) => fin(v)) and every successor w' of w has a successor v' of v with
// label(w') subset of label(v') and v' simulates w'.  With label(w) subset of label(v) the edge u->w adds no
// word to the language.  The reference's nested-optional construction of x{m,n} (Parser.cpp:133-137) leaves
// many such jump-ahead edges; pruning them turns bounded repeats back into plain shift chains.
// Returns true if an edge was removed.  Nodes that become unreachable are dropped.
// Cheap sufficient form of the same pruning for big graphs: v certainly simulates w when it is final if w is,
// and follow(w) is a subset of follow(v) (v can copy every move of w).  Siblings are tried in order of decreasing
// out-degree, a few per edge; follow sets are compared as bitsets.  Returns true if an edge was removed.
bool prune_by_containment(std::vector<Node> &nodes) {
    const uint32_t n = (uint32_t)nodes.size();
    const uint32_t words = (n + 63) / 64;
    std::vector<uint64_t> fs((size_t)n * words, 0);
    for (uint32_t u = 0; u < n; u++) for (uint32_t v : nodes[u].follow) fs[(size_t)u * words + (v >> 6)] |= 1ULL << (v & 63);
    auto contained = [&](uint32_t w, uint32_t v) {              // follow(w) subset of follow(v)
        const uint64_t *a = &fs[(size_t)w * words], *b = &fs[(size_t)v * words];
        for (uint32_t i = 0; i < words; i++) if (a[i] & ~b[i]) return false;
        return true;
    };
    bool removed = false;
    std::vector<uint32_t> order;
    for (uint32_t u = 0; u < n; u++) {
        std::vector<uint32_t> &f = nodes[u].follow;
        if (f.size() < 2) continue;
        order.assign(f.begin(), f.end());
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return nodes[a].follow.size() != nodes[b].follow.size() ? nodes[a].follow.size() > nodes[b].follow.size() : a < b; });
        std::vector<uint32_t> kept;
        for (uint32_t w : f) {
            bool drop = false;
            int tried = 0;
            for (uint32_t v : order) {
                if (v == w) continue;
                if (nodes[v].follow.size() < nodes[w].follow.size()) break;
                if (++tried > 6) break;
                if ((nodes[w].fin && !nodes[v].fin) || !subset(nodes[w].label, nodes[v].label) || !contained(w, v)) continue;
                // mutual cover: keep the lower index
                const bool mutual = nodes[v].follow.size() == nodes[w].follow.size() && nodes[v].fin == nodes[w].fin &&
                                    subset(nodes[v].label, nodes[w].label) && contained(v, w);
                if (mutual && w < v) continue;
                drop = true;
                break;
            }
            if (drop) removed = true; else kept.push_back(w);
        }
        f.swap(kept);                                            // (fs keeps the old rows: still supersets, still sound)
    }
    if (!removed) return false;
    keep_reachable(nodes);
    return true;
}

bool prune_by_simulation(std::vector<Node> &nodes) {
    const uint32_t n = (uint32_t)nodes.size();
    if (n > 160) return false;                                   // O(n^2 deg^2): small graphs only
    // sim[q*n+p] = 1: p simulates q
    std::vector<uint8_t> sim((size_t)n * n, 0);
    for (uint32_t q = 0; q < n; q++) for (uint32_t p2 = 0; p2 < n; p2++) sim[(size_t)q * n + p2] = (!nodes[q].fin || nodes[p2].fin) ? 1 : 0;
    bool changed = true;
    while (changed) {
        changed = false;
        for (uint32_t q = 0; q < n; q++) for (uint32_t p2 = 0; p2 < n; p2++) {
            if (!sim[(size_t)q * n + p2] || q == p2) continue;
            bool ok = true;
            for (uint32_t qs : nodes[q].follow) {
                bool found = false;
                for (uint32_t ps : nodes[p2].follow)
                    if (sim[(size_t)qs * n + ps] && subset(nodes[qs].label, nodes[ps].label)) { found = true; break; }
                if (!found) { ok = false; break; }
            }
            if (!ok) { sim[(size_t)q * n + p2] = 0; changed = true; }
        }
    }
    bool removed = false;
    for (uint32_t u = 0; u < n; u++) {
        std::vector<uint32_t> &f = nodes[u].follow;
        std::vector<uint8_t> drop(f.size(), 0);
        for (size_t i = 0; i < f.size(); i++) {
            const uint32_t w = f[i];
            for (size_t j = 0; j < f.size() && !drop[i]; j++) {
                const uint32_t v = f[j];
                if (i == j || drop[j] || !sim[(size_t)w * n + v] || !subset(nodes[w].label, nodes[v].label)) continue;
                // mutual cover: keep the lower index
                const bool mutual = sim[(size_t)v * n + w] && subset(nodes[v].label, nodes[w].label);
                if (mutual && w < v) continue;
                drop[i] = 1;
            }
        }
        std::vector<uint32_t> kept;
        for (size_t i = 0; i < f.size(); i++) if (!drop[i]) kept.push_back(f[i]); else removed = true;
        f.swap(kept);
    }
    if (!removed) return false;
    keep_reachable(nodes);                                       // drop nodes no longer reachable from node 0
    return true;
}

// Twin merge: nodes with the same finality, the same predecessor SET and the same follow SET differ only in the label
// they are entered on; one node with the union of the labels accepts the same words (every path through the merged node
// on a character of label(u) is a path through u, and the same for v).  This is what re-joins the two halves of a
// character class that the in-label split or an alternation of literals (a|b) made into separate positions, where the
// bisimulation quotients (same label only) cannot.  Node 0 (no label) is never merged.  Returns true if anything merged.
bool merge_twins(std::vector<Node> &nodes) {
    const uint32_t n = (uint32_t)nodes.size();
    std::vector<std::vector<uint32_t>> pred(n);
    for (uint32_t u = 0; u < n; u++) for (uint32_t v : nodes[u].follow) pred[v].push_back(u);
    std::map<std::tuple<bool, std::vector<uint32_t>, std::vector<uint32_t>>, uint32_t> groups;
    std::vector<uint32_t> leader(n);
    bool any = false;
    for (uint32_t u = 0; u < n; u++) {
        leader[u] = u;
        if (u == 0) continue;
        auto key = std::make_tuple((bool)nodes[u].fin, nodes[u].follow, pred[u]);      // both vectors are sorted
        auto it = groups.find(key);
        if (it == groups.end()) groups.emplace(std::move(key), u);
        else { leader[u] = it->second; any = true; }
    }
    if (!any) return false;
    std::vector<int64_t> id(n, -1);
    uint32_t next = 0;
    for (uint32_t u = 0; u < n; u++) if (leader[u] == u) id[u] = next++;
    std::vector<Node> merged(next);
    for (uint32_t u = 0; u < n; u++) {
        Node &m = merged[(size_t)id[leader[u]]];
        m.label.w[0] |= nodes[u].label.w[0]; m.label.w[1] |= nodes[u].label.w[1];
        if (leader[u] != u) continue;
        m.fin = nodes[u].fin;
        for (uint32_t v : nodes[u].follow) m.follow.push_back((uint32_t)id[leader[v]]);
    }
    for (Node &m : merged) sort_unique(m.follow);
    nodes.swap(merged);
    return true;
}

}  // namespace

Reduced reduce(const Trimmed &t) {
    Reduced red;
    std::memcpy(red.cls, t.cls, sizeof red.cls);
    red.ncls = t.ncls;
    red.cls_rep = t.cls_rep;
    if (t.n == 0) return red;
    // ---- split states by in-label: node (state, label); node 0 = the initial state before any input
    std::vector<Node> nodes(1);
    nodes[0].fin = t.is_final[t.initial];
    std::vector<std::map<CharSet, uint32_t>> copies(t.n);
    for (uint32_t s = 0; s < t.n; s++)
        for (const Edge &e : t.out[s]) {
            auto &m = copies[e.to];
            if (m.find(e.on) == m.end()) {
                m.emplace(e.on, (uint32_t)nodes.size());
                Node nd; nd.label = e.on; nd.fin = t.is_final[e.to];
                nodes.push_back(nd);
            }
        }
    std::vector<std::vector<uint32_t>> follow_of_state(t.n);
    for (uint32_t s = 0; s < t.n; s++) {
        for (const Edge &e : t.out[s]) follow_of_state[s].push_back(copies[e.to].at(e.on));
        sort_unique(follow_of_state[s]);
    }
    nodes[0].follow = follow_of_state[t.initial];
    for (uint32_t s = 0; s < t.n; s++) for (auto &kv : copies[s]) nodes[kv.second].follow = follow_of_state[s];
    // ---- the dominated edges trim() dropped may have been the only way into some nodes
    keep_reachable(nodes, true);
    // ---- shrink
    for (int round = 0; round < 8; round++) {
        bool c = prune_by_containment(nodes);              // first: it cuts the edge count the quotients iterate over
        bool a = quotient(nodes, true);
        bool b = quotient(nodes, false);
        bool d = prune_by_simulation(nodes);
        bool e = merge_twins(nodes);
        if (!a && !b && !c && !d && !e) break;
    }
    red.nodes.swap(nodes);
    return red;
}

}  // namespace rrx
