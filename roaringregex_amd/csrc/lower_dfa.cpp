// lower_dfa.cpp — the DFA programs: subset construction, minimisation, search, contains and pattern-set tables (see lower.hpp).
#include "lower_internal.hpp"

#include <map>

namespace rrx {

// ------------------------------------------------------------------------------------------ DFA lowering
// Hopcroft's partition refinement, shared by minimise_into and multi_product: the coarsest partition of the D states of the complete
// table nxt[D][K] that refines their labels (values below `nlabels`) and is stable under every class.  block[i] = the block of
// state i; returns the number of blocks.  The partition starts as the labels present, in label order.  (The "recompute every
// signature until nothing splits" form took one round per state on a chain - a{1,n} is n rounds over n states: 0.45 s at
// n = 2400, minutes at 16000.)
template <class Label>
static uint32_t refine_partition(const std::vector<uint32_t> &nxt, const std::vector<Label> &kind, const uint32_t nlabels, const uint32_t K,
                                 std::vector<uint32_t> &block) {
    const uint32_t D = (uint32_t)kind.size();
    block.assign(D, 0);
    // inverse transitions per class, CSR: inv[k][first[k][t] .. first[k][t + 1]) = the states that go to t on class k
    std::vector<uint32_t> first((size_t)K * (D + 1), 0), inv((size_t)K * D);
    for (uint32_t i = 0; i < D; i++) for (uint32_t k = 0; k < K; k++) first[(size_t)k * (D + 1) + nxt[(size_t)i * K + k] + 1]++;
    for (uint32_t k = 0; k < K; k++) for (uint32_t t2 = 0; t2 < D; t2++) first[(size_t)k * (D + 1) + t2 + 1] += first[(size_t)k * (D + 1) + t2];
    {
        std::vector<uint32_t> fill(first);
        for (uint32_t i = 0; i < D; i++)
            for (uint32_t k = 0; k < K; k++) inv[(size_t)k * D + fill[(size_t)k * (D + 1) + nxt[(size_t)i * K + k]]++] = i;
    }
    // the partition: elems holds the states block by block; a block is elems[lo[b] .. hi[b]).  It starts as the kinds present.
    std::vector<uint32_t> elems(D), loc(D), lo, hi, marked;
    {
        std::vector<uint32_t> n_of(nlabels, 0), at(nlabels, 0);
        for (uint32_t i = 0; i < D; i++) n_of[kind[i]]++;
        for (uint32_t q = 1; q < nlabels; q++) at[q] = at[q - 1] + n_of[q - 1];
        for (uint32_t q = 0; q < nlabels; q++) if (n_of[q]) { lo.push_back(at[q]); hi.push_back(at[q] + n_of[q]); }
        for (uint32_t i = 0; i < D; i++) { const uint32_t p = at[kind[i]]++; elems[p] = i; loc[i] = p; }
        for (uint32_t b = 0; b < lo.size(); b++) for (uint32_t q = lo[b]; q < hi[b]; q++) block[elems[q]] = b;
    }
    marked.assign(lo.size(), 0);
    std::vector<uint8_t> queued;                    // [block][class]
    std::vector<std::pair<uint32_t, uint32_t>> work;
    auto enqueue = [&](uint32_t b, uint32_t k) {
        if (queued.size() < (size_t)(b + 1) * K) queued.resize((size_t)(b + 1) * K, 0);
        if (!queued[(size_t)b * K + k]) { queued[(size_t)b * K + k] = 1; work.emplace_back(b, k); }
    };
    {
        uint32_t largest = 0;                       // every starting block but the largest is a splitter
        for (uint32_t b = 1; b < lo.size(); b++) if (hi[b] - lo[b] > hi[largest] - lo[largest]) largest = b;
        for (uint32_t b = 0; b < lo.size(); b++) if (b != largest) for (uint32_t k = 0; k < K; k++) enqueue(b, k);
    }
    std::vector<uint32_t> touched, splitter;
    while (!work.empty()) {
        const uint32_t B = work.back().first, k = work.back().second;
        work.pop_back();
        queued[(size_t)B * K + k] = 0;
        splitter.assign(elems.begin() + lo[B], elems.begin() + hi[B]);      // (B itself may split below)
        touched.clear();
        for (uint32_t t2 : splitter)
            for (uint32_t q = first[(size_t)k * (D + 1) + t2]; q < first[(size_t)k * (D + 1) + t2 + 1]; q++) {
                const uint32_t i = inv[(size_t)k * D + q], b = block[i];
                const uint32_t at = loc[i], to = lo[b] + marked[b];          // move i into the marked prefix of its block
                if (at < to) continue;                                       // (already marked)
                const uint32_t other = elems[to];
                elems[to] = i; loc[i] = to; elems[at] = other; loc[other] = at;
                if (!marked[b]++) touched.push_back(b);
            }
        for (uint32_t b : touched) {
            const uint32_t m = marked[b];
            marked[b] = 0;
            if (m == hi[b] - lo[b]) continue;                                // the whole block goes there: no split
            const uint32_t nb = (uint32_t)lo.size();                         // the marked prefix becomes block nb
            lo.push_back(lo[b]); hi.push_back(lo[b] + m); marked.push_back(0);
            lo[b] += m;
            for (uint32_t q = lo[nb]; q < hi[nb]; q++) block[elems[q]] = nb;
            const bool nb_smaller = hi[nb] - lo[nb] <= hi[b] - lo[b];
            for (uint32_t c = 0; c < K; c++) {
                if (queued.size() >= (size_t)(b + 1) * K && queued[(size_t)b * K + c]) enqueue(nb, c);
                else enqueue(nb_smaller ? nb : b, c);
            }
        }
    }
    return (uint32_t)lo.size();
}
// The order both minimisations number their blocks by: rep[b] = the first state of block b, and the blocks in breadth-first order
// from the block of state `from`, classes ascending - an order that depends on the language and its byte classes only, not on
// which equivalent automaton the caller saw.  Blocks that `from` does not reach are not in it.
static std::vector<uint32_t> block_order(const std::vector<uint32_t> &nxt, const std::vector<uint32_t> &block, const uint32_t count, const uint32_t K,
                                         const uint32_t from, std::vector<uint32_t> &rep) {
    rep.assign(count, UINT32_MAX);
    for (uint32_t i = 0; i < block.size(); i++) if (rep[block[i]] == UINT32_MAX) rep[block[i]] = i;
    std::vector<uint32_t> order{block[from]};
    std::vector<uint8_t> seen(count, 0);
    seen[block[from]] = 1;
    for (size_t h = 0; h < order.size(); h++)
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t nb = block[nxt[(size_t)rep[order[h]] * K + k]];
            if (!seen[nb]) { seen[nb] = 1; order.push_back(nb); }
        }
    return order;
}
// Minimisation of a complete table over K classes and its renumbering.  kind[i]: 0 = rejecting, 1 = accepting, 2 = the ESCAPE state
// of a sampled table (kept apart from the dead state it would otherwise merge with).  State 0 is the dead state, state 1 the start.
static bool minimise_into(const std::vector<uint32_t> &nxt, const std::vector<uint8_t> &kind, const uint32_t K, DfaProgram &d) {
    const uint32_t D = (uint32_t)kind.size();
    std::vector<uint32_t> block;
    const uint32_t count = refine_partition(nxt, kind, 3, K, block);
    // renumber: the dead block -> 0, the others in block_order from the start state (the dead block, absorbing, adds nothing to it)
    std::vector<int64_t> id(count, -1);
    uint32_t next_id = 0;
    id[block[0]] = next_id++;
    {
        std::vector<uint32_t> rep;
        for (uint32_t b : block_order(nxt, block, count, K, 1, rep)) if (id[b] < 0) id[b] = next_id++;
        for (uint32_t b = 0; b < count; b++) if (id[b] < 0) id[b] = next_id++;    // (none: every set is reachable)
    }
    if (count > 65535) return false;
    d.nstates = count;
    d.accepting.assign(count, 0);
    d.next.assign((size_t)count * K, 0);
    bool any_escape = false;
    for (uint32_t i = 0; i < D; i++) any_escape = any_escape || kind[i] == 2;
    if (any_escape) d.escaped.assign(count, 0);
    for (uint32_t i = 0; i < D; i++) {
        uint32_t b = (uint32_t)id[block[i]];
        d.accepting[b] = kind[i] == 1;
        if (kind[i] == 2) d.escaped[b] = 1;
        for (uint32_t k = 0; k < K; k++) d.next[(size_t)b * K + k] = (uint16_t)id[block[nxt[(size_t)i * K + k]]];
    }
    d.start = (uint32_t)id[block[1]];
    d.accepts_empty = d.accepting[d.start];
    return true;
}
// One step of the subset construction on a position graph, as lower_dfa (every set, eagerly) and lower_dfa_sampled (the sets a text
// reaches, the union cached per set) take it.
namespace {
struct SubsetStep {
    const std::vector<Node> &nodes;
    std::vector<std::vector<uint8_t>> enters;           // [node][class]: the node is entered on the class (never on class 0)
    std::vector<uint32_t> seen_at;                      // scratch of follows(): the epoch a node was last met in
    uint32_t epoch = 0;
    explicit SubsetStep(const Reduced &red) : nodes(red.nodes), enters(red.nodes.size(), std::vector<uint8_t>(red.ncls, 0)), seen_at(red.nodes.size(), 0) {
        for (uint32_t u = 1; u < nodes.size(); u++) for (uint32_t k = 1; k < red.ncls; k++) enters[u][k] = nodes[u].label.has(red.cls_rep[k]);
    }
    // all = the union of the follow sets of `set`: each node once, then sorted
    void follows(const std::vector<uint32_t> &set, std::vector<uint32_t> &all) {
        all.clear();
        epoch++;
        for (uint32_t u : set) for (uint32_t v : nodes[u].follow) if (seen_at[v] != epoch) { seen_at[v] = epoch; all.push_back(v); }
        std::sort(all.begin(), all.end());
    }
    // appends the members of such a union that are entered on class k
    void entered(const std::vector<uint32_t> &all, uint32_t k, std::vector<uint32_t> &v) const { if (k) for (uint32_t x : all) if (enters[x][k]) v.push_back(x); }
    bool accepts(const std::vector<uint32_t> &set) const { return std::any_of(set.begin(), set.end(), [&](uint32_t u) { return nodes[u].fin; }); }
};
}  // namespace
// Subset construction + minimisation.  `sticky`: the initial node stays in every set and no byte kills (the
// automaton of "anything, then the pattern": search_dfas below); class 0 then gets a real column.
static bool subset_construct(const Reduced &red, uint32_t max_states, bool sticky, DfaProgram &d) {
    if (red.nodes.empty()) { d = dead_dfa(red); return true; }
    d = classes_of(red);
    const uint32_t K = red.ncls;
    SubsetStep step(red);
    std::map<std::vector<uint32_t>, uint32_t> ids;
    std::vector<std::vector<uint32_t>> sets;
    std::vector<uint32_t> nxt;                          // raw [state][class]
    size_t budget = (size_t)24 << 20;                   // total set elements: give up early on exploding automata
    auto intern = [&](std::vector<uint32_t> &&v) -> int64_t {
        auto it = ids.find(v);
        if (it != ids.end()) return it->second;
        if (sets.size() >= max_states || v.size() > budget) return -1;
        budget -= v.size();
        uint32_t id = (uint32_t)sets.size();
        ids.emplace(v, id);
        sets.push_back(std::move(v));
        return id;
    };
    intern({});                                         // 0 = dead (unreachable when sticky)
    intern({0});                                        // 1 = start: the initial node
    std::vector<uint32_t> all;
    for (uint32_t cur = 0; cur < sets.size(); cur++) {
        nxt.resize((size_t)(cur + 1) * K, 0);
        step.follows(sets[cur], all);
        for (uint32_t k = sticky ? 0 : 1; k < K; k++) {
            std::vector<uint32_t> v;
            if (sticky && cur != 0) v.push_back(0);     // node 0 sorts first; it is entered on nothing
            step.entered(all, k, v);
            int64_t id = intern(std::move(v));
            if (id < 0) return false;
            nxt[(size_t)cur * K + k] = (uint32_t)id;
        }
    }
    const uint32_t D = (uint32_t)sets.size();
    std::vector<uint8_t> kind(D, 0);
    for (uint32_t i = 0; i < D; i++) kind[i] = step.accepts(sets[i]);
    return minimise_into(nxt, kind, K, d);
}
bool lower_dfa(const Reduced &red, uint32_t max_states, DfaProgram &d) { return subset_construct(red, max_states, false, d); }

bool lower_dfa_sampled(const Reduced &red, const uint8_t *sample, uint32_t pieces, uint32_t piece_bytes, uint32_t max_states, DfaProgram &d,
                       SampledTableStats *stats) {
    d = classes_of(red);
    if (red.nodes.empty() || !sample || max_states < 4) return false;
    const uint32_t K = red.ncls;
    SubsetStep step(red);
    constexpr uint32_t kOpen = UINT32_MAX, kEscape = UINT32_MAX - 1;
    std::map<std::vector<uint32_t>, uint32_t> ids;
    std::vector<std::vector<uint32_t>> sets, unions;    // unions[i]: the union of the follow sets of set i (made when first needed)
    std::vector<uint8_t> has_union;
    std::vector<uint32_t> nxt;                          // [set][class]: set id, kOpen, kEscape
    const uint32_t budget = max_states - 1;             // (one row is the escape state)
    size_t elements = (size_t)8 << 20;
    auto add_set = [&](std::vector<uint32_t> &&v) -> uint32_t {
        const uint32_t id = (uint32_t)sets.size();
        ids.emplace(v, id);
        elements -= std::min(elements, v.size());
        sets.push_back(std::move(v));
        unions.emplace_back(); has_union.push_back(0);
        nxt.resize((size_t)(id + 1) * K, kOpen);
        nxt[(size_t)id * K] = 0;                        // class 0: nothing moves - the dead set
        return id;
    };
    add_set({});                                        // 0 = dead
    for (uint32_t k = 0; k < K; k++) nxt[k] = 0;
    add_set({0});                                       // 1 = start
    auto resolve = [&](uint32_t cur, uint32_t k) -> uint32_t {      // the transition (cur, k): an id, or kEscape when the budget is spent
        uint32_t &slot = nxt[(size_t)cur * K + k];
        if (slot != kOpen) return slot;
        if (!has_union[cur]) { step.follows(sets[cur], unions[cur]); has_union[cur] = 1; }
        std::vector<uint32_t> v;
        step.entered(unions[cur], k, v);
        auto it = ids.find(v);
        uint32_t to;
        if (it != ids.end()) to = it->second;
        else if (sets.size() < budget && v.size() <= elements) to = add_set(std::move(v));
        else to = kEscape;
        return nxt[(size_t)cur * K + k] = to;           // (add_set may have moved nxt: index again)
    };
    SampledTableStats st;
    // ---- the sets the sample reaches
    for (uint32_t p = 0; p < pieces; p++) {
        const uint8_t *t = sample + (size_t)p * piece_bytes;
        uint32_t i = 0;
        while (i < piece_bytes && t[i] != '\n') i++;    // a piece begins inside somebody's line: enter at the first line start
        i++;
        uint32_t cur = 1;
        if (i < piece_bytes) st.sample_lines++;
        for (; i < piece_bytes; i++) {
            const uint8_t c = t[i];
            if (c == '\n') { cur = 1; if (i + 1 < piece_bytes) st.sample_lines++; continue; }
            if (cur == kEscape) continue;               // until the end of the line
            st.sample_bytes_stepped++;
            cur = resolve(cur, c < 0x80 ? red.cls[c] : 0);
            if (cur == kEscape) st.sample_escapes++;
        }
    }
    st.sets_from_sample = (uint32_t)sets.size();
    if (!st.sample_bytes_stepped) return false;
    // ---- closure: the transitions still open, breadth-first over the sets in the order they were found
    for (uint32_t cur = 0; cur < sets.size(); cur++)
        for (uint32_t k = 1; k < K; k++) (void)resolve(cur, k);
    st.sets_from_closure = (uint32_t)sets.size() - st.sets_from_sample;
    // ---- the table: the escape state last; it leaves on class 0 only (whatever the set was, that byte kills it: a plain reject)
    const uint32_t D = (uint32_t)sets.size() + 1, esc = D - 1;
    std::vector<uint32_t> full((size_t)D * K);
    std::vector<uint8_t> kind(D, 0);
    for (uint32_t i = 0; i + 1 < D; i++) {
        kind[i] = step.accepts(sets[i]);
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t to = nxt[(size_t)i * K + k];
            if (to == kEscape) st.open_transitions++;
            full[(size_t)i * K + k] = to == kEscape ? esc : to;
        }
    }
    kind[esc] = 2;
    full[(size_t)esc * K] = 0;
    for (uint32_t k = 1; k < K; k++) full[(size_t)esc * K + k] = esc;
    if (stats) *stats = st;
    if (!st.open_transitions) kind[esc] = 0;            // the closure closed everything: an ordinary table (the escape row is unreachable)
    return minimise_into(full, kind, K, d);
}

// The pattern read right to left, as a graph of the same shape: node w stands for "a byte of label(w) has just been
// consumed backwards and the automaton is in the predecessors of w"; it is final iff the initial node is a predecessor.
static Reduced reversed(const Reduced &r) {
    Reduced o;
    o.ncls = r.ncls;
    std::memcpy(o.cls, r.cls, sizeof o.cls);
    o.cls_rep = r.cls_rep;
    const size_t N = r.nodes.size();
    if (!N) return o;
    o.nodes.resize(N);
    o.nodes[0].fin = r.nodes[0].fin;
    for (size_t w = 1; w < N; w++) {
        o.nodes[w].label = r.nodes[w].label;
        if (r.nodes[w].fin) o.nodes[0].follow.push_back((uint32_t)w);
    }
    for (size_t u = 0; u < N; u++)
        for (uint32_t w : r.nodes[u].follow) {
            if (u == 0) o.nodes[w].fin = true;
            else o.nodes[w].follow.push_back((uint32_t)u);
        }
    for (auto &n : o.nodes) sort_unique(n.follow);
    return o;
}
bool search_dfas(const Reduced &r, uint32_t max_states, DfaProgram &fwd, DfaProgram &rev) {
    return subset_construct(r, max_states, true, fwd) && subset_construct(reversed(r), max_states, false, rev);
}
bool lower_dfa_reversed(const Reduced &r, uint32_t max_states, DfaProgram &rev) { return subset_construct(reversed(r), max_states, false, rev); }
bool search_longest_dfas(const Reduced &r, uint32_t max_states, DfaProgram &starts, DfaProgram &anchored) {
    if (subset_construct(reversed(r), max_states, true, starts) && subset_construct(r, max_states, false, anchored)) return true;
    starts = DfaProgram();
    anchored = DfaProgram();
    return false;
}

// "Does the line contain a match": the forward search table with every accepting state folded into one absorbing accepting
// state FOUND (the line's verdict is in, it waits for the '\n'), minimised again.  Row 0 of the forward table - the empty set,
// which the sticky construction never reaches - is already absorbing and rejecting: it stays row 0 as the SKIP row of the batch
// kernels (a lane whose stripe begins inside somebody else's line waits in it).  Class 0 is an ordinary column here.
bool contains_dfa(const DfaProgram &fwd, DfaProgram &out) {
    const uint32_t K = fwd.ncls, D = fwd.nstates;
    if (D < 2) { out = dead_dfa(fwd); return true; }    // the empty language: SKIP is all there is, and the start
    out = classes_of(fwd);
    // minimise_into wants the dead state as 0 and the start as 1: the forward table has them there
    if (fwd.start != 1 || fwd.accepting[0]) return false;
    std::vector<uint32_t> nxt((size_t)D * K);
    std::vector<uint8_t> kind(D);
    for (uint32_t s = 0; s < D; s++) {
        kind[s] = fwd.accepting[s] ? 1 : 0;
        for (uint32_t k = 0; k < K; k++) nxt[(size_t)s * K + k] = fwd.accepting[s] ? s : fwd.next[(size_t)s * K + k];
    }
    return minimise_into(nxt, kind, K, out);
}

bool search_fwd_dfa(const Reduced &r, uint32_t max_states, DfaProgram &fwd) { return subset_construct(r, max_states, true, fwd); }

// ------------------------------------------------------------------------------------------ pattern sets
MultiProgram multi_unit() {
    MultiProgram u;
    u.nstates = 1; u.ncls = 1;
    std::memset(u.cls, 0, sizeof u.cls);
    u.next = {0};
    u.mask = {0};
    return u;
}

bool multi_product(const MultiProgram &a, const DfaProgram &b, uint32_t bit, MultiProgram &o) {
    o = MultiProgram();
    // the common byte classes: one per pair (class of a, class of b) that some byte has
    std::vector<uint32_t> ca, cb;                       // the pair of a common class
    {
        std::vector<int32_t> id((size_t)a.ncls * b.ncls, -1);
        for (int c = 0; c < 256; c++) {
            const size_t key = (size_t)a.cls[c] * b.ncls + b.cls[c];
            if (id[key] < 0) { id[key] = (int32_t)ca.size(); ca.push_back(a.cls[c]); cb.push_back(b.cls[c]); }
            o.cls[c] = (uint8_t)id[key];
        }
    }
    const uint32_t K = (uint32_t)ca.size();
    // breadth first over the reachable tuples
    PairInterner rows;
    const std::vector<std::pair<uint32_t, uint32_t>> &tuples = rows.pairs;
    rows.intern(a.start, b.start);
    std::vector<uint32_t> nxt;
    for (uint32_t cur = 0; cur < tuples.size(); cur++) {
        const auto [sa, sb] = tuples[cur];
        for (uint32_t k = 0; k < K; k++)
            nxt.push_back((uint32_t)rows.intern(a.next[(size_t)sa * a.ncls + ca[k]], b.next[(size_t)sb * b.ncls + cb[k]]));
        if (tuples.size() > kMultiMaxRows) return false;
    }
    const uint32_t D = (uint32_t)tuples.size();
    // the masks, and the partition they seed: label = the rank of the mask among the masks present
    std::vector<uint32_t> mask(D), label(D);
    {
        std::map<uint32_t, uint32_t> rank;
        for (uint32_t i = 0; i < D; i++) rank.emplace(mask[i] = a.mask[tuples[i].first] | (b.accepting[tuples[i].second] ? bit : 0u), 0u);
        uint32_t n = 0;
        for (auto &kv : rank) kv.second = n++;
        for (uint32_t i = 0; i < D; i++) label[i] = rank[mask[i]];
        std::vector<uint32_t> block;
        const uint32_t count = refine_partition(nxt, label, n, K, block);
        // number the blocks in block_order from the start's (every tuple is reachable: all of them), then the rows without a mask first
        std::vector<uint32_t> rep;
        std::vector<uint32_t> order = block_order(nxt, block, count, K, 0, rep);
        std::stable_partition(order.begin(), order.end(), [&](uint32_t b2) { return mask[rep[b2]] == 0; });
        std::vector<uint32_t> id(count);
        for (uint32_t r = 0; r < count; r++) id[order[r]] = r;
        o.nstates = count; o.ncls = K; o.start = id[block[0]];
        o.next.assign((size_t)count * K, 0);
        o.mask.assign(count, 0);
        o.first_hit = count;
        for (uint32_t r = 0; r < count; r++) {
            const uint32_t i = rep[order[r]];
            o.mask[r] = mask[i];
            o.full |= mask[i];
            if (mask[i] && o.first_hit == count) o.first_hit = r;
            for (uint32_t k = 0; k < K; k++) o.next[(size_t)r * K + k] = (uint16_t)id[block[nxt[(size_t)i * K + k]]];
        }
    }
    return true;
}

}  // namespace rrx
