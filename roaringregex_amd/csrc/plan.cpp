// plan.cpp — engine choice, table forms, search plan and program dumps (plan.hpp).  Plain C++: no HIP header, no device call.
#include "plan.hpp"

#include "../../include/rrx.h"

namespace rrx {

size_t dfa2_table_bytes(const Dfa2Program &d) { return (size_t)d.nstates * (d.ncols | 1u) * 4; }
bool dfa2_fits(const Dfa2Program &d) { return dfa2_table_bytes(d) <= dev::kDfa2MaxTable; }
bool lower_dfa2_that_fits(const DfaProgram &d, Dfa2Program &out, bool items) {
    return d.nstates <= 4096 && lower_dfa2(d, 1024, out, items) && dfa2_fits(out);
}

static size_t classed_entries(const DfaProgram &d) { return (size_t)d.nstates * (d.ncls + 2); }
bool wide_fits(const DfaProgram &d) { return d.nstates <= dev::kWideMaxStates; }
bool classed_fits(const DfaProgram &d) { return classed_entries(d) <= dev::kClassedMaxEntries; }
bool global_fits(const DfaProgram &d) { return classed_entries(d) < ((size_t)1 << 24); }

bool LineTables::decide(int requested_engine) {
    wide = wide_fits(dfa) && requested_engine != RRX_ENGINE_DFA_GLOBAL;
    global = requested_engine == RRX_ENGINE_DFA_GLOBAL || (!wide && !classed_fits(dfa));
    if (global && !global_fits(dfa)) return false;
    // stride-2 form: when the table (rows of distinct pair columns) fits next to the 32 KiB pair table
    has_dfa2 = !global && requested_engine != RRX_ENGINE_DFA && lower_dfa2_that_fits(dfa, dfa2);
    // ... and its pair table a byte per entry where the largest column offset fits one: what the indexed match kernels then read
    byte_pairs = has_dfa2 && dfa2_byte_pairs_fit(dfa2);
    return true;
}
const char *LineTables::name() const {
    return has_dfa2 ? "dfa-stride2-table" : global ? "dfa-global-table" : wide ? "dfa-wide-table" : "dfa-classed-table";
}
void LineTables::pack(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, Image &img, DeviceTables &t) const {
    pack_dfa_tables(dfa, wide, global, has_dfa2 ? &dfa2 : nullptr, rows, cols, img, t, has_dfa2 && byte_pairs);
}

bool ItemsForms::stride2(const LineTables &lt) {
    if (lt.has_dfa2 && state2 == 0) state2 = lower_dfa2_that_fits(lt.dfa, dfa2, /*items=*/true) ? 1 : 2;
    return state2 == 1;
}
bool ItemsForms::pack(const LineTables &lt, Image &img, dev::LineDfaDevice &t) const { return pack_items(lt.dfa, img, t); }
bool ItemsForms::pack2(const LineTables &lt, Image &img, dev::Dfa2Device &t) {
    return stride2(lt) && pack_dfa2(dfa2, {}, {}, img, t, dev::kDfa2PItemsBytes);
}

void plan_engines(const std::string &pattern, int engine, Programs &p) {
    p.requested = engine;
    p.ref = build_reference_automaton(pattern);
    p.trimmed = trim(p.ref);
    const Reduced red = reduce(p.trimmed);
    const bool nfa_only = engine == RRX_ENGINE_NFA || engine == RRX_ENGINE_NFA_WAVE || engine == RRX_ENGINE_NFA_BLOCK || engine == RRX_ENGINE_NFA_SPARSE;
    if (engine == RRX_ENGINE_AUTO || engine == RRX_ENGINE_NFA) p.has_nfa = lower_nfa(red, dev::kMaxNfaWords * 32, p.nfa, /*allow_carry=*/true, /*gaps=*/true);
    if (!nfa_only) p.has_dfa = lower_dfa(red, kMaxSubsetStates, p.match.dfa) && p.match.decide(engine);      // (DFA, DFA_GLOBAL, DFA2, AUTO)
    // the wave-cooperative form: when asked for, or as the last resort of AUTO
    if (engine == RRX_ENGINE_NFA_WAVE || (engine == RRX_ENGINE_AUTO && !p.has_nfa && !p.has_dfa))
        p.has_wave = lower_nfa(red, dev::kGroupMaxBits, p.nfa_wave, /*allow_carry=*/false, /*gaps=*/true);
    // the wave-resident form (any automaton up to 65536 positions): when asked for, or when nothing else took it
    if (engine == RRX_ENGINE_NFA_BLOCK || engine == RRX_ENGINE_NFA_SPARSE || (engine == RRX_ENGINE_AUTO && !p.has_nfa && !p.has_dfa && !p.has_wave))
        p.has_block = lower_nfa(red, dev::kBlockMaxBits, p.nfa_block, /*allow_carry=*/false, /*gaps=*/true);
    // AUTO: the LDS-resident table when it fits, else the register-resident NFA, else the table in global memory
    if (engine == RRX_ENGINE_NFA) p.engine = p.has_nfa ? RRX_ENGINE_NFA : 0;
    else if (engine == RRX_ENGINE_DFA || engine == RRX_ENGINE_DFA_GLOBAL) p.engine = p.has_dfa ? RRX_ENGINE_DFA : 0;
    else if (engine == RRX_ENGINE_NFA_WAVE) p.engine = p.has_wave ? RRX_ENGINE_NFA_WAVE : 0;
    else if (engine == RRX_ENGINE_NFA_BLOCK || engine == RRX_ENGINE_NFA_SPARSE) p.engine = p.has_block ? engine : 0;
    else if (engine == RRX_ENGINE_DFA2) p.engine = p.match.has_dfa2 ? RRX_ENGINE_DFA : 0;
    else p.engine = (p.has_dfa && !p.match.global) ? RRX_ENGINE_DFA : p.has_nfa ? RRX_ENGINE_NFA : p.has_dfa ? RRX_ENGINE_DFA
                    : p.has_wave ? RRX_ENGINE_NFA_WAVE : p.has_block ? RRX_ENGINE_NFA_BLOCK : 0;
}
const char *Programs::engine_name() const {
    if (engine == RRX_ENGINE_NFA_WAVE) return "nfa-group-cooperative";
    if (engine == RRX_ENGINE_NFA_BLOCK) return "nfa-wave-resident";
    if (engine == RRX_ENGINE_NFA_SPARSE) return "nfa-wave-sparse";
    return engine == RRX_ENGINE_DFA ? match.name() : "nfa-shift-and";
}
bool Programs::accepts_empty() const {
    return has_nfa ? nfa.accepts_empty : has_wave ? nfa_wave.accepts_empty : has_block ? nfa_block.accepts_empty : match.dfa.accepts_empty;
}

// byte -> column of the line product table: the forward table's class, '\n' the last column
static uint32_t search_line_column(const SearchLineProgram &line, const DfaProgram &fwd, int c) { return c == '\n' ? line.ncols - 1 : fwd.cls[c]; }

bool plan_search(const Reduced &red, bool use_anchored, bool accepts_empty, SearchLdsBytes lds_bytes, SearchPlan &s) {
    s = SearchPlan();
    const bool ok = search_dfas(red, kMaxSubsetStates, s.fwd, s.rev);
    s.nullable = accepts_empty;
    if (ok && !s.nullable) {
        // the product with the anchored table tells the hits whose match starts at the line start (no walk back); a
        // product beyond the row budget: the forward table alone (every hit walks)
        DfaProgram anchored;
        if (!(use_anchored && lower_dfa(red, kMaxSubsetStates, anchored) && lower_search_line(s.fwd, &anchored, 65534, s.line)) &&
            !lower_search_line(s.fwd, nullptr, 65534, s.line))
            s.line = SearchLineProgram();
    }
    if (s.line.nrows) {
        uint32_t column[256];
        for (int c = 0; c < 256; c++) column[c] = search_line_column(s.line, s.fwd, c);
        if (!lower_search_line2(s.line, column, 16383, s.line2)) s.line2 = SearchLine2Program();
    }
    // the stripe-wise kernel's layout of that table: LDS if it fits beside the reverse table, the job pools and a result
    // window, else HBM/L2 (device.hpp: SearchChunkDevice)
    const SearchLine2Program &s2 = s.line2;
    if (s2.nrows && s.fwd.ncls < 128) {
        dev::SearchChunkDevice c = search_chunk_layout(s2, s.fwd, s.rev, /*in_global=*/false);
        bool fits = s2.ncols <= 127 && c.base_row + s2.nrows <= 4096 && lds_bytes(c) <= dev::kSearchChunkLdsBudget;
        if (!fits) {
            c = search_chunk_layout(s2, s.fwd, s.rev, /*in_global=*/true);
            fits = lds_bytes(c) <= dev::kSearchChunkLdsBudget;      // (the reverse table has no global form)
        }
        if (fits) s.layout = c;
    }
    return ok && (s.nullable || s.layout.nrows);
}

bool plan_search_longest(const Reduced &red, bool accepts_empty, SearchLongestPlan &s) {
    s = SearchLongestPlan();
    if (!search_longest_dfas(red, kMaxSubsetStates, s.starts, s.anchored)) return false;
    s.nullable = accepts_empty;
    s.empty = true;
    for (uint8_t a : s.anchored.accepting) s.empty = s.empty && !a;
    return true;
}

bool plan_contains_nfa(const Programs &p, NfaProgram &out) {
    if (p.has_nfa) out = p.nfa;
    else if (!lower_nfa(reduce(p.trimmed), dev::kMaxNfaWords * 32, out, /*allow_carry=*/true, /*gaps=*/true)) return false;
    contains_b_rows(out);
    return true;
}

bool lower_multi_member(const std::string &pattern, DfaProgram &out) {
    return search_fwd_dfa(reduce(trim(build_reference_automaton(pattern))), kMaxSubsetStates, out);
}

void plan_multi(const std::vector<DfaProgram> &members, bool force_global, uint32_t max_rows, MultiPlan &out) {
    out = MultiPlan();
    if (!max_rows || max_rows > kMultiMaxRows) max_rows = kMultiMaxRows;
    auto in_lds = [](const MultiProgram &t) { return dev::multi_lds_bytes(t.nstates, t.ncls) <= dev::kPlainDfaLdsBudget; };
    auto close = [&](MultiGroup &g) {
        g.in_global = force_global || !in_lds(g.table);
        out.groups.push_back(std::move(g));
        g = MultiGroup();
    };
    MultiGroup open;
    for (uint32_t k = 0; k < members.size(); k++) {
        const uint32_t bit = 1u << k;
        MultiProgram with;
        if (open.members && multi_product(open.table, members[k], bit, with) && with.nstates <= max_rows && (force_global || in_lds(with))) {
            open.table = std::move(with);
            open.members |= bit;
            continue;
        }
        if (open.members) close(open);
        (void)multi_product(multi_unit(), members[k], bit, open.table);      // (a member alone: at most kMaxSubsetStates pairs)
        open.members = bit;
    }
    if (open.members) close(open);
}

void append_words(std::vector<uint32_t> &w, const MultiProgram &d) {
    w.insert(w.end(), {d.nstates, d.ncls, d.start, d.first_hit, d.full});
    w.insert(w.end(), d.cls, d.cls + 256);
    w.insert(w.end(), d.next.begin(), d.next.end());
    w.insert(w.end(), d.mask.begin(), d.mask.end());
}

void append_words(std::vector<uint32_t> &w, const NfaProgram &p, bool csr) {
    w.insert(w.end(), {p.W, p.nbits, p.n_exc, p.accepts_empty ? 1u : 0u});
    for (auto *v : {&p.init, &p.fin, &p.chain, &p.self, &p.excm, &p.cgrp, &p.ctgt, &p.B}) w.insert(w.end(), v->begin(), v->end());
    if (!csr) w.insert(w.end(), p.X.begin(), p.X.end());
    else for (auto *v : {&p.xoff, &p.xtgt}) w.insert(w.end(), v->begin(), v->end());
}
void append_words(std::vector<uint32_t> &w, const DfaProgram &d, bool escaped) {
    w.insert(w.end(), {d.nstates, d.ncls, d.start, d.accepts_empty ? 1u : 0u});
    w.insert(w.end(), d.cls, d.cls + 256);
    w.insert(w.end(), d.accepting.begin(), d.accepting.end());
    w.insert(w.end(), d.next.begin(), d.next.end());
    if (escaped) w.insert(w.end(), d.escaped.begin(), d.escaped.end());
}
// (entries: next | result bits << 16 | verdict pairs << 24)
void append_words(std::vector<uint32_t> &w, const Dfa2Program &d, bool pair_dim) {
    w.insert(w.end(), {d.nstates, d.ncols, d.start, d.accepts_empty ? 1u : 0u});
    if (pair_dim) w.push_back(d.pair_dim);
    w.insert(w.end(), d.pair_col.begin(), d.pair_col.end());
    w.insert(w.end(), d.next2.begin(), d.next2.end());
}
void append_words(std::vector<uint32_t> &w, const SearchLineProgram &d, const DfaProgram &fwd) {
    w.insert(w.end(), {d.nrows, d.ncols, d.start, d.skip});
    for (int c = 0; c < 256; c++) w.push_back(search_line_column(d, fwd, c));
    w.insert(w.end(), d.table.begin(), d.table.end());
}
void append_words(std::vector<uint32_t> &w, const SearchLine2Program &d, const dev::SearchChunkDevice &layout) {
    w.insert(w.end(), {d.nrows, d.ncols, d.start, d.skip, layout.nrows ? (layout.in_global ? 2u : 1u) : 0u});
    w.insert(w.end(), d.pair_col.begin(), d.pair_col.end());
    w.insert(w.end(), d.first.begin(), d.first.end());
    w.insert(w.end(), d.all.begin(), d.all.end());
}

}  // namespace rrx
