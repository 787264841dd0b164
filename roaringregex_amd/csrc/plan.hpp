// plan.hpp — the decisions between a pattern and its device images (host only: no HIP): which programs are lowered for a
// requested engine and which engine AUTO ends on, which forms of a DFA table fit the device, how the search tables are planned,
// and how a program is dumped as words (rrx_program_words).  The fit rules are stated here or nowhere: the ABI layer (regex.cpp) and the
// sanitizer driver (tests/cpp/host_pipeline_driver.cpp) both call them.
#pragma once
#include <string>
#include <vector>

#include "device.hpp"
#include "lower.hpp"
#include "pack.hpp"

namespace rrx {

constexpr uint32_t kMaxSubsetStates = 16384;   // subset construction is abandoned beyond this

// The stride-2 size rule: the table (rows of `ncols | 1` entries) fits the LDS region next to the pair table.
size_t dfa2_table_bytes(const Dfa2Program &d);
bool dfa2_fits(const Dfa2Program &d);
// The stride-2 form of `d` (items: lower_dfa2's items form) if there is one that fits: at most 4096 states, 1024 pair columns.
bool lower_dfa2_that_fits(const DfaProgram &d, Dfa2Program &out, bool items = false);

// Which forms of a line table fit the device (the driver packs every one that does; decide() picks among them)
bool wide_fits(const DfaProgram &d);           // byte-indexed rows
bool classed_fits(const DfaProgram &d);        // class-indexed rows in LDS
bool global_fits(const DfaProgram &d);         // class-indexed rows in global memory

// A DFA as the batch kernels run it: the byte-stride line table in one of its forms and, where it fits, the stride-2 table.
struct LineTables {
    DfaProgram dfa;
    Dfa2Program dfa2;
    bool has_dfa2 = false;
    bool byte_pairs = false;     // the stride-2 table also gets the byte-wide pair table (pack.hpp: dfa2_byte_pairs_fit)
    bool wide = false;          // byte-indexed rows (<= kWideMaxStates states) or class-indexed rows
    bool global = false;         // class-indexed table too large for LDS, kept in global memory
    // The forms of `dfa` under the requested RRX_ENGINE_*; false: no table (the global form holds 2^24 entries).
    bool decide(int requested_engine);
    const char *name() const;    // (stride-2: the byte-stride table still serves corpora with bytes >= 0x80)
    // rows / cols: the order of the stride-2 table in LDS (empty: as numbered)
    void pack(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, Image &img, DeviceTables &t) const;
};

// The items tables of one LineTables, host side (explicit items stepped stripe-wise: kernels_items.hip).  The byte-stride form is
// pack_items on the table's DFA.  The stride-2 form (items with a separator byte each, trim 1) is lower_dfa2's items form - one
// symbol more than the line table's -, lowered at its first use, and only where the line table has a stride-2 form at all.
struct ItemsForms {
    Dfa2Program dfa2;            // the stride-2 items program (where stride2() holds)
    bool stride2(const LineTables &lt);          // false: `lt` has no stride-2 form, or the items form does not fit the same LDS region
    bool pack(const LineTables &lt, Image &img, dev::LineDfaDevice &t) const;       // false: more states than 16-bit row offsets allow
    bool pack2(const LineTables &lt, Image &img, dev::Dfa2Device &t);               // false: no stride2()
private:
    int state2 = 0;              // 0 not tried, 1 there, 2 does not fit
};

// What a pattern compiles to.  `engine`: the RRX_ENGINE_* it runs on, 0 where none admits the automaton.
struct Programs {
    RefAutomaton ref;
    Trimmed trimmed;
    bool has_nfa = false, has_dfa = false;
    NfaProgram nfa;
    NfaProgram nfa_wave;         // up to 4096 positions, no carry groups (wave-cooperative engine)
    bool has_wave = false;
    NfaProgram nfa_block;        // up to 65536 positions, exception edges in CSR form (wave-resident engine)
    bool has_block = false;
    LineTables match;
    int requested = 0;           // the RRX_ENGINE_* asked for (plan_engines)
    int engine = 0;
    const char *engine_name() const;
    bool accepts_empty() const;
};
// Lowers what the requested RRX_ENGINE_* needs and picks the engine; throws what the front end and the lowering throw.
void plan_engines(const std::string &pattern, int requested_engine, Programs &out);

// The search tables: the forward "anything, then the pattern" DFA and the reverse DFA, the line product table (nrows = 0: not
// built), its stride-2 form, what the stripe-wise kernel runs, and that kernel's layout of it without the pointers.
struct SearchPlan {
    DfaProgram fwd, rev;
    SearchLineProgram line;
    SearchLine2Program line2;
    dev::SearchChunkDevice layout;
    bool nullable = false;       // the pattern accepts the empty string: every offset is a match, no table (empty_matches)
};
// `lds_bytes`: what the kernel needs of the LDS for a layout (dev::search_chunks_lds_bytes; the arithmetic lives with the kernel).
// false: the tables do not fit the device; fwd / rev are built all the same where they determinise (rrx_program_words).
using SearchLdsBytes = size_t (*)(const dev::SearchChunkDevice &);
bool plan_search(const Reduced &red, bool use_anchored, bool accepts_empty, SearchLdsBytes lds_bytes, SearchPlan &out);

// The tables of the leftmost-longest search per item (lower.hpp: search_longest_dfas).  No fit rule: the lane-per-item kernel takes
// plain tables of any size (LDS or HBM/L2).
struct SearchLongestPlan {
    DfaProgram starts, anchored;
    bool nullable = false;       // the pattern accepts the empty string: start = 0 everywhere, the starts table is not stepped
    bool empty = false;          // the empty language (no accepting state in `anchored`): no match anywhere, no table
};
// false: one of the two tables does not determinise within kMaxSubsetStates (both stay empty).
bool plan_search_longest(const Reduced &red, bool accepts_empty, SearchLongestPlan &out);

// The program of contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA; RRX_PROGRAM_CONTAINS_NFA dumps it): the lane program of the
// pattern - p.nfa where the regex has one, else lowered here with the lane engine's limits, whatever engine the regex was compiled
// for - with the contains B rows (pack.hpp: contains_b_rows).  false: no lane program (more than kMaxNfaWords * 32 positions).
bool plan_contains_nfa(const Programs &p, NfaProgram &out);

// A pattern set (rrx_multi): its members' forward search tables in set order, cut into GROUPS of members that share one product table.
constexpr uint32_t kMultiMaxPatterns = 32;
struct MultiGroup {
    MultiProgram table;
    uint32_t members = 0;        // bit k: member k of the set is in this group (= what table.full can reach, and the empty languages)
    bool in_global = false;      // the table stays in HBM/L2: asked for, or one member alone is beyond the LDS budget
};
struct MultiPlan {
    std::vector<MultiGroup> groups;
};
// The table of one member from its pattern: the front end, then the forward search table ("any bytes, then the pattern").  Throws
// what the front end and the lowering throw; false where the forward table does not determinise within kMaxSubsetStates.
bool lower_multi_member(const std::string &pattern, DfaProgram &out);
// Greedy in set order: member k joins the open group if the minimised product with it has at most max_rows rows (0: kMultiMaxRows)
// and - unless force_global - its LDS form fits kPlainDfaLdsBudget; else the group closes and k opens the next one.  A member is
// always admitted to a group of its own, so every set of members compiles.
void plan_multi(const std::vector<DfaProgram> &members, bool force_global, uint32_t max_rows, MultiPlan &out);

// rrx_program_words: the word layouts that tests/program_replay.py reads.
void append_words(std::vector<uint32_t> &w, const NfaProgram &p, bool csr);                   // csr: xoff / xtgt in the place of X
void append_words(std::vector<uint32_t> &w, const DfaProgram &d, bool escaped = false);       // escaped: then the escaped flag per state
void append_words(std::vector<uint32_t> &w, const Dfa2Program &d, bool pair_dim = false);     // pair_dim: a fifth header word
void append_words(std::vector<uint32_t> &w, const SearchLineProgram &d, const DfaProgram &fwd);
void append_words(std::vector<uint32_t> &w, const SearchLine2Program &d, const dev::SearchChunkDevice &layout);
// rrx_multi_program_words: [nstates, ncls, start, first_hit, full], cls[256], next[nstates][ncls], mask[nstates]
void append_words(std::vector<uint32_t> &w, const MultiProgram &d);

}  // namespace rrx
