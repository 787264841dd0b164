// lower_tables.cpp — the table forms the kernels read: line-mode search table, stride-2 tables (see lower.hpp).
#include "lower_internal.hpp"

namespace rrx {

namespace {

// The columns of a stride-2 table (the image of every row under one symbol pair) -> ids in first-seen order; symbol pairs that
// act alike on every row share one.  Hash buckets with a full comparison.
struct ColumnInterner {
    std::unordered_map<uint64_t, std::vector<uint32_t>> by_hash;    // hash of a column -> columns with that hash
    std::vector<std::vector<uint32_t>> cols;
    // the id of `col`; -1 where it is new and max_cols columns are held already
    int64_t intern(const std::vector<uint32_t> &col, uint32_t max_cols) {
        uint64_t h = 1469598103934665603ull;
        for (uint32_t v : col) h = (h ^ v) * 1099511628211ull;
        std::vector<uint32_t> &bucket = by_hash[h];
        for (uint32_t cand : bucket) if (cols[cand] == col) return cand;
        if (cols.size() >= max_cols) return -1;
        bucket.push_back((uint32_t)cols.size());
        cols.push_back(col);
        return (int64_t)cols.size() - 1;
    }
    // the entries [from, from + R) of every column as a table [R][columns]
    std::vector<uint32_t> by_rows(uint32_t R, size_t from = 0) const {
        const size_t C = cols.size();
        std::vector<uint32_t> t(R * C);
        for (size_t c = 0; c < C; c++) for (uint32_t r = 0; r < R; r++) t[r * C + c] = cols[c][from + r];
        return t;
    }
};

// pair_col[dim][dim]: the column of the byte pair (c1, c2), from sym_pair_col[nsyms][nsyms] and the bytes' symbols sym[dim]
std::vector<uint16_t> byte_pair_columns(const std::vector<uint32_t> &sym_pair_col, uint32_t nsyms, const uint32_t *sym, unsigned dim) {
    std::vector<uint16_t> pair_col((size_t)dim * dim);
    for (unsigned c1 = 0; c1 < dim; c1++)
        for (unsigned c2 = 0; c2 < dim; c2++) pair_col[c1 * dim + c2] = (uint16_t)sym_pair_col[(size_t)sym[c1] * nsyms + sym[c2]];
    return pair_col;
}

}  // namespace

// Line-mode search table: the product of the sticky forward table (where does the first match END) and the anchored table
// of the pattern itself (is the line's prefix up to here accepted: then the match STARTS at the line start and no walk back
// is needed).  Rows = reachable pairs + SKIP (last), columns = byte classes + '\n' (last).
bool lower_search_line(const DfaProgram &fwd, const DfaProgram *anchored, uint32_t max_rows, SearchLineProgram &o) {
    o = SearchLineProgram();
    const uint32_t K = fwd.ncls;
    if ((anchored && anchored->ncls != K) || fwd.accepting[fwd.start]) return false;   // (patterns that accept "" take another path)
    // without the anchored table: a one-state stand-in that accepts nothing - the rows are the forward states, no hit is anchored
    const DfaProgram none = dead_dfa(fwd);
    const DfaProgram &anch = anchored ? *anchored : none;
    PairInterner rows;                                                    // (anchored state, sticky state) -> row
    const std::vector<std::pair<uint32_t, uint32_t>> &pairs = rows.pairs;
    const size_t cap = max_rows ? max_rows - 1 : 0;                       // a new pair is refused when pairs + SKIP would reach max_rows
    if (rows.intern(anch.start, fwd.start, cap) < 0) return false;
    std::vector<uint32_t> raw;                                            // [pair][K]: next pair | flags, SKIP = 0xffff
    for (size_t cur = 0; cur < pairs.size(); cur++) {
        const uint32_t a = pairs[cur].first, f = pairs[cur].second;
        raw.resize((cur + 1) * K);
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t a2 = k ? anch.next[(size_t)a * K + k] : 0u;  // class 0 kills the anchored run
            const uint32_t f2 = fwd.next[(size_t)f * K + k];
            if (fwd.accepting[f2]) raw[cur * K + k] = 0xffffu | kSearchHit | (anch.accepting[a2] ? kSearchAnchored : 0u);
            else {
                const int64_t id = rows.intern(a2, f2, cap);
                if (id < 0) return false;
                raw[cur * K + k] = (uint32_t)id;
            }
        }
    }
    const uint32_t P = (uint32_t)pairs.size();
    o.nrows = P + 1; o.ncols = K + 1; o.start = 0; o.skip = P;
    o.table.assign((size_t)o.nrows * o.ncols, 0);
    for (uint32_t r = 0; r < P; r++) {
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t v = raw[(size_t)r * K + k];
            o.table[(size_t)r * o.ncols + k] = ((v & 0xffffu) == 0xffffu ? P : (v & 0xffffu)) | (v & 0xffff0000u);
        }
        o.table[(size_t)r * o.ncols + K] = o.start | kSearchNewline;
    }
    for (uint32_t k = 0; k < K; k++) o.table[(size_t)P * o.ncols + k] = P;
    o.table[(size_t)P * o.ncols + K] = o.start | kSearchNewline;
    return true;
}

// Stride-2 form of the line-mode search table: both forms (first match: a hit leads to SKIP; all matches: back to the start
// row) composed with themselves, the pair columns shared between them so that one pair table serves both.
bool lower_search_line2(const SearchLineProgram &s, const uint32_t *column, uint32_t max_cols, SearchLine2Program &o) {
    o = SearchLine2Program();
    const uint32_t R = s.nrows, C = s.ncols;
    if (!R || (uint64_t)C * C * R > ((uint64_t)1 << 28)) return false;              // (host work: two passes over C * C * R entries)
    o.nrows = R; o.start = s.start; o.skip = s.skip;
    auto flags_of = [](uint32_t v) -> uint32_t { return (v & kSearchNewline) ? 1u : (v & kSearchHit) ? ((v & kSearchAnchored) ? 3u : 2u) : 0u; };
    // one step of either form: -> next row, flags
    auto step = [&](uint32_t row, uint32_t sym, bool restart, uint32_t &f) -> uint32_t {
        const uint32_t v = s.table[(size_t)row * C + sym];
        f = flags_of(v);
        return (restart && (f & 2u)) ? s.start : (v & 0xffffu);
    };
    ColumnInterner columns;                                                         // [column][2 * R]: the first form, then the restart form
    std::vector<uint32_t> sym_pair_col((size_t)C * C);
    std::vector<uint32_t> col(2 * (size_t)R);
    for (uint32_t a = 0; a < C; a++)
        for (uint32_t b = 0; b < C; b++) {
            for (uint32_t form = 0; form < 2; form++)
                for (uint32_t r = 0; r < R; r++) {
                    uint32_t f1, f2;
                    const uint32_t r1 = step(r, a, form != 0, f1);
                    const uint32_t r2 = step(r1, b, form != 0, f2);
                    col[(size_t)form * R + r] = r2 | (f1 << 2 | f2) << 24;
                }
            const int64_t id = columns.intern(col, max_cols);
            if (id < 0) return false;
            sym_pair_col[(size_t)a * C + b] = (uint32_t)id;
        }
    o.ncols = (uint32_t)columns.cols.size();
    o.first = columns.by_rows(R);
    o.all = columns.by_rows(R, R);
    o.pair_col = byte_pair_columns(sym_pair_col, C, column, 128);
    return true;
}

// ------------------------------------------------------------------------------------------ stride-2 lowering
bool lower_dfa2(const DfaProgram &d, uint32_t max_cols, Dfa2Program &o, bool items) {
    o = Dfa2Program();
    const uint32_t D = d.nstates, K = d.ncls, NL = K;            // symbols 0..K-1 = byte classes, K = '\n'
    o.nstates = D; o.start = d.start; o.accepts_empty = d.accepts_empty;
    const bool two_bit = !d.escaped.empty();                     // a line end reports (accepted, escaped)
    const uint32_t kb = two_bit ? 2u : 1u;
    auto step = [&](uint32_t s, uint32_t sym, uint32_t &line, uint32_t &verdict) -> uint32_t {
        if (sym == NL) { line = 1; verdict = two_bit ? (uint32_t)d.accepting[s] << 1 | d.escaped[s] : d.accepting[s]; return d.start; }
        line = 0; verdict = 0;
        return d.next[(size_t)s * K + sym];
    };
    ColumnInterner columns;
    std::vector<uint32_t> sym_pair_col((size_t)(K + 1) * (K + 1));
    std::vector<uint32_t> col(D);
    for (uint32_t a = 0; a <= K; a++)
        for (uint32_t b = 0; b <= K; b++) {
            for (uint32_t s = 0; s < D; s++) {
                uint32_t l1, v1, l2, v2;
                const uint32_t s1 = step(s, a, l1, v1);
                const uint32_t s2 = step(s1, b, l2, v2);
                const uint32_t verdicts = (l1 && l2) ? (v1 << kb | v2) : l1 ? v1 : v2;
                col[s] = s2 | ((l1 + l2) * kb) << 16 | verdicts << 24;
            }
            const int64_t id = columns.intern(col, max_cols);
            if (id < 0) return false;
            sym_pair_col[(size_t)a * (K + 1) + b] = (uint32_t)id;
        }
    o.ncols = (uint32_t)columns.cols.size();
    o.next2 = columns.by_rows(D);
    // what ends a line: the code 128 of the items form ('\n' is an ordinary byte there), '\n' of the line form
    o.pair_dim = items ? 129u : 128u;
    uint32_t sym[129];
    for (unsigned c = 0; c < 128; c++) sym[c] = d.cls[c];
    sym[items ? 128 : '\n'] = NL;
    o.pair_col = byte_pair_columns(sym_pair_col, K + 1, sym, o.pair_dim);
    return true;
}

}  // namespace rrx
