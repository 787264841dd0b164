// host_pipeline_driver.cpp — runs the host compile pipeline (pattern -> reference-numbered automaton -> trim ->
// reduce -> NFA / DFA / stride-2 programs) over the patterns given on stdin, one per line.  Built by
// tests/test_lowering.py with -fsanitize=address,undefined (sanitizers run on the CPU build only) from
// csrc/frontend.cpp + csrc/lower.cpp + csrc/pack.cpp: no HIP involved.  Prints one summary line per pattern.
//
// Every device image whose preconditions the programs meet is packed (csrc/pack.hpp), copied, bound to the copy and decoded
// back here - independently of the packer - against the program it was packed from.  A mismatch aborts; the line before
// "done" counts the images checked per kind.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "frontend.hpp"
#include "lower.hpp"
#include "pack.hpp"

using namespace rrx;

namespace {

#define CHECK(cond)                                                                                               \
    do {                                                                                                          \
        if (!(cond)) { std::fprintf(stderr, "image check failed: %s (line %d)\n", #cond, __LINE__); std::abort(); } \
    } while (0)

struct Counts { size_t line = 0, stride2 = 0, items = 0, search = 0, lane = 0, group = 0, wave = 0, sparse = 0; } g_n;

// the image as the device would hold it: a copy of its bytes, the descriptors bound to the copy
struct Copy {
    std::vector<uint8_t> bytes;
    explicit Copy(const Image &img) : bytes(img.bytes) { img.bind(bytes.data()); }
    size_t at(const void *p) const { return (size_t)(static_cast<const uint8_t *>(p) - bytes.data()); }
};

bool bit(const std::vector<uint32_t> &v, uint32_t b) { return (v[b >> 5] >> (b & 31)) & 1u; }

// lane l reads copy l % R of every entry: all R copies of entry i (at dword i * R + k) must agree, offsets + 4 k
void check_line(const DfaProgram &dfa, bool wide, bool global) {
    Image img;
    DeviceTables t;
    pack_dfa_tables(dfa, wide, global, nullptr, {}, {}, img, t);
    Copy cp(img);
    const dev::LineDfaDevice &L = t.line;
    const uint32_t R = 1u << L.rep_log2, S = L.stride / R, K = dfa.ncls;
    CHECK(L.wide == (wide ? 1u : 0u) && L.in_global == (global ? 1u : 0u) && L.nrows == dfa.nstates && (!global || R == 1));
    const uint32_t row_unit = global ? S : S * 4 * R;                 // global: entry index of a row; LDS: its byte offset
    const uint32_t nl_bit = global ? 30 : 16, acc_bit = global ? 31 : 24, field = global ? 0x3fffffffu : 0xffffu;
    CHECK(L.start_off == dfa.start * row_unit);
    CHECK(cp.at(t.dfa.cls) + 256 <= cp.bytes.size() && t.dfa.nstates == dfa.nstates);
    for (int c = 0; c < 256; c++) CHECK(t.dfa.cls[c] == dfa.cls[c] && L.cls[c] == (c == '\n' ? K : dfa.cls[c]));
    for (size_t i = 0; i < dfa.next.size(); i++) CHECK(t.dfa.next[i] == dfa.next[i]);
    for (uint32_t d = 0; d < dfa.nstates; d++) CHECK(t.dfa.acc[d] == dfa.accepting[d]);
    for (uint32_t d = 0; d < dfa.nstates; d++)
        for (uint32_t c = 0; c < (wide ? 128u : 256u); c++) {
            const uint32_t col = wide ? c : L.cls[c];
            const uint32_t want_row = c == '\n' ? dfa.start : dfa.next[(size_t)d * K + dfa.cls[c]];
            const uint32_t want_flags = c == '\n' ? (1u << nl_bit | (dfa.accepting[d] ? 1u << acc_bit : 0u)) : 0u;
            for (uint32_t k = 0; k < R; k++) {
                const uint32_t e = L.table[((size_t)d * S + col) * R + k];
                CHECK((e & field) == want_row * row_unit + 4 * k && (e & ~field) == want_flags);
            }
        }
    g_n.line++;
}

// a stride-2 table in the order rows / cols (empty: as numbered): every (state, pair) through P and the slots gives next2
void check_dfa2(const Dfa2Program &p, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t p_region) {
    Image img;
    dev::Dfa2Device d;
    CHECK(pack_dfa2(p, rows, cols, img, d, p_region));
    Copy cp(img);
    const bool ordered = !rows.empty();
    auto rs = [&](uint32_t s) { return ordered ? rows[s] : s; };
    auto cs = [&](uint32_t c) { return ordered ? cols[c] : c; };
    const uint32_t R = 1u << d.rep_log2, dim = p.pair_dim;
    CHECK(d.nrows == p.nstates && d.stride == (p.ncols | 1u) * R && d.start_off == rs(p.start) * d.stride * 4);
    CHECK(cp.at(d.P) == 0 && cp.at(d.T2) == (p_region ? p_region : ((dim * dev::kDfa2PStride * 2 + 15) & ~15u)));
    for (uint32_t c1 = 0; c1 < dim; c1++)
        for (uint32_t c2 = 0; c2 < dev::kDfa2PStride; c2++)
            CHECK(d.P[c1 * dev::kDfa2PStride + c2] == (c2 < dim ? cs(p.pair_col[c1 * dim + c2]) * 4 * R : 0u));
    for (size_t b = dim * dev::kDfa2PStride * 2; b < cp.at(d.T2); b++) CHECK(cp.bytes[b] == 0);     // (the items form's P region)
    for (uint32_t s = 0; s < p.nstates; s++)
        for (uint32_t c = 0; c < p.ncols; c++) {
            const uint32_t v = p.next2[(size_t)s * p.ncols + c];
            for (uint32_t k = 0; k < R; k++) {
                const uint32_t e = d.T2[(rs(s) * d.stride * 4 + cs(c) * 4 * R + 4 * k) / 4];
                CHECK((e & 0xffffu) == rs(v & 0xffffu) * d.stride * 4 + 4 * k && (e & 0xffff0000u) == (v & 0xffff0000u));
            }
        }
    g_n.stride2++;
}

// a seeded random order of the table's rows (state 0 keeps slot 0) and columns
void random_order(const Dfa2Program &p, std::mt19937 &rng, std::vector<uint32_t> &rows, std::vector<uint32_t> &cols) {
    rows.resize(p.nstates); cols.resize(p.ncols);
    for (uint32_t i = 0; i < p.nstates; i++) rows[i] = i;
    for (uint32_t i = 0; i < p.ncols; i++) cols[i] = i;
    if (p.nstates > 1) std::shuffle(rows.begin() + 1, rows.end(), rng);
    std::shuffle(cols.begin(), cols.end(), rng);
}

void check_items(const DfaProgram &dfa) {
    Image img;
    dev::LineDfaDevice L;
    if (!pack_items(dfa, img, L)) return;
    Copy cp(img);
    const uint32_t R = 1u << L.rep_log2, S = L.stride / R, row_bytes = L.stride * 4;
    CHECK(S == dev::kItemColumns && L.wide == 1 && L.start_off == dfa.start * row_bytes);
    for (uint32_t q = 0; q < dfa.nstates; q++)
        for (uint32_t c = 0; c <= dev::kItemEndColumn; c++) {
            uint32_t want;
            if (c == dev::kItemEndColumn) want = dfa.start * row_bytes | 1u << 16 | (dfa.accepting[q] ? 1u << 24 : 0u);
            else {
                const uint32_t nx = dfa.next[(size_t)q * dfa.ncls + dfa.cls[c]];         // (column 128: any byte >= 0x80)
                want = nx * row_bytes | (dfa.accepting[nx] ? 0x80u << 16 : 0u);
            }
            for (uint32_t k = 0; k < R; k++) CHECK(L.table[((size_t)q * S + c) * R + k] == want + 4 * k);
        }
    g_n.items++;
}

void check_search(const SearchLine2Program &s2, const DfaProgram &fwd, const DfaProgram &rev, bool in_global) {
    const dev::SearchChunkDevice layout = search_chunk_layout(s2, fwd, rev, in_global);
    if (!in_global && (s2.ncols > 127 || layout.base_row + s2.nrows > 4096)) return;
    Image img;
    dev::SearchChunkDevice d;
    pack_search(s2, fwd, rev, layout, img, d);
    Copy cp(img);
    CHECK(d.nrows == s2.nrows && d.ncols2 == s2.ncols && d.start_row == s2.start && d.skip_row == s2.skip && d.in_global == (in_global ? 1u : 0u));
    CHECK(d.nr == rev.nstates && d.ncls == fwd.ncls && d.start_r == rev.start);
    for (int c = 0; c < 256; c++) CHECK(d.cls[c] == fwd.cls[c]);
    for (uint32_t c1 = 0; c1 < 128; c1++)
        for (uint32_t c2 = 0; c2 < 128; c2++) {
            const uint32_t col = s2.pair_col[c1 * 128 + c2];
            CHECK(in_global ? d.P16[c1 * dev::kSearchP16Stride + c2] == 4 * col : d.P8[c1 * dev::kSearchP8Stride + c2] == 2 * col);
        }
    CHECK((d.row_bytes / 4) % 2 == 1 || in_global);
    for (int form = 0; form < 2; form++) {                         // first match, all matches
        const std::vector<uint32_t> &src = form ? s2.all : s2.first;
        const uint16_t *T = form ? d.T2_all : d.T2;
        const uint32_t *G = form ? d.G2_all : d.G2;
        for (uint32_t r = 0; r < s2.nrows; r++)
            for (uint32_t c = 0; c < s2.ncols; c++) {
                const uint32_t v = src[(size_t)r * s2.ncols + c], next = v & 0xffffffu, events = v >> 24;
                if (in_global) {
                    const uint32_t e = G[(size_t)r * s2.ncols + c];
                    CHECK((e & 0x0fffffffu) == next * s2.ncols * 4 && e >> 28 == events);
                } else {
                    const uint32_t e = T[(size_t)r * (d.row_bytes / 2) + c];
                    CHECK(e >> 4 == d.base_row + next && (e & 15u) == events);
                }
            }
    }
    for (size_t i = 0; i < (size_t)rev.nstates * rev.ncls; i++) {
        const uint16_t nx = rev.next[i];
        CHECK((d.rev[i] & 0x7fffu) == nx && ((d.rev[i] >> 15) != 0) == (rev.accepting[nx] != 0));
    }
    g_n.search++;
}

void check_masks(const NfaProgram &p, const uint32_t *M, uint32_t WP) {
    const std::vector<uint32_t> *src[3] = {&p.fin, &p.self, &p.excm};
    for (int k = 0; k < 3; k++)
        for (uint32_t w = 0; w < WP; w++) CHECK(M[(size_t)k * WP + w] == (w < p.W ? (*src[k])[w] : 0u));
}

void check_lane(const NfaProgram &p) {
    Image img;
    dev::NfaDevice d;
    pack_lane_nfa(p, img, d);
    Copy cp(img);
    const uint32_t WP = d.W;
    CHECK(WP >= p.W && WP <= (uint32_t)dev::kMaxNfaWords && d.nbits == p.nbits);
    CHECK(d.any_exc == (p.n_exc ? 1u : 0u) && d.any_carry == (p.n_carry ? 1u : 0u));
    bool any_self = false;
    const std::vector<uint32_t> *src[7] = {&p.init, &p.fin, &p.chain, &p.self, &p.excm, &p.cgrp, &p.ctgt};
    const uint32_t *dst[7] = {d.masks.init, d.masks.fin, d.masks.chain, d.masks.self, d.masks.excm, d.masks.cgrp, d.masks.ctgt};
    for (int k = 0; k < 7; k++)
        for (uint32_t w = 0; w < (uint32_t)dev::kMaxNfaWords; w++) CHECK(dst[k][w] == (w < p.W ? (*src[k])[w] : 0u));
    for (uint32_t w = 0; w < p.W; w++) any_self |= p.self[w] != 0;
    CHECK(d.any_self == (any_self ? 1u : 0u));
    for (uint32_t c = 0; c < 256; c++)
        for (uint32_t w = 0; w < WP; w++) CHECK(d.B[c * WP + w] == (w < p.W ? p.B[(size_t)c * p.W + w] : 0u));
    for (uint32_t b = 0; b < p.nbits; b++)
        for (uint32_t w = 0; w < WP; w++) CHECK(d.X[(size_t)b * WP + w] == (w < p.W ? p.X[(size_t)b * p.W + w] : 0u));
    g_n.lane++;
}

// the exception targets of position b as a set of WP words
std::vector<uint32_t> targets(const NfaProgram &p, uint32_t b, uint32_t WP) {
    std::vector<uint32_t> row(WP, 0);
    for (uint32_t i = p.xoff[b]; i < p.xoff[b + 1]; i++) row[p.xtgt[i] >> 5] |= 1u << (p.xtgt[i] & 31);
    return row;
}

void check_group(const NfaProgram &p, const Trimmed &t) {
    Image img;
    dev::GroupNfaDevice d;
    if (!pack_group_nfa(p, t, img, d)) return;
    Copy cp(img);
    const uint32_t WP = d.G * d.K;
    CHECK(WP * 32 >= p.nbits && d.nbits == p.nbits && d.ncls == t.ncls);
    check_masks(p, d.masks, WP);
    for (int c = 0; c < 256; c++) CHECK(d.cls[c] == ((c == 0 || c >= 128) ? 0 : t.cls[c]));
    for (uint32_t cl = 0; cl < t.ncls; cl++)
        for (uint32_t w = 0; w < WP; w++) CHECK(d.Bcls[(size_t)cl * WP + w] == (cl && w < p.W ? p.B[(size_t)t.cls_rep[cl] * p.W + w] : 0u));
    uint32_t rows = 0;
    for (uint32_t b = 0; b < p.nbits; b++) {
        if (!bit(p.excm, b)) { CHECK(d.xidx[b] == 0xffff); continue; }
        CHECK(d.xidx[b] == rows);
        const std::vector<uint32_t> want = targets(p, b, WP);
        for (uint32_t w = 0; w < WP; w++) CHECK(d.X[(size_t)rows * WP + w] == want[w]);
        rows++;
    }
    CHECK(d.n_exc == rows);
    g_n.group++;
}

void check_wave(const NfaProgram &p, const Trimmed &t, bool sparse) {
    const uint32_t need = (p.W + 63) / 64;
    uint32_t WL = 0;
    for (uint32_t w : {1u, 2u, 3u, 4u, 6u, 8u, 12u, 16u, 24u, 32u})
        if (!WL && need <= w && (!sparse || (w & (w - 1)) == 0)) WL = w;
    if (!WL) return;
    Image img;
    dev::WaveNfaDevice d;
    pack_wave_nfa(p, t, WL, sparse, img, d);
    Copy cp(img);
    const uint32_t WP = 64 * WL;
    CHECK(d.WL == WL && d.nbits == p.nbits);
    check_masks(p, d.masks, WP);
    for (uint32_t c = 0; c < 257; c++)
        for (uint32_t w = 0; w < WP; w++)
            CHECK(d.Bbyte[(size_t)c * WP + w] == (c == 256 ? (w == 0 ? 1u : 0u) : (c && c < 128 && w < p.W) ? p.B[(size_t)c * p.W + w] : 0u));
    for (size_t b = 0; b < p.xoff.size(); b++) CHECK(d.xoff[b] == p.xoff[b]);
    for (size_t i = 0; i < p.xtgt.size(); i++) CHECK(d.xtgt[i] == p.xtgt[i]);
    if (sparse) {
        CHECK(d.ncls == t.ncls);
        for (int c = 0; c < 256; c++) CHECK(d.cls[c] == t.cls[c]);
        for (uint32_t k = 0; k < t.ncls; k++)
            for (uint32_t w = 0; w < WP; w++) CHECK(d.Bcls[(size_t)k * WP + w] == (k && w < p.W ? p.B[(size_t)t.cls_rep[k] * p.W + w] : 0u));
    } else {
        CHECK(!d.Bcls && !d.cls && d.ncls == 0);
    }
    (sparse ? g_n.sparse : g_n.wave)++;
}

void check_images(const Trimmed &t, const Reduced &r, const NfaProgram *nfa, const NfaProgram *wave, const DfaProgram *dfa,
                  const Dfa2Program *dfa2, std::mt19937 &rng) {
    if (nfa) check_lane(*nfa);
    if (wave) { check_group(*wave, t); check_wave(*wave, t, false); check_wave(*wave, t, true); }
    if (dfa) {
        const size_t classed = (size_t)dfa->nstates * (dfa->ncls + 2);
        if (dfa->nstates <= dev::kWideMaxStates) check_line(*dfa, true, false);
        if (classed <= dev::kClassedMaxEntries) check_line(*dfa, false, false);
        if (classed < ((size_t)1 << 24)) check_line(*dfa, false, true);
        check_items(*dfa);
        Dfa2Program items;
        if (dfa2 && lower_dfa2(*dfa, 1024, items, /*items=*/true) && (size_t)items.nstates * (items.ncols | 1u) * 4 <= dev::kDfa2MaxTable)
            check_dfa2(items, {}, {}, dev::kDfa2PItemsBytes);
    }
    if (dfa2 && (size_t)dfa2->nstates * (dfa2->ncols | 1u) * 4 <= dev::kDfa2MaxTable) {
        std::vector<uint32_t> rows, cols;
        check_dfa2(*dfa2, rows, cols, 0);
        random_order(*dfa2, rng, rows, cols);
        check_dfa2(*dfa2, rows, cols, 0);
    }
    DfaProgram fwd, rev, anchored;
    if (!search_dfas(r, 16384, fwd, rev) || fwd.ncls >= 128) return;
    SearchLineProgram line;
    if (!(lower_dfa(r, 16384, anchored) && lower_search_line(fwd, &anchored, 65534, line)) && !lower_search_line(fwd, nullptr, 65534, line)) return;
    uint32_t column[256];
    for (int c = 0; c < 256; c++) column[c] = c == '\n' ? line.ncols - 1 : fwd.cls[c];
    SearchLine2Program s2;
    if (!lower_search_line2(line, column, 16383, s2)) return;
    check_search(s2, fwd, rev, false);
    if ((size_t)s2.nrows * s2.ncols * 4 < ((size_t)1 << 28)) check_search(s2, fwd, rev, true);      // (row offsets of the global form: 28 bits)
}

}  // namespace

int main() {
    std::string p;
    size_t n = 0, rejected = 0;
    std::mt19937 rng(2024);
    while (std::getline(std::cin, p)) {
        n++;
        try {
            rrx::RefAutomaton a = rrx::build_reference_automaton(p.c_str());
            rrx::Trimmed t = rrx::trim(a);
            rrx::Reduced r = rrx::reduce(t);
            rrx::NfaProgram nfa, wave;
            rrx::DfaProgram dfa;
            rrx::Dfa2Program dfa2;
            const bool has_nfa = rrx::lower_nfa(r, 512, nfa, true);
            const bool has_wave = rrx::lower_nfa(r, 4096, wave, false);
            const bool has_dfa = rrx::lower_dfa(r, 16384, dfa);
            const bool has_dfa2 = has_dfa && rrx::lower_dfa2(dfa, 1024, dfa2);
            std::printf("%zu ok useful %u nodes %zu nfa %d/%u wave %d dfa %d/%u dfa2 %d/%u\n", n, t.n, r.nodes.size(), (int)has_nfa,
                        has_nfa ? nfa.nbits : 0u, (int)has_wave, (int)has_dfa, has_dfa ? dfa.nstates : 0u, (int)has_dfa2,
                        has_dfa2 ? dfa2.ncols : 0u);
            check_images(t, r, has_nfa ? &nfa : nullptr, has_wave ? &wave : nullptr, has_dfa ? &dfa : nullptr, has_dfa2 ? &dfa2 : nullptr, rng);
        } catch (const rrx::PatternError &e) {
            rejected++;
            std::printf("%zu rejected %s\n", n, e.what());
        }
    }
    std::printf("packed line %zu stride2 %zu items %zu search %zu lane %zu group %zu wave %zu sparse %zu\n", g_n.line, g_n.stride2, g_n.items,
                g_n.search, g_n.lane, g_n.group, g_n.wave, g_n.sparse);
    std::printf("done %zu rejected %zu\n", n, rejected);
    return 0;
}
