// host_pipeline_driver.cpp — runs the host compile pipeline (pattern -> reference-numbered automaton -> trim ->
// reduce -> NFA / DFA / stride-2 programs) over the patterns given on stdin, one per line.  Built by
// tests/test_lowering.py with -fsanitize=address,undefined (sanitizers run on the CPU build only) from
// the host pipeline's units (csrc/host_sources.mk: HOST_SRCS): no HIP involved.  Prints one summary line per pattern.
//
// Every device image whose preconditions the programs meet - by the library's own fit rules (csrc/plan.hpp) - is packed
// (csrc/pack.hpp), copied, bound to the copy and decoded back here - independently of the packer - against the program it was
// packed from; so is the image of the engine and table forms that RRX_ENGINE_AUTO chooses for the pattern ("chosen").  A
// mismatch aborts; the line before "done" counts the images checked per kind.
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
#include "plan.hpp"
#include "../../include/rrx.h"

using namespace rrx;

namespace {

#define CHECK(cond)                                                                                               \
    do {                                                                                                          \
        if (!(cond)) { std::fprintf(stderr, "image check failed: %s (line %d)\n", #cond, __LINE__); std::abort(); } \
    } while (0)

struct Counts { size_t line = 0, stride2 = 0, items = 0, search = 0, lane = 0, group = 0, wave = 0, sparse = 0, chosen = 0; } g_n;

// the image as the device would hold it: a copy of its bytes, the descriptors bound to the copy
struct Copy {
    std::vector<uint8_t> bytes;
    explicit Copy(const Image &img) : bytes(img.bytes) { img.bind(bytes.data()); }
    size_t at(const void *p) const { return (size_t)(static_cast<const uint8_t *>(p) - bytes.data()); }
};

bool bit(const std::vector<uint32_t> &v, uint32_t b) { return (v[b >> 5] >> (b & 31)) & 1u; }

void decode_dfa2(const Dfa2Program &p, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t p_region, const dev::Dfa2Device &d,
                 const Copy &cp);

// The tables of a table engine in the forms `lt` says, the stride-2 table in the order rows / cols.
// lane l reads copy l % R of every entry: all R copies of entry i (at dword i * R + k) must agree, offsets + 4 k
void check_line(const LineTables &lt, const std::vector<uint32_t> &rows = {}, const std::vector<uint32_t> &cols = {}) {
    const DfaProgram &dfa = lt.dfa;
    const bool wide = lt.wide, global = lt.global;
    Image img;
    DeviceTables t;
    lt.pack(rows, cols, img, t);
    Copy cp(img);
    if (lt.has_dfa2) decode_dfa2(lt.dfa2, rows, cols, 0, t.dfa2, cp);
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
void check_line(const DfaProgram &dfa, bool wide, bool global) {
    LineTables lt;
    lt.dfa = dfa; lt.wide = wide; lt.global = global;
    check_line(lt);
}

// a stride-2 table in the order rows / cols (empty: as numbered): every (state, pair) through P and the slots gives next2
void decode_dfa2(const Dfa2Program &p, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t p_region, const dev::Dfa2Device &d,
                 const Copy &cp) {
    const bool ordered = !rows.empty();
    auto rs = [&](uint32_t s) { return ordered ? rows[s] : s; };
    auto cs = [&](uint32_t c) { return ordered ? cols[c] : c; };
    const uint32_t R = 1u << d.rep_log2, dim = p.pair_dim;
    CHECK(d.nrows == p.nstates && d.stride == (p.ncols | 1u) * R && d.start_off == rs(p.start) * d.stride * 4);
    CHECK(cp.at(d.P) % 16 == 0 && cp.at(d.T2) - cp.at(d.P) == (p_region ? p_region : ((dim * dev::kDfa2PStride * 2 + 15) & ~15u)));
    for (uint32_t c1 = 0; c1 < dim; c1++)
        for (uint32_t c2 = 0; c2 < dev::kDfa2PStride; c2++)
            CHECK(d.P[c1 * dev::kDfa2PStride + c2] == (c2 < dim ? cs(p.pair_col[c1 * dim + c2]) * 4 * R : 0u));
    for (size_t b = cp.at(d.P) + dim * dev::kDfa2PStride * 2; b < cp.at(d.T2); b++) CHECK(cp.bytes[b] == 0);     // (the items form's P region)
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
void check_dfa2(const Dfa2Program &p, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t p_region) {
    Image img;
    dev::Dfa2Device d;
    CHECK(pack_dfa2(p, rows, cols, img, d, p_region));
    Copy cp(img);
    CHECK(cp.at(d.P) == 0);
    decode_dfa2(p, rows, cols, p_region, d, cp);
}

// a seeded random order of the table's rows (state 0 keeps slot 0) and columns
void random_order(const Dfa2Program &p, std::mt19937 &rng, std::vector<uint32_t> &rows, std::vector<uint32_t> &cols) {
    rows.resize(p.nstates); cols.resize(p.ncols);
    for (uint32_t i = 0; i < p.nstates; i++) rows[i] = i;
    for (uint32_t i = 0; i < p.ncols; i++) cols[i] = i;
    if (p.nstates > 1) std::shuffle(rows.begin() + 1, rows.end(), rng);
    std::shuffle(cols.begin(), cols.end(), rng);
}

// The items tables of `dfa` as the library forms them (ItemsForms): the stride-2 items table where the DFA has a stride-2 form
// (has_dfa2) and the items form fits, and the byte-stride items table.
void check_items(const DfaProgram &dfa, bool has_dfa2) {
    LineTables lt;
    lt.dfa = dfa; lt.has_dfa2 = has_dfa2;
    ItemsForms forms;
    if (forms.stride2(lt)) {
        Image img2;
        dev::Dfa2Device d2;
        CHECK(forms.pack2(lt, img2, d2));
        Copy cp2(img2);
        CHECK(cp2.at(d2.P) == 0);
        decode_dfa2(forms.dfa2, {}, {}, dev::kDfa2PItemsBytes, d2, cp2);
    }
    Image img;
    dev::LineDfaDevice L;
    if (!forms.pack(lt, img, L)) return;
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

void check_search(const SearchLine2Program &s2, const DfaProgram &fwd, const DfaProgram &rev, const dev::SearchChunkDevice &layout) {
    const bool in_global = layout.in_global != 0;
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

// The LDS the search kernel needs for a layout is the kernel's own arithmetic (kernels_search.hip); here every layout that
// pack_search can lay out passes (row offsets of the global form: 28 bits), so that plan_search hands out the LDS form wherever
// the table admits it and the global form elsewhere.
size_t any_packable_layout(const dev::SearchChunkDevice &c) {
    return c.in_global && (size_t)c.nrows * c.ncols2 * 4 >= ((size_t)1 << 28) ? dev::kSearchChunkLdsBudget + 1 : 0;
}

void check_images(const Trimmed &t, const Reduced &r, const NfaProgram *nfa, const NfaProgram *wave, const DfaProgram *dfa,
                  const Dfa2Program *dfa2, std::mt19937 &rng) {
    if (nfa) check_lane(*nfa);
    if (wave) { check_group(*wave, t); check_wave(*wave, t, false); check_wave(*wave, t, true); }
    if (dfa) {
        if (wide_fits(*dfa)) check_line(*dfa, true, false);
        if (classed_fits(*dfa)) check_line(*dfa, false, false);
        if (global_fits(*dfa)) check_line(*dfa, false, true);
        check_items(*dfa, dfa2 != nullptr);
    }
    if (dfa2 && dfa2_fits(*dfa2)) {
        std::vector<uint32_t> rows, cols;
        check_dfa2(*dfa2, rows, cols, 0);
        random_order(*dfa2, rng, rows, cols);
        check_dfa2(*dfa2, rows, cols, 0);
    }
    // the search tables as the library plans them, with and without the anchored table, in both layouts
    for (const bool anchored : {true, false}) {
        SearchPlan s;
        (void)plan_search(r, anchored, /*accepts_empty=*/false, any_packable_layout, s);
        if (!s.layout.nrows) continue;
        check_search(s.line2, s.fwd, s.rev, s.layout);
        const dev::SearchChunkDevice global = search_chunk_layout(s.line2, s.fwd, s.rev, /*in_global=*/true);
        if (!s.layout.in_global && any_packable_layout(global) <= dev::kSearchChunkLdsBudget) check_search(s.line2, s.fwd, s.rev, global);
    }
}

// what RRX_ENGINE_AUTO runs the pattern on: the image of that engine, for a table engine in exactly the forms it chose
void check_chosen(const Programs &p) {
    if (p.engine == RRX_ENGINE_DFA) check_line(p.match);
    else if (p.engine == RRX_ENGINE_NFA) check_lane(p.nfa);
    else if (p.engine == RRX_ENGINE_NFA_WAVE) check_group(p.nfa_wave, p.trimmed);
    else if (p.engine == RRX_ENGINE_NFA_BLOCK) check_wave(p.nfa_block, p.trimmed, false);
    else return;
    g_n.chosen++;
}

}  // namespace

int main() {
    std::string p;
    size_t n = 0, rejected = 0;
    std::mt19937 rng(2024);
    while (std::getline(std::cin, p)) {
        n++;
        try {
            rrx::Programs chosen;
            rrx::plan_engines(p, RRX_ENGINE_AUTO, chosen);
            const rrx::Trimmed &t = chosen.trimmed;
            rrx::Reduced r = rrx::reduce(t);
            rrx::NfaProgram nfa, wave;
            rrx::DfaProgram dfa;
            rrx::Dfa2Program dfa2;
            const bool has_nfa = rrx::lower_nfa(r, 512, nfa, true);
            const bool has_wave = rrx::lower_nfa(r, 4096, wave, false);
            const bool has_dfa = rrx::lower_dfa(r, 16384, dfa);
            const bool has_dfa2 = has_dfa && rrx::lower_dfa2(dfa, 1024, dfa2);
            std::printf("%zu ok useful %u nodes %zu nfa %d/%u wave %d dfa %d/%u dfa2 %d/%u engine %s\n", n, t.n, r.nodes.size(), (int)has_nfa,
                        has_nfa ? nfa.nbits : 0u, (int)has_wave, (int)has_dfa, has_dfa ? dfa.nstates : 0u, (int)has_dfa2,
                        has_dfa2 ? dfa2.ncols : 0u, chosen.engine ? chosen.engine_name() : "none");
            check_images(t, r, has_nfa ? &nfa : nullptr, has_wave ? &wave : nullptr, has_dfa ? &dfa : nullptr, has_dfa2 ? &dfa2 : nullptr, rng);
            check_chosen(chosen);
        } catch (const rrx::PatternError &e) {
            rejected++;
            std::printf("%zu rejected %s\n", n, e.what());
        }
    }
    std::printf("packed line %zu stride2 %zu items %zu search %zu lane %zu group %zu wave %zu sparse %zu chosen %zu\n", g_n.line, g_n.stride2, g_n.items,
                g_n.search, g_n.lane, g_n.group, g_n.wave, g_n.sparse, g_n.chosen);
    std::printf("done %zu rejected %zu\n", n, rejected);
    return 0;
}
