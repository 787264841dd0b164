// pack.cpp — lowered programs -> device images (pack.hpp).  Plain C++: no HIP header, no device call.
#include "pack.hpp"

#include <cstring>

namespace rrx {

size_t Image::put(const void *p, size_t n) {
    const size_t off = (bytes.size() + 15) & ~(size_t)15;
    bytes.resize(off + n);
    if (n) std::memcpy(bytes.data() + off, p, n);
    return off;
}

static int instantiated_width(uint32_t W) { return W <= 4 ? (int)W : W <= 6 ? 6 : W <= 8 ? 8 : W <= 12 ? 12 : 16; }

void pack_dfa_tables(const DfaProgram &dfa, bool wide, bool global, const Dfa2Program *dfa2, const std::vector<uint32_t> &rows,
                     const std::vector<uint32_t> &cols, Image &img, DeviceTables &t, bool byte_pairs) {
    img.put(t.dfa.cls, dfa.cls, 256);
    img.put(t.dfa.next, dfa.next.data(), dfa.next.size() * 2);
    img.put(t.dfa.acc, dfa.accepting.data(), dfa.accepting.size());
    t.dfa.nstates = dfa.nstates; t.dfa.ncls = dfa.ncls; t.dfa.start = dfa.start;
    // line-mode table: entry = next row byte offset (16 bits) | nl << 16 | accept << 24; the '\n' column of
    // every row goes to the start row and carries the verdict of the line that just ended.
    const uint32_t D = dfa.nstates, K = dfa.ncls;
    uint32_t stride = wide ? dev::kWideColumns : (K + 1);
    if (!wide && !(stride & 1)) stride++;                       // odd row stride spreads rows over LDS banks
    // Wide form: R = 2^rep interleaved copies (copy k of logical dword i at dword i*R + k), lane l reads copy
    // l % R: its reads only touch LDS banks = l (mod R), so a half-wave splits into R groups that cannot
    // conflict with each other.  Row byte offsets must stay 16-bit: D * stride * 4 * R <= 65536.
    uint32_t rep = 0;
    if (wide && !global) while (rep < 5 && (size_t)D * stride * 4 * (2u << rep) <= 65536) rep++;
    const uint32_t R = 1u << rep;
    std::vector<uint32_t> T((size_t)D * stride, 0);
    uint8_t lcls[256];
    for (int c = 0; c < 256; c++) lcls[c] = dfa.cls[c];
    lcls['\n'] = (uint8_t)K;                                     // own column for the line terminator
    const uint32_t row_bytes = global ? stride : stride * 4;     // global form: entry indices, not byte offsets
    const int nl_bit = global ? 30 : 16, acc_bit = global ? 31 : 24;
    for (uint32_t d = 0; d < D; d++) {
        uint32_t *row = &T[(size_t)d * stride];
        const uint32_t nl_entry = dfa.start * row_bytes | 1u << nl_bit | (dfa.accepting[d] ? 1u << acc_bit : 0u);
        if (wide) {
            for (uint32_t c = 0; c < 128; c++) row[c] = (uint32_t)dfa.next[(size_t)d * K + dfa.cls[c]] * row_bytes;
            row['\n'] = nl_entry;
            row[128] = (uint32_t)dfa.next[(size_t)d * K + dfa.cls[128]] * row_bytes;    // any byte >= 0x80: class 0 - the dead row 0 on
                                                                                         //   a match table, a live row on a contains table
        } else {
            for (uint32_t k = 0; k < K; k++) row[k] = (uint32_t)dfa.next[(size_t)d * K + k] * row_bytes;
            row[K] = nl_entry;
        }
    }
    if (R > 1) {                                                 // interleave the copies; offsets scale by R
        std::vector<uint32_t> TR(T.size() * R);
        for (size_t i = 0; i < T.size(); i++)
            for (uint32_t k = 0; k < R; k++) TR[i * R + k] = (T[i] & 0xffffu) * R + 4 * k + (T[i] & 0xffff0000u);
        T.swap(TR);
    }
    img.put(t.line.table, T.data(), T.size() * 4);
    img.put(t.line.cls, lcls, 256);
    if (dfa2) (void)pack_dfa2(*dfa2, rows, cols, img, t.dfa2, 0, byte_pairs);
    t.line.nrows = D; t.line.stride = stride * R; t.line.start_off = dfa.start * row_bytes * R;
    t.line.wide = wide ? 1 : 0; t.line.rep_log2 = rep; t.line.in_global = global ? 1 : 0;
}

uint32_t dfa2_copies_log2(const Dfa2Program &dfa2) {
    const uint32_t D2 = dfa2.nstates, C2 = dfa2.ncols, s2 = C2 | 1u;
    uint32_t rep2 = 0;
    while (rep2 < 5 && (size_t)D2 * s2 * 4 * (2u << rep2) <= dev::kDfa2TableBudget && (size_t)C2 * 4 * (2u << rep2) <= 65535) rep2++;
    return rep2;
}
bool dfa2_byte_pairs_fit(const Dfa2Program &dfa2) {
    return dfa2.pair_dim == 128 && dfa2.ncols && ((size_t)(dfa2.ncols - 1) * 4 << dfa2_copies_log2(dfa2)) <= 255;
}

bool pack_dfa2(const Dfa2Program &dfa2, const std::vector<uint32_t> &rs, const std::vector<uint32_t> &cs, Image &img, dev::Dfa2Device &d,
               uint32_t p_region, bool byte_pairs) {
    const uint32_t D2 = dfa2.nstates, C2 = dfa2.ncols, s2 = C2 | 1u;
    const uint32_t rep2 = dfa2_copies_log2(dfa2);
    const uint32_t R2 = 1u << rep2;
    std::vector<uint32_t> T2((size_t)D2 * s2 * R2, 0);
    const bool ordered = rs.size() == D2 && cs.size() == C2 && rs[0] == 0;
    auto row_slot = [&](uint32_t st) { return ordered ? rs[st] : st; };
    auto col_slot = [&](uint32_t col) { return ordered ? cs[col] : col; };
    for (uint32_t st = 0; st < D2; st++)
        for (uint32_t col = 0; col < C2; col++) {
            const uint32_t v = dfa2.next2[(size_t)st * C2 + col];
            const uint32_t row_off = row_slot(v & 0xffffu) * s2 * 4 * R2;
            for (uint32_t k = 0; k < R2; k++) T2[((size_t)row_slot(st) * s2 + col_slot(col)) * R2 + k] = (row_off + 4 * k) | (v & 0xffff0000u);
        }
    const unsigned dim = dfa2.pair_dim;                 // 128; items form: 129 (code 128 = END OF ITEM: a row more, and the pad column 128)
    std::vector<uint16_t> P(dim * dev::kDfa2PStride, 0);
    for (unsigned c1 = 0; c1 < dim; c1++)
        for (unsigned c2 = 0; c2 < dim; c2++) P[c1 * dev::kDfa2PStride + c2] = (uint16_t)(col_slot(dfa2.pair_col[c1 * dim + c2]) * 4 * R2);
    d.nrows = D2; d.stride = s2 * R2; d.start_off = row_slot(dfa2.start) * s2 * 4 * R2; d.rep_log2 = rep2;
    if (p_region && P.size() * 2 > p_region) return false;
    img.put(d.P, P.data(), P.size() * 2);
    if (p_region) img.bytes.resize(img.bytes.size() - P.size() * 2 + p_region);
    img.put(d.T2, T2.data(), T2.size() * 4);
    if (byte_pairs) {                                   // the same entries a byte each (the caller has asked dfa2_byte_pairs_fit)
        if (!dfa2_byte_pairs_fit(dfa2)) return false;
        std::vector<uint8_t> P8(dev::kDfa2P8Bytes, 0);
        for (unsigned c1 = 0; c1 < 128; c1++)
            for (unsigned c2 = 0; c2 < 128; c2++) P8[c1 * dev::kDfa2P8Stride + c2] = (uint8_t)P[c1 * dev::kDfa2PStride + c2];
        img.put(d.P8, P8.data(), P8.size());
    }
    return true;
}

bool pack_items(const DfaProgram &dfa, Image &img, dev::LineDfaDevice &d) {
    // rows of kItemColumns entries (odd: a column's entries of different rows spread over all LDS banks), R interleaved
    // copies like the wide line table (lane l reads copy l % R: only banks congruent to l mod R)
    const uint32_t D = dfa.nstates, stride = dev::kItemColumns;
    uint32_t rep = 0;
    while (rep < 3 && (size_t)D * stride * 4 * (2u << rep) <= 60 * 1024) rep++;
    const uint32_t R = 1u << rep, row_bytes = stride * 4 * R;
    if (!D || (size_t)D * row_bytes > 65535) return false;
    std::vector<uint32_t> T((size_t)D * stride * R, 0);
    for (uint32_t q = 0; q < D; q++)
        for (uint32_t c = 0; c < stride; c++) {
            uint32_t v;
            if (c <= 128) {                                                      // byte 2, bit 7: the row it leads to is accepting (what a trim-0
                const uint32_t nx = dfa.next[(size_t)q * dfa.ncls + dfa.cls[c]];  // item that ends on this byte reports; as a shift count it is 0)
                v = nx * row_bytes | (dfa.accepting[nx] ? 0x80u << 16 : 0u);
            }
            else if (c == dev::kItemEndColumn) v = dfa.start * row_bytes | 1u << 16 | (dfa.accepting[q] ? 1u << 24 : 0u);
            else v = 0;                                                          // padding column: never read
            for (uint32_t k = 0; k < R; k++) T[((size_t)q * stride + c) * R + k] = (v & 0xffff0000u) | ((v & 0xffffu) + 4 * k);
        }
    img.put(d.table, T.data(), T.size() * 4);
    d.nrows = D; d.stride = stride * R; d.start_off = dfa.start * row_bytes; d.wide = 1; d.rep_log2 = rep; d.in_global = 0;
    return true;
}

// A DFA in the plain form of the lane-per-item kernels: cls / next / acc
static void put_plain(const DfaProgram &p, Image &img, dev::DfaDevice &t) {
    img.put(t.cls, p.cls, 256);
    img.put(t.next, p.next.data(), p.next.size() * 2);
    img.put(t.acc, p.accepting.data(), p.accepting.size());
    t.nstates = p.nstates; t.ncls = p.ncls; t.start = p.start;
}
// Row 0 is the dead row: rejecting, every class back to itself (the kernels stop a lane there)
static bool row0_dead(const DfaProgram &p) {
    if (p.accepting[0]) return false;
    for (uint32_t k = 0; k < p.ncls; k++)
        if (p.next[k] != 0) return false;
    return true;
}

bool pack_search_items(const DfaProgram &fwd, const DfaProgram &rev, Image &img, dev::SearchItemsDevice &d) {
    if (!fwd.nstates || !rev.nstates || !row0_dead(rev)) return false;
    put_plain(fwd, img, d.fwd);
    put_plain(rev, img, d.rev);
    return true;
}

bool pack_search_longest(const DfaProgram &starts, const DfaProgram &anchored, Image &img, dev::SearchLongestDevice &d) {
    if (!starts.nstates || !anchored.nstates || !row0_dead(anchored)) return false;
    put_plain(starts, img, d.starts);
    put_plain(anchored, img, d.anchored);
    return true;
}

bool pack_group(const DfaProgram &a, const DfaProgram &rev_bc, const DfaProgram &b, const DfaProgram &rev_c, Image &img, dev::GroupDevice &d) {
    if (!b.nstates) return false;
    const DfaProgram *const progs[] = {&a, &rev_bc, &b, &rev_c};
    dev::DfaDevice *const tables[] = {&d.a, &d.rev_bc, &d.b, &d.rev_c};
    for (int k = 0; k < 4; k++) {
        if (!progs[k]->nstates) continue;                        // an absent part: no table
        if (!row0_dead(*progs[k])) return false;                 // both passes of the split kernel stop a lane in row 0
        put_plain(*progs[k], img, *tables[k]);
    }
    return true;
}

void pack_multi(const MultiProgram &p, Image &img, dev::MultiDevice &d) {
    img.put(d.cls, p.cls, 256);
    img.put(d.next, p.next.data(), p.next.size() * 2);
    img.put(d.mask, p.mask.data(), p.mask.size() * 4);
    d.nstates = p.nstates; d.ncls = p.ncls; d.start = p.start; d.first_hit = p.first_hit; d.full = p.full;
}

void pack_lane_nfa(const NfaProgram &nfa, Image &img, dev::NfaDevice &d) {
    const uint32_t W = nfa.W, WP = (uint32_t)instantiated_width(W);
    std::vector<uint32_t> B((size_t)256 * WP, 0), X((size_t)nfa.nbits * WP, 0);
    for (uint32_t c = 0; c < 256; c++) for (uint32_t w = 0; w < W; w++) B[(size_t)c * WP + w] = nfa.B[(size_t)c * W + w];
    for (uint32_t b = 0; b < nfa.nbits; b++) for (uint32_t w = 0; w < W; w++) X[(size_t)b * WP + w] = nfa.X[(size_t)b * W + w];
    img.put(d.B, B.data(), B.size() * 4);
    img.put(d.X, X.data(), X.size() * 4);
    d.W = WP; d.nbits = nfa.nbits; d.any_exc = nfa.n_exc ? 1 : 0; d.any_carry = nfa.n_carry ? 1 : 0;
    for (uint32_t w = 0; w < W; w++) if (nfa.self[w]) d.any_self = 1;
    std::memset(&d.masks, 0, sizeof d.masks);
    for (uint32_t w = 0; w < W; w++) {
        d.masks.init[w] = nfa.init[w]; d.masks.fin[w] = nfa.fin[w]; d.masks.chain[w] = nfa.chain[w];
        d.masks.self[w] = nfa.self[w]; d.masks.excm[w] = nfa.excm[w];
        d.masks.cgrp[w] = nfa.cgrp[w]; d.masks.ctgt[w] = nfa.ctgt[w];
    }
}

void contains_b_rows(NfaProgram &nfa) {
    const uint32_t W = nfa.W;
    for (uint32_t c = 0; c < 256; c++) {
        uint32_t *row = &nfa.B[(size_t)c * W];
        if (c == 0 || c >= 0x80) for (uint32_t w = 0; w < W; w++) row[w] = 0;
        row[0] |= 1u;
    }
}

bool pack_group_nfa(const NfaProgram &nfa, const Trimmed &trimmed, Image &img, dev::GroupNfaDevice &d) {
    // group-cooperative form: G lanes x K words (device.hpp: group_geometry), a B row per byte CLASS
    const uint32_t W = nfa.W, N = nfa.nbits;
    uint32_t G = 0, K = 0;
    if (!dev::group_geometry(N, &G, &K)) return false;
    const uint32_t WP = G * K, NC = trimmed.ncls;
    std::vector<uint32_t> M((size_t)3 * WP, 0), B((size_t)NC * WP, 0);
    const std::vector<uint32_t> *src[3] = {&nfa.fin, &nfa.self, &nfa.excm};
    for (int k = 0; k < 3; k++) for (uint32_t w = 0; w < W; w++) M[(size_t)k * WP + w] = (*src[k])[w];
    for (uint32_t cl = 1; cl < NC; cl++) {                        // class 0 (0x00, >= 0x80, bytes nothing moves on): empty row
        const uint32_t c = trimmed.cls_rep[cl];
        for (uint32_t w = 0; w < W; w++) B[(size_t)cl * WP + w] = nfa.B[(size_t)c * W + w];
    }
    uint8_t cmap[256];
    for (int c = 0; c < 256; c++) cmap[c] = (c == 0 || c >= 128) ? 0 : trimmed.cls[c];
    // slots (word index within a lane) that carry masks at all: a slot whose B rows are all ones on every POSITION IN USE for
    // every class >= 1 needs no AND (positions beyond nbits are never set: their row bits do not matter)
    uint32_t self_slots = 0, b_slots = 0, exc_slots = 0;
    for (uint32_t w = 0; w < WP; w++) {
        const uint32_t used = w * 32 >= N ? 0u : (N - w * 32 >= 32 ? 0xffffffffu : (1u << (N - w * 32)) - 1u);
        if (w < W && nfa.self[w]) self_slots |= 1u << (w % K);
        if (w < W && nfa.excm[w]) exc_slots |= 1u << (w % K);
        for (uint32_t cl = 1; cl < NC; cl++)
            if ((B[(size_t)cl * WP + w] & used) != used) b_slots |= 1u << (w % K);
    }
    std::vector<uint16_t> xidx(N, 0xffff);
    std::vector<uint32_t> X;
    uint32_t rows = 0;
    for (uint32_t b = 0; b < N; b++) {
        if (!((nfa.excm[b >> 5] >> (b & 31)) & 1u)) continue;
        xidx[b] = (uint16_t)rows++;
        X.resize((size_t)rows * WP, 0);
        for (uint32_t i = nfa.xoff[b]; i < nfa.xoff[b + 1]; i++) {      // (the CSR lists exist at every size, dense rows only up to 4096 positions)
            const uint32_t tv = nfa.xtgt[i];
            X[(size_t)(rows - 1) * WP + (tv >> 5)] |= 1u << (tv & 31);
        }
    }
    if (X.empty()) X.assign(WP, 0);
    img.put(d.masks, M.data(), M.size() * 4);
    img.put(d.Bcls, B.data(), B.size() * 4);
    img.put(d.X, X.data(), X.size() * 4);
    img.put(d.xidx, xidx.data(), xidx.size() * 2);
    img.put(d.cls, cmap, 256);
    d.G = G; d.K = K; d.nbits = N; d.n_exc = rows; d.ncls = NC; d.exc_mode = (rows == 1 && xidx[0] == 0) ? 2 : 0;
    d.self_slots = self_slots; d.b_slots = b_slots; d.exc_slots = exc_slots;
    return true;
}

void pack_wave_nfa(const NfaProgram &nfa, const Trimmed &trimmed, uint32_t WL, bool sparse, Image &img, dev::WaveNfaDevice &d) {
    // wave-resident form: 64 lanes x WL words, a B row per byte value (+ the line-mode '\n' row), exception edges as CSR
    // (word w of the set sits at flat index w - dense form: lane w / WL, index w % WL; sparse form: row w / 64, lane w % 64)
    const uint32_t W = nfa.W, N = nfa.nbits, WP = 64 * WL;
    std::vector<uint32_t> M((size_t)3 * WP, 0), B((size_t)257 * WP, 0);
    const std::vector<uint32_t> *src[3] = {&nfa.fin, &nfa.self, &nfa.excm};
    for (int k = 0; k < 3; k++) for (uint32_t w = 0; w < W; w++) M[(size_t)k * WP + w] = (*src[k])[w];
    for (uint32_t c = 1; c < 128; c++)                            // 0x00 and >= 0x80: empty rows
        for (uint32_t w = 0; w < W; w++) B[(size_t)c * WP + w] = nfa.B[(size_t)c * W + w];
    B[(size_t)256 * WP] = 1u;                                     // '\n' in line mode: {position 0}
    std::vector<uint32_t> xt = nfa.xtgt;
    if (xt.empty()) xt.push_back(0);
    img.put(d.masks, M.data(), M.size() * 4);
    img.put(d.Bbyte, B.data(), B.size() * 4);
    img.put(d.xoff, nfa.xoff.data(), nfa.xoff.size() * 4);
    img.put(d.xtgt, xt.data(), xt.size() * 4);
    d.WL = WL; d.nbits = N;
    if (sparse) {                                                 // rows per byte class too (LDS-resident when they fit)
        const uint32_t K = trimmed.ncls;
        std::vector<uint32_t> BC((size_t)K * WP, 0);
        for (uint32_t k = 1; k < K; k++)
            for (uint32_t w = 0; w < W; w++) BC[(size_t)k * WP + w] = nfa.B[(size_t)trimmed.cls_rep[k] * W + w];
        img.put(d.Bcls, BC.data(), BC.size() * 4);
        img.put(d.cls, trimmed.cls, 256);
        d.ncls = K;
    }
    for (uint32_t w = 0; w < W; w++) {
        if (nfa.self[w]) d.self_words |= 1u << (w % WL);
        if (nfa.excm[w]) d.exc_words |= 1u << (w % WL);
    }
}

dev::SearchChunkDevice search_chunk_layout(const SearchLine2Program &s2, const DfaProgram &fwd, const DfaProgram &rev, bool in_global) {
    dev::SearchChunkDevice c;
    c.nrows = s2.nrows; c.ncols2 = s2.ncols; c.start_row = s2.start; c.skip_row = s2.skip;
    c.nr = rev.nstates; c.ncls = fwd.ncls; c.start_r = rev.start;
    if (in_global) { c.in_global = 1; return c; }
    uint32_t rb = (2 * s2.ncols + 3) & ~3u;
    if (((rb >> 2) & 1u) == 0) rb += 4;                           // an odd number of dwords per row: rows spread over the LDS banks
    c.row_bytes = rb; c.base_row = (dev::kSearchP8Bytes + rb - 1) / rb;
    return c;
}

void pack_search(const SearchLine2Program &s2, const DfaProgram &fwd, const DfaProgram &rev, const dev::SearchChunkDevice &layout, Image &img,
                 dev::SearchChunkDevice &d) {
    d = layout;
    img.put(d.cls, fwd.cls, 256);
    // The line-mode product table in its stride-2 form (lower_search_line2), laid out for LDS (16-bit entries, a byte-wide
    // pair table) or for HBM/L2 (32-bit entries, a 16-bit pair table in LDS): device.hpp, SearchChunkDevice.
    const uint32_t K = fwd.ncls, NR = rev.nstates;
    if (!d.in_global) {
        const uint32_t rb = d.row_bytes, br = d.base_row;
        std::vector<uint8_t> p8(dev::kSearchP8Bytes, 0);
        for (unsigned c1 = 0; c1 < 128; c1++)
            for (unsigned c2 = 0; c2 < 128; c2++) p8[c1 * dev::kSearchP8Stride + c2] = (uint8_t)(2 * s2.pair_col[c1 * 128 + c2]);
        auto lay = [&](const std::vector<uint32_t> &src) {
            std::vector<uint16_t> T((size_t)s2.nrows * (rb / 2), 0);
            for (uint32_t r = 0; r < s2.nrows; r++)
                for (uint32_t c = 0; c < s2.ncols; c++) {
                    const uint32_t v = src[(size_t)r * s2.ncols + c];
                    T[(size_t)r * (rb / 2) + c] = (uint16_t)((br + (v & 0xffffffu)) << 4 | (v >> 24));
                }
            return T;
        };
        const std::vector<uint16_t> T = lay(s2.first), TA = lay(s2.all);
        img.put(d.P8, p8.data(), p8.size());
        img.put(d.T2, T.data(), T.size() * 2);
        img.put(d.T2_all, TA.data(), TA.size() * 2);
    } else {
        std::vector<uint16_t> p16((size_t)128 * dev::kSearchP16Stride, 0);
        for (unsigned c1 = 0; c1 < 128; c1++)
            for (unsigned c2 = 0; c2 < 128; c2++) p16[c1 * dev::kSearchP16Stride + c2] = (uint16_t)(4 * s2.pair_col[c1 * 128 + c2]);
        auto lay = [&](const std::vector<uint32_t> &src) {
            std::vector<uint32_t> T(src.size());
            for (size_t i = 0; i < src.size(); i++) T[i] = (src[i] & 0xffffffu) * s2.ncols * 4u | (src[i] >> 24) << 28;
            return T;
        };
        const std::vector<uint32_t> T = lay(s2.first), TA = lay(s2.all);
        img.put(d.P16, p16.data(), p16.size() * 2);
        img.put(d.G2, T.data(), T.size() * 4);
        img.put(d.G2_all, TA.data(), TA.size() * 4);
    }
    std::vector<uint16_t> rv(((size_t)NR * K + 1) & ~(size_t)1, 0);
    for (size_t i = 0; i < (size_t)NR * K; i++) { const uint16_t nx = rev.next[i]; rv[i] = (uint16_t)(nx | (rev.accepting[nx] ? 0x8000u : 0u)); }
    img.put(d.rev, rv.data(), rv.size() * 2);
}

}  // namespace rrx
