// dfa2_byte_pairs_driver.cpp — the byte-wide pair table of the stride-2 match table (csrc/device.hpp: Dfa2Device::P8), on the host.
// Reads patterns from stdin, one per line; for each one that AUTO gives a stride-2 table, packs the match table's image the way
// the library does (LineTables::decide / LineTables::pack), as numbered and in a seeded random order, binds it to a copy and checks
//   - the form is chosen exactly when (ncols - 1) * 4 << rep_log2 <= 255, rep_log2 read from the packed descriptor;
//   - where it is chosen, P8[c1 * kDfa2P8Stride + c2] == P[c1 * kDfa2PStride + c2] for all 128 x 128 pairs, the eight pad bytes
//     of every row are zero, and P8 lies inside the image at a 16-byte boundary; elsewhere the descriptor holds no P8.
// Then the rule itself on synthetic programs at the bound (64 and 65 columns unreplicated, 32 / 33 and 16 / 17 with copies), and
// pack_dfa2 refusing a byte-wide table that does not fit.  Built by tests/test_dfa2_byte_pairs_lowering.py with
// -fsanitize=address,undefined from the host pipeline's units (csrc/host_sources.mk: HOST_SRCS): no HIP involved.  A mismatch aborts.
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
        if (!(cond)) { std::fprintf(stderr, "byte-pair check failed: %s (line %d)\n", #cond, __LINE__); std::abort(); } \
    } while (0)

// the image of `lt` in the order rows / cols, bound to a copy: true if it holds the byte-wide table (then checked entry by entry)
bool check_image(const LineTables &lt, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t *rep_log2) {
    Image img;
    DeviceTables t;
    lt.pack(rows, cols, img, t);
    std::vector<uint8_t> copy(img.bytes);
    img.bind(copy.data());
    const dev::Dfa2Device &d = t.dfa2;
    *rep_log2 = d.rep_log2;
    const bool fits = ((size_t)(lt.dfa2.ncols - 1) * 4 << d.rep_log2) <= 255;
    CHECK(lt.byte_pairs == fits && (d.P8 != nullptr) == fits);
    CHECK(d.P != nullptr && d.T2 != nullptr);
    if (!d.P8) return false;
    const size_t at = (size_t)(d.P8 - copy.data());
    CHECK(at % 16 == 0 && at + dev::kDfa2P8Bytes <= copy.size());
    CHECK(dev::kDfa2P8Bytes % 16 == 0 && dev::kDfa2P8Stride >= 128);
    const bool ordered = !cols.empty();
    for (uint32_t c1 = 0; c1 < 128; c1++)
        for (uint32_t c2 = 0; c2 < dev::kDfa2P8Stride; c2++) {
            const uint32_t e8 = d.P8[c1 * dev::kDfa2P8Stride + c2];
            if (c2 >= 128) { CHECK(e8 == 0); continue; }
            const uint32_t col = lt.dfa2.pair_col[c1 * 128 + c2];
            CHECK(e8 == d.P[c1 * dev::kDfa2PStride + c2]);
            CHECK(e8 == ((ordered ? cols[col] : col) * 4u << d.rep_log2));     // ... and both are the column's byte offset
        }
    return true;
}

Dfa2Program synthetic(uint32_t nstates, uint32_t ncols) {
    Dfa2Program p;
    p.nstates = nstates; p.ncols = ncols; p.start = 1;
    p.pair_col.resize(128 * 128);
    for (uint32_t i = 0; i < 128 * 128; i++) p.pair_col[i] = (uint16_t)(i % ncols);
    p.next2.resize((size_t)nstates * ncols);
    for (size_t i = 0; i < p.next2.size(); i++) p.next2[i] = (uint32_t)(i % nstates);
    return p;
}

void check_rule(uint32_t nstates, uint32_t ncols, uint32_t want_rep, bool want_fit) {
    const Dfa2Program p = synthetic(nstates, ncols);
    CHECK(dfa2_fits(p));
    CHECK(dfa2_copies_log2(p) == want_rep && dfa2_byte_pairs_fit(p) == want_fit);
    Image img;
    dev::Dfa2Device d;
    CHECK(pack_dfa2(p, {}, {}, img, d, 0, /*byte_pairs=*/true) == want_fit);     // asked for where it does not fit: refused
    std::vector<uint8_t> copy(img.bytes);
    img.bind(copy.data());
    CHECK(d.rep_log2 == want_rep && (d.P8 != nullptr) == want_fit);
    if (want_fit)
        for (uint32_t i = 0; i < 128 * 128; i++) CHECK(d.P8[(i / 128) * dev::kDfa2P8Stride + i % 128] == ((i % ncols) * 4u << want_rep));
    Image img16;
    dev::Dfa2Device d16;
    CHECK(pack_dfa2(p, {}, {}, img16, d16) && d16.P8 == nullptr);                // not asked for: the u16 table alone
    Dfa2Program items = p;
    items.pair_dim = 129;                                                        // the items form never has one
    CHECK(!dfa2_byte_pairs_fit(items));
}

}  // namespace

int main() {
    std::string p;
    size_t n = 0, stride2 = 0, byte_wide = 0;
    std::mt19937 rng(2025);
    while (std::getline(std::cin, p)) {
        n++;
        try {
            Programs chosen;
            plan_engines(p, RRX_ENGINE_AUTO, chosen);
            const LineTables &lt = chosen.match;
            if (chosen.engine != RRX_ENGINE_DFA || !lt.has_dfa2) { std::printf("%zu no-stride2\n", n); continue; }
            stride2++;
            uint32_t rep = 0, rep_ordered = 0;
            const bool has = check_image(lt, {}, {}, &rep);
            std::vector<uint32_t> rows(lt.dfa2.nstates), cols(lt.dfa2.ncols);
            for (uint32_t i = 0; i < rows.size(); i++) rows[i] = i;
            for (uint32_t i = 0; i < cols.size(); i++) cols[i] = i;
            if (rows.size() > 1) std::shuffle(rows.begin() + 1, rows.end(), rng);
            std::shuffle(cols.begin(), cols.end(), rng);
            CHECK(check_image(lt, rows, cols, &rep_ordered) == has && rep_ordered == rep);
            byte_wide += has ? 1 : 0;
            std::printf("%zu stride2 states %u cols %u rep %u byte_pairs %d\n", n, lt.dfa2.nstates, lt.dfa2.ncols, rep, (int)has);
        } catch (const PatternError &e) {
            std::printf("%zu rejected\n", n);
        }
    }
    // the bound itself.  160 rows of 65 | 1 entries are past half the table budget: one copy; 4 rows are copied 2^5 times unless the
    // column offsets stop it
    check_rule(160, 64, 0, true);     // 63 * 4 = 252
    check_rule(160, 65, 0, false);    // 64 * 4 = 256
    check_rule(100, 32, 1, true);     // 31 * 4 * 2 = 248
    check_rule(100, 33, 1, false);    // 32 * 4 * 2 = 256
    check_rule(4, 2, 5, true);        // 1 * 4 * 32 = 128
    check_rule(4, 3, 5, false);       // 2 * 4 * 32 = 256
    check_rule(4, 1, 5, true);        // a single column: offset 0
    std::printf("done %zu stride2 %zu byte_pairs %zu\n", n, stride2, byte_wide);
    return 0;
}
