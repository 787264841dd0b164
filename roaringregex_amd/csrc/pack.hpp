// pack.hpp — lowered programs -> the exact bytes the kernels read (host only: no HIP).  Each packer appends to an Image (the
// bytes of one device allocation) and fills the descriptor(s) of the kernels that read it; their pointer fields are set by
// Image::bind, to the device allocation the image is uploaded to or to a host copy of it (a check on the CPU).  The layouts
// decide the LDS bank pattern of every kernel, so they change here or nowhere.
#pragma once
#include <functional>
#include <vector>

#include "device.hpp"
#include "lower.hpp"

namespace rrx {

struct Image {
    std::vector<uint8_t> bytes;
    size_t put(const void *p, size_t n);                 // appends at the next 16-byte boundary; returns that offset
    template <class T> void put(const T *&field, const void *p, size_t n) {      // ... and `field` will point there
        const size_t off = put(p, n);
        binds.push_back([f = &field, off](const uint8_t *base) { *f = reinterpret_cast<const T *>(base + off); });
    }
    // every field given to put() points into a copy of `bytes` at `base` (the descriptors must not have moved since)
    void bind(const void *base) const { for (auto &b : binds) b(static_cast<const uint8_t *>(base)); }
private:
    std::vector<std::function<void(const uint8_t *)>> binds;
};

// The descriptors of a regex's program tables (those of its engine are filled in).
struct DeviceTables {
    dev::NfaDevice nfa;
    dev::DfaDevice dfa;          // plain form (extents kernel)
    dev::LineDfaDevice line;     // line-mode form (batch kernel)
    dev::GroupNfaDevice group;   // group-cooperative NFA (16/32 lanes per string)
    dev::Dfa2Device dfa2;        // stride-2 line-mode table (corpora without bytes >= 0x80)
    dev::WaveNfaDevice block;    // wave-resident NFA (up to 65536 positions)
};

// Table engine: the plain DFA arrays (cls / next / acc), the line-mode table (wide with R interleaved copies, classed, or the
// global form) and, with `dfa2`, the stride-2 table in the order rows / cols (empty: as numbered).
void pack_dfa_tables(const DfaProgram &dfa, bool wide, bool global, const Dfa2Program *dfa2, const std::vector<uint32_t> &rows,
                     const std::vector<uint32_t> &cols, Image &img, DeviceTables &t, bool byte_pairs = false);
// A stride-2 table: P (pair -> byte offset of its column), then T2 rows of `ncols | 1` entries, R interleaved copies, entry = LDS
// byte offset of the next row | lines << 16 | verdicts << 24.  p_region: P's bytes, zero-filled (false if P does not fit them).
// byte_pairs (only where dfa2_byte_pairs_fit): behind T2 the byte-wide pair table P8 with the same entries (device.hpp).
bool pack_dfa2(const Dfa2Program &dfa2, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, Image &img, dev::Dfa2Device &d,
               uint32_t p_region = 0, bool byte_pairs = false);
uint32_t dfa2_copies_log2(const Dfa2Program &dfa2);      // log2 of the interleaved copies pack_dfa2 makes of T2
// Every entry of the pair table fits a byte: (ncols - 1) * 4 << dfa2_copies_log2 <= 255, on the line form (128 codes) only.
bool dfa2_byte_pairs_fit(const Dfa2Program &dfa2);
// The items table: the plain table, wide, kItemColumns columns (129 = END OF ITEM); false where row offsets pass 16 bits.
bool pack_items(const DfaProgram &dfa, Image &img, dev::LineDfaDevice &d);
void pack_lane_nfa(const NfaProgram &nfa, Image &img, dev::NfaDevice &d);
// The B rows of "contains a match" on a lane program (init = {position 0}, which no row of the lowering holds): position 0 goes
// into every row - it stays live on every byte, a match may start anywhere - and the rows of 0x00 and 0x80 ... 0xFF become exactly
// {position 0}: ordinary text that no pattern takes.  The '\n' row is the pattern's own plus position 0 (the items form steps it;
// the corpus kernel overwrites it in LDS).  Everything else of the program stays: the step is linear in the set.
void contains_b_rows(NfaProgram &nfa);
bool pack_group_nfa(const NfaProgram &nfa, const Trimmed &trimmed, Image &img, dev::GroupNfaDevice &d);     // false: no group_geometry
// WL: wave_words_per_lane, or for the sparse form (rows per byte class too) sparse_rows
void pack_wave_nfa(const NfaProgram &nfa, const Trimmed &trimmed, uint32_t WL, bool sparse, Image &img, dev::WaveNfaDevice &d);

// The stripe-wise search kernel's layout of `s2` in LDS or in HBM/L2 (device.hpp: SearchChunkDevice), without the pointers;
// pack_search lays the tables out for it: cls, the pair table, T2 / T2_all (or G2 / G2_all) and the reverse table.
dev::SearchChunkDevice search_chunk_layout(const SearchLine2Program &s2, const DfaProgram &fwd, const DfaProgram &rev, bool in_global);
void pack_search(const SearchLine2Program &s2, const DfaProgram &fwd, const DfaProgram &rev, const dev::SearchChunkDevice &layout, Image &img,
                 dev::SearchChunkDevice &d);
// The lane-per-item search kernel's tables: fwd and rev in the plain form (cls / next / acc each), one image.  false where the
// reverse table's row 0 is not its dead row - rejecting, every class back to itself (lower_dfa's numbering; the kernel stops a
// lane there) - or a table is empty.
bool pack_search_items(const DfaProgram &fwd, const DfaProgram &rev, Image &img, dev::SearchItemsDevice &d);
// The leftmost-longest kernel's tables: starts and anchored in the plain form, one image.  false where the anchored table's row 0
// is not its dead row - rejecting, every class back to itself (the kernel stops a lane there) - or a table is empty.
bool pack_search_longest(const DfaProgram &starts, const DfaProgram &anchored, Image &img, dev::SearchLongestDevice &d);
// The four tables of a pattern split at a capture group (device.hpp: GroupDevice) in the plain form, one image; a table without
// states is an absent part and stays empty.  false where some table's row 0 is not its dead row, or B has no table.
bool pack_group(const DfaProgram &a, const DfaProgram &rev_bc, const DfaProgram &b, const DfaProgram &rev_c, Image &img, dev::GroupDevice &d);
// The product table of one group of a pattern set (device.hpp: MultiDevice): cls, next and the masks, with first_hit and full.
void pack_multi(const MultiProgram &p, Image &img, dev::MultiDevice &d);

}  // namespace rrx
