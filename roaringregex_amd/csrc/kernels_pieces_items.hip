// kernels_pieces_items.hip — regexp_extract_all and split on explicit items, WRITTEN on the device as a list<binary> column
// (rrx_pieces_sizes / _fill, rrx_extract_all_longest_*, rrx_split_longest_*): from a column (bytes, offsets, trim) and a match list
// per item (the CSR arrays every rrx_search_all* entry returns) to the pieces of every item - its matches (RRX_PIECES_MATCHES) or
// what lies between them (RRX_PIECES_GAPS) - as list offsets, piece offsets and the pieces' bytes.  No table, no regex.
// Two kernels: SIZES (a lane per item) names every piece by (absolute source offset, length); FILL copies the bytes and divides its
// work by OUTPUT bytes alone - not by item and not by piece: what a wave does does not depend on how long an item or a match is.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// SIZES.  One lane per item (item_lanes.hpp: the loop, the item's span), walking its matches in order with the CLAMPING RULE: t the
// item without its separator, L its length, a_0 = 0 and for match k: s' = clamp(s_k, a_k, L), e' = clamp(e_k, s', L), the match
// piece [s', e'), the gap piece [a_k, s'), a_{k+1} = e'; the last gap [a_m, L).  For the list of a search this is the identity; for
// any other list every piece still lies inside the item and the pieces are in order.  Item i with m matches owns the piece slots
// P .. P + m (MATCHES: m of them, P = first[i] - first[0]; GAPS: m + 1, P = first[i] - first[0] + i): list_off[i] = P, the lane of
// the last item also stores list_off[nitems]; piece_len[slot] = the piece's length saturated at ~0u, piece_src[slot] = off[i] + the
// piece's start: an absolute offset into the byte buffer.  Exactly the slots 0 .. npieces - 1 and the nitems + 1 list words are
// written, with plain stores.  too_long (may be null): set to 1 by every lane that meets a piece of 2^30 bytes or more - the same
// value from every lane, a plain store (the one-call forms zero the word and read it back: scan_counts carries 30 bits).
__global__ __launch_bounds__(kThreads) void pieces_sizes_kernel(const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                const uint64_t *__restrict__ first, const uint32_t *__restrict__ match_start,
                                                                const uint32_t *__restrict__ match_end, uint32_t gaps, uint64_t *__restrict__ list_off,
                                                                uint32_t *__restrict__ piece_len, uint64_t *__restrict__ piece_src,
                                                                uint32_t *__restrict__ too_long) {
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        const ItemSpan sp = item_span(off, i, trim);
        const uint64_t b = sp.b, L = sp.e - sp.b, base = first[0], f0 = first[i], f1 = first[i + 1];
        uint64_t slot_out = f0 - base + (gaps ? i : 0);
        list_off[i] = slot_out;
        if (i + 1 == nitems) list_off[nitems] = f1 - base + (gaps ? nitems : 0);
        auto piece = [&](uint64_t from, uint64_t to) {
            const uint64_t n = to - from;
            piece_src[slot_out] = b + from;
            piece_len[slot_out] = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;
            if (too_long && n >= ((uint64_t)1 << 30)) *too_long = 1;
            slot_out++;
        };
        uint64_t a = 0;
        for (uint64_t slot = f0; slot < f1; slot++) {
            uint64_t s = match_start[slot], en = match_end[slot];
            s = s < a ? a : s > L ? L : s;
            en = en < s ? s : en > L ? L : en;
            if (gaps) piece(a, s);
            else piece(s, en);
            a = en;
        }
        if (gaps) piece(a, L);
    });
}

// FILL.  out[piece_off[p] + r] = bytes[piece_src[p] + r] for r < piece_off[p + 1] - piece_off[p], for the npieces pieces.  The work
// is the output range [lo, hi) = [piece_off[0], piece_off[npieces]), which only the device knows: the grid is a fixed one and every
// wave takes CHUNKS of kPiecesChunk bytes of it, grid-stride - chunk c to wave c mod (waves of the grid).  Chunks are cut at
// dword-aligned ADDRESSES: the sweep starts at the dword that holds out + lo, `mis` bytes in front of it, chunk c is the bytes
// [c * kPiecesChunk, (c + 1) * kPiecesChunk) from there on; a wave sweeps its chunk in turns of 256 bytes, lane l the four bytes of
// one aligned dword.  A dword that lies wholly inside [lo, hi) is stored as one; the partial first and last dwords of the WHOLE
// range byte by byte: no byte outside [lo, hi) is written, every byte inside exactly once.  No atomics, no memset, no LDS.
// Which piece: per chunk the wave finds pa = the last piece whose offset is <= the chunk's first byte and pb = the same for its
// last byte, by a 64-WAY SEARCH (wave_last_le: lane l probes one of 64 evenly spaced entries of the range, a ballot keeps one
// 64th: six rounds at most for 2^32 pieces; for pb the range is first cut to the kPiecesChunk + 1 entries behind pa, which hold it
// unless more empty pieces than that lie inside the chunk).  Per output byte q the lane then finds the last p in [pa, pb] with
// piece_off[p] <= q by a binary search of its own - "the last" skips every run of empty pieces by construction - and what it found
// holds up to lim = piece_off[p + 1]: the other bytes of the dword reuse it while q < lim (the later searches of a dword start at p).
// Source bytes: a dword whose four bytes lie in one piece is read as one dword where its source address is aligned, as two aligned
// dwords and a funnel shift where both of them lie wholly inside the piece, and byte by byte otherwise - the standing rule of
// item_lanes.hpp: a wide load only where all its bytes lie inside the piece.  No byte outside [piece_src[p], piece_src[p] + len_p)
// is read.  Offsets that do not ascend are the caller's error: the stores stay inside [lo, hi) even then.
// Every lane of a wave makes every turn of the chunk loop and of the searches' rounds (the ballots are the wave's).

// the last index in [a, b) whose entry is <= q, for ascending entries with v[a] <= q; a and b are the same in every lane
__device__ __forceinline__ uint64_t wave_last_le(const uint64_t *__restrict__ v, uint64_t a, uint64_t b, uint64_t q, uint32_t lane) {
    while (b - a > 1) {
        const uint64_t step = (b - a + 63) >> 6, idx = a + lane * step;
        const uint64_t votes = __ballot(idx < b && v[idx] <= q);       // a prefix of the lanes, lane 0 among them
        a += (uint64_t)(__popcll(votes | 1) - 1) * step;
        b = a + step < b ? a + step : b;
    }
    return a;
}

__global__ __launch_bounds__(kThreads, 8) void pieces_fill_kernel(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ piece_src,
                                                                 const uint64_t *__restrict__ piece_off, size_t npieces, uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = piece_off[0], hi = piece_off[npieces];
    if (hi <= lo) return;
    const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(out) + lo) & 3u);
    const uint64_t span = (hi - lo) + mis;                              // the sweep: bytes [0, span) from the aligned dword of out + lo on
    const uint64_t nchunks = (span + kPiecesChunk - 1) / kPiecesChunk;
    const uint64_t waves = (uint64_t)gridDim.x * (kThreads / 64);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (the chunk and the searches' bounds: scalar registers)
    for (uint64_t chunk = (uint64_t)blockIdx.x * (kThreads / 64) + wave; chunk < nchunks; chunk += waves) {
        const uint64_t rel0 = chunk * kPiecesChunk, rel1 = rel0 + kPiecesChunk < span ? rel0 + kPiecesChunk : span;
        const uint64_t q_first = lo + (rel0 < mis ? 0 : rel0 - mis), q_last = lo + (rel1 - mis) - 1;
        const uint64_t pa = wave_last_le(piece_off, 0, npieces, q_first, lane);
        uint64_t near = pa + kPiecesChunk + 1;                          // (a chunk holds the first byte of kPiecesChunk pieces at most)
        if (near >= npieces || piece_off[near] <= q_last) near = npieces;
        const uint64_t pb = wave_last_le(piece_off, pa, near, q_last, lane);
        for (uint64_t rel = rel0 + lane * 4; rel < rel1; rel += 256) {
            const uint32_t c0 = rel < mis ? mis - (uint32_t)rel : 0u;                          // (rel < mis: rel == 0)
            const uint32_t c1 = span - rel < 4 ? (uint32_t)(span - rel) : 4u;
            // the piece that holds the byte located last: output bytes below lim come from bytes[origin + q]
            uint64_t p = pa, lim = 0, origin = 0;
            auto locate = [&](uint64_t q) {
                uint64_t above = pb;                                    // the last p in [p, pb] with piece_off[p] <= q
                while (p < above) {
                    const uint64_t mid = p + ((above - p + 1) >> 1);
                    if (piece_off[mid] <= q) p = mid;
                    else above = mid - 1;
                }
                lim = piece_off[p + 1];
                origin = piece_src[p] - piece_off[p];
            };
            uint32_t word = 0;
            const uint64_t q0 = lo + (rel + c0 - mis);
            locate(q0);
            const uint8_t *src = bytes + (origin + q0);
            if (c0 == 0 && c1 == 4 && lim - q0 >= 4) {                  // the four bytes of one piece
                const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
                if (sh == 0) word = *reinterpret_cast<const uint32_t *>(src);
                else if (q0 - piece_off[p] >= sh && lim - q0 >= 8 - sh) {                       // both aligned dwords inside the piece
                    const uint32_t *w = reinterpret_cast<const uint32_t *>(src - sh);
                    word = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> (8 * sh));
                } else word = src[0] | (uint32_t)src[1] << 8 | (uint32_t)src[2] << 16 | (uint32_t)src[3] << 24;
            } else {
                for (uint32_t c = c0; c < c1; c++) {
                    const uint64_t q = q0 + (c - c0);
                    if (q >= lim) locate(q);
                    word |= (uint32_t)bytes[origin + q] << (8 * c);
                }
            }
            uint8_t *dst = out + (lo + rel) - mis;                      // (4-byte aligned; below out + lo only where c0 > 0: not stored to)
            if (c0 == 0 && c1 == 4) *reinterpret_cast<uint32_t *>(dst) = word;
            else for (uint32_t c = c0; c < c1; c++) dst[c] = (uint8_t)(word >> (8 * c));
        }
    }
}

}  // namespace

int pieces_sizes(const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_start, const uint32_t *match_end,
                 bool gaps, uint64_t *list_off, uint32_t *piece_len, uint64_t *piece_src, uint32_t *too_long, void *stream) {
    if (!nitems) return 0;
    return launch_item_lanes<pieces_sizes_kernel>(0, nitems, kReplaceMaxBlocks, stream, off, nitems, trim, first, match_start, match_end, gaps ? 1u : 0u,
                                                  list_off, piece_len, piece_src, too_long);
}

int pieces_fill(const uint8_t *bytes, const uint64_t *piece_src, const uint64_t *piece_off, size_t npieces, uint8_t *out, void *stream) {
    if (!npieces) return 0;
    // the output's size is on the device: a full grid whatever it is - a wave without a chunk reads two words and ends
    hipLaunchKernelGGL(pieces_fill_kernel, dim3((unsigned)kPiecesMaxBlocks), dim3(kThreads), 0, (hipStream_t)stream, bytes, piece_src, piece_off, npieces, out);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
