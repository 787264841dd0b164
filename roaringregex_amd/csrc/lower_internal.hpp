// lower_internal.hpp — what the lower_*.cpp units share.  Nothing outside them includes this.
#pragma once
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <utility>

#include "lower.hpp"

namespace rrx {

using Node = Reduced::Node;

inline void sort_unique(std::vector<uint32_t> &v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
inline bool subset(const CharSet &x, const CharSet &y) { return !(x.w[0] & ~y.w[0]) && !(x.w[1] & ~y.w[1]); }

// An empty table over the byte classes of `src` (a Reduced or a DfaProgram) ...
template <class Src> DfaProgram classes_of(const Src &src) {
    DfaProgram d;
    std::memcpy(d.cls, src.cls, sizeof d.cls);
    d.ncls = src.ncls;
    return d;
}
// ... and the table of the empty language over them: one dead row, which is the start.
template <class Src> DfaProgram dead_dfa(const Src &src) {
    DfaProgram d = classes_of(src);
    d.nstates = 1; d.start = 0; d.accepting = {0}; d.next.assign(d.ncls, 0);
    return d;
}

// Pairs of states numbered in first-seen order (the rows of a product table).
struct PairInterner {
    std::unordered_map<uint64_t, uint32_t> ids;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    // the id of (a, b); -1 where the pair is new and `cap` pairs are held already
    int64_t intern(uint32_t a, uint32_t b, size_t cap = SIZE_MAX) {
        const uint64_t key = ((uint64_t)a << 32) | b;
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        if (pairs.size() >= cap) return -1;
        ids.emplace(key, (uint32_t)pairs.size());
        pairs.emplace_back(a, b);
        return (int64_t)pairs.size() - 1;
    }
};

}  // namespace rrx
