// The host side of a pattern set (rrx_multi) under AddressSanitizer + UBSan (CPU only): pattern -> lower_multi_member (the front
// end, the forward search table) -> plan_multi (product, minimisation, grouping) at several row limits and in the global
// form -> pack_multi, the image copied and every group's table stepped from the copy over a few items exactly as the kernel is
// specified.  The OR of the groups' masks must equal what the members' own tables say; a mismatch aborts.
// build + run: make -C tools/sanitize multi            (the sets below)
//              make -C tools/sanitize multi SETS=file  (one set per line: its patterns in hex, separated by blanks)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../roaringregex_amd/csrc/frontend.hpp"
#include "../../roaringregex_amd/csrc/lower.hpp"
#include "../../roaringregex_amd/csrc/pack.hpp"
#include "../../roaringregex_amd/csrc/plan.hpp"

using namespace rrx;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #cond, __LINE__); std::abort(); } \
    } while (0)

typedef std::vector<std::string> Set;

static std::vector<Set> read_sets(const char *path) {
    std::vector<Set> sets;
    std::ifstream in(path);
    CHECK(in.good());
    for (std::string line; std::getline(in, line);) {
        std::istringstream words(line);
        Set s;
        for (std::string hex; words >> hex;) {
            CHECK(hex.size() % 2 == 0);
            std::string p;
            for (size_t i = 0; i < hex.size(); i += 2) p.push_back((char)std::stoi(hex.substr(i, 2), nullptr, 16));
            s.push_back(p);
        }
        if (!s.empty()) sets.push_back(s);
    }
    return sets;
}

// The member's own verdict: its forward search table from the start, every byte through its class - some state on the way accepts
static bool member_contains(const DfaProgram &d, const std::string &item) {
    uint32_t s = d.start;
    bool hit = d.accepting[s] != 0;
    for (unsigned char c : item) {
        s = d.next[(size_t)s * d.ncls + d.cls[c]];
        hit = hit || d.accepting[s];
    }
    return hit;
}

// The kernel's walk on one group's table, from a copy of the image
static uint32_t group_mask(const dev::MultiDevice &t, const std::string &item) {
    uint32_t s = t.start;
    CHECK(s < t.nstates);
    uint32_t m = t.mask[s];
    for (unsigned char c : item) {
        if (m == t.full) break;
        CHECK(t.cls[c] < t.ncls);
        s = t.next[(size_t)s * t.ncls + t.cls[c]];
        CHECK(s < t.nstates);
        if (s >= t.first_hit) m |= t.mask[s];
    }
    return m;
}

int main(int argc, char **argv) {
    std::vector<Set> sets = {{"ab+c"},
                             {"ab+c", "a*", "(a|b)*abb", "[0-9]+\\.[0-9]+", "x?y?z?", "k(1|10|100)", "a{2,4}b", ".*c", "c.*", "[^a]b"},
                             {"a\nb", "k\n+1", "ab+c", "ab+c"},
                             {"[]", "a*", "[]"},
                             {"[A-Za-z0-9._]+@[A-Za-z0-9.]+", "(http|https|ftp)://[a-z0-9.]+(/[a-z0-9]+)*", "[0-9]{1,3}(\\.[0-9]{1,3}){3}"}};
    if (argc > 1) sets = read_sets(argv[1]);
    const std::vector<std::string> items = {"", "a", "abbc", "zzabbbc\xff", "k100 1.5 aabb", "a\nb", "k\n\n1", "x@y.z http://a.b/c 10.0.0.1", std::string("ab\0c", 4),
                                            "yzabck1.25\xc3\xa9" "aab", "ccccccccccccccccccccccccccccccccab"};
    size_t plans = 0;
    for (const Set &set : sets) {
        CHECK(!set.empty() && set.size() <= kMultiMaxPatterns);
        std::vector<DfaProgram> members(set.size());
        for (size_t k = 0; k < set.size(); k++) CHECK(lower_multi_member(set[k], members[k]));
        const uint32_t all = set.size() == 32 ? ~0u : (1u << set.size()) - 1u;
        for (int global = 0; global < 2; global++)
            for (uint32_t max_rows : {0u, 1u, 8u, 16u, 64u}) {
                MultiPlan plan;
                plan_multi(members, global != 0, max_rows, plan);
                CHECK(!plan.groups.empty());
                Image img;
                std::vector<dev::MultiDevice> t(plan.groups.size());
                uint32_t seen = 0;
                for (size_t g = 0; g < plan.groups.size(); g++) {
                    const MultiGroup &grp = plan.groups[g];
                    const MultiProgram &p = grp.table;
                    CHECK(grp.members && !(grp.members & seen) && grp.members > seen);
                    seen |= grp.members;
                    CHECK(!max_rows || p.nstates <= max_rows || !(grp.members & (grp.members - 1)));
                    CHECK(global ? grp.in_global : grp.in_global == (dev::multi_lds_bytes(p.nstates, p.ncls) > dev::kPlainDfaLdsBudget));
                    CHECK(p.nstates && p.nstates <= kMultiMaxRows && p.next.size() == (size_t)p.nstates * p.ncls && p.mask.size() == p.nstates);
                    uint32_t full = 0;
                    for (uint32_t s = 0; s < p.nstates; s++) {
                        CHECK((p.mask[s] == 0) == (s < p.first_hit));
                        full |= p.mask[s];
                    }
                    CHECK(full == p.full && !(full & ~grp.members));
                    pack_multi(p, img, t[g]);
                }
                CHECK(seen == all);
                std::vector<uint8_t> copy(img.bytes);
                img.bind(copy.data());
                for (const std::string &item : items) {
                    uint32_t got = 0, want = 0;
                    for (const dev::MultiDevice &d : t) got |= group_mask(d, item);
                    for (size_t k = 0; k < set.size(); k++) want |= member_contains(members[k], item) ? 1u << k : 0u;
                    if (got != want) { std::fprintf(stderr, "set of %zu, max_rows %u, global %d: %08x, the members say %08x\n", set.size(), max_rows, global, got, want); std::abort(); }
                }
                plans++;
            }
    }
    DfaProgram d;                                     // a forward table that does not determinise: no member
    CHECK(!lower_multi_member("(a|b)*a(a|b){40}", d));
    std::printf("multi product host pipeline: %zu sets, %zu plans ok\n", sets.size(), plans);
    return 0;
}
