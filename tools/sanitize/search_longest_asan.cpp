// The host side of the leftmost-longest search under AddressSanitizer + UBSan (CPU only): pattern -> reduce -> plan_search_longest
// (the starts table and the anchored table) -> pack_search_longest, the image copied and both tables stepped from the copy over a few
// items exactly as the kernel is specified.  Known answers abort on a mismatch.
// build + run: make -C tools/sanitize longest
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../roaringregex_amd/csrc/frontend.hpp"
#include "../../roaringregex_amd/csrc/lower.hpp"
#include "../../roaringregex_amd/csrc/pack.hpp"
#include "../../roaringregex_amd/csrc/plan.hpp"
#include "../../include/rrx.h"

using namespace rrx;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #cond, __LINE__); std::abort(); } \
    } while (0)

struct Case { const char *pattern, *item; long start, end; };

static void search(const dev::SearchLongestDevice &t, bool nullable, const std::string &item, long &start, long &end) {
    auto step = [](const dev::DfaDevice &d, uint32_t s, unsigned char c) { return (uint32_t)d.next[(size_t)s * d.ncls + d.cls[c]]; };
    start = nullable ? 0 : -1;
    end = -1;
    if (!nullable) {
        uint32_t s = t.starts.start;
        for (long q = (long)item.size() - 1; q >= 0; q--) {
            s = step(t.starts, s, (unsigned char)item[q]);
            CHECK(s < t.starts.nstates);
            if (t.starts.acc[s]) start = q;
        }
        if (start < 0) return;
    }
    uint32_t s = t.anchored.start;
    if (nullable) end = 0;
    for (size_t p = (size_t)start; p < item.size() && s; p++) {
        s = step(t.anchored, s, (unsigned char)item[p]);
        CHECK(s < t.anchored.nstates);
        if (t.anchored.acc[s]) end = (long)p + 1;
    }
    CHECK(end >= 0);
}

int main() {
    const Case cases[] = {{"[0-9]+", "abc 12345 x", 4, 9}, {"abcd|c", "abcd", 0, 4}, {"ab|b+", "abbb", 0, 2}, {"a*", "aaab", 0, 3}, {"a*", "baa", 0, 0},
                          {"a*", "", 0, 0}, {"ab+c", "zzabbbc\xff", 2, 7}, {"ab+c", "ab", -1, -1}, {"x[ab]{12}a[ab]*", "xbbbbbbbbbbbbabab", 0, 17}};
    size_t n = 0;
    for (const Case &c : cases) {
        Programs progs;
        plan_engines(c.pattern, RRX_ENGINE_AUTO, progs);
        SearchLongestPlan plan;
        CHECK(plan_search_longest(reduce(progs.trimmed), progs.accepts_empty(), plan) && !plan.empty);
        Image img;
        dev::SearchLongestDevice t;
        CHECK(pack_search_longest(plan.starts, plan.anchored, img, t));
        std::vector<uint8_t> copy(img.bytes);
        img.bind(copy.data());
        long start, end;
        search(t, plan.nullable, c.item, start, end);
        if (start != c.start || end != c.end) { std::fprintf(stderr, "%s on %s: [%ld, %ld)\n", c.pattern, c.item, start, end); std::abort(); }
        n++;
    }
    Programs progs;                                   // the empty language: no table
    plan_engines("[]", RRX_ENGINE_AUTO, progs);
    SearchLongestPlan plan;
    CHECK(plan_search_longest(reduce(progs.trimmed), progs.accepts_empty(), plan) && plan.empty);
    Programs big;                                     // one of the two does not determinise: neither is kept
    plan_engines("(a|b)*a(a|b){40}", RRX_ENGINE_AUTO, big);
    CHECK(!plan_search_longest(reduce(big.trimmed), false, plan) && !plan.starts.nstates && !plan.anchored.nstates);
    std::printf("search_longest host pipeline: %zu cases ok\n", n);
    return 0;
}
