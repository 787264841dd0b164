// table_order.cpp — see table_order.hpp.
#include "table_order.hpp"

#include <algorithm>
#include <memory>

namespace rrx {

Dfa2OrderStats order_dfa2(const Dfa2Program &d, const uint8_t *sample, uint32_t lanes, uint32_t bytes_per_lane,
                          std::vector<uint32_t> &row_slot, std::vector<uint32_t> &col_slot) {
    Dfa2OrderStats st;
    const uint32_t D = d.nstates, C = d.ncols, P = C | 1u;
    row_slot.resize(D); col_slot.resize(C);
    for (uint32_t i = 0; i < D; i++) row_slot[i] = i;
    for (uint32_t i = 0; i < C; i++) col_slot[i] = i;
    const uint32_t groups = lanes / 32, steps = bytes_per_lane / 2;
    if (!groups || !steps || D < 2 || C < 2) return st;
    // ---- the half-waves: per group and step the DISTINCT (row, column) pairs its 32 lanes look up
    struct Entry { uint16_t row, col; };
    std::vector<Entry> entries;
    std::vector<uint32_t> first;                                  // half-wave h: entries[first[h] .. first[h + 1])
    std::vector<uint64_t> freq_row(D, 0), freq_col(C, 0);
    std::vector<uint32_t> state(32);
    for (uint32_t g = 0; g < groups; g++) {
        std::fill(state.begin(), state.end(), 0u);                // dead: a stripe begins inside somebody else's line
        for (uint32_t k = 0; k < steps; k++) {
            first.push_back((uint32_t)entries.size());
            Entry hw[32];
            uint32_t n = 0;
            for (uint32_t l = 0; l < 32; l++) {
                const uint8_t *t = sample + ((size_t)g * 32 + l) * bytes_per_lane + 2 * k;
                const uint32_t c1 = t[0] < 0x80 ? t[0] : 0, c2 = t[1] < 0x80 ? t[1] : 0;       // (a corpus with bytes >= 0x80 does not get here)
                const uint32_t col = d.pair_col[c1 * 128 + c2], row = state[l];
                freq_row[row]++; freq_col[col]++;
                bool seen = false;
                for (uint32_t q = 0; q < n && !seen; q++) seen = hw[q].row == row && hw[q].col == col;
                if (!seen) hw[n++] = Entry{(uint16_t)row, (uint16_t)col};
                state[l] = d.next2[(size_t)row * C + col] & 0xffffu;
            }
            entries.insert(entries.end(), hw, hw + n);
        }
    }
    first.push_back((uint32_t)entries.size());
    const uint32_t H = (uint32_t)first.size() - 1;
    st.half_waves = H;
    auto cost_of = [&](uint32_t h) -> uint32_t {                  // the fullest bank of half-wave h
        uint8_t bank[32] = {0};
        uint32_t worst = 0;
        for (uint32_t q = first[h]; q < first[h + 1]; q++) {
            const uint32_t b = (row_slot[entries[q].row] * P + col_slot[entries[q].col]) & 31u;
            if (++bank[b] > worst) worst = bank[b];
        }
        return worst;
    };
    std::vector<uint8_t> hw_cost(H);
    uint64_t best = 0;
    for (uint32_t h = 0; h < H; h++) { hw_cost[h] = (uint8_t)cost_of(h); best += hw_cost[h]; }
    st.before = (double)best / H;
    // a swap only changes the half-waves that hold an entry of one of the two rows (columns): their lists
    std::vector<std::vector<uint32_t>> in_row(D), in_col(C);
    for (uint32_t h = 0; h < H; h++)
        for (uint32_t q = first[h]; q < first[h + 1]; q++) {
            std::vector<uint32_t> &r = in_row[entries[q].row], &c = in_col[entries[q].col];
            if (r.empty() || r.back() != h) r.push_back(h);
            if (c.empty() || c.back() != h) c.push_back(h);
        }
    std::vector<uint32_t> stamp(H, 0), touched;
    uint32_t epoch = 0;
    constexpr uint32_t kTop = 32;                                 // the hottest rows, then the hottest columns
    for (int pass = 0; pass < 2; pass++) {                        // pass 0: rows, pass 1: columns
        std::vector<uint32_t> &slot = pass == 0 ? row_slot : col_slot;
        const std::vector<uint64_t> &freq = pass == 0 ? freq_row : freq_col;
        const std::vector<std::vector<uint32_t>> &in = pass == 0 ? in_row : in_col;
        const uint32_t n = pass == 0 ? D : C, mult = pass == 0 ? P : 1u;
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return freq[a] != freq[b] ? freq[a] > freq[b] : a < b; });
        // the change of the total if k and j trade slots (the slots are left traded; the caller trades back or keeps)
        auto trade = [&](uint32_t k, uint32_t j) -> int64_t {
            std::swap(slot[k], slot[j]);
            epoch++;
            touched.clear();
            int64_t delta = 0;
            for (const std::vector<uint32_t> *list : {&in[k], &in[j]})
                for (uint32_t h : *list) {
                    if (stamp[h] == epoch) continue;
                    stamp[h] = epoch;
                    touched.push_back(h);
                    delta += (int64_t)cost_of(h) - hw_cost[h];
                }
            st.evaluations++;
            return delta;
        };
        for (uint32_t oi = 0; oi < n && oi < kTop; oi++) {
            const uint32_t k = order[oi];
            if (!freq[k] || (pass == 0 && k == 0)) continue;
            // candidates: for every other bank residue, the least used member that sits there
            int64_t cand[32];
            for (int r = 0; r < 32; r++) cand[r] = -1;
            for (uint32_t j = 0; j < n; j++) {
                if (j == k || (pass == 0 && j == 0)) continue;
                const uint32_t r = (slot[j] * mult) & 31u;
                if (cand[r] < 0 || freq[j] < freq[(size_t)cand[r]]) cand[r] = j;
            }
            int64_t pick = -1, pick_delta = 0;
            const uint32_t mine = (slot[k] * mult) & 31u;
            for (int r = 0; r < 32; r++) {
                if (cand[r] < 0 || (uint32_t)r == mine) continue;
                const uint32_t j = (uint32_t)cand[r];
                const int64_t d = trade(k, j);
                if (d < pick_delta) { pick_delta = d; pick = j; }
                std::swap(slot[k], slot[j]);
            }
            if (pick >= 0) {
                (void)trade(k, (uint32_t)pick);
                for (uint32_t h : touched) hw_cost[h] = (uint8_t)cost_of(h);
                best = (uint64_t)((int64_t)best + pick_delta);
            }
        }
    }
    st.after = (double)best / H;
    return st;
}

bool TableOrderSearch::start(const Dfa2Program &d, std::vector<uint8_t> sample, uint32_t lanes, uint32_t bytes_per_lane, bool background, Apply apply) {
    // (shared_ptr: std::function wants a copyable callable)
    auto text = std::make_shared<std::vector<uint8_t>>(std::move(sample));
    return OnceTask::start([&d, text, lanes, bytes_per_lane, apply]() {
        std::vector<uint32_t> rows, cols;
        const Dfa2OrderStats st = order_dfa2(d, text->data(), lanes, bytes_per_lane, rows, cols);
        apply(std::move(rows), std::move(cols), st);
    }, background);
}

}  // namespace rrx
