// multi.cpp — rrx_multi: a set of up to 32 patterns, its members cut into groups that share one product table each (plan.hpp:
// plan_multi), and the entries that say which of the patterns every item of a batch contains (rrx_multi_contains_extents /
// _items: kernels_multi_items.hip, one launch per group) or every line of a '\n'-corpus (rrx_multi_contains_corpus:
// kernels_multi_corpus.hip, the same launches stripe-wise), with the two readers of a mask column (rrx_multi_counts, rrx_multi_plane).
#include "items.hpp"

using namespace rrx;

// The plan and, per device, the groups' tables in one image.  Everything an entry could refuse for is settled at compile.
struct rrx_multi {
    size_t npatterns = 0;
    MultiPlan plan;
    mutable std::mutex mu;
    mutable std::map<int, OnDevice<std::vector<dev::MultiDevice>>> on_device;      // (under `mu`)
    // The tables on `device`, uploaded once
    int tables(int device, const std::vector<dev::MultiDevice> **out) const {
        std::lock_guard<std::mutex> lock(mu);
        auto it = on_device.find(device);
        if (it == on_device.end()) {
            Image img;
            OnDevice<std::vector<dev::MultiDevice>> t;
            t.d.resize(plan.groups.size());                          // (sized before the packer takes the fields' addresses)
            for (size_t g = 0; g < plan.groups.size(); g++) pack_multi(plan.groups[g].table, img, t.d[g]);
            const hipError_t e = upload(device, img, t.mem);
            if (e != hipSuccess) return hip_fail(e, "device table upload");
            it = on_device.emplace(device, std::move(t)).first;
        }
        *out = &it->second.d;
        return RRX_OK;
    }
};

namespace {

// One launch per group that can find anything: the first one stores the masks, the others OR theirs in.  No such group - every
// member the empty language -: the masks are cleared.  launch(table, in_global, first): a dev:: launcher on the nmasks items.
template <class Launch>
int multi_launches(const rrx_multi *m, int device, size_t nmasks, uint32_t *d_mask, void *stream, Launch launch) {
    if (!nmasks) return RRX_OK;
    const std::vector<dev::MultiDevice> *t = nullptr;
    const int rc = m->tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    bool first = true;
    for (size_t g = 0; g < t->size(); g++) {
        if (!(*t)[g].full) continue;
        const int lrc = launched(launch((*t)[g], m->plan.groups[g].in_global, first), "multi contains launch");
        if (lrc) return lrc;
        first = false;
    }
    if (first) HIP_TRY(hipMemsetAsync(d_mask, 0, nmasks * sizeof(uint32_t), (hipStream_t)stream));
    return RRX_OK;
}
int multi_contains(const rrx_multi *m, const ItemBatch &b, uint32_t *d_mask, void *stream) {
    return multi_launches(m, b.device, b.nitems, d_mask, stream, [&](const dev::MultiDevice &t, bool in_global, bool first) {
        return dev::multi_contains_extents(t, in_global, first, b.bytes, b.off, b.nitems, b.trim, d_mask, stream);
    });
}

}  // namespace

extern "C" {

int rrx_multi_compile_ex(const char *const *patterns, size_t npatterns, int engine, uint32_t max_rows, rrx_multi **out) {
    if (!patterns || !out) return fail(RRX_ERR_ARG, "null argument");
    *out = nullptr;
    if (!npatterns || npatterns > kMultiMaxPatterns) return fail(RRX_ERR_ARG, "a pattern set holds 1 to 32 patterns");
    if (engine != RRX_ENGINE_AUTO && engine != RRX_ENGINE_DFA && engine != RRX_ENGINE_DFA_GLOBAL)
        return fail(RRX_ERR_ARG, "a pattern set runs on tables: RRX_ENGINE_AUTO, RRX_ENGINE_DFA or RRX_ENGINE_DFA_GLOBAL");
    for (size_t k = 0; k < npatterns; k++)
        if (!patterns[k]) return fail(RRX_ERR_ARG, "pattern " + std::to_string(k) + ": null argument");
    std::vector<DfaProgram> members(npatterns);
    for (size_t k = 0; k < npatterns; k++) {
        const std::string who = "pattern " + std::to_string(k) + ": ";
        try {
            if (!lower_multi_member(patterns[k], members[k]))
                return fail(RRX_ERR_UNSUPPORTED, who + "the forward search automaton does not determinise within the state budget");
        } catch (const PatternError &e) {
            return fail(RRX_ERR_PATTERN, who + e.what());
        } catch (const BudgetError &e) {
            return fail(RRX_ERR_UNSUPPORTED, who + e.what());
        } catch (const std::exception &e) {
            return fail(RRX_ERR_PATTERN, who + "internal: " + e.what());
        }
    }
    std::unique_ptr<rrx_multi> m(new rrx_multi());
    m->npatterns = npatterns;
    plan_multi(members, engine == RRX_ENGINE_DFA_GLOBAL, max_rows, m->plan);
    *out = m.release();
    return RRX_OK;
}
int rrx_multi_compile(const char *const *patterns, size_t npatterns, rrx_multi **out) { return rrx_multi_compile_ex(patterns, npatterns, RRX_ENGINE_AUTO, 0, out); }
void rrx_multi_free(rrx_multi *m) { delete m; }
size_t rrx_multi_patterns(const rrx_multi *m) { return m ? m->npatterns : 0; }
size_t rrx_multi_groups(const rrx_multi *m) { return m ? m->plan.groups.size() : 0; }
uint32_t rrx_multi_group_mask(const rrx_multi *m, size_t group) { return m && group < m->plan.groups.size() ? m->plan.groups[group].members : 0; }
uint32_t rrx_multi_group_states(const rrx_multi *m, size_t group) { return m && group < m->plan.groups.size() ? m->plan.groups[group].table.nstates : 0; }
size_t rrx_multi_program_words(const rrx_multi *m, size_t group, uint32_t *out, size_t cap) {
    if (!m || group >= m->plan.groups.size()) return 0;
    std::vector<uint32_t> w;
    append_words(w, m->plan.groups[group].table);
    for (size_t i = 0; i < w.size() && i < cap; i++) out[i] = w[i];
    return w.size();
}

int rrx_multi_contains_extents(const rrx_multi *m, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                               uint32_t *d_mask, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!batch_args_ok(m, b, {d_mask})) return fail(RRX_ERR_ARG, "null argument");
    return multi_contains(m, b, d_mask, stream);
}
int rrx_multi_contains_items(const rrx_multi *m, const rrx_items *it, uint32_t *d_mask, void *stream) {
    if (!it || !batch_args_ok(m, batch_of(it), {d_mask})) return fail(RRX_ERR_ARG, "null argument");
    return multi_contains(m, batch_of(it), d_mask, stream);
}

int rrx_multi_contains_corpus(const rrx_multi *m, const rrx_corpus *c, uint32_t *d_mask, void *stream) {
    if (!m || !c || !d_mask) return fail(RRX_ERR_ARG, "null argument");
    return multi_launches(m, c->device, c->nlines, d_mask, stream, [&](const dev::MultiDevice &t, bool in_global, bool first) {
        return dev::multi_contains_corpus(t, in_global, first, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_mask, stream);
    });
}

int rrx_multi_counts(int device, const uint32_t *d_mask, size_t nitems, uint64_t *d_counts, void *stream) {
    if (!d_counts || (nitems && !d_mask)) return fail(RRX_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemsetAsync(d_counts, 0, kMultiMaxPatterns * sizeof(uint64_t), (hipStream_t)stream));
    return launched(dev::multi_counts(d_mask, nitems, reinterpret_cast<unsigned long long *>(d_counts), stream), "multi counts launch");
}
int rrx_multi_plane(int device, const uint32_t *d_mask, size_t nitems, uint32_t pattern, uint32_t *d_bits, void *stream) {
    if (nitems && (!d_mask || !d_bits)) return fail(RRX_ERR_ARG, "null argument");
    if (pattern >= kMultiMaxPatterns) return fail(RRX_ERR_ARG, "a mask has bits 0 to 31");
    if (!nitems) return RRX_OK;
    HIP_TRY(hipSetDevice(device));
    return launched(dev::multi_plane(d_mask, nitems, pattern, d_bits, stream), "multi plane launch");
}

}  // extern "C"
