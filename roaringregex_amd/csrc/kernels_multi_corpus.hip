// kernels_multi_corpus.hip — "which patterns of a set does each line contain" (rrx_multi_contains_corpus): the product table of a
// group of members (lower.hpp: MultiProgram) stepped stripe-wise over a '\n'-corpus, a lane per stripe as in the batch kernel.
#include "multi_engines.hpp"

namespace rrx {
namespace dev {
namespace {

// Lane g owns the lines that START in stripe g - lines lo .. past - 1, from the corpus' stripe index exactly as recheck_escaped_kernel
// takes them - and walks from the stripe's first byte: a stripe that begins inside somebody else's line is skipped to behind its
// first '\n', and the last line is followed past the end of the stripe to its '\n' or to the end of the data.  A lane without a
// line of its own leaves at once.  Per line the items kernel's walk: m = mask[start], per byte the row steps and the rows that
// carry a mask (s >= first_hit) OR theirs in; at the '\n' (at the end of the data for a last line without one) the line's word is
// stored (FIRST) or ORed into - the lane owns the word: plain loads and stores, nothing to clear beforehand.  Once m == full
// (`done`; also while skipping, and once the lane's last line is out) the table rests and the text is tested for '\n' a 32-bit
// word at a time.  The text comes 16 bytes per load from 16-byte aligned addresses, a 128-byte line per burst while one lies inside
// the data; the slots are named (TextRound), never indexed: nothing lives in scratch.  No byte at or beyond nbytes is read.
template <class Engine, bool FIRST>
__global__ __launch_bounds__(kThreads) void multi_contains_corpus_kernel(MultiDevice prog, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                                          const uint64_t *__restrict__ stripe_base, size_t nstripes,
                                                                          uint32_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Engine eng;
    eng.load(prog, smem);
    __syncthreads();
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= nstripes) return;
    const uint64_t b0 = stripe_base[g], b1 = stripe_base[g + 1];
    const bool fresh = (b0 & kFreshStripe) != 0;
    const bool next_fresh = g + 1 < nstripes ? (b1 & kFreshStripe) != 0 : bytes[nbytes - 1] == '\n';
    const uint64_t lo = line_of(b0) + (fresh ? 0u : 1u);                          // the lines that start in my stripe: lo .. past - 1
    const uint64_t past = line_of(b1) + (next_fresh ? 0u : 1u);
    if (past <= lo) return;
    const int32_t mine = (int32_t)(past - lo);                                    // (a stripe holds at most kMaxStripe of them)
    uint32_t *__restrict__ word_of = out + lo;
    const uint32_t first_hit = prog.first_hit, full = prog.full, start = prog.start;
    const uint32_t m0 = eng.mask[start];

    int32_t line = fresh ? 0 : -1;                 // relative to lo; -1: the line my stripe begins in, somebody else's
    uint32_t s = start, m = m0;
    bool done = !fresh || m0 == full;              // nothing to step until the next '\n'
    auto store = [&]() { word_of[line] = FIRST ? m : word_of[line] | m; };
    auto one = [&](uint32_t c) {
        if (c == '\n') {
            if (line < mine) {                     // (line == mine: my last line is out)
                if (line >= 0) store();
                line++;
                s = start; m = m0;
                done = m0 == full || line == mine;
            }
        } else if (!done) {
            s = eng.step(s, c);
            if (s >= first_hit) { m |= eng.mask[s]; done = m == full; }
        }
    };
    auto four = [&](uint32_t w) {
        if (done && !newline_flags(w)) return;
#pragma unroll
        for (int k = 0; k < 4; k++) one((w >> (8 * k)) & 0xffu);
    };
    auto sixteen = [&](const uint4 &v) { four(v.x); four(v.y); four(v.z); four(v.w); };

    size_t pos = g * (size_t)stripe;               // 16-byte aligned: the corpus' base is, and a stripe is a power of two >= 512
    while (line < mine && pos + kRound <= nbytes) {
        TextRound<kRound / 16> buf;
        buf.load(reinterpret_cast<const uint4 *>(bytes + pos));
        buf.for_each_slot(sixteen);
        pos += kRound;
    }
    for (; line < mine && pos + 16 <= nbytes; pos += 16) sixteen(load_text(reinterpret_cast<const uint4 *>(bytes + pos)));
    for (; line < mine && pos < nbytes; pos++) one(bytes[pos]);
    if (line >= 0 && line < mine) store();         // the corpus ends without '\n': the end of the data ends my last line
}

template <class Engine, bool FIRST>
int launch_one(const MultiDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes, uint32_t *out,
               void *stream) {
    auto k = multi_contains_corpus_kernel<Engine, FIRST>;
    const size_t lds = Engine::lds_bytes(p);
    static LdsAttr attr;
    const hipError_t e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(k), lds);
    if (e != hipSuccess) return (int)e;
    const size_t blocks = (nstripes + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, p, bytes, nbytes, stripe, stripe_base, nstripes, out);
    return (int)hipGetLastError();
}
template <class Engine>
int launch_multi_corpus(const MultiDevice &p, bool first, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes,
                        uint32_t *out, void *stream) {
    if (first) return launch_one<Engine, true>(p, bytes, nbytes, stripe, stripe_base, nstripes, out, stream);
    return launch_one<Engine, false>(p, bytes, nbytes, stripe, stripe_base, nstripes, out, stream);
}

}  // namespace

int multi_contains_corpus(const MultiDevice &p, bool in_global, bool first, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                          size_t nstripes, uint32_t *out, void *stream) {
    if (!nstripes || !nbytes) return 0;
    if (!p.nstates || !p.next || !p.cls || !p.mask || p.start >= p.nstates) return (int)hipErrorInvalidValue;
    if (in_global || MultiLdsEngine::lds_bytes(p) > kPlainDfaLdsBudget)
        return launch_multi_corpus<MultiGlobalEngine>(p, first, bytes, nbytes, stripe, stripe_base, nstripes, out, stream);
    return launch_multi_corpus<MultiLdsEngine>(p, first, bytes, nbytes, stripe, stripe_base, nstripes, out, stream);
}

}  // namespace dev
}  // namespace rrx
