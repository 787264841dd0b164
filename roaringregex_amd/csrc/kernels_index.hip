// kernels_index.hip — what a corpus index and a result bitmap need and no engine does: newline counts per stripe and their
// scan, line offsets, the matches of patterns that accept "", bitmap expansion and count, the results mailed to the host.
// Shared device code: kernels_common.hpp.
#include "kernels_common.hpp"

namespace rrx {
namespace dev {
namespace {

__global__ void mail_results_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ flags, const uint8_t *__restrict__ last_byte,
                                    uint64_t *__restrict__ mail, const uint32_t *__restrict__ own) {
    if (threadIdx.x || blockIdx.x) return;
    mail[0] = line_of(*total);
    mail[1] = flags ? *flags : 0u;
    mail[2] = last_byte ? *last_byte : (uint64_t)'\n';
    mail[3] = own ? own[0] : 0u;
    mail[4] = own ? own[1] : 0u;
    __threadfence_system();
}

// ============================================================================================ line index
// Can the batch kernel's workgroups store their result words without a cleared bitmap?  Lane = workgroup.  The lines of
// workgroup b lie in the bitmap words [first word of b, first word of b + 1]: where the first words are strictly increasing no
// word has more than two writers (own[0] stays 0); own[1] = the longest such range, which has to fit the kernel's LDS window.
// The last workgroup's range ends with the bitmap.
__global__ __launch_bounds__(256) void own_words_kernel(const uint64_t *__restrict__ stripe_base, size_t nstripes, size_t nworkgroups,
                                                        const uint8_t *__restrict__ last_byte, uint32_t *__restrict__ own) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nworkgroups) return;
    const uint64_t first = line_of(stripe_base[b * kThreads]) >> 5;
    uint64_t last;
    if (b + 1 < nworkgroups) {
        last = line_of(stripe_base[(b + 1) * kThreads]) >> 5;
        if (last <= first) { atomicOr(&own[0], 1u); return; }
    } else {
        const uint64_t nlines = line_of(stripe_base[nstripes]) + (*last_byte != '\n' ? 1u : 0u);      // (> 0: the corpus is not empty)
        last = (nlines - 1) >> 5;
    }
    const uint64_t span = last - first;
    atomicMax(&own[1], span < 0xffffffffull ? (uint32_t)span : 0xffffffffu);
}

// counts[g] = number of '\n' in stripe g, streamed exactly like the match kernel streams it.  Also raises
// *flags bit 0 if any byte >= 0x80 occurs (the match kernel then clamps such bytes to the dead column).
__global__ __launch_bounds__(256) void count_newlines_kernel(const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                              uint32_t *__restrict__ counts, size_t nstripes,
                                                              uint32_t *__restrict__ flags) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nstripes) return;
    const size_t start = g * (size_t)stripe;
    const size_t end = start + stripe < nbytes ? start + stripe : nbytes;
    const uint4 *src = reinterpret_cast<const uint4 *>(bytes + start);
    const int units = (int)((end - start) / 16);
    uint32_t cnt = 0, high = 0;
    int u = 0;
    for (; u + 4 <= units; u += 4) {       // 64-byte bursts: with next to no work per byte this is the fastest feed
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = src[u + i];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t x = w[j] ^ 0x0a0a0a0au;                                        // zero byte <=> '\n'
                uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);    // exact zero-byte test
                cnt += __popc(z);
                high |= w[j];
            }
        }
    }
    for (size_t p = start + (size_t)u * 16; p < end; p++) { cnt += bytes[p] == '\n'; high |= bytes[p]; }
    // bit 31: the stripe ends on a '\n', i.e. the next stripe starts a fresh line (the scan moves it to bit 63 of
    // that stripe's base, so the match kernels need not probe the byte before their stripe)
    counts[g] = cnt | (bytes[end - 1] == '\n' ? kEndsOnNewline : 0u);
    if (high & 0x80808080u) atomicOr(flags, 1u);
}

// The same counts, a WAVE per stripe: lane l reads 16 bytes at l*16 of every KiB of the stripe, so a wave instruction
// reads one contiguous KiB (the lane-per-stripe kernel above reads like the match kernel does, 64 lines 64 stripes apart
// per instruction, and reaches 4.8 TB/s; nothing here has to agree with the match kernel's geometry but the counts).
// Stripes are multiples of 1 KiB; the corpus' last, partial stripe is counted byte by byte.
__global__ __launch_bounds__(256) void count_newlines_wave_kernel(const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                                   uint32_t *__restrict__ counts, size_t nstripes,
                                                                   uint32_t *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const size_t nwaves = (size_t)gridDim.x * 4;
    uint32_t high = 0;
    for (size_t g = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6; g < nstripes; g += nwaves) {
        const size_t start = g * (size_t)stripe;
        const size_t end = start + stripe < nbytes ? start + stripe : nbytes;
        uint32_t cnt = 0, last = 0;
        if (end - start == stripe) {
            const uint4 *src = reinterpret_cast<const uint4 *>(bytes + start) + lane;
            const int n = (int)(stripe >> 10);                       // KiB per stripe: 1, 2, 4, 8, 16
            for (int i = 0; i < n; i += 4) {
                uint4 v[4];
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i + k < n) v[k] = src[(size_t)(i + k) * 64];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (i + k < n) {
                        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const uint32_t x = w[j] ^ 0x0a0a0a0au;                                        // zero byte <=> '\n'
                            const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);    // exact zero-byte test
                            cnt += __popc(z);
                            high |= w[j];
                        }
                        last = v[k].w >> 24;                         // (lane 63 of the last KiB: the stripe's last byte)
                    }
                }
            }
            last = __shfl(last, 63, 64);
        } else {
            for (size_t p = start + lane; p < end; p += 64) { const uint32_t b = bytes[p]; cnt += b == '\n'; high |= b; }
            last = bytes[end - 1];
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) counts[g] = cnt | (last == '\n' ? kEndsOnNewline : 0u);
    }
    if (__ballot((high & 0x80808080u) != 0) && lane == 0) atomicOr(flags, 1u);
}

// bytes[i] = bit i of the accept bitmap (the byte-per-line form of the result)
__global__ __launch_bounds__(256) void expand_bits_kernel(const uint32_t *__restrict__ bits, size_t nlines, uint8_t *__restrict__ out) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;          // one 32-line word -> 32 bytes
    if (w * 32 >= nlines) return;
    const uint32_t v = bits[w];
    if (w * 32 + 32 <= nlines) {
        uint4 o[2];
        uint32_t *p = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint32_t n = (v >> (4 * j)) & 0xfu;
            p[j] = (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
        }
        uint4 *dst = reinterpret_cast<uint4 *>(out + w * 32);
        dst[0] = o[0]; dst[1] = o[1];
    } else {
        for (size_t i = w * 32; i < nlines; i++) out[i] = (uint8_t)((v >> (i & 31)) & 1u);
    }
}

// exclusive scan of n counts into n+1 bases, two levels: (1) every workgroup sums its chunk of kScanChunk
// counts; (2) one workgroup scans the chunk sums; (3) every workgroup scans its chunk from its chunk base.
constexpr int kScanChunk = 4096;
__global__ __launch_bounds__(256) void scan_chunk_sums_kernel(const uint32_t *__restrict__ counts, size_t n, uint64_t *__restrict__ sums) {
    __shared__ uint64_t part[4];
    const size_t lo = (size_t)blockIdx.x * kScanChunk;
    uint64_t s = 0;
    for (size_t i = lo + threadIdx.x; i < lo + kScanChunk && i < n; i += 256) s += counts[i] & kCountMask;
#pragma unroll
    for (int d = 32; d; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// exclusive prefix over the workgroup of one value per thread (NW waves): shuffles inside a wave, the NW wave totals
// through LDS.  (The first version let thread 0 walk the partial sums one by one: 10-50 us per scan kernel, as much as
// the one-shot entry's compaction.)
template <int NW>
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t *wave_tot, uint64_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint64_t off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint64_t t = wave_tot[w];
        if (w < wave) off += t;
        tot += t;
    }
    total = tot;
    return off + inc - v;
}
__global__ __launch_bounds__(1024) void scan_sums_kernel(uint64_t *__restrict__ sums, size_t nchunks, uint64_t *__restrict__ total) {
    __shared__ uint64_t wave_tot[16];
    const size_t per = (nchunks + 1023) / 1024;
    const size_t lo = threadIdx.x * per < nchunks ? threadIdx.x * per : nchunks, hi = lo + per < nchunks ? lo + per : nchunks;
    uint64_t s = 0;
    for (size_t i = lo; i < hi; i++) s += sums[i];
    uint64_t all;
    uint64_t run = block_exclusive_scan<16>(s, wave_tot, all);
    if (threadIdx.x == 0) *total = all;
    for (size_t i = lo; i < hi; i++) { uint64_t v = sums[i]; sums[i] = run; run += v; }
}
__global__ __launch_bounds__(256) void scan_chunks_kernel(const uint32_t *__restrict__ counts, size_t n, const uint64_t *__restrict__ sums,
                                                           uint64_t *__restrict__ base) {
    __shared__ uint64_t wave_tot[4];
    constexpr int kPer = kScanChunk / 256;
    const size_t lo = (size_t)blockIdx.x * kScanChunk + (size_t)threadIdx.x * kPer;
    uint32_t c[kPer];
    uint32_t before = 0;                                   // the count word in front of mine (its kEndsOnNewline flag)
    if (lo + kPer <= n) {
        const uint4 *src = reinterpret_cast<const uint4 *>(counts + lo);      // lo is a multiple of kPer = 16 words
#pragma unroll
        for (int k = 0; k < kPer / 4; k++) { const uint4 v = src[k]; c[4 * k] = v.x; c[4 * k + 1] = v.y; c[4 * k + 2] = v.z; c[4 * k + 3] = v.w; }
    } else {
#pragma unroll
        for (int k = 0; k < kPer; k++) c[k] = lo + k < n ? counts[lo + k] : 0u;
    }
    if (lo && lo < n) before = counts[lo - 1];
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) s += c[k] & kCountMask;
    uint64_t all;
    uint64_t run = sums[blockIdx.x] + block_exclusive_scan<4>(s, wave_tot, all);
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (lo + k < n) {
            const bool fresh = lo + k == 0 || ((k ? c[k - 1] : before) & kEndsOnNewline);
            base[lo + k] = run | (fresh ? kFreshStripe : 0);
        }
        run += c[k] & kCountMask;
    }
}

// ============================================================================================ search: patterns that accept ""
// The stripe-wise kernels (kernels_search.hip) serve every pattern that does not accept the empty string.  One that does has
// a match [k, k) at EVERY offset k = 0 .. length of its line (the search moves on by one byte after an empty match), whatever
// the text: no table, only the line lengths.  line_offsets_kernel (once per corpus): lane = stripe, every '\n' at p inside the
// stripe starts the next line at p + 1 (line numbers from the stripe index).  empty_matches_kernel: lane = line.
__global__ __launch_bounds__(256) void line_offsets_kernel(const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                           const uint64_t *__restrict__ stripe_base, size_t nstripes,
                                                           uint64_t *__restrict__ line_off) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nstripes) return;
    const size_t start = g * (size_t)stripe, end = start + stripe < nbytes ? start + stripe : nbytes;
    uint64_t line = line_of(stripe_base[g]);             // index of the line that contains my first byte
    if (g == 0) line_off[0] = 0;
    size_t pos = start;
    for (; pos + 16 <= end; pos += 16) {                 // stripes start 16-byte aligned
        const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t x = w[j] ^ 0x0a0a0a0au;
            uint32_t hit = (x - 0x01010101u) & ~x & 0x80808080u;        // exact for the lowest flagged byte; refined below
            while (hit) {
                const int k = (__ffs((int)hit) - 1) >> 3;
                if (((w[j] >> (8 * k)) & 0xffu) == '\n') line_off[++line] = pos + 4 * j + k + 1;
                hit &= hit - 1;
            }
        }
    }
    for (; pos < end; pos++)
        if (bytes[pos] == '\n') line_off[++line] = pos + 1;
}

// FILL = false: count[i] = length of line i + 1.  FILL = true: the matches of line i go to the slots first[i], first[i] + 1, ...
template <bool FILL>
__global__ __launch_bounds__(256) void empty_matches_kernel(const uint64_t *__restrict__ line_off, size_t nlines, uint32_t *__restrict__ count,
                                                            const uint64_t *__restrict__ first, uint32_t *__restrict__ match_start,
                                                            uint32_t *__restrict__ match_end, uint64_t cap) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlines) return;
    const uint64_t len = line_off[i + 1] - 1 - line_off[i];      // the line without its '\n'
    if (!FILL) { count[i] = (uint32_t)(len + 1); return; }
    const uint64_t slot = first[i];
    for (uint64_t k = 0; k <= len && slot + k < cap; k++) { match_start[slot + k] = (uint32_t)k; match_end[slot + k] = (uint32_t)k; }
}

}  // namespace

int count_newlines_per_stripe(const uint8_t *bytes, size_t nbytes, uint32_t stripe, uint32_t *counts, size_t nstripes, uint32_t *flags,
                              void *stream) {
    if (!nstripes) return 0;
    // (from 4 KiB stripes on: 8 GiB 1.63 ms against 1.8-1.95; at 1 KiB stripes the reduction per stripe makes it the slower
    // of the two, 2.4 ms against 1.7)
    if (stripe % 1024 == 0 && stripe >= 4096) {                      // a wave per stripe, the waves take stripe after stripe
        size_t blocks = (nstripes + 3) / 4;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(count_newlines_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bytes, nbytes, stripe, counts, nstripes, flags);
        return (int)hipGetLastError();
    }
    size_t blocks = (nstripes + 255) / 256;
    hipLaunchKernelGGL(count_newlines_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bytes, nbytes, stripe, counts, nstripes, flags);
    return (int)hipGetLastError();
}
int expand_bits(const uint32_t *bits, size_t nlines, uint8_t *out, void *stream) {
    if (!nlines) return 0;
    size_t words = (nlines + 31) / 32, blocks = (words + 255) / 256;
    hipLaunchKernelGGL(expand_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bits, nlines, out);
    return (int)hipGetLastError();
}
int scan_counts(const uint32_t *counts, uint64_t *base, uint64_t *chunk_sums, size_t n, void *stream) {
    const size_t nchunks = (n + kScanChunk - 1) / kScanChunk;
    hipStream_t st = (hipStream_t)stream;
    if (nchunks) hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, counts, n, chunk_sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, chunk_sums, nchunks, base + n);
    if (nchunks) hipLaunchKernelGGL(scan_chunks_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, counts, n, chunk_sums, base);
    return (int)hipGetLastError();
}
size_t scan_scratch_words(size_t n) { return (n + kScanChunk - 1) / kScanChunk + 1; }
// popcount of the first `nlines` bits of a result bitmap (bits of the last word beyond them ignored), added to *count, which the
// caller has zeroed on the same stream: a sum per lane, per wave (DPP/shuffle reduction), one atomic per wave
__global__ __launch_bounds__(256) void bitmap_count_kernel(const uint32_t *__restrict__ bits, size_t nlines, unsigned long long *__restrict__ count) {
    const size_t words = (nlines + 31) / 32;
    const uint32_t tail = (uint32_t)(nlines & 31u);
    unsigned long long n = 0;
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
        uint32_t v = bits[w];
        if (w + 1 == words && tail) v &= (1u << tail) - 1u;
        n += (uint32_t)__popc(v);
    }
    for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, n);
}
int bitmap_count(const uint32_t *bits, size_t nlines, unsigned long long *count, void *stream) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof *count, (hipStream_t)stream);
    if (e != hipSuccess || !nlines) return (int)e;
    size_t blocks = ((nlines + 31) / 32 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(bitmap_count_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bits, nlines, count);
    return (int)hipGetLastError();
}
int mail_results(const uint64_t *total, const uint32_t *flags, const uint8_t *last_byte, uint64_t *mail, void *stream, const uint32_t *own) {
    hipLaunchKernelGGL(mail_results_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, total, flags, last_byte, mail, own);
    return (int)hipGetLastError();
}
int own_words_check(const uint64_t *stripe_base, size_t nstripes, const uint8_t *last_byte, uint32_t *own, void *stream) {
    const size_t nworkgroups = (nstripes + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(own_words_kernel, dim3((unsigned)((nworkgroups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stripe_base, nstripes, nworkgroups,
                       last_byte, own);
    return (int)hipGetLastError();
}
int build_line_offsets(const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes,
                       uint64_t *line_off, void *stream) {
    if (!nstripes) return 0;
    hipLaunchKernelGGL(line_offsets_kernel, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bytes, nbytes, stripe,
                       stripe_base, nstripes, line_off);
    return (int)hipGetLastError();
}
int empty_matches(const uint64_t *line_off, size_t nlines, uint32_t *count, const uint64_t *first, uint32_t *match_start, uint32_t *match_end,
                  void *stream, size_t cap) {
    if (!nlines) return 0;
    const dim3 grid((unsigned)((nlines + 255) / 256));
    if (first) hipLaunchKernelGGL(empty_matches_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, line_off, nlines, count, first, match_start, match_end, (uint64_t)cap);
    else hipLaunchKernelGGL(empty_matches_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, line_off, nlines, count, first, match_start, match_end, (uint64_t)cap);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
