/*
 * rrx.h — C ABI of the MI355X-native RoaringRegex hot path (librrx.so).
 *
 * The reference has no FFI; its only interface is the C++ iterator facade of src/inc/regex.h.  This ABI is
 * what a binding for that facade binds for the hot path: each entry point names the reference interface it
 * replaces (paths relative to the reference's src/).  include/rregex.hpp rebuilds the reference's C++ names
 * (Regex::RRegex, get_acceptance_iter, IteratorWrapper, Match) on top of it; INTEGRATION.md shows the
 * reference-side stub.
 *
 * Conventions: plain pointers and sizes only; no exception crosses the boundary — every function returns
 * RRX_OK or an error code and rrx_last_error() describes the last failure on the calling thread
 * (the reference throws std::runtime_error, Parser.cpp:36,155).  "d_" parameters are DEVICE pointers
 * (hipMalloc'ed on `device`); `stream` is a hipStream_t (NULL = default stream); launches are asynchronous
 * on that stream.  There is no CPU matcher behind this ABI: matching requires a gfx950 device.
 */
#ifndef RRX_H
#define RRX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rrx_regex rrx_regex;    /* a compiled pattern: replaces Regex::RRegex, regex.h:212-228        */
typedef struct rrx_corpus rrx_corpus;  /* a device-resident batch of '\n'-delimited strings + its line index */

enum { RRX_OK = 0, RRX_ERR_PATTERN = 1, RRX_ERR_ARG = 2, RRX_ERR_HIP = 3, RRX_ERR_UNSUPPORTED = 4 };

/* engine selection for rrx_compile_ex */
enum { RRX_ENGINE_AUTO = 0, RRX_ENGINE_NFA = 1, RRX_ENGINE_DFA = 2, RRX_ENGINE_DFA_GLOBAL = 3 /* table kept in HBM/L2 */,
       RRX_ENGINE_NFA_WAVE = 4 /* state set spread over 8, 16 or 32 lanes of a wave, 2-8 words per lane: up to 8192 positions */,
       RRX_ENGINE_DFA2 = 5 /* table with one dependent lookup per two bytes (AUTO prefers it when it fits) */,
       RRX_ENGINE_NFA_BLOCK = 8 /* wave-resident NFA: one wave holds one state set of up to 65536 positions (32 words per lane),
                                   exception edges as sparse lists (the reference's Roaring class, Parser.cpp:165, at any
                                   size); dense: a byte costs the whole set */,
       RRX_ENGINE_NFA_SPARSE = 10 /* the same with the set kept as a LIST OF ITS NON-EMPTY BLOCKS of 2048 positions (a bit mask):
                                   a byte costs the live blocks only (README.md:18-21: sets are sparse) - three times a dense
                                   word per live block, so for texts on which few blocks are live; never chosen by AUTO */ };

/* ---- compile: RRegex::RRegex(const char*), Parser.cpp:161-170 (host only, no device needed) ---------- */
int rrx_compile(const char *pattern, rrx_regex **out);
int rrx_compile_ex(const char *pattern, int engine, rrx_regex **out);
void rrx_free(rrx_regex *re);
const char *rrx_last_error(void);

/* ---- what the reference would have built (for parity checks on the construction) -------------------- */
uint32_t rrx_num_states(const rrx_regex *re);      /* states_n, Parser.cpp:163                               */
int      rrx_set_class(const rrx_regex *re);       /* 1,2,4 = BitSet<W>, 0 = Roaring: Parser.cpp:165-168     */
uint32_t rrx_ref_initial(const rrx_regex *re);     /* initial_state, regex.h:81                              */
int      rrx_ref_is_final(const rrx_regex *re, uint32_t state);                 /* final_states, regex.h:177 */
/* forward row T[idx(state,c,true)] (NFA.cc:9-12) as ascending state numbers; returns its cardinality */
uint32_t rrx_ref_row(const rrx_regex *re, uint32_t state, unsigned c, uint32_t *out, uint32_t cap);

/* ---- what the device runs ---------------------------------------------------------------------------- */
int         rrx_engine(const rrx_regex *re);       /* RRX_ENGINE_NFA or RRX_ENGINE_DFA                       */
const char *rrx_engine_name(const rrx_regex *re);
uint32_t    rrx_useful_states(const rrx_regex *re);
uint32_t    rrx_byte_classes(const rrx_regex *re);
/* 1 if the stride-2 table of this regex is laid out in a PROFILED order, 2 while the search for one is running, else 0.  At a
 * regex' first rrx_match_corpus against a corpus of 64 MiB or more a background thread (tens of ms of host work, once per
 * regex; tables small enough to be replicated are left alone) orders the rows and columns of the table by a 64 KiB sample of
 * that corpus' text so that fewer of a half-wave's lookups fall into one LDS bank, uploads the table again in that order
 * (its own hipMalloc + copies, no lock held) and swaps the descriptors in under the regex' mutex, which launches take for the
 * length of a copy: launches before the swap run on the table as numbered.  rrx_set_option can forbid it.  *before / *after: the mean
 * number of distinct entries in the fullest bank per half-wave on that sample (either may be NULL).  Results never depend
 * on the order.                                                                                                        */
int         rrx_table_order(const rrx_regex *re, double *conflict_before, double *conflict_after);
/* The same ordering from a text sample the CALLER provides (host memory), before the regex' first match: `lanes` (a multiple of
 * 32) pieces of `bytes_per_lane` bytes each, lane-major - 32 consecutive pieces are stepped in lockstep the way a half-wave
 * steps 32 neighbouring stripes, so take them from 32 places of the text a stripe (some KiB) apart.  Host only.              */
int         rrx_order_table(rrx_regex *re, const void *sample, uint32_t lanes, uint32_t bytes_per_lane);
/* Per-regex options.  RRX_OPT_BACKGROUND_ORDER (default 1): 0 forbids the library to start a thread of its own and to
 * allocate device memory behind the caller's back for the profiled table order above - the table then stays as numbered
 * unless the caller orders it himself with rrx_order_table (which runs in the calling thread).  Set it before the regex'
 * first rrx_match_corpus; a search that is already running is not stopped.  RRX_ERR_ARG for an unknown option.          */
/* RRX_OPT_FLUSH_SLOTS (default 0 = automatic): the stride-2 batch kernel lets all lanes flush their result bits together every
 * `value` slots (16 bytes of a lane's text; 1, 2, 4, 8, 16 or 32); automatic: from the corpus' mean line length, about eight
 * line ends per period.  A tuning knob: results never depend on it.  A period of 32 - the automatic choice from 33 bytes per
 * line on - runs the kernel that has it compiled in, every other one the kernel that takes it per launch
 * (rrx_match_flush_slots tells which).                                                                                    */
/* RRX_OPT_SAMPLED_TABLE (default 1): 0 keeps an automaton whose subset construction explodes on the NFA lane engine for every
 * launch (see rrx_learn_table).                                                                                          */
/* RRX_OPT_UNITS_PER_WORKGROUP: ACCEPTED AND IGNORED.  It chose a kernel that handed its stripes out in units of 64 inside the
 * workgroup; that kernel was no faster on any config (profiles/r04_unit_handout_ab.txt) and is gone.  The value is still
 * checked (0 ... 65536, RRX_ERR_ARG otherwise) so that callers written for it keep working; it changes nothing.          */
/* RRX_OPT_SEARCH_ANCHORED (default 1): the search kernels' forward table is the product of "any bytes, then the pattern" with
 * the pattern's own table, which tells the matches that start at the line start (no walk back to find the start); 0 builds the
 * forward table alone - fewer rows, every match start walked back to - which is also what a product beyond 65534 rows falls
 * back to.  Same results.  Set it before the regex' first search (RRX_ERR_ARG afterwards).                                  */
/* RRX_OPT_ITEMS_STRIDE2 (default 1): large batches of explicit items with a separator byte each (rrx_match_extents /
 * rrx_match_items, trim 1) are stepped two bytes per lookup by a stride-2 table of their own - every byte value an ordinary
 * symbol, '\n' too, the separator a 129th - where the regex has a stride-2 table; 0 keeps them on the byte-stride items kernel
 * (which serves trim 0 either way).  Same results.                                                                         */
/* RRX_OPT_CONTAINS_NFA (default 0): which engine rrx_contains_corpus, rrx_contains_extents and rrx_contains_items run on.
 * 0: the contains table alone - a pattern without one, (a|b)*a(a|b){40}, is RRX_ERR_UNSUPPORTED.  1: where the regex has no contains
 * table (its forward search automaton does not determinise within the state budget, or the table passes 2^24 entries) the three
 * entries run on the shift-and NFA lane engine, the engine of rrx_match_corpus for such patterns, on a program of its own
 * (RRX_PROGRAM_CONTAINS_NFA), built at the first use whatever engine the regex was compiled for; this needs a lane program of at
 * most 16 words (512 positions after reduction) - beyond that RRX_ERR_UNSUPPORTED stays, its text naming both reasons.  2: the NFA
 * lane engine always, also where a table exists (tests, A/B measurements).  Same results on every route, exactly those written at
 * the three entries.  The NFA route is bound by the VALU and in another speed class than the tables, which is why a caller opts in.
 * On it rrx_contains_corpus is one hipMemsetAsync and one kernel (it can be captured into a graph once the program is uploaded:
 * after a first call), the items entries are a lane per item at every size - no extent bound, nothing read back, no scratch, no
 * event -, and a pattern that accepts the empty string or has an empty language is answered with a fill, no kernel.
 * rrx_contains_engine_name then says "nfa-shift-and"; rrx_contains_states keeps reporting the table's states (0: none).  May be set
 * at any time; any other value: RRX_ERR_ARG.                                                                                  */
enum { RRX_OPT_BACKGROUND_ORDER = 1, RRX_OPT_UNITS_PER_WORKGROUP = 2, RRX_OPT_SAMPLED_TABLE = 3, RRX_OPT_FLUSH_SLOTS = 4, RRX_OPT_SEARCH_ANCHORED = 5,
       RRX_OPT_ITEMS_STRIDE2 = 6, RRX_OPT_CONTAINS_NFA = 7 };
int         rrx_set_option(rrx_regex *re, int option, int64_t value);
/* The SAMPLED TABLE (an automaton that does not determinise - AUTO leaves it on the NFA lane engine - over text whose live sets
 * are few, README.md:18-21): the state sets a text sample reaches are interned into a table, every transition the sample and a
 * bounded closure leave open leads to an ESCAPE state.  rrx_match_corpus then runs the stride-2 table kernel (two result bits
 * per line: accepted, escaped) and lets the NFA engine decide the escaped lines: the result is exact for ANY text, text that
 * resembles the sample runs at table speed.  Built once per regex: by the first rrx_match_corpus against a corpus of 64 MiB or
 * more, from the corpus' own sample, in a background thread (RRX_OPT_BACKGROUND_ORDER 0: in the caller's) - or here, from `text`
 * (host memory, whole lines; the first line fragment is skipped), in the caller's thread.  The table gets the largest state budget
 * of 2048, 1024, ... 64 at which its stride-2 form fits the device.  A table that more than 2 % of its OWN
 * sample's lines leave is not installed (every escaped line is read twice: text whose live sets are not few - random a/b lines
 * under (a|b)*a(a|b){40} - stays on the NFA engine at its full rate).  RRX_ERR_UNSUPPORTED: the regex is not on the NFA lane
 * engine by AUTO's choice, no table fits, or the sample escapes from it.  rrx_sampled_table: 1 = in use, 2 = being built, 0 = none,
 * 3 = RETIRED: a launch of at least 1024 lines saw more than 5 % of them escape (every launch leaves its count in pinned host
 * memory, the next one looks at it without waiting) - the regex is back on the NFA engine, and the first launch against a corpus of 64 MiB
 * or more after that LEARNS THE TABLE AGAIN from that corpus' sample (as the first build: beside the caller, or in the launch
 * itself with RRX_OPT_BACKGROUND_ORDER 0; at most three times per regex; a new table is under the same two rules; state 1 again
 * when it is in); *table_states, *open_transitions (entries that lead to ESCAPE) describe the table.  Host only.             */
int         rrx_learn_table(rrx_regex *re, const void *text, size_t nbytes);
int         rrx_sampled_table(const rrx_regex *re, uint32_t *table_states, uint32_t *open_transitions);
/* *lines = the number of lines the NFA engine had to decide in the regex' LAST sampled-table launch on `device` (synchronous:
 * waits for the device).  A table whose escapes stay above a few per cent of the lines was learnt from the wrong text.      */
int         rrx_sampled_escapes(const rrx_regex *re, int device, uint64_t *lines);
uint32_t    rrx_words_per_set(const rrx_regex *re); /* 32-bit words of the register-resident state set (NFA) */
int         rrx_accepts_empty(const rrx_regex *re); /* Processor::operator*() on the initial set, NFA.cc:103-107 */
/* Serialised device program as 32-bit words (layout: DESIGN.md "Device programs"); returns the word count
 * (call with cap = 0 to size the buffer).  kind = RRX_ENGINE_NFA / _DFA / _NFA_WAVE / _DFA2 / _NFA_BLOCK (NFA layout with
 * the exception rows replaced by the CSR arrays xoff[nbits+1], xtgt[]), or one of the two search tables below (DFA
 * layout); 0 if that form was not built.                                                                      */
#define RRX_PROGRAM_SEARCH_FWD 6   /* "any bytes, then the pattern": accepting where a match ends              */
#define RRX_PROGRAM_SEARCH_REV 7   /* the pattern right to left: accepting where a match starts                */
#define RRX_PROGRAM_DFA2_ORDER 11  /* [nstates, ncols, row_slot[nstates], col_slot[ncols]]: the stride-2 table's profiled order
                                      (0 words while the table is laid out as numbered)                                  */
#define RRX_PROGRAM_SEARCH_LINE 9  /* the forward table as the stripe-wise search kernel runs it: [nrows, ncols, start row,
                                      SKIP row, column of byte[256], entry[nrows][ncols]], entry = next row | '\n' << 16 |
                                      hit << 17 | match-starts-at-the-line-start << 18 (0 words: form not available)   */
#define RRX_PROGRAM_SEARCH_LINE2 14 /* its stride-2 form, what the kernel steps (two bytes per dependent lookup): [nrows, ncols, start row,
                                      SKIP row, layout (1: LDS, 2: HBM/L2, 0: the stripe-wise kernel is not used), column of the byte
                                      pair[128][128], first[nrows][ncols], all[nrows][ncols]], entry = next row | events << 24, events =
                                      flags of the first byte << 2 | of the second; flags 1 '\n', 2 hit, 3 hit that starts at the restart
                                      point; first: a hit leads to SKIP, all: back to the start row                         */
#define RRX_PROGRAM_SAMPLED_DFA 12  /* the sampled table (rrx_learn_table): the DFA layout, then escaped[nstates] (1: the ESCAPE state) */
#define RRX_PROGRAM_SAMPLED_DFA2 13 /* its stride-2 form as the kernel runs it: the DFA2 layout, byte 2 of an entry = RESULT BITS shifted
                                       in (two per line end: accepted, escaped), byte 3 = those bits                          */
#define RRX_PROGRAM_DFA2_ITEMS 15 /* the stride-2 table of explicit items with a separator each (rrx_match_extents / rrx_match_items, trim 1):
                                    [nstates, ncols, start, accepts_empty, 129, column of the code pair[129][129], next2[nstates][ncols]] - codes
                                    0 ... 127 the byte values ('\n' an ordinary byte), 128 END OF ITEM; entries as in the DFA2 layout.  0 words
                                    where the regex has no stride-2 table or this form does not fit beside the pair table              */
#define RRX_PROGRAM_CONTAINS_DFA 16  /* the contains table (rrx_contains_corpus), DFA layout: state 0 = SKIP, class 0 a live column   */
#define RRX_PROGRAM_CONTAINS_DFA2 17 /* its stride-2 form, DFA2 layout; 0 words where it does not fit                                */
#define RRX_PROGRAM_CONTAINS_DFA2_ITEMS 18 /* the contains table's stride-2 ITEMS form (rrx_contains_extents / rrx_contains_items, trim 1), in exactly
                                    the RRX_PROGRAM_DFA2_ITEMS layout; 0 words where the contains table has no stride-2 form (RRX_ENGINE_DFA /
                                    _DFA_GLOBAL too) or the items form does not fit.  (The byte-stride forms step RRX_PROGRAM_CONTAINS_DFA.)   */
#define RRX_PROGRAM_SEARCH_STARTS 19   /* leftmost-longest search (rrx_search_longest_extents): "any bytes, then the pattern right to left",
                                         DFA layout - stepped from an item's last byte down, accepting where a match starts; no dead row  */
#define RRX_PROGRAM_SEARCH_ANCHORED 20 /* ... and the pattern's own DFA, DFA layout: state 0 dead and absorbing, class 0 leads there - stepped
                                         forwards from a match start, accepting where a match from there ends.  Both: 0 words where one
                                         of the two does not determinise within the state budget                                          */
#define RRX_PROGRAM_CONTAINS_NFA 25    /* the program of contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA; dumped whatever the option says),
                                         RRX_ENGINE_NFA layout, with the B rows as its kernels see them: position 0 (bit 0 of word 0) in every
                                         row, the rows of 0x00 and 0x80 ... 0xFF exactly {position 0}, the '\n' row the pattern's own plus
                                         position 0 (the items kernel steps it; the corpus kernel puts {position 0} in its place).  0 words
                                         where the pattern has no lane program of at most 16 words                                       */
size_t rrx_program_words(const rrx_regex *re, int kind, uint32_t *out, size_t cap);

/* ---- batch of strings: the replacement for calling get_acceptance_iter(line)++ per string ------------ *
 * regex.h:225-227 + 156-162, for every '\n'-delimited string of a device-resident buffer.  A final fragment
 * without '\n' is a string too.  Bytes 0x00 and >= 0x80 reject their string (the reference cannot express
 * the former and has undefined behaviour on the latter, NFA.cc:10,97).                                       */
int    rrx_corpus_create(int device, const void *d_bytes, size_t nbytes, void *stream, rrx_corpus **out);
/* same with an explicit stripe (bytes per GPU lane: a power of two in [512, 16384]; 0 = chosen from nbytes and the mean line length:
 * 512 bytes up to 128 MiB - a lane steps its stripe as one chain of dependent lookups, short stripes are what makes a small corpus
 * fast -, 2 KiB at 1 GiB, 4 KiB at 8 GiB, longer for long lines) */
int    rrx_corpus_create_ex(int device, const void *d_bytes, size_t nbytes, uint32_t stripe_bytes, void *stream,
                            rrx_corpus **out);
uint32_t rrx_corpus_stripe_bytes(const rrx_corpus *c);
size_t rrx_corpus_num_lines(const rrx_corpus *c);
size_t rrx_corpus_num_bytes(const rrx_corpus *c);
void   rrx_corpus_free(rrx_corpus *c);
size_t rrx_corpus_bitmap_words(const rrx_corpus *c);   /* 32-bit words of the accept bitmap: ceil(lines / 32) */
/* 1: the stride-2 table kernel can run on this corpus as ONE launch, without the clear of the bitmap in front of it - every
 * workgroup stores the bitmap words it alone writes, and a word it shares with its neighbour is settled through an exchange slot
 * (DESIGN.md 6.1).  0: some bitmap word lies in the line ranges of three workgroups (lines longer than a workgroup's text:
 * 1024 stripes) - every launch clears the bitmap and merges with atomics, as every other engine does.  Decided once, with the
 * index.  *span_words (may be NULL): the longest run of bitmap words of one workgroup behind its first; a regex whose table
 * leaves a shorter result window in LDS (1024 ... 11776 words, by the size of its table) takes the clear on this corpus too,
 * and so does a launch on a stream that is being captured.  Read-only.                                                     */
int    rrx_corpus_one_launch(const rrx_corpus *c, uint32_t *span_words);
/* The common flush period, in slots, of the stride-2 table kernel for this regex on this corpus (RRX_OPT_FLUSH_SLOTS, or the
 * automatic choice); *compiled_in (may be NULL) = 1 if that is the kernel with the period compiled in.  Read-only.         */
uint32_t rrx_match_flush_slots(const rrx_regex *re, const rrx_corpus *c, int *compiled_in);
/* THE HOT PATH.  Writes the accept BITMAP: bit (i & 31) of d_accept_bits[i >> 5] = 1 iff string i is accepted
 * (i.e. *it has a value, regex.h:160-162; its Match is then [start of string i, its terminator)).
 * d_accept_bits holds rrx_corpus_bitmap_words() words; every one of them is written on `stream`, whatever it held.  */
int rrx_match_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_accept_bits, void *stream);
/* The same for a device-resident buffer that has no rrx_corpus yet, in ONE call: with the lane engines (tables, NFA) the
 * text is read once (the newline index is a by-product of the match: per-stripe counts, a scan, a compaction of the
 * lanes' verdict streams); the cooperative engines build the index first.  d_accept_bits holds cap_words words (zeroed and
 * filled on `stream`); *nlines = number of strings; RRX_ERR_ARG if the bitmap is too small.  Synchronous (the line count
 * comes back through pinned memory: one wait, no copies).  The regex handle keeps the scratch of its largest call until
 * rrx_free: 12 bytes per stripe + the lanes' verdict streams, worst case 1 bit per byte of text (one line per byte).   */
int rrx_match_device(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint32_t *d_accept_bits,
                     size_t cap_words, size_t *nlines, void *stream);
/* One byte per string (0/1) from the bitmap; d_accept holds nlines bytes, 16-byte aligned.                  */
int rrx_bitmap_to_bytes(int device, const uint32_t *d_accept_bits, size_t nlines, uint8_t *d_accept, void *stream);

/* Search (the reference's README promises match iterators, its code has acceptance only: SURVEY.md 8(f).1).  For
 * string i of the corpus: the substring [d_start[i], d_end[i]) (offsets relative to the start of the string) that the
 * pattern accepts as a whole string (regex.h:156-162) with the smallest end, and among those the smallest start;
 * 0xFFFFFFFF in both when no substring is accepted.  Bytes the pattern cannot match (including NUL and >= 0x80) are
 * ordinary text here.  One kernel (kernels_search.hip) for every pattern: its forward table in LDS when it fits, in HBM/L2
 * otherwise; RRX_ERR_UNSUPPORTED only when the REVERSE table does not fit 64 KiB of LDS, the forward table has more than 65534
 * rows, or its stride-2 form more than 256 MiB.  A pattern that accepts the empty string matches [0, 0) in every string.  */
int rrx_search_corpus(const rrx_regex *re, const rrx_corpus *corpus, uint32_t *d_start, uint32_t *d_end, void *stream);
/* WHICH strings contain a match (what grep answers; the reference has acceptance only).  Replaces rrx_search_corpus + a test of
 * d_start[i] != 0xFFFFFFFF, which pays for match starts nobody asked for, and rrx_match_corpus on ".*(p).*", which rejects every
 * string that holds a NUL or a byte >= 0x80.  Bit (i & 31) of d_bits[i >> 5] = 1 iff rrx_search_corpus would report a match for
 * string i, i.e. iff some substring of it is accepted by the pattern as a whole string.  NUL and bytes >= 0x80 are ordinary text
 * that no pattern takes; a pattern that accepts the empty string is contained in every string, the empty one included; an
 * empty-language pattern in none.  d_bits holds rrx_corpus_bitmap_words() words, zeroed and filled on `stream`, asynchronously
 * (an empty corpus writes nothing).  Runs the batch kernels of rrx_match_corpus on a table of its own, built at the first use:
 * the forward search table with every accepting state folded into one absorbing state, minimised - never more states than
 * RRX_PROGRAM_SEARCH_FWD has.  Forms and fit rules as the match path's (stride-2 table, wide / classed LDS table, table in
 * HBM/L2; a regex compiled with RRX_ENGINE_DFA / RRX_ENGINE_DFA_GLOBAL stays on the byte-stride LDS / global table); text with
 * bytes >= 0x80 keeps the stride-2 kernel.  RRX_ERR_UNSUPPORTED where the forward search automaton does not determinise within
 * the state budget or the table passes 2^24 entries.                                                                        */
int         rrx_contains_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_bits, void *stream);
const char *rrx_contains_engine_name(const rrx_regex *re);   /* "dfa-stride2-table", ... as rrx_engine_name; NULL + rrx_last_error() if unsupported; host only */
uint32_t    rrx_contains_states(const rrx_regex *re);        /* states of the contains table, SKIP included; 0 if unsupported; host only */
/* *d_count (a device word, zeroed and filled on `stream`) = set bits among the first nlines bits of a result bitmap - bits of the
 * last word beyond nlines are ignored, nlines 0 gives 0: `grep -c` on either bitmap without a host round trip.             */
int         rrx_bitmap_count(int device, const uint32_t *d_bits, size_t nlines, uint64_t *d_count, void *stream);
/* ALL lazy matches of every string, left to right (what the reference's CLI is documented to print, README.md:30): the
 * k-th match of a string is the search above applied to the rest of the string after the previous match (one byte
 * further after an empty match).  Two passes: _count writes d_count[i] = matches of string i; the caller turns the
 * counts into the exclusive prefix d_first[i] (u64); _fill writes the matches of string i to the slots d_first[i] ...   */
int rrx_search_all_count(const rrx_regex *re, const rrx_corpus *corpus, uint32_t *d_count, void *stream);
int rrx_search_all_fill(const rrx_regex *re, const rrx_corpus *corpus, const uint64_t *d_first, uint32_t *d_start,
                        uint32_t *d_end, void *stream);

/* The same in ONE call and one pass over the text: d_first[i] (u64, nlines + 1 entries, d_first[nlines] = *total) =
 * slot of the first match of string i, the matches of string i at d_start/d_end[d_first[i] .. d_first[i + 1]).  The
 * match arrays hold `cap` entries: matches beyond are counted, not written - if *total > cap call again with arrays of
 * *total entries (d_first is complete either way).  Synchronous (returns *total).  Calls on one corpus must not
 * overlap (they share the corpus' scratch).                                                                        */
int rrx_search_all(const rrx_regex *re, const rrx_corpus *corpus, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end,
                   size_t cap, size_t *total, void *stream);

/* explicit extents: item i = d_bytes[d_off[i] .. d_off[i+1] - trim); '\n' is an ordinary character here.  Asynchronous on
 * `stream`.  Large batches on a table engine (>= 65536 items) build an item index in a scratch buffer the regex handle keeps
 * until rrx_free (1 bit per byte + 8 bytes per stripe of the batch's extent).  The host does not know the extent; it takes
 * what is left of the allocation behind d_bytes (hipMemGetAddressRange) as its bound and nothing is read back - as long as
 * that bound is plausible for the batch, at most max(128 bytes per item, 16 MiB).  A batch inside a far larger allocation (a
 * memory pool, a caching allocator's block) and memory whose range the runtime does not report (pool, virtual or managed
 * memory) cost one synchronisation on `stream`: d_off[0] and d_off[nitems] are read back.  Calls with one regex on
 * different streams are ordered on the device by an event, not on the host.                                               */
int rrx_match_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems,
                      uint32_t trim, uint8_t *d_accept, void *stream);

/* A batch of items indexed ONCE and matched by many patterns (what rrx_corpus is for delimited text): the item-end
 * bitmap and the stripe index of section DESIGN.md 6.5 are built here (synchronous) and kept.  rrx_match_items fills
 * d_accept[i] (one byte per item, 16-byte aligned for the fast path) on `stream`; batches or patterns that do not admit the
 * stripe-wise kernel run as rrx_match_extents.  d_bytes and d_off must outlive the handle.  One match at a time per
 * handle (it owns the result scratch).                                                                              */
typedef struct rrx_items rrx_items;
int rrx_items_create(int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, void *stream,
                     rrx_items **out);
size_t rrx_items_count(const rrx_items *items);
int rrx_items_stripe_wise(const rrx_items *items);         /* 1: the batch admits the stripe-wise kernel */
void rrx_items_free(rrx_items *items);
int rrx_match_items(const rrx_regex *re, const rrx_items *items, uint8_t *d_accept, void *stream);

/* WHICH items contain a match: rrx_contains_corpus for explicit items (an offsets array over one byte buffer - an Arrow string
 * column), where ".*(p).*" through rrx_match_items rejects every item that holds a NUL or a UTF-8 byte and re-packing the column
 * as '\n'-delimited text is wrong as soon as an item holds a '\n'.  Item i is d_bytes[d_off[i] .. d_off[i+1] - trim), as in
 * rrx_match_extents.  Bit (i & 31) of d_bits[i >> 5] = 1 iff some substring of item i, the empty one included, is accepted by the
 * pattern as a whole string (regex.h:156-162).  '\n' is an ordinary byte and may be part of a match; NUL and bytes >= 0x80 are
 * ordinary text that no pattern takes; a pattern that accepts the empty string is contained in every item, an empty item
 * included; an empty-language pattern in none.  d_bits holds ceil(nitems / 32) 32-bit words (4-byte aligned), zeroed and filled on
 * `stream`, the bits of the last word beyond nitems 0 - the shape of rrx_contains_corpus' result (and of an Arrow boolean column):
 * rrx_bitmap_count and rrx_bitmap_to_bytes apply.  nitems == 0 writes nothing and returns RRX_OK.  RRX_ERR_UNSUPPORTED exactly
 * where rrx_contains_corpus returns it (no contains table within the state budget, or one beyond 2^24 entries); whether the regex'
 * MATCH engine is a table engine plays no part.  Both calls are asynchronous on `stream` - except where rrx_match_extents
 * synchronises too: a large batch inside an implausibly large allocation, or in memory whose range is not reported, has d_off[0]
 * and d_off[nitems] read back, by the same bound rule.  Large batches (>= 65536 items, >= 8 MiB; every indexed batch that admits
 * it) run the stripe-wise items kernels on the contains table's items forms - byte-stride up to about 126 states, stride-2 for
 * trim 1 (RRX_OPT_ITEMS_STRIDE2; not for a regex compiled with RRX_ENGINE_DFA / RRX_ENGINE_DFA_GLOBAL) -, all others a lane per
 * item, which stops reading an item at its first match.  Scratch and stream ordering as rrx_match_extents / rrx_match_items.    */
int rrx_contains_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                         uint32_t *d_bits, void *stream);
int rrx_contains_items(const rrx_regex *re, const rrx_items *items, uint32_t *d_bits, void *stream);

/* WHERE the first match of every item is: rrx_search_corpus for explicit items (what regexp_extract, find and substring need of a
 * string column; re-packing the column as '\n'-delimited text is wrong as soon as an item holds a '\n', and costs a copy and an
 * index pass).  Item i is d_bytes[d_off[i] .. d_off[i+1] - trim), as in rrx_contains_extents; a trim larger than the item's
 * length leaves the empty item.  [d_start[i], d_end[i]) - offsets relative to the start of item i - is the substring of item i
 * that the pattern accepts as a whole string (regex.h:156-162) with the smallest end, and among those the smallest start;
 * 0xFFFFFFFF in both when no substring is accepted.  '\n' is an ordinary byte and may be part of a match; NUL and bytes >= 0x80
 * are ordinary text that no pattern takes.  A pattern that accepts the empty string gives [0, 0) for every item, an empty item
 * included (two fills, no table, no kernel); an empty-language pattern 0xFFFFFFFF everywhere.  d_start and d_end hold nitems
 * words each; every one of them is written on `stream`, whatever it held.  nitems == 0 writes nothing and returns RRX_OK - a
 * regex without search tables is still reported.  Both calls are FULLY asynchronous on `stream` and can be captured into a graph:
 * a lane per item on the two plain search tables (RRX_PROGRAM_SEARCH_FWD to the first accepting position, RRX_PROGRAM_SEARCH_REV
 * back from there to the last accepting one), the kernel reads the offsets itself - no extent bound, no read-back, no scratch, no
 * event, unlike rrx_match_extents; rrx_search_items uses the handle's bytes, offsets, item count, trim and device only (not its
 * index).  Both tables sit in LDS when together they fit 64 KiB, else - and for a regex compiled with RRX_ENGINE_DFA_GLOBAL - in
 * HBM/L2.  RRX_ERR_ARG for null arguments (checked before any device call); RRX_ERR_UNSUPPORTED only where the forward or the
 * reverse search automaton does not determinise within the state budget (16384 states) - the fit rules of rrx_search_corpus'
 * kernel play no part.  LONG ITEMS: offsets are 32-bit - only matches that end at or before offset 0xFFFFFFFE of their item are
 * reported, the forward pass stops there.  This is NOT what a regex user calls the first match - [0-9]+ on "abc 12345 x" answers
 * [4, 5), "1": rrx_search_longest_extents / rrx_search_longest_items below give the leftmost-longest match, [4, 9).              */
int rrx_search_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                       uint32_t *d_start, uint32_t *d_end, void *stream);
int rrx_search_items(const rrx_regex *re, const rrx_items *items, uint32_t *d_start, uint32_t *d_end, void *stream);

/* The LEFTMOST-LONGEST match of every item: what regexp_extract, find and substring mean in every SQL engine, in POSIX and in RE2's
 * longest-match mode.  Item i is d_bytes[d_off[i] .. d_off[i+1] - trim); a trim larger than the item's length leaves the empty
 * item.  d_start[i] is the smallest s such that some item[s, e) is accepted by the pattern as a whole string (regex.h:156-162);
 * d_end[i] is the largest e such that item[d_start[i], e) is accepted; offsets relative to the start of item i.  No match gives
 * 0xFFFFFFFF in both.  '\n' is an ordinary byte and may be part of a match; NUL and bytes >= 0x80 are ordinary text that no pattern
 * takes.  A pattern that accepts the empty string has d_start[i] = 0 for every item; d_end[i] is the longest accepted prefix, 0 if
 * none other; an empty item gives [0, 0).  An empty-language pattern gives 0xFFFFFFFF everywhere (two fills, no table).  d_start and
 * d_end hold nitems words each; every one of the 2 x nitems words is written on `stream`, whatever it held.  nitems == 0 writes
 * nothing and returns RRX_OK - an unsupported regex is still reported.  Both calls are FULLY asynchronous on `stream` and can be
 * captured into a graph once the tables are uploaded (the first call on a device uploads them): no read-back, no scratch, no event,
 * no extent bound; rrx_search_longest_items uses the handle's bytes, offsets, item count, trim and device only (not its index).
 * A lane per item, two passes over two tables of their own (neither RRX_PROGRAM_SEARCH_FWD nor _REV is used): backwards on
 * RRX_PROGRAM_SEARCH_STARTS from the item's last byte to its first - that table has no dead row, so the WHOLE item is read, there is
 * no early exit -, then forwards on RRX_PROGRAM_SEARCH_ANCHORED from the start found to the item's end or the table's dead row.  A
 * pattern that accepts the empty string runs the second pass alone.  Both tables sit in LDS when together they fit 64 KiB, else -
 * and for a regex compiled with RRX_ENGINE_DFA_GLOBAL - in HBM/L2.  RRX_ERR_ARG for null arguments (checked before any device
 * call); RRX_ERR_UNSUPPORTED only where one of the two tables does not determinise within the state budget (16384 states), for an
 * empty batch too.  LONG ITEMS: offsets are 32-bit - an item longer than 0xFFFFFFFE bytes is searched as if it ended at its offset
 * 0xFFFFFFFE.                                                                                                                */
int rrx_search_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                               uint32_t *d_start, uint32_t *d_end, void *stream);
int rrx_search_longest_items(const rrx_regex *re, const rrx_items *items, uint32_t *d_start, uint32_t *d_end, void *stream);

/* The LEFTMOST-LONGEST match of every LINE of a '\n'-corpus: what grep -o prints first on each line.  ONE RULE: d_start and d_end hold
 * rrx_corpus_num_lines(c) words each, and words i are exactly what rrx_search_longest_extents writes for an item made of the bytes
 * of line i without its '\n'.  So: offsets are relative to the line's first byte and 0xFFFFFFFF in both words means no match;
 * leftmost beats longer; NUL and bytes >= 0x80 are text that no pattern takes; a final fragment without '\n' is a line; no match
 * spans a '\n' - the byte never reaches a table - and a pattern that holds '\n' matches only through its '\n'-free words; a pattern
 * that accepts the empty string gives d_start[i] = 0 and d_end[i] = the longest accepted prefix on every line, [0, 0) on an empty
 * one; an empty-language pattern gives 0xFFFFFFFF everywhere (two fills, no table, no pass over the text); a line longer than
 * 0xFFFFFFFE bytes is searched as if it ended at its offset 0xFFFFFFFE.  Every one of the 2 x lines words is written on `stream`,
 * whatever it held, and nothing behind them; a corpus of zero lines writes nothing and returns RRX_OK - an unsupported regex is
 * still reported.  A lane per stripe of the text on the corpus' own stripe index: no offsets array is built or used.  FULLY
 * asynchronous on `stream` and capturable into a graph once the tables are uploaded (the first call on a device uploads them): no
 * read-back, no scratch, no event.  Tables, their placement and RRX_ERR_UNSUPPORTED as for rrx_search_longest_extents; RRX_ERR_ARG
 * for a null re, c, d_start or d_end, before any device call.                                                                 */
int rrx_search_longest_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_start, uint32_t *d_end, void *stream);

/* EVERY match of every item, left to right: rrx_search_all* for explicit items (what regexp_count, regexp_extract_all,
 * regexp_replace and split need of a string column).  Item i is d_bytes[d_off[i] .. d_off[i+1] - trim), as in rrx_search_extents.
 * The matches of an item are those of rrx_search_extents applied repeatedly TO THE REST OF THE ITEM behind the previous match:
 * match k is the accepted substring of item[p_k:] with the smallest end, and among those the smallest start; p_0 = 0, p_{k+1} = the
 * end of match k, one byte further after an empty match; offsets are relative to the start of the item.  A match never starts
 * before the end of the previous one, even where a longer substring reaching back across it would be accepted ("ab|bab" on "abab":
 * [0,2) and [2,4), not [1,4)).  '\n' is an ordinary byte and may be part of a match; NUL and bytes >= 0x80 are ordinary text that
 * no pattern takes.  A pattern that accepts the empty string has the matches [k, k) for k = 0 ... length of the item - length + 1
 * of them, 1 for an empty item (no table, no text); an empty-language pattern has none.  LONG ITEMS as rrx_search_extents: only
 * matches that end at or before offset 0xFFFFFFFE of their item are found.
 * Two passes: _count writes d_count[i] = matches of item i - every one of the nitems words, whatever it held; the caller turns the
 * counts into the exclusive prefix d_first[i] (u64); _fill writes match k of item i to slot d_first[i] + k of d_start / d_end and no
 * other slot.  Both are FULLY asynchronous on `stream` and can be captured into a graph once the tables are uploaded: no read-back,
 * no scratch, no event, no extent bound.  A lane per item on the two plain search tables (kernels_search_all_items.hip), both in
 * LDS when together they fit 64 KiB, else - and for a regex compiled with RRX_ENGINE_DFA_GLOBAL - in HBM/L2; _count steps the
 * forward table alone and resets it at every match end, _fill walks back on the reverse table from every match end to the end of
 * the previous match.  A wave of 64 consecutive items takes as long as its longest item, and a lane's result stores are scattered.
 * The one-call form mirrors rrx_search_all: d_first has nitems + 1 entries, d_first[nitems] = *total; the match arrays hold `cap`
 * entries, matches in slots >= cap are counted, not written - if *total > cap call again with arrays of *total entries (d_first
 * is complete either way).  Synchronous (returns *total).  It is _count, a device scan and _fill, the counts and the scan's scratch
 * in device memory the call allocates and frees: calls share nothing and may overlap.  The scan carries 30 bits per count: an item
 * with 2^30 or more matches needs the two-pass form.  nitems == 0: d_first[0] = 0, *total = 0.
 * rrx_search_all_items* use the handle's bytes, offsets, item count, trim and device only (not its index).
 * RRX_ERR_ARG for null arguments, checked before any device call (d_start / d_end may be null where nothing can be written:
 * cap == 0 or nitems == 0); RRX_ERR_UNSUPPORTED exactly where rrx_search_extents returns it, for an empty batch too.          */
int rrx_search_all_extents_count(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                 uint32_t *d_count, void *stream);
int rrx_search_all_extents_fill(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream);
int rrx_search_all_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                           uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total, void *stream);
int rrx_search_all_items_count(const rrx_regex *re, const rrx_items *items, uint32_t *d_count, void *stream);
int rrx_search_all_items_fill(const rrx_regex *re, const rrx_items *items, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end,
                              void *stream);
int rrx_search_all_items(const rrx_regex *re, const rrx_items *items, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap,
                         size_t *total, void *stream);

/* EVERY LEFTMOST-LONGEST match of every item, left to right: what regexp_count, regexp_extract_all, regexp_replace and split mean
 * in every SQL engine, in POSIX and in RE2's longest-match mode ([0-9]+ on "a1 22 333": [1,2) [3,5) [6,9), where
 * rrx_search_all_extents reports six one-digit matches).  Item i is d_bytes[d_off[i] .. d_off[i+1] - trim), as in
 * rrx_search_longest_extents.  Match k of an item is the leftmost-longest match of item[p_k:] - the smallest start s >= p_k such
 * that some item[s, e) is accepted as a whole string, then the largest such e; p_0 = 0, p_{k+1} = the end of match k, one byte
 * further after an empty match; the search goes on while p_k <= length and stops at the first p_k without a match.  Offsets are
 * relative to the start of the item.  '\n', NUL and bytes >= 0x80 are ordinary text, as in rrx_search_longest_extents.  A pattern
 * that accepts the empty string matches at every position that no non-empty match covers: a* on "baab" gives [0,0) [1,3) [3,3)
 * [4,4) (Python's findall).  An empty-language pattern has no matches: the counts are 0 (a fill: no table, no text pass).  LONG
 * ITEMS: an item is searched as if it ended at its offset 0xFFFFFFFE.
 * Two phases per item, a lane per item (kernels_search_all_longest_items.hip) on the two tables of rrx_search_longest_extents,
 * placed as there: backwards on RRX_PROGRAM_SEARCH_STARTS over the WHOLE item, recording a MARK bit for every offset at which some
 * match starts; then forwards - the next mark at or behind p, RRX_PROGRAM_SEARCH_ANCHORED from there to the item's end or the
 * table's dead row, the last accepting position is the end, p = that end, and again.  The marks make this linear in the item.
 * The marks live in d_marks, a buffer of the caller's: rrx_search_all_longest_marks_words(extent_bytes, nitems) 32-bit words
 * (extent_bytes / 32 + nitems + 1) for any extent_bytes >= d_off[nitems] - d_off[0] - the size of the byte buffer will do.  Host
 * only, pure.  The bit of byte g of item i is bit (g - d_off[0]) & 31 of word ((g - d_off[0]) >> 5) + i: no two items share a word,
 * nothing has to be cleared, words outside the items' ranges are left as they were.
 * Two passes: _count writes the marks and d_count[i] = matches of item i - every one of the nitems count words, whatever it held;
 * the caller turns the counts into the exclusive prefix d_first[i] (u64); _fill, given the marks that _count left for the same
 * regex, batch and trim, writes match k of item i to slot d_first[i] + k of d_start / d_end - exactly the slots d_first[i] ..
 * d_first[i] + count[i] and nothing else.  Both are FULLY asynchronous on `stream` and can be captured into a graph once the
 * tables are uploaded: no read-back, no scratch of their own, no event, no extent bound.  _count reads an item about twice and
 * writes an eighth of it; _fill reads the marks and the matched bytes.  A d_marks shorter than
 * rrx_search_all_longest_marks_words(extent, nitems) is the caller's error, as a short d_start is; a marks_words below nitems + 1
 * is rejected (RRX_ERR_ARG: that bound needs no extent).  A pattern that accepts the empty string never touches d_marks.
 * KNOWN COST of such a pattern: the anchored walk restarts at every offset that no non-empty match covers, and each restart
 * runs to the dead row - (a*b)? on a long run of 'a' without a 'b' is quadratic in the run.
 * The one-call form mirrors rrx_search_all_extents: d_first has nitems + 1 entries, d_first[nitems] = *total; the match arrays
 * hold `cap` entries, matches in slots >= cap are counted, not written - if *total > cap call again with arrays of *total entries
 * (d_first is complete either way).  Synchronous (returns *total).  It reads d_off[0] and d_off[nitems] back to size the marks,
 * then runs _count, a device scan and _fill, the counts, the marks and the scan's scratch in device memory the call allocates and
 * frees.  The scan carries 30 bits per count.  nitems == 0: d_first[0] = 0, *total = 0.
 * rrx_search_all_longest_items* use the handle's bytes, offsets, item count, trim and device only (not its index).
 * RRX_ERR_ARG for null arguments, checked before any device call (d_marks is required when nitems > 0; d_start / d_end may be
 * null where nothing can be written: the one-call form with cap == 0 or nitems == 0); RRX_ERR_UNSUPPORTED exactly where
 * rrx_search_longest_extents returns it, for an empty batch too - nothing is written then.                                       */
size_t rrx_search_all_longest_marks_words(size_t extent_bytes, size_t nitems);
int rrx_search_all_longest_extents_count(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                         uint32_t *d_marks, size_t marks_words, uint32_t *d_count, void *stream);
int rrx_search_all_longest_extents_fill(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                        const uint32_t *d_marks, size_t marks_words, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end,
                                        void *stream);
int rrx_search_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                   uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total, void *stream);
int rrx_search_all_longest_items_count(const rrx_regex *re, const rrx_items *items, uint32_t *d_marks, size_t marks_words, uint32_t *d_count,
                                       void *stream);
int rrx_search_all_longest_items_fill(const rrx_regex *re, const rrx_items *items, const uint32_t *d_marks, size_t marks_words,
                                      const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream);
int rrx_search_all_longest_items(const rrx_regex *re, const rrx_items *items, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap,
                                 size_t *total, void *stream);

/* regexp_replace on a string column, WRITTEN on the device: from a column, a match list per item and a literal replacement to the
 * new column (d_out_off[nitems + 1], d_out).  Item i is t = d_bytes[d_off[i] .. d_off[i+1] - trim), empty where trim exceeds its
 * length.  Its matches (s_0,e_0) ... (s_{m-1},e_{m-1}) are in order, s_0 >= 0, e_k >= s_k, s_{k+1} >= e_k, e_{m-1} <= length; the
 * output item is t[0:s_0] + R + t[e_0:s_1] + R + ... + R + t[e_{m-1}:], R the replacement: rep_len >= 0 literal bytes (a
 * replacement with group references: rrx_replace_template_* / rrx_replace_groups_longest_* below).  An empty match inserts R at its position (a* on "baab" with "<>": "<>b<><>b<>"), an
 * item without matches is copied verbatim, the `trim` separator bytes are never copied: the output column has no separators.  This
 * is Python's re.sub(p, lambda m: R, t) for the list re.finditer names.
 * THE MATCH LIST is the shape every rrx_search_all* one-call form returns (and the two-pass forms once the caller's prefix has one
 * more entry): d_first has nitems + 1 entries, match k of item i is slot d_first[i] + k of d_start / d_end, offsets relative to the
 * item; d_pos[slot] belongs to the same slot (the arrays are indexed by the slot itself, d_first[0] need not be 0).  The two generic
 * entries take a list and no regex - they do not know where it came from: the lists of rrx_search_all_extents* (earliest end first)
 * work as well as the leftmost-longest ones.
 * rrx_replace_matches_sizes (pass 1, a lane per item walking its matches): d_len[i] = length of output item i - every one of the
 * nitems words, whatever it held; a length beyond 32 bits saturates at 0xFFFFFFFF - and d_pos[slot] = the offset inside the OUTPUT
 * item at which that match's R begins, s_k - sum_{j<k} (e_j - s_j) + k * rep_len (32 bits), for exactly the slots d_first[0] ..
 * d_first[nitems].  The caller turns d_len into the prefix d_out_off (u64, nitems + 1 entries); d_out_off[0] may be any value: a
 * running offset into a larger buffer.
 * rrx_replace_matches_fill (pass 2, the bytes): writes exactly d_out[d_out_off[0] .. d_out_off[nitems]) and, for every item, nothing
 * outside [d_out_off[i], d_out_off[i+1]) whatever the lists hold; it reads no input byte outside an item - a source offset at or
 * beyond the item's end yields a 0 byte.  d_rep is a DEVICE pointer (may be null when rep_len == 0); d_out may be null when nothing
 * can be written; d_bytes, d_rep and d_out may sit at any address.  The kernel is driven by OUTPUT bytes (kernels_replace_items.hip):
 * a wave takes 64 consecutive items and sweeps their output range 256 contiguous bytes per turn, whole dwords aligned by address;
 * per byte the item is found among the wave's 64 staged output offsets and the segment among the item's d_pos entries.  One long
 * item is one wave's work.
 * Both generic entries are FULLY asynchronous on `stream` and can be captured into a graph: no read-back, no scratch, no event, no
 * extent bound.  nitems == 0 writes nothing and returns RRX_OK.  RRX_ERR_ARG for null arguments, checked before any device call
 * (d_start / d_end / d_pos are required when nitems > 0 even where the lists are empty).
 * The one-call forms replace EVERY LEFTMOST-LONGEST match of `re` (rrx_search_all_longest_extents' list) and mirror that entry:
 * synchronous; everything temporary - marks, counts, the match arrays, d_pos, d_len, the scans' scratch, a copy of `rep`, which is
 * a HOST pointer here - lives in device memory the call allocates and frees.  d_out_off has nitems + 1 entries, d_out_off[0] = 0,
 * complete either way, *total = d_out_off[nitems]; d_out holds `cap` bytes: if *total > cap NO byte of d_out is written - call
 * again with *total bytes.  The scan carries 30 bits per count: a call that meets an item whose OUTPUT has 2^30 bytes or more
 * returns RRX_ERR_UNSUPPORTED instead of a wrong column (use the search entries and the two generic passes, with a prefix of the
 * caller's own).  An empty-language pattern copies the items; a pattern that accepts the empty string follows the rule above.
 * nitems == 0: d_out_off[0] = 0, *total = 0.  RRX_ERR_ARG for null arguments, checked before any device call (rep may be null when
 * rep_len == 0, d_out when cap == 0); RRX_ERR_UNSUPPORTED exactly where rrx_search_longest_extents returns it, for an empty batch
 * too.  rrx_replace_all_longest_items uses the handle's bytes, offsets, item count, trim and device only (not its index).
 * LONG ITEMS: matches end at or before offset 0xFFFFFFFE of their item, the rest of a longer item is copied verbatim (not tested:
 * no test of a few seconds reaches it); d_pos is 32-bit, so the generic passes need every R to begin below 2^32 in its output item. */
int rrx_replace_matches_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first, const uint32_t *d_start,
                              const uint32_t *d_end, uint32_t rep_len, uint32_t *d_len, uint32_t *d_pos, void *stream);
int rrx_replace_matches_fill(int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first,
                             const uint32_t *d_end, const uint32_t *d_pos, const void *d_rep, uint32_t rep_len, const uint64_t *d_out_off, void *d_out,
                             void *stream);
int rrx_replace_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                    const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out, size_t cap, size_t *total, void *stream);
int rrx_replace_all_longest_items(const rrx_regex *re, const rrx_items *items, const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out,
                                  size_t cap, size_t *total, void *stream);

/* regexp_extract_all and split on a string column, WRITTEN on the device as an Arrow list<binary> column: from a column and a match
 * list per item to the PIECES of every item.  Item i is t = d_bytes[d_off[i] .. d_off[i+1] - trim), L its length; its matches
 * (s_0,e_0) ... (s_{m-1},e_{m-1}) come in the shape rrx_replace_matches_sizes takes (d_first[nitems + 1], match k in slot
 * d_first[i] + k of d_start / d_end, d_first[0] need not be 0).  Two modes:
 *   RRX_PIECES_MATCHES (extract_all): m pieces, piece k = t[s_k:e_k];
 *   RRX_PIECES_GAPS (split): m + 1 pieces, piece k = t[e_{k-1}:s_k] with e_{-1} = 0 and s_m = L.
 * For a pattern without groups these are Python's [x.group() for x in re.finditer(p, t)] and re.split(p, t): [0-9]+ on "a1 22 333"
 * gives "1" "22" "333" and "a" " " " " ""; a* on "baab" gives "" "aa" "" "" and "" "b" "" "b" "".  The gaps joined are the item with
 * every match replaced by nothing.  CLAMPING: with a_0 = 0, for each k: s' = clamp(s_k, a_k, L), e' = clamp(e_k, s', L), the match
 * piece is [s', e'), the gap piece [a_k, s'), a_{k+1} = e'; the last gap is [a_m, L) - the identity for the list of a search, and no
 * list makes the kernels read outside the item.
 * THE COLUMN: d_list_off[nitems + 1] (u64) - the pieces of item i are d_list_off[i] .. d_list_off[i+1]: d_first[i] - d_first[0] for
 * MATCHES, d_first[i] - d_first[0] + i for GAPS; d_piece_off[npieces + 1] (u64) - the bytes of piece p are d_out[d_piece_off[p] ..
 * d_piece_off[p+1]); d_out - the pieces' bytes one behind the other, no separators.
 * rrx_pieces_sizes (pass 1, a lane per item walking its matches): d_list_off - all nitems + 1 words - and for every piece p
 * d_piece_len[p] (u32, saturated at 0xFFFFFFFF) and d_piece_src[p] (u64: d_off[i] + the piece's clamped start, an absolute offset
 * into d_bytes), exactly the slots 0 .. npieces - 1.  The caller turns d_piece_len into the prefix d_piece_off (npieces + 1 entries;
 * entry 0 may be any value: a running offset into a larger buffer).
 * rrx_pieces_fill (pass 2, the bytes): d_out[d_piece_off[p] + r] = d_bytes[d_piece_src[p] + r] for r < d_piece_off[p+1] -
 * d_piece_off[p]: exactly the bytes d_out[d_piece_off[0] .. d_piece_off[npieces]), each once; no byte of d_bytes outside a piece is
 * read.  It takes any ascending d_piece_off and any d_piece_src - it does not know where they came from (a first-match-only
 * regexp_extract column is rrx_search_longest_extents and this entry).  The kernel divides its work by OUTPUT BYTES alone
 * (kernels_pieces_items.hip): the waves of a fixed grid take chunks of 4 KiB of the output range, whole dwords aligned by address,
 * 256 contiguous bytes per wave instruction, the piece of a byte found by searches over d_piece_off - one piece of 64 MiB costs
 * every wave what 64 MiB of short pieces cost.  d_bytes and d_out may sit at any address and may be null where nothing can be read
 * or written.
 * Both generic entries are FULLY asynchronous on `stream` and can be captured into a graph: no read-back, no scratch, no event.
 * nitems == 0 / npieces == 0 write nothing and return RRX_OK.  RRX_ERR_ARG for null arguments and for a mode other than the two,
 * checked before any device call.
 * The one-call forms take EVERY LEFTMOST-LONGEST match of `re` (rrx_search_all_longest_extents' list) and mirror
 * rrx_replace_all_longest_extents: synchronous; everything temporary lives in device memory the call allocates and frees.
 * d_list_off has nitems + 1 entries, entry 0 = 0, complete either way; *npieces and *total (the bytes of all pieces) are exact
 * either way.  d_piece_off holds pieces_cap + 1 entries (entry 0 = 0) and is written iff *npieces <= pieces_cap; d_out holds `cap`
 * bytes and is written iff additionally *total <= cap - otherwise not a byte of it: call again with the exact sizes.  nitems == 0:
 * d_list_off[0] = 0, d_piece_off[0] = 0, both counts 0.  The empty language: extract_all gives empty lists, split one piece per
 * item, the item; a pattern that accepts the empty string follows the rule above.  RRX_ERR_ARG for null arguments, checked before
 * any device call (d_out may be null when cap == 0); RRX_ERR_UNSUPPORTED exactly where rrx_search_longest_extents returns it, for an
 * empty batch too, and for a piece of 2^30 bytes or more (the scan carries 30 bits per length: use rrx_search_all_longest_extents
 * and the generic pair with a prefix of the caller's own).  The _items forms use the handle's bytes, offsets, item count, trim and
 * device only (not its index).  LONG ITEMS: matches end at or before offset 0xFFFFFFFE of their item (not tested: no test of a few
 * seconds reaches it).                                                                                                              */
#define RRX_PIECES_MATCHES 0
#define RRX_PIECES_GAPS 1
int rrx_pieces_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first, const uint32_t *d_start,
                     const uint32_t *d_end, int mode, uint64_t *d_list_off, uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream);
int rrx_pieces_fill(int device, const void *d_bytes, const uint64_t *d_piece_src, const uint64_t *d_piece_off, size_t npieces, void *d_out,
                    void *stream);
int rrx_extract_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                    uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap, size_t *npieces,
                                    size_t *total, void *stream);
int rrx_extract_all_longest_items(const rrx_regex *re, const rrx_items *items, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap,
                                  void *d_out, size_t cap, size_t *npieces, size_t *total, void *stream);
int rrx_split_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                              uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap, size_t *npieces,
                              size_t *total, void *stream);
int rrx_split_longest_items(const rrx_regex *re, const rrx_items *items, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap,
                            void *d_out, size_t cap, size_t *npieces, size_t *total, void *stream);

/* THE ROWS A RESULT BITMAP SELECTS, WRITTEN AS A NEW COLUMN: SELECT col WHERE col RLIKE p, and what `grep` prints.  From a bitmap in
 * the result layout - bit i & 31 of word i >> 5 = row i: what rrx_match_corpus, rrx_contains_* and rrx_multi_plane write - to the
 * surviving rows' numbers, their offsets and their bytes, without a host step.
 * SELECTION RULE: with invert 0 a row is selected iff its bit is 1, with invert 1 iff its bit is 0 (grep -v).  The bits of the last
 * word beyond nbits are never selected, whatever they hold and whatever invert is.
 * rrx_bitmap_rank: d_rank[w] = the number of selected bits in the words in front of word w, for w = 0 .. nwords = ceil(nbits / 32);
 * d_rank[nwords] is the number of selected rows.  Plain numbers.  d_rank holds rank_words u64 words, rrx_bitmap_rank_words(nbits)
 * (host only) at least: the nwords + 1 entries and behind them what the scan needs (its chunk sums and the popcount words it sums);
 * a shorter rank_words is RRX_ERR_ARG.  nbits == 0 writes d_rank[0] = 0.  Plain multi-launch scans: no workgroup waits for another.
 * rrx_filter_sizes (an offsets column: item i = d_bytes[d_off[i] .. d_off[i+1] - trim)): for the k-th selected item i - k its rank -
 * d_row[k] = i, d_piece_src[k] = d_off[i], d_piece_len[k] = the item's length after trim (0 where trim exceeds it), saturated at
 * 0xFFFFFFFF.  Exactly the slots 0 .. nsel - 1 and nothing else; nitems == 0 writes nothing.
 * rrx_filter_corpus_sizes: the same triples for the LINES of a corpus, from the text and the corpus' own stripe index - no offsets
 * array is built or used.  A line is what rrx_search_longest_corpus calls a line (a final fragment without '\n' is one);
 * d_piece_src[k] = the absolute offset of the line's first byte, d_piece_len[k] = its length without the '\n', plus 1 when
 * keep_newline is set and the line has its '\n' in the text.  With keep_newline = 1 the filled output is again '\n'-delimited text
 * that rrx_corpus_create accepts (grep p1 | grep p2 without a host step); with keep_newline = 0 it is a column with trim 0.  A lane
 * of the kernel owns the lines that start in one stripe; one without a selected line reads no text at all.
 * THE BYTES: the caller prefixes d_piece_len into d_piece_off (nsel + 1 entries) and calls rrx_pieces_fill(device, d_bytes,
 * d_piece_src, d_piece_off, nsel, d_out, stream): d_piece_off is the new column's offsets array.
 * These entries are FULLY asynchronous on `stream` and can be captured into a graph: no read-back, no event, no scratch beyond the
 * caller's arrays.  d_rank must be the rank of the same d_bits, nbits (nitems; the corpus' line count) and invert: the slots come
 * from it.  RRX_ERR_ARG for null arguments, checked before any device call.
 * THE ONE-CALL FORMS apply the pattern's CONTAINS bitmap (rrx_contains_extents / _items / _corpus; the _items form keeps the indexed
 * batch's stripe-wise kernels): synchronous; everything temporary lives in device memory the call allocates and frees.  The cap
 * protocol of rrx_extract_all_longest_extents: *nrows and *total (the bytes of the new column) are exact either way; d_row (rows_cap
 * entries) and d_out_off (rows_cap + 1 entries, entry 0 = 0) are written iff *nrows <= rows_cap; d_out holds `cap` bytes and is
 * written iff additionally *total <= cap - otherwise not a byte of it: call again with the exact sizes.  With zero rows in (nitems
 * == 0, a corpus of zero lines) or zero rows selected: d_out_off[0] = 0 whatever rows_cap is, both counts 0, nothing else written.
 * A pattern that accepts the empty string selects every row; the empty language none - all of them with invert.  RRX_ERR_ARG for
 * null arguments, checked before any device call (d_row may be null when rows_cap == 0, d_out when cap == 0); RRX_ERR_UNSUPPORTED
 * exactly where the corresponding rrx_contains_* entry returns it (so RRX_OPT_CONTAINS_NFA applies), for an empty input too, and
 * for a selected row of 2^30 bytes or more (the scan carries 30 bits per length: use the contains entry and the generic entries
 * with a prefix of the caller's own).                                                                                              */
size_t rrx_bitmap_rank_words(size_t nbits);
int rrx_bitmap_rank(int device, const uint32_t *d_bits, size_t nbits, int invert, uint64_t *d_rank, size_t rank_words, void *stream);
int rrx_filter_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint32_t *d_bits, int invert, const uint64_t *d_rank,
                     uint64_t *d_row, uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream);
int rrx_filter_corpus_sizes(const rrx_corpus *c, const uint32_t *d_bits, int invert, int keep_newline, const uint64_t *d_rank, uint64_t *d_row,
                            uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream);
int rrx_filter_contains_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, int invert,
                                uint64_t *d_row, uint64_t *d_out_off, size_t rows_cap, void *d_out, size_t cap, size_t *nrows, size_t *total,
                                void *stream);
int rrx_filter_contains_items(const rrx_regex *re, const rrx_items *items, int invert, uint64_t *d_row, uint64_t *d_out_off, size_t rows_cap,
                              void *d_out, size_t cap, size_t *nrows, size_t *total, void *stream);
int rrx_filter_contains_corpus(const rrx_regex *re, const rrx_corpus *c, int invert, int keep_newline, uint64_t *d_row, uint64_t *d_out_off,
                               size_t rows_cap, void *d_out, size_t cap, size_t *nrows, size_t *total, void *stream);

/* regexp_extract with a CAPTURE GROUP on a string column: where, inside the leftmost-longest match of every item, does one
 * TOP-LEVEL group of the pattern sit.  The pattern is a concatenation P = A (B) C and the wanted group is (B); A and C may be absent,
 * parentheses inside A, B and C are plain grouping.  regexp_extract(col, 'https?://([^/]+)/.*', 1) is group 1 of that pattern.
 * SEMANTICS.  For item t let [s, e) be its leftmost-longest match under P, exactly what rrx_search_longest_extents reports.  Then
 *   i = the LARGEST offset in [s, e] such that A accepts t[s:i) and BC accepts t[i:e)     (A absent: i = s),
 *   j = the LARGEST offset in [i, e] such that B accepts t[i:j) and C accepts t[j:e)      (C absent: j = e),
 * and the group is [i, j), relative to the item start; no match: 0xFFFFFFFF in both words.  "Accepts" is the reference's whole-string
 * acceptance (regex.h:156-162), as in every other entry.  This is the longest-match rule applied to the prefix as a whole, then to
 * the group: the natural continuation of the leftmost-longest rule, and what a user expects wherever the split is unambiguous.  It
 * is NOT POSIX's subexpression-by-subexpression rule where A is itself ambiguous: (a|ab)(c|bcd)?(d*), group 3, on "abcd" - A =
 * (a|ab)(c|bcd)? accepts all of "abcd" (a + bcd), so the answer here is [4,4); POSIX answers [3,4).  '\n', NUL and bytes >= 0x80 are
 * ordinary text, as in rrx_search_longest_extents; LONG ITEMS follow the rule there (an item is searched as if it ended at its offset
 * 0xFFFFFFFE).
 * COMPILING.  `group` counts the unescaped '(' outside brackets, left to right from 1, nested ones too (as SQL does).  RRX_ERR_ARG:
 * group is 0 or larger than the number of groups, unknown engine, null argument.  RRX_ERR_PATTERN: the whole pattern does not compile.
 * RRX_ERR_UNSUPPORTED, with the reason in the error text: the selected group is not at nesting depth 1; it is directly followed by
 * '*', '+', '?' or '{'; the top level holds a '|'; the group is empty, the parentheses do not pair up or a part does not compile on
 * its own; one of the four tables below does not determinise within the state budget (16384 states), or the whole pattern has no
 * leftmost-longest tables - so that no device entry can fail for that reason.  The pattern is split on the front end's own token
 * vector (no substring is lexed again).  The handle holds the whole pattern as an ordinary regex (rrx_group_regex: for
 * rrx_search_longest_*, contains and so on; it belongs to the handle, do not free it) and four tables in the DFA layout, each with
 * state 0 dead and absorbing and class 0 leading there:                                                                              */
#define RRX_PROGRAM_GROUP_A 21      /* A, anchored, forwards; 0 words where A is absent                                              */
#define RRX_PROGRAM_GROUP_REV_BC 22 /* (B)C right to left, anchored; 0 words where A is absent (the first launch is skipped)         */
#define RRX_PROGRAM_GROUP_B 23      /* B, anchored, forwards (always there; not launched where C is absent)                          */
#define RRX_PROGRAM_GROUP_REV_C 24  /* C right to left, anchored; 0 words where C is absent                                          */
/* rrx_group_part: the source text of part `which` (0 / 1 / 2 = A / B / C) into buf, at most cap bytes, no terminator; returns its
 * length (0 for an absent part, and for a `which` other than the three).  rrx_group_program_words: the table `which` (one of the
 * four kinds above) as rrx_program_words dumps a DFA.  Both are host only: for tests and error messages.
 * THE DEVICE ENTRIES.  One lane-per-item kernel, "the longest split point", is launched twice: on (reverse (B)C, A) over [s, e] it
 * gives i, on (reverse C, B) over [i, e] it gives j; a launch whose part is absent is skipped.  Each launch walks backwards from
 * the stretch's end on the reverse table, leaving a MARK bit for every offset p whose rest t[p:end) the right-hand part accepts, then
 * forwards from the stretch's start on the forward table: the last marked offset at which the left-hand part accepts is the answer.
 * d_marks is rrx_search_all_longest_marks_words' buffer in its layout extended by one position, the stretch's end: the bit of
 * absolute offset g of item i is bit (g - d_off[0]) & 31 of word ((g - d_off[0]) >> 5) + i; rrx_search_all_longest_marks_words
 * (extent, nitems) words hold them for every extent >= d_off[nitems] - d_off[0].  It needs no clearing and holds nothing the caller can use
 * afterwards; words at or beyond marks_words are never touched, marks_words < nitems + 1 is rejected (RRX_ERR_ARG), and d_marks may
 * be null only when both A and C are absent (no launch).
 * rrx_group_spans_*: from ANY span list (d_match_start, d_match_end: for example what rrx_search_longest_extents wrote for
 * rrx_group_regex) to the group's spans.  The output arrays may be the same buffers as the input arrays.  A span that is not a match
 * of P reports no match (where A or C is present: with both absent the span IS the group and is passed through); a start of
 * 0xFFFFFFFF reports no match; spans are clamped into their item, so no byte outside an item is read whatever the list holds.
 * rrx_extract_group_longest_*: rrx_search_longest_* on the whole pattern into the two group arrays, then the two launches in place.
 * All four are fully asynchronous - no read-back, no scratch of their own, no event: once the handle's tables are on the device (its
 * first call there) they can be captured into a graph.  Every one of the 2 x nitems result words is written; an item for which
 * either step finds no split reports 0xFFFFFFFF in BOTH words.  nitems == 0 writes nothing and returns RRX_OK.  Null arguments give
 * RRX_ERR_ARG, checked before any device call.  The empty language reports no match everywhere: two fills and no table.  Tables are
 * placed as rrx_search_longest_extents places its two (LDS while a launch's pair fits 64 KiB, else - and under
 * RRX_ENGINE_DFA_GLOBAL - HBM/L2).  The _items forms use the handle's bytes, offsets, item count, trim and device only.           */
typedef struct rrx_group rrx_group;
int rrx_group_compile(const char *pattern, int group, rrx_group **out);
int rrx_group_compile_ex(const char *pattern, int group, int engine, rrx_group **out);
void rrx_group_free(rrx_group *grp);
const rrx_regex *rrx_group_regex(const rrx_group *grp);
size_t rrx_group_part(const rrx_group *grp, int which, char *buf, size_t cap);
size_t rrx_group_program_words(const rrx_group *grp, int which, uint32_t *out, size_t cap);
int rrx_group_spans_extents(const rrx_group *grp, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                            const uint32_t *d_match_start, const uint32_t *d_match_end, uint32_t *d_marks, size_t marks_words,
                            uint32_t *d_group_start, uint32_t *d_group_end, void *stream);
int rrx_group_spans_items(const rrx_group *grp, const rrx_items *items, const uint32_t *d_match_start, const uint32_t *d_match_end,
                          uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start, uint32_t *d_group_end, void *stream);
int rrx_extract_group_longest_extents(const rrx_group *grp, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                      uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start, uint32_t *d_group_end, void *stream);
int rrx_extract_group_longest_items(const rrx_group *grp, const rrx_items *items, uint32_t *d_marks, size_t marks_words,
                                    uint32_t *d_group_start, uint32_t *d_group_end, void *stream);

/* THE GROUP'S SPAN FOR EVERY MATCH OF A MATCH LIST: rrx_group_spans_* with a list per item in the shape every rrx_search_all*
 * one-call form returns - d_first has nitems + 1 entries, match k of item i is slot d_first[i] + k of d_match_start / d_match_end, the
 * arrays (the two outputs too) are indexed by the slot itself, d_first[0] need not be 0.  For every slot the answer is exactly what
 * rrx_group_spans_extents gives for that span on that item: the rule for i and j above, spans clamped into the item, a start of
 * 0xFFFFFFFF passed on as "none", no split: 0xFFFFFFFF in both words, a span that is no match of P: none where A or C is present.
 * Exactly the slots d_first[0] .. d_first[nitems] of d_group_start / d_group_end are written; they may be the input arrays.  d_marks,
 * its size (rrx_search_all_longest_marks_words) and the rejection of marks_words < nitems + 1 are those of rrx_group_spans_extents.
 * Fully asynchronous - no read-back, no scratch - and capturable into a graph once the handle's tables are on the device.  A lane
 * per ITEM walks the item's slots in order (kernels_group_items.hip: longest_split_list_kernel), the two phases per slot:
 * consecutive matches of an item share mark words, and a lane's stores to them follow one another.  Launched as rrx_group_spans_*
 * launches; an absent part's copy and the empty language's fill run over the slot range as a small kernel (the host does not know
 * the range).  An item with many matches is one lane's work.                                                                      */
int rrx_group_spans_list_extents(const rrx_group *grp, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                 const uint64_t *d_first, const uint32_t *d_match_start, const uint32_t *d_match_end, uint32_t *d_marks,
                                 size_t marks_words, uint32_t *d_group_start, uint32_t *d_group_end, void *stream);
int rrx_group_spans_list_items(const rrx_group *grp, const rrx_items *items, const uint64_t *d_first, const uint32_t *d_match_start,
                               const uint32_t *d_match_end, uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start,
                               uint32_t *d_group_end, void *stream);

/* regexp_replace WITH GROUP REFERENCES: regexp_replace(col, '([0-9]+)/([0-9]+)/([0-9]+)', '\3-\1-\2').
 * THE TEMPLATE (rrx_template, host only to compile): the bytes of `rep` are literal except '\': \0 ... \9 is a reference (0 the
 * whole match; ONE digit: \12 is group 1 followed by a literal 2), \\ is one backslash; any other byte behind '\' and a trailing
 * '\' give RRX_ERR_PATTERN with the offset of that '\' in rrx_last_error().  Adjacent literals merge; a template is at most 32
 * segments (literals and references; more: RRX_ERR_UNSUPPORTED); the empty template is valid and has none.  rrx_template_refs: the
 * distinct referenced groups >= 1 in ascending order into groups[0 .. cap), returns their number - the r-th of them is PLANE r
 * below.  rrx_template_segments (for tests): refs[k] = -1 for a literal, else the referenced group; lit_lens[k] = the literal's
 * length (0 for a reference), at most cap entries each; lits receives the literals' bytes one behind the other, at most lits_cap;
 * returns the number of segments.  Null arrays are skipped.
 * THE TWO GENERIC PASSES mirror rrx_replace_matches_sizes / _fill argument for argument, with BOTH d_start and d_end in both and, in
 * place of the literal, the template and the spans of its references: word r * plane_stride + q of d_ref_start / d_ref_end is the
 * span of plane r in slot q (relative to the item; plane_stride >= the largest slot + 1; both pointers may be null when the template
 * references no group >= 1).  The replacement R_q of slot q is its segments one behind the other: a literal's bytes; for \0
 * t[s':e') of the match; for \g t[s':e') of its plane's span - s' = min(s, L), e' = clamp(e, s', L) for an item of L bytes, and a
 * start of 0xFFFFFFFF contributes nothing: no byte outside the item is read, whatever the arrays hold.  Everything else is the
 * literal pair's with R_k in place of R: d_pos[slot] = where R_k begins in the output item, d_len[i] saturated, the output item
 * t[0:s_0] + R_0 + t[e_0:s_1] + ... + R_{m-1} + t[e_{m-1}:] (the text behind a match from the raw d_end, a source offset at or beyond
 * the item's end yields 0), exactly d_out[d_out_off[0] .. d_out_off[nitems]) written, d_out_off[0] any value, RRX_ERR_ARG for null
 * arguments before any device call.  Both passes are fully asynchronous and capturable once the template has been used on that
 * device (its first use uploads the segment program, 12 bytes per segment, and the literals).  The kernels
 * (kernels_replace_template_items.hip) are the literal pair's with one walk over the segments per match (sizes) and per located
 * byte (fill); the segment program is in LDS.  The literal entries are untouched and remain the faster way for a fixed R.
 * THE ONE-CALL FORMS replace every leftmost-longest match of ONE pattern: groups[g - 1] is the rrx_group handle of group g of that
 * pattern (null for a group the template does not reference; ngroups entries).  RRX_ERR_ARG before any device call: no handle is
 * non-null, the non-null handles do not share their pattern's bytes, the template references a group without a handle, null
 * arguments (d_out may be null when cap == 0).  The first non-null handle's rrx_group_regex searches; then
 * rrx_group_spans_list_* into one plane per referenced group, the template's sizes, the scan, its fill.  All else mirrors
 * rrx_replace_all_longest_extents: synchronous, temporaries allocated and freed by the call, d_out_off complete and *total exact
 * either way, not a byte of d_out written when *total > cap, RRX_ERR_UNSUPPORTED for an output item of 2^30 bytes or more and
 * exactly where the search returns it, nitems == 0: d_out_off[0] = 0; the empty language copies the items.  EACH GROUP'S SPAN
 * FOLLOWS ITS OWN rrx_group RULE INDEPENDENTLY: for an ambiguous pattern the spans of two groups need not come from one parse
 * (each is the longest-prefix rule above applied to that group's own A(B)C split; see the POSIX note there).  Out of scope, as for
 * rrx_group: nested, repeated or alternated groups; $1 and \g<name>; replacing only the n-th match.                               */
typedef struct rrx_template rrx_template;
int rrx_template_compile(const void *rep, size_t rep_len, rrx_template **out);
void rrx_template_free(rrx_template *tpl);
size_t rrx_template_refs(const rrx_template *tpl, int *groups, size_t cap);
size_t rrx_template_segments(const rrx_template *tpl, int *refs, uint32_t *lit_lens, size_t cap, void *lits, size_t lits_cap);
int rrx_replace_template_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first, const uint32_t *d_start,
                               const uint32_t *d_end, const rrx_template *tpl, const uint32_t *d_ref_start, const uint32_t *d_ref_end,
                               size_t plane_stride, uint32_t *d_len, uint32_t *d_pos, void *stream);
int rrx_replace_template_fill(int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first,
                              const uint32_t *d_start, const uint32_t *d_end, const uint32_t *d_pos, const rrx_template *tpl,
                              const uint32_t *d_ref_start, const uint32_t *d_ref_end, size_t plane_stride, const uint64_t *d_out_off, void *d_out,
                              void *stream);
int rrx_replace_groups_longest_extents(const rrx_group *const *groups, size_t ngroups, const rrx_template *tpl, int device, const void *d_bytes,
                                       const uint64_t *d_off, size_t nitems, uint32_t trim, uint64_t *d_out_off, void *d_out, size_t cap,
                                       size_t *total, void *stream);
int rrx_replace_groups_longest_items(const rrx_group *const *groups, size_t ngroups, const rrx_template *tpl, const rrx_items *items,
                                     uint64_t *d_out_off, void *d_out, size_t cap, size_t *total, void *stream);

/* A SET OF PATTERNS ON A STRING COLUMN: which of up to 32 patterns does each item contain (log classification, rule lists,
 * CASE WHEN col RLIKE p1 ... WHEN col RLIKE pK) - one walk over the column instead of one per pattern.
 * THE RULE: for the set p_0 .. p_{K-1}, 1 <= K <= 32, bit k of d_mask[i] is set exactly when rrx_contains_extents on p_k sets bit i
 * of its bitmap for the same batch and trim.  All else follows: '\n', NUL and bytes >= 0x80 are ordinary text inside an item; the
 * bit of a pattern that accepts the empty string is always set, that of the empty language never; the bytes behind an item's trim
 * are never read; a pattern may occur twice (its two bits agree).  Bits K .. 31 of every mask are 0.
 * COMPILING: every member goes through the front end to its forward search table ("any bytes, then the pattern": accepting
 * exactly where a match ends).  RRX_ERR_PATTERN: a member does not parse; RRX_ERR_UNSUPPORTED: a member's forward table does not
 * determinise within the state budget (16384 states) - rrx_last_error() names the member's index in both cases, and there is no
 * fallback for such a member.  RRX_ERR_ARG: npatterns == 0 or > 32, a null pointer (the array, a member, out), an engine other
 * than RRX_ENGINE_AUTO / _DFA / _DFA_GLOBAL.  The members are cut into GROUPS, greedy in set order; a group shares one PRODUCT
 * table (a row = a tuple of member states, its mask = the bits of the members whose state is accepting; minimised; rows with an
 * empty mask numbered first), stepped once per byte whatever the number of members.  Member k joins the open group if the
 * minimised product with it has at most max_rows rows (0: 65535, what 16-bit rows allow; a product is abandoned beyond 65535
 * tuples, so compile time is bounded) and fits 64 KiB of LDS; otherwise the group closes and k opens the next one.  A member
 * beyond the LDS budget on its own is a group of its own in HBM/L2; RRX_ENGINE_DFA_GLOBAL leaves every group there and drops the
 * LDS criterion.  Every set of individually admissible patterns compiles.
 * rrx_multi_patterns / _groups: K and the number of groups.  rrx_multi_group_mask: the members of group g as a bit mask (the
 * groups' masks partition the set), _group_states: the rows of its table; 0 for a group that is not there.
 * rrx_multi_program_words(m, group, out, cap): the table of a group as words, the number of words returned (cap = 0 sizes it):
 *   [nstates, ncls, start row, first_hit, full], cls[256] (byte -> class), next[nstates][ncls], mask[nstates]
 * Rows below first_hit have an empty mask, rows from first_hit on a non-empty one; full = the OR of all masks.  The answer for an
 * item: m = mask[start]; for every byte c: s = next[s][cls[c]], m |= mask[s]; the item's mask is the OR of m over the groups.
 * THE ENTRIES: item i = d_bytes[d_off[i] .. d_off[i+1] - trim), as in rrx_contains_extents; d_mask: nitems 32-bit words, every
 * one of them written (the first group's launch stores, the others OR - the lane owns its word: no atomics, nothing to clear
 * beforehand), none beyond.  A lane stops reading its item once it holds every bit its group can give.  One launch per group; a
 * set of empty languages only costs one memset.  Tables are uploaded once per device at the first call there; from then on the
 * entries are asynchronous on `stream` and can be captured into a graph.  nitems == 0 writes nothing and returns RRX_OK;
 * RRX_ERR_ARG for null arguments, checked before any device call.  The _items form uses the handle's bytes, offsets, item count,
 * trim and device only.
 * rrx_multi_counts: d_counts[k] (32 uint64 counters in device memory, zeroed here on `stream`) = the items among the first
 * nitems whose mask has bit k.  rrx_multi_plane: bit `pattern` (< 32, RRX_ERR_ARG otherwise) of every mask as a bitmap in the
 * layout of rrx_contains_extents - ceil(nitems / 32) whole words, the bits beyond nitems 0 - so that rrx_bitmap_count and
 * rrx_bitmap_to_bytes apply.  Both take any column of masks and no handle.
 * THE '\n'-CORPUS FORM, rrx_multi_contains_corpus: d_mask holds rrx_corpus_num_lines(c) 32-bit words, and word i is exactly what
 * rrx_multi_contains_extents writes for an item made of the bytes of line i without its terminator - bit k is set exactly when
 * member k is contained in line i.  All else follows: NUL and bytes >= 0x80 are ordinary text; a final fragment without '\n' is a
 * line; an empty line gets the bits of the members that accept the empty string; bits K .. 31 are 0; a match never spans a '\n'
 * ("ab" '\n' "c" does not contain ab+c), and a member whose pattern holds a '\n' can match only through its '\n'-free words.  For
 * the members without '\n' in their pattern, bit k of word i also equals bit i of rrx_contains_corpus on member k.  A lane per
 * stripe of the corpus, which reads its text in consecutive 16-byte loads and finds its line numbers through the corpus' index, in
 * the place of a lane per item; one launch per group as above.  Every one of the words is written (the lane that owns a line owns
 * its word: no atomics, nothing to clear beforehand), none beyond; a corpus of zero lines writes nothing and returns RRX_OK.
 * Tables are uploaded at the first call on the device; from then on the entry is asynchronous on `stream` and can be captured
 * into a graph: no read-back, no scratch, no event.  RRX_ERR_ARG for a null m, c or d_mask, checked before any device call.
 * rrx_multi_counts and rrx_multi_plane apply to its output with nitems = the number of lines; the plane then has the layout of
 * rrx_contains_corpus' bitmap.
 * Not here: a stride-2 form of the product table, more than 32 patterns per handle.                                              */
typedef struct rrx_multi rrx_multi;
int rrx_multi_compile(const char *const *patterns, size_t npatterns, rrx_multi **out);
int rrx_multi_compile_ex(const char *const *patterns, size_t npatterns, int engine, uint32_t max_rows, rrx_multi **out);
void rrx_multi_free(rrx_multi *m);
size_t rrx_multi_patterns(const rrx_multi *m);
size_t rrx_multi_groups(const rrx_multi *m);
uint32_t rrx_multi_group_mask(const rrx_multi *m, size_t group);
uint32_t rrx_multi_group_states(const rrx_multi *m, size_t group);
size_t rrx_multi_program_words(const rrx_multi *m, size_t group, uint32_t *out, size_t cap);
int rrx_multi_contains_extents(const rrx_multi *m, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                               uint32_t *d_mask, void *stream);
int rrx_multi_contains_items(const rrx_multi *m, const rrx_items *items, uint32_t *d_mask, void *stream);
int rrx_multi_contains_corpus(const rrx_multi *m, const rrx_corpus *c, uint32_t *d_mask, void *stream);
int rrx_multi_counts(int device, const uint32_t *d_mask, size_t nitems, uint64_t *d_counts, void *stream);
int rrx_multi_plane(int device, const uint32_t *d_mask, size_t nitems, uint32_t pattern, uint32_t *d_bits, void *stream);

/* ONE device-resident string of any length (regex.h:156-159: operator++ consumes the whole string; '\n' and every
 * other byte are ordinary, a NUL or a byte >= 0x80 rejects).  d_accept[0] = 1 iff accepted.  Strings of 32 KiB and
 * more are split into chunks that are stepped in parallel from every table state (automata with <= 254 table
 * states); synchronous with respect to `stream`.  d_bytes needs no alignment: a string may start at any address
 * (a chunk that does not start on a 16-byte boundary is read byte by byte instead of sixteen bytes per load).    */
int rrx_match_string(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint8_t *d_accept, void *stream);

/* WHERE the leftmost-longest match inside ONE device-resident string of any length is.  One rule: d_span[0] and d_span[1] (device
 * memory, two u64) are the start and the end that rrx_search_longest_extents writes for the one-item batch off = {0, nbytes},
 * trim = 0 over the same bytes, widened to 64 bits - ~0ull in both for no match - without that entry's cap at offset 0xFFFFFFFE.
 * So: the smallest start, then the largest end from there; '\n', NUL and bytes >= 0x80 are ordinary text of their class; a pattern
 * that accepts the empty string gives start 0 and the longest accepted prefix; the empty string gives [0, 0) or none; the empty
 * language gives none without a kernel.  rrx_contains_string: d_found[0] = 1 exactly when d_span[0] != ~0ull (the backward pass
 * alone).  d_bytes needs no alignment.
 * Strings of 2 KiB and more are cut into chunks that are walked in parallel (both search tables of at most 254 states): backwards
 * over the whole string on the starts table, then forwards from the start found on the anchored table in windows that grow (256
 * bytes, then 15 times what has been walked), until the table is dead or the string ends - a short match costs a short forward
 * walk.  Shorter strings, larger tables and RRX_ENGINE_DFA_GLOBAL go through rrx_search_longest_extents as one item; on that path
 * a string beyond 0xFFFFFFFE bytes is refused with RRX_ERR_UNSUPPORTED (it is never answered short).
 * Both entries are synchronous with respect to `stream` (one small read-back per pass and forward window) and take the handle's
 * scratch (concurrent callers of one regex take turns), as rrx_match_string does.  RRX_ERR_ARG for a null re, d_span / d_found,
 * or a null d_bytes with nbytes > 0, before any device call; RRX_ERR_UNSUPPORTED where rrx_search_longest_extents reports it.  */
int rrx_search_longest_string(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint64_t *d_span, void *stream);
int rrx_contains_string(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint8_t *d_found, void *stream);

/* ---- host-buffer conveniences (PCIe inclusive; synchronous) ------------------------------------------ */
/* bytes/accept are HOST pointers; *nlines receives the number of strings; at most cap results are written */
int rrx_match_host(const rrx_regex *re, int device, const void *bytes, size_t nbytes, uint8_t *accept, size_t cap,
                   size_t *nlines);
/* One NUL-terminated host string: `auto it = r.get_acceptance_iter(text)++; *it` (test/main.cpp:25-27).
 * *accepted = has_value(); *len = strlen(text) = Match.end - Match.start.                                   */
int rrx_match_cstr(const rrx_regex *re, int device, const char *text, int *accepted, size_t *len);

#ifdef __cplusplus
}
#endif
#endif
