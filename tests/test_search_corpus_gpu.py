"""rrx_search_corpus, rrx_search_all_count, rrx_search_all_fill and rrx_search_all through the C ABI on the corpora of
tests/search_cases.py: features placed at every residue of a lane, an event word, a byte pair, a walk's word and a chunk; the end of
the data at every length around a lane and a chunk; chunks that own one line less, as many and more than any staging length; match
ends at the limits of the packed staging entries; dense walks; NUL and bytes >= 0x80; the global form, the forward table alone, the
stripe that is the chunk; patterns that accept the empty string.  The expectation never replays a device table (the oracle's brute
force per cell, composed: tests/test_search_corpus_cases.py proves the composition on the host).  Every output array is poisoned and
stands between 64 poisoned guard words.

What a one-line slip in kernels_search.hip would meet (by reading; nobody runs a broken kernel on a shared machine):
  * `owned = ls <= my_end_rel`: test_e_dense_walks - a matching line that starts at a lane's first byte behind more lines than the staging
    array holds; the lane before would write "no match" over its result at the end of the pass (test_c_staging_length has such lines too);
  * `fits` with 0x10000 for 0x8000: test_d_packing_limits - the needle that is its whole line's head and ends 0x8000 behind the line start would be
    staged with bit 31 set before the parked hits are taken, and read back as one;
  * `hi_ord <= kStageLines`: test_c_staging_length - the chunk that owns exactly kStageLines lines behind an open one parks ordinal
    kStageLines outside the array and never writes that line: its poison stays;
  * `at <= all.cap`: every case, at every cap below the total - slot `cap` must still hold its poison;
  * `room > 2u` for `room > 3u`: test_a_bounded_walks - "caaab", where "aaab" from inside the match before is accepted (kFill, kAll);
  * a text word without its clean_word: test_f_high_bytes_and_nul - a byte >= 0x80 at each of the sixteen offsets of a slot, in the lane's
    own bytes and in the stretch it follows, next to a match."""
import ctypes as C
import functools

import numpy as np
import pytest

import roaringregex_amd as rr
import search_cases as sc
from patterns import EMAIL

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_pieces_items_gpu import GUARD, Words  # noqa: E402  (needs torch)

BEHIND = np.frombuffer(b"bc\nabc " * 12, dtype=np.uint8)           # what lies behind a corpus in the same allocation: matches, if it were read


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert GUARD == 64


@functools.lru_cache(maxsize=None)
def regex(pattern, anchored=True):
    r = rr.RRegex(pattern)
    if not anchored:
        r.set_search_anchored(False)
    if pattern == sc.GLOBAL_FORM:
        assert int(r.program(rr.PROGRAM_SEARCH_LINE2)[4]) == 2, "layout: HBM/L2 (else these cases no longer reach the global form)"
    return r


def device_corpus(data, stripe=0):
    """The corpus as a slice of a larger allocation: at least 64 owned bytes behind it, which would change results if they were read."""
    n = len(data)
    buf = torch.empty(n + len(BEHIND), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.copy_(torch.from_numpy(np.concatenate([data, BEHIND])))
    return rr.Corpus(buf[:n], stripe=stripe)


class Want:
    """The expectation as the arrays the entries write."""

    def __init__(self, first_want, all_want):
        self.start = np.array([f[0] for f in first_want], dtype=np.int32)
        self.end = np.array([f[1] for f in first_want], dtype=np.int32)
        self.count = np.array([len(w) for w in all_want], dtype=np.int32)
        self.first = np.concatenate([[0], np.cumsum(self.count, dtype=np.int64)]).astype(np.int64)
        flat = np.array([m for w in all_want for m in w], dtype=np.int32).reshape(-1, 2)
        self.all_start, self.all_end = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
        self.total = int(self.first[-1])
        assert len(self.all_start) == self.total


def same(got, want, what, array):
    assert got.shape == want.shape, (what, array, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, array, "entry", int(bad[0]), "got", int(got[bad[0]]), "want", int(want[bad[0]]), "wrong entries", int(bad.size))


def caps_for(want, starts, nbytes, light):
    total = want.total
    caps = {0, 1, max(total - 1, 0), total, total + 5}
    if not light:
        several = np.nonzero(want.count >= 2)[0]
        if several.size:                                            # inside one line's matches
            caps.add(int(want.first[several[several.size // 2]]) + 1)
        nchunks = (nbytes + sc.CHUNK - 1) // sc.CHUNK
        for k in {nchunks // 2, nchunks - 1} - {0}:                 # the first slot of a chunk: that of the first line that starts in it
            line = int(np.searchsorted(starts, k * sc.CHUNK))
            if line < len(want.count):
                caps |= {int(want.first[line]), int(want.first[line]) + 1}
    return sorted(caps)


def search_all_once(r, corpus, want, cap, what, stream=None):
    """One rrx_search_all at `cap`: d_first and *total complete, the first min(cap, total) slots exact, every slot behind them and every
    guard word still poisoned."""
    n, total = len(want.count), want.total
    d_first = Words(n + 1, torch.int64)
    room = max(total, cap) + 8
    d_start, d_end = Words(room, torch.int32), Words(room, torch.int32)
    tot = C.c_size_t(0x5A5A)
    if stream is not None:
        torch.cuda.synchronize()                                    # the poison is in place before another stream writes
    s = rr._stream_ptr(stream)
    rr._check(rr._L.rrx_search_all(r._h, corpus._h, d_first.ptr, d_start.ptr if cap else None, d_end.ptr if cap else None, cap, C.byref(tot), s))
    torch.cuda.synchronize()
    assert tot.value == total, (what, "cap", cap, "*total", tot.value, total)
    same(d_first.written(what), want.first, (what, "cap", cap), "d_first")
    k = min(cap, total)
    same(d_start.written((what, "cap", cap, "slots >= cap or guards of d_start were written"), k), want.all_start[:k], (what, "cap", cap), "d_start")
    same(d_end.written((what, "cap", cap, "slots >= cap or guards of d_end were written"), k), want.all_end[:k], (what, "cap", cap), "d_end")
    return tot.value


def run_all_modes(r, corpus, first_want, all_want, what, starts=None, want=None, light=False):
    """Every entry of the corpus search on one corpus, every output poisoned and guarded, against the expectation."""
    L, s = rr._L, rr._stream_ptr(None)
    want = want or Want(first_want, all_want)
    n, total = corpus.num_lines, want.total
    assert n == len(first_want) == len(all_want), (what, "lines", n, len(first_want))
    if starts is None:
        starts = np.zeros(1, dtype=np.int64)
    # first match
    d_start, d_end = Words(n, torch.int32), Words(n, torch.int32)
    rr._check(L.rrx_search_corpus(r._h, corpus._h, d_start.ptr, d_end.ptr, s))
    torch.cuda.synchronize()
    same(d_start.written(what), want.start, what, "search_corpus d_start")
    same(d_end.written(what), want.end, what, "search_corpus d_end")
    # count, the caller's prefix, fill
    d_count = Words(n, torch.int32)
    rr._check(L.rrx_search_all_count(r._h, corpus._h, d_count.ptr, s))
    torch.cuda.synchronize()
    counts = d_count.written(what)
    same(counts, want.count, what, "search_all_count d_count")
    first = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)[:-1]]).astype(np.int64)
    d_first = torch.from_numpy(first).cuda()
    f_start, f_end = Words(total, torch.int32), Words(total, torch.int32)
    rr._check(L.rrx_search_all_fill(r._h, corpus._h, C.c_void_p(d_first.data_ptr()), f_start.ptr, f_end.ptr, s))
    torch.cuda.synchronize()
    same(f_start.written(what), want.all_start, what, "search_all_fill d_start")
    same(f_end.written(what), want.all_end, what, "search_all_fill d_end")
    assert np.array_equal(d_first.cpu().numpy(), first), (what, "search_all_fill wrote d_first")
    # one call, at every cap; the retry at *total
    for cap in caps_for(want, starts, corpus.num_bytes, light):
        got = search_all_once(r, corpus, want, cap, what)
        if cap == 1 and got > cap:
            search_all_once(r, corpus, want, got, (what, "retry at *total"))
    if not light:
        for k in range(3):                                          # the scratch is zeroed per call
            search_all_once(r, corpus, want, max(total - 1, 0) if k == 1 else total, (what, "call", k, "in a row"))
        side = torch.cuda.Stream()
        search_all_once(r, corpus, want, total, (what, "side stream"), stream=side)
        d_start, d_end = Words(n, torch.int32), Words(n, torch.int32)
        torch.cuda.synchronize()
        rr._check(L.rrx_search_corpus(r._h, corpus._h, d_start.ptr, d_end.ptr, rr._stream_ptr(side)))
        side.synchronize()
        same(d_start.written(what), want.start, what, "search_corpus d_start, side stream")
        same(d_end.written(what), want.end, what, "search_corpus d_end, side stream")


def run_case(pattern, case, what, stripe=0, anchored=True, light=False, want=None):
    corpus = device_corpus(case.data, stripe)
    assert stripe == 0 or corpus.stripe == stripe
    run_all_modes(regex(pattern, anchored), corpus, case.first_want, case.all_want, (pattern[:20], what, "stripe", corpus.stripe, "anchored", anchored),
                  starts=case.starts, want=want, light=light)


# ------------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def built(name, *args):
    case = getattr(sc, name)(*args)
    case = case[0] if name == "staging_case" else case
    return case, Want(case.first_want, case.all_want)


def run_built(pattern, name, args, what, **how):
    case, want = built(name, *args)
    run_case(pattern, case, what, want=want, **how)


@pytest.mark.parametrize("final_newline", [True, False])
def test_a_residues(final_newline):
    run_built("ab+c", "residue_case", ("ab+c", 1, 11, final_newline), "residues")


def test_a_bounded_walks():
    run_built(sc.BOUNDED, "bounded_walk_case", (), "bounded walks")


@functools.lru_cache(maxsize=None)
def end_base(pattern):
    return sc.end_of_data_base(pattern)


def end_of_data(pattern, lengths, **how):
    ran = 0
    for n in lengths:
        for variant in sc.END_VARIANTS:
            case = sc.end_of_data_case(pattern, end_base(pattern), n, variant)
            if case is None:
                assert variant == "match_at_end" and n < len(sc.SPECS[pattern].lead[0]), "only a match that does not fit n bytes may be missing"
                continue
            assert len(case.data) == n
            run_case(pattern, case, ("end of data", n, variant), light=True, **how)
            ran += 1
    return ran


@pytest.mark.parametrize("group", range(len(sc.END_LENGTHS)))
def test_b_end_of_data(group):
    lengths = sc.END_LENGTHS[group]
    assert end_of_data("ab+c", lengths) >= 4 * len(lengths) - 2


STAGING = [("as is", sc.STAGE_MULTIPLES, None), ("multi", sc.STAGE_MULTIPLES, "multi")] + [("plain %d" % k, piece, "plain") for k, piece in enumerate(sc.STAGE_PIECES)]


@pytest.mark.parametrize("pattern", ["ab+c", EMAIL, sc.GLOBAL_FORM])
@pytest.mark.parametrize("name,multiples,pad", STAGING, ids=[s[0] for s in STAGING])
def test_c_staging_length(pattern, name, multiples, pad):
    case, _ = sc.staging_case(pattern, multiples, pad)
    assert len(case.data) <= 8 << 20
    run_case(pattern, case, ("staging", name))


@pytest.mark.parametrize("pattern", [sc.LONG, "ab+c"])
@pytest.mark.parametrize("long_walk", [True, False])
def test_d_packing_limits(pattern, long_walk):
    run_built(pattern, "packing_case", (pattern, long_walk), ("packing", "long walk" if long_walk else "short walk"))


def test_d_a_line_with_more_matches_than_any_staging_array():
    run_built(sc.KEYWORD, "dense_line_case", (), "dense line")


@pytest.mark.parametrize("pattern", ["ab+c", sc.KEYWORD])
def test_e_dense_walks(pattern):
    run_built(pattern, "dense_walks_case", (pattern,), "dense walks")


def test_f_high_bytes_and_nul():
    run_built("ab+c", "odd_bytes_case", ("ab+c",), "odd bytes")
    run_built("ab+c", "single_high_byte_case", ("ab+c",), "one high byte")


FORMS = {"global form": dict(pattern=sc.GLOBAL_FORM), "forward table alone": dict(pattern="ab+c", anchored=False),
         "stripe = chunk": dict(pattern="ab+c", stripe=16384), "stripe 512": dict(pattern="ab+c", stripe=512)}
REDUCED_OFFSETS = tuple(sc.PACK_OFFSETS[k] for k in (1, 2, 5, 6, 8, 9))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("part", ["a", "b", "d"])
def test_g_forms(form, part):
    how = dict(FORMS[form])
    pattern = how.pop("pattern")
    if part == "a":
        run_built(pattern, "residue_case", (pattern, 5), ("residues", form), **how)
    elif part == "b":
        every = [n for group in sc.END_LENGTHS for n in group]
        lengths = [n for n in every if n % 3 == 0 or n in (1, 255, 256, 257, 16383, 16384, 16385)]
        lengths += [next(n for n in every if n % 16 == r) for r in range(16) if r not in {n % 16 for n in lengths}]
        assert {n % 16 for n in lengths} == set(range(16)) and len(lengths) < len(every) // 2
        end_of_data(pattern, lengths, **how)
    else:
        # (the global-form pattern has no needle that is one match and nothing else: its matches may start anywhere in a run of [ab])
        for long_walk in ((False,) if pattern == sc.GLOBAL_FORM else (True, False)):
            run_built(pattern, "packing_case", (pattern, long_walk, REDUCED_OFFSETS), ("packing", form, long_walk), **how)


@pytest.mark.parametrize("pattern", sc.EMPTY_ACCEPTING)
@pytest.mark.parametrize("stripe", [512, 16384])
def test_h_patterns_that_accept_the_empty_string(pattern, stripe):
    for final_newline in (True, False):
        case = sc.empty_case(stripe, final_newline)
        want = Want(case.first_want, case.all_want)
        corpus = device_corpus(case.data, stripe)
        assert corpus.stripe == stripe
        run_all_modes(regex(pattern), corpus, case.first_want, case.all_want, (pattern, "accepts the empty string", stripe, final_newline),
                      starts=case.starts, want=want)
