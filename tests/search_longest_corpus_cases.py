"""What the CPU and the device tests of rrx_search_longest_corpus share: texts cut from the shared short items, the corpus built by
hand around stripe, load and line boundaries, and the references that need no device.  Nothing here is a test."""
import functools
import re

import numpy as np

import roaringregex_amd as rr
from contains_cases import split_lines
from test_contains_items_lowering import MAX_ITEM, NEWLINE_PATTERNS
from test_search_longest_items_lowering import GREEDY_RE, START_CASES, SearchLongestReplay, reference_set, want_for

# the patterns that run over geometry_corpus(): the two whose greedy Python search names the leftmost-longest substring, a nullable
# one, the literal that "ab" '\n' "c" must not match, START_CASES' patterns and the patterns that hold a '\n'
GEOMETRY_PATTERNS = ["ab+c", "a{1,300}", "a*", "abc"] + list(dict.fromkeys(p for p, _ in START_CASES)) + NEWLINE_PATTERNS


@functools.lru_cache(maxsize=None)
def reference_texts():
    """[(pattern, text, want)]: per pattern of reference_set() its items that hold no '\\n', each followed by '\\n', and the brute
    force's rows for them.  The patterns that hold a '\\n' are checked through an oracle that reads 'x' for '\\n': their lines get
    'z' for 'x' and a brute force of their own."""
    out = []
    for p, items, want, _ in reference_set():
        keep = [i for i, it in enumerate(items) if b"\n" not in it]
        assert len(keep) > len(items) // 2
        keep = keep + keep[::-1] + keep[::2] + keep[1::2] + keep               # about 2 KB: four stripes of 512 bytes, in four orders
        lines = [items[i] for i in keep]
        if "\n" in p:
            lines = [ln.replace(b"x", b"z") for ln in lines]
            rows = want_for(p, lines)
        else:
            rows = want[keep]
        rows.setflags(write=False)
        out.append((p, b"".join(ln + b"\n" for ln in lines), rows))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def geometry_corpus():
    """-> (bytes, {line: (start, end)} for "ab+c", {line: (start, end)} for "a{1,300}"); filler 'z', offsets absolute.  At stripe 512:
    line 0 ends on stripe 0's last byte; line 1 fills stripe 1 and its '\\n' is stripe 2's first byte; line 2 is 1300 bytes over a
    stripe without '\\n'; "\\n\\n" astride 2559 | 2560 makes stripe 5 fresh with a '\\n' as its first byte; "\\n\\n\\n" at 3070 .. 3072."""
    buf, abc, run = bytearray(), {}, {}

    def fill_to(pos, plant=()):
        at = len(buf)
        assert pos >= at
        buf.extend(b"z" * (pos - at))
        for off, word in plant:
            assert at <= off and off + len(word) <= pos
            buf[off:off + len(word)] = word

    def end_line(want=None, want_run=None):
        i = bytes(buf).count(b"\n")
        if want:
            abc[i] = want
        if want_run:
            run[i] = want_run
        buf.extend(b"\n")

    fill_to(511, [(0, b"abbc")]); end_line((0, 4), (0, 1))                     # the first bytes of a line; '\n' = stripe 0's last byte
    fill_to(1024, [(1019, b"abbbc")]); end_line((507, 512), (507, 508))        # the last bytes of a line; '\n' = stripe 2's first byte
    start = len(buf)                                                           # line 2: 1300 bytes; "abc" across 1535 | 1536, a later match loses
    fill_to(start + 1300, [(1534, b"abc"), (2100, b"abbc")]); end_line((1534 - start, 1537 - start), (1534 - start, 1535 - start))
    assert start == 1025 and len(buf) > 2048
    fill_to(2559); end_line(); end_line()                                      # "\n\n" astride 2559 | 2560: an empty line in a fresh stripe
    start = len(buf)
    fill_to(3070, [(2686, b"abbc")]); end_line((2686 - start, 2690 - start), (2686 - start, 2687 - start))      # across the 16-byte boundary 2688
    end_line(); end_line()                                                     # "\n\n\n" at 3070, 3071 | 3072
    start = len(buf)                                                           # starts in stripe 6, ends in stripe 7, whose lane owns the line
    fill_to(3700, [(3581, b"abbbc")]); end_line((3581 - start, 3586 - start), (3581 - start, 3582 - start))
    buf.extend(b"zzab"); end_line(None, (2, 3))                                # "ab" '\n' "c": no match spans the '\n'
    buf.extend(b"czz"); end_line()
    buf.extend(b"z" * 5 + b"a" * 1000 + b"zzz"); end_line(None, (5, 305))      # a thousand starts: the smallest wins, 300 bytes from it
    for (_, item), want, want_run in zip(START_CASES, [(0, 3), (2, 5), (0, 4), None, None], [(0, 1), (2, 3), (0, 1), None, None]):
        buf.extend(item); end_line(want, want_run)
    buf.extend(b"zzabc"); end_line((2, 5), (2, 3))
    buf.extend(b"abczz"); end_line((0, 3), (0, 1))
    data = bytes(buf)
    assert data[511] == 10 and data[1024] == 10 and b"\n" not in data[1536:2048] and data[2559:2561] == b"\n\n" and data[3070:3073] == b"\n\n\n"
    assert data[1534:1537] == b"abc" and data[2686:2690] == b"abbc" and 2688 % 16 == 0 and data[3581:3586] == b"abbbc" and b"x" not in data
    return data, abc, run


def greedy_rows(p, lines):
    """Python's greedy search for the two patterns of GREEDY_RE: the leftmost-longest substring at any line length."""
    c = re.compile(GREEDY_RE[p])
    ms = [c.search(ln) for ln in lines]
    return np.array([(m.start(), m.end()) if m else (-1, -1) for m in ms], dtype=np.int32).reshape(len(lines), 2)


def by_hand_rows(planted, nlines):
    rows = np.full((nlines, 2), -1, dtype=np.int32)
    for i, se in planted.items():
        rows[i] = se
    return rows


@functools.lru_cache(maxsize=None)
def geometry_wants():
    """{pattern: int32 [lines, 2]} for geometry_corpus() from the CPU alone: the per-item replay of the two tables on every line (it
    is the specification of rrx_search_longest_extents, checked against the brute force where that can run), equal to the brute
    force on the lines it can take, to Python's greedy search for the patterns of GREEDY_RE and to the rows planted by hand."""
    data, abc, run = geometry_corpus()
    lines = split_lines(data)
    short = [i for i, ln in enumerate(lines) if len(ln) <= MAX_ITEM]
    out = {}
    for p in GEOMETRY_PATTERNS:
        rows = SearchLongestReplay(rr.RRegex(p)).search_items(lines)
        assert (rows[short] == want_for(p, [lines[i] for i in short])).all(), p
        if p in GREEDY_RE:
            assert (rows == greedy_rows(p, lines)).all(), p
        rows.setflags(write=False)
        out[p] = rows
    assert (out["ab+c"] == by_hand_rows(abc, len(lines))).all() and (out["a{1,300}"] == by_hand_rows(run, len(lines))).all()
    assert (out["a*"][:, 0] == 0).all() and int(out["a*"][:, 1].max()) == 1         # (the longest accepted PREFIX)
    return out
